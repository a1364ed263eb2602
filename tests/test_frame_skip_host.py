"""frame_skip without a GPU: the config key, the length helper, a stream slot's bookkeeping against plain
slicing, align's frame-to-seconds conversion, and the two calls' declarations."""
import os
import re
import types

import numpy as np
import pytest

import frame_skip_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLES = os.path.join(HERE, 'golden', 'sample_set')


def config_with(tmp_path, value):
    out = []
    for ln in open(os.path.join(SAMPLES, 'toy.config')).read().splitlines():
        out.append('output=' + SAMPLES if ln.startswith('output=') else ln)
        if ln.strip() == '[Parameters]' and value is not None:
            out.append('frame_skip=' + value)
    p = tmp_path / 'toy.config'
    p.write_text('\n'.join(out) + '\n')
    return str(p)


def test_config_key_absent_is_one(tmp_path):
    from neuralasr_amd.config import Config
    assert Config(config_with(tmp_path, None), True).frame_skip == 1


@pytest.mark.parametrize('text,want', [('1', 1), ('3', 3), (' 8 ', 8)])
def test_config_key_parsed(tmp_path, text, want):
    from neuralasr_amd.config import Config
    c = Config(config_with(tmp_path, text), True)
    assert c.frame_skip == want and isinstance(c.frame_skip, int)


@pytest.mark.parametrize('text', ['0', '9', '-2', '2.5', 'two'])
def test_config_key_refused(tmp_path, text):
    from neuralasr_amd.config import Config
    with pytest.raises(ValueError, match='frame_skip'):
        Config(config_with(tmp_path, text), True)


def test_length_helper_against_range():
    from neuralasr_amd.engine import skip_frames
    for s in range(1, 9):
        for n in range(0, 41):
            assert skip_frames(n, s) == len(range(0, n, s)) == R.net_len(n, s), (n, s)
        got = skip_frames(np.arange(41, dtype=np.int32), s)
        assert got.tolist() == [len(range(0, n, s)) for n in range(41)]
    for bad in (0, 9):
        with pytest.raises(ValueError, match='frame_skip'):
            skip_frames(10, bad)


def test_engine_logit_lens_uses_the_handles_skip():
    """Engine.logit_lens without a library: the method reads frame_skip and nothing else"""
    from neuralasr_amd.engine import Engine
    fake = types.SimpleNamespace(frame_skip=3)
    got = Engine.logit_lens(fake, [41, 40, 39, 7, 1])
    assert got.dtype == np.int32 and got.tolist() == [14, 14, 13, 3, 1]


@pytest.mark.parametrize('s', range(1, 9))
def test_stream_bookkeeping_against_slicing(s):
    """For random feed splits of an utterance: the kept rows per feed, from the running phase alone, concatenated, are
    rows[::s]; the count per feed is what the rule says (frame_skip_ref.feed_kept)."""
    from neuralasr_amd.engine import stream_keep
    rng = np.random.default_rng(s)
    for trial in range(50):
        n_rows = int(rng.integers(0, 60))
        rows = np.arange(n_rows)
        phase, pos, kept_all = 0, 0, []
        while pos < n_rows or rng.random() < 0.2:              # (empty feeds too, and some behind the end)
            n = int(min(n_rows - pos, rng.integers(0, 12)))
            first, kept, after = stream_keep(phase, n, s)
            idx, want_after = R.feed_kept(phase, n, s)
            assert kept == len(idx) and after == want_after == (pos + n) % s
            assert idx == [first + j * s for j in range(kept)]
            assert kept <= -(-n // s) and (kept == 0 or first + (kept - 1) * s < n)     # what skip_rows_kernel relies on
            kept_all.extend(rows[pos:pos + n][first::s][:kept].tolist())
            assert rows[pos:pos + n][first::s].size == kept
            phase, pos = after, pos + n
        assert kept_all == rows[::s].tolist()


def test_the_issues_stream_splits():
    """the GPU test's feeds: 23 rows as [5, 1, 7, 0, 10] and 10 rows as [0, 4, 4, 2, 0], s = 3"""
    from neuralasr_amd.engine import stream_keep
    for splits, want in (([5, 1, 7, 0, 10], [2, 0, 3, 0, 3]), ([0, 4, 4, 2, 0], [0, 2, 1, 1, 0])):
        phase, got = 0, []
        for n in splits:
            _, kept, phase = stream_keep(phase, n, 3)
            got.append(kept)
        assert got == want and sum(got) == R.net_len(sum(splits), 3)


def test_align_frame_to_seconds():
    from neuralasr_amd import align

    class Symbols:
        def get_sym(self, i):
            return 'abc'[i]
    spans = [(0, 0, 1), (2, 4, 4)]
    for s, want in ((None, ['a 0.00 0.02', 'c 0.04 0.05']), (1, ['a 0.00 0.02', 'c 0.04 0.05']),
                    (3, ['a 0.00 0.06', 'c 0.12 0.15'])):
        cfg = types.SimpleNamespace(symbols=Symbols())
        if s is not None:
            cfg.frame_skip = s
        assert align.frame_seconds(cfg) == pytest.approx((s or 1) * 0.01)
        lines, score = align.report(cfg, True, -1.5, spans)
        assert lines == want and score == -1.5
    # a network's logit frames have a time when there is one per frame it sees
    def net(s, frames):
        return types.SimpleNamespace(config=types.SimpleNamespace(frame_skip=s),
                                     engine=types.SimpleNamespace(logit_frames=frames))
    assert align.frames_have_time(net(3, lambda T: -(-T // 3)))
    assert align.frames_have_time(net(1, lambda T: T))
    assert not align.frames_have_time(net(3, lambda T: 2 * -(-T // 3)))
    assert not align.frames_have_time(net(1, lambda T: 2 * T))


def test_lib_declares_both_calls():
    from neuralasr_amd import _lib
    header = open(os.path.join(os.path.dirname(HERE), 'include', 'nasr.h')).read()
    for name in ('nasr_set_frame_skip', 'nasr_get_frame_skip'):
        assert name in _lib.SYMBOLS
        assert re.search(r'\bint %s\(nasr_handle h, int\*? s\);' % name, header), name
    lib = _lib.load()
    assert len(lib.nasr_set_frame_skip.argtypes) == 2 and len(lib.nasr_get_frame_skip.argtypes) == 2
