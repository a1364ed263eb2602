"""tests/lc_train_ref.py (the fp64 model of latency-controlled training) against the look-ahead session's
reference, against the oracle in the limiting case, and against central differences; the chunk_frames config key.  CPU only."""
import numpy as np
import pytest

from oracle import nasr_oracle as O
from tests import lc_train_ref as LC
from tests import lookahead_ref as LR

SPEC = O.ModelSpec(7, 6, 2, True, 'concat', 5)
SPEC3 = O.ModelSpec(5, 4, 3, True, 'concat', 5)


def rand_params(spec, seed):
    rs = np.random.RandomState(seed)
    return [p + 0.05 * rs.randn(*p.shape) for p in O.init_params(spec, seed=seed)]


# ------------------------------------------------------------------------------------------- the window arithmetic
def test_windows():
    # T_b <= C + R: one window, the whole utterance
    assert LC.windows(1, 4, 3) == [(0, 1, 1)]
    assert LC.windows(7, 4, 3) == [(0, 7, 7)]
    # T_b = jC + R: the window that reaches the end is the last (no window of R rows behind it)
    assert LC.windows(11, 4, 3) == [(0, 7, 4), (4, 7, 7)]
    assert LC.windows(15, 4, 3) == [(0, 7, 4), (4, 7, 4), (8, 7, 7)]
    # T_b = jC + R + 1
    assert LC.windows(8, 4, 3) == [(0, 7, 4), (4, 4, 4)]
    assert LC.windows(12, 4, 3) == [(0, 7, 4), (4, 7, 4), (8, 4, 4)]
    # C = 1: every row but the last R + 1 is a window of its own
    assert LC.windows(5, 1, 2) == [(0, 3, 1), (1, 3, 1), (2, 3, 3)]
    # R > C: windows overlap more than once
    assert LC.windows(23, 3, 7) == [(0, 10, 3), (3, 10, 3), (6, 10, 3), (9, 10, 3), (12, 10, 3), (15, 8, 8)]
    for T in range(1, 40):
        for C, R in ((4, 3), (1, 2), (3, 7), (5, 1), (50, 20)):
            w = LC.windows(T, C, R)
            assert sum(E for _, _, E in w) == T                                   # every row is emitted once
            assert all(s == k * C for k, (s, _, _) in enumerate(w))
            assert all(P == C + R and E == C for _, P, E in w[:-1])
            s, P, E = w[-1]
            assert E == P == T - s and R < P <= C + R or len(w) == 1
            feeds = LC.session_feeds(T, C, R)
            assert sum(feeds) == T and feeds[0] == min(T, C + R)


# ------------------------------------------------------------------------------------------- forward: the session's logits
@pytest.mark.parametrize('C,R', [(4, 3), (1, 2), (3, 7)])
def test_forward_is_the_session_fed_on_the_schedule(C, R):
    """lengths T_b <= C+R, = jC+R, = jC+R+1 and one more; the session is fed C+R, C, ..., remainder with `last` (an empty
    remainder: its flush of the R held rows, which the rule's last window has computed already)"""
    spec, params = SPEC, rand_params(SPEC, 3)
    lens = sorted({1, C + R, C + R + 1, 2 * C + R, 3 * C + R, 3 * C + R + 1, 4 * C + R + 2})
    T = max(lens)
    feats = np.random.RandomState(1).randn(len(lens), T, spec.feature_size)
    logits = LC.forward(spec, params, feats, lens, C, R)
    assert logits.shape == (T, len(lens), spec.num_classes)
    for b, n in enumerate(lens):
        feeds = LC.session_feeds(n, C, R)
        got, _ = LR.run_session(spec, params, feats[b, :n], feeds, R)
        got = np.concatenate(got)
        assert got.shape[0] == n
        assert np.abs(logits[:n, b] - got).max() <= 1e-10, (n, feeds)
        assert np.array_equal(logits[n:, b], np.tile(params[-1], (T - n, 1)))       # zero outputs: the bias


def test_the_split_matters():
    """... and it is not the whole-utterance network"""
    spec, params = SPEC, rand_params(SPEC, 3)
    feats = np.random.RandomState(2).randn(1, 19, spec.feature_size)
    a = LC.forward(spec, params, feats, [19], 4, 3)
    b = O.network_forward(spec, params, feats, [19])[0]
    assert np.abs(a - b).max() > 1e-6


# ------------------------------------------------------------------------------------------- the limiting case
def test_one_window_is_the_oracle():
    spec, params = SPEC, rand_params(SPEC, 4)
    feats, seq_len, labels, label_len = O.synth_batch(spec, 3, 12, seed=5, var_len=True, Lmin=1, Lmax=4)
    lo, nllo, go, logo = O.network_loss_and_grads(spec, params, feats, seq_len, labels, label_len)
    for C, R in ((8, 4), (1, 11), (12, 1), (100, 100)):
        loss, nll, grads, logits = LC.loss_and_grads(spec, params, feats, seq_len, labels, label_len, C, R)
        assert abs(loss - lo) <= 1e-9 * abs(lo)
        assert np.abs(nll - nllo).max() <= 1e-9 * np.abs(nllo).max()
        assert np.abs(logits - logo).max() <= 1e-9
        for (name, _), g, ref in zip(spec.param_shapes(), grads, go):
            assert np.linalg.norm(g - ref) <= 1e-9 * max(np.linalg.norm(ref), 1e-30), name


# ------------------------------------------------------------------------------------------- the gradient's carry path
def test_gradient_through_the_carry_by_central_differences():
    """forward kernel and bias of every layer at L = 3, a dozen entries each: the forward direction's parameters reach the
    loss through the state carried from window to window, which autograd must follow"""
    spec, params = SPEC3, rand_params(SPEC3, 6)
    C, R = 3, 2
    feats, seq_len, labels, label_len = O.synth_batch(spec, 2, 14, seed=7, var_len=True, Lmin=1, Lmax=3)
    seq_len = np.asarray([14, 9])
    assert len(LC.windows(14, C, R)) >= 4
    loss, _, grads, _ = LC.loss_and_grads(spec, params, feats, seq_len, labels, label_len, C, R)

    def f(p):
        lg = LC.forward(spec, p, feats, seq_len, C, R)
        return float(O.ctc_loss_and_grad(lg, labels, label_len, seq_len)[0].mean())

    assert abs(f(params) - loss) <= 1e-12
    rs = np.random.RandomState(8)
    eps = 1e-5
    for l in range(spec.num_layers):
        for pi in (4 * l, 4 * l + 1):                    # l/fw/kernel, l/fw/bias
            g = grads[pi]
            scale = np.abs(g).max()
            assert scale > 0
            for _ in range(12):
                idx = tuple(rs.randint(0, n) for n in g.shape)
                hi = [q.copy() for q in params]
                lo = [q.copy() for q in params]
                hi[pi][idx] += eps
                lo[pi][idx] -= eps
                num = (f(hi) - f(lo)) / (2 * eps)
                assert abs(num - g[idx]) <= 1e-6 * max(abs(g[idx]), scale), (spec.param_shapes()[pi][0], idx, num, g[idx])


# ------------------------------------------------------------------------------------------- config key, command line
def _config(tmp_path, extra=''):
    from neuralasr_amd.config import Config
    p = tmp_path / 'c.config'
    p.write_text('[Parameters]\nsamplerate=8000\nnumcep=13\nnumcontext=2\nlabel_context=0\nbatch_size=2\nepochs=1\n'
                 'learningrate=0.001\nmodel_dir=%s\nstart_step=0\nreport_step=1\nnum_gpus=1\npunc_regex=[^a-z0-9 ]\n'
                 'network=networks.bilstm_ctc_net.BiLstm3x500CTCNet\n%s[Train]\n[Test]\ninput=%s\n[MFCC Featurizer]\n'
                 % (tmp_path / 'model', extra, tmp_path / 'test.scp'))
    return Config(str(p))


def test_config_key(tmp_path, caplog):
    import logging
    from neuralasr_amd.config import log
    assert _config(tmp_path).chunk_frames == 0
    assert _config(tmp_path, 'stream_lookahead=20\n').chunk_frames == 0
    c = _config(tmp_path, 'chunk_frames=50\nstream_lookahead=20\n')
    assert (c.chunk_frames, c.stream_lookahead) == (50, 20)
    assert _config(tmp_path, 'chunk_frames=0\n').chunk_frames == 0
    assert _config(tmp_path, 'chunk_frames=4096\nstream_lookahead=1\n').chunk_frames == 4096
    with caplog.at_level(logging.INFO, logger=log.name):
        c.print_config()
    assert 'chunk_frames=50' in caplog.text
    for bad in ('-1', '4097', 'some'):
        with pytest.raises(ValueError, match='chunk_frames'):
            _config(tmp_path, 'chunk_frames=%s\nstream_lookahead=4\n' % bad)
    # chunk_frames without a look-ahead: the message names both keys
    for extra in ('chunk_frames=50\n', 'chunk_frames=50\nstream_lookahead=0\n'):
        with pytest.raises(ValueError) as e:
            _config(tmp_path, extra)
        assert 'chunk_frames' in str(e.value) and 'stream_lookahead' in str(e.value)


def test_decode_wav_takes_its_default_chunk_from_the_key():
    from neuralasr_amd import decode_wav
    a = decode_wav.parse_args(['c', 'w', '--stream'])
    assert a.chunk_frames == 50 and not a.chunk_frames_given
    a = decode_wav.parse_args(['c', 'w', '--stream', '--chunk-frames', '50'])
    assert a.chunk_frames == 50 and a.chunk_frames_given


def test_binding_lists_the_calls():
    from neuralasr_amd import _lib
    assert 'nasr_set_chunking' in _lib.SYMBOLS and 'nasr_get_chunking' in _lib.SYMBOLS
