"""Host side of the waveform augmentation of `train --from-audio`: the draws of kinds 3 to 5 of
augment.Augmenter (and kinds 0 to 2 as they were), prepare_rir, the list files, the config keys and their refusals, the
arrays an AudioBatch carries through shard(), the C ABI, and the rules' own float64 restatement.  No GPU."""
import ctypes
import os

import numpy as np
import pytest

import wave_aug_ref as ref
from test_augment_host import ROOT, SR, cfg_ns, make_corpus


def write_banks(d, noise_secs=(0.11, 0.3, 0.05), rir_taps=(40, 700, 9), noise_rate=SR):
    """three noise WAVs and three RIR WAVs with their list files under d: (noise_list, rir_list)"""
    from neuralasr_amd.features import write_wav16
    rs = np.random.RandomState(17)
    os.makedirs(str(d), exist_ok=True)
    lists = []
    for kind, sizes in (('noise', [int(noise_rate * s) for s in noise_secs]), ('rir', list(rir_taps))):
        names = []
        for i, n in enumerate(sizes):
            a = 0.05 * rs.randn(n)
            if kind == 'rir':                 # a direct path behind 3 samples of delay, then a decaying tail
                a = 0.3 * rs.randn(n) * np.exp(-np.arange(n) / (0.3 * n))
                a[:3] *= 0.01
                a[3] = 0.9
            names.append('%s%d.wav' % (kind, i))
            write_wav16(os.path.join(str(d), names[-1]), a, noise_rate if kind == 'noise' else SR)
        path = os.path.join(str(d), kind + '.lst')
        with open(path, 'w') as fh:
            fh.write('# %s files\n\n' % kind + '\n'.join(names) + '\n')      # relative to the list file
        lists.append(path)
    return tuple(lists)


def wave_ns(d, **kw):
    noise_list, rir_list = write_banks(d)
    base = dict(noise_list=noise_list, rir_list=rir_list, noise_prob=0.6, rir_prob=0.5, noise_snr=(-5.0, 25.0), augment_seed=3)
    base.update(kw)
    return cfg_ns(**base)


# ---------------------------------------------------------------------------------------------------- draws
def test_wave_draws_are_in_range_and_follow_their_rules(tmp_path):
    from neuralasr_amd.augment import KIND_NOISE, KIND_PLACE, KIND_RIR, Augmenter, unit
    a = Augmenter(wave_ns(tmp_path))
    assert a.clip_len == [int(SR * 0.11), int(SR * 0.3), int(SR * 0.05)] and a.n_rirs == 3
    B = 16
    seen_r, seen_c, none_r, none_c = set(), set(), 0, 0
    for counter in range(1, 30):
        rir, noise, off, snr = a.wave(counter, B)
        assert rir.dtype == noise.dtype == np.int32 and off.dtype == np.int64 and snr.dtype == np.float32
        assert rir.shape == noise.shape == off.shape == snr.shape == (B,)
        for i in range(B):
            r0, r1 = a.raw(counter, i, KIND_RIR)
            assert rir[i] == (r1 % 3 if unit(r0) < 0.5 else -1)
            r0, r1 = a.raw(counter, i, KIND_NOISE)
            if unit(r0) < 0.6:
                c = r1 % 3
                p0, p1 = a.raw(counter, i, KIND_PLACE)
                assert noise[i] == c and off[i] == p0 % a.clip_len[c] and 0 <= off[i] < a.clip_len[c]
                assert snr[i] == np.float32(-5.0 + 30.0 * unit(p1)) and -5.0 <= snr[i] <= 25.0
            else:
                assert noise[i] == -1 and off[i] == 0 and snr[i] == 0
        seen_r.update(int(v) for v in rir)
        seen_c.update(int(v) for v in noise)
        none_r += int(np.sum(rir < 0))
        none_c += int(np.sum(noise < 0))
    assert seen_r == {-1, 0, 1, 2} and seen_c == {-1, 0, 1, 2}
    n = 29 * B                               # 464 draws: the shares are near 0.5 and 0.4 (5 sigma of a binomial is 0.12)
    assert abs(none_r / n - 0.5) < 0.12 and abs(none_c / n - 0.4) < 0.12
    assert 0.0 <= unit(0) < unit((1 << 64) - 1) < 1.0


def test_wave_draws_are_a_pure_function_of_their_key(tmp_path):
    from neuralasr_amd.augment import KIND_NOISE, KIND_PLACE, KIND_RIR, Augmenter
    ns = wave_ns(tmp_path, noise_prob=1.0, rir_prob=1.0)
    a = Augmenter(ns)
    first = a.wave(7, 6)
    np.random.seed(5)
    np.random.rand(3)
    a.wave(9, 4)
    a.masks(7, [50, 60])
    again = Augmenter(ns).wave(7, 6)
    assert all(np.array_equal(x, y) for x, y in zip(first, again))
    for kind in (KIND_RIR, KIND_NOISE, KIND_PLACE):
        base = a.raw(7, 1, kind)
        ns1 = wave_ns(tmp_path, augment_seed=4)
        others = [Augmenter(ns1).raw(7, 1, kind), a.raw(8, 1, kind), Augmenter(ns, rank=1).raw(7, 1, kind), a.raw(7, 2, kind)]
        others += [a.raw(7, 1, k) for k in range(6) if k != kind]
        assert len({base, *others}) == 10    # seed, counter, rank, utterance and kind: each one matters
    # an utterance's draws do not depend on what stands beside it, and change with the counter
    assert all(np.array_equal(x[:3], y) for x, y in zip(first, a.wave(7, 3)))
    assert not all(np.array_equal(x, y) for x, y in zip(first, a.wave(8, 6)))
    # a kind that is off gives no array, and the other kind's draws stay
    only_noise = Augmenter(wave_ns(tmp_path, noise_prob=1.0, rir_list=None)).wave(7, 6)
    assert only_noise[0] is None and all(np.array_equal(x, y) for x, y in zip(only_noise[1:], first[1:]))
    only_rir = Augmenter(wave_ns(tmp_path, rir_prob=1.0, noise_list=None)).wave(7, 6)
    assert np.array_equal(only_rir[0], first[0]) and only_rir[1:] == (None, None, None)
    off = Augmenter(cfg_ns())
    assert off.wave(7, 6) == (None, None, None, None)


def test_kinds_0_to_2_draw_what_they_drew_before():
    """values recorded from the commit before the waveform kinds were added: same seed, counter, rank, utterance, kind"""
    from neuralasr_amd.augment import KIND_FREQ, KIND_SPEED, KIND_TIME, Augmenter
    assert (KIND_SPEED, KIND_TIME, KIND_FREQ) == (0, 1, 2)
    a = Augmenter(cfg_ns(speed_perturb=(0.9, 1.0, 1.1), augment_seed=7), rank=1)
    assert a.raw(5, 2, 0, 0) == (16956493743443214531, 134460585232940179)
    assert a.raw(5, 2, 1, 3) == (11216491071506481057, 7145790089430682533)
    assert a.raw(5, 2, 2, 1) == (1515019005672624212, 8255717536768630351)
    assert a.speed(11, [4000, 2400, 3000], None, None) == ([8000, 8800, 8000], [1.0, 1.1, 1.0])
    tm, fm = a.masks(11, [50, 7, 200])
    assert tm.tolist() == [[[43, 2], [14, 10]], [[6, 0], [0, 7]], [[105, 1], [187, 1]]]
    assert fm.tolist() == [[[1, 0], [9, 3]], [[2, 1], [0, 1]], [[6, 2], [7, 5]]]


def test_batch_carries_the_draws_and_shard_slices_them(tmp_path):
    from neuralasr_amd.augment import Augmenter
    from neuralasr_amd.features import AudioBatch
    from neuralasr_amd.networks.hipnetwork import take_shard
    rs = np.random.RandomState(0)
    audios = [0.1 * rs.randn(n).astype(np.float32) for n in (4000, 2400, 3000, 1700)]
    a = Augmenter(wave_ns(tmp_path, noise_prob=1.0, rir_prob=1.0))
    b = a.batch(4, audios, None)
    rir, noise, off, snr = a.wave(4, 4)
    assert np.array_equal(b.rir, rir) and np.array_equal(b.noise, noise) and np.array_equal(b.noise_off, off)
    assert np.array_equal(b.snr_db, snr) and b.time_masks is not None
    w = b.wave()
    assert w.rir is b.rir and w.noise is b.noise and w.noise_off is b.noise_off and w.snr_db is b.snr_db
    labels, ll = np.zeros((4, 2), np.int32), [1, 1, 1, 1]
    for n, k, lo, hi in ((2, 0, 0, 2), (2, 1, 2, 4), (4, 3, 3, 4)):
        f = take_shard(b, labels, b.seq_len, ll, n, k)[0]
        assert np.array_equal(f.rir, rir[lo:hi]) and np.array_equal(f.noise, noise[lo:hi])
        assert np.array_equal(f.noise_off, off[lo:hi]) and np.array_equal(f.snr_db, snr[lo:hi])
        assert np.array_equal(f.time_masks, b.time_masks[lo:hi]) and len(f) == hi - lo
    plain = AudioBatch(SR, audios)
    assert plain.wave() is None and plain.shard(1, 3).rir is None and plain.shard(1, 3).snr_db is None
    with pytest.raises(ValueError, match='rir must hold 4 values'):
        AudioBatch(SR, audios, rir=[0, 1])
    with pytest.raises(ValueError, match='noise needs noise_off and snr_db'):
        AudioBatch(SR, audios, noise=[0, 1, 0, -1])


# ---------------------------------------------------------------------------------------------------- banks
def test_prepare_rir():
    from neuralasr_amd.augment import MAX_RIR_TAPS, prepare_rir
    rs = np.random.RandomState(1)
    for n, peak in ((1, 0), (50, 0), (50, 17), (9000, 5), (20000, 9000), (8192, 0)):
        h = 0.2 * rs.randn(n)
        h[peak] = -3.0 if n % 2 else 3.0
        p = prepare_rir(h)
        assert p.dtype == np.float32 and p.size == min(n - peak, MAX_RIR_TAPS) <= 8192
        assert int(np.argmax(np.abs(p))) == 0                                   # the direct path is tap 0
        assert abs(float(np.sum(p.astype(np.float64) ** 2)) - 1.0) < 1e-6       # unit energy, up to the float32 cast
        kept = h[peak:peak + MAX_RIR_TAPS]
        assert np.array_equal(p, (kept / np.sqrt(np.sum(kept * kept))).astype(np.float32))
    assert MAX_RIR_TAPS == 8192
    for bad in ([], [0.0, 0.0], [1.0, np.nan], [np.inf]):
        with pytest.raises(ValueError, match='finite, non-zero'):
            prepare_rir(bad)


def test_list_files_and_clip_lengths(tmp_path):
    from neuralasr_amd.augment import clip_length, read_list
    from neuralasr_amd.features import resample_length
    noise_list, rir_list = write_banks(tmp_path, noise_rate=16000)
    paths = read_list(noise_list)
    assert [os.path.basename(p) for p in paths] == ['noise0.wav', 'noise1.wav', 'noise2.wav'] and all(os.path.isabs(p) for p in paths)
    # a clip at another rate counts the samples it has once it is resampled
    assert [clip_length(p, SR) for p in paths] == [resample_length(int(16000 * s), 16000, SR)[0] for s in (0.11, 0.3, 0.05)]
    assert [clip_length(p, 16000) for p in paths] == [int(16000 * s) for s in (0.11, 0.3, 0.05)]
    assert [clip_length(p, SR) for p in read_list(rir_list)] == [40, 700, 9]
    empty = tmp_path / 'empty.lst'
    empty.write_text('# nothing\n\n')
    with pytest.raises(ValueError, match='lists no WAV file'):
        read_list(str(empty))


# ---------------------------------------------------------------------------------------------------- config
def test_config_keys_defaults_and_refusals(tmp_path):
    from neuralasr_amd.config import Config
    cfg_path, _ = make_corpus(tmp_path)
    c = Config(str(cfg_path), True)
    assert (c.noise_list, c.rir_list, c.noise_prob, c.rir_prob, c.wave_on, c.augment_on) == (None, None, 0.0, 0.0, False, False)
    cfg_path, _ = make_corpus(tmp_path, extra='noise_list=/x/noise.lst\n')
    c = Config(str(cfg_path), True)
    assert (c.noise_list, c.noise_prob, c.noise_snr, c.rir_list, c.rir_prob) == ('/x/noise.lst', 1.0, (10.0, 20.0), None, 0.0)
    assert c.wave_on and c.augment_on
    cfg_path, _ = make_corpus(tmp_path, extra='noise_list=n.lst\nnoise_prob=0.25\nnoise_snr=-5, 40\nrir_list=r.lst\nrir_prob=0.5\n')
    c = Config(str(cfg_path), True)
    assert (c.noise_list, c.noise_prob, c.noise_snr, c.rir_list, c.rir_prob) == ('n.lst', 0.25, (-5.0, 40.0), 'r.lst', 0.5)
    cfg_path, _ = make_corpus(tmp_path, extra='noise_list=n.lst\nnoise_prob=0\nrir_list=r.lst\nrir_prob=0.0\n')
    c = Config(str(cfg_path), True)
    assert not c.wave_on and not c.augment_on                                   # lists with probability 0: off
    cfg_path, _ = make_corpus(tmp_path, extra='noise_list=n.lst\nnoise_snr=7,7\n')
    assert Config(str(cfg_path), True).noise_snr == (7.0, 7.0)
    both = 'noise_list=n.lst\nrir_list=r.lst\n'
    for bad, text in ((both + 'noise_prob=1.5', "'noise_prob' must be a number in [0,1], not '1.5'"),
                      (both + 'noise_prob=-0.1', "'noise_prob' must be a number in [0,1], not '-0.1'"),
                      (both + 'noise_prob=often', "'noise_prob' must be a number in [0,1], not 'often'"),
                      (both + 'rir_prob=2', "'rir_prob' must be a number in [0,1], not '2'"),
                      (both + 'rir_prob=nan', "'rir_prob' must be a number in [0,1], not 'nan'"),
                      (both + 'noise_snr=20,10', "'noise_snr' must be lo,hi in dB with lo <= hi, not '20,10'"),
                      (both + 'noise_snr=10', "'noise_snr' must be lo,hi in dB with lo <= hi, not '10'"),
                      (both + 'noise_snr=0,inf', "'noise_snr' must be lo,hi in dB with lo <= hi, not '0,inf'"),
                      (both + 'noise_snr=a,b', "'noise_snr' must be lo,hi in dB with lo <= hi, not 'a,b'"),
                      (both + 'noise_snr=1,2,3', "'noise_snr' must be lo,hi in dB with lo <= hi, not '1,2,3'"),
                      ('noise_list=', "'noise_list' must name a file that lists WAV paths"),
                      ('rir_list=', "'rir_list' must name a file that lists WAV paths"),
                      ('noise_prob=0.5', "'noise_prob' needs 'noise_list'"),
                      ('noise_snr=0,10', "'noise_snr' needs 'noise_list'"),
                      ('noise_list=n.lst\nrir_prob=0.5', "'rir_prob' needs 'rir_list'")):
        cfg_path, _ = make_corpus(tmp_path, extra=bad + '\n')
        with pytest.raises(ValueError) as e:
            Config(str(cfg_path), True)
        assert text in str(e.value) and str(cfg_path) in str(e.value), (bad, str(e.value))


def test_train_without_from_audio_refuses_the_keys(tmp_path):
    from neuralasr_amd import train
    noise_list, rir_list = write_banks(tmp_path / 'banks')
    for extra in ('noise_list=%s\n' % noise_list, 'rir_list=%s\nrir_prob=0.3\n' % rir_list):
        cfg_path, _ = make_corpus(tmp_path, extra=extra)
        with pytest.raises(ValueError) as e:
            train.main([str(cfg_path)])
        assert 'noise_list, rir_list) need --from-audio' in str(e.value)
    cfg_path, _ = make_corpus(tmp_path, rand_shift=3, extra='noise_list=%s\n' % noise_list)
    with pytest.raises(ValueError, match='rand_shift'):
        train.main([str(cfg_path), '--from-audio'])


def test_training_feed_draws_and_validation_feed_does_not(tmp_path):
    """the feed of `train --from-audio` with the keys on: the training batches carry the draws of the step they train, the
    validation batches none"""
    from neuralasr_amd import train
    from neuralasr_amd.config import Config
    noise_list, rir_list = write_banks(tmp_path / 'banks')
    keys = 'noise_list=%s\nnoise_snr=0,30\nrir_list=%s\nrir_prob=0.5\naugment_seed=9\nsym_file=${MFCC Featurizer:output}/symbols\n'
    cfg_path, out = make_corpus(tmp_path, extra=keys % (noise_list, rir_list))
    os.makedirs(str(out), exist_ok=True)
    config = Config(str(cfg_path), True)
    feed, valid = train.audio_datasets(str(cfg_path), config)
    b, _, _, _ = feed.get_next_batch()
    want = feed.augmenter.wave(1, len(b))
    assert all(np.array_equal(x, y) for x, y in zip((b.rir, b.noise, b.noise_off, b.snr_db), want))
    assert (b.noise >= 0).all() and b.time_masks is None and b.wave() is not None
    b2, _, _, _ = feed.get_next_batch()
    assert all(np.array_equal(x, y) for x, y in zip((b2.rir, b2.noise, b2.noise_off, b2.snr_db), feed.augmenter.wave(2, len(b2))))
    if valid is not None:
        v, _, _, _ = valid.get_next_batch()
        assert v.wave() is None and v.rir is None and v.noise is None


# ---------------------------------------------------------------------------------------------------- ABI
def test_wave_symbols_and_struct_layout(tmp_path):
    import shutil
    import subprocess
    from neuralasr_amd import _lib
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    H, fp, ip = ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32)
    lp, cp, ap = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int), ctypes.POINTER(_lib.BatchAug)
    wp, ci = ctypes.POINTER(_lib.WaveAug), ctypes.c_int
    audio = [H, H, fp, lp, ip, ip, ip, ci, ci, ip, cp]
    for name, args in (('nasr_upload_batch_audio_wave', audio + [ap, wp]), ('nasr_stage_batch_audio_wave', audio + [ap, wp, cp]),
                       ('nasr_featurizer_set_noise', [H, fp, lp, ci]), ('nasr_featurizer_set_rirs', [H, fp, lp, ci]),
                       ('nasr_augment_audio', [H, fp, lp, ip, ci, wp, fp, ctypes.c_int64])):
        assert name in _lib.SYMBOLS
        assert hasattr(raw, name), name + ' is not exported by libnasr.so'
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args
    header = open(os.path.join(ROOT, 'include', 'nasr.h')).read()
    assert '#define NASR_AUG_MAX_RIR_TAPS 8192' in header and _lib.AUG_MAX_RIR_TAPS == 8192
    for name in ('nasr_upload_batch_audio_wave', 'nasr_featurizer_set_noise', 'nasr_featurizer_set_rirs', 'nasr_augment_audio'):
        decl = header[:header.index('int ' + name + '(')]
        assert '(No counterpart in the reference' in decl[decl.rindex('/*'):], name
    W = _lib.WaveAug
    assert [n for n, _ in W._fields_] == ['rir', 'noise', 'noise_off', 'snr_db']
    assert (W.rir.offset, W.noise.offset, W.noise_off.offset, W.snr_db.offset, ctypes.sizeof(W)) == (0, 8, 16, 24, 32)
    gcc = shutil.which('gcc')
    if gcc:                                              # the layout a C caller sees
        src = tmp_path / 'wave.c'
        src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "nasr.h"\nint main(void) {\n'
                       '  printf("%zu %zu %zu %zu %zu %d\\n", sizeof(nasr_wave_aug), offsetof(nasr_wave_aug, rir),\n'
                       '         offsetof(nasr_wave_aug, noise), offsetof(nasr_wave_aug, noise_off), offsetof(nasr_wave_aug, snr_db),\n'
                       '         NASR_AUG_MAX_RIR_TAPS);\n  return 0;\n}\n')
        exe = tmp_path / 'wave'
        r = subprocess.run([gcc, '-std=c99', '-Wall', '-Werror', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
        assert [int(x) for x in out.stdout.split()] == [32, 0, 8, 16, 24, 8192]


def test_engine_wave_struct_checks_shapes():
    from neuralasr_amd.engine import WaveAug
    st, keep = WaveAug([0, -1, 2], None, None, None).struct(3)
    assert [st.rir[i] for i in range(3)] == [0, -1, 2] and not st.noise and not st.noise_off and not st.snr_db
    assert keep[0].dtype == np.int32
    st, keep = WaveAug(None, [1, -1], [5, 0], [12.5, 0]).struct(2)
    assert not st.rir and [st.noise[i] for i in range(2)] == [1, -1] and st.noise_off[0] == 5 and st.snr_db[0] == 12.5
    assert keep[2].dtype == np.int64 and keep[3].dtype == np.float32
    with pytest.raises(ValueError, match=r'rir must be \[B=4\]'):
        WaveAug([0, 1, 2], None, None, None).struct(4)


# ---------------------------------------------------------------------------------------------------- the rules
@pytest.mark.parametrize('snr', [-5.0, 0.0, 12.25, 40.0])
def test_reference_reaches_the_requested_snr(snr):
    """on the float64 restatement alone: 10 log10(Ps / (g^2 Pn)) is the request to 1e-9 dB, for a clip that wraps, a
    clip of one sample and one longer than the utterance, at a non-zero offset"""
    rs = np.random.RandomState(3)
    y = (0.1 * rs.randn(1000)).astype(np.float32)
    for L, off in ((37, 0), (37, 36), (1, 0), (5000, 4321)):
        clip = (0.3 * rs.randn(L)).astype(np.float32)
        n = ref.noise_track(clip, off, y.size)
        assert n.shape == y.shape and n[0] == clip[off] and n[-1] == clip[(off + 999) % L]
        g = ref.gain64(y, n, snr)
        assert abs(ref.snr_db(y, g * n.astype(np.float64)) - snr) < 1e-9
    assert ref.gain64(np.zeros(10, np.float32), np.ones(10, np.float32), snr) == 0.0
    assert ref.gain64(np.ones(10, np.float32), np.zeros(10, np.float32), snr) == 0.0


def test_reference_fir_is_the_truncated_convolution():
    rs = np.random.RandomState(4)
    x = rs.randn(20).astype(np.float32)
    for K in (1, 2, 20, 31):
        h = rs.randn(K).astype(np.float32)
        y, mag = ref.fir(x, h)
        want = [sum(float(h[k]) * float(x[t - k]) for k in range(min(K - 1, t) + 1)) for t in range(20)]
        assert y.shape == (20,) and np.allclose(y, want, rtol=1e-13, atol=1e-13) and (mag >= np.abs(y) - 1e-12).all()
    assert np.array_equal(ref.fir(x, [1.0])[0], x.astype(np.float64))
    assert ref.gamma(8192) == 8192 * ref.U / (1 - 8192 * ref.U)
