"""GPU: the waveform augmentation of a batch given as audio (neuralasr_amd/csrc/wave_aug.hip behind
nasr_augment_audio / nasr_upload_batch_audio_wave / nasr_stage_batch_audio_wave).  The FIR and the mix against the float64
restatement of tests/wave_aug_ref.py under bounds that follow from float32 arithmetic alone; batch invariance, and the
whole path into a model handle, as bits."""
import ctypes
import os

import numpy as np
import pytest

import wave_aug_ref as ref
from test_gpu_audio_batch import C, assert_same, init, lstm, observe, same, state
from test_gpu_augment import loop_config, ragged_labels, run_loop, same_checkpoint
from test_gpu_mfcc import speech_like
from test_wave_aug_host import write_banks

pytestmark = pytest.mark.gpu

SR = 16000
# the issue's sizes, and the edges of this implementation: a tile is 1024 outputs, a chunk 512 taps, a turn of the inner
# loop 16 taps
FIR_N = (1, 63, 64, 65, 300, 1000, 1024, 1025, 4097)
FIR_K = (1, 2, 15, 16, 17, 64, 65, 512, 513, 1025, 8192)


def rng_f32(seed, n, scale=1.0):
    return (scale * np.random.RandomState(seed).randn(n)).astype(np.float32)


def fir_taps(K):
    """K taps of a decaying tail behind a direct path, unit energy: what prepare_rir hands over"""
    h = np.random.RandomState(1000 + K).randn(K) * np.exp(-np.arange(K) / (0.25 * K + 1))
    h[0] = 1.0
    return (h / np.sqrt(np.sum(h * h))).astype(np.float32)


RIRS = [fir_taps(K) for K in FIR_K] + [np.array([1.0], np.float32)]
UNIT = len(FIR_K)                                   # the index of h = [1.0]
# clips: one that wraps several times in any utterance, one sample, one longer than the utterances, digital silence
CLIPS = [rng_f32(21, 37, 0.2), np.array([0.25], np.float32), rng_f32(22, 5000, 0.05), np.zeros(50, np.float32), rng_f32(23, 700, 0.1)]
WRAP, ONE, LONG, SILENT, MID = range(5)


@pytest.fixture(scope='module')
def fz():
    from neuralasr_amd.features import Featurizer
    f = Featurizer(SR, 13, 2)
    f.set_rirs(RIRS)
    f.set_noise(CLIPS)
    yield f
    f.close()


def wave(B, rir=None, noise=None, off=None, snr=None):
    from neuralasr_amd.engine import WaveAug
    if noise is not None:
        off = [0] * B if off is None else off
        snr = [10.0] * B if snr is None else snr
    return WaveAug(rir, noise, off, snr)


# ---------------------------------------------------------------------------------------------------- the FIR
@pytest.mark.parametrize('ki', range(len(FIR_K)), ids=['K%d' % k for k in FIR_K])
def test_fir_is_within_the_dot_product_bound(fz, ki):
    """|y - y_ref| <= gamma_K sum_k |h[k] x[t-k]| with gamma_K = K u / (1 - K u), u = 2^-24: the bound of a length-K float32 dot
    product in any order.  One batch holds every N, so K > N (N = 1 ... 300 under K = 8192) and the tile edges are in it."""
    K, h = FIR_K[ki], RIRS[ki]
    xs = [rng_f32(10 * K + i, n, 0.3) for i, n in enumerate(FIR_N)]
    got = fz.augment_audio(xs, None, wave(len(xs), rir=[ki] * len(xs)))
    for n, x, y in zip(FIR_N, xs, got):
        want, mag = ref.fir(x, h)
        assert y.dtype == np.float32 and y.shape == (n,)
        err = np.abs(y.astype(np.float64) - want)
        bound = ref.gamma(K) * mag
        worst = int(np.argmax(err - bound))
        assert (err <= bound).all(), 'N %d K %d: sample %d off by %g, bound %g' % (n, K, worst, err[worst], bound[worst])
        if K > 1 and n > 1:
            assert not same(y, x)


def test_unit_impulse_gives_the_input(fz):
    xs = [rng_f32(3 + i, n, 0.3) for i, n in enumerate(FIR_N)]
    got = fz.augment_audio(xs, None, wave(len(xs), rir=[UNIT] * len(xs)))
    for x, y in zip(xs, got):
        assert np.array_equal(y, x)


# ---------------------------------------------------------------------------------------------------- the mix
MIX_CASES = [  # (N, clip, offset, snr_db)
    (1000, WRAP, 0, -5.0), (1000, WRAP, 36, 40.0), (4097, WRAP, 11, 40.0), (1000, ONE, 0, -5.0), (65, ONE, 0, 40.0),
    (1000, LONG, 4321, -5.0), (2049, LONG, 4999, 40.0), (1, WRAP, 5, -5.0), (1025, MID, 699, 12.5),
]


def test_mix_is_within_three_roundings_and_reaches_the_snr(fz):
    """|z - z_ref| <= 4u (|y| + |g n|): the gain's rounding (and one more for its last bit, the float64 sums being taken in
    another order), the product's and the sum's.  The achieved SNR of the returned waveform, in float64, is the request
    to 1e-3 dB."""
    xs = [rng_f32(40 + i, c[0], 0.3) for i, c in enumerate(MIX_CASES)]
    B = len(xs)
    w = wave(B, noise=[c[1] for c in MIX_CASES], off=[c[2] for c in MIX_CASES], snr=[c[3] for c in MIX_CASES])
    got = fz.augment_audio(xs, None, w)
    for (n, clip, off, snr), x, z in zip(MIX_CASES, xs, got):
        want, g, track = ref.mix(x, CLIPS[clip], off, snr)
        assert g > 0 and z.shape == (n,)
        err = np.abs(z.astype(np.float64) - want)
        bound = 4 * ref.U * (np.abs(x.astype(np.float64)) + np.abs(np.float64(g) * track.astype(np.float64)))
        worst = int(np.argmax(err - bound))
        assert (err <= bound).all(), 'case %r: sample %d off by %g, bound %g' % ((n, clip, off, snr), worst, err[worst], bound[worst])
        achieved = ref.snr_db(x, z.astype(np.float64) - x.astype(np.float64))
        assert abs(achieved - snr) < 1e-3, ((n, clip, off, snr), achieved)


def test_silence_on_either_side_leaves_the_input(fz):
    """an all-zero clip (Pn = 0) and an all-zero utterance (Ps = 0): g = 0, the output is the input"""
    x = rng_f32(60, 1000, 0.3)
    zero = np.zeros(777, np.float32)
    got = fz.augment_audio([x, zero, x], None, wave(3, noise=[SILENT, WRAP, -1], off=[7, 3, 0], snr=[5.0, 5.0, 0.0]))
    assert same(got[0], x) and same(got[1], zero) and same(got[2], x)


def test_reverberation_comes_first_and_the_snr_is_taken_against_it(fz):
    ki = FIR_K.index(513)
    x = rng_f32(61, 3000, 0.3)
    y = fz.augment_audio([x], None, wave(1, rir=[ki]))[0]
    z = fz.augment_audio([x], None, wave(1, rir=[ki], noise=[MID], off=[123], snr=[7.0]))[0]
    assert abs(ref.snr_db(y, z.astype(np.float64) - y.astype(np.float64)) - 7.0) < 1e-3
    want, g, track = ref.mix(y, CLIPS[MID], 123, 7.0)
    bound = 4 * ref.U * (np.abs(y.astype(np.float64)) + np.abs(np.float64(g) * track.astype(np.float64)))
    assert (np.abs(z.astype(np.float64) - want) <= bound).all()


# ---------------------------------------------------------------------------------------------------- bitwise
def mixed_batch():
    """RIR only, noise only, both, neither (with -0.0f samples), and one resampled from 44.1 kHz with both"""
    audios = [speech_like(5000, SR, 1), speech_like(2100, SR, 2), speech_like(7001, SR, 3), speech_like(1300, SR, 4),
              speech_like(9000, 44100, 5)]
    audios[3][::7] = -0.0
    rates = [SR, SR, SR, SR, 44100]
    w = dict(rir=[FIR_K.index(1025), -1, FIR_K.index(8192), -1, FIR_K.index(65)], noise=[-1, WRAP, LONG, -1, MID],
             off=[0, 30, 4000, 0, 650], snr=[0.0, 3.0, 20.0, 0.0, -5.0])
    return audios, rates, w


def pick(w, idx):
    return wave(len(idx), **{k: [v[i] for i in idx] for k, v in w.items()})


def test_batch_invariance_and_repeatability(fz):
    audios, rates, w = mixed_batch()
    first = fz.augment_audio(audios, rates, pick(w, range(5)))
    first = [a.copy() for a in first]
    again = fz.augment_audio(audios, rates, pick(w, range(5)))
    for a, b in zip(first, again):
        assert same(a, b), 'two runs differ'
    plain = fz.resample(audios, rates)
    for i in range(5):
        alone = fz.augment_audio([audios[i]], [rates[i]], pick(w, [i]))[0]
        assert same(alone, first[i]), 'utterance %d alone differs from its place in the batch' % i
        assert same(first[i], plain[i]) == (i == 3)
    assert np.signbit(first[3][::7]).all() and same(first[3], audios[3])        # neither: the bits of nasr_resample's output
    perm = [4, 2, 0, 3, 1]
    shuffled = fz.augment_audio([audios[i] for i in perm], [rates[i] for i in perm], pick(w, perm))
    for k, i in enumerate(perm):
        assert same(shuffled[k], first[i]), 'utterance %d moved to place %d' % (i, k)
    # without a wave the call is nasr_resample; without rates the samples are taken as they are
    for a, b in zip(fz.augment_audio(audios, rates, None), plain):
        assert same(a, b)
    assert same(fz.augment_audio([audios[3]], None, None)[0], audios[3])
    t = fz.times()
    assert all(v >= 0 for v in t)


# ---------------------------------------------------------------------------------------------------- the whole path
def route_batch():
    audios, rates, w = mixed_batch()
    seq_labels = ragged_labels([10, 10, 10, 10, 10], False)
    return audios, rates, w, seq_labels[0], seq_labels[1]


def masks_for(seq):
    tm = np.zeros((len(seq), 2, 2), np.int32)
    fm = np.zeros((len(seq), 1, 2), np.int32)
    for b, n in enumerate(int(x) for x in seq):
        tm[b] = [(0, min(2, n)), (n // 2, min(3, n - n // 2))]
        fm[b] = [(b % 10, 3)]
    return tm, fm


@pytest.mark.parametrize('masked', [False, True], ids=['plain', 'masks'])
def test_upload_and_stage_are_bitwise_the_plain_upload_of_the_augmented_audio(fz, masked):
    """logits, loss, gradients and the parameters after a step of a small BiLSTM handle: nasr_upload_batch_audio_wave, and
    nasr_stage_batch_audio_wave followed by the commit, against nasr_upload_batch_audio(_aug) of nasr_augment_audio's
    output at the config rate"""
    from neuralasr_amd.engine import BatchAug
    audios, rates, w, labels, ll = route_batch()
    wv = pick(w, range(5))
    e = lstm(fz.width)
    before = state(e)
    try:
        z = [a.copy() for a in fz.augment_audio(audios, rates, wv)]
        seq, T = e.upload_batch_audio(fz, z, labels, ll, None)
        aug = BatchAug(13, *masks_for(seq)) if masked else None
        init(e)
        e.upload_batch_audio(fz, z, labels, ll, None, aug=aug)
        want = observe(e, 5, T)
        init(e)
        got_seq, got_T = e.upload_batch_audio(fz, audios, labels, ll, rates, aug=aug, wave=wv)
        assert [int(t) for t in got_seq] == [int(t) for t in seq] and got_T == T
        note = '(recurrence %r at create, %r now)' % (before, state(e))
        assert_same(observe(e, 5, T), want, 'synchronous ' + note)
        init(e)
        s_seq, s_T, ticket = e.stage_batch_audio(fz, audios, labels, ll, rates, aug=aug, wave=wv)
        assert ticket is not None and [int(t) for t in s_seq] == [int(t) for t in seq] and s_T == T
        e.commit_batch(ticket)
        assert_same(observe(e, 5, T), want, 'staged ' + note)
        # not vacuous: the un-augmented batch gives other logits
        init(e)
        e.upload_batch_audio(fz, audios, labels, ll, rates, aug=aug)
        assert not same(e.forward_resident(5, T), want['logits'])
    finally:
        e.close()


@pytest.mark.parametrize('family', ['wavenet', 'las'])
def test_whole_path_on_the_other_handles(fz, family):
    from neuralasr_amd.engine import LasEngine, WaveNetEngine
    audios, rates, w, _, _ = route_batch()
    labels, ll = ragged_labels([10] * 5, family == 'las')
    wv = pick(w, range(5))

    def make():                              # two handles: batch-norm and sampling state change with a step
        if family == 'wavenet':
            return init(WaveNetEngine(fz.width, C, num_blocks=1, rates=(1, 2), learning_rate=1e-3), seed=4)
        return init(LasEngine(fz.width, C, sampling_probability=0.1, seed=5, learning_rate=1e-3), seed=6)
    a, b = make(), make()
    try:
        z = [x.copy() for x in fz.augment_audio(audios, rates, wv)]
        _, T = a.upload_batch_audio(fz, z, labels, ll, None)
        b.upload_batch_audio(fz, audios, labels, ll, rates, wave=wv)
        assert_same(observe(b, 5, T, ctc=family != 'las'), observe(a, 5, T, ctc=family != 'las'))
    finally:
        a.close()
        b.close()


def test_null_wave_is_the_aug_call(fz):
    from neuralasr_amd.engine import BatchAug, WaveAug
    audios, rates, _, labels, ll = route_batch()
    e = lstm(fz.width)
    try:
        seq, T = e.upload_batch_audio(fz, audios, labels, ll, rates)
        aug = BatchAug(13, *masks_for(seq))
        st, keep = aug.struct(5)
        for masks in (None, ctypes.byref(st)):
            init(e)
            e.upload_batch_audio(fz, audios, labels, ll, rates, aug=aug if masks else None)
            want = observe(e, 5, T)
            init(e)
            rc, _, _ = e._audio_call(e.lib.nasr_upload_batch_audio_wave, fz, audios, labels, ll, rates, masks, None)
            assert rc == 0
            assert_same(observe(e, 5, T), want, 'wave = NULL')
            init(e)
            ticket = ctypes.c_int(-1)
            rc, _, _ = e._audio_call(e.lib.nasr_stage_batch_audio_wave, fz, audios, labels, ll, rates, masks, None, ctypes.byref(ticket))
            assert rc == 0 and ticket.value >= 0
            e.commit_batch(ticket.value)
            assert_same(observe(e, 5, T), want, 'staged, wave = NULL')
            init(e)
            e.upload_batch_audio(fz, audios, labels, ll, rates, aug=aug if masks else None, wave=WaveAug(None, None, None, None))
            assert_same(observe(e, 5, T), want, 'a wave without arrays')
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- errors
def test_banks_are_checked():
    from neuralasr_amd import _lib
    from neuralasr_amd.features import Featurizer
    f = Featurizer(SR, 13, 2)
    e = lstm(f.width)
    x = rng_f32(1, 500, 0.1)
    try:
        def refused(call, text, code=_lib.NASR_ERR_ARG):
            with pytest.raises(_lib.NasrError) as err:
                call()
            assert err.value.code == code and text in str(err.value), str(err.value)
        ok = np.ones(4, np.float32)
        refused(lambda: f.set_noise([ok, np.zeros(0, np.float32)]), 'nasr_featurizer_set_noise: noise clip 1 is empty')
        refused(lambda: f.set_noise([ok, ok, np.array([0, np.nan], np.float32)]), 'nasr_featurizer_set_noise: noise clip 2 holds a value that is not finite')
        refused(lambda: f.set_rirs([np.array([1, np.inf], np.float32)]), 'nasr_featurizer_set_rirs: RIR 0 holds a value that is not finite')
        refused(lambda: f.set_rirs([ok, np.zeros(0, np.float32)]), 'nasr_featurizer_set_rirs: RIR 1 is empty')
        refused(lambda: f.set_rirs([ok, ok, np.ones(8193, np.float32)]), 'nasr_featurizer_set_rirs: RIR 2 has 8193 taps')
        f.set_rirs([np.ones(8192, np.float32) / 8192])                            # the limit itself is taken
        for fn in (e.lib.nasr_featurizer_set_noise, e.lib.nasr_featurizer_set_rirs):
            assert fn(e.h, None, None, 0) == _lib.NASR_ERR_STATE                   # a model handle
        # no bank yet, a bank, the bank freed again
        refused(lambda: f.augment_audio([x], None, wave(1, noise=[0])), 'utterance 0 asks for noise clip 0, the featurizer has no noise bank')
        f.set_noise([ok])
        assert f.augment_audio([x], None, wave(1, noise=[0]))[0].shape == x.shape
        f.set_noise([])
        refused(lambda: f.augment_audio([x], None, wave(1, noise=[0])), 'has no noise bank')
        f.set_rirs([])
        refused(lambda: f.augment_audio([x, x], None, wave(2, rir=[-1, 0])), 'utterance 1 asks for RIR 0, the featurizer has no RIR bank')
        assert same(f.augment_audio([x], None, wave(1, rir=[-1], noise=[-1]))[0], x)   # nothing asked for: no bank needed
    finally:
        e.close()
        f.close()


def test_bad_waves_are_refused_and_leave_the_resident_batch(fz):
    from neuralasr_amd import _lib
    audios, rates, w, labels, ll = route_batch()
    e = lstm(fz.width)
    try:
        seq, T = e.upload_batch_audio(fz, audios, labels, ll, rates, wave=pick(w, range(5)))
        resident = e.forward_resident(5, T)

        def bad(**kw):
            v = {k: list(x) for k, x in w.items()}
            for k, (i, x) in kw.items():
                v[k][i] = x
            return pick(v, range(5))
        cases = [(bad(rir=(2, len(RIRS))), 'utterance 2: RIR index %d is outside the bank' % len(RIRS)),
                 (bad(rir=(0, -2)), 'utterance 0: RIR index -2 is outside the bank'),
                 (bad(noise=(1, len(CLIPS))), 'utterance 1: noise index %d is outside the bank' % len(CLIPS)),
                 (bad(noise=(4, -7)), 'utterance 4: noise index -7 is outside the bank'),
                 (bad(off=(1, 37)), "utterance 1: noise_off 37 is outside clip 0's [0,36]"),
                 (bad(off=(2, -1)), 'utterance 2: noise_off -1 is outside clip 2'),
                 (bad(snr=(4, np.nan)), 'utterance 4: snr_db is not finite'),
                 (bad(snr=(1, np.inf)), 'utterance 1: snr_db is not finite')]
        for wv, text in cases:
            for call in (lambda: e.upload_batch_audio(fz, audios, labels, ll, rates, wave=wv),
                         lambda: e.stage_batch_audio(fz, audios, labels, ll, rates, wave=wv),
                         lambda: fz.augment_audio(audios, rates, wv)):
                with pytest.raises(_lib.NasrError) as err:
                    call()
                assert err.value.code == _lib.NASR_ERR_ARG and text in str(err.value), str(err.value)
            assert same(e.forward_resident(5, T), resident), text
        # values that are not read are not checked: the offset and the SNR of an utterance without noise
        fine = bad(off=(0, 10 ** 9), snr=(3, np.nan))
        e.upload_batch_audio(fz, audios, labels, ll, rates, wave=fine)
        assert same(e.forward_resident(5, T), resident)
        # refused staged batches gave their slots back
        t1 = e.stage_batch_audio(fz, audios, labels, ll, rates, wave=pick(w, range(5)))[2]
        t2 = e.stage_batch_audio(fz, audios, labels, ll, rates)[2]
        assert t1 is not None and t2 is not None
        e.discard_batch(t1)
        e.discard_batch(t2)
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------- the loop
def wave_keys(d):
    noise_list, rir_list = write_banks(os.path.join(str(d), 'banks'), noise_rate=16000)      # the noise is resampled to 8 kHz
    return 'noise_list=%s\nnoise_prob=0.8\nnoise_snr=0,20\nrir_list=%s\nrir_prob=0.7\naugment_seed=7\n' % (noise_list, rir_list)


@pytest.fixture(scope='module')
def wave_run(tmp_path_factory):
    d = tmp_path_factory.mktemp('wave_loop')
    ckpt, step, kernels = run_loop(loop_config(d, keys=wave_keys(d)))
    assert step == 3 and int(ckpt['step']) == 3
    return ckpt, kernels


def test_loop_is_repeatable_and_differs_from_the_plain_loop(wave_run, tmp_path):
    want, kernels = wave_run
    (tmp_path / 'again').mkdir()
    (tmp_path / 'plain').mkdir()
    again, step, k2 = run_loop(loop_config(tmp_path / 'again', keys=wave_keys(tmp_path / 'again')))
    assert step == 3 and same_checkpoint(again, want), 'two augmented runs differ (recurrence %r and %r)' % (kernels, k2)
    plain, step, _ = run_loop(loop_config(tmp_path / 'plain', keys=''))
    assert step == 3 and not same(plain['params'], want['params'])


def test_resumed_loop_ends_with_the_bits_of_the_uninterrupted_one(wave_run, tmp_path):
    want, kernels = wave_run
    keys = wave_keys(tmp_path)
    two, step, _ = run_loop(loop_config(tmp_path, keys=keys, epochs=2))
    assert step == 2 and not same(two['params'], want['params'])
    resumed, step, k2 = run_loop(loop_config(tmp_path, keys=keys, epochs=1, start_step=2))
    assert step == 3 and int(resumed['step']) == 3
    assert same_checkpoint(resumed, want), 'the resumed run differs (recurrence %r and %r)' % (kernels, k2)
