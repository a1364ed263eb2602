"""GPU: SpecAugment masks and speed perturbation.  The masked context expansion
(expand_context_masked_kernel behind nasr_upload_batch_context_aug / nasr_upload_batch_audio_aug /
nasr_stage_batch_audio_aug) against NumPy on the host: the centre frames with the masked frames and columns set to 0,
restacked with the utterance's pad value and uploaded whole with the plain nasr_upload_batch.  Everything is compared as
bits, on one handle wherever the LSTM recurrence is in the path (tests/test_gpu_audio_batch.py says why)."""
import os

import numpy as np
import pytest

from test_augment_host import SR, cfg_ns, make_corpus
from test_gpu_audio_batch import C, assert_same, init, lstm, observe, same, state
from test_gpu_feat import RAGGED_FRAMES, ragged

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------- the host reference
def restack(centre, pad, ctx):
    """include_context (utils.py:8-21) of centre [L, ncep] with `pad` where the window leaves the utterance"""
    L, n = centre.shape
    out = np.full((L, 2 * ctx + 1, n), pad, np.float32)
    for w in range(2 * ctx + 1):
        ts = np.arange(L) + w - ctx
        ok = (ts >= 0) & (ts < L)
        out[ok, w] = centre[ts[ok]]
    return out.reshape(L, -1)


def host_masked(feats, seq, ctx, ncep, sw, tm, fm):
    """the stacked array [B, T, (2 ctx + 1) ncep] whose centre columns went through the masks"""
    out = np.zeros_like(feats)
    for b, L in enumerate(int(x) for x in seq):
        centre = feats[b, :L, ctx * ncep:(ctx + 1) * ncep].copy()
        for t0, tw in ([] if tm is None else tm[b]):
            centre[t0:t0 + tw] = 0.0
        for f0, fw in ([] if fm is None else fm[b]):
            for blk in range(ncep // sw):
                centre[:, blk * sw + f0:blk * sw + f0 + fw] = 0.0
        out[b, :L] = restack(centre, feats[b, 0, 0], ctx)
    return out


def stacked_batch(seq, ctx, ncep, seed):
    """normalised, context-stacked features of random centre frames, as preprocess_mfcc makes them (utils.py:24-31)"""
    rs = np.random.RandomState(seed)
    feats = np.zeros((len(seq), max(seq), (2 * ctx + 1) * ncep), np.float32)
    for b, L in enumerate(seq):
        st = restack(rs.randn(L, ncep).astype(np.float32), 0.0, ctx)
        feats[b, :L] = ((st - st.mean()) / st.std()).astype(np.float32)
    return feats


SEQ = (23, 9, 1)
# per utterance, 8 time masks of (first frame, width) and 3 frequency masks of (first static column, width); static_width 13
MASKS = {
    # utterance 0: at t0 = 0, ending at len, width 0, two overlapping, all 8 in use; utterance 1: one mask over the whole
    # utterance; utterance 2 (one frame): none with a width, one starting at len.  Frequency: at column 0, ending at
    # static_width, width 0; a narrow one; the full width.
    'A': ([[(0, 2), (20, 3), (11, 0), (5, 4), (7, 4), (15, 1), (23, 0), (17, 2)],
           [(0, 9)] + [(0, 0)] * 7,
           [(1, 0)] + [(0, 0)] * 7],
          [[(0, 3), (10, 3), (5, 0)], [(4, 2), (0, 0), (13, 0)], [(0, 13), (0, 0), (0, 0)]]),
    # utterance 0: its last frame only, every column masked; utterance 1: first frame, last frame, overlapping and nested
    # masks; utterance 2: its one frame masked.
    'B': ([[(22, 1)] + [(0, 0)] * 7,
           [(0, 1), (8, 1), (3, 3), (4, 4), (4, 1), (2, 0), (9, 0), (0, 0)],
           [(0, 1)] + [(0, 0)] * 7],
          [[(0, 13), (0, 0), (0, 0)], [(12, 1), (0, 1), (6, 0)], [(0, 1), (1, 12), (0, 0)]]),
}


@pytest.mark.parametrize('ctx', [0, 2, 10])
@pytest.mark.parametrize('ncep,sw', [(13, 13), (39, 13)])
def test_masked_expansion_is_bitwise_the_host_masking(ncep, sw, ctx):
    """1-layer BiLSTM, H 24, C 7, B 3 (13 empty columns of Bp 16), T 23, lengths 23 / 9 / 1; ctx 10 is wider than the short
    utterances.  Logits, loss, gradients and the parameters after one Adam step: the rows past seq_len and the padded
    feature columns F..Fp are inputs of the same GEMMs, so the equality covers them."""
    from neuralasr_amd.engine import BatchAug, Engine
    B, T, F = len(SEQ), max(SEQ), (2 * ctx + 1) * ncep
    feats = stacked_batch(SEQ, ctx, ncep, seed=ncep + ctx)
    for b, L in enumerate(SEQ):             # the reference's restacking is the identity without masks
        assert same(restack(feats[b, :L, ctx * ncep:(ctx + 1) * ncep], feats[b, 0, 0], ctx), feats[b, :L])
    labels = np.array([[1, 2, 3], [4, 5, 0], [2, 0, 0]], np.int32)
    label_len = [3, 2, 1]
    e = init(Engine(F, 24, 1, True, 'stack_reshape', 7, learning_rate=1e-3))
    before = state(e)
    try:
        for name, (tm, fm) in MASKS.items():
            tm, fm = np.asarray(tm, np.int32), np.asarray(fm, np.int32)
            assert tm.shape == (B, 8, 2) and fm.shape == (B, 3, 2)
            want_feats = host_masked(feats, SEQ, ctx, ncep, sw, tm, fm)
            assert not same(want_feats, feats)
            init(e)
            e.upload_batch(want_feats, SEQ, labels, label_len)
            want = observe(e, B, T)
            init(e)
            assert e.upload_batch_context(feats, SEQ, labels, label_len, ctx, ncep, aug=BatchAug(sw, tm, fm)) is True
            got = observe(e, B, T)
            assert_same(got, want, 'mask set %s (recurrence %r at create, %r now)' % (name, before, state(e)))
            assert np.all(np.isfinite(got['logits'])) and np.isfinite(got['loss'])
    finally:
        e.close()


def test_no_mask_is_the_plain_call():
    """aug=None, and masks that all have width 0, give the bits of the plain upload_batch_context"""
    from neuralasr_amd.engine import BatchAug, Engine
    ctx, ncep = 2, 13
    feats = stacked_batch(SEQ, ctx, ncep, seed=1)
    labels, label_len = np.array([[1, 2], [3, 0], [4, 0]], np.int32), [2, 1, 1]
    e = init(Engine(feats.shape[2], 24, 1, True, 'stack_reshape', 7, learning_rate=1e-3))
    try:
        assert e.upload_batch_context(feats, SEQ, labels, label_len, ctx, ncep)
        want = observe(e, 3, 23)
        zero_t = np.zeros((3, 8, 2), np.int32)
        zero_t[:, :, 0] = [[0, 1, 2, 3, 4, 5, 6, 23], [0, 9, 1, 2, 3, 4, 5, 6], [0, 1, 0, 1, 0, 1, 0, 1]]     # starts without widths
        zero_f = np.zeros((3, 2, 2), np.int32)
        zero_f[:, :, 0] = 13
        for aug in (None, BatchAug(13, zero_t, zero_f), BatchAug(13, None, None), BatchAug(13, zero_t, None)):
            init(e)
            assert e.upload_batch_context(feats, SEQ, labels, label_len, ctx, ncep, aug=aug)
            assert_same(observe(e, 3, 23), want, repr(aug))
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------- the audio route
def audio_case(kind):
    from neuralasr_amd.features import Featurizer
    if kind == 'logfbank':
        return Featurizer(SR, 40, 2, kind='logfbank', deltas=2)
    return Featurizer(SR, 13, 2)


def ragged_masks(f, seq):
    """three time and two frequency masks per utterance from the product's own policy, and the edges by hand"""
    from neuralasr_amd.augment import Augmenter
    a = Augmenter(cfg_ns(numcep=f.numcep, spec_time_masks=3, spec_time_width=30, spec_freq_masks=2, spec_freq_width=8))
    tm, fm = a.masks(5, seq)
    tm[2, 0] = (0, 4)                        # the 104-frame utterance: at its first frame and at its last
    tm[2, 1] = (100, 4)
    tm[1, 0] = (0, 1)                        # the one-frame utterance: its frame
    fm[0, 0] = (0, 2)
    fm[0, 1] = (f.numcep - 3, 3)
    assert tm[:, :, 1].any() and fm[:, :, 1].any()
    return tm, fm


def ragged_labels(seq, dense):
    rs = np.random.RandomState(2)
    if dense:
        return rs.randint(0, C, size=(len(seq), 4)).astype(np.int32), [int(rs.randint(1, 5)) for _ in seq]
    label_len = [min(2, t) for t in seq]
    labels = np.zeros((len(seq), 2), np.int32)
    for b, n in enumerate(label_len):
        labels[b, :n] = (1 + b % 5, 7)[:n]
    return labels, label_len


def host_route(e, f, audios, labels, label_len, tm, fm):
    """Featurizer.compute, host masking, zero-padding, plain upload"""
    got = f.compute(audios)
    seq = [x.shape[0] for x in got]
    feats = np.zeros((len(got), max(seq), f.width), np.float32)
    for b, x in enumerate(got):
        feats[b, :seq[b]] = x
    e.upload_batch(host_masked(feats, seq, f.numcontext, f.frame_width, f.numcep, tm, fm), seq, labels, label_len)
    return seq, max(seq)


@pytest.mark.parametrize('kind', ['logfbank', 'mfcc'])
def test_audio_route_is_bitwise_the_host_masking(kind):
    """the ragged 8 kHz batch of tests/test_gpu_feat.py (1 to 104 frames), features=logfbank numcep=40 deltas=2
    numcontext=2 (frames of 120 columns in three blocks of 40) and the MFCC default; synchronous and staged"""
    from neuralasr_amd.engine import BatchAug
    f = audio_case(kind)
    audios, seq = list(ragged()), list(RAGGED_FRAMES)
    B, T = len(seq), max(seq)
    tm, fm = ragged_masks(f, seq)
    labels, label_len = ragged_labels(seq, False)
    e = lstm(f.width)
    before = state(e)
    try:
        assert host_route(e, f, audios, labels, label_len, tm, fm) == (seq, T)
        want = observe(e, B, T)
        init(e)
        aug = BatchAug(f.numcep, tm, fm)
        got_seq, got_T = e.upload_batch_audio(f, audios, labels, label_len, None, aug=aug)
        assert [int(t) for t in got_seq] == seq and got_T == T
        got = observe(e, B, T)
        note = '(recurrence %r at create, %r now)' % (before, state(e))
        assert_same(got, want, 'synchronous ' + note)
        # the same without masks differs: the comparison above is not vacuous
        init(e)
        e.upload_batch_audio(f, audios, labels, label_len, None)
        assert not same(e.forward_resident(B, T), want['logits'])
        # staged, then committed
        init(e)
        s_seq, s_T, ticket = e.stage_batch_audio(f, audios, labels, label_len, None, aug=aug)
        assert ticket is not None and [int(t) for t in s_seq] == seq and s_T == T
        e.commit_batch(ticket)
        assert_same(observe(e, B, T), want, 'staged ' + note)
    finally:
        e.close()
        f.close()


@pytest.mark.parametrize('family', ['wavenet', 'las'])
def test_audio_route_on_the_other_handles(family):
    from neuralasr_amd.engine import BatchAug, LasEngine, WaveNetEngine
    f = audio_case('logfbank')
    audios, seq = list(ragged()), list(RAGGED_FRAMES)
    B, T = len(seq), max(seq)
    tm, fm = ragged_masks(f, seq)
    labels, label_len = ragged_labels(seq, family == 'las')

    def make():                              # two handles: batch-norm and sampling state change with a step
        if family == 'wavenet':
            return init(WaveNetEngine(f.width, C, num_blocks=1, rates=(1, 2), learning_rate=1e-3), seed=4)
        return init(LasEngine(f.width, C, sampling_probability=0.1, seed=5, learning_rate=1e-3), seed=6)
    a, b = make(), make()
    try:
        host_route(a, f, audios, labels, label_len, tm, fm)
        b.upload_batch_audio(f, audios, labels, label_len, None, aug=BatchAug(f.numcep, tm, fm))
        assert_same(observe(b, B, T, ctc=family != 'las'), observe(a, B, T, ctc=family != 'las'))
    finally:
        a.close()
        b.close()
        f.close()


# ---------------------------------------------------------------------------------------------- errors
def test_bad_masks_are_refused_and_leave_the_handle_as_it_was():
    from neuralasr_amd import _lib
    from neuralasr_amd.engine import BatchAug, Engine
    from neuralasr_amd.features import Featurizer
    ctx, ncep = 2, 13
    feats = stacked_batch(SEQ, ctx, ncep, seed=1)
    labels, label_len = np.array([[1, 2], [3, 0], [4, 0]], np.int32), [2, 1, 1]

    def make():
        return init(Engine(feats.shape[2], 24, 1, True, 'stack_reshape', 7, learning_rate=1e-3))
    e, fresh = make(), make()
    f = Featurizer(SR, 13, 2, deltas=2)                    # frames of 39 columns
    fe = lstm(f.width)
    audios = [ragged()[k] for k in (4, 2, 1)]             # 9, 104 and 1 frames
    try:
        good = BatchAug(13, np.array([[(3, 4)], [(0, 2)], [(0, 1)]], np.int32), np.array([[(2, 3)]] * 3, np.int32))
        assert e.upload_batch_context(feats, SEQ, labels, label_len, ctx, ncep, aug=good)
        resident = e.forward_resident(3, 23)

        def refused(text, aug, **kw):
            with pytest.raises(_lib.NasrError) as err:
                if kw:
                    fe.upload_batch_audio(f, audios, labels, label_len, None, aug=aug)
                else:
                    e.upload_batch_context(feats, SEQ, labels, label_len, ctx, ncep, aug=aug)
            assert err.value.code == _lib.NASR_ERR_ARG and text in str(err.value), str(err.value)

        def tmask(b, k, t0, tw, n=2):
            m = np.zeros((3, n, 2), np.int32)
            m[b, k] = (t0, tw)
            return m
        refused('time mask 1 of utterance 1', BatchAug(13, tmask(1, 1, 8, 2), None))        # one frame past seq_len = 9
        refused('time mask 0 of utterance 2', BatchAug(13, tmask(2, 0, 1, 1), None))
        refused('time mask 0 of utterance 0', BatchAug(13, tmask(0, 0, -1, 1), None))       # a negative start
        refused('time mask 1 of utterance 0', BatchAug(13, tmask(0, 1, 3, -1), None))
        refused('frequency mask 1 of utterance 2', BatchAug(13, None, tmask(2, 1, 12, 2)))
        refused('frequency mask 0 of utterance 0', BatchAug(13, None, tmask(0, 0, -2, 1)))
        refused('n_time = 9', BatchAug(13, tmask(0, 0, 0, 1, n=9), None))
        refused('n_freq = 9', BatchAug(13, None, tmask(0, 0, 0, 1, n=9)))
        refused('static_width 5 does not divide', BatchAug(5, tmask(0, 0, 0, 1), None))
        refused('static_width 0 does not divide', BatchAug(0, tmask(0, 0, 0, 1), None))
        # the resident batch is still the one from before the refusals
        assert same(e.forward_resident(3, 23), resident)
        # audio: the masks are checked against the seq_len the call computes, static_width against the featurizer's numcep
        refused("static_width 39 is not the featurizer's numcep 13", BatchAug(39, tmask(0, 0, 0, 1), None), audio=True)
        refused('time mask 0 of utterance 2', BatchAug(13, tmask(2, 0, 0, 2), None), audio=True)
        refused('time mask 1 of utterance 0', BatchAug(13, tmask(0, 1, 9, 1), None), audio=True)
        seq, T = fe.upload_batch_audio(f, audios, labels, label_len, None, aug=BatchAug(13, tmask(0, 1, 8, 1), None))
        assert [int(t) for t in seq] == [9, 104, 1] and np.all(np.isfinite(fe.forward_resident(3, T)))
        # a refused staged batch gives its slot back: two more can be staged
        with pytest.raises(_lib.NasrError):
            fe.stage_batch_audio(f, audios, labels, label_len, None, aug=BatchAug(13, tmask(2, 0, 0, 2), None))
        t1 = fe.stage_batch_audio(f, audios, labels, label_len, None)[2]
        t2 = fe.stage_batch_audio(f, audios, labels, label_len, None, aug=BatchAug(13, tmask(0, 1, 8, 1), None))[2]
        assert t1 is not None and t2 is not None
        fe.discard_batch(t1)
        fe.discard_batch(t2)
        # a step on the handle afterwards matches a fresh handle
        assert state(e) == state(fresh)
        init(e)
        for h in (e, fresh):
            assert h.upload_batch_context(feats, SEQ, labels, label_len, ctx, ncep, aug=good)
        assert_same(observe(e, 3, 23), observe(fresh, 3, 23), '(recurrence %r and %r)' % (state(e), state(fresh)))
    finally:
        for h in (e, fresh, fe, f):
            h.close()


# ---------------------------------------------------------------------------------------------- the loop
KEYS = ('spec_time_masks=2\nspec_time_width=6\nspec_time_ratio=0.5\nspec_freq_masks=2\nspec_freq_width=4\n'
        'speed_perturb=0.9,1.0,1.1\naugment_seed=7\n')
NET = 'networks.lstm_ctc_net.SmallLstmCTCNet'       # 1 x 128, no stack_reshape merge: two towers may take audio


def loop_config(d, keys=KEYS, epochs=3, start_step=0, num_gpus=1, batch_size=5):
    """make_corpus with one batch of the 5 training utterances per epoch: every step trains the same utterances"""
    cfg_path, out = make_corpus(d, batch_size=batch_size, extra=keys + 'sym_file=${MFCC Featurizer:output}/symbols\n')
    os.makedirs(out, exist_ok=True)
    text = cfg_path.read_text()
    for a, b in (('networks.bilstm_ctc_net.BiLstmCTCNet', NET), ('epochs=1\n', 'epochs=%d\n' % epochs),
                 ('start_step=0\n', 'start_step=%d\n' % start_step), ('num_gpus=1\n', 'num_gpus=%d\n' % num_gpus)):
        assert a in text
        text = text.replace(a, b)
    cfg_path.write_text(text)
    return cfg_path


def run_loop(cfg_path):
    """train --from-audio; (the last checkpoint's arrays, the step it was written at, the recurrence the handle ended with)"""
    from neuralasr_amd import train
    from neuralasr_amd.config import Config
    net = train.main([str(cfg_path), '--from-audio'])
    net._settle()
    kernels = state(net.engine)
    step = net.global_step
    net.engine.close()
    with np.load(os.path.join(Config(str(cfg_path), True).model_dir, 'model-%d.npz' % step)) as z:
        return {k: z[k].copy() for k in z.files}, step, kernels


def same_checkpoint(a, b):
    return sorted(a) == sorted(b) and all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a)


@pytest.fixture(scope='module')
def augmented_run(tmp_path_factory):
    """three augmented steps, run once for the tests below: (checkpoint of step 3, recurrence)"""
    ckpt, step, kernels = run_loop(loop_config(tmp_path_factory.mktemp('aug_loop')))
    assert step == 3 and int(ckpt['step']) == 3
    return ckpt, kernels


def test_loop_is_repeatable_and_differs_from_the_plain_loop(augmented_run, tmp_path):
    want, kernels = augmented_run
    (tmp_path / 'again').mkdir()
    (tmp_path / 'plain').mkdir()
    again, step, k2 = run_loop(loop_config(tmp_path / 'again'))
    assert step == 3 and int(again['step']) == 3
    assert same_checkpoint(again, want), 'two augmented runs differ (recurrence %r and %r)' % (kernels, k2)
    plain, step, _ = run_loop(loop_config(tmp_path / 'plain', keys=''))
    assert step == 3 and not same(plain['params'], want['params'])


def test_resumed_loop_ends_with_the_bits_of_the_uninterrupted_one(augmented_run, tmp_path):
    want, kernels = augmented_run
    two, step, _ = run_loop(loop_config(tmp_path, epochs=2))
    assert step == 2 and int(two['step']) == 2 and not same(two['params'], want['params'])
    resumed, step, k2 = run_loop(loop_config(tmp_path, epochs=1, start_step=2))
    assert step == 3 and int(resumed['step']) == 3
    assert same_checkpoint(resumed, want), 'the resumed run differs (recurrence %r and %r)' % (kernels, k2)


def loop_network(d, **kw):
    """(training network, its training feed as train --from-audio builds it, the config)"""
    from neuralasr_amd import train
    from neuralasr_amd.config import Config
    cfg_path = loop_config(d, **kw)
    config = Config(str(cfg_path), True)
    feed, _ = train.audio_datasets(str(cfg_path), config)
    return config.load_network(fortraining=True), feed, config


def test_one_tower_and_two_towers_feed_the_same_masked_inputs(tmp_path):
    """The first training batch of 4 utterances as one tower, and as num_gpus=2 towers time-sliced in one process: the
    towers' uploads carry the global batch's masks sliced, and every utterance's logits are the same bits."""
    from neuralasr_amd.networks.hipnetwork import take_shard
    (tmp_path / 'one').mkdir()
    (tmp_path / 'two').mkdir()
    one, feed1, _ = loop_network(tmp_path / 'one', batch_size=4)
    two, feed2, cfg2 = loop_network(tmp_path / 'two', batch_size=2, num_gpus=2)
    try:
        assert cfg2.batch_size == 4 and two._towers() == (2, [0, 1]) and state(one.engine) == state(two.engine)
        b1, l1, s1, ll1 = feed1.get_next_batch()
        b2, l2, s2, ll2 = feed2.get_next_batch()
        assert b1.rates == b2.rates and same(b1.time_masks, b2.time_masks) and same(b1.freq_masks, b2.freq_masks)
        assert b1.time_masks[:, :, 1].any() and b1.freq_masks[:, :, 1].any() and set(b1.rates) - {SR, 16000}
        one._upload(b1, np.asarray(l1), list(s1), list(ll1))
        whole = one.engine.forward_resident(4, b1.shape[1])
        two.engine.set_params(one.engine.get_params())
        sent = []
        plain = two.engine.upload_batch_audio
        two.engine.upload_batch_audio = lambda *a: sent.append(a[5]) or plain(*a)
        for k in (0, 1):
            f, l, s, ll = take_shard(b2, l2, s2, ll2, 2, k)
            two._upload(f, l, s, ll)
            part = two.engine.forward_resident(2, f.shape[1])
            for i in range(2):
                n = int(s[i])
                assert n == int(s1[2 * k + i]) and same(part[:n, i], whole[:n, 2 * k + i]), 'utterance %d' % (2 * k + i)
        # and the step itself: the sliced towers upload those masks, validation uploads none
        loss, ler = two.train(b2, l2, s2, ll2)
        assert np.isfinite(loss) and len(sent) == 4
        for k, aug in enumerate(sent):
            assert aug.static_width == 13
            assert same(aug.time_masks, b1.time_masks[2 * (k % 2):2 * (k % 2) + 2])
            assert same(aug.freq_masks, b1.freq_masks[2 * (k % 2):2 * (k % 2) + 2])
        del sent[:]
        two.validate(b2, l2, s2, ll2)
        assert len(sent) >= 2 and all(a is None for a in sent)
    finally:
        one.engine.close()
        two.engine.close()


def test_speed_perturbation_is_the_upload_at_the_perturbed_rates(tmp_path):
    from neuralasr_amd.augment import KIND_SPEED
    net, feed, config = loop_network(tmp_path, keys='speed_perturb=0.9,1.1\n')
    try:
        b, labels, seq, ll = feed.get_next_batch()
        assert b.time_masks is None and b.freq_masks is None
        feed.dataset.reset_epoch()
        audios, native, _, _ = feed.dataset.get_next_batch()
        rates = [int(round(r * (0.9, 1.1)[feed.augmenter.raw(1, i, KIND_SPEED)[0] % 2])) for i, r in enumerate(native)]
        assert b.rates == rates and all(r != n for r, n in zip(rates, native))
        net._upload(b, np.asarray(labels), list(seq), list(ll))
        got = net.engine.forward_resident(len(b), b.shape[1])
        want_seq, T = net.engine.upload_batch_audio(net.featurizer(), audios, labels, ll, rates)
        assert [int(t) for t in want_seq] == [int(t) for t in seq] and T == b.shape[1]
        assert same(net.engine.forward_resident(len(b), T), got)
        plain_seq, _ = net.engine.upload_batch_audio(net.featurizer(), audios, labels, ll, native)
        assert [int(t) for t in plain_seq] != [int(t) for t in seq]
    finally:
        net.engine.close()
