"""GPU: the padding of the parameter-shaped buffers stays exactly 0.

Every model runs on padded buffers (Hp = round_up(H, 64), Fp / Cp to 32, dense widths to 64); the Adam sweep covers the
padding, the getters and setters do not see it.  The model is the H-unit network only while the padding of P is 0, and
nothing but the kernels' contract (kernels.h, "units") keeps it there.  These tests look at the padding itself, through
the device alias of the gradient buffer: no tolerance anywhere, every assertion is == 0, equality of bits, or != in the
control."""
import numpy as np
import pytest

from oracle import nasr_oracle as O

pytestmark = pytest.mark.gpu

HEAD = 32   # floats in front of the gradients in the alias, the step's fault word at [0] (include/nasr.h, nasr_grad_device_count)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def read_alias(e):
    """the whole device gradient buffer [head | np_int gradients], as the handle's stream has left it"""
    e.synchronize()
    return e.grad_tensor().cpu().numpy()


def layout(e):
    """(pad, pos) of a handle from what nasr_set_grads does - it scatters a TF-order array into the internal layout and
    zero-fills the rest: pad = boolean mask over the alias of the floats that are padding (a float is real iff it lies past
    the head and reads 1.0 after set_grads(ones)); pos[i] = where TF-order element i lies in the alias (the same probe with
    every element's own index + 1 as its bit pattern)."""
    n = e.param_count
    e.set_grads(np.ones(n, np.float32))
    buf = read_alias(e)
    assert buf.size == e.grad_device_ptr()[1]
    real = np.zeros(buf.size, bool)
    real[HEAD:] = buf[HEAD:] == 1.0
    pad = ~real
    pad[:HEAD] = False
    assert int(real.sum()) == n
    assert int(pad.sum()) > 0, 'no padding in this model: the case would be vacuous'
    assert not bits(buf)[pad].any()                      # the zero-fill: +0
    e.set_grads(np.arange(1, n + 1, dtype=np.uint32).view(np.float32))
    tags = bits(read_alias(e))
    assert np.array_equal(tags[HEAD:] != 0, real[HEAD:])
    at = np.flatnonzero(real)
    pos = np.empty(n, np.int64)
    pos[tags[at].astype(np.int64) - 1] = at
    return pad, pos


def assert_padding_zero(e, pad, pos, what):
    """after compute_grads: every padding float of the gradient buffer is 0, the fault word too, and the real floats are
    get_grads() bit for bit (which checks the mask and the map)"""
    e.synchronize()
    assert not e.step_void()
    buf = read_alias(e)
    assert buf[0] == 0.0
    bad = np.flatnonzero(pad & (buf != 0.0))
    print(what, 'padding floats', int(pad.sum()), 'non-zero', bad.size, 'largest',
          float(np.abs(buf[bad]).max()) if bad.size else 0.0, 'first at', int(bad[0]) - HEAD if bad.size else None)
    assert bad.size == 0, (what, bad.size, float(np.abs(buf[bad]).max()), int(bad[0]) - HEAD)
    assert np.array_equal(bits(buf[pos]), bits(e.get_grads())), what


def make_engine(spec, lr=1e-3):
    from neuralasr_amd.engine import Engine
    return Engine(spec.feature_size, spec.hidden, spec.num_layers, spec.bidirectional, spec.merge, spec.num_classes,
                  forget_bias=spec.forget_bias, learning_rate=lr, pre=spec.pre, post=spec.post, relu_clip=spec.relu_clip,
                  dropout=spec.dropout)


def rand_params(spec, seed):
    rs = np.random.RandomState(seed)
    return O.flatten([p + 0.05 * rs.randn(*p.shape) for p in O.init_params(spec, seed=seed)]).astype(np.float32)


def ragged_batch(spec, B, T, seed):
    """seq_len mixed (one utterance a third of T: many masked steps), one label empty"""
    feats, seq_len, labels, label_len = O.synth_batch(spec, B, T, seed=seed, var_len=True, Lmin=1, Lmax=max(1, T // 5))
    seq_len[0] = max(int(label_len[0]) * 2 + 1, T // 3)
    feats[0, seq_len[0]:] = 0.0
    label_len[1] = 0
    labels[1, :] = 0
    return feats, seq_len, labels, label_len


SPEC_A = O.ModelSpec(13, 70, 2, True, 'concat', 29)

# name: (spec, B, T, recurrence modes, chunking)
LSTM_CASES = {
    'a': (SPEC_A, 17, 40, ('persistent', 'per-step'), None),                                 # Hp 128, Bp 32: two rounds
    'b': (O.ModelSpec(13, 50, 1, False, 'none', 29), 5, 33, ('persistent', 'per-step'), None),   # Hp 64, odd T
    # Hp 512 from 460.  Two rounds of 8 groups x 4 utterances need Bp 48, i.e. B in 33..48 (Bp = round_up(B, 16)): c2 is
    # that shape, the one tests/test_gpu_persist.py runs (B 40, T 18); c is the same model at B 18 (Bp 32, one round), T 40
    'c': (O.ModelSpec(12, 460, 1, False, 'none', 7), 18, 40, ('persistent', 'per-step'), None),
    'c2': (O.ModelSpec(12, 460, 1, False, 'none', 7), 40, 18, ('persistent', 'per-step'), None),
    # the dense stages' padded widths (40 -> 64, 24 -> 64).  The library takes dense stages around a bidirectional stack
    # only with merge = concat; the other bidirectional merge (stack_reshape, the directions' outputs through one
    # projection) is d2, without dense stages
    'd': (O.ModelSpec(13, 70, 1, True, 'concat', 33, pre=(40,), post=24, relu_clip=20.0), 6, 21, ('persistent', 'per-step'), None),
    'd2': (O.ModelSpec(13, 70, 1, True, 'stack_reshape', 33), 6, 21, ('persistent', 'per-step'), None),
    # a window shorter than T: the carry form of the step BPTT.  Chunked passes run on the per-step kernels, and the
    # library chunks bidirectional concat networks only (a look-ahead of at least one frame)
    'e': (O.ModelSpec(13, 70, 2, True, 'concat', 29), 5, 40, ('per-step',), (8, 5)),
}
LSTM_PARAMS = [(name, mode) for name, c in LSTM_CASES.items() for mode in c[3]]


def lstm_handle(name, mode, graph):
    spec, B, T, _, chunk = LSTM_CASES[name]
    e = make_engine(spec)
    e.set_params(rand_params(spec, 5))
    pad, pos = layout(e)
    if mode == 'persistent':
        assert e.recurrence_mode == 'persistent', 'MI355X (8 XCDs x 32 CUs) must pass the census at create time'
    else:
        e.set_recurrence_mode(False)
        assert e.recurrence_mode == 'per-step'
    e.set_graph_mode(graph)
    if chunk:
        e.set_chunking(*chunk)
        assert chunk[0] + chunk[1] < T
    return e, pad, pos, ragged_batch(spec, B, T, seed=7 * B + T)


@pytest.mark.parametrize('name,mode', LSTM_PARAMS, ids=['%s-%s' % p for p in LSTM_PARAMS])
def test_gradient_padding_is_zero_after_compute_grads(name, mode):
    """Before the persistent BPTT stored +0 in dG of the padded units, every persistent case here failed, at exactly the
    padded j-gate bias columns (one float per padded unit, direction and layer; the weight gradients' fp16 planes flushed
    theirs): a 232 floats, the largest 9.88e-42 = 7051 units of 2^-149; b 14, 2.25e-42; c 52, 9.70e-42; c2 52, 8.45e-42;
    d and d2 116, 1.38e-42.  The per-step cases, the chunked one, LAS and WaveNet were 0 then as now."""
    e, pad, pos, batch = lstm_handle(name, mode, graph=False)
    e.upload_batch(*batch)
    e.compute_grads()
    assert_padding_zero(e, pad, pos, '%s-%s' % (name, mode))
    if mode == 'persistent':
        assert e.recurrence_mode == 'persistent'        # it did not pass by falling back to the per-step kernels
        assert e.persist_stats()[0] == 0
    e.close()


def test_gradient_padding_is_zero_under_replayed_graphs():
    """case a on the per-step kernels with graph mode on: the first step captures the layers' step graphs, the second
    replays them"""
    e, pad, pos, batch = lstm_handle('a', 'per-step', graph=True)
    for step in range(2):
        e.upload_batch(*batch)
        e.compute_grads()
        e.synchronize()
    assert_padding_zero(e, pad, pos, 'a-per-step-graph')
    assert e.recurrence_mode == 'per-step'
    e.close()


def test_gradient_padding_is_zero_las():
    """The LAS handle (250 units in 256, F 8 in 32, C 12 in 32; the pair layout of the pyramid's inputs and the memory
    columns have padding of their own).  Its np_int region holds parameters and their padding only."""
    from tests import las_ref
    from neuralasr_amd.engine import LasEngine
    F, C, B, T, U = 8, 12, 5, 17, 6
    e = LasEngine(F, C, sampling_probability=0.0, seed=5, learning_rate=1e-3)
    e.set_params(las_ref.initial_params(F, C, seed=3))
    pad, pos = layout(e)
    feats, seq, labels, ll = las_ref.make_batch(B, T, F, U, C, np.random.RandomState(11), empty=True)
    e.upload_batch(feats, seq, labels, ll)
    e.compute_grads()
    assert_padding_zero(e, pad, pos, 'las')
    e.close()


def test_gradient_padding_is_zero_wavenet():
    """The WaveNet handle (F 11 in 32 rows of conv_in, C 7 in 32 columns of conv_2).  Its np_int region holds parameters
    and their padding only: the batch-norm moving statistics live apart."""
    import wavenet_ref as W
    from neuralasr_amd.engine import WaveNetEngine
    spec = W.Spec(11, 7, num_blocks=1, rates=(1, 2))
    B, T = 5, 19
    e = WaveNetEngine(spec.F, spec.C, num_blocks=spec.nb, rates=spec.rates, learning_rate=1e-3)
    e.set_params(W.init_params(spec, 9))
    pad, pos = layout(e)
    seq = np.array([T, 7, 12, 19, 10], np.int32)
    feats, seq, labels, ll = W.synth_batch(spec, B, T, seed=3, seq_len=seq, label_len=[3, 0, 2, 4, 1])
    e.upload_batch(feats, seq, labels, ll)
    e.compute_grads()
    assert_padding_zero(e, pad, pos, 'wavenet')
    e.close()


# ------------------------------------------------------------------------------------------------ the trajectory
def _same_bits(a, b, what):
    assert np.array_equal(bits(a), bits(b)), what


def _round_trip(e, ema):
    """what a checkpoint keeps, read and written back: re-scattering zero-fills the padding of P, M, V (and E)"""
    e.set_params(e.get_params())
    m, v, t = e.get_adam_state()
    e.set_adam_state(m, v, t)
    if ema:
        e.set_ema_state(e.get_ema(), e.ema()[1])


def _loss_bits(e, batch):
    loss, nll = e.loss(*batch)
    return np.concatenate([bits(np.float32(loss)).ravel(), bits(nll)])


@pytest.mark.parametrize('mode,ema', [('persistent', 0.0), ('per-step', 0.0), ('persistent', 0.99)],
                         ids=['persistent', 'per-step', 'persistent-ema'])
def test_trajectory_does_not_depend_on_the_padding(mode, ema):
    """30 steps at learning_rate 1e-2 on spec a, T 128, B 32.  Then (1) the loss of the batch is the same bits before and
    after the handle's own state went through the getters and setters, which holds iff the padding of P was 0; (2) three
    more steps on that handle and on a twin that ran the same 30 steps without the round trip give the same parameters,
    moments, average and losses bit for bit, which covers the padding of M, V and E.

    Control, so that the detector is not blind: gradients of 1e-3 written into the padding of the gradient alias behind
    compute_grads (the real floats stay the step's), five times, each followed by apply_adam(1.0) - a plain sweep, it moves
    the padding of P by about learning_rate per step.  The loss before and after the round trip must then differ.
    Measured on MI355X, two runs: 52.4005 against 51.3775 after the round trip (difference 1.023) and 52.4168 against 51.3767
    (1.040) in persistent mode, with and without averaging; 55.607 against 53.671 (1.936) and 76.035 against 54.576 (21.46)
    on the per-step kernels.  (With live padding the handle is outside the kernels' contract, and the control's figures
    differed between the two runs - presumably padded units then read what the contract lets a buffer hold; everything
    before the control is the same bits on both handles.)"""
    import torch
    spec, B, T = SPEC_A, 32, 128
    batch = ragged_batch(spec, B, T, seed=3)
    p0 = rand_params(spec, 5)
    handles = []
    for twin in range(2):
        e = make_engine(spec, lr=1e-2)
        e.set_recurrence_mode(mode == 'persistent')
        assert e.recurrence_mode == mode
        e.set_params(p0)
        if ema:
            e.set_ema(ema)
        handles.append(e)
    a, b = handles
    pad, _ = layout(a)                                   # (planted gradients are not applied: the next step computes its own)
    for e in handles:
        for _ in range(30):
            e.train_step(*batch)
        assert not e.step_void()
    before = _loss_bits(a, batch)
    _round_trip(a, ema)
    after = _loss_bits(a, batch)
    _same_bits(before, after, 'the loss changed when the state was read and written back: the padding of P was not 0')
    losses = [[e.train_step(*batch) for _ in range(3)] for e in handles]
    _same_bits(losses[0], losses[1], 'losses of the three steps after the round trip')
    _same_bits(a.get_params(), b.get_params(), 'P')
    (ma, va, ta), (mb, vb, tb) = a.get_adam_state(), b.get_adam_state()
    assert ta == tb == 33
    _same_bits(ma, mb, 'M')
    _same_bits(va, vb, 'V')
    if ema:
        assert a.ema() == b.ema()
        _same_bits(a.get_ema(), b.get_ema(), 'E')
    for e in handles:
        assert not e.step_void() and e.recurrence_mode == mode
        if mode == 'persistent':
            assert e.persist_stats()[0] == 0
    b.close()

    # the control
    where = torch.from_numpy(np.flatnonzero(pad)).cuda()
    gt = a.grad_tensor()
    for _ in range(5):
        a.upload_batch(*batch)
        a.compute_grads()
        a.synchronize()
        gt[where] = 1e-3
        torch.cuda.synchronize()
        a.apply_adam(1.0)
    assert not a.step_void()
    before = _loss_bits(a, batch)
    _round_trip(a, ema)
    after = _loss_bits(a, batch)
    lb, la = float(before[:1].view(np.float32)[0]), float(after[:1].view(np.float32)[0])
    print('control %s ema %g: loss with live padding %.9g, after the round trip %.9g, difference %.9g' % (mode, ema, lb, la, lb - la))
    assert before[0] != after[0], 'the detector is blind at this shape'
    a.close()
