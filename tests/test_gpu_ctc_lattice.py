"""GPU: every instantiation of the CTC lattice of csrc/ctc.hip, up to the 511-label limit, against the fp64 oracle
(tf.nn.ctc_loss, networks/tfnetwork.py:58-59), the reference computed inside each test.

The alpha / beta kernel is picked by two values.  KS, the lattice states per lane, is ceil((2 Lmax + 1) / 64) of the WIDTH
Lmax of the label array, not of the longest label (ensure_shape in nasr_batch.hip, wn_ensure_shape in nasr_wavenet.hip),
rounded up to an instantiation.  The engineered kernel (2b) runs where Cp == 32 and C <= 31 (ctc_fast_ok), the plain
log-domain kernel (2) everywhere else; ctc_grad_kernel reads the workspace of either with the same KS:

    Lmax (width)     KS   C = 29, 31   C = 32, 40
    31               2    fast         plain          (ceil(63 / 64) = 1: two states per lane at least)
    32, 63           2    fast         plain
    64, 95           3    fast         plain
    96, 127          4    fast         plain
    128, 159         5    fast         plain
    160, 191         6    fast         plain
    192, 223         7    fast         plain
    224, 255         8    fast         plain
    256, 383         12   fast         plain          (ceil(513 / 64) = 9 .. 12)
    384, 511         16   fast         plain          (13 .. 16)
    512              -    NasrError 'label length'

Every batch holds four utterances: a label that fills the width, one far below it (the padding columns decide KS), an empty
label and a pinned one (L + adjacent repeats = seq_len: every frame forced), ragged, T up to 1100 (17 turns of the 64-row
emission ring of (2b) and of the greedy collapse).  The padding of the label array holds class ids, not zeros.  The network
is small (H 16) so that the lattice dominates the gradient; the projection bias gradient b, the frame sum of the lattice's
logit gradient, is checked on its own.

Tolerances are those of test_gpu_edges.py and test_gpu_ctc_sweep.py (nll rtol 3e-5 atol 1e-5, loss 3e-5, the whole gradient
and b 1e-4; measured at most 2.4e-5, at Lmax 511, T 1100) except where the lattice's own fp32 arithmetic at length exceeds
them.  The values measured on an MI355X are next to each tolerance.  tools/ctc_fp32_model.py, recursion (2) in numpy fp32
with correctly rounded exp and log against the fp64 oracle on the same logits, gives errors of the same order at the same
cases (quoted below), and rescaling its columns every frame instead of every 4 does not lower them; both kernels, whose
arithmetic differs, land at about twice that model.  The logits themselves are not the cause: the engine's are within 3e-7
of the oracle's (1.5e-5 scaled by 60), and noise of 5e-6 on them moves b by 2e-7."""
import json

import numpy as np
import pytest

import test_gpu_wavenet as TW
import wavenet_ref as W
from oracle import nasr_oracle as O

pytestmark = pytest.mark.gpu

# the instantiations and the label-array widths at both edges of each
LMAX_BY_KS = {2: (31, 32, 63), 3: (64, 95), 4: (96, 127), 5: (128, 159), 6: (160, 191), 7: (192, 223), 8: (224, 255),
              12: (256, 383), 16: (384, 511)}
KERNEL_C = {'fast': 29, 'plain': 40}          # 29: the reference's character set
GTOL = 1e-4
# the projection scaled by 60, T 1000: whole gradient / b measured 1.5e-4 / 1.3e-4 (KS 8, fast; plain 1.2e-4 / 9.8e-5) and
# 5.6e-4 / 6.7e-4 (KS 16, fast; plain 4.4e-4 / 5.0e-4); the fp32 model gives b 7e-5 and 2.6e-4
GTOL_SHARP = {8: 5e-4, 16: 2e-3}
# WaveNet, Lmax 450, T 600: front/conv_in/W measured 8.3e-5 against TOL_GRAD 1e-5 (set on small shapes: T 60, 8 labels);
# the fp32 model of the lattice alone, the rest of the network in fp64, gives 3.2e-5 there
TOL_GRAD_WN_LONG = 2.5e-4


def ks_of(Lmax):
    """the instantiation the host picks for a label array of width Lmax (nasr_batch.hip: KSa)"""
    ks = max(1, (2 * Lmax + 1 + 63) // 64)
    return 2 if ks <= 1 else ks if ks <= 8 else 12 if ks <= 12 else 16


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def lattice_batch(C, Lmax, seed, T=None):
    """B 4 on a label array of width Lmax: [label well below the width, label = the width, empty label, pinned label]"""
    rs = np.random.RandomState(seed)
    T = T or min(1100, 2 * Lmax + 100)
    Ls, Lp = max(1, Lmax // 4), max(2, 2 * Lmax // 3)
    rep = Lp // 3
    seq_len = np.array([T - T // 5, T, T // 3 + 1, Lp + rep], np.int32)
    label_len = np.array([Ls, Lmax, 0, Lp], np.int32)
    labels = rs.randint(0, C - 1, size=(4, Lmax)).astype(np.int32)
    labels[3, :Lp] = O.pinned_label(rs, Lp, rep, C)
    assert O.ctc_feasible(labels[1], T) and not O.ctc_feasible(labels[3, :Lp], Lp + rep - 1)
    feats = rs.randn(4, T, 5).astype(np.float32)
    for b in range(4):
        feats[b, seq_len[b]:] = 0
    return feats, seq_len, labels, label_len


def net_params(spec, seed, scale=1.0):
    """the oracle's initialisation, moved off it, with the projection W, b scaled by `scale`, rounded through fp32"""
    rs = np.random.RandomState(seed)
    params = [p + 0.05 * rs.randn(*p.shape) for p in O.init_params(spec, seed=seed)]
    params[-2], params[-1] = params[-2] * scale, params[-1] * scale
    return [p.astype(np.float32).astype(np.float64) for p in params]


def engine_for(spec):
    from neuralasr_amd.engine import Engine
    return Engine(spec.feature_size, spec.hidden, spec.num_layers, spec.bidirectional, spec.merge, spec.num_classes,
                  learning_rate=1e-3)


def check_case(e, spec, params, batch, gtol, tag, logit_atol=2e-4):
    """loss, per-utterance nll, the whole gradient and b's alone against the oracle; bitwise the same a second time; the
    greedy decode of the engine's own logits"""
    feats, seq_len, labels, label_len = batch
    e.set_params(O.flatten(params))
    loss, nll, grads = e.loss_and_grads(feats, seq_len, labels, label_len)
    lo, nllo, go, logits_o = O.network_loss_and_grads(spec, params, feats, seq_len, labels, label_len)
    gof = O.flatten(go)
    (_, boff, br, bc), = [t for t in e.tensors() if t[0] == 'b']
    err = dict(loss=abs(loss - lo) / abs(lo), nll=float(np.max(np.abs(nll - nllo) / np.abs(nllo))),
               grad=rel(grads, gof), b=rel(grads[boff:boff + br * bc], go[-1]))
    again = e.loss_and_grads(feats, seq_len, labels, label_len)
    lg = e.forward(feats, seq_len)
    err['logits'] = float(max(np.abs(lg[:seq_len[b], b] - logits_o[:seq_len[b], b]).max() for b in range(len(seq_len))))
    got = e.greedy_decode(feats, seq_len)
    print(tag, 'T %d' % feats.shape[1], json.dumps({k: float('%.3g' % v) for k, v in err.items()}),
          'decoded', [len(h) for h in got])
    assert loss == pytest.approx(lo, rel=3e-5)
    np.testing.assert_allclose(nll, nllo, rtol=3e-5, atol=1e-5)
    assert err['grad'] <= gtol and err['b'] <= gtol, err
    assert again[0] == loss
    np.testing.assert_array_equal(again[1], nll)
    np.testing.assert_array_equal(again[2], grads)
    assert err['logits'] <= logit_atol
    assert got == O.greedy_decode(lg.astype(np.float64), seq_len)
    return loss, grads


MATRIX = [(ks, Lmax, kind) for ks, widths in LMAX_BY_KS.items() for Lmax in widths for kind in KERNEL_C]


@pytest.mark.parametrize('KS,Lmax,kernel', MATRIX, ids=['KS%d-Lmax%d-%s' % c for c in MATRIX])
def test_every_instantiation_matches_the_oracle(KS, Lmax, kernel):
    assert ks_of(Lmax) == KS
    C = KERNEL_C[kernel]
    spec = O.ModelSpec(5, 16, 1, True, 'concat', C)
    e = engine_for(spec)
    check_case(e, spec, net_params(spec, Lmax), lattice_batch(C, Lmax, seed=Lmax * 7 + C), GTOL,
               'KS %d Lmax %d %s C %d:' % (KS, Lmax, kernel, C))
    e.close()


@pytest.mark.parametrize('C,kernel', [(31, 'fast'), (32, 'plain')], ids=['C31-fast', 'C32-plain'])
def test_class_count_edges_at_KS12(C, kernel):
    """C 31: the fast kernel with the blank in column 30, beside the NEG column 31 idle states park on; C 32: Cp = 32 but
    no spare column, the plain kernel.  Lmax 383, KS 12."""
    spec = O.ModelSpec(5, 16, 1, True, 'concat', C)
    batch = lattice_batch(C, 383, seed=C)
    assert (batch[2][1] == C - 2).sum() > 5                  # the label next to the blank, many times
    e = engine_for(spec)
    check_case(e, spec, net_params(spec, C), batch, GTOL, 'KS 12 Lmax 383 %s C %d:' % (kernel, C))
    e.close()


SHARP = [(ks, Lmax, kind) for ks, Lmax in ((8, 255), (16, 511)) for kind in KERNEL_C]


@pytest.mark.parametrize('KS,Lmax,kernel', SHARP, ids=['KS%d-Lmax%d-%s' % c for c in SHARP])
def test_sharp_posteriors_over_thirty_ring_turns(KS, Lmax, kernel):
    """The projection scaled by 60 (posteriors as sharp as a trained net's, the column level moving by 2^80 from one frame
    to the next, as in test_gpu_edges.test_ctc_lattice_on_flat_sharp_and_pinned_posteriors) at T 1000: more than 30 turns
    of the 32-frame chunks through the emission ring, 250 column offsets per walk."""
    assert ks_of(Lmax) == KS
    C = KERNEL_C[kernel]
    spec = O.ModelSpec(5, 16, 1, True, 'concat', C)
    e = engine_for(spec)
    check_case(e, spec, net_params(spec, Lmax + 1, scale=60.0), lattice_batch(C, Lmax, seed=Lmax + C, T=1000),
               GTOL_SHARP[KS], 'sharp KS %d Lmax %d %s C %d:' % (KS, Lmax, kernel, C), logit_atol=60 * 2e-4)
    e.close()


def test_label_limit_and_a_rejected_batch_leaves_no_stale_shape():
    """511 labels train; a 512-wide label array is refused (the lattice has 16 states per lane at most) before anything is
    sized for it; the same handle then computes the 511-wide batch bitwise as before and a batch of another shape as the
    oracle does."""
    from neuralasr_amd import _lib
    spec = O.ModelSpec(5, 16, 1, True, 'concat', 29)
    params = net_params(spec, 511)
    e = engine_for(spec)
    b511 = lattice_batch(29, 511, seed=5110)
    loss, grads = check_case(e, spec, params, b511, GTOL, 'limit, Lmax 511:')
    feats, seq_len, labels, label_len = lattice_batch(29, 512, seed=5120)
    with pytest.raises(_lib.NasrError, match='label length'):
        e.loss_and_grads(feats, seq_len, labels, label_len)
    with pytest.raises(_lib.NasrError, match='label length'):            # the width decides, not the longest label
        e.loss_and_grads(feats, seq_len, labels, np.minimum(label_len, 40))
    again = e.loss_and_grads(*b511)
    assert again[0] == loss
    np.testing.assert_array_equal(again[2], grads)
    check_case(e, spec, params, lattice_batch(29, 300, seed=3000, T=777), GTOL, 'after the refusal, Lmax 300:')
    lo = O.network_loss_and_grads(spec, params, *b511)[0]
    assert e.train_step(*b511) == pytest.approx(lo, rel=3e-5)
    p1 = e.get_params()
    assert np.isfinite(p1).all() and not np.array_equal(p1, O.flatten(params).astype(np.float32))
    e.close()


def test_wavenet_handle_at_KS16():
    """The WaveNet handle sizes the lattice in its own shape code (wn_ensure_shape): Lmax 450 (KS 16), C 29, T 600,
    against the fp64 torch model of tests/wavenet_ref.py with test_gpu_wavenet's loss tolerance and TOL_GRAD_WN_LONG for the
    gradients; 512 labels are refused."""
    from neuralasr_amd import _lib
    spec = W.Spec(13, 29, num_blocks=1)
    Lmax, T = 450, 600
    assert ks_of(Lmax) == 16
    _, seq_len, labels, label_len = lattice_batch(29, Lmax, seed=450, T=T)
    rs = np.random.RandomState(451)
    feats = rs.randn(4, T, spec.F).astype(np.float32)
    for b in range(4):
        feats[b, seq_len[b]:] = 0
    e = TW.engine(spec)
    flat = TW.start_params(spec, 12)
    e.set_params(flat)
    rep = {}
    try:
        TW.check_pass(spec, e, flat, feats, seq_len, labels, label_len, TW.TOL_LOSS, TOL_GRAD_WN_LONG, rep)
    finally:
        print('wavenet KS 16 Lmax %d T %d:' % (Lmax, T), json.dumps(rep))
    wide = np.concatenate([labels, labels[:, :62]], 1)
    with pytest.raises(_lib.NasrError, match='label length'):
        e.loss_and_grads(feats, seq_len, wide, label_len)
    e.close()
