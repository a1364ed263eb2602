"""An independent fp64 torch-CPU model of the reference's LAS (networks/las.py) for the tests: the pyramidal BiLSTM encoder,
the attention decoder with the per-step input ids given (so that a GPU pass's scheduled samples can be replayed),
sequence_loss, and the sampling hash of neuralasr_amd/csrc/las.hip.  The same model runs in torch fp32 (dtype=), which
prices what fp32 arithmetic costs on a batch; trained_like() moves initial weights into the regime of a trained network
(peaked attention, saturating gates); per_tensor_errors() is the gradient metric; MUTANTS are two deliberately wrong
models the host tests use to show that the metric would notice a broken attention backward pass."""
import numpy as np
import torch

from neuralasr_amd.networks.las import tensor_specs

H = 250
# (k_att, k_rec) of trained_like(): what tests/test_las_host.py asserts of each regime is what the GPU tests rest on
REGIMES = {'moderate': (8, 2), 'peaked': (16, 3)}
MUTANTS = ('q_detached', 'alpha_detached')   # forward(mutant=): q cut before the score / alpha cut before the context


def _np_dtype(dtype):
    return {torch.float64: np.float64, torch.float32: np.float32}[dtype]


def unflatten(flat, F, C, dtype=torch.float64):
    out, off = {}, 0
    nd = _np_dtype(dtype)
    for name, r, c in tensor_specs(F, C):
        n = r * c
        t = torch.tensor(np.asarray(flat[off:off + n], nd).reshape(r, c) if c > 1 else
                         np.asarray(flat[off:off + n], nd), requires_grad=True)
        out[name] = t
        off += n
    return out


def tensor_slices(F, C):
    """name -> slice of the flat TF-order vector"""
    out, off = {}, 0
    for name, r, c in tensor_specs(F, C):
        out[name] = slice(off, off + r * c)
        off += r * c
    return out


def initial_params(F, C, seed=3):
    """LAS.initial_params without an engine (the flat TF-order vector, fp32)"""
    from neuralasr_amd.networks.las import LAS
    tensors = [(name, sl.start, r, c) for (name, r, c), sl in zip(tensor_specs(F, C), tensor_slices(F, C).values())]
    return LAS.initial_params(LAS.__new__(LAS), tensors, seed)


def make_batch(B, T, F, U, C, rs, empty=False, must_use=()):
    """feats [B,T,F] zero past seq, seq, labels [B,U], label lengths (utterance 0 empty if asked).  must_use: classes that
    are written into utterance 1's first labels, whose length then covers them (so that they count in the loss)."""
    feats = rs.randn(B, T, F).astype(np.float32)
    seq = rs.randint(1, T + 1, size=B)
    for b in range(B):
        feats[b, seq[b]:] = 0
    labels = rs.randint(0, C, size=(B, U)).astype(np.int32)
    ll = rs.randint(0, U + 1, size=B).astype(np.int32)
    if empty:
        ll[0] = 0
    if must_use:
        labels[1, :len(must_use)] = must_use
        ll[1] = max(ll[1], len(must_use))
    return feats, seq, labels, ll


REGIME_SHAPES = ((40, 5, 9), (17, 17, 12))   # (T, B, U): L4 = 6 and 4 memory frames


def regime_case(regime, T, B, U, F=16, C=12, must_use=()):
    """The batch and parameters of a regime test, the same for the host test of its conditions and for the GPU test:
    (flat, feats, seq, labels, label lengths), utterance 0 with an empty label.  The batch seeds of REGIME_SHAPES are
    picked among 0..13 for the conditions tests/test_las_host.py asserts (with B = 5 and random label lengths the share
    of attention_v's gradient in the peaked regime runs from 2e-4 to 5e-3 from batch to batch)."""
    rs = np.random.RandomState({(40, 5, 9): 6, (17, 17, 12): 7}.get((T, B, U), T * 100 + B + U))
    flat = trained_like(initial_params(F, C, seed=3), F, C, *REGIMES[regime])
    return (flat,) + make_batch(B, T, F, U, C, rs, empty=True, must_use=must_use)


def trained_like(flat, F, C, k_att, k_rec):
    """Initial parameters moved towards what training makes of them: the attention's three tensors times k_att (sharper
    scores), every encoder kernel and the decoder's kernel times k_rec (gates that saturate); rounded through fp32."""
    out = np.array(flat, np.float64)
    for name, sl in tensor_slices(F, C).items():
        if name in ('attention_v', 'memory_layer/kernel', 'query_layer/kernel'):
            out[sl] *= k_att
        elif name == 'decoder_lstm/kernel' or (name.startswith('bidirectional_rnn/') and name.endswith('/kernel')):
            out[sl] *= k_rec
    return out.astype(np.float32)


def per_tensor_errors(g, g_ref, F, C):
    """name -> ||g_t - ref_t|| / max(||ref_t||, 1e-3 * ||ref||): every tensor against its own size, so that a small
    tensor's gradient is not hidden behind a large one's (the floor only keeps a tensor that is zero from dividing by it)"""
    g, g_ref = np.asarray(g, np.float64), np.asarray(g_ref, np.float64)
    floor = 1e-3 * np.linalg.norm(g_ref)
    # (1e-30: a batch without a label has a zero gradient, which only zeros match)
    return {name: float(np.linalg.norm(g[sl] - g_ref[sl]) / max(np.linalg.norm(g_ref[sl]), floor, 1e-30))
            for name, sl in tensor_slices(F, C).items()}


def rel_norm(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(a - ref) / max(np.linalg.norm(ref), 1e-30))


TOL_MARGIN, TOL_FLOOR = 4.0, 2e-6


def tolerances(ref, ref32, F, C):
    """What a correct fp32 implementation may differ from the fp64 model `ref` = (loss, logits, gradient) on this batch,
    priced by the same model in torch fp32 (`ref32`): TOL_MARGIN times its error, floored at TOL_FLOOR, for the loss
    (relative), the logits (rel_norm) and the worst tensor of per_tensor_errors.  The margin: another fp32 implementation
    sums in other orders (k-ascending fmaf chains, MFMA blocks) than torch's CPU kernels, so its error is another draw of
    the same size, not a smaller one.  Returns (tolerances, the fp32 model's errors), both {'loss', 'logits', 'grad'}."""
    e32 = {'loss': abs(ref32[0] - ref[0]) / max(abs(ref[0]), 1e-30), 'logits': rel_norm(ref32[1], ref[1]),
           'grad': max(per_tensor_errors(ref32[2], ref[2], F, C).values())}
    return {k: max(TOL_MARGIN * v, TOL_FLOOR) for k, v in e32.items()}, e32


def tensor_shares(g_ref, F, C):
    """name -> ||ref_t|| / ||ref||"""
    g_ref = np.asarray(g_ref, np.float64)
    n = np.linalg.norm(g_ref)
    return {name: float(np.linalg.norm(g_ref[sl]) / n) for name, sl in tensor_slices(F, C).items()}


def _cell(x, h, c, W, b):
    g = torch.cat([x, h], 1) @ W + b
    i, j, f, o = g.split(g.shape[1] // 4, 1)
    c = c * torch.sigmoid(f + 1.0) + torch.sigmoid(i) * torch.tanh(j)
    return torch.tanh(c) * torch.sigmoid(o), c


def forward(P, feats, labels, ids, dtype=torch.float64, alphas=None, mutant=None):
    """feats [B,T,F], labels [B,U], ids [B,U] (the inputs fed to every step) -> logits [B,U,C].  alphas: a list that
    receives every step's attention weights [B,L4] (numpy).  mutant: one of MUTANTS, a model whose backward pass is wrong
    on purpose (its forward values are the right ones)."""
    assert mutant is None or mutant in MUTANTS
    x = torch.tensor(np.asarray(feats, _np_dtype(dtype)))
    B = x.shape[0]
    for i in range(4):
        if x.shape[1] % 2:
            x = torch.cat([x, torch.zeros(B, 1, x.shape[2], dtype=x.dtype)], 1)
        L = x.shape[1]
        outs = []
        finals = []
        for d in ('fw', 'bw'):
            W, b = P['bidirectional_rnn/%s/%s_%d/kernel' % (d, d, i)], P['bidirectional_rnn/%s/%s_%d/bias' % (d, d, i)]
            h = torch.zeros(B, H, dtype=x.dtype)
            c = torch.zeros(B, H, dtype=x.dtype)
            seq = [None] * L
            order = range(L) if d == 'fw' else range(L - 1, -1, -1)
            for t in order:
                h, c = _cell(x[:, t], h, c, W, b)
                seq[t] = h
            outs.append(torch.stack(seq, 1))
            finals.append((h, c))
        mem = torch.cat(outs, 2)
        x = torch.cat([mem[:, 0::2], mem[:, 1::2]], 2)
    hd = torch.cat([finals[0][0], finals[1][0]], 1)
    cd = torch.cat([finals[0][1], finals[1][1]], 1)
    keys = mem @ P['memory_layer/kernel']
    C = P['projection_layer/bias'].shape[0]
    a = torch.zeros(B, H, dtype=x.dtype)
    ids = torch.tensor(np.asarray(ids, np.int64))
    logits = []
    for t in range(ids.shape[1]):
        inp = torch.cat([torch.nn.functional.one_hot(ids[:, t], C).to(x.dtype), a], 1)
        hd, cd = _cell(inp, hd, cd, P['decoder_lstm/kernel'], P['decoder_lstm/bias'])
        q = hd @ P['query_layer/kernel']
        if mutant == 'q_detached':
            q = q.detach()
        score = (torch.tanh(keys + q[:, None, :]) * P['attention_v']).sum(2)
        alpha = torch.softmax(score, 1)
        if alphas is not None:
            alphas.append(alpha.detach().numpy().copy())
        if mutant == 'alpha_detached':
            alpha = alpha.detach()
        ctx = (alpha[:, :, None] * mem).sum(1)
        a = torch.cat([hd, ctx], 1) @ P['attention_layer/kernel']
        logits.append(a @ P['projection_layer/kernel'] + P['projection_layer/bias'])
    return torch.stack(logits, 1)


def sequence_loss(logits, labels, labels_len):
    U = logits.shape[1]
    w = torch.tensor((np.arange(U)[None, :] < np.asarray(labels_len)[:, None]).astype(np.float64)).to(logits.dtype)
    ce = torch.nn.functional.cross_entropy(logits.reshape(-1, logits.shape[2]),
                                           torch.tensor(np.asarray(labels, np.int64)).reshape(-1), reduction='none')
    return (ce * w.reshape(-1)).sum() / (w.sum() + 1e-12)


def loss_and_grads(flat, F, C, feats, labels, labels_len, ids=None, dtype=torch.float64, alphas=None, mutant=None):
    """(loss, logits [B,U,C], flat gradient in TF order) computed in dtype (fp64, or fp32 to price fp32 arithmetic)"""
    P = unflatten(flat, F, C, dtype)
    ids = labels if ids is None else ids
    logits = forward(P, feats, labels, ids, dtype, alphas, mutant)
    loss = sequence_loss(logits, labels, labels_len)
    loss.backward()
    # (a mutant may cut a tensor off the loss altogether: its gradient is zero)
    g = np.concatenate([(torch.zeros_like(P[n]) if P[n].grad is None else P[n].grad).numpy().ravel()
                        for n, _, _ in tensor_specs(F, C)])
    return float(loss.detach()), logits.detach().numpy(), g


def lowbias32(x):
    x = np.uint32(x)
    with np.errstate(over='ignore'):
        x ^= x >> np.uint32(16); x = np.uint32(x * np.uint32(0x7FEB352D))
        x ^= x >> np.uint32(15); x = np.uint32(x * np.uint32(0x846CA68B))
        x ^= x >> np.uint32(16)
    return np.uint32(x)


def sample_uniforms(seed, counter, tower, t, b):
    """(u0, u1): the 24-bit Bernoulli and inverse-CDF draws of utterance b's input at step t"""
    with np.errstate(over='ignore'):
        key = np.uint32((seed + 0x9E3779B9 * (tower + 1) + 0x85EBCA6B * counter) & 0xFFFFFFFF)
    base = np.uint32(((t * 64 + b) * 2) & 0xFFFFFFFF)
    return int(lowbias32(base ^ key) >> np.uint32(8)), int(lowbias32(np.uint32(base + 1) ^ key) >> np.uint32(8))
