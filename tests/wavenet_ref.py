"""An independent fp64 torch-CPU model of the reference's WaveNet (networks/wavenet.py) for the WaveNet tests: F.conv1d
with dilation r and padding 3r for atrous_conv2d 'SAME', batch norm with tf.contrib.layers.batch_norm's statistics,
F.ctc_loss, autograd for the gradients, TF's Adam and the moving-statistics recurrence.  Not collected (no test_ prefix)."""
import numpy as np
import torch
import torch.nn.functional as F

KS = 7


class Spec:
    def __init__(self, feature_size, num_classes, num_blocks=3, rates=(1, 2, 4, 8, 16), dim=128, eps=1e-3, decay=0.99):
        self.F, self.C, self.nb, self.rates, self.dim = feature_size, num_classes, num_blocks, tuple(rates), dim
        self.eps, self.decay = eps, decay

    def blocks(self):
        return [(i, r) for i in range(self.nb) for r in self.rates]

    @property
    def sites(self):
        return 2 + 3 * len(self.blocks())


def tensor_specs(spec):
    """(name, rows, cols) in TF variable creation order."""
    D = spec.dim
    out = [('front/conv_in/W', spec.F, D)]

    def bn(scope):
        out.extend([(scope + '/BatchNorm/beta', D, 1), (scope + '/BatchNorm/gamma', D, 1)])
    bn('front/conv_in')
    for i, r in spec.blocks():
        n = 'block_%d_%d' % (i, r)
        for kind in ('conv_filter', 'conv_gate'):
            out.append(('%s/%s%s/W' % (n, kind, n), KS * D, D))
            bn('%s/%s%s' % (n, kind, n))
        out.append(('%s/conv_out%s/W' % (n, n), D, D))
        bn('%s/conv_out%s' % (n, n))
    out.append(('logit/conv_1/W', D, D))
    bn('logit/conv_1')
    out.append(('logit/conv_2/W', D, spec.C))
    return out


def bessel_sites(spec):
    """Per BN site: True where the update uses the N/(N-1) variance (the 1x1 convolutions: fused batch norm)."""
    out = [True]
    for _ in spec.blocks():
        out += [False, False, True]
    return out + [True]


def unflatten(spec, flat):
    P, o = {}, 0
    for name, r, c in tensor_specs(spec):
        P[name] = torch.tensor(np.asarray(flat[o:o + r * c], dtype=np.float64).reshape(r, c) if c > 1 else
                               np.asarray(flat[o:o + r * c], dtype=np.float64))
        o += r * c
    return P


def flatten_grads(spec, P):
    return np.concatenate([P[n].grad.detach().numpy().ravel() for n, _, _ in tensor_specs(spec)])


def init_params(spec, seed):
    """he_uniform with wavenet.py's _get_fans quirk; beta 0, gamma 1."""
    rs = np.random.RandomState(seed)
    chunks = []
    for name, r, c in tensor_specs(spec):
        if name.endswith('/W'):
            fan = r if ('/conv_filter' in name or '/conv_gate' in name) else np.sqrt(r * c)
            s = np.sqrt(1.0 / fan)
            chunks.append(rs.uniform(-s, s, r * c))
        elif name.endswith('gamma'):
            chunks.append(np.ones(r * c))
        else:
            chunks.append(np.zeros(r * c))
    return np.concatenate(chunks).astype(np.float32)


def forward(spec, P, feats, training, bn=None):
    """logits [T,B,C] (fp64 torch) and, in training mode, the per-site batch statistics [(mean, population var, n)].
    Inference mode reads bn = (moving_mean [S,D], moving_var [S,D])."""
    D = spec.dim
    x = torch.as_tensor(np.asarray(feats, dtype=np.float64))
    B, T, _ = x.shape
    stats = []
    names = iter([n for n, _, _ in tensor_specs(spec) if n.endswith('/beta')])
    site = [0]

    def bnorm(y):
        s = site[0]
        site[0] += 1
        scope = next(names)[:-len('/beta')]
        if training:
            m = y.mean(dim=(0, 1))
            v = ((y - m) ** 2).mean(dim=(0, 1))
            stats.append((m.detach().numpy(), v.detach().numpy(), B * T))
        else:
            m = torch.as_tensor(np.asarray(bn[0][s], np.float64))
            v = torch.as_tensor(np.asarray(bn[1][s], np.float64))
        return (y - m) / torch.sqrt(v + spec.eps) * P[scope + '/gamma'] + P[scope + '/beta']

    z = torch.tanh(bnorm(x @ P['front/conv_in/W']))
    skip = 0
    for i, r in spec.blocks():
        n = 'block_%d_%d' % (i, r)
        zt = z.permute(0, 2, 1)

        def dconv(w):
            return F.conv1d(zt, w.reshape(KS, D, D).permute(2, 1, 0), dilation=r, padding=(KS // 2) * r).permute(0, 2, 1)
        f = torch.tanh(bnorm(dconv(P['%s/conv_filter%s/W' % (n, n)])))
        g = torch.sigmoid(bnorm(dconv(P['%s/conv_gate%s/W' % (n, n)])))
        o = torch.tanh(bnorm((f * g) @ P['%s/conv_out%s/W' % (n, n)]))
        z = o + z
        skip = skip + o
    s2 = torch.tanh(bnorm(skip @ P['logit/conv_1/W']))
    logits = (s2 @ P['logit/conv_2/W']).permute(1, 0, 2)
    return logits, stats


def ctc_mean(logits, seq_len, labels, label_len):
    C = logits.shape[2]
    tg = torch.as_tensor(np.concatenate([np.asarray(labels[b][:int(label_len[b])], np.int64) for b in range(len(seq_len))]
                                        + [np.zeros(0, np.int64)]))
    nll = F.ctc_loss(F.log_softmax(logits, dim=2), tg, torch.as_tensor([int(s) for s in seq_len]),
                     torch.as_tensor([int(x) for x in label_len]), blank=C - 1, reduction='none')
    return nll.mean(), nll


def loss_and_grads(spec, flat, feats, seq_len, labels, label_len):
    """(loss, flat grads in TF order, batch statistics) of a training-mode pass."""
    P = unflatten(spec, flat)
    for t in P.values():
        t.requires_grad_(True)
    logits, stats = forward(spec, P, feats, True)
    loss, _ = ctc_mean(logits, seq_len, labels, label_len)
    loss.backward()
    return float(loss), flatten_grads(spec, P), stats


def eval_loss(spec, flat, feats, seq_len, labels, label_len, bn):
    with torch.no_grad():
        logits, _ = forward(spec, unflatten(spec, flat), feats, False, bn)
        loss, nll = ctc_mean(logits, seq_len, labels, label_len)
    return float(loss), nll.numpy(), logits.numpy()


def greedy(logits_tm, seq_len):
    """tf.nn.ctc_greedy_decoder(merge_repeated=True) on [T,B,C] logits."""
    C = logits_tm.shape[2]
    out = []
    for b, L in enumerate(seq_len):
        am = np.argmax(logits_tm[:int(L), b], axis=1)
        hyp, prev = [], -1
        for a in am:
            if a != prev and a != C - 1:
                hyp.append(int(a))
            prev = a
        out.append(hyp)
    return out


def bn_initial(spec):
    S, D = spec.sites, spec.dim
    return {'mm': np.zeros((S, D), np.float32), 'mv': np.ones((S, D), np.float32), 'biased': np.zeros((S, D), np.float32),
            'n': 0}


def update_variance(spec, stats):
    """The variance each site's update uses: N/(N-1) var at the 1x1 sites (N-1 taken as 1 for N = 1), var at the dilated."""
    out = []
    for (m, v, n), bes in zip(stats, bessel_sites(spec)):
        out.append(v * (n / max(n - 1, 1)) if bes else v)
    return np.stack([m for m, _, _ in stats]).astype(np.float32), np.stack(out).astype(np.float32)


def bn_update(spec, state, mean, v):
    """One moving-statistics update in fp32 (moving_averages.assign_moving_average, zero_debias for the mean only)."""
    f = np.float32
    omd = f(1.0 - float(f(spec.decay)))
    n = state['n'] + 1
    biased = (state['biased'] - (state['biased'] - f(mean).astype(f)) * omd).astype(f)
    debias = f(f(1) - np.power(f(1) - omd, f(n)))
    mv = (state['mv'] - (state['mv'] - v.astype(f)) * omd).astype(f)
    return {'mm': (biased / debias).astype(f), 'mv': mv, 'biased': biased, 'n': n}


def adam_tf(p, g, m, v, t, lr, b1=0.9, b2=0.999, eps=1e-8):
    """tf.train.AdamOptimizer's update at step t (1-based), fp64."""
    lr_t = lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t)
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    return p - lr_t * m / (np.sqrt(v) + eps), m, v


def synth_batch(spec, B, T, seed, Lmax=5, seq_len=None, label_len=None):
    """Features zero past seq_len (dataset.py pads with zeros), labels in [0, C-2]."""
    rs = np.random.RandomState(seed)
    seq = np.asarray(seq_len if seq_len is not None else rs.randint(max(1, T // 2), T + 1, size=B), np.int32)
    seq[0] = T if seq_len is None else seq[0]
    feats = rs.randn(B, T, spec.F).astype(np.float32)
    for b in range(B):
        feats[b, seq[b]:] = 0
    if label_len is None:
        label_len = [min(int(rs.randint(1, Lmax + 1)), max(0, (int(s) - 1) // 2)) for s in seq]
    ll = np.asarray(label_len, np.int32)
    labels = np.zeros((B, max(1, int(ll.max()) if B else 1)), np.int32)
    for b in range(B):
        labels[b, :ll[b]] = rs.randint(0, spec.C - 1, size=ll[b])
    return feats, seq, labels, ll
