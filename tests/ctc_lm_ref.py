"""An independent float64 restatement of the CTC prefix beam search fused with a dense n-gram table (include/nasr.h:
nasr_ctc_beam_search_lm), and the exhaustive scorer that pins it on tiny inputs.  The per-frame procedure
is TF's (advance the live prefixes, then grow them by one label while the grown prefix can still enter the beam); the
fusion rule: every prefix carries its context index, and mass that flows from a prefix to its extension by label c gets
weight * logp[ctx(prefix)][c] + bonus; blank and repeat updates of a prefix itself get nothing; the best path is chosen
by total + weight * eos[ctx]."""
import itertools

import numpy as np

NEG = -np.inf


def _log_softmax(x):
    x = np.asarray(x, np.float64)
    m = x.max()
    return x - (m + np.log(np.exp(x - m).sum()))


def _lse(a, b):
    if a == NEG:
        return b
    if b == NEG:
        return a
    m = max(a, b)
    return m + np.log(np.exp(a - m) + np.exp(b - m))


def root_context(order, C, bos_id):
    ctx = 0
    for _ in range(order - 1):
        ctx = ctx * C + bos_id
    return ctx


class _Prefix(object):
    __slots__ = ('up', 'label', 'ctx', 'kids', 'o_tot', 'o_blank', 'o_label', 'tot', 'blank', 'lab')

    def __init__(self, up, label, ctx):
        self.up, self.label, self.ctx, self.kids = up, label, ctx, {}
        self.o_tot = self.o_blank = self.o_label = NEG
        self.tot = self.blank = self.lab = NEG

    def clear_new(self):
        self.tot = self.blank = self.lab = NEG

    def clear_old(self):
        self.o_tot = self.o_blank = self.o_label = NEG


def beam_search_lm(logits, beam_width, merge_repeated, lm_logp, lm_eos, order, bos_id, weight, bonus):
    """logits [T, C] (blank = C-1) -> (ids, fused score of the best path, gap to the second-best live path; inf when the
    beam ends with one path)"""
    logits = np.asarray(logits, np.float64)
    T, C = logits.shape
    blank = C - 1
    lm_logp = np.asarray(lm_logp, np.float64)
    lm_eos = np.asarray(lm_eos, np.float64)
    K = C ** (order - 1)
    assert lm_logp.shape == (K, C) and lm_eos.shape == (K,)

    def flow(prefix, c):
        return weight * lm_logp[prefix.ctx, c] + bonus

    root = _Prefix(None, -1, root_context(order, C, bos_id))
    root.tot = root.blank = 0.0
    beam = [root]

    def bottom():
        return min(range(len(beam)), key=lambda i: beam[i].tot)

    def admit(p):
        if len(beam) < beam_width:
            beam.append(p)
        else:
            i = bottom()
            if p.tot > beam[i].tot:
                beam[i] = p

    def can_enter(total):
        return total > NEG and (len(beam) < beam_width or total > beam[bottom()].tot)

    for t in range(T):
        lp = _log_softmax(logits[t])
        live = sorted(beam, key=lambda p: -p.tot)
        beam = []
        for p in live:
            p.o_tot, p.o_blank, p.o_label = p.tot, p.blank, p.lab
        for p in live:
            if p.up is not None:
                if p.up.tot != NEG:
                    carried = p.up.o_blank if p.label == p.up.label else p.up.o_tot
                    p.lab = _lse(p.lab, carried + flow(p.up, p.label))
                p.lab += lp[p.label]
            p.blank = p.o_tot + lp[blank]
            p.tot = _lse(p.blank, p.lab)
            admit(p)
        for p in live:
            if not can_enter(p.o_tot):
                continue
            for c in range(C):
                if c == blank:
                    continue
                carried = p.o_blank if c == p.label else p.o_tot
                grown = lp[c] + (carried + flow(p, c))
                kid = p.kids.get(c)
                if not can_enter(grown):
                    if kid is not None and kid.tot == NEG:
                        kid.clear_old()
                    continue
                if kid is None:
                    kid = p.kids[c] = _Prefix(p, c, (p.ctx * C + c) % K)
                if kid.tot != NEG:
                    continue
                kid.tot, kid.blank, kid.lab = grown, NEG, grown
                if len(beam) == beam_width:
                    beam[bottom()].clear_new()
                admit(kid)
    finals = sorted((p.tot + weight * lm_eos[p.ctx] for p in beam), reverse=True)
    best = max(beam, key=lambda p: p.tot + weight * lm_eos[p.ctx])
    ids, last, p = [], -1, best
    while p.up is not None:
        if not merge_repeated or p.label != last:
            ids.append(p.label)
        last = p.label
        p = p.up
    gap = finals[0] - finals[1] if len(finals) > 1 and finals[1] > NEG else np.inf
    return ids[::-1], finals[0], gap


def exhaustive(logits, lm_logp, lm_eos, order, bos_id, weight, bonus):
    """every labelling's log P_ctc(y) + sum_i (weight * lm(y_i | y_<i) + bonus) + weight * eos(ctx(y)) by enumeration of all
    alignments: (best labelling, its score, gap to the second)"""
    logits = np.asarray(logits, np.float64)
    T, C = logits.shape
    blank = C - 1
    K = C ** (order - 1)
    p = np.exp(np.stack([_log_softmax(r) for r in logits]))
    mass = {}
    for path in itertools.product(range(C), repeat=T):
        y, prev = [], None
        for k in path:
            if k != prev and k != blank:
                y.append(k)
            prev = k
        pr = 1.0
        for t, k in enumerate(path):
            pr *= p[t, k]
        mass[tuple(y)] = mass.get(tuple(y), 0.0) + pr
    scored = []
    for y, pr in mass.items():
        ctx, s = root_context(order, C, bos_id), np.log(pr)
        for c in y:
            s += weight * float(lm_logp[ctx, c]) + bonus
            ctx = (ctx * C + c) % K
        scored.append((s + weight * float(lm_eos[ctx]), y))
    scored.sort(reverse=True)
    gap = scored[0][0] - scored[1][0] if len(scored) > 1 else np.inf
    return list(scored[0][1]), scored[0][0], gap
