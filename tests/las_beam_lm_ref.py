"""The LAS beam search fused with an n-gram table (nasr_las_beam_set_lm) as a NumPy restatement in float32
and the score kernel's operation order: tests/las_beam_ref.py's search with one more term in an unfinished row's
log-probs, lp = ((l - max) - lse) + (weight * table[ctx][w]) with the product and the sum rounded separately, and a context
index per beam row (start_id in every digit at first; a finished parent's context is kept, any other becomes
(ctx*C + word) mod K).  penalty, log_softmax and gather_tree are las_beam_ref's own; without a table the search is
las_beam_ref.beam_search itself (Replay is its fp64 model, used as the logits callback)."""
import numpy as np

from tests.las_beam_ref import F32, FLT_LOWEST, Replay, beam_search, gather_tree, log_softmax, penalty  # noqa: F401


def start_context(order, C, start_id):
    ctx = 0
    for _ in range(order - 1):
        ctx = ctx * C + start_id
    return ctx


def step(logits, log_probs, finished, lengths, ctx, end_id, weight, table, lm_weight):
    """one fused step: las_beam_ref.step's outputs plus the rows' new contexts [B,W]"""
    B, W, C = logits.shape
    K = table.shape[0]
    with np.errstate(over='ignore', invalid='ignore'):
        lp = log_softmax(logits)
        lm = (F32(lm_weight) * table[ctx]).astype(F32)            # the rounded product ...
        lp = (lp + lm).astype(F32)                                # ... joins in a rounded sum
        is_end = np.arange(C) == end_id
        lp = np.where(finished[..., None], np.where(is_end, F32(0), FLT_LOWEST)[None, None, :], lp).astype(F32)
        total = (log_probs[..., None] + lp).astype(F32)
        len_s = lengths[..., None] + ((~finished)[..., None] & ~is_end[None, None, :]).astype(np.int64)
        score = (total / penalty(len_s, weight)).astype(F32)
    flat = score.reshape(B, W * C)
    idx = np.arange(W * C)
    order = np.stack([np.lexsort((idx, -flat[b].astype(np.float64))) for b in range(B)])
    sel = order[:, :W]
    scores = np.take_along_axis(flat, sel, 1)
    parent, word = sel // C, sel % C
    new_lp = np.take_along_axis(total.reshape(B, W * C), sel, 1)
    prev_fin = np.take_along_axis(finished, parent, 1)
    fin = prev_fin | (word == end_id)
    lens = np.take_along_axis(lengths, parent, 1) + (~prev_fin).astype(np.int64)
    pctx = np.take_along_axis(ctx, parent, 1)
    new_ctx = np.where(prev_fin, pctx, (pctx * C + word) % K)
    return scores, word, parent, new_lp, fin, lens, np.take_along_axis(flat, order, 1), new_ctx


def beam_search_lm(logits_fn, B, W, C, start_id, end_id, max_steps, weight, table, order, lm_weight):
    """las_beam_ref.beam_search with the table [K][C] fused at lm_weight; the result also holds 'ctx' [B,W], the final
    contexts, and 'done_at' [B]: the step after which every beam of the utterance was finished (max_steps if never)"""
    table = np.asarray(table, F32).reshape(C ** (order - 1), C)
    log_probs = np.full((B, W), -np.inf, F32)
    log_probs[:, 0] = 0
    finished = np.ones((B, W), bool)
    finished[:, 0] = False
    lengths = np.zeros((B, W), np.int64)
    ids = np.full((B, W), start_id, np.int64)
    ctx = np.full((B, W), start_context(order, C, start_id), np.int64)
    parent = None
    tr = {'scores': [], 'word': [], 'parent': [], 'margin': []}
    done_at = np.full(B, max_steps, np.int64)
    for t in range(max_steps):
        logits = np.asarray(logits_fn(t, parent, ids), F32)
        sc, word, parent, log_probs, finished, lengths, srt, ctx = step(logits, log_probs, finished, lengths, ctx, end_id,
                                                                        weight, table, lm_weight)
        ids = word
        tr['scores'].append(sc)
        tr['word'].append(word)
        tr['parent'].append(parent)
        top = srt[:, :W + 1].astype(np.float64)
        with np.errstate(invalid='ignore'):
            d = top[:, :-1] - top[:, 1:]
        ok = np.isfinite(top[:, 1:]) & (top[:, 1:] > -1e30) & (d != 0)
        tr['margin'].append(float(d[ok].min()) if ok.any() else np.inf)
        done_at = np.where(finished.all(axis=1) & (done_at == max_steps), t, done_at)
        if finished.all():
            break
    out = {k: np.stack(v) if k != 'margin' else np.asarray(v) for k, v in tr.items()}
    out.update(log_probs=log_probs, finished=finished, lengths=lengths, steps=len(tr['word']), ctx=ctx, done_at=done_at)
    out['ids'] = gather_tree(out['word'], out['parent'], lengths.max(axis=1), end_id)
    return out


def contexts_along(word, parent, order, C, start_id, end_id):
    """the final contexts [B,W] that the update rule gives along a recorded trace word / parent [T,B,W] (integers only)"""
    T, B, W = word.shape
    K = C ** (order - 1)
    ctx = np.full((B, W), start_context(order, C, start_id), np.int64)
    fin = np.ones((B, W), bool)
    fin[:, 0] = False
    for t in range(T):
        pf = np.take_along_axis(fin, parent[t], 1)
        pc = np.take_along_axis(ctx, parent[t], 1)
        ctx = np.where(pf, pc, (pc * C + word[t]) % K)
        fin = pf | (word[t] == end_id)
    return ctx
