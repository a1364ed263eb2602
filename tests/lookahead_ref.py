"""float64 restatement of a look-ahead session on a bidirectional (concat) LSTM CTC network, for ONE stream (DESIGN.md
§18): what tests/test_gpu_lookahead.py compares the session's logits and saved forward state with.

The rule: the session holds up to R feature rows.  A feed of n new rows has P = held + n pending rows; it emits E = P rows
when it is the utterance's last feed, else E = max(0, P - R), and the last P - E rows stay held.  With E = 0 nothing runs.
Else the WINDOW, all P pending rows, runs through the whole network: dense stages row by row, every layer's forward
direction from the saved state (the state saved for the next feed is the one after row E - 1), every layer's backward
direction from zero at row P - 1 down to row 0; logits come back for rows 0 .. E-1.

Cell and dense arithmetic as tests/stream_ref.py (min(relu(x W + b), clip) without dropout); the
parameter order is oracle.nasr_oracle.ModelSpec.param_shapes.  tests/test_lookahead_host.py pins it to
oracle.nasr_oracle.network_forward: one window over the whole utterance gives the whole utterance's logits."""
import numpy as np


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def zero_state(spec):
    """[L][2][H]: per layer the forward direction's c, then its h"""
    return np.zeros((spec.num_layers, 2, spec.hidden))


def emitted(held, n, R, last):
    """(E, rows held afterwards) of a feed of n new rows behind `held` held ones"""
    P = held + n
    E = P if last else max(0, P - R)
    return E, P - E


def _cell(x, h, c, kernel, bias, H, fb):
    g = np.concatenate([x, h]) @ kernel + bias
    c = c * _sig(g[2 * H:3 * H] + fb) + _sig(g[0:H]) * np.tanh(g[H:2 * H])
    return np.tanh(c) * _sig(g[3 * H:4 * H]), c


def run_window(spec, params, x, state, E):
    """x [P, F]: one window, P >= E >= 1; state [L][2][H] before it.  Returns (logits [E, C], the state after row E - 1)."""
    assert spec.bidirectional and spec.merge == 'concat' and not any(spec.dropout)
    p = [np.asarray(q, np.float64) for q in params]
    x = np.asarray(x, np.float64)
    state = np.array(state, np.float64)
    P, H = x.shape[0], spec.hidden
    assert 1 <= E <= P
    pi = 0
    for _ in spec.pre:
        x = np.minimum(np.maximum(x @ p[pi + 1] + p[pi], 0.0), spec.relu_clip)       # (b_i, h_i)
        pi += 2
    for l in range(spec.num_layers):
        kf, bf, kb, bb = p[pi:pi + 4]
        pi += 4
        out = np.zeros((P, 2 * H))
        c, h = state[l, 0].copy(), state[l, 1].copy()
        for t in range(P):
            h, c = _cell(x[t], h, c, kf, bf, H, spec.forget_bias)
            out[t, :H] = h
            if t == E - 1:
                state[l, 0], state[l, 1] = c, h
        c, h = np.zeros(H), np.zeros(H)
        for t in range(P - 1, -1, -1):
            h, c = _cell(x[t], h, c, kb, bb, H, spec.forget_bias)
            out[t, H:] = h
        x = out
    if spec.deepspeech:
        if spec.post:
            x = np.minimum(np.maximum(x @ p[pi + 1] + p[pi], 0.0), spec.relu_clip)
            pi += 2
        logits = x @ p[pi + 1] + p[pi]                                                # (b6, h6)
    else:
        logits = x @ p[pi] + p[pi + 1]                                                # (W, b)
    return logits[:E], state


def run_session(spec, params, utt, feeds, R, last=True):
    """utt [T, F] fed as feeds[k] new rows in feed k (0 allowed; their sum is at most T); `last`: the final feed declares
    the utterance complete.  Returns (logits, states): per feed the emitted logits [E_k, C] (E_k may be 0) and the forward
    state [L][2][H] after it."""
    utt = np.asarray(utt, np.float64).reshape(-1, spec.feature_size)
    assert sum(feeds) <= len(utt) and R >= 1
    state = zero_state(spec)
    held = np.zeros((0, spec.feature_size))
    pos, logits, states = 0, [], []
    for k, n in enumerate(feeds):
        pend = np.concatenate([held, utt[pos:pos + n]])
        pos += n
        E, keep = emitted(len(held), n, R, last and k == len(feeds) - 1)
        if E > 0:
            lg, state = run_window(spec, params, pend, state, E)
        else:
            lg = np.zeros((0, spec.num_classes))
        held = pend[E:]
        assert len(held) == keep
        logits.append(lg)
        states.append(state.copy())
    return logits, states
