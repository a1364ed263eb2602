"""float64 restatement of a unidirectional LSTM CTC network run chunk by chunk with carried state: what
tests/test_gpu_stream.py compares the stream session's saved (c, h) with.  The cell is SURVEY.md Appendix A.1
(g = [x,h]·kernel + bias; i,j,f,o; c' = c·σ(f+forget_bias) + σ(i)·tanh(j); h' = tanh(c')·σ(o)), the dense stages are
min(relu(x W + b), clip) without dropout; the parameter order is oracle.nasr_oracle.ModelSpec.param_shapes.
tests/test_stream_host.py pins it to oracle.nasr_oracle.network_forward: chunks with carried state give the whole
utterance's logits."""
import numpy as np


def _sig(x):
    return 1.0 / (1.0 + np.exp(-x))


def zero_state(spec):
    """[L][2][H]: per layer c, then h"""
    return np.zeros((spec.num_layers, 2, spec.hidden))


def run_chunk(spec, params, x, state):
    """x [n, F]: the next n frames of ONE stream; state [L][2][H] before them.  Returns (logits [n, C], state after
    them).  n = 0 returns the state as it is."""
    assert not spec.bidirectional and not any(spec.dropout)
    p = [np.asarray(q, np.float64) for q in params]
    x = np.asarray(x, np.float64)
    state = np.array(state, np.float64)
    pi = 0
    for _ in spec.pre:
        x = np.minimum(np.maximum(x @ p[pi + 1] + p[pi], 0.0), spec.relu_clip)       # (b_i, h_i)
        pi += 2
    H = spec.hidden
    for l in range(spec.num_layers):
        kernel, bias = p[pi], p[pi + 1]
        pi += 2
        c, h = state[l, 0].copy(), state[l, 1].copy()
        out = np.zeros((x.shape[0], H))
        for t in range(x.shape[0]):
            g = np.concatenate([x[t], h]) @ kernel + bias
            c = c * _sig(g[2 * H:3 * H] + spec.forget_bias) + _sig(g[0:H]) * np.tanh(g[H:2 * H])
            h = np.tanh(c) * _sig(g[3 * H:4 * H])
            out[t] = h
        state[l, 0], state[l, 1] = c, h
        x = out
    if spec.deepspeech:
        if spec.post:
            x = np.minimum(np.maximum(x @ p[pi + 1] + p[pi], 0.0), spec.relu_clip)
            pi += 2
        return x @ p[pi + 1] + p[pi], state                                           # (b6, h6)
    return x @ p[pi] + p[pi + 1], state                                               # (W, b)


def state_after(spec, params, x):
    """the state [L][2][H] after all frames of x [n, F], from zero"""
    return run_chunk(spec, params, x, zero_state(spec))[1]
