"""NumPy fp64 reference of the LSTM recurrence kernels (csrc/lstm.hip, lstm_persist.hip, lstm_wide.hip) and the error
model a correct kernel of each arithmetic class must stay inside.  The counterpart of gemm_ref.py; used by
tests/test_rec_ref_host.py (CPU) and tests/test_gpu_rec_kernels.py.

Layout, as csrc/kernels.h: rows r = t*Bp + b; gates / dG [T][Bp][D][Hp][4] (column d*4Hp + 4j + g, g = i, j, f, o);
c / out / dOut [T][Bp][D][Hp]; U [D][Hp][Hp][4] (row = contracted unit k).  Direction 1 consumes frame len-1-s at step s,
so in FRAME terms: frame t of row b is computed iff t < seq_len[b], and the state it starts from is that of frame t-1
(direction 0) or t+1 (direction 1), the initial state at the first frame visited.

  forward / backward      the fp64 recurrence and its BPTT (pinned to oracle/nasr_oracle.py by the host test)
  KINDS                   the arithmetic classes: accumulation depth, fp16 planes or not - read from the kernels
  fwd_step_bound          per-element bound of ONE step from given previous state (+ the bound carried on that state)
  check_forward           local check (every step from the kernel's own previous state), running check, output contract
  check_backward          running check of dG along an fp64 trajectory, output contract, rowpart / colpart
  emulate_*               fp32 NumPy models of the arithmetic classes (the bound must hold them)
  cases / make_inputs     the cases the GPU test runs, as data

Error model, one line per term (u = 2^-24; every constant below is one of these):
  product      (depth + 2) u sum_k |h_k U_k|      depth = a wave's K share + the adds of the LDS / partial-sum reduction
  planes (f16) sum_k |h_k| dU_k + dh_k |U_k|,  dU = max(2^-23 |U|, 2^-39 colmax),  dh = max(2^-23 |h|, 2^-36)
               (two fp16 parts under a scale that puts the column maximum in [2^14, 2^15): half an fp16 subnormal step is
               2^-25 there; h travels as parts of h 2^14 with the low part divided by 8 - the epoch bit's price - so its
               floor is 8 * 2^-25 / 2^14; the wide kernel's parts of 2 h, the low one times 2^10, have the same floor,
               2^-25 / 2^10 / 2)
  dropped      2^-22 sum_k |h_k U_k|              the h2 U2 product the fp16 form leaves out
  sum          u (|x| + |pre|) (+ u |f + forget_bias|)   the adds of the hoisted input half and of the forget bias
  activation   4 u (sigmoid), 8 u (tanh) absolute: v_exp_f32 and v_rcp_f32 are 1-ulp instructions, x log2e is rounded
  propagation  first order through c' = c f + i j and h = tanh(c') o, with the second-derivative remainder of the
               activations (max |sigmoid''| = 1/(6 sqrt 3), max |tanh''| = 4/(3 sqrt 3)) and u per rounded operation
  BPTT         the same product term over the gate columns (+ 2 u for the epoch bit the persistent kernel stores in the last
               mantissa bit of every partial sum), u per operation of lstm_cell_bwd_tc, 8 u on tanh(c), and
               1 - x^2 carrying u (x^2 + |1 - x^2|): an ABSOLUTE error of order u where the factor itself is small
  wide BPTT    planes on both sides: U^T under per-unit (row of U) scales, dU = max(2^-23 |U|, 2^-39 rowmax); dG times the
               power-of-two S of its (direction, utterance) that puts max |dOut| in [2^5, 2^6), d(dG) = max(2^-23 |dG|,
               2^-25 / S); the dropped product 2^-22 sum |dG U|
  underflow    2^-126 per operation of the BPTT cell (8 per dG, times max(1, |c_prev|), the one factor above 1) and per add
               of its product: a result below the smallest normal fp32 number is rounded to a subnormal or flushed
"""
from dataclasses import dataclass
from functools import lru_cache
import zlib

import numpy as np

import gemm_ref as G

U24 = 2.0 ** -24
SIG_ABS = 4 * U24
TANH_ABS = 8 * U24
SIG_D2 = 1.0 / (6.0 * np.sqrt(3.0))
TANH_D2 = 4.0 / (3.0 * np.sqrt(3.0))
POISON = np.float32(1e30)
TINY = 2.0 ** -126                # smallest normal fp32 number
RUNNING_LIMIT = 2.0 ** -10        # the running forward check applies while its bound stays below this


def rup(x, m):
    return (x + m - 1) // m * m


# ------------------------------------------------------------------ arithmetic classes
@dataclass(frozen=True)
class Kind:
    name: str
    f16: bool = False
    bwd: bool = False

    def depth(self, Hp):
        """Longest accumulation chain, in adds, of one output of the recurrent product."""
        n = self.name
        if n == 'step_fwd':        # lstm_fwd_step_kernel: a wave contracts Hp/4 units, acc0 + acc1, 4-wave LDS sum
            return Hp // 4 + 1 + 3
        if n == 'persist_fwd':     # lstm_persist_fwd_kernel: KW = Hp/4 units per wave, (a0+a1)+(a2+a3), (g0+g1)+(g2+g3);
            return Hp // 4 + 2 + 2     # (f16: the three plane products are three of the four accumulators)
        if n == 'wide_fwd':        # lstm_wide_fwd_kernel: an XCD contracts KS = Hp/8 units, h1 U2 and h1 U1 in ONE accumulator
            return 2 * (Hp // 8) + 1 + 8     # (2 KS terms), + the h2 U1 accumulator, the 8 XCDs' partial sums one after the other
        if n == 'step_bwd':
            if Hp > 512 and Hp % 128 == 0:     # two-launch form: 4 K slices of 32 units x one gate per wave, 4-wave sum,
                return 128 + 3 + Hp // 128 + 1 + 1   # Hp/128 partials in two chains + their sum, + dOut
            return 32 + 3 + Hp // 32 + 1       # 32 units of one gate per wave, 4-wave sum, Hp/32 partials, + dOut
        if n == 'wide_bwd':        # lstm_wide_bwd_kernel: a workgroup contracts 256 = Hp/8 gate columns, the three plane products in
            return 3 * (Hp // 8) + 16 + 1 + 1    # ONE accumulator; the XCD's 32 partial sums in two chains of 16 + their sum, + dOut
        if n == 'persist_bwd':     # a CU contracts its 4 NU = Hp/8 gate columns (4 chains + 2), 32 producers summed
            return Hp // 8 + 2 + 32 + 1 + 2    # (8 + 2 levels: counted as 32), + dOut, + 2 for the epoch bit of the partials
        raise KeyError(n)


KINDS = {
    'step_fwd': Kind('step_fwd'), 'step_carry': Kind('step_fwd'), 'persist_fwd32': Kind('persist_fwd'),
    'persist_fwd16': Kind('persist_fwd', f16=True), 'wide_fwd': Kind('wide_fwd', f16=True), 'step_bwd': Kind('step_bwd', bwd=True),
    'persist_bwd': Kind('persist_bwd', bwd=True), 'wide_bwd': Kind('wide_bwd', f16=True, bwd=True),
}


def _sig(x):
    with np.errstate(over='ignore'):
        return 1.0 / (1.0 + np.exp(-x))


# ------------------------------------------------------------------ one forward step, fp64, and its bound
def cell(U, pre, hp, cp, fb, mutant=None):
    """U [Hp][Hp][4], pre [n][Hp][4], hp / cp [n][Hp] -> act [n][Hp][4], c, h (fp64)."""
    Hp = U.shape[0]
    U2 = U.reshape(Hp, 4 * Hp)
    rec = hp @ U2
    if mutant in ('u_high_plane', 'drop_h1u2', 'drop_h2u1'):
        s, inv = G.scale_model(G.line_max(U2.astype(np.float32), 0))
        Us = U2 * s.astype(np.float64)
        u1 = Us.astype(np.float16).astype(np.float64)
        hv = hp * 16384.0
        h1 = hv.astype(np.float16).astype(np.float64)
        if mutant == 'u_high_plane':
            rec = hp @ (u1 * inv)
        elif mutant == 'drop_h1u2':
            rec = rec - (h1 / 16384.0) @ ((Us - u1) * inv)
        else:
            rec = rec - ((hv - h1) / 16384.0) @ (u1 * inv)
    z = pre + rec.reshape(-1, Hp, 4)
    gi, gj = (1, 0) if mutant == 'swap_ij' else (0, 1)
    si = _sig(z[..., gi])
    tj = np.tanh(z[..., gj])
    sf = _sig(z[..., 2] + (0.0 if mutant == 'no_forget_bias' else fb))
    so = _sig(z[..., 3])
    c = cp * sf + si * tj
    h = np.tanh(c) * so
    return np.stack([si, tj, sf, so], -1), c, h


def fwd_step_bound(kind, U, pre, hp, cp, fb, ehp=None, ecp=None):
    """Bounds (e_act [n][Hp][4], e_c, e_h) on one step of a correct kernel of `kind` against cell() of the same inputs;
    ehp / ecp: bounds already carried by hp / cp (the running check; None = the inputs are the kernel's own)."""
    Hp = U.shape[0]
    aU = np.abs(U.reshape(Hp, 4 * Hp))
    ah = np.abs(hp)
    if ehp is not None:
        ah = ah + ehp
    S = ah @ aU
    e = (kind.depth(Hp) + 2) * U24 * S
    if kind.f16:
        cmax = aU.max(axis=0)
        dU = np.maximum(2.0 ** -23 * aU, 2.0 ** -39 * cmax[None, :])
        dh = np.where(ah == 0, 0.0, np.maximum(2.0 ** -23 * ah, 2.0 ** -36))
        e = e + ah @ dU + dh @ aU + 2.0 ** -22 * S
    if ehp is not None:
        e = e + ehp @ aU
    act, c, h = cell(U, pre, hp, cp, fb)
    with np.errstate(over='ignore'):
        z = pre + (hp @ U.reshape(Hp, 4 * Hp)).reshape(-1, Hp, 4)
    e = e.reshape(-1, Hp, 4) + U24 * (np.abs(pre) + np.abs(z))
    e[..., 2] += U24 * np.abs(z[..., 2] + fb)
    d1 = np.stack([act[..., 0] * (1 - act[..., 0]), 1 - act[..., 1] ** 2, act[..., 2] * (1 - act[..., 2]),
                   act[..., 3] * (1 - act[..., 3])], -1)
    d2 = np.array([SIG_D2, TANH_D2, SIG_D2, SIG_D2])
    ab = np.array([SIG_ABS, TANH_ABS, SIG_ABS, SIG_ABS])
    ea = d1 * e + 0.5 * d2 * e * e + ab
    ei, ej, ef, eo = (ea[..., g] for g in range(4))
    si, tj, sf, so = (act[..., g] for g in range(4))
    acp = np.abs(cp)
    ec = acp * ef + np.abs(si) * ej + np.abs(tj) * ei + ei * ej + U24 * (np.abs(cp * sf) + np.abs(si * tj) + np.abs(c))
    if ecp is not None:
        ec = ec + ecp * (sf + ef)
    tc = np.tanh(c)
    etc = (1 - tc * tc) * ec + 0.5 * TANH_D2 * ec * ec + TANH_ABS
    eh = so * etc + np.abs(tc) * eo + etc * eo + U24 * np.abs(h)
    return ea, ec, eh


# ------------------------------------------------------------------ whole passes, frame-indexed
def _dims(pre):
    T, Bp, D, Hp, _ = pre.shape
    return T, Bp, D, Hp


def _prev_index(T, Bp, seq_len, d):
    """(valid [T][Bp], prev frame [T][Bp] or -1 = the initial state) of direction d."""
    t = np.arange(T)[:, None]
    ln = np.asarray(seq_len, dtype=np.int64)[None, :]
    valid = t < ln
    if d == 0:
        prev = np.where(t > 0, t - 1, -1) + 0 * ln
    else:
        prev = np.where(t + 1 < ln, t + 1, -1)
    return valid, np.where(valid, prev, -1)


def forward(U, pre, seq_len, fb, h0=None, c0=None, mutant=None):
    """fp64 forward pass.  U [D][Hp][Hp][4], pre [T][Bp][D][Hp][4], seq_len [Bp], h0 / c0 [D][Bp][Hp] or None.
    Returns (act, c, h) frame-indexed, zeros where a frame is not computed.  mutant: a WRONG model (host test)."""
    T, Bp, D, Hp = _dims(pre)
    U = np.asarray(U, dtype=np.float64)
    pre = np.asarray(pre, dtype=np.float64)
    ln = np.asarray(seq_len, dtype=np.int64)
    act = np.zeros((T, Bp, D, Hp, 4))
    c = np.zeros((T, Bp, D, Hp))
    h = np.zeros((T, Bp, D, Hp))
    rows = np.arange(Bp)
    for d in range(D):
        hs = np.zeros((Bp, Hp)) if h0 is None else np.array(h0[d], dtype=np.float64)
        cs = np.zeros((Bp, Hp)) if c0 is None else np.array(c0[d], dtype=np.float64)
        hold = hs.copy()
        for s in range(T):
            valid = s < ln
            tb = np.where(valid, (ln - 1 - s) if (d == 1 and mutant != 'bwd_reads_s') else s, 0)
            hin = hs
            if mutant == 'stale_slice' and s > 0:      # one producer's Hp/32 units still hold the step before
                hin = hs.copy()
                hin[:, :Hp // 32] = hold[:, :Hp // 32]
            with np.errstate(over='ignore', invalid='ignore'):
                a_, c_, h_ = cell(U[d], pre[tb, rows, d], hin, cs, fb, mutant)
            v = valid[:, None]
            hold = hs
            if mutant == 'state_not_zeroed':     # a finished row keeps publishing its last h: the output past seq_len
                h[s, rows[~valid], d] = hs[~valid]
            hs = np.where(v, h_, 0.0 if mutant != 'state_not_zeroed' else hs)
            cs = np.where(v, c_, 0.0)
            act[tb[valid], rows[valid], d] = a_[valid]
            c[tb[valid], rows[valid], d] = c_[valid]
            h[tb[valid], rows[valid], d] = h_[valid]
    return act, c, h


def backward(U, act, c, dout, seq_len, mutant=None, kind=None, c0=None):
    """fp64 BPTT from the stored activations and c.  Returns dG [T][Bp][D][Hp][4] (zero where a frame is not computed);
    with `kind` also the running bound of a correct kernel of that class: (dG, e_dG).  c0 [D][Bp][Hp] or None: the carried
    c the forward pass started from - at step 0 the forget gate's derivative reads it instead of 0."""
    T, Bp, D, Hp = _dims(act)
    U = np.asarray(U, dtype=np.float64)
    act = np.asarray(act, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    dout = np.asarray(dout, dtype=np.float64)
    ln = np.asarray(seq_len, dtype=np.int64)
    dG = np.zeros((T, Bp, D, Hp, 4))
    eG = np.zeros((T, Bp, D, Hp, 4))
    rows = np.arange(Bp)
    depth = kind.depth(Hp) if kind else 0
    for d in range(D):
        Ut = U[d].reshape(Hp, 4 * Hp).T          # [4Hp gate columns][Hp units]
        aUt = np.abs(Ut)
        dgn = np.zeros((Bp, 4 * Hp))
        egn = np.zeros((Bp, 4 * Hp))
        dc = np.zeros((Bp, Hp))
        edc = np.zeros((Bp, Hp))
        c0d = 0.0 if c0 is None else np.asarray(c0[d], dtype=np.float64)
        if kind and kind.name == 'wide_bwd':
            dUt = np.maximum(2.0 ** -23 * aUt, 2.0 ** -39 * aUt.max(axis=0)[None, :])
            Sb = wide_dg_scale(dout[:, :, d], ln).astype(np.float64)
        for s in range(T - 1, -1, -1):
            valid = s < ln
            tb = np.where(valid, (ln - 1 - s) if d == 1 else s, 0)
            tp = np.where(valid & (s > 0), tb + 1 if d == 1 else tb - 1, tb)
            a = act[tb, rows, d]
            cc = c[tb, rows, d]
            cpv = np.where((s > 0), c[tp, rows, d], c0d)
            do = dout[tb, rows, d]
            with np.errstate(over='ignore', invalid='ignore'):
                rec = dgn @ Ut
                dh = do + rec
                tc = cc if mutant == 'c_for_tanhc' else np.tanh(cc)
                si, tj, sf, so = (a[..., g] for g in range(4))
                A = 1 - tc * tc
                term = dh * so * A
                dct = (0.0 if mutant == 'dc_dropped' else dc) + term
                gx = dct * tj * si * (1 - si)
                gy = dct * si * (1 - tj * tj)
                gz = dct * cpv * sf * (1 - sf)
                gw = dh * tc * so * (1 - so)
                dcn = dct * sf
                if kind:
                    Sa = (np.abs(dgn) + egn) @ aUt
                    edh = (depth + 2) * U24 * (Sa + np.abs(do)) + egn @ aUt + depth * TINY
                    if kind.name == 'wide_bwd':
                        adg = np.abs(dgn) + egn
                        ddg = np.where(adg == 0, 0.0, np.maximum(2.0 ** -23 * adg, 2.0 ** -25 / Sb[:, None]))
                        edh = edh + adg @ dUt + ddg @ aUt + 2.0 ** -22 * Sa
                    eA = 2 * np.abs(tc) * TANH_ABS + TANH_ABS ** 2 + U24 * (tc * tc + np.abs(A))
                    eterm = edh * np.abs(so * A) + (np.abs(dh) + edh) * so * eA + 2 * U24 * np.abs(term)
                    edct = edc + eterm + U24 * np.abs(dct) + 4 * TINY
                    fl = 8 * TINY * np.maximum(1.0, np.abs(cpv))
                    adct = np.abs(dct) + edct
                    ex = edct * np.abs(tj * si * (1 - si)) + 4 * U24 * np.abs(gx) + fl
                    ey = edct * np.abs(si * (1 - tj * tj)) + adct * si * U24 * (tj * tj + np.abs(1 - tj * tj)) + 2 * U24 * np.abs(gy) + fl
                    ez = edct * np.abs(cpv * sf * (1 - sf)) + 4 * U24 * np.abs(gz) + fl
                    ew = edh * np.abs(tc * so * (1 - so)) + (np.abs(dh) + edh) * so * (1 - so) * TANH_ABS + 4 * U24 * np.abs(gw) + fl
                    edcn = edct * sf + U24 * np.abs(dcn) + TINY
            v = valid[:, None]
            g4 = np.where(v[..., None], np.stack([gx, gy, gz, gw], -1), 0.0)
            dgn = g4.reshape(Bp, 4 * Hp)
            dc = np.where(v, dcn, 0.0)
            dG[tb[valid], rows[valid], d] = g4[valid]
            if kind:
                e4 = np.where(v[..., None], np.stack([ex, ey, ez, ew], -1), 0.0)
                egn = e4.reshape(Bp, 4 * Hp)
                edc = np.where(v, edcn, 0.0)
                eG[tb[valid], rows[valid], d] = e4[valid]
    return (dG, eG) if kind else dG


def wide_dg_scale(dout_d, seq_len):
    """The wide BPTT's dG scale of every utterance [Bp] (float32 powers of two): largest |dOut| over the utterance's
    frames and units -> [2^5, 2^6); 1 where there is no gradient.  dout_d [T][Bp][Hp]."""
    T, Bp = dout_d.shape[:2]
    valid = np.arange(T)[:, None] < np.asarray(seq_len)[None, :]
    a = np.where(valid[:, :, None], np.abs(np.asarray(dout_d, dtype=np.float32)), np.float32(0))
    mx = a.max(axis=(0, 2))
    ok = (mx > 0) & (mx < np.float32(3e38))
    _, e = np.frexp(np.where(ok, mx, np.float32(1)))
    return np.where(ok, np.ldexp(np.float32(1), 6 - e), np.float32(1)).astype(np.float32)


# ------------------------------------------------------------------ checks
def _ratio(got, ref, bound, mask):
    """max |got - ref| / bound over mask (inf for a non-finite value); 0 for an empty mask."""
    if not mask.any():
        return 0.0
    g = np.asarray(got, dtype=np.float64)[mask]
    r, b = ref[mask], bound[mask]
    with np.errstate(invalid='ignore', divide='ignore'):
        q = np.where(np.abs(g - r) == 0, 0.0, np.abs(g - r) / b)
    q = np.where(np.isfinite(g), q, np.inf)
    return float(np.max(np.where(np.isnan(q), np.inf, q)))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_forward(kind, inp, got_act, got_c, got_h, fill_bits=None):
    """Accounts for every float of the three output buffers of a forward pass.  inp: make_inputs(case); got_*: the
    buffers [T][Bp][D][Hp](4) as float32.  Returns dict(local=, running=, running_bound=, problems=[...]): the largest
    ratios |got - ref| / bound and the violations of the output contract:
      gates  computed frames: the activations;  elsewhere: the caller's bytes, untouched
      c      computed frames: c;                elsewhere: untouched (the fill pattern)
      out    computed frames: h;                every other frame of every row b < Bp: exactly +0
      units j >= H of c and out at computed frames: exactly 0"""
    U, pre, ln, fb, H = inp['U'], inp['pre'], inp['seq_len'], inp['fb'], inp['H']
    T, Bp, D, Hp = _dims(pre)
    problems = []
    local = running = rbound = 0.0
    U64 = U.astype(np.float64)
    for d in range(D):
        valid, prev = _prev_index(T, Bp, ln, d)
        tt, bb = np.nonzero(valid)
        pt = prev[tt, bb]
        h0 = np.zeros((Bp, Hp)) if inp.get('h0') is None else inp['h0'][d].astype(np.float64)
        c0 = np.zeros((Bp, Hp)) if inp.get('c0') is None else inp['c0'][d].astype(np.float64)
        hp = np.where((pt >= 0)[:, None], got_h[np.maximum(pt, 0), bb, d].astype(np.float64), h0[bb])
        cp = np.where((pt >= 0)[:, None], got_c[np.maximum(pt, 0), bb, d].astype(np.float64), c0[bb])
        if not (np.isfinite(hp).all() and np.isfinite(cp).all()):
            problems.append(f'd{d}: non-finite state in a computed frame')
            hp, cp = np.nan_to_num(hp, posinf=0, neginf=0), np.nan_to_num(cp, posinf=0, neginf=0)
        x = pre[tt, bb, d].astype(np.float64)
        a_, c_, h_ = cell(U64[d], x, hp, cp, fb)
        ea, ec, eh = fwd_step_bound(kind, U64[d], x, hp, cp, fb)
        m = np.ones(a_.shape, dtype=bool)
        local = max(local, _ratio(got_act[tt, bb, d], a_, ea, m), _ratio(got_c[tt, bb, d], c_, ec, m[..., 0]),
                    _ratio(got_h[tt, bb, d], h_, eh, m[..., 0]))
        # ---- the output contract
        gc, gh = got_c[tt, bb, d], got_h[tt, bb, d]
        if H < Hp and (np.any(_bits(gc[:, H:]) & 0x7fffffff) or np.any(_bits(gh[:, H:]) & 0x7fffffff)):
            problems.append(f'd{d}: padded units of c / out are not 0')
        inv = ~valid
        if np.any(_bits(got_h[:, :, d][inv])):
            problems.append(f'd{d}: out is not +0 past seq_len')
        if np.any(_bits(got_act[:, :, d][inv]) != _bits(pre[:, :, d][inv])):
            problems.append(f'd{d}: gates were written at a frame that is not computed')
        if fill_bits is not None and np.any(_bits(got_c[:, :, d][inv]) != fill_bits):
            problems.append(f'd{d}: c was written at a frame that is not computed')
    # ---- running check: an independent fp64 trajectory with the bound carried along
    ra, rc, rh, Ea, Ec, Eh = forward_running(kind, inp)
    vm = (np.arange(T)[:, None] < np.asarray(ln)[None, :])[:, :, None, None] & np.ones((1, 1, D, Hp), dtype=bool)
    rbound = float(np.nan_to_num(max(Ea[vm].max(), Ec[vm].max(), Eh[vm].max()), nan=np.inf)) if vm.any() else 0.0
    if rbound <= RUNNING_LIMIT:
        running = max(_ratio(got_act, ra, Ea, vm[..., None] & np.ones(4, dtype=bool)), _ratio(got_c, rc, Ec, vm),
                      _ratio(got_h, rh, Eh, vm))
    else:
        running = None
    return dict(local=local, running=running, running_bound=rbound, problems=problems)


def forward_running(kind, inp):
    """fp64 trajectory from the inputs alone and the bound a correct kernel's trajectory stays within."""
    U, pre, ln, fb = inp['U'].astype(np.float64), inp['pre'].astype(np.float64), np.asarray(inp['seq_len'], np.int64), inp['fb']
    T, Bp, D, Hp = _dims(pre)
    act, c, h = np.zeros(pre.shape), np.zeros(pre.shape[:4]), np.zeros(pre.shape[:4])
    Ea, Ec, Eh = np.zeros(pre.shape), np.zeros(pre.shape[:4]), np.zeros(pre.shape[:4])
    rows = np.arange(Bp)
    for d in range(D):
        hs = np.zeros((Bp, Hp)) if inp.get('h0') is None else inp['h0'][d].astype(np.float64)
        cs = np.zeros((Bp, Hp)) if inp.get('c0') is None else inp['c0'][d].astype(np.float64)
        ehs, ecs = np.zeros((Bp, Hp)), np.zeros((Bp, Hp))
        for s in range(T):
            valid = s < ln
            if not valid.any():
                break
            tb = np.where(valid, (ln - 1 - s) if d == 1 else s, 0)
            x = np.where(valid[:, None, None], pre[tb, rows, d], 0.0)
            a_, c_, h_ = cell(U[d], x, hs, cs, fb)
            with np.errstate(over='ignore', invalid='ignore'):      # a bound that has left the fp64 range is inf
                ea, ec, eh = fwd_step_bound(kind, U[d], x, hs, cs, fb, np.nan_to_num(ehs, nan=np.inf), np.nan_to_num(ecs, nan=np.inf))
            v = valid[:, None]
            hs, cs, ehs, ecs = np.where(v, h_, 0.0), np.where(v, c_, 0.0), np.where(v, eh, 0.0), np.where(v, ec, 0.0)
            i = (tb[valid], rows[valid], d)
            act[i], c[i], h[i], Ea[i], Ec[i], Eh[i] = a_[valid], c_[valid], h_[valid], ea[valid], ec[valid], eh[valid]
    return act, c, h, Ea, Ec, Eh


def check_backward(kind, inp, got_dg, rowpart=None, colpart=None):
    """dG against the running bound; dG is exactly +0 at every frame that is not computed (rows b >= B included) and in
    the gate columns of padded units; rowpart / colpart, reduced over their parts, are max |dG| of the kernel's own dG."""
    U, ln, H = inp['U'], inp['seq_len'], inp['H']
    T, Bp, D, Hp = _dims(inp['act'])
    ref, e = backward(U, inp['act'], inp['c'], inp['dout'], ln, kind=kind, c0=inp.get('c0'))
    valid = (np.arange(T)[:, None] < np.asarray(ln)[None, :])
    vm = valid[:, :, None, None, None] & np.ones((1, 1, D, Hp, 4), dtype=bool)
    problems = []
    ratio = _ratio(got_dg, ref, e, vm)
    if np.any(_bits(got_dg)[~vm]):
        problems.append('dG is not +0 at a frame that is not computed')
    # padded units: dOut, U's rows and the activation tanh(j) are 0 there, so the per-step kernels compute exactly 0.  The
    # persistent kernel's partial sums carry their epoch in the last mantissa bit (a zero partial sum of an odd use is the
    # smallest subnormal 2^-149, and 32 of them make dh), so it stores +0 there instead of what it computed: the bias
    # gradient sums these columns over T * B rows, and Adam divides what is left by eps (tests/test_padding_host.py)
    pad_limit = 0.0
    if H < Hp and not np.all(np.abs(np.asarray(got_dg, dtype=np.float64)[:, :, :, H:][vm[:, :, :, H:]]) <= pad_limit):
        problems.append(f'dG of padded units exceeds {pad_limit:g}')
    if rowpart is not None:
        a = np.abs(np.asarray(got_dg, dtype=np.float32))
        rmax = a.reshape(T * Bp, D, Hp * 4).max(axis=2)                       # [R][D]
        rp = rowpart.reshape(D, 32, T * Bp).max(axis=1)                       # [D][R]
        if np.any(_bits(rp.T) != _bits(rmax)):
            problems.append('rowpart is not max |dG| per frame row')
        cmax = a.reshape(T * Bp, D * Hp * 4).max(axis=0)
        cp = colpart.reshape(8 // D, D * Hp * 4).max(axis=0)
        if np.any(_bits(cp) != _bits(cmax)):
            problems.append('colpart is not max |dG| per gate column')
    return dict(running=ratio, problems=problems)


# ------------------------------------------------------------------ fp32 emulations of the arithmetic classes
def _exp_(x):
    with np.errstate(over='ignore', under='ignore'):
        return np.exp2((x * np.float32(1.44269504088896341)).astype(np.float32)).astype(np.float32)


def sigmoid_f32(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over='ignore', divide='ignore'):
        return (np.float32(1) / (np.float32(1) + _exp_(-x))).astype(np.float32)


def tanh_f32(x):
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(over='ignore', divide='ignore'):
        return (np.float32(1) - np.float32(2) * (np.float32(1) / (np.float32(1) + _exp_(np.float32(2) * x)))).astype(np.float32)


def _chain_product(A, B, shares, group=None, block=1):
    """fp32 product A [n][K] x B [K][N] in chain order: `shares` contiguous K shares, each ONE sequential chain; then every
    `group` consecutive chains are summed one after the other, and the group sums one after the other.  block > 1: a
    link of the chain is the fp32 sum of `block` products (one MFMA of that depth)."""
    n, K = A.shape
    L = K // shares
    N = B.shape[1]
    A3 = np.ascontiguousarray(A.astype(np.float32).reshape(n, shares, L).transpose(1, 0, 2))
    B3 = B.astype(np.float32).reshape(shares, L, N)
    acc = np.zeros((shares, n, N), dtype=np.float32)
    for k in range(0, L, block):
        if block == 1:
            acc += A3[:, :, k][:, :, None] * B3[:, k, :][:, None, :]
        else:
            acc += np.matmul(A3[:, :, k:k + block], B3[:, k:k + block, :])
    group = group or shares
    part = acc.reshape(shares // group, group, n, N)
    g = part[:, 0]
    for i in range(1, group):
        g = g + part[:, i]
    tot = g[0]
    for i in range(1, g.shape[0]):
        tot = tot + g[i]
    return tot


def _rec_f32(kind, U2, hs):
    if not kind.f16:
        return _chain_product(hs, U2, 4)
    s, inv = G.scale_model(G.line_max(U2, 0))
    Us = (U2 * s[None, :]).astype(np.float32)
    u1 = Us.astype(np.float16)
    u2 = (Us - u1.astype(np.float32)).astype(np.float16)
    f = lambda x: x.astype(np.float32)
    if kind.name == 'wide_fwd':      # parts of 2 h (clamped below 2), the low one times 2^10; 8 XCD slices, MFMAs of 32 products
        v2 = (hs * np.float32(2)).astype(np.float32)
        h1 = np.clip(v2, np.float32(-1.9990234375), np.float32(1.9990234375)).astype(np.float16)
        h2 = ((v2 - f(h1)) * np.float32(1024)).astype(np.float16)
        t = _chain_product(f(h1), f(u2), 8, block=32) + _chain_product(f(h1), f(u1), 8, block=32)
        t = t + _chain_product(f(h2), f(u1), 8, block=32) * np.float32(1.0 / 1024.0)
        return (t * (inv * np.float32(0.5))[None, :]).astype(np.float32)
    v = (hs * np.float32(16384)).astype(np.float32)
    h1 = v.astype(np.float16)
    h2 = ((v - h1.astype(np.float32)) * np.float32(0.125)).astype(np.float16)
    acc = (_chain_product(f(h2), f(u1), 4) * np.float32(8) + _chain_product(f(h1), f(u2), 4)) + _chain_product(f(h1), f(u1), 4)
    return (acc * (inv * np.float32(1.0 / 16384.0))[None, :]).astype(np.float32)


def emulate_forward(kind, inp):
    """The forward pass in fp32 with the fast activations and the plane arithmetic of `kind`; buffers as the kernel
    leaves them (gates in place, c untouched = NaN here, out +0 past seq_len)."""
    U, pre, ln, fb = inp['U'], inp['pre'], np.asarray(inp['seq_len'], np.int64), np.float32(inp['fb'])
    T, Bp, D, Hp = _dims(pre)
    act = pre.copy()
    c = np.full(pre.shape[:4], np.nan, dtype=np.float32)
    h = np.zeros(pre.shape[:4], dtype=np.float32)
    rows = np.arange(Bp)
    for d in range(D):
        U2 = U[d].reshape(Hp, 4 * Hp)
        hs = np.zeros((Bp, Hp), np.float32) if inp.get('h0') is None else inp['h0'][d].astype(np.float32)
        cs = np.zeros((Bp, Hp), np.float32) if inp.get('c0') is None else inp['c0'][d].astype(np.float32)
        for s in range(T):
            valid = s < ln
            if not valid.any():
                break
            tb = np.where(valid, (ln - 1 - s) if d == 1 else s, 0)
            x = np.where(valid[:, None, None], pre[tb, rows, d], np.float32(0))
            z = (x + _rec_f32(kind, U2, hs).reshape(Bp, Hp, 4)).astype(np.float32)
            a = np.stack([sigmoid_f32(z[..., 0]), tanh_f32(z[..., 1]), sigmoid_f32(z[..., 2] + fb), sigmoid_f32(z[..., 3])], -1)
            cn = (cs * a[..., 2] + a[..., 0] * a[..., 1]).astype(np.float32)
            hn = (tanh_f32(cn) * a[..., 3]).astype(np.float32)
            v = valid[:, None]
            hs, cs = np.where(v, hn, np.float32(0)), np.where(v, cn, np.float32(0))
            i = (tb[valid], rows[valid], d)
            act[i], c[i], h[i] = a[valid], cn[valid], hn[valid]
    return act, c, h


def emulate_backward(kind, inp):
    U, ln = inp['U'], np.asarray(inp['seq_len'], np.int64)
    act, c, dout, c0 = inp['act'], inp['c'], inp['dout'], inp.get('c0')
    T, Bp, D, Hp = _dims(act)
    dG = np.zeros(act.shape, dtype=np.float32)
    rows = np.arange(Bp)
    one = np.float32(1)
    # the chains of one output, as an order of the gate columns 4j + g and a chain length:
    #   step_bwd        wave g of block ks contracts gate g of units [32 ks, 32 ks + 32): 4 Hp/32 chains of 32
    #   its wide form   a block walks 4 K slices with its accumulators kept: chains of 128
    #   persist_bwd     producer m contracts the 4 NU columns of its NU = Hp/32 units in 4 chains (column % 4)
    #   wide_bwd        member nb contracts the columns of units 256 kt + 8 nb + i (kt, i < 8): 32 chains of 256, MFMAs of 32
    L = 32 if kind.name == 'step_bwd' else Hp // 32
    if kind.name == 'step_bwd' and Hp > 512 and Hp % 128 == 0:
        L = 128
    blk, g4i, ju = np.meshgrid(np.arange(Hp // L), np.arange(4), np.arange(L), indexing='ij')
    order = (4 * (L * blk + ju) + g4i).reshape(-1)
    shares = 4 * Hp // L
    wide = kind.name == 'wide_bwd'
    if wide:
        nb, kt, i8, g4i = np.meshgrid(np.arange(32), np.arange(8), np.arange(8), np.arange(4), indexing='ij')
        order = (4 * (256 * kt + 8 * nb + i8) + g4i).reshape(-1)
        shares = 32
    f = lambda x: x.astype(np.float32)
    for d in range(D):
        Ut = np.ascontiguousarray(U[d].reshape(Hp, 4 * Hp).T)
        if wide:
            rs, rinv = G.scale_model(G.line_max(Ut, 0))
            Us = (Ut * rs[None, :]).astype(np.float32)
            u1 = Us.astype(np.float16)
            u2 = (Us - f(u1)).astype(np.float16)
            Sb = wide_dg_scale(dout[:, :, d], ln)
        dgn = np.zeros((Bp, 4 * Hp), np.float32)
        dc = np.zeros((Bp, Hp), np.float32)
        for s in range(T - 1, -1, -1):
            valid = s < ln
            tb = np.where(valid, (ln - 1 - s) if d == 1 else s, 0)
            tp = np.where(valid & (s > 0), tb + 1 if d == 1 else tb - 1, tb)
            a, cc, do = act[tb, rows, d], c[tb, rows, d], dout[tb, rows, d]
            cpv = c[tp, rows, d] if s > 0 else c0[d] if c0 is not None else np.zeros((Bp, Hp), np.float32)
            with np.errstate(over='ignore', invalid='ignore'):
                if wide:
                    sv = (dgn * Sb[:, None]).astype(np.float32)
                    p1 = sv.astype(np.float16)
                    p2 = (sv - f(p1)).astype(np.float16)
                    rec = (_chain_product(f(p2)[:, order], f(u1)[order], 32, block=32) +
                           _chain_product(f(p1)[:, order], f(u2)[order], 32, block=32) +
                           _chain_product(f(p1)[:, order], f(u1)[order], 32, block=32))
                    rec = (rec * ((np.float32(1) / Sb)[:, None] * rinv[None, :])).astype(np.float32)
                else:
                    rec = _chain_product(dgn[:, order], Ut[order], shares, 4)
                dh = (do + rec).astype(np.float32)
                tc = tanh_f32(cc)
                si, tj, sf, so = (a[..., g] for g in range(4))
                dct = (dc + dh * so * (one - tc * tc)).astype(np.float32)
                g4 = np.stack([dct * tj * si * (one - si), dct * si * (one - tj * tj), dct * cpv * sf * (one - sf),
                               dh * tc * so * (one - so)], -1).astype(np.float32)
                dcn = (dct * sf).astype(np.float32)
            v = valid[:, None]
            g4 = np.where(v[..., None], g4, np.float32(0))
            dgn = g4.reshape(Bp, 4 * Hp)
            dc = np.where(v, dcn, np.float32(0))
            dG[tb[valid], rows[valid], d] = g4[valid]
    return dG


# ------------------------------------------------------------------ the cases
@dataclass(frozen=True)
class Case:
    path: str          # key of KINDS
    Hp: int
    H: int
    B: int
    D: int
    T: int
    lens: str          # 'full', 'ragged' (one row of length 1, one of length T), 'short' (the shortest far below T),
                       # 'ragged0' (ragged, and row 1 has length 0: a stream slot without frames, validate_chunk admits it)
    regime: str        # 'init', 'sat', 'long', 'tiny', 'colrange', 'aligned' (make_inputs)
    lean: bool = False
    parts: bool = False
    seed: int = 0
    carry: bool = False    # step_bwd: step 0 in its carry form, from a carried c0 (a window of chunked training)

    @property
    def id(self):
        return (f'{self.path}-Hp{self.Hp}-H{self.H}-B{self.B}-D{self.D}-T{self.T}-{self.lens}-{self.regime}' +
                ('-lean' if self.lean else '') + ('-parts' if self.parts else '') + ('-carry' if self.carry else ''))


def cases():
    C = Case
    out = [
        # per-step forward: every NQ instantiation (Hp/64 = 1, 2, 4, 8, 16) and the generic form (Hp 576, 640)
        C('step_fwd', 64, 50, 5, 2, 12, 'ragged', 'init'), C('step_fwd', 128, 128, 17, 1, 7, 'full', 'sat'),
        C('step_fwd', 256, 250, 16, 2, 5, 'short', 'colrange'), C('step_fwd', 512, 500, 64, 2, 3, 'ragged', 'tiny'),
        C('step_fwd', 1024, 1000, 1, 1, 3, 'full', 'init'), C('step_fwd', 576, 570, 1, 2, 4, 'ragged', 'init'),
        C('step_fwd', 640, 640, 33, 2, 4, 'short', 'sat'), C('step_fwd', 64, 50, 5, 2, 300, 'ragged', 'long'),
        C('step_carry', 64, 50, 5, 1, 6, 'ragged0', 'init'), C('step_carry', 128, 100, 17, 2, 4, 'short', 'sat'),
        C('step_carry', 64, 50, 5, 1, 300, 'ragged', 'long'),
        # a row b < B of length 0 on the batch paths too: the kernels treat it like a padded row
        C('step_fwd', 64, 50, 5, 2, 6, 'ragged0', 'init'), C('persist_fwd16', 64, 50, 5, 2, 6, 'ragged0', 'init'),
        C('step_bwd', 64, 50, 5, 2, 6, 'ragged0', 'init'), C('persist_bwd', 64, 50, 5, 2, 6, 'ragged0', 'init', parts=True),
        # per-step BPTT: KSP = Hp/32 = 2, 4, 8, 16, the generic form (576) and the two-launch form (640, 1024)
        C('step_bwd', 64, 50, 5, 2, 12, 'ragged', 'init'), C('step_bwd', 128, 128, 17, 1, 7, 'full', 'sat'),
        C('step_bwd', 256, 250, 16, 2, 5, 'short', 'init'), C('step_bwd', 512, 500, 64, 2, 3, 'ragged', 'init'),
        C('step_bwd', 576, 570, 1, 2, 5, 'ragged', 'init'), C('step_bwd', 640, 600, 33, 2, 4, 'short', 'sat'),
        C('step_bwd', 1024, 1000, 1, 1, 3, 'full', 'init'), C('step_bwd', 64, 50, 5, 2, 300, 'ragged', 'long'),
        # ... with step 0 in its carry form: the one-launch kernel's CARRY instantiation, and lstm_bwd_cell_carry_kernel
        C('step_bwd', 64, 50, 5, 2, 3, 'ragged', 'init', carry=True), C('step_bwd', 640, 600, 5, 1, 2, 'ragged', 'init', carry=True),
    ]
    # the persistent kernels: every NU = Hp/32 of the launcher's dispatch (2, 4, ..., 16)
    Bs = [5, 17, 1, 33, 16, 64, 5, 17]
    regs = ['init', 'sat', 'tiny', 'colrange', 'init', 'sat', 'colrange', 'init']
    lens = ['ragged', 'short', 'full', 'ragged', 'short', 'ragged', 'full', 'ragged']
    for i, Hp in enumerate(range(64, 513, 64)):
        H = Hp if i % 3 == 1 else Hp - 14
        T = 12 if Hp <= 128 else (6 if Hp <= 256 else 4)
        D = 2 - (i % 2)
        for p in ('persist_fwd32', 'persist_fwd16'):
            out.append(C(p, Hp, H, Bs[i], D, T, lens[i], regs[i]))
        out.append(C('persist_bwd', Hp, H, Bs[i], D, T, lens[i], 'sat' if regs[i] == 'sat' else 'init', parts=i % 2 == 0))
    # the wide kernel: Hp = 2048 only, one launch per direction, MT = Bp/16 = 1 and 2
    out += [C('wide_fwd', 2048, 2000, 5, 2, 3, 'ragged', 'init'), C('wide_fwd', 2048, 2048, 17, 1, 4, 'short', 'tiny'),
            C('wide_fwd', 2048, 2000, 16, 1, 2, 'ragged', 'sat'), C('wide_fwd', 2048, 2000, 5, 1, 3, 'ragged0', 'colrange'),
            # every h of step 0 a quarter of an fp16 step above a power of two: the h2 U1 products all have one sign
            C('wide_fwd', 2048, 2048, 1, 1, 2, 'full', 'aligned'),
            C('wide_bwd', 2048, 2000, 5, 2, 3, 'ragged', 'init'), C('wide_bwd', 2048, 2048, 17, 1, 4, 'short', 'sat')]
    # several rounds over the batch with an ODD T: use_epoch's uses of a buffer per round differ between the two buffers,
    # and the round barrier (the flag words, tagbase = round * T) is crossed twice
    out += [C(p, 64, 50, 33, 2, 5, 'ragged', 'init', parts=p == 'persist_bwd') for p in ('persist_fwd32', 'persist_fwd16', 'persist_bwd')]
    out += [C('persist_fwd32', 64, 50, 5, 2, 300, 'ragged', 'long'), C('persist_fwd16', 64, 50, 5, 2, 300, 'ragged', 'long'),
            C('persist_fwd16', 64, 50, 5, 1, 300, 'ragged', 'tiny'),
            C('persist_bwd', 64, 50, 5, 2, 300, 'ragged', 'long', parts=True),
            C('persist_bwd', 512, 500, 33, 2, 4, 'ragged', 'init', lean=True, parts=True),
            C('persist_bwd', 512, 512, 17, 1, 3, 'full', 'sat', lean=True)]
    return out


PLANTED = [30.0, -30.0, 88.0, -88.0, 89.0, -89.0, 200.0, -200.0, 1e4, -1e4]


def _seq_len(case, rng):
    B, T, Bp = case.B, case.T, rup(case.B, 16)
    ln = np.zeros(Bp, dtype=np.int32)
    if case.lens == 'full':
        ln[:B] = T
    elif case.lens in ('ragged', 'ragged0'):
        ln[:B] = rng.integers(1, T + 1, size=B)
        ln[0] = T
        if B > 1:
            ln[B - 1] = 1
        if case.lens == 'ragged0':
            ln[1] = 0
    else:
        ln[:B] = rng.integers(1, max(2, T // 3) + 1, size=B)
        ln[B // 2] = T
    return ln


@lru_cache(maxsize=4)
def make_inputs(case):
    """The buffers of a case (read-only: shared between tests).  Forward paths: U, pre (poisoned where no frame is
    computed), seq_len, fb, h0 / c0 (carry).  BPTT paths: U, act / c (the fp64 forward pass of an init-like or saturated
    input, rounded to fp32 - independent of the forward kernels; from c0 when the case carries), dout, all poisoned the
    same way."""
    seed = zlib.crc32(case.id.encode()) + case.seed
    rng = np.random.default_rng(seed)
    Hp, H, B, D, T = case.Hp, case.H, case.B, case.D, case.T
    Bp = rup(B, 16)
    ln = _seq_len(case, rng)
    reg = case.regime
    U = np.zeros((D, Hp, Hp, 4), dtype=np.float32)
    a = 40.0 / H if reg == 'long' else 1.0 / np.sqrt(H)       # long: sum_k |U_k,col| ~ 20
    U[:, :H, :H] = rng.uniform(-a, a, size=(D, H, H, 4))
    if reg == 'colrange':
        U[:, :H, 1, 0] *= 2.0 ** 10
        U[:, :H, 2, 1] = 0
        U[:, :H, 3, 2] = np.where(U[:, :H, 3, 2] > 0, 1e-20, -1e-20)
    pre = np.zeros((T, Bp, D, Hp, 4), dtype=np.float32)
    x = rng.standard_normal((T, Bp, D, H, 4))
    if reg == 'sat':
        x *= 8
        flat = x.reshape(-1, 4)
        for g in range(4):
            idx = rng.choice(flat.shape[0], size=len(PLANTED), replace=False)
            flat[idx, g] = PLANTED
        # ... and in frames that are certainly computed: frame 0 of row 0
        for k, v in enumerate(PLANTED):
            x[0, 0, :, k % H, :] = v
    elif reg == 'long':
        x = x * 0.5 + np.array([6.0, 3.0, 6.0, 0.0])
    elif reg == 'tiny':
        x[..., 3] = -25 + 0.5 * x[..., 3]
    elif reg == 'aligned':
        # U >= 0; step 0: i and j saturated (c = 1), o such that every h = 0.25 (1 + 2^-12): 2 h (and h 2^14) lies a quarter
        # of an fp16 step above a power of two, so the low part of every h is + 2^-12 h and the h2 U1 products add up;
        # step 1: the input half cancels the recurrent one, so that the gates sit where their derivatives are large
        U[:, :H, :H] = np.abs(U[:, :H, :H])
        h0 = 0.25 * (1 + 2.0 ** -12)
        so = h0 / np.tanh(_sig(30.0) * np.tanh(30.0))
        x[0] = np.array([30.0, 30.0, 0.0, np.log(so / (1 - so))])
        x[1:] = x[1:] - h0 * U[:, :H, :H].astype(np.float64).sum(axis=1)[None, None]
    pre[:, :, :, :H] = x
    valid = np.arange(T)[:, None] < ln[None, :]
    out = dict(U=U, seq_len=ln, fb=1.0, H=H, B=B, Bp=Bp, valid=valid)
    fb = out['fb']
    if case.path == 'step_carry':
        st = rng.uniform(-1, 1, size=(D, B, 2, H)).astype(np.float32)
        st[:, :, 0] *= 3
        out['state'] = st
        out['c0'] = np.zeros((D, Bp, Hp), dtype=np.float32)
        out['h0'] = np.zeros((D, Bp, Hp), dtype=np.float32)
        out['c0'][:, :B, :H], out['h0'][:, :B, :H] = st[:, :, 0], st[:, :, 1]
    if case.carry:            # the carried c of a window's BPTT, poisoned as everything else in the rows b >= B
        c0 = np.full((D, Bp, Hp), POISON, dtype=np.float32)
        c0[:, :B] = 0
        c0[:, :B, :H] = rng.uniform(-3, 3, size=(D, B, H))
        out['c0'] = c0
    if KINDS[case.path].bwd:
        act, c, _ = forward(U, pre, ln, fb, None, out.get('c0'))
        act, c = act.astype(np.float32), c.astype(np.float32)
        # dOut ~ N(0,1) x a per-frame factor spanning 2^-20 .. 1 inside an utterance and 2^-20 .. 2^10 between utterances
        dout = np.zeros((T, Bp, D, Hp), dtype=np.float32)
        ft = 2.0 ** -(20.0 * ((np.arange(T) * 7) % max(T, 2)) / max(T - 1, 1))
        fbm = 2.0 ** (-20.0 + 30.0 * ((np.arange(Bp) * 5) % max(B, 2)) / max(B - 1, 1))
        dout[:, :, :, :H] = rng.standard_normal((T, Bp, D, H)) * ft[:, None, None, None] * fbm[None, :, None, None]
        act[~valid], c[~valid], dout[~valid] = POISON, POISON, POISON
        out.update(act=act, c=c, dout=dout)
    pre[~valid] = POISON
    out['pre'] = pre
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out
