"""ctypes side of tests/kernel_harness/harness.hip, rec_harness.hip and ctc_harness.hip (neuralasr_amd/libnasr_kt.so, built by
neuralasr_amd/build.py): the GEMM-layer, recurrence and CTC launchers of csrc/kernels.h, callable with NumPy arrays.  Every call raises on a HIP error or a refused
argument; outputs come back as fresh arrays whose untouched bytes still hold FILL."""
import ctypes
import os
from ctypes import POINTER, Structure, c_double, c_float, c_int, c_longlong, c_ubyte, c_ulonglong, c_void_p

import numpy as np

import gemm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KT_PATH = os.path.join(ROOT, 'neuralasr_amd', 'libnasr_kt.so')
SYMBOLS = ['kt_gemm_pick_split', 'kt_gemm_tp_tile_rows', 'kt_gemm_tph_pick_split', 'kt_tp_split2_parts', 'kt_tph_bytes',
           'kt_gemm_f32', 'kt_tph_scales', 'kt_tph_scales_batch', 'kt_tph_scales_from_parts', 'kt_tph_split2', 'kt_gemm_tph',
           'kt_colsum', 'kt_colsum_parts', 'kt_reduce_slabs', 'kt_reduce_slabs_rows',
           'kt_persist_dgmax_floats', 'kt_lstm_step_fwd', 'kt_lstm_step_bwd', 'kt_lstm_step_bwd_carry',
           'kt_lstm_persist_fwd', 'kt_lstm_persist_bwd', 'kt_lstm_wide_fwd', 'kt_lstm_wide_bwd',
           'kt_ctc_pass', 'kt_ctc_greedy', 'kt_mean']

FILL = 0xCD                                   # pre-fill byte of every output buffer
FILL_F32 = np.frombuffer(bytes([FILL] * 4), dtype=np.float32)[0]


class KtGemm(Structure):
    _fields_ = [(n, c_int) for n in ('M', 'N', 'K', 'lda', 'ldb', 'ldc', 'a_col', 'b_col', 'a_shift', 'a_rows', 'split_k')]


class KtScaleJob(Structure):
    _fields_ = [('src', c_void_p), ('src_floats', c_longlong), ('rows', c_int), ('K', c_int), ('ld', c_int), ('pad', c_int),
                ('row_scale', c_void_p), ('row_inv', c_void_p), ('col_scale', c_void_p), ('col_inv', c_void_p)]


class KtTph(Structure):
    _fields_ = ([(n, c_int) for n in ('M', 'N', 'K', 'KA', 'KB', 'ldc', 'a_kshift', 'a_kshift1', 'split_k', 'tile_rows',
                                      'nbatch', 'side')] +
                [(n, c_longlong) for n in ('a_bstride', 'b_bstride', 'c_bstride', 'ainv_bstride', 'binv_bstride')] +
                [('a_rows', c_int), ('b_rows', c_int)])


class KtRec(Structure):
    _fields_ = ([(n, c_int) for n in ('T', 'B', 'Bp', 'H', 'Hp', 'D')] + [('forget_bias', c_float)] +
                [(n, c_int) for n in ('f16', 'lean', 'parts', 'fill')])


class KtCtc(Structure):
    _fields_ = ([(n, c_int) for n in ('Tp', 'B', 'Bp', 'C', 'Cp', 'Lmax')] + [('scale', c_float)] +
                [(n, c_int) for n in ('plain', 'ws_fill', 'fill')])


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(KT_PATH):
            raise ImportError(f'{KT_PATH} is missing: run `python -m neuralasr_amd.build`')
        _lib = ctypes.CDLL(KT_PATH)
        _lib.kt_tph_bytes.restype = c_ulonglong
        _lib.kt_persist_dgmax_floats.restype = c_ulonglong
    return _lib


def _f(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_float))


def _i(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_int))


def _b(a):
    return None if a is None else a.ctypes.data_as(POINTER(c_ubyte))


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def _i32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.int32)


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f'{what}: ' + ('arguments refused by the harness' if rc == -1 else f'HIP error {rc}'))


def _out(n):
    return np.zeros(n, dtype=np.float32)


def gemm_f32(c):
    """Runs a gemm_ref.GemmCase; returns the whole C buffer [c_rows][ldc]."""
    A, B = _f32(c.A), _f32(c.B)
    d = KtGemm(c.M, c.N, c.K, A.shape[1], B.shape[1], c.ldc, int(c.a_col), int(c.b_col), c.a_shift, c.a_rows, c.split_k)
    C = _out(c.c_rows * c.ldc)
    a_map, c_map, bias = _i32(c.a_map), _i32(c.c_map), _f32(c.bias)
    rc = lib().kt_gemm_f32(ctypes.byref(d), _f(A), c_longlong(A.size), _f(B), c_longlong(B.size), _f(C), c_longlong(C.size),
                           _i(a_map), 0 if a_map is None else a_map.size, _i(c_map), _f(bias), FILL)
    _check(rc, 'kt_gemm_f32')
    return C.reshape(c.c_rows, c.ldc)


def tph_planes(c, poison=False, gap=(0, 0, 0, 0, 0)):
    """Planes, inverse scales and strides of a gemm_ref.TphCase, built with the Python encoder and scale model.  poison: NaN
    in the plane rows [M, rup32(M)) / [N, rup32(N)) (needs operands of exactly M / N rows).  gap: extra (A row blocks, B row
    blocks, C floats, a_inv floats, b_inv floats) between the two batches, so that all five strides differ."""
    nb = 2 if c.nbatch > 1 else 1
    planes, invs = [[], []], [[], []]
    for o, mats in enumerate((c.A, c.B)):
        for b in range(nb):
            x = np.asarray(mats[b], dtype=np.float32)
            s, inv = R.scale_model(R.line_max(x, 1))
            h1, h2 = R.split_parts(x * s[:, None])
            if poison:
                pad = (-x.shape[0]) % 32
                h1 = np.vstack([h1, np.full((pad, x.shape[1]), np.nan, np.float16)])
                h2 = np.vstack([h2, np.full((pad, x.shape[1]), np.nan, np.float16)])
            planes[o].append(R.tph_encode_parts(h1, h2))
            invs[o].append(inv)
    out = {}
    for o, key in enumerate('ab'):
        nkb = (np.asarray((c.A, c.B)[o][0]).shape[1] + 15) // 16
        stride = planes[o][0].size + gap[o] * nkb * 2048
        buf = np.full(stride * (nb - 1) + planes[o][nb - 1].size, 0xFF, dtype=np.uint8)      # the gap: NaN halves
        istride = invs[o][0].size + gap[3 + o]
        ibuf = np.full(istride * (nb - 1) + invs[o][nb - 1].size, np.nan, dtype=np.float32)
        for b in range(nb):
            buf[b * stride:b * stride + planes[o][b].size] = planes[o][b]
            ibuf[b * istride:b * istride + invs[o][b].size] = invs[o][b]
        out[key] = (buf, stride, ibuf, istride)
    out['c_bstride'] = c.c_rows * c.ldc + gap[2]
    return out


def gemm_tph(c, planes=None, fp32=False):
    """Runs a gemm_ref.TphCase: from planes (tph_planes(c) unless given) or, fp32=True, from the fp32 operands through
    launch_tph_scales + launch_tph_split2.  Returns the C buffer(s) [nbatch][c_rows][ldc] (nbatch == 2 with split_k > 1:
    c_bstride = M * N as GemmTPHDesc demands)."""
    nb = 2 if c.nbatch > 1 else 1
    KA, KB = np.asarray(c.A[0]).shape[1], np.asarray(c.B[0]).shape[1]
    d = KtTph(M=c.M, N=c.N, K=c.K, KA=KA, KB=KB, ldc=c.ldc, a_kshift=c.a_kshift, a_kshift1=c.a_kshift1, split_k=c.split_k,
              tile_rows=c.tile_rows, nbatch=c.nbatch, side=int(c.side))
    bias, c_map = _f32(c.bias), _i32(c.c_map)
    if fp32:
        assert nb == 1
        A, B = _f32(c.A[0]), _f32(c.B[0])
        d.a_rows, d.b_rows = A.shape[0], B.shape[0]
        c_bstride = c.c_rows * c.ldc
        C = _out(c_bstride)
        rc = lib().kt_gemm_tph(ctypes.byref(d), _f(A), _f(B), None, c_longlong(0), None, c_longlong(0), None, None, _f(C),
                               c_longlong(C.size), _f(bias), _i(c_map), FILL)
    else:
        p = planes or tph_planes(c)
        (ab, d.a_bstride, ai, d.ainv_bstride), (bb, d.b_bstride, bi, d.binv_bstride) = p['a'], p['b']
        c_bstride = d.c_bstride = p['c_bstride']
        d.a_rows, d.b_rows = ai.size, bi.size
        C = _out(c_bstride * (nb - 1) + c.c_rows * c.ldc)
        rc = lib().kt_gemm_tph(ctypes.byref(d), None, None, _b(ab), c_longlong(ab.size), _b(bb), c_longlong(bb.size), _f(ai),
                               _f(bi), _f(C), c_longlong(C.size), _f(bias), _i(c_map), FILL)
    _check(rc, 'kt_gemm_tph')
    return C, c_bstride


def tph_scales(src, rows, K, want_rows=True, want_cols=True):
    src = _f32(src)
    rs, ri, cs, ci = (_out(rows) if want_rows else None, _out(rows) if want_rows else None,
                      _out(K) if want_cols else None, _out(K) if want_cols else None)
    rc = lib().kt_tph_scales(_f(src), c_longlong(src.size), rows, K, src.shape[1], _f(rs), _f(ri), _f(cs), _f(ci), FILL)
    _check(rc, 'kt_tph_scales')
    return rs, ri, cs, ci


def tph_scales_batch(jobs):
    """jobs: [(src 2-D, rows, K, want_rows)] -> [(rs, ri, cs, ci)]"""
    arr = (KtScaleJob * len(jobs))()
    keep, outs = [], []
    for j, (src, rows, K, want_rows) in enumerate(jobs):
        src = _f32(src)
        o = (_out(rows) if want_rows else None, _out(rows) if want_rows else None, _out(K), _out(K))
        keep.append(src)
        outs.append(o)
        arr[j] = KtScaleJob(src.ctypes.data, src.size, rows, K, src.shape[1], 0, *[None if a is None else a.ctypes.data for a in o])
    _check(lib().kt_tph_scales_batch(arr, len(jobs), FILL), 'kt_tph_scales_batch')
    return outs


def tph_scales_from_parts(rowpart, colpart):
    rowpart, colpart = _f32(rowpart), _f32(colpart)
    nrp, rows = rowpart.shape if rowpart is not None else (0, 0)
    ncp, K = colpart.shape if colpart is not None else (0, 0)
    rs, ri, cs, ci = (_out(rows) if rows else None, _out(rows) if rows else None, _out(K) if K else None, _out(K) if K else None)
    rc = lib().kt_tph_scales_from_parts(_f(rowpart), nrp, rows, _f(rs), _f(ri), _f(colpart), ncp, K, _f(cs), _f(ci), FILL)
    _check(rc, 'kt_tph_scales_from_parts')
    return rs, ri, cs, ci


def tph_split2(src, rows, K, row_scale=None, rs=1.0, col_scale=None, cs=1.0, rowmap=None, rowmap2=None, col2=0):
    """-> (tpN bytes, tpT bytes, colpart [parts][K])"""
    src = _f32(src)
    tpN = np.zeros(R.tph_bytes(rows, K), dtype=np.uint8)
    tpT = np.zeros(R.tph_bytes(K, rows), dtype=np.uint8)
    parts = lib().kt_tp_split2_parts(rows)
    colpart = _out(parts * K)
    row_scale, col_scale, rowmap, rowmap2 = _f32(row_scale), _f32(col_scale), _i32(rowmap), _i32(rowmap2)
    rc = lib().kt_tph_split2(_f(src), src.shape[0], rows, K, src.shape[1], _f(row_scale), c_float(rs), _f(col_scale), c_float(cs),
                             _b(tpN), _b(tpT), _f(colpart), _i(rowmap), _i(rowmap2), col2, FILL)
    _check(rc, 'kt_tph_split2')
    return tpN, tpT, colpart.reshape(parts, K)


def colsum(M, R_, N, pad=4):
    M = _f32(M)
    out = _out(N + pad)
    _check(lib().kt_colsum(_f(M), R_, N, M.shape[1], _f(out), out.size, FILL), 'kt_colsum')
    return out


def colsum_parts(part, N, pad=4):
    part = _f32(part)
    out = _out(N + pad)
    _check(lib().kt_colsum_parts(_f(part), part.shape[0], N, _f(out), out.size, FILL), 'kt_colsum_parts')
    return out


def reduce_slabs(slabs, pad=4):
    slabs = _f32(slabs)
    S, n = slabs.shape[0], slabs[0].size
    out = _out(n + pad)
    _check(lib().kt_reduce_slabs(_f(slabs), S, c_longlong(n), _f(out), c_longlong(out.size), FILL), 'kt_reduce_slabs')
    return out


def reduce_slabs_rows(slabs, ldc, rowmap, out_rows):
    slabs, rowmap = _f32(slabs), _i32(rowmap)
    S, M, N = slabs.shape
    out = _out(out_rows * ldc)
    rc = lib().kt_reduce_slabs_rows(_f(slabs), S, M, N, ldc, _i(rowmap), _f(out), c_longlong(out.size), FILL)
    _check(rc, 'kt_reduce_slabs_rows')
    return out.reshape(out_rows, ldc)


# ------------------------------------------------------------------ the recurrence (rec_harness.hip)
class RecurrenceAbort(RuntimeError):
    """A resident kernel reported through XcdCtl::error, the sticky word or the fault float."""


def _rec_desc(inp, pre, **kw):
    T, Bp, D, Hp = pre.shape[:4]
    return KtRec(T=T, B=inp['B'], Bp=Bp, H=inp['H'], Hp=Hp, D=D, forget_bias=inp['fb'], fill=FILL, **kw)


def _rec_status(status, what):
    if status.any():
        raise RecurrenceAbort(f'{what}: error word {status[0]:#x}, sticky word {status[1]:#x}, fault {status[2]}')


def lstm_forward(path, inp):
    """Runs a forward path of rec_ref.KINDS on rec_ref.make_inputs buffers -> (gates, c, out), frame-indexed
    [T][Bp][D][Hp](4) float32; gates = the caller's pre-activations with the activations written over them."""
    pre = inp['pre']
    T, Bp, D, Hp = pre.shape[:4]
    U = _f32(inp['U'])
    g = np.array(pre, dtype=np.float32, order='C')
    c, o = _out(T * Bp * D * Hp), _out(T * Bp * D * Hp)
    sq = _i32(inp['seq_len'])
    if path in ('step_fwd', 'step_carry'):
        d = _rec_desc(inp, pre)
        st = _f32(inp['state']) if path == 'step_carry' else None
        _check(lib().kt_lstm_step_fwd(ctypes.byref(d), _f(U), _f(g), _f(c), _f(o), _i(sq), _f(st)), 'kt_lstm_step_fwd')
    else:
        d = _rec_desc(inp, pre, f16=int(path == 'persist_fwd16'))
        status = np.full(3, 0xFFFFFFFF, dtype=np.uint32)
        name = 'kt_lstm_wide_fwd' if path == 'wide_fwd' else 'kt_lstm_persist_fwd'
        rc = getattr(lib(), name)(ctypes.byref(d), _f(U), _f(g), _f(c), _f(o), _i(sq), status.ctypes.data_as(c_void_p))
        _check(rc, name)
        _rec_status(status, name)
    return g, c.reshape(T, Bp, D, Hp), o.reshape(T, Bp, D, Hp)


def lstm_backward(path, inp, lean=False, parts=False):
    """Runs a BPTT path -> (dG [T][Bp][D][Hp][4], rowpart [D*32][T*Bp] or None, colpart [8/D][D*4Hp] or None).
    'step_bwd' with inp['c0'] [D][Bp][Hp]: step 0 in its carry form."""
    act = inp['act']
    T, Bp, D, Hp = act.shape[:4]
    U, a, c, do = _f32(inp['U']), _f32(act), _f32(inp['c']), _f32(inp['dout'])
    dg = _out(act.size)
    sq = _i32(inp['seq_len'])
    rp = cp = None
    if path == 'step_bwd':
        d = _rec_desc(inp, act)
        if inp.get('c0') is None:
            _check(lib().kt_lstm_step_bwd(ctypes.byref(d), _f(U), _f(a), _f(c), _f(do), _f(dg), _i(sq)), 'kt_lstm_step_bwd')
        else:
            rc = lib().kt_lstm_step_bwd_carry(ctypes.byref(d), _f(U), _f(a), _f(c), _f(do), _f(dg), _i(sq), _f(_f32(inp['c0'])))
            _check(rc, 'kt_lstm_step_bwd_carry')
    elif path == 'wide_bwd':
        d = _rec_desc(inp, act)
        status = np.full(3, 0xFFFFFFFF, dtype=np.uint32)
        rc = lib().kt_lstm_wide_bwd(ctypes.byref(d), _f(U), _f(a), _f(c), _f(do), _f(dg), _i(sq), status.ctypes.data_as(c_void_p))
        _check(rc, 'kt_lstm_wide_bwd')
        _rec_status(status, 'kt_lstm_wide_bwd')
    else:
        d = _rec_desc(inp, act, lean=int(lean), parts=int(parts))
        if parts:
            rp, cp = _out(D * 32 * T * Bp), _out((8 // D) * D * 4 * Hp)
            assert rp.size + cp.size == lib().kt_persist_dgmax_floats(T, Bp, Hp, D), 'rowpart / colpart are not what the library allocates'
        status = np.full(3, 0xFFFFFFFF, dtype=np.uint32)
        rc = lib().kt_lstm_persist_bwd(ctypes.byref(d), _f(U), _f(a), _f(c), _f(do), _f(dg), _f(rp), _f(cp), _i(sq),
                                       status.ctypes.data_as(c_void_p))
        _check(rc, 'kt_lstm_persist_bwd')
        _rec_status(status, 'kt_lstm_persist_bwd')
        if parts:
            rp, cp = rp.reshape(D * 32, T * Bp), cp.reshape(8 // D, D * 4 * Hp)
    return dg.reshape(act.shape), rp, cp


# ------------------------------------------------------------------ the CTC kernels (ctc_harness.hip)
FILL_I32 = np.frombuffer(bytes([FILL] * 4), dtype=np.int32)[0]
FILL_F64 = np.frombuffer(bytes([FILL] * 8), dtype=np.float64)[0]


def rup(x, m):
    return (x + m - 1) // m * m


def ctc_desc(Tp, B, C, Lmax, scale=1.0, plain=False, ws_fill=0xFF, **over):
    """The launch's shape with the padded sizes the library derives (over: fields set to something else, for the refusals)."""
    d = dict(Tp=Tp, B=B, Bp=rup(B, 16), C=C, Cp=rup(C, 32), Lmax=Lmax, scale=scale, plain=int(plain), ws_fill=ws_fill, fill=FILL)
    d.update(over)
    return KtCtc(**d)


def ctc_pass_raw(d, logits, seq_len, labels, label_len):
    """kt_ctc_pass on buffers taken as they are -> (rc, gradient, logz, nll, logp); the outputs hold FILL (the gradient: the
    caller's logits) where nothing was written - all of them after a refusal."""
    g = np.array(logits, dtype=np.float32, order='C')
    sq, lab, ll = _i32(seq_len), _i32(labels), _i32(label_len)
    logz = np.full(min(max(d.Tp, 1) * max(d.Bp, 1), 1 << 22), FILL_F32, np.float32)
    nll, logp = np.full(64, FILL_F32, np.float32), np.full(64, FILL_F64, np.float64)
    rc = lib().kt_ctc_pass(ctypes.byref(d), _f(g), _i(sq), _i(lab), _i(ll), _f(logz), _f(nll), logp.ctypes.data_as(POINTER(c_double)))
    return rc, g, logz, nll, logp


def ctc_pass(logits, seq_len, labels, label_len, C, scale=1.0, plain=False, ws_fill=0xFF):
    """logZ, alpha / beta and the gradient over logits [Tp][Bp][Cp] (seq_len [Bp], labels [B][Lmax], label_len [B]) ->
    dict(grad [Tp][Bp][Cp], logz [Tp][Bp], nll [Bp], logp [Bp]); the entries of nll / logp from B on hold FILL."""
    Tp, Bp, Cp = logits.shape
    B, Lmax = np.shape(labels)
    d = ctc_desc(Tp, B, C, Lmax, scale, plain, ws_fill)
    assert (d.Bp, d.Cp) == (Bp, Cp) and len(seq_len) == Bp and len(label_len) == B
    rc, g, logz, nll, logp = ctc_pass_raw(d, logits, seq_len, labels, label_len)
    _check(rc, 'kt_ctc_pass')
    return dict(grad=g, logz=logz.reshape(Tp, Bp), nll=nll[:Bp], logp=logp[:Bp])


def ctc_greedy_raw(d, logits, seq_len):
    lg, sq = _f32(logits), _i32(seq_len)
    ids = np.full(min(max(d.B, 1) * max(d.Tp, 1), 1 << 22), FILL_I32, np.int32)
    lens = np.full(64, FILL_I32, np.int32)
    rc = lib().kt_ctc_greedy(ctypes.byref(d), _f(lg), _i(sq), _i(ids), _i(lens))
    return rc, ids, lens


def ctc_greedy(logits, seq_len, B, C):
    """argmax + collapse over logits [Tp][Bp][Cp] -> (ids [B][Tp], lens [Bp]); FILL where nothing was written."""
    Tp, Bp, Cp = logits.shape
    d = ctc_desc(Tp, B, C, 1)
    assert (d.Bp, d.Cp) == (Bp, Cp) and len(seq_len) == Bp
    rc, ids, lens = ctc_greedy_raw(d, logits, seq_len)
    _check(rc, 'kt_ctc_greedy')
    return ids.reshape(B, Tp), lens[:Bp]


def mean(v, pad=3):
    """launch_mean -> out [1 + pad]: the mean, then FILL"""
    v = _f32(v)
    out = _out(1 + pad)
    _check(lib().kt_mean(_f(v), v.size, _f(out), out.size, FILL), 'kt_mean')
    return out


# ------------------------------------------------------------------ checks shared by the GPU tests
def untouched(buf):
    """Mask of the floats that still hold the pre-fill pattern."""
    return np.asarray(buf, dtype=np.float32).view(np.uint32) == np.uint32(int.from_bytes(bytes([FILL] * 4), 'little'))


def expected_buffer(C64, rows, c_rows, ldc):
    """(expected [c_rows][ldc] fp64, written mask) of a result scattered by rows[]."""
    exp = np.zeros((c_rows, ldc))
    mask = np.zeros((c_rows, ldc), dtype=bool)
    N = C64.shape[1]
    for m, r in enumerate(rows):
        if r >= 0:
            exp[r, :N] = C64[m]
            mask[r, :N] = True
    return exp, mask
