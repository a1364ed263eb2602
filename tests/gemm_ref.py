"""NumPy fp64 reference of the GEMM layer (csrc/gemm.hip, csrc/gemm_tph.hip), written from the contracts in csrc/kernels.h
and the layout comment of gemm_tph.hip - not from any kernel.  Used by tests/test_gemm_ref_host.py (CPU) and the GPU tests
test_gpu_gemm_kernels.py / test_gpu_tph_planes.py.

  GemmCase / TphCase   one launch, as data: what the harness uploads and what gemm_ref restates
  gemm_ref(case)       -> (C64 [nbatch][M][N] fp64, rows [M]: physical result row of each logical row, -1 = not written)
  tph_encode / tph_decode   the tiled-planes layout TPH[row/32][k/16][part][32 x 16], slot ((r<<1) | (h ^ ((r>>3)&1))) << 4
  scale_model          (2^(15-e), 2^(e-15)) with max < 2^e
  tph_bound / f32_bound     the per-element error the file headers promise
"""
from dataclasses import dataclass, field
from functools import lru_cache
from typing import List, Optional

import numpy as np

U24 = 2.0 ** -24


# ------------------------------------------------------------------ descriptors
@dataclass
class GemmCase:
    """GemmDesc with its buffers: A / B are the PHYSICAL 2-D arrays (rows x ld)."""
    A: np.ndarray
    B: np.ndarray
    M: int
    N: int
    K: int
    ldc: int
    c_rows: int                      # physical rows of the C buffer
    a_col: bool = False
    b_col: bool = False
    a_map: Optional[np.ndarray] = None
    a_shift: int = 0
    a_rows: int = 0
    c_map: Optional[np.ndarray] = None
    bias: Optional[np.ndarray] = None
    split_k: int = 1


@dataclass
class TphCase:
    """GemmTPHDesc in logical terms: batch b multiplies A[b] [>= M rows][KA] by B[b] [>= N rows][KB]^T (unscaled fp32
    matrices; the planes hold them times their row scales, which the epilogue takes out again, exactly)."""
    A: List[np.ndarray]
    B: List[np.ndarray]
    M: int
    N: int
    K: int
    ldc: int
    c_rows: int
    a_kshift: int = 0
    a_kshift1: int = 0
    bias: Optional[np.ndarray] = None
    split_k: int = 1
    tile_rows: int = 0
    side: bool = False
    c_map: Optional[np.ndarray] = None
    nbatch: int = 1
    extra: dict = field(default_factory=dict)


def _rows_of(case, M):
    if case.c_map is None:
        return np.arange(M, dtype=np.int64)
    return np.asarray(case.c_map[:M], dtype=np.int64)


def gemm_ref(case):
    """fp64 restatement of GemmDesc / GemmTPHDesc.  Returns (C64 [nbatch][M][N], rows [M])."""
    if isinstance(case, GemmCase):
        return _gemm_f32_ref(case)
    return _gemm_tph_ref(case)


def _gemm_f32_ref(c):
    A = np.asarray(c.A, dtype=np.float64)
    B = np.asarray(c.B, dtype=np.float64)
    M, N, K = c.M, c.N, c.K

    def phys(logical):       # kernels.h: a_map (-1 = zero row), else logical + a_shift; rows outside [0, a_rows) are zero
        r = int(c.a_map[logical]) if c.a_map is not None else logical + c.a_shift
        return r if 0 <= r < c.a_rows else -1

    Al = np.zeros((M, K))
    if not c.a_col:          # A(m,k) = A[row(m)*lda + k]
        for m in range(M):
            r = phys(m)
            if r >= 0:
                Al[m] = A[r, :K]
    else:                    # A(m,k) = A[row(k)*lda + m]
        for k in range(K):
            r = phys(k)
            if r >= 0:
                Al[:, k] = A[r, :M]
    Bl = B[:N, :K].T if c.b_col else B[:K, :N]      # B(k,n) = B[n*ldb + k] / B[k*ldb + n]
    C = Al @ Bl
    if c.bias is not None:
        C = C + np.asarray(c.bias, dtype=np.float64)[None, :N]
    return C[None], _rows_of(c, M)


def tph_operands(c, b):
    """The two factors of batch b as fp64 [M][K] / [N][K]: A read at k + shift, both zero outside their own k extent."""
    shift = c.a_kshift1 if b else c.a_kshift
    A = np.asarray(c.A[b], dtype=np.float64)[:c.M]
    B = np.asarray(c.B[b], dtype=np.float64)[:c.N]
    Al = np.zeros((c.M, c.K))
    Bl = np.zeros((c.N, c.K))
    k = np.arange(c.K)
    ka = k + shift
    ok = (ka >= 0) & (ka < A.shape[1])
    Al[:, k[ok]] = A[:, ka[ok]]
    kb = k[k < B.shape[1]]
    Bl[:, kb] = B[:, kb]
    return Al, Bl


def _gemm_tph_ref(c):
    out = []
    for b in range(2 if c.nbatch > 1 else 1):
        Al, Bl = tph_operands(c, b)
        C = Al @ Bl.T
        if c.bias is not None and c.split_k == 1:
            C = C + np.asarray(c.bias, dtype=np.float64)[None, :c.N]
        out.append(C)
    return np.stack(out), _rows_of(c, c.M)


# ------------------------------------------------------------------ tiled planes
def tph_bytes(rows, K):
    return ((rows + 31) // 32) * ((K + 15) // 16) * 2 * 1024


@lru_cache(maxsize=64)
def _tph_index(rows_p, nkb, part):
    """fp16-element index of (row, k) for every row < rows_p (a multiple of 32) and k < 16 nkb (cached: read-only)."""
    r = np.arange(rows_p)[:, None]
    k = np.arange(nkb * 16)[None, :]
    rb, rr, kb, kk = r // 32, r % 32, k // 16, k % 16
    h, e = kk >> 3, kk & 7
    slot16 = (((rr << 1) | (h ^ ((rr >> 3) & 1))) << 4) // 2     # the slot is in bytes: 8 fp16 each
    idx = ((rb * nkb + kb) * 2 + part) * 512 + slot16 + e
    idx.setflags(write=False)
    return idx


def split_parts(v):
    """h1 = fp16(v), h2 = fp16(v - h1) of fp32 values (the subtraction in fp32, where it is exact)."""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(invalid='ignore', over='ignore'):
        h1 = v.astype(np.float16)
        h2 = (v - h1.astype(np.float32)).astype(np.float16)
    return h1, h2


def tph_encode_parts(h1, h2):
    """Two fp16 matrices [rows][K] -> the plane bytes (uint8, tph_bytes(rows, K)); everything outside is zero."""
    rows, K = h1.shape
    rows_p, nkb = (rows + 31) // 32 * 32, (K + 15) // 16
    out = np.zeros(tph_bytes(rows, K) // 2, dtype=np.float16)
    for part, h in enumerate((h1, h2)):
        full = np.zeros((rows_p, nkb * 16), dtype=np.float16)
        full[:rows, :K] = h
        out[_tph_index(rows_p, nkb, part)] = full
    return out.view(np.uint8)


def tph_encode(x, scale):
    """Planes of the fp32 matrix x [rows][K] times its per-row power-of-two scales."""
    v = np.asarray(x, dtype=np.float32) * np.asarray(scale, dtype=np.float32)[:, None]
    return tph_encode_parts(*split_parts(v))


def tph_decode(buf, rows, K):
    """Plane bytes -> (h1, h2) as fp16 [rup32(rows)][16 ceil(K/16)]: padding included, so a test can look at it."""
    rows_p, nkb = (rows + 31) // 32 * 32, (K + 15) // 16
    b16 = np.asarray(buf, dtype=np.uint8).view(np.float16)
    assert b16.size == tph_bytes(rows, K) // 2
    return b16[_tph_index(rows_p, nkb, 0)], b16[_tph_index(rows_p, nkb, 1)]


# ------------------------------------------------------------------ scales
def line_max(x, axis):
    """Largest magnitude along a line the way fmaxf folds it from 0: a NaN element is dropped, inf stays."""
    a = np.abs(np.asarray(x, dtype=np.float32))
    return np.max(np.where(np.isnan(a), np.float32(0), a), axis=axis, initial=np.float32(0))


def scale_model(m):
    """(scale, inv) = (2^(15-e), 2^(e-15)) with m < 2^e, e clamped to +-100; e = 15 (scale 1) for an all-zero line and for a
    maximum that is not finite or >= 3e38."""
    m = np.asarray(m, dtype=np.float32)
    ok = (m > 0) & (m < np.float32(3.0e38))
    _, e = np.frexp(np.where(ok, m, np.float32(1)))       # m = f 2^e, f in [0.5, 1)
    e = np.where(ok, e, 15)
    e = np.clip(e, -100, 100)
    return np.ldexp(np.float32(1), 15 - e).astype(np.float32), np.ldexp(np.float32(1), e - 15).astype(np.float32)


# ------------------------------------------------------------------ bounds
def f32_bound(A, B, K, splits=1):
    """fp32 accumulation of K terms plus the slab sum: (K + splits + 2) 2^-24 sum_k |a_k b_k|.  A [M][K], B [N][K]."""
    S = np.abs(np.asarray(A, dtype=np.float64)) @ np.abs(np.asarray(B, dtype=np.float64)).T
    return (K + splits + 2) * U24 * S


def tph_bound(A, B, K, splits=1, amax=None, bmax=None):
    """What gemm_tph.hip's header promises per element of A [M][K] * B [N][K]^T:
      sum_k (|a_k| db_k + |b_k| da_k),  dx_k = max(2^-23 |x_k|, 2^-39 linemax(x))   the two fp16 parts of each operand
      2^-22 sum_k |a_k b_k|                                                         the dropped h2 * h2' product
      (K + splits + 2) 2^-24 sum_k |a_k b_k|                                        fp32 accumulation and the slab sum
    amax / bmax: the line maxima the scales were taken from (default: of the rows given)."""
    A = np.abs(np.asarray(A, dtype=np.float64))
    B = np.abs(np.asarray(B, dtype=np.float64))
    amax = A.max(axis=1) if amax is None else np.asarray(amax, dtype=np.float64)
    bmax = B.max(axis=1) if bmax is None else np.asarray(bmax, dtype=np.float64)
    dA = np.maximum(2.0 ** -23 * A, 2.0 ** -39 * amax[:, None])
    dB = np.maximum(2.0 ** -23 * B, 2.0 ** -39 * bmax[:, None])
    S = A @ B.T
    return A @ dB.T + dA @ B.T + 2.0 ** -22 * S + (K + splits + 2) * U24 * S


# ------------------------------------------------------------------ data regimes
def exact_matrix(rng, rows, cols):
    """Small integers in [-4, 4]: every partial sum of up to 4096 products is exact in fp32 and in one fp16 plane."""
    return rng.integers(-4, 5, size=(rows, cols)).astype(np.float32)


def precision_matrix(rng, rows, cols, row_spread=0, zero_row=None, zero_col=None):
    """fp32 with full 24-bit significands, magnitudes 2^-20 .. 2^20 inside a row, rows spread over 2^+-row_spread."""
    mant = (rng.integers(1 << 23, 1 << 24, size=(rows, cols)).astype(np.float64)) * 2.0 ** -23      # [1, 2), 24 bits
    x = mant * 2.0 ** rng.integers(-20, 20, size=(rows, cols)) * rng.choice([-1.0, 1.0], size=(rows, cols))
    if row_spread:
        x = x * 2.0 ** rng.integers(-row_spread, row_spread + 1, size=(rows, 1))
    if zero_row is not None and zero_row < rows:
        x[zero_row] = 0
    if zero_col is not None and zero_col < cols:
        x[:, zero_col] = 0
    out = x.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), x)      # nothing rounded: the reference sees the operands exactly
    return out


# name -> M, N, K, split_k, nbatch, tile_rows, side, c_map: one precision case per gemm_tph_kernel instantiation, one
# split-K, one two-batch (tests/test_gemm_ref_host.py checks the bound's sensitivity at exactly these)
PRECISION_CASES = {
    't256': dict(M=260, N=260, K=80, tile_rows=256),
    't192': dict(M=196, N=68, K=48, tile_rows=192),
    'side': dict(M=132, N=196, K=80, side=True),
    't256_cmap': dict(M=260, N=68, K=48, tile_rows=256, c_map=True),
    't192_cmap': dict(M=196, N=260, K=80, tile_rows=192, c_map=True),
    'split3': dict(M=196, N=68, K=208, split_k=3),      # 13 k-blocks in slices of 6, 6, 1
    'batch2': dict(M=36, N=68, K=80, nbatch=2, a_kshift=-16, a_kshift1=16),
}


def precision_case(name):
    """The TphCase of PRECISION_CASES[name], deterministic."""
    p = dict(PRECISION_CASES[name])
    seed = sorted(PRECISION_CASES).index(name)
    rng = np.random.default_rng(1000 + seed)
    M, N, K = p['M'], p['N'], p['K']
    nb = p.get('nbatch', 1)
    A = [precision_matrix(rng, M, K, 30, zero_row=1, zero_col=2) for _ in range(nb)]
    B = [precision_matrix(rng, N, K, 30, zero_row=3) for _ in range(nb)]
    c_map = None
    c_rows = M
    if p.get('c_map'):
        c_rows = M + 8
        c_map = rng.permutation(c_rows)[:M].astype(np.int32)
        c_map[::7] = -1
    return TphCase(A=A, B=B, M=M, N=N, K=K, ldc=N, c_rows=c_rows, a_kshift=p.get('a_kshift', 0), a_kshift1=p.get('a_kshift1', 0),
                   split_k=p.get('split_k', 1), tile_rows=p.get('tile_rows', 0), side=p.get('side', False), c_map=c_map, nbatch=nb)


def tph_emulate(A, B, amax=None, bmax=None, drop_h2=False, drop_cross=False, scale_off_row=None, drop_kblock=None):
    """The three-product scheme in NumPy on A [M][K], B [N][K] (fp32): row scales, two fp16 parts, per k-block the three
    products added to an fp32 accumulator (one rounding per product block), the inverse scales at the end.  The keyword
    arguments break it the way a wrong kernel would."""
    A = np.asarray(A, dtype=np.float32)
    B = np.asarray(B, dtype=np.float32)
    sa, ia = scale_model(line_max(A, 1) if amax is None else amax)
    sb, ib = scale_model(line_max(B, 1) if bmax is None else bmax)
    a1, a2 = (h.astype(np.float64) for h in split_parts(A * sa[:, None]))
    b1, b2 = (h.astype(np.float64) for h in split_parts(B * sb[:, None]))
    if drop_h2:
        a2, b2 = np.zeros_like(a2), np.zeros_like(b2)
    acc = np.zeros((A.shape[0], B.shape[0]), dtype=np.float32)
    K = A.shape[1]
    for kb in range((K + 15) // 16):
        if kb == drop_kblock:
            continue
        s = slice(16 * kb, min(K, 16 * kb + 16))
        terms = [(a2, b1), (a1, b2), (a1, b1)]          # smallest first, as chain3
        if drop_cross:
            terms = terms[1:]
        for x, y in terms:
            acc = (acc.astype(np.float64) + x[:, s] @ y[:, s].T).astype(np.float32)
    ia = ia.astype(np.float64).copy()
    if scale_off_row is not None:
        ia[scale_off_row] *= 2
    return acc.astype(np.float64) * ia[:, None] * ib.astype(np.float64)[None, :]
