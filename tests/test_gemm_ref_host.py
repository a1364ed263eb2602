"""CPU checks of the GEMM kernel tests' own tools: the plane codec and fp64 reference of tests/gemm_ref.py against
hand-written cases, the sensitivity of tph_bound (a wrong three-product scheme must leave it by a factor >= 10 at every
precision case), and the harness library's build and symbols."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import gemm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ planes
@pytest.mark.parametrize('rows,K', [(1, 4), (32, 16), (33, 17), (70, 50), (64, 64), (31, 15)])
def test_plane_codec_round_trip(rows, K):
    rng = np.random.default_rng(rows * 100 + K)
    h1 = rng.standard_normal((rows, K)).astype(np.float16)
    h2 = (rng.standard_normal((rows, K)) * 1e-3).astype(np.float16)
    buf = R.tph_encode_parts(h1, h2)
    assert buf.dtype == np.uint8 and buf.size == R.tph_bytes(rows, K)
    d1, d2 = R.tph_decode(buf, rows, K)
    assert np.array_equal(d1[:rows, :K], h1) and np.array_equal(d2[:rows, :K], h2)
    for d in (d1, d2):                       # ragged edges: everything outside the matrix is zero
        pad = d.copy()
        pad[:rows, :K] = 0
        assert not pad.any()
    # every fp16 slot of the buffer is the image of exactly one (row, k, part)
    idx = np.concatenate([R._tph_index(d1.shape[0], d1.shape[1] // 16, p).ravel() for p in (0, 1)])
    assert np.array_equal(np.sort(idx), np.arange(buf.size // 2))


def test_plane_layout_by_hand():
    """TPH[row/32][k/16][part][32 x 16], slot ((r<<1) | (h ^ ((r>>3)&1))) << 4 bytes, 8 fp16 per slot."""
    rows, K = 40, 40                         # 2 row blocks x 3 k-blocks
    h1 = np.zeros((rows, K), np.float16)
    h2 = np.zeros((rows, K), np.float16)
    h1[0, 0] = 1      # tile 0, part 0, slot 0, element 0
    h1[0, 9] = 2      # r = 0, h = 1: slot 1 -> byte 16, element 1
    h1[8, 1] = 3      # r = 8: the halves swap: h = 0 -> slot (16 | 1) = 17, element 1
    h2[35, 37] = 4    # row block 1, k-block 2, part 1, r = 3, h = 0 (k % 16 = 5): slot 6, element 5
    b16 = R.tph_encode_parts(h1, h2).view(np.float16)
    want = {0: 1, 8 * 1 + 1: 2, 8 * 17 + 1: 3, ((1 * 3 + 2) * 2 + 1) * 512 + 8 * 6 + 5: 4}
    assert {int(i): float(b16[i]) for i in np.flatnonzero(b16)} == want


def test_split_parts_hold_24_bits():
    rng = np.random.default_rng(3)
    v = R.precision_matrix(rng, 64, 64)
    s, inv = R.scale_model(R.line_max(v, 1))
    x = v * s[:, None]
    assert np.all((R.line_max(x, 1) >= 2.0 ** 14) & (R.line_max(x, 1) < 2.0 ** 15))
    h1, h2 = R.split_parts(x)
    err = np.abs(h1.astype(np.float64) + h2.astype(np.float64) - x.astype(np.float64))
    assert np.all(err <= np.maximum(2.0 ** -23 * np.abs(x), 2.0 ** -39 * 2.0 ** 15))


def test_scale_model_by_hand():
    m = np.array([0, 1, 0.75, 2.0 ** 14, np.nextafter(np.float32(2 ** 15), np.float32(0)), np.inf, 3.2e38, 1e-45, np.nan],
                 np.float32)
    s, inv = R.scale_model(m)
    #        zero  1 < 2^1  .75 < 2^0  2^14 < 2^15  < 2^15  inf  >= 3e38  denormal: e = -100  NaN as a maximum
    want = [0, 14, 15, 0, 0, 0, 0, 115, 0]
    assert np.array_equal(s, np.ldexp(np.float32(1), want)) and np.all(s * inv == 1)
    assert R.line_max(np.array([[np.nan, -3, 2], [np.nan, np.nan, np.nan], [1, np.inf, 0]], np.float32), 1).tolist() == [3, 0, np.inf]


# ------------------------------------------------------------------ gemm_ref against hand-written cases
def _phys(rng, rows, ld):
    return rng.integers(-4, 5, size=(rows, ld)).astype(np.float32)


def test_gemm_ref_f32_layouts():
    rng = np.random.default_rng(5)
    M, N, K = 8, 12, 4
    for a_col in (False, True):
        for b_col in (False, True):
            A = _phys(rng, K if a_col else M, 16)
            B = _phys(rng, N if b_col else K, 16)
            c = R.GemmCase(A=A, B=B, M=M, N=N, K=K, ldc=N, c_rows=M, a_col=a_col, b_col=b_col, a_rows=A.shape[0])
            C, rows = R.gemm_ref(c)
            Al = A[:K, :M].T if a_col else A[:M, :K]
            Bl = B[:N, :K].T if b_col else B[:K, :N]
            assert np.array_equal(C[0], Al.astype(np.float64) @ Bl) and np.array_equal(rows, np.arange(M))


def test_gemm_ref_f32_maps_shift_bias():
    rng = np.random.default_rng(6)
    M, N, K = 4, 4, 4
    A, B = _phys(rng, 6, 8), _phys(rng, K, 4)
    bias = np.array([1, 2, 4, 8], np.float32)
    # shift: logical row m reads physical m + 2; a_rows = 5 clips physical row 5 (logical 3)
    C, _ = R.gemm_ref(R.GemmCase(A=A, B=B, M=M, N=N, K=K, ldc=N, c_rows=M, a_shift=2, a_rows=5, bias=bias))
    want = np.vstack([A[2, :K], A[3, :K], A[4, :K], np.zeros(K)]).astype(np.float64) @ B + bias
    assert np.array_equal(C[0], want)
    # negative shift clips at the other end
    C, _ = R.gemm_ref(R.GemmCase(A=A, B=B, M=M, N=N, K=K, ldc=N, c_rows=M, a_shift=-1, a_rows=6))
    assert np.array_equal(C[0], np.vstack([np.zeros(K), A[0, :K], A[1, :K], A[2, :K]]).astype(np.float64) @ B)
    # a_map in the row role, with -1 and a row past a_rows; c_map scatters and drops
    a_map = np.array([5, -1, 0, 3], np.int32)
    c_map = np.array([2, -1, 0, 5], np.int32)
    C, rows = R.gemm_ref(R.GemmCase(A=A, B=B, M=M, N=N, K=K, ldc=N, c_rows=6, a_map=a_map, a_rows=5, c_map=c_map))
    assert np.array_equal(C[0], np.vstack([np.zeros(K), np.zeros(K), A[0, :K], A[3, :K]]).astype(np.float64) @ B)
    assert rows.tolist() == [2, -1, 0, 5]
    # a_map in the k role (a_col): logical k reads physical row a_map[k]
    At = _phys(rng, 6, 8)
    C, _ = R.gemm_ref(R.GemmCase(A=At, B=B, M=M, N=N, K=K, ldc=N, c_rows=M, a_col=True, a_map=a_map, a_rows=5))
    Al = np.stack([np.zeros(M), np.zeros(M), At[0, :M], At[3, :M]], axis=1)
    assert np.array_equal(C[0], Al.astype(np.float64) @ B)


def test_gemm_ref_tph_features():
    rng = np.random.default_rng(7)
    M, N, K = 4, 8, 32
    A = [_phys(rng, M, 48), _phys(rng, M, 48)]
    B = [_phys(rng, N, 32), _phys(rng, N, 32)]
    bias = np.arange(N, dtype=np.float32)
    C, rows = R.gemm_ref(R.TphCase(A=A[:1], B=B[:1], M=M, N=N, K=K, ldc=N, c_rows=M, bias=bias))
    assert np.array_equal(C[0], A[0][:, :K].astype(np.float64) @ B[0].T + bias)
    # bias only with split 1
    C, _ = R.gemm_ref(R.TphCase(A=A[:1], B=B[:1], M=M, N=N, K=K, ldc=N, c_rows=M, bias=bias, split_k=2))
    assert np.array_equal(C[0], A[0][:, :K].astype(np.float64) @ B[0].T)
    # two batches, the dU shifts: batch 0 reads A at k - 16 (zero for k < 16), batch 1 at k + 16 (zero from K_A = 48 on)
    C, _ = R.gemm_ref(R.TphCase(A=A, B=B, M=M, N=N, K=K, ldc=N, c_rows=M, nbatch=2, a_kshift=-16, a_kshift1=16))
    want0 = np.hstack([np.zeros((M, 16)), A[0][:, :16]]).astype(np.float64) @ B[0].T
    want1 = A[1][:, 16:48].astype(np.float64) @ B[1].T
    assert np.array_equal(C[0], want0) and np.array_equal(C[1], want1)
    # K_B shorter than K: B is zero past its extent
    C, _ = R.gemm_ref(R.TphCase(A=A[:1], B=[B[0][:, :16]], M=M, N=N, K=K, ldc=N, c_rows=M))
    assert np.array_equal(C[0], A[0][:, :16].astype(np.float64) @ B[0][:, :16].T)
    c_map = np.array([3, -1, 1, 0], np.int32)
    _, rows = R.gemm_ref(R.TphCase(A=A[:1], B=B[:1], M=M, N=N, K=K, ldc=N, c_rows=M, c_map=c_map))
    assert rows.tolist() == [3, -1, 1, 0]


def test_exact_regime_is_exact():
    """|x| <= 4, K <= 4096: |sum| <= 2^16 in fp32; scaled by 2^12 (max 4 -> [2^14, 2^15)) an fp16 holds every such integer."""
    x = np.arange(-4, 5, dtype=np.float32)[None, :]
    s, _ = R.scale_model(R.line_max(x, 1))
    h1, h2 = R.split_parts(x * s[:, None])
    assert s[0] == 2.0 ** 12 and np.array_equal(h1.astype(np.float32), x * s[0]) and not h2.any()
    assert 16 * 4096 < 2 ** 24


# ------------------------------------------------------------------ sensitivity of the bound
def _operands(name):
    c = R.precision_case(name)
    out = []
    for b in range(2 if c.nbatch > 1 else 1):
        Al, Bl = R.tph_operands(c, b)
        # the scales come from the whole stored rows, shifted out or not
        out.append((Al.astype(np.float32), Bl.astype(np.float32), R.line_max(c.A[b], 1), R.line_max(c.B[b], 1)))
    return c, out


@pytest.mark.parametrize('name', sorted(R.PRECISION_CASES))
def test_bound_holds_for_the_scheme_and_not_for_a_broken_one(name):
    c, ops = _operands(name)
    smallest = np.inf
    for Al, Bl, amax, bmax in ops:
        C64 = Al.astype(np.float64) @ Bl.astype(np.float64).T
        bound = R.tph_bound(Al, Bl, c.K, c.split_k, amax, bmax)
        good = R.tph_emulate(Al, Bl, amax, bmax)
        nz = bound > 0
        assert np.all(np.abs(good - C64) <= bound)
        assert np.all(good[~nz] == 0)
        live_row = int(np.flatnonzero(np.abs(Al).sum(axis=1) > 0)[0])
        # the k-block that matters most somewhere: the one holding the largest product of some element
        kb = int(np.argmax(np.abs(Al[live_row] * Bl[0])) // 16)
        for broken in (dict(drop_h2=True), dict(drop_cross=True), dict(scale_off_row=live_row), dict(drop_kblock=kb)):
            bad = R.tph_emulate(Al, Bl, amax, bmax, **broken)
            factor = np.max(np.abs(bad - C64)[nz] / bound[nz])
            print(f'{name}: {broken} leaves the bound by a factor {factor:.3g}')
            smallest = min(smallest, factor)
    assert smallest >= 10, smallest


def test_f32_bound_is_the_accumulation_term():
    rng = np.random.default_rng(9)
    A, B = R.precision_matrix(rng, 8, 36), R.precision_matrix(rng, 12, 36)
    S = np.abs(A.astype(np.float64)) @ np.abs(B.astype(np.float64)).T
    assert np.array_equal(R.f32_bound(A, B, 36, 3), (36 + 3 + 2) * 2.0 ** -24 * S)
    full = R.tph_bound(A, B, 36, 3)
    assert np.all(full >= R.f32_bound(A, B, 36, 3) + 2.0 ** -22 * S)
    # a plain fp32 dot product in k order stays inside it
    acc = np.zeros((8, 12), np.float32)
    for k in range(36):
        acc = (acc.astype(np.float64) + np.outer(A[:, k].astype(np.float64), B[:, k].astype(np.float64))).astype(np.float32)
    assert np.all(np.abs(acc - A.astype(np.float64) @ B.astype(np.float64).T) <= R.f32_bound(A, B, 36, 1))


# ------------------------------------------------------------------ the harness library
def test_harness_library_builds_and_exports_its_entry_points():
    """libnasr_kt.so comes out of the same build as libnasr.so, loads (every symbol it needs resolves), exports the kt_*
    entry points of tests/kernel_harness.py, and needs nothing from outside that libnasr.so does not need as well."""
    from neuralasr_amd import _lib, build
    import kernel_harness as H
    build.build()
    assert os.path.exists(H.KT_PATH) and os.path.dirname(H.KT_PATH) == os.path.dirname(_lib.LIB_PATH)
    lib = ctypes.CDLL(H.KT_PATH)
    for n in H.SYMBOLS:
        assert hasattr(lib, n), f'{n} is not exported by libnasr_kt.so'
    nm = shutil.which('nm')
    assert nm, 'binutils nm is needed to compare the two libraries\' undefined symbols'

    def syms(path, flag):
        out = subprocess.run([nm, '-D', flag, path], capture_output=True, text=True, check=True).stdout
        return {line.split()[-1].split('@')[0] for line in out.splitlines() if line.strip()}
    exported = {s for s in syms(H.KT_PATH, '--defined-only') if s.startswith('kt_')}
    assert exported == set(H.SYMBOLS)
    # all three layers: the GEMMs, the recurrence, the CTC kernels
    assert {'kt_gemm_tph', 'kt_lstm_persist_bwd', 'kt_ctc_pass', 'kt_ctc_greedy', 'kt_mean'} <= exported
    extra = syms(H.KT_PATH, '--undefined-only') - syms(_lib.LIB_PATH, '--undefined-only')
    assert not extra, f'libnasr_kt.so needs symbols libnasr.so does not: {sorted(extra)}'
    out = subprocess.run(['strings', '-a', H.KT_PATH], capture_output=True, text=True).stdout if shutil.which('strings') else 'gfx950'
    assert 'gfx950' in out
