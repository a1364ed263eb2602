"""The two GEMM files against fp64, launch by launch (tests/kernel_harness -> libnasr_kt.so, the objects of libnasr.so):
csrc/gemm.hip (gemm_kernel<a_col, b_col>, block tile 128 x 128 x 16) and csrc/gemm_tph.hip (gemm_tph_kernel<4,2,4>,
<3,2,4>, their CMAP forms and <4,1,3>; block tile 256 | 192 x 256, side 128 x 192, a step = two k-blocks of 16).

Exact regime: integers in [-4, 4], power-of-two scales and biases, K <= 4096 - every partial sum is exact in fp32 and in one
fp16 plane, so the result must equal gemm_ref's fp64 BITWISE whatever the k order, split or batch.  It carries the indexing
cases.  Precision regime: full 24-bit significands over 2^-20 .. 2^20 (rows over 2^+-30 for the planes), held to
tph_bound / f32_bound element-wise.  Poison: NaN wherever the contract says nothing is read; every output byte outside
the logical result must keep the harness's pre-fill."""
import zlib

import numpy as np
import pytest

import gemm_ref as R
import kernel_harness as H

pytestmark = pytest.mark.gpu

RATIOS = {}          # largest err / bound per precision case (printed; DESIGN.md quotes a run)


def check_exact(out, C64, rows, c_rows, ldc, what):
    exp, mask = H.expected_buffer(C64, rows, c_rows, ldc)
    out = out.reshape(c_rows, ldc)
    assert np.array_equal(H.untouched(out), ~mask), f'{what}: bytes outside the result were written (or result bytes were not)'
    assert np.all(np.isfinite(out[mask])), f'{what}: the kernel read something it must not'
    bad = np.flatnonzero(out[mask].astype(np.float64) != exp[mask])
    assert bad.size == 0, f'{what}: {bad.size} elements differ from fp64, first {out[mask][bad[0]]} vs {exp[mask][bad[0]]}'


def check_bound(out, C64, bound, rows, c_rows, ldc, what):
    exp, mask = H.expected_buffer(C64, rows, c_rows, ldc)
    bnd, _ = H.expected_buffer(bound, rows, c_rows, ldc)
    out = out.reshape(c_rows, ldc)
    assert np.array_equal(H.untouched(out), ~mask), what
    assert np.all(np.isfinite(out[mask])), what
    err = np.abs(out[mask].astype(np.float64) - exp[mask])
    b = bnd[mask]
    ratio = float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1), np.where(err > 0, np.inf, 0))))
    RATIOS[what] = max(RATIOS.get(what, 0.0), ratio)
    print(f'err/bound {what}: {ratio:.4f}')
    assert np.all(err <= b), f'{what}: err / bound = {ratio}'


# =================================================================== gemm.hip
def f32_case(rng, M, N, K, a_col, b_col, split_k=1, bias=False, c_map=False, a_shift=0, a_rows=None, a_map=None,
             precision=False):
    """A GemmCase with every ld 4 wider than the logical width, NaN in columns [K, ld), in the rows outside [0, a_rows) and
    in the rows no logical index reaches; C has two spare rows (eight and a permutation with -1 under c_map)."""
    gen = (lambda r, c: R.precision_matrix(rng, r, c, zero_row=1, zero_col=2)) if precision else (lambda r, c: R.exact_matrix(rng, r, c))
    na = K if a_col else M                      # logical indices that pick a row of A
    wa = M if a_col else K
    a_rows = na if a_rows is None else a_rows
    A = np.full((a_rows + 2, wa + 4), np.nan, np.float32)
    A[:, :wa] = gen(a_rows + 2, wa)
    B = np.full((N if b_col else K, (K if b_col else N) + 4), np.nan, np.float32)
    B[:, :B.shape[1] - 4] = gen(B.shape[0], B.shape[1] - 4)
    read = {int(a_map[i]) if a_map is not None else i + a_shift for i in range(na)}
    for r in range(A.shape[0]):
        if r not in read or r >= a_rows:
            A[r] = np.nan
    cm, c_rows = None, M + 2
    if c_map:
        c_rows = M + 8
        cm = rng.permutation(c_rows)[:M].astype(np.int32)
        cm[::5] = -1
    b = (2.0 ** rng.integers(-2, 4, size=N)).astype(np.float32) if bias else None
    return R.GemmCase(A=A, B=B, M=M, N=N, K=K, ldc=N + 4, c_rows=c_rows, a_col=a_col, b_col=b_col, a_map=a_map, a_shift=a_shift,
                      a_rows=a_rows, c_map=cm, bias=b, split_k=split_k)


def run_f32_exact(c, what):
    C64, rows = R.gemm_ref(c)
    check_exact(H.gemm_f32(c), C64[0], rows, c.c_rows, c.ldc, what)


LAYOUTS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.mark.parametrize('a_col,b_col', LAYOUTS)
def test_f32_shapes(a_col, b_col):
    """Every tile edge: M, N below / at / above one and two 128-tiles, K below / at / above the 16-k tile (K tails 4, 12, 20,
    36, 132), ld > width, NaN outside."""
    rng = np.random.default_rng(11)
    for M in (4, 124, 128, 132, 260):
        for N in (4, 124, 128, 132, 260):
            for K in (4, 12, 16, 20, 36, 132):
                run_f32_exact(f32_case(rng, M, N, K, a_col, b_col), f'f32 {a_col} {b_col} {M}x{N}x{K}')


@pytest.mark.parametrize('a_col,b_col', LAYOUTS)
def test_f32_split_k(a_col, b_col):
    """split_k 1..3 at a K tail; K = 80 with split_k = 4 runs as 3 splits (the trailing one is dropped) - the slabs are NaN
    until written, so a reduction over a slab nobody wrote shows; bias and c_map go through the reduction kernel."""
    rng = np.random.default_rng(12)
    for split in (1, 2, 3):
        run_f32_exact(f32_case(rng, 132, 124, 132, a_col, b_col, split_k=split), f'split {split}')
    run_f32_exact(f32_case(rng, 132, 260, 80, a_col, b_col, split_k=4), 'dropped split')
    run_f32_exact(f32_case(rng, 132, 124, 36, a_col, b_col, split_k=2, bias=True), 'split + bias')
    run_f32_exact(f32_case(rng, 132, 124, 36, a_col, b_col, split_k=3, c_map=True), 'split + c_map')
    run_f32_exact(f32_case(rng, 260, 132, 132, a_col, b_col, split_k=3, bias=True, c_map=True), 'split + bias + c_map')
    run_f32_exact(f32_case(rng, 132, 124, 20, a_col, b_col, bias=True, c_map=True), 'bias + c_map, one split')


@pytest.mark.parametrize('a_col', [False, True])
def test_f32_shift_rows_and_map(a_col):
    """a_shift = +-16 with a_rows clipping at both ends; a_map as a permutation with -1 entries and entries past a_rows - in
    the row role (!a_col) and in the k role (a_col)."""
    rng = np.random.default_rng(13)
    M, N, K = 132, 124, 36
    n = K if a_col else M
    for shift, a_rows in ((16, n), (-16, n), (16, n + 16), (-16, n - 20)):
        run_f32_exact(f32_case(rng, M, N, K, a_col, False, a_shift=shift, a_rows=a_rows), f'shift {shift} a_rows {a_rows}')
    a_rows = n + 6
    a_map = rng.permutation(a_rows + 3)[:n].astype(np.int32)        # some entries >= a_rows: they read as zero
    a_map[::7] = -1
    for b_col in (False, True):
        run_f32_exact(f32_case(rng, M, N, K, a_col, b_col, a_rows=a_rows, a_map=a_map), 'a_map')
    run_f32_exact(f32_case(rng, M, N, K, a_col, False, a_rows=a_rows, a_map=a_map, split_k=2, c_map=True), 'a_map + split + c_map')


@pytest.mark.parametrize('a_col,b_col', LAYOUTS)
def test_f32_precision(a_col, b_col):
    rng = np.random.default_rng(14)
    for split in (1, 3):
        c = f32_case(rng, 132, 124, 132, a_col, b_col, split_k=split, precision=True)
        C64, rows = R.gemm_ref(c)
        A = np.nan_to_num(c.A[:c.K, :c.M].T if a_col else c.A[:c.M, :c.K])
        B = np.nan_to_num(c.B[:c.N, :c.K] if b_col else c.B[:c.K, :c.N].T)
        check_bound(H.gemm_f32(c), C64[0], R.f32_bound(A, B, c.K, split), rows, c.c_rows, c.ldc,
                    f'gemm_f32 a_col={int(a_col)} b_col={int(b_col)} split={split}')


def test_f32_pick_split():
    for M in (4, 128, 132, 260, 2048):
        for N in (4, 128, 260):
            for K in (4, 36, 127, 128, 132, 255, 256, 1040, 4096):
                s = H.lib().kt_gemm_pick_split(M, N, K)
                assert 1 <= s <= max(1, K // 128), (M, N, K, s)


# =================================================================== gemm_tph.hip
MODES = {'t192': dict(tile_rows=192), 't256': dict(tile_rows=256), 'side': dict(side=True)}
_mats = {}


def exact_op(rows, K, tag):
    """Integer operand [rows][K] and nothing else, cached: shared by the cases (and never modified)."""
    key = (rows, K, tag)
    if key not in _mats:
        rng = np.random.default_rng(zlib.crc32(repr(key).encode()))
        x = R.exact_matrix(rng, rows, K)
        if rows > 2:
            x[1] = 0                               # an all-zero row: scale 1
            x[2] = np.sign(x[2])                   # a row whose maximum is 1: another scale than its neighbours
        x.setflags(write=False)
        _mats[key] = x
    return _mats[key]


def tph_expected_rows(c, rows):
    """`side` never scatters in its epilogue (launch_gemm_tph: scatter = c_map && split_k == 1 && !side): with one split it
    writes row m to row m whatever c_map says; with split_k > 1 the reduction scatters for every instantiation."""
    return np.arange(c.M) if (c.side and c.c_map is not None and launched_splits(c) == 1) else rows


def launched_splits(c):
    kbs = (c.K + 15) // 16
    per = ((kbs + max(1, c.split_k) - 1) // max(1, c.split_k) + 1) & ~1
    return (kbs + per - 1) // per


def run_tph_exact(c, what, poison=True, gap=(0, 0, 0, 0, 0)):
    C64, rows = R.gemm_ref(c)
    rows = tph_expected_rows(c, rows)
    p = H.tph_planes(c, poison=poison, gap=gap)
    out, stride = H.gemm_tph(c, p)
    for b in range(C64.shape[0]):
        check_exact(out[b * stride:b * stride + c.c_rows * c.ldc], C64[b], rows, c.c_rows, c.ldc, f'{what} batch {b}')
    if C64.shape[0] == 2:
        assert np.all(H.untouched(out[c.c_rows * c.ldc:stride])), f'{what}: the gap between the two results was written'


def tph_case(M, N, K, mode, KA=None, KB=None, ldc_pad=4, **kw):
    nb = kw.get('nbatch', 1)
    A = [exact_op(M, KA or K, f'A{b}') for b in range(nb)]
    B = [exact_op(N, KB or K, f'B{b}') for b in range(nb)]
    if kw.get('split_k', 1) > 1 and 'c_map' not in kw:
        ldc_pad = 0                                # GemmTPHDesc: split_k > 1 needs ldc == N
    c_rows = kw.pop('c_rows', M + (0 if nb > 1 and kw.get('split_k', 1) > 1 else 1))
    return R.TphCase(A=A, B=B, M=M, N=N, K=K, ldc=N + ldc_pad, c_rows=c_rows, **MODES[mode], **kw)


def make_c_map(M, extra=8, seed=0):
    rng = np.random.default_rng(100 + seed)
    cm = rng.permutation(M + extra)[:M].astype(np.int32)
    cm[::5] = -1
    return cm


@pytest.mark.parametrize('mode', sorted(MODES))
def test_tph_shapes(mode):
    """M, N below / at / above the row-block, 192- and 256-tile edges, K of 1, 2, 3, 5 and 65 k-blocks (20: a ragged one),
    with a bias; plane rows [M, rup32(M)) and [N, rup32(N)) hold NaN."""
    bias = (2.0 ** np.arange(-3, 5)).astype(np.float32)
    for M in (4, 36, 192, 196, 260):
        for N in (4, 68, 192, 256, 260):
            for K in (16, 20, 48, 80, 1040):
                c = tph_case(M, N, K, mode, bias=np.resize(bias, N))
                run_tph_exact(c, f'tph {mode} {M}x{N}x{K}')


@pytest.mark.parametrize('mode', sorted(MODES))
def test_tph_unequal_k_extents(mode):
    """nkbA != nkbB: the shorter operand reads as zero past its own extent."""
    for KA, KB in ((80, 48), (48, 80), (16, 80), (80, 20)):
        run_tph_exact(tph_case(36, 68, 80, mode, KA=KA, KB=KB), f'KA {KA} KB {KB}')


@pytest.mark.parametrize('mode', sorted(MODES))
def test_tph_split_k(mode):
    """K = 1040 = 65 k-blocks: slices of 34 + 31 (split 2), 22 + 22 + 21 (3), 14 x 4 + 9 (5) - even chunks, an odd tail.  The
    slabs are NaN until written.  With c_map the reduction scatters (launch_reduce_slabs_rows) for every instantiation."""
    for split in (1, 2, 3, 5):
        run_tph_exact(tph_case(196, 68, 1040, mode, split_k=split), f'split {split}')
        run_tph_exact(tph_case(196, 68, 1040, mode, split_k=split, c_map=make_c_map(196), c_rows=204), f'split {split} c_map')
    for split in (2, 5):
        run_tph_exact(tph_case(36, 68, 1040, mode, split_k=split, nbatch=2, a_kshift=-16, a_kshift1=16), f'split {split} x 2')


@pytest.mark.parametrize('mode', sorted(MODES))
def test_tph_two_batches(mode):
    """nbatch == 2 with all five strides distinct (gaps of NaN between the batches' operands and inverse scales, the gap
    between the results must stay untouched); the dU form a_kshift = -16 / a_kshift1 = +16, and +-32; with unequal shifts
    batch 1 cannot pass by reading batch 0's."""
    gap = (1, 2, 12, 5, 9)
    for s0, s1 in ((-16, 16), (16, -16), (-32, 32), (32, 0), (0, -32)):
        c = tph_case(36, 68, 80, mode, nbatch=2, a_kshift=s0, a_kshift1=s1)
        C64, _ = R.gemm_ref(c)
        assert not np.array_equal(C64[0], C64[1])
        run_tph_exact(c, f'shifts {s0} {s1}', gap=gap)
    run_tph_exact(tph_case(196, 260, 48, mode, nbatch=2, a_kshift=-16, a_kshift1=16), 'two batches, several tiles', gap=gap)


@pytest.mark.parametrize('mode', sorted(MODES))
def test_tph_c_map_one_split(mode):
    """A permutation with -1: t192 / t256 take their CMAP instantiations and scatter in the epilogue; rows the map drops and
    rows nobody names keep the pre-fill.  `side` has no CMAP form: launch_gemm_tph gives it the plain epilogue, so with one
    split it IGNORES c_map and writes row m to row m (its callers, the side-stream weight gradients, never pass one)."""
    for M, N, K in ((196, 68, 48), (260, 260, 80), (36, 4, 16)):
        c = tph_case(M, N, K, mode, c_map=make_c_map(M), c_rows=M + 8, bias=np.ones(N, np.float32))
        run_tph_exact(c, f'c_map {M}x{N}x{K}')


def swizzle_on(gx, gy, gz):
    """launch_gemm_tph's rule: some split of the 8 XCDs into pr x pc x pz pads the grid by at most 1/8."""
    total = gx * gy * gz
    for pz in (1, 2, 4, 8):
        for pr in (1, 2, 4, 8):
            if pr * pz <= 8:
                pc = 8 // (pz * pr)
                padded = 8 * -(-gy // pr) * -(-gx // pc) * -(-gz // pz)
                if padded * 8 <= total * 9:
                    return padded
    return 0


def test_tph_xcd_swizzle_grids():
    """Grids that turn the XCD tile order on - exactly (8 = 2 x 2 x 2 tiles), with a padded sub-grid in z (15 K slices -> 16,
    2 x 23 -> 48), in the rows (15 row tiles -> 16) and with two batches in z (2 x 4 slices) - and small ones that leave it off
    (3 x 3 x 1 and 1 x 5 x 2: no multiple of 8 within 9/8 of 9 or 10 tiles).  The result never depends on it."""
    grids = [
        # case, (gx, gy, gz), padded size (0: off)
        (tph_case(200, 260, 128, 'side', split_k=2), (2, 2, 2), 8),
        (tph_case(36, 68, 480, 't192', split_k=15), (1, 1, 15), 16),
        (tph_case(4, 260, 736, 't256', split_k=23), (2, 1, 23), 48),
        (tph_case(1796, 4, 16, 'side'), (1, 15, 1), 16),
        (tph_case(36, 68, 256, 'side', split_k=4, nbatch=2, a_kshift=-16, a_kshift1=16), (1, 1, 8), 8),
        (tph_case(36, 68, 480, 't256', split_k=15, c_map=make_c_map(36), c_rows=44), (1, 1, 15), 16),
        (tph_case(260, 388, 48, 'side'), (3, 3, 1), 0),
        (tph_case(36, 68, 320, 't256', split_k=5, nbatch=2), (1, 1, 10), 0),
        (tph_case(388, 516, 16, 't192'), (3, 3, 1), 0),
    ]
    for c, grid, padded in grids:
        tm, tn = (128, 192) if c.side else (c.tile_rows, 256)
        assert (-(-c.N // tn), -(-c.M // tm), launched_splits(c) * c.nbatch) == grid
        assert swizzle_on(*grid) == padded, (grid, swizzle_on(*grid))
        run_tph_exact(c, f'grid {grid}')


@pytest.mark.parametrize('mode', sorted(MODES))
def test_tph_contraction_runs_over_whole_steps(mode):
    """The contract of GemmTPHDesc::K (kernels.h): a step is two k-blocks, so the kernel contracts over k in [0, Kc),
    Kc = 32 ceil(K / 32).  Whatever the operands hold in [K, Kc) ENTERS the sum - that is k-block ceil(K/16) when that count
    is odd, and the rest of a ragged k-block - and nothing from Kc on is read.  Every caller passes planes written for
    exactly K (nasr_pass.hip: launch_tph_split2 over the same `rows`, compacted or not, so nkb = ceil(K/16) and the ragged
    tail is zeros), which is why the requirement is documented and not worked around in the k-loop.
    Here K_A, K_B > K: NaN from Kc on (A: from Kc + its shift on) must not matter, integers in [K, Kc) must be summed, zeros
    there give the product over K."""
    M, N = 36, 68
    for K, KX, shift, split in ((48, 96, 0, 1), (20, 64, 0, 1), (64, 96, 0, 1), (48, 112, 16, 1), (48, 96, -16, 1),
                                (208, 256, 0, 3), (16, 48, 0, 1)):
        Kc = (K + 31) // 32 * 32
        for zero_tail in (False, True):
            A = exact_op(M, KX, 'cA').copy()
            B = exact_op(N, KX, 'cB').copy()
            if zero_tail:
                A[:, max(0, K + shift):], B[:, K:] = 0, 0
            ref = R.TphCase(A=[A], B=[B], M=M, N=N, K=K if zero_tail else Kc, ldc=N, c_rows=M, a_kshift=shift, split_k=split,
                            **MODES[mode])
            C64, rows = R.gemm_ref(ref)
            if zero_tail:
                Al, Bl = R.tph_operands(ref, 0)
                assert np.array_equal(C64[0], Al[:, :K] @ Bl[:, :K].T)
            run = R.TphCase(A=[A.copy()], B=[B.copy()], M=M, N=N, K=K, ldc=N, c_rows=M, a_kshift=shift, split_k=split, **MODES[mode])
            p = H.tph_planes(run, poison=True)
            for o, (x, lo) in enumerate(((run.A[0], Kc + shift), (run.B[0], Kc))):     # NaN in the k-blocks nobody may read
                h1, h2 = R.tph_decode(p['ab'[o]][0], x.shape[0], KX)
                h1, h2 = h1.copy(), h2.copy()
                h1[:, lo:], h2[:, lo:] = np.nan, np.nan
                p['ab'[o]] = (R.tph_encode_parts(h1, h2),) + p['ab'[o]][1:]
            out, _ = H.gemm_tph(run, p)
            check_exact(out, C64[0], rows, M, N, f'K {K} of {KX}, shift {shift}, split {split}, zero tail {zero_tail}')


@pytest.mark.parametrize('name', sorted(R.PRECISION_CASES))
def test_tph_precision(name):
    """One case per instantiation, one split-K, one two-batch, through launch_tph_scales + launch_tph_split2 where the
    harness can (one batch) and the Python planes otherwise; the same inputs tests/test_gemm_ref_host.py proves sensitive."""
    c = R.precision_case(name)
    C64, rows = R.gemm_ref(c)
    rows = tph_expected_rows(c, rows)
    nb = C64.shape[0]
    out, stride = H.gemm_tph(c, fp32=True) if nb == 1 else H.gemm_tph(c, H.tph_planes(c, poison=True))
    for b in range(nb):
        Al, Bl = R.tph_operands(c, b)
        bound = R.tph_bound(Al, Bl, c.K, launched_splits(c), R.line_max(c.A[b], 1), R.line_max(c.B[b], 1))
        check_bound(out[b * stride:b * stride + c.c_rows * c.ldc], C64[b], bound, rows, c.c_rows, c.ldc, f'gemm_tph {name}')


def test_tph_host_choices():
    """gemm_tp_tile_rows is 192 or 256; gemm_tph_pick_split stays in [1, 64], keeps >= 32 k-blocks per slice when it splits,
    and the slice length the launcher derives from it is an even number of k-blocks."""
    L = H.lib()
    for M in (4, 36, 192, 196, 260, 388, 516, 2048):
        assert L.kt_gemm_tp_tile_rows(M) in (192, 256)
        for N in (4, 68, 260):
            for K in (16, 20, 48, 80, 1040, 1056, 4096, 65536):
                for nb in (1, 2):
                    s = L.kt_gemm_tph_pick_split(M, N, K, nb)
                    kbs = (K + 15) // 16
                    assert 1 <= s <= 64 and (s == 1 or kbs // s >= 32), (M, N, K, nb, s)
                    per = ((kbs + s - 1) // s + 1) & ~1
                    assert per % 2 == 0 and per * s >= kbs
    # 576 = 3 x 192 wastes a quarter of 256-row tiles; 196 and 256 are no better off with 192-row ones
    assert [L.kt_gemm_tp_tile_rows(M) for M in (576, 196, 256, 512)] == [192, 256, 256, 256]
