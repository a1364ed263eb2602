"""The passes around the fp16-plane GEMM, launch by launch against tests/gemm_ref.py: operand scales (launch_tph_scales,
_batch, _from_parts), the fp32 -> two-plane split (launch_tph_split2, every form its callers use) and the reductions
(launch_colsum, launch_colsum_parts, launch_reduce_slabs, launch_reduce_slabs_rows).  Scales and planes are bitwise;
sums are bitwise on integers and within f32_bound on full-significand data."""
import numpy as np
import pytest

import gemm_ref as R
import kernel_harness as H

pytestmark = pytest.mark.gpu

F32 = np.float32
SHAPES = [(70, 50, 64), (64, 64, 64), (1, 4, 4)]          # rows, K, ld


def scale_matrix(rng, rows, K, ld):
    """Lines with the maxima that matter: a power of two, one ulp below one, all zero, denormal only, inf - as rows and, where
    the matrix is large enough, as columns.  Columns [K, ld) hold NaN: nobody reads them."""
    x = np.full((rows, ld), np.nan, F32)
    x[:, :K] = R.precision_matrix(rng, rows, K, 10)
    if rows >= 8 and K >= 8:
        x[:, :K] = np.where(np.abs(x[:, :K]) >= 2.0 ** 20, F32(1), x[:, :K])
        x[0, :K] = 0
        x[1, :K] = 0; x[1, 3] = 1e-42                     # denormal only
        x[2, 5] = -2.0 ** 24                              # exactly a power of two: the next exponent
        x[3, 6] = np.nextafter(F32(2.0 ** 25), F32(0))    # one ulp below
        x[4, 7] = -np.inf
        x[:, 0] = 0
        x[:, 1] = 0; x[5, 1] = -1e-42                     # a denormal-only column
        x[:, 2] = 0; x[6, 2] = 2.0 ** -3
    return x


def check_scales(got, src, rows, K):
    rs, ri, cs, ci = got
    for scale, inv, axis, n in ((rs, ri, 1, rows), (cs, ci, 0, K)):
        if scale is None:
            continue
        ws, wi = R.scale_model(R.line_max(src[:rows, :K], axis))
        assert np.array_equal(scale.view(np.uint32), ws.view(np.uint32)), (axis, scale, ws)
        assert np.array_equal(inv.view(np.uint32), wi.view(np.uint32))
        assert np.all(scale * inv == 1)


@pytest.mark.parametrize('rows,K,ld', SHAPES)
def test_scales_single(rows, K, ld):
    rng = np.random.default_rng(rows)
    src = scale_matrix(rng, rows, K, ld)
    check_scales(H.tph_scales(src, rows, K), src, rows, K)                       # rows + columns: the batch kernels, one job
    check_scales(H.tph_scales(src, rows, K, want_cols=False), src, rows, K)      # rows only: absmax_part + scale_final


def test_scales_nan_is_dropped():
    """A NaN element does not poison its line: fmaxf returns its other argument, so the line's scale comes from the finite
    elements (an all-NaN line counts as all zero: scale 1).  The planes of that element then hold NaN and so does every
    product that touches it - a NaN in an operand surfaces in the result, not in the scales of its neighbours."""
    rng = np.random.default_rng(2)
    src = scale_matrix(rng, 70, 50, 64)
    src[10, 4] = np.nan
    src[11, :50] = np.nan
    got = H.tph_scales(src, 70, 50)
    check_scales(got, src, 70, 50)
    assert got[0][11] == 1 and got[0][10] == R.scale_model(R.line_max(np.delete(src[10, :50], 4), 0))[0]


@pytest.mark.parametrize('njobs', [3, 17])
def test_scales_batch(njobs):
    """Jobs of unequal size in one call; 17 cross TPH_MAX_JOBS = 16 (two launch pairs, the workspace carried on)."""
    rng = np.random.default_rng(njobs)
    shapes = [SHAPES[i % 3] for i in range(njobs)]
    srcs = [scale_matrix(rng, *s) for s in shapes]
    jobs = [(src, s[0], s[1], i % 4 != 1) for i, (src, s) in enumerate(zip(srcs, shapes))]
    for (src, rows, K, want_rows), got in zip(jobs, H.tph_scales_batch(jobs)):
        assert (got[0] is not None) == want_rows
        check_scales(got, src, rows, K)


def test_scales_from_parts():
    rng = np.random.default_rng(5)
    rowpart = np.abs(scale_matrix(rng, 5, 70, 70))       # [nrp][rows]: partial maxima, reduced over the parts
    colpart = np.abs(scale_matrix(rng, 9, 50, 50))
    rowpart[:, 8] = 0
    for rp, cp in ((rowpart, colpart), (rowpart, None), (None, colpart)):
        rs, ri, cs, ci = H.tph_scales_from_parts(rp, cp)
        for part, scale, inv in ((rp, rs, ri), (cp, cs, ci)):
            if part is not None:
                ws, wi = R.scale_model(R.line_max(part, 0))
                assert np.array_equal(scale.view(np.uint32), ws.view(np.uint32)) and np.array_equal(inv.view(np.uint32), wi.view(np.uint32))


# ------------------------------------------------------------------ split2
def want_planes(x, scale):
    return R.split_parts(np.asarray(x, F32) * np.asarray(scale, F32)[:, None])


def check_planes(buf, rows, K, h1, h2, what):
    d1, d2 = R.tph_decode(buf, rows, K)
    for d, h, part in ((d1, h1, 'h1'), (d2, h2, 'h2')):
        full = np.zeros(d.shape, np.float16)              # tile regions outside the matrix: zeros
        full[:rows, :K] = h
        assert np.array_equal(d.view(np.uint16), full.view(np.uint16)), f'{what} {part}'


def split_source(rng, phys_rows, K, ld, precision=True):
    src = np.full((phys_rows, ld), np.nan, F32)
    src[:, :K] = R.precision_matrix(rng, phys_rows, K, 10, zero_row=1, zero_col=2) if precision else R.exact_matrix(rng, phys_rows, K)
    return src


@pytest.mark.parametrize('rows,K,ld', [(70, 50, 64), (64, 64, 64), (4, 4, 4), (130, 20, 24)])
def test_split2_planes_and_column_sums(rows, K, ld):
    """tpN = planes of x * row scale, tpT = planes of x^T * column scale: h1 == fp16(x s), h2 == fp16(x s - h1) for every
    element, zeros in the rest of every tile; colpart summed by launch_colsum_parts against the fp64 column sums."""
    rng = np.random.default_rng(rows + K)
    for precision in (True, False):
        src = split_source(rng, rows, K, ld, precision)
        x = src[:, :K]
        rs, _ = R.scale_model(R.line_max(x, 1))
        cs, _ = R.scale_model(R.line_max(x, 0))
        tpN, tpT, colpart = H.tph_split2(src, rows, K, row_scale=rs, col_scale=cs)
        check_planes(tpN, rows, K, *want_planes(x, rs), 'tpN')
        check_planes(tpT, K, rows, *want_planes(x.T, cs), 'tpT')
        out = H.colsum_parts(colpart, K)
        assert np.all(H.untouched(out[K:]))
        want = x.astype(np.float64).sum(axis=0)
        bound = R.f32_bound(x.T, np.ones((1, rows)), rows, colpart.shape[0])[:, 0]
        err = np.abs(out[:K].astype(np.float64) - want)
        assert np.all(err <= bound) and (precision or np.all(err == 0))


def test_split2_constant_scale():
    """row_scale == NULL / col_scale == NULL: the constants rs / cs scale every line."""
    rng = np.random.default_rng(8)
    src = split_source(rng, 70, 50, 64)
    x = src[:, :50] * F32(2.0 ** -40)                     # |x| < 2^-9: rs = 2^20, cs = 2^22 keep it inside fp16
    src[:, :50] = x
    tpN, tpT, _ = H.tph_split2(src, 70, 50, rs=2.0 ** 20, cs=2.0 ** 22)
    check_planes(tpN, 70, 50, *want_planes(x, np.full(70, 2.0 ** 20)), 'tpN')
    check_planes(tpT, 50, 70, *want_planes(x.T, np.full(50, 2.0 ** 22)), 'tpT')


def test_split2_rowmap():
    """Logical row i = physical row rowmap[i], -1 = a zero row; rows of src the map does not name hold NaN.  rowmap2 takes
    over from column col2 on (a multiple of 64, as the callers pass: Hp of a bidirectional layer)."""
    rng = np.random.default_rng(9)
    rows, K, ld, phys = 70, 128, 132, 90
    src = split_source(rng, phys, K, ld)
    m1 = rng.permutation(phys)[:rows].astype(np.int32)
    m2 = rng.permutation(phys)[:rows].astype(np.int32)
    m1[::6] = -1
    m2[3::6] = -1
    for r in set(range(phys)) - set(m1.tolist()) - set(m2.tolist()):
        src[r] = np.nan

    def gather(m, cols):
        return np.where((m >= 0)[:, None], src[np.maximum(m, 0)][:, cols], F32(0))
    for maps, col2 in (((m1, None), 0), ((m1, m2), 64)):
        x = gather(m1, slice(0, K))
        if maps[1] is not None:
            x[:, col2:] = gather(m2, slice(col2, K))
            src2 = src
        else:
            src2 = src.copy()
            for r in set(m2.tolist()) - set(m1.tolist()) - {-1}:
                src2[r] = np.nan
        rs, _ = R.scale_model(R.line_max(x, 1))
        cs, _ = R.scale_model(R.line_max(x, 0))
        tpN, tpT, colpart = H.tph_split2(src2, rows, K, row_scale=rs, col_scale=cs, rowmap=maps[0], rowmap2=maps[1], col2=col2)
        check_planes(tpN, rows, K, *want_planes(x, rs), 'tpN')
        check_planes(tpT, K, rows, *want_planes(x.T, cs), 'tpT')
        out = H.colsum_parts(colpart, K)
        err = np.abs(out[:K].astype(np.float64) - x.astype(np.float64).sum(axis=0))
        assert np.all(err <= R.f32_bound(x.T, np.ones((1, rows)), rows, colpart.shape[0])[:, 0])


# ------------------------------------------------------------------ reductions
@pytest.mark.parametrize('R_', [1, 31, 33, 130])
def test_colsum(R_):
    rng = np.random.default_rng(R_)
    for N in (4, 60, 68):
        for precision in (False, True):
            src = split_source(rng, R_, N, N + 4, precision)
            out = H.colsum(src, R_, N)
            assert np.all(H.untouched(out[N:]))
            x = src[:, :N]
            err = np.abs(out[:N].astype(np.float64) - x.astype(np.float64).sum(axis=0))
            assert np.all(err <= R.f32_bound(x.T, np.ones((1, R_)), R_, 32)[:, 0]) and (precision or np.all(err == 0))


def test_reduce_slabs():
    rng = np.random.default_rng(21)
    for S, shape in ((1, (4, 4)), (3, (36, 68)), (5, (130, 20))):
        for precision in (False, True):
            slabs = np.stack([split_source(rng, shape[0], shape[1], shape[1], precision) for _ in range(S)])
            out = H.reduce_slabs(slabs)
            n = shape[0] * shape[1]
            assert np.all(H.untouched(out[n:]))
            flat = slabs.reshape(S, n)
            err = np.abs(out[:n].astype(np.float64) - flat.astype(np.float64).sum(axis=0))
            assert np.all(err <= R.f32_bound(flat.T, np.ones((1, S)), S, 1)[:, 0]) and (precision or np.all(err == 0))


def test_reduce_slabs_rows():
    """out[map[m]] = sum of the slabs' row m; rows with map[m] == -1 are dropped, rows nobody names and the columns [N, ldc)
    keep the pre-fill."""
    rng = np.random.default_rng(22)
    for S, M, N in ((1, 4, 4), (3, 36, 68), (5, 130, 20)):
        for precision in (False, True):
            slabs = np.stack([split_source(rng, M, N, N, precision) for _ in range(S)])
            rowmap = rng.permutation(M + 5)[:M].astype(np.int32)
            rowmap[::4] = -1
            out = H.reduce_slabs_rows(slabs, N + 4, rowmap, M + 5)
            want, mask = H.expected_buffer(slabs.astype(np.float64).sum(axis=0), rowmap, M + 5, N + 4)
            bound, _ = H.expected_buffer(R.f32_bound(slabs.reshape(S, -1).T, np.ones((1, S)), S, 1)[:, 0].reshape(M, N), rowmap, M + 5, N + 4)
            assert np.array_equal(H.untouched(out), ~mask)
            err = np.abs(out[mask].astype(np.float64) - want[mask])
            assert np.all(err <= bound[mask]) and (precision or np.all(err == 0))
