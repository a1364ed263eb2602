"""gemm_tph_kernel's k-loop and epilogue were restructured (csrc/gemm_tph.hip: the fragments of a step's second k-block are
read from LDS among the MFMAs of its first; the epilogue loads its scales ahead of straight-line stores) WITHOUT changing a
bit of any result: per accumulator the products are still x1 y0, x0 y1, x0 y0 over ascending k-blocks.

test_keeps_the_parents_bits: every instantiation on operands with full 24-bit significands, hashed (SHA-256) and compared
with tests/golden/gemm_tph_parent.json, recorded on an MI355X from the parent commit by tests/golden/make_gemm_tph_golden.py
(cases and digest come from there).  The integer operands of test_gpu_gemm_kernels.py cannot see a changed summation order;
these can.  A mismatch is a bug in the kernel: the fixture is never regenerated to make it pass.

test_repeated_launches_are_exact: a screen for a race between the operand DMA, the barrier and the fragment reads of the
loop.  One integer-operand shape per instantiation with >= 32 workgroups and six steps per slice, launched 30 times; every
output must be bitwise the fp64 result.  A wrong tile here is a race in the loop - found by reading the wait and barrier
placement, not by running this again."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_gemm_tph_golden as G  # noqa: E402

import gemm_ref as R  # noqa: E402
import kernel_harness as H  # noqa: E402
import test_gpu_gemm_kernels as K  # noqa: E402  (tph_case, check_exact, make_c_map: the exact regime's helpers)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def golden():
    with open(G.OUT) as f:
        return json.load(f)


@pytest.mark.parametrize('mode', sorted(G.MODES))
def test_keeps_the_parents_bits(mode, golden):
    bad = []
    for name, p in G.mode_cases(mode):
        want, got = golden[G.case_id(mode, name)], G.record(G.run_case(mode, name, p))
        print(G.case_id(mode, name), got['sha256'][:16], want['sha256'][:16], got['max_abs'], want['max_abs'])
        if got['sha256'] != want['sha256']:
            bad.append(name)
    assert not bad, f'{mode}: results differ from the parent commit in {bad}'


REPEATS = 30
# 1024 x 2048 x 176: 11 k-blocks = six steps (the last k-block missing); 4 x 8 tiles of 256 x 256, 6 x 8 of 192 x 256,
# 8 x 11 of 128 x 192
REPEAT_MODES = {
    't256': ('t256', False), 't192': ('t192', False), 'side': ('side', False),
    't256_cmap': ('t256', True), 't192_cmap': ('t192', True),
}


@pytest.mark.parametrize('inst', sorted(REPEAT_MODES))
def test_repeated_launches_are_exact(inst):
    mode, cmap = REPEAT_MODES[inst]
    M, N, Kd = 1024, 2048, 176
    kw = dict(c_map=K.make_c_map(M), c_rows=M + 8) if cmap else {}
    c = K.tph_case(M, N, Kd, mode, **kw)
    tm, tn = (128, 192) if c.side else (c.tile_rows, 256)
    assert -(-M // tm) * -(-N // tn) >= 32 and (-(-Kd // 16) + 1) // 2 >= 5
    C64, rows = R.gemm_ref(c)
    planes = H.tph_planes(c, poison=True)
    first = None
    for i in range(REPEATS):
        out, _ = H.gemm_tph(c, planes)
        if first is None:
            K.check_exact(out, C64[0], rows, c.c_rows, c.ldc, f'{inst} launch 0')
            first = out
        elif not np.array_equal(out.view(np.uint32), first.view(np.uint32)):
            K.check_exact(out, C64[0], rows, c.c_rows, c.ldc, f'{inst} launch {i}')
            pytest.fail(f'{inst}: launch {i} differs from launch 0, which was exact')
