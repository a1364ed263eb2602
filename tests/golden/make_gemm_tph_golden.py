"""Generates tests/golden/gemm_tph_parent.json: SHA-256 digests of what launch_gemm_tph writes for the cases below, through
the kernel harness (tests/kernel_harness -> libnasr_kt.so) on operands with full 24-bit significands (gemm_ref.precision_matrix,
the generator of gemm_ref.PRECISION_CASES).  tests/test_gpu_gemm_tph_parent_bits.py runs the same cases and compares.

The exact tests of tests/test_gpu_gemm_kernels.py use small integers, whose sums are exact in any order; on these operands
every change of the summation order inside gemm_tph_kernel - the order of the three products of an accumulator, of the
k-blocks, of the split-K slices - changes result bits.  Run it on an MI355X with the commit BEFORE a change to the k-loop
built (`python tests/golden/make_gemm_tph_golden.py [out.json [libnasr_kt.so]]`); a change that claims to keep every bit is
then measured against what that commit computed.  A mismatch is fixed in the kernel, never by running this again.

Only data is written: digests, and per case the largest magnitude of the result (a reader of a failing test sees the scale).

The planes are built on the host (kernel_harness.tph_planes), so nothing but the GEMM and its slab reduction is hashed."""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
OUT = os.path.join(HERE, 'gemm_tph_parent.json')
if TESTS not in sys.path:
    sys.path.insert(0, TESTS)

import gemm_ref as R  # noqa: E402
import kernel_harness as H  # noqa: E402

# instantiation -> launch_gemm_tph's choice: <4,2,4>, <3,2,4>, <4,1,3>, <4,2,4,CMAP>, <3,2,4,CMAP>
MODES = {
    't256': dict(tile_rows=256), 't192': dict(tile_rows=192), 'side': dict(side=True),
    't256_cmap': dict(tile_rows=256, c_map=True), 't192_cmap': dict(tile_rows=192, c_map=True),
}
SIZES = (36, 68, 196, 260)
# K -> steps of two k-blocks: 16: one, its second k-block missing; 32: one; 48: two, the last half missing; 96: three;
# 112: four, the last half missing
KS = (16, 32, 48, 96, 112)


def mode_cases(mode):
    """[(name, dict)] of one instantiation: the smallest shapes that reach every path of the k-loop - prologue only, prologue
    + last step, one and two turns of the steady-state loop, the missing second k-block, split-K slices with an odd tail
    (1040 = 65 k-blocks: 22 + 22 + 21), two batches with opposite shifts, operands of unequal k extent, and M, N below,
    between and above the row-block and tile edges."""
    mi = sorted(MODES).index(mode)
    cmap = 'cmap' in mode
    out = []
    for i, K in enumerate(KS):
        M, N = SIZES[(i + mi) % 4], SIZES[(i + 2 * mi + 1) % 4]
        out.append((f'{M}x{N}x{K}', dict(M=M, N=N, K=K)))
    out.append(('260x260x96', dict(M=260, N=260, K=96)))
    out.append(('196x68x1040', dict(M=196, N=68, K=1040)))
    out.append(('196x68x1040_split3', dict(M=196, N=68, K=1040, split_k=3)))
    out.append(('68x36x112_KA48', dict(M=68, N=36, K=112, KA=48)))
    out.append(('36x196x112_KB32', dict(M=36, N=196, K=112, KB=32)))
    if not cmap:            # GemmTPHDesc: c_map goes with one batch only
        out.append(('36x68x112_batch2', dict(M=36, N=68, K=112, nbatch=2, a_kshift=-16, a_kshift1=16)))
        out.append(('196x260x1040_batch2_split3', dict(M=196, N=260, K=1040, nbatch=2, a_kshift=-16, a_kshift1=16, split_k=3)))
    return out


def case_id(mode, name):
    return f'{mode}/{name}'


def make_case(mode, name, p):
    """The TphCase: deterministic in (mode, name)."""
    seed = int.from_bytes(hashlib.sha256(case_id(mode, name).encode()).digest()[:4], 'little')
    rng = np.random.default_rng(seed)
    M, N, K = p['M'], p['N'], p['K']
    nb = p.get('nbatch', 1)
    A = [R.precision_matrix(rng, M, p.get('KA', K), 30, zero_row=1, zero_col=2) for _ in range(nb)]
    B = [R.precision_matrix(rng, N, p.get('KB', K), 30, zero_row=3) for _ in range(nb)]
    m = MODES[mode]
    c_map, c_rows = None, M
    if m.get('c_map'):
        c_rows = M + 8
        c_map = rng.permutation(c_rows)[:M].astype(np.int32)
        c_map[::7] = -1
    return R.TphCase(A=A, B=B, M=M, N=N, K=K, ldc=N, c_rows=c_rows, a_kshift=p.get('a_kshift', 0), a_kshift1=p.get('a_kshift1', 0),
                     split_k=p.get('split_k', 1), tile_rows=m.get('tile_rows', 0), side=m.get('side', False), c_map=c_map, nbatch=nb)


def digest(x):
    """SHA-256 over the float32 bytes of x + 0.0: the sign of an exact zero does not count."""
    a = np.ascontiguousarray(np.asarray(x, np.float32) + np.float32(0.0))
    return hashlib.sha256(a.tobytes()).hexdigest()


def run_case(mode, name, p):
    """-> the whole C buffer launch_gemm_tph wrote into (both batches, the harness's pre-fill where nothing is written)."""
    out, _ = H.gemm_tph(make_case(mode, name, p))
    return out


def record(out):
    with np.errstate(invalid='ignore'):
        finite = out[np.isfinite(out) & ~H.untouched(out)]
    return {'sha256': digest(out), 'max_abs': float(np.max(np.abs(finite))) if finite.size else 0.0}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else OUT
    if len(sys.argv) > 2:
        H.KT_PATH = os.path.abspath(sys.argv[2])
    doc = {'_note': 'SHA-256 of float32(C + 0.0) bytes of launch_gemm_tph, taken on an MI355X from the commit before the '
                    'fragment prefetch in the k-loop of gemm_tph_kernel.  tests/golden/make_gemm_tph_golden.py'}
    for mode in sorted(MODES):
        for name, p in mode_cases(mode):
            doc[case_id(mode, name)] = record(run_case(mode, name, p))
            print(case_id(mode, name), doc[case_id(mode, name)]['sha256'][:16], flush=True)
    with open(out_path, 'w') as f:
        json.dump(doc, f, indent=1)
        f.write('\n')
    print('wrote', out_path)


if __name__ == '__main__':
    main()
