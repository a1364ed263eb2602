"""Builds neuralasr_amd/libnasr.so (the HIP kernels + C ABI of include/nasr.h) for gfx950 with hipcc.
In-tree, explicit `hipcc -shared -fPIC`; cross-compiles without a GPU.  `python -m neuralasr_amd.build`.
Also neuralasr_amd/libnasr_kt.so: the kernel tests' entry points (tests/kernel_harness/harness.hip for the GEMM layer,
rec_harness.hip for the recurrence, ctc_harness.hip for the CTC kernels) over the very gemm.o / gemm_tph.o / optim.o /
lstm.o / lstm_persist.o / lstm_wide.o / ctc.o objects of libnasr.so."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, 'csrc')
LIB = os.path.join(HERE, 'libnasr.so')
KT_LIB = os.path.join(HERE, 'libnasr_kt.so')
KT_DIR = os.path.join(HERE, '..', 'tests', 'kernel_harness')
KT_SRCS = ['harness.hip', 'rec_harness.hip', 'ctc_harness.hip']
KT_HEADERS = [os.path.join(KT_DIR, 'arena.h')]
# the objects of libnasr.so the kernel tests link against (optim.o also holds test_hook(), which the recurrence launchers call)
KT_OBJS = ['gemm.o', 'gemm_tph.o', 'optim.o', 'lstm.o', 'lstm_persist.o', 'lstm_wide.o', 'ctc.o']
SOURCES = ['gemm.hip', 'gemm_tph.hip', 'lstm.hip', 'rows.hip', 'lstm_persist.hip', 'lstm_wide.hip', 'ctc.hip', 'dense.hip', 'optim.hip', 'nasr_layout.hip',
           'nasr_rec.hip', 'nasr_batch.hip', 'nasr_pass.hip', 'nasr_stream.hip', 'nasr_lstm.hip', 'nasr_api.hip', 'nasr_distill.hip', 'nasr_comm.hip', 'beam.cpp',
           'wavenet.hip', 'nasr_wavenet.hip', 'las.hip', 'las_beam.hip', 'nasr_las.hip', 'mfcc.hip', 'nasr_fz.hip', 'resample.hip', 'wave_aug.hip']
HEADERS = [os.path.join(CSRC, 'kernels.h'), os.path.join(CSRC, 'dispatch.h'), os.path.join(CSRC, 'lstm_device.h'), os.path.join(CSRC, 'nasr_ctx.h'), os.path.join(CSRC, 'nasr_lstm.h'), os.path.join(CSRC, 'wavenet.h'), os.path.join(CSRC, 'las.h'), os.path.join(CSRC, 'las_beam.h'), os.path.join(CSRC, 'resample.h'), os.path.join(CSRC, 'wave_aug.h'),
           os.path.join(CSRC, 'mfcc.h'), os.path.join(CSRC, 'nasr_fz.h'), os.path.join(HERE, '..', 'include', 'nasr.h')]
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function']
# wave_aug.hip: the FIR's 8 x 8 register window is plain v_fmac_f32; the SLP vectoriser would pack pairs of them into
# v_pk_fma_f32, which runs at the same rate on gfx950 and needs a v_mov per misaligned pair
EXTRA_FLAGS = {'wave_aug.hip': ['-fno-slp-vectorize']}


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return 'hipcc'


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force=False, verbose=False):
    hipcc = _hipcc()
    bdir = os.path.join(HERE, 'build')
    os.makedirs(bdir, exist_ok=True)
    jobs = []
    objs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(bdir, os.path.splitext(s)[0] + '.o')
        objs.append(obj)
        if force or _stale(obj, [src] + HEADERS):
            jobs.append([hipcc] + FLAGS + EXTRA_FLAGS.get(s, []) + ['-c', src, '-o', obj])

    def run(cmd):
        if verbose:
            print(' '.join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError('hipcc failed:\n' + ' '.join(cmd) + '\n' + r.stdout + r.stderr)
        if verbose and r.stderr.strip():
            print(r.stderr)

    kt_objs = []
    for s in KT_SRCS:
        src = os.path.join(KT_DIR, s)
        obj = os.path.join(bdir, 'kt_' + os.path.splitext(s)[0] + '.o')
        kt_objs.append(obj)
        if force or _stale(obj, [src] + KT_HEADERS + HEADERS):
            jobs.append([hipcc] + FLAGS + ['-c', src, '-o', obj])

    with ThreadPoolExecutor(max_workers=min(4, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(LIB, objs):
        run([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs + ['-lpthread'])
    kt_objs += [os.path.join(bdir, o) for o in KT_OBJS]
    if force or jobs or _stale(KT_LIB, kt_objs):
        run([hipcc, '--offload-arch=gfx950', '-shared', '-fPIC', '-o', KT_LIB] + kt_objs)
    return LIB


if __name__ == '__main__':
    print(build(force='--force' in sys.argv, verbose=True))
