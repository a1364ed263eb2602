"""The recurrence kernels, called directly through tests/kernel_harness (the code objects of libnasr.so), against the fp64
reference and error model of tests/rec_ref.py - step by step from the kernel's own previous state (forward), along an
fp64 trajectory with the bound carried (forward while the bound stays below 2^-10, BPTT always).

Launchers of csrc/kernels.h covered, each in the order the library calls it (nasr_pass.hip / nasr_rec.hip):
  lstm.hip          launch_repack_u, launch_lstm_fwd_step (NQ = 1, 2, 4, 8, 16 and the generic form at Hp 576 / 640),
                    launch_lstm_fwd_step_carry behind launch_stream_load_state, lstm_bwd_partials (inside the harness), launch_lstm_bwd_step
                    (KSP = 2, 4, 8, 16, the generic form at Hp 576, the two-launch form at Hp 640 / 1024)
  lstm_persist.hip  persist_supported, persist_prepare, persist_image_floats, persist_xch_floats, persist_hx_bytes,
                    persist_px_bytes, launch_repack_persist (fp32 and fp16-plane images, behind launch_tph_scales_batch),
                    launch_lstm_persist_fwd (fp16 planes and cinv == NULL, every NU = 2 .. 16), launch_lstm_persist_bwd
                    (every NU, plain and lean, with and without rowpart / colpart), persist_dgmax_floats
  lstm_wide.hip     wide_supported, wide_prepare, wide_image_bytes, wide_hx_bytes, wide_part_bytes, launch_repack_wide
                    behind launch_tph_scales_batch (both scale sets), launch_lstm_wide_fwd (one launch per direction,
                    MT = 1 and 2), launch_repack_wide_bwd, launch_wide_row_scales, wide_px_bytes, launch_lstm_wide_bwd
The state and window helpers of the stream sessions have their own tests.

Every float of every output buffer is accounted for: within the bound of the fp64 value, exactly +0 where the file
headers promise zero, or the untouched fill pattern (rec_ref.check_forward / check_backward state the contract).  Inputs
hold 1e30 in the rows b >= B and in the frames past seq_len; none of it may reach a valid output.  `pytest -s` prints the
largest ratio of every case."""
import numpy as np
import pytest

import kernel_harness as H
import rec_ref as R

pytestmark = pytest.mark.gpu

CASES = R.cases()
FILL_BITS = np.uint32(int.from_bytes(bytes([H.FILL] * 4), 'little'))


def _run(case):
    kind = R.KINDS[case.path]
    inp = R.make_inputs(case)
    if kind.bwd:
        return H.lstm_backward(case.path, inp, lean=case.lean, parts=case.parts)
    return H.lstm_forward(case.path, inp)


@pytest.mark.parametrize('case', CASES, ids=lambda c: c.id)
def test_recurrence_kernel_against_fp64(case):
    kind = R.KINDS[case.path]
    inp = R.make_inputs(case)
    got = _run(case)          # a non-zero error / sticky / fault word raises
    if kind.bwd:
        dg, rp, cp = got
        r = R.check_backward(kind, inp, dg, rp, cp)
        print(f'\n{case.path:14s} {case.regime:9s} {case.id}: running {r["running"]:.3f}')
        assert not r['problems'], r['problems']
        assert r['running'] <= 1, r
        if rp is not None:    # the parts nobody writes: member CUs' rows of padded unit slots do not exist; all are written
            assert not H.untouched(rp).any() and not H.untouched(cp).any()
        return
    act, c, h = got
    r = R.check_forward(kind, inp, act, c, h, FILL_BITS)
    run = 'n/a (bound %.1e)' % r['running_bound'] if r['running'] is None else '%.3f' % r['running']
    print(f'\n{case.path:14s} {case.regime:9s} {case.id}: local {r["local"]:.3f} running {run}')
    v = inp['valid']
    assert np.isfinite(act[v]).all() and np.isfinite(c[v]).all() and np.isfinite(h).all()
    assert not r['problems'], r['problems']
    assert r['local'] <= 1, r
    if case.regime in ('init', 'sat'):
        assert r['running'] is not None and r['running_bound'] <= R.RUNNING_LIMIT
    assert r['running'] is None or r['running'] <= 1, r


@pytest.mark.parametrize('path', sorted(R.KINDS))
def test_two_runs_give_identical_bytes(path):
    case = next(c for c in CASES if c.path == path)
    a, b = _run(case), _run(case)
    for x, y in zip(a, b):
        assert (x is None and y is None) or np.array_equal(R._bits(x), R._bits(y))


def test_harness_refuses_what_the_kernels_cannot_take():
    case = CASES[0]
    inp = dict(R.make_inputs(case))
    sq = np.array(inp['seq_len'])
    sq[case.B] = 1                                  # a padded row with a length
    with pytest.raises(RuntimeError, match='refused'):
        H.lstm_forward('step_fwd', dict(inp, seq_len=sq))
    sq = np.array(inp['seq_len'])
    sq[0] = case.T + 1
    with pytest.raises(RuntimeError, match='refused'):
        H.lstm_forward('persist_fwd32', dict(inp, seq_len=sq))
    with pytest.raises(RuntimeError, match='refused'):
        H.lstm_forward('step_fwd', dict(inp, H=case.Hp + 1))
