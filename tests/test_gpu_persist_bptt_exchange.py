"""GPU: the persistent BPTT kernel (lstm_persist_bwd_kernel, csrc/lstm_persist.hip) computes what the commit before its
16-byte exchange loads computed, BIT FOR BIT.  The kernel reads the 32 producers' partial rows as eight dwordx4 loads per
lane and reduces them across the four lane groups in the order the 4-byte form used ((s0 + s1) + (s2 + s3), each s_g the
producers g, g + 4, ... summed from zero); tanh(c) comes from the memory wave.  None of that may move
a bit: loss, nll and the flat gradient of every case are compared by SHA-256 with tests/golden/persist_bptt_parent.json,
recorded on an MI355X from the parent commit (tests/golden/make_persist_bptt_golden.py; digests of float32(x + 0.0), so the
sign of an exact zero does not count).  A mismatch is a bug in the kernel's summation order, not a reason to regenerate.

The cases are the smallest that reach every part: every NU instantiation (Hp 64 ... 512), a partly filled 16-byte row set
(H 180, 300), B 1 / 5 / 16 / 19 bidirectional (two rounds) / 40 unidirectional (two rounds: the flag barrier between
rounds), ragged lengths with one utterance of about T/3 (masked timesteps; the first valid BPTT timestep far into the launch),
two layers.  Each case also agrees with the per-timestep kernels at the tolerances of tests/test_gpu_persist.py and gives
identical bytes twice."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_persist_bptt_golden as G  # noqa: E402

pytestmark = [pytest.mark.gpu]


@pytest.fixture(scope='module')
def golden():
    with open(G.OUT) as f:
        return json.load(f)


@pytest.mark.parametrize('case', G.CASES, ids=G.case_id)
def test_persistent_bptt_keeps_the_parents_bits(case, golden):
    e, batch, loss, nll, grads = G.run_case(case)
    try:
        assert e.recurrence_mode == 'persistent'
        # twice: identical bytes
        loss2, nll2, grads2 = e.loss_and_grads(*batch)
        assert e.recurrence_mode == 'persistent' and e.persist_stats()[0] == 0
        assert np.float32(loss).tobytes() == np.float32(loss2).tobytes()
        assert nll.tobytes() == nll2.tobytes()
        assert grads.tobytes() == grads2.tobytes()
        assert np.isfinite(grads).all() and np.isfinite(loss)

        # the parent commit's bits
        want, got = golden[G.case_id(case)], G.record(loss, nll, grads)
        print(G.case_id(case), 'loss', got['loss_value'], 'parent', want['loss_value'], 'grad norm', got['grad_norm'],
              'parent', want['grad_norm'])
        assert got['loss'] == want['loss']
        assert got['nll'] == want['nll']
        assert got['grads'] == want['grads']

        # the per-timestep kernels on the same step (tolerances of tests/test_gpu_persist.py)
        e.set_recurrence_mode(False)
        assert e.recurrence_mode == 'per-step'
        loss_s, nll_s, grads_s = e.loss_and_grads(*batch)
        assert loss == pytest.approx(loss_s, rel=2e-6)
        assert np.linalg.norm(grads - grads_s) <= 2e-5 * np.linalg.norm(grads_s)
    finally:
        e.close()
