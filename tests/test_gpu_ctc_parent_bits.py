"""GPU: the CTC kernels of csrc/ctc.hip compute what the commit before its four lattice walks came to share one state
set-up, one forward and one backward step, one column rescale and one final-column epilogue computed, BIT FOR BIT.  Loss
path: every instantiation (label-array widths 31 .. 511, KS 2 .. 8, 12, 16) of the engineered lattice (C 29) and of the plain
one (C 40) on the batch, parameters and engine of test_gpu_ctc_lattice.py, and the projection scaled by 60 at the widths 224
and 511 (paths die there and the rescale meets NEG): the loss, the per-utterance nll, the flat gradient and the greedy ids.
Alignment: Engine.align_logits on seeded integer-valued and float logits, every instantiation with the back-pointers in LDS
and in the global workspace (asserted with Engine.align_in_lds): the paths and the fp64 scores.  All are compared by SHA-256
with tests/golden/ctc_parent.json, recorded on an MI355X from the parent commit (tests/golden/make_ctc_parent_golden.py,
which ran every case twice, each on a fresh engine, and kept only those whose runs agreed; floats digested as
float32(x + 0.0), so the sign of an exact zero does not count).  A mismatch is a bug in the code, not a reason to
regenerate.  There are no tolerances."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_ctc_parent_golden as G  # noqa: E402

pytestmark = [pytest.mark.gpu]


@pytest.fixture(scope='module')
def golden():
    with open(G.OUT) as f:
        return json.load(f)


@pytest.mark.parametrize('case', G.CASES, ids=G.case_id)
def test_the_ctc_kernels_keep_the_parents_bits(case, golden):
    got, want = G.run_case(case), golden[G.case_id(case)]
    print(G.case_id(case), {k: (got[k][:12], want[k][:12]) for k in sorted(want)})
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        assert got[key] == want[key], key
