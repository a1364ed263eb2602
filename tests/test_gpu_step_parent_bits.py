"""GPU: every user of the per-timestep recurrence kernels computes what the commit before their driving loops were merged
computed, BIT FOR BIT.  A whole batch in the per-step mode (with and without the hipGraph replay), the windows of a chunked
batch and a stream feed share one runner of a window of steps and one load-carry kernel (csrc/lstm.hip), and one owner of
the per-step operand images (ensure_step_images, csrc/nasr_rec.hip).  None of that may move a bit: the logits, the loss,
the flat gradient, the loss of every train_step and the parameters and Adam state after them are compared by SHA-256 with
tests/golden/step_parent.json, recorded on an MI355X from the parent commit (tests/golden/make_step_parent_golden.py; floats
digested as float32(x + 0.0), so the sign of an exact zero does not count).  The recurrence launches of a pass are compared
in plain.  A mismatch is a bug in the shared code, not a reason to regenerate.  There are no tolerances.  (The stream-feed
route: tests/test_gpu_stream_parent_bits.py.)

The cases are the smallest that reach each merged place: ragged lengths with a 1-frame utterance, two directions and one,
padded units (H 70 of Hp 128) and two M tiles (B 17), graph mode off and on (the second step replays the cached graphs), the
generic NQ = 0 / KSP = 0 forms (H 576); chunked training with the persistent kind left as the handle's mode (the passes
rebuild the per-step operand images, again after set_params, and chunking off again leaves the handle's own kind as it was)
at (C, R) = (4, 3), (1, 2) - every window carries, dc enters the chain at step 0 - and (3, 7), and (8, 3) at T 6, one window
of W = T <= C rows; and H 640, the two-launch wide BPTT with a carried c0 (lstm_bwd_cell_carry_kernel)."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_step_parent_golden as G  # noqa: E402

pytestmark = [pytest.mark.gpu]

DIGESTS = ('logits', 'loss', 'nll', 'grads', 'params', 'adam_m', 'adam_v')
PLAIN = ('launches_grads', 'launches_step', 'launches_whole', 'adam_step', 'mode_after')


@pytest.fixture(scope='module')
def golden():
    with open(G.OUT) as f:
        return json.load(f)


@pytest.mark.parametrize('case', G.CASES, ids=G.case_id)
def test_every_step_keeps_the_parents_bits(case, golden):
    got, want = G.run_case(case), golden[G.case_id(case)]
    print(G.case_id(case), 'mode', got['mode'], 'parent', want['mode'], 'launches', got['launches_grads'], got['launches_step'],
          got.get('launches_whole'), 'parent', want['launches_grads'], want['launches_step'], want.get('launches_whole'),
          'sum|logits|', got['logits_abs_sum'], 'parent', want['logits_abs_sum'], 'sum|grads|', got['grads_abs_sum'], 'parent',
          want['grads_abs_sum'], 'losses', got['step_losses'], 'parent', want['step_losses'])
    # the recorded recurrence mode decides whether the chunked passes rebuild the operand images themselves: another mode is
    # another test
    assert got['mode'] == want['mode']
    for key in PLAIN:
        assert got.get(key) == want.get(key), key
    for key in DIGESTS:
        assert got[key] == want[key], key
    assert got['steps'] == want['steps']
