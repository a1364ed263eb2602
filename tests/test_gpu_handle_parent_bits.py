"""GPU: the handle computes what the commit before the LSTM family's state moved out of nasr_ctx into LstmState
(csrc/nasr_lstm.h) computed, BIT FOR BIT, on the paths the other parent fixtures do not reach: the persistent kind with the
weight-gradient side stream and the deferred bucket events switched on and off, the narrow persistent kind, row compaction
on and off in the handle's own recurrence mode and on the per-step kernels, the literal stack_reshape net, a
DeepSpeech-shaped net with dropout, the wide kind, a WaveNet handle with its batch-norm state, a staged and committed step
with its published results and logits, gradient clipping, and forced alignment.  The logits, the loss, the per-utterance nll,
the flat gradient, the loss of two train_steps and the parameters and Adam state after them are compared by SHA-256 with
tests/golden/handle_parent.json, recorded on an MI355X from the parent commit (tests/golden/make_handle_parent_golden.py,
which ran every case twice and kept only those whose runs agreed; floats digested as float32(x + 0.0), so the sign of an
exact zero does not count).  The recurrence mode, the recurrence launches of every pass, the rows a pass covered and what
the setters answered are compared in plain: a moved member changes no launch and no message.  A mismatch is a bug in the
code, not a reason to regenerate.  There are no tolerances."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_handle_parent_golden as G  # noqa: E402

pytestmark = [pytest.mark.gpu]


@pytest.fixture(scope='module')
def golden():
    with open(G.OUT) as f:
        return json.load(f)


@pytest.mark.parametrize('case', G.CASES, ids=G.case_id)
def test_the_handle_keeps_the_parents_bits(case, golden):
    got, want = G.run_case(case), golden[G.case_id(case)]
    print(G.case_id(case), 'mode', got['mode'], 'parent', want['mode'], 'launches', got['launches'], got['launches_step'], 'parent',
          want['launches'], want['launches_step'], 'sum|logits|', got['logits_abs_sum'], 'parent', want['logits_abs_sum'],
          'sum|grads|', got['grads_abs_sum'], 'parent', want['grads_abs_sum'], 'losses', got['step_losses'], 'parent',
          want['step_losses'])
    # the recorded recurrence mode decides which kernels ran: another mode is another test
    assert got['mode'] == want['mode']
    assert sorted(got) == sorted(want)
    for key in sorted(want):          # digests and plain values alike: every key of the record, the variants' included
        assert got[key] == want[key], key
