"""GPU: every route into a stream session computes what the commit before their merge computed, BIT FOR BIT.  Frames or
samples, with or without a look-ahead: the four feeds share one plan (a session without look-ahead is R = 0), one runner
(upload, operand-image rebuild, pass, fetch, advance; csrc/nasr_stream.hip) and one pair of state kernels
(stream_load_state_kernel with the direction in blockIdx.y, stream_save_state_kernel with the feed's per-slot counts by
value; csrc/lstm.hip).  None of that may move a bit: after every feed the rows each slot emitted (logits[:rows[b], b]; the
other rows are unspecified), stream_state(), stream_frames() and the row counts are compared by SHA-256 with
tests/golden/stream_parent.json, recorded on an MI355X from the parent commit (tests/golden/make_stream_parent_golden.py;
floats digested as float32(x + 0.0), so the sign of an exact zero does not count).  A mismatch is a bug in the shared code,
not a reason to regenerate.  There are no tolerances.

The cases are the smallest that reach each merged place: a chunk longer than every slot's rows (the caller's Tc, not the
longest slot's, decides how the bulk GEMMs split their sums), a chunk of idle slots, a reset between feeds, two M tiles
with padded slots, padded units (H 70 of Hp 128), set_params between two feeds with the persistent recurrence in use (the
session rebuilds the per-step operand images), feeds that only hold, a slot that gets fewer rows than it holds, an
utterance shorter than the look-ahead, `last` without rows or samples, Tc = 0 on the samples route, a reused slot."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_stream_parent_golden as G  # noqa: E402

pytestmark = [pytest.mark.gpu]

KEYS = ('rows_digest', 'frames_digest', 'logits', 'state')


@pytest.fixture(scope='module')
def golden():
    with open(G.OUT) as f:
        return json.load(f)


@pytest.mark.parametrize('case', G.CASES, ids=G.case_id)
def test_every_feed_keeps_the_parents_bits(case, golden):
    got, want = G.run_case(case), golden[G.case_id(case)]
    for k, (g, w) in enumerate(zip(got['feeds'], want['feeds'])):
        print(G.case_id(case), 'feed', k, 'rows', g['rows'], 'parent', w['rows'], 'frames', g['frames'], 'parent', w['frames'],
              'sum|logits|', g['logits_abs_sum'], 'parent', w['logits_abs_sum'])
    # the recorded recurrence mode decides whether the session rebuilds the operand images itself: another mode is another test
    assert got['mode'] == want['mode']
    assert len(got['feeds']) == len(want['feeds'])
    for k, (g, w) in enumerate(zip(got['feeds'], want['feeds'])):
        assert g['rows'] == w['rows'] and g['frames'] == w['frames'] and g['T_out'] == w['T_out'], k
        for key in KEYS:
            assert g[key] == w[key], (k, key)
