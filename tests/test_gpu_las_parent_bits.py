"""GPU: the LAS training pass and beam search compute what the commit before their shared decoder step computed, BIT FOR
BIT.  Both run one host function for the decoder step (las_decoder_step, csrc/nasr_las.hip), one attention kernel
(las_attend_kernel, csrc/las.hip: row r attends over utterance r / W, rows >= nrows get a zero context, alpha and the done
word optional), one final-state gather and one wave_sum (csrc/las.h).  None of that may move a bit: loss, nll, the flat
gradient, the logits, the fed ids and the sampled flags of every training case, and ids, scores, words, parents, log-probs,
lengths, finished flags, step count and n-gram contexts of every search, are compared by SHA-256 with
tests/golden/las_parent.json, recorded on an MI355X from the parent commit (tests/golden/make_las_parent_golden.py; floats
digested as float32(x + 0.0), so the sign of an exact zero does not count).  A mismatch is a bug in the shared code, not a
reason to regenerate.  There are no tolerances.

The cases are the smallest that reach each place the shared code can go wrong: fewer frames than the attention kernel's
four waves (L4 2), L4 no multiple of four (14), one and two blocks of 16 padded rows, every step fed a sample (the fed ids
hang on the logits' bits); searches with nrows 4 and 15 of R 16, nrows = R, nrows 18 of R 32 with an order-2 table, W = 1,
and one that ends after 3 of 20 steps, where the done word is raised inside a chunk of eight enqueued steps and the
chunk's remaining attention launches return at once."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_las_parent_golden as G  # noqa: E402

pytestmark = [pytest.mark.gpu]


@pytest.fixture(scope='module')
def golden():
    with open(G.OUT) as f:
        return json.load(f)


@pytest.mark.parametrize('case', G.TRAIN, ids=G.train_id)
def test_training_pass_keeps_the_parents_bits(case, golden):
    e, got = G.run_train(case)
    e.close()
    want = golden[G.train_id(case)]
    print(G.train_id(case), 'loss', got['loss_value'], 'parent', want['loss_value'], 'grad norm', got['grad_norm'], 'parent',
          want['grad_norm'], 'samples', got['samples'], 'parent', want['samples'])
    for k in ('loss', 'nll', 'logits', 'fed_ids', 'sampled', 'grads'):
        assert got[k] == want[k], k


@pytest.mark.parametrize('case', G.SEARCH, ids=G.search_id)
def test_beam_search_keeps_the_parents_bits(case, golden):
    e, got = G.run_search(case)
    e.close()
    want = golden[G.search_id(case)]
    print(G.search_id(case), 'steps', got['steps'], 'parent', want['steps'], 'best', got['best'], 'parent', want['best'],
          'its score', got['best_score'], 'parent', want['best_score'])
    if case[7]:   # the early end: inside a chunk of eight steps
        assert got['steps'] < case[5] and got['steps'] % 8 != 0
    assert got['steps'] == want['steps']
    for k in G.BEAM_KEYS + (('lm_context',) if case[6] else ()):
        assert got[k] == want[k], k
