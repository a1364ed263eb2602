"""GPU: every route out of the feature front end computes what the commit before the front end was split computed, BIT FOR
BIT.  The kernels and their launchers stand in csrc/mfcc.hip behind csrc/mfcc.h, the featurizer handle in csrc/nasr_fz.hip,
and one normalise kernel (mfcc_norm_kernel<RULE, FORM>) serves the whole-utterance and the causal rule, the stacked rows
and the batch slot's centre frames.  None of that may move a bit: the features and their (mean, std) pairs of compute(), the
samples of resample() and augment_audio(), the logits of batches given as audio (upload_batch_audio, both rules) and of a
stream session fed samples are compared by SHA-256 with tests/golden/frontend_parent.json, recorded on an MI355X from the
parent commit (tests/golden/make_frontend_parent_golden.py; float32 bytes, the statistics as float64 bytes).  A mismatch is
a bug in the code, not a reason to regenerate.  There are no tolerances.

The cases (all at 8 kHz: frames of 200 samples, 80 apart): five configurations - MFCC with numcontext 2 and 0, log-mel
filterbank with two delta levels, the causal rule with norm_min_frames 5 and 50 - each over one call of utterances of 1, 200
and 201 samples and of 2 to 6, 49 to 51, 256, 257 and 513 frames, one of them exact zeros; four utterances at 8000, 16000,
11025 and 44100 Hz, and all four at 8000 Hz; reverberation and noise from banks of two; batches of three with a 1-frame
utterance last; a stream session of two slots fed 100, 700 and 2200 samples, one ended by `last` on its final piece and one
by an empty `last` feed."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
import make_frontend_parent_golden as G  # noqa: E402

pytestmark = [pytest.mark.gpu]


@pytest.fixture(scope='module')
def golden():
    with open(G.OUT) as f:
        return json.load(f)


@pytest.mark.parametrize('case', G.CASES, ids=G.case_id)
def test_the_front_end_keeps_the_parents_bits(case, golden):
    got, want = G.run_case(case), golden[G.case_id(case)]
    print(G.case_id(case), 'sum|.|', got['abs_sum'], 'parent', want['abs_sum'],
          {k: (v, want.get(k)) for k, v in got.items() if k in ('frames', 'samples', 'seq_len', 'T', 'rows')})
    assert sorted(got) == sorted(want)
    for key in sorted(got):
        if key != 'abs_sum':                      # (a float printed for the reader; the digests are the check)
            assert got[key] == want[key], key
