"""CPU: the inputs of tests/test_gpu_history.py (tests/history_ref.py).  Every batch a history or a probe uses passes the
library's own feasibility rule - also at frame skip 3 and in the windows of chunking 4 + 3 -, the family's fp64 reference
gives a finite loss on it with the probe's parameters, the two variants of a history differ in every feature value, and
the probe shapes have the residues and edges the GPU test names.

Needs the built library (python -m neuralasr_amd.build, or __graft_entry__.build()): the frame arithmetic it checks the
batches with (skip_frames, num_frames) is the library's own; no GPU."""
import numpy as np
import pytest

import history_ref as H
from neuralasr_amd.engine import skip_frames
from oracle import nasr_oracle as O

FAMILIES = list(H.TABLE)


def batches(f):
    """(name, variant, batch) of everything the family's histories and its probe feed"""
    out = [('probe', 0, f.probe_batch())]
    for name in f.batch_names():
        out += [(name, v, f.batch(name, v)) for v in H.VARIANTS]
    if 'audio' in f.histories:
        for v in H.VARIANTS:
            audios, seq, labels, ll, tm, fm = f.audio_batch(v)
            out.append(('audio', v, (None, seq, labels, ll)))
    return out


def test_the_table_is_the_families():
    assert sorted(H.CASES) == sorted((n, h) for n in FAMILIES for h in H.family(n).histories)
    assert all(h in H.HISTORIES for _, h in H.CASES)
    kinds = {H.family(n).kind for n in FAMILIES}
    assert kinds == {'lstm', 'wavenet', 'las'}
    merges = {H.family(n).spec.merge for n in FAMILIES if H.family(n).kind == 'lstm'}
    assert merges == {'stack_reshape', 'concat', 'none'}
    # every history runs somewhere, and the poison only where no resident recurrence can meet it
    assert {h for _, h in H.CASES} == set(H.HISTORIES)
    for n, h in H.CASES:
        f = H.family(n)
        if h == 'poison':
            assert f.kind != 'lstm' or not f.persistent
        assert H.HISTORIES[h](f), (n, h)               # no empty history


@pytest.mark.parametrize('name', FAMILIES)
def test_every_batch_is_feasible(name):
    f = H.family(name)
    for bname, v, (_, seq, labels, ll) in batches(f):
        B = len(seq)
        assert 1 <= B <= 64 and seq.min() >= 1 and labels.shape[0] == B and ll.shape == (B,)
        assert (ll >= 0).all() and (ll <= labels.shape[1]).all()
        if not f.ctc:
            assert labels.min() >= 0 and labels.max() < f.C
            continue
        assert labels.min() >= 0 and labels.max() <= f.C - 2
        for skip in (1, 3):
            # validate_batch (csrc/nasr_batch.hip): labels + adjacent repeats <= network frames.  Chunking 4 + 3
            # leaves the network frames what they are (include/nasr.h): the same rule holds under it.
            for b in range(B):
                assert O.ctc_feasible(labels[b, :ll[b]], skip_frames(int(seq[b]), skip)), (bname, v, b, skip)


@pytest.mark.parametrize('name', FAMILIES)
def test_the_reference_loss_is_finite_on_every_batch(name):
    f = H.family(name)
    for bname, v, bt in batches(f):
        if bt[0] is None:
            continue                                    # audio: the features exist on the device only
        loss = f.reference_loss(*bt)
        assert np.isfinite(loss) and loss > 0, (bname, v, loss)


@pytest.mark.parametrize('name', FAMILIES)
def test_the_variants_differ_in_every_feature_value(name):
    f = H.family(name)
    for bname in f.batch_names():
        a, b = f.batch(bname, 0), f.batch(bname, 1)
        assert a[0].shape == b[0].shape and a[1].tolist() == b[1].tolist() and a[3].tolist() == b[3].tolist()
        assert a[2].shape == b[2].shape
        live = np.arange(a[0].shape[1])[None, :] < a[1][:, None]
        assert (a[0][live] != b[0][live]).all() and (a[0][live] != 0).all() and (b[0][live] != 0).all()
        assert (a[0][~live] == 0).all() and (b[0][~live] == 0).all()
        if f.ctc and bname == 'big':
            assert (a[2] != b[2]).any()
    if 'audio' in f.histories:
        a, b = f.audio_batch(0), f.audio_batch(1)
        assert all((x != y).all() for x, y in zip(a[0], b[0])) and a[1].tolist() == b[1].tolist()
        # the masks lie inside every utterance and the static block
        for s, (t0, tw) in zip(a[1], a[4][:, 0]):
            assert t0 + tw <= s
        assert (a[5][:, 0].sum(1) <= f.F).all()


def test_probe_shapes_have_the_stated_edges():
    rows = sum(H.PROBE_SEQ)
    assert rows % 32 % 2 == 1 and -(-rows // 16) % 2 == 1 and max(H.PROBE_SEQ) == 37
    for name in FAMILIES:
        f = H.family(name)
        feats, seq, labels, ll = f.probe_batch()
        B, T, F = feats.shape
        assert int(seq.max()) == T and len(set(seq.tolist())) == B          # ragged, one full-length utterance
        big = f.batch('big', 0)
        assert big[0].shape[0] > B and big[0].shape[1] > T and (big[0].shape[0] + 15) // 16 != (B + 15) // 16
        assert big[2].shape[1] >= 4 * labels.shape[1]
        if f.kind == 'lstm' and not f.spec.deepspeech:
            assert (B, T, F) == (5, 37, 13) and tuple(seq) == H.PROBE_SEQ and f.spec.num_classes == 7
            assert f.compaction == (name != 'bilstm-concat-all-rows')
            assert 20 * rows <= 17 * T * 16                                 # the library's own threshold for compacting
        if f.ctc:
            assert H.states_per_lane(big[2].shape[1]) != H.states_per_lane(labels.shape[1])
        for other, Bo in (('small', 3), ('b17', 17)):
            assert f.batch(other, 0)[0].shape[0] == Bo
    # chunking 4 + 3 at T 20: the full-length utterance runs in at least 3 windows
    T = H.SHAPES['chunk'][1]
    assert len([k for k in range(T) if 4 * k < T and (k == 0 or 4 * (k - 1) + 7 < T)]) >= 3
    # WaveNet T 23: of rate 16's taps only +-16 can fall inside, and never on both sides of a frame
    assert 16 < 23 < 32
    assert H.family('las').probe_batch()[0].shape[1] % 2 == 1


def test_featurizer_inputs():
    clip = H.featurizer_clip()
    assert clip.dtype == np.float32 and np.isfinite(clip).all() and clip.size % 80 != 0
