"""Host side of CTC forced alignment: the fp64 restatement against exhaustive enumeration, its tie rules on
hand-worked cases, the path -> spans conversion, the command line's text -> ids step, and the host-only threshold call."""
import itertools
import math

import numpy as np
import pytest

import ctc_align_ref as R


def all_labels(max_len, symbols=2):
    for n in range(max_len + 1):
        for lab in itertools.product(range(symbols), repeat=n):
            yield list(lab)


def test_restatement_finds_the_best_of_every_valid_path():
    """every label over 2 symbols up to 3 long (repeats included), every F up to 6: the restatement's path is the best of
    all valid paths, found by enumeration; Gaussian logits, so no ties"""
    rs = np.random.RandomState(11)
    cases = 0
    for lab in all_labels(3):
        for F in range(1, 7):
            if not R.feasible(lab, F):
                with pytest.raises(ValueError):
                    R.align(rs.randn(F, 3), lab)
                continue
            x = rs.randn(F, 3)
            paths = R.enumerate_paths(lab, F, 2)
            assert paths and all(R.is_valid_path(p, lab, 2) for p in paths)
            sums = [R.path_sum(x, lab, p) for p in paths]
            best = int(np.argmax(sums))
            for every in (4, 0, 1):
                path, score, vmax, gap = R.align(x, lab, rescale_every=every)
                assert list(path) == paths[best], (lab, F, every)
                assert abs(R.path_sum(x, lab, path) - sums[best]) <= 1e-12
                assert abs(score - R.path_score(x, lab, paths[best])) <= 1e-12
                assert gap > 0 and np.isfinite(vmax)
            cases += 1
    assert cases == 60          # 15 labels x 6 lengths, less the 30 infeasible pairs


def test_all_zero_logits_pin_both_tie_rules():
    """every path scores the same: the end state is S-1, and walking back a state stays while it can, then comes from s-1,
    then from s-2"""
    z = np.zeros((5, 3))
    path, score, _, gap = R.align(z, [0, 1])
    # state 4 is reachable from frame 2 on (stay, stay); before that 3 <- 1 is the only way: a skip, since l'_3 = 1 != l'_1 = 0
    assert list(path) == [1, 3, 4, 4, 4]
    assert gap == 0.0 and abs(score - 5 * -math.log(3)) < 1e-12
    # one label: 2 <- 2 (stay) at frame 2, then 2 <- 1 (state 2 does not exist at frame 0)
    assert list(R.align(np.zeros((3, 3)), [0])[0]) == [1, 2, 2]
    # label [0, 1], 4 frames: 4 stays while it exists (frames 3, 2), comes from 3 (a blank takes no skip), and 3 at frame 1 has
    # only the skip from 1 behind it
    x = np.zeros((4, 3))
    assert list(R.align(x, [0, 1])[0]) == [1, 3, 4, 4]
    # 3 at frame 2 (forced by a bonus on label 1 there) can come from 3, 2 or 1 at frame 1, all equal: it stays
    x = np.zeros((4, 3))
    x[2, 1] = 1.0
    x[3, 1] = 1.0
    assert list(R.align(x, [0, 1])[0]) == [1, 3, 3, 3]


def test_repeat_label_at_minimal_length_has_one_path():
    """[0, 0] needs the blank between its two ids: 3 frames, the path 1 2 3, however bad that blank is"""
    x = np.zeros((3, 3))
    x[1, 2] = -10.0
    path, score, _, _ = R.align(x, [0, 0])
    assert list(path) == [1, 2, 3]
    assert R.enumerate_paths([0, 0], 3, 2) == [[1, 2, 3]]
    assert abs(score - R.path_score(x, [0, 0], [1, 2, 3])) < 1e-12
    with pytest.raises(ValueError):
        R.align(np.zeros((2, 3)), [0, 0])


def test_empty_label_is_all_blank():
    rs = np.random.RandomState(3)
    x = rs.randn(4, 5)
    path, score, _, gap = R.align(x, [])
    assert list(path) == [0, 0, 0, 0] and gap == np.inf
    assert abs(score - float((x[:, 4] - R.logz_rows(x)).sum())) < 1e-12


def test_spans_of_hand_made_paths():
    from neuralasr_amd.align import spans
    # a symbol held for several frames, leading and trailing blanks
    assert spans([0, 0, 1, 1, 1, 2, 2], [7]) == [(7, 2, 4)]
    # blanks between repeats
    assert spans([1, 2, 2, 3, 3, 4], [5, 5]) == [(5, 0, 0), (5, 3, 4)]
    # a skipped blank (1 -> 3), and the -1 tail of a padded row
    assert spans(np.array([1, 3, 3, 4, -1, -1], np.int32), [2, 9]) == [(2, 0, 0), (9, 1, 2)]
    # nothing to report for an empty label
    assert spans([0, 0, -1], []) == []
    with pytest.raises(ValueError):
        spans([0, 1, 2, 2], [4, 6])           # not a path of this label: label 1 is never visited


def test_the_las_network_refuses():
    """LAS has no CTC lattice: align and align_audio raise before they touch a handle"""
    from neuralasr_amd.networks.las import LAS
    net = LAS.__new__(LAS)
    for call in (lambda: net.align(np.zeros((1, 4, 3)), [[1]], [4], [1]), lambda: net.align_audio([np.zeros(800)], [8000], [[1]], [1])):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert 'CTC' in str(e.value)


def toy_config(tmp_path, texts):
    from neuralasr_amd.features import write_wav16
    rs = np.random.RandomState(2)
    rows = []
    for i, text in enumerate(texts):
        wav, txt = tmp_path / ('u%d.wav' % i), tmp_path / ('u%d.txt' % i)
        write_wav16(wav, 0.1 * rs.randn(4000), 8000)
        txt.write_text(text + '\n')
        rows.append('%s,%s,%d' % (wav, txt, 500 + i))
    (tmp_path / 'data.csv').write_text('\n'.join(rows) + '\n')
    cfg = tmp_path / 'a.config'
    cfg.write_text(
        '[Parameters]\nsamplerate=8000\nnumcep=13\nnumcontext=2\nlabel_context=1\nbatch_size=2\nepochs=1\n'
        'learningrate=0.001\nmodel_dir=%s\nstart_step=0\nreport_step=1\nnum_gpus=1\npunc_regex=[^a-z0-9 ]\n'
        'sym_file=%s\nnetwork=networks.lstm_ctc_net.LstmCTCNet\n'
        '[Train]\ninput=%s/train.scp\n[Test]\ninput=%s/test.scp\n'
        '[MFCC Featurizer]\ninput=%s\noutput=%s\nstart_marker=^\nend_marker=$$\n'
        % (tmp_path / 'model', tmp_path / 'symbols', tmp_path, tmp_path, tmp_path / 'data.csv', tmp_path))
    return cfg


def test_text_to_ids_is_the_datasets(tmp_path):
    """the command line's ids for a transcript = the ids the dataset gives it (label_context n-grams between the markers),
    and a symbol the table does not hold is an error that names it, with nothing inserted"""
    from neuralasr_amd.align import text_ids
    from neuralasr_amd.audio_dataset import AudioDataSet, prepare_symbols
    from neuralasr_amd.config import Config
    from neuralasr_amd.preprocess_mfcc import update_symbols
    from neuralasr_amd.utils import read_label_text
    texts = ['Hello world.', 'A cat, a dog!', 'low gear', 'the end', 'old road']
    cfg = toy_config(tmp_path, texts)
    prepare_symbols(Config(str(cfg), True))                  # writes the symbol file
    config = Config(str(cfg), True)
    ds = AudioDataSet(config.mfcc_input, config, 'train')
    by_wav = {wav: labels for wav, labels in ds.X}
    known = config.symbols.counter
    for i in range(4):                                       # the training rows
        clean = read_label_text(str(tmp_path / ('u%d.txt' % i)), config.punc_regex)
        ids = text_ids(config, clean)
        assert ids.dtype == np.int32
        assert np.array_equal(ids, by_wav[str(tmp_path / ('u%d.wav' % i))])
        assert np.array_equal(ids, update_symbols(config, clean))
        assert ids[0] == config.symbols.get_id('^') and ids[-1] == config.symbols.get_id('$')
    with pytest.raises(ValueError) as e:
        text_ids(config, 'hex')                              # 'hex' holds the n-gram 'hex', which no transcript has
    assert "'hex'" in str(e.value)
    assert config.symbols.counter == known


def test_backpointer_threshold_is_a_function_of_frames_and_label_length():
    """host only: back-pointers take 8 / 16 / 32 bits per lane and frame for labels up to 127 / 255 / 511 ids and stay in
    LDS up to 56 KiB: 896 / 448 / 224 frames after the first"""
    from neuralasr_amd import _lib
    lib = _lib.load()
    f = lib.nasr_ctc_align_lds
    for L, last in ((0, 897), (12, 897), (127, 897), (128, 449), (200, 449), (255, 449), (256, 225), (511, 225)):
        assert f(1, L) == 1 and f(last, L) == 1 and f(last + 1, L) == 0 and f(5000, L) == 0, (L, last)
    assert f(0, 3) < 0 and f(10, -1) < 0 and f(10, 512) < 0
