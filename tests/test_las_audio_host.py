"""Host side of audio for the LAS network and decode.py: the two resident entry points are declared, exported and bound, and
`decode --from-audio` composes the batches that preprocess_mfcc + DataSet compose for the test list (names, labels and
seq_len; the features need a GPU)."""
import ctypes
import os

import numpy as np
import pytest

from test_audio_batch_host import host_featurize, make_corpus

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAS = 'network=networks.las.LAS'
BILSTM = 'network=networks.bilstm_ctc_net.BiLstmCTCNet'


def test_resident_symbols_are_declared_exported_and_bound():
    from neuralasr_amd import _lib
    lib = _lib.load()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    H, fp, ip, i, f = (ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_int32), ctypes.c_int,
                       ctypes.c_float)
    header = open(os.path.join(ROOT, 'include', 'nasr.h')).read()
    for name, args in (('nasr_las_forward_resident', [H, i, fp]),
                       ('nasr_las_beam_search_resident', [H, i, i, i, i, f, ip])):
        assert name in _lib.SYMBOLS
        assert hasattr(raw, name), name + ' is not exported by libnasr.so'
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == args
        decl = header[:header.index('int ' + name + '(')]
        comment = decl[decl.rindex('/*'):]
        assert comment.rstrip().endswith('*/'), name + ' has no comment of its own'
        assert 'networks/las.py:' in comment and 'utils.py:24-31' in comment


def las_config(cfg_path):
    """make_corpus's config with the LAS network"""
    text = cfg_path.read_text()
    assert BILSTM in text
    cfg_path.write_text(text.replace(BILSTM, LAS))
    return cfg_path


@pytest.mark.parametrize('network', ['bilstm', 'las'])
def test_decode_from_audio_composes_the_batches_of_the_test_list(tmp_path, monkeypatch, network):
    from neuralasr_amd import decode, preprocess_mfcc
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    from neuralasr_amd.features import AudioBatch
    cfg_path, out = make_corpus(tmp_path)
    if network == 'las':
        las_config(cfg_path)
    preprocess_mfcc.main([str(cfg_path)], featurize=host_featurize(Config(str(cfg_path))))
    seen = []
    monkeypatch.setattr(decode, 'decode', lambda data, config: seen.append((data, config)))
    decode.main([str(cfg_path), '--from-audio'])
    (feed, config), = seen
    assert (config.batch_size, config.epochs, config.rand_shift) == (1, 1, 0)
    cfg2 = Config(str(cfg_path), True)
    cfg2.batch_size, cfg2.epochs, cfg2.rand_shift = 1, 1, 0
    ds = DataSet(str(out / 'test.scp'), cfg2)
    names = [os.path.basename(p)[:-4] for p in ds.X]
    assert feed.names() == names == ['utt10', 'utt09', 'utt08']
    assert feed.get_feature_shape() == ds.get_feature_shape() and feed.get_label_shape() == ds.get_label_shape()
    n = 0
    while ds.has_more_batches():
        assert feed.has_more_batches()
        _, labels, seq_len, labels_len = ds.get_next_batch()
        b, alabels, aseq_len, alabels_len = feed.get_next_batch()
        assert isinstance(b, AudioBatch) and len(b) == 1
        assert np.array_equal(alabels, labels) and list(alabels_len) == list(labels_len)
        assert [int(t) for t in aseq_len] == [int(t) for t in seq_len] and b.shape == (1, int(seq_len[0]), 65)
        n += 1
    assert n == 3 and not feed.has_more_batches()
    # without the flag: the pickled test list, as before
    del seen[:]
    decode.main([str(cfg_path)])
    assert isinstance(seen[0][0], DataSet) and seen[0][0].X == ds.X


def test_decode_from_audio_needs_the_csv_and_a_network_that_takes_audio(tmp_path, monkeypatch):
    from neuralasr_amd import decode
    from neuralasr_amd.networks.las import LAS as LasNet
    cfg_path, _ = make_corpus(tmp_path)
    las_config(cfg_path)
    monkeypatch.setattr(decode, 'decode', lambda data, config: pytest.fail('decode() must not start'))
    monkeypatch.setattr(LasNet, 'takes_audio', False)
    with pytest.raises(ValueError, match='takes audio'):
        decode.main([str(cfg_path), '--from-audio'])
    monkeypatch.undo()
    monkeypatch.setattr(decode, 'decode', lambda data, config: pytest.fail('decode() must not start'))
    text = cfg_path.read_text()
    csv = 'input=%s\n' % (tmp_path / 'data.csv')
    assert csv in text
    cfg_path.write_text(text.replace(csv, ''))
    with pytest.raises(ValueError, match='MFCC Featurizer'):
        decode.main([str(cfg_path), '--from-audio'])


def test_las_takes_audio():
    from neuralasr_amd.networks.hipnetwork import HipNetwork
    from neuralasr_amd.networks.las import LAS as LasNet
    assert LasNet.takes_audio is True
    assert LasNet.audio_batch is HipNetwork.audio_batch and LasNet.stage_batch is not HipNetwork.stage_batch
