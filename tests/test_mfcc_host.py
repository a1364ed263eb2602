"""The MFCC front end's host side, no GPU: the WAV reader, psf's frame count and filterbank as the library builds them,
the transcription and label helpers, and preprocess_mfcc's split / sort / filter / pickle with the featurizer injected."""
import pickletools
import struct

import numpy as np
import pytest

import mfcc_ref as R
from neuralasr_amd import features
from neuralasr_amd.utils import read_label_text


def riff(path, tag, channels, rate, bits, payload, extensible_sub=None):
    """A RIFF/WAVE file: fmt (16 bytes, or 40 with WAVE_FORMAT_EXTENSIBLE) then data."""
    block = channels * bits // 8
    fmt = struct.pack('<HHIIHH', tag, channels, rate, rate * block, block, bits)
    if extensible_sub is not None:
        guid = struct.pack('<H', extensible_sub) + b'\x00\x00\x00\x00\x10\x00\x80\x00\x00\xaa\x00\x38\x9b\x71'
        fmt += struct.pack('<HHI', 22, bits, 0) + guid
    body = b'WAVE' + b'fmt ' + struct.pack('<I', len(fmt)) + fmt + b'LIST' + struct.pack('<I', 3) + b'abc\x00'
    body += b'data' + struct.pack('<I', len(payload)) + payload
    with open(path, 'wb') as fh:
        fh.write(b'RIFF' + struct.pack('<I', len(body)) + body)
    return str(path)


def test_read_wav_pcm_widths_and_float(tmp_path):
    i16 = np.array([0, 1, -1, 32767, -32768], dtype='<i2')
    y = features.read_wav(riff(tmp_path / 'a.wav', 1, 1, 16000, 16, i16.tobytes()), 16000)
    assert y.dtype == np.float32 and np.array_equal(y, i16.astype(np.float32) / 32768)

    u8 = np.array([0, 128, 255, 1], dtype=np.uint8)
    y = features.read_wav(riff(tmp_path / 'b.wav', 1, 1, 8000, 8, u8.tobytes()), 8000)
    assert np.array_equal(y, (u8.astype(np.float32) - 128) / 128)

    v24 = [0, 1, -1, (1 << 23) - 1, -(1 << 23), 12345]
    raw = b''.join(struct.pack('<i', v)[:3] for v in v24)
    y = features.read_wav(riff(tmp_path / 'c.wav', 1, 1, 8000, 24, raw), 8000)
    assert np.array_equal(y, np.array(v24, dtype=np.float64).astype(np.float32) / np.float32(2 ** 23))

    i32 = np.array([0, 1, -1, 2 ** 31 - 1, -2 ** 31, 123456789], dtype='<i4')
    y = features.read_wav(riff(tmp_path / 'd.wav', 1, 1, 8000, 32, i32.tobytes()), 8000)
    assert np.array_equal(y, (i32.astype(np.float64) / 2 ** 31).astype(np.float32))

    f32 = np.array([0.5, -0.25, 1e-3], dtype='<f4')
    y = features.read_wav(riff(tmp_path / 'e.wav', 3, 1, 8000, 32, f32.tobytes()), 8000)
    assert np.array_equal(y, f32)
    f64 = np.array([0.1, -0.3], dtype='<f8')
    y = features.read_wav(riff(tmp_path / 'f.wav', 3, 1, 8000, 64, f64.tobytes()), 8000)
    assert np.array_equal(y, f64.astype(np.float32))


def test_read_wav_extensible_and_stereo(tmp_path):
    i16 = np.array([[100, -300], [7, 8], [-32768, 32767]], dtype='<i2')      # [frames, channels]
    y = features.read_wav(riff(tmp_path / 's.wav', 0xFFFE, 2, 16000, 16, i16.tobytes(), extensible_sub=1), 16000)
    ch = (i16.astype(np.float32) / 32768).T
    assert np.array_equal(y, np.mean(ch, axis=0))
    f32 = np.array([0.25, 0.5, -1.0, 0.125], dtype='<f4')
    y = features.read_wav(riff(tmp_path / 't.wav', 0xFFFE, 1, 16000, 32, f32.tobytes(), extensible_sub=3), 16000)
    assert np.array_equal(y, f32)


def test_read_wav_errors(tmp_path):
    p = riff(tmp_path / 'a.wav', 1, 1, 22050, 16, b'\x00\x00' * 4)
    with pytest.raises(ValueError, match='22050.*16000'):
        features.read_wav(p, 16000)
    p = riff(tmp_path / 'b.wav', 2, 1, 16000, 4, b'\x00' * 8)          # MS ADPCM
    with pytest.raises(ValueError, match='unsupported'):
        features.read_wav(p, 16000)
    p = tmp_path / 'c.wav'
    p.write_bytes(b'not a wav file at all')
    with pytest.raises(ValueError, match='RIFF'):
        features.read_wav(str(p), 16000)


@pytest.mark.parametrize('n', [1, 399, 400, 401, 560])
def test_frame_count(n):
    assert features.num_frames(n, 16000) == R.num_frames(n, 16000)
    assert features.num_frames(n, 8000) == R.num_frames(n, 8000)
    assert features.num_frames(n, 22050) == R.num_frames(n, 22050)
    assert [features.num_frames(k, 16000) for k in (1, 399, 400, 401, 560, 561)] == [1, 1, 1, 2, 2, 3]


@pytest.mark.parametrize('sr,empty', [(16000, 13), (8000, 5)])
def test_filterbank_table(sr, empty):
    bins, w = features.filterbank(sr)
    assert np.array_equal(bins, R.filterbank_bins(sr).astype(np.int32))
    ref = R.filterbank(sr)
    assert np.array_equal(w, ref.astype(np.float32))
    assert int((ref.sum(axis=1) == 0).sum()) == empty
    assert int((w.sum(axis=1) == 0).sum()) == empty


def test_read_label_text(tmp_path):
    p = tmp_path / 't.txt'
    p.write_text('  Hello,   World!\nIt\'s  "fine".\r\n')
    assert read_label_text(str(p), '[^a-z0-9 ]') == 'hello__worldits_fine'


class _Cfg:
    def __init__(self, label_context, start=None, end=None):
        from neuralasr_amd.symbols import Symbols
        self.label_context, self.start_marker, self.end_marker = label_context, start, end
        self.symbols = Symbols(label_context)
        self.symbols.insert_padding()
        for m in (start, end):
            if m:
                self.symbols.insert_sym(m)


def test_update_symbols():
    from neuralasr_amd.preprocess_mfcc import update_symbols
    c = _Cfg(0)
    assert list(update_symbols(c, 'abba')) == [1, 2, 2, 1]
    c = _Cfg(0, '^', '$')
    assert list(update_symbols(c, 'ab')) == [1, 3, 4, 2]
    c = _Cfg(1)
    ids = update_symbols(c, 'ab_a')
    assert [c.symbols.get_sym(i) for i in ids] == ['^ab', 'ab_', 'b_a', '_a^']
    c = _Cfg(1, '^', '$')
    ids = update_symbols(c, 'ab')
    assert [c.symbols.get_sym(i) for i in ids] == ['^', '^ab', 'ab^', '$']


def _wav(path, n):
    return riff(path, 1, 1, 8000, 16, np.zeros(n, dtype='<i2').tobytes())


def test_preprocess_split_sort_filter_and_pickle(tmp_path):
    from neuralasr_amd import preprocess_mfcc as P
    from neuralasr_amd.dataset import DataSet
    rows = []
    # (name, size, transcript, frames the fake featurizer gives)
    spec = [('u0', 30, 'bb', 5), ('u1', 10, 'a', 5), ('u2', 30, 'aa', 5), ('u3', 20, 'toolongtext', 3),
            ('u4', 5, 'ab', 5), ('u5', 9, 'ba', 5), ('u6', 9, 'x', 5), ('u7', 1, 'y', 5), ('u8', 2, 'z', 5),
            ('u9', 3, 'ab', 5)]
    frames = {}
    for name, size, text, T in spec:
        wav = _wav(tmp_path / (name + '.wav'), 8)
        txt = tmp_path / (name + '.txt')
        txt.write_text(text)
        frames[wav] = T
        rows.append('%s,%s,%d' % (wav, txt, size))
    rows.insert(3, '%s,%s,%d' % (tmp_path / 'missing.wav', tmp_path / 'u0.txt', 4))
    out = tmp_path / 'out'
    (tmp_path / 'in.csv').write_text('\n'.join(rows) + '\n')
    (tmp_path / 't.config').write_text(
        '[Parameters]\nsamplerate=8000\nnumcep=2\nnumcontext=0\nlabel_context=0\nbatch_size=2\nepochs=1\n'
        'learningrate=0.001\nmodel_dir=m\nstart_step=0\nreport_step=1\nnum_gpus=1\npunc_regex=[^a-z0-9 ]\n'
        'sym_file=${MFCC Featurizer:output}/symbols\nnetwork=networks.bilstm_ctc_net.BiLstmCTCNet\n'
        '[Train]\ninput=${MFCC Featurizer:output}/train.scp\n[Test]\ninput=${MFCC Featurizer:output}/test.scp\n'
        '[MFCC Featurizer]\ninput=%s\noutput=%s\nstart_marker=^\nend_marker=$$\n' % (tmp_path / 'in.csv', out))
    seen = []

    def fake(paths):
        seen.extend(paths)
        return [np.full((frames[p], 2), float(i), dtype=np.float32) for i, p in enumerate(paths)]
    P.main([str(tmp_path / 't.config')], featurize=fake)
    train = (out / 'train.scp').read_text().split()
    test = (out / 'test.scp').read_text().split()
    # 11 rows: the first 8 train (missing.wav among them, skipped); sorted by size, ties in CSV order; u3 filtered
    assert train == ['u4.pkl', 'u5.pkl', 'u6.pkl', 'u1.pkl', 'u0.pkl', 'u2.pkl']
    assert test == ['u7.pkl', 'u8.pkl', 'u9.pkl']
    assert 'u3.wav' in ' '.join(seen) and 'missing.wav' not in ' '.join(seen)
    # symbols: padding, markers, then the training set's characters in sorted order, the test set's, blank last
    syms = dict(line.split() for line in (out / 'symbols').read_text().splitlines())
    assert syms == {'<padding>': '0', '^': '1', '$': '2', 'a': '3', 'b': '4', 'x': '5', 'y': '6', 'z': '7',
                    '<blank>': '8'}
    raw = (out / 'u4.pkl').read_bytes()
    ops = [(op.name, arg) for op, arg, _ in pickletools.genops(raw)]
    names = [a for _, a in ops if isinstance(a, str)]
    assert 'audiosample' in names and names[names.index('audiosample') + 1] == 'AudioSample'
    assert 'neuralasr_amd.audiosample' not in names
    # loads in the project's DataSet
    from neuralasr_amd.config import Config
    cfg = Config(str(tmp_path / 't.config'), True)
    ds = DataSet(str(out / 'train.scp'), cfg)
    mfccs, labels, seq_len, label_len = ds.get_next_batch()
    assert mfccs.shape == (2, 5, 2) and list(labels[0][:4]) == [1, 3, 4, 2]
    mfcc, lab, T, L = ds.load_pkl(str(out / 'u4.pkl'))
    assert mfcc.dtype == np.float32 and mfcc.shape == (5, 2) and list(lab) == [1, 3, 4, 2] and T == 5 and L == 4
