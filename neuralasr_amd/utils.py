"""The reference's utils.py: include_context, read_label_text, sparse_tuple_from, and
compute_mfcc_and_read_transcription on the GPU front end of features.py (librosa and python_speech_features are not
needed)."""
import re

import numpy as np


def include_context(audio_mfcc, numcontext, numcep):
    """Stack numcontext frames either side of every frame (reference: utils.py:8-21): [T,numcep] ->
    [T,(2*numcontext+1)*numcep], zero frames beyond the ends."""
    audio_mfcc = np.asarray(audio_mfcc)
    T = audio_mfcc.shape[0]
    pad = np.zeros((numcontext, numcep), dtype=audio_mfcc.dtype)
    ext = np.concatenate((pad, audio_mfcc, pad))
    win = 2 * numcontext + 1
    out = np.empty((T, win * numcep), dtype=audio_mfcc.dtype)
    for w in range(win):
        out[:, w * numcep:(w + 1) * numcep] = ext[w:w + T]
    return out


def sparse_tuple_from(sequences, output_lengths):
    """dense padded labels + lengths -> (indices int64 [n,2], values int32 [n], shape int64 [2])
    (reference: utils.py:44-58), the feed of tf.sparse_placeholder.  The HIP path takes the dense form
    directly; this is kept for callers that expect the tuple."""
    idx, vals = [], []
    for n, seq in enumerate(sequences):
        L = int(output_lengths[n])
        idx.extend((n, k) for k in range(L))
        vals.extend(seq[:L])
    indices = np.asarray(idx, dtype=np.int64).reshape(-1, 2)
    values = np.asarray(vals, dtype=np.int32)
    shape = np.asarray([len(sequences), indices[:, 1].max() + 1], dtype=np.int64)
    return indices, values, shape


def read_label_text(txtfile, punc_regex):
    """The cleaned transcription of a text file (reference: utils.py:34-41): newlines dropped, stripped, lowercased,
    punc_regex removed, one pass of '  ' -> ' ', then ' ' -> '_'."""
    with open(txtfile, 'r') as f:
        transcription = f.read().replace('\n', '').replace('\r', '')
    transcription = transcription.strip().lower()
    clean_transcription = re.sub(punc_regex, '', transcription)
    return clean_transcription.replace('  ', ' ').replace(' ', '_')


_featurizers = {}


def normalization_of(config):
    """the front end's normalisation keywords of a config (Config.normalization, norm_min_frames); the whole-utterance
    rule for a config object without them"""
    return dict(normalization=getattr(config, 'normalization', 'utterance'),
                norm_min_frames=getattr(config, 'norm_min_frames', None))


def featurizer(sr, numcontext, numcep, kind='mfcc', deltas=0, normalization='utterance', norm_min_frames=None):
    """One GPU featurizer per (sr, numcontext, numcep, kind, deltas, normalization, norm_min_frames) for the process."""
    key = (int(sr), int(numcontext), int(numcep), kind, int(deltas), normalization, norm_min_frames)
    if key not in _featurizers:
        from .features import Featurizer
        _featurizers[key] = Featurizer(sr, numcep, numcontext, kind=kind, deltas=deltas, normalization=normalization,
                                       norm_min_frames=norm_min_frames)
    return _featurizers[key]


def convert_to_mfcc(wavfile, sr, numcontext, numcep, kind='mfcc', deltas=0, normalization='utterance',
                    norm_min_frames=None):
    """float32 [T, (2*numcontext+1)*numcep*(1+deltas)] normalised features of a WAV file (reference: utils.py:24-31; MFCC,
    or the log-mel filterbank for kind='logfbank', with `deltas` levels of delta columns); a file at another rate than
    sr is resampled to it on the GPU, as librosa.load(wavfile, mono=True, sr=sr) does.  normalization='causal': the running
    normalisation of DESIGN.md §16 in the place of the whole-utterance one."""
    from .features import read_wav_native
    audio, rate = read_wav_native(wavfile)
    return featurizer(sr, numcontext, numcep, kind, deltas, normalization, norm_min_frames).compute([audio], rates=[rate])[0]


def compute_mfcc_and_read_transcription(wavfile, sr, numcontext, numcep, punc_regex=None, txtfile=None, kind='mfcc',
                                        deltas=0, normalization='utterance', norm_min_frames=None):
    """(reference: utils.py:61-68) the features, and the cleaned transcription when txtfile is given."""
    audio_mfcc = convert_to_mfcc(wavfile, sr, numcontext, numcep, kind, deltas, normalization, norm_min_frames)
    if txtfile:
        return audio_mfcc, read_label_text(txtfile, punc_regex)
    return audio_mfcc
