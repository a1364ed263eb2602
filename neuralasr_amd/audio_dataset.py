"""Batch reader over the [MFCC Featurizer] input CSV (`wav,txt,size` rows): DataSet's interface and batch composition
(reference: dataset.py:12-91) on what preprocess_mfcc.py:33-93 would have pickled, without the pickles.  A batch is
(audios, rates, labels, labels_len): the float32 utterances at their files' own rates and the padded label ids; the
features are made on the GPU when the batch is uploaded (HipNetwork.train_audio, Engine.upload_batch_audio).

The rules are preprocess_mfcc's: the first int(0.8 n) rows are the training set, the rest the test set; each set sorted by
the size column, ties in CSV order; a row whose files are missing is skipped with a warning; an utterance is kept when
its cleaned transcription has no more characters than it has frames; labels are update_symbols' ids against the config's
symbol table.  rand_shift is not supported: its roll-and-crop leaves real neighbour frames where the context pads were."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .features import num_frames, read_wav_native, resample_length, wav_info
from .logger import get_logger
from .preprocess_mfcc import READ_THREADS, read_rows, sort_rows, split_rows, update_symbols
from .utils import read_label_text

logger = get_logger()


_kept = {}        # (CSV path, its mtime, samplerate, punc_regex) -> (kept training rows, kept test rows): one pass over a corpus per process


def kept_sets(filename, config):
    """(training rows, test rows) of the CSV as kept_rows keeps them; read once per process and CSV"""
    key = (os.path.abspath(filename), os.path.getmtime(filename), config.samplerate, config.punc_regex)
    if key not in _kept:
        train_rows, test_rows = split_rows(read_rows(filename))
        _kept[key] = (kept_rows(train_rows, config), kept_rows(test_rows, config))
    return _kept[key]


def kept_rows(rows, config):
    """[(wav, txt, cleaned transcription)] of one set in size order: write_data's filter (preprocess_mfcc.py:33-62).
    The frame count comes from the WAV's header; no audio is decoded here."""
    out = []
    for wav, txt, _ in sort_rows(rows):
        if not os.path.exists(wav):
            logger.warning(wav + ' does not exist.')
            continue
        if not os.path.exists(txt):
            logger.warning(txt + ' does not exist.')
            continue
        size, rate = wav_info(wav)
        n = size if rate == config.samplerate else resample_length(size, rate, config.samplerate)[0]
        clean = read_label_text(txt, config.punc_regex)
        if len(clean) <= num_frames(n, config.samplerate):
            out.append((wav, txt, clean))
    return out


def prepare_symbols(config):
    """The symbol table preprocess_mfcc.main would write for config.mfcc_input, when the config has none yet: padding, the
    markers, the n-grams of the training set and then of the test set in their size order, blank last."""
    sym = config.symbols
    if sym.counter > 0:
        return
    sym.insert_padding()
    if config.start_marker:
        sym.insert_sym(config.start_marker)
    if config.end_marker:
        sym.insert_sym(config.end_marker)
    for kept in kept_sets(config.mfcc_input, config):
        for _, _, clean in kept:
            update_symbols(config, clean)
    sym.insert_blank()
    if config.sym_file:
        config.write_symbols()


class AudioDataSet:
    def __init__(self, filename, config, which='train'):
        if which not in ('train', 'test'):
            raise ValueError("which must be 'train' or 'test'")
        if getattr(config, 'rand_shift', 0) > 0:
            raise ValueError('rand_shift > 0 cannot be combined with batches from audio: the roll-and-crop of dataset.py:23-31 '
                             'leaves real neighbour frames where the context pads were, which the centre-frame form of a '
                             'batch cannot express; set rand_shift=0 or train from the pickled features')
        self.filename = filename
        self.config = config
        self.index = 0
        prepare_symbols(config)
        self.padding_id = config.symbols.get_padding_id()
        known = config.symbols.counter
        self.X = []                                   # (wav, labels) in DataSet's order
        self.chars = {}                               # wav -> characters of its cleaned transcription (kept_rows' filter)
        self.last_chars = []                          # those of the batch get_next_batch returned last
        for wav, _, clean in kept_sets(filename, config)[0 if which == 'train' else 1]:
            self.X.append((wav, update_symbols(config, clean)))
            self.chars[wav] = len(clean)
        if config.symbols.counter != known:
            raise ValueError('%s holds symbols that %s does not: run preprocess_mfcc, or remove the symbol file to have '
                             'it rebuilt' % (filename, config.sym_file))

    def names(self):
        """the utterances' names, as preprocess_mfcc would name their pickles"""
        return [os.path.basename(wav).replace('.wav', '') for wav, _ in self.X]

    def load(self, item):
        wav, labels = item
        audio, rate = read_wav_native(wav)
        return audio, rate, labels, labels.shape[0]

    def reset_epoch(self):
        self.index = 0

    def has_more_batches(self):
        return self.index < len(self.X)

    def get_next_batch(self):
        bs = self.config.batch_size
        picks = [self.X[self.index]]
        self.index += 1
        while self.index % bs > 0:
            if self.index >= len(self.X):
                if len(picks) == bs:
                    break
                self.index -= 1          # tail batch: the last file again until it is full (dataset.py:33-40)
            picks.append(self.X[self.index])
            self.index += 1
        with ThreadPoolExecutor(max_workers=READ_THREADS) as ex:
            items = list(ex.map(self.load, picks))
        self.last_chars = [self.chars[wav] for wav, _ in picks]
        max_label = max(n for _, _, _, n in items)
        labels = np.full((len(items), max_label), self.padding_id, dtype=np.int32)
        for i, (_, _, l, n) in enumerate(items):
            labels[i, :n] = l
        return [a for a, _, _, _ in items], [r for _, r, _, _ in items], labels, [n for _, _, _, n in items]

    def get_feature_shape(self):
        return [self.config.batch_size, None, self.config.feature_size]

    def get_label_shape(self):
        return [self.config.batch_size, None, 1]

    def get_num_of_sample(self):
        return len(self.X)


class AudioFeed:
    """An AudioDataSet as train_model reads a DataSet: every batch as (features.AudioBatch, labels, seq_len, labels_len).
    With an `augmenter` (augment.Augmenter; the training feed of `train --from-audio` only) every batch is drawn speed
    factors and SpecAugment masks under the counter of the global step it will train: config.start_step + the number of
    batches handed out, this one included."""

    def __init__(self, dataset, augmenter=None):
        self.dataset = dataset
        self.augmenter = augmenter
        self.handed_out = 0

    def __getattr__(self, name):
        return getattr(self.dataset, name)

    def get_next_batch(self):
        from .features import AudioBatch
        audios, rates, labels, labels_len = self.dataset.get_next_batch()
        cfg = self.dataset.config
        self.handed_out += 1
        if self.augmenter is not None:
            b = self.augmenter.batch(cfg.start_step + self.handed_out, audios, rates, self.dataset.last_chars)
        else:
            b = AudioBatch(cfg.samplerate, audios, rates, cfg.feature_size)
        return b, labels, b.seq_len, labels_len
