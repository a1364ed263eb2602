"""WAV files and transcripts -> pickled AudioSample files, train.scp / test.scp and the symbol table
(reference: preprocess_mfcc.py:18-93).  `python -m neuralasr_amd.preprocess_mfcc CONFIG`.

The CSV ([MFCC Featurizer] input) has rows `wav,txt,size`, no header.  The first int(0.8 n) rows are the training set,
the rest the test set; each set is sorted by the numeric size column with a stable sort (pandas' default quicksort,
which the reference uses, may order equal sizes differently).  A row whose files are missing is skipped with a
warning; an utterance is kept when its cleaned transcription has no more characters than it has frames.  Features are
computed on the GPU in batches; the pickles name the class `audiosample.AudioSample`, as the reference's do, so they
load in this DataSet and in the reference's."""
import argparse
import csv
import os
import pickle
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from .audiosample import AudioSample
from .config import Config
from .logger import get_logger
from .utils import featurizer, normalization_of, read_label_text

logger = get_logger()

TRAIN_FRACTION = 0.8
BATCH_FILES = 64          # utterances featurised per GPU call
READ_THREADS = 4


def label_ngrams(config, clean_transcription):
    """The label_context n-grams of a transcription padded with start_marker (or '^'), one per character."""
    num_context = config.label_context
    padded_str = (config.start_marker if config.start_marker else '^') * num_context
    padded_transcript = padded_str + clean_transcription + padded_str
    return [padded_transcript[i:i + (2 * num_context + 1)] for i in range(len(padded_transcript) - num_context * 2)]


def update_symbols(config, clean_transcription):
    """Label ids of a transcription: label_context n-grams over the transcription padded with start_marker (or '^'),
    between the optional start and end markers; new n-grams enter the symbol table (reference: preprocess_mfcc.py:18-30)."""
    sym = config.symbols
    labels = [sym.get_id(config.start_marker)] if config.start_marker else []
    for gram in label_ngrams(config, clean_transcription):
        labels.append(sym.insert_sym(gram))
    if config.end_marker:
        labels.append(sym.get_id(config.end_marker))
    return np.asarray(labels, dtype=np.int32)


class _SamplePickler(pickle._Pickler):
    """Writes the class reference as `audiosample.AudioSample`, the module path of the reference's pickles."""

    def save_global(self, obj, name=None):
        if obj is AudioSample and self.proto >= 4:
            self.save('audiosample')
            self.save('AudioSample')
            self.write(pickle.STACK_GLOBAL)
            self.memoize(obj)
            return
        super().save_global(obj, name)


def dump_sample(sample, path):
    with open(path, 'wb') as fh:
        _SamplePickler(fh, protocol=4).dump(sample)


def read_rows(csv_path):
    with open(csv_path, newline='') as fh:
        return [tuple(r[:3]) for r in csv.reader(fh) if r]


def split_rows(rows):
    n_train = int(len(rows) * TRAIN_FRACTION)
    return rows[:n_train], rows[n_train:]


def sort_rows(rows):
    return sorted(rows, key=lambda r: float(r[2]))     # stable: equal sizes keep their CSV order


def gpu_featurize(config):
    """paths -> features, the WAVs read on a few host threads and featurised on the GPU in one call (files at another
    rate than the config's resampled to it there)."""
    from .features import read_wav_native
    fz = featurizer(config.samplerate, config.numcontext, config.numcep, config.features, config.deltas,
                    **normalization_of(config))

    def run(paths):
        with ThreadPoolExecutor(max_workers=READ_THREADS) as ex:
            audios, rates = zip(*ex.map(read_wav_native, paths))
        return fz.compute(list(audios), rates=list(rates))
    return run


def write_data(rows, config, scp_file_name, featurize=None):
    """(reference: preprocess_mfcc.py:33-62) the samples of one set, in size order, and their list file."""
    rows = sort_rows(rows)
    featurize = featurize or gpu_featurize(config)
    logger.info('Writing List of MFCC files to: ' + scp_file_name)
    logger.info('Writing MFCC to: ' + config.mfcc_output)
    present = []
    for wav, txt, _ in rows:
        logger.info(wav)
        if not os.path.exists(wav):
            logger.warning(wav + ' does not exist.')
        elif not os.path.exists(txt):
            logger.warning(txt + ' does not exist.')
        else:
            present.append((wav, txt))
    with open(scp_file_name, 'w') as f:
        for b in range(0, len(present), BATCH_FILES):
            chunk = present[b:b + BATCH_FILES]
            mfccs = featurize([wav for wav, _ in chunk])
            for (wav, txt), mfcc in zip(chunk, mfccs):
                clean_transcription = read_label_text(txt, config.punc_regex)
                if len(clean_transcription) <= mfcc.shape[0]:
                    labels = update_symbols(config, clean_transcription)
                    filename = os.path.basename(wav).replace('.wav', '')
                    f.write(filename + '.pkl\n')
                    dump_sample(AudioSample(filename, mfcc, labels, clean_transcription),
                                os.path.join(config.mfcc_output, filename + '.pkl'))


def main(argv=None, featurize=None):
    parser = argparse.ArgumentParser(description='Convert audio files into mfcc for training ASR')
    parser.add_argument('config', help='Configuration file.')
    args = parser.parse_args(argv)
    config = Config(args.config)
    if not os.path.exists(config.mfcc_output):
        os.makedirs(config.mfcc_output)
    train_rows, test_rows = split_rows(read_rows(config.mfcc_input))
    config.symbols.insert_padding()
    if config.start_marker:
        config.symbols.insert_sym(config.start_marker)
    if config.end_marker:
        config.symbols.insert_sym(config.end_marker)
    write_data(train_rows, config, os.path.join(config.mfcc_output, 'train.scp'), featurize)
    write_data(test_rows, config, os.path.join(config.mfcc_output, 'test.scp'), featurize)
    config.symbols.insert_blank()
    config.write_symbols()


if __name__ == '__main__':
    main()
