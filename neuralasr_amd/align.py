"""Forced alignment of one WAV file against its transcript with a trained CTC model (the reference has
no aligner).  `python -m neuralasr_amd.align CONFIG WAV TXT`: the transcript becomes label ids the way preprocess_mfcc /
audio_dataset make them (read_label_text, label_context n-grams, the start and end markers) against the model's symbol
table - a symbol the table does not hold is an error, nothing is inserted; the network's align() / align_audio() finds the
best CTC path on the GPU; the output is one log line per symbol, `sym start end`, and the path's log-probability.
With ema_decay in the config the network loads the checkpoint's averaged parameters.

Times are seconds, frame x 0.01 (the front end's winstep), when the network has one logit frame per feature frame; with
frame_skip = s in the config a logit frame is one of the network's frames, s x 0.01 s.  The
literal BiLstmCTCNet (merge 'stack_reshape') has 2T logit frames that its reshape of the (fw, bw) tuple scrambles over
utterances and directions: they have no time, so there the lines carry logit-frame indices."""
import argparse

import numpy as np

from .config import Config
from .logger import get_logger
from .preprocess_mfcc import label_ngrams
from .utils import compute_mfcc_and_read_transcription, normalization_of, read_label_text

logger = get_logger()

WINSTEP = 0.01        # seconds per feature frame (features.py, utils.py:26)


def spans(path_row, label):
    """[(symbol id, first frame, last frame)] in label order from one row of the alignment's path: label i owns the
    frames whose state is 2i+1; blank frames (even states) and the -1 tail belong to no symbol.  Every label of a valid
    path is visited; one that is not (a path from somewhere else) raises."""
    label = [int(x) for x in label]
    first, last = [None] * len(label), [None] * len(label)
    for t, s in enumerate(path_row):
        s = int(s)
        if s < 0:
            break
        if s & 1:
            i = s >> 1
            if first[i] is None:
                first[i] = t
            last[i] = t
    if any(f is None for f in first):
        raise ValueError('path visits no frame of label %d' % first.index(None))
    return [(label[i], first[i], last[i]) for i in range(len(label))]


def text_ids(config, clean_transcription):
    """The label ids of a cleaned transcription, as preprocess_mfcc.update_symbols makes them, against a FIXED symbol
    table: an n-gram or marker the table does not hold raises ValueError naming it."""
    sym = config.symbols
    grams = ([config.start_marker] if config.start_marker else []) + label_ngrams(config, clean_transcription) + \
            ([config.end_marker] if config.end_marker else [])
    ids = []
    for g in grams:
        if g not in sym.sym_to_id:
            raise ValueError('symbol %r of the transcript is not in the symbol table %s' % (g, config.sym_file))
        ids.append(sym.get_id(g))
    return np.asarray(ids, dtype=np.int32)


def frame_seconds(config):
    """the seconds one network frame stands for: the front end's winstep times the config's frame_skip"""
    return int(getattr(config, 'frame_skip', 1)) * WINSTEP


def frames_have_time(network, T=100):
    """one logit frame per frame the network sees (nasr_logit_frames(T) == ceil(T / frame_skip))?  Not under the
    stack_reshape merge."""
    s = int(getattr(network.config, 'frame_skip', 1)) if hasattr(network, 'config') else 1
    return network.engine.logit_frames(T) == (T + s - 1) // s


def report(config, timed, score, symbol_spans):
    if not timed:
        logger.info('This network reshapes the (fw, bw) output tuple into 2T logit frames (stack_reshape, SURVEY.md D3): a '
                    'logit frame is no point in time; printing logit-frame indices.')
    lines = []
    step = frame_seconds(config)
    for sid, a, b in symbol_spans:
        sym = config.symbols.get_sym(sid)
        line = '%s %.2f %.2f' % (sym, a * step, (b + 1) * step) if timed else '%s %d %d' % (sym, a, b)
        logger.info('Aligned: ' + line)
        lines.append(line)
    logger.info('Score: %.6f' % score)
    return lines, score


def main(argv=None):
    parser = argparse.ArgumentParser(description='Align a transcript to an audio file using a trained CTC model.')
    parser.add_argument('config', help='Configuration file.')
    parser.add_argument('input', help='Audio file path')
    parser.add_argument('transcript', help='Text file with the transcript')
    args = parser.parse_args(argv)
    config = Config(args.config, True)
    ids = text_ids(config, read_label_text(args.transcript, config.punc_regex))
    network = config.load_network(fortraining=False)
    labels = ids.reshape(1, -1)
    try:
        timed = frames_have_time(network)
        if getattr(network, 'takes_audio', False):
            from .features import read_wav_native
            audio, rate = read_wav_native(args.input)
            (score, sp), = network.align_audio([audio], [rate], labels, [ids.size])
        else:
            mfcc = compute_mfcc_and_read_transcription(args.input, config.samplerate, config.numcontext, config.numcep,
                                                       kind=config.features, deltas=config.deltas,
                                                       **normalization_of(config))
            (score, sp), = network.align(np.expand_dims(mfcc, axis=0), labels, [mfcc.shape[0]], [ids.size])
    finally:
        engine = getattr(network, 'engine', None)        # the handle goes with the call, not with the collector
        if engine is not None:
            engine.close()
    return report(config, timed, score, sp)


if __name__ == '__main__':
    main()
