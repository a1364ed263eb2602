"""Transcribe one WAV file with a trained model (reference: decode_wav.py:12-32).
`python -m neuralasr_amd.decode_wav CONFIG WAV`: the features of utils.compute_mfcc_and_read_transcription, the
configured network's decoder, and a 'Decoded: ...' log line.  A network that takes audio (HipNetwork.takes_audio) gets the samples:
its features are made on the GPU and stay there.  Every other network class takes features, so every one works.
With ema_decay in the config the network loads the checkpoint's averaged parameters.
`--stream [--chunk-frames N]`: a causal network (LstmCTCNet) is fed the file's frames N at a time (default 50 = 0.5 s), with a
'Partial: ...' line after every chunk whose hypothesis changed.  With normalization=utterance (the default) the features
are computed over the whole file first: the reference normalises by whole-utterance mean and std (utils.py:29), so frames a
model trained that way understands exist only then.  With normalization=causal the SAMPLES are fed,
N * frame_step per feed, and the session's front end normalises as they arrive; a file at another rate than the config's
is resampled whole on the GPU first and then chunked.
`--lookahead-frames R`: a bidirectional network (BiLstmConcatCTCNet, BiLstm3x500CTCNet, DeepSpeech without dropout) streams
with R frames of look-ahead (default: the config key stream_lookahead) on either route; its partial
hypotheses trail the audio by the chunk plus R frames, and the text depends on the chunking."""
import argparse

import numpy as np

from .config import Config
from .logger import get_logger
from .utils import compute_mfcc_and_read_transcription, normalization_of

logger = get_logger()


def report(config, output):
    str_decoded = config.symbols.convert_to_str(output)
    logger.info('Decoded: ' + str_decoded)
    return str_decoded


def decode(config, mfcc, seq_len, network=None):
    network = network or config.load_network(fortraining=False)
    return report(config, network.decode(mfcc, seq_len))


def features_of(config, network, path):
    """The file's normalised, context-stacked frames [T, feature_size] on the host, from the network's GPU front end when it
    has one"""
    if getattr(network, 'takes_audio', False):
        from .features import read_wav_native
        audio, rate = read_wav_native(path)
        return np.asarray(network.featurizer().compute([audio], rates=[rate])[0], dtype=np.float32)
    return np.asarray(compute_mfcc_and_read_transcription(path, config.samplerate, config.numcontext, config.numcep,
                                                          kind=config.features, deltas=config.deltas,
                                                          **normalization_of(config)), dtype=np.float32)


def decode_stream(config, network, feats, chunk_frames, lookahead=None):
    """Feed feats [T, F] to network.stream() chunk_frames at a time: a 'Partial:' line after every chunk whose hypothesis
    changed, then the usual 'Decoded:' line.  Returns the final text.  lookahead: the look-ahead frames of a bidirectional
    network (None: the config's stream_lookahead)."""
    if chunk_frames < 1:
        raise ValueError('--chunk-frames must be >= 1')
    rec = network.stream(1) if lookahead is None else network.stream(1, lookahead=lookahead)
    try:
        last = None
        for t in range(0, len(feats), chunk_frames):
            ids = rec.feed([feats[t:t + chunk_frames]])[0]
            if ids != last:
                logger.info('Partial: ' + config.symbols.convert_to_str(np.asarray(ids, dtype=np.int64)))
                last = ids
        ids, _ = rec.finish(0)
    finally:
        rec.close()
    return report(config, np.asarray(ids, dtype=np.int64))


def decode_stream_audio(config, network, audio, rate, chunk_frames, lookahead=None):
    """Feed the file's SAMPLES to network.stream(), chunk_frames * frame_step at a time (normalization=causal): the same
    'Partial:' and 'Decoded:' lines as decode_stream.  A file at another rate is resampled whole first."""
    if chunk_frames < 1:
        raise ValueError('--chunk-frames must be >= 1')
    fz = network.featurizer()
    if rate != config.samplerate:
        audio = fz.resample([audio], [rate])[0]
    step = chunk_frames * fz.frame_params()[1]
    rec = network.stream(1) if lookahead is None else network.stream(1, lookahead=lookahead)
    try:
        prev = None
        for t in range(0, len(audio), step):
            ids = rec.feed_audio([audio[t:t + step]], [t + step >= len(audio)])[0]
            if ids != prev:
                logger.info('Partial: ' + config.symbols.convert_to_str(np.asarray(ids, dtype=np.int64)))
                prev = ids
        ids, _ = rec.finish(0)
    finally:
        rec.close()
    return report(config, np.asarray(ids, dtype=np.int64))


def parse_args(argv=None):
    parser = argparse.ArgumentParser(description='Convert a given audio file into text using trained model.')
    parser.add_argument('config', help='Configuration file.')
    parser.add_argument('input', help='Audio file path')
    parser.add_argument('--stream', action='store_true',
                        help='feed the file in chunks to a causal network and log partial hypotheses: its samples when the '
                             'config says normalization=causal (a file at another rate is resampled whole on the GPU '
                             'first and then chunked), else the frames of the features computed over the whole file')
    class _Given(argparse.Action):      # (main() tells a --chunk-frames that was given from the default)
        def __call__(self, parser, namespace, values, option_string=None):
            setattr(namespace, self.dest, values)
            setattr(namespace, self.dest + '_given', True)
    parser.set_defaults(chunk_frames_given=False)
    parser.add_argument('--chunk-frames', type=int, default=50, action=_Given,
                        help='frames per chunk with --stream (default: the config key chunk_frames when it is set, else 50 = 0.5 s); '
                             'samples are fed chunk-frames * frame_step at a time.  Input frames, whatever frame_skip says')
    parser.add_argument('--lookahead-frames', type=int, default=None,
                        help='with --stream on a bidirectional network: frames of right context the backward direction gets '
                             'beyond the frames a feed emits (overrides the config key stream_lookahead)')
    args = parser.parse_args(argv)
    if args.chunk_frames < 1:
        parser.error('--chunk-frames must be >= 1')
    if args.lookahead_frames is not None and args.lookahead_frames < 1:
        parser.error('--lookahead-frames must be >= 1')
    return args


def main(argv=None):
    args = parse_args(argv)
    config = Config(args.config, True)
    network = config.load_network(fortraining=False)
    if not args.chunk_frames_given and getattr(config, 'chunk_frames', 0) > 0:
        # a model trained in windows is served with the chunk it was trained with: chunk_frames counts the
        # network's frames, --chunk-frames input frames
        args.chunk_frames = config.chunk_frames * getattr(config, 'frame_skip', 1)
    if args.stream:
        if not hasattr(network, 'stream'):
            raise SystemExit('--stream: network %s cannot stream' % type(network).__name__)
        if getattr(config, 'normalization', 'utterance') == 'causal':
            from .features import read_wav_native
            audio, rate = read_wav_native(args.input)
            return decode_stream_audio(config, network, audio, rate, args.chunk_frames, args.lookahead_frames)
        return decode_stream(config, network, features_of(config, network, args.input), args.chunk_frames, args.lookahead_frames)
    if getattr(network, 'takes_audio', False):
        from .features import read_wav_native
        audio, rate = read_wav_native(args.input)
        return report(config, network.decode_audio([audio], [rate]))
    mfcc = compute_mfcc_and_read_transcription(args.input, config.samplerate, config.numcontext, config.numcep,
                                               kind=config.features, deltas=config.deltas, **normalization_of(config))
    mfcc = np.expand_dims(mfcc, axis=0)
    seq_len = np.asarray(mfcc.shape[1], dtype=np.int32)
    return decode(config, mfcc, [seq_len], network)


if __name__ == '__main__':
    main()
