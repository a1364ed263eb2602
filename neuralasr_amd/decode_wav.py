"""Transcribe one WAV file with a trained model (reference: decode_wav.py:12-32).
`python -m neuralasr_amd.decode_wav CONFIG WAV`: the features of utils.compute_mfcc_and_read_transcription, the
configured network's decoder, and a 'Decoded: ...' log line.  A network that takes audio (HipNetwork.takes_audio) gets the samples:
its features are made on the GPU and stay there.  Every other network class takes features, so every one works."""
import argparse

import numpy as np

from .config import Config
from .logger import get_logger
from .utils import compute_mfcc_and_read_transcription

logger = get_logger()


def report(config, output):
    str_decoded = config.symbols.convert_to_str(output)
    logger.info('Decoded: ' + str_decoded)
    return str_decoded


def decode(config, mfcc, seq_len, network=None):
    network = network or config.load_network(fortraining=False)
    return report(config, network.decode(mfcc, seq_len))


def main(argv=None):
    parser = argparse.ArgumentParser(description='Convert a given audio file into text using trained model.')
    parser.add_argument('config', help='Configuration file.')
    parser.add_argument('input', help='Audio file path')
    args = parser.parse_args(argv)
    config = Config(args.config, True)
    network = config.load_network(fortraining=False)
    if getattr(network, 'takes_audio', False):
        from .features import read_wav_native
        audio, rate = read_wav_native(args.input)
        return report(config, network.decode_audio([audio], [rate]))
    mfcc = compute_mfcc_and_read_transcription(args.input, config.samplerate, config.numcontext, config.numcep,
                                               kind=config.features, deltas=config.deltas)
    mfcc = np.expand_dims(mfcc, axis=0)
    seq_len = np.asarray(mfcc.shape[1], dtype=np.int32)
    return decode(config, mfcc, [seq_len], network)


if __name__ == '__main__':
    main()
