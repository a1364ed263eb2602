"""Evaluation over the test list, one utterance at a time (reference: decode.py:14-54).
With ema_decay in the config the network loads the checkpoint's averaged parameters.

  python -m neuralasr_amd.decode <config>
  python -m neuralasr_amd.decode <config> --from-audio    # the test set of the [MFCC Featurizer] input CSV: features made on the GPU"""
import argparse
import time

import numpy as np

from .config import Config, network_class
from .dataset import DataSet
from .logger import get_logger

logger = get_logger()


def decode(dataTest, config):
    logger.info('Batch Dimensions: ' + str(dataTest.get_feature_shape()))
    logger.info('Label Dimensions: ' + str(dataTest.get_label_shape()))
    network = config.load_network(fortraining=False)
    steps, spent, loss_sum, ler_sum = 0, 0.0, 0.0, 0.0
    while dataTest.has_more_batches():
        steps += 1
        t0 = time.time()
        mfccs, labels, seq_len, labels_len = dataTest.get_next_batch()
        output, loss, ler = network.evaluate(mfccs, labels, seq_len, labels_len)
        logger.info('Valid: batch_cost = %.4f' % loss + ', batch_ler = %.4f' % ler)
        spent += time.time() - t0
        loss_sum += loss
        ler_sum += ler
        logger.info('Decoded: ' + config.symbols.convert_to_str(np.asarray(output).ravel()))
        logger.info('Original: ' + config.symbols.convert_to_str(np.asarray(labels[0])))
    logger.info('Finished Decoding!!!')
    logger.info('Decoded Time = %.4fs, avg_loss = %.4f, avg_ler = %.4f' % (spent, loss_sum / steps, ler_sum / steps))


def main(argv=None):
    ap = argparse.ArgumentParser(description='Decode test data using trained model.')
    ap.add_argument('config', help='Configuration file.')
    ap.add_argument('--from-audio', action='store_true',
                    help='read the test set\'s WAV files and transcripts from the [MFCC Featurizer] input CSV instead of '
                         'pickled features; the features are made on the GPU for every utterance')
    args = ap.parse_args(argv)
    config = Config(args.config, True)
    config.batch_size = 1
    config.epochs = 1
    config.rand_shift = 0
    decode(audio_dataset(args.config, config) if args.from_audio else DataSet(config.test_input, config), config)


def audio_dataset(configfile, config):
    """--from-audio: the test set of the [MFCC Featurizer] input CSV as decode() reads a DataSet; the batches hold audio
    (features.AudioBatch), which a network with takes_audio evaluates through the GPU front end."""
    from .audio_dataset import AudioDataSet, AudioFeed
    if not config.mfcc_input:
        raise ValueError("--from-audio needs 'input' in the [MFCC Featurizer] section of " + configfile)
    if not getattr(network_class(config.network), 'takes_audio', False):
        raise ValueError('--from-audio needs a network that takes audio; %s takes features: run preprocess_mfcc and '
                         'decode without the flag' % config.network)
    return AudioFeed(AudioDataSet(config.mfcc_input, config, 'test'))


if __name__ == '__main__':
    main()
