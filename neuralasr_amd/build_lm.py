"""Build the n-gram model of the beam searches from the training set's labels (lm.py).

  python -m neuralasr_amd.build_lm CONFIG [--order N] [--delta D] [--output FILE]

Reads the label id sequences of the pickled training set ([Train] input) and writes one .npz: to --output, else to the
config's lm_file, else to <[MFCC Featurizer] output>/lm.npz."""
import argparse
import os

from . import lm
from .config import Config
from .logger import get_logger

logger = get_logger()


def build_lm(config, order=3, delta=0.5, output=None):
    sequences, bos_id = lm.label_sequences(config)
    model = lm.build(sequences, order, config.symbols.counter, bos_id, delta)
    output = output or config.lm_file or os.path.join(config.mfcc_output or '.', 'lm.npz')
    model.save(output)
    logger.info('Wrote an order-%d model over %d symbols (%d contexts, bos_id %d) counted on %d sequences to: %s' % (
        model.order, model.num_classes, model.K, model.bos_id, len(sequences), output))
    return output


def main(argv=None):
    ap = argparse.ArgumentParser(description='Build an n-gram language model over the training labels.')
    ap.add_argument('config', help='Configuration file.')
    ap.add_argument('--order', type=int, default=3, help='n-gram order, 1..4 (default 3)')
    ap.add_argument('--delta', type=float, default=0.5, help='Dirichlet smoothing weight per outcome (default 0.5)')
    ap.add_argument('--output', help='model file (default: the config\'s lm_file)')
    args = ap.parse_args(argv)
    return build_lm(Config(args.config, True), args.order, args.delta, args.output)


if __name__ == '__main__':
    main()
