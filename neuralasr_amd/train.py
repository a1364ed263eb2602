"""Training loop (reference: train.py:14-63): epochs x batches, cumulative wall time, checkpoint + log +
one validation batch every report_step, same log-line formats (plus one "Grad:" line behind every "Step:" line when the
config's max_grad_norm switches gradient clipping on, one "Distill:" line when its teacher_config switches
distillation on, and one "LR:" line when one of its lr_* keys sets a learning-rate schedule).

  python -m neuralasr_amd.train <config>
  python -m neuralasr_amd.train <config> --from-audio     # from the [MFCC Featurizer] input CSV: features made on the GPU per batch
  python -m torch.distributed.run --nproc-per-node N -m neuralasr_amd.train <config>   # num_gpus = N"""
import argparse
import os
import time

from .config import Config
from .dataset import DataSet
from .logger import get_logger

logger = get_logger()


def train_model(dataTrain, datavalid, config, prefetch=2):
    """The loop of train.py:14-47.  With a network that offers begin_step / finish_step / stage_batch (HipNetwork) the
    next batch is loaded, padded and staged towards the GPU BETWEEN the two halves of a step, i.e. while the device runs
    that step: one host thread, no idle device.  `prefetch` = 0 keeps the reference's order (load, then train) with
    synchronous uploads; other networks get a loader thread that runs `prefetch` batches ahead."""
    logger.info('Batch Dimensions: ' + str(dataTrain.get_feature_shape()))
    logger.info('Label Dimensions: ' + str(dataTrain.get_label_shape()))
    network = config.load_network(fortraining=True)
    spent, loss_sum, ler_sum = 0.0, 0.0, 0.0     # train_time_sec is never reset (train.py:20,26,34)
    counted = 0                                  # steps of the window whose values count (all of them, normally)
    split = prefetch and all(hasattr(network, a) for a in ('begin_step', 'finish_step', 'stage_batch'))
    lazy_ok = split and hasattr(network, 'mean_over_ranks')      # finish_step(lazy=True) is HipNetwork's

    window = []                                   # (loss, mean_ler or a handle with .result()) of the steps since the last log line

    def report(loss, mean_ler):
        nonlocal loss_sum, ler_sum, counted
        window.append((loss, mean_ler))
        if network.global_step % config.report_step == 0:
            lazy = False
            for lo, le in window:
                if hasattr(le, 'result'):             # HipNetwork: the step's beam search ran on host threads meanwhile
                    le, lazy = le.result(), True
                # a step whose forward pass was void on some rank (HipNetwork: a persistent-recurrence abort, repeated one
                # call later) reports NaN on every rank: it stays out of the window's means instead of turning them into NaN
                if lo == lo and le == le:
                    loss_sum += lo
                    ler_sum += le
                    counted += 1
            del window[:]
            if lazy and hasattr(network, 'mean_over_ranks'):
                ler_sum = network.mean_over_ranks(ler_sum)     # lazily decoded LERs are local until here (one collective per log line)
            network.save_checkpoint()
            # train.py:32-34 divides by report_step; `counted` equals it unless a void step was left out
            den = counted if 0 < counted < config.report_step else config.report_step
            logger.info('Step: %04d' % network.global_step + ', cost = %.4f' % (loss_sum / den) +
                        ', ler = %.4f' % (ler_sum / den) + ', time = %.4f' % spent)
            loss_sum = ler_sum = 0.0
            counted = 0
            if getattr(config, 'lr_schedule_on', False):
                # lr_warmup_steps / lr_decay_* (DESIGN.md §23): the step size this step was applied with
                logger.info('LR: %.6g' % config.learning_rate_at(network.global_step))
            if getattr(config, 'max_grad_norm', 0.0) > 0:
                # max_grad_norm: the optimiser steps since the last log line, read where save_checkpoint has
                # just waited for the device anyway
                gc = network.engine.grad_clip_stats(reset=True)
                logger.info('Grad: norm = %.4f' % gc['last_norm'] + ', max = %.4f' % gc['window_max_norm'] +
                            ', clipped %d of %d' % (gc['clipped'], gc['steps']) + ', skipped %d' % gc['skipped'])
                if gc['skipped'] > 0:
                    logger.warning('%d optimiser step(s) skipped: their gradient had a non-finite norm (parameters and Adam '
                                   'state were left as they were)' % gc['skipped'])
            if getattr(config, 'teacher_config', None):
                # teacher_config: the two parts of the last step's loss, read behind the same wait
                ctc, kd = network.engine.distill_loss()
                logger.info('Distill: ctc = %.4f' % ctc + ', kd = %.4f' % kd)
            if datavalid:
                if not datavalid.has_more_batches():
                    datavalid.reset_epoch()
                vm, vl, vs, vll = datavalid.get_next_batch()
                vloss, vler = network.validate(vm, vl, vs, vll)
                logger.info('Valid: cost = %.4f' % vloss + ', ler = %.4f' % vler)

    if split:
        def all_batches():                                # epochs x batches, in the reference's order
            for _ in range(config.epochs):
                while dataTrain.has_more_batches():
                    yield dataTrain.get_next_batch()
                dataTrain.reset_epoch()
        it = all_batches()
        t0 = time.time()
        cur = next(it, None)
        while cur is not None:
            network.begin_step(*cur)
            nxt = next(it, None)                          # loaded, padded and staged under the step the device is running
            if nxt is not None:
                network.stage_batch(*nxt)
            loss, mean_ler = network.finish_step(lazy=True) if lazy_ok else network.finish_step()
            spent += time.time() - t0
            report(loss, mean_ler)
            t0 = time.time()
            cur = nxt
        network.discard_staged()
        logger.info('Finished training!!!')
        return network
    for _ in range(config.epochs):
        batches = dataTrain.prefetch(prefetch) if prefetch else iter(dataTrain.get_next_batch, None)
        while True:
            t0 = time.time()
            if not prefetch and not dataTrain.has_more_batches():
                break
            try:
                mfccs, labels, seq_len, labels_len = next(batches)
            except StopIteration:
                break
            loss, mean_ler = network.train(mfccs, labels, seq_len, labels_len)
            spent += time.time() - t0
            report(loss, mean_ler)
        dataTrain.reset_epoch()
        if hasattr(network, 'discard_staged'):
            network.discard_staged()
    logger.info('Finished training!!!')
    return network


def main(argv=None):
    ap = argparse.ArgumentParser(description='Train speech recognizer on featurized mfcc files.')
    ap.add_argument('config', help='Configuration file.')
    ap.add_argument('--from-audio', action='store_true',
                    help='read WAV files and transcripts from the [MFCC Featurizer] input CSV instead of pickled features; '
                         'the features are made on the GPU for every batch (needs rand_shift=0)')
    args = ap.parse_args(argv)
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')))
        dist.init_process_group('nccl')
    config = Config(args.config, isTraining=True)
    if args.from_audio:
        dataTrain, dataValid = audio_datasets(args.config, config)
    else:
        if config.augment_on:
            raise ValueError('the augmentation keys (spec_time_masks, spec_freq_masks, speed_perturb, noise_list, rir_list) need '
                             '--from-audio: the masks, the perturbed rates, the noise and the reverberation are applied where the '
                             'GPU makes the features; pickled features are not masked')
        dataTrain = DataSet(config.train_input, config)
        dataValid = None
        if config.test_input:
            config_test = Config(args.config, isTraining=True)
            config_test.epochs = None
            dataValid = DataSet(config_test.test_input, config_test)
    return train_model(dataTrain, dataValid, config)


def audio_datasets(configfile, config):
    """--from-audio: the training and the validation set of the [MFCC Featurizer] input CSV as train_model reads them.
    The batches hold audio (features.AudioBatch); HipNetwork stages and uploads them through the GPU front end.  With an
    augmentation key switched on the training feed draws speed factors, SpecAugment masks, noise clips and room impulse
    responses (augment.py)."""
    from .audio_dataset import AudioDataSet, AudioFeed
    if config.rand_shift > 0:
        raise ValueError('--from-audio cannot be combined with rand_shift > 0 (rand_shift=%d): the roll-and-crop leaves real '
                         'neighbour frames where the context pads were, and a batch from audio is rebuilt from centre frames '
                         'and pad values; set rand_shift=0 or train from the pickled features' % config.rand_shift)
    if not config.mfcc_input:
        raise ValueError("--from-audio needs 'input' in the [MFCC Featurizer] section of " + configfile)
    augmenter = None
    if config.augment_on:       # the training feed only: validation and decode never augment
        import torch.distributed as dist
        from .augment import Augmenter
        augmenter = Augmenter(config, rank=dist.get_rank() if dist.is_available() and dist.is_initialized() else 0)
    dataTrain = AudioFeed(AudioDataSet(config.mfcc_input, config, 'train'), augmenter)     # (writes the symbol table when there is none)
    dataValid = None
    if config.test_input:
        config_test = Config(configfile, isTraining=True)
        config_test.epochs = None
        valid = AudioDataSet(config_test.mfcc_input, config_test, 'test')
        dataValid = AudioFeed(valid) if valid.get_num_of_sample() else None
    return dataTrain, dataValid


if __name__ == '__main__':
    main()
