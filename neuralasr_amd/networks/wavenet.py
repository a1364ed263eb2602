"""WaveNet (reference: networks/wavenet.py:7-175): a 1x1 convolution with batch norm and tanh, num_blocks x rates residual
blocks of gated dilated convolutions (kernel size 7) with batch norm, a 1x1 convolution with batch norm and tanh over the
skip sum and a last 1x1 convolution to the classes; every convolution is bias-free.  The locals of the reference's
create_network are class attributes here.  `network=networks.wavenet.WaveNet` selects it.

Batch norm is tf.contrib.layers.batch_norm (decay 0.99, epsilon 1e-3, zero_debias_moving_mean, updates_collections=None):
train() normalises with the batch's statistics and updates the moving ones; validate / evaluate / decode use the moving
statistics.  With num_gpus > 1 every tower normalises with its own statistics and applies its own update (make_parallel
shares the variables): time-sliced towers in one process apply theirs in tower order, processes exchange their batch
statistics over the torch.distributed group and apply them in rank order, so every rank holds the same moving statistics.
Checkpoints carry the batch-norm state (bn_moving_mean, bn_moving_var, bn_biased, bn_updates) beside the variables."""
import numpy as np

from ..engine import WaveNetEngine
from .hipnetwork import HipNetwork


class WaveNet(HipNetwork):
    num_blocks = 3
    rates = (1, 2, 4, 8, 16)
    num_dim = 128
    kernel_size = 7
    bn_decay = 0.99
    bn_epsilon = 1e-3                      # tf.contrib.layers.batch_norm's default
    num_hidden = num_dim                   # (checkpoint meta)
    num_layers = 0
    bidirectional = False
    merge = 'none'

    def make_engine(self, config, device, stream):
        e = WaveNetEngine(config.feature_size, self.num_classes, num_blocks=self.num_blocks, rates=self.rates,
                          dim=self.num_dim, kernel_size=self.kernel_size, bn_epsilon=self.bn_epsilon,
                          bn_decay=self.bn_decay, learning_rate=config.learningrate, device_id=device, stream=stream)
        if self.coll.world > 1:
            e.set_bn_hold(True)            # after_compute_grads applies every rank's update in rank order
        return e

    @staticmethod
    def fan_in(name, rows, cols, kernel_size=7):
        """wavenet.py:_get_fans: the 1x1 conv1d kernels are 3-D [1, in, out] and fall into its "no specific assumptions"
        branch, fan_in = sqrt(1*in*out); the dilated kernels are 4-D [1, k, in, out], fan_in = k*in."""
        if '/conv_filter' in name or '/conv_gate' in name:
            return float(rows)             # rows = k * in
        return float(np.sqrt(rows * cols))

    def initial_params(self, tensors, seed):
        """he_uniform: U(-sqrt(1/fan_in), sqrt(1/fan_in)) for the kernels; beta 0, gamma 1."""
        rs = np.random.RandomState(seed)
        chunks = []
        for name, _, rows, cols in tensors:
            if name.endswith('/W'):
                s = np.sqrt(1.0 / self.fan_in(name, rows, cols))
                chunks.append(rs.uniform(-s, s, size=rows * cols))
            elif name.endswith('/gamma'):
                chunks.append(np.ones(rows * cols))
            else:
                chunks.append(np.zeros(rows * cols))
        return np.concatenate(chunks).astype(np.float32)

    def model_state(self):
        mm, mv, bs, n = self.engine.bn_state()
        return {'bn_moving_mean': mm, 'bn_moving_var': mv, 'bn_biased': bs, 'bn_updates': np.int64(n)}

    def restore_model_state(self, npz):
        if 'bn_moving_mean' in npz:
            self.engine.set_bn_state(npz['bn_moving_mean'], npz['bn_moving_var'], npz['bn_biased'], int(npz['bn_updates']))

    def after_compute_grads(self):
        """The towers' moving-statistics updates, in rank order, on every rank."""
        import torch
        m, v = self.engine.batch_stats()
        t = torch.from_numpy(np.concatenate([m.ravel(), v.ravel()]))
        parts = [torch.empty_like(t) for _ in range(self.coll.world)]
        self.coll.dist.all_gather(parts, t, group=self.coll.scalar_group)
        k = m.size
        self.engine.apply_bn_stats([p[:k].numpy().reshape(m.shape) for p in parts],
                                   [p[k:].numpy().reshape(m.shape) for p in parts])
