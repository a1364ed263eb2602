"""GPU, two processes: LAS.train / validate with one process per tower (two ranks on the one GPU, gloo) against ONE process
time-slicing the same two towers, with scheduled sampling on (p = 0.1): both layouts draw every tower's samples with the
step's counter and the tower's index, so they feed the same inputs and reach the same parameters and sampling state."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

STEPS = 3


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _net_worker(rank, world, port, cfg_path, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), LOCAL_RANK='0', RANK=str(rank), WORLD_SIZE=str(world))
    import torch
    import torch.distributed as dist
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        cfg = Config(cfg_path, True)
        cfg.model_dir = os.path.join(out_dir, 'model')
        net = cfg.load_network(fortraining=True)
        assert net.coll.world == 2 and net._towers() == (2, [rank])
        batch = DataSet(cfg.train_input, cfg).get_next_batch()
        outs = [net.train(*batch) for _ in range(STEPS)]
        v = net.validate(*batch)
        np.savez(os.path.join(out_dir, 'n%d.npz' % rank), params=net.engine.get_params(), outs=np.array(outs, np.float64),
                 valid=np.array(v, np.float64), counter=net.engine.sampling_state()[2])
    finally:
        dist.destroy_process_group()


def test_las_two_ranks_equal_two_time_sliced_towers(tmp_path):
    import torch.multiprocessing as mp
    from test_gpu_network import make_config
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    cfg_path = make_config(tmp_path, network='networks.las.LAS')
    mp.spawn(_net_worker, args=(2, _free_port(), cfg_path, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / 'n0.npz'), np.load(tmp_path / 'n1.npz')
    np.testing.assert_array_equal(r0['params'], r1['params'])
    assert int(r0['counter']) == int(r1['counter']) == STEPS + 1
    cfg = Config(cfg_path, True)
    assert cfg.num_gpus == 2
    cfg.model_dir = str(tmp_path / 'model_ref')
    ref = cfg.load_network(fortraining=True)                    # both towers in this process
    p0 = ref.engine.sampling_state()
    assert p0[0] == pytest.approx(0.1) and p0[2] == 0
    batch = DataSet(cfg.train_input, cfg).get_next_batch()
    want = np.array([ref.train(*batch) for _ in range(STEPS)], np.float64)
    valid = np.array(ref.validate(*batch), np.float64)
    assert ref.engine.sampling_state()[2] == STEPS + 1
    # losses and LERs: the ranks average theirs over the ranks, the single process over its towers
    np.testing.assert_allclose(r0['outs'], want, rtol=2e-5, atol=1e-6)
    np.testing.assert_allclose(r0['valid'], valid, rtol=2e-5, atol=1e-6)
    # the gradient mean is summed in a different order (all-reduce in fp32 vs the host's fp64): Adam amplifies the
    # last-bit differences of near-zero gradients up to the step size
    np.testing.assert_allclose(r0['params'], ref.engine.get_params(), rtol=0, atol=2e-4)
