"""GPU: the WaveNet CTC network (nasr_create_wavenet, networks/wavenet.py) against the independent fp64 torch-CPU model of
tests/wavenet_ref.py: logits, loss, every gradient tensor and the batch statistics of a training-mode pass, the halo of
the dilated convolutions at small T, the batch padding, empty labels, Adam steps with the moving-statistics updates,
inference with the moving statistics, determinism, the full-size step, the plugin end to end and two ranks.

Errors are measured as |got - want| / |want| (2-norm) per tensor, with |want| floored at 1e-3 of the whole gradient's norm:
with two rows per channel (B 1, T 2) batch norm's output no longer depends on its input (x_hat = +-1 up to epsilon) and the
gradients of the convolutions before it cancel to what epsilon leaves.  The tolerances are about 3x what an MI355X showed
(WaveNet section; the measured values are next to each tolerance)."""
import json
import os
import socket
import types

import numpy as np
import pytest

import wavenet_ref as W

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLES = os.path.join(HERE, 'golden', 'sample_set')

# small shapes: measured loss <= 4e-7 relative, gradient tensors <= 2.9e-6, batch mean / variance <= 5e-7
TOL_LOSS, TOL_GRAD = 1.5e-6, 1e-5
# two rows per channel (B 1, T 2): measured loss 1.8e-6, gradient tensors 1.5e-3 (see test_halo_...)
TOL_LOSS_N2, TOL_GRAD_N2 = 1e-5, 5e-3
# full size (B 16, T 500, F 546): measured loss 8e-8, gradient tensors <= 1.35e-5 (front/conv_in/W)
TOL_LOSS_FULL, TOL_GRAD_FULL = 3e-7, 6e-5
# three Adam steps against three torch steps: loss of steps 2-3 (measured 1.8e-7), the whole update (1.0e-4), Adam's
# moments (3.3e-5), BN state (7.7e-6 of max|state| + 1)
TOL_LOSS_STEPS, TOL_UPDATE, TOL_MOMENTS, TOL_BN = 1e-6, 5e-4, 1e-4, 3e-5


def rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / nb) if nb > 0 else float(np.linalg.norm(a))


def engine(spec, lr=1e-3, **kw):
    from neuralasr_amd.engine import WaveNetEngine
    return WaveNetEngine(spec.F, spec.C, num_blocks=spec.nb, rates=spec.rates, learning_rate=lr, **kw)


def start_params(spec, seed):
    """he_uniform kernels, gamma and beta moved off 1 and 0 so that their gradients' paths are exercised."""
    p = W.init_params(spec, seed).astype(np.float64)
    rs = np.random.RandomState(seed + 100)
    o = 0
    for name, r, c in W.tensor_specs(spec):
        if name.endswith('gamma'):
            p[o:o + r] = 1 + 0.2 * rs.randn(r)
        elif name.endswith('beta'):
            p[o:o + r] = 0.2 * rs.randn(r)
        o += r * c
    return p.astype(np.float32)


def grad_errors(spec, e, g, g_ref):
    out = {}
    floor = 1e-3 * np.linalg.norm(np.asarray(g_ref, np.float64))
    for name, off, r, c in e.tensors():
        a, b = np.asarray(g[off:off + r * c], np.float64), np.asarray(g_ref[off:off + r * c], np.float64)
        out[name] = float(np.linalg.norm(a - b) / max(np.linalg.norm(b), floor))
    return out


def check_pass(spec, e, flat, feats, seq, labels, ll, tol_loss, tol_grad, report=None):
    loss, nll, g = e.loss_and_grads(feats, seq, labels, ll)
    loss_r, g_r, stats = W.loss_and_grads(spec, flat, feats, seq, labels, ll)
    errs = grad_errors(spec, e, g, g_r)
    m, v = e.batch_stats()
    m_r, v_r = W.update_variance(spec, stats)
    worst = max(errs, key=errs.get)
    if report is not None:
        report.update(loss=abs(loss - loss_r) / abs(loss_r), grad=errs[worst], worst=worst,
                      mean=rel(m, m_r), var=rel(v, v_r))
    assert abs(loss - loss_r) <= tol_loss * abs(loss_r), (loss, loss_r)
    assert errs[worst] <= tol_grad, (worst, errs[worst])
    assert rel(v, v_r) <= tol_grad and np.abs(m - m_r).max() <= tol_grad * (np.abs(m_r).max() + 1)
    return loss, g


def test_full_model_training_pass_against_torch():
    spec = W.Spec(39, 29)
    e = engine(spec)
    assert e.param_count == sum(r * c for _, r, c in W.tensor_specs(spec))
    assert [n for n, _, _, _ in e.tensors()] == [n for n, _, _ in W.tensor_specs(spec)]
    flat = start_params(spec, 5)
    e.set_params(flat)
    np.testing.assert_array_equal(e.get_params(), flat)
    feats, seq, labels, ll = W.synth_batch(spec, 5, 60, seed=7, Lmax=8)
    assert len(set(seq.tolist())) > 1
    e.set_step_decode(True, logits=True, greedy=False)
    rep = {}
    check_pass(spec, e, flat, feats, seq, labels, ll, TOL_LOSS, TOL_GRAD, rep)
    # the training pass's own logits (batch statistics), as the step publishes them
    lg = e.step_logits(5, 60)
    lg_r, _ = W.forward(spec, W.unflatten(spec, flat), feats, True)
    lg_r = lg_r.detach().numpy()
    for b in range(5):
        assert rel(lg[:seq[b], b], lg_r[:seq[b], b]) < TOL_GRAD
    print('full model, B 5 T 60:', json.dumps(rep))
    e.close()


@pytest.mark.parametrize('T', [1, 2, 7, 40])
@pytest.mark.parametrize('B', [1, 17, 64])
def test_halo_batch_padding_and_empty_labels(B, T):
    """T below the receptive field (every tap of rate 16 falls outside at T = 7), a batch padded to Bp = 16 / 32 / 64 rows
    (those rows must not enter the statistics), one utterance with an empty label."""
    spec = W.Spec(11, 7, num_blocks=1)
    e = engine(spec)
    flat = start_params(spec, 9)
    e.set_params(flat)
    rs = np.random.RandomState(B * 100 + T)
    seq = rs.randint(1, T + 1, size=B)
    seq[0] = T
    ll = [0] + [min(2, (int(s) - 1) // 2) for s in seq[1:]]
    feats, seq, labels, ll = W.synth_batch(spec, B, T, seed=B + T, seq_len=seq, label_len=ll)
    rep = {}
    # two rows per channel: batch norm's output is +-1 up to epsilon, its input gradient the cancellation of two terms
    # ~1e3 times larger (measured 1.5e-3 for a conv kernel at B 1, T 2)
    n2 = B * T == 2
    check_pass(spec, e, flat, feats, seq, labels, ll, TOL_LOSS_N2 if n2 else TOL_LOSS, TOL_GRAD_N2 if n2 else TOL_GRAD, rep)
    print('B %d T %d:' % (B, T), json.dumps(rep))
    e.close()


def bn_close(e, st, tol=2e-6):
    mm, mv, bs, n = e.bn_state()
    assert n == st['n']
    for got, want in ((mm, st['mm']), (mv, st['mv']), (bs, st['biased'])):
        assert np.abs(got - want).max() <= tol * (np.abs(want).max() + 1), np.abs(got - want).max()


def test_three_adam_steps_then_inference_with_the_moving_statistics():
    spec = W.Spec(39, 29, num_blocks=1, rates=(1, 2, 4))
    lr = 1e-3
    e = engine(spec, lr=lr)
    flat = start_params(spec, 11)
    e.set_params(flat)
    feats, seq, labels, ll = W.synth_batch(spec, 6, 30, seed=12, Lmax=6)
    p = flat.astype(np.float64)
    m = np.zeros_like(p)
    v = np.zeros_like(p)
    st = W.bn_initial(spec)
    rep = {}
    for t in range(1, 4):
        loss = e.train_step(feats, seq, labels, ll)
        loss_r, g, stats = W.loss_and_grads(spec, p.astype(np.float32), feats, seq, labels, ll)
        rep['loss%d' % t] = abs(loss - loss_r) / abs(loss_r)
        p, m, v = W.adam_tf(p, g, m, v, t, lr)
        st = W.bn_update(spec, st, *W.update_variance(spec, stats))
    got_p = e.get_params()
    gm, gv, step = e.get_adam_state()
    # Adam divides by sqrt(v): entries whose gradient is ~1e-8 move by a rounding-sized fraction of lr either way, so the
    # update is compared as a whole, and the two parameter paths part by that much from step 2 on
    rep['update'] = rel(got_p.astype(np.float64) - flat, p - flat)
    rep['adam_m'] = max(rel(gm[o:o + r * c], m[o:o + r * c]) for _, o, r, c in e.tensors())
    rep['adam_v'] = max(rel(gv[o:o + r * c], v[o:o + r * c]) for _, o, r, c in e.tensors())
    mm, mv, bs, n = e.bn_state()
    rep['bn'] = max(float(np.abs(a - b).max() / (np.abs(b).max() + 1))
                    for a, b in ((mm, st['mm']), (mv, st['mv']), (bs, st['biased'])))
    print('three steps:', json.dumps(rep))
    assert step == 3 and n == 3
    assert rep['loss1'] <= TOL_LOSS and max(rep['loss2'], rep['loss3']) <= TOL_LOSS_STEPS
    assert rep['update'] < TOL_UPDATE and rep['adam_m'] < TOL_MOMENTS and rep['adam_v'] < TOL_MOMENTS
    assert rep['bn'] < TOL_BN
    # inference (validate / evaluate / decode): the moving statistics, nothing updated
    e.set_params(p.astype(np.float32))
    mm, mv, _, _ = e.bn_state()
    loss, nll = e.loss(feats, seq, labels, ll)
    loss_r, nll_r, lg_r = W.eval_loss(spec, p.astype(np.float32), feats, seq, labels, ll, (mm, mv))
    assert abs(loss - loss_r) <= TOL_LOSS * abs(loss_r)
    assert rel(nll, nll_r) <= TOL_LOSS
    lg = e.forward(feats, seq)
    for b in range(6):
        assert rel(lg[:seq[b], b], lg_r[:seq[b], b]) < TOL_GRAD
    assert e.greedy_decode(feats, seq) == W.greedy(lg_r, seq)
    for a, b in zip(e.bn_state(), (mm, mv, bs, n)):     # unchanged by the inference calls
        np.testing.assert_array_equal(a, b)
    e.close()


def test_two_runs_are_bitwise_equal():
    spec = W.Spec(39, 29)
    e = engine(spec)
    flat = start_params(spec, 13)
    feats, seq, labels, ll = W.synth_batch(spec, 9, 45, seed=14)
    out = []
    for _ in range(2):
        e.set_params(flat)
        st0 = W.bn_initial(spec)
        e.set_bn_state(st0['mm'], st0['mv'], st0['biased'], 0)
        loss, nll, g = e.loss_and_grads(feats, seq, labels, ll)
        out.append((loss, g, e.bn_state()))
    (l0, g0, s0), (l1, g1, s1) = out
    assert l0 == l1
    np.testing.assert_array_equal(g0, g1)
    for a, b in zip(s0, s1):
        np.testing.assert_array_equal(a, b)
    e.close()


def test_full_size_step_against_torch():
    spec = W.Spec(546, 29)
    e = engine(spec)
    assert e.param_count == 3788416
    flat = start_params(spec, 17)
    e.set_params(flat)
    feats, seq, labels, ll = W.synth_batch(spec, 16, 500, seed=18, Lmax=60)
    rep = {}
    check_pass(spec, e, flat, feats, seq, labels, ll, TOL_LOSS_FULL, TOL_GRAD_FULL, rep)
    print('full size:', json.dumps(rep))
    e.close()


# ---------------------------------------------------------------------------------------------- the plugin
def make_config(tmp_path, **over):
    lines = open(os.path.join(SAMPLES, 'toy.config')).read().splitlines()
    over = dict({'output': SAMPLES, 'model_dir': str(tmp_path / 'model'), 'network': 'networks.wavenet.WaveNet'}, **over)
    out = []
    for ln in lines:
        key = ln.split('=')[0]
        out.append('%s=%s' % (key, over[key]) if key in over and '=' in ln else ln)
    p = tmp_path / 'toy.config'
    p.write_text('\n'.join(out) + '\n')
    return str(p)


def test_plugin_trains_resumes_and_infers(tmp_path):
    from neuralasr_amd import train as train_mod
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    cfg = Config(make_config(tmp_path, num_gpus=1, epochs=2), True)
    train = DataSet(cfg.train_input, cfg)
    valid = DataSet(cfg.test_input, Config(make_config(tmp_path, num_gpus=1), True))
    net = train_mod.train_model(train, valid, cfg)
    assert type(net).__name__ == 'WaveNet' and net.global_step >= 2
    step = net.global_step
    net.save_checkpoint()
    want_p = net.engine.get_params()
    want_m, want_v, want_s = net.engine.get_adam_state()
    want_bn = net.engine.bn_state()
    assert want_bn[3] == step
    with np.load(os.path.join(cfg.model_dir, 'model-%d.npz' % step)) as z:
        assert sorted(z.files) == ['adam_m', 'adam_v', 'bn_biased', 'bn_moving_mean', 'bn_moving_var', 'bn_updates',
                                   'meta', 'params', 'step']
    cfg2 = Config(make_config(tmp_path, num_gpus=1, start_step=step), True)
    net2 = cfg2.load_network(fortraining=True)
    np.testing.assert_array_equal(net2.engine.get_params(), want_p)
    m2, v2, s2 = net2.engine.get_adam_state()
    np.testing.assert_array_equal(m2, want_m)
    np.testing.assert_array_equal(v2, want_v)
    assert s2 == want_s
    for a, b in zip(net2.engine.bn_state(), want_bn):
        np.testing.assert_array_equal(a, b)
    # validate / evaluate / decode against torch eval with the moving statistics
    spec = W.Spec(cfg.feature_size, cfg.symbols.counter)
    ds = DataSet(cfg.test_input, cfg)
    mfccs, labels, seq_len, labels_len = ds.get_next_batch()
    sl = [int(s) for s in seq_len]
    loss_r, _, lg_r = W.eval_loss(spec, want_p, mfccs, sl, labels, labels_len, want_bn[:2])
    vl = net2.validate(mfccs, labels, seq_len, labels_len)
    assert float(vl[0]) == pytest.approx(loss_r, rel=TOL_LOSS)
    hy = net2.engine.beam_search(lg_r.astype(np.float32), sl, 100, merge_repeated=True)[0]
    ids, loss, ler = net2.evaluate(mfccs, labels, seq_len, labels_len)
    assert ids.tolist() == [i for h in hy for i in h]
    assert float(loss) == pytest.approx(loss_r, rel=TOL_LOSS)
    assert net2.decode(mfccs, seq_len).tolist() == [i for h in hy for i in h]
    for a, b in zip(net2.engine.bn_state(), want_bn):       # inference left the moving statistics alone
        np.testing.assert_array_equal(a, b)


def test_plugin_time_sliced_towers_apply_their_updates_in_tower_order(tmp_path):
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    from neuralasr_amd.parallel import take_shard
    cfg = Config(make_config(tmp_path, num_gpus=2, batch_size=4), True)
    net = cfg.load_network(fortraining=True)
    spec = W.Spec(cfg.feature_size, cfg.symbols.counter)
    flat = net.engine.get_params()
    ds = DataSet(cfg.train_input, cfg)
    mfccs, labels, seq_len, labels_len = ds.get_next_batch()
    st = W.bn_initial(spec)
    gsum = 0
    for k in range(2):
        f, l, s, ll = take_shard(mfccs, labels, seq_len, labels_len, 2, k)
        _, g, stats = W.loss_and_grads(spec, flat, f, [int(x) for x in s], l, ll)
        gsum = gsum + g
        st = W.bn_update(spec, st, *W.update_variance(spec, stats))
    loss, _ = net.train(mfccs, labels, seq_len, labels_len)
    assert np.isfinite(loss)
    bn_close(net.engine, st)
    p, _, _ = W.adam_tf(flat.astype(np.float64), gsum / 2, 0, 0, 1, cfg.learningrate)
    du = rel(net.engine.get_params().astype(np.float64) - flat, p - flat)
    print('two towers: update', du)
    assert du < 1e-3                                    # measured 2.6e-4


# ---------------------------------------------------------------------------------------------- two ranks
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


SPEC2 = dict(feature_size=15, num_classes=9, num_blocks=1, rates=(1, 4))


def _batch2():
    spec = W.Spec(15, 9, num_blocks=1, rates=(1, 4))
    return spec, W.synth_batch(spec, 8, 24, seed=21, Lmax=4)


def _worker(rank, world, port, out_dir):
    os.environ['MASTER_ADDR'] = '127.0.0.1'
    os.environ['MASTER_PORT'] = str(port)
    import torch
    import torch.distributed as dist
    from neuralasr_amd.networks.wavenet import WaveNet
    from neuralasr_amd.parallel import Collective, take_shard
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        torch.cuda.set_device(0)
        ts = torch.cuda.Stream()
        torch.cuda.set_stream(ts)
        spec, (feats, seq, labels, ll) = _batch2()
        e = engine(spec, stream=ts.cuda_stream)
        e.set_params(W.init_params(spec, 3))
        e.set_bn_hold(True)
        net = types.SimpleNamespace(engine=e, coll=Collective())
        f, l, s, lll = take_shard(feats, labels, list(seq), list(ll), world, rank)
        gt = e.grad_tensor()
        for _ in range(2):
            e.upload_batch(f, s, l, lll)
            e.compute_grads()
            WaveNet.after_compute_grads(net)              # the plugin's exchange: every rank's update, in rank order
            torch.cuda.synchronize()
            dist.all_reduce(gt, op=dist.ReduceOp.SUM)
            torch.cuda.synchronize()
            e.apply_adam(1.0 / world)
            assert not e.step_void()
        mm, mv, bs, n = e.bn_state()
        np.savez(os.path.join(out_dir, 'r%d.npz' % rank), params=e.get_params(), mm=mm, mv=mv, bs=bs, n=n)
        e.close()
    finally:
        dist.destroy_process_group()


def test_two_ranks_hold_the_same_moving_statistics_in_rank_order(tmp_path):
    import multiprocessing as mp
    from neuralasr_amd.parallel import take_shard
    ctx = mp.get_context('spawn')
    port = _free_port()
    ps = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path))) for r in range(2)]
    for p in ps:
        p.start()
    for p in ps:
        p.join(600)
    assert all(p.exitcode == 0 for p in ps), [p.exitcode for p in ps]
    r0, r1 = (np.load(os.path.join(str(tmp_path), 'r%d.npz' % r)) for r in range(2))
    for k in ('params', 'mm', 'mv', 'bs', 'n'):
        np.testing.assert_array_equal(r0[k], r1[k])
    # the rank-order sequence of updates, with the parameters each step saw
    spec, (feats, seq, labels, ll) = _batch2()
    p = W.init_params(spec, 3).astype(np.float64)
    m = v = 0
    st = W.bn_initial(spec)
    for t in range(1, 3):
        gs = 0
        for k in range(2):
            f, l, s, lll = take_shard(feats, labels, list(seq), list(ll), 2, k)
            _, g, stats = W.loss_and_grads(spec, p.astype(np.float32), f, [int(x) for x in s], l, lll)
            gs = gs + g
            st = W.bn_update(spec, st, *W.update_variance(spec, stats))
        p, m, v = W.adam_tf(p, gs / 2, m, v, t, 1e-3)
    assert int(r0['n']) == 4
    for got, want in ((r0['mm'], st['mm']), (r0['mv'], st['mv']), (r0['bs'], st['biased'])):
        assert np.abs(got - want).max() <= 1e-5 * (np.abs(want).max() + 1)
