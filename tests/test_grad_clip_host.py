"""Gradient clipping without a GPU: the config key and the fp64 restatement of the rule (tests/grad_clip_ref.py) against
torch.nn.utils.clip_grad_norm_."""
import math
import os

import numpy as np
import pytest

import grad_clip_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLES = os.path.join(HERE, 'golden', 'sample_set')


def config_with(tmp_path, value):
    lines = open(os.path.join(SAMPLES, 'toy.config')).read().splitlines()
    out = []
    for ln in lines:
        out.append('output=' + SAMPLES if ln.startswith('output=') else ln)
        if ln.strip() == '[Parameters]' and value is not None:
            out.append('max_grad_norm=' + value)
    p = tmp_path / 'toy.config'
    p.write_text('\n'.join(out) + '\n')
    return str(p)


def test_config_key_absent_is_off(tmp_path):
    from neuralasr_amd.config import Config
    assert Config(config_with(tmp_path, None), True).max_grad_norm == 0.0


@pytest.mark.parametrize('text,want', [('0', 0.0), ('5', 5.0), ('0.25', 0.25), ('inf', math.inf)])
def test_config_key_accepted(tmp_path, text, want):
    from neuralasr_amd.config import Config
    assert Config(config_with(tmp_path, text), True).max_grad_norm == want


@pytest.mark.parametrize('text', ['-1', 'nan', 'abc', '-inf'])
def test_config_key_refused(tmp_path, text):
    from neuralasr_amd.config import Config
    with pytest.raises(ValueError, match='max_grad_norm'):
        Config(config_with(tmp_path, text), True)


def test_restatement_agrees_with_torch_clip_grad_norm():
    import torch
    rs = np.random.RandomState(0)
    clipped = kept = 0
    for trial in range(40):
        shapes = [(rs.randint(1, 40), rs.randint(1, 30)) for _ in range(rs.randint(1, 5))]
        gs = [rs.randn(*s) * 10.0 ** rs.uniform(0, 3) for s in shapes]
        flat = np.concatenate([g.ravel() for g in gs])
        norm = float(np.sqrt(np.dot(flat, flat)))
        if norm < 1.0:      # torch's 1e-6 in the denominator is within 1e-6 relative only from norm 1 upwards
            continue
        max_norm = norm * float(np.exp(rs.uniform(-2, 2)))
        if abs(norm - max_norm) <= 1e-5 * max_norm:
            continue
        ps = [torch.nn.Parameter(torch.zeros(s, dtype=torch.float64)) for s in shapes]
        for p, g in zip(ps, gs):
            p.grad = torch.from_numpy(g.copy())
        total = float(torch.nn.utils.clip_grad_norm_(ps, max_norm))
        skip, n_ref, coef = R.decide(flat, max_norm)
        assert not skip
        assert n_ref == pytest.approx(total, rel=1e-12)
        # torch scales by min(1, max_norm / (norm + 1e-6)): read the coefficient it applied off the largest element
        k = int(np.argmax(np.abs(flat)))
        coef_t = float(torch.cat([p.grad.ravel() for p in ps])[k]) / flat[k]
        assert abs(coef - coef_t) <= 1e-6 * coef
        assert (coef < 1.0) == (coef_t < 1.0)          # the same decision away from the threshold
        clipped += coef < 1.0
        kept += coef == 1.0
    assert clipped >= 5 and kept >= 5


def test_restatement_skips_non_finite_and_keeps_zero():
    g = np.zeros(10)
    assert R.decide(g, 1.0) == (False, 0.0, 1.0)
    for bad in (np.inf, -np.inf, np.nan):
        g = np.ones(10)
        g[3] = bad
        skip, norm, coef = R.decide(g, 1.0)
        assert skip and coef is None and not np.isfinite(norm)
    p, m, v, step, info = R.clipped_step(np.ones(10), g, np.zeros(10), np.zeros(10), 4, 1e-3, 1.0)
    assert step == 4 and info['skip'] and np.all(p == 1) and np.all(m == 0) and np.all(v == 0)
    assert R.decide(np.full(4, 3.0), np.inf, 0.5) == (False, 3.0, 1.0)      # inf measures, never scales


class _StubEngine:
    def __init__(self):
        self.resets = []

    def grad_clip_stats(self, reset=False):
        self.resets.append(reset)
        k = len(self.resets)
        return {'last_norm': 1.5 * k, 'window_max_norm': 2.25 * k, 'last_coef': 0.5, 'steps': 2, 'clipped': 1,
                'skipped': k - 1}


class _StubNet:
    def __init__(self, config):
        self.global_step = config.start_step
        self.engine = _StubEngine()

    def train(self, mfccs, labels, seq_len, labels_len):
        self.global_step += 1
        return np.float32(1.0), np.float32(0.5)

    def save_checkpoint(self):
        pass


@pytest.mark.parametrize('value', [None, '0', '5'])
def test_train_model_logs_one_grad_line_per_step_line_only_with_the_key(tmp_path, caplog, value):
    import logging
    from neuralasr_amd import train as train_mod
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    text = open(config_with(tmp_path, value)).read().replace('model_dir=.model_toy', 'model_dir=' + str(tmp_path / 'm'))
    (tmp_path / 'c.config').write_text(text)
    cfg = Config(str(tmp_path / 'c.config'), True)
    holder = {}

    def fake_load(fortraining=False):
        holder['net'] = _StubNet(cfg)
        return holder['net']
    cfg.load_network = fake_load
    with caplog.at_level(logging.INFO, logger='NeuralASR'):
        train_mod.train_model(DataSet(cfg.train_input, cfg), None, cfg)
    recs = [(r.levelno, r.getMessage()) for r in caplog.records]
    msgs = [m for _, m in recs]
    steps = [i for i, m in enumerate(msgs) if m.startswith('Step: ')]
    assert len(steps) == 2                       # 2 epochs x 2 batches, report_step 2
    grads = [m for m in msgs if m.startswith('Grad: ')]
    if value != '5':
        assert grads == [] and holder['net'].engine.resets == []
        assert not any(lv >= logging.WARNING for lv, _ in recs)
        return
    assert [msgs[i + 1] for i in steps] == grads == [
        'Grad: norm = 1.5000, max = 2.2500, clipped 1 of 2, skipped 0',
        'Grad: norm = 3.0000, max = 4.5000, clipped 1 of 2, skipped 1']
    assert holder['net'].engine.resets == [True, True]          # the window is cleared behind every line
    warns = [m for lv, m in recs if lv >= logging.WARNING]
    assert len(warns) == 1 and 'skipped' in warns[0] and msgs.index(warns[0]) == steps[1] + 2
