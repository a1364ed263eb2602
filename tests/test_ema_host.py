"""Parameter averaging and the learning-rate schedule without a GPU: the config keys, the schedule against
hand-written numbers, and the fp64 restatement of the average (tests/ema_ref.py) against its closed form and against
torch.optim.swa_utils."""
import os

import numpy as np
import pytest

import ema_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLES = os.path.join(HERE, 'golden', 'sample_set')
KEYS = ('ema_decay', 'lr_warmup_steps', 'lr_decay_steps', 'lr_decay_rate', 'lr_staircase')


def config_with(tmp_path, **extra):
    lines = open(os.path.join(SAMPLES, 'toy.config')).read().splitlines()
    out = []
    for ln in lines:
        out.append('output=' + SAMPLES if ln.startswith('output=') else ln)
        if ln.strip() == '[Parameters]':
            out += ['%s=%s' % kv for kv in extra.items()]
    p = tmp_path / 'toy.config'
    p.write_text('\n'.join(out) + '\n')
    return str(p)


def test_defaults_are_off_and_change_nothing(tmp_path):
    from neuralasr_amd.config import Config
    cfg = Config(config_with(tmp_path), True)
    assert (cfg.ema_decay, cfg.lr_warmup_steps, cfg.lr_decay_steps, cfg.lr_decay_rate, cfg.lr_staircase) == (0.0, 0, 0, 1.0, 0)
    assert cfg.lr_schedule_on is False
    assert cfg.learningrate == 0.005 and cfg.max_grad_norm == 0.0
    for s in (1, 2, 1000):
        assert cfg.learning_rate_at(s) == float(np.float32(0.005))
    # what a run writes into its model_dir is the file as it was read
    dst = tmp_path / 'copy.config'
    cfg.write(str(dst))
    assert not any(k in dst.read_text() for k in KEYS)


def test_keys_parse(tmp_path):
    from neuralasr_amd.config import Config
    cfg = Config(config_with(tmp_path, ema_decay='0.999', lr_warmup_steps='100', lr_decay_steps='2000', lr_decay_rate='0.5',
                             lr_staircase='1'), True)
    assert (cfg.ema_decay, cfg.lr_warmup_steps, cfg.lr_decay_steps, cfg.lr_decay_rate, cfg.lr_staircase) == (0.999, 100, 2000, 0.5, 1)
    assert cfg.lr_schedule_on is True
    only_ema = Config(config_with(tmp_path, ema_decay='0.5'), True)
    assert only_ema.ema_decay == 0.5 and only_ema.lr_schedule_on is False
    assert Config(config_with(tmp_path, lr_decay_rate='1'), True).lr_decay_rate == 1.0


@pytest.mark.parametrize('key,text', [('ema_decay', '0'), ('ema_decay', '1'), ('ema_decay', '-0.5'), ('ema_decay', 'nan'),
                                      ('ema_decay', 'abc'), ('lr_warmup_steps', '-1'), ('lr_warmup_steps', '1.5'),
                                      ('lr_decay_steps', '-2'), ('lr_decay_steps', 'x'), ('lr_decay_rate', '0'),
                                      ('lr_decay_rate', '1.01'), ('lr_decay_rate', 'nan'), ('lr_staircase', '2'),
                                      ('lr_staircase', '-1'), ('lr_staircase', 'yes')])
def test_bad_values_are_refused_by_name(tmp_path, key, text):
    from neuralasr_amd.config import Config
    with pytest.raises(ValueError, match="'%s' must be" % key):
        Config(config_with(tmp_path, **{key: text}), True)


def test_schedule_against_hand_written_numbers():
    # base 0.01, warm-up 4 steps, halved every 10 steps behind it
    args = dict(warmup=4, decay_steps=10, rate=0.5)
    assert R.lr_schedule(0.01, 1, staircase=False, **args) == pytest.approx(0.0025, rel=1e-15)
    assert R.lr_schedule(0.01, 4, staircase=False, **args) == pytest.approx(0.01, rel=1e-15)
    assert R.lr_schedule(0.01, 5, staircase=False, **args) == pytest.approx(0.01 * 0.9330329915368074, rel=1e-14)   # 2^-0.1
    assert R.lr_schedule(0.01, 5, staircase=True, **args) == pytest.approx(0.01, rel=1e-15)
    assert R.lr_schedule(0.01, 13, staircase=True, **args) == pytest.approx(0.01, rel=1e-15)      # (13 - 4) / 10 floors to 0
    assert R.lr_schedule(0.01, 14, staircase=True, **args) == pytest.approx(0.005, rel=1e-15)     # the boundary
    assert R.lr_schedule(0.01, 14, staircase=False, **args) == pytest.approx(0.005, rel=1e-15)
    assert R.lr_schedule(0.01, 24, staircase=True, **args) == pytest.approx(0.0025, rel=1e-15)
    # no warm-up, no decay
    assert R.lr_schedule(0.01, 7, 0, 0, 0.5, False) == 0.01
    assert R.lr_schedule(0.01, 10, 0, 10, 0.5, False) == pytest.approx(0.005, rel=1e-15)


def test_config_schedule_is_the_restatement_rounded_to_fp32(tmp_path):
    from neuralasr_amd.config import Config
    for stair in (0, 1):
        cfg = Config(config_with(tmp_path, lr_warmup_steps='3', lr_decay_steps='4', lr_decay_rate='0.7',
                                 lr_staircase=str(stair)), True)
        for s in range(1, 20):
            want = float(np.float32(R.lr_schedule(cfg.learningrate, s, 3, 4, 0.7, bool(stair))))
            assert cfg.learning_rate_at(s) == want, (stair, s)


@pytest.mark.parametrize('decay', [0.05, 0.4, 0.999])
def test_average_of_a_constant_has_the_closed_form(decay):
    rs = np.random.RandomState(2)
    e0, p = rs.randn(50), rs.randn(50)
    for n0 in (0, 3):
        for N in (1, 6, 12):
            e, n = R.ema_run(e0, [p] * N, decay, n0=n0)
            prod = np.prod([min(decay, (1.0 + k) / (10.0 + k)) for k in range(n0, n0 + N)])
            assert n == n0 + N
            np.testing.assert_allclose(e - p, (e0 - p) * prod, rtol=1e-12, atol=1e-15)
    e, _ = R.ema_run(e0, [p] * 5, decay, constant=True)
    np.testing.assert_allclose(e - p, (e0 - p) * decay ** 5, rtol=1e-12, atol=1e-15)


def test_the_ramp_hands_over_where_it_meets_the_decay():
    assert [R.ema_decay_at(0.4, n) for n in (0, 4, 5, 6)] == [0.1, 5.0 / 14.0, 0.4, 0.4]
    assert R.ema_decay_at(0.05, 0) == 0.05
    assert R.ema_decay_at(0.999, 11) == 12.0 / 21.0


def test_constant_decay_agrees_with_torch_swa_utils():
    torch = pytest.importorskip('torch')
    swa = pytest.importorskip('torch.optim.swa_utils')
    if not hasattr(swa, 'get_ema_multi_avg_fn'):
        pytest.skip('this torch has no get_ema_multi_avg_fn')
    rs = np.random.RandomState(4)
    e0 = rs.randn(3, 40)
    ps = [rs.randn(3, 40) for _ in range(7)]
    fn = swa.get_ema_multi_avg_fn(0.9)
    shadow = [torch.tensor(r, dtype=torch.float64) for r in e0]
    for p in ps:
        fn(shadow, [torch.tensor(r, dtype=torch.float64) for r in p], 0)
    want, _ = R.ema_run(e0, ps, 0.9, constant=True)
    np.testing.assert_allclose(np.stack([t.numpy() for t in shadow]), want, rtol=1e-13, atol=1e-15)


class _StubNet:
    def __init__(self, config):
        self.global_step = config.start_step

    def train(self, mfccs, labels, seq_len, labels_len):
        self.global_step += 1
        return np.float32(1.0), np.float32(0.5)

    def save_checkpoint(self):
        pass


@pytest.mark.parametrize('keys', [{}, {'ema_decay': '0.9'}, {'lr_warmup_steps': '4', 'lr_decay_steps': '10', 'lr_decay_rate': '0.5'}],
                         ids=['no_key', 'ema_only', 'schedule'])
def test_train_model_logs_one_lr_line_per_step_line_only_with_a_schedule_key(tmp_path, caplog, keys):
    import logging
    from neuralasr_amd import train as train_mod
    from neuralasr_amd.config import Config
    from neuralasr_amd.dataset import DataSet
    text = open(config_with(tmp_path, **keys)).read().replace('model_dir=.model_toy', 'model_dir=' + str(tmp_path / 'm'))
    (tmp_path / 'c.config').write_text(text)
    cfg = Config(str(tmp_path / 'c.config'), True)
    cfg.load_network = lambda fortraining=False: _StubNet(cfg)
    with caplog.at_level(logging.INFO, logger='NeuralASR'):
        train_mod.train_model(DataSet(cfg.train_input, cfg), None, cfg)
    msgs = [r.getMessage() for r in caplog.records]
    steps = [i for i, m in enumerate(msgs) if m.startswith('Step: ')]
    assert [msgs[i][:10] for i in steps] == ['Step: 0002', 'Step: 0004']      # 2 epochs x 2 batches, report_step 2
    lrs = [m for m in msgs if m.startswith('LR: ')]
    if 'lr_warmup_steps' not in keys:
        assert lrs == []
        return
    assert [msgs[i + 1] for i in steps] == lrs == ['LR: 0.0025', 'LR: 0.005']   # 0.005 * 2/4, 0.005 * 4/4
