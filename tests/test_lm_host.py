"""The n-gram model of the beam searches on the host (neuralasr_amd/lm.py, build_lm.py, the config keys): the
builder on tests/golden/sample_set against a dictionary-count restatement, the bos rule, the file, the config keys and the
context arithmetic.  No GPU."""
import itertools
import os

import numpy as np
import pytest

from neuralasr_amd import lm
from neuralasr_amd.build_lm import build_lm, main as build_lm_main
from neuralasr_amd.config import Config
from neuralasr_amd.dataset import DataSet

HERE = os.path.dirname(os.path.abspath(__file__))
SAMPLES = os.path.join(HERE, 'golden', 'sample_set')


def write_config(tmp_path, extra_parameters=(), extra_featurizer=(), name='toy.config'):
    """tests/golden/sample_set/toy.config re-rooted at this checkout, with extra lines in two of its sections"""
    lines = []
    for ln in open(os.path.join(SAMPLES, 'toy.config')).read().splitlines():
        if ln.startswith('output='):
            ln = 'output=' + SAMPLES
        if ln.startswith('model_dir='):
            ln = 'model_dir=' + str(tmp_path / 'model')
        lines.append(ln)
        if ln == '[Parameters]':
            lines.extend(extra_parameters)
        if ln == '[MFCC Featurizer]':
            lines.extend(extra_featurizer)
    p = tmp_path / name
    p.write_text('\n'.join(lines) + '\n')
    return str(p)


def training_labels(config):
    data = DataSet(config.train_input, config)
    return [[int(x) for x in data.load_pkl(f)[1]] for f in data.X]


def dictionary_model(seqs, order, C, bos, delta):
    """P_k(x | h) = (N(h, x) + delta*(C+1)*P_{k-1}(x | h')) / (N(h) + delta*(C+1)) from dictionaries keyed by explicit
    history tuples (oldest first); x = C is the end of the sequence"""
    counts = [{} for _ in range(order + 1)]
    for k in range(1, order + 1):
        for s in seqs:
            padded = [bos] * (k - 1) + list(s)
            for i, x in enumerate(list(s) + [C]):
                h = tuple(padded[i:i + k - 1])
                counts[k][(h, x)] = counts[k].get((h, x), 0) + 1

    def prob(k, h, x):
        if k == 0:
            return 1.0 / (C + 1)
        n_h = sum(counts[k].get((h, y), 0) for y in range(C + 1))
        return (counts[k].get((h, x), 0) + delta * (C + 1) * prob(k - 1, h[1:], x)) / (n_h + delta * (C + 1))

    return prob


@pytest.mark.parametrize('order', [1, 2, 3, 4])
def test_builder_on_the_sample_set(tmp_path, order):
    c = Config(write_config(tmp_path), True)
    C = c.symbols.counter
    seqs = training_labels(c)
    assert len(seqs) >= 3 and all(seqs)
    got_seqs, bos = lm.label_sequences(c)
    assert got_seqs == seqs and bos == c.symbols.get_padding_id() == 0         # no start marker: the padding id
    P = lm.probabilities(seqs, order, C, bos, 0.5)
    assert P.dtype == np.float64 and P.shape == (C ** (order - 1), C + 1)
    np.testing.assert_allclose(P.sum(axis=1), 1.0, rtol=0, atol=1e-14)         # every row sums to 1 in fp64
    prob = dictionary_model(seqs, order, C, bos, 0.5)
    want = np.array([[prob(order, h, x) for x in range(C + 1)] for h in itertools.product(range(C), repeat=order - 1)])
    np.testing.assert_allclose(P, want, rtol=1e-13, atol=0)
    out = build_lm(c, order=order, output=str(tmp_path / 'lm.npz'))
    m = lm.NGramLM.load(out)
    assert (m.order, m.num_classes, m.bos_id, m.K) == (order, C, 0, C ** (order - 1))
    assert m.logp.dtype == np.float32 and m.eos.dtype == np.float32
    assert m.logp.tobytes() == np.log(want[:, :C]).astype(np.float32).tobytes()
    assert m.eos.tobytes() == np.log(want[:, C]).astype(np.float32).tobytes()
    # the file round-trips
    m.save(str(tmp_path / 'again.npz'))
    n = lm.NGramLM.load(str(tmp_path / 'again.npz'))
    assert n.logp.tobytes() == m.logp.tobytes() and n.eos.tobytes() == m.eos.tobytes()
    assert (n.order, n.num_classes, n.bos_id) == (m.order, m.num_classes, m.bos_id)
    assert sorted(np.load(out).files) == ['bos_id', 'eos', 'logp', 'num_classes', 'order']


def test_delta_and_command_line(tmp_path):
    cfg = write_config(tmp_path, extra_parameters=['lm_file=' + str(tmp_path / 'cli.npz')])
    assert build_lm_main([cfg, '--order', '2', '--delta', '0.25']) == str(tmp_path / 'cli.npz')
    c = Config(cfg, True)
    m = lm.NGramLM.load(c.lm_file)
    want = lm.probabilities(training_labels(c), 2, c.symbols.counter, 0, 0.25)
    assert m.order == 2 and m.logp.tobytes() == np.log(want[:, :-1]).astype(np.float32).tobytes()
    assert m.logp.tobytes() != lm.build(training_labels(c), 2, c.symbols.counter, 0, 0.5).logp.tobytes()


def test_bos_rule_with_a_start_marker(tmp_path):
    """a start marker whose id opens the sequences is bos_id: history only, never predicted"""
    plain = Config(write_config(tmp_path), True)
    seqs = training_labels(plain)
    first = seqs[0][0]
    sym = plain.symbols.get_sym(first)
    assert any(s[0] != first for s in seqs) or all(s[0] == first for s in seqs)
    c = Config(write_config(tmp_path, extra_featurizer=['start_marker=' + sym], name='marked.config'), True)
    got, bos = lm.label_sequences(c)
    assert bos == first
    assert got == [s[1:] if s[0] == first else s for s in seqs]
    P = lm.probabilities(got, 2, c.symbols.counter, bos, 0.5)
    prob = dictionary_model(got, 2, c.symbols.counter, bos, 0.5)
    np.testing.assert_allclose(P, [[prob(2, (h,), x) for x in range(c.symbols.counter + 1)] for h in range(c.symbols.counter)],
                               rtol=1e-13)
    # the marker's own row holds the counts of what follows the start; with the padding id as bos that row differs
    assert not np.allclose(P[first], lm.probabilities(seqs, 2, plain.symbols.counter, 0, 0.5)[first])
    # a marker that opens no sequence: the padding id again
    other = [s for s in plain.symbols.sym_to_id if plain.symbols.get_id(s) not in {q[0] for q in seqs}][0]
    d = Config(write_config(tmp_path, extra_featurizer=['start_marker=' + other], name='unused.config'), True)
    assert lm.label_sequences(d) == (seqs, 0)


def test_config_keys(tmp_path):
    plain_file = write_config(tmp_path)
    plain = Config(plain_file, True)
    assert plain.lm_file is None and plain.lm_weight == 0.0 and plain.lm_bonus == 0.0
    plain.write(str(tmp_path / 'written.config'))
    text = (tmp_path / 'written.config').read_text()
    assert 'lm_' not in text
    # what it writes today: the parsed file as configparser writes it
    from configparser import ConfigParser, ExtendedInterpolation
    import io
    cp = ConfigParser(interpolation=ExtendedInterpolation())
    cp.read(plain_file)
    buf = io.StringIO()
    cp.write(buf)
    assert text == buf.getvalue()
    keyed = Config(write_config(tmp_path, ['lm_file=' + str(tmp_path / 'm.npz'), 'lm_weight=0.35', 'lm_bonus=-1.5'],
                                name='keyed.config'), True)
    assert (keyed.lm_file, keyed.lm_weight, keyed.lm_bonus) == (str(tmp_path / 'm.npz'), 0.35, -1.5)
    keyed.write(str(tmp_path / 'keyed_written.config'))
    back = Config(str(tmp_path / 'keyed_written.config'), True)
    assert (back.lm_file, back.lm_weight, back.lm_bonus) == (keyed.lm_file, keyed.lm_weight, keyed.lm_bonus)


def test_class_count_mismatch_raises(tmp_path):
    c = Config(write_config(tmp_path, ['lm_file=' + str(tmp_path / 'm.npz')]), True)
    C = c.symbols.counter
    lm.build([[1, 2]], 2, C + 1, 0).save(c.lm_file)
    with pytest.raises(ValueError) as e:
        lm.load_for(c)
    assert str(C) in str(e.value) and str(C + 1) in str(e.value)
    lm.build([[1, 2]], 2, C, 0).save(c.lm_file)
    assert lm.load_for(c).num_classes == C
    assert lm.load_for(Config(write_config(tmp_path, name='nokey.config'), True)) is None


def test_table_limits():
    assert lm.num_contexts(4, 64) == 64 ** 3
    for order, C in ((0, 5), (5, 5), (4, 65), (3, 257)):
        with pytest.raises(ValueError):
            lm.num_contexts(order, C)
    with pytest.raises(ValueError):
        lm.NGramLM(np.zeros((5, 5), np.float32), np.zeros(5, np.float32), 2, 5, 5)
    with pytest.raises(ValueError):
        lm.NGramLM(np.zeros((5, 4), np.float32), np.zeros(5, np.float32), 2, 5, 0)


@pytest.mark.parametrize('order', [1, 2, 3, 4])
def test_context_arithmetic(order):
    """(ctx*C + w) mod K walks the explicit history tuples; the most recent id is the lowest digit"""
    C, bos = 5, 3
    K = lm.num_contexts(order, C)
    tuples = list(itertools.product(range(C), repeat=order - 1))                # oldest first, in index order
    assert len(tuples) == K
    for ctx, h in enumerate(tuples):
        assert lm.context_of(h, order, C, bos) == ctx
        if order > 1:
            assert ctx % C == h[-1]
        for w in range(C):
            want = tuples.index((h + (w,))[1:]) if order > 1 else 0
            assert lm.extend(ctx, w, C, K) == want
    assert lm.context_of([], order, C, bos) == tuples.index((bos,) * (order - 1))
    rs = np.random.RandomState(order)
    seq = rs.randint(0, C, 12).tolist()
    ctx = lm.context_of([], order, C, bos)
    for i, w in enumerate(seq):
        ctx = lm.extend(ctx, w, C, K)
        hist = ([bos] * (order - 1) + seq[:i + 1])[-(order - 1):] if order > 1 else []
        assert ctx == tuples.index(tuple(hist))
