"""GPU: what the one upload path relies on.  A one-call entry point is the upload plus the *_resident call (so HipNetwork
may run inference as _upload + *_resident), the network on host features is the engine's one-call path and still uploads
them whole, and features of the wrong width never reach the library.  Everything is compared as bits."""
import numpy as np
import pytest

from neuralasr_amd.config import Config
from neuralasr_amd.dataset import DataSet
from test_gpu_audio_batch import init, same
from test_gpu_network import make_config

pytestmark = pytest.mark.gpu

F, C, B, T = 12, 5, 3, 9                      # B = 3: 13 empty columns of Bp = 16
SEQ, LABEL_LEN = [9, 5, 1], [2, 1, 0]
LABELS = np.array([[1, 3], [2, 0], [0, 0]], np.int32)
SHAPES = [(1, True, 'stack_reshape'), (2, False, 'none')]      # the first: the row-map path


def feats(width=F, seed=0):
    return np.random.default_rng(seed).standard_normal((B, T, width)).astype(np.float32)


@pytest.fixture(scope='module', params=SHAPES, ids=lambda p: p[2])
def engine(request):
    from neuralasr_amd.engine import Engine
    layers, bidirectional, merge = request.param
    e = init(Engine(F, 16, layers, bidirectional, merge, C))
    yield e
    e.close()


def test_one_call_is_upload_plus_resident(engine):
    e, f = engine, feats()
    stats = e.persist_stats()                 # a handle that fell back to the per-step kernels in between computes other bits
    want = e.forward(f, SEQ)
    e.upload_batch(f, SEQ, None, None)
    assert want.shape == (e.logit_frames(T), B, C) and same(e.forward_resident(B, T), want)

    loss, nll = e.loss(f, SEQ, LABELS, LABEL_LEN)
    e.upload_batch(f, SEQ, LABELS, LABEL_LEN)
    loss_r, nll_r = e.loss_resident(B)
    assert np.isfinite(loss) and same(np.float32(loss), np.float32(loss_r)) and same(nll, nll_r)

    hyps = e.greedy_decode(f, SEQ)
    e.upload_batch(f, SEQ, None, None)
    assert e.greedy_decode_resident(B, T) == hyps

    path, score = e.align(f, SEQ, LABELS, LABEL_LEN)
    e.upload_batch(f, SEQ, LABELS, LABEL_LEN)
    path_r, score_r = e.align_resident(B, T)
    assert np.array_equal(path, path_r) and np.array_equal(score.view(np.uint64), score_r.view(np.uint64))
    assert e.persist_stats() == stats


def test_a_wrong_feature_width_is_refused_before_the_library_sees_it(engine):
    e, good, wide = engine, feats(), feats(F + 1)
    e.upload_batch(good, SEQ, LABELS, LABEL_LEN)
    frames, before = e.resident_frames(), e.forward_resident(B, T)
    assert frames == sum(SEQ)
    calls = [lambda: e.upload_batch(wide, SEQ, LABELS, LABEL_LEN),
             lambda: e.upload_batch_context(wide, SEQ, LABELS, LABEL_LEN, 1, F // 3),
             lambda: e.stage_batch(wide, SEQ, LABELS, LABEL_LEN),
             lambda: e.loss(wide, SEQ, LABELS, LABEL_LEN),
             lambda: e.loss_and_grads(wide, SEQ, LABELS, LABEL_LEN),
             lambda: e.train_step(wide, SEQ, LABELS, LABEL_LEN),
             lambda: e.greedy_decode(wide, SEQ)]
    for call in calls:
        with pytest.raises(ValueError, match='feature size'):
            call()
        assert e.resident_frames() == frames
    assert same(e.forward_resident(B, T), before)


def test_the_network_on_features_is_the_engines_one_call_path(tmp_path):
    from neuralasr_amd.align import spans
    cfg = Config(make_config(tmp_path, num_gpus='1', batch_size='3'), True)
    net = cfg.load_network(fortraining=True)
    try:
        e = net.engine
        assert type(net).__name__ == 'BiLstmCTCNet' and cfg.numcontext > 0 and net._towers() == (1, [0])
        f, labels, s, ll = DataSet(cfg.train_input, cfg).get_next_batch()
        assert f.shape[0] == 3 and isinstance(f, np.ndarray)
        labels = np.asarray(labels, np.int32).reshape(3, -1)
        context_uploads = []
        plain = e.upload_batch_context
        e.upload_batch_context = lambda *a, **k: context_uploads.append(a) or plain(*a, **k)
        stats = e.persist_stats()

        want_loss = np.float32(e.loss(f, s, labels, ll)[0])
        assert same(net.validate(f, labels, s, ll)[0], want_loss)
        assert not context_uploads                          # inference still uploads whole

        want_ids = e.beam_search(e.forward(f, s), s, 100, merge_repeated=True)[0]
        assert np.array_equal(net.decode(f, s), np.asarray([i for h in want_ids for i in h], dtype=np.int64))

        path, score = e.align(f, s, labels, ll)
        want = [(float(score[b]), spans(path[b], labels[b, :int(ll[b])])) for b in range(3)]
        got = net.align(f, labels, s, ll)
        assert [sp for _, sp in got] == [sp for _, sp in want]
        assert np.array_equal(np.array([x for x, _ in got]).view(np.uint64), np.array([x for x, _ in want]).view(np.uint64))
        assert not context_uploads and e.persist_stats() == stats

        loss, _ = net.train(f, labels, s, ll)
        assert np.isfinite(loss) and len(context_uploads) == 1
    finally:
        net.engine.close()
