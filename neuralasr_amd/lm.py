"""An n-gram language model over symbol ids for the two beam searches (not part of the reference, whose
To-Do list only names "language model decoding").

The decoders consume a dense float32 table logp[K][C], C = config.symbols.counter, K = C^(n-1), n in 1..4.  Row `ctx` is
the history id(t-1), ..., id(t-n+1) written in base C with the most recent id as the lowest digit, so extending a context
by w gives (ctx*C + w) mod K; for n = 1 there is one row.  eos[K] is the log-probability that the sequence ends after the
history; histories before the start of a sequence are filled with bos_id.  A model is one .npz (logp, eos, order,
num_classes, bos_id); a table of more than 2^24 entries is refused.

Smoothing is this project's own choice: recursive Dirichlet interpolation in float64 over the C+1 outcomes of a history
(the C symbols and the end of the sequence),
    P_k(x | h) = (N(h, x) + delta*(C+1) * P_{k-1}(x | h')) / (N(h) + delta*(C+1)),
h' = h without its oldest symbol, P_0 uniform, so every row sums to 1 before the rounding to float32."""
import numpy as np

MAX_ORDER = 4
MAX_ENTRIES = 1 << 24


def num_contexts(order, num_classes):
    """K = C^(order-1); ValueError when the order is out of 1..4 or the table K*C would exceed 2^24 entries"""
    order, C = int(order), int(num_classes)
    if not 1 <= order <= MAX_ORDER:
        raise ValueError('the n-gram order must be in 1..%d, not %d' % (MAX_ORDER, order))
    if C < 2:
        raise ValueError('an n-gram model needs at least 2 classes, not %d' % C)
    K = C ** (order - 1)
    if K * C > MAX_ENTRIES:
        raise ValueError('an order-%d table over %d classes has %d entries: more than 2^24' % (order, C, K * C))
    return K


def context_of(history, order, num_classes, bos_id):
    """The context index of a history (oldest id first): its last order-1 ids, short histories filled with bos_id from the
    left; the most recent id is the lowest digit."""
    n = int(order) - 1
    h = ([int(bos_id)] * n + [int(x) for x in history])[-n:] if n else []
    ctx = 0
    for x in h:
        ctx = ctx * int(num_classes) + x
    return ctx


def extend(ctx, w, num_classes, K):
    """the context after symbol w follows context ctx"""
    return (int(ctx) * int(num_classes) + int(w)) % int(K)


class NGramLM(object):
    def __init__(self, logp, eos, order, num_classes, bos_id):
        self.order, self.num_classes, self.bos_id = int(order), int(num_classes), int(bos_id)
        self.K = num_contexts(self.order, self.num_classes)
        if not 0 <= self.bos_id < self.num_classes:
            raise ValueError('bos_id %d is not a class of %d' % (self.bos_id, self.num_classes))
        self.logp = np.ascontiguousarray(logp, np.float32)
        self.eos = np.ascontiguousarray(eos, np.float32)
        if self.logp.shape != (self.K, self.num_classes) or self.eos.shape != (self.K,):
            raise ValueError('an order-%d model over %d classes needs logp [%d][%d] and eos [%d], not %s and %s' % (
                self.order, self.num_classes, self.K, self.num_classes, self.K, self.logp.shape, self.eos.shape))

    @property
    def root(self):
        """the context of an empty sequence: bos_id in every digit"""
        return context_of([], self.order, self.num_classes, self.bos_id)

    def score(self, ids):
        """(sum of log P(id | history) over the sequence, log P(end | whole sequence)) in float64 from the float32 table"""
        ctx, total = self.root, 0.0
        for w in ids:
            total += float(self.logp[ctx, int(w)])
            ctx = extend(ctx, w, self.num_classes, self.K)
        return total, float(self.eos[ctx])

    def save(self, filename):
        with open(filename, 'wb') as fh:
            np.savez(fh, logp=self.logp, eos=self.eos, order=np.int32(self.order),
                     num_classes=np.int32(self.num_classes), bos_id=np.int32(self.bos_id))

    @classmethod
    def load(cls, filename):
        with np.load(filename) as z:
            return cls(z['logp'], z['eos'], int(z['order']), int(z['num_classes']), int(z['bos_id']))


def load_for(config):
    """The model config.lm_file names, checked against the config's symbol table; None without the key."""
    if not getattr(config, 'lm_file', None):
        return None
    lm = NGramLM.load(config.lm_file)
    if lm.num_classes != config.symbols.counter:
        raise ValueError('the language model %s has num_classes %d but the symbol table has %d symbols' % (
            config.lm_file, lm.num_classes, config.symbols.counter))
    return lm


def probabilities(sequences, order, num_classes, bos_id, delta=0.5):
    """float64 [K][C+1]: P(x | ctx) of the smoothed order-`order` model counted on `sequences` (lists of ids); column C is
    the end of the sequence.  A sequence's leading bos_id is history only."""
    C = int(num_classes)
    K = num_contexts(order, C)
    if not delta > 0:
        raise ValueError('delta must be positive')
    prior = float(delta) * (C + 1)
    P = np.full((1, C + 1), 1.0 / (C + 1))                     # P_0, uniform; then P_1 .. P_order over histories of k-1 ids
    for k in range(1, int(order) + 1):
        Kk = C ** (k - 1)
        N = np.zeros((Kk, C + 1))
        for seq in sequences:
            seq = [int(x) for x in seq]
            for pos, x in enumerate(seq + [C]):
                N[context_of(seq[:pos], k, C, bos_id), x] += 1
        lower = P[np.arange(Kk) % P.shape[0]]                   # h' = h without its oldest (highest) digit
        P = (N + prior * lower) / (N.sum(axis=1, keepdims=True) + prior)
    assert P.shape == (K, C + 1)
    return P


def label_sequences(config):
    """(sequences, bos_id): the label id sequences of the pickled training set ([Train] input).  With a start_marker whose
    id opens a sequence, that id is bos_id and is dropped from the sequence (history only, never predicted); otherwise
    bos_id is the padding id."""
    from .dataset import DataSet
    data = DataSet(config.train_input, config)
    seqs = [[int(x) for x in np.asarray(data.load_pkl(f)[1]).ravel()] for f in data.X]
    start = None
    if getattr(config, 'start_marker', None) and config.start_marker in config.symbols.sym_to_id:
        start = config.symbols.get_id(config.start_marker)
    if start is not None and any(s and s[0] == start for s in seqs):
        return [s[1:] if s and s[0] == start else s for s in seqs], start
    return seqs, config.symbols.get_padding_id()


def build(sequences, order, num_classes, bos_id, delta=0.5):
    P = probabilities(sequences, order, num_classes, bos_id, delta)
    with np.errstate(divide='ignore'):
        L = np.log(P)
    return NGramLM(L[:, :-1].astype(np.float32), L[:, -1].astype(np.float32), order, num_classes, bos_id)

