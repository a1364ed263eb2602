"""Streaming recognition with a causal network (the reference decodes whole utterances,
networks/tfnetwork.py:179-181).  StreamingRecognizer feeds chunks of feature frames to the engine's stream session, which
carries every LSTM layer's (c, h) per slot on the GPU, and each slot's logits to that slot's own incremental CTC beam
search on the host; the current hypothesis is there after every chunk.

The features are the caller's: the reference normalises by whole-utterance mean and std (utils.py:29), so frames that
match a trained model exist only once the utterance is complete (`decode_wav --stream` therefore featurizes the whole
file first and chunks the normalised frames)."""
import numpy as np

from .engine import BeamStream


class StreamingRecognizer:
    """`slots` concurrent streams on `network` (a HipNetwork whose engine can stream: unidirectional LSTM layers, no
    dropout; any other raises the library's message here).  The decoder is the network's, as in decode(): beam_width,
    merge_repeated as TF's default, and language_model() fused with config.lm_weight / lm_bonus when the config names
    one; decoder = 'greedy' streams with a beam of width 1."""

    def __init__(self, network, slots=1):
        self.network = network
        self.engine = network.engine
        self.slots = int(slots)
        self.feature_size = int(network.config.feature_size)
        settle = getattr(network, '_settle', None)
        if settle:
            settle()
        self.engine.stream_open(self.slots)
        lm = network.language_model()
        width = network.beam_width if getattr(network, 'decoder', 'beam') == 'beam' else 1
        kw = {} if lm is None else dict(lm=lm, lm_weight=network.config.lm_weight, lm_bonus=network.config.lm_bonus)
        self.beams = [BeamStream(network.num_classes, width, True, **kw) for _ in range(self.slots)]

    def feed(self, chunks):
        """chunks: one entry per slot, float32 [n_b, F] (the slot's next frames) or None (the slot is idle).  Pads to the
        longest, runs the chunk on the GPU, feeds every slot's beam with its own frames.  Returns the current hypothesis
        (list of ids) of every slot."""
        if len(chunks) != self.slots:
            raise ValueError('%d chunks for %d slots' % (len(chunks), self.slots))
        arrs = [None if c is None else np.asarray(c, dtype=np.float32) for c in chunks]
        for a in arrs:
            if a is not None and (a.ndim != 2 or a.shape[1] != self.feature_size):
                raise ValueError('a chunk must be [n, %d], not %s' % (self.feature_size, a.shape))
        n = np.asarray([0 if a is None else a.shape[0] for a in arrs], dtype=np.int32)
        Tc = int(n.max())
        if Tc > 0:
            feats = np.zeros((self.slots, Tc, self.feature_size), np.float32)
            for b, a in enumerate(arrs):
                if n[b]:
                    feats[b, :n[b]] = a
            logits = self.engine.stream_feed(feats, n)
            for b in range(self.slots):
                if n[b]:
                    self.beams[b].feed(logits[:n[b]], slot=b)
        return [beam.best()[0] for beam in self.beams]

    def hypothesis(self, slot=0):
        """(ids, log-probability) of `slot` as it stands."""
        return self.beams[slot].best()

    def finish(self, slot=0):
        """The final (ids, log-probability) of `slot`; the slot's device state and beam then start a new utterance."""
        out = self.beams[slot].best()
        self.engine.stream_reset([slot])
        self.beams[slot].reset()
        return out

    def close(self):
        if self.engine is not None:
            for beam in self.beams:
                beam.close()
            self.engine.stream_close()
            self.engine = None
