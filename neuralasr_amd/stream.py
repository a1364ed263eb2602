"""Streaming recognition with a causal network (the reference decodes whole utterances,
networks/tfnetwork.py:179-181).  StreamingRecognizer feeds chunks of feature frames to the engine's stream session, which
carries every LSTM layer's (c, h) per slot on the GPU, and each slot's logits to that slot's own incremental CTC beam
search on the host; the current hypothesis is there after every chunk.

feed() takes the caller's features: the reference normalises by whole-utterance mean and std (utils.py:29), so frames that
match a model trained that way exist only once the utterance is complete (`decode_wav --stream` then featurizes the whole
file first and chunks the normalised frames).  feed_audio() takes SAMPLES: with normalization=causal in the config
 the network's featurizer normalises as the audio arrives, the session's front end keeps each slot's sample
tail and running statistics on the GPU, and the rows a feed makes go straight into the chunk.

A bidirectional (concat) network streams with a look-ahead: StreamingRecognizer(network, slots, lookahead=R)
opens a look-ahead session, whose feeds hold each slot's last R rows back for their right context; the beams get the rows a
feed emits, and finish() flushes the rest.  The hypothesis then depends on how the input was split into feeds."""
import contextlib

import numpy as np

from .engine import BeamStream


class StreamingRecognizer:
    """`slots` concurrent streams on `network` (a HipNetwork whose engine can stream: unidirectional LSTM layers, no
    dropout - or, with lookahead = R frames, bidirectional concat layers; any other raises the library's message here).  The decoder is the network's, as in decode(): beam_width,
    merge_repeated as TF's default, and language_model() fused with config.lm_weight / lm_bonus when the config names
    one; decoder = 'greedy' streams with a beam of width 1."""

    def __init__(self, network, slots=1, lookahead=None):
        self.network = network
        self.engine = network.engine
        self.slots = int(slots)
        self.lookahead = None if lookahead is None else int(lookahead)
        self.feature_size = int(network.config.feature_size)
        self.frame_skip = int(getattr(network.config, 'frame_skip', 1))     # (the engine has it already: HipNetwork set it)
        settle = getattr(network, '_settle', None)
        if settle:
            settle()
        if self.lookahead is None:
            self.engine.stream_open(self.slots)
        else:
            self.engine.stream_open_lookahead(self.slots, self.lookahead)
        # per slot, what finish() has to complete first: None, 'rows' (look-ahead: rows that no `last` has flushed yet) or
        # 'audio' (feed_audio: samples that no `last` has completed yet)
        self._open = [None] * self.slots
        lm = network.language_model()
        width = network.beam_width if getattr(network, 'decoder', 'beam') == 'beam' else 1
        kw = {} if lm is None else dict(lm=lm, lm_weight=network.config.lm_weight, lm_bonus=network.config.lm_bonus)
        self.beams = [BeamStream(network.num_classes, width, True, **kw) for _ in range(self.slots)]
        self._audio = False                      # feed_audio attached the network's featurizer to the session
        # a training network with ema_decay runs every feed on its averaged parameters
        self._averaged = getattr(network, '_averaged', contextlib.nullcontext)

    def _padded(self, arrs, n):
        """the chunk [slots, max n, F]: slot b's n[b] rows, zeros behind them"""
        feats = np.zeros((self.slots, int(n.max()), self.feature_size), np.float32)
        for b, a in enumerate(arrs):
            if n[b]:
                feats[b, :n[b]] = a
        return feats

    def _deliver(self, logits, rows, got, last, kind):
        """Hands every slot's rows[b] emitted rows to its beam and notes what is open: a slot that got input is `kind`
        until a `last` completes it.  Returns the current hypothesis of every slot."""
        for b in range(self.slots):
            if rows[b]:
                self.beams[b].feed(logits[:rows[b]], slot=b)
            if last is not None and last[b]:
                self._open[b] = None
            elif got[b] and kind:
                self._open[b] = kind
        return [beam.best()[0] for beam in self.beams]

    def feed(self, chunks, last=None):
        """chunks: one entry per slot, float32 [n_b, F] (the slot's next frames) or None (the slot is idle).  Pads to the
        longest, runs the chunk on the GPU, feeds every slot's beam with its own frames.  Returns the current hypothesis
        (list of ids) of every slot.  With a look-ahead the last `lookahead` frames of a slot wait for their right
        context: the beam gets the rows the feed emitted, and last[b] true (look-ahead only) flushes slot b."""
        if len(chunks) != self.slots:
            raise ValueError('%d chunks for %d slots' % (len(chunks), self.slots))
        arrs = [None if c is None else np.asarray(c, dtype=np.float32) for c in chunks]
        for a in arrs:
            if a is not None and (a.ndim != 2 or a.shape[1] != self.feature_size):
                raise ValueError('a chunk must be [n, %d], not %s' % (self.feature_size, a.shape))
        n = np.asarray([0 if a is None else a.shape[0] for a in arrs], dtype=np.int32)
        if self.lookahead is not None:
            with self._averaged():
                logits, rows = self.engine.stream_feed_lookahead(self._padded(arrs, n), n, last)
            return self._deliver(logits, rows, n, last, 'rows')
        if last is not None and any(last):
            raise ValueError('`last` means something only with a look-ahead')
        if n.max() == 0:                         # (the library refuses a chunk without rows)
            return [beam.best()[0] for beam in self.beams]
        if self.frame_skip == 1:
            with self._averaged():
                logits = self.engine.stream_feed(self._padded(arrs, n), n)
            return self._deliver(logits, n, n, None, None)
        # under frame_skip a slot's new logit rows are the rows the session kept, not the rows it was given:
        # the rows the library reports, as the growth of its per-slot count
        before = self.engine.stream_frames()
        with self._averaged():
            logits = self.engine.stream_feed(self._padded(arrs, n), n)
        return self._deliver(logits, self.engine.stream_frames() - before, n, None, None)

    def feed_audio(self, chunks, last=None):
        """chunks: one entry per slot, float32 [n_b] samples at config.samplerate (the slot's next samples) or None (the
        slot is idle); last: per slot, true when the slot's utterance ends with these samples.  The session's front end
        makes the rows that the samples so far allow (none while fewer than norm_min_frames frames are complete, and
        numcontext frames are held back for their right context until `last`), the network runs over them, and every
        slot's beam is fed with its own.  Returns the current hypothesis of every slot.  Needs normalization=causal."""
        if len(chunks) != self.slots:
            raise ValueError('%d chunks for %d slots' % (len(chunks), self.slots))
        if not self._audio:
            self.engine.stream_attach_audio(self.network.featurizer())
            self._audio = True
        with self._averaged():
            logits, rows = self.engine.stream_feed_audio(chunks, last)
        return self._deliver(logits, rows, [c is not None and np.size(c) for c in chunks], last, 'audio')

    def hypothesis(self, slot=0):
        """(ids, log-probability) of `slot` as it stands."""
        return self.beams[slot].best()

    def finish(self, slot=0):
        """The final (ids, log-probability) of `slot`; the slot's device state and beam then start a new utterance.  A
        slot whose audio (feed_audio) no `last` has completed is completed first, with an empty feed."""
        if self._open[slot]:
            flush = self.feed_audio if self._open[slot] == 'audio' else self.feed
            flush([None] * self.slots, [b == slot for b in range(self.slots)])
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
