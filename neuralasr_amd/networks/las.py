"""LAS (reference: networks/las.py): Listen, Attend and Spell.  A 4-layer pyramidal BiLSTM encoder (250 units per direction;
an odd length gets one zero frame, both directions run over every padded frame, frame pairs are concatenated between
layers) and an attention decoder (BasicLSTMCell(500) in an AttentionWrapper, Bahdanau attention with 500 units over the top
layer's output and no memory mask, attention layer 250, projection to the classes), trained with scheduled sampling
(probability 0.1) and sequence_loss.  `network=networks.las.LAS` selects it.  Labels are dense [B, U]; the decoder runs U
steps and step t is fed labels[:, t] itself, as the reference does.

train() / validate() run the training graph (sampling on, as the reference's validate does); the LER is argmax(logits) x
sequence_mask against the labels, both with id 0 dropped (dense_to_sparse).  With num_gpus > 1 every tower computes its own
sequence_loss and the gradients are averaged (time-sliced in one process, or one process per GPU); every tower of a step
draws with the step's sampling counter and keys its samples by its tower index, and the counter advances once per step,
so both layouts feed the same inputs and end with the same counter.  Checkpoints carry the sampling state (las_sampling) beside the variables.

decode() / evaluate() run the reference's inference graph on the GPU (LasEngine.beam_search): BeamSearchDecoder of TF 1.15
with beam_width 1000, maximum_iterations 100 and length_penalty_weight 0.5, starting from start_marker and ending at
end_marker, then gather_tree; the model is beam 0 of the gathered ids [B, T_dec].  evaluate()'s loss is the reference's
sequence_loss over the step scores [B, T_dec, W] taken as logits; its graph cannot build unless T_dec == U, so here it is
NaN then (beam_sequence_loss).

Every call takes a features.AudioBatch in the place of the padded features (audio_batch, the *_audio calls): a tower's
shard goes through the GPU front end into the handle's batch slot (LasEngine.upload_batch_audio) and the passes and the
beam search run on that resident batch, so no feature crosses to the host or back.

With lm_file in the config the beam search of decode() / evaluate() is fused with that n-gram model at lm_weight
(LasEngine.set_lm); train() and validate() run the training graph and are not touched by it."""
import numpy as np

from ..engine import LasEngine
from ..features import AudioBatch
from .hipnetwork import HipNetwork, take_shard


def pyramid_lengths(T, layers=4):
    """Frames each encoder layer runs over: L1 = T + T%2, L(i+1) = L(i)/2 + (L(i)/2)%2."""
    out, L = [], T + T % 2
    for _ in range(layers):
        out.append(L)
        L = L // 2 + (L // 2) % 2
    return out


def tensor_specs(F, C, H=250):
    """(name, rows, cols) of every variable in TF creation order (networks/las.py), without a GPU."""
    specs = []
    for i in range(4):
        I = F if i == 0 else 4 * H
        for d in ('fw', 'bw'):
            scope = 'bidirectional_rnn/%s/%s_%d' % (d, d, i)
            specs.append((scope + '/kernel', I + H, 4 * H))
            specs.append((scope + '/bias', 4 * H, 1))
    specs += [('memory_layer/kernel', 2 * H, 2 * H), ('decoder_lstm/kernel', C + H + 2 * H, 8 * H),
              ('decoder_lstm/bias', 8 * H, 1), ('query_layer/kernel', 2 * H, 2 * H), ('attention_v', 2 * H, 1),
              ('attention_layer/kernel', 4 * H, H), ('projection_layer/kernel', H, C), ('projection_layer/bias', C, 1)]
    return specs


def edit_distance(a, b):
    d = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        prev, d[0] = d[0], i
        for j in range(1, len(b) + 1):
            cur = d[j]
            d[j] = min(d[j] + 1, d[j - 1] + 1, prev + (a[i - 1] != b[j - 1]))
            prev = cur
    return d[len(b)]


def label_error_rate(model, labels):
    """tf.edit_distance(dense_to_sparse(model), dense_to_sparse(labels)) averaged over the batch: id 0 is dropped from
    both, the distance is normalised by the reference's length (an empty reference gives inf when the hypothesis is not
    empty, 0 when both are)."""
    model, labels = np.asarray(model), np.asarray(labels)
    lers = []
    for m, l in zip(model, labels):
        h = [int(x) for x in m if x != 0]
        r = [int(x) for x in l if x != 0]
        if not r:
            lers.append(0.0 if not h else float('inf'))
        else:
            lers.append(edit_distance(h, r) / len(r))
    return float(np.mean(lers))


def beam_sequence_loss(scores, labels, labels_len):
    """sequence_loss(scores, labels, sequence_mask(labels_len, U)) of the reference's evaluate graph, with the step scores
    [B, T_dec, W] as logits over W classes, evaluated literally in float32 (inf and NaN as they come): per entry
    logsumexp(scores) - scores[label], times the mask, summed / (sum of the mask + 1e-12).  TF's graph only builds when
    T_dec == U, and a label id must be a class (< W): NaN otherwise."""
    scores = np.asarray(scores, np.float32)
    labels = np.asarray(labels, np.int64)
    B, Td, W = scores.shape
    U = labels.shape[1]
    if Td != U or (labels.size and (labels.min() < 0 or labels.max() >= W)):
        return np.float32(np.nan)
    w = (np.arange(U)[None, :] < np.asarray(labels_len)[:, None]).astype(np.float32)
    with np.errstate(all='ignore'):
        m = scores.max(axis=2, keepdims=True)
        lse = (np.log(np.exp(scores - m).sum(axis=2, dtype=np.float32)) + m[:, :, 0]).astype(np.float32)
        picked = np.take_along_axis(scores, labels[:, :, None], axis=2)[:, :, 0]
        ce = (lse - picked) * w
        return np.float32(ce.sum(dtype=np.float32) / np.float32(w.sum(dtype=np.float32) + np.float32(1e-12)))


def model_ids(logits, labels_len):
    """argmax(logits) x sequence_mask(labels_len, U)"""
    U = logits.shape[1]
    w = (np.arange(U)[None, :] < np.asarray(labels_len)[:, None]).astype(np.int64)
    return np.argmax(logits, axis=2) * w


class LAS(HipNetwork):
    num_hidden = 250
    num_layers = 4
    bidirectional = True
    merge = 'none'
    device_context = False                   # features are uploaded whole
    sampling_probability = 0.1
    sampling_seed = 1
    # the inference graph (networks/las.py, fortraining=False)
    beam_width = 1000
    max_decode_steps = 100
    length_penalty_weight = 0.5

    def make_engine(self, config, device, stream):
        e = LasEngine(config.feature_size, self.num_classes, num_hidden=self.num_hidden, num_layers=self.num_layers,
                      sampling_probability=self.sampling_probability, seed=self.sampling_seed,
                      learning_rate=config.learningrate, device_id=device, stream=stream)
        if self.coll.world > 1:
            p, seed, counter, _ = e.sampling_state()
            e.set_sampling_state(p, seed, counter, self.coll.rank)
        if getattr(config, 'lm_file', None):
            from ..lm import load_for
            e.set_lm(load_for(config), config.lm_weight)
        return e

    def initial_params(self, tensors, seed):
        """glorot-uniform kernels and attention_v (a 1-D variable: fan_in = fan_out = its length), zero biases"""
        rs = np.random.RandomState(seed)
        chunks = []
        for name, _, rows, cols in tensors:
            if name.endswith('kernel'):
                lim = np.sqrt(6.0 / (rows + cols))
            elif name == 'attention_v':
                lim = np.sqrt(6.0 / (2 * rows))
            else:
                chunks.append(np.zeros(rows * cols))
                continue
            chunks.append(rs.uniform(-lim, lim, size=rows * cols))
        return np.concatenate(chunks).astype(np.float32)

    def model_state(self):
        p, seed, counter, _ = self.engine.sampling_state()
        return {'las_sampling': np.asarray([seed, counter], np.int64), 'las_sampling_p': np.float32(p)}

    def restore_model_state(self, npz):
        if 'las_sampling' in npz:
            seed, counter = (int(x) for x in npz['las_sampling'])
            _, _, _, tower = self.engine.sampling_state()
            self.engine.set_sampling_state(float(npz['las_sampling_p']), seed, counter, tower)

    # ------------------------------------------------------------------ the step
    def _tower_pass(self, f, l, s, ll, tower, counter, grads):
        """one tower's pass of a step; every tower of a step draws with the step's counter (its own tower index keys its
        samples), so time-sliced towers and one process per tower feed the same inputs"""
        p, seed, _, _ = self.engine.sampling_state()
        self.engine.set_sampling_state(p, seed, counter, tower)
        self._upload(f, l, s, ll, training=grads)      # (validate runs the training graph on unmasked features)
        if grads:
            self.engine.compute_grads()
        else:
            self.engine.las_forward_resident(sample=True)
        loss = self.engine.get_loss()
        ler = label_error_rate(model_ids(self.engine.logits(), ll), l)
        return loss, ler

    def begin_step(self, mfccs, labels, seq_len, labels_len):
        self.global_step += 1
        self._begun = (mfccs, labels, seq_len, labels_len)

    def _next_counter(self, counter):
        """one counter value per step (train or validate), whatever the number of towers"""
        p, seed, _, tower = self.engine.sampling_state()
        self.engine.set_sampling_state(p, seed, counter + 1, tower)

    def finish_step(self, lazy=False):
        mfccs, labels, seq_len, labels_len = self._begun
        self._begun = None
        n, mine = self._towers()
        counter = self.engine.sampling_state()[2]
        if len(mine) == 1:
            f, l, s, ll = take_shard(mfccs, labels, seq_len, labels_len, n, mine[0])
            loss, ler = self._tower_pass(f, l, s, ll, mine[0], counter, True)
            self._next_counter(counter)
            if self.coll.world > 1:
                if self._grad_tensor is None:
                    self._grad_tensor = self.engine.grad_tensor()
                self.coll.all_reduce_sum_(self._grad_tensor)
            self._apply_adam(1.0 / n)
            if self.coll.world > 1:
                loss, ler = self.coll.mean_scalars([loss, ler])
            return np.float32(loss), np.float32(ler)
        losses, lers, gsum = [], [], None
        for k in mine:
            f, l, s, ll = take_shard(mfccs, labels, seq_len, labels_len, n, k)
            loss, ler = self._tower_pass(f, l, s, ll, k, counter, True)
            losses.append(loss)
            lers.append(ler)
            g = self.engine.get_grads().astype(np.float64)
            gsum = g if gsum is None else gsum + g
        self._next_counter(counter)
        self.engine.set_grads((gsum / n).astype(np.float32))
        self._apply_adam(1.0)
        return np.float32(np.mean(losses)), np.float32(np.mean(lers))

    def stage_batch(self, mfccs, labels, seq_len, labels_len):
        return False

    def _settle(self):
        pass

    def validate(self, mfccs, labels, seq_len, labels_len):
        """the training graph's loss and LER (sampling on; no update)"""
        n, mine = self._towers()
        counter = self.engine.sampling_state()[2]
        losses, lers = [], []
        with self._averaged():                 # (ema_decay: the averaged variables; the sampling state is not one)
            for k in mine:
                f, l, s, ll = take_shard(mfccs, labels, seq_len, labels_len, n, k)
                loss, ler = self._tower_pass(f, l, s, ll, k, counter, False)
                losses.append(loss)
                lers.append(ler)
        self._next_counter(counter)
        loss, ler = float(np.mean(losses)), float(np.mean(lers))
        if self.coll.world > 1:
            loss, ler = self.coll.mean_scalars([loss, ler])
        return [np.float32(loss), np.float32(ler)]

    def _markers(self):
        start, end = getattr(self.config, 'start_marker', None), getattr(self.config, 'end_marker', None)
        if not start or not end:
            raise ValueError('LAS decoding needs start_marker and end_marker in the [MFCC Featurizer] section of the config '
                             '(preprocess_mfcc writes them into the labels)')
        return self.config.symbols.get_id(start), self.config.symbols.get_id(end)

    def _beam_search(self, mfccs, seq_len, trace):
        start, end = self._markers()
        args = (self.beam_width, self.max_decode_steps, start, end, self.length_penalty_weight)
        with self._averaged():
            if isinstance(mfccs, AudioBatch):
                self._upload_audio(mfccs)             # the front end once; the search reads the resident batch
                return self.engine.beam_search_resident(*args, trace=trace)
            return self.engine.beam_search(mfccs, seq_len, *args, trace=trace)

    def evaluate(self, mfccs, labels, seq_len, labels_len):
        """[model [B, T_dec], loss, ler]: beam 0 of the gathered ids, beam_sequence_loss of the step scores, and the LER of
        the model against the labels (id 0 dropped from both; the end marker stays in the hypothesis)"""
        out = self._beam_search(mfccs, seq_len, True)
        model = out['predicted_ids'][:, :, 0].astype(np.int64)
        loss = beam_sequence_loss(out['scores'], labels, labels_len)
        return [model, np.float32(loss), np.float32(label_error_rate(model, labels))]

    def decode(self, mfccs, seq_len):
        """the first utterance's model: beam 0 of the gathered ids [T_dec]"""
        out = self._beam_search(mfccs, seq_len, False)
        return out['predicted_ids'][0, :, 0].astype(np.int64)

    def align(self, mfccs, labels, seq_len, labels_len):
        raise NotImplementedError('forced alignment walks the CTC lattice of a label; the LAS network has no CTC output '
                                  '(its attention weights are not an alignment this package defines)')

    def align_audio(self, audios, rates, labels, labels_len):
        return self.align(None, labels, None, labels_len)
