/* nasr.h — C ABI of libnasr.so: the MI355X (gfx950) implementation of NeuralASR's CTC training
 * hot path ((Bi)LSTM stack -> affine projection -> CTC loss/gradient -> Adam), one handle per
 * GPU / process.
 *
 * The reference has no FFI: its hot path is a TensorFlow-1 graph driven from Python
 * (/root/reference/networks/tfnetwork.py).  Each entry point below names the reference
 * interface it replaces; the Python `Network` subclass in neuralasr_amd/networks binds them
 * with ctypes (INTEGRATION.md shows the stub a NeuralASR maintainer would add).
 *
 * Conventions
 *   - every function returns 0 on success, <0 on error; nasr_last_error() gives the message
 *     (NASR_ERR_INFEASIBLE mirrors TF's "Not enough time for target transition sequence").
 *   - the caller owns every host buffer; the library owns all device memory.
 *   - one host thread per handle; a handle is not re-entrant (tfnetwork.py: one Session).
 *   - features are batch-major float32 [B,T,F] C-contiguous, zero past seq_len (dataset.py:75-77);
 *     labels int32 [B,Lmax] padded with 0; label ids in [0, C-2]; blank = C-1 (A.4).
 *   - flat parameter / gradient order is TF variable order: per layer (fw kernel [I+H,4H] rows
 *     [input;h], gate columns i,j,f,o; fw bias [4H]; bw kernel; bw bias) or (kernel, bias);
 *     then W [Hin,C], b [C]  (SURVEY.md §8b, Appendix A.1).
 *   - there is NO CPU fallback: nasr_create fails when no gfx950 device is usable.
 */
#ifndef NASR_H
#define NASR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NASR_OK 0
#define NASR_ERR_ARG (-1)        /* bad argument / shape */
#define NASR_ERR_HIP (-2)        /* HIP runtime error */
#define NASR_ERR_INFEASIBLE (-3) /* CTC: label needs more frames than seq_len (TF InvalidArgument) */
#define NASR_ERR_STATE (-4)      /* call order (e.g. backward without a resident batch) */

#define NASR_MERGE_NONE 0          /* unidirectional (networks/lstm_ctc_net.py:17-23) */
#define NASR_MERGE_STACK_RESHAPE 1 /* literal BiLstmCTCNet: tf.reshape on the (fw,bw) tuple
                                      (networks/bilstm_ctc_net.py:33,45) */
#define NASR_MERGE_CONCAT 2        /* tf.concat(outputs, 2) (networks/deepspeech.py:103) */

typedef struct nasr_ctx* nasr_handle;

/* Model + optimiser shape.  Replaces the hard-coded locals of create_network
 * (networks/bilstm_ctc_net.py:14, networks/lstm_ctc_net.py:14-15) and the AdamOptimizer
 * defaults of setup_training_network (networks/tfnetwork.py:116-117). */
typedef struct {
  int32_t feature_size;  /* F = (2*numcontext+1)*numcep  (config.py:25) */
  int32_t hidden;        /* H: LSTM units per direction */
  int32_t num_layers;
  int32_t bidirectional; /* 0 | 1 */
  int32_t merge;         /* NASR_MERGE_* */
  int32_t num_classes;   /* C = symbols.counter (networks/tfnetwork.py:18); blank = C-1 */
  float forget_bias;     /* 1.0 (BasicLSTMCell / LSTMCell default) */
  float learning_rate;   /* config.learningrate */
  float beta1, beta2, epsilon; /* 0.9, 0.999, 1e-8 */
  /* DeepSpeech family (networks/deepspeech.py:10-132): clipped-ReLU dense stages with dropout in front of the LSTM
   * stack (layers 1-3: widths n_hidden, n_hidden, 2*n_cell_dim) and one between the stack and the logits (layer 5).
   * All zero for the (Bi)LstmCTCNet models.  With any of them set the variable order is the creation order of
   * deepspeech.py: b1,h1,b2,h2,b3,h3, fw kernel, fw bias, bw kernel, bw bias, b5,h5, b6,h6 (bias BEFORE weight). */
  int32_t num_pre;       /* 0..3 dense stages before the stack */
  int32_t pre_width[3];
  int32_t post_width;    /* 0 = none */
  float relu_clip;       /* 20.0 */
  float dropout[4];      /* drop probability of the pre stages, then of the post stage ([0.05,0.05,0.05] and 0.05) */
} nasr_model_cfg;

/* Phase timings of the last nasr_compute_grads / nasr_apply_adam (HIP events on the handle's
 * stream), milliseconds.  Used by bench.py's roofline object. */
typedef struct {
  float pack_ms;      /* feature transpose+pad into time-major HBM layout */
  float xproj_ms;     /* input-to-hidden GEMMs (all layers) */
  float rec_fwd_ms;   /* forward recurrence: all layers' per-timestep kernels */
  float proj_ctc_ms;  /* projection GEMM + CTC (logZ, alpha/beta, gradient) */
  float proj_bwd_ms;  /* projection backward GEMMs */
  float rec_bwd_ms;   /* BPTT: all layers' per-timestep kernels */
  float wgrad_ms;     /* weight-gradient / input-gradient GEMMs + bias column sums */
  float adam_ms;      /* fused Adam + recurrent-weight repack */
  float total_ms;
  int32_t rec_fwd_launches; /* kernel launches of the recurrence in rec_fwd_ms (T per layer, or 1 when persistent) */
  int32_t rec_bwd_launches;
} nasr_phase_times;

/* ---- lifetime ---------------------------------------------------------------------------
 * nasr_create replaces TensorFlowNetwork.__init__ graph construction + tf.Session
 * (networks/tfnetwork.py:14-43).  `stream` is a hipStream_t to launch on (NULL: the library
 * creates its own); pass torch.cuda.current_stream().cuda_stream to order the handle's work
 * with torch.distributed collectives.  Parameters start at zero: call nasr_set_params. */
int nasr_create(const nasr_model_cfg* cfg, int device_id, void* stream, nasr_handle* out);
int nasr_destroy(nasr_handle h);
/* message of the CALLING THREAD's last failed call on h (h NULL: of a failed nasr_create); valid until that thread's next
 * failing call.  Per thread, so that nasr_stage_batch* on a loader thread and the training thread never read or overwrite
 * each other's text. */
const char* nasr_last_error(nasr_handle h);
const char* nasr_backend(nasr_handle h);    /* "hip-gfx950" */
int nasr_synchronize(nasr_handle h);        /* hipStreamSynchronize on the handle's stream */

/* ---- parameters / optimiser state (replaces tf.train.Saver's view of the variables,
 * networks/tfnetwork.py:40,142-164; TF variable order) ------------------------------------ */
int64_t nasr_param_count(nasr_handle h);
int nasr_num_tensors(nasr_handle h);
/* name (<=63 chars), offset into the flat vector, rows, cols (cols = 1 for vectors) */
int nasr_tensor_info(nasr_handle h, int idx, char name[64], int64_t* offset, int64_t* rows, int64_t* cols);
int nasr_set_params(nasr_handle h, const float* flat, int64_t n);
int nasr_get_params(nasr_handle h, float* flat, int64_t n);
int nasr_set_adam_state(nasr_handle h, const float* m, const float* v, int64_t n, int64_t step);
int nasr_get_adam_state(nasr_handle h, float* m, float* v, int64_t n, int64_t* step);
int nasr_set_learning_rate(nasr_handle h, float lr);
/* the step size the next nasr_apply_adam is launched with: the create call's, or what nasr_set_learning_rate set last (a
 * launch argument: a step already enqueued keeps its own) */
int nasr_get_learning_rate(nasr_handle h, float* lr);

/* ---- one-call entry points over host buffers -------------------------------------------
 * nasr_train_step replaces sess.run([optimizer, loss]) of TensorFlowNetwork.train
 * (networks/tfnetwork.py:183-190) for one tower: forward, CTC, backward, Adam.  loss_out =
 * reduce_mean of the per-utterance CTC NLL (networks/tfnetwork.py:59). */
int nasr_train_step(nasr_handle h, const float* feats, const int32_t* seq_len, const int32_t* labels,
                    const int32_t* label_len, int B, int T, int Lmax, float* loss_out);
/* forward only (inference graph, networks/tfnetwork.py:33-37): logits_out is time-major
 * [T',B,C] with T' = nasr_logit_frames(h,T) (2T for STACK_RESHAPE; of ceil(T/s) frames under nasr_set_frame_skip(h, s)).
 * May be NULL. */
int nasr_forward(nasr_handle h, const float* feats, const int32_t* seq_len, int B, int T, float* logits_out);
int nasr_logit_frames(nasr_handle h, int T);
/* loss of validate()/evaluate() (networks/tfnetwork.py:166-177): forward + CTC, no update.
 * nll_out [B] per-utterance (may be NULL). */
int nasr_loss(nasr_handle h, const float* feats, const int32_t* seq_len, const int32_t* labels,
              const int32_t* label_len, int B, int T, int Lmax, float* loss_out, float* nll_out);
/* parity hook: loss + d loss/d every variable, TF order, no update.  flat_grads_out [param_count]. */
int nasr_loss_and_grads(nasr_handle h, const float* feats, const int32_t* seq_len, const int32_t* labels,
                        const int32_t* label_len, int B, int T, int Lmax, float* loss_out, float* nll_out,
                        float* flat_grads_out);
/* tf.nn.ctc_greedy_decoder(merge_repeated=True), the decoder named at networks/tfnetwork.py:62-63:
 * ids_out [B, T'] (row b holds lens_out[b] ids), lens_out [B]. */
int nasr_greedy_decode(nasr_handle h, const float* feats, const int32_t* seq_len, int B, int T,
                       int32_t* ids_out, int32_t* lens_out);

/* ---- data-parallel building blocks (one shard per GPU; replaces make_parallel +
 * average_gradients, networks/tfnetwork.py:72-140).  Typical step on every rank:
 *   nasr_upload_batch(shard) ; nasr_compute_grads ; all-reduce(sum) nasr_grad_device_ptr over
 *   RCCL ; nasr_apply_adam(1/world) ; nasr_get_loss
 * The gradient buffer is one flat fp32 device array of nasr_grad_device_count elements in the
 * library's padded internal layout (identical on every rank; padding elements are always 0).  Its first 32
 * floats are not gradients: the first of them is the step's FAULT word (0, or 1 when this rank's persistent
 * recurrence gave up).  Reduce the whole array: a non-zero sum makes nasr_apply_adam a no-op on every rank and
 * nasr_get_loss return NASR_ERR_HIP ("step void"), so the replicas never diverge.
 *
 * Overlapping the exchange with the backward pass (the reference's towers cannot: average_gradients waits for
 * every tower's full gradient list, tfnetwork.py:72-86): the array is cut into nasr_grad_bucket_count()
 * contiguous buckets in the order nasr_compute_grads completes them (top LSTM layer + W + b first, then one per
 * layer going down, the bottom layer + the fault word last; a one-layer net has one bucket).
 * nasr_grad_bucket(i) gives bucket i's [offset, offset + count) in floats from nasr_grad_device_ptr();
 * nasr_grad_bucket_wait(i, s) makes HIP stream s wait until the nasr_compute_grads call issued before it has
 * finished bucket i (no host sync).  All-reduce bucket i on s after that wait, for i = 0 .. count-1, then make the
 * handle's stream wait for s before nasr_apply_adam.  The buckets cover the whole array exactly once. */
int nasr_upload_batch(nasr_handle h, const float* feats, const int32_t* seq_len, const int32_t* labels,
                      const int32_t* label_len, int B, int T, int Lmax);
/* Same, but the context stacking of utils.py:8-21 (include_context) happens on the device: `centre` is the
 * un-stacked [B,T,numcep] slice (for features made by preprocess_mfcc.py: columns [numcontext*numcep,
 * (numcontext+1)*numcep) of the stacked array), pad_value[b] the value the stacked array holds in the
 * out-of-utterance context frames of utterance b (its element [b,0,0]).  Needs feature_size ==
 * (2*numcontext+1)*numcep.  Moves 1/(2*numcontext+1) of the bytes over PCIe.  `numcep` here is the width of one
 * un-stacked frame: nasr_mfcc_width of the features' config (the static columns and their deltas). */
int nasr_upload_batch_context(nasr_handle h, const float* centre, const float* pad_value, int numcontext, int numcep,
                              const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
                              int Lmax);
/* The input pipeline's half of the step (dataset.py:33-40 loads and train.py:23-26 times the NEXT batch inside the
 * step): nasr_stage_batch copies a batch into one of the handle's staging slots - host side
 * through pinned memory (hipHostMalloc), device side with hipMemcpyAsync on the handle's COPY stream - while the
 * compute stream is busy with the current step, and returns a ticket; nasr_commit_batch(ticket) makes that batch the
 * resident one (the compute stream waits for the slot's copy event; no host sync).  At most two batches
 * staged ahead (NASR_ERR_STATE beyond that); a synchronous upload always finds a slot.  nasr_stage_batch* may be called from another host thread than the rest
 * of the handle's calls (a loader thread); everything else stays one thread per handle.  The synchronous
 * nasr_upload_batch* = stage on the compute stream + commit. */
int nasr_stage_batch(nasr_handle h, const float* feats, const int32_t* seq_len, const int32_t* labels,
                     const int32_t* label_len, int B, int T, int Lmax, int* ticket);
int nasr_stage_batch_context(nasr_handle h, const float* centre, const float* pad_value, int numcontext, int numcep,
                             const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
                             int Lmax, int* ticket);
/* (utils.py:24-31 feeding dataset.py:33-40) A batch straight from audio: the utterances audio[offsets[b] ..
 * offsets[b+1]) at rates[b] Hz (NULL: all at the featurizer's samplerate) go through `featurizer`'s front end - resampler,
 * features, whole-utterance normalisation (or the causal rule, nasr_mfcc_cfg.norm = 1: every pad value is then 0) - on
 * the device, and its last kernel writes the normalised centre frames
 * [B,T,D] (D = nasr_mfcc_width of the featurizer's config; zeros past an utterance's end) and the pad values straight into `model`'s batch slot, in the layout of
 * nasr_upload_batch_context: no feature crosses PCIe in either direction.  T = the longest utterance's nasr_mfcc_frames,
 * seq_len_out[b] = utterance b's; both are computed on the host and written before anything is launched.  The slot holds
 * the same bits as nasr_featurize_rates + zero-padding to T + nasr_upload_batch_context give it.  Staging runs copies
 * and kernels on the model's copy stream; a later nasr_featurize* / nasr_resample on the featurizer handle is ordered
 * behind them by an event (no host wait).  One thread at a time per featurizer handle.  nasr_commit_batch,
 * nasr_discard_batch and the two-ahead limit apply.  NASR_ERR_STATE: `featurizer` is not a featurizer handle, `model` is
 * one, or they sit on different devices; NASR_ERR_ARG: feature_size != (2*numcontext+1)*D, a bad rate or a
 * too-short utterance (named), and what nasr_upload_batch refuses, with the computed seq_len. */
int nasr_upload_batch_audio(nasr_handle model, nasr_handle featurizer, const float* audio, const int64_t* offsets,
                            const int32_t* rates, const int32_t* labels, const int32_t* label_len, int B, int Lmax,
                            int32_t* seq_len_out, int* T_out);
/* (utils.py:24-31 feeding dataset.py:33-40) the same as the staging half of a step: see nasr_stage_batch */
int nasr_stage_batch_audio(nasr_handle model, nasr_handle featurizer, const float* audio, const int64_t* offsets,
                           const int32_t* rates, const int32_t* labels, const int32_t* label_len, int B, int Lmax,
                           int32_t* seq_len_out, int* T_out, int* ticket);
/* (No counterpart in the reference: its only augmentation is rand_shift, dataset.py:23-31.)  SpecAugment masks for a
 * batch in the centre form: utterance b's time mask k zeroes the normalised centre frames [t0, t0 + tw), its frequency
 * mask k the columns [f0, f0 + fw) of every static_width-wide block of a frame ([static | delta | delta-delta]: column
 * j of each block derives from filter j).  0 is the utterance's own mean after the whole-utterance normalisation (the
 * running mean under the causal rule), which is computed before masking.  The context stacking runs on the masked frames: a masked frame is masked in every window
 * it appears in, the pad values are never masked.  A mask of width 0 is no mask. */
#define NASR_AUG_MAX_MASKS 8
typedef struct {
  int32_t static_width;      /* width of the frame's static block; must divide the frame width */
  int32_t n_time, n_freq;    /* masks per utterance, each 0..NASR_AUG_MAX_MASKS */
  const int32_t* time_mask;  /* [B][n_time][2]: first frame, width (0 = no mask) */
  const int32_t* freq_mask;  /* [B][n_freq][2]: first static column, width */
} nasr_batch_aug;
/* (No counterpart in the reference.)  nasr_upload_batch_context with the masks of `aug` applied on the device, inside the
 * kernel that stacks the context: the masks travel with the batch's other integer arrays, there is no extra pass, buffer
 * or launch.  The result is bitwise what nasr_upload_batch gives for the stacked array of the masked centre frames.
 * aug == NULL, or masks that all have width 0: nasr_upload_batch_context itself.  NASR_ERR_ARG, before anything is
 * launched and with the resident batch kept, names the utterance and the mask: t0 < 0, tw < 0, t0 + tw > seq_len[b];
 * f0 < 0, fw < 0, f0 + fw > static_width; a count outside 0..NASR_AUG_MAX_MASKS; static_width not a divisor of numcep. */
int nasr_upload_batch_context_aug(nasr_handle h, const float* centre, const float* pad_value, int numcontext, int numcep,
                                  const int32_t* seq_len, const int32_t* labels, const int32_t* label_len, int B, int T,
                                  int Lmax, const nasr_batch_aug* aug);
/* (No counterpart in the reference.)  nasr_upload_batch_audio / nasr_stage_batch_audio with the masks of `aug`: the same
 * rules, checked against the seq_len the call itself computes; static_width must be the featurizer's numcep (the
 * width of the static block of its frames).  aug == NULL: the plain call. */
int nasr_upload_batch_audio_aug(nasr_handle model, nasr_handle featurizer, const float* audio, const int64_t* offsets,
                                const int32_t* rates, const int32_t* labels, const int32_t* label_len, int B, int Lmax,
                                int32_t* seq_len_out, int* T_out, const nasr_batch_aug* aug);
int nasr_stage_batch_audio_aug(nasr_handle model, nasr_handle featurizer, const float* audio, const int64_t* offsets,
                               const int32_t* rates, const int32_t* labels, const int32_t* label_len, int B, int Lmax,
                               int32_t* seq_len_out, int* T_out, const nasr_batch_aug* aug, int* ticket);
/* (No counterpart in the reference: its only augmentation is rand_shift, dataset.py:23-31.)  Waveform augmentation of a
 * batch that is given as audio, on the samples at the featurizer's rate, behind the resampler: every
 * array is [B].  rir[b] (rir NULL: none) is an index into the featurizer's RIR bank (nasr_featurizer_set_rirs) or -1:
 * utterance x [N] with the RIR h [K] becomes y[t] = sum_{k=0..min(K-1,t)} h[k] x[t-k], t in [0,N) (the tail is dropped:
 * seq_len never changes), accumulated in float32 in an order that depends on (N, K, t) alone; -1: y is x, bit for bit.
 * noise[b] (noise NULL: none) is an index into the noise bank (nasr_featurizer_set_noise) or -1: with the clip c [L] and
 * noise_off[b] = o in [0,L), n[t] = c[(o+t) mod L], Ps = sum y^2 and Pn = sum n^2 over [0,N) in float64 in a fixed order,
 * g = float32(sqrt(Ps/Pn) 10^(-snr_db[b]/20)) (0 when Ps or Pn is 0) and z[t] = y[t] + g n[t] in float32 (two roundings);
 * -1: z is y, bit for bit.  noise_off and snr_db are read for the utterances with noise[b] >= 0 only. */
#define NASR_AUG_MAX_RIR_TAPS 8192
typedef struct {
  const int32_t* rir;        /* [B] index into the RIR bank, -1: none; NULL: none for the whole batch */
  const int32_t* noise;      /* [B] index into the noise bank, -1: none; NULL: none for the whole batch */
  const int64_t* noise_off;  /* [B] first sample of the clip, in [0, its length) */
  const float* snr_db;       /* [B] finite */
} nasr_wave_aug;
/* (No counterpart in the reference.)  nasr_upload_batch_audio_aug / nasr_stage_batch_audio_aug with the waveform
 * augmentation `wave` between the resampler and the spectral kernel: everything downstream runs on z unchanged, and the
 * result is bitwise that of the plain call on nasr_augment_audio's output.  wave == NULL (or both of its index arrays
 * NULL): the _aug call itself, no further launch and no further buffer.  NASR_ERR_ARG, before anything is launched and
 * with the resident batch kept, names the utterance: an index outside its bank (or no bank set), noise_off outside the
 * clip, a non-finite snr_db, noise without noise_off or snr_db. */
int nasr_upload_batch_audio_wave(nasr_handle model, nasr_handle featurizer, const float* audio, const int64_t* offsets,
                                 const int32_t* rates, const int32_t* labels, const int32_t* label_len, int B, int Lmax,
                                 int32_t* seq_len_out, int* T_out, const nasr_batch_aug* aug, const nasr_wave_aug* wave);
int nasr_stage_batch_audio_wave(nasr_handle model, nasr_handle featurizer, const float* audio, const int64_t* offsets,
                                const int32_t* rates, const int32_t* labels, const int32_t* label_len, int B, int Lmax,
                                int32_t* seq_len_out, int* T_out, const nasr_batch_aug* aug, const nasr_wave_aug* wave,
                                int* ticket);
int nasr_commit_batch(nasr_handle h, int ticket);
int nasr_discard_batch(nasr_handle h, int ticket);   /* give a staged batch's slot back unused */
/* nasr_forward / nasr_loss / nasr_greedy_decode on the batch that is resident already (nasr_upload_batch*,
 * nasr_commit_batch): what validation and decoding from audio run after nasr_upload_batch_audio.  NASR_ERR_STATE
 * without a resident batch (nasr_loss_resident: without labels in it). */
int nasr_forward_resident(nasr_handle h, float* logits_out);
int nasr_loss_resident(nasr_handle h, float* loss_out, float* nll_out);
int nasr_greedy_decode_resident(nasr_handle h, int32_t* ids_out, int32_t* lens_out);
int nasr_compute_grads(nasr_handle h);          /* forward+CTC+backward on the resident batch (async) */
/* ---- in-library gradient exchange: average_gradients (tfnetwork.py:72-86) for hosts without torch.distributed ------
 * One RCCL rank per handle (one process per GPU, or one host thread per handle).  librccl.so is bound with dlopen when
 * the first of these calls is made.  Rank 0 calls nasr_comm_unique_id and hands the 128 bytes to the other ranks by
 * the host's own means (MPI_Bcast, a file, a socket); every rank then calls nasr_comm_init (it blocks until all have
 * joined).  Per step:  nasr_compute_grads(h); nasr_comm_allreduce_grads(h); nasr_apply_adam(h, 1.f / nranks);
 * nasr_comm_allreduce_grads enqueues one sum all-reduce per gradient bucket on the handle's communication stream, each
 * behind its bucket's completion event (so the upper layers' gradients cross xGMI under the backward pass of the layers
 * below), and makes the handle's stream wait for the last one: no host synchronisation.  The step's fault word travels
 * in the last bucket, so a void step (nasr_step_void) is void on every rank.  nasr_comm_mean averages a few host floats
 * over the ranks (the reduce_mean of loss / LER at tfnetwork.py:135-136); without a communicator it leaves them as
 * they are.  It runs on a communicator and a stream of its own (ncclCommSplit of the handle's communicator at
 * nasr_comm_init), so it neither waits for the gradient buckets of a step in flight nor for the compute stream; with a
 * librccl that has no ncclCommSplit it shares the gradient communicator and is executed behind the buckets issued
 * before it (one communicator runs its collectives in issue order). */
int nasr_comm_unique_id(void* id128);
int nasr_comm_init(nasr_handle h, const void* id128, int rank, int nranks);
int nasr_comm_size(nasr_handle h);
int nasr_comm_allreduce_grads(nasr_handle h);
int nasr_comm_mean(nasr_handle h, float* vals, int n);
int nasr_comm_destroy(nasr_handle h);
/* In persistent mode bucket i's event is held back over the NEXT persistent BPTT launch (the layer below's), so that
 * a collective released by nasr_grad_bucket_wait co-runs with that layer's GEMM phase rather than with a launch whose
 * hand-offs want every CU's memory queue to themselves (default on, NASR_BUCKET_DEFER=0 at create); 0 records every
 * bucket's event as soon as its gradients are complete. */
int nasr_set_bucket_defer(nasr_handle h, int defer);
void* nasr_grad_device_ptr(nasr_handle h);
int64_t nasr_grad_device_count(nasr_handle h);
int nasr_grad_bucket_count(nasr_handle h);
int nasr_grad_bucket(nasr_handle h, int i, int64_t* offset, int64_t* count);
int nasr_grad_bucket_wait(nasr_handle h, int i, void* hip_stream);
int nasr_apply_adam(nasr_handle h, float grad_scale);
/* Global-norm gradient clipping with a non-finite guard (not part of the reference, whose optimiser step
 * - tfnetwork.py:116-139, average_gradients then apply_gradients - clips nothing and checks nothing).  With max_norm > 0
 * nasr_apply_adam (and nasr_train_step through it) first measures norm = |grad_scale| * sqrt(sum g_i^2) of the gradient
 * buffer as it stands then, i.e. after an all-reduce, in fp64 and in a fixed order (the same bits on every run and every
 * rank), and decides on the device, without a host round trip:
 *   - fault word set: the step is void as ever; nothing is measured, scaled or counted;
 *   - norm not finite: the step is SKIPPED - parameters, moments and Adam's step count stay as they were, `skipped`
 *     counts it; the fault word stays 0, so the step is not void, is not repeated and nasr_settle_* report nothing;
 *   - otherwise coef = norm > max_norm ? max_norm / norm : 1 (tf.clip_by_global_norm's rule; in double, rounded to fp32)
 *     and Adam runs on g * (grad_scale * coef), one fp32 product per element: with coef == 1 bit for bit the step
 *     without clipping.  max_norm = +inf measures and guards but never scales.
 * 0 = off (the default): nasr_apply_adam launches exactly what it launched before.  Negative or NaN: NASR_ERR_ARG.
 * nasr_get_grad_clip_stats synchronises: norm and coefficient of the last step that was not void, the largest finite norm and the
 * numbers of applied (steps), scaled (clipped) and skipped steps since the window was last cleared (reset != 0 clears
 * it behind the read). */
typedef struct {
  double last_norm, window_max_norm;
  float last_coef;
  int64_t steps, clipped, skipped;
} nasr_clip_stats;
int nasr_set_grad_clip(nasr_handle h, float max_norm);
int nasr_get_grad_clip(nasr_handle h, float* max_norm);
int nasr_get_grad_clip_stats(nasr_handle h, nasr_clip_stats* out, int reset);
/* Parameter averaging (not part of the reference, which checkpoints and decodes the last iterate only):
 * tf.train.ExponentialMovingAverage(decay, num_updates) of every trainable variable.  With decay in (0,1) the handle holds a
 * second parameter image E, and every nasr_apply_adam that is applied updates it inside the Adam sweep, from the
 * parameters P that sweep has just written:
 *   E <- E + (1 - d_n)(P - E),  d_n = min(decay, (1 + n) / (10 + n)),  n = updates applied so far, then n + 1
 * (d_n and 1 - d_n in double on the device, rounded to fp32; per element e = fma(1 - d_n, p - e, e)).  A void step (fault
 * word set) and a skipped step (non-finite norm under nasr_set_grad_clip) leave E and n as they leave P, M, V and Adam's
 * count.  P, M, V get the bits they get without averaging.
 * nasr_set_ema: 0 = off (the default; frees E: nasr_apply_adam launches exactly what it launched before).  The first call
 * with a decay in (0,1) allocates E, copies P into it (TF's initial shadow value) and sets n = 0; a later one only changes
 * the decay.  Anything else: NASR_ERR_ARG.  nasr_set_params does not touch E.
 * nasr_get_ema: the decay (0 = off), n (synchronises; 0 when off) and whether the average is live (below); each may be NULL. */
int nasr_set_ema(nasr_handle h, float decay);
int nasr_get_ema(nasr_handle h, float* decay, int64_t* updates, int* live);
/* E and n out of / into the handle, in the TF variable order of nasr_get_params / nasr_set_params (a checkpoint's view);
 * updates may be NULL in the getter.  NASR_ERR_STATE while averaging is off. */
int nasr_get_ema_state(nasr_handle h, float* flat, int64_t n, int64_t* updates);
int nasr_set_ema_state(nasr_handle h, const float* flat, int64_t n, int64_t updates);
/* Exchanges the CONTENTS of P and E on the handle's stream and rebuilds the operand images derived from P, so that every
 * forward-only call (nasr_forward*, nasr_loss*, nasr_greedy_decode*, nasr_ctc_align*, nasr_stream_feed*, the beam searches,
 * a distillation teacher's pass) runs on the average; nasr_get_params then returns the average and nasr_get_ema_state the
 * training parameters.  While the average is live (an odd number of swaps) nasr_compute_grads, nasr_apply_adam,
 * nasr_train_step, nasr_set_ema_state and nasr_set_ema(h, 0) return NASR_ERR_STATE and name themselves.  A second swap puts
 * P, E and every derived image back bit for bit.  NASR_ERR_STATE while averaging is off. */
int nasr_ema_swap(nasr_handle h);
/* Diagnostics - what ONE GPU can show of a collective that co-runs with the step (average_gradients moved under the
 * backward pass, tfnetwork.py:72-86): waits on `hip_stream` for bucket i like nasr_grad_bucket_wait, then launches there a
 * kernel shaped like a ring all-reduce step over that bucket - nblocks workgroups of 256 threads, each sweeping its slice
 * `passes` times with 16-byte loads and stores, the data unchanged.  tools/rccl_standin.py, tests/test_gpu_persist.py. */
int nasr_diag_bucket_traffic(nasr_handle h, int i, void* hip_stream, int nblocks, int passes);
/* The gradients of tfnetwork.py:120-128 are a set: nothing orders dW(l) before the backward pass of layer l-1.  With the
 * persistent recurrence, 500-wide layers and more than one layer, layer l's weight gradients run on a side stream beside the
 * persistent BPTT launch of layer l-1 (bitwise the gradients of the serial order).  On by default
 * (NASR_WGRAD_OVERLAP=0 at nasr_create turns it off); nasr_set_wgrad_overlap switches it for A/B measurements. */
int nasr_set_wgrad_overlap(nasr_handle h, int enabled);
int nasr_get_wgrad_overlap(nasr_handle h); /* g*grad_scale, TF Adam, step += 1 (async) */
/* copy the gradients out (TF order) / load externally reduced gradients (TF order) for nasr_apply_adam:
 * the single-process form of average_gradients (several towers time-sliced on one GPU). */
int nasr_get_grads(nasr_handle h, float* flat, int64_t n);
int nasr_set_grads(nasr_handle h, const float* flat, int64_t n);
int nasr_get_loss(nasr_handle h, float* loss_out);    /* synchronises; loss of last compute_grads */
/* synchronises; *void_out = 1 when the (all-reduced) fault word of the last step is set: nasr_apply_adam was a no-op on
 * every rank and the caller should run the step again (a rank whose persistent recurrence aborted has switched to the
 * per-step kernels by then).  Call it after nasr_apply_adam on every rank: all ranks get the same answer. */
int nasr_step_void(nasr_handle h, int* void_out);
/* The values Network.train returns (tfnetwork.py:183-190: loss, and the decode the LER is computed from) are known after
 * the forward pass and the CTC kernels; the backward pass, the gradient exchange and Adam need not be waited for.  With
 * nasr_set_step_decode(1) every nasr_compute_grads copies the loss, the fault word as it stands after the forward pass and
 * the greedy decode (ids [B][T'] row-major, lens [B]) to pinned host memory right behind the CTC kernels;
 * nasr_get_step_results waits for THAT copy only.  A host that returns from train() at this point enqueues the next
 * step while the device still runs the backward pass of this one: the device never waits for the host.  fault_out = 1:
 * this rank's forward recurrence aborted, the values are meaningless (then use nasr_step_void and repeat the step).
 * nasr_settle_step(h, previous, &v) waits for the END of the latest (previous = 0) or the one-before-latest (1) step
 * that reached nasr_apply_adam and says whether it was void (on every rank: the fault word is all-reduced with the
 * gradients); a void step's Adam launch was a no-op and is taken out of the step count.
 * A host that runs more than one step ahead names the step instead: nasr_step_token(h) = the sequence number of the
 * optimiser step nasr_apply_adam enqueued last (> 0; 0 = none yet), nasr_settle_token(h, token, &v) waits for the end of
 * exactly that step.  The library remembers the last 4 steps; an older token is NASR_ERR_STATE.  (What the reference
 * gets from sess.run returning, tfnetwork.py:188-190: the step is over and its update applied - here per step, without a
 * stream synchronisation.) */
int nasr_get_step_results(nasr_handle h, float* loss_out, int* fault_out, int32_t* ids_out, int32_t* lens_out);
int nasr_settle_step(nasr_handle h, int previous, int* void_out);
int64_t nasr_step_token(nasr_handle h);
int nasr_settle_token(nasr_handle h, int64_t token, int* void_out);
int nasr_resident_frames(nasr_handle h, int64_t* frames); /* sum(seq_len) of the resident batch: input frames, whatever the frame skip */
/* Ragged batches.  DataSet.get_next_batch (dataset.py:75-77) pads every utterance to the longest of its batch and
 * tf.nn.(bidirectional_)dynamic_rnn (networks/bilstm_ctc_net.py:40-53) masks by sequence_length.  Here, when at least
 * 15 % of a training batch's T x B frame rows are such padding, the operand passes and GEMMs of a plain (Bi)LSTM stack work
 * on the frames t < seq_len[b] only (gathered on the way in, scattered on the way out); the recurrences still run T steps.
 * Results are the uncompacted ones up to summation order.  On by default (NASR_COMPACT=0 in the environment: off);
 * a change takes effect with the next batch uploaded or committed.  nasr_resident_rows: the rows those passes cover for
 * the resident batch - sum(seq_len) when compacted, T x (B rounded up to 16) otherwise. */
int nasr_set_row_compaction(nasr_handle h, int enabled);
int nasr_resident_rows(nasr_handle h, int64_t* rows);
/* B and T of the resident batch as the caller gave them (0, 0 without one): what the *_resident calls size their outputs
 * by, through nasr_logit_frames(h, T). */
int nasr_resident_shape(nasr_handle h, int* B, int* T);

/* TensorFlowNetwork.train fetches mean_ler with every step (networks/tfnetwork.py:188-189): with
 * step-decode enabled nasr_compute_grads / nasr_loss also run the greedy decoder on the step's logits
 * (before the CTC gradient overwrites them); nasr_get_decoded returns that result (synchronises). */
int nasr_set_step_decode(nasr_handle h, int enabled);
/* enabled = 3: the step's logits are copied out as well (pinned memory, behind the CTC forward kernels, before the CTC
 * gradient overwrites them): nasr_get_step_logits waits for that copy only and returns them time-major [T',B,C], as
 * nasr_forward does.  The host can then run the reference's own decoder (nasr_ctc_beam_search) for the step's mean_ler
 * while the device runs the backward pass and the steps behind it (tfnetwork.py:61-70,188-189).  enabled = 2: the same
 * without the greedy decoder (a host with its own decoder has no use for it): nasr_get_step_results then returns loss and
 * fault word with empty hypotheses. */
int nasr_get_step_logits(nasr_handle h, float* logits_out);
int nasr_get_decoded(nasr_handle h, int32_t* ids_out /*[B,T']*/, int32_t* lens_out /*[B]*/);

/* create_model (networks/tfnetwork.py:61-64): tf.nn.ctc_beam_search_decoder on host logits, time-major
 * [T',B,C] (as nasr_forward returns them); TF defaults are beam_width 100, merge_repeated 1, top path only.
 * ids_out [B,T'] (row b holds lens_out[b] ids), logp_out [B] = log-probability of the best beam (may be NULL).
 * Host code (one thread per utterance), no GPU work. */
int nasr_ctc_beam_search(const float* logits, const int32_t* seq_len, int B, int Tp, int C, int beam_width,
                         int merge_repeated, int32_t* ids_out, int32_t* lens_out, float* logp_out);
/* The same search fused with a dense n-gram model over the label ids (not part of the reference).
 * lm_logp [K][C] float32 log-probabilities, K = C^(order-1), order in [1,4], K*C <= 2^24; row ctx is the history
 * id(t-1), ..., id(t-order+1) with the most recent id as the lowest digit in base C, histories before the start filled with
 * bos_id (in [0,C-1]); lm_eos [K]: the log-probability that the sequence ends after the history.  Every beam entry carries
 * the context of its prefix; wherever mass flows from an entry to its extension by label c, that contribution gets
 * weight * lm_logp[ctx(entry)][c] + bonus added (blank and repeat updates of an entry itself get nothing), pruning uses the
 * fused totals, and the top path is the one with the largest total + weight * lm_eos[ctx], which logp_out receives.  The
 * score of a labelling y is therefore log P_ctc(y) + sum_i (weight * lm(y_i | y_<i) + bonus) + weight * eos(ctx(y)).
 * merge_repeated collapses the output only: contexts are those of the unmerged prefix.  Every entry of lm_logp and lm_eos
 * must be finite (not checked here: the call would read the whole table every time; a forbidden symbol is a large negative
 * value, not -inf, since 0 * -inf is NaN and weight 0 would no longer be the plain search).  lm_logp == NULL: exactly
 * nasr_ctc_beam_search (the remaining LM arguments are not read). */
int nasr_ctc_beam_search_lm(const float* logits, const int32_t* seq_len, int B, int Tp, int C, int beam_width,
                            int merge_repeated, const float* lm_logp, const float* lm_eos, int order, int bos_id,
                            float weight, float bonus, int32_t* ids_out, int32_t* lens_out, float* logp_out);

/* ---- streaming recognition -----------------------------------------------------
 * A causal network (networks/lstm_ctc_net.py: unidirectional LSTM cells) fed chunk by chunk: a stream session keeps, per
 * LSTM layer and stream slot, the cell's (c, h) in fp32 on the device, and a feed is a forward pass over one chunk that
 * starts every slot from its saved state and saves the state at the slot's last frame.  The logits of an utterance fed in
 * chunks are those of nasr_forward on the whole utterance up to summation order (the bulk GEMMs split their sums by the
 * row count), not bit for bit; the same sequence of feeds gives the same bits.  Feeds run the per-timestep recurrence
 * kernels whatever nasr_get_recurrence_mode says, leave that mode and nasr_get_persist_stats alone, and change nothing
 * of the parameters, Adam's state, the gradient buffer, the dropout state or the clip statistics.  Batch calls
 * between feeds are allowed and do not touch the stream state; parameters may change between feeds (nasr_set_params, a
 * training step): the state is simply carried. */
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  Opens the handle's stream session with
 * S slots (concurrent streams), 1 <= S <= 64 (else NASR_ERR_ARG), all state zero.  NASR_ERR_STATE, with the reason in
 * nasr_last_error: a second open; a bidirectional config; a dropout probability > 0 (the reference applies dropout in
 * every graph, keyed by the pass counter); a WaveNet, LAS or featurizer handle. */
int nasr_stream_open(nasr_handle h, int S);
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  Ends the session and frees its
 * state.  NASR_ERR_STATE without one, as for every call below. */
int nasr_stream_close(nasr_handle h);
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  Zeroes the state and the frame count
 * of the n slots listed (slots == NULL: of every slot), and their front-end state when the session takes samples
 * (nasr_stream_attach_audio): a new utterance starts there.  A slot outside [0,S-1]:
 * NASR_ERR_ARG, nothing reset. */
int nasr_stream_reset(nasr_handle h, const int32_t* slots, int n);
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  One chunk: feats [S][Tc][F], n_frames
 * [S] with n_frames[b] in [0,Tc] frames of slot b (0: the slot is idle in this chunk and keeps its state).  logits_out
 * time-major [Tc][S][C] as nasr_forward returns them; rows t >= n_frames[b] are unspecified.  Synchronises.  The chunk
 * replaces the resident batch as nasr_forward does, and is itself none for the *_resident calls: they answer NASR_ERR_STATE
 * until the next upload.  NASR_ERR_ARG, with the resident batch kept: Tc < 1, an n_frames outside [0,Tc], a null
 * buffer. */
int nasr_stream_feed(nasr_handle h, const float* feats, const int32_t* n_frames, int Tc, float* logits_out);
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  frames_out [S]: the frames each slot
 * has consumed since its reset. */
int nasr_stream_frames(nasr_handle h, int64_t* frames_out);
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  The session's state, [L][S][2][H]
 * float32: per layer and slot the cell's c, then its h, as of the slot's last frame; n must be L*S*2*H.  Synchronises. */
int nasr_stream_get_state(nasr_handle h, float* state, int64_t n);
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  Replaces the session's state (the
 * layout of nasr_stream_get_state; the frame counts stay): continuing on another handle with the same parameters gives
 * the first handle's logits bit for bit.  The state does not carry a slot's frame-skip phase (nasr_set_frame_skip): every
 * slot starts at phase 0 behind this call, as if its next input row were its utterance's first. */
int nasr_stream_set_state(nasr_handle h, const float* state, int64_t n);
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances, utils.py:29 normalises them whole.)  The
 * session takes SAMPLES from now on: `featurizer`, a featurizer handle with norm = 1 (the causal rule at nasr_mfcc_cfg), turns
 * each slot's samples into the chunk's stacked rows on the device.  Called once, after nasr_stream_open;
 * the featurizer must outlive the session, its scratch buffers are shared with its other calls (ordered by an event, as
 * for nasr_upload_batch_audio; one thread at a time per featurizer handle).  Per slot the device keeps the un-framed tail
 * of the samples with the one sample in front of it that pre-emphasis reads, the running sums S1, S2, the raw frames that
 * wait for the norm_min_frames-th (at most that many) and a ring of the last 2*numcontext normalised frames: nothing
 * grows with the utterance.  NASR_ERR_STATE: `featurizer` is not a featurizer handle, sits on another device, has
 * norm != 1, or samples are attached already; NASR_ERR_ARG: feature_size != (2*numcontext+1)*D. */
int nasr_stream_attach_audio(nasr_handle model, nasr_handle featurizer);
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  Host only: what a
 * nasr_stream_feed_audio of n_samples [S] new samples per slot, with last [S] (nullable), would emit now: rows_out [S] and
 * *Tc_out = their maximum, which sizes logits_out.  With n samples of an utterance received, Fc = 0 if n < frame_len else
 * 1 + (n - frame_len) / frame_step frames are complete, and the rows that exist are nasr_mfcc_frames(n) once the utterance
 * is declared finished, else 0 while Fc < norm_min_frames, else max(0, Fc - numcontext); a feed emits the difference.  The
 * errors are those of the feed; nothing changes. */
int nasr_stream_audio_rows(nasr_handle model, const int64_t* n_samples, const uint8_t* last, int32_t* rows_out, int* Tc_out);
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  One feed of samples at the
 * featurizer's rate (no resampling in a session): slot b's new samples are audio[offsets[b] .. offsets[b+1]), none is
 * allowed (the slot is idle, or finishing); last[b] != 0 (last nullable) declares slot b's utterance complete: only then is
 * a zero-padded final frame made.  On the handle's stream: the samples are appended to each slot's tail, the spectral
 * kernel of nasr_featurize runs on the newly complete frames, the running sums advance frame by frame, every frame u
 * whose n_u = max(u+1, norm_min_frames) frames (capped by the utterance's own at `last`) exist is normalised with exactly
 * S[n_u] - whenever its samples happen to arrive - and a kernel writes the chunk's stacked rows [S][Tc][F] into the chunk's
 * batch slot; then the forward pass of nasr_stream_feed.  rows_out [S] and *Tc_out as nasr_stream_audio_rows gives them;
 * logits_out [Tc][S][C] (logits_rows >= Tc rows of it), rows t >= rows_out[b] of slot b unspecified.  The logits are, bit
 * for bit, those of nasr_stream_feed given the rows of nasr_featurize (norm = 1) of the whole utterance.  Tc = 0: no
 * forward pass runs and the resident batch is kept.  After a feed with last[b] the slot waits for nasr_stream_reset, which
 * also clears its front-end state; until then any sample or `last` for it is NASR_ERR_STATE.  NASR_ERR_ARG, nothing
 * changed: `last` on a slot that has received no sample at all (named), offsets that decrease, logits_rows < Tc, more
 * than 2^28 samples; NASR_ERR_STATE: no samples attached. */
int nasr_stream_feed_audio(nasr_handle model, const float* audio, const int64_t* offsets, const uint8_t* last, int32_t* rows_out,
                           int* Tc_out, float* logits_out, int64_t logits_rows);

/* ---- streaming the bidirectional networks with a bounded look-ahead -------------------------------
 * The latency-controlled BiLSTM: a look-ahead session of S slots and R look-ahead frames keeps, per slot, the FORWARD
 * direction's (c, h) per layer (the layout of nasr_stream_get_state) and up to R held feature rows.  A feed gives slot b
 * n[b] >= 0 new rows and an optional last[b]; with P = held[b] + n[b] pending rows it emits E = P rows with last[b], else
 * E = max(0, P - R), and the last P - E rows stay held.  A slot with E = 0 runs nothing; if every slot has E = 0 no pass
 * runs and the resident batch is kept.  A slot with E > 0 runs its WINDOW, all P pending rows, through the whole network:
 * dense stages row by row, every layer's forward direction from the saved state (saved again as of row E - 1), every
 * layer's backward direction from zero at row P - 1 down to row 0; logits are returned for rows 0 .. E-1, and the P - E
 * look-ahead rows are computed again as the head of the next window.  THE RESULT DEPENDS ON HOW THE INPUT WAS SPLIT INTO
 * FEEDS: a frame's backward context is between R and R + E - 1 frames.  It is the whole-utterance network (to fp32
 * tolerance) when one window covers the utterance.  The same feeds give the same bits.  What nasr_stream_open's comment
 * says about the per-step kernels, the handle's parameters and batch calls between feeds holds here too.
 * On such a session nasr_stream_reset (the held rows go too), _close, _frames (rows EMITTED) and _get_state (the forward
 * state) work; nasr_stream_set_state only while no slot holds rows (else NASR_ERR_STATE); nasr_stream_feed is
 * NASR_ERR_STATE, as nasr_stream_feed_lookahead and nasr_stream_lookahead_rows are on a session of nasr_stream_open.
 * nasr_stream_attach_audio / _feed_audio / _audio_rows work: the rows the causal front end makes for a feed join the
 * slot's pending rows on the device, the window rule applies to them, `last` completes the front end's hold-back and
 * the look-ahead, and rows_out / Tc_out count the rows emitted after both. */
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  Opens a look-ahead session: 1 <= S <= 64
 * slots, 1 <= R <= 1024 look-ahead frames (else NASR_ERR_ARG), all state zero, nothing held.  NASR_ERR_STATE, with the
 * reason in nasr_last_error: a unidirectional config (use nasr_stream_open); NASR_MERGE_STACK_RESHAPE (its logits mix frames of
 * the whole padded batch: no chunk of it is a point in time); a dropout probability > 0; a WaveNet, LAS or featurizer
 * handle; a second session. */
int nasr_stream_open_lookahead(nasr_handle h, int S, int R);
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  Host only: what a
 * nasr_stream_feed_lookahead of n_frames [S] new rows per slot, with last [S] (nullable), would emit now: rows_out [S] = the
 * E of every slot, *Te_out = their maximum, which sizes logits_out.  NASR_ERR_ARG: an n_frames < 0; NASR_ERR_STATE: a row
 * or `last` for a slot that has had `last` and no reset.  Nothing changes. */
int nasr_stream_lookahead_rows(nasr_handle h, const int32_t* n_frames, const uint8_t* last, int32_t* rows_out, int* Te_out);
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  One feed of finished feature rows: feats
 * [S][Tc][F] (nullable when no slot has a new row), n_frames [S] in [0,Tc], last [S] nullable.  rows_out [S] and *Te_out as
 * nasr_stream_lookahead_rows gives them; logits_out time-major [Te][S][C] (logits_rows >= Te rows of it), rows
 * t >= rows_out[b] of slot b unspecified.  Synchronises when a pass runs; the window then replaces the resident batch as a
 * chunk of nasr_stream_feed does.  After a feed with last[b] the slot waits for nasr_stream_reset.  Refused with nothing
 * changed - NASR_ERR_ARG: an n_frames[b] outside [0,Tc], logits_rows < Te, a null buffer; NASR_ERR_STATE: a row or `last`
 * for a slot that has had `last` and no reset, a session that takes samples, a session without look-ahead. */
int nasr_stream_feed_lookahead(nasr_handle h, const float* feats, const int32_t* n_frames, const uint8_t* last, int Tc,
                               int32_t* rows_out, int* Te_out, float* logits_out, int64_t logits_rows);

/* ---- training and evaluating a bidirectional network as a look-ahead session runs it ---------------
 * (No counterpart in the reference, which trains and decodes whole utterances.)  Latency-controlled training: with chunk
 * length C >= 1 and look-ahead R >= 1 set, EVERY whole-batch pass of the handle - nasr_forward*, nasr_greedy_decode*,
 * nasr_loss*, nasr_loss_and_grads, nasr_compute_grads, nasr_train_step, nasr_ctc_align and nasr_ctc_align_resident - runs,
 * for each utterance of T_b frames on its own, the windows k = 0, 1, ... of rows [kC, min(kC + C + R, T_b)): the first
 * window that reaches the utterance's end is its last and emits all its rows, every earlier one emits its first C.  In
 * every layer the forward direction continues from its state after the last row the window before emitted (zero for
 * window 0), the backward direction starts from zero at the window's last row, and all the window's rows go up to the
 * next layer.  The utterance's logits are the emitted rows in order; projection, CTC loss, decoding and alignment read
 * them as ever.  These are the logits a session of nasr_stream_open_lookahead(h, S, R) returns when it is fed C + R rows,
 * then C rows per feed, then the rest with `last`; with C + R >= T_b it is the whole-utterance network.  Gradients flow
 * through the carried forward state; two runs give the same bits.  The passes run on the per-step kernels whatever
 * nasr_get_recurrence_mode says and leave that mode alone; stream sessions, parameters, Adam state, gradient buckets,
 * clipping and checkpoints are unaffected.  The recurrence's activations take (C + R) / C times the memory.
 * C = 0 (R ignored) turns it off: the default.  A change drops the resident batch (the next *_resident call or
 * nasr_compute_grads needs a new upload), and a batch staged before the change is refused at nasr_commit_batch.
 * NASR_ERR_ARG: C outside [1,4096] (and not 0), R outside [1,1024].  NASR_ERR_STATE, with the reason in nasr_last_error and
 * nothing changed: a unidirectional config (its graph is causal already); NASR_MERGE_STACK_RESHAPE; dense stages (the
 * DeepSpeech family, in this version); a dropout probability > 0; a WaveNet, LAS or featurizer handle; an open stream
 * session.  A batch whose windows need more than 2^22 rows is refused at its upload (NASR_ERR_ARG). */
int nasr_set_chunking(nasr_handle h, int C, int R);
/* *C, *R (either nullable) as set; 0, 0 when off. */
int nasr_get_chunking(nasr_handle h, int* C, int* R);

/* ---- frame skip: low-frame-rate input for the LSTM CTC networks --------------------------------------
 * (No counterpart in the reference: the rule is this project's own.  Its effect on the label error rate is not measured.)
 * With skip s in [1,8] the network sees input frames 0, s, 2s, ... of every utterance: network frame j is input frame j*s,
 * an utterance of len input frames has ceil(len/s) network frames and a batch of T input frames ceil(T/s).  A kept frame's
 * context window is exactly what the input frame's window was (frames before 0 and from len on are the utterance's pad
 * value, SpecAugment-masked frames stay masked); with s <= 2*numcontext+1 no input sample is lost.  Everything behind the
 * input layout - recurrence, dense stages, projection, CTC, greedy decode, alignment, distillation, row compaction,
 * chunked training, stream sessions - sees network frames only.
 * Callers keep passing input T, input seq_len and input features in every upload form, and SpecAugment masks in input
 * frames.  nasr_logit_frames(h, T) returns the logit frames of ceil(T/s) network frames, and every output sized by it is in
 * network frames: logits, greedy ids, alignment paths, step logits.  nasr_resident_shape keeps returning the caller's
 * input B, T and nasr_resident_frames keeps counting input frames; nasr_resident_rows counts network rows.  The CTC
 * feasibility check (NASR_ERR_INFEASIBLE) is made against network frames.  nasr_set_chunking(C, R) and
 * nasr_stream_open_lookahead(S, R) count network frames.
 * In a stream session the caller feeds input rows (or samples): the session keeps, per slot, how many input rows the
 * utterance has had, modulo s, and a feed keeps the new rows whose index in the utterance is a multiple of s.
 * nasr_stream_feed's chunk then has ceil(Tc/s) rows (logits_out [ceil(Tc/s)][S][C]); rows_out, Te_out and
 * nasr_stream_frames report kept rows.  nasr_stream_reset clears a slot's count; nasr_stream_set_state does not carry it.
 * s = 1, the default, is the library without the call, bit for bit.  A change drops the resident batch, and a batch staged
 * before the change is refused at nasr_commit_batch.  NASR_ERR_ARG: s outside [1,8].  NASR_ERR_STATE, nothing changed: a
 * WaveNet or LAS handle with s != 1 (the convolutions need every frame; LAS has its pyramid); an open stream session. */
int nasr_set_frame_skip(nasr_handle h, int s);
/* *s as set; 1 on a WaveNet or LAS handle. */
int nasr_get_frame_skip(nasr_handle h, int* s);

/* The CTC beam search as a state that lives between calls - host only, the procedure and arithmetic of
 * nasr_ctc_beam_search(_lm), which is open + one feed + best + close on this very code: feeding an utterance's frames in
 * any split gives its ids and log-probability bit for bit.  One handle per thread. */
typedef struct nasr_beam* nasr_beam_handle;
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  A search over C classes (blank = C-1)
 * before its first frame.  lm_logp == NULL: the plain search (the remaining LM arguments are not read); else the fused
 * one with the arguments and rules of nasr_ctc_beam_search_lm.  The tables are borrowed: they must outlive the handle.
 * NASR_ERR_ARG: C < 2, beam_width < 1, out == NULL, bad LM arguments. */
int nasr_ctc_beam_open(int C, int beam_width, int merge_repeated, const float* lm_logp, const float* lm_eos, int order,
                       int bos_id, float weight, float bonus, nasr_beam_handle* out);
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  The next n_frames frames: frame t at
 * logits + t * frame_stride (C raw logits each; frame_stride >= C floats, S*C for slot b's column of a [Tc][S][C] array).
 * n_frames = 0 is allowed. */
int nasr_ctc_beam_feed(nasr_beam_handle s, const float* logits, int64_t frame_stride, int n_frames);
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  The top path of the frames fed so far
 * (the empty one before the first), at any time and without disturbing the search: *len_out ids into ids_out [cap],
 * logp_out (may be NULL) as nasr_ctc_beam_search(_lm) reports it.  cap smaller than the hypothesis: NASR_ERR_ARG, with
 * *len_out set and ids_out untouched. */
int nasr_ctc_beam_best(nasr_beam_handle s, int32_t* ids_out, int cap, int32_t* len_out, float* logp_out);
/* (No counterpart in the reference: tfnetwork.py:179-181 decodes whole utterances.)  Frees the search (NULL: nothing). */
int nasr_ctc_beam_close(nasr_beam_handle s);

/* ---- CTC forced alignment (not part of the reference, which has no aligner) ------------
 * For utterance b with F = seq_len[b] logit frames (the frames the CTC loss uses) and its label of length L: the path pi over the
 * S = 2L+1 states of the extended label (blank = C-1 at even states) that starts in {0,1}, ends in {S-1,S-2}, moves by 0, 1 or
 * (onto a non-blank state that differs from the one two below) 2 states per frame and maximises the sum of the RAW logits
 * x(t, l'_pi(t)).  Equal predecessors: stay, then s-1, then s-2; equal end states: S-1.  path_out [B][T'] int32: pi(t) for
 * t < F, -1 from F on; score_out [B] float64: sum_t (x(t, l'_pi(t)) - logZ(t)), the natural-log probability of the path.
 * All on the device (max-plus walk with 2-bit back-pointers and the way back, one wave per utterance); two calls give the
 * same bits.  An infeasible label is NASR_ERR_INFEASIBLE before anything is launched, as for the loss.  LAS handles answer
 * NASR_ERR_STATE; argument errors are NASR_ERR_ARG.  The alignment has workspaces of its own: the resident batch, the
 * parameters, the last loss pass's results and the gradients stay as they were (the calls on a batch run the forward pass,
 * as nasr_forward_resident does).
 * nasr_ctc_align: upload (with labels), forward, align. */
int nasr_ctc_align(nasr_handle h, const float* feats, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len,
                   int B, int T, int Lmax, int32_t* path_out /*[B,T']*/, double* score_out /*[B]*/);
/* The same on the batch that is resident already, by whichever upload (nasr_upload_batch_audio included: an alignment from
 * audio never sees features on the host).  NASR_ERR_STATE without a resident batch with labels.  No counterpart in the
 * reference. */
int nasr_ctc_align_resident(nasr_handle h, int32_t* path_out, double* score_out);
/* The same kernels on the caller's logits (host, time-major [T',B,C], as nasr_forward returns them; seq_len in logit
 * frames), on the handle's device and stream: C is the caller's (>= 2), independent of the handle's model; the resident
 * batch is not touched.  No counterpart in the reference. */
int nasr_ctc_align_logits(nasr_handle h, const float* logits, const int32_t* seq_len, const int32_t* labels,
                          const int32_t* label_len, int B, int Tp, int C, int Lmax, int32_t* path_out, double* score_out);
/* Host only: 1 when a batch whose longest utterance has F frames and whose longest label has L ids keeps its back-pointers
 * in LDS, 0 when they go through the handle's global workspace (a function of F and L alone); < 0 on F < 1 or L outside
 * [0,511].  No counterpart in the reference. */
int nasr_ctc_align_lds(int F, int L);

/* ---- teacher-student distillation beside the CTC loss (not part of the reference) -------------------
 * With student logits z and teacher logits y [T',B,C], weight a, temperature tau, p = softmax(y / tau) and
 * q = softmax(z / tau) over the C classes, and len_b the logit frames of utterance b that the CTC loss uses:
 *   kd_b = sum_{t < len_b, c} p_c (log p_c - log q_c),   KD = tau^2 mean_b kd_b,   loss = (1 - a) CTC + a KD,
 *   dloss/dz[t,b,c] = (1 - a) dCTC/dz[t,b,c] + a tau (q_c - p_c) / B,   exactly 0 where the CTC gradient is 0 by layout
 * (frames t >= len_b, padding utterances, padded class columns).  The term is computed in the loss pass, row-wise in
 * fp32 with max-subtracted log-softmaxes and summed per utterance in fp64 in a fixed order: two runs give the same bits.
 * The loss that nasr_get_loss, nasr_get_step_results, nasr_loss* and nasr_train_step report is then the combined one.
 *
 * nasr_set_distill: weight in [0, 1), temperature in [0.25, 16], both finite, else NASR_ERR_ARG.  weight = 0 is off, the
 * default: every step is bit for bit the step without this section, and nothing of it is launched or allocated.
 * NASR_ERR_STATE with the reason: a LAS or featurizer handle; a NASR_MERGE_STACK_RESHAPE network, whose logit rows are
 * no frames.  With weight > 0 the term takes part in every loss pass for which teacher logits are valid:
 *   - teacher logits belong to the resident batch; any upload, commit or stream feed drops them;
 *   - nasr_compute_grads (and nasr_train_step, nasr_loss_and_grads through it) without them is NASR_ERR_STATE, nothing
 *     changed; nasr_loss_resident and nasr_loss without them return the plain CTC loss.
 * The teacher logits are never written by a step: loss and gradient passes on the same resident batch repeat bit for bit. */
int nasr_set_distill(nasr_handle h, float weight, float temperature);
/* either pointer nullable */
int nasr_get_distill(nasr_handle h, float* weight, float* temperature);
/* Teacher logits for the resident batch from host memory, time-major [T',B,C] as nasr_forward returns them.
 * Synchronises.  NASR_ERR_STATE without a resident batch. */
int nasr_set_teacher_logits(nasr_handle h, const float* logits);
/* The same from device to device, without a host synchronisation: the logits of `teacher`'s last forward pass
 * (nasr_forward*, nasr_greedy_decode*; not a gradient pass, which consumes them) on its own resident batch.  The teacher
 * is any CTC handle (either family, whole-utterance or chunked) on the same device whose resident batch agrees with h's
 * in B, logit frames, C and every seq_len[b]; anything else is NASR_ERR_STATE with the reason, nothing changed.  The two
 * handles may run on different streams: h's stream waits for the teacher's forward pass, and the teacher's stream waits
 * for the copy before it runs anything enqueued later.  The teacher's step fault word travels with the logits and the
 * student's step takes it into its own: a teacher whose persistent recurrence gave up makes the student's step void. */
int nasr_take_teacher_logits(nasr_handle h, nasr_handle teacher);
/* Synchronises.  The two parts of the last loss pass: *ctc the batch-mean CTC loss, *kd = KD above, or 0 when the term
 * took no part; with the term, (1 - a) * ctc + a * kd evaluated in double and rounded to float is the published loss. */
int nasr_get_distill_loss(nasr_handle h, float* ctc, float* kd);
/* The term's kernels on the caller's logits (host, [Tp,B,C] with C the handle's num_classes; seq_len in logit frames,
 * each in [1,Tp]): dlogits_out [Tp,B,C] = a tau (q - p) / B and kd_out [B] = kd_b.  weight in [0, 1).  The handle's
 * resident batch, teacher logits, settings and results stay as they were. */
int nasr_distill_logits(nasr_handle h, const float* student, const float* teacher, const int32_t* seq_len, int B, int Tp,
                        float weight, float temperature, float* dlogits_out, double* kd_out);

/* create_metric (networks/tfnetwork.py:66-70): mean over the batch of Levenshtein(hyp, truth)/len(truth)
 * (tf.edit_distance normalize=True, Appendix A.7).  Host code, no GPU work.  hyp_ids [B,hyp_stride],
 * labels [B,Lmax].  An empty truth gives inf for a non-empty hypothesis and 0 otherwise, as TF does. */
int nasr_label_error_rate(const int32_t* hyp_ids, const int32_t* hyp_lens, int hyp_stride, const int32_t* labels,
                          const int32_t* label_len, int Lmax, int B, float* ler_out);

/* tf.nn.dropout of the dense stages (networks/deepspeech.py:50,59,68,113; applied in every graph, training or not).
 * TensorFlow's random stream is not reproducible, so the keep-mask of forward pass number `counter` is a pure function
 * of (seed, counter, stage, frame, utterance, unit): see neuralasr_amd/csrc/dense.hip.  Every forward pass uses the
 * current counter and then increments it; nasr_set_dropout_state pins both (tests, resuming). */
int nasr_set_dropout_state(nasr_handle h, uint32_t seed, uint32_t counter);
int nasr_get_dropout_state(nasr_handle h, uint32_t* seed, uint32_t* counter);

/* ---- measurement ------------------------------------------------------------------------ */
int nasr_set_profiling(nasr_handle h, int enabled); /* record HIP events around the phases */
int nasr_get_phase_times(nasr_handle h, nasr_phase_times* out); /* synchronises */
int nasr_set_graph_mode(nasr_handle h, int enabled); /* capture the per-timestep loops in hipGraphs */
/* How the recurrence of tf.nn.(bidirectional_)dynamic_rnn (networks/bilstm_ctc_net.py:24-28,
 * networks/lstm_ctc_net.py:22-23) runs: 1 = one persistent launch per layer pass (one XCD per direction and
 * utterance slice, recurrent matrix resident in registers), 2 = a layer of 2048 cells (networks/deepspeech.py:70-103):
 * one persistent launch per DIRECTION and pass (the matrix resident in the registers of all 256 CUs as fp16 planes),
 * 0 = one launch per timestep.  nasr_set_recurrence_mode(0)
 * forces the per-step kernels; (1) asks for the persistent ones again and returns NASR_ERR_STATE where the device or
 * the hidden size does not support them.  A persistent launch wants every CU of the device for itself: if another
 * process or handle keeps CUs busy for longer than its bounded spins (~0.5 s), the launch gives up, the step is void
 * (nasr_step_void) and this handle continues on the per-step kernels. */
int nasr_get_recurrence_mode(nasr_handle h);
int nasr_set_recurrence_mode(nasr_handle h, int persistent);
/* After an abort the handle serves NASR_PERSIST_REARM (default 200; 0 = never) clean steps on the per-step kernels,
 * then repeats the placement census of nasr_create at the start of a step and returns to the persistent kernels if it
 * passes; every further abort doubles the wait.  aborts / rearms: how often each has happened on this handle (a rank
 * that sits on the per-step kernels slows every rank of a data-parallel job: bench.py reports these per rank). */
int nasr_get_persist_stats(nasr_handle h, int* aborts, int* rearms);

/* ---- the WaveNet CTC network (networks/wavenet.py) ------------------------------------------
 * front/conv_in (1x1 conv F->dim, batch norm, tanh); num_blocks x num_rates residual blocks of a gated dilated
 * convolution (kernel_size taps at rates[r], filter tanh(BN) times gate sigmoid(BN)), a 1x1 conv with BN and tanh, the
 * residual sum and the skip sum; logit/conv_1 (1x1, BN, tanh) over the skip sum; logit/conv_2 (1x1 to the classes, no BN).
 * Every convolution is bias-free.  The reference has num_blocks 3, rates (1,2,4,8,16), dim 128, kernel_size 7: only
 * dim 128 and kernel_size 7 are implemented.  Batch norm is tf.contrib.layers.batch_norm(decay, epsilon, center, scale,
 * zero_debias_moving_mean): gradient passes (nasr_compute_grads, nasr_loss_and_grads, nasr_train_step) normalise with the
 * batch statistics over all T x B frames (padding frames past seq_len included) and update the moving statistics;
 * nasr_forward, nasr_loss and the decoders use the moving statistics.  Flat parameter order = TF variable creation order:
 * front/conv_in/W [F,dim], .../BatchNorm/beta, gamma; per block block_<i>_<r>/conv_filterblock_<i>_<r>/W [k*dim,dim] (row
 * tap*dim + in channel), beta, gamma, conv_gate... likewise, conv_out... [dim,dim], beta, gamma; logit/conv_1/W, beta,
 * gamma; logit/conv_2/W [dim,C].  nasr_create_wavenet returns an ordinary handle: every call above that is not about the
 * recurrence works on it; nasr_*_recurrence_mode, nasr_set_wgrad_overlap, nasr_set_row_compaction and
 * nasr_*_dropout_state return NASR_ERR_STATE. */
typedef struct {
  int32_t feature_size;  /* F */
  int32_t num_classes;   /* C; blank = C-1 */
  int32_t dim;           /* 128 */
  int32_t kernel_size;   /* 7 */
  int32_t num_blocks;    /* 3 */
  int32_t num_rates;     /* 5 (<= 8) */
  int32_t rates[8];      /* 1, 2, 4, 8, 16 */
  float bn_epsilon;      /* 1e-3 (contrib batch_norm's default) */
  float bn_decay;        /* 0.99 */
  float learning_rate;
  float beta1, beta2, epsilon; /* Adam: 0.9, 0.999, 1e-8 */
} nasr_wavenet_cfg;
int nasr_create_wavenet(const nasr_wavenet_cfg* cfg, int device_id, void* stream, nasr_handle* out);
/* Batch-norm state: S = 2 + 3*num_blocks*num_rates sites in variable creation order (conv_in; per block filter, gate,
 * conv_out; conv_1), dim channels each: nasr_wavenet_bn_count = S*dim floats per array.  moving_mean, moving_variance, the
 * zero-debias accumulator `biased` and the update count (TF's local_step) - what a checkpoint carries besides the
 * trainable variables. */
int64_t nasr_wavenet_bn_count(nasr_handle h);
int nasr_wavenet_get_bn_state(nasr_handle h, float* moving_mean, float* moving_var, float* biased, int64_t n,
                              int64_t* updates);
int nasr_wavenet_set_bn_state(nasr_handle h, const float* moving_mean, const float* moving_var, const float* biased,
                              int64_t n, int64_t updates);
/* Data parallelism (make_parallel: every tower applies its own update).  hold = 1: gradient passes leave the moving
 * statistics alone; nasr_wavenet_get_batch_stats returns the last gradient pass's per-site batch mean and the variance its
 * update would use (N/(N-1) x the batch variance at the 1x1 sites, the batch variance at the dilated ones), [S][dim];
 * nasr_wavenet_apply_bn_stats applies `count` such updates in order ([count][S][dim] each). */
int nasr_wavenet_set_bn_hold(nasr_handle h, int hold);
int nasr_wavenet_get_batch_stats(nasr_handle h, float* mean, float* var, int64_t n);
int nasr_wavenet_apply_bn_stats(nasr_handle h, const float* mean, const float* var, int64_t n, int count);

/* ---- the LAS network (networks/las.py: Listen, Attend and Spell) ------------------------------
 * A 4-layer pyramidal BiLSTM encoder (250 units per direction; an odd length gets one zero frame, both directions run over
 * every padded frame whatever seq_len says, frame pairs are concatenated between layers) and an attention decoder
 * (BasicLSTMCell(500) in an AttentionWrapper: Bahdanau attention with 500 units over the top layer's output, no memory mask,
 * attention layer 250, projection to the classes).  Training decodes U = Lmax steps; step t is fed labels[:, t] (the
 * reference's literal input, not labels[:, t-1]) and, from step 1 on, with probability p a sample from softmax(logits_{t-1})
 * (ScheduledEmbeddingTrainingHelper).  The loss is sequence_loss: sum of w*CE / (sum w + 1e-12), w = t < label_len[b].
 * Labels are dense [B][Lmax] ids in [0, num_classes-1]; every entry, padding included, must be a valid id (it is fed).
 * The common calls work on the handle: parameters (TF variable order, nasr_tensor_info), Adam, batches, nasr_compute_grads,
 * nasr_loss (nll_out: per-utterance sum of w*CE), nasr_loss_and_grads, nasr_train_step, gradient buffer and buckets, the
 * fault word, step tokens, nasr_comm_*.  The CTC-only calls (nasr_forward, nasr_greedy_decode, nasr_set_step_decode with
 * a greedy pass, nasr_logit_frames) return NASR_ERR_STATE.
 * Variables: per layer l = 0..3: bidirectional_rnn/fw/fw_l/kernel [I+250, 1000] (I = F for l = 0, else 1000), .../bias,
 * bidirectional_rnn/bw/bw_l/kernel, .../bias; memory_layer/kernel [500,500]; decoder_lstm/kernel [C+250+500, 2000] (rows:
 * one-hot input, previous attention, h), decoder_lstm/bias; query_layer/kernel [500,500]; attention_v [500];
 * attention_layer/kernel [1000,250] (rows: h, context); projection_layer/kernel [250,C], projection_layer/bias [C].
 * Scheduled sampling is defined by a counter-based hash (neuralasr_amd/csrc/las.hip, first comment): every sampling pass
 * (nasr_compute_grads, nasr_loss, nasr_las_forward[_resident] with sample = 1) uses the current counter and then increments it. */
typedef struct {
  int32_t feature_size;
  int32_t num_classes;
  int32_t num_hidden;          /* 250 (the reference's) */
  int32_t num_layers;          /* 4 */
  float sampling_probability;  /* 0.1 */
  uint32_t seed;               /* of the sampling hash */
  float learning_rate;
  float beta1, beta2, epsilon;
} nasr_las_cfg;
int nasr_create_las(const nasr_las_cfg* cfg, int device_id, void* stream, nasr_handle* out);
/* sampling probability, hash seed, pass counter and tower index (a checkpoint carries them; towers key their own draws) */
int nasr_las_set_sampling(nasr_handle h, float p, uint32_t seed, uint32_t counter, int tower);
int nasr_las_get_sampling(nasr_handle h, float* p, uint32_t* seed, uint32_t* counter, int* tower);
/* a forward pass of the decoder over labels [B][U] (sample = 0: every step fed its label; 1: scheduled sampling), its
 * logits [B][U][C] (or NULL); the loss is left for nasr_get_loss */
int nasr_las_forward(nasr_handle h, const float* feats, const int32_t* seq_len, const int32_t* labels, const int32_t* label_len,
                     int B, int T, int U, int sample, float* logits_out);
/* (networks/las.py:120-122,133-138: the training graph's sess.run, fed by utils.py:24-31) nasr_las_forward without its
 * upload: the decoder pass over the batch that is resident already, uploaded by any route (nasr_upload_batch,
 * nasr_upload_batch_context, nasr_upload_batch_audio, nasr_commit_batch), with the labels in it.  The sampling state and
 * nasr_las_get_logits / get_fed_ids / get_sampled behave as after nasr_las_forward.  NASR_ERR_STATE: not a LAS handle,
 * or no resident batch; NASR_ERR_ARG: the resident batch has no labels. */
int nasr_las_forward_resident(nasr_handle h, int sample, float* logits_out);
/* of the last decoder pass: logits [B][U][C], the ids fed to each step [B][U] */
int nasr_las_get_logits(nasr_handle h, float* logits_out);
int nasr_las_get_fed_ids(nasr_handle h, int32_t* ids_out);
/* of the last decoder pass: 1 where the step's input was a scheduled sample, else 0 [B][U] (step 0 is never sampled) */
int nasr_las_get_sampled(nasr_handle h, int32_t* sampled_out);
/* Beam-search decoding (the reference's inference graph: BeamSearchDecoder of TF 1.15 with length penalty, then
 * gather_tree).  The encoder runs over feats [B][T][F] (B in [1,64], seq_len in [1,T]); every utterance's memory and final
 * (c, h) are tiled to beam_width beams (in [1,1024]); beam 0 starts with log-prob 0 and beams 1.. start finished with
 * -inf; every step feeds the chosen ids (start_id first).  A step scores total / ((5 + len)^p / 6^p) and keeps the exact
 * top beam_width of each utterance's beam_width * C candidates (score descending, equal scores by index beam*C + id
 * ascending).  The search stops after the step at which every beam is finished (or after max_steps, in [1,1000]);
 * *steps_out = T_dec, the steps run.  start_id / end_id in [0, num_classes-1], length_penalty finite and >= 0.
 * A search has buffers of its own: it does not replace the uploaded batch and leaves the parameters, the Adam state, the
 * gradient buffer, the sampling state and the last decoder pass's loss, logits and ids as they were (it is not a sampling
 * pass).  With nasr_set_profiling on, the search records its device-timed phases (nasr_las_beam_get_times). */
int nasr_las_beam_search(nasr_handle h, const float* feats, const int32_t* seq_len, int B, int T, int beam_width, int max_steps,
                         int start_id, int end_id, float length_penalty, int32_t* steps_out);
/* (networks/las.py:77-104,124-131: the inference graph's beam decoder and its sess.run, fed by utils.py:24-31)
 * nasr_las_beam_search with the encoder fed from the resident batch's time-major features, where nasr_upload_batch* or
 * nasr_commit_batch put them: B, T and seq_len are the resident batch's, no feature is copied from the host and nothing is
 * packed again.  The search only reads the resident batch: a nasr_compute_grads after it gives the gradients it would have
 * given without it.  The argument ranges and nasr_las_beam_get_* are those of nasr_las_beam_search.  NASR_ERR_STATE: not a
 * LAS handle, or no resident batch. */
int nasr_las_beam_search_resident(nasr_handle h, int beam_width, int max_steps, int start_id, int end_id, float length_penalty,
                                  int32_t* steps_out);
/* of the last search: the gathered ids (gather_tree) [B][T_dec][W] */
int nasr_las_beam_get_ids(nasr_handle h, int32_t* ids_out);
/* of the last search, any output may be NULL: every step's top-W scores, chosen word ids and parent beams [B][T_dec][W] */
int nasr_las_beam_get_trace(nasr_handle h, float* scores_out, int32_t* word_out, int32_t* parent_out);
/* of the last search, any output may be NULL: the final log-probs, lengths and finished flags (0 / 1) [B][W] */
int nasr_las_beam_get_final(nasr_handle h, float* log_probs_out, int32_t* lengths_out, int32_t* finished_out);
/* n-gram fusion inside the search (not part of the reference).  logp [K][C] float32, C = the handle's
 * num_classes, K = C^(order-1), order in [1,4], K*C <= 2^24, weight and every entry finite (checked: NASR_ERR_ARG, and
 * the table set before stays): copied to the device once, owned by the handle
 * and used by every later nasr_las_beam_search / _resident.  Every beam row carries the context of its hypothesis (the last
 * order-1 ids, the most recent as the lowest digit in base C, start_id in every digit at the start); an unfinished row's
 * step log-probs become ((l - max) - lse) + (weight * logp[ctx][w]) in float32, product and sum rounded separately; a
 * finished row's are unchanged; a row's next context is its parent's when the parent was finished, else
 * (ctx[parent]*C + word) mod K.  The end marker is an ordinary class of the table.  logp == NULL removes the table: the
 * search is then bit for bit the plain one.  NASR_ERR_STATE: not a LAS handle. */
int nasr_las_beam_set_lm(nasr_handle h, const float* logp, int order, float weight);
/* of the last search: the final context index of every beam [B][W] (all 0 when no table was set) */
int nasr_las_beam_get_lm_context(nasr_handle h, int32_t* ctx_out);
/* of the last search when it ran with profiling on (else NASR_ERR_STATE): device-timed ms of 7 phases: encoder (with the
 * feature copy, keys and initial state), decoder GEMMs, decoder cell, attention, selection (scores, top-W, update),
 * gather_tree, and the host's waits between chunks of steps */
int nasr_las_beam_get_times(nasr_handle h, float* ms_out);

/* ---- the feature front end (utils.py:24-31: convert_to_mfcc) ------------------------------------
 * python_speech_features 0.6's mfcc(audio, samplerate, numcep=numcep, nfilt=128) on float32 audio: pre-emphasis in
 * float32 (two roundings), frames of round_half_up(winlen*sr) samples every round_half_up(winstep*sr), zero-padded tail,
 * rectangular window, then in float64 |rfft(frame, nfft)|^2 / nfft (frames longer than nfft truncated), frame energy, the triangular mel
 * filterbank over [0, sr/2], log (exact zeros -> float64 eps), DCT-II (ortho), the lifter, c0 <- log(energy); then
 * include_context (utils.py:8-21) and the whole-utterance (X - mean(X)) / std(X) of utils.py:29, in float64.
 * kind = 1 stops after the log: psf 0.6's logfbank(audio, samplerate, nfilt=numcep), the log filterbank energies
 * themselves (no DCT, no lifter, no energy column).
 * deltas = 1 or 2 appends psf 0.6's delta(feat, N=2) of the static columns, and for 2 also delta(delta(feat, 2), 2):
 * delta[t] = ((p[t+1] - p[t-1]) + 2 (p[t+2] - p[t-2])) / 10 in float64, p the array edge-replicated by 2 frames inside
 * its own utterance; the second level replicates the edges of the delta array (it does not look at deltas that the
 * first level would have beyond the edge).  A frame is then D = numcep * (1 + deltas) wide, [static | delta |
 * delta-delta], and include_context and the normalisation work on D-wide frames (one mean and one std over the stacked
 * matrix, zero pads included).  Both restate psf's documented procedure; neither is pinned against the package, nor is
 * the summation order against numpy.dot's inside psf's delta.
 * norm = 1 (no counterpart in the reference) replaces the whole-utterance normalisation by a causal rule
 * that can be computed while the audio arrives.  x[u] is un-normalised frame u of an utterance of T frames (D columns),
 * M = norm_min_frames.  In float64, without fused multiply-adds: p1[u] = sum_k x[u][k] and p2[u] = sum_k x[u][k]^2 with
 * the columns in ascending order; S1[n] = S1[n-1] + p1[n-1] and likewise S2, S[0] = 0, strictly in frame order (no
 * parallel scan: a chunked and a whole-utterance run must agree bit for bit).  Frame u is normalised once, with the first
 * n_u = min(T, max(u+1, M)) frames: N = n_u D, mean = S1[n_u] / N, var = S2[n_u] / N - mean mean, sd = sqrt(var) if
 * var > 0, else 1 (digital silence must not put NaNs into a carried LSTM state), y[u][k] = (float)((x[u][k] - mean) / sd).
 * Every frame counts once.  Row t of the output is y[t-numcontext .. t+numcontext], an out-of-utterance context frame is
 * exact 0.0f (the running mean), so the pad value of every utterance in the batch-slot form is 0.  mean_std reports
 * (mean, sd) at n = T.  norm = 1 with deltas > 0 is refused: psf's delta looks 2 (or 4) frames ahead and replicates the end of
 * the array, which needs a look-ahead rule of its own.  A zeroed norm / norm_min_frames is the whole-utterance rule.
 * nasr_create_featurizer returns an ordinary handle: nasr_last_error, nasr_synchronize and nasr_destroy work on it and
 * every model call returns NASR_ERR_STATE.  Only nfft = 512 (psf 0.6's default) is implemented; 1 <= nfilt <= 128. */
typedef struct {
  int32_t samplerate, numcep, numcontext; /* config.samplerate, numcep, numcontext; 1 <= numcep <= nfilt */
  int32_t nfilt, nfft;                    /* 128, 512 (utils.py:26) */
  double winlen, winstep;                 /* 0.025, 0.01 s */
  float preemph;                          /* 0.97 */
  int32_t ceplifter, append_energy;       /* 22, 1 */
  int32_t kind;                           /* 0: MFCC; 1: log-mel filterbank, numcep filters: numcep must equal nfilt,
                                             ceplifter and append_energy are ignored */
  int32_t deltas;                         /* 0, 1 (+ delta) or 2 (+ delta and delta-delta) */
  int32_t norm;                           /* 0: whole-utterance normalisation (utils.py:29); 1: the causal rule above */
  int32_t norm_min_frames;                /* M of the causal rule, in [1,1000]; read only when norm = 1 */
} nasr_mfcc_cfg;
int nasr_create_featurizer(const nasr_mfcc_cfg* cfg, int device_id, void* stream, nasr_handle* out);
/* Host only (no device needed): the frame count of an utterance of num_samples >= 1 samples (psf framesig: 1 if
 * num_samples <= frame_len, else 1 + ceil((num_samples - frame_len) / frame_step)); < 0 on a bad cfg or length. */
int64_t nasr_mfcc_frames(const nasr_mfcc_cfg* cfg, int64_t num_samples);
/* Host only: the width D = numcep * (1 + deltas) of one un-stacked frame; < 0 on a bad cfg. */
int nasr_mfcc_width(const nasr_mfcc_cfg* cfg);
/* Host only: the filterbank the kernels use (psf get_filterbanks), bin edges [nfilt+2] and weights [nfilt][nfft/2+1]
 * (float32 copies of the kernels' float64 table); either may be NULL. */
int nasr_mfcc_filterbank(const nasr_mfcc_cfg* cfg, int32_t* bins, float* weights);
/* The features of n utterances: utterance i is audio[offsets[i] .. offsets[i+1]) (float32, at least one sample each).
 * out [out_rows][(2*numcontext+1)*D] (D = nasr_mfcc_width) receives the utterances' normalised rows one after another; out_rows must be
 * the sum of their nasr_mfcc_frames.  mean_std (nullable) [n][2]: each utterance's mean and std (ddof 0) over its
 * stacked matrix, zero pads included.  Returns when out is written (utils.py:24-31 for every utterance). */
int nasr_featurize(nasr_handle h, const float* audio, const int64_t* offsets, int n, float* out, int64_t out_rows,
                   double* mean_std);
/* The last nasr_featurize's, nasr_featurize_rates', nasr_resample's or nasr_augment_audio's device-timed phases: host-to-device copies,
 * kernels (the resampling kernel included), device-to-host copies (ms). */
int nasr_featurize_times(nasr_handle h, float* h2d_ms, float* kernel_ms, float* d2h_ms);

/* ---- resampling to the config rate (utils.py:25: librosa.load(wavfile, mono=True, sr=sr)) -------
 * librosa 0.6-0.9's resample(y, rate, sr, res_type='kaiser_best'): resampy 0.2 then fix_length.  ratio = sr / rate
 * in float64; resampy makes int(n * ratio) samples (none: it raises) by band-limited sinc interpolation (64 zero
 * crossings, 512 table entries per crossing, Kaiser window, the table scaled by ratio when ratio < 1) on its
 * sequential float64 time register, summing each output in float32 after every tap; librosa zero-pads them to
 * ceil(n * ratio).  An utterance already at sr is left as it is. */
/* Host only (utils.py:25): resampy's kaiser_best half window, float64 [len], len = 32769. */
int nasr_resample_filter(double* table, int64_t len);
/* Host only (utils.py:25): librosa's length ceil(n * ratio) of n >= 1 samples at in_rate resampled to out_rate, and
 * resampy's filtered length int(n * ratio) in *filtered (nullable); < 0 on a rate <= 0, n < 1, or when resampy would
 * raise (int(n * ratio) < 1). */
int64_t nasr_resample_length(int32_t in_rate, int32_t out_rate, int64_t n, int64_t* filtered);
/* (utils.py:25) Utterance i, audio[offsets[i] .. offsets[i+1]) at rates[i] Hz, resampled to the featurizer's
 * samplerate; out [out_len] receives the utterances' nasr_resample_length samples one after another.  NASR_ERR_ARG,
 * naming the utterance, on a rate <= 0 or an utterance too short; NASR_ERR_STATE on a model handle. */
int nasr_resample(nasr_handle h, const float* audio, const int64_t* offsets, const int32_t* rates, int n, float* out,
                  int64_t out_len);
/* (utils.py:24-31 after utils.py:25's resampling) nasr_featurize of the utterances resampled as nasr_resample does,
 * on the device: the resampled samples never leave it.  out_rows is the sum of the nasr_mfcc_frames of their
 * resampled lengths.  Utterances at the samplerate give bitwise what nasr_featurize gives them. */
int nasr_featurize_rates(nasr_handle h, const float* audio, const int64_t* offsets, const int32_t* rates, int n,
                         float* out, int64_t out_rows, double* mean_std);

/* ---- waveform augmentation banks (the rules are at nasr_wave_aug) -----------------
 * (No counterpart in the reference: its only augmentation is rand_shift, dataset.py:23-31.)  The featurizer's noise
 * bank: clip i is samples[offsets[i] .. offsets[i+1]) (float32, at the featurizer's samplerate), offsets [n_clips+1]
 * ascending from offsets[0] >= 0.  Uploaded once; it lives on the handle until it is replaced or the handle is destroyed.
 * n_clips = 0 (samples and offsets may be NULL) frees the bank.  Replacing it waits for the batch-slot call that may
 * still read the old one.  NASR_ERR_ARG, naming the clip: an empty clip, a non-finite sample; NASR_ERR_STATE on a model
 * handle. */
int nasr_featurizer_set_noise(nasr_handle fz, const float* samples, const int64_t* offsets, int n_clips);
/* (No counterpart in the reference.)  The featurizer's bank of room impulse responses, in the same form: RIR i is
 * taps[offsets[i] .. offsets[i+1]), 1 to NASR_AUG_MAX_RIR_TAPS taps, used as they are (augment.prepare_rir makes the
 * direct path tap 0 and the energy 1).  n_rirs = 0 frees the bank.  NASR_ERR_ARG, naming the RIR: no tap, more than
 * NASR_AUG_MAX_RIR_TAPS, a non-finite tap; NASR_ERR_STATE on a model handle. */
int nasr_featurizer_set_rirs(nasr_handle fz, const float* taps, const int64_t* offsets, int n_rirs);
/* (No counterpart in the reference.)  nasr_resample followed by the waveform augmentation `wave` (nullable): the
 * resampler and the three kernels that nasr_upload_batch_audio_wave runs, and the waveform z comes back: out [out_len],
 * out_len the sum of the utterances' nasr_resample_length.  rates == NULL: every utterance is at the samplerate.
 * nasr_featurize_times covers it (kernels: the resampler and the augmentation).  The refusals of nasr_resample and of
 * nasr_upload_batch_audio_wave. */
int nasr_augment_audio(nasr_handle fz, const float* audio, const int64_t* offsets, const int32_t* rates, int n,
                       const nasr_wave_aug* wave, float* out, int64_t out_len);

#ifdef __cplusplus
}
#endif
#endif /* NASR_H */
