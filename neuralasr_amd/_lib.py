"""ctypes binding of libnasr.so (include/nasr.h).  There is no CPU fallback: if the HIP library is
missing or no gfx950 device is usable, everything here raises."""
import ctypes
import os
from ctypes import POINTER, Structure, byref, c_char, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint8, c_uint32, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libnasr.so')

NASR_OK = 0
NASR_ERR_ARG = -1
NASR_ERR_HIP = -2
NASR_ERR_INFEASIBLE = -3
NASR_ERR_STATE = -4

MERGE_NONE, MERGE_STACK_RESHAPE, MERGE_CONCAT = 0, 1, 2
MERGE_BY_NAME = {'none': MERGE_NONE, 'stack_reshape': MERGE_STACK_RESHAPE, 'concat': MERGE_CONCAT}

# every symbol include/nasr.h declares (tests/test_abi.py checks the .so exports exactly these)
SYMBOLS = [
    'nasr_create', 'nasr_destroy', 'nasr_last_error', 'nasr_backend', 'nasr_synchronize', 'nasr_param_count',
    'nasr_num_tensors', 'nasr_tensor_info', 'nasr_set_params', 'nasr_get_params', 'nasr_set_adam_state',
    'nasr_get_adam_state', 'nasr_set_learning_rate', 'nasr_train_step', 'nasr_forward', 'nasr_logit_frames',
    'nasr_loss', 'nasr_loss_and_grads', 'nasr_greedy_decode', 'nasr_upload_batch', 'nasr_compute_grads',
    'nasr_grad_device_ptr', 'nasr_grad_device_count', 'nasr_grad_bucket_count', 'nasr_grad_bucket',
    'nasr_grad_bucket_wait', 'nasr_apply_adam', 'nasr_get_grads', 'nasr_set_grads',
    'nasr_upload_batch_context', 'nasr_label_error_rate', 'nasr_set_step_decode', 'nasr_get_decoded', 'nasr_ctc_beam_search', 'nasr_ctc_beam_search_lm', 'nasr_get_loss', 'nasr_resident_frames',
    'nasr_set_profiling', 'nasr_get_phase_times', 'nasr_set_graph_mode',
    'nasr_get_recurrence_mode', 'nasr_set_recurrence_mode', 'nasr_set_dropout_state', 'nasr_get_dropout_state',
    'nasr_step_void', 'nasr_get_persist_stats', 'nasr_stage_batch', 'nasr_stage_batch_context', 'nasr_commit_batch',
    'nasr_discard_batch', 'nasr_set_bucket_defer', 'nasr_comm_unique_id', 'nasr_comm_init', 'nasr_comm_size',
    'nasr_comm_allreduce_grads', 'nasr_comm_mean', 'nasr_comm_destroy', 'nasr_get_step_results', 'nasr_settle_step',
    'nasr_step_token', 'nasr_settle_token', 'nasr_diag_bucket_traffic', 'nasr_get_step_logits',
    'nasr_set_wgrad_overlap', 'nasr_get_wgrad_overlap', 'nasr_set_row_compaction', 'nasr_resident_rows',
    'nasr_create_wavenet', 'nasr_wavenet_bn_count', 'nasr_wavenet_get_bn_state', 'nasr_wavenet_set_bn_state',
    'nasr_wavenet_set_bn_hold', 'nasr_wavenet_get_batch_stats', 'nasr_wavenet_apply_bn_stats',
    'nasr_create_las', 'nasr_las_set_sampling', 'nasr_las_get_sampling', 'nasr_las_forward', 'nasr_las_get_logits',
    'nasr_las_get_fed_ids', 'nasr_las_get_sampled', 'nasr_las_beam_search', 'nasr_las_beam_get_ids',
    'nasr_las_beam_get_trace', 'nasr_las_beam_get_final', 'nasr_las_beam_get_times', 'nasr_las_forward_resident',
    'nasr_las_beam_search_resident', 'nasr_las_beam_set_lm', 'nasr_las_beam_get_lm_context',
    'nasr_create_featurizer', 'nasr_mfcc_frames', 'nasr_mfcc_width', 'nasr_mfcc_filterbank', 'nasr_featurize', 'nasr_featurize_times',
    'nasr_resample_filter', 'nasr_resample_length', 'nasr_resample', 'nasr_featurize_rates',
    'nasr_upload_batch_audio', 'nasr_stage_batch_audio', 'nasr_forward_resident', 'nasr_loss_resident',
    'nasr_greedy_decode_resident',
    'nasr_upload_batch_context_aug', 'nasr_upload_batch_audio_aug', 'nasr_stage_batch_audio_aug',
    'nasr_ctc_align', 'nasr_ctc_align_resident', 'nasr_ctc_align_logits', 'nasr_ctc_align_lds', 'nasr_resident_shape',
    'nasr_set_grad_clip', 'nasr_get_grad_clip', 'nasr_get_grad_clip_stats',
    'nasr_stream_open', 'nasr_stream_close', 'nasr_stream_reset', 'nasr_stream_feed', 'nasr_stream_frames',
    'nasr_stream_get_state', 'nasr_stream_set_state',
    'nasr_stream_attach_audio', 'nasr_stream_audio_rows', 'nasr_stream_feed_audio',
    'nasr_stream_open_lookahead', 'nasr_stream_lookahead_rows', 'nasr_stream_feed_lookahead',
    'nasr_ctc_beam_open', 'nasr_ctc_beam_feed', 'nasr_ctc_beam_best', 'nasr_ctc_beam_close',
    'nasr_featurizer_set_noise', 'nasr_featurizer_set_rirs', 'nasr_upload_batch_audio_wave', 'nasr_stage_batch_audio_wave',
    'nasr_augment_audio',
    'nasr_set_chunking', 'nasr_get_chunking', 'nasr_set_frame_skip', 'nasr_get_frame_skip',
    'nasr_set_distill', 'nasr_get_distill', 'nasr_set_teacher_logits', 'nasr_take_teacher_logits', 'nasr_get_distill_loss',
    'nasr_distill_logits',
    'nasr_get_learning_rate', 'nasr_set_ema', 'nasr_get_ema', 'nasr_get_ema_state', 'nasr_set_ema_state', 'nasr_ema_swap',
]


class ModelCfg(Structure):
    _fields_ = [('feature_size', c_int32), ('hidden', c_int32), ('num_layers', c_int32), ('bidirectional', c_int32),
                ('merge', c_int32), ('num_classes', c_int32), ('forget_bias', c_float), ('learning_rate', c_float),
                ('beta1', c_float), ('beta2', c_float), ('epsilon', c_float),
                ('num_pre', c_int32), ('pre_width', c_int32 * 3), ('post_width', c_int32), ('relu_clip', c_float),
                ('dropout', c_float * 4)]


class WaveNetCfg(Structure):
    _fields_ = [('feature_size', c_int32), ('num_classes', c_int32), ('dim', c_int32), ('kernel_size', c_int32),
                ('num_blocks', c_int32), ('num_rates', c_int32), ('rates', c_int32 * 8), ('bn_epsilon', c_float),
                ('bn_decay', c_float), ('learning_rate', c_float), ('beta1', c_float), ('beta2', c_float),
                ('epsilon', c_float)]


class LasCfg(Structure):
    _fields_ = [('feature_size', c_int32), ('num_classes', c_int32), ('num_hidden', c_int32), ('num_layers', c_int32),
                ('sampling_probability', c_float), ('seed', c_uint32), ('learning_rate', c_float), ('beta1', c_float),
                ('beta2', c_float), ('epsilon', c_float)]


class MfccCfg(Structure):
    _fields_ = [('samplerate', c_int32), ('numcep', c_int32), ('numcontext', c_int32), ('nfilt', c_int32),
                ('nfft', c_int32), ('winlen', c_double), ('winstep', c_double), ('preemph', c_float),
                ('ceplifter', c_int32), ('append_energy', c_int32), ('kind', c_int32), ('deltas', c_int32),
                ('norm', c_int32), ('norm_min_frames', c_int32)]


AUG_MAX_MASKS = 8      # NASR_AUG_MAX_MASKS


class BatchAug(Structure):
    _fields_ = [('static_width', c_int32), ('n_time', c_int32), ('n_freq', c_int32),
                ('time_mask', POINTER(c_int32)), ('freq_mask', POINTER(c_int32))]


AUG_MAX_RIR_TAPS = 8192      # NASR_AUG_MAX_RIR_TAPS


class WaveAug(Structure):
    _fields_ = [('rir', POINTER(c_int32)), ('noise', POINTER(c_int32)), ('noise_off', POINTER(c_int64)),
                ('snr_db', POINTER(c_float))]


class PhaseTimes(Structure):
    _fields_ = [('pack_ms', c_float), ('xproj_ms', c_float), ('rec_fwd_ms', c_float), ('proj_ctc_ms', c_float),
                ('proj_bwd_ms', c_float), ('rec_bwd_ms', c_float), ('wgrad_ms', c_float), ('adam_ms', c_float),
                ('total_ms', c_float), ('rec_fwd_launches', c_int32), ('rec_bwd_launches', c_int32)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class ClipStats(Structure):
    _fields_ = [('last_norm', c_double), ('window_max_norm', c_double), ('last_coef', c_float), ('steps', c_int64),
                ('clipped', c_int64), ('skipped', c_int64)]

    def as_dict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class NasrError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f'libnasr error {code}: {msg}')
        self.code = code


class InfeasibleLabelError(NasrError, ValueError):
    """CTC: "Not enough time for target transition sequence" (TF raises InvalidArgumentError)."""


_lib = None


def load():
    """dlopen libnasr.so, building it first if the sources are newer (dev container).  Raises if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f'{LIB_PATH} is missing: run `python -m neuralasr_amd.build` (hipcc, gfx950). '
                          'neuralasr_amd has no CPU fallback.')
    lib = ctypes.CDLL(LIB_PATH)
    fp, ip = POINTER(c_float), POINTER(c_int32)
    H = c_void_p
    sig = {
        'nasr_create': (c_int, [POINTER(ModelCfg), c_int, c_void_p, POINTER(H)]),
        'nasr_destroy': (c_int, [H]),
        'nasr_last_error': (c_char_p, [H]),
        'nasr_backend': (c_char_p, [H]),
        'nasr_synchronize': (c_int, [H]),
        'nasr_param_count': (c_int64, [H]),
        'nasr_num_tensors': (c_int, [H]),
        'nasr_tensor_info': (c_int, [H, c_int, POINTER(c_char * 64), POINTER(c_int64), POINTER(c_int64), POINTER(c_int64)]),
        'nasr_set_params': (c_int, [H, fp, c_int64]),
        'nasr_get_params': (c_int, [H, fp, c_int64]),
        'nasr_set_adam_state': (c_int, [H, fp, fp, c_int64, c_int64]),
        'nasr_get_adam_state': (c_int, [H, fp, fp, c_int64, POINTER(c_int64)]),
        'nasr_set_learning_rate': (c_int, [H, c_float]),
        'nasr_get_learning_rate': (c_int, [H, fp]),
        'nasr_set_ema': (c_int, [H, c_float]),
        'nasr_get_ema': (c_int, [H, fp, POINTER(c_int64), POINTER(c_int)]),
        'nasr_get_ema_state': (c_int, [H, fp, c_int64, POINTER(c_int64)]),
        'nasr_set_ema_state': (c_int, [H, fp, c_int64, c_int64]),
        'nasr_ema_swap': (c_int, [H]),
        'nasr_train_step': (c_int, [H, fp, ip, ip, ip, c_int, c_int, c_int, fp]),
        'nasr_forward': (c_int, [H, fp, ip, c_int, c_int, fp]),
        'nasr_logit_frames': (c_int, [H, c_int]),
        'nasr_loss': (c_int, [H, fp, ip, ip, ip, c_int, c_int, c_int, fp, fp]),
        'nasr_loss_and_grads': (c_int, [H, fp, ip, ip, ip, c_int, c_int, c_int, fp, fp, fp]),
        'nasr_greedy_decode': (c_int, [H, fp, ip, c_int, c_int, ip, ip]),
        'nasr_upload_batch': (c_int, [H, fp, ip, ip, ip, c_int, c_int, c_int]),
        'nasr_upload_batch_context': (c_int, [H, fp, fp, c_int, c_int, ip, ip, ip, c_int, c_int, c_int]),
        'nasr_compute_grads': (c_int, [H]),
        'nasr_grad_device_ptr': (c_void_p, [H]),
        'nasr_grad_device_count': (c_int64, [H]),
        'nasr_grad_bucket_count': (c_int, [H]),
        'nasr_grad_bucket': (c_int, [H, c_int, POINTER(c_int64), POINTER(c_int64)]),
        'nasr_grad_bucket_wait': (c_int, [H, c_int, c_void_p]),
        'nasr_apply_adam': (c_int, [H, c_float]),
        'nasr_set_grad_clip': (c_int, [H, c_float]),
        'nasr_get_grad_clip': (c_int, [H, fp]),
        'nasr_get_grad_clip_stats': (c_int, [H, POINTER(ClipStats), c_int]),
        'nasr_get_grads': (c_int, [H, fp, c_int64]),
        'nasr_set_grads': (c_int, [H, fp, c_int64]),
        'nasr_label_error_rate': (c_int, [ip, ip, c_int, ip, ip, c_int, c_int, fp]),
        'nasr_set_step_decode': (c_int, [H, c_int]),
        'nasr_get_decoded': (c_int, [H, ip, ip]),
        'nasr_ctc_beam_search': (c_int, [fp, ip, c_int, c_int, c_int, c_int, c_int, ip, ip, fp]),
        'nasr_ctc_beam_search_lm': (c_int, [fp, ip, c_int, c_int, c_int, c_int, c_int, fp, fp, c_int, c_int, c_float, c_float,
                                            ip, ip, fp]),
        'nasr_get_loss': (c_int, [H, fp]),
        'nasr_resident_frames': (c_int, [H, POINTER(c_int64)]),
        'nasr_resident_rows': (c_int, [H, POINTER(c_int64)]),
        'nasr_resident_shape': (c_int, [H, POINTER(c_int), POINTER(c_int)]),
        'nasr_set_row_compaction': (c_int, [H, c_int]),
        'nasr_set_profiling': (c_int, [H, c_int]),
        'nasr_get_phase_times': (c_int, [H, POINTER(PhaseTimes)]),
        'nasr_set_graph_mode': (c_int, [H, c_int]),
        'nasr_get_recurrence_mode': (c_int, [H]),
        'nasr_set_recurrence_mode': (c_int, [H, c_int]),
        'nasr_set_dropout_state': (c_int, [H, c_uint32, c_uint32]),
        'nasr_get_dropout_state': (c_int, [H, POINTER(c_uint32), POINTER(c_uint32)]),
        'nasr_step_void': (c_int, [H, POINTER(c_int)]),
        'nasr_get_persist_stats': (c_int, [H, POINTER(c_int), POINTER(c_int)]),
        'nasr_stage_batch': (c_int, [H, fp, ip, ip, ip, c_int, c_int, c_int, POINTER(c_int)]),
        'nasr_stage_batch_context': (c_int, [H, fp, fp, c_int, c_int, ip, ip, ip, c_int, c_int, c_int, POINTER(c_int)]),
        'nasr_upload_batch_audio': (c_int, [H, H, fp, POINTER(c_int64), ip, ip, ip, c_int, c_int, ip, POINTER(c_int)]),
        'nasr_stage_batch_audio': (c_int, [H, H, fp, POINTER(c_int64), ip, ip, ip, c_int, c_int, ip, POINTER(c_int),
                                           POINTER(c_int)]),
        'nasr_upload_batch_context_aug': (c_int, [H, fp, fp, c_int, c_int, ip, ip, ip, c_int, c_int, c_int, POINTER(BatchAug)]),
        'nasr_upload_batch_audio_aug': (c_int, [H, H, fp, POINTER(c_int64), ip, ip, ip, c_int, c_int, ip, POINTER(c_int),
                                                POINTER(BatchAug)]),
        'nasr_stage_batch_audio_aug': (c_int, [H, H, fp, POINTER(c_int64), ip, ip, ip, c_int, c_int, ip, POINTER(c_int),
                                               POINTER(BatchAug), POINTER(c_int)]),
        'nasr_upload_batch_audio_wave': (c_int, [H, H, fp, POINTER(c_int64), ip, ip, ip, c_int, c_int, ip, POINTER(c_int),
                                                 POINTER(BatchAug), POINTER(WaveAug)]),
        'nasr_stage_batch_audio_wave': (c_int, [H, H, fp, POINTER(c_int64), ip, ip, ip, c_int, c_int, ip, POINTER(c_int),
                                                POINTER(BatchAug), POINTER(WaveAug), POINTER(c_int)]),
        'nasr_featurizer_set_noise': (c_int, [H, fp, POINTER(c_int64), c_int]),
        'nasr_featurizer_set_rirs': (c_int, [H, fp, POINTER(c_int64), c_int]),
        'nasr_augment_audio': (c_int, [H, fp, POINTER(c_int64), ip, c_int, POINTER(WaveAug), fp, c_int64]),
        'nasr_forward_resident': (c_int, [H, fp]),
        'nasr_loss_resident': (c_int, [H, fp, fp]),
        'nasr_greedy_decode_resident': (c_int, [H, ip, ip]),
        'nasr_ctc_align': (c_int, [H, fp, ip, ip, ip, c_int, c_int, c_int, ip, POINTER(c_double)]),
        'nasr_ctc_align_resident': (c_int, [H, ip, POINTER(c_double)]),
        'nasr_ctc_align_logits': (c_int, [H, fp, ip, ip, ip, c_int, c_int, c_int, c_int, ip, POINTER(c_double)]),
        'nasr_ctc_align_lds': (c_int, [c_int, c_int]),
        'nasr_commit_batch': (c_int, [H, c_int]),
        'nasr_discard_batch': (c_int, [H, c_int]),
        'nasr_set_bucket_defer': (c_int, [H, c_int]),
        'nasr_comm_unique_id': (c_int, [c_void_p]),
        'nasr_comm_init': (c_int, [H, c_void_p, c_int, c_int]),
        'nasr_comm_size': (c_int, [H]),
        'nasr_comm_allreduce_grads': (c_int, [H]),
        'nasr_comm_mean': (c_int, [H, fp, c_int]),
        'nasr_comm_destroy': (c_int, [H]),
        'nasr_get_step_results': (c_int, [H, fp, POINTER(c_int), ip, ip]),
        'nasr_settle_step': (c_int, [H, c_int, POINTER(c_int)]),
        'nasr_step_token': (c_int64, [H]),
        'nasr_settle_token': (c_int, [H, c_int64, POINTER(c_int)]),
        'nasr_diag_bucket_traffic': (c_int, [H, c_int, c_void_p, c_int, c_int]),
        'nasr_get_step_logits': (c_int, [H, fp]),
        'nasr_set_wgrad_overlap': (c_int, [H, c_int]),
        'nasr_get_wgrad_overlap': (c_int, [H]),
        'nasr_create_wavenet': (c_int, [POINTER(WaveNetCfg), c_int, c_void_p, POINTER(H)]),
        'nasr_wavenet_bn_count': (c_int64, [H]),
        'nasr_wavenet_get_bn_state': (c_int, [H, fp, fp, fp, c_int64, POINTER(c_int64)]),
        'nasr_wavenet_set_bn_state': (c_int, [H, fp, fp, fp, c_int64, c_int64]),
        'nasr_wavenet_set_bn_hold': (c_int, [H, c_int]),
        'nasr_wavenet_get_batch_stats': (c_int, [H, fp, fp, c_int64]),
        'nasr_wavenet_apply_bn_stats': (c_int, [H, fp, fp, c_int64, c_int]),
        'nasr_create_las': (c_int, [POINTER(LasCfg), c_int, c_void_p, POINTER(H)]),
        'nasr_las_set_sampling': (c_int, [H, c_float, c_uint32, c_uint32, c_int]),
        'nasr_las_get_sampling': (c_int, [H, POINTER(c_float), POINTER(c_uint32), POINTER(c_uint32), POINTER(c_int)]),
        'nasr_las_forward': (c_int, [H, fp, ip, ip, ip, c_int, c_int, c_int, c_int, fp]),
        'nasr_las_forward_resident': (c_int, [H, c_int, fp]),
        'nasr_las_get_logits': (c_int, [H, fp]),
        'nasr_las_get_fed_ids': (c_int, [H, ip]),
        'nasr_las_get_sampled': (c_int, [H, ip]),
        'nasr_las_beam_search': (c_int, [H, fp, ip, c_int, c_int, c_int, c_int, c_int, c_int, c_float, ip]),
        'nasr_las_beam_search_resident': (c_int, [H, c_int, c_int, c_int, c_int, c_float, ip]),
        'nasr_las_beam_get_ids': (c_int, [H, ip]),
        'nasr_las_beam_get_trace': (c_int, [H, fp, ip, ip]),
        'nasr_las_beam_get_final': (c_int, [H, fp, ip, ip]),
        'nasr_las_beam_get_times': (c_int, [H, fp]),
        'nasr_las_beam_set_lm': (c_int, [H, fp, c_int, c_float]),
        'nasr_las_beam_get_lm_context': (c_int, [H, ip]),
        'nasr_create_featurizer': (c_int, [POINTER(MfccCfg), c_int, c_void_p, POINTER(H)]),
        'nasr_mfcc_frames': (c_int64, [POINTER(MfccCfg), c_int64]),
        'nasr_mfcc_width': (c_int, [POINTER(MfccCfg)]),
        'nasr_mfcc_filterbank': (c_int, [POINTER(MfccCfg), ip, fp]),
        'nasr_featurize': (c_int, [H, fp, POINTER(c_int64), c_int, fp, c_int64, POINTER(c_double)]),
        'nasr_featurize_times': (c_int, [H, fp, fp, fp]),
        'nasr_resample_filter': (c_int, [POINTER(c_double), c_int64]),
        'nasr_resample_length': (c_int64, [c_int32, c_int32, c_int64, POINTER(c_int64)]),
        'nasr_resample': (c_int, [H, fp, POINTER(c_int64), ip, c_int, fp, c_int64]),
        'nasr_featurize_rates': (c_int, [H, fp, POINTER(c_int64), ip, c_int, fp, c_int64, POINTER(c_double)]),
        'nasr_stream_open': (c_int, [H, c_int]),
        'nasr_stream_close': (c_int, [H]),
        'nasr_stream_reset': (c_int, [H, ip, c_int]),
        'nasr_stream_feed': (c_int, [H, fp, ip, c_int, fp]),
        'nasr_stream_frames': (c_int, [H, POINTER(c_int64)]),
        'nasr_stream_get_state': (c_int, [H, fp, c_int64]),
        'nasr_stream_set_state': (c_int, [H, fp, c_int64]),
        'nasr_stream_attach_audio': (c_int, [H, H]),
        'nasr_stream_audio_rows': (c_int, [H, POINTER(c_int64), POINTER(c_uint8), ip, POINTER(c_int)]),
        'nasr_stream_feed_audio': (c_int, [H, fp, POINTER(c_int64), POINTER(c_uint8), ip, POINTER(c_int), fp, c_int64]),
        'nasr_stream_open_lookahead': (c_int, [H, c_int, c_int]),
        'nasr_set_chunking': (c_int, [H, c_int, c_int]),
        'nasr_get_chunking': (c_int, [H, POINTER(c_int), POINTER(c_int)]),
        'nasr_set_frame_skip': (c_int, [H, c_int]),
        'nasr_get_frame_skip': (c_int, [H, POINTER(c_int)]),
        'nasr_stream_lookahead_rows': (c_int, [H, ip, POINTER(c_uint8), ip, POINTER(c_int)]),
        'nasr_stream_feed_lookahead': (c_int, [H, fp, ip, POINTER(c_uint8), c_int, ip, POINTER(c_int), fp, c_int64]),
        'nasr_ctc_beam_open': (c_int, [c_int, c_int, c_int, fp, fp, c_int, c_int, c_float, c_float, POINTER(c_void_p)]),
        'nasr_ctc_beam_feed': (c_int, [c_void_p, fp, c_int64, c_int]),
        'nasr_ctc_beam_best': (c_int, [c_void_p, ip, c_int, ip, fp]),
        'nasr_ctc_beam_close': (c_int, [c_void_p]),
        'nasr_set_distill': (c_int, [H, c_float, c_float]),
        'nasr_get_distill': (c_int, [H, fp, fp]),
        'nasr_set_teacher_logits': (c_int, [H, fp]),
        'nasr_take_teacher_logits': (c_int, [H, H]),
        'nasr_get_distill_loss': (c_int, [H, fp, fp]),
        'nasr_distill_logits': (c_int, [H, fp, fp, ip, c_int, c_int, c_float, c_float, fp, POINTER(c_double)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(lib, handle, rc):
    if rc == NASR_OK:
        return
    msg = lib.nasr_last_error(handle)
    msg = msg.decode() if msg else ''
    if rc == NASR_ERR_INFEASIBLE:
        raise InfeasibleLabelError(rc, msg)
    raise NasrError(rc, msg)
