"""ctypes binding of libosw_hip.so (include/osw.h).

The product path has NO CPU fallback: if the library is missing or the device is
absent, loading raises ``RuntimeError`` with the reason.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OSW_LIB", os.path.join(_HERE, "lib", "libosw_hip.so"))

OSW_OK = 0


class osw_dims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_mels", "n_audio_ctx", "n_audio_state", "n_audio_head", "n_audio_layer",
                                          "n_vocab", "n_text_ctx", "n_text_state", "n_text_head", "n_text_layer")]


class osw_window(C.Structure):
    _fields_ = [("clip", C.c_int32), ("seek", C.c_int32), ("segment_size", C.c_int32)]


class osw_decode_opts(C.Structure):
    _fields_ = [("task_token", C.c_int32), ("language_token", C.c_int32), ("suppress_blank", C.c_int32),
                ("without_timestamps", C.c_int32), ("max_initial_timestamp_index", C.c_int32),
                ("max_length", C.c_int32), ("suppress_tokens", C.POINTER(C.c_int32)), ("n_suppress", C.c_int32),
                ("eot", C.c_int32), ("sot", C.c_int32), ("sot_prev", C.c_int32), ("no_speech", C.c_int32),
                ("no_timestamps", C.c_int32), ("timestamp_begin", C.c_int32), ("blank", C.c_int32),
                ("first_lang", C.c_int32), ("n_langs", C.c_int32),
                ("prefix_tokens", C.POINTER(C.c_int32)), ("n_prefix", C.c_int32),
                ("language_tokens", C.POINTER(C.c_int32)),
                ("beam_size", C.c_int32), ("patience", C.c_float), ("length_penalty", C.c_float),
                ("num_hypotheses", C.c_int32), ("temperature", C.c_float), ("best_of", C.c_int32),
                ("seed", C.c_uint64), ("token_budget", C.POINTER(C.c_int32)),
                ("repetition_penalty", C.c_float), ("no_repeat_ngram_size", C.c_int32)]


class osw_window_result(C.Structure):
    _fields_ = [("tokens", C.POINTER(C.c_int32)), ("max_tokens", C.c_int32), ("n_tokens", C.POINTER(C.c_int32)),
                ("sum_logprob", C.POINTER(C.c_float)), ("no_speech_prob", C.POINTER(C.c_float)),
                ("language", C.POINTER(C.c_int32)), ("logits_dump", C.POINTER(C.c_float)),
                ("dump_steps", C.c_int32)]


class osw_session_window(C.Structure):
    _fields_ = [("tag", C.c_int64), ("seek", C.c_int32), ("segment_size", C.c_int32), ("language_token", C.c_int32),
                ("token_budget", C.c_int32), ("n_prefix", C.c_int32), ("prefix", C.POINTER(C.c_int32)),
                ("clip", C.c_int64)]


class osw_align_window(C.Structure):
    _fields_ = [("window", C.c_int32), ("sot", C.c_int32), ("language", C.c_int32), ("task", C.c_int32),
                ("no_timestamps", C.c_int32), ("eot", C.c_int32), ("tokens", C.POINTER(C.c_int32)),
                ("n_tokens", C.c_int32), ("num_frames", C.c_int32), ("median_filter_width", C.c_int32)]


class osw_align_result(C.Structure):
    _fields_ = [("token_frame", C.POINTER(C.c_int32)), ("token_prob", C.POINTER(C.c_double)), ("stride", C.c_int32)]


class osw_enc_gemm_desc(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("M", "N", "K", "variant", "epi", "heads_T", "heads_H", "heads_nb")] +
                [(n, C.c_int64) for n in ("lda", "a_grp_rows", "a_grp_stride", "a_count", "ldc", "c_grp_rows",
                                          "c_grp_stride", "c_offset", "c_bytes", "pos_count")] +
                [("A", C.c_void_p), ("W", C.c_void_p), ("bias", C.POINTER(C.c_float)), ("pos", C.POINTER(C.c_float)),
                 ("heads_slot", C.POINTER(C.c_int32)), ("C", C.c_void_p)])


_SELECT_ARRAYS = ("logits", "pos", "state", "prompt", "cur_tok", "tokens", "budget", "anc", "bwin", "best_tok",
                  "lp_hist", "best_lp", "lang_probs", "counters")
_SELECT_FLOAT = ("logits", "lp_hist", "best_lp", "lang_probs")


class osw_retry_window(C.Structure):
    _fields_ = [("tag", C.c_int64), ("temperature", C.c_float), ("seed", C.c_uint64), ("language_token", C.c_int32)]


class osw_select_io(C.Structure):
    """osw_debug_select_step's arrays: every ``*_len`` counts 32-bit words (include/osw.h)."""
    ARRAYS, FLOAT = _SELECT_ARRAYS, _SELECT_FLOAT
    _fields_ = ([(n, C.c_int32) for n in ("mode", "n_prefix", "rows", "max_tok", "pstride")] +
                [(n + "_len", C.c_int64) for n in _SELECT_ARRAYS] +
                [(n, C.POINTER(C.c_float if n in _SELECT_FLOAT else C.c_int32)) for n in _SELECT_ARRAYS])


class osw_profile(C.Structure):
    _fields_ = [("mel_ms", C.c_double), ("encoder_ms", C.c_double), ("crosskv_ms", C.c_double),
                ("decoder_ms", C.c_double), ("total_ms", C.c_double), ("decode_steps", C.c_int64),
                ("enc_gemm_ms", C.c_double), ("enc_gemm_launches", C.c_int64), ("enc_gemm_flops", C.c_double),
                ("enc_attn_ms", C.c_double), ("enc_attn_launches", C.c_int64), ("enc_attn_flops", C.c_double),
                ("mel_kernel_ms", C.c_double), ("mel_kernel_launches", C.c_int64), ("mel_kernel_bytes", C.c_double),
                ("xattn_ms", C.c_double), ("xattn_launches", C.c_int64), ("xattn_bytes", C.c_double)]

    def as_dict(self) -> dict:
        return {n: getattr(self, n) for n, _ in self._fields_}


P = C.POINTER
_SIGS = {
    "osw_version": (C.c_char_p, []),
    "osw_last_error": (C.c_char_p, []),
    "osw_device_count": (C.c_int, [P(C.c_int32)]),
    "osw_create": (C.c_int, [P(osw_dims), C.c_int32, C.c_int32, P(C.c_void_p)]),
    "osw_destroy": (C.c_int, [C.c_void_p]),
    "osw_create_sibling": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_void_p)]),
    "osw_set_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    "osw_get_weight": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64]),
    # int8 decoder weights (STT_COMPUTE_TYPE=int8_float16): q int8 [N][K], one fp32 multiplier per row
    "osw_set_weight_quant": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, P(C.c_float), C.c_int64, C.c_int64]),
    "osw_weight_is_quant": (C.c_int, [C.c_void_p, C.c_char_p, P(C.c_int32)]),
    "osw_init_weight_uniform": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.c_int64, C.c_float, C.c_float,
                                          C.c_int64, C.c_int64]),
    "osw_finalize": (C.c_int, [C.c_void_p]),
    "osw_log_mel": (C.c_int, [C.c_void_p, C.c_void_p, P(C.c_int64), C.c_int32, C.c_int32, P(C.c_int32)]),
    "osw_get_mel": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), C.c_int64]),
    "osw_encode_windows": (C.c_int, [C.c_void_p, P(osw_window), C.c_int32]),
    "osw_get_encoder_output": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), C.c_int64]),
    "osw_decode_windows": (C.c_int, [C.c_void_p, C.c_int32, P(osw_decode_opts), P(osw_window_result)]),
    # a re-decode of some of the encoded windows (faster-whisper's generate_with_fallback retries)
    "osw_decode_window_list": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_int32), P(osw_decode_opts),
                                         P(osw_window_result)]),
    "osw_transcribe_batch": (C.c_int, [C.c_void_p, C.c_void_p, P(C.c_int64), C.c_int32, C.c_int32,
                                       P(osw_decode_opts), P(osw_window_result)]),
    "osw_transcribe_refill": (C.c_int, [C.c_void_p, C.c_void_p, P(C.c_int64), C.c_int32, C.c_int32,
                                        P(osw_decode_opts), P(osw_window_result), C.c_int32]),
    "osw_session_begin": (C.c_int, [C.c_void_p, P(osw_decode_opts)]),
    "osw_session_add": (C.c_int, [C.c_void_p, C.c_void_p, P(C.c_int64), C.c_int32, P(osw_session_window)]),
    "osw_session_step": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, P(osw_window_result), P(C.c_int64), C.c_int32,
                                   P(C.c_int32), P(C.c_int32), P(C.c_int32)]),
    "osw_session_release_clip": (C.c_int, [C.c_void_p, C.c_int64]),
    "osw_session_end": (C.c_int, [C.c_void_p]),
    # word timestamps on a session: finished windows keep their slots until aligned or released
    "osw_session_hold": (C.c_int, [C.c_void_p, C.c_int32]),
    "osw_session_align": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_int64), P(osw_align_window), P(osw_align_result)]),
    "osw_session_release": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_int64)]),
    # temperature fallback on a session: a held window decodes again in its slot with sampled rows
    "osw_session_retries": (C.c_int, [C.c_void_p, C.c_int32]),
    "osw_session_retry": (C.c_int, [C.c_void_p, C.c_int32, P(osw_retry_window)]),
    # confidences (replace ctranslate2's return_scores per token, faster-whisper's language_probability /
    # all_language_probs and WhisperModel.detect_language)
    "osw_set_confidences": (C.c_int, [C.c_void_p, C.c_int32]),
    "osw_get_token_logprobs": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), C.c_int32, P(C.c_int32)]),
    "osw_get_language_probs": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), C.c_int32]),
    "osw_detect_language": (C.c_int, [C.c_void_p, C.c_int32, P(osw_decode_opts), P(C.c_float), P(C.c_float)]),
    # word timestamps (replace ctranslate2 Whisper.align as faster-whisper's find_alignment calls it)
    "osw_set_alignment_heads": (C.c_int, [C.c_void_p, P(C.c_int32), C.c_int32]),
    "osw_align_windows": (C.c_int, [C.c_void_p, C.c_int32, P(osw_align_window), P(osw_align_result)]),
    "osw_get_alignment_matrix": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), C.c_int64, P(C.c_int32),
                                           P(C.c_int32)]),
    "osw_debug_dtw": (C.c_int, [C.c_void_p, P(C.c_float), C.c_int32, C.c_int32, P(C.c_int32), P(C.c_int32),
                                P(C.c_int32)]),
    # the alignment pass's other kernels, one production launcher per call (tests/test_gpu_align_kernels.py)
    "osw_debug_align_post": (C.c_int, [C.c_void_p, P(C.c_float), C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       P(C.c_int32), P(C.c_int32), P(C.c_int32), P(C.c_int32), P(C.c_float),
                                       P(C.c_float), P(C.c_float)]),
    "osw_debug_align_tail": (C.c_int, [C.c_void_p, P(C.c_float), C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                       P(C.c_int32), P(C.c_int32), P(C.c_int32), P(C.c_int32), C.c_int32,
                                       P(C.c_float), P(C.c_int32), P(C.c_int32)]),
    "osw_debug_align_self_attn": (C.c_int, [C.c_void_p, P(C.c_float), C.c_int32, P(C.c_float), P(C.c_float),
                                            P(C.c_float), C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_int32),
                                            P(C.c_float)]),
    "osw_debug_align_scores": (C.c_int, [C.c_void_p, P(C.c_float), C.c_int32, P(C.c_float), C.c_void_p, C.c_int32,
                                         C.c_int32, C.c_int32, P(C.c_int32), C.c_int32, C.c_int32, C.c_int32,
                                         P(C.c_int32), P(C.c_int32), C.c_int32, C.c_int32, P(C.c_float)]),
    # the history-rules kernel alone (replaces ctranslate2's RepetitionPenalty / NoRepeatNgram processors)
    "osw_debug_history_rules": (C.c_int, [C.c_void_p, P(C.c_float), C.c_int32, C.c_int32, P(C.c_int32), C.c_int32,
                                          P(C.c_int32), C.c_float, C.c_int32]),
    "osw_debug_history_rules_time": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_int32,
                                               C.c_int32, P(C.c_float)]),
    # one selection step (select kernel + beam update) on host logits and state (tests/test_gpu_select.py)
    "osw_debug_select_step": (C.c_int, [C.c_void_p, P(osw_decode_opts), P(osw_select_io)]),
    "osw_debug_select_step_rows": (C.c_int, [C.c_void_p, P(osw_decode_opts), P(osw_select_io), C.c_int32,
                                             P(C.c_float), P(C.c_uint64)]),
    "osw_encoder_layer_debug": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), P(C.c_float), C.c_int32]),
    "osw_debug_gemm": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                 P(C.c_float), C.c_int32, P(C.c_float)]),
    # one attention launch on host data (parity tests)
    "osw_debug_enc_attn": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "osw_debug_dec_xattn": (C.c_int, [C.c_void_p, P(C.c_float), C.c_int32, P(C.c_float), C.c_void_p, C.c_void_p,
                                      C.c_int32, C.c_int32, C.c_int32, P(C.c_float)]),
    "osw_debug_dec_xattn_windows": (C.c_int, [C.c_void_p, P(C.c_float), C.c_int32, P(C.c_float), C.c_void_p,
                                              C.c_void_p, C.c_int32, P(C.c_int32), C.c_int32, C.c_int32, C.c_int32,
                                              P(C.c_float)]),
    "osw_debug_dec_self_attn": (C.c_int, [C.c_void_p, P(C.c_float), C.c_int32, P(C.c_float), C.c_void_p, C.c_void_p,
                                          C.c_int32, P(C.c_int32), C.c_int32, P(C.c_int32), C.c_int32,
                                          P(C.c_float)]),
    # one launch of the decoder's linear path on host data (parity tests)
    "osw_debug_dec_gemm": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p, C.c_int32, P(C.c_float), C.c_int64, P(C.c_int32)]),
    "osw_debug_dec_gemm_quant": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_void_p, P(C.c_float), C.c_int32, P(C.c_float), C.c_int64,
                                        P(C.c_int32)]),
    "osw_debug_dec_gemm_time": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, P(C.c_float), C.c_int32, C.c_int32, C.c_int32, P(C.c_float),
                                          P(C.c_float)]),
    "osw_debug_logits_profile": (C.c_int, [C.c_void_p, P(C.c_double), P(C.c_int64)]),
    "osw_debug_dec_resln": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, P(C.c_float), C.c_int32,
                                      P(C.c_float), P(C.c_float), P(C.c_float), P(C.c_float), C.c_void_p,
                                      P(C.c_float), P(C.c_int32), P(C.c_int32), C.c_int32, C.c_int32, C.c_int32,
                                      C.c_void_p, C.c_int32, C.c_int32, P(C.c_float), C.c_void_p, C.c_void_p,
                                      P(C.c_float), C.c_int64, P(C.c_int32)]),
    "osw_debug_dec_gelu": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, P(C.c_float), C.c_int32,
                                     P(C.c_float), C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                     P(C.c_float), C.c_int64, P(C.c_int32)]),
    # one launch of the encoder's tiled GEMM / LayerNorm on host data (parity tests)
    "osw_debug_enc_gemm": (C.c_int, [C.c_void_p, P(osw_enc_gemm_desc)]),
    "osw_debug_enc_layernorm": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, P(C.c_float), P(C.c_float),
                                          P(C.c_float), C.c_void_p]),
    # the log-mel front end's raw values and its window-packing kernel alone (parity tests)
    "osw_debug_get_logmel": (C.c_int, [C.c_void_p, C.c_int32, P(C.c_float), C.c_int64, P(C.c_float)]),
    "osw_debug_mel_windows": (C.c_int, [C.c_void_p, P(osw_window), C.c_int32, C.c_void_p, C.c_int64]),
    "osw_debug_hold_capture": (C.c_int, [C.c_void_p, C.c_int32]),
    "osw_set_encoder_baton_min": (C.c_int, [C.c_void_p, C.c_int32]),
    "osw_set_profiling": (C.c_int, [C.c_void_p, C.c_int32]),
    "osw_get_profile": (C.c_int, [C.c_void_p, P(osw_profile)]),
    "osw_stream": (C.c_void_p, [C.c_void_p]),
    "osw_ingest_mean_square": (C.c_int, [C.c_int32, P(C.c_int16), C.c_int64, C.c_int32, P(C.c_float)]),
    "osw_ingest_apply_gain": (C.c_int, [C.c_int32, P(C.c_int16), C.c_int64, C.c_int32, C.c_int32, C.c_float,
                                        P(C.c_int16)]),
    "osw_ingest_resample": (C.c_int, [C.c_int32, P(C.c_int16), C.c_int64, C.c_int32, C.c_int32, P(C.c_float),
                                      C.c_int32, P(C.c_int16), C.c_int64]),
}
EXPORTED = tuple(_SIGS)

_lib = None
_lock = threading.Lock()


def load() -> C.CDLL:
    """Load libosw_hip.so (raises RuntimeError if it is absent: no fallback)."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"libosw_hip.so not found at {LIB_PATH}: build it with `python __graft_entry__.py` "
                               "or `make -C open-speech_amd/csrc` (there is no CPU fallback)")
        lib = C.CDLL(LIB_PATH)
        for name, (res, args) in _SIGS.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        _lib = lib
        return lib


OSW_EINVAL = -22
OSW_EHIP = -100
OSW_ESTATE = -101
OSW_ECAPTURE = -102


class OswError(RuntimeError):
    """A non-zero return code of libosw_hip.so (``rc``) with its osw_last_error() text."""

    def __init__(self, msg: str, rc: int):
        super().__init__(msg)
        self.rc = rc


class OswDeviceError(OswError):
    """OSW_EHIP: a HIP runtime error on the context's device (the batcher fails the GPU over)."""


class OswCaptureError(OswError):
    """OSW_ECAPTURE: a stream capture was refused or invalidated.  Not a device fault: the
    context and the GPU stay usable (the batcher fails only the affected requests)."""


def check(rc: int, what: str = "") -> None:
    if rc != OSW_OK:
        msg = load().osw_last_error().decode(errors="replace")
        cls = {OSW_EHIP: OswDeviceError, OSW_ECAPTURE: OswCaptureError}.get(rc, OswError)
        raise cls(f"{what} failed ({rc}): {msg}", rc)
