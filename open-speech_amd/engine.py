"""Python handle on one libosw_hip.so context (one GPU).

This is the layer the backend (``backend.py``) and the bench drive; it converts
numpy arrays to the C ABI of ``include/osw.h`` and back.  It replaces the
``WhisperModel`` object the reference constructs at
``src/backends/faster_whisper.py:40-45``.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from dataclasses import dataclass, field

import numpy as np

from . import _lib
from .dims import SpecialTokens, WhisperDims
from .weights import F16, canonical_specs, make_tensor


@dataclass
class DecodeConfig:
    task: str = "transcribe"
    language_token: int | None = None       # None -> detect
    suppress_tokens: tuple = ()
    suppress_blank: bool = True
    without_timestamps: bool = False
    max_initial_timestamp_index: int | None = 50
    max_length: int = 448
    beam_size: int = 1                      # 1 = greedy (parity mode); the reference runs 5
    patience: float = 1.0
    length_penalty: float = 1.0
    num_hypotheses: int = 1
    temperature: float = 0.0                # > 0: faster-whisper's sampling branch (best_of rows per window)
    best_of: int = 5
    seed: int = 0
    # length control (bench only; not a faster-whisper option): window i ends with
    # <|endoftext|> after token_budget[i] sampled tokens (<= 0: no limit)
    token_budget: tuple | None = None
    # faster-whisper's repetition_penalty / no_repeat_ngram_size (CTranslate2 logits processors)
    # over what the row sampled so far in its window: 1.0 / 0 = off
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    # per-token log-probabilities and language probabilities (osw_set_confidences): what
    # CTranslate2's return_scores and faster-whisper's language_probability / all_language_probs
    # give; tokens, sum_logprob, no_speech_prob and language are the same bits on and off
    confidences: bool = False


@dataclass
class WindowOutput:
    tokens: list
    sum_logprob: float
    no_speech_prob: float
    language: int
    logits: np.ndarray | None = field(default=None, repr=False)
    # DecodeConfig.confidences (None when off).  cum_logprobs: the device's fp32 cumulative
    # log-probability after each token, with a closing <|endoftext|> entry when the row ended with
    # one (its last entry is sum_logprob, bit for bit); token_logprobs: their float64 differences,
    # one per returned token; eot_logprob: the closing step's, None for a row cut at max_length;
    # language_probs: softmax over the language tokens at <|startoftranscript|> [n_langs]
    token_logprobs: list | None = None
    eot_logprob: float | None = None
    language_probs: np.ndarray | None = field(default=None, repr=False)
    cum_logprobs: np.ndarray | None = field(default=None, repr=False)


def split_cumulative(cum: np.ndarray, n_tokens: int):
    """(token_logprobs, eot_logprob) from a window's cumulative fp32 log-probabilities: the
    differences of neighbours in float64; entry ``n_tokens``, if present, is the <|endoftext|>
    step's."""
    lp = np.diff(np.asarray(cum, dtype=np.float64), prepend=0.0)
    return lp[:n_tokens].tolist(), (float(lp[n_tokens]) if len(lp) > n_tokens else None)


@dataclass
class AlignWindow:
    """One window of ``WhisperEngine.align``: ``window`` indexes the last encode / decode
    call, ``tokens`` are its text tokens (ids below <|endoftext|>, timestamps removed),
    ``num_frames`` its segment_size in mel frames."""
    window: int
    tokens: list
    num_frames: int
    language: int
    task: str = "transcribe"
    median_filter_width: int = 7


@dataclass
class Alignment:
    token_frame: np.ndarray   # [n + 1] first key frame (0.02 s units) of each text token and of <|endoftext|>
    token_prob: np.ndarray    # [n] softmax(logits[:eot])[token]


# csrc/seltypes.h SelState / BeamWin as numpy records (debug_select_step)
SEL_STATE = np.dtype([("n_sampled", "i4"), ("last", "i4"), ("penult", "i4"), ("last_ts", "i4"), ("done", "i4"),
                      ("lang", "i4"), ("sum_lp", "f4"), ("nsp", "f4"), ("plen", "i4"), ("n_lp", "i4")])
BEAM_WIN = np.dtype([("n_hyp", "i4"), ("best_len", "i4"), ("done", "i4"), ("best_nlp", "i4"), ("best_norm", "f4"),
                     ("best_raw", "f4")])


def _i32p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class WhisperEngine:
    def __init__(self, dims: WhisperDims, device: int = 0, max_batch: int = 16, _parent: "WhisperEngine" = None):
        self.lib = _lib.load()
        self.dims = dims
        self.device = device
        self.max_batch = max_batch
        self.max_rows = 5 * max_batch   # decoder rows: windows x beam_size
        self.st = SpecialTokens.for_vocab(dims.n_vocab)
        ctx = C.c_void_p()
        if _parent is None:
            d = _lib.osw_dims(dims.n_mels, dims.n_audio_ctx, dims.n_audio_state, dims.n_audio_head,
                              dims.n_audio_layer, dims.n_vocab, dims.n_text_ctx, dims.n_text_state,
                              dims.n_text_head, dims.n_text_layer)
            _lib.check(self.lib.osw_create(C.byref(d), device, max_batch, C.byref(ctx)), "osw_create")
        else:
            _lib.check(self.lib.osw_create_sibling(_parent.ctx, max_batch, C.byref(ctx)), "osw_create_sibling")
        self.ctx = ctx
        self._nframes: list[int] = []
        self._conf = False

    def sibling(self, max_batch: int | None = None) -> "WhisperEngine":
        """A second engine on the same GPU sharing this one's (loaded) weights, with its
        own stream and workspaces: drive it from another thread to overlap batches."""
        e = WhisperEngine(self.dims, self.device, max_batch or self.max_batch, _parent=self)
        if getattr(self, "_align_heads", None):
            e.set_alignment_heads(self._align_heads)
        return e

    # ------------------------------------------------------------ weights
    def set_weight(self, name: str, arr: np.ndarray) -> None:
        a = np.ascontiguousarray(arr)
        _lib.check(self.lib.osw_set_weight(self.ctx, name.encode(), a.ctypes.data_as(C.c_void_p), a.nbytes),
                   f"osw_set_weight({name})")

    def get_weight(self, name: str) -> np.ndarray:
        """The tensor as stored on the device (enc.conv1.w with its mel axis padded to a
        multiple of 64)."""
        sp = {s.name: s for s in canonical_specs(self.dims)}[name]
        dt = np.float16 if sp.dtype == F16 else np.float32
        n = int(np.prod(sp.shape))
        if name == "enc.conv1.w":
            n = self.dims.n_audio_state * 3 * ((self.dims.n_mels + 63) // 64 * 64)
        out = np.empty(n, dt)
        _lib.check(self.lib.osw_get_weight(self.ctx, name.encode(), out.ctypes.data_as(C.c_void_p), out.nbytes),
                   f"osw_get_weight({name})")
        return out

    def set_weight_q8(self, name: str, q: np.ndarray, mult: np.ndarray) -> None:
        """Int8 weights for one decoder matrix (osw_set_weight_quant): W[n][k] ~ q[n][k] * mult[n], q int8
        [N][K], mult float32 [N].  Accepted for dec.tok and dec.lN.{qkv,o,xq,xo,fc1,fc2}.w."""
        q = np.asarray(q)
        mult = np.asarray(mult)
        if q.dtype != np.int8 or q.ndim != 2 or mult.shape != (q.shape[0],):
            raise ValueError(f"{name}: q int8 [N][K] and mult [N] expected, got {q.dtype} {q.shape} / {mult.shape}")
        q = np.ascontiguousarray(q)
        m = np.ascontiguousarray(mult, dtype=np.float32)
        _lib.check(self.lib.osw_set_weight_quant(self.ctx, name.encode(), q.ctypes.data_as(C.c_void_p),
                                              m.ctypes.data_as(C.POINTER(C.c_float)), q.size, m.size),
                   f"osw_set_weight_quant({name})")

    def weight_is_q8(self, name: str) -> bool:
        """Whether decoder matrix ``name`` holds int8 weights; a name that cannot raises OswError."""
        out = C.c_int32()
        _lib.check(self.lib.osw_weight_is_quant(self.ctx, name.encode(), C.byref(out)), f"osw_weight_is_quant({name})")
        return bool(out.value)

    def load_weights(self, w: dict) -> None:
        """Upload every canonical tensor; a ``weights.QuantizedMatrix`` value goes through set_weight_q8."""
        from .weights import QuantizedMatrix
        for sp in canonical_specs(self.dims):
            arr = w[sp.name]
            if isinstance(arr, QuantizedMatrix):
                if tuple(arr.q.shape) != tuple(sp.shape):
                    raise ValueError(f"{sp.name}: int8 shape {arr.q.shape}, expected {sp.shape}")
                self.set_weight_q8(sp.name, arr.q, arr.mult)
                continue
            want = np.float16 if sp.dtype == F16 else np.float32
            self.set_weight(sp.name, np.asarray(arr, dtype=want))
        _lib.check(self.lib.osw_finalize(self.ctx), "osw_finalize")

    def init_random(self, seed: int = 0, text_pos: float | None = None, **spec_kw) -> None:
        """Deterministic random weights: large fp16 matrices generated on the device by
        the counter hash, small fp32 tensors generated by numpy (same values as
        ``weights.random_weights(dims, seed, text_pos, **spec_kw)``)."""
        from .weights import text_positional
        for i, sp in enumerate(canonical_specs(self.dims, **spec_kw)):
            if sp.name == "dec.pos" and text_pos:
                self.set_weight(sp.name, text_positional(self.dims, seed, text_pos, **spec_kw))
                continue
            device_ok = sp.dtype == F16 and sp.kind == "uniform" and not (
                sp.name == "enc.conv1.w" and self.dims.n_mels % 64)
            if device_ok:
                _lib.check(self.lib.osw_init_weight_uniform(self.ctx, sp.name.encode(), seed, i, sp.scale, sp.offset,
                                                            sp.zero_lo, sp.zero_hi), f"init {sp.name}")
            else:
                self.set_weight(sp.name, make_tensor(sp, self.dims, seed, i))
        _lib.check(self.lib.osw_finalize(self.ctx), "osw_finalize")

    # ------------------------------------------------------------ stages
    def log_mel(self, clips: list, on_device_ptr: int | None = None, offsets: np.ndarray | None = None) -> list[int]:
        """Compute and keep resident the log-mel of each int16 clip."""
        if on_device_ptr is None:
            arrs = [np.asarray(x, dtype=np.int16) for x in clips]
            offs = np.zeros(len(arrs) + 1, np.int64)
            offs[1:] = np.cumsum([len(a) for a in arrs])
            pcm = np.concatenate(arrs) if offs[-1] else np.zeros(1, np.int16)
            ptr, on_dev = pcm.ctypes.data_as(C.c_void_p), 0
            n = len(arrs)
        else:
            offs = np.ascontiguousarray(offsets, dtype=np.int64)
            ptr, on_dev, n = C.c_void_p(on_device_ptr), 1, len(offs) - 1
        nf = np.zeros(n, np.int32)
        _lib.check(self.lib.osw_log_mel(self.ctx, ptr, offs.ctypes.data_as(C.POINTER(C.c_int64)), n, on_dev,
                                        _i32p(nf)), "osw_log_mel")
        self._nframes = nf.tolist()
        return self._nframes

    def get_mel(self, clip: int) -> np.ndarray:
        nf = self._nframes[clip]
        out = np.empty((self.dims.n_mels, nf), np.float32)
        _lib.check(self.lib.osw_get_mel(self.ctx, clip, out.ctypes.data_as(C.POINTER(C.c_float)), out.size),
                   "osw_get_mel")
        return out

    def encode(self, windows: list) -> None:
        arr = (_lib.osw_window * len(windows))(*[_lib.osw_window(int(c), int(s), int(z)) for c, s, z in windows])
        _lib.check(self.lib.osw_encode_windows(self.ctx, arr, len(windows)), "osw_encode_windows")

    def encoder_output(self, window: int) -> np.ndarray:
        out = np.empty((self.dims.n_audio_ctx, self.dims.n_audio_state), np.float32)
        _lib.check(self.lib.osw_get_encoder_output(self.ctx, window, out.ctypes.data_as(C.POINTER(C.c_float)),
                                                   out.size), "osw_get_encoder_output")
        return out

    def encoder_layer(self, layer: int, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x, dtype=np.float32)
        y = np.empty_like(x)
        _lib.check(self.lib.osw_encoder_layer_debug(self.ctx, layer, x.ctypes.data_as(C.POINTER(C.c_float)),
                                                    y.ctypes.data_as(C.POINTER(C.c_float)), x.shape[0]),
                   "osw_encoder_layer_debug")
        return y

    def _opts(self, cfg: DecodeConfig, n: int, prefix: list | None, languages: list | None = None):
        st = self.st
        sup = np.ascontiguousarray(np.asarray(cfg.suppress_tokens, dtype=np.int32).reshape(-1))
        if prefix:
            lens = {len(p) for p in prefix}
            if len(lens) != 1:
                raise ValueError("all windows of one decode call need the same prefix length")
            pre = np.ascontiguousarray(np.asarray(prefix, dtype=np.int32).reshape(-1))
            n_pre = len(prefix[0])
        else:
            pre = np.zeros(1, np.int32)
            n_pre = 0
        # an English-only model: the start sequence is <|startoftranscript|> alone (osw.h: task_token < 0)
        task = -1 if not st.multilingual else st.transcribe if cfg.task == "transcribe" else st.translate
        o = _lib.osw_decode_opts(
            task_token=task, language_token=-1 if cfg.language_token is None else int(cfg.language_token),
            suppress_blank=int(cfg.suppress_blank), without_timestamps=int(cfg.without_timestamps),
            max_initial_timestamp_index=-1 if cfg.max_initial_timestamp_index is None
            else int(cfg.max_initial_timestamp_index),
            max_length=int(cfg.max_length), suppress_tokens=_i32p(sup), n_suppress=len(sup) if sup.size else 0,
            eot=st.eot, sot=st.sot, sot_prev=st.sot_prev, no_speech=st.no_speech, no_timestamps=st.no_timestamps,
            timestamp_begin=st.timestamp_begin, blank=st.blank, first_lang=st.first_lang, n_langs=st.n_langs,
            prefix_tokens=_i32p(pre), n_prefix=n_pre, beam_size=int(cfg.beam_size), patience=float(cfg.patience),
            length_penalty=float(cfg.length_penalty), num_hypotheses=int(cfg.num_hypotheses),
            temperature=float(cfg.temperature), best_of=int(cfg.best_of), seed=int(cfg.seed) & 0xFFFFFFFFFFFFFFFF,
            repetition_penalty=float(cfg.repetition_penalty), no_repeat_ngram_size=int(cfg.no_repeat_ngram_size))
        budget = None
        if cfg.token_budget is not None:
            if len(cfg.token_budget) != n:
                raise ValueError("one token budget per window")
            budget = np.ascontiguousarray(cfg.token_budget, dtype=np.int32)
            o.token_budget = _i32p(budget)
        langs = None
        if languages is not None:
            if len(languages) != n:
                raise ValueError("one language token per window")
            langs = np.ascontiguousarray([-1 if x is None else int(x) for x in languages], dtype=np.int32)
            o.language_tokens = _i32p(langs)
        return o, (sup, pre, langs, budget)

    def _result(self, n: int, dump_steps: int):
        mt = self.dims.n_text_ctx
        bufs = dict(tokens=np.zeros((n, mt), np.int32), n=np.zeros(n, np.int32), lp=np.zeros(n, np.float32),
                    nsp=np.zeros(n, np.float32), lang=np.zeros(n, np.int32))
        dump = np.zeros((n, dump_steps, self.dims.n_vocab), np.float32) if dump_steps else None
        r = _lib.osw_window_result(
            tokens=_i32p(bufs["tokens"]), max_tokens=mt, n_tokens=_i32p(bufs["n"]),
            sum_logprob=bufs["lp"].ctypes.data_as(C.POINTER(C.c_float)),
            no_speech_prob=bufs["nsp"].ctypes.data_as(C.POINTER(C.c_float)), language=_i32p(bufs["lang"]),
            logits_dump=dump.ctypes.data_as(C.POINTER(C.c_float)) if dump is not None else None,
            dump_steps=dump_steps)
        return r, bufs, dump

    def _set_confidences(self, on: bool) -> None:
        if bool(on) != self._conf:
            _lib.check(self.lib.osw_set_confidences(self.ctx, int(bool(on))), "osw_set_confidences")
            self._conf = bool(on)

    def _outputs(self, n, bufs, dump, conf: bool = False) -> list[WindowOutput]:
        outs = [WindowOutput(tokens=bufs["tokens"][i, :bufs["n"][i]].tolist(), sum_logprob=float(bufs["lp"][i]),
                             no_speech_prob=float(bufs["nsp"][i]), language=int(bufs["lang"][i]),
                             logits=None if dump is None else dump[i]) for i in range(n)]
        if conf:
            self._fetch_confidences(outs)
        return outs

    def _fetch_confidences(self, outs: list) -> None:
        """The confidences of the windows the last decode call returned, fetched after it
        (osw_get_alignment_matrix's way): host copies, no device work."""
        f32p = C.POINTER(C.c_float)
        for i, out in enumerate(outs):
            cum = np.zeros(self.dims.n_text_ctx + 1, np.float32)
            cnt = C.c_int32()
            _lib.check(self.lib.osw_get_token_logprobs(self.ctx, i, cum.ctypes.data_as(f32p), len(cum),
                                                       C.byref(cnt)), "osw_get_token_logprobs")
            probs = None
            if self.st.multilingual:
                probs = np.zeros(self.st.n_langs, np.float32)
                _lib.check(self.lib.osw_get_language_probs(self.ctx, i, probs.ctypes.data_as(f32p), len(probs)),
                           "osw_get_language_probs")
            out.cum_logprobs = cum[:cnt.value].copy()
            out.token_logprobs, out.eot_logprob = split_cumulative(out.cum_logprobs, len(out.tokens))
            out.language_probs = probs

    def detect_language(self, n: int, return_logits: bool = False):
        """Language probabilities [n][n_langs] of the ``n`` windows last encoded
        (osw_detect_language: one decoder step on <|startoftranscript|>; replaces
        ``WhisperModel.detect_language``).  A later ``decode`` of the same windows is not
        affected.  ``return_logits``: also the raw logits the softmax was taken over."""
        if not self.st.multilingual:
            raise ValueError("an English-only model has no language to detect (its language is 'en')")
        o, keep = self._opts(DecodeConfig(), n, None)
        f32p = C.POINTER(C.c_float)
        probs = np.zeros((n, self.st.n_langs), np.float32)
        raw = np.zeros((n, self.st.n_langs), np.float32) if return_logits else None
        _lib.check(self.lib.osw_detect_language(self.ctx, int(n), C.byref(o), probs.ctypes.data_as(f32p),
                                                raw.ctypes.data_as(f32p) if raw is not None else None),
                   "osw_detect_language")
        del keep
        return (probs, raw) if return_logits else probs

    def decode(self, n: int, cfg: DecodeConfig, prefix: list | None = None, dump_steps: int = 0,
               languages: list | None = None, windows: list | None = None) -> list[WindowOutput]:
        """Decode the ``n`` windows last encoded, or with ``windows`` (``n`` distinct indices into
        the last encode call; osw_decode_window_list) just those: entry i of ``prefix``,
        ``languages``, ``cfg.token_budget`` and of the result belongs to ``windows[i]``, and the
        result is what encoding only those windows in that order and decoding them gives, bit for
        bit.  The encoded windows stay as they are for later ``decode`` / ``align`` calls."""
        o, keep = self._opts(cfg, n, prefix, languages)
        r, bufs, dump = self._result(n, dump_steps)
        self._set_confidences(cfg.confidences)
        if windows is None:
            _lib.check(self.lib.osw_decode_windows(self.ctx, n, C.byref(o), C.byref(r)), "osw_decode_windows")
        else:
            if len(windows) != n:
                raise ValueError("one window index per decoded window")
            idx = np.ascontiguousarray([int(w) for w in windows], dtype=np.int32).reshape(-1)
            if not n:
                idx = np.zeros(1, np.int32)
            _lib.check(self.lib.osw_decode_window_list(self.ctx, n, _i32p(idx), C.byref(o), C.byref(r)),
                       "osw_decode_window_list")
        del keep
        return self._outputs(n, bufs, dump, cfg.confidences)

    def transcribe_batch(self, clips: list, cfg: DecodeConfig, device_pcm: int | None = None,
                         offsets: np.ndarray | None = None) -> list[WindowOutput]:
        if device_pcm is None:
            arrs = [np.asarray(x, dtype=np.int16) for x in clips]
            offs = np.zeros(len(arrs) + 1, np.int64)
            offs[1:] = np.cumsum([len(a) for a in arrs])
            pcm = np.concatenate(arrs)
            ptr, on_dev = pcm.ctypes.data_as(C.c_void_p), 0
        else:
            offs = np.ascontiguousarray(offsets, dtype=np.int64)
            ptr, on_dev = C.c_void_p(device_pcm), 1
        n = len(offs) - 1
        o, keep = self._opts(cfg, n, None)
        r, bufs, dump = self._result(n, 0)
        self._set_confidences(cfg.confidences)
        _lib.check(self.lib.osw_transcribe_batch(self.ctx, ptr, offs.ctypes.data_as(C.POINTER(C.c_int64)), n, on_dev,
                                                 C.byref(o), C.byref(r)), "osw_transcribe_batch")
        del keep
        return self._outputs(n, bufs, dump, cfg.confidences)

    def transcribe_refill(self, clips: list, cfg: DecodeConfig, device_pcm: int | None = None,
                          offsets: np.ndarray | None = None, refill_min: int | None = None) -> list[WindowOutput]:
        """Greedy transcription of window 0 of every clip with row refill
        (osw_transcribe_refill): any number of clips through max_batch decoder rows, a
        finished window's row refilled with the next clip once ``refill_min`` rows are
        free (default ``distributed.REFILL_MIN``).  ``cfg.token_budget``, if given, is per
        clip; the language is detected per clip (``cfg.language_token`` None) or fixed."""
        if refill_min is None:
            from .distributed import REFILL_MIN
            refill_min = REFILL_MIN
        if device_pcm is None:
            arrs = [np.asarray(x, dtype=np.int16) for x in clips]
            offs = np.zeros(len(arrs) + 1, np.int64)
            offs[1:] = np.cumsum([len(a) for a in arrs])
            pcm = np.concatenate(arrs)
            ptr, on_dev = pcm.ctypes.data_as(C.c_void_p), 0
        else:
            offs = np.ascontiguousarray(offsets, dtype=np.int64)
            ptr, on_dev = C.c_void_p(device_pcm), 1
        n = len(offs) - 1
        o, keep = self._opts(cfg, n, None)
        r, bufs, dump = self._result(n, 0)
        self._set_confidences(cfg.confidences)
        _lib.check(self.lib.osw_transcribe_refill(self.ctx, ptr, offs.ctypes.data_as(C.POINTER(C.c_int64)), n, on_dev,
                                                  C.byref(o), C.byref(r), int(refill_min)), "osw_transcribe_refill")
        del keep
        return self._outputs(n, bufs, dump, cfg.confidences)

    # ------------------------------------------------------------ decode sessions
    def session_begin(self, cfg: DecodeConfig, hold: bool = False, retries: int | None = None) -> None:
        """Open a continuous-batching decode session (osw_session_begin): windows added
        with ``session_add`` are admitted into free decoder slots between chunks of
        decoder steps, each with its own clip, seek, prefix and language.  Temperature 0
        only (greedy or beam search, beam_size <= 5); ``cfg.token_budget`` is per window
        (``session_add``), not here.  ``hold`` (osw_session_hold, word timestamps): a window
        ``session_step`` returns keeps its slot and cross-K/V until ``session_align`` or
        ``session_release`` names its tag.  ``retries`` (osw_session_retries; needs ``hold``): the
        ``best_of`` of the session's temperature fallback, 1 to 5; a slot then keeps
        max(beam_size, best_of) decoder rows and ``session_retry`` decodes a held window again."""
        o, keep = self._opts(dataclasses.replace(cfg, token_budget=None), 0, None)
        self._set_confidences(cfg.confidences)  # (the session keeps the setting it begins with)
        self._sess_conf = bool(cfg.confidences)
        _lib.check(self.lib.osw_session_begin(self.ctx, C.byref(o)), "osw_session_begin")
        del keep
        if hold:
            self.session_hold(True)
        if retries is not None:
            self.session_retries(retries)
        self._sess_res = self._result(self.max_batch, 0)
        self._sess_tags = np.zeros(self.max_batch, np.int64)

    def session_add(self, windows: list) -> None:
        """Queue windows: each a dict with ``tag`` (int), ``pcm`` (int16 clip), ``seek``,
        ``segment_size`` (mel frames) and optional ``language_token`` (None: detect),
        ``prefix`` (the <|startofprev|> prompt tokens), ``token_budget`` and ``clip`` (an int
        key >= 0: the clip's log-mel is computed when its first window is added and stays
        resident, so later windows of the key may carry ``pcm=None``; release it with
        ``session_release_clip``)."""
        if not windows:
            return
        empty = np.zeros(0, np.int16)
        arrs = [empty if w.get("pcm") is None else np.asarray(w["pcm"], dtype=np.int16) for w in windows]
        offs = np.zeros(len(arrs) + 1, np.int64)
        offs[1:] = np.cumsum([len(a) for a in arrs])
        pcm = np.concatenate(arrs) if offs[-1] else np.zeros(1, np.int16)
        pres = [np.ascontiguousarray(w.get("prefix") or [0], dtype=np.int32) for w in windows]
        arr = (_lib.osw_session_window * len(windows))()
        for i, w in enumerate(windows):
            lang = w.get("language_token")
            arr[i] = _lib.osw_session_window(
                tag=int(w["tag"]), seek=int(w["seek"]), segment_size=int(w["segment_size"]),
                language_token=-1 if lang is None else int(lang), token_budget=int(w.get("token_budget") or 0),
                n_prefix=len(w.get("prefix") or ()), prefix=_i32p(pres[i]),
                clip=-1 if w.get("clip") is None else int(w["clip"]))
        _lib.check(self.lib.osw_session_add(self.ctx, pcm.ctypes.data_as(C.c_void_p),
                                            offs.ctypes.data_as(C.POINTER(C.c_int64)), len(windows), arr),
                   "osw_session_add")

    def session_step(self, max_chunks: int = 64, refill_min: int = 1):
        """Run decoder chunks until windows finish (at most ``max_chunks`` chunks of 4
        steps).  Returns ([(tag, WindowOutput)], n_active, n_queued)."""
        r, bufs, _ = self._sess_res
        nd, na, nq = C.c_int32(), C.c_int32(), C.c_int32()
        _lib.check(self.lib.osw_session_step(self.ctx, int(max_chunks), int(refill_min), C.byref(r),
                                             self._sess_tags.ctypes.data_as(C.POINTER(C.c_int64)), self.max_batch,
                                             C.byref(nd), C.byref(na), C.byref(nq)), "osw_session_step")
        outs = self._outputs(nd.value, bufs, None, getattr(self, "_sess_conf", False))
        return [(int(self._sess_tags[i]), outs[i]) for i in range(nd.value)], na.value, nq.value

    def session_hold(self, enable: bool = True) -> None:
        """osw_session_hold: only between ``session_begin`` and the first ``session_add``."""
        _lib.check(self.lib.osw_session_hold(self.ctx, 1 if enable else 0), "osw_session_hold")

    def session_align(self, windows: list) -> list:
        """osw_session_align: ``[(tag, AlignWindow)]`` of held windows (``AlignWindow.window`` is
        ignored) -> one ``Alignment`` each, bit for bit ``align``'s after a batched decode; their
        slots are free afterwards.  ``alignment_matrix(i)`` then returns entry i's M."""
        if not windows:
            return []
        tags = np.ascontiguousarray([int(t) for t, _ in windows], dtype=np.int64)
        return self._align([w for _, w in windows], lambda n, arr, res: _lib.check(
            self.lib.osw_session_align(self.ctx, n, tags.ctypes.data_as(C.POINTER(C.c_int64)), arr, res),
            "osw_session_align"))

    def session_retries(self, best_of: int) -> None:
        """osw_session_retries: only in a hold-mode session before its first ``session_add``."""
        _lib.check(self.lib.osw_session_retries(self.ctx, int(best_of)), "osw_session_retries")

    def session_retry(self, entries: list) -> None:
        """osw_session_retry: ``[(tag, temperature, seed, language_token)]`` of held windows.  Each
        decodes again in its slot, from step 0 of the prompt it was admitted with, ``best_of``
        rows sampling at ``temperature`` with ``seed`` (``language_token``: the language attempt 0
        reported; None for an English-only model); ``session_step`` returns it again, held, with the
        best row: bit for bit ``decode``'s result for the window alone at these settings."""
        if not entries:
            return
        arr = (_lib.osw_retry_window * len(entries))()
        for i, (tag, temperature, seed, lang) in enumerate(entries):
            arr[i] = _lib.osw_retry_window(tag=int(tag), temperature=float(temperature),
                                           seed=int(seed) & 0xFFFFFFFFFFFFFFFF,
                                           language_token=-1 if lang is None else int(lang))
        _lib.check(self.lib.osw_session_retry(self.ctx, len(entries), arr), "osw_session_retry")

    def session_release(self, tags) -> None:
        """osw_session_release: free held windows' slots without aligning them."""
        tags = np.ascontiguousarray([int(t) for t in tags], dtype=np.int64)
        if len(tags):
            _lib.check(self.lib.osw_session_release(self.ctx, len(tags), tags.ctypes.data_as(C.POINTER(C.c_int64))),
                       "osw_session_release")

    def session_release_clip(self, clip: int) -> None:
        _lib.check(self.lib.osw_session_release_clip(self.ctx, int(clip)), "osw_session_release_clip")

    def session_end(self) -> None:
        _lib.check(self.lib.osw_session_end(self.ctx), "osw_session_end")

    # ------------------------------------------------------------ word timestamps
    def set_alignment_heads(self, heads: list | None) -> None:
        """The cross-attention heads word timing reads, as (layer, head) pairs; None or
        empty: every head of the last ``n_text_layer // 2`` layers (upstream's default)."""
        pairs = [(int(l), int(h)) for l, h in (heads or [])]
        arr = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1) if pairs else np.zeros(2, np.int32)
        _lib.check(self.lib.osw_set_alignment_heads(self.ctx, _i32p(arr), len(pairs)), "osw_set_alignment_heads")
        self._align_heads = pairs

    def align(self, windows: list) -> list:
        """Cross-attention alignment + DTW (osw_align_windows) of ``AlignWindow``s over the
        cross-K/V resident from the last encode / decode call; one ``Alignment`` each."""
        if not windows:
            return []
        return self._align(windows, lambda n, arr, res: _lib.check(
            self.lib.osw_align_windows(self.ctx, n, arr, res), "osw_align_windows"))

    def _align(self, windows: list, call) -> list:
        st = self.st
        stride = max(len(w.tokens) for w in windows) + 1
        toks = [np.ascontiguousarray(w.tokens if len(w.tokens) else [0], dtype=np.int32) for w in windows]
        arr = (_lib.osw_align_window * len(windows))()
        for i, w in enumerate(windows):
            # an English-only model forces [sot, no_timestamps, tokens..., eot] (language and task < 0)
            arr[i] = _lib.osw_align_window(
                window=int(w.window), sot=st.sot, language=int(w.language) if st.multilingual else -1,
                task=-1 if not st.multilingual else st.transcribe if w.task == "transcribe" else st.translate,
                no_timestamps=st.no_timestamps,
                eot=st.eot, tokens=_i32p(toks[i]), n_tokens=len(w.tokens), num_frames=int(w.num_frames),
                median_filter_width=int(w.median_filter_width))
        tf = np.zeros((len(windows), stride), np.int32)
        tp = np.zeros((len(windows), stride), np.float64)
        res = _lib.osw_align_result(token_frame=_i32p(tf), token_prob=tp.ctypes.data_as(C.POINTER(C.c_double)),
                                    stride=stride)
        call(len(windows), arr, C.byref(res))
        del toks
        return [Alignment(tf[i, :len(w.tokens) + 1].copy() if len(w.tokens) else np.zeros(0, np.int32),
                          tp[i, :len(w.tokens)].copy()) for i, w in enumerate(windows)]

    def alignment_matrix(self, window: int) -> np.ndarray:
        """M [n + 1][F] of ``window`` as the last ``align`` call left it, or of entry ``window`` of
        the last ``session_align`` call (parity tests)."""
        T, F = C.c_int32(), C.c_int32()
        _lib.check(self.lib.osw_get_alignment_matrix(self.ctx, int(window), None, 0, C.byref(T), C.byref(F)),
                   "osw_get_alignment_matrix")
        out = np.empty((T.value, F.value), np.float32)
        if out.size:
            _lib.check(self.lib.osw_get_alignment_matrix(self.ctx, int(window),
                                                         out.ctypes.data_as(C.POINTER(C.c_float)), out.size,
                                                         C.byref(T), C.byref(F)), "osw_get_alignment_matrix")
        return out

    def debug_dtw(self, x: np.ndarray):
        """The DTW kernel alone on a cost matrix x [T][F]: (text_indices, time_indices)."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        T, F = x.shape
        ti = np.zeros(T + F, np.int32)
        fi = np.zeros(T + F, np.int32)
        n = C.c_int32()
        _lib.check(self.lib.osw_debug_dtw(self.ctx, x.ctypes.data_as(C.POINTER(C.c_float)), T, F, _i32p(ti),
                                          _i32p(fi), C.byref(n)), "osw_debug_dtw")
        return ti[:n.value].copy(), fi[:n.value].copy()

    def debug_align_post(self, scores: np.ndarray, length, head, frames, width):
        """launch_align_post alone (osw_debug_align_post): scores fp32 [slots][heads][pstride][TK], one
        len / head / frames / width per slot.  Returns (stats [slots][heads][pstride][2], colstats
        [slots][heads][TK][2], M [slots][pstride][TK]); what the kernels did not write holds 0xff bytes."""
        s = np.ascontiguousarray(scores, dtype=np.float32)
        n_slots, n_heads, pstride, TK = s.shape
        meta = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (length, head, frames, width)]
        if any(a.shape != (n_slots,) for a in meta):
            raise ValueError("one len, head, frames and width per slot")
        stats = np.empty((n_slots, n_heads, pstride, 2), np.float32)
        cs = np.empty((n_slots, n_heads, TK, 2), np.float32)
        M = np.empty((n_slots, pstride, TK), np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(self.lib.osw_debug_align_post(self.ctx, s.ctypes.data_as(fp), n_slots, n_heads, pstride, TK,
                                                 *[_i32p(a) for a in meta], stats.ctypes.data_as(fp),
                                                 cs.ctypes.data_as(fp), M.ctypes.data_as(fp)), "osw_debug_align_post")
        return stats, cs, M

    def debug_align_tail(self, logits: np.ndarray, eot: int, pos: int, slot, length, head, forced: np.ndarray,
                         token_logprob: np.ndarray, cur_tok, done):
        """launch_align_tail alone (osw_debug_align_tail): logits fp32 [rows][V], forced [rows][ctx],
        token_logprob [slots][ctx].  Returns copies (token_logprob, cur_tok, done) as the launch left them."""
        lg = np.ascontiguousarray(logits, dtype=np.float32)
        rows, V = lg.shape
        f = np.ascontiguousarray(forced, dtype=np.int32)
        lp = np.array(token_logprob, dtype=np.float32, order="C", ndmin=2)
        ctx = f.shape[1]
        per_row = [np.ascontiguousarray(a, dtype=np.int32).reshape(-1) for a in (slot, length, head)]
        ct = np.array(cur_tok, dtype=np.int32, order="C").reshape(-1)
        dn = np.array(done, dtype=np.int32, order="C").reshape(-1)
        if f.shape != (rows, ctx) or lp.shape[1] != ctx or any(a.shape != (rows,) for a in per_row + [ct, dn]):
            raise ValueError("shapes: logits [rows][V], forced [rows][ctx], token_logprob [slots][ctx], the rest [rows]")
        fp = C.POINTER(C.c_float)
        _lib.check(self.lib.osw_debug_align_tail(self.ctx, lg.ctypes.data_as(fp), rows, V, int(eot), ctx, int(pos),
                                                 *[_i32p(a) for a in per_row], _i32p(f), lp.shape[0],
                                                 lp.ctypes.data_as(fp), _i32p(ct), _i32p(dn)), "osw_debug_align_tail")
        return lp, ct, dn

    def debug_align_self_attn(self, qkv_slabs: np.ndarray, bias: np.ndarray, kcache: np.ndarray, vcache: np.ndarray,
                              pos: int, done):
        """launch_align_self_attn alone (osw_debug_align_self_attn): qkv_slabs fp32 [ks][rows][3D], bias
        [3D], fp32 caches [rows][H][ctx][64], done [rows].  Returns (out fp32 [rows][D] = hi + lo, NaN
        where nothing was written, kcache, vcache), the caches as the kernel left them (copies)."""
        q = np.ascontiguousarray(qkv_slabs, dtype=np.float32)
        ks, rows, D3 = q.shape
        kc = np.array(kcache, dtype=np.float32, order="C")
        vc = np.array(vcache, dtype=np.float32, order="C")
        b = np.ascontiguousarray(bias, dtype=np.float32)
        dn = np.ascontiguousarray(done, dtype=np.int32).reshape(-1)
        H, ctx = kc.shape[1:3]
        if D3 != 3 * 64 * H or kc.shape != (rows, H, ctx, 64) or vc.shape != kc.shape or b.shape != (D3,) or \
                dn.shape != (rows,):
            raise ValueError("shapes: qkv [ks][rows][3D], bias [3D], caches [rows][H][ctx][64], done [rows]")
        out = np.empty((rows, 64 * H), np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(self.lib.osw_debug_align_self_attn(self.ctx, q.ctypes.data_as(fp), ks, b.ctypes.data_as(fp),
                                                      kc.ctypes.data_as(fp), vc.ctypes.data_as(fp), rows, H, ctx,
                                                      int(pos), _i32p(dn), out.ctypes.data_as(fp)),
                   "osw_debug_align_self_attn")
        return out, kc, vc

    def debug_align_scores(self, q_slabs: np.ndarray, bias, K: np.ndarray, layer_heads, n_heads: int, pos: int,
                           slot, length, scores: np.ndarray) -> np.ndarray:
        """launch_align_scores alone (osw_debug_align_scores): q_slabs fp32 [ks][rows][D], bias [D] or
        None, K fp16 [rows][H][T][64], layer_heads pairs (head, head_idx), scores fp32
        [slots][n_heads][pstride][T].  Returns a copy of scores as the launch left it."""
        q = np.ascontiguousarray(q_slabs, dtype=np.float32)
        K = np.ascontiguousarray(K, dtype=np.float16)
        ks, rows, Dm = q.shape
        H, T = K.shape[1:3]
        lh = np.ascontiguousarray(layer_heads, dtype=np.int32).reshape(-1, 2)
        sc = np.array(scores, dtype=np.float32, order="C")
        sl = np.ascontiguousarray(slot, dtype=np.int32).reshape(-1)
        ln = np.ascontiguousarray(length, dtype=np.int32).reshape(-1)
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        if K.shape != (rows, H, T, 64) or Dm != 64 * H or sc.ndim != 4 or sc.shape[1] != n_heads or sc.shape[3] != T or \
                sl.shape != (rows,) or ln.shape != (rows,) or (b is not None and b.shape != (Dm,)):
            raise ValueError("shapes: q [ks][rows][D], K [rows][H][T][64], scores [slots][n_heads][pstride][T]")
        fp = C.POINTER(C.c_float)
        _lib.check(self.lib.osw_debug_align_scores(self.ctx, q.ctypes.data_as(fp), ks,
                                                   None if b is None else b.ctypes.data_as(fp),
                                                   K.ctypes.data_as(C.c_void_p), rows, H, T, _i32p(lh), len(lh),
                                                   int(n_heads), int(pos), _i32p(sl), _i32p(ln), sc.shape[2],
                                                   sc.shape[0], sc.ctypes.data_as(fp)), "osw_debug_align_scores")
        return sc

    def debug_history_rules(self, logits: np.ndarray, tokens: np.ndarray, n_hist, repetition_penalty: float = 1.0,
                            no_repeat_ngram_size: int = 0) -> np.ndarray:
        """The history-rules kernel alone: logits [rows][V] with row r's history
        ``tokens[r, :n_hist[r]]``; returns the processed logits (the input is not changed)."""
        x = np.array(logits, dtype=np.float32, order="C", ndmin=2)
        t = np.ascontiguousarray(np.atleast_2d(tokens), dtype=np.int32)
        n = np.ascontiguousarray(n_hist, dtype=np.int32).reshape(-1)
        if t.shape[0] != x.shape[0] or n.shape[0] != x.shape[0]:
            raise ValueError("one history and one length per logits row")
        _lib.check(self.lib.osw_debug_history_rules(self.ctx, x.ctypes.data_as(C.POINTER(C.c_float)), x.shape[0],
                                                    x.shape[1], _i32p(t), t.shape[1], _i32p(n),
                                                    float(repetition_penalty), int(no_repeat_ngram_size)),
                   "osw_debug_history_rules")
        return x

    SELECT_MODES = {"batch": 0, "refill": 1, "session": 2}

    def debug_select_step(self, cfg: DecodeConfig, state: dict, mode: str = "batch", n_prefix: int = 0,
                          rows_per_slot: int | None = None, row_inv_temp=None, row_seed=None) -> dict:
        """One selection step (select kernel, and the beam update for ``cfg.beam_size`` > 1) on the
        caller's logits and state (osw_debug_select_step).  ``state`` maps the names of
        ``_lib.osw_select_io.ARRAYS`` to arrays: ``logits`` [rows][V], ``pos`` [1] or [rows],
        ``state`` [rows] of ``SEL_STATE``, ``prompt`` [rows][pstride], ``cur_tok`` [rows], ``tokens``
        [rows][max_tok], optionally ``budget`` [rows]; beam: ``anc`` [rows][n_text_ctx], ``bwin``
        [windows] of ``BEAM_WIN``, ``best_tok`` [windows][max_tok]; with ``cfg.confidences``
        ``lp_hist``, ``best_lp``, ``lang_probs``.  Returns copies as the step left them, plus
        ``counters`` (the context's arrival and ticket counters); the input is not changed.
        ``rows_per_slot`` with ``row_inv_temp`` / ``row_seed`` [rows] (osw_debug_select_step_rows,
        session mode): the step of a retry session with that many rows per window slot."""
        self._set_confidences(cfg.confidences)
        cfg = dataclasses.replace(cfg, token_budget=None)
        o, keep = self._opts(cfg, 0, None)
        out = {}
        io = _lib.osw_select_io()
        for name in _lib.osw_select_io.ARRAYS:
            a = state.get(name)
            if name == "counters":
                a = np.full(1 + len(state["state"]), -1, np.int32)
            if a is None:
                continue
            if name in ("state", "bwin"):
                a = np.array(a, dtype=SEL_STATE if name == "state" else BEAM_WIN, order="C")
                words = a.view(np.int32)
            else:
                a = np.array(a, dtype=np.float32 if name in _lib.osw_select_io.FLOAT else np.int32, order="C")
                words = a
            out[name] = a
            setattr(io, name, words.ctypes.data_as(type(getattr(io, name))))
            setattr(io, name + "_len", words.size)
        io.mode = self.SELECT_MODES[mode]
        io.n_prefix = int(n_prefix)
        io.rows = len(out["state"])
        io.max_tok = out["tokens"].shape[1]
        io.pstride = out["prompt"].shape[1]
        if rows_per_slot is None:
            _lib.check(self.lib.osw_debug_select_step(self.ctx, C.byref(o), C.byref(io)), "osw_debug_select_step")
        else:
            rit = np.ascontiguousarray(row_inv_temp, dtype=np.float32)
            rsd = np.ascontiguousarray(row_seed, dtype=np.uint64)
            if len(rit) != io.rows or len(rsd) != io.rows:
                raise ValueError("row_inv_temp / row_seed need one entry per row")
            _lib.check(self.lib.osw_debug_select_step_rows(
                self.ctx, C.byref(o), C.byref(io), int(rows_per_slot), rit.ctypes.data_as(C.POINTER(C.c_float)),
                rsd.ctypes.data_as(C.POINTER(C.c_uint64))), "osw_debug_select_step_rows")
        del keep
        return out

    def debug_history_rules_time(self, rows: int, n_hist: int, repetition_penalty: float = 1.0,
                                 no_repeat_ngram_size: int = 0, iters: int = 200) -> float:
        """Mean microseconds per launch of the history-rules kernel on ``rows`` rows of the
        model's vocabulary, each with ``n_hist`` tokens of history (HIP events)."""
        us = C.c_float()
        _lib.check(self.lib.osw_debug_history_rules_time(self.ctx, int(rows), self.dims.n_vocab, int(n_hist),
                                                         float(repetition_penalty), int(no_repeat_ngram_size),
                                                         int(iters), C.byref(us)), "osw_debug_history_rules_time")
        return us.value

    def debug_gemm(self, A: np.ndarray, W: np.ndarray, variant: int = 0, iters: int = 1):
        """C = A·Wᵀ (fp16 in, fp32 out) through one GEMM kernel variant; returns (C, mean ms)."""
        A = np.ascontiguousarray(A, dtype=np.float16)
        W = np.ascontiguousarray(W, dtype=np.float16)
        M, K = A.shape
        N = W.shape[0]
        out = np.empty((M, N), np.float32)
        ms = C.c_float()
        _lib.check(self.lib.osw_debug_gemm(self.ctx, M, N, K, variant, A.ctypes.data_as(C.c_void_p),
                                           W.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.POINTER(C.c_float)),
                                           iters, C.byref(ms)), "osw_debug_gemm")
        return out, ms.value

    ATTN_AUTO = 0

    @staticmethod
    def attn_form(eager: bool = False, qb128: bool = False, pipe: bool = False) -> int:
        """An explicit encoder-attention form for debug_enc_attn (osw.h OSW_ATTN_FORM*)."""
        return 1 | (2 if eager else 0) | (4 if qb128 else 0) | (8 if pipe else 0)

    def debug_enc_attn(self, qkv: np.ndarray, form: int = 0) -> np.ndarray:
        """One encoder-attention launch: qkv fp16 [3][nb][H][T][64] -> fp16 [nb*T][H*64], T the
        engine's n_audio_ctx (1500 at the 30 s default window)."""
        qkv = np.ascontiguousarray(qkv, dtype=np.float16)
        three, nb, H, T, hd = qkv.shape
        if (three, T, hd) != (3, self.dims.n_audio_ctx, 64):
            raise ValueError(f"qkv must be [3][nb][H][{self.dims.n_audio_ctx}][64]")
        out = np.empty((nb * T, H * hd), np.float16)
        _lib.check(self.lib.osw_debug_enc_attn(self.ctx, qkv.ctypes.data_as(C.c_void_p), nb, H, int(form),
                                               out.ctypes.data_as(C.c_void_p)), "osw_debug_enc_attn")
        return out

    def debug_dec_xattn(self, q_slabs: np.ndarray, bias, K: np.ndarray, V: np.ndarray, beam: int = 1,
                        legacy: bool | int = False) -> np.ndarray:
        """One decoder cross-attention launch: q_slabs fp32 [ks][rows][D], bias [D] or None, K and V
        fp16 [W][H][T][64] (T the engine's n_audio_ctx), rows = W * beam -> fp32 [rows][D] (the hi + lo
        halves summed).  ``legacy``: False / 0 the chunk kernels the decoder launches, True / 1 one
        workgroup per (row, head), 2 the chunk kernels' full-width forms (6 keys per lane, 3 key tiles
        per wave) whatever T is."""
        q = np.ascontiguousarray(q_slabs, dtype=np.float32)
        K = np.ascontiguousarray(K, dtype=np.float16)
        V = np.ascontiguousarray(V, dtype=np.float16)
        ks, rows, Dm = q.shape
        W, H = K.shape[:2]
        if K.shape != (W, H, self.dims.n_audio_ctx, 64) or V.shape != K.shape or Dm != self.dims.n_text_state or \
                H != self.dims.n_text_head or rows != W * beam:
            raise ValueError("shapes: q [ks][W*beam][D], K/V [W][H][n_audio_ctx][64] with the engine's H and D")
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        if b is not None and b.shape != (Dm,):
            raise ValueError("bias must be [D]")
        out = np.empty((rows, Dm), np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(self.lib.osw_debug_dec_xattn(self.ctx, q.ctypes.data_as(fp), ks,
                                                None if b is None else b.ctypes.data_as(fp),
                                                K.ctypes.data_as(C.c_void_p), V.ctypes.data_as(C.c_void_p), rows,
                                                int(beam), int(legacy), out.ctypes.data_as(fp)),
                   "osw_debug_dec_xattn")
        return out

    def debug_dec_xattn_windows(self, q_slabs: np.ndarray, bias, K: np.ndarray, V: np.ndarray, window_map,
                                beam: int = 1, legacy: bool | int = False) -> np.ndarray:
        """``debug_dec_xattn`` with a window map (osw_debug_dec_xattn_windows): K and V fp16
        [kv_windows][H][T][64], q_slabs fp32 [ks][len(window_map) * beam][D]; row group w
        attends window ``window_map[w]``."""
        q = np.ascontiguousarray(q_slabs, dtype=np.float32)
        K = np.ascontiguousarray(K, dtype=np.float16)
        V = np.ascontiguousarray(V, dtype=np.float16)
        wm = np.ascontiguousarray([int(w) for w in window_map], dtype=np.int32).reshape(-1)
        ks, rows, Dm = q.shape
        KW, H = K.shape[:2]
        if K.shape != (KW, H, self.dims.n_audio_ctx, 64) or V.shape != K.shape or Dm != self.dims.n_text_state or \
                H != self.dims.n_text_head or rows != len(wm) * beam:
            raise ValueError("shapes: q [ks][len(window_map)*beam][D], K/V [kv_windows][H][n_audio_ctx][64] with the "
                             "engine's H and D")
        b = None if bias is None else np.ascontiguousarray(bias, dtype=np.float32)
        if b is not None and b.shape != (Dm,):
            raise ValueError("bias must be [D]")
        out = np.empty((rows, Dm), np.float32)
        fp = C.POINTER(C.c_float)
        mp = _i32p(wm if len(wm) else np.zeros(1, np.int32))
        _lib.check(self.lib.osw_debug_dec_xattn_windows(self.ctx, q.ctypes.data_as(fp), ks,
                                                        None if b is None else b.ctypes.data_as(fp),
                                                        K.ctypes.data_as(C.c_void_p), V.ctypes.data_as(C.c_void_p),
                                                        KW, mp, rows, int(beam), int(legacy),
                                                        out.ctypes.data_as(fp)), "osw_debug_dec_xattn_windows")
        return out

    def debug_dec_self_attn(self, qkv_slabs: np.ndarray, bias: np.ndarray, kcache: np.ndarray, vcache: np.ndarray,
                            pos, ancestry: np.ndarray | None = None, group: int = 1):
        """One decoder self-attention launch: qkv_slabs fp32 [ks][rows][3D], bias [3D], caches fp16
        [rows][H][ctx][64], pos an int or one per row, ancestry [rows][ctx] or None.  Returns
        (out fp32 [rows][D], kcache, vcache) with the caches as the kernel left them (copies)."""
        q = np.ascontiguousarray(qkv_slabs, dtype=np.float32)
        ks, rows, D3 = q.shape
        H, ctx, Dm = self.dims.n_text_head, self.dims.n_text_ctx, self.dims.n_text_state
        kc = np.array(kcache, dtype=np.float16, order="C")
        vc = np.array(vcache, dtype=np.float16, order="C")
        b = np.ascontiguousarray(bias, dtype=np.float32)
        if D3 != 3 * Dm or kc.shape != (rows, H, ctx, 64) or vc.shape != kc.shape or b.shape != (3 * Dm,):
            raise ValueError("shapes: qkv [ks][rows][3D], bias [3D], caches [rows][H][ctx][64]")
        per_row = not np.isscalar(pos)
        p = np.ascontiguousarray(np.atleast_1d(pos), dtype=np.int32)
        if per_row and p.shape != (rows,):
            raise ValueError("one position per row")
        anc = None
        if ancestry is not None:
            anc = np.ascontiguousarray(ancestry, dtype=np.int32)
            if anc.shape != (rows, ctx):
                raise ValueError("ancestry must be [rows][ctx]")
        out = np.empty((rows, Dm), np.float32)
        fp = C.POINTER(C.c_float)
        _lib.check(self.lib.osw_debug_dec_self_attn(self.ctx, q.ctypes.data_as(fp), ks, b.ctypes.data_as(fp),
                                                    kc.ctypes.data_as(C.c_void_p), vc.ctypes.data_as(C.c_void_p),
                                                    rows, _i32p(p), int(per_row), None if anc is None else _i32p(anc),
                                                    int(group), out.ctypes.data_as(fp)), "osw_debug_dec_self_attn")
        return out, kc, vc

    DEBUG_GUARD = 256  # floats of guard band behind every fp32 result of the debug_dec_* calls

    @staticmethod
    def _guarded(raw: np.ndarray, shape) -> np.ndarray:
        """The result part of a debug call's output; raises if the guard band behind it was written."""
        n = int(np.prod(shape))
        if not (raw[n:].view(np.uint32) == 0xFFFFFFFF).all():
            raise AssertionError("a kernel wrote past its result (guard band changed)")
        return raw[:n].reshape(shape).copy()

    def debug_dec_gemm(self, form: int, A_hi: np.ndarray, A_lo, W: np.ndarray, use_wf: bool = False) -> np.ndarray:
        """(A_hi + A_lo)·Wᵀ through a decoder GEMM launcher (osw_debug_dec_gemm): fp16 A_hi, A_lo [M][K]
        (A_lo None: one operand), W [N][K].  form 0 / 1: fp32 slabs [ks][M][N] of the skinny / tiled
        split-K launcher; form 2: the logits route's [M][N].  An element the kernel did not write is NaN."""
        A_hi = np.ascontiguousarray(A_hi, dtype=np.float16)
        W = np.ascontiguousarray(W, dtype=np.float16)
        lo = None if A_lo is None else np.ascontiguousarray(A_lo, dtype=np.float16)
        M, K = A_hi.shape
        N = W.shape[0]
        if W.shape != (N, K) or (lo is not None and lo.shape != (M, K)):
            raise ValueError("shapes: A_hi, A_lo [M][K], W [N][K]")
        # the launcher chooses the split (at most K / 64 slabs); what lies behind the result is guard band
        raw = np.empty((1 if form == 2 else max(K // 64, 1)) * M * N + self.DEBUG_GUARD, np.float32)
        ks = C.c_int32()
        vp = C.c_void_p
        _lib.check(self.lib.osw_debug_dec_gemm(self.ctx, int(form), M, N, K, A_hi.ctypes.data_as(vp),
                                               None if lo is None else lo.ctypes.data_as(vp), W.ctypes.data_as(vp),
                                               int(bool(use_wf)), raw.ctypes.data_as(C.POINTER(C.c_float)), raw.size,
                                               C.byref(ks)), "osw_debug_dec_gemm")
        return self._guarded(raw, (M, N) if form == 2 else (ks.value, M, N))

    def debug_dec_gemm_q8(self, form: int, A_hi: np.ndarray, A_lo: np.ndarray, q: np.ndarray, mult: np.ndarray,
                          use_q8_stream: bool = True) -> np.ndarray:
        """debug_dec_gemm on int8 weights (osw_debug_dec_gemm_quant): q int8 [N][K], mult float32 [N].
        use_q8_stream: the skinny kernel streams the int8 fragments; else the fp16(q) copy with the
        multipliers through the same launcher.  Forms 3 / 4 (the opt-in tails) are refused."""
        A_hi = np.ascontiguousarray(A_hi, dtype=np.float16)
        lo = np.ascontiguousarray(A_lo, dtype=np.float16)
        q = np.asarray(q)
        if q.dtype != np.int8:
            raise ValueError("q must be int8")
        q = np.ascontiguousarray(q)
        m = np.ascontiguousarray(mult, dtype=np.float32)
        M, K = A_hi.shape
        N = q.shape[0]
        if q.shape != (N, K) or lo.shape != (M, K) or m.shape != (N,):
            raise ValueError("shapes: A_hi, A_lo [M][K], q [N][K], mult [N]")
        raw = np.empty((1 if form == 2 else max(K // 64, 1)) * M * N + self.DEBUG_GUARD, np.float32)
        ks = C.c_int32()
        vp = C.c_void_p
        _lib.check(self.lib.osw_debug_dec_gemm_quant(self.ctx, int(form), M, N, K, A_hi.ctypes.data_as(vp),
                                                  lo.ctypes.data_as(vp), q.ctypes.data_as(vp),
                                                  m.ctypes.data_as(C.POINTER(C.c_float)), int(bool(use_q8_stream)),
                                                  raw.ctypes.data_as(C.POINTER(C.c_float)), raw.size, C.byref(ks)),
                   "osw_debug_dec_gemm_quant")
        return self._guarded(raw, (M, N) if form == 2 else (ks.value, M, N))

    def debug_dec_gemm_time(self, A_hi, A_lo, q, mult, copies: int = 1, warm: int = 20, launches: int = 200):
        """Per-launch microseconds of the skinny split-K projection with float16 and with int8 weights,
        alternating (osw_debug_dec_gemm_time) -> (us_f16 [launches], us_q8 [launches])."""
        A_hi = np.ascontiguousarray(A_hi, dtype=np.float16)
        lo = np.ascontiguousarray(A_lo, dtype=np.float16)
        q = np.ascontiguousarray(q, dtype=np.int8)
        m = np.ascontiguousarray(mult, dtype=np.float32)
        (M, K), N = A_hi.shape, q.shape[0]
        if q.shape != (N, K) or lo.shape != (M, K) or m.shape != (N,):
            raise ValueError("shapes: A_hi, A_lo [M][K], q [N][K], mult [N]")
        a, b = np.zeros(launches, np.float32), np.zeros(launches, np.float32)
        vp, fp = C.c_void_p, C.POINTER(C.c_float)
        _lib.check(self.lib.osw_debug_dec_gemm_time(self.ctx, M, N, K, A_hi.ctypes.data_as(vp), lo.ctypes.data_as(vp),
                                                    q.ctypes.data_as(vp), m.ctypes.data_as(fp), int(copies), int(warm),
                                                    int(launches), a.ctypes.data_as(fp), b.ctypes.data_as(fp)),
                   "osw_debug_dec_gemm_time")
        return a, b

    def debug_logits_profile(self):
        """(ms, launches) of the fused step's logits GEMM since set_profiling(True, eager_decode=True)."""
        ms, n = C.c_double(), C.c_int64()
        _lib.check(self.lib.osw_debug_logits_profile(self.ctx, C.byref(ms), C.byref(n)), "osw_debug_logits_profile")
        return ms.value, n.value

    def debug_dec_resln(self, x, gain, shift, slabs=None, bias=None, embed=None, W=None, direct: bool = False,
                        use_wf: bool = False):
        """Residual update + LayerNorm (osw_debug_dec_resln).  x fp32 [rows][D]; slabs fp32 [ks][rows][D]
        with bias [D] or None, or embed = (tok_emb fp16 [V][D], pos_emb fp32 [ctx][D], tok [rows], pos, pos_row)
        for the embedding entry (pos [rows] when pos_row else one position).
        W None: the standalone kernel; returns (x', y_hi, y_lo).
        W fp16 [N][D]: the fused PRO_RESLN GEMM (one row); returns (x', out, x_after) with out the slabs
        [ks][rows][N], or with direct C [rows][N], and x_after the input buffer as the kernel left it."""
        x = np.array(x, dtype=np.float32, order="C")
        rows, Dm = x.shape
        fp, vp = C.POINTER(C.c_float), C.c_void_p
        g = np.ascontiguousarray(gain, dtype=np.float32)
        b = np.ascontiguousarray(shift, dtype=np.float32)
        if g.shape != (Dm,) or b.shape != (Dm,):
            raise ValueError("gain and shift must be [D]")
        s = bi = te = pe = tk = ps = None
        ks = ctx = V = pos_row = 0
        if embed is None:
            s = np.ascontiguousarray(slabs, dtype=np.float32)
            ks = s.shape[0]
            if s.shape != (ks, rows, Dm):
                raise ValueError("slabs must be [ks][rows][D]")
            if bias is not None:
                bi = np.ascontiguousarray(bias, dtype=np.float32)
                if bi.shape != (Dm,):
                    raise ValueError("bias must be [D]")
        else:
            te, pe, tk, ps, pos_row = embed
            te = np.ascontiguousarray(te, dtype=np.float16)
            pe = np.ascontiguousarray(pe, dtype=np.float32)
            tk = np.ascontiguousarray(tk, dtype=np.int32)
            ps = np.ascontiguousarray(np.atleast_1d(ps), dtype=np.int32)
            V, ctx = te.shape[0], pe.shape[0]
            if te.shape != (V, Dm) or pe.shape != (ctx, Dm) or tk.shape != (rows,) or \
                    ps.shape != ((rows,) if pos_row else (1,)):
                raise ValueError("embed: tok_emb [V][D], pos_emb [ctx][D], tok [rows], pos [rows] or one")
        ptr = lambda a, t: None if a is None else a.ctypes.data_as(t)
        x_out = np.empty_like(x)
        kso = C.c_int32()
        if W is None:
            hi, lo = np.empty((rows, Dm), np.float16), np.empty((rows, Dm), np.float16)
            _lib.check(self.lib.osw_debug_dec_resln(self.ctx, 0, 0, rows, Dm, ptr(s, fp), ks, ptr(bi, fp), ptr(x, fp),
                                                    ptr(g, fp), ptr(b, fp), ptr(te, vp), ptr(pe, fp),
                                                    None if tk is None else _i32p(tk),
                                                    None if ps is None else _i32p(ps), ctx, V, int(bool(pos_row)),
                                                    None, 0, 0, ptr(x_out, fp), ptr(hi, vp), ptr(lo, vp), None, 0,
                                                    C.byref(kso)), "osw_debug_dec_resln")
            return x_out, hi, lo
        W = np.ascontiguousarray(W, dtype=np.float16)
        N = W.shape[0]
        if W.shape != (N, Dm):
            raise ValueError("W must be [N][D]")
        raw = np.empty((1 if direct else max(Dm // 64, 1)) * rows * N + self.DEBUG_GUARD, np.float32)
        _lib.check(self.lib.osw_debug_dec_resln(self.ctx, 1, int(bool(direct)), rows, Dm, ptr(s, fp), ks, ptr(bi, fp),
                                                ptr(x, fp), ptr(g, fp), ptr(b, fp), ptr(te, vp), ptr(pe, fp),
                                                None if tk is None else _i32p(tk), None if ps is None else _i32p(ps),
                                                ctx, V, int(bool(pos_row)), ptr(W, vp), N, int(bool(use_wf)),
                                                ptr(x_out, fp), None, None, ptr(raw, fp), raw.size, C.byref(kso)),
                   "osw_debug_dec_resln")
        return x_out, self._guarded(raw, (rows, N) if direct else (kso.value, rows, N)), x

    def debug_dec_gelu(self, slabs, bias, W=None, use_wf: bool = False):
        """GELU reduce gelu(bias + Σ slabs) (osw_debug_dec_gelu): slabs fp32 [ks][M][K4], bias [K4].
        W None: the standalone kernel, returns the fp16 pair (y_hi, y_lo) [M][K4]; W fp16 [N][K4]: the
        fused PRO_GELU GEMM, returns its slabs [ks'][M][N]."""
        s = np.ascontiguousarray(slabs, dtype=np.float32)
        ks, M, K4 = s.shape
        bi = np.ascontiguousarray(bias, dtype=np.float32)
        if bi.shape != (K4,):
            raise ValueError("bias must be [K4]")
        fp, vp = C.POINTER(C.c_float), C.c_void_p
        kso = C.c_int32()
        if W is None:
            hi, lo = np.empty((M, K4), np.float16), np.empty((M, K4), np.float16)
            _lib.check(self.lib.osw_debug_dec_gelu(self.ctx, 0, M, K4, s.ctypes.data_as(fp), ks, bi.ctypes.data_as(fp),
                                                   None, 0, 0, hi.ctypes.data_as(vp), lo.ctypes.data_as(vp), None, 0,
                                                   C.byref(kso)), "osw_debug_dec_gelu")
            return hi, lo
        W = np.ascontiguousarray(W, dtype=np.float16)
        N = W.shape[0]
        if W.shape != (N, K4):
            raise ValueError("W must be [N][K4]")
        raw = np.empty(max(K4 // 64, 1) * M * N + self.DEBUG_GUARD, np.float32)
        _lib.check(self.lib.osw_debug_dec_gelu(self.ctx, 1, M, K4, s.ctypes.data_as(fp), ks, bi.ctypes.data_as(fp),
                                               W.ctypes.data_as(vp), N, int(bool(use_wf)), None, None,
                                               raw.ctypes.data_as(fp), raw.size, C.byref(kso)), "osw_debug_dec_gelu")
        return self._guarded(raw, (kso.value, M, N))

    EPI_F16, EPI_F16_GELU, EPI_F32_RESID, EPI_F32_GELU_POS, EPI_F32, EPI_HEADS = range(6)

    def debug_enc_gemm(self, A: np.ndarray, W: np.ndarray, Cbuf: np.ndarray, *, M: int, epi: int, variant: int = 0,
                       lda: int | None = None, a_grp_rows: int | None = None, a_grp_stride: int = 0,
                       ldc: int | None = None, c_grp_rows: int | None = None, c_grp_stride: int = 0,
                       c_offset: int = 0, bias=None, pos=None, heads=None, heads_slot=None) -> np.ndarray:
        """One tiled encoder GEMM launch with the full argument set (osw_debug_enc_gemm): A a flat fp16
        buffer whose row m starts at (m // a_grp_rows) * a_grp_stride + (m % a_grp_rows) * lda, W fp16
        [N][K], Cbuf the whole output buffer (fp16 for EPI_F16 / EPI_F16_GELU / EPI_HEADS, fp32 for the
        others) as it is before the launch; returns a copy of it as the kernel left it.  heads =
        (heads_T, heads_H, heads_nb) for EPI_HEADS.  The library checks every precondition; this wrapper
        only the sizes of the host arrays it hands over."""
        A = np.ascontiguousarray(A, dtype=np.float16).ravel()
        W = np.ascontiguousarray(W, dtype=np.float16)
        N, K = W.shape
        f16 = epi in (self.EPI_F16, self.EPI_F16_GELU, self.EPI_HEADS)
        out = np.array(Cbuf, dtype=np.float16 if f16 else np.float32, order="C").ravel()
        fp = C.POINTER(C.c_float)
        d = _lib.osw_enc_gemm_desc()
        d.M, d.N, d.K, d.variant, d.epi = int(M), N, K, int(variant), int(epi)
        d.heads_T, d.heads_H, d.heads_nb = (int(v) for v in (heads or (0, 0, 0)))
        d.lda = K if lda is None else int(lda)
        d.a_grp_rows = int(M) if a_grp_rows is None else int(a_grp_rows)
        d.a_grp_stride = int(a_grp_stride)
        d.a_count = A.size
        d.ldc = (0 if epi == self.EPI_HEADS else N) if ldc is None else int(ldc)
        d.c_grp_rows = int(M) if c_grp_rows is None else int(c_grp_rows)
        d.c_grp_stride, d.c_offset, d.c_bytes = int(c_grp_stride), int(c_offset), out.nbytes
        d.A, d.W, d.C = A.ctypes.data, W.ctypes.data, out.ctypes.data
        keep = [A, W, out]
        if bias is not None:
            b = np.ascontiguousarray(bias, dtype=np.float32)
            if b.shape != (N,):
                raise ValueError("bias must be [N]")
            d.bias = b.ctypes.data_as(fp)
            keep.append(b)
        if pos is not None:
            p = np.ascontiguousarray(pos, dtype=np.float32)
            d.pos, d.pos_count = p.ctypes.data_as(fp), p.size
            keep.append(p)
        if heads_slot is not None:
            sl = np.ascontiguousarray(heads_slot, dtype=np.int32)
            if d.heads_T < 1 or sl.shape != (int(M) // d.heads_T,):
                raise ValueError("heads_slot must hold one slot per window")
            d.heads_slot = _i32p(sl)
            keep.append(sl)
        _lib.check(self.lib.osw_debug_enc_gemm(self.ctx, C.byref(d)), "osw_debug_enc_gemm")
        return out

    def debug_enc_layernorm(self, x: np.ndarray, gain, shift, y: np.ndarray) -> np.ndarray:
        """The encoder's LayerNorm (osw_debug_enc_layernorm) on x fp32 [M][D]: y fp16 [M_alloc][D] is the
        output buffer as it is before the launch (M_alloc >= M); returns a copy as the kernel left it."""
        x = np.ascontiguousarray(x, dtype=np.float32)
        M, Dm = x.shape
        g = np.ascontiguousarray(gain, dtype=np.float32)
        b = np.ascontiguousarray(shift, dtype=np.float32)
        out = np.array(y, dtype=np.float16, order="C")
        if g.shape != (Dm,) or b.shape != (Dm,) or out.ndim != 2 or out.shape[1] != Dm:
            raise ValueError("shapes: x [M][D], gain and shift [D], y [M_alloc][D]")
        fp = C.POINTER(C.c_float)
        _lib.check(self.lib.osw_debug_enc_layernorm(self.ctx, M, out.shape[0], Dm, x.ctypes.data_as(fp),
                                                    g.ctypes.data_as(fp), b.ctypes.data_as(fp),
                                                    out.ctypes.data_as(C.c_void_p)), "osw_debug_enc_layernorm")
        return out

    def debug_get_logmel(self, clip: int) -> tuple[np.ndarray, np.float32]:
        """The raw fp32 log10 mel of a clip of the last log_mel, time-major [n_frames][n_mels], as the
        kernel stored it, and the clip's maximum as the kernels read it (osw_debug_get_logmel)."""
        out = np.empty((self._nframes[clip], self.dims.n_mels), np.float32)
        mx = C.c_float()
        _lib.check(self.lib.osw_debug_get_logmel(self.ctx, int(clip), out.ctypes.data_as(C.POINTER(C.c_float)),
                                                 out.size, C.byref(mx)), "osw_debug_get_logmel")
        return out, np.float32(mx.value)

    def debug_mel_windows(self, windows: list) -> np.ndarray:
        """mel_window_kernel alone on (clip, seek, segment_size) windows of the resident log-mel
        (osw_debug_mel_windows): the conv stem's operand X1 as fp16 [n][2 * n_audio_ctx + 2][C1]
        ([n][3002][C1] at the 30 s default window)."""
        arr = (_lib.osw_window * len(windows))(*[_lib.osw_window(int(c), int(s), int(z)) for c, s, z in windows])
        c1 = (self.dims.n_mels + 63) // 64 * 64
        out = np.empty((len(windows), 2 * self.dims.n_audio_ctx + 2, c1), np.float16)
        _lib.check(self.lib.osw_debug_mel_windows(self.ctx, arr, len(windows), out.ctypes.data_as(C.c_void_p),
                                                  out.size), "osw_debug_mel_windows")
        return out

    def hold_capture(self, hold_ms: int) -> None:
        """Test hook (osw_debug_hold_capture): hold a stream capture open on this context's
        stream for ``hold_ms`` under the decode-graph capture's locks; raises if the
        capture was invalidated meanwhile by another thread's call."""
        _lib.check(self.lib.osw_debug_hold_capture(self.ctx, int(hold_ms)), "osw_debug_hold_capture")

    def set_encoder_baton_min(self, min_windows: int) -> None:
        """Encoders of fewer windows skip the sibling lanes' encoder baton (0: never skip)."""
        _lib.check(self.lib.osw_set_encoder_baton_min(self.ctx, int(min_windows)), "osw_set_encoder_baton_min")

    # ------------------------------------------------------------ profiling
    def set_profiling(self, on: bool, eager_decode: bool = False) -> None:
        """Per-stage HIP-event timers; ``eager_decode`` launches the decode steps without
        their hipGraph so the decoder cross-attention is timed too."""
        _lib.check(self.lib.osw_set_profiling(self.ctx, 2 if on and eager_decode else int(on)), "osw_set_profiling")

    def profile(self) -> dict:
        p = _lib.osw_profile()
        _lib.check(self.lib.osw_get_profile(self.ctx, C.byref(p)), "osw_get_profile")
        return p.as_dict()

    def stream(self) -> int:
        return int(self.lib.osw_stream(self.ctx) or 0)

    def close(self) -> None:
        if getattr(self, "ctx", None):
            self.lib.osw_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
