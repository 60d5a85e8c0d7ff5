"""Window scheduling and segment assembly (faster-whisper 1.2.1 ``generate_segments``,
upstream, not vendored), batched across clips.

For every clip the 30 s seek loop of faster-whisper runs unchanged — window k+1
depends on window k's last timestamp and (with ``condition_on_previous_text``) its
tokens — but the windows of DIFFERENT clips that are due at the same time are
encoded and decoded together on the GPU (grouped by prompt length, since every
window of one decode call shares its prompt length).

Semantics restated (beam search width ``beam_size`` — 5 in the reference, 1 = greedy
for the parity mode — at temperature 0.0; the reference passes a scalar ``temperature``
at ``src/backends/faster_whisper.py:238``, so there is no fallback, and a request with
temperature > 0 takes faster-whisper's sampling branch: ``best_of`` samples per window,
the best kept, and the previous-text prompt reset when temperature > 0.5):
  content_frames = n_frames - 1; segment_size = min(nb_max_frames, content_frames - seek)
  nb_max_frames = 100 * chunk_length (``TranscribeOptions.chunk_length``, seconds, 1..30, default 30:
  faster-whisper's ``transcribe(chunk_length=...)``, restated from the upstream code, not pinned; the
  window is zero-padded to nb_max_frames and the encoder runs on 50 * chunk_length positions, so the
  engine's model must have been loaded with the same window: ``WhisperDims.with_chunk_length``)
  prompt = [<|startofprev|>] + previous_tokens[-223:] (if any) + [sot, lang, task]
  avg_logprob = sum_logprob / (len(tokens) + 1); compression_ratio of the window text
  skip window if no_speech_prob > 0.6 and avg_logprob < -1.0  (seek += segment_size)
  split at consecutive timestamp pairs; single timestamp ending -> seek += segment_size,
  else seek += last_timestamp_position * 2; drop segments with start == end or blank text

Word timestamps (``TranscribeOptions.word_timestamps``; faster-whisper ``add_word_timestamps``
/ ``find_alignment`` / ``merge_punctuations``, restated from the upstream code, not pinned):
after a window's decode its text tokens are aligned on the GPU (``engine.align``), split
into words, clamped and attached to the window's segments, and the seek rule gains
  not single_timestamp_ending and last_word_end > time_offset -> seek = round(last_word_end * 100)
with ``last_speech_timestamp`` carried from window to window.

Temperature fallback (``TranscribeOptions.temperature`` a sequence, e.g. faster-whisper's default
ladder (0.0, 0.2, 0.4, 0.6, 0.8, 1.0); faster-whisper ``generate_with_fallback``, restated from
the upstream code, not pinned).  Every window of a chunk is decoded at temperatures[0] as above;
then, per window and for each temperature T_k in order:
  decode (beam or greedy at T_k == 0, else ``best_of`` sampled rows), avg_logprob, text, ratio
  needs_fallback = compression_ratio > compression_ratio_threshold   (else: "below the ratio")
  needs_fallback |= avg_logprob < log_prob_threshold
  needs_fallback = False if no_speech_prob > no_speech_threshold and avg_logprob < log_prob_threshold
  (a threshold that is None switches its own test off); stop at the first T_k that needs none
  every T_k failed: keep the highest avg_logprob among the below-the-ratio results (among all
  when there are none; the first on ties) and report the last temperature as the window's
The windows of a chunk that still need a retry are decoded together at the next temperature with
``engine.decode(..., windows=[their indices in the chunk])`` (osw_decode_window_list: only they
are decoded, from the cross-K/V the chunk's one encoder call left; nothing is encoded or detected
again: the language tokens are attempt 0's).  ``Segment.temperature`` and the
``prompt_reset_on_temperature`` test use the window's own final temperature; the silence skip,
the segment split, the confidences and the word alignment run once, on the kept result.
Seeds: attempt k of chunk call number ``calls`` (which advances once per chunk) samples with
  (opts.seed + 0x9E3779B1 * calls + 0x85EBCA6B * k) mod 2**64
so k = 0 is the scalar-temperature seed.  The chunk size uses the largest row group (beam_size or
best_of) of any attempt.
"""
from __future__ import annotations

import itertools
import math
from dataclasses import dataclass, field

import numpy as np

from .dims import FRAMES_PER_SECOND, HOP_LENGTH, INPUT_STRIDE, TIME_PRECISION, check_chunk_length
from .engine import DecodeConfig
from .tokenizer import WhisperTokenizer, compression_ratio

FRAME_SEC = 0.01


@dataclass
class TranscribeOptions:
    task: str = "transcribe"
    language: str | None = None
    initial_prompt: str | None = None
    condition_on_previous_text: bool = True
    no_speech_threshold: float | None = 0.6
    log_prob_threshold: float | None = -1.0
    compression_ratio_threshold: float | None = 2.4
    suppress_blank: bool = True
    suppress_tokens: tuple = (-1,)
    without_timestamps: bool = False
    max_initial_timestamp: float = 1.0
    # a float, or a sequence of floats: faster-whisper's fallback ladder (module docstring); kept
    # as a float when it has one entry, else as a tuple
    temperature: float | tuple = 0.0
    beam_size: int = 5             # faster-whisper / reference default (src/backends/faster_whisper.py:237)
    patience: float = 1.0
    length_penalty: float = 1.0
    best_of: int = 5               # faster-whisper default; used when temperature > 0
    prompt_reset_on_temperature: float = 0.5
    seed: int = 0
    # faster-whisper's max_new_tokens: a window's decode stops after this many sampled
    # tokens (max_length = prompt length + max_new_tokens, which may not exceed 448)
    max_new_tokens: int | None = None
    # bench-only length control (HipWhisperBackend(length_control=...)): random weights never emit
    # <|endoftext|>, so each window's decode is cut at ceil(rate * window seconds) + 2
    tokens_per_second: float | None = None
    # per-word start / end / probability on every segment (faster-whisper word_timestamps=True)
    word_timestamps: bool = False
    prepend_punctuations: str = "\"'“¿([{-"
    append_punctuations: str = "\"'.。,，!！?？:：”)]}、"
    # faster-whisper's repetition_penalty / no_repeat_ngram_size (CTranslate2's constraints:
    # penalty > 0, size >= 0); 1.0 / 0 = off
    repetition_penalty: float = 1.0
    no_repeat_ngram_size: int = 0
    # per-token log-probabilities on every segment and the detected language's probability
    # (OpenAI include[]=logprobs; faster-whisper language_probability / all_language_probs)
    token_logprobs: bool = False
    # language detection only (faster-whisper WhisperModel.detect_language, one window): the
    # result carries the language and its probabilities, no segments
    detect_only: bool = False
    # seconds of audio per encoder window (faster-whisper chunk_length; module docstring).  A
    # property of the loaded model: the serving layer writes its own into every request
    chunk_length: int = 30

    def __post_init__(self):
        self.chunk_length = check_chunk_length(self.chunk_length)
        t = self.temperature
        if isinstance(t, (str, bytes)):
            raise ValueError(f"temperature must be a number or a sequence of numbers, got {t!r}")
        try:
            ladder = tuple(float(x) for x in t) if hasattr(t, "__iter__") else (float(t),)
        except (TypeError, ValueError):
            raise ValueError(f"temperature must be a number or a sequence of numbers, got {t!r}") from None
        if not ladder:
            raise ValueError("temperature: an empty sequence")
        if not all(math.isfinite(x) and x >= 0 for x in ladder):
            raise ValueError(f"temperature entries must be finite and >= 0, got {t!r}")
        if hasattr(t, "__iter__"):
            self.temperature = ladder[0] if len(ladder) == 1 else ladder
        if not float(self.repetition_penalty) > 0:
            raise ValueError(f"repetition_penalty must be > 0, got {self.repetition_penalty!r}")
        if int(self.no_repeat_ngram_size) < 0:
            raise ValueError(f"no_repeat_ngram_size must be >= 0, got {self.no_repeat_ngram_size!r}")

    @property
    def temperatures(self) -> tuple:
        t = self.temperature
        return tuple(t) if isinstance(t, tuple) else (t,)

    def key(self):
        # the fallback thresholds join only when they differ from the defaults, so the key of
        # every earlier configuration stays what it was
        th = (self.compression_ratio_threshold, self.log_prob_threshold, self.no_speech_threshold)
        k = self._key() + (() if th == (2.4, -1.0, 0.6) else (th,))
        # likewise the window length: the 30 s key is what it was, any other adds its field
        return k if self.chunk_length == 30 else k + (("chunk_length", self.chunk_length),)

    @property
    def nb_max_frames(self) -> int:
        """Mel frames per window: 100 * chunk_length."""
        return FRAMES_PER_SECOND * self.chunk_length

    def _key(self):
        return (self.task, self.language, self.initial_prompt, self.condition_on_previous_text,
                self.without_timestamps, tuple(self.suppress_tokens), self.suppress_blank, self.beam_size,
                self.patience, self.length_penalty, self.temperature, self.best_of, self.tokens_per_second,
                self.max_new_tokens, self.word_timestamps, self.prepend_punctuations, self.append_punctuations,
                float(self.repetition_penalty), int(self.no_repeat_ngram_size), bool(self.token_logprobs),
                bool(self.detect_only))


@dataclass
class Word:
    start: float
    end: float
    word: str
    probability: float


@dataclass
class Segment:
    id: int
    seek: int
    start: float
    end: float
    text: str
    tokens: list
    temperature: float
    avg_logprob: float
    compression_ratio: float
    no_speech_prob: float
    words: list | None = None      # [Word] with word_timestamps, else None
    token_logprobs: list | None = None   # with TranscribeOptions.token_logprobs: one per entry of ``tokens``


@dataclass
class ClipResult:
    segments: list = field(default_factory=list)
    language: str = "en"
    duration: float = 0.0
    # faster-whisper TranscriptionInfo semantics: a detected language's probability and every
    # language's (code, probability) by falling probability, from the window that set the clip's
    # language (needs TranscribeOptions.token_logprobs or detect_only); a language given by the
    # caller: 1.0 and None
    language_probability: float | None = None
    all_language_probs: list | None = None


def split_segments_by_timestamps(tokens: list, tb: int, time_offset: float, segment_size: int,
                                 segment_duration: float, seek: int, token_logprobs: list | None = None):
    """faster-whisper ``_split_segments_by_timestamps`` (openai transcribe.py logic).  With
    ``token_logprobs`` (one per token) every segment also carries the slice of them that
    matches its ``tokens``."""
    if token_logprobs is not None and len(token_logprobs) != len(tokens):
        raise ValueError("one log-probability per token")
    current = []
    single_timestamp_ending = len(tokens) >= 2 and tokens[-2] < tb <= tokens[-1]
    consecutive = [i for i in range(len(tokens)) if i > 0 and tokens[i] >= tb and tokens[i - 1] >= tb]
    if consecutive:
        slices = list(consecutive)
        if single_timestamp_ending:
            slices.append(len(tokens))
        last_slice = 0
        for cur in slices:
            sliced = tokens[last_slice:cur]
            start_pos = sliced[0] - tb
            end_pos = sliced[-1] - tb
            current.append(dict(seek=seek, start=time_offset + start_pos * TIME_PRECISION,
                                end=time_offset + end_pos * TIME_PRECISION, tokens=sliced))
            if token_logprobs is not None:
                current[-1]["token_logprobs"] = token_logprobs[last_slice:cur]
            last_slice = cur
        if single_timestamp_ending:
            seek += segment_size
        else:
            last_ts_pos = tokens[last_slice - 1] - tb
            seek += last_ts_pos * INPUT_STRIDE
    else:
        duration = segment_duration
        ts = [t for t in tokens if t >= tb]
        if ts and ts[-1] != tb:
            duration = (ts[-1] - tb) * TIME_PRECISION
        current.append(dict(seek=seek, start=time_offset, end=time_offset + duration, tokens=tokens))
        if token_logprobs is not None:
            current[-1]["token_logprobs"] = token_logprobs
        seek += segment_size
    return current, seek, single_timestamp_ending


@dataclass
class _ClipState:
    idx: int
    content_frames: int
    seek: int = 0
    all_tokens: list = field(default_factory=list)
    prompt_reset_since: int = 0
    lang_token: int | None = None
    done: bool = False
    result: ClipResult = field(default_factory=ClipResult)
    last_speech_timestamp: float = 0.0   # word timestamps: end of the last word so far


def transcribe_clips(engine, pcm_list: list, opts: TranscribeOptions, tok: WhisperTokenizer,
                     suppress: tuple) -> list[ClipResult]:
    """Run the seek loop for a batch of int16 clips on one engine (all share `opts`)."""
    st = tok.special
    if opts.detect_only and not st.multilingual:  # nothing to detect: no engine call at all
        return [_english_clip(ClipResult(duration=len(p) / 16000.0), True) for p in pcm_list]
    nf = engine.log_mel(pcm_list)
    if opts.detect_only:
        return _detect_clips(engine, pcm_list, nf, tok, opts.nb_max_frames)
    lang_token = _given_language(opts, tok)
    init_tokens = tok.encode(" " + opts.initial_prompt.strip()) if opts.initial_prompt else []
    states = []
    for i, n in enumerate(nf):
        s = _ClipState(idx=i, content_frames=max(0, n - 1), all_tokens=list(init_tokens), lang_token=lang_token)
        s.result.duration = len(pcm_list[i]) / 16000.0
        s.done = s.content_frames <= 0
        if lang_token is not None:
            s.result.language_probability = 1.0
        if not st.multilingual:
            _english_clip(s.result, bool(opts.token_logprobs))
        states.append(s)
    max_init = int(round(opts.max_initial_timestamp / TIME_PRECISION))
    temps = opts.temperatures

    def rows_per_window(t):  # decoder rows per window: best_of samples, or the beam
        return max(1, int(opts.best_of)) if t > 0 else max(1, int(opts.beam_size))

    group = max(rows_per_window(t) for t in temps)  # the largest of any attempt
    B = max(1, min(engine.max_batch, getattr(engine, "max_rows", engine.max_batch) // group))
    calls = 0
    while True:
        active = [s for s in states if not s.done]
        if not active:
            break
        # group due windows by prompt (prefix) length and by "language known"
        groups: dict = {}
        for s in active:
            prev = s.all_tokens[s.prompt_reset_since:]
            prefix = ([st.sot_prev] + prev[-(448 // 2 - 1):]) if prev else []
            groups.setdefault((len(prefix), s.lang_token is None), []).append((s, prefix))
        for (_plen, _detect), members in groups.items():
            for lo in range(0, len(members), B):
                chunk = members[lo:lo + B]
                wins = []
                for s, _ in chunk:
                    size = min(opts.nb_max_frames, s.content_frames - s.seek)
                    wins.append((s.idx, s.seek, size))
                engine.encode(wins)
                # (an English-only model's start sequence has no language token: nothing to name)
                langs = None if (_detect or not st.multilingual) else [s.lang_token for s, _ in chunk]
                max_length = 448
                if opts.max_new_tokens is not None:
                    max_length = (_plen + _start_len(st) + (1 if opts.without_timestamps else 0) +
                                  int(opts.max_new_tokens))
                    if max_length > 448:
                        raise ValueError(f"the prompt is {max_length - int(opts.max_new_tokens)} tokens and "
                                         f"max_new_tokens is {opts.max_new_tokens}: their sum exceeds the "
                                         "model's maximum length (448)")
                budgets = tuple(int(np.ceil(opts.tokens_per_second * z * FRAME_SEC)) + 2
                                for _, _, z in wins) if opts.tokens_per_second else None

                def attempt_cfg(k, which=None, max_length=max_length, calls=calls, budgets=budgets):
                    # attempt k of this chunk, for the windows `which` of it (None: all of them)
                    t = temps[k]
                    return DecodeConfig(
                        max_length=max_length, task=opts.task, language_token=None, suppress_tokens=suppress,
                        suppress_blank=opts.suppress_blank, without_timestamps=opts.without_timestamps,
                        max_initial_timestamp_index=max_init, beam_size=1 if t > 0 else max(1, int(opts.beam_size)),
                        patience=opts.patience, length_penalty=opts.length_penalty, temperature=t,
                        best_of=opts.best_of,
                        seed=attempt_seed(opts.seed, calls, k),
                        repetition_penalty=float(opts.repetition_penalty),
                        no_repeat_ngram_size=int(opts.no_repeat_ngram_size), confidences=bool(opts.token_logprobs),
                        token_budget=None if budgets is None else
                        (budgets if which is None else tuple(budgets[i] for i in which)))

                calls += 1
                prefixes = [p for _, p in chunk] if _plen else None
                outs = engine.decode(len(chunk), attempt_cfg(0), prefix=prefixes, languages=langs)
                win_temps = [temps[0]] * len(chunk)
                if len(temps) > 1:
                    outs, win_temps = _fallback(engine, chunk, outs, prefixes, attempt_cfg, temps, opts, tok)
                if not opts.word_timestamps:
                    for (s, _), w, out, t in zip(chunk, wins, outs, win_temps):
                        _consume(s, w, out, opts, tok, t)
                    continue
                # word timestamps: one alignment call for the chunk's windows while their
                # cross-K/V is still resident, then the segments with their words
                from .engine import AlignWindow
                plans = [_plan(s, w, out, opts, tok, t) for (s, _), w, out, t in zip(chunk, wins, outs, win_temps)]
                req = [(i, p) for i, p in enumerate(plans) if p is not None and p["text_tokens"]]
                # the forced sequence adds 5 positions (3 for an English-only model): a window that
                # decoded more text tokens than fit (a model that never emits <|endoftext|>) aligns
                # the ones that do
                room = 448 - (_start_len(st) + 2)
                als = engine.align([AlignWindow(window=i, tokens=p["text_tokens"][:room], num_frames=wins[i][2],
                                                language=outs[i].language, task=opts.task)
                                    for i, p in req]) if req else []
                aligned = {i: _pad_alignment(a, len(p["text_tokens"])) for (i, p), a in zip(req, als)}
                for i, ((s, _), w, out) in enumerate(zip(chunk, wins, outs)):
                    if plans[i] is not None:
                        _apply(s, w, out, opts, tok, plans[i], aligned.get(i))
    for s in states:
        code = tok.language_code(s.lang_token) if s.lang_token is not None else (opts.language or "en")
        s.result.language = code
    return [s.result for s in states]


def attempt_seed(seed: int, call: int, k: int) -> int:
    """The sampling seed of attempt ``k`` (the index into the temperature ladder) of chunk call
    number ``call`` of a ``transcribe_clips`` run.  A clip transcribed alone makes one call per
    window, so there ``call`` is the window's number in the clip (0-based, windows skipped as
    silence included): what a session lane passes for its retries."""
    return (int(seed) + 0x9E3779B1 * int(call) + 0x85EBCA6B * int(k)) & (2**64 - 1)


def needs_fallback(out, avg_logprob: float, cr: float, opts: TranscribeOptions):
    """faster-whisper ``generate_with_fallback``'s tests on one decode result: (needs a retry at
    the next temperature, is below the compression-ratio threshold)."""
    needs, below = False, False
    if opts.compression_ratio_threshold is not None:
        if cr > opts.compression_ratio_threshold:
            needs = True
        else:
            below = True
    if opts.log_prob_threshold is not None and avg_logprob < opts.log_prob_threshold:
        needs = True
    if (opts.no_speech_threshold is not None and out.no_speech_prob > opts.no_speech_threshold
            and opts.log_prob_threshold is not None and avg_logprob < opts.log_prob_threshold):
        needs = False  # silence
    return needs, below


def _fallback(engine, chunk: list, outs0: list, prefixes, attempt_cfg, temps: tuple, opts: TranscribeOptions,
              tok: WhisperTokenizer):
    """The retries of one chunk after its attempt 0 (module docstring): the kept result and the
    final temperature of every window.  A clip whose language attempt 0 detected keeps it (and
    that window's language probabilities): the retries name it."""
    n = len(chunk)
    for (s, _), out in zip(chunk, outs0):
        if s.lang_token is None:
            s.lang_token = out.language
            _set_language_probs(s.result, getattr(out, "language_probs", None), out.language, tok)
    tried = [[] for _ in range(n)]   # per window: (avg_logprob, below the ratio, result) of every attempt
    final = [temps[0]] * n
    kept = list(outs0)
    failing = []
    for k in range(len(temps)):
        if k == 0:
            which, outs = list(range(n)), outs0
        else:
            which = failing
            outs = engine.decode(len(which), attempt_cfg(k, which),
                                 prefix=[prefixes[i] for i in which] if prefixes else None,
                                 languages=[chunk[i][0].lang_token for i in which] if tok.special.multilingual
                                 else None, windows=list(which))
        failing = []
        for i, out in zip(which, outs):
            avg = out.sum_logprob / (len(out.tokens) + 1)
            needs, below = needs_fallback(out, avg, compression_ratio(tok.decode(out.tokens).strip()), opts)
            tried[i].append((avg, below, out))
            final[i] = temps[k]
            if needs:
                failing.append(i)
            else:
                kept[i] = out
        if not failing:
            break
    for i in failing:  # every temperature failed
        pool = [r for r in tried[i] if r[1]] or tried[i]
        kept[i] = max(pool, key=lambda r: r[0])[2]
    return kept, final


def _set_language_probs(res: ClipResult, probs, lang_token: int, tok: WhisperTokenizer) -> None:
    """faster-whisper's language_probability / all_language_probs from the window that set the
    clip's language (nothing when the engine recorded no probabilities)."""
    if probs is None:
        return
    p = np.asarray(probs, dtype=np.float64)
    res.language_probability = float(p[lang_token - tok.special.first_lang])
    res.all_language_probs = [(tok.language_code(tok.special.first_lang + int(i)), float(p[i]))
                              for i in np.argsort(-p, kind="stable")]


ENGLISH_LANG = -1  # _ClipState.lang_token of an English-only model's clips: known, and no token


def _given_language(opts: TranscribeOptions, tok: WhisperTokenizer):
    """The clips' language token when the options name the language (None: detect it)."""
    if not tok.special.multilingual:
        return ENGLISH_LANG
    return tok.language_token(opts.language) if (opts.language and opts.task == "transcribe") else None


def _start_len(st) -> int:
    """Tokens of the start sequence: sot, language, task; an English-only model's is sot alone."""
    return 3 if st.multilingual else 1


def _english_clip(res: ClipResult, want_probs: bool) -> ClipResult:
    """faster-whisper's TranscriptionInfo for a model that is not multilingual: "en" with
    probability 1, never detected."""
    res.language = "en"
    res.language_probability = 1.0
    if want_probs:
        res.all_language_probs = [("en", 1.0)]
    return res


def _detect_clips(engine, pcm_list: list, nf: list, tok: WhisperTokenizer, nb_max_frames: int) -> list[ClipResult]:
    """TranscribeOptions.detect_only: the language of every clip's first window (nb_max_frames frames)
    (faster-whisper ``detect_language`` with language_detection_segments = 1)."""
    out = []
    B = max(1, engine.max_batch)
    for lo in range(0, len(pcm_list), B):
        idx = list(range(lo, min(lo + B, len(pcm_list))))
        engine.encode([(i, 0, max(1, min(nb_max_frames, nf[i] - 1))) for i in idx])
        probs = engine.detect_language(len(idx))
        for i, p in zip(idx, probs):
            lang = tok.special.first_lang + int(np.argmax(p))
            res = ClipResult(language=tok.language_code(lang), duration=len(pcm_list[i]) / 16000.0)
            _set_language_probs(res, p, lang, tok)
            out.append(res)
    return out


# ------------------------------------------------------------ one clip at a time
# (the runner's decode-session lanes, runner.py: each clip's seek loop advances on its own,
# its next window queued into the session as soon as the previous one is consumed)

def session_supported(opts: TranscribeOptions) -> bool:
    """Decode sessions (osw_session_*) hold one decode configuration for every window:
    temperature 0 (one entry: no fallback ladder), beam_size <= 5, and no max_new_tokens
    (whose max_length depends on each window's prompt length)."""
    if opts.word_timestamps:   # the alignment pass needs the window's cross-K/V of a batched decode call
        return False
    if opts.detect_only:       # one decoder step per clip, no seek loop
        return False
    temps = opts.temperatures   # (a fallback ladder takes the batched seek loop: its retries are decode calls)
    return len(temps) == 1 and not (temps[0] > 0) and opts.max_new_tokens is None and 1 <= int(opts.beam_size) <= 5


def word_session_supported(opts: TranscribeOptions) -> bool:
    """Word timing on a decode session (osw_session_hold / osw_session_align): a request with
    ``word_timestamps`` whose other options a session can hold.  ``session_supported`` itself
    keeps answering False for it: a driver without the hold / align calls must leave such a
    request to the batched seek loop."""
    if not opts.word_timestamps:
        return False
    import dataclasses
    return session_supported(dataclasses.replace(opts, word_timestamps=False))


def fallback_session_supported(opts: TranscribeOptions) -> bool:
    """A temperature ladder on a decode session (osw_session_retries / osw_session_retry): attempt 0
    is the session's temperature-0 mode and a window that needs a fallback decodes again in its
    slot with ``best_of`` sampled rows.  True for a ladder of two or more entries that starts at 0
    and is > 0 afterwards, with 1 <= best_of <= 5, whose other options a session can hold (with or
    without word timing).  ``session_supported`` and ``word_session_supported`` keep answering
    False for a ladder: a driver without the retry call leaves it to the batched seek loop."""
    temps = opts.temperatures
    if len(temps) < 2 or temps[0] != 0 or not all(t > 0 for t in temps[1:]):
        return False
    if not 1 <= int(opts.best_of) <= 5:
        return False
    import dataclasses
    base = dataclasses.replace(opts, temperature=0.0)
    return session_supported(base) or word_session_supported(base)


def fallback_verdict(tried: list, out, temps: tuple, opts: TranscribeOptions, tok: WhisperTokenizer):
    """One attempt of a window on a session lane, by ``_fallback``'s rule: ``tried`` holds the
    window's earlier attempts and gets this one; returns ``(retry, kept)``: the index into ``temps``
    of the attempt to make next with ``kept`` None, or None with the result to keep (this one, or
    when every temperature failed the best ``avg_logprob`` among those below the ratio, among all
    without one).  The window's final temperature is ``temps[len(tried) - 1]``."""
    avg = out.sum_logprob / (len(out.tokens) + 1)
    needs, below = needs_fallback(out, avg, compression_ratio(tok.decode(out.tokens).strip()), opts)
    tried.append((avg, below, out))
    if not needs:
        return None, out
    if len(tried) < len(temps):
        return len(tried), None
    pool = [r for r in tried if r[1]] or tried
    return None, max(pool, key=lambda r: r[0])[2]


def session_config(opts: TranscribeOptions, suppress: tuple) -> DecodeConfig:
    """The session-wide decode configuration (transcribe_clips' per-call one, minus the
    per-window prefix, language and token budget)."""
    return DecodeConfig(max_length=448, task=opts.task, language_token=None, suppress_tokens=suppress,
                        suppress_blank=opts.suppress_blank, without_timestamps=opts.without_timestamps,
                        max_initial_timestamp_index=int(round(opts.max_initial_timestamp / TIME_PRECISION)),
                        beam_size=max(1, int(opts.beam_size)), patience=opts.patience,
                        length_penalty=opts.length_penalty, repetition_penalty=float(opts.repetition_penalty),
                        no_repeat_ngram_size=int(opts.no_repeat_ngram_size), confidences=bool(opts.token_logprobs))


def clip_state(idx: int, pcm: np.ndarray, opts: TranscribeOptions, tok: WhisperTokenizer) -> _ClipState:
    """transcribe_clips' per-clip state (log_mel's frame count is len // 160 + 1, the
    content frames one fewer)."""
    lang_token = _given_language(opts, tok)
    init_tokens = tok.encode(" " + opts.initial_prompt.strip()) if opts.initial_prompt else []
    s = _ClipState(idx=idx, content_frames=len(pcm) // HOP_LENGTH, all_tokens=list(init_tokens),
                   lang_token=lang_token)
    s.result.duration = len(pcm) / 16000.0
    s.done = s.content_frames <= 0
    if lang_token is not None:
        s.result.language_probability = 1.0
    if not tok.special.multilingual:
        _english_clip(s.result, bool(opts.token_logprobs))
    return s


def next_window(s: _ClipState, opts: TranscribeOptions, tok: WhisperTokenizer) -> dict:
    """The clip's next window: seek, segment_size, prompt prefix, language, token budget."""
    prev = s.all_tokens[s.prompt_reset_since:]
    prefix = ([tok.special.sot_prev] + prev[-(448 // 2 - 1):]) if prev else []
    size = min(opts.nb_max_frames, s.content_frames - s.seek)
    budget = int(np.ceil(opts.tokens_per_second * size * FRAME_SEC)) + 2 if opts.tokens_per_second else 0
    lang = s.lang_token if tok.special.multilingual else None  # (English-only: no language token)
    return dict(seek=s.seek, segment_size=size, prefix=prefix, language_token=lang, token_budget=budget)


def note_language(s: _ClipState, out, tok: WhisperTokenizer) -> None:
    """A clip whose language attempt 0 of its first window detected keeps it, with that window's
    language probabilities (``_fallback``): a lane calls this before it retries the window."""
    if s.lang_token is None:
        s.lang_token = out.language
        _set_language_probs(s.result, getattr(out, "language_probs", None), out.language, tok)


def consume_window(s: _ClipState, win: dict, out, opts: TranscribeOptions, tok: WhisperTokenizer,
                   temperature=None) -> None:
    """``temperature``: the window's own final one (a fallback ladder), None: the options' scalar."""
    _consume(s, (s.idx, win["seek"], win["segment_size"]), out, opts, tok, temperature)


def plan_window(s: _ClipState, win: dict, out, opts: TranscribeOptions, tok: WhisperTokenizer, temperature=None):
    """``consume_window`` in two halves, for word timing on a session: the window's segments before
    they are kept (None: skipped as silence, the seek already moved), with ``text_tokens``."""
    return _plan(s, (s.idx, win["seek"], win["segment_size"]), out, opts, tok, temperature)


def align_request(plan, win: dict, out, opts: TranscribeOptions, tok: WhisperTokenizer):
    """The ``AlignWindow`` of a planned window, as transcribe_clips asks for it (None: nothing to
    align — a skipped window or one without text tokens).  The forced sequence adds 5 positions
    (3 for an English-only model): a window that decoded more text tokens than fit aligns the
    ones that do (``pad_alignment`` covers the rest)."""
    if plan is None or not plan["text_tokens"]:
        return None
    from .engine import AlignWindow
    room = 448 - (_start_len(tok.special) + 2)
    return AlignWindow(window=0, tokens=plan["text_tokens"][:room], num_frames=win["segment_size"],
                       language=out.language, task=opts.task)


def pad_alignment(alignment, plan):
    return _pad_alignment(alignment, len(plan["text_tokens"]))


def apply_window(s: _ClipState, win: dict, out, opts: TranscribeOptions, tok: WhisperTokenizer, plan: dict,
                 alignment) -> None:
    """Keep a planned window's segments, with their words when ``alignment`` is given; the seek
    moves to the last word's end as in transcribe_clips."""
    _apply(s, (s.idx, win["seek"], win["segment_size"]), out, opts, tok, plan, alignment)


def finish_clip(s: _ClipState, opts: TranscribeOptions, tok: WhisperTokenizer) -> ClipResult:
    s.result.language = tok.language_code(s.lang_token) if s.lang_token is not None else (opts.language or "en")
    return s.result


def _consume(s: _ClipState, win, out, opts: TranscribeOptions, tok: WhisperTokenizer, temperature=None) -> None:
    plan = _plan(s, win, out, opts, tok, temperature)
    if plan is not None:
        _apply(s, win, out, opts, tok, plan, None)


def _plan(s: _ClipState, win, out, opts: TranscribeOptions, tok: WhisperTokenizer, temperature=None):
    """The window's segments before they are kept (None: the window was skipped as silence),
    with the text tokens word timing aligns.  ``temperature``: the window's own final one
    (None: the options' scalar)."""
    st = tok.special
    _, seek, segment_size = win
    if s.lang_token is None:
        s.lang_token = out.language
        _set_language_probs(s.result, getattr(out, "language_probs", None), out.language, tok)
    tokens = out.tokens
    avg_logprob = out.sum_logprob / (len(tokens) + 1)
    text = tok.decode(tokens).strip()
    cr = compression_ratio(text)
    if opts.no_speech_threshold is not None:
        skip = out.no_speech_prob > opts.no_speech_threshold
        if opts.log_prob_threshold is not None and avg_logprob > opts.log_prob_threshold:
            skip = False
        if skip:
            s.seek = seek + segment_size
            s.done = s.seek >= s.content_frames
            return None
    time_offset = seek * FRAME_SEC
    lps = getattr(out, "token_logprobs", None) if opts.token_logprobs else None
    segs, new_seek, single_ending = split_segments_by_timestamps(tokens, st.timestamp_begin, time_offset, segment_size,
                                                                 segment_size * FRAME_SEC, seek, lps)
    text_tokens = [int(t) for sg in segs for t in sg["tokens"] if t < st.eot]
    return dict(segs=segs, new_seek=new_seek, single_ending=single_ending, avg_logprob=avg_logprob, cr=cr,
                text_tokens=text_tokens, time_offset=time_offset,
                temperature=opts.temperatures[0] if temperature is None else temperature)


def _apply(s: _ClipState, win, out, opts: TranscribeOptions, tok: WhisperTokenizer, plan: dict, alignment) -> None:
    """Keep the planned segments (with their words when ``alignment`` is given) and move the seek."""
    _, seek, segment_size = win
    segs, new_seek, avg_logprob, cr = plan["segs"], plan["new_seek"], plan["avg_logprob"], plan["cr"]
    temperature = plan["temperature"]
    if opts.word_timestamps:
        lang = tok.language_code(s.lang_token) if s.lang_token is not None else opts.language
        s.last_speech_timestamp = add_word_timestamps(segs, tok, alignment, lang, opts.prepend_punctuations,
                                                      opts.append_punctuations, s.last_speech_timestamp)
        last_word_end = _last_word_end(segs)
        if not plan["single_ending"] and last_word_end is not None and last_word_end > plan["time_offset"]:
            new_seek = round(last_word_end / FRAME_SEC)
        if last_word_end is not None:
            s.last_speech_timestamp = last_word_end
    for sg in segs:
        t = sg["tokens"]
        txt = tok.decode(t)
        if sg["start"] == sg["end"] or not txt.strip():
            continue
        s.all_tokens.extend(t)
        s.result.segments.append(Segment(id=len(s.result.segments), seek=seek, start=sg["start"], end=sg["end"],
                                         text=txt, tokens=list(t), temperature=temperature,
                                         avg_logprob=avg_logprob, compression_ratio=cr,
                                         no_speech_prob=out.no_speech_prob,
                                         words=[Word(**w) for w in sg["words"]] if "words" in sg else None,
                                         token_logprobs=list(sg["token_logprobs"]) if "token_logprobs" in sg
                                         else None))
    if not opts.condition_on_previous_text or temperature > opts.prompt_reset_on_temperature:
        s.prompt_reset_since = len(s.all_tokens)
    s.seek = new_seek
    s.done = s.seek >= s.content_frames


# ------------------------------------------------------------ word timestamps
SENTENCE_END_MARKS = ".。!！?？"


def find_alignment(tok: WhisperTokenizer, text_tokens: list, alignment, language: str | None) -> list:
    """faster-whisper ``find_alignment`` after CTranslate2's ``align`` [upstream]: words with
    the first frame of their first token as start, of the next word's first token as end
    (the <|endoftext|> frame for the last word), and the mean token probability."""
    if alignment is None or not text_tokens:
        return []
    words, word_tokens = tok.split_to_word_tokens(list(text_tokens) + [tok.special.eot], language)
    if len(word_tokens) <= 1:
        return []
    bounds = np.pad(np.cumsum([len(t) for t in word_tokens[:-1]]), (1, 0))
    times = np.asarray(alignment.token_frame, dtype=np.float64) * TIME_PRECISION
    probs = np.asarray(alignment.token_prob, dtype=np.float64)
    return [dict(word=w, tokens=list(t), start=float(times[i]), end=float(times[j]),
                 probability=float(np.mean(probs[i:j])))
            for w, t, i, j in zip(words, word_tokens, bounds[:-1], bounds[1:])]


def merge_punctuations(alignment: list, prepended: str, appended: str) -> None:
    """faster-whisper ``merge_punctuations`` [upstream], in place: merged words keep their
    own times, the absorbed entry becomes an empty word without tokens."""
    i, j = len(alignment) - 2, len(alignment) - 1
    while i >= 0:
        prev, foll = alignment[i], alignment[j]
        if prev["word"].startswith(" ") and prev["word"].strip() in prepended:
            foll["word"] = prev["word"] + foll["word"]
            foll["tokens"] = prev["tokens"] + foll["tokens"]
            prev["word"] = ""
            prev["tokens"] = []
        else:
            j = i
        i -= 1
    i, j = 0, 1
    while j < len(alignment):
        prev, foll = alignment[i], alignment[j]
        if not prev["word"].endswith(" ") and foll["word"] in appended:
            prev["word"] = prev["word"] + foll["word"]
            prev["tokens"] = prev["tokens"] + foll["tokens"]
            foll["word"] = ""
            foll["tokens"] = []
        else:
            i = j
        j += 1


def add_word_timestamps(segs: list, tok: WhisperTokenizer, alignment, language: str | None, prepend: str,
                        append: str, last_speech_timestamp: float) -> float:
    """faster-whisper ``add_word_timestamps`` [upstream] for one window: ``segs`` are the
    window's segment dicts (``split_segments_by_timestamps``), each gains ``"words"`` and may
    have its start / end moved to its words; returns the new last_speech_timestamp."""
    if not segs:
        return last_speech_timestamp
    per_seg = [[t for t in sg["tokens"] if t < tok.special.eot] for sg in segs]
    text_tokens = list(itertools.chain.from_iterable(per_seg))
    words_all = find_alignment(tok, text_tokens, alignment, language)
    durations = np.array([w["end"] - w["start"] for w in words_all])
    durations = durations[durations.nonzero()]
    median_duration = min(0.7, float(np.median(durations))) if len(durations) else 0.0
    max_duration = median_duration * 2
    if len(durations):
        # words at sentence boundaries no longer than twice the median word duration
        for i in range(1, len(words_all)):
            w = words_all[i]
            if w["end"] - w["start"] > max_duration:
                if w["word"] in SENTENCE_END_MARKS:
                    w["end"] = w["start"] + max_duration
                elif words_all[i - 1]["word"] in SENTENCE_END_MARKS:
                    w["start"] = w["end"] - max_duration
    merge_punctuations(words_all, prepend, append)
    time_offset = segs[0]["seek"] * FRAME_SEC
    wi = 0
    for sg, toks in zip(segs, per_seg):
        saved, words = 0, []
        while wi < len(words_all) and saved < len(toks):
            t = words_all[wi]
            if t["word"]:
                words.append(dict(word=t["word"], start=round(time_offset + t["start"], 2),
                                  end=round(time_offset + t["end"], 2), probability=t["probability"]))
            saved += len(t["tokens"])
            wi += 1
        if words:
            # the first and second word after a pause no longer than twice the median duration
            if words[0]["end"] - last_speech_timestamp > median_duration * 4 and (
                    words[0]["end"] - words[0]["start"] > max_duration
                    or (len(words) > 1 and words[1]["end"] - words[0]["start"] > max_duration * 2)):
                if len(words) > 1 and words[1]["end"] - words[1]["start"] > max_duration:
                    boundary = max(words[1]["end"] / 2, words[1]["end"] - max_duration)
                    words[0]["end"] = words[1]["start"] = boundary
                words[0]["start"] = max(0, words[0]["end"] - max_duration)
            # prefer the segment-level start / end when the first / last word is too long
            if sg["start"] < words[0]["end"] and sg["start"] - 0.5 > words[0]["start"]:
                words[0]["start"] = max(0, min(words[0]["end"] - median_duration, sg["start"]))
            else:
                sg["start"] = words[0]["start"]
            if sg["end"] > words[-1]["start"] and sg["end"] + 0.5 < words[-1]["end"]:
                words[-1]["end"] = max(words[-1]["start"] + median_duration, sg["end"])
            else:
                sg["end"] = words[-1]["end"]
            last_speech_timestamp = sg["end"]
        sg["words"] = words
    return last_speech_timestamp


def _pad_alignment(a, n: int):
    """Text tokens beyond the aligned ones take the <|endoftext|> frame and probability 0."""
    k = len(a.token_prob)
    if k >= n:
        return a
    from .engine import Alignment
    tf = np.asarray(a.token_frame)
    return Alignment(np.concatenate([tf[:k], np.full(n - k + 1, tf[-1], tf.dtype)]),
                     np.concatenate([np.asarray(a.token_prob, np.float64), np.zeros(n - k)]))


def _last_word_end(segs: list):
    """faster-whisper ``get_end`` [upstream]: the last word's end, else the last segment's."""
    for sg in reversed(segs):
        for w in reversed(sg.get("words") or []):
            return w["end"]
    return segs[-1]["end"] if segs else None


def verbose_dict(task: str, res: ClipResult) -> dict:
    """The ``verbose_json`` shape of ``src/backends/faster_whisper.py:251-272``; with word
    timestamps every segment gains ``words`` and the response a flat ``words`` list (the
    OpenAI ``timestamp_granularities[]=word`` shape)."""
    out = _verbose_dict(task, res)
    if any(sg.words is not None for sg in res.segments):
        for d, sg in zip(out["segments"], res.segments):
            d["words"] = [{"start": w.start, "end": w.end, "word": w.word, "probability": w.probability}
                          for w in (sg.words or [])]
        out["words"] = [{"word": w.word, "start": w.start, "end": w.end}
                        for sg in res.segments for w in (sg.words or [])]
    return out


def _verbose_dict(task: str, res: ClipResult) -> dict:
    full = "".join(sg.text for sg in res.segments).strip()
    return {
        "task": task, "language": res.language, "duration": res.duration, "text": full,
        "segments": [{"id": i, "seek": int(sg.seek), "start": sg.start, "end": sg.end, "text": sg.text,
                      "tokens": list(sg.tokens) if sg.tokens else [], "temperature": sg.temperature,
                      "avg_logprob": sg.avg_logprob, "compression_ratio": sg.compression_ratio,
                      "no_speech_prob": sg.no_speech_prob} for i, sg in enumerate(res.segments)],
    }


def _ts(seconds: float, sep: str) -> str:
    h = int(seconds // 3600)
    m = int((seconds % 3600) // 60)
    s = int(seconds % 60)
    ms = int((seconds % 1) * 1000)
    return f"{h:02d}:{m:02d}:{s:02d}{sep}{ms:03d}"


def to_srt(segments) -> str:
    """``FasterWhisperBackend._to_srt`` (src/backends/faster_whisper.py:313-321)."""
    return "\n".join(f"{i}\n{_ts(s.start, ',')} --> {_ts(s.end, ',')}\n{s.text.strip()}\n"
                     for i, s in enumerate(segments, 1))


def to_vtt(segments) -> str:
    """``FasterWhisperBackend._to_vtt`` (src/backends/faster_whisper.py:323-330)."""
    lines = ["WEBVTT\n"]
    for s in segments:
        lines.append(f"{_ts(s.start, '.')} --> {_ts(s.end, '.')}\n{s.text.strip()}\n")
    return "\n".join(lines)


def logprobs_list(res: ClipResult, tok: WhisperTokenizer) -> list:
    """OpenAI's ``include[]=logprobs`` shape over the text tokens (ids below <|endoftext|>) of
    every segment, in order."""
    eot = tok.special.eot
    out = []
    for sg in res.segments:
        for t, lp in zip(sg.tokens, sg.token_logprobs or ()):
            if t < eot:
                b = tok.token_bytes(t)
                out.append({"token": b.decode("utf-8", errors="replace"), "logprob": float(lp), "bytes": list(b)})
    return out


def shape_response(task: str, res: ClipResult, response_format: str, tok: WhisperTokenizer | None = None,
                   logprobs: bool = False) -> dict:
    """Return shapes by format (src/backends/faster_whisper.py:251-281).  ``logprobs`` (with
    ``tok``): ``json`` / ``verbose_json`` gain ``logprobs`` and ``language_probability``,
    ``verbose_json`` segments ``token_logprobs``; the other formats and ``logprobs=False`` are
    the reference's shapes unchanged."""
    full = "".join(sg.text for sg in res.segments).strip()
    if logprobs and response_format in ("json", "verbose_json"):
        out = verbose_dict(task, res) if response_format == "verbose_json" else {"text": full}
        if response_format == "verbose_json":
            for d, sg in zip(out["segments"], res.segments):
                d["token_logprobs"] = [float(x) for x in (sg.token_logprobs or [])]
        out["logprobs"] = logprobs_list(res, tok)
        out["language_probability"] = res.language_probability
        return out
    if response_format == "verbose_json":
        return verbose_dict(task, res)
    if response_format == "text":
        return {"text": full, "raw_text": True}
    if response_format == "srt":
        return {"text": to_srt(res.segments), "raw_text": True}
    if response_format == "vtt":
        return {"text": to_vtt(res.segments), "raw_text": True}
    return {"text": full}


def np_int16(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.int16)
