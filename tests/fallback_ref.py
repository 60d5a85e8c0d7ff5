"""Temperature fallback restated in plain Python, one window at a time: faster-whisper 1.2.1
``generate_with_fallback`` (upstream, restated from the rule, not pinned) and the single-clip
seek loop around it.  Written from the rule as ``DESIGN.md`` §4.6 states it, not from
``open_speech_amd/segments.py``, which the tests compare with it; the pieces it shares with
the package are the segment split and the compression ratio, which have tests of their own.

``decode_fn(k, temperature, prefix, language)`` returns the window's result at attempt ``k``
(an object with ``tokens``, ``sum_logprob``, ``no_speech_prob``, ``language``).
"""
from dataclasses import dataclass, field

from open_speech_amd.segments import split_segments_by_timestamps
from open_speech_amd.tokenizer import compression_ratio

MASK64 = 2**64 - 1


def attempt_seed(seed: int, calls: int, k: int) -> int:
    """The documented sampling seed of attempt ``k`` of chunk call number ``calls``."""
    return (seed + 0x9E3779B1 * calls + 0x85EBCA6B * k) % 2**64


def temperatures(opts) -> tuple:
    t = opts.temperature
    return tuple(t) if isinstance(t, (tuple, list)) else (float(t),)


@dataclass
class Attempt:
    result: object
    avg_logprob: float
    temperature: float
    compression_ratio: float


def generate_with_fallback(decode_fn, opts, tok) -> tuple:
    """(kept Attempt with the window's final temperature, every Attempt made)."""
    made, below = [], []
    ladder = temperatures(opts)
    for k, t in enumerate(ladder):
        res = decode_fn(k, t)
        avg = res.sum_logprob / (len(res.tokens) + 1)
        cr = compression_ratio(tok.decode(res.tokens).strip())
        a = Attempt(res, avg, t, cr)
        made.append(a)
        retry = False
        if opts.compression_ratio_threshold is not None:
            if cr > opts.compression_ratio_threshold:
                retry = True
            else:
                below.append(a)
        if opts.log_prob_threshold is not None and avg < opts.log_prob_threshold:
            retry = True
        if (opts.no_speech_threshold is not None and res.no_speech_prob > opts.no_speech_threshold
                and opts.log_prob_threshold is not None and avg < opts.log_prob_threshold):
            retry = False
        if not retry:
            return a, made
    best = None
    for a in (below or made):      # the highest avg_logprob, the first on ties
        if best is None or a.avg_logprob > best.avg_logprob:
            best = a
    return Attempt(best.result, best.avg_logprob, ladder[-1], best.compression_ratio), made


@dataclass
class ClipTrace:
    segments: list = field(default_factory=list)   # dicts: seek, start, end, tokens, temperature, avg_logprob, ...
    windows: list = field(default_factory=list)    # per window: dict(seek, prefix, attempts, temperature, reset)
    language: int | None = None


def transcribe_clip(window_fn, content_frames: int, opts, tok, language: int | None = None) -> ClipTrace:
    """One clip's seek loop without word timestamps, every window through
    ``generate_with_fallback``.  ``window_fn(seek, size)`` returns that window's ``decode_fn``
    taking (k, temperature, prefix, language)."""
    st = tok.special
    tr = ClipTrace(language=language)
    seek, all_tokens, since = 0, [], 0
    while seek < content_frames:
        size = min(3000, content_frames - seek)
        prev = all_tokens[since:]
        prefix = ([st.sot_prev] + prev[-223:]) if prev else []
        fn = window_fn(seek, size)
        known = [tr.language]

        def decode_fn(k, t, fn=fn, prefix=prefix, known=known):
            res = fn(k, t, prefix, known[0])
            if known[0] is None:
                known[0] = res.language     # attempt 0 detects; the retries name it
            return res
        kept, made = generate_with_fallback(decode_fn, opts, tok)
        tr.language = known[0]
        win = dict(seek=seek, prefix=list(prefix), attempts=len(made), temperature=kept.temperature, reset=False)
        tr.windows.append(win)
        res = kept.result
        if opts.no_speech_threshold is not None and res.no_speech_prob > opts.no_speech_threshold and not (
                opts.log_prob_threshold is not None and kept.avg_logprob > opts.log_prob_threshold):
            seek += size
            continue
        segs, new_seek, _ = split_segments_by_timestamps(res.tokens, st.timestamp_begin, seek * 0.01, size,
                                                         size * 0.01, seek)
        for sg in segs:
            if sg["start"] == sg["end"] or not tok.decode(sg["tokens"]).strip():
                continue
            all_tokens.extend(sg["tokens"])
            tr.segments.append(dict(seek=seek, start=sg["start"], end=sg["end"], tokens=list(sg["tokens"]),
                                    temperature=kept.temperature, avg_logprob=kept.avg_logprob,
                                    compression_ratio=kept.compression_ratio, no_speech_prob=res.no_speech_prob))
        if not opts.condition_on_previous_text or kept.temperature > opts.prompt_reset_on_temperature:
            since = len(all_tokens)
            win["reset"] = True
        seek = new_seek
    return tr
