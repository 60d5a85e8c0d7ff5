"""Temperature fallback without a GPU: ``transcribe_clips`` with a temperature ladder against
the window-by-window restatement of ``tests/fallback_ref.py`` on randomized scripted engines,
the directed cases of faster-whisper's ``generate_with_fallback``, the decode calls the retries
make (which windows, which configuration, which seed), and the options / backend plumbing."""
import os
import re

import numpy as np
import pytest

import fallback_ref as fr
from open_speech_amd import _lib
from open_speech_amd import dims as D
from open_speech_amd.backend import HipWhisperBackend, fallback_temperatures
from open_speech_amd.engine import WindowOutput
from open_speech_amd.segments import TranscribeOptions, session_supported, transcribe_clips
from open_speech_amd.tokenizer import WhisperTokenizer
from test_backend_cpu import MID, FakeEngine, wav

N_VOCAB = 51866
ST = D.SpecialTokens.for_vocab(N_VOCAB)
TB = ST.timestamp_begin
TOK = WhisperTokenizer(N_VOCAB)
LADDER = (0.0, 0.4, 0.8)


class ScriptedEngine:
    """``script(clip, seek, temperature) -> WindowOutput``; every decode call is recorded."""

    def __init__(self, script, max_batch=4, max_rows=None):
        self.script, self.max_batch = script, max_batch
        if max_rows is not None:
            self.max_rows = max_rows
        self.calls, self._wins = [], []

    def log_mel(self, clips):
        return [len(c) // 160 + 1 for c in clips]

    def encode(self, wins):
        self._wins = list(wins)

    def decode(self, n, cfg, prefix=None, dump_steps=0, languages=None, **kw):
        assert set(kw) <= {"windows"}
        idx = list(kw["windows"]) if "windows" in kw else list(range(len(self._wins)))
        assert n == len(idx) and len(set(idx)) == n and all(0 <= i < len(self._wins) for i in idx)
        assert prefix is None or len(prefix) == n
        assert languages is None or len(languages) == n
        assert cfg.token_budget is None or len(cfg.token_budget) == n
        self.calls.append(dict(n=n, windows=list(kw["windows"]) if "windows" in kw else None, wins=list(self._wins),
                               temperature=cfg.temperature, beam_size=cfg.beam_size, best_of=cfg.best_of,
                               seed=cfg.seed, prefix=[list(p) for p in prefix] if prefix else None,
                               languages=None if languages is None else list(languages)))
        return [self.script(self._wins[i][0], self._wins[i][1], cfg.temperature) for i in idx]


def clip(seconds):
    return np.zeros(int(seconds * 16000), np.int16)


def out(avg, repetitive=False, nsp=0.01, text=(1000, 1001, 1002), lang=ST.first_lang, shape="end"):
    """A window result whose avg_logprob is ``avg``; ``repetitive``: a compression ratio far
    above 2.4 (one token 40 times), else far below it."""
    body = [1500] * 40 if repetitive else list(text)
    if shape == "end":        # closes on a timestamp: the seek moves by the whole window
        tokens = [TB] + body + [TB + 100]
    elif shape == "pair":     # a consecutive pair, then unfinished text: the seek moves to the pair
        tokens = [TB] + body + [TB + 400, TB + 400, 1200, 1201]
    else:                     # no timestamps at all
        tokens = list(body)
    return WindowOutput(tokens, float(avg) * (len(tokens) + 1), float(nsp), int(lang))


def seg_tuple(sg):
    if isinstance(sg, dict):
        return (sg["seek"], sg["start"], sg["end"], list(sg["tokens"]), sg["temperature"], sg["avg_logprob"],
                sg["compression_ratio"], sg["no_speech_prob"])
    return (sg.seek, sg.start, sg.end, list(sg.tokens), sg.temperature, sg.avg_logprob, sg.compression_ratio,
            sg.no_speech_prob)


def one_window(script, opts, seconds=30.0):
    """A single clip through transcribe_clips with a dict script {temperature: WindowOutput}
    (or {(seek, temperature): ...})."""
    def fn(c, seek, t):
        return script[(seek, t)] if (seek, t) in script else script[t]
    eng = ScriptedEngine(fn)
    res = transcribe_clips(eng, [clip(seconds)], opts, TOK, ())
    return res[0], eng


# --------------------------------------------------------------------------- randomized scripts
def random_script(seed):
    def script(c, seek, t):
        rng = np.random.default_rng([seed, c, seek, int(round(t * 1000))])
        return out(avg=rng.choice([-0.3, -0.8, -1.4, -2.5]), repetitive=rng.random() < 0.35,
                   nsp=rng.choice([0.01, 0.5, 0.9]), text=tuple(int(x) for x in rng.integers(1000, 1100, rng.integers(1, 6))),
                   lang=ST.first_lang + c % 3, shape=rng.choice(["end", "pair", "none"]))
    return script


def random_opts(rng):
    ladder = [(0.0, 0.4, 0.8), (0.0, 0.2, 0.4, 0.6, 0.8, 1.0), (0.0, 0.6), (0.2, 0.7), (0.0,), 0.0][rng.integers(6)]
    return TranscribeOptions(
        temperature=ladder, seed=int(rng.integers(0, 2**40)), beam_size=int(rng.choice([1, 5])),
        best_of=int(rng.choice([1, 3, 5])), language=[None, "en"][rng.integers(2)],
        condition_on_previous_text=bool(rng.random() < 0.8),
        compression_ratio_threshold=[2.4, None][int(rng.random() < 0.25)],
        log_prob_threshold=[-1.0, None, -0.5][rng.integers(3)],
        no_speech_threshold=[0.6, None][int(rng.random() < 0.25)])


def check_against_reference(seed):
    rng = np.random.default_rng(seed)
    opts = random_opts(rng)
    temps = fr.temperatures(opts)
    script = random_script(seed)
    seconds = [float(rng.choice([12.0, 30.0, 47.5, 61.0, 85.0])) for _ in range(rng.integers(1, 4))]
    eng = ScriptedEngine(script, max_batch=int(rng.choice([1, 2, 4])), max_rows=int(rng.choice([5, 10, 20])))
    results = transcribe_clips(eng, [clip(s) for s in seconds], opts, TOK, ())
    given = TOK.language_token("en") if opts.language else None
    traces = []
    for c, (s, res) in enumerate(zip(seconds, results)):
        tr = fr.transcribe_clip(lambda seek, size, c=c: (lambda k, t, prefix, language: script(c, seek, t)),
                                len(clip(s)) // 160, opts, TOK, given)
        traces.append(tr)
        assert [seg_tuple(x) for x in res.segments] == [seg_tuple(x) for x in tr.segments], (seed, c)
        assert [x.id for x in res.segments] == list(range(len(res.segments)))
        if tr.language is not None:
            assert res.language == TOK.language_code(tr.language)
    # the calls: attempt 0 of a chunk without windows=, then its retries with the failing indices
    attempts = {(c, w["seek"]): w["attempts"] for c, tr in enumerate(traces) for w in tr.windows}
    prefixes = {(c, w["seek"]): w["prefix"] for c, tr in enumerate(traces) for w in tr.windows}
    seen, chunk_no, k, expect = {}, -1, 0, None
    group = max(max(1, opts.best_of) if t > 0 else max(1, opts.beam_size) for t in temps)
    for call in eng.calls:
        if call["windows"] is None:
            assert expect in (None, []), "a chunk's retries come before the next chunk"
            chunk_no, k = chunk_no + 1, 0
            idx = list(range(call["n"]))
            assert call["n"] <= max(1, min(eng.max_batch, eng.max_rows // group))
            for i, w in enumerate(call["wins"]):   # the prompt every window of the reference saw
                assert (call["prefix"][i] if call["prefix"] else []) == prefixes[(w[0], w[1])]
                assert (call["languages"] is None) == (given is None and not any(
                    x[0] == w[0] and x[1] < w[1] for x in seen))
        else:
            k += 1
            idx = call["windows"]
            assert idx == expect and idx, "retries carry exactly the windows that failed the attempt before"
            assert call["languages"] is not None and all(x is not None for x in call["languages"])
            for j, i in enumerate(idx):
                w = call["wins"][i]
                assert (call["prefix"][j] if call["prefix"] else []) == prefixes[(w[0], w[1])]
        t = temps[k]
        assert call["temperature"] == t and call["best_of"] == opts.best_of
        assert call["beam_size"] == (1 if t > 0 else opts.beam_size)
        assert call["seed"] == fr.attempt_seed(opts.seed, chunk_no, k)
        for i in idx:
            w = call["wins"][i]
            seen[(w[0], w[1])] = seen.get((w[0], w[1]), 0) + 1
        expect = [i for i in idx if attempts[(call["wins"][i][0], call["wins"][i][1])] > k + 1]
    assert expect in (None, [])
    assert seen == attempts, seed
    return len(temps) > 1 and any(v > 1 for v in attempts.values())


def test_random_scripts_match_the_reference():
    retried = sum(check_against_reference(seed) for seed in range(240))
    assert retried >= 60   # (the scripts do fail windows: the comparison is not vacuous)


# --------------------------------------------------------------------------- directed cases
def test_first_passing_temperature_wins():
    script = {0.0: out(-2.0), 0.4: out(-0.5, text=(1100, 1101)), 0.8: out(-0.1, text=(1200,))}
    res, eng = one_window(script, TranscribeOptions(temperature=LADDER))
    assert [c["temperature"] for c in eng.calls] == [0.0, 0.4]
    assert len(res.segments) == 1 and res.segments[0].temperature == 0.4
    assert res.segments[0].tokens == script[0.4].tokens and res.segments[0].avg_logprob == pytest.approx(-0.5)
    # a passing first attempt makes no retry
    res, eng = one_window({0.0: out(-0.5)}, TranscribeOptions(temperature=LADDER))
    assert len(eng.calls) == 1 and res.segments[0].temperature == 0.0
    # too repetitive at 0: the ratio test alone asks for the retry
    res, eng = one_window({0.0: out(-0.2, repetitive=True), 0.4: out(-0.9)}, TranscribeOptions(temperature=LADDER))
    assert [c["temperature"] for c in eng.calls] == [0.0, 0.4] and res.segments[0].temperature == 0.4


def test_silence_clears_the_fallback():
    res, eng = one_window({0.0: out(-2.0, nsp=0.9)}, TranscribeOptions(temperature=LADDER))
    assert len(eng.calls) == 1 and res.segments == []      # no retry, and the window is skipped as silence
    # without a no_speech_threshold the same window is retried
    script = {0.0: out(-2.0, nsp=0.9), 0.4: out(-0.5, nsp=0.9)}
    res, eng = one_window(script, TranscribeOptions(temperature=LADDER, no_speech_threshold=None))
    assert len(eng.calls) == 2 and res.segments[0].temperature == 0.4


def test_thresholds_of_none_switch_their_tests_off():
    res, eng = one_window({0.0: out(-2.0)}, TranscribeOptions(temperature=LADDER, log_prob_threshold=None))
    assert len(eng.calls) == 1 and res.segments[0].temperature == 0.0
    res, eng = one_window({0.0: out(-0.2, repetitive=True)},
                          TranscribeOptions(temperature=LADDER, compression_ratio_threshold=None))
    assert len(eng.calls) == 1 and res.segments[0].temperature == 0.0


@pytest.mark.parametrize("avgs,kept", [((-0.2, -1.5, -1.2), 0.8), ((-0.2, -1.2, -1.5), 0.4),
                                       ((-0.2, -1.3, -1.3), 0.4)])
def test_all_failed_some_below_the_ratio(avgs, kept):
    """Temperature 0 is too repetitive (whatever its avg_logprob), the others fail the
    log-probability test: the best of those below the ratio is kept (the first on a tie), and
    the last temperature is the window's."""
    script = {0.0: out(avgs[0], repetitive=True), 0.4: out(avgs[1], text=(1100, 1101)),
              0.8: out(avgs[2], text=(1200, 1201))}
    res, eng = one_window(script, TranscribeOptions(temperature=LADDER))
    assert [c["temperature"] for c in eng.calls] == [0.0, 0.4, 0.8]
    assert len(res.segments) == 1
    assert res.segments[0].tokens == script[kept].tokens
    assert res.segments[0].temperature == 0.8


def test_all_failed_none_below_the_ratio():
    script = {0.0: out(-0.5, repetitive=True), 0.4: out(-0.3, repetitive=True, text=()),
              0.8: out(-0.4, repetitive=True)}
    script[0.4].tokens[1] = 1501   # tell the three apart
    res, eng = one_window(script, TranscribeOptions(temperature=LADDER))
    assert len(eng.calls) == 3
    assert res.segments[0].tokens == script[0.4].tokens and res.segments[0].temperature == 0.8
    assert res.segments[0].avg_logprob == pytest.approx(-0.3)


def test_prompt_is_reset_by_the_windows_final_temperature():
    first_low = {(0, 0.0): out(-2.0), (0, 0.4): out(-0.5), (3000, 0.0): out(-0.5)}
    res, eng = one_window(first_low, TranscribeOptions(temperature=LADDER), seconds=60.0)
    second = [c for c in eng.calls if c["wins"][0][1] == 3000]
    assert second[0]["prefix"] == [[ST.sot_prev] + first_low[(0, 0.4)].tokens]   # 0.4 <= 0.5: the text conditions
    first_high = {(0, 0.0): out(-2.0), (0, 0.4): out(-2.0), (0, 0.8): out(-0.5), (3000, 0.0): out(-0.5)}
    res, eng = one_window(first_high, TranscribeOptions(temperature=LADDER), seconds=60.0)
    second = [c for c in eng.calls if c["wins"][0][1] == 3000]
    assert second[0]["prefix"] is None                                            # 0.8 > 0.5: reset
    assert [s.temperature for s in res.segments] == [0.8, 0.0]


# --------------------------------------------------------------------------- the calls
def test_retries_name_the_failing_windows_and_follow_the_seed_formula():
    fail = {0: (), 1: (0.0, 0.4), 2: (0.0,)}     # clip -> the temperatures it fails at

    def script(c, seek, t):
        return out(-2.0 if t in fail[c] else -0.5, lang=ST.first_lang + c)
    opts = TranscribeOptions(temperature=LADDER, seed=1234, beam_size=5, best_of=3)
    eng = ScriptedEngine(script, max_batch=4, max_rows=20)
    res = transcribe_clips(eng, [clip(30.0)] * 3, opts, TOK, ())
    assert [(c["windows"], c["temperature"], c["beam_size"], c["best_of"]) for c in eng.calls] == [
        (None, 0.0, 5, 3), ([1, 2], 0.4, 1, 3), ([1], 0.8, 1, 3)]
    assert [c["seed"] for c in eng.calls] == [1234, (1234 + 0x85EBCA6B) % 2**64, (1234 + 2 * 0x85EBCA6B) % 2**64]
    assert eng.calls[0]["languages"] is None                   # detected at attempt 0 ...
    assert eng.calls[1]["languages"] == [ST.first_lang + 1, ST.first_lang + 2]   # ... and named afterwards
    assert eng.calls[2]["languages"] == [ST.first_lang + 1]
    assert [r.segments[0].temperature for r in res] == [0.0, 0.8, 0.4]
    assert [r.language for r in res] == [TOK.language_code(ST.first_lang + c) for c in range(3)]


def test_chunk_size_uses_the_largest_row_group():
    eng = ScriptedEngine(lambda c, seek, t: out(-0.5), max_batch=4, max_rows=20)
    transcribe_clips(eng, [clip(30.0)] * 4, TranscribeOptions(temperature=(0.0, 0.4), beam_size=1, best_of=5), TOK, ())
    assert [c["n"] for c in eng.calls] == [4]          # 20 rows / 5 = 4 windows
    eng = ScriptedEngine(lambda c, seek, t: out(-0.5), max_batch=4, max_rows=10)
    transcribe_clips(eng, [clip(30.0)] * 4, TranscribeOptions(temperature=(0.0, 0.4), beam_size=1, best_of=5), TOK, ())
    assert [c["n"] for c in eng.calls] == [2, 2]       # greedy attempt 0, but the retries need 5 rows a window
    assert [c["seed"] for c in eng.calls] == [0, 0x9E3779B1]


@pytest.mark.parametrize("temperature", [0.0, 0.7, (0.7,)])
def test_scalar_temperature_makes_no_retry_and_keeps_its_seeds(temperature):
    eng = ScriptedEngine(lambda c, seek, t: out(-2.0), max_batch=2, max_rows=10)   # every window "fails"
    opts = TranscribeOptions(temperature=temperature, seed=99)
    res = transcribe_clips(eng, [clip(61.0), clip(30.0), clip(30.0)], opts, TOK, ())
    assert all(c["windows"] is None for c in eng.calls) and len(eng.calls) >= 3
    assert [c["seed"] for c in eng.calls] == [(99 + 0x9E3779B1 * i) % 2**64 for i in range(len(eng.calls))]
    t = 0.7 if temperature else 0.0
    assert {c["temperature"] for c in eng.calls} == {t}
    assert {c["beam_size"] for c in eng.calls} == {1 if t else 5}
    assert all(s.temperature == t for r in res for s in r.segments)


def test_stand_in_engines_without_the_keyword_keep_working():
    """Attempt 0 is the call of the parent commit: an engine whose decode() has no windows=
    serves every request that needs no retry."""
    class Old(ScriptedEngine):
        def decode(self, n, cfg, prefix=None, dump_steps=0, languages=None):
            return super().decode(n, cfg, prefix=prefix, dump_steps=dump_steps, languages=languages)
    eng = Old(lambda c, seek, t: out(-0.5))
    res = transcribe_clips(eng, [clip(30.0)], TranscribeOptions(temperature=LADDER), TOK, ())
    assert len(res[0].segments) == 1 and len(eng.calls) == 1


# --------------------------------------------------------------------------- options
def test_options_hold_a_float_or_a_tuple():
    d = TranscribeOptions()
    assert d.temperature == 0.0 and isinstance(d.temperature, float) and d.temperatures == (0.0,)
    assert d.key() == (d.task, d.language, d.initial_prompt, d.condition_on_previous_text, d.without_timestamps,
                       tuple(d.suppress_tokens), d.suppress_blank, d.beam_size, d.patience, d.length_penalty, 0.0,
                       d.best_of, d.tokens_per_second, d.max_new_tokens, d.word_timestamps, d.prepend_punctuations,
                       d.append_punctuations, 1.0, 0, False, False)
    lad = TranscribeOptions(temperature=[0.0, 0.2, 0.4])
    assert lad.temperature == (0.0, 0.2, 0.4) and lad.temperatures == (0.0, 0.2, 0.4)
    hash(lad.key())
    assert lad.key() != d.key() and lad.key() != TranscribeOptions(temperature=(0.0, 0.2)).key()
    one = TranscribeOptions(temperature=(0.3,))
    assert one.temperature == 0.3 and isinstance(one.temperature, float)
    assert one.key() == TranscribeOptions(temperature=0.3).key()
    assert TranscribeOptions(temperature=np.arange(0.0, 1.0 + 1e-6, 0.5)).temperature == (0.0, 0.5, 1.0)
    # a batch shares one opts: the thresholds separate requests
    for kw in (dict(compression_ratio_threshold=2.0), dict(log_prob_threshold=-0.5), dict(no_speech_threshold=0.5),
               dict(compression_ratio_threshold=None), dict(log_prob_threshold=None), dict(no_speech_threshold=None)):
        assert TranscribeOptions(**kw).key() != d.key(), kw
        hash(TranscribeOptions(**kw).key())
    assert TranscribeOptions(log_prob_threshold=-0.5).key() != TranscribeOptions(log_prob_threshold=-0.7).key()


@pytest.mark.parametrize("bad", [(), [], -0.1, (0.0, -0.2), float("nan"), (0.0, float("inf")), "0.2", (0.0, None),
                                 None])
def test_bad_temperatures_raise(bad):
    with pytest.raises(ValueError):
        TranscribeOptions(temperature=bad)


def test_sessions_stay_at_one_temperature():
    assert session_supported(TranscribeOptions())
    assert session_supported(TranscribeOptions(temperature=(0.0,)))
    assert not session_supported(TranscribeOptions(temperature=(0.0, 0.2)))
    assert not session_supported(TranscribeOptions(temperature=(0.0, 0.0)))
    assert not session_supported(TranscribeOptions(temperature=0.2))


# --------------------------------------------------------------------------- backend
ENV = "STT_HIP_TEMPERATURE_INCREMENT_ON_FALLBACK"


def test_env_ladder_follows_the_arange_rule(monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    assert fallback_temperatures(0.0) == 0.0 and fallback_temperatures(None) == 0.0
    assert fallback_temperatures(0.3) == 0.3
    assert fallback_temperatures([0.0, 0.5]) == (0.0, 0.5)
    monkeypatch.setenv(ENV, "0")
    assert fallback_temperatures(0.3) == 0.3
    for t, x in ((0.0, 0.2), (0.1, 0.25), (0.5, 0.5), (0.0, 0.3), (0.9, 0.2), (1.0, 0.2)):
        monkeypatch.setenv(ENV, str(x))
        want = tuple(float(v) for v in np.arange(t, 1.0 + 1e-6, x))
        got = fallback_temperatures(t)
        assert (got if isinstance(got, tuple) else (got,)) == want, (t, x)
        assert isinstance(got, tuple) == (len(want) > 1)
    monkeypatch.setenv(ENV, "0.2")
    assert len(fallback_temperatures(0.0)) == 6 and fallback_temperatures(0.0)[-1] == pytest.approx(1.0)
    assert fallback_temperatures((0.0, 0.5)) == (0.0, 0.5)     # an explicit ladder is not extended


class KwEngine(FakeEngine):
    """The scripted stand-in of test_backend_cpu with the windows= keyword, recording configurations."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.cfgs, self.session_cfgs = [], []

    def decode(self, n, cfg, prefix=None, dump_steps=0, languages=None, **kw):
        self.cfgs.append((cfg.temperature, kw.get("windows")))
        if "windows" not in kw:
            return super().decode(n, cfg, prefix=prefix, dump_steps=dump_steps, languages=languages)
        return [self.script(self._wins[i], -1, prefix[j] if prefix else [], languages[j])
                for j, i in enumerate(kw["windows"])]

    def session_begin(self, cfg):
        self.session_cfgs.append(cfg)
        return super().session_begin(cfg)


def backend_run(monkeypatch, env=None, avg=-2.0, continuous="0", **kw):
    monkeypatch.setenv("STT_HIP_CONTINUOUS", continuous)
    monkeypatch.delenv(ENV, raising=False)
    if env is not None:
        monkeypatch.setenv(ENV, env)
    holder = []

    def factory(dims, gpu, mb):
        e = KwEngine(dims, gpu, mb, lambda w, i, p, l: WindowOutput([TB, 1000, 1001, TB + 100], avg * 5, 0.01,
                                                                    ST.first_lang))
        holder.append(e)
        return e
    b = HipWhisperBackend(engine_factory=factory)
    try:
        r = b.transcribe(wav(30.0), MID, response_format="verbose_json", **kw)
    finally:
        b.unload_model(MID)
    return r, [c for e in holder for c in e.cfgs], [c for e in holder for c in e.session_cfgs]


def test_backend_passes_a_ladder_and_keeps_a_scalar(monkeypatch):
    r, cfgs, sess = backend_run(monkeypatch, temperature=[0.0, 0.4, 0.8])
    assert cfgs == [(0.0, None), (0.4, [0]), (0.8, [0])] and not sess
    assert [s["temperature"] for s in r["segments"]] == [0.8]
    # the scalar call of the reference: one decode, whatever the result looks like
    r, cfgs, sess = backend_run(monkeypatch)
    assert cfgs == [(0.0, None)] and [s["temperature"] for s in r["segments"]] == [0.0]
    r, cfgs, sess = backend_run(monkeypatch, temperature=0.3)
    assert cfgs == [(pytest.approx(0.3), None)]
    # the env knob turns the scalar into openai-whisper's ladder
    r, cfgs, sess = backend_run(monkeypatch, env="0.5")
    assert cfgs == [(0.0, None), (0.5, [0]), (1.0, [0])]
    # the thresholds travel with the request: a looser one accepts attempt 0
    r, cfgs, sess = backend_run(monkeypatch, temperature=[0.0, 0.4], log_prob_threshold=-3.0)
    assert cfgs == [(0.0, None)]
    r, cfgs, sess = backend_run(monkeypatch, temperature=[0.0, 0.4], avg=-0.2)
    assert cfgs == [(0.0, None)]
    # a ladder request takes the batched seek loop of an idle lane, a scalar one a session
    r, cfgs, sess = backend_run(monkeypatch, continuous="1", temperature=[0.0, 0.4])
    assert cfgs == [(0.0, None), (0.4, [0])] and not sess
    r, cfgs, sess = backend_run(monkeypatch, continuous="1")
    assert sess and not cfgs


def test_translate_takes_the_ladder(monkeypatch):
    monkeypatch.setenv("STT_HIP_CONTINUOUS", "0")
    monkeypatch.delenv(ENV, raising=False)
    holder = []

    def factory(dims, gpu, mb):
        e = KwEngine(dims, gpu, mb, lambda w, i, p, l: WindowOutput([TB, 1000, TB + 100], -8.0, 0.01, ST.first_lang))
        holder.append(e)
        return e
    b = HipWhisperBackend(engine_factory=factory)
    try:
        b.translate(wav(30.0), MID, temperature=(0.0, 1.0), compression_ratio_threshold=2.0, log_prob_threshold=-1.5)
    finally:
        b.unload_model(MID)
    assert [c for e in holder for c in e.cfgs] == [(0.0, None), (1.0, [0])]


def test_new_entries_are_in_the_header_and_the_binding():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "osw.h")) as f:
        header = f.read()
    for name in ("osw_decode_window_list", "osw_debug_dec_xattn_windows"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in _lib.EXPORTED
    assert len(_lib._SIGS["osw_decode_window_list"][1]) == 5
    assert len(_lib._SIGS["osw_debug_dec_xattn_windows"][1]) == 12
    assert re.search(r'"osw-hip 0\.2 gfx950"', open(os.path.join(root, "open-speech_amd", "csrc", "osw.hip")).read())
