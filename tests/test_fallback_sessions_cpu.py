"""A temperature ladder on the continuous-batching lanes, host side: a stand-in engine that scripts
every window's decode output from (clip frames, seek, temperature), serves the batched interface
(log_mel / encode / decode with ``windows=`` / align) and the session one (session_begin(hold,
retries) / add / step / retry / align / release) and records every call.  Checked: the predicate
``segments.fallback_session_supported`` (and that the two older predicates answer as before), the
routing (the engine's ``session_retry``, STT_HIP_FALLBACK_SESSIONS), and that ``runner._SessionLane``
drives the retries by the rule of DESIGN.md section 4.6: against tests/fallback_ref.py, a
window-by-window restatement, the segments with their temperatures, the prompts, and the retry
calls' tags, temperatures, seeds (``attempt_seed(seed, window number, attempt)``) and languages are
equal, and no step ever runs with a window still held."""
import dataclasses

import os
import tempfile

import numpy as np

import fallback_ref as fr
import tokfix
import test_word_sessions_cpu as tw
from open_speech_amd import segments as S
from open_speech_amd.engine import WhisperEngine, WindowOutput
from open_speech_amd.tokenizer import WhisperTokenizer
from test_fallback_cpu import ST, TOK, ScriptedEngine, clip, out, seg_tuple
from test_word_sessions_cpu import names, run_lanes


class NoRetryEngine(ScriptedEngine):
    """``script(clip frames, seek, temperature) -> WindowOutput``.  A session window finishes in the
    first step after its admission or its retry; at most ``max_batch`` windows hold slots.  This
    class has the sessions of the parent commit (hold / align / release), ``RetryEngine`` below adds
    the retries."""

    def __init__(self, script, max_batch=4, align=None):
        super().__init__(lambda c, seek, t: script(self._frames[c], seek, t), max_batch=max_batch, max_rows=5 * max_batch)
        self.raw, self.log, self.prompts, self._align = script, [], {}, align

    def log_mel(self, clips):
        self._frames = [len(c) // 160 for c in clips]
        return super().log_mel(clips)

    def decode(self, n, cfg, **kw):
        self.log.append(("decode", n))
        return super().decode(n, cfg, **kw)

    def align(self, windows):
        self.log.append(("align", len(windows)))
        return [self._align(w) for w in windows]

    def session_begin(self, cfg, hold=False):
        assert cfg.temperature == 0
        self.log.append(("begin", (hold, None)))
        self._sess = dict(q=[], clips={}, slots={}, held=set(), hold=hold, retries=None)

    def session_add(self, wins):
        s = self._sess
        for w in wins:
            if w.get("pcm") is not None:
                s["clips"][w["clip"]] = len(w["pcm"]) // 160
            s["q"].append(w)
            self.prompts.setdefault(w["clip"], []).append(list(w["prefix"]))
        self.log.append(("add", [w["tag"] for w in wins]))

    def session_step(self, max_chunks=1, refill_min=1):
        s = self._sess
        if s["held"]:
            self.log.append(("violation", sorted(s["held"])))   # a step with windows still held
        while s["q"] and len(s["slots"]) < self.max_batch:
            w = s["q"].pop(0)
            s["slots"][w["tag"]] = dict(w=w, t=0.0, decoding=True)
        if max_chunks == 0:
            return [], sum(x["decoding"] for x in s["slots"].values()), len(s["q"])
        done = []
        for tag, x in s["slots"].items():
            if x["decoding"]:
                done.append((tag, self.raw(s["clips"][x["w"]["clip"]], x["w"]["seek"], x["t"])))
                x["decoding"] = False
        if s["hold"]:
            s["held"].update(t for t, _ in done)
        else:
            for t, _ in done:
                del s["slots"][t]
        self.log.append(("step", [t for t, _ in done]))
        return done, 0, len(s["q"])

    def _take_held(self, tags):
        tags = list(tags)
        assert set(tags) <= self._sess["held"] and len(set(tags)) == len(tags), (tags, self._sess["held"])
        self._sess["held"].difference_update(tags)
        return tags

    def session_release(self, tags):
        for tag in self._take_held(tags):
            del self._sess["slots"][tag]
        self.log.append(("release", list(tags)))

    def session_align(self, windows):
        for tag in self._take_held([t for t, _ in windows]):
            del self._sess["slots"][tag]
        self.log.append(("session_align", [t for t, _ in windows]))
        return [self._align(w) for _, w in windows]

    def session_release_clip(self, key):
        self._sess["clips"].pop(key, None)

    def session_end(self):
        self.log.append(("end", sorted(self._sess["held"])))
        self._sess = None


class RetryEngine(NoRetryEngine):
    def session_begin(self, cfg, hold=False, retries=None):
        assert retries is None or hold
        super().session_begin(cfg, hold)
        self.log[-1] = ("begin", (hold, retries))
        self._sess["retries"] = retries

    def session_retry(self, entries):
        assert self._sess["retries"] is not None and entries
        for tag in self._take_held([e[0] for e in entries]):
            self._sess["slots"][tag]["decoding"] = True
        for tag, t, seed, lang in entries:
            assert t > 0
            self._sess["slots"][tag]["t"] = t
        self.log.append(("retry", [tuple(e) for e in entries]))


def test_exists_only_with_the_feature():
    assert callable(S.fallback_session_supported) and callable(S.attempt_seed) and callable(S.fallback_verdict)
    assert callable(WhisperEngine.session_retry) and callable(WhisperEngine.session_retries)


def test_attempt_seed_is_the_documented_formula():
    for seed, n, k in ((0, 0, 0), (77, 3, 2), (2**64 - 1, 5, 1), (2**40 + 17, 123, 5)):
        assert S.attempt_seed(seed, n, k) == fr.attempt_seed(seed, n, k) == (seed + 0x9E3779B1 * n + 0x85EBCA6B * k) % 2**64


def test_predicate_truth_table():
    O = S.TranscribeOptions
    yes = [dict(temperature=(0.0, 0.2)), dict(temperature=(0.0, 0.2, 0.4, 0.6, 0.8, 1.0)), dict(temperature=(0.0, 1.0), best_of=1),
           dict(temperature=(0.0, 0.4), beam_size=1, best_of=3), dict(temperature=(0.0, 0.4), word_timestamps=True),
           dict(temperature=(0.0, 0.4), repetition_penalty=1.2, token_logprobs=True, tokens_per_second=4.0),
           dict(temperature=[0, 0.5]), dict(temperature=(0.0, 0.4), chunk_length=5)]
    no = [dict(), dict(temperature=0.0), dict(temperature=(0.0,)), dict(temperature=0.4), dict(temperature=(0.2, 0.4)),
          dict(temperature=(0.0, 0.0)), dict(temperature=(0.0, 0.4, 0.0)), dict(temperature=(0.0, 0.4), best_of=0),
          dict(temperature=(0.0, 0.4), best_of=6), dict(temperature=(0.0, 0.4), beam_size=6),
          dict(temperature=(0.0, 0.4), max_new_tokens=10), dict(temperature=(0.0, 0.4), detect_only=True),
          dict(temperature=(0.0, 0.4), word_timestamps=True, beam_size=8)]
    for kw in yes:
        assert S.fallback_session_supported(O(**kw)), kw
        # the older predicates answer what they answered: False for any ladder
        assert not S.session_supported(O(**kw)) and not S.word_session_supported(O(**kw)), kw
    for kw in no:
        assert not S.fallback_session_supported(O(**kw)), kw
    assert S.session_supported(O()) and S.session_supported(O(temperature=(0.0,)))
    assert S.word_session_supported(O(word_timestamps=True)) and not S.session_supported(O(word_timestamps=True))
    for kw in (dict(temperature=0.4), dict(max_new_tokens=10), dict(beam_size=6), dict(detect_only=True)):
        assert not S.session_supported(O(**kw)) and not S.word_session_supported(O(word_timestamps=True, **kw)), kw


LADDER = dict(language="en", beam_size=1, temperature=(0.0, 0.4, 0.8))


def passing(frames, seek, t):
    return out(-0.3)


def test_routing_by_engine_and_knob(monkeypatch):
    monkeypatch.delenv("STT_HIP_FALLBACK_SESSIONS", raising=False)
    opts = S.TranscribeOptions(**LADDER)
    eng = RetryEngine(passing)
    run_lanes(eng, TOK, [clip(30.0)], opts)
    assert ("begin", (True, 5)) in eng.log and "decode" not in names(eng.log)
    # an engine without session_retry keeps the batched seek loop
    eng = NoRetryEngine(passing)
    assert not hasattr(eng, "session_retry")
    run_lanes(eng, TOK, [clip(30.0)], opts)
    assert "begin" not in names(eng.log) and "decode" in names(eng.log)
    for knob, sess in (("0", False), ("1", True), ("", True)):
        monkeypatch.setenv("STT_HIP_FALLBACK_SESSIONS", knob)
        eng = RetryEngine(passing)
        run_lanes(eng, TOK, [clip(30.0)], opts)
        assert ("begin" in names(eng.log)) == sess and ("decode" in names(eng.log)) == (not sess), knob
    monkeypatch.delenv("STT_HIP_FALLBACK_SESSIONS")
    # what no session holds stays batched; a ladder-free request begins a session without retries
    for kw in (dict(temperature=(0.2, 0.6)), dict(temperature=0.4), dict(temperature=(0.0, 0.4), best_of=6)):
        eng = RetryEngine(passing)
        run_lanes(eng, TOK, [clip(30.0)], S.TranscribeOptions(**{**LADDER, **kw}))
        assert "begin" not in names(eng.log) and "decode" in names(eng.log), kw
    eng = RetryEngine(passing)
    run_lanes(eng, TOK, [clip(30.0)], S.TranscribeOptions(language="en", beam_size=1))
    assert ("begin", (False, None)) in eng.log and "retry" not in names(eng.log)
    # word timing with a ladder needs both capabilities and both knobs
    monkeypatch.setenv("STT_HIP_WORD_SESSIONS", "0")
    eng = RetryEngine(passing, align=lambda w: None)
    assert not BatchLaneProbe(eng).ok(S.TranscribeOptions(word_timestamps=True, **LADDER))
    monkeypatch.delenv("STT_HIP_WORD_SESSIONS")
    assert BatchLaneProbe(eng).ok(S.TranscribeOptions(word_timestamps=True, **LADDER))


class BatchLaneProbe:
    """_SessionLane._session_ok of a one-lane continuous runner over `eng`."""

    def __init__(self, eng):
        self.eng = eng

    def ok(self, opts):
        from open_speech_amd.runner import BatchRunner
        runner = BatchRunner([self.eng], TOK, continuous=True)
        try:
            return runner.queues[0].lanes[0]._session_ok(opts)
        finally:
            runner.close()


def random_script(seed):
    def script(frames, seek, t):
        rng = np.random.default_rng([seed, frames, seek, int(round(t * 1000))])
        return out(avg=rng.choice([-0.3, -0.8, -1.4, -2.5]), repetitive=rng.random() < 0.35,
                   nsp=rng.choice([0.01, 0.5, 0.9]), text=tuple(int(x) for x in rng.integers(1000, 1100, rng.integers(1, 6))),
                   lang=ST.first_lang + frames % 3, shape=rng.choice(["end", "pair", "none"]))
    return script


def random_opts(rng):
    ladder = [(0.0, 0.4, 0.8), (0.0, 0.2, 0.4, 0.6, 0.8, 1.0), (0.0, 0.6)][rng.integers(3)]
    return S.TranscribeOptions(
        temperature=ladder, seed=int(rng.integers(0, 2**40)), beam_size=int(rng.choice([1, 5])),
        best_of=int(rng.choice([1, 3, 5])), language=[None, "en"][rng.integers(2)],
        condition_on_previous_text=bool(rng.random() < 0.8),
        compression_ratio_threshold=[2.4, None][int(rng.random() < 0.25)],
        log_prob_threshold=[-1.0, None, -0.5][rng.integers(3)],
        no_speech_threshold=[0.6, None][int(rng.random() < 0.25)])


def check_lane_against_reference(seed):
    rng = np.random.default_rng(seed)
    opts = random_opts(rng)
    temps = fr.temperatures(opts)
    script = random_script(seed)
    seconds = [float(s) for s in rng.choice([12.0, 30.0, 47.5, 61.0, 85.0], size=rng.integers(1, 4), replace=False)]
    eng = RetryEngine(script, max_batch=int(rng.choice([1, 2, 4])))
    results = run_lanes(eng, TOK, [clip(s) for s in seconds], opts)
    log = eng.log
    assert "violation" not in names(log) and "decode" not in names(log), (seed, log)
    assert log[0] == ("begin", (True, opts.best_of)) and log[-1] == ("end", []), (seed, log[0], log[-1])
    given = TOK.language_token("en") if opts.language else None
    retries = {}       # tag -> [(temperature, seed, language)] in order
    for n, v in log:
        if n == "retry":
            assert len({e[0] for e in v}) == len(v)
            for tag, t, sd, lang in v:
                retries.setdefault(tag, []).append((t, sd, lang))
    # between two steps: at most one retry call, and everything the step returned is retried or released
    steps = [i for i, (n, _) in enumerate(log) if n == "step"]
    for a, b in zip(steps, steps[1:] + [len(log)]):
        between = log[a + 1:b]
        assert names(between).count("retry") <= 1, (seed, between)
        moved = [e[0] for n, v in between if n == "retry" for e in v] + [t for n, v in between if n == "release" for t in v]
        assert sorted(moved) == sorted(log[a][1]), (seed, log[a], between)
    any_retry = False
    for c, (sec, res) in enumerate(zip(seconds, results)):
        frames = len(clip(sec)) // 160
        tr = fr.transcribe_clip(lambda seek, size: (lambda k, t, prefix, language: script(frames, seek, t)),
                                frames, opts, TOK, given)
        assert isinstance(res, S.ClipResult), (seed, res)
        assert [seg_tuple(x) for x in res.segments] == [seg_tuple(x) for x in tr.segments], (seed, c)
        tag = c + 1     # (the requests were taken in order)
        assert eng.prompts[tag] == [w["prefix"] for w in tr.windows], (seed, c)
        if tr.language is not None:
            assert res.language == TOK.language_code(tr.language)
        # the retry calls of this clip, window by window: temperatures 1 .. attempts-1 of the ladder,
        # the documented seeds, the language attempt 0 of the clip's first window reported
        want = [(temps[k], fr.attempt_seed(opts.seed, n, k), given if given is not None else tr.language)
                for n, w in enumerate(tr.windows) for k in range(1, w["attempts"])]
        assert retries.get(tag, []) == want, (seed, c)
        any_retry = any_retry or bool(want)
    # ... and the lanes return what the batched loop returns for each clip alone
    for sec, res in zip(seconds, results):
        alone = S.transcribe_clips(RetryEngine(script), [clip(sec)], opts, TOK, ())[0]
        assert res == alone, seed
    return any_retry


def test_random_scripts_match_the_reference():
    retried = sum(check_lane_against_reference(seed) for seed in range(60))
    assert retried >= 20   # (the scripts do fail windows: the comparison is not vacuous)


def one_clip(script, opts, seconds=30.0, **kw):
    eng = RetryEngine(script, **kw)
    res = run_lanes(eng, TOK, [clip(seconds)], opts)[0]
    assert "violation" not in names(eng.log) and eng.log[-1] == ("end", [])
    return res, eng


def test_every_temperature_failed():
    """All three attempts fail: the kept result is the best avg_logprob among those below the ratio,
    the window's temperature the last one tried (so the prompt is reset after it)."""
    by_t = {0.0: out(-2.0, text=(1001,)), 0.4: out(-1.2, text=(1002,)), 0.8: out(-1.1, repetitive=True)}
    res, eng = one_clip(lambda f, seek, t: by_t[t] if seek == 0 else out(-0.3, text=(1003,)), S.TranscribeOptions(**LADDER),
                        seconds=45.0)
    assert [e[1] for n, v in eng.log if n == "retry" for e in v] == [0.4, 0.8]
    assert res.segments[0].tokens[1] == 1002 and res.segments[0].temperature == 0.8
    assert res.segments[1].temperature == 0.0
    assert eng.prompts[1][1] == []           # 0.8 > prompt_reset_on_temperature: no previous text for window 2


def test_silence_clears_the_retry():
    """A low avg_logprob with a high no-speech probability needs no fallback: the window is
    released without a retry and skipped as silence."""
    res, eng = one_clip(lambda f, seek, t: out(-2.0, nsp=0.9), S.TranscribeOptions(**LADDER))
    assert "retry" not in names(eng.log) and ("release", [1]) in eng.log and res.segments == []


def test_a_request_failing_while_held_releases_its_window():
    """Clip 1's retry returns an output the lane cannot digest: the request fails, its held
    window is released, and clip 2 goes on through its own retry."""
    def script(frames, seek, t):
        if frames == 1000 and t > 0:
            return WindowOutput(tokens=None, sum_logprob=-1.0, no_speech_prob=0.1, language=ST.first_lang)
        return out(-2.0 if t == 0 else -0.3)
    eng = RetryEngine(script)
    res = run_lanes(eng, TOK, [clip(10.0), clip(20.0)], S.TranscribeOptions(**LADDER))
    assert isinstance(res[0], TypeError) and isinstance(res[1], S.ClipResult) and res[1].segments[0].temperature == 0.4
    assert "violation" not in names(eng.log) and eng.log[-1] == ("end", [])
    assert ("release", [1]) in eng.log
    assert [sorted(e[0] for e in v) for n, v in eng.log if n == "retry"] == [[1, 2]]


def test_ladder_with_word_timestamps_aligns_once_on_the_kept_result():
    """tests/test_word_sessions_cpu.py's script with the first window of every clip failing at
    temperature 0: it is retried, and only the kept result is aligned, once; the words and
    segments are transcribe_clips'."""
    with tempfile.TemporaryDirectory() as d:
        tk = WhisperTokenizer(tw.N_VOCAB, tokfix.build_tokenizer_json(os.path.join(d, "tokenizer.json")))
    base = tw.Script(tk)

    def script(frames, seek, t):
        o = base.out(frames, seek)
        if seek == 0 and t == 0:
            o = dataclasses.replace(o, sum_logprob=-3.0 * (len(o.tokens) + 1))
        return o
    opts = S.TranscribeOptions(language="en", beam_size=1, word_timestamps=True, temperature=(0.0, 0.4))
    clips = [tw.clip(1000), tw.clip(1200)]
    eng = RetryEngine(script, align=base.align)
    res = run_lanes(eng, tk, clips, opts)
    log = eng.log
    assert "violation" not in names(log) and log[0] == ("begin", (True, 5)) and log[-1] == ("end", [])
    assert [sorted(e[0] for e in v) for n, v in log if n == "retry"] == [[1, 2]]
    assert [sorted(v) for n, v in log if n == "session_align"] == [[1, 2]]     # once, after the retry
    want = S.transcribe_clips(RetryEngine(script, align=base.align), clips, opts, tk, ())
    for r, w in zip(res, want):
        assert r == w and r.segments and all(s.words for s in r.segments)
        assert r.segments[0].temperature == 0.4
