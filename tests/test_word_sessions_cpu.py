"""Word-timestamp requests on the continuous-batching lanes, host side: a stub engine that
scripts every window's decode output and alignment from the window itself (clip length and seek),
serves both the batched interface (log_mel / encode / decode / align) and the session one
(session_begin(hold) / add / step / align / release) and records every call.  Checked: the
routing (segments.word_session_supported, the engine's session_align, STT_HIP_WORD_SESSIONS), the
hold discipline of runner._SessionLane (everything a step returned is aligned or released before
the next step, one session_align per step for all of its windows with text, silence and
no-text windows released, a request that fails after its window finished releases it), and that
the lanes return what transcribe_clips returns on the same outputs."""

import numpy as np
import pytest

from open_speech_amd import segments as S
from open_speech_amd.dims import SpecialTokens
from open_speech_amd.engine import Alignment, WhisperEngine, WindowOutput
from open_speech_amd.runner import BatchRunner
from open_speech_amd.tokenizer import WhisperTokenizer

import tokfix

N_VOCAB = 51866
ST = SpecialTokens.for_vocab(N_VOCAB)
TB = ST.timestamp_begin
HELLO = " Hello world."


@pytest.fixture(scope="module")
def tok(tmp_path_factory):
    return WhisperTokenizer(N_VOCAB, tokfix.build_tokenizer_json(str(tmp_path_factory.mktemp("tok") / "tokenizer.json")))


def clip(frames):
    return np.zeros(160 * frames, np.int16)


class Script:
    """The decode output of window (clip frames, seek) and the alignment of a token list.
    A 1000-frame clip: text ending in a timestamp pair at seek 0 (the last word ends at 0.80 s, so
    the next window starts at frame 80), a lone timestamp at seek 80 (no text: the seek moves
    by 200), silence after that.  A 1200-frame clip: text ending in a single timestamp (consumed
    whole).  A 700-frame clip: an output the seek loop cannot digest (tokens None)."""

    def __init__(self, tok):
        self.ids = tok.encode(HELLO)
        self.al = Alignment(np.array([0, 5, 25, 40, 50]), np.array([0.5, 0.7, 0.9, 0.3]))

    def out(self, frames, seek):
        text = WindowOutput(tokens=[TB] + self.ids + [TB + 100, TB + 100], sum_logprob=-1.0, no_speech_prob=0.1,
                            language=ST.first_lang)
        if frames == 700:
            return WindowOutput(tokens=None, sum_logprob=-1.0, no_speech_prob=0.1, language=ST.first_lang)
        if frames == 1200:
            return WindowOutput(tokens=text.tokens[:-1], sum_logprob=-2.0, no_speech_prob=0.2, language=ST.first_lang)
        if seek == 0:
            return text
        if seek == 80:
            return WindowOutput(tokens=[TB + 100], sum_logprob=-1.0, no_speech_prob=0.1, language=ST.first_lang)
        return WindowOutput(tokens=[], sum_logprob=-50.0, no_speech_prob=0.95, language=ST.first_lang)

    def align(self, w):
        assert list(w.tokens) == self.ids
        return self.al


class BatchedEngine:
    """The batched interface only: what the stand-in engines of the older CPU tests offer."""
    max_batch = 4
    max_rows = 20

    def __init__(self, script):
        self.script, self.log, self.windows = script, [], []

    def log_mel(self, clips):
        self._frames = [len(c) // 160 for c in clips]
        return [f + 1 for f in self._frames]

    def encode(self, wins):
        self._wins = list(wins)
        self.windows += [(self._frames[i], seek, size) for i, seek, size in wins]

    def decode(self, n, cfg, prefix=None, languages=None):
        self.log.append(("decode", n))
        return [self.script.out(self._frames[i], seek) for i, seek, _ in self._wins]

    def align(self, windows):
        self.log.append(("align", len(windows)))
        return [self.script.align(w) for w in windows]

    # (sessions without hold, so that requests without word timing still ride them)
    def session_begin(self, cfg):
        self.log.append(("begin", False))
        self._sess = dict(q=[], clips={}, held=set(), hold=False)

    def session_add(self, wins):
        s = self._sess
        for w in wins:
            if w.get("pcm") is not None:
                s["clips"][w["clip"]] = len(w["pcm"]) // 160
            s["q"].append(w)
        self.log.append(("add", [w["tag"] for w in wins]))

    def session_step(self, max_chunks=1, refill_min=1):
        s = self._sess
        if s["held"]:
            self.log.append(("violation", sorted(s["held"])))   # a step with windows still held
        if max_chunks == 0:
            return [], len(s["q"]), 0
        done = []
        for w in s["q"][:self.max_batch]:      # every admitted window finishes in its first step
            frames = s["clips"][w["clip"]]
            self.windows.append((frames, w["seek"], w["segment_size"]))
            done.append((w["tag"], self.script.out(frames, w["seek"])))
        del s["q"][:self.max_batch]
        if s["hold"]:
            s["held"].update(t for t, _ in done)
        self.log.append(("step", [t for t, _ in done]))
        return done, 0, len(s["q"])

    def session_release_clip(self, key):
        self._sess["clips"].pop(key, None)

    def session_end(self):
        self.log.append(("end", sorted(self._sess["held"])))
        self._sess = None


class SessionEngine(BatchedEngine):
    """... and the hold / align / release calls."""

    def session_begin(self, cfg, hold=False):
        super().session_begin(cfg)
        self.log[-1] = ("begin", hold)
        self._sess["hold"] = hold

    def session_align(self, windows):
        tags = [t for t, _ in windows]
        assert set(tags) <= self._sess["held"] and len(set(tags)) == len(tags)
        self._sess["held"].difference_update(tags)
        self.log.append(("session_align", tags))
        return [self.script.align(w) for _, w in windows]

    def session_release(self, tags):
        tags = list(tags)
        assert set(tags) <= self._sess["held"] and len(set(tags)) == len(tags)
        self._sess["held"].difference_update(tags)
        self.log.append(("release", tags))


OPTS = dict(language="en", word_timestamps=True, beam_size=1)


def run_lanes(eng, tok, clips, opts, timeout=30):
    """The clips as concurrent requests of one continuous lane, queued together."""
    runner = BatchRunner([eng], tok, continuous=True)
    try:
        dq = runner.queues[0]
        with dq.cv:                                  # (the lane takes them in one admission)
            futs = [runner.submit(c, opts) for c in clips]
        out = []
        for f in futs:
            try:
                out.append(f.result(timeout=timeout))
            except Exception as e:  # noqa: BLE001 - the request's own failure
                out.append(e)
        return out
    finally:
        runner.close()


def names(log):
    return [n for n, _ in log]


def test_exists_only_with_the_feature():
    assert callable(S.word_session_supported) and callable(S.plan_window) and callable(S.apply_window)
    for name in ("session_align", "session_release", "session_hold"):
        assert callable(getattr(WhisperEngine, name))


def test_word_session_supported():
    on = S.TranscribeOptions(word_timestamps=True)
    assert S.word_session_supported(on) and not S.session_supported(on)
    assert not S.word_session_supported(S.TranscribeOptions())              # nothing to hold
    for kw in (dict(temperature=(0.0, 0.2)), dict(temperature=0.4), dict(max_new_tokens=10), dict(beam_size=6),
               dict(detect_only=True)):
        assert not S.word_session_supported(S.TranscribeOptions(word_timestamps=True, **kw)), kw
        assert not S.session_supported(S.TranscribeOptions(**kw)), kw
    assert S.word_session_supported(S.TranscribeOptions(word_timestamps=True, beam_size=5, repetition_penalty=1.2,
                                                        token_logprobs=True))


def test_routing_by_options_engine_and_knob(tok, monkeypatch):
    script = Script(tok)
    monkeypatch.delenv("STT_HIP_WORD_SESSIONS", raising=False)
    # the default: a session with hold
    eng = SessionEngine(script)
    run_lanes(eng, tok, [clip(1200)], S.TranscribeOptions(**OPTS))
    assert ("begin", True) in eng.log and "session_align" in names(eng.log) and "decode" not in names(eng.log)
    # an engine without session_align keeps the batched seek loop
    eng = BatchedEngine(script)
    run_lanes(eng, tok, [clip(1200)], S.TranscribeOptions(**OPTS))
    assert "begin" not in names(eng.log) and "decode" in names(eng.log) and "align" in names(eng.log)
    # STT_HIP_WORD_SESSIONS=0 too; any other value leaves the default
    for knob, sess in (("0", False), ("1", True), ("", True)):
        monkeypatch.setenv("STT_HIP_WORD_SESSIONS", knob)
        eng = SessionEngine(script)
        run_lanes(eng, tok, [clip(1200)], S.TranscribeOptions(**OPTS))
        assert ("session_align" in names(eng.log)) == sess and ("decode" in names(eng.log)) == (not sess), knob
    monkeypatch.delenv("STT_HIP_WORD_SESSIONS")
    # a request the sessions cannot hold stays batched, one without word timing holds nothing
    eng = SessionEngine(script)
    run_lanes(eng, tok, [clip(1200)], S.TranscribeOptions(temperature=(0.0, 0.2), **OPTS))
    assert "begin" not in names(eng.log) and "align" in names(eng.log)
    eng = SessionEngine(script)
    run_lanes(eng, tok, [clip(1200)], S.TranscribeOptions(language="en", beam_size=1))
    assert ("begin", False) in eng.log and not {"session_align", "release", "align"} & set(names(eng.log))


def test_hold_discipline_and_results_equal_transcribe_clips(tok):
    script = Script(tok)
    clips = [clip(1000), clip(1200), clip(1000)]
    opts = S.TranscribeOptions(**OPTS)
    eng = SessionEngine(script)
    res = run_lanes(eng, tok, clips, opts)
    log = eng.log
    assert "violation" not in names(log), log
    assert log[0] == ("begin", True) and log[-1] == ("end", [])        # nothing left held
    # after every step: at most one session_align, holding exactly the step's windows with text,
    # and the others released, all before the next step
    steps = [i for i, (n, _) in enumerate(log) if n == "step"]
    text_steps = 0
    for a, b in zip(steps, steps[1:] + [len(log)]):
        done = log[a][1]
        between = log[a + 1:b]
        aligned = [t for n, tags in between if n == "session_align" for t in tags]
        released = [t for n, tags in between if n == "release" for t in tags]
        assert names(between).count("session_align") <= 1, between
        assert sorted(aligned + released) == sorted(done), (done, between)
        text_steps += len(aligned) >= 2
    assert text_steps >= 1                       # the first windows of the three clips went in one call
    # the three kinds of window: text (aligned), no text and silence (released)
    n_aligned = sum(len(tags) for n, tags in log if n == "session_align")
    n_released = sum(len(tags) for n, tags in log if n == "release")
    assert (n_aligned, n_released) == (3, 4), log   # 1000-frame clips: text, no text, silence; 1200: text
    # ... and the results are transcribe_clips' on the same outputs, window for window
    ref = BatchedEngine(script)
    want = S.transcribe_clips(ref, clips, opts, tok, ())
    assert sorted(eng.windows) == sorted(ref.windows)
    assert (1000, 80, 920) in eng.windows and (1000, 280, 720) in eng.windows   # the seek moved by the last word's end
    for r, w in zip(res, want):
        assert r.segments and r.segments == w.segments
        assert [s.words for s in r.segments] == [s.words for s in w.segments] and all(s.words for s in r.segments)
        assert [s.seek for s in r.segments] == [s.seek for s in w.segments]
        assert r == w


def test_a_request_failing_after_its_window_finished_releases_it(tok):
    script = Script(tok)
    eng = SessionEngine(script)
    res = run_lanes(eng, tok, [clip(700), clip(1200)], S.TranscribeOptions(**OPTS))
    assert isinstance(res[0], TypeError) and isinstance(res[1], S.ClipResult) and res[1].segments[0].words
    log = eng.log
    assert "violation" not in names(log) and log[-1] == ("end", []), log
    first = log[[n for n, _ in log].index("step")]
    assert len(first[1]) == 2
    bad = first[1][0]
    assert ("release", [bad]) in log and ("session_align", [first[1][1]]) in log
    # the lane is left without a held slot: the next request runs through the same lane
    eng2 = SessionEngine(script)
    res = run_lanes(eng2, tok, [clip(700)], S.TranscribeOptions(**OPTS))
    assert isinstance(res[0], TypeError) and eng2.log[-1] == ("end", []) and "violation" not in names(eng2.log)


def test_session_align_refusal_ends_the_session_and_fails_its_requests(tok):
    class Refusing(SessionEngine):
        def session_align(self, windows):
            raise ValueError("refused")
    eng = Refusing(Script(tok))
    res = run_lanes(eng, tok, [clip(1200)], S.TranscribeOptions(**OPTS))
    assert isinstance(res[0], ValueError)
    assert eng.log[-1][0] == "end"            # the lane's handler ended the session, which frees what is held
