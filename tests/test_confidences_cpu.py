"""Per-token log-probabilities and language probabilities, host side (no GPU): the slices of
``token_logprobs`` stay aligned with ``tokens`` through the segment split, the response shapes
with ``include=["logprobs"]`` on and off, the options key, faster-whisper's language_probability
semantics, the C ABI's new prototypes and the pinned struct sizes.  The engine is the scripted
stand-in of test_backend_cpu.py; a token's scripted log-probability is a function of its id, so
a slice that slipped by one shows."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import test_backend_cpu as tb
from open_speech_amd import _lib
from open_speech_amd.engine import DecodeConfig, WindowOutput, split_cumulative
from open_speech_amd.segments import (ClipResult, Segment, TranscribeOptions, session_supported, shape_response,
                                      split_segments_by_timestamps)
from open_speech_amd.tokenizer import WhisperTokenizer, _byte_decoder

ST, TB, MID = tb.ST, tb.TB, tb.MID
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lp_of(t):
    return -((int(t) % 977) + 1) / 1000.0


def probs_for(lang):
    p = np.full(ST.n_langs, 0.2 / (ST.n_langs - 1), np.float32)
    p[lang - ST.first_lang] = 0.8
    return p


def out_of(tokens, sum_lp=-0.5, nsp=0.01, lang=ST.first_lang + 2, conf=True):
    if not conf:
        return WindowOutput(list(tokens), sum_lp, nsp, lang)
    return WindowOutput(list(tokens), sum_lp, nsp, lang, token_logprobs=[lp_of(t) for t in tokens],
                        eot_logprob=-0.25, language_probs=probs_for(lang))


class ConfEngine(tb.FakeEngine):
    """The scripted engine plus what this feature adds: outputs carry confidences only when the
    decode configuration asks for them, and ``detect_language``."""

    def decode(self, n, cfg, prefix=None, dump_steps=0, languages=None):
        self.confs = getattr(self, "confs", []) + [cfg.confidences]
        outs = super().decode(n, cfg, prefix, dump_steps, languages)
        return outs if cfg.confidences else [WindowOutput(o.tokens, o.sum_logprob, o.no_speech_prob, o.language)
                                             for o in outs]

    def session_begin(self, cfg):
        self.confs = getattr(self, "confs", []) + [cfg.confidences]
        super().session_begin(cfg)

    def session_step(self, max_chunks=1, refill_min=1):
        done, a, q = super().session_step(max_chunks, refill_min)
        if not self._sess["cfg"].confidences:
            done = [(t, WindowOutput(o.tokens, o.sum_logprob, o.no_speech_prob, o.language)) for t, o in done]
        return done, a, q

    def detect_language(self, n):
        assert n == len(self._wins)
        self.detects = getattr(self, "detects", 0) + 1
        return np.stack([probs_for(ST.first_lang + 7)] * n)


def backend(script, holder=None):
    from open_speech_amd.backend import HipWhisperBackend

    def factory(dims, gpu, mb):
        e = ConfEngine(dims, gpu, mb, script)
        if holder is not None:
            holder.append(e)
        return e
    return HipWhisperBackend(engine_factory=factory)


# --------------------------------------------------------------------------- the split
def _check_aligned(segs):
    for sg in segs:
        assert sg["token_logprobs"] == [lp_of(t) for t in sg["tokens"]]


def test_split_consecutive_timestamps_slices_logprobs_like_tokens():
    toks = [TB, 10, TB + 40, TB + 40, 11, 12]
    segs, seek, single = split_segments_by_timestamps(toks, TB, 5.0, 3000, 30.0, 500, [lp_of(t) for t in toks])
    assert not single and seek == 500 + 80 and len(segs) == 1
    assert segs[0]["tokens"] == [TB, 10, TB + 40]
    _check_aligned(segs)


def test_split_single_timestamp_ending_slices_logprobs_like_tokens():
    toks = [TB, 10, 11, TB + 50, TB + 50, 12, TB + 120]
    segs, seek, single = split_segments_by_timestamps(toks, TB, 0.0, 3000, 30.0, 0, [lp_of(t) for t in toks])
    assert single and seek == 3000
    assert [len(s["tokens"]) for s in segs] == [4, 3]
    assert sum(len(s["token_logprobs"]) for s in segs) == len(toks)
    _check_aligned(segs)


def test_split_without_pairs_keeps_the_whole_list_and_off_adds_no_key():
    toks = [TB, 10, 11, 12]
    segs, _, _ = split_segments_by_timestamps(toks, TB, 0.0, 3000, 30.0, 0, [lp_of(t) for t in toks])
    assert len(segs) == 1
    _check_aligned(segs)
    segs, _, _ = split_segments_by_timestamps(toks, TB, 0.0, 3000, 30.0, 0)
    assert "token_logprobs" not in segs[0]
    with pytest.raises(ValueError):
        split_segments_by_timestamps(toks, TB, 0.0, 3000, 30.0, 0, [0.0])


# --------------------------------------------------------------------------- through the backend
def _script(w, i, p, l):
    """60 s: window 0 is silence (skipped), window 1 has two blank segments between two kept ones."""
    if w[1] == 0:
        return out_of([TB, 5, TB + 10], sum_lp=-9.0, nsp=0.95)
    return out_of([TB, 500, 501, TB + 50, TB + 50, TB + 50, TB + 50, 502, TB + 100])


@pytest.mark.parametrize("continuous", ["1", "0"])
def test_segments_keep_logprobs_through_skip_and_blank_drop(monkeypatch, continuous):
    monkeypatch.setenv("STT_HIP_CONTINUOUS", continuous)
    monkeypatch.delenv("STT_HIP_LOGPROBS", raising=False)
    holder = []
    b = backend(_script, holder)
    try:
        r = b.transcribe(tb.wav(60.0), MID, response_format="verbose_json", include=["logprobs"])
    finally:
        b.unload_model(MID)
    assert [s["tokens"] for s in r["segments"]] == [[TB, 500, 501, TB + 50], [TB + 50, 502, TB + 100]]
    assert all(s["seek"] == 3000 for s in r["segments"])
    for s in r["segments"]:
        assert s["token_logprobs"] == [lp_of(t) for t in s["tokens"]]
    # OpenAI's shape over the text tokens in order (no tokenizer.json here: "<|id|>" stand-ins)
    assert [e["logprob"] for e in r["logprobs"]] == [lp_of(t) for t in (500, 501, 502)]
    assert [e["token"] for e in r["logprobs"]] == ["<|500|>", "<|501|>", "<|502|>"]
    assert all(bytes(e["bytes"]).decode() == e["token"] for e in r["logprobs"])
    # detected language: from the window that set it (the skipped first one)
    assert r["language_probability"] == pytest.approx(0.8)
    assert all(holder[0].confs) and holder[0].confs
    json.dumps(r)


def test_include_off_is_the_current_shape(monkeypatch):
    monkeypatch.delenv("STT_HIP_LOGPROBS", raising=False)
    b = backend(_script)
    try:
        audio = tb.wav(60.0)
        got = {}
        for fmt in ("json", "verbose_json", "text", "srt", "vtt"):
            got[fmt] = [b.transcribe(audio, MID, response_format=fmt, **kw)
                        for kw in (dict(), dict(include=[]), dict(include=["logprobs"]))]
    finally:
        b.unload_model(MID)
    for fmt, (plain, empty, on) in got.items():
        assert json.dumps(plain) == json.dumps(empty)
        if fmt in ("text", "srt", "vtt"):
            assert json.dumps(on) == json.dumps(plain)        # never touched
    assert set(got["json"][0]) == {"text"}
    assert set(got["json"][2]) == {"text", "logprobs", "language_probability"}
    v_off, v_on = got["verbose_json"][0], got["verbose_json"][2]
    assert set(v_off) == {"task", "language", "duration", "text", "segments"}
    seg_keys = {"id", "seek", "start", "end", "text", "tokens", "temperature", "avg_logprob", "compression_ratio",
                "no_speech_prob"}
    assert all(set(s) == seg_keys for s in v_off["segments"])
    assert set(v_on) == set(v_off) | {"logprobs", "language_probability"}
    assert all(set(s) == seg_keys | {"token_logprobs"} for s in v_on["segments"])
    for k in v_off:       # everything that was there is unchanged
        if k != "segments":
            assert v_on[k] == v_off[k]
    assert [{k: s[k] for k in seg_keys} for s in v_on["segments"]] == v_off["segments"]


def test_env_default_and_translate(monkeypatch):
    monkeypatch.setenv("STT_HIP_LOGPROBS", "1")
    b = backend(_script)
    try:
        assert "logprobs" in b.transcribe(tb.wav(60.0), MID)
        assert "logprobs" not in b.transcribe(tb.wav(60.0), MID, include=[])
        assert "logprobs" in b.translate(tb.wav(60.0), MID, include=["logprobs"])
    finally:
        b.unload_model(MID)


def test_language_given_is_probability_one_and_no_list(monkeypatch):
    monkeypatch.delenv("STT_HIP_LOGPROBS", raising=False)
    from open_speech_amd.runner import BatchRunner
    tok = WhisperTokenizer(51866)
    for continuous in (False, True):
        r = BatchRunner([ConfEngine(None, 0, 4, _script)], tok, continuous=continuous)
        try:
            pcm = tb.synth.chirp_clip(0, 60.0)
            given = r.transcribe(pcm, TranscribeOptions(language="de", token_logprobs=True))
            found = r.transcribe(pcm, TranscribeOptions(token_logprobs=True))
            off = r.transcribe(pcm, TranscribeOptions())
        finally:
            r.close()
        assert given.language == "de" and given.language_probability == 1.0 and given.all_language_probs is None
        assert found.language_probability == pytest.approx(0.8)
        codes = [c for c, _ in found.all_language_probs]
        assert codes[0] == found.language and len(codes) == ST.n_langs
        ps = [p for _, p in found.all_language_probs]
        assert ps == sorted(ps, reverse=True)
        assert off.language_probability is None and off.all_language_probs is None
        assert all(s.token_logprobs is None for s in off.segments)
        assert all(len(s.token_logprobs) == len(s.tokens) for s in found.segments) and found.segments


def test_backend_detect_language(monkeypatch):
    holder = []
    b = backend(_script, holder)
    try:
        r = b.detect_language(tb.wav(45.0), MID)
    finally:
        b.unload_model(MID)
    tok = WhisperTokenizer(51866)
    assert r["language"] == tok.language_code(ST.first_lang + 7)
    assert r["language_probability"] == pytest.approx(0.8)
    assert r["all_language_probs"][0] == (r["language"], r["language_probability"])
    assert r["language_probability"] == max(p for _, p in r["all_language_probs"])
    e = [x for x in holder if getattr(x, "detects", 0)]
    assert len(e) == 1 and e[0]._wins == [(0, 0, 3000)] and not e[0].calls     # one window, no decode


# --------------------------------------------------------------------------- options and helpers
def test_key_separates_the_settings_and_sessions_stay_supported():
    a, b = TranscribeOptions(), TranscribeOptions(token_logprobs=True)
    assert a.key() != b.key() and a.key() == TranscribeOptions(token_logprobs=False).key()
    assert TranscribeOptions(detect_only=True).key() != a.key()
    assert session_supported(a) and session_supported(b)
    assert not session_supported(TranscribeOptions(detect_only=True))
    assert DecodeConfig().confidences is False
    o = WindowOutput([1], -1.0, 0.0, 0)
    assert o.token_logprobs is None and o.eot_logprob is None and o.language_probs is None


def test_split_cumulative_counts():
    cum = np.array([-0.5, -0.75, -3.0], np.float32)
    lps, eot = split_cumulative(cum, 2)           # two tokens and the closing <|endoftext|> step
    assert lps == [-0.5, -0.25] and eot == -2.25
    lps, eot = split_cumulative(cum, 3)           # cut at max_length: no closing entry
    assert lps == [-0.5, -0.25, -2.25] and eot is None
    # a zero-token window: one entry when its row ended with <|endoftext|>, none otherwise
    assert split_cumulative(np.array([-7.0], np.float32), 0) == ([], -7.0)
    assert split_cumulative(np.zeros(0, np.float32), 0) == ([], None)
    # float64 differences of the fp32 values, not fp32 differences
    c = np.array([-100.0, -100.00001], np.float32)
    assert split_cumulative(c, 2)[0][1] == float(c[1]) - float(c[0])


def test_shape_response_takes_logprobs_from_segments():
    sg = Segment(id=0, seek=0, start=0.0, end=1.0, text="x", tokens=[TB, 7, ST.eot + 3, 9], temperature=0.0,
                 avg_logprob=-0.1, compression_ratio=1.0, no_speech_prob=0.0, token_logprobs=[-0.1, -0.2, -0.3, -0.4])
    res = ClipResult(segments=[sg], language="en", language_probability=0.5)
    out = shape_response("transcribe", res, "json", WhisperTokenizer(51866), True)
    assert [(e["token"], e["logprob"]) for e in out["logprobs"]] == [("<|7|>", -0.2), ("<|9|>", -0.4)]
    assert out["language_probability"] == 0.5
    assert shape_response("transcribe", res, "json") == {"text": "x"}


def test_token_bytes():
    tok = WhisperTokenizer(51866)
    assert tok.token_bytes(123) == b"<|123|>"
    table = _byte_decoder()
    assert len(table) == 256 and sorted(table.values()) == list(range(256))
    assert table["A"] == 65 and table["Ġ"] == 32 and table["Ċ"] == 10     # 'Ġ' is space, 'Ċ' newline


# --------------------------------------------------------------------------- the C ABI
NEW = ("osw_set_confidences", "osw_get_token_logprobs", "osw_get_language_probs", "osw_detect_language")


def test_new_prototypes_and_pinned_struct_sizes():
    for name in NEW:
        assert name in _lib._SIGS and _lib._SIGS[name][0] is C.c_int
    assert _lib._SIGS["osw_get_token_logprobs"][1] == [C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.c_int32,
                                                      C.POINTER(C.c_int32)]
    assert C.sizeof(_lib.osw_window_result) == 64
    assert C.sizeof(_lib.osw_decode_opts) == 144
    header = open(os.path.join(ROOT, "include", "osw.h")).read()
    for name in NEW:
        assert f"int {name}(osw_ctx* ctx" in header
    assert "chunks of 8 decoder steps" not in header
    lib = _lib.load()
    for name in NEW:
        assert getattr(lib, name).argtypes == _lib._SIGS[name][1]
    assert b"0.2" in lib.osw_version()
    # no context: an error code, not a crash (the getters are OSW_ESTATE only on a live context)
    n = C.c_int32()
    assert lib.osw_get_token_logprobs(None, 0, None, 0, C.byref(n)) == -22
    assert lib.osw_set_confidences(None, 1) == -22
