"""Host side of the shorter encoder windows (faster-whisper's ``chunk_length``, no GPU): the seek
loop against tests/chunk_ref.py's restatement, the options' key and defaults, the loaders'
cropping of the positional table, the refused values, the serving knob STT_HIP_CHUNK_LENGTH, and
the inequality that keeps every cross-attention key chunk non-empty."""
import json

import numpy as np
import pytest

import chunk_ref as CR
from open_speech_amd import ct2, model_store, synth, weights
from open_speech_amd import dims as D
from open_speech_amd.backend import HipWhisperBackend
from open_speech_amd.engine import WindowOutput
from open_speech_amd.runner import BatchRunner
from open_speech_amd.segments import (TranscribeOptions, clip_state, consume_window, finish_clip, next_window,
                                      transcribe_clips)
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens

ST = D.SpecialTokens.for_vocab(51866)
TB = ST.timestamp_begin


def script(seek, size):
    """A window's tokens from its position alone: pairs of timestamps inside the window (so the seek
    moves by the last timestamp), a single timestamp ending on every third window (the seek moves by
    the whole window), text ids that name the window."""
    k = seek // 37
    last = max(2, min(size // 2, 40 + 13 * (k % 5)))      # timestamp positions are 2 frames each
    mid = last // 2
    a, b = 1000 + k % 700, 2000 + (3 * k) % 700
    if k % 3 == 2:
        return [TB, a, TB + mid, TB + mid, b, TB + last]
    return [TB, a, TB + mid, TB + mid, b, TB + last, TB + last]


class ScriptEngine:
    max_batch = 2
    max_rows = 10

    def __init__(self):
        self.wins, self.calls = [], []

    def log_mel(self, clips):
        return [(len(c) + 160) // 160 for c in clips]

    def encode(self, wins):
        self.wins = list(wins)

    def decode(self, n, cfg, prefix=None, dump_steps=0, languages=None):
        outs = []
        for k, (_, seek, size) in enumerate(self.wins):
            self.calls.append((seek, size, list(prefix[k]) if prefix else []))
            outs.append(WindowOutput(script(seek, size), -1.0, 0.01, ST.first_lang))
        return outs


@pytest.mark.parametrize("s", [5, 10])
def test_seek_loop_with_short_windows(s):
    """A 23 s clip in 5 s and 10 s windows: seeks, sizes, prompts and segments are the restatement's;
    no window is longer than nb_max_frames = 100 s, and the one-clip-at-a-time path (the session
    lanes') walks the same windows."""
    tok = WhisperTokenizer(51866)
    sup = get_suppressed_tokens(tok, [-1])
    pcm = synth.chirp_clip(1, 23.0)
    opts = TranscribeOptions(beam_size=1, chunk_length=s)
    assert opts.nb_max_frames == 100 * s
    eng = ScriptEngine()
    res = transcribe_clips(eng, [pcm], opts, tok, sup)[0]
    seen = []

    def decode_window(seek, size, prompt):
        seen.append((seek, size, list(prompt)))
        return script(seek, size), -1.0, 0.01

    nf = (len(pcm) + 160) // 160
    wins = CR.seek_loop(decode_window, nf, ST, tok.decode, 100 * s)
    assert eng.calls == seen
    assert len(wins) > 23 // s and all(1 <= w.size <= 100 * s for w in wins)
    assert wins[0].size == 100 * s and wins[-1].seek + wins[-1].size == nf - 1
    assert any(w.seek % (100 * s) for w in wins), "no window started at a timestamp"
    assert [(g.start, g.end, g.tokens) for g in res.segments] == [(a, b, t) for w in wins for a, b, t in w.segments]
    assert [g.seek for g in res.segments] == [w.seek for w in wins for _ in w.segments]
    # the 30 s loop takes the whole clip as its first window: the option changes the schedule
    eng30 = ScriptEngine()
    transcribe_clips(eng30, [pcm], TranscribeOptions(beam_size=1), tok, sup)
    assert eng30.calls[0][:2] == (0, 2300)
    # one clip at a time
    st = clip_state(0, pcm, opts, tok)
    walked = []
    while not st.done:
        w = next_window(st, opts, tok)
        walked.append((w["seek"], w["segment_size"], w["prefix"]))
        consume_window(st, w, WindowOutput(script(w["seek"], w["segment_size"]), -1.0, 0.01, ST.first_lang), opts, tok)
    assert walked == seen
    got = finish_clip(st, opts, tok)
    assert [(g.start, g.end, g.tokens) for g in got.segments] == [(g.start, g.end, g.tokens) for g in res.segments]


def test_detect_only_uses_the_first_window():
    tok = WhisperTokenizer(51866)

    class Eng(ScriptEngine):
        def detect_language(self, n):
            p = np.zeros((n, ST.n_langs), np.float32)
            p[:, 3] = 1.0
            return p

    for s, want in ((30, 2300), (5, 500)):
        eng = Eng()
        transcribe_clips(eng, [synth.chirp_clip(1, 23.0)], TranscribeOptions(detect_only=True, chunk_length=s), tok, ())
        assert eng.wins == [(0, 0, want)]


def test_key_and_defaults():
    d = TranscribeOptions()
    assert d.chunk_length == 30 and d.nb_max_frames == 3000
    today = (d.task, d.language, d.initial_prompt, d.condition_on_previous_text, d.without_timestamps,
             tuple(d.suppress_tokens), d.suppress_blank, d.beam_size, d.patience, d.length_penalty, 0.0,
             d.best_of, d.tokens_per_second, d.max_new_tokens, d.word_timestamps, d.prepend_punctuations,
             d.append_punctuations, 1.0, 0, False, False)
    # chunk_length = 30 is no option at all: today's key; any other value adds its field
    assert d.key() == today and TranscribeOptions(chunk_length=30).key() == today
    assert TranscribeOptions(chunk_length=30.0).chunk_length == 30
    assert TranscribeOptions(chunk_length=10).key() == today + (("chunk_length", 10),)
    assert TranscribeOptions(chunk_length=10).key() != TranscribeOptions(chunk_length=5).key()
    hash(TranscribeOptions(chunk_length=10, log_prob_threshold=-0.5).key())


@pytest.mark.parametrize("bad", [0, 31, 7.5, -5, "x", None, True, float("nan")])
def test_refused_values(bad):
    with pytest.raises(ValueError, match="chunk_length"):
        TranscribeOptions(chunk_length=bad)
    with pytest.raises(ValueError, match="chunk_length"):
        D.TINY_TEST.with_chunk_length(bad)
    with pytest.raises(ValueError, match="chunk_length"):
        BatchRunner([], WhisperTokenizer(51866), chunk_length=bad)


def test_with_chunk_length():
    for s in range(1, 31):
        d = D.LARGE_V3_TURBO.with_chunk_length(s)
        assert d.n_audio_ctx == 50 * s and d.n_frames == 100 * s and d.chunk_length == s
        assert d == D.WhisperDims(n_audio_ctx=50 * s)
    assert D.TINY_TEST.with_chunk_length(30) == D.TINY_TEST
    assert D.TINY_TEST.with_chunk_length("5").n_audio_ctx == 250


def test_no_cross_attention_chunk_is_empty():
    """(8 - 1) ceil(T / 8) < T for every T = 50 s: the last of the 8 key chunks holds a key.  (It
    fails for some T the library refuses, e.g. 49.)"""
    for s in range(1, 31):
        assert CR.no_chunk_empty(50 * s), s
        xu, nt = CR.chunk_forms(50 * s)
        assert 1 <= xu <= 6 and 1 <= nt <= 3 and CR.xper(50 * s) <= min(32 * xu, 64 * nt)
    assert CR.chunk_forms(1500) == (6, 3) and CR.chunk_forms(1300) == (6, 3) and CR.chunk_forms(250) == (1, 1)
    assert not CR.no_chunk_empty(49) and not CR.no_chunk_empty(9)


# --------------------------------------------------------------------------- loaders
def test_random_weights_crop_the_table():
    d = D.MICRO_TEST
    full = weights.random_weights(d, seed=3)
    short = weights.random_weights(d.with_chunk_length(5), seed=3)
    assert short["enc.pos"].shape == (250, d.n_audio_state)
    np.testing.assert_array_equal(short["enc.pos"], full["enc.pos"][:250])
    for k in full:
        if k != "enc.pos":
            np.testing.assert_array_equal(short[k], full[k], err_msg=k)


def test_hf_directory_is_cropped(tmp_path):
    from safetensors.numpy import save_file
    d = D.MICRO_TEST
    canon = weights.random_weights(d, seed=3)
    snap = tmp_path / "models--org--micro-whisper" / "snapshots" / "abc"
    snap.mkdir(parents=True)
    sd = {k: v for k, v in weights.to_hf_state_dict(canon, d).items() if k != "proj_out.weight"}
    save_file(sd, str(snap / "model.safetensors"))
    cfg = {"num_mel_bins": d.n_mels, "d_model": d.n_audio_state, "encoder_attention_heads": d.n_audio_head,
           "encoder_layers": d.n_audio_layer, "decoder_attention_heads": d.n_text_head,
           "decoder_layers": d.n_text_layer, "vocab_size": d.n_vocab, "max_source_positions": 1500}
    (snap / "config.json").write_text(json.dumps(cfg))
    assert model_store.resolve("org/micro-whisper", str(tmp_path)).dims == d
    assert model_store.resolve("org/micro-whisper", str(tmp_path), chunk_length=30).dims == d
    src = model_store.resolve("org/micro-whisper", str(tmp_path), chunk_length=10)
    assert src.dims == d.with_chunk_length(10)
    w = model_store.load_weights(src)
    assert w["enc.pos"].shape == (500, d.n_audio_state) and w["enc.pos"].flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(w["enc.pos"], canon["enc.pos"][:500])
    np.testing.assert_array_equal(w["dec.pos"], canon["dec.pos"])
    with pytest.raises(ValueError, match="chunk_length"):
        model_store.resolve("org/micro-whisper", str(tmp_path), chunk_length=31)
    # a checkpoint with a shorter table than the window asked for
    with pytest.raises(ValueError, match="fewer than"):
        weights.from_hf_state_dict({**weights.to_hf_state_dict(weights.random_weights(d.with_chunk_length(5), seed=3),
                                                               d.with_chunk_length(5))}, d.with_chunk_length(6))


def test_ct2_header_is_cropped(tmp_path):
    d = D.MICRO_TEST
    canon = weights.random_weights(d, seed=3)
    snap = tmp_path / "models--org--micro-ct2" / "snapshots" / "x"
    snap.mkdir(parents=True)
    v, al = ct2.canonical_to_ct2(canon, d)
    ct2.write_model_bin(str(snap / "model.bin"), v, al)
    src = model_store.resolve("org/micro-ct2", str(tmp_path), chunk_length=1)
    assert src.kind == "ct2" and src.dims == d.with_chunk_length(1)
    w = model_store.load_weights(src)
    np.testing.assert_array_equal(w["enc.pos"], canon["enc.pos"][:50])
    assert set(w) == set(canon)


# --------------------------------------------------------------------------- serving knob
class KnobEngine(ScriptEngine):
    def __init__(self, dims, gpu, max_batch):
        super().__init__()
        self.dims, self.device, self.max_batch = dims, gpu, max_batch

    def init_random(self, seed=0):
        pass

    def close(self):
        pass


def test_serving_knob(monkeypatch):
    made = []

    def factory(dims, gpu, mb):
        made.append(KnobEngine(dims, gpu, mb))
        return made[-1]

    monkeypatch.setenv("STT_HIP_LANES", "1")
    monkeypatch.setenv("STT_HIP_CONTINUOUS", "0")
    for bad in ("0", "31", "7.5", "abc"):
        monkeypatch.setenv("STT_HIP_CHUNK_LENGTH", bad)
        with pytest.raises(ValueError, match="chunk_length"):
            HipWhisperBackend(engine_factory=factory).load_model("random:micro-test")
    assert not made
    monkeypatch.setenv("STT_HIP_CHUNK_LENGTH", "5")
    be = HipWhisperBackend(engine_factory=factory)
    try:
        be.load_model("random:micro-test")
        assert made[-1].dims == D.MICRO_TEST.with_chunk_length(5)
        out = be.transcribe(synth.to_wav_bytes(synth.chirp_clip(1, 23.0)), "random:micro-test")
        assert out["text"] is not None
        assert len(made[-1].calls) >= 5 and all(size <= 500 for _, size, _ in made[-1].calls)
    finally:
        be.unload_model("random:micro-test")
    monkeypatch.delenv("STT_HIP_CHUNK_LENGTH")
    be = HipWhisperBackend(engine_factory=factory)
    try:
        be.load_model("random:micro-test")
        assert made[-1].dims == D.MICRO_TEST
        be.transcribe(synth.to_wav_bytes(synth.chirp_clip(1, 23.0)), "random:micro-test")
        assert made[-1].calls[0][:2] == (0, 2300)
    finally:
        be.unload_model("random:micro-test")
