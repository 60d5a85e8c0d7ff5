"""Word timestamps, host side: the test helper's numpy DTW / median filter against
transformers' own, the word splitter, ``add_word_timestamps`` and the seek rule against
hand-derived expectations (tests/tokfix.py tokenizer, a stub engine that returns scripted
``token_frame`` / ``token_prob``), the response shapes, and option routing."""
import json

import numpy as np
import pytest

from open_speech_amd import model_store
from open_speech_amd import segments as S
from open_speech_amd.dims import MICRO_TEST, SpecialTokens
from open_speech_amd.engine import Alignment, WindowOutput
from open_speech_amd.tokenizer import WhisperTokenizer

import align_ref
import tokfix

N_VOCAB = 51866
ST = SpecialTokens.for_vocab(N_VOCAB)
TB = ST.timestamp_begin


@pytest.fixture(scope="module")
def tok(tmp_path_factory):
    return WhisperTokenizer(N_VOCAB, tokfix.build_tokenizer_json(str(tmp_path_factory.mktemp("tok") / "tokenizer.json")))


# ------------------------------------------------------------ the helper itself
def test_numpy_dtw_equals_transformers():
    from transformers.models.whisper.generation_whisper import _dynamic_time_warping
    rng = np.random.default_rng(7)
    for k in range(100):
        T, F = int(rng.integers(1, 13)), int(rng.integers(1, 41))
        x = rng.standard_normal((T, F)).astype(np.float32) if k < 50 else align_ref.tie_matrix(rng, T, F)
        ti, fi = align_ref.dtw(x)
        rt, rf = _dynamic_time_warping(x)
        np.testing.assert_array_equal(ti, rt)
        np.testing.assert_array_equal(fi, rf)
        assert len(align_ref.token_frames(ti, fi)) == T


def test_numpy_median_filter_equals_transformers():
    import torch
    from transformers.models.whisper.generation_whisper import _median_filter
    rng = np.random.default_rng(8)
    for F in (1, 2, 3, 4, 7, 8, 33):
        a = rng.standard_normal((1, 3, 5, F)).astype(np.float32)
        np.testing.assert_array_equal(align_ref.median_filter(a, 7), _median_filter(torch.from_numpy(a), 7).numpy())


# ------------------------------------------------------------ word splitting
def test_split_to_word_tokens(tok):
    ids = tok.encode(" Hello world. This is a test")
    assert [tok.decode([i]) for i in ids] == [" ", "Hello", " world", ".", " This", " is", " a", " test"]
    words, toks = tok.split_to_word_tokens(ids + [ST.eot], "en")
    assert words == [" Hello", " world", ".", " This", " is", " a", " test", "<|endoftext|>"]
    assert toks == [ids[0:2], [ids[2]], [ids[3]], [ids[4]], [ids[5]], [ids[6]], [ids[7]], [ST.eot]]
    # languages written without spaces: every complete UTF-8 piece is a word
    words, toks = tok.split_to_word_tokens(ids + [ST.eot], "ja")
    assert words == [" ", "Hello", " world", ".", " This", " is", " a", " test", "<|endoftext|>"]
    assert toks == [[i] for i in ids] + [[ST.eot]]
    # sub-words without a leading space join the word before them
    ids = tok.encode(" Don't stop: it's only")
    assert tok.split_to_word_tokens(ids + [ST.eot], "en")[0] == [" Don't", " stop", ":", " it's", " only",
                                                                 "<|endoftext|>"]


def test_split_keeps_incomplete_utf8_together(tok):
    ids = tok.encode(" 日本")
    assert len(ids) == 7         # a space and two characters of three byte-level tokens each
    words, toks = tok.split_to_word_tokens(ids + [ST.eot], "ja")
    assert words == [" ", "日", "本", "<|endoftext|>"]
    assert toks == [ids[0:1], ids[1:4], ids[4:7], [ST.eot]]
    assert tok.split_to_word_tokens(ids + [ST.eot], "en")[0] == [" 日本", "<|endoftext|>"]


# ------------------------------------------------------------ add_word_timestamps
HELLO = " Hello world."     # tokens [" ", "Hello", " world", "."]


def seg_dict(tokens, start, end, seek=0):
    return dict(seek=seek, start=start, end=end, tokens=list(tokens))


def test_add_word_timestamps_merges_punctuation(tok):
    ids = tok.encode(HELLO)
    assert len(ids) == 4
    # frames of " ", "Hello", " world", ".", <|endoftext|>
    al = Alignment(np.array([0, 5, 25, 40, 50]), np.array([0.5, 0.7, 0.9, 0.3]))
    segs = [seg_dict([TB] + ids + [TB + 100], 0.0, 2.0)]
    o = S.TranscribeOptions()
    last = S.add_word_timestamps(segs, tok, al, "en", o.prepend_punctuations, o.append_punctuations, 0.0)
    # " Hello" = frames 0 .. 25, " world" 25 .. 40, "." 40 .. 50; "." joins " world" and keeps
    # the times of " world" (upstream merges text and tokens only)
    assert segs[0]["words"] == [
        dict(word=" Hello", start=0.0, end=0.5, probability=pytest.approx(0.6)),
        dict(word=" world.", start=0.5, end=0.8, probability=pytest.approx(0.9))]
    # no word is too long: the segment takes its words' start and end
    assert segs[0]["start"] == 0.0 and segs[0]["end"] == 0.8 and last == 0.8


def test_add_word_timestamps_prepended_punctuation_and_two_segments(tok):
    a, b = tok.encode(" said"), tok.encode(" ( second")
    assert len(a) == 1 and len(b) == 2
    al = Alignment(np.array([10, 20, 30, 45]), np.array([0.2, 0.4, 0.8]))
    segs = [seg_dict([TB] + a + [TB + 10], 5.0, 5.2, seek=500), seg_dict([TB + 10] + b + [TB + 50], 5.2, 6.0, seek=500)]
    o = S.TranscribeOptions()
    S.add_word_timestamps(segs, tok, al, "en", o.prepend_punctuations, o.append_punctuations, 5.0)
    # times are offset by the window's seek (5.00 s); " (" is prepended to " second", which keeps its times
    assert segs[0]["words"] == [dict(word=" said", start=5.2, end=5.4, probability=pytest.approx(0.2))]
    assert segs[1]["words"] == [dict(word=" ( second", start=5.6, end=5.9, probability=pytest.approx(0.8))]
    assert (segs[0]["start"], segs[0]["end"], segs[1]["start"], segs[1]["end"]) == (5.2, 5.4, 5.6, 5.9)


def test_add_word_timestamps_clamps_long_first_word(tok):
    ids = tok.encode(HELLO)
    al = Alignment(np.array([0, 0, 100, 110, 120]), np.ones(4) * 0.5)
    segs = [seg_dict([TB] + ids + [TB + 150], 0.0, 3.0)]
    o = S.TranscribeOptions()
    last = S.add_word_timestamps(segs, tok, al, "en", o.prepend_punctuations, o.append_punctuations, 0.0)
    # durations 2.0, 0.2, 0.2: median 0.2, max 0.4.  " Hello" ends 2.0 s after the last speech
    # (> 4 x median) and lasts 2.0 > 0.4, so it starts at 2.0 - 0.4; the segment follows its words
    w = segs[0]["words"]
    assert [x["word"] for x in w] == [" Hello", " world."]
    assert w[0]["start"] == pytest.approx(1.6) and w[0]["end"] == 2.0
    assert w[1]["start"] == 2.0 and w[1]["end"] == 2.2
    assert segs[0]["start"] == pytest.approx(1.6) and segs[0]["end"] == 2.2 and last == 2.2


def test_add_word_timestamps_without_alignment(tok):
    segs = [seg_dict([TB, TB + 50], 0.0, 1.0)]
    assert S.add_word_timestamps(segs, tok, None, "en", "", "", 3.0) == 3.0
    assert segs[0]["words"] == [] and (segs[0]["start"], segs[0]["end"]) == (0.0, 1.0)


# ------------------------------------------------------------ the seek loop with a stub engine
class StubEngine:
    """Scripted decode outputs per call; ``align`` returns the scripted alignment of each
    requested window and records what it was asked."""
    max_batch = 4
    max_rows = 20

    def __init__(self, outputs, alignments):
        self.outputs, self.alignments = list(outputs), alignments
        self.encoded, self.align_calls = [], []

    def log_mel(self, clips):
        return [len(c) // 160 + 1 for c in clips]

    def encode(self, wins):
        self.encoded.append(list(wins))

    def decode(self, n, cfg, prefix=None, languages=None):
        return [self.outputs.pop(0) for _ in range(n)]

    def align(self, windows):
        self.align_calls.append(windows)
        return [self.alignments[tuple(w.tokens)] for w in windows]


SILENCE = WindowOutput(tokens=[], sum_logprob=-50.0, no_speech_prob=0.95, language=ST.first_lang)
PCM10 = np.zeros(160000, np.int16)      # 10 s: 1000 content frames


def run_stub(tok, tokens, word_timestamps=True, n_windows=2):
    ids = tok.encode(HELLO)
    al = {tuple(ids): Alignment(np.array([0, 5, 25, 40, 50]), np.array([0.5, 0.7, 0.9, 0.3]))}
    out = WindowOutput(tokens=[t if t >= 0 else ids[-t - 1] for t in tokens], sum_logprob=-1.0, no_speech_prob=0.1,
                       language=ST.first_lang)
    eng = StubEngine([out] + [SILENCE] * n_windows, al)
    opts = S.TranscribeOptions(language="en", word_timestamps=word_timestamps, beam_size=1)
    res = S.transcribe_clips(eng, [PCM10], opts, tok, ())[0]
    return eng, res


T_SINGLE = [TB, -1, -2, -3, -4, TB + 100]               # ends in a single timestamp
T_PAIR = [TB, -1, -2, -3, -4, TB + 100, TB + 100]       # ends in a timestamp pair


def test_seek_rule_single_timestamp_ending(tok):
    eng, res = run_stub(tok, T_SINGLE)
    # a single timestamp at the end: the window is consumed whole, with or without words
    assert eng.encoded == [[(0, 0, 1000)]]
    assert len(eng.align_calls) == 1 and eng.align_calls[0][0].num_frames == 1000
    assert eng.align_calls[0][0].tokens == tok.encode(HELLO) and eng.align_calls[0][0].window == 0
    assert [w.word for w in res.segments[0].words] == [" Hello", " world."]
    assert (res.segments[0].start, res.segments[0].end) == (0.0, 0.8)


def test_seek_rule_moves_to_last_word_end(tok):
    eng, res = run_stub(tok, T_PAIR)
    # without words the pair at 2.00 s would move the seek to frame 200; the last word ends at
    # 0.80 s > time_offset, so the next window starts at round(0.80 * 100) = 80
    assert eng.encoded == [[(0, 0, 1000)], [(0, 80, 920)]]
    eng, res = run_stub(tok, T_PAIR, word_timestamps=False)
    assert eng.encoded == [[(0, 0, 1000)], [(0, 200, 800)]] and eng.align_calls == []
    assert res.segments[0].words is None


def test_window_without_text_tokens(tok):
    # a lone timestamp: one segment 0 .. 2.00 s of blank text, dropped.  No words, so the last
    # "word end" is the segment's end (upstream get_end) and the seek moves there
    out = WindowOutput(tokens=[TB + 100], sum_logprob=-1.0, no_speech_prob=0.1, language=ST.first_lang)
    eng = StubEngine([out, SILENCE], {})
    res = S.transcribe_clips(eng, [PCM10], S.TranscribeOptions(language="en", word_timestamps=True, beam_size=1), tok,
                             ())[0]
    assert eng.align_calls == [] and res.segments == [] and eng.encoded == [[(0, 0, 1000)], [(0, 200, 800)]]


# ------------------------------------------------------------ response shapes
def test_verbose_json_unchanged_without_words(tok):
    _, res = run_stub(tok, T_SINGLE, word_timestamps=False)
    ids = tok.encode(HELLO)
    want = {"task": "transcribe", "language": "en", "duration": 10.0, "text": "Hello world.",
            "segments": [{"id": 0, "seek": 0, "start": 0.0, "end": 2.0, "text": " Hello world.",
                          "tokens": [TB] + ids + [TB + 100], "temperature": 0.0, "avg_logprob": -1.0 / 7,
                          "compression_ratio": S.compression_ratio("Hello world."), "no_speech_prob": 0.1}]}
    assert json.dumps(S.verbose_dict("transcribe", res)) == json.dumps(want)


def test_verbose_json_words_shape(tok):
    _, res = run_stub(tok, T_SINGLE)
    d = S.verbose_dict("transcribe", res)
    assert list(d) == ["task", "language", "duration", "text", "segments", "words"]
    assert d["segments"][0]["words"] == [
        {"start": 0.0, "end": 0.5, "word": " Hello", "probability": pytest.approx(0.6)},
        {"start": 0.5, "end": 0.8, "word": " world.", "probability": pytest.approx(0.9)}]
    assert d["words"] == [{"word": " Hello", "start": 0.0, "end": 0.5}, {"word": " world.", "start": 0.5, "end": 0.8}]
    assert "".join(w["word"] for w in d["segments"][0]["words"]) == d["segments"][0]["text"]
    assert S.shape_response("transcribe", res, "json") == {"text": "Hello world."}


# ------------------------------------------------------------ options and model files
def test_word_timestamps_take_the_batched_loop():
    on, off = S.TranscribeOptions(word_timestamps=True), S.TranscribeOptions()
    assert S.session_supported(off) and not S.session_supported(on)
    assert on.key() != off.key()
    assert S.Segment(0, 0, 0.0, 1.0, "x", [], 0.0, 0.0, 0.0, 0.0).words is None


def test_alignment_heads_from_model_files(tmp_path):
    src = model_store.ModelSource("m", MICRO_TEST, "hf", path=str(tmp_path))
    assert model_store.alignment_heads(src) is None
    assert model_store.alignment_heads(model_store.ModelSource("random:micro-test", MICRO_TEST, "random")) is None
    L, H = MICRO_TEST.n_text_layer, MICRO_TEST.n_text_head
    (tmp_path / "generation_config.json").write_text(json.dumps({"alignment_heads": [[L - 1, 0], [0, H - 1]]}))
    assert model_store.alignment_heads(src) == [(L - 1, 0), (0, H - 1)]
    (tmp_path / "generation_config.json").write_text(json.dumps({"alignment_heads": [[L, 0]]}))   # out of range
    assert model_store.alignment_heads(src) is None
    (tmp_path / "config.json").write_text(json.dumps({"alignment_heads": [[0, 0]]}))               # CTranslate2 layout
    assert model_store.alignment_heads(src) == [(0, 0)]
