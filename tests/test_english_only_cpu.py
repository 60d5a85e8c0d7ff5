"""English-only Whisper models (n_vocab 51864) without a GPU: the special-token ids, the
restated decoding loops of tests/english_ref.py pinned against transformers' own ``generate``
for a model that is not multilingual, the host logic (prompts without language and task
tokens, the language and task coercions, language detection without the engine, the
suppressed-token expansion) and the unchanged C ABI struct sizes."""
import ctypes
import dataclasses
import json
import logging
import os

import numpy as np
import pytest

import tokfix
from open_speech_amd import _lib
from open_speech_amd import dims as D
from open_speech_amd import synth
from open_speech_amd.engine import DecodeConfig, WindowOutput
from open_speech_amd.segments import TranscribeOptions, session_supported, transcribe_clips
from open_speech_amd.tokenizer import (NON_SPEECH_TOKENS_MULTILINGUAL, WhisperTokenizer, get_suppressed_tokens)
from oracle import decode as odec
from test_backend_cpu import FakeEngine, make_backend

import english_ref as eref

GOLD = os.path.join(os.path.dirname(__file__), "golden")
EN = D.SpecialTokens.for_vocab(51864)
TB = EN.timestamp_begin
MICRO_EN = dataclasses.replace(D.MICRO_TEST, n_vocab=51864)


# --------------------------------------------------------------------------- ids
def test_english_only_ids():
    assert not EN.multilingual
    assert (EN.eot, EN.sot, EN.first_lang, EN.n_langs) == (50256, 50257, 50258, 99)
    assert (EN.translate, EN.transcribe, EN.sot_lm, EN.sot_prev) == (50357, 50358, 50359, 50360)
    assert (EN.no_speech, EN.no_timestamps, EN.timestamp_begin, EN.blank) == (50361, 50362, 50363, 220)
    assert EN.timestamp_begin + 1500 == 51863


def test_multilingual_ids_unchanged():
    a, b = D.SpecialTokens.for_vocab(51865), D.SpecialTokens.for_vocab(51866)
    assert a.multilingual and b.multilingual
    assert (a.eot, a.sot, a.first_lang, a.n_langs, a.translate, a.transcribe, a.sot_lm, a.sot_prev, a.no_speech,
            a.no_timestamps, a.timestamp_begin) == (50257, 50258, 50259, 99, 50358, 50359, 50360, 50361, 50362,
                                                    50363, 50364)
    assert (b.eot, b.sot, b.first_lang, b.n_langs, b.translate, b.transcribe, b.sot_lm, b.sot_prev, b.no_speech,
            b.no_timestamps, b.timestamp_begin) == (50257, 50258, 50259, 100, 50359, 50360, 50361, 50362, 50363,
                                                    50364, 50365)
    # other sizes below 51865 keep the multilingual ids (tests use them)
    c = D.SpecialTokens.for_vocab(51000)
    assert c.multilingual and c.eot == 50257 and c.timestamp_begin == 50364


def test_presets():
    assert D.PRESETS["tiny-en-test"] == D.TINY_EN_TEST
    assert D.TINY_EN_TEST == dataclasses.replace(D.TINY_TEST, n_vocab=51864)
    from open_speech_amd import model_store
    assert model_store.resolve("random:tiny-en-test").dims == D.TINY_EN_TEST


@pytest.fixture(scope="module")
def tok_path(tmp_path_factory):
    return tokfix.build_tokenizer_json(str(tmp_path_factory.mktemp("tok_en") / "tokenizer.json"), 51864)


def test_tokenizer_json_round_trips_the_special_ids(tok_path):
    tk = WhisperTokenizer(51864, tok_path)
    raw = tk._tok
    assert raw.get_vocab_size() == 51864
    for text, tid in (("<|endoftext|>", EN.eot), ("<|startoftranscript|>", EN.sot), ("<|en|>", EN.first_lang),
                      ("<|translate|>", EN.translate), ("<|transcribe|>", EN.transcribe),
                      ("<|startoflm|>", EN.sot_lm), ("<|startofprev|>", EN.sot_prev), ("<|nospeech|>", EN.no_speech),
                      ("<|notimestamps|>", EN.no_timestamps), ("<|0.00|>", TB), ("<|30.00|>", 51863)):
        assert raw.token_to_id(text) == tid, text
        assert raw.id_to_token(tid) == text
    ids = tk.encode(" Hello world.")
    assert ids and all(0 <= t < EN.eot for t in ids) and tk.decode([TB] + ids + [EN.eot]) == " Hello world."


def test_tokenizer_language_and_suppressed_tokens(tok_path, caplog):
    tk = WhisperTokenizer(51864, tok_path)
    assert tk.language_token("en") is None and tk.language_token("fr") is None and tk.language_token("xx") is None
    assert tk.language_code(EN.first_lang + 3) == "en" and tk.language_code(-1) == "en"
    specials = {EN.transcribe, EN.translate, EN.sot, EN.sot_prev, EN.sot_lm}
    sup = get_suppressed_tokens(tk, [-1])     # from tokenizer.json, as for a multilingual model
    assert specials < set(sup) and set(sup) == set(tk.non_speech_tokens()) | specials and len(sup) > 25
    # without a tokenizer.json: the special-token part only, a warning, never the multilingual table
    import open_speech_amd.tokenizer as T
    T._warned_no_table = False
    with caplog.at_level(logging.WARNING):
        bare = get_suppressed_tokens(WhisperTokenizer(51864), [-1])
        again = get_suppressed_tokens(WhisperTokenizer(51864), [-1, 7])
    assert set(bare) == specials and set(again) == specials | {7}
    assert not set(bare) & {t for t in NON_SPEECH_TOKENS_MULTILINGUAL if t < EN.eot}
    assert sum("English-only vocabulary" in r.getMessage() for r in caplog.records) == 1
    # a multilingual vocabulary keeps its table
    assert set(NON_SPEECH_TOKENS_MULTILINGUAL) < set(get_suppressed_tokens(WhisperTokenizer(51865), [-1]))


# --------------------------------------------------------------------------- transformers pin
MAX_NEW = 24


@pytest.fixture(scope="module")
def hf():
    """transformers' model at TINY_EN_TEST dims with the golden's weights, one clip's features
    and encoder output."""
    import torch
    meta = json.load(open(os.path.join(GOLD, "tiny_en_model.json")))
    d = D.TINY_EN_TEST
    w = eref.golden_weights(d, meta["seed"], meta["text_pos"], meta["nospeech_mix"], tuple(meta["sot_positions"]))
    model, sup = eref.hf_english_model(d, w)
    feat, size = eref.hf_window_features(synth.chirp_clip(3, 6.0), d.n_mels)
    with torch.no_grad():
        enc = model.model.encoder(input_features=feat).last_hidden_state
    mask = torch.zeros(1, 3000, dtype=torch.long)
    mask[:, :size] = 1
    return d, model, sup, feat, mask, enc, eref.HFStepper(model, enc)


def _first_window(model, feat, mask, **kw):
    """The first window's generated ids (transformers' ``generate`` walks the whole clip; every
    segment of a window carries that window's full sequence as ``result``)."""
    out = model.generate(input_features=feat, attention_mask=mask, max_new_tokens=MAX_NEW, return_segments=True, **kw)
    return out["segments"][0][0]["result"].tolist()


def _strip(seq, prompt):
    assert seq[:len(prompt)] == prompt, (seq[:len(prompt) + 2], prompt)
    return seq[len(prompt):]


def test_greedy_with_timestamps_equals_generate(hf):
    d, model, sup, feat, mask, enc, stepper = hf
    seq = _first_window(model, feat, mask, return_timestamps=True)
    opts = odec.DecodeOptions(suppress_tokens=sup, max_length=1 + MAX_NEW)
    r = eref.greedy_from_encoder(stepper, None, EN, opts=opts)
    assert r.tokens == _strip(seq, [EN.sot]) and len(r.tokens) == MAX_NEW
    assert r.tokens[0] >= TB and r.language == -1
    # the golden's ids come from the same loop on the same model
    gold = np.load(os.path.join(GOLD, "tiny_en_model.npz"))["chirp/ts/ids"].tolist()
    assert r.tokens == gold[:MAX_NEW]


def test_greedy_without_timestamps_equals_generate(hf):
    d, model, sup, feat, mask, enc, stepper = hf
    seq = model.generate(input_features=feat, return_timestamps=False, max_new_tokens=MAX_NEW)[0].tolist()
    opts = odec.DecodeOptions(suppress_tokens=sup, without_timestamps=True, max_length=2 + MAX_NEW)
    r = eref.greedy_from_encoder(stepper, None, EN, opts=opts)
    assert r.tokens == seq[-MAX_NEW:] and all(t < EN.eot for t in r.tokens)


def test_greedy_with_previous_text_equals_generate(hf):
    import torch
    d, model, sup, feat, mask, enc, stepper = hf
    prev = [int((i * 97 + 13) % 50000) for i in range(4)]
    seq = model.generate(input_features=feat, return_timestamps=False, max_new_tokens=MAX_NEW,
                         prompt_ids=torch.tensor([EN.sot_prev] + prev))[0].tolist()
    prompt = eref.prompt_tokens(EN, prev, True)
    assert prompt == [EN.sot_prev] + prev + [EN.sot, EN.no_timestamps]
    opts = odec.DecodeOptions(suppress_tokens=sup, without_timestamps=True, max_length=len(prompt) + MAX_NEW)
    r = eref.greedy_from_encoder(stepper, None, EN, prev_tokens=prev, opts=opts)
    assert r.tokens == seq[-MAX_NEW:]
    gold = np.load(os.path.join(GOLD, "tiny_en_model.npz"))["chirp/nots4/ids"].tolist()
    assert r.tokens == gold[:MAX_NEW]


def test_beam5_equals_transformers_beam_search(hf):
    """tools/make_hf_pins.py's configuration (transformers' beam search with Whisper's processors
    and CTranslate2's log-softmax renormalisation, length penalty 1 with the generated length
    counting <|endoftext|>) from the prompt [sot]."""
    import torch
    from transformers import GenerationConfig
    from transformers.generation.logits_process import (LogitsProcessor, LogitsProcessorList,
                                                        SuppressTokensAtBeginLogitsProcessor,
                                                        SuppressTokensLogitsProcessor, WhisperTimeStampLogitsProcessor)
    from transformers.generation.utils import GenerationMixin
    from transformers.modeling_outputs import BaseModelOutput

    class Renorm(LogitsProcessor):
        def __call__(self, input_ids, scores):
            return torch.log_softmax(scores, dim=-1)

    d, model, sup, feat, mask, enc, stepper = hf
    K, max_len = 5, 1 + 12
    gts = GenerationConfig(no_timestamps_token_id=EN.no_timestamps, eos_token_id=EN.eot, max_initial_timestamp_index=50)
    procs = LogitsProcessorList([SuppressTokensAtBeginLogitsProcessor([EN.blank, EN.eot], 1),
                                 SuppressTokensLogitsProcessor(list(sup)), WhisperTimeStampLogitsProcessor(gts, 1),
                                 Renorm()])
    gc = GenerationConfig(num_beams=K, early_stopping=True, length_penalty=1.0, max_length=max_len,
                          eos_token_id=EN.eot, pad_token_id=EN.eot, decoder_start_token_id=EN.sot, do_sample=False,
                          num_return_sequences=K, output_scores=True, return_dict_in_generate=True)
    out = GenerationMixin.generate(model, decoder_input_ids=torch.tensor([[EN.sot]]),
                                   encoder_outputs=BaseModelOutput(last_hidden_state=enc), generation_config=gc,
                                   logits_processor=procs)
    best = out.sequences[0].tolist()[1:]
    best = best[:best.index(EN.eot)] if EN.eot in best else best
    opts = odec.DecodeOptions(suppress_tokens=sup, max_length=max_len)
    r = eref.beam_from_encoder(stepper, None, EN, opts=opts,
                               beam=odec.BeamOptions(beam_size=K, num_hypotheses=K, length_penalty=1.0,
                                                     length_counts_eot=True))
    assert r.tokens == best
    assert r.hypotheses and abs(max(h[2] for h in r.hypotheses) - float(out.sequences_scores[0])) < 1e-3


def test_no_speech_prob_is_the_raw_sot_softmax(hf):
    import torch
    d, model, sup, feat, mask, enc, stepper = hf
    with torch.no_grad():
        lg = model(encoder_outputs=(enc,), decoder_input_ids=torch.tensor([[EN.sot]])).logits[0, -1]
    want = float(torch.softmax(lg.double(), -1)[EN.no_speech])
    assert want > 0.1
    for nots in (False, True):
        opts = odec.DecodeOptions(suppress_tokens=sup, without_timestamps=nots, max_length=8)
        assert abs(eref.greedy_from_encoder(stepper, None, EN, opts=opts).no_speech_prob - want) < 1e-6
    assert abs(eref.beam_from_encoder(stepper, None, EN, opts=odec.DecodeOptions(suppress_tokens=sup, max_length=4))
               .no_speech_prob - want) < 1e-6


# --------------------------------------------------------------------------- host logic
@pytest.fixture(scope="module")
def model_dir(tmp_path_factory):
    return tokfix.make_hf_model_dir(str(tmp_path_factory.mktemp("micro_en_hf")), MICRO_EN)


def _script(tk):
    a, c = tk.encode(" Hello world."), tk.encode(" Whisper transcribes speech into text with timestamps.")

    def script(w, i, prefix, lang):
        if w[1] == 0:
            return WindowOutput([TB] + a + [TB + 150, TB + 150] + c, -4.0, 0.01, -1)
        return WindowOutput([TB] + c + [TB + 500], -3.0, 0.02, -1)
    return script


def test_prompts_carry_no_language_or_task(model_dir, caplog):
    tk = WhisperTokenizer(51864, model_dir + "/tokenizer.json")
    holder = []
    be = make_backend(_script(tk), holder)
    prompt = "  Meeting notes. "
    wav = synth.to_wav_bytes(synth.chirp_clip(0, 45.0))
    with caplog.at_level(logging.WARNING):
        res = be.transcribe(audio=wav, model=model_dir, response_format="verbose_json", prompt=prompt)
    assert not [r for r in caplog.records if "English-only" in r.getMessage()]
    eng = holder[0]
    assert res["language"] == "en" and res["segments"]
    init = tk.encode(" " + prompt.strip())
    (w0, pre0, lang0, task0), (w1, pre1, lang1, task1) = eng.calls[0], eng.calls[1]
    assert pre0 == [EN.sot_prev] + init                      # the prefix is unchanged in form
    kept = [t for s in res["segments"] if s["seek"] == 0 for t in s["tokens"]]
    assert pre1 == [EN.sot_prev] + (init + kept)[-(448 // 2 - 1):]
    assert lang0 is None and lang1 is None and task0 == task1 == "transcribe"
    for _, pre, _, _ in eng.calls:                           # no language or task token anywhere
        assert not [t for t in pre[1:] if EN.eot <= t < TB]
    be.unload_model(model_dir)


def test_language_and_translate_are_coerced_with_one_warning(model_dir, caplog):
    tk = WhisperTokenizer(51864, model_dir + "/tokenizer.json")
    holder = []
    be = make_backend(_script(tk), holder)
    wav = synth.to_wav_bytes(synth.chirp_clip(1, 20.0))
    plain = be.transcribe(audio=wav, model=model_dir, response_format="verbose_json")
    for call in (lambda: be.transcribe(audio=wav, model=model_dir, language="fr", response_format="verbose_json"),
                 lambda: be.translate(audio=wav, model=model_dir, response_format="verbose_json")):
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            got = call()
        assert len([r for r in caplog.records if "English-only" in r.getMessage()]) == 1
        assert got["language"] == "en" and got["text"] == plain["text"]
        assert set(got) == set(plain)                        # response shapes are unchanged
    assert {c[2] for c in holder[0].calls} == {None} and {c[3] for c in holder[0].calls} == {"transcribe"}
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        be.transcribe(audio=wav, model=model_dir, language="en", response_format="json")
    assert not [r for r in caplog.records if "English-only" in r.getMessage()]
    be.unload_model(model_dir)


def test_detect_language_never_calls_the_engine(model_dir):
    class Untouchable(FakeEngine):
        def log_mel(self, clips):
            raise AssertionError("the engine was called")
        encode = decode = detect_language = log_mel

    tk = WhisperTokenizer(51864, model_dir + "/tokenizer.json")
    eng = Untouchable(MICRO_EN, 0, 4)
    res = transcribe_clips(eng, [synth.chirp_clip(2, 3.0)], TranscribeOptions(detect_only=True), tk, ())
    assert (res[0].language, res[0].language_probability, res[0].all_language_probs) == ("en", 1.0, [("en", 1.0)])
    assert res[0].segments == [] and res[0].duration == 3.0
    holder = []
    be = make_backend(None, holder)
    det = be.detect_language(audio=synth.to_wav_bytes(synth.chirp_clip(2, 3.0)), model=model_dir)
    assert det == {"language": "en", "language_probability": 1.0, "all_language_probs": [("en", 1.0)]}
    assert not any(e.calls for e in holder)
    be.unload_model(model_dir)


def test_clip_result_language_fields(model_dir):
    tk = WhisperTokenizer(51864, model_dir + "/tokenizer.json")
    eng = FakeEngine(MICRO_EN, 0, 4, _script(tk))
    pcm = [synth.chirp_clip(3, 20.0)]
    r = transcribe_clips(eng, pcm, TranscribeOptions(), tk, ())[0]
    assert (r.language, r.language_probability, r.all_language_probs) == ("en", 1.0, None)
    r = transcribe_clips(eng, pcm, TranscribeOptions(token_logprobs=True), tk, ())[0]
    assert (r.language, r.language_probability, r.all_language_probs) == ("en", 1.0, [("en", 1.0)])


def test_max_new_tokens_adds_to_the_shorter_prompt(model_dir):
    tk = WhisperTokenizer(51864, model_dir + "/tokenizer.json")
    seen = []

    class Eng(FakeEngine):
        def decode(self, n, cfg, prefix=None, dump_steps=0, languages=None):
            seen.append((cfg.max_length, len(prefix[0]) if prefix else 0, cfg.without_timestamps))
            return super().decode(n, cfg, prefix, dump_steps, languages)

    for nots in (False, True):
        eng = Eng(MICRO_EN, 0, 4, _script(tk))
        transcribe_clips(eng, [synth.chirp_clip(3, 40.0)], TranscribeOptions(max_new_tokens=17, without_timestamps=nots),
                         tk, ())
    assert seen and all(ml == plen + 1 + (1 if nots else 0) + 17 for ml, plen, nots in seen)


def test_session_supported_answers_as_before():
    assert session_supported(TranscribeOptions())
    assert session_supported(TranscribeOptions(beam_size=5))
    assert not session_supported(TranscribeOptions(word_timestamps=True))
    assert not session_supported(TranscribeOptions(detect_only=True))
    assert not session_supported(TranscribeOptions(temperature=(0.0, 0.2)))
    assert not session_supported(TranscribeOptions(max_new_tokens=5))
    assert not session_supported(TranscribeOptions(beam_size=6))


def test_engine_options_carry_the_sentinel():
    """WhisperEngine._opts without a context: task_token < 0 exactly for the English-only vocabulary."""
    from open_speech_amd.engine import WhisperEngine

    class Bare(WhisperEngine):
        def __init__(self, n_vocab):
            self.st = D.SpecialTokens.for_vocab(n_vocab)

    o, _ = Bare(51864)._opts(DecodeConfig(task="translate"), 1, None)
    assert o.task_token == -1 and (o.eot, o.sot, o.no_speech, o.timestamp_begin) == (50256, 50257, 50361, 50363)
    o, _ = Bare(51865)._opts(DecodeConfig(task="translate"), 1, None)
    assert o.task_token == 50358
    with pytest.raises(ValueError):
        Bare(51864).detect_language(1)


# --------------------------------------------------------------------------- ABI
def test_struct_sizes_are_unchanged():
    assert ctypes.sizeof(_lib.osw_decode_opts) == 144
    assert ctypes.sizeof(_lib.osw_window_result) == 64
    assert ctypes.sizeof(_lib.osw_dims) == 40
    assert ctypes.sizeof(_lib.osw_window) == 12
    assert ctypes.sizeof(_lib.osw_profile) == 8 * 18
    assert ctypes.sizeof(_lib.osw_align_window) == 48
    assert ctypes.sizeof(_lib.osw_session_window) == 48
    assert (_lib.OSW_EINVAL, _lib.OSW_ESTATE) == (-22, -101)
    if os.path.exists(_lib.LIB_PATH):
        assert b"0.2" in _lib.load().osw_version()
