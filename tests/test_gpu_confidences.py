"""Per-token log-probabilities and language probabilities on the GPU (DecodeConfig.confidences;
csrc/select.h select_finalize / lang_softmax, csrc/decode.hip beam_update_body).

What is pinned: the recorded values are the selection's own (the last cumulative entry is
sum_logprob bit for bit, in every mode), recording changes nothing else, each per-token value
replays from the GPU's own dumped logits, every decode path gives the same bits, a beam
hypothesis' history follows it through source-row switches, and the language distribution is
the softmax of the <|startoftranscript|> language logits."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest

import history_rules_ref as hr
from open_speech_amd import dims as D
from open_speech_amd import synth, weights
from open_speech_amd.engine import DecodeConfig, WhisperEngine
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CLIPS = [(11, 30.0), (21, 30.0), (5, 8.4)]
BUDGETS = (30, 0, 9)     # window 0 and 2 end by token budget, window 1 is cut at max_length
MODES = dict(greedy=dict(max_length=64), sampling=dict(max_length=64, temperature=0.7, best_of=5, seed=3),
             beam=dict(max_length=40, beam_size=5))


def bits(x):
    return np.asarray(x, dtype=np.float32).reshape(-1).view(np.uint32)


@pytest.fixture(scope="module")
def tiny():
    d = D.TINY_TEST
    w = weights.random_weights(d, seed=1234, emb_std=0.5)
    eng = WhisperEngine(d, device=0, max_batch=4)
    eng.load_weights(w)
    sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
    yield d, eng, sup, w
    eng.close()


def _encode(eng, clips):
    pcm = [synth.chirp_clip(s, secs) for s, secs in clips]
    nf = eng.log_mel(pcm)
    eng.encode([(i, 0, min(3000, nf[i] - 1)) for i in range(len(pcm))])
    return pcm


@pytest.fixture(scope="module")
def runs(tiny):
    """Every mode's 3-window decode with the flag off and on, computed once."""
    d, eng, sup, _ = tiny
    _encode(eng, CLIPS)
    out = {}
    for name, kw in MODES.items():
        cfg = DecodeConfig(suppress_tokens=sup, token_budget=BUDGETS, **kw)
        out[name] = (eng.decode(3, cfg), eng.decode(3, dataclasses.replace(cfg, confidences=True)))
    return out


def _check_invariant(o):
    """The sum invariant and the entry count of one window's output; returns whether its row
    ended with an <|endoftext|> step."""
    cum = o.cum_logprobs
    ended = o.eot_logprob is not None
    assert len(cum) == len(o.tokens) + (1 if ended else 0)
    assert len(o.token_logprobs) == len(o.tokens)
    assert len(cum) >= 1 and bits(cum[-1])[0] == bits(o.sum_logprob)[0], (cum[-1], o.sum_logprob)
    lps = o.token_logprobs + ([o.eot_logprob] if ended else [])
    assert max(lps) <= 0.0, max(lps)
    return ended


# ------------------------------------------------------------------ 1. the sum invariant
@pytest.mark.parametrize("mode", list(MODES))
def test_sum_invariant_bitwise(runs, mode):
    _, on = runs[mode]
    ended = [_check_invariant(o) for o in on]
    n_max = MODES[mode]["max_length"] - 3
    assert len(on[1].tokens) == n_max and not ended[1]          # cut at max_length: no closing entry
    assert len(on[0].tokens) == BUDGETS[0] and len(on[2].tokens) == BUDGETS[2]
    if mode != "beam":
        # greedy / sampling rows emit <|endoftext|> once the budget is spent; beam search treats
        # the budget step as its last one, so its winner ends with that step's token instead
        assert ended[0] and ended[2]
    print(mode, [(len(o.tokens), len(o.cum_logprobs), o.sum_logprob) for o in on])


# ------------------------------------------------------------------ 2. on does not change the decode
@pytest.mark.parametrize("mode", list(MODES))
def test_on_does_not_change_the_decode(runs, mode):
    off, on = runs[mode]
    for a, b in zip(off, on):
        assert a.tokens == b.tokens
        assert bits(a.sum_logprob)[0] == bits(b.sum_logprob)[0]
        assert bits(a.no_speech_prob)[0] == bits(b.no_speech_prob)[0]
        assert a.language == b.language
        assert a.token_logprobs is None and a.eot_logprob is None and a.language_probs is None
        assert a.cum_logprobs is None


# ------------------------------------------------------------------ 3. greedy replay
@pytest.mark.parametrize("m", [0, 3])
def test_greedy_replay_on_own_logits(tiny, m):
    """Each recorded per-token value is log_softmax(process_logits(raw, history))[token] of the
    GPU's own dumped raw logits (with no_repeat_ngram_size = 3: of the penalised logits), within
    1e-4 + 1e-3 |lp|: the per-token share and the relative part of the existing replay bound on
    the sum (test_gpu_history_rules.py)."""
    from oracle import decode as odec
    d, eng, sup, _ = tiny
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    _encode(eng, CLIPS[:1])
    cfg = DecodeConfig(suppress_tokens=sup, max_length=64, no_repeat_ngram_size=m, confidences=True)
    out = eng.decode(1, cfg, dump_steps=60)[0]
    _check_invariant(out)
    opts = odec.DecodeOptions(suppress_tokens=sup, max_length=64)
    hist, worst = [], 0.0
    assert len(out.tokens) >= 60
    for i in range(60):
        x = odec.process_logits(hr.history_rules(out.logits[i], hist, 1.0, m), hist, st, opts)
        assert int(np.argmax(x)) == out.tokens[i], i
        ref = float(odec.log_softmax(x)[out.tokens[i]])
        err = abs(ref - out.token_logprobs[i])
        worst = max(worst, err)
        assert err <= 1e-4 + 1e-3 * abs(ref), (i, ref, out.token_logprobs[i])
        hist.append(out.tokens[i])
    print("greedy replay m =", m, "max |d lp|", worst)
    # the captured-graph path (no dump) records the same bits
    again = eng.decode(1, cfg)[0]
    assert again.tokens == out.tokens and np.array_equal(bits(again.cum_logprobs), bits(out.cum_logprobs))


# ------------------------------------------------------------------ 4. sampling replay
def test_sampling_replay_on_own_logits(tiny):
    """test_gpu_history_rules.py's recipe: one sampled row (best_of = 1) at batch 1 with its
    seed, the first 8 draws replayed on the dumped logits; the recorded value is the drawn
    token's log-probability under the rule-masked, untempered distribution."""
    from oracle import decode as odec
    d, eng, sup, _ = tiny
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    _encode(eng, CLIPS[:1])
    T, seed = 0.7, 77
    cfg = DecodeConfig(suppress_tokens=sup, max_length=64, temperature=T, best_of=1, seed=seed, confidences=True)
    out = eng.decode(1, cfg, dump_steps=8)[0]
    _check_invariant(out)
    opts = odec.DecodeOptions(suppress_tokens=sup, max_length=64)
    hist, worst = [], 0.0
    assert len(out.tokens) >= 8
    for i in range(8):
        x = odec.process_logits(out.logits[i], hist, st, opts)
        t = odec.sample_token(x, 1.0 / T, seed, 0, 2 + i)   # prompt = sot, lang, task: first pick at step 2
        assert t == out.tokens[i], i
        ref = float(odec.log_softmax(x)[t])
        err = abs(ref - out.token_logprobs[i])
        worst = max(worst, err)
        assert err <= 1e-4 + 1e-3 * abs(ref), (i, ref, out.token_logprobs[i])
        hist.append(t)
    print("sampling replay max |d lp|", worst)
    again = eng.decode(1, cfg)[0]
    assert again.tokens == out.tokens and np.array_equal(bits(again.cum_logprobs), bits(out.cum_logprobs))


# ------------------------------------------------------------------ 5. every path gives the same bits
def _session(eng, cfg, wins):
    """Two windows queued at different times: the second joins while the first decodes."""
    eng.session_begin(cfg)
    got = {}
    try:
        eng.session_add(wins[:1])
        res, _, _ = eng.session_step(max_chunks=1)
        got.update(res)
        eng.session_add(wins[1:])
        for _ in range(400):
            res, active, queued = eng.session_step(max_chunks=2)
            got.update(res)
            if active == 0 and queued == 0:
                break
    finally:
        eng.session_end()
    return got


def _same(a, b, what):
    assert a.tokens == b.tokens, what
    assert np.array_equal(bits(a.cum_logprobs), bits(b.cum_logprobs)), \
        (what, float(np.max(np.abs(a.cum_logprobs.astype(np.float64) - b.cum_logprobs))))
    assert np.array_equal(bits(a.language_probs), bits(b.language_probs)), what


@pytest.mark.parametrize("beam", [1, 5])
def test_every_path_gives_the_same_bits(tiny, beam):
    d, eng, sup, _ = tiny
    cfg = DecodeConfig(suppress_tokens=sup, max_length=48, beam_size=beam, confidences=True)
    pcm = [synth.chirp_clip(s, secs) for s, secs in CLIPS]
    _encode(eng, CLIPS[:1])
    alone = eng.decode(1, dataclasses.replace(cfg, token_budget=BUDGETS[:1]))[0]
    _check_invariant(alone)
    three = eng.transcribe_batch(pcm, dataclasses.replace(cfg, token_budget=(30, 9, 17)))
    _same(alone, three[0], "batch of 3")
    wins = [dict(tag=i, pcm=pcm[i], seek=0, segment_size=min(3000, len(pcm[i]) // 160), token_budget=(30, 9)[i])
            for i in range(2)]
    got = _session(eng, cfg, wins)
    assert sorted(got) == [0, 1]
    _same(alone, got[0], "decode session")
    _check_invariant(got[1])
    if beam == 1:
        sib = eng.sibling(max_batch=2)
        try:
            out = sib.transcribe_refill(pcm, dataclasses.replace(cfg, token_budget=(30, 9, 17)), refill_min=1)
        finally:
            sib.close()
        _same(alone, out[0], "row refill")
        for o in out:
            _check_invariant(o)
        for a, b in zip(three, out):
            _same(a, b, "batch of 3 vs row refill")


_CHILD = """
import sys
sys.path.insert(0, %r)
import osw_path
osw_path.load()
import numpy as np
from open_speech_amd import dims as D, synth, weights
from open_speech_amd.engine import DecodeConfig, WhisperEngine
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens
d = D.TINY_TEST
eng = WhisperEngine(d, device=0, max_batch=1)
eng.load_weights(weights.random_weights(d, seed=1234, emb_std=0.5))
sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
nf = eng.log_mel([synth.chirp_clip(11, 30.0)])
eng.encode([(0, 0, min(3000, nf[0] - 1))])
o = eng.decode(1, DecodeConfig(suppress_tokens=sup, max_length=48, token_budget=(30,), confidences=True))[0]
print("CUM", o.cum_logprobs.view(np.uint32).tolist())
print("LANG", o.language_probs.view(np.uint32).tolist())
eng.close()
"""


def test_batch1_fused_selection_records_the_same_bits(tiny):
    """Batch-1 greedy runs select_finalize in the logits GEMM's epilogue; with
    OSW_NO_FUSE_SELECT (read once per process, hence the child process) the select kernel runs
    it.  Both record the same bits.  (No test compared the two paths before this one.)"""
    d, eng, sup, _ = tiny
    _encode(eng, CLIPS[:1])
    here = eng.decode(1, DecodeConfig(suppress_tokens=sup, max_length=48, token_budget=(30,), confidences=True))[0]
    env = dict(os.environ, OSW_NO_FUSE_SELECT="1")
    p = subprocess.run([sys.executable, "-c", _CHILD % ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = dict(l.split(" ", 1) for l in p.stdout.splitlines() if l.startswith(("CUM ", "LANG ")))
    assert eval(lines["CUM"]) == bits(here.cum_logprobs).tolist()
    assert eval(lines["LANG"]) == bits(here.language_probs).tolist()


# ------------------------------------------------------------------ 6. beam history follows the hypothesis
@pytest.fixture(scope="module")
def switching(tiny):
    """A beam-5 window whose winner was not the top hypothesis at every length, i.e. whose
    ancestry changed source rows: with token_budget = b the decode ends at step b and returns
    the top hypothesis of that length; where that is not the winner's prefix, the winner's
    prefix sat in another row then, and it sits in row 0 at the end.  The plain decode on these
    weights falls into a one-token loop (beam sum -0.38 over 37 tokens) and its winner never
    leaves row 0 (10 clips scanned), so the window decodes with no_repeat_ngram_size on, which
    the beam kernels see only as other logits; the first setting that switches is used."""
    d, eng, sup, _ = tiny
    for m, clip in [(2, CLIPS[0]), (3, CLIPS[0]), (1, CLIPS[0]), (2, CLIPS[1]), (2, CLIPS[2])]:
        base = DecodeConfig(suppress_tokens=sup, max_length=40, beam_size=5, no_repeat_ngram_size=m)
        _encode(eng, [clip])
        off = eng.decode(1, base)[0]
        tops = {b: eng.decode(1, dataclasses.replace(base, token_budget=(b,)))[0] for b in range(1, len(off.tokens))}
        moved = [b for b, o in tops.items() if o.tokens != off.tokens[:b]]
        print("no_repeat_ngram_size", m, "clip", clip, "winner's prefix was not the top hypothesis at lengths", moved)
        if moved:
            on = eng.decode(1, dataclasses.replace(base, confidences=True))[0]
            return off, on, tops, moved
    return None


def test_beam_history_follows_the_hypothesis(switching):
    assert switching is not None, "no clip whose beam-5 winner switched source rows"
    off, on, tops, moved = switching
    assert len(moved) >= 1
    assert on.tokens == off.tokens and bits(on.sum_logprob)[0] == bits(off.sum_logprob)[0]
    _check_invariant(on)
    # where the winner's prefix was the top hypothesis, the budgeted run's score is that entry
    same = [b for b in tops if b not in moved]
    for b in same:
        assert bits(tops[b].sum_logprob)[0] == bits(on.cum_logprobs[b - 1])[0], b
    print("entries checked against budgeted runs:", len(same), "of", len(on.tokens))


# ------------------------------------------------------------------ 7. language probabilities
@pytest.fixture(scope="module")
def langs(tiny):
    d, eng, sup, _ = tiny
    _encode(eng, CLIPS)
    cfg = DecodeConfig(suppress_tokens=sup, max_length=24, confidences=True)
    before = eng.decode(3, cfg)
    enc = [eng.encoder_output(i) for i in range(3)]
    probs, raw = eng.detect_language(3, return_logits=True)
    after = eng.decode(3, cfg)
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    given = eng.decode(3, cfg, languages=[st.first_lang + 5] * 3)
    return before, after, given, probs, raw, enc


def test_language_probs_are_the_softmax_of_the_language_logits(tiny, langs):
    """Against numpy float64 on osw_detect_language's own raw logits: relative 1e-5 (+ 1e-7
    absolute): a fast fp32 exp of an argument up to ~30 carries ~30 log2(e) 2^-24 = 2.6e-6."""
    d = tiny[0]
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    before, after, given, probs, raw, _ = langs
    x = raw.astype(np.float64)
    ref = np.exp(x - x.max(1, keepdims=True))
    ref /= ref.sum(1, keepdims=True)
    s = probs.astype(np.float64).sum(1)
    print("sum", s, "max rel", float(np.max(np.abs(probs - ref) / ref)))
    assert np.all(np.abs(s - 1.0) <= 1e-5)
    assert np.all(np.abs(probs - ref) <= 1e-5 * ref + 1e-7)
    for i in range(3):
        assert st.first_lang + int(np.argmax(before[i].language_probs)) == before[i].language
        # decode()'s distribution with no prefix is detect_language's, bit for bit
        assert np.array_equal(bits(before[i].language_probs), bits(probs[i]))
        # a given language still returns the distribution
        assert given[i].language == st.first_lang + 5
        assert np.array_equal(bits(given[i].language_probs), bits(probs[i]))
        # a decode after detect_language returns what it returned before it
        a, b = before[i], after[i]
        assert a.tokens == b.tokens and bits(a.sum_logprob)[0] == bits(b.sum_logprob)[0]
        assert np.array_equal(bits(a.cum_logprobs), bits(b.cum_logprobs))
        assert np.array_equal(bits(a.language_probs), bits(b.language_probs))
        assert a.language == b.language and a.no_speech_prob == b.no_speech_prob


def test_language_probs_against_the_oracle(tiny, langs):
    """The GPU logits are held to 2e-2 of the fp16 oracle's at these dims (test_gpu_parity.py),
    so p_gpu / p_oracle lies within e^(+-0.04) and the argmax matches where the oracle's top-2
    language margin exceeds 4e-2."""
    from oracle import decode as odec
    from oracle.model import WhisperOracle
    d, eng, sup, w = tiny
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    _, _, _, probs, _, enc = langs
    orc = WhisperOracle(d, w, fp16=True)
    qualify, worst = 0, 0.0
    for i in range(3):
        r = odec.greedy_from_encoder(orc, orc.cross_kv(enc[i]), st,
                                     opts=odec.DecodeOptions(suppress_tokens=sup, max_length=4))
        x = r.prompt_logits[0][st.first_lang:st.first_lang + st.n_langs].astype(np.float64)
        p = np.exp(x - x.max())
        p /= p.sum()
        top = np.sort(x)[::-1]
        margin = float(top[0] - top[1])
        ratio = float(np.max(np.abs(probs[i] - p) / p))
        worst = max(worst, ratio)
        print("window", i, "oracle top-2 language margin", margin, "max |dp| / p", ratio)
        if margin > 4e-2:
            qualify += 1
            assert int(np.argmax(probs[i])) == int(np.argmax(p))
        assert np.all(np.abs(probs[i] - p) <= p * (np.exp(0.04) - 1.0))
    print("measured max |dp| / p", worst, "bound", float(np.exp(0.04) - 1.0))
    assert qualify >= 2


def test_entry_points_refuse_what_the_header_says(tiny):
    """Flag off: the getters return OSW_ESTATE (-101); an index past the last call's results and
    a wrong n_langs are OSW_EINVAL (-22); while a session is open osw_detect_language and
    osw_set_confidences return OSW_EINVAL like the other decode entries."""
    import ctypes as C
    d, eng, sup, _ = tiny
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    f32p = C.POINTER(C.c_float)
    _encode(eng, CLIPS[:1])
    cfg = DecodeConfig(suppress_tokens=sup, max_length=16)
    eng.decode(1, cfg)
    n, probs = C.c_int32(), np.zeros(st.n_langs, np.float32)
    assert eng.lib.osw_get_token_logprobs(eng.ctx, 0, None, 0, C.byref(n)) == -101
    assert eng.lib.osw_get_language_probs(eng.ctx, 0, probs.ctypes.data_as(f32p), st.n_langs) == -101
    on = eng.decode(1, dataclasses.replace(cfg, confidences=True))[0]
    assert eng.lib.osw_get_token_logprobs(eng.ctx, 0, None, 0, C.byref(n)) == 0 and n.value == len(on.cum_logprobs)
    assert eng.lib.osw_get_token_logprobs(eng.ctx, 1, None, 0, C.byref(n)) == -22
    assert eng.lib.osw_get_language_probs(eng.ctx, 0, probs.ctypes.data_as(f32p), st.n_langs - 1) == -22
    small = np.zeros(2, np.float32)
    assert eng.lib.osw_get_token_logprobs(eng.ctx, 0, small.ctypes.data_as(f32p), 2, C.byref(n)) == -22
    eng.session_begin(cfg)
    try:
        with pytest.raises(RuntimeError):
            eng.detect_language(1)
        assert eng.lib.osw_set_confidences(eng.ctx, 0) == -22
    finally:
        eng.session_end()
    # the context still decodes, and detects, as before
    _encode(eng, CLIPS[:1])
    again = eng.decode(1, dataclasses.replace(cfg, confidences=True))[0]
    assert again.tokens == on.tokens and np.array_equal(bits(again.cum_logprobs), bits(on.cum_logprobs))
    assert np.array_equal(bits(eng.detect_language(1)[0]), bits(on.language_probs))


# ------------------------------------------------------------------ 8. turbo dims
def test_turbo_text_golden_with_confidences():
    """The benchmarked dims with the text golden's weights, first golden clip: ids equal the
    golden's with the flag on, the sum invariant holds, and at the steps whose full-vocabulary
    logits the golden holds the recorded value is within 1e-3 of
    log_softmax(process_logits(golden logits, golden history))[token]."""
    import json
    from oracle import decode as odec
    m = json.load(open(os.path.join(GOLD, "meta.json")))["turbo_text"]
    z = np.load(os.path.join(GOLD, "turbo_text.npz"))
    d = D.LARGE_V3_TURBO
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    eng = WhisperEngine(d, device=0, max_batch=1)
    try:
        eng.init_random(seed=m["seed"], text_pos=m["text_pos"])
        eng.set_weight("dec.pos", z["pos_table"])
        sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
        eng.log_mel([synth.chirp_clip(0, 30.0)])
        eng.encode([(0, 0, 3000)])
        out = eng.decode(1, DecodeConfig(suppress_tokens=sup, confidences=True))[0]
    finally:
        eng.close()
    pre = "chirp0/"
    want = z[pre + "ids"].tolist()
    assert out.tokens == want
    _check_invariant(out)
    assert abs(out.sum_logprob - float(z[pre + "sum_logprob"])) <= 1e-4 * (len(want) + 1)
    opts = odec.DecodeOptions(suppress_tokens=sup)
    worst, n = 0.0, 0
    for j, s in enumerate(z[pre + "full_steps"].tolist()):
        if s >= len(want):
            continue
        x = odec.process_logits(z[pre + "full_logits"][j], want[:s], st, opts)
        ref = float(odec.log_softmax(x)[want[s]])
        worst = max(worst, abs(ref - out.token_logprobs[s]))
        n += 1
    print("turbo per-token |d lp| max", worst, "over", n, "full-vocabulary steps")
    assert n >= 4 and worst <= 1e-3


# ------------------------------------------------------------------ 9. through the backend
def test_backend_logprobs_continuous_equals_batched(monkeypatch):
    from open_speech_amd.backend import HipWhisperBackend
    mid = "random:tiny-test:1234"
    monkeypatch.setenv("STT_HIP_MAX_BATCH", "4")
    monkeypatch.delenv("STT_HIP_LOGPROBS", raising=False)
    wav = synth.to_wav_bytes(synth.chirp_clip(11, 75.0))

    def run(continuous):
        if continuous:
            monkeypatch.delenv("STT_HIP_CONTINUOUS", raising=False)   # the default: continuous lanes
        else:
            monkeypatch.setenv("STT_HIP_CONTINUOUS", "0")
        b = HipWhisperBackend()
        try:
            return (b.transcribe(wav, mid, response_format="verbose_json", include=["logprobs"]),
                    b.detect_language(wav, mid))
        finally:
            b.unload_model(mid)

    (cont, det), (batch, det2) = run(True), run(False)
    assert cont["segments"] and len({s["seek"] for s in cont["segments"]}) >= 2
    assert [s["tokens"] for s in cont["segments"]] == [s["tokens"] for s in batch["segments"]]
    assert cont["logprobs"] == batch["logprobs"] and cont["logprobs"]
    assert [s["token_logprobs"] for s in cont["segments"]] == [s["token_logprobs"] for s in batch["segments"]]
    for s in cont["segments"]:
        assert len(s["token_logprobs"]) == len(s["tokens"])
        assert max(s["token_logprobs"]) <= 0.0
    eot = D.SpecialTokens.for_vocab(D.TINY_TEST.n_vocab).eot
    assert len(cont["logprobs"]) == sum(1 for s in cont["segments"] for t in s["tokens"] if t < eot)
    assert cont["language_probability"] == batch["language_probability"]
    assert det == det2
    assert det["language_probability"] == max(p for _, p in det["all_language_probs"])
    assert dict(det["all_language_probs"])[det["language"]] == det["language_probability"]
