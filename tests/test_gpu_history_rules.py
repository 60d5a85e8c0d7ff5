"""repetition_penalty / no_repeat_ngram_size on the GPU (csrc/decode.hip history_rules_kernel).

Free-running id equality against the oracle is not the yardstick: on the test weights the
oracle's own top-2 margins with a rule on (0.004-0.06) are below the GPU-to-oracle logit
agreement (~1e-2).  The checks here do not depend on margins: the kernel alone bit for bit
against the numpy restatement (tests/history_rules_ref.py, pinned to transformers in
test_history_rules_cpu.py), replays on the GPU's own dumped logits, structural properties
(no repeated n-gram), and the same ids on every decode path."""
import dataclasses

import numpy as np
import pytest

import history_rules_ref as hr
from open_speech_amd import dims as D
from open_speech_amd import synth, weights
from open_speech_amd.engine import DecodeConfig, WhisperEngine
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens

pytestmark = pytest.mark.gpu

CLIP = 11          # chirp_clip(11, 30.0): greedy and beam 5 fall into a one-token loop on these weights
STRIDE = 448


@pytest.fixture(scope="module")
def tiny():
    d = D.TINY_TEST
    eng = WhisperEngine(d, device=0, max_batch=4)
    eng.load_weights(weights.random_weights(d, seed=1234, emb_std=0.5))
    sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
    yield d, eng, sup
    eng.close()


def _encode(eng, seed, secs=30.0):
    pcm = synth.chirp_clip(seed, secs)
    nf = eng.log_mel([pcm])[0]
    eng.encode([(0, 0, min(3000, nf - 1))])
    return pcm


@pytest.fixture(scope="module")
def plain(tiny):
    """The rules-off results every test compares with, computed once."""
    d, eng, sup = tiny
    _encode(eng, CLIP)
    greedy = eng.decode(1, DecodeConfig(suppress_tokens=sup, max_length=64))[0]
    beam = eng.decode(1, DecodeConfig(suppress_tokens=sup, max_length=40, beam_size=5))[0]
    return greedy, beam


def _differs(a, b):
    return sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))


# ------------------------------------------------------------------ 1. the kernel alone
def _logits(rng, rows, V):
    x = (rng.standard_normal((rows, V)) * 3).astype(np.float32)
    x[:, 0] = -np.inf
    x[:, 1] = 0.0
    x[:, 2] = -0.0
    x[:, 3] = np.float32(1e-41)      # subnormal
    x[:, 4] = np.float32(-2.5)
    x[:, 5] = np.float32(7.25)
    return x


def _history(kind, n, V, r):
    if kind == "one":
        h = [r % 6] * n
    elif kind == "distinct":          # (V = 33: distinct up to 33 tokens, then period 33)
        h = [(i + r) % V for i in range(n)]
    elif kind == "period2":
        h = [(3, V - 1)[i % 2] for i in range(n)]
    else:
        h = [(2, 4, 7 + r % 5)[i % 3] for i in range(n)]
    return h


def _check_kernel(eng, x, hists, p, m):
    rows, V = x.shape
    toks = np.full((rows, STRIDE), -7, np.int32)      # (past n_hist: never read)
    for r, h in enumerate(hists):
        toks[r, :len(h)] = h
    n = [len(h) for h in hists]
    got = eng.debug_history_rules(x, toks, n, repetition_penalty=p, no_repeat_ngram_size=m)
    for r, h in enumerate(hists):
        ref = hr.history_rules(x[r], h, repetition_penalty=p, no_repeat_ngram_size=m)
        bad = np.flatnonzero(got[r].view(np.uint32) != ref.view(np.uint32))
        assert bad.size == 0, (V, p, m, r, n[r], bad[:5], got[r][bad[:5]], ref[bad[:5]])
        untouched = np.ones(V, bool)
        untouched[list(set(h))] = False
        assert np.array_equal(got[r].view(np.uint32)[untouched], x[r].view(np.uint32)[untouched])
    return got


@pytest.mark.parametrize("V", [33, 51865])
def test_kernel_matches_restatement_bitwise(tiny, V):
    d, eng, _ = tiny
    rng = np.random.default_rng(V)
    modes = [(p, 0) for p in (1.3, 10.0)] + [(1.0, m) for m in (1, 2, 3, 8, 448)] + \
            [(p, m) for p in (1.3, 10.0) for m in (1, 2, 3, 8, 448)]
    changed = 0
    for p, m in modes:
        ns = sorted({0, 1, max(m - 1, 0), m, 255, 256, 257, 447} | ({448} if m == 448 else set()))
        hists = [_history(kind, n, V, r) for kind in ("one", "distinct", "period2", "period3")
                 for r, n in enumerate(ns)]
        x = _logits(rng, len(hists), V)
        got = _check_kernel(eng, x, hists, p, m)
        changed += int((got.view(np.uint32) != x.view(np.uint32)).sum())
        if m:   # a token both penalised and banned stays -inf: the loop token of a full one-token row
            r = ns.index(447 if m <= 447 else 448)
            assert got[r, hists[r][0]] == -np.inf
    assert changed > 0


def test_kernel_rows_1_and_3(tiny):
    d, eng, _ = tiny
    rng = np.random.default_rng(3)
    for V in (33, 51865):
        _check_kernel(eng, _logits(rng, 1, V), [_history("period3", 40, V, 0)], 1.3, 3)
        _check_kernel(eng, _logits(rng, 3, V), [_history("period2", 257, V, 0), [], _history("one", 5, V, 2)], 10.0, 2)
    # both rules off: nothing is launched, the row comes back as it went in
    x = _logits(rng, 1, 33)
    assert np.array_equal(eng.debug_history_rules(x, np.zeros((1, 8), np.int32), [8]).view(np.uint32),
                          x.view(np.uint32))


def test_kernel_entry_rejects_bad_arguments(tiny):
    d, eng, _ = tiny
    x = np.zeros((1, 33), np.float32)
    with pytest.raises(RuntimeError):     # n_hist > stride
        eng.debug_history_rules(x, np.zeros((1, 4), np.int32), [5], no_repeat_ngram_size=2)
    with pytest.raises(RuntimeError):     # stride > n_text_ctx
        eng.debug_history_rules(x, np.zeros((1, d.n_text_ctx + 1), np.int32), [2], no_repeat_ngram_size=2)
    for bad in (-1, 33):                  # a token outside [0, V)
        with pytest.raises(RuntimeError):
            eng.debug_history_rules(x, np.array([[1, bad, 2]], np.int32), [3], repetition_penalty=1.3)


# ------------------------------------------------------------------ 2. greedy replay
@pytest.mark.parametrize("p,m", [(1.0, 3), (10.0, 0), (1.3, 2)])
def test_greedy_replay_on_own_logits(tiny, plain, p, m):
    """Every pick is the argmax of process_logits(history_rules(raw logits)), replayed on the
    GPU's own dumped raw logits; sum_logprob is the penalised distribution's."""
    from oracle import decode as odec
    d, eng, sup = tiny
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    _encode(eng, CLIP)
    cfg = DecodeConfig(suppress_tokens=sup, max_length=64, repetition_penalty=p, no_repeat_ngram_size=m)
    out = eng.decode(1, cfg, dump_steps=60)[0]
    opts = odec.DecodeOptions(suppress_tokens=sup, max_length=64)
    hist, total = [], 0.0
    for i in range(min(60, len(out.tokens) + 1)):
        x = odec.process_logits(hr.history_rules(out.logits[i], hist, p, m), hist, st, opts)
        t = int(np.argmax(x))
        assert t == (out.tokens[i] if i < len(out.tokens) else st.eot), (i, t, out.tokens)
        total += float(odec.log_softmax(x)[t])
        if t == st.eot:
            break
        hist.append(t)
    scored = out
    if len(out.tokens) > 60:   # the 61st pick's logits were not dumped: the same decode cut after 60 picks
        scored = eng.decode(1, dataclasses.replace(cfg, max_length=3 + 60))[0]
        assert scored.tokens == out.tokens[:60]
    print("sum_logprob", scored.sum_logprob, "replayed", total)
    assert abs(scored.sum_logprob - total) <= 1e-4 * (len(scored.tokens) + 1) + 1e-3 * abs(total)
    # the captured-graph path (no dump) picks the same ids
    again = eng.decode(1, cfg)[0]
    assert again.tokens == out.tokens and again.sum_logprob == out.sum_logprob
    n_diff = _differs(out.tokens, plain[0].tokens)
    print("differs from rules-off at", n_diff, "of", len(out.tokens))
    if (p, m) in ((1.0, 3), (10.0, 0)):
        assert n_diff >= 50
    if m == 3:
        assert not hr.has_repeated_ngram(out.tokens, 3)
    if m == 2:
        assert not hr.has_repeated_ngram(out.tokens, 2)


# ------------------------------------------------------------------ 3. sampling replay
def test_sampling_replay_on_own_logits(tiny):
    from oracle import decode as odec
    d, eng, sup = tiny
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    _encode(eng, CLIP)
    T, seed, p, m = 1.0, 77, 1.3, 2
    cfg = DecodeConfig(suppress_tokens=sup, max_length=64, temperature=T, best_of=1, seed=seed,
                       repetition_penalty=p, no_repeat_ngram_size=m)
    out = eng.decode(1, cfg, dump_steps=8)[0]
    opts = odec.DecodeOptions(suppress_tokens=sup, max_length=64)
    hist = []
    for i in range(min(8, len(out.tokens) + 1)):
        x = odec.process_logits(hr.history_rules(out.logits[i], hist, p, m), hist, st, opts)
        t = odec.sample_token(x, 1.0 / T, seed, 0, 2 + i)   # prompt = sot, lang, task: first pick at step 2
        assert t == (out.tokens[i] if i < len(out.tokens) else st.eot), i
        if t == st.eot:
            break
        hist.append(t)
    assert eng.decode(1, cfg)[0].tokens == out.tokens
    assert not hr.has_repeated_ngram(out.tokens, 2)


# ------------------------------------------------------------------ 4. beam 5
def test_beam_rules(tiny, plain):
    d, eng, sup = tiny
    base = DecodeConfig(suppress_tokens=sup, max_length=40, beam_size=5)
    clips = [synth.chirp_clip(CLIP, 30.0), synth.chirp_clip(5, 8.4), synth.chirp_clip(21, 30.0)]
    for m in (3, 1):
        cfg = dataclasses.replace(base, no_repeat_ngram_size=m)
        one = eng.transcribe_batch(clips[:1], cfg)[0]
        assert len(one.tokens) > m
        assert not hr.has_repeated_ngram(one.tokens, m), one.tokens
        assert one.tokens != plain[1].tokens
        again = eng.transcribe_batch(clips[:1], cfg)[0]
        assert again.tokens == one.tokens and again.sum_logprob == one.sum_logprob
        three = eng.transcribe_batch(clips, cfg)
        assert three[0].tokens == one.tokens
        # (the bound of test_beam_batch_equals_single: 5 vs 15 decoder rows, other GEMM row groups)
        assert abs(one.sum_logprob - three[0].sum_logprob) < 5e-3 * max(1.0, abs(one.sum_logprob))
        for o in three:
            assert not hr.has_repeated_ngram(o.tokens, m)


# ------------------------------------------------------------------ 5. the same result on every path
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


@pytest.mark.parametrize("beam", [1, 5])
@pytest.mark.parametrize("p,m", [(1.0, 3), (1.3, 0)])
def test_same_ids_on_every_path(tiny, beam, p, m):
    d, eng, sup = tiny
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    cfg = DecodeConfig(suppress_tokens=sup, max_length=48, beam_size=beam, repetition_penalty=p,
                       no_repeat_ngram_size=m)
    clips = [synth.chirp_clip(CLIP, 30.0), synth.chirp_clip(21, 30.0), synth.chirp_clip(5, 8.4)]
    budgets = [30, 9, 17]
    prefixes = [None, [st.sot_prev, 400, 401, 402, 403], None]

    def alone(i, prefix):
        nf = eng.log_mel([clips[i]])[0]
        eng.encode([(0, 0, min(3000, nf - 1))])
        c = dataclasses.replace(cfg, token_budget=(budgets[i],))
        return eng.decode(1, c, prefix=[prefix] if prefix else None)[0]

    ref = [alone(i, prefixes[i]) for i in range(3)]
    assert len({tuple(r.tokens) for r in ref}) == 3
    wins = [dict(tag=i, pcm=clips[i], seek=0, segment_size=min(3000, len(clips[i]) // 160), prefix=prefixes[i],
                 token_budget=budgets[i]) for i in range(2)]
    got = _session(eng, cfg, wins)
    assert sorted(got) == [0, 1]
    for i in range(2):
        assert got[i].tokens == ref[i].tokens, (i, got[i].tokens, ref[i].tokens)
    if beam == 1:
        # row refill: 3 clips through 2 rows (no prefixes there), budgets so a row is refilled mid-way
        sib = eng.sibling(max_batch=2)
        try:
            out = sib.transcribe_refill(clips, dataclasses.replace(cfg, token_budget=tuple(budgets)), refill_min=1)
        finally:
            sib.close()
        plain_ref = [ref[0], alone(1, None), ref[2]]
        for i in range(3):
            assert out[i].tokens == plain_ref[i].tokens, (i, out[i].tokens, plain_ref[i].tokens)


# ------------------------------------------------------------------ 6. rules off is the parent
def test_rules_off_is_unchanged(tiny, plain):
    d, eng, sup = tiny
    clips = [synth.chirp_clip(CLIP, 30.0), synth.chirp_clip(21, 30.0), synth.chirp_clip(5, 8.4)]
    for kw, batch in ((dict(max_length=64), clips[:1]), (dict(max_length=64), clips),
                      (dict(max_length=40, beam_size=5), clips[:1])):
        a = eng.transcribe_batch(batch, DecodeConfig(suppress_tokens=sup, **kw))
        b = eng.transcribe_batch(batch, DecodeConfig(suppress_tokens=sup, repetition_penalty=1.0,
                                                     no_repeat_ngram_size=0, **kw))
        for x, y in zip(a, b):
            assert x.tokens == y.tokens and x.sum_logprob == y.sum_logprob and x.no_speech_prob == y.no_speech_prob
    assert eng.transcribe_batch(clips[:1], DecodeConfig(suppress_tokens=sup, max_length=64))[0].tokens == plain[0].tokens


def test_batch1_with_rule_equals_row_of_batch2(tiny):
    """Batch-1 greedy gives up the fused selection while a rule is on: the window decodes as
    it does as row 0 of a batch of 2 (the plain select kernel both times)."""
    d, eng, sup = tiny
    clips = [synth.chirp_clip(CLIP, 30.0), synth.chirp_clip(21, 30.0)]
    cfg = DecodeConfig(suppress_tokens=sup, max_length=64, no_repeat_ngram_size=3, repetition_penalty=1.3)
    one = eng.transcribe_batch(clips[:1], cfg)[0]
    two = eng.transcribe_batch(clips, cfg)[0]
    assert one.tokens == two.tokens
    # 1 vs 2 decoder rows may sum the GEMMs' split-K slabs in another order: rounding noise only
    assert abs(one.sum_logprob - two.sum_logprob) <= 1e-4 * (len(one.tokens) + 1) + 1e-3 * abs(one.sum_logprob)
    assert one.no_speech_prob == pytest.approx(two.no_speech_prob, rel=1e-5)


# ------------------------------------------------------------------ 7. through the backend
def test_backend_no_repeat_ngram(monkeypatch):
    from open_speech_amd.backend import HipWhisperBackend
    mid = "random:tiny-test:1234"
    monkeypatch.setenv("STT_HIP_MAX_BATCH", "4")
    for k in ("STT_HIP_REPETITION_PENALTY", "STT_HIP_NO_REPEAT_NGRAM_SIZE"):
        monkeypatch.delenv(k, raising=False)
    wav = synth.to_wav_bytes(synth.chirp_clip(CLIP, 40.0))

    def run(continuous, **kw):
        if continuous:
            monkeypatch.delenv("STT_HIP_CONTINUOUS", raising=False)   # the default: continuous lanes
        else:
            monkeypatch.setenv("STT_HIP_CONTINUOUS", "0")
        b = HipWhisperBackend()
        try:
            return b.transcribe(wav, mid, response_format="verbose_json", **kw)
        finally:
            b.unload_model(mid)

    cont = run(True, no_repeat_ngram_size=3)
    batch = run(False, no_repeat_ngram_size=3)
    off = run(True)
    key = ("id", "seek", "start", "end", "text", "tokens", "temperature", "compression_ratio")
    assert [[s[k] for k in key] for s in cont["segments"]] == [[s[k] for k in key] for s in batch["segments"]]
    for a, b in zip(cont["segments"], batch["segments"]):
        assert a["avg_logprob"] == pytest.approx(b["avg_logprob"], rel=1e-5, abs=1e-6)
    assert cont["segments"] and len({s["seek"] for s in cont["segments"]}) >= 2
    # a window's segments are slices of its tokens: no 3-gram inside them occurs twice in the window
    n_grams = 0
    for seek in {s["seek"] for s in cont["segments"]}:
        grams = [tuple(s["tokens"][i:i + 3]) for s in cont["segments"] if s["seek"] == seek
                 for i in range(len(s["tokens"]) - 2)]
        assert len(grams) == len(set(grams)), seek
        n_grams += len(grams)
    assert n_grams > 20
    assert [s["tokens"] for s in off["segments"]] != [s["tokens"] for s in cont["segments"]]
