"""Int8 decoder weights (STT_COMPUTE_TYPE=int8_float16) on the GPU: the int8 weight stream of
gemm_skinny_kernel and the multipliers in the skinny, wide and tiled epilogues kernel by kernel
(osw_debug_dec_gemm_quant; references and the bound: tests/q8_ref.py), then whole decodes: an int8
engine against a float16 engine bit for bit (power-of-two multipliers, where the two must agree
exactly), against the fp16 oracle on the dequantised weights (general multipliers), and through the
backend from a CTranslate2 directory with int8 variables.

Every kernel-level test prints its worst |err| / bound.  Measured on an MI355X (DESIGN.md 4.9 has
the record): worst |err| / bound 0.026 / 0.024 (form 0, K 384 / 1536), 0.026 (form 2 split), 0.062
(form 2, the unsplit (32730, 384) projection), 0.025 (form 1), all same-sign; uniform <= 0.012.
(a), (b) and (d) held bit for bit at every shape and row count, and the float16 and int8 engines
of the model-level tests agreed bit for bit.  General multipliers: worst |logit difference| to the
fp16 oracle on the dequantised weights 2.4e-4 (atol 2e-2).
"""
import numpy as np
import pytest

import dec_gemm_ref as R
import q8_ref as Q
from open_speech_amd import _lib, synth, weights
from open_speech_amd import dims as D
from open_speech_amd.engine import DecodeConfig, WhisperEngine
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens

pytestmark = pytest.mark.gpu
F32, F16, F64 = np.float32, np.float16, np.float64


@pytest.fixture(scope="module")
def eng():
    d = D.WhisperDims(n_mels=80, n_audio_state=128, n_audio_head=2, n_audio_layer=1, n_text_state=128,
                      n_text_head=2, n_text_layer=1)
    e = WhisperEngine(d, device=0, max_batch=1)
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint16)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def f16_path(eng, form, hi, lo, h, mult, N, K):
    """The float16 path on W = fp16(q) with each slab (or the unsplit product) multiplied by mult in
    numpy float32: the same MFMA inputs, one fp32 multiply.  The split vocabulary projection sums
    its scaled slabs in slab order (splitk_reduce_kernel), so its slabs come from form 0."""
    M = hi.shape[0]
    if form == 2 and Q.case_ksplit(2, M, N, K) > 1:
        return R.sum_slabs(Q.scale_slabs(eng.debug_dec_gemm(0, hi, lo, h, use_wf=True), mult))
    return Q.scale_slabs(eng.debug_dec_gemm(form, hi, lo, h, use_wf=True), mult)


# --------------------------------------------------------------------------- kernel level
@pytest.mark.parametrize("fam", ["same-sign", "uniform"])
@pytest.mark.parametrize("form,N,K,rows", Q.GPU_CASES, ids=[f"f{c[0]}-{c[1]}x{c[2]}" for c in Q.GPU_CASES])
def test_q8_gemm(eng, fam, form, N, K, rows):
    """Per shape and row count: (a) the int8 stream and the fp16(q) stream give the same bits; (b)
    both equal the float16 path on fp16(q) with one float32 multiply; (c) the slab sum is within
    G S + 2^-24 |ref| of the float64 (hi + lo) (q mult)^T; (d) a row's bits do not depend on the
    row count (skinny MT 1 / MT 2 row groups, the remapped grid, skinny unsplit vs the wide 256
    tile, two row tiles); (e) the guard band behind the result is untouched (debug_dec_gemm_q8
    raises otherwise)."""
    Mmax = max(rows)
    hi, lo, q, mult = Q.q8_inputs(fam, Mmax, N, K, seed=N + K)
    h = q.astype(F16)
    bound, ref = Q.q8_bound(hi, lo, q, mult)
    first, worst = None, 0.0
    for M in rows:
        what = f"q8 {fam} form {form} M {M} N {N} K {K}"
        c1 = eng.debug_dec_gemm_q8(form, hi[:M], lo[:M], q, mult, use_q8_stream=True)
        c0 = eng.debug_dec_gemm_q8(form, hi[:M], lo[:M], q, mult, use_q8_stream=False)
        assert np.isfinite(c1).all(), f"{what}: an element was not written"
        assert same_bits(c1, c0), f"{what}: (a) the int8 stream changes the result"
        assert same_bits(c1, f16_path(eng, form, hi[:M], lo[:M], h, mult, N, K)), \
            f"{what}: (b) differs from the float16 path times the multiplier"
        total = (c1 if form == 2 else R.sum_slabs(c1)).astype(F64)
        r = float((np.abs(total - ref[:M]) / bound[:M]).max())
        worst = max(worst, r)
        assert r <= 1, (what, "(c)", r)
        if first is None:
            first = c1
        else:
            assert same_bits(c1, np.ascontiguousarray(first[..., :M, :])), f"{what}: (d) a row's bits depend on the row count"
    print(f"q8 {fam} form {form} N {N} K {K}: worst |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("form,N,K,rows", [(0, 384, 384, (65, 5, 1)), (2, 32730, 384, (24, 1)), (1, 1536, 1536, (65,))],
                         ids=["f0-384x384", "f2-32730x384", "f1-1536x1536"])
def test_q8_gemm_exact_family(eng, form, N, K, rows):
    """Small-integer activations and weights, multipliers powers of two: every slab equals the
    reference exactly, so a dropped, repeated or misplaced byte of the int8 fragments, k32 step,
    column or multiplier is an integer-sized difference."""
    hi, lo, q, mult = Q.q8_inputs("exact", max(rows), N, K, seed=N + K)
    R.assert_exact(hi, lo, q.astype(F16), K)
    for M in rows:
        ks = Q.case_ksplit(form, M, N, K)
        want = Q.scale_slabs(R.gemm_ref_exact(hi[:M], lo[:M], q.astype(F16), ks), mult)
        want = want[0] if form == 2 else want
        for stream in (True, False):
            c = eng.debug_dec_gemm_q8(form, hi[:M], lo[:M], q, mult, use_q8_stream=stream)
            bad = np.argwhere(c != want)
            assert bad.size == 0, (form, M, stream, "first differences:", bad[:8].tolist(), c[tuple(bad[0])],
                                   want[tuple(bad[0])])


def test_q8_refusals(eng):
    """The opt-in last-arriver tails have no int8 form and are refused by their launchers, a name
    that is no decoder matrix and a wrong size by osw_set_weight_quant: errors, and the context works
    afterwards."""
    hi, lo, q, mult = Q.q8_inputs("uniform", 1, 384, 128, seed=1)
    for form in (3, 4):
        for stream in (True, False):
            with pytest.raises(_lib.OswError, match="int8"):
                eng.debug_dec_gemm_q8(form, hi, lo, q, mult, use_q8_stream=stream)
    d = eng.dims
    Dd = d.n_text_state
    good_q, good_m = np.zeros((Dd, Dd), np.int8), np.ones(Dd, F32)
    with pytest.raises(_lib.OswError):
        eng.set_weight_q8("enc.l0.o.w", good_q, good_m)           # an encoder matrix
    with pytest.raises(_lib.OswError):
        eng.set_weight_q8("dec.crosskv.w", np.zeros((2 * Dd, Dd), np.int8), np.ones(2 * Dd, F32))
    with pytest.raises(_lib.OswError):
        eng.set_weight_q8("dec.l0.o.b", good_q, good_m)           # a vector
    with pytest.raises(_lib.OswError):
        eng.set_weight_q8("dec.l0.o.w", np.zeros((Dd, 2 * Dd), np.int8), good_m)   # wrong size
    with pytest.raises(_lib.OswError):
        eng.set_weight_q8("dec.l0.o.w", good_q, np.full(Dd, np.inf, F32))           # a multiplier not finite
    with pytest.raises(_lib.OswError):
        eng.weight_is_q8("enc.l0.fc1.w")
    with pytest.raises(ValueError):
        eng.set_weight_q8("dec.l0.o.w", good_q.astype(np.int16), good_m)
    assert eng.weight_is_q8("dec.l0.o.w") is False
    eng.set_weight_q8("dec.l0.o.w", good_q, good_m)
    assert eng.weight_is_q8("dec.l0.o.w") is True
    assert np.array_equal(eng.get_weight("dec.l0.o.w"), np.zeros(Dd * Dd, F16))   # fp16(q)
    eng.set_weight("dec.l0.o.w", np.zeros((Dd, Dd), F16))                          # float16 again
    assert eng.weight_is_q8("dec.l0.o.w") is False
    c = eng.debug_dec_gemm_q8(0, hi, lo, q, mult)
    assert np.isfinite(c).all()


def test_q8_weight_round_trip(eng):
    """osw_set_weight_quant leaves fp16(q) in the tensor (what osw_get_weight returns)."""
    Dd = eng.dims.n_text_state
    q = np.random.default_rng(3).integers(-127, 128, (4 * Dd, Dd)).astype(np.int8)
    eng.set_weight_q8("dec.l0.fc1.w", q, np.linspace(0.001, 0.01, 4 * Dd).astype(F32))
    assert np.array_equal(eng.get_weight("dec.l0.fc1.w").reshape(q.shape), q.astype(F16))


# --------------------------------------------------------------------------- model level: bit equality
SUP = get_suppressed_tokens(WhisperTokenizer(D.TINY_TEST.n_vocab), [-1])
NCLIPS = 33


@pytest.fixture(scope="module")
def pair():
    """Engine A: float16, loaded with q * 2^-k (exact in fp16).  Engine B: the same q and 2^-k through
    set_weight_q8.  Power-of-two multipliers scale every partial sum exactly, so every output of
    the two must be the same bits; a difference is a bug of the int8 path."""
    d = D.TINY_TEST
    w = weights.random_weights(d, seed=1234, emb_std=0.5)
    wa, wb = dict(w), dict(w)
    for n in weights.q8_names(d):
        q, mult, h = Q.pow2_quantize(np.asarray(w[n], F32))
        wa[n], wb[n] = h, weights.QuantizedMatrix(q, mult)
    a = WhisperEngine(d, device=0, max_batch=NCLIPS)
    b = WhisperEngine(d, device=0, max_batch=NCLIPS)
    try:
        a.load_weights(wa)
        b.load_weights(wb)
        assert b.weight_is_q8("dec.tok") and b.weight_is_q8("dec.l3.fc2.w") and not a.weight_is_q8("dec.tok")
        clips = [synth.chirp_clip(100 + i, 30.0) for i in range(NCLIPS)]
        yield d, a, b, clips
    finally:
        a.close()
        b.close()


def _same_outputs(oa, ob, what, logits=False):
    assert len(oa) == len(ob)
    for i, (x, y) in enumerate(zip(oa, ob)):
        assert x.tokens == y.tokens, (what, i, "ids")
        assert np.float32(x.sum_logprob).tobytes() == np.float32(y.sum_logprob).tobytes(), (what, i, "sum_logprob")
        assert np.float32(x.no_speech_prob).tobytes() == np.float32(y.no_speech_prob).tobytes(), (what, i, "no_speech_prob")
        assert x.language == y.language, (what, i)
        if logits:
            assert x.logits is not None and same_bits(x.logits, y.logits), (what, i, "logits dump")
        if x.cum_logprobs is not None or y.cum_logprobs is not None:
            assert same_bits(np.asarray(x.cum_logprobs, F32), np.asarray(y.cum_logprobs, F32)), (what, i, "log-probs")


@pytest.mark.parametrize("n", [1, 3, 12, 24, 33])
def test_q8_greedy_equals_float16_bitwise(pair, n):
    """Greedy, 12 dumped steps then graph-replayed ones: 1 window (the fused step with the
    selection in the logits GEMM), 3 (the GELU prologue), 12 (the standalone kernels, MT 1), 24
    (MT 2, the wide logits), 33 (two row groups)."""
    d, a, b, clips = pair
    cfg = DecodeConfig(suppress_tokens=SUP, max_length=32)
    outs = []
    for e in (a, b):
        e.log_mel(clips[:n])
        e.encode([(i, 0, 3000) for i in range(n)])
        outs.append(e.decode(n, cfg, dump_steps=12))
    _same_outputs(outs[0], outs[1], f"greedy {n}", logits=True)
    assert len(outs[1][0].tokens) > 12


@pytest.mark.parametrize("n", [1, 13])
def test_q8_beam_equals_float16_bitwise(pair, n):
    """Beam 5 at 1 and 13 windows (5 and 65 decoder rows), token log-probabilities on."""
    d, a, b, clips = pair
    cfg = DecodeConfig(suppress_tokens=SUP, max_length=24, beam_size=5, confidences=True)
    outs = []
    for e in (a, b):
        e.log_mel(clips[:n])
        e.encode([(i, 0, 3000) for i in range(n)])
        outs.append(e.decode(n, cfg))
    _same_outputs(outs[0], outs[1], f"beam {n}")
    assert outs[1][0].cum_logprobs is not None


def test_q8_session_equals_float16_bitwise(pair):
    """One decode session, windows with and without prefixes, fixed and detected languages,
    different budgets, added in two portions."""
    d, a, b, clips = pair
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    wins = []
    for i in range(9):
        prefix = [st.sot_prev] + [100 + (13 * i + 7 * j) % 300 for j in range(3 + i % 5)] if i % 3 == 1 else None
        wins.append(dict(tag=500 + i, pcm=clips[i], seek=0, segment_size=3000,
                         language_token=None if i % 2 else st.first_lang + i, prefix=prefix, token_budget=5 + (7 * i) % 13))
    cfg = DecodeConfig(suppress_tokens=SUP, max_length=40)
    got = []
    for e in (a, b):
        e.session_begin(cfg)
        res = {}
        try:
            e.session_add(wins[:5])
            added, guard = False, 0
            while True:
                done, active, queued = e.session_step(max_chunks=2)
                res.update(dict(done))
                if not added:
                    e.session_add(wins[5:])
                    added = True
                    continue
                if active == 0 and queued == 0:
                    break
                guard += 1
                assert guard < 500
        finally:
            e.session_end()
        got.append(res)
    assert sorted(got[0]) == sorted(got[1]) == [w["tag"] for w in wins]
    tags = sorted(got[0])
    _same_outputs([got[0][t] for t in tags], [got[1][t] for t in tags], "session")


def test_q8_kind_is_fixed_once_graphs_or_siblings_exist():
    """A matrix changes between float16 and int8 only while nothing has its kind baked in: refused
    once this context holds a decode graph, and while a sibling context lives; same-kind uploads
    stay allowed.  An int8 dec.tok with a float16 dec.l0.qkv.w is refused at finalize and by a
    decode at 1 row and at 12 alike."""
    d = D.MICRO_TEST
    w = weights.random_weights(d, seed=7, emb_std=0.5)
    o = weights.quantize_rows(np.asarray(w["dec.l0.o.w"], F32))
    e = WhisperEngine(d, device=0, max_batch=12)
    try:
        e.load_weights(w)
        sib = e.sibling()
        try:
            with pytest.raises(_lib.OswError, match="sibling"):
                e.set_weight_q8("dec.l0.o.w", o.q, o.mult)
            e.set_weight("dec.l0.o.w", w["dec.l0.o.w"])           # the same kind: allowed
        finally:
            sib.close()
        e.set_weight_q8("dec.l0.o.w", o.q, o.mult)                # no sibling left, no graph yet
        assert e.weight_is_q8("dec.l0.o.w")
        cfg = DecodeConfig(suppress_tokens=get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1]), max_length=24)
        clips = [synth.chirp_clip(i, 30.0) for i in range(12)]
        assert len(e.transcribe_batch(clips[:1], cfg)[0].tokens) > 8   # captures a decode graph
        with pytest.raises(_lib.OswError, match="graphs"):
            e.set_weight("dec.l0.o.w", w["dec.l0.o.w"])           # int8 -> float16
        with pytest.raises(_lib.OswError, match="graphs"):
            e.set_weight_q8("dec.l0.fc1.w", np.zeros(w["dec.l0.fc1.w"].shape, np.int8),
                            np.ones(w["dec.l0.fc1.w"].shape[0], F32))    # float16 -> int8
        e.set_weight_q8("dec.l0.o.w", o.q, o.mult)                # the same kind: allowed
        assert e.weight_is_q8("dec.l0.o.w") and not e.weight_is_q8("dec.l0.fc1.w")
    finally:
        e.close()
    m = WhisperEngine(d, device=0, max_batch=12)
    try:
        t = weights.quantize_rows(np.asarray(w["dec.tok"], F32))
        with pytest.raises(_lib.OswError, match="dec.l0.qkv.w"):
            m.load_weights({**w, "dec.tok": t})                   # refused when the weights are finalized
        m.load_weights(w)
        m.set_weight_q8("dec.tok", t.q, t.mult)                   # set again afterwards: refused by every decode
        for n in (1, 12):
            with pytest.raises(_lib.OswError, match="dec.l0.qkv.w"):
                m.transcribe_batch(clips[:n], cfg)
        qkv = weights.quantize_rows(np.asarray(w["dec.l0.qkv.w"], F32))
        m.set_weight_q8("dec.l0.qkv.w", qkv.q, qkv.mult)
        assert len(m.transcribe_batch(clips[:1], cfg)[0].tokens) > 8
    finally:
        m.close()


# --------------------------------------------------------------------------- model level: general multipliers
def test_q8_greedy_matches_fp16_oracle():
    """quantize_rows multipliers: the GPU logits against the fp16 oracle given the dequantised
    weights, test_gpu_parity's 2e-2 atol; ids equal wherever the oracle's top-2 margin exceeds 4e-2."""
    from oracle import decode as odec
    from oracle.model import WhisperOracle
    d = D.TINY_TEST
    w = weights.random_weights(d, seed=1234, emb_std=0.5)
    wq = weights.quantize_decoder(w, d)
    wdeq = {n: (v.dequantize() if isinstance(v, weights.QuantizedMatrix) else v) for n, v in wq.items()}
    e = WhisperEngine(d, device=0, max_batch=1)
    try:
        e.load_weights(wq)
        st = D.SpecialTokens.for_vocab(d.n_vocab)
        e.log_mel([synth.chirp_clip(11, 30.0)])
        e.encode([(0, 0, 3000)])
        enc = e.encoder_output(0)
        steps = 6
        out = e.decode(1, DecodeConfig(suppress_tokens=SUP, max_length=32), dump_steps=steps)[0]
    finally:
        e.close()
    orc = WhisperOracle(d, wdeq, fp16=True)
    r = odec.greedy_from_encoder(orc, orc.cross_kv(enc), st, opts=odec.DecodeOptions(suppress_tokens=SUP, max_length=32),
                                 keep_logits=steps)
    worst = 0.0
    for i in range(steps):
        worst = max(worst, float(np.abs(out.logits[i] - r.step_logits[i]).max()))
        np.testing.assert_allclose(out.logits[i], r.step_logits[i], atol=2e-2, rtol=0)
    print(f"int8 vs fp16 oracle on the dequantised weights: worst |logit difference| = {worst:.3e} (atol 2e-2)")
    assert out.language == r.language
    # ids: equal wherever the oracle's margin exceeds 4e-2.  At the first difference the GPU's token
    # must be within 4e-2 of the oracle's choice in the oracle's own logits; after such a flip the
    # two sequences are different texts and are not compared further.
    for k, (g, o) in enumerate(zip(out.tokens, r.tokens)):
        if g == o:
            continue
        assert k < steps, f"ids differ at step {k}, beyond the dumped logits"
        margin = float(r.step_logits[k][o] - r.step_logits[k][g])
        assert margin <= 4e-2, f"ids differ at step {k} with an oracle margin of {margin:.3g}"
        break


# --------------------------------------------------------------------------- backend
def test_q8_backend_int8_ct2_directory(monkeypatch, tmp_path):
    """A CTranslate2 directory whose model.bin holds int8 decoder variables, under
    STT_COMPUTE_TYPE=int8_float16: the engine's decoder matrices are int8, the encoder's are
    refused the question, and transcribe of a 12 s WAV returns the engine-level decode of the same
    weights."""
    from test_q8_ref_cpu import int8_ct2_variables
    from open_speech_amd import model_store
    from open_speech_amd.backend import HipWhisperBackend
    from open_speech_amd.ct2 import write_model_bin

    d = D.TINY_TEST
    w = weights.random_weights(d, seed=77, emb_std=0.5)
    v, aliases = int8_ct2_variables(w, d, all_linear=False)
    mdir = tmp_path / "tiny_int8_ct2"
    mdir.mkdir()
    write_model_bin(str(mdir / "model.bin"), v, aliases)
    engines = []

    def factory(dims, gpu, max_batch):
        engines.append(WhisperEngine(dims, device=gpu, max_batch=max_batch))
        return engines[-1]

    monkeypatch.setenv("STT_COMPUTE_TYPE", "int8_float16")
    monkeypatch.setenv("STT_HIP_BEAM_SIZE", "1")
    monkeypatch.setenv("STT_HIP_CONTINUOUS", "0")
    monkeypatch.setenv("STT_HIP_MAX_BATCH", "2")
    monkeypatch.setenv("STT_HIP_GPUS", "0")
    monkeypatch.setenv("STT_HIP_LANES", "1")
    pcm = synth.chirp_clip(5, 12.0)
    b = HipWhisperBackend(engine_factory=factory)
    b.load_model(str(mdir))
    try:
        info = b.loaded_models()[0]
        assert (info["compute_type"] if isinstance(info, dict) else info.compute_type) == "int8_float16"
        assert engines[0].weight_is_q8("dec.l0.fc1.w") and engines[0].weight_is_q8("dec.tok")
        with pytest.raises(_lib.OswError):
            engines[0].weight_is_q8("enc.l0.fc1.w")
        r = b.transcribe(synth.to_wav_bytes(pcm), str(mdir), response_format="verbose_json")
    finally:
        b.unload_model(str(mdir))
    src = model_store.resolve(str(mdir))
    wq = model_store.load_weights(src, "int8_float16")
    assert isinstance(wq["dec.l0.fc1.w"], weights.QuantizedMatrix)
    e = WhisperEngine(d, device=0, max_batch=2)
    try:
        e.load_weights(wq)
        nf = e.log_mel([pcm])[0]
        e.encode([(0, 0, nf - 1)])
        tok = WhisperTokenizer(d.n_vocab, src.tokenizer_json)
        out = e.decode(1, DecodeConfig(suppress_tokens=get_suppressed_tokens(tok, [-1])))[0]
    finally:
        e.close()
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    got = [t for s in r["segments"] for t in s["tokens"] if t < st.eot]
    assert got == [t for t in out.tokens if t < st.eot], (got[:12], out.tokens[:12])
    assert len(got) > 0
