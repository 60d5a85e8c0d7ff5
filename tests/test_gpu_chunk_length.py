"""Shorter encoder windows (faster-whisper's ``chunk_length``; contexts with n_audio_ctx = T =
50 * chunk_length) on the GPU: the window packing, the two attention kernels
alone at the smallest T (a single partial key tile, a query block with fewer than 64 queries,
7-key cross-attention chunks), the whole model against the oracle, the seek loop, a 1280-wide
context, and the 30 s window through the new path bit for bit.  References: tests/chunk_ref.py.

Every test but the refusals of osw_create and the last one fails on a library that serves the
30 s window only: osw_create refuses the contexts.  The cross-attention cases at T = 500, 1000 and
1250 are there for the kernel instantiations the windows of 1, 5 and 15 s do not reach.
"""
import json
import os

import numpy as np
import pytest

import attn_ref as R
import chunk_ref as CR
import mel_ref as M
from open_speech_amd import _lib
from open_speech_amd import dims as D
from open_speech_amd import synth, weights
from open_speech_amd.engine import DecodeConfig, WhisperEngine
from open_speech_amd.segments import (TranscribeOptions, clip_state, consume_window, finish_clip, next_window,
                                      session_config, session_supported, transcribe_clips)
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _small(T, width=128, layers=1):
    return D.WhisperDims(n_mels=80, n_audio_ctx=T, n_audio_state=width, n_audio_head=width // 64,
                         n_audio_layer=layers, n_text_state=width, n_text_head=width // 64, n_text_layer=layers)


_engines = {}


@pytest.fixture(scope="module")
def small_engine():
    """One weightless 128-wide context per T, made on first use (the debug entries need no weights)."""
    def get(T):
        if T not in _engines:
            _engines[T] = WhisperEngine(_small(T), device=0, max_batch=5)
        return _engines[T]
    yield get
    for e in _engines.values():
        e.close()
    _engines.clear()


# --------------------------------------------------------------------------- osw_create
@pytest.mark.parametrize("T", [0, 25, 49, 75, 1475, 1501, 1550, 3000])
def test_create_refuses_other_windows(T):
    d = _small(T)
    cd = _lib.osw_dims(d.n_mels, d.n_audio_ctx, d.n_audio_state, d.n_audio_head, d.n_audio_layer, d.n_vocab,
                       d.n_text_ctx, d.n_text_state, d.n_text_head, d.n_text_layer)
    import ctypes as C
    lib, ctx = _lib.load(), C.c_void_p()
    assert lib.osw_create(C.byref(cd), 0, 1, C.byref(ctx)) == -22
    assert not ctx.value and b"n_audio_ctx" in lib.osw_last_error()


# --------------------------------------------------------------------------- 1. window packing
@pytest.mark.parametrize("T", [50, 250])
def test_window_packing(small_engine, T):
    """mel_window_kernel with n_fr = 2 T frames: seek 0, a window that ends inside the clip, a clip
    shorter than the window (whole and from a seek), a 1-frame clip, a size above the window; every
    fp16 value, the two border rows and the pad columns."""
    eng, n_fr, n_mels = small_engine(T), 2 * T, 80
    assert eng.log_mel(M.window_clips()) == [6501, 101, 1]
    raws = [eng.debug_get_logmel(i) for i in range(3)]
    calls = [[(M.A, 0, n_fr), (M.A, 6501 - n_fr // 2, n_fr), (M.A, 1234, n_fr // 3), (M.A, 3000, 3000)],
             [(M.B_, 0, n_fr), (M.B_, 101 - 7, n_fr), (M.C_, 0, n_fr), (M.A, 6500, 1)]]
    total = 0
    for batch in calls:
        x1 = eng.debug_mel_windows(batch).view(np.uint16)
        assert x1.shape == (len(batch), n_fr + 2, M.c1_of(n_mels))
        for w, (clip, seek, size) in enumerate(batch):
            raw, mx = raws[clip]
            want = CR.window_x1(raw, mx, seek, size, n_mels, n_fr)
            assert int((x1[w] != want).sum()) == 0, (clip, seek, size)
            assert not x1[w, 0].any() and not x1[w, n_fr + 1].any() and not x1[w, :, n_mels:].any()
            total += want.size
    print(f"T={T}: {total} fp16 values bit-identical")


# --------------------------------------------------------------------------- 2. encoder attention
@pytest.mark.parametrize("T", [50, 150, 250, 750])
def test_enc_attn_short_windows(small_engine, T):
    """T = 50: fewer than 64 keys and one sub-64-query block; 150, 250, 750: tails of 22, 58 and 46
    keys.  Key T - 1 ties with a mid key.  Bound: attn_ref's 2^-9 max|V|; the 64- and 128-query
    forms give the same bits."""
    eng = small_engine(T)
    for nb, H in ((1, 2), (2, 3)):
        qkv = CR.enc_inputs(nb, H, T, seed=nb)
        ref, tol = R.enc_attn_ref(qkv), R.enc_tolerance(qkv[2])
        # the tie is live: on the rows that weight key T - 1 most, the mid key carries as much
        s = qkv[0, 0, 0].astype(np.float64) @ qkv[1, 0, 0].astype(np.float64).T * 0.125
        p = np.exp(s - s.max(1, keepdims=True))
        p /= p.sum(1, keepdims=True)
        top = np.argmax(p[:, T - 1])
        assert p[top, T - 1] > 0.05 and p[top, CR.enc_mid_key(T)] > 0.05
        outs = {}
        for name, form in (("auto", WhisperEngine.ATTN_AUTO), ("q64", WhisperEngine.attn_form(qb128=False)),
                           ("q128", WhisperEngine.attn_form(qb128=True))):
            o = eng.debug_enc_attn(qkv, form)
            assert o.shape == (nb * T, H * 64) and np.isfinite(o).all(), name
            err = float(np.abs(o.astype(np.float64) - ref).max())
            print(f"enc_attn T={T} {nb}x{H} {name}: max |out - ref| = {err:.3e} (bound {tol:.3e})")
            assert err <= tol, (name, err, tol)
            outs[name] = o
        np.testing.assert_array_equal(outs["q64"], outs["q128"], err_msg="64 vs 128 queries")
        np.testing.assert_array_equal(outs["q64"], outs["auto"], err_msg="auto")


# --------------------------------------------------------------------------- 3. cross-attention
FORMS = ((0, "launcher's"), (2, "full"))     # debug_dec_xattn's legacy argument


@pytest.mark.parametrize("T", [500, 1000, 1250])
def test_dec_xattn_other_instantiations(small_engine, T):
    """The instantiations the three windows below do not reach: 2, 4 and 5 keys per lane (greedy) and
    1, 2 and 3 key tiles per wave (beam 5) at 63, 125 and 157 keys per chunk, each against float64
    and against the full-width form."""
    assert CR.chunk_forms(T) == {500: (2, 1), 1000: (4, 2), 1250: (5, 3)}[T]
    for beam in (1, 5):
        _xattn_check(small_engine(T), T, beam, (1,), W=2)


@pytest.mark.parametrize("T", [50, 250, 750])
@pytest.mark.parametrize("beam", [1, 5])
def test_dec_xattn_short_windows(small_engine, T, beam):
    """The chunk kernels at per = ceil(T / 8) = 7, 32 and 94 keys per chunk, markers on both sides
    of every chunk edge: the instantiation the launcher picks at T (greedy: 1, 1 and 3 keys per lane;
    beam 5, ks = 1: 1, 1 and 2 key tiles per wave; beam 5, ks = 9: the VALU beam form) and the
    full-width form forced.  The debug entry keeps 64 NaN keys behind the last key of K and V, so a
    load past T makes the output NaN.  Bound: attn_ref.decoder_tolerance (8x a float32 numpy
    evaluation, floor 1e-5 max|V|)."""
    _xattn_check(small_engine(T), T, beam, (1, 9), W=3)


def _xattn_check(eng, T, beam, kss, W):
    H = eng.dims.n_text_head
    assert CR.no_chunk_empty(T)
    for ks in kss:
        slabs, bias, K, V, kinds = CR.xattn_inputs(W, H, T, beam, ks, seed=10 * beam + ks)
        assert CR.marker_weights(slabs, bias, K, beam, kinds, T) > 1.0 / (4 * len(CR.x_markers(T)))
        ref = R.xattn_ref(slabs, bias, K, V, beam)
        tol, e32 = R.decoder_tolerance(ref, R.xattn_ref(slabs, bias, K, V, beam, np.float32, R.attend_f32), 1.0)
        outs = {}
        for legacy, name in FORMS:
            out = eng.debug_dec_xattn(slabs, bias, K, V, beam=beam, legacy=legacy)
            assert np.isfinite(out).all(), (name, "a NaN: a key past T was read, or an element not written")
            err = float(np.abs(out.astype(np.float64) - ref).max())
            print(f"xattn T={T} beam={beam} ks={ks} {name} form: max |out - ref| = {err:.3e} "
                  f"(float32 numpy {e32:.3e}, bound {tol:.3e})")
            assert err <= tol, (name, err, tol)
            outs[legacy] = out
        if beam == 1 or ks > 8:
            # the VALU forms skip keys that contributed p = 0 and no maximum: the same bits
            np.testing.assert_array_equal(outs[0], outs[2])
        # a window gives the same bits at any batch index, in each form
        perm = [2, 0, 1][3 - W:] if W == 3 else [1, 0]
        rows = np.concatenate([np.arange(beam) + w * beam for w in perm])
        for legacy, name in FORMS:
            b = eng.debug_dec_xattn(slabs[:, rows], bias, K[perm], V[perm], beam=beam, legacy=legacy)
            np.testing.assert_array_equal(b, outs[legacy][rows], err_msg=name)
            one = eng.debug_dec_xattn(slabs[:, (W - 1) * beam:], bias, K[W - 1:], V[W - 1:], beam=beam, legacy=legacy)
            np.testing.assert_array_equal(one, outs[legacy][(W - 1) * beam:], err_msg=name)


def test_dec_xattn_refuses_unknown_form(small_engine):
    eng = small_engine(50)
    slabs, bias, K, V, _ = CR.xattn_inputs(1, eng.dims.n_text_head, 50, 1, 1)
    with pytest.raises(_lib.OswError) as ei:
        eng.debug_dec_xattn(slabs, bias, K, V, legacy=3)
    assert ei.value.rc == -22


# --------------------------------------------------------------------------- 4. whole model
@pytest.fixture(scope="module", params=[5, 1], ids=["T250", "T50"])
def tiny_short(request):
    """Tiny dims at chunk_length 5 and 1 with the varied-text weights of the tiny text golden
    (weights.text_positional: distinct ids with a margin)."""
    from oracle.model import WhisperOracle
    m = json.load(open(os.path.join(GOLD, "meta.json")))["tiny_text"]
    d = D.TINY_TEST.with_chunk_length(request.param)
    w = weights.random_weights(d, seed=m["seed"], text_pos=m["text_pos"])
    assert w["enc.pos"].shape == (d.n_audio_ctx, d.n_audio_state)
    eng = WhisperEngine(d, device=0, max_batch=2)
    eng.load_weights(w)
    eng.log_mel([synth.chirp_clip(3, 30.0)])
    eng.encode([(0, 0, d.n_frames)])
    yield d, eng, w, WhisperOracle(d, w, fp16=True), eng.encoder_output(0)
    eng.close()


def test_tiny_encoder_matches_oracle(tiny_short):
    d, eng, w, orc, enc = tiny_short
    assert enc.shape == (d.n_audio_ctx, d.n_audio_state)
    mel = eng.get_mel(0)[:, :d.n_frames]
    ref = orc.encode(mel)
    err = np.abs(enc - ref)
    print(f"T={d.n_audio_ctx}: encoder max |err| {err.max():.3e} mean {err.mean():.3e}")
    np.testing.assert_allclose(enc, ref, atol=2e-2, rtol=0)      # test_gpu_parity's encoder bounds
    assert err.mean() < 2e-3


def test_tiny_greedy_and_beam_match_oracle(tiny_short):
    from oracle import decode as odec
    d, eng, w, orc, enc = tiny_short
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
    xkv = orc.cross_kv(enc)
    opts = odec.DecodeOptions(suppress_tokens=sup, max_length=3 + 40)
    out = eng.decode(1, DecodeConfig(suppress_tokens=sup, max_length=3 + 40))[0]
    r = odec.greedy_from_encoder(orc, xkv, st, opts=opts)
    print(f"T={d.n_audio_ctx}: no-speech gpu {out.no_speech_prob:.6f} oracle {r.no_speech_prob:.6f}; "
          f"{len(set(r.tokens))} distinct ids of {len(r.tokens)}")
    assert out.language == r.language
    assert abs(out.no_speech_prob - r.no_speech_prob) < 2e-3   # fp16 GPU vs numpy: test_gpu_parity's bound
    assert len(set(r.tokens)) >= 16
    assert out.tokens == r.tokens
    probs = eng.detect_language(1)
    assert st.first_lang + int(np.argmax(probs[0])) == r.language
    outb = eng.decode(1, DecodeConfig(suppress_tokens=sup, max_length=3 + 24, beam_size=5))[0]
    rb = odec.beam_from_encoder(orc, xkv, st, opts=odec.DecodeOptions(suppress_tokens=sup, max_length=3 + 24),
                                beam=odec.BeamOptions(beam_size=5))
    assert outb.tokens == rb.tokens and outb.language == rb.language
    assert abs(outb.sum_logprob - rb.sum_logprob) <= 1e-4 * (len(rb.tokens) + 1) + 1e-3 * abs(rb.sum_logprob)


# --------------------------------------------------------------------------- 6. long-form
class Recorder:
    """transcribe_clips' engine seam, recording each window's encoder output and decode."""

    def __init__(self, eng):
        self.eng, self.max_batch, self.max_rows = eng, eng.max_batch, eng.max_rows
        self.enc, self.calls, self._wins = {}, [], []

    def log_mel(self, clips):
        return self.eng.log_mel(clips)

    def encode(self, wins):
        self._wins = list(wins)
        self.eng.encode(wins)
        for k, (_clip, seek, size) in enumerate(wins):
            self.enc[(seek, size)] = self.eng.encoder_output(k)

    def decode(self, n, cfg, prefix=None, dump_steps=0, languages=None):
        outs = self.eng.decode(n, cfg, prefix=prefix, languages=languages)
        for k, w in enumerate(self._wins):
            self.calls.append((w[1], w[2], list(prefix[k]) if prefix else [], outs[k]))
        return outs


@pytest.fixture(scope="module")
def longform():
    d = D.TINY_TEST.with_chunk_length(5)
    w = weights.random_weights(d, seed=1234, emb_std=0.5)
    eng = WhisperEngine(d, device=0, max_batch=2)
    eng.load_weights(w)
    yield d, eng, w, synth.chirp_clip(41, 23.0)
    eng.close()


@pytest.mark.parametrize("beam", [1, 5])
def test_longform_chunk5_matches_oracle(longform, beam):
    """A 23 s clip in 5 s windows (max_new_tokens 24 bounds the oracle's cost: random weights never
    emit <|endoftext|>): seeks, sizes, prompts and ids window by window and the segment list against
    chunk_ref.seek_loop with the oracle decoding the GPU's own encoder outputs."""
    from oracle import decode as odec
    from oracle.model import WhisperOracle
    d, eng, w, pcm = longform
    tok = WhisperTokenizer(d.n_vocab)
    st = tok.special
    sup = get_suppressed_tokens(tok, [-1])
    rec = Recorder(eng)
    opts = TranscribeOptions(beam_size=beam, max_new_tokens=24, chunk_length=5)
    res = transcribe_clips(rec, [pcm], opts, tok, sup)[0]
    gpu = {(s, z): (p, o) for s, z, p, o in rec.calls}
    assert len(rec.calls) >= 5 and all(z <= 500 for _, z, _, _ in rec.calls)
    for enc in rec.enc.values():
        assert enc.shape == (250, d.n_audio_state)
    orc = WhisperOracle(d, w, fp16=True)
    lang = {}

    def decode_window(seek, size, prompt):
        assert (seek, size) in rec.enc, f"the GPU never encoded window (seek {seek}, size {size})"
        xkv = orc.cross_kv(rec.enc[(seek, size)])
        o = odec.DecodeOptions(suppress_tokens=sup, max_length=len(prompt) + 3 + 24)
        if beam == 1:
            r = odec.greedy_from_encoder(orc, xkv, st, language=lang.get("tok"), prev_tokens=prompt[1:], opts=o)
        else:
            r = odec.beam_from_encoder(orc, xkv, st, language=lang.get("tok"), prev_tokens=prompt[1:], opts=o,
                                       beam=odec.BeamOptions(beam_size=beam))
        lang.setdefault("tok", r.language)
        gp, go = gpu[(seek, size)]
        assert gp == prompt, f"window {seek}: prompt differs"
        assert go.tokens == r.tokens, f"window {seek}: GPU ids differ from the oracle's"
        assert abs(go.sum_logprob - r.sum_logprob) <= 1e-4 * (len(r.tokens) + 1) + 1e-3 * abs(r.sum_logprob)
        return go.tokens, go.sum_logprob, go.no_speech_prob

    nf = (len(pcm) + 160) // 160
    wins = CR.seek_loop(decode_window, nf, st, tok.decode, 500)
    assert [(x.seek, x.size) for x in wins] == [(s, z) for s, z, _, _ in rec.calls]
    want = [(a, b, t) for x in wins for a, b, t in x.segments]
    assert [(sg.start, sg.end, sg.tokens) for sg in res.segments] == want
    assert res.duration == pytest.approx(23.0)


@pytest.mark.parametrize("beam", [1, 5])
def test_longform_chunk5_session_equals_batched(longform, beam):
    """The same clip window by window through a decode session (the serving lanes' path: clip_state /
    next_window / consume_window) gives the batched loop's segments."""
    d, eng, w, pcm = longform
    tok = WhisperTokenizer(d.n_vocab)
    sup = get_suppressed_tokens(tok, [-1])
    opts = TranscribeOptions(beam_size=beam, chunk_length=5, tokens_per_second=4.0)
    assert session_supported(opts)
    want = transcribe_clips(eng, [pcm], opts, tok, sup)[0]
    s = clip_state(0, pcm, opts, tok)
    eng.session_begin(session_config(opts, sup))
    n = 0
    try:
        while not s.done:
            win = next_window(s, opts, tok)
            assert win["segment_size"] <= 500
            eng.session_add([dict(tag=n, pcm=pcm, seek=win["seek"], segment_size=win["segment_size"],
                                  language_token=win["language_token"], prefix=win["prefix"] or None,
                                  token_budget=win["token_budget"])])
            res = []
            for _ in range(400):
                res, active, queued = eng.session_step(max_chunks=8)
                if res:
                    break
            assert len(res) == 1 and res[0][0] == n
            consume_window(s, win, res[0][1], opts, tok)
            n += 1
            assert n < 64
    finally:
        eng.session_end()
    got = finish_clip(s, opts, tok)
    assert n >= 5
    assert [(g.seek, g.start, g.end, g.tokens) for g in got.segments] == \
        [(g.seek, g.start, g.end, g.tokens) for g in want.segments]
    assert got.language == want.language


# --------------------------------------------------------------------------- 5. pinned to transformers
def test_chunk_tiny_matches_transformers_golden():
    """tools/make_chunk_golden.py: an fp32 transformers Whisper of tiny dims with
    max_source_positions = 250 and the cropped table.  Every greedy id identical (the golden's
    smallest top-2 margin, >= 0.5, is in chunk_tiny.json); the log-softmax of the first steps within the
    bar test_gpu_parity.py holds the tiny model's logits to (max 0.1, mean 0.01)."""
    m = json.load(open(os.path.join(GOLD, "chunk_tiny.json")))["chunk_tiny"]
    z = np.load(os.path.join(GOLD, "chunk_tiny.npz"))
    assert m["min_top2_margin"] >= 0.5 and m["n_audio_ctx"] == 250
    d = D.TINY_TEST.with_chunk_length(m["chunk_length"])
    eng = WhisperEngine(d, device=0, max_batch=2)
    try:
        eng.load_weights(weights.random_weights(d, seed=m["seed"], text_pos=m["text_pos"]))
        eng.log_mel([synth.chirp_clip(3, 30.0)])
        eng.encode([(0, 0, d.n_frames)])
        enc = eng.encoder_output(0)
        np.testing.assert_allclose(np.linalg.norm(enc.astype(np.float64), axis=1), z["enc_rownorm"], rtol=2e-2)
        sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
        n_full = len(z["full_steps"])
        out = eng.decode(1, DecodeConfig(suppress_tokens=sup), dump_steps=n_full)[0]
        want = z["ids"].tolist()
        assert len(set(want)) >= 150
        assert out.language == int(z["language"])
        assert abs(out.no_speech_prob - float(z["no_speech_prob"])) < 2e-3
        assert out.tokens == want, next(k for k in range(len(want)) if k >= len(out.tokens) or out.tokens[k] != want[k])

        def lsm(x):
            x = np.asarray(x, np.float64)
            mx = x.max()
            return x - (mx + np.log(np.exp(x - mx).sum()))

        for i, step in enumerate(z["full_steps"]):
            err = np.abs(lsm(out.logits[int(step)]) - lsm(z["full_logits"][i]))
            print(f"chunk tiny step {int(step)}: log-softmax max |err| {err.max():.3e} mean {err.mean():.3e}")
            assert err.max() < 0.1 and err.mean() < 0.01
    finally:
        eng.close()


# --------------------------------------------------------------------------- 7. alignment
@pytest.fixture(scope="module")
def aligned():
    import align_ref  # noqa: F401
    from open_speech_amd.engine import AlignWindow
    z = np.load(os.path.join(GOLD, "align_chunk_tiny.npz"))
    wins = [{k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(f"w{i}/")} for i in range(int(z["n_windows"]))]
    d = D.TINY_TEST.with_chunk_length(int(z["chunk_length"]))
    eng = WhisperEngine(d, device=0, max_batch=4)
    eng.load_weights(weights.random_weights(d, seed=1234, emb_std=0.5))
    eng.log_mel([synth.chirp_clip(3, 30.0)])
    eng.encode([(0, int(w["seek"]), int(w["num_frames"])) for w in wins])
    al = eng.align([AlignWindow(window=i, tokens=w["forced"][4:-1].tolist(), num_frames=int(w["num_frames"]),
                                language=int(z["language"])) for i, w in enumerate(wins)])
    Ms = [eng.alignment_matrix(i) for i in range(len(wins))]
    yield eng, wins, al, Ms
    eng.close()


@pytest.mark.parametrize("i", [0, 1, 2])
def test_alignment_at_T250(aligned, i):
    """M against the transformers golden within its matrix_tol (measured by the tool on the reference
    alone; the softmax runs over the model's 250 keys, F = num_frames // 2 <= 250 frames are kept,
    and the median filter reflects at F), token_frame = the numpy DTW of the GPU's own M exactly,
    token probabilities within the log-softmax bar of tests/test_gpu_align.py (1e-3)."""
    import align_ref
    eng, wins, al, Ms = aligned
    w, M = wins[i], Ms[i]
    n = len(w["forced"]) - 5
    assert M.shape == w["M"].shape == (n + 1, int(w["num_frames"]) // 2) and M.shape[1] <= 250
    delta, tol = float(np.abs(M - w["M"]).max()), float(w["matrix_tol"])
    print(f"T=250 n {n} F {M.shape[1]}: max |M_gpu - M_gold| {delta:.4g} (matrix_tol {tol:.4g})")
    assert delta <= tol
    ti, fi = align_ref.dtw(-M)
    np.testing.assert_array_equal(al[i].token_frame, align_ref.token_frames(ti, fi))
    gt, gf = eng.debug_dtw(-M)
    np.testing.assert_array_equal(gt, ti)
    np.testing.assert_array_equal(gf, fi)
    c_gpu = align_ref.path_cost(-w["M"], ti, fi)
    c_gold = align_ref.path_cost(-w["M"], w["text_indices"], w["time_indices"])
    assert c_gpu - c_gold <= 2 * len(ti) * delta
    err = np.abs(np.log(al[i].token_prob.astype(np.float64)) - np.log(w["token_prob"])).max()
    print(f"T=250 n {n}: max |d log token_prob| {err:.3e}")
    assert err <= 1e-3


# --------------------------------------------------------------------------- 8. 1280-wide context
def test_wide_context_at_T250():
    """1280 wide, 1 + 1 layers, T = 250: one encoder block (float4 LayerNorm, the 20-head layouts,
    the tile chooser at M = 250) and a 16-step greedy decode against the oracle, at the bounds of
    tests/test_gpu_widths.py (ids compared while the oracle's own top-2 margin is clear)."""
    from oracle import decode as odec
    from oracle.model import WhisperOracle
    d = D.WhisperDims(n_mels=80, n_audio_state=1280, n_audio_head=20, n_audio_layer=1, n_text_state=1280,
                      n_text_head=20, n_text_layer=1).with_chunk_length(5)
    w = weights.random_weights(d, seed=2, text_pos=80.0)
    eng = WhisperEngine(d, device=0, max_batch=1)
    try:
        eng.load_weights(w)
        orc = WhisperOracle(d, w, fp16=True)
        x = weights.hash_uniform(77, 0, 250 * 1280, 1.0, 0.0).reshape(250, 1280)
        y, ref = eng.encoder_layer(0, x), orc.encoder_layer(0, x)
        err = np.abs(y - ref)
        print(f"1280 wide T=250: encoder_layer max |err| {err.max():.3e} mean {err.mean():.3e}")
        np.testing.assert_allclose(y, ref, atol=2e-2, rtol=0)
        assert err.mean() < 2e-3
        st = D.SpecialTokens.for_vocab(d.n_vocab)
        eng.log_mel([synth.chirp_clip(3, 30.0)])
        eng.encode([(0, 0, 500)])
        enc = eng.encoder_output(0)
        sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
        out = eng.decode(1, DecodeConfig(suppress_tokens=sup, max_length=3 + 16), dump_steps=4)[0]
        opts = odec.DecodeOptions(suppress_tokens=sup, max_length=3 + 16)
        r = odec.greedy_from_encoder(orc, orc.cross_kv(enc), st, opts=opts, keep_logits=16)
        for i in range(4):
            np.testing.assert_allclose(out.logits[i], r.step_logits[i], atol=2e-2, rtol=0)
        n_cmp = 0
        for i, lg in enumerate(r.step_logits):
            v = np.sort(odec.process_logits(lg, r.tokens[:i], st, opts))
            if v[-1] - v[-2] < 0.1:
                break
            n_cmp = i + 1
        print(f"1280 wide T=250: {n_cmp} of 16 steps compared")
        assert n_cmp >= 12, n_cmp
        assert out.tokens[:n_cmp] == r.tokens[:n_cmp] and out.language == r.language
    finally:
        eng.close()


# --------------------------------------------------------------------------- 9. chunk_length = 30
def test_chunk_length_30_is_todays_context():
    """with_chunk_length(30) and a checkpoint-layout load through the cropping loader give the
    encoder output and ids of a context built as before, bit for bit."""
    d = D.TINY_TEST
    d30 = d.with_chunk_length(30)
    assert d30 == d
    w = weights.random_weights(d, seed=1234, emb_std=0.5)
    w30 = weights.from_hf_state_dict(weights.to_hf_state_dict(w, d), d30)
    sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
    cfg = DecodeConfig(suppress_tokens=sup, max_length=40)
    got = []
    for dims, ww in ((d, w), (d30, w30)):
        eng = WhisperEngine(dims, device=0, max_batch=2)
        try:
            eng.load_weights(ww)
            eng.log_mel([synth.chirp_clip(11, 30.0), synth.chirp_clip(12, 9.7)])
            eng.encode([(0, 0, 3000), (1, 0, 970)])
            encs = [eng.encoder_output(i) for i in range(2)]
            outs = eng.decode(2, cfg)
            beam = eng.decode(2, DecodeConfig(suppress_tokens=sup, max_length=24, beam_size=5))
            got.append((encs, outs, beam))
        finally:
            eng.close()
    (ea, oa, ba), (eb, ob, bb) = got
    for i in range(2):
        np.testing.assert_array_equal(ea[i], eb[i])
        assert oa[i].tokens == ob[i].tokens and oa[i].sum_logprob == ob[i].sum_logprob
        assert ba[i].tokens == bb[i].tokens and ba[i].sum_logprob == bb[i].sum_logprob
