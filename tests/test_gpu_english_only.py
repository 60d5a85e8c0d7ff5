"""English-only Whisper models (n_vocab 51864: ``tiny.en`` ... ``medium.en``) on the GPU.

The start sequence is <|startoftranscript|> alone (osw.h: ``task_token < 0``), so with
timestamps one decoder step yields both the no-speech probability (raw logits) and the first
sampled token (rule-masked logits): the combined step of select.h ``sot_sample_step``, in the
select kernels, the batch-1 logits GEMM's fused selection, beam search's first expansion,
sessions and row refill.

Dims ``TINY_EN_TEST``, three short clips, the golden of tools/make_english_golden.py
(transformers fp32 stepped by tests/english_ref.py, minimum top-2 margin in
tests/golden/tiny_en_model.json).  Bounds are those of tests/test_gpu_parity.py and
tests/test_gpu_turbo.py: ids exact, no_speech_prob within 2e-3, sum_logprob within
1e-4 (n + 1) + 1e-3 |ref|, log-softmax of the first sampled step's raw logits within 1e-3.
"""
import ctypes as C
import dataclasses
import json
import os

import numpy as np
import pytest

from open_speech_amd import _lib
from open_speech_amd import dims as D
from open_speech_amd import synth
from open_speech_amd.engine import AlignWindow, DecodeConfig, WhisperEngine
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens
from oracle import decode as odec

import align_ref
import english_ref as eref

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
LSM_TOL = 1e-3
NSP_TOL = 2e-3
CLIPS = {"chirp": lambda: synth.chirp_clip(3, 6.0), "tone": lambda: synth.tone_clip(4.2),
         "noise": lambda: synth.noise_clip(5, 5.0)}


def prefix_tokens(n):
    return [int((i * 97 + 13) % 50000) for i in range(n)]


def lp_bound(n, ref):
    return 1e-4 * (n + 1) + 1e-3 * abs(ref)


class Env:
    pass


@pytest.fixture(scope="module")
def en():
    e = Env()
    e.meta = json.load(open(os.path.join(GOLD, "tiny_en_model.json")))
    e.z = np.load(os.path.join(GOLD, "tiny_en_model.npz"))
    e.d = D.TINY_EN_TEST
    e.st = D.SpecialTokens.for_vocab(e.d.n_vocab)
    e.w = eref.golden_weights(e.d, e.meta["seed"], e.meta["text_pos"], e.meta["nospeech_mix"],
                              tuple(e.meta["sot_positions"]))
    e.eng = WhisperEngine(e.d, device=0, max_batch=4)
    e.eng.load_weights(e.w)
    e.sup = get_suppressed_tokens(WhisperTokenizer(e.d.n_vocab), [-1])
    e.names = list(e.meta["clips"])
    e.clips = [CLIPS[n]() for n in e.names]
    e.max_new = e.meta["max_new"]
    e._orc = None
    yield e
    e.eng.close()


def encode_all(e, idx=None):
    nf = e.eng.log_mel(e.clips)
    idx = range(len(e.clips)) if idx is None else idx
    e.eng.encode([(i, 0, nf[i] - 1) for i in idx])


def cfg_ts(e, **kw):
    return DecodeConfig(suppress_tokens=e.sup, max_length=1 + e.max_new, **kw)


def oracle(e):
    if e._orc is None:
        from oracle.model import WhisperOracle
        e._orc = WhisperOracle(e.d, e.w, fp16=True)
    return e._orc


@pytest.fixture(scope="module")
def greedy3(en):
    """The three clips decoded greedily with timestamps in one call (first step's logits dumped)."""
    encode_all(en)
    return en.eng.decode(3, cfg_ts(en), dump_steps=1)


def test_special_ids_and_sentinel(en):
    st = en.st
    assert (st.eot, st.sot, st.no_speech, st.no_timestamps, st.timestamp_begin) == (50256, 50257, 50361, 50362, 50363)
    o, keep = en.eng._opts(cfg_ts(en), 3, None)
    assert o.task_token < 0
    del keep


def test_greedy_batch3_with_timestamps(en, greedy3):
    """Fails on a tree without the English-only start sequence (no TINY_EN_TEST, and a prompt
    [sot] cannot be expressed)."""
    for name, out in zip(en.names, greedy3):
        pre = f"{name}/ts/"
        want = en.z[pre + "ids"].tolist()
        ref_lp, ref_nsp = float(en.z[pre + "sum_logprob"]), float(en.z[pre + "no_speech_prob"])
        a = odec.log_softmax(out.logits[0])
        b = odec.log_softmax(en.z[pre + "first_logits"])
        lsm = float(np.abs(a - b).max())
        print(f"{name}: ids equal {out.tokens == want}, nsp {out.no_speech_prob:.6f} vs {ref_nsp:.6f}, sum_logprob "
              f"{out.sum_logprob:.5f} vs {ref_lp:.5f} (bound {lp_bound(len(want), ref_lp):.4f}), first-step "
              f"log-softmax max |d| {lsm:.3e}, golden min margin {float(en.z[pre + 'margins'].min()):.3f}")
        assert out.language == -1
        assert out.tokens == want, name
        assert ref_nsp > 0.1 and abs(out.no_speech_prob - ref_nsp) <= NSP_TOL
        assert abs(out.sum_logprob - ref_lp) <= lp_bound(len(want), ref_lp)
        assert lsm <= LSM_TOL
        assert out.tokens[0] >= en.st.timestamp_begin   # the combined step picks under the initial-timestamp rule


@pytest.mark.parametrize("n_prev", [4, 223])
def test_greedy_without_timestamps_after_previous_text(en, n_prev):
    """<|startoftranscript|> is an ordinary forced step here (followed by <|notimestamps|>): its
    raw logits give no_speech_prob, no language is written."""
    prev = prefix_tokens(n_prev)
    prompt = eref.prompt_tokens(en.st, prev, True)
    encode_all(en)
    cfg = DecodeConfig(suppress_tokens=en.sup, without_timestamps=True, max_length=len(prompt) + en.max_new)
    outs = en.eng.decode(3, cfg, prefix=[prompt[:-2]] * 3)
    for name, out in zip(en.names, outs):
        pre = f"{name}/nots{n_prev}/"
        want = en.z[pre + "ids"].tolist()
        ref_lp, ref_nsp = float(en.z[pre + "sum_logprob"]), float(en.z[pre + "no_speech_prob"])
        print(f"{name}: nsp {out.no_speech_prob:.3e} vs {ref_nsp:.3e}, sum_logprob {out.sum_logprob:.5f} vs {ref_lp:.5f}")
        assert out.language == -1
        assert out.tokens == want, name
        assert abs(out.no_speech_prob - ref_nsp) <= NSP_TOL
        assert abs(out.sum_logprob - ref_lp) <= lp_bound(len(want), ref_lp)


def test_batch1_fused_selection_equals_batch_of_three(en, greedy3):
    """One decoder row selects in the logits GEMM's epilogue (SelFuse), three rows in
    select_kernel: the same window must give the same tokens, sum_logprob and no_speech_prob,
    bit for bit.  (The two paths merge their log-sum-exp partials in different orders; on the
    golden's peaked distributions the fp32 results coincide: measured difference 0 for all
    three clips.)"""
    nf = en.eng.log_mel(en.clips)
    for i, name in enumerate(en.names):
        en.eng.encode([(i, 0, nf[i] - 1)])
        one = en.eng.decode(1, cfg_ts(en))[0]
        ref = greedy3[i]
        print(f"{name}: tokens equal {one.tokens == ref.tokens}; sum_logprob {one.sum_logprob!r} vs "
              f"{ref.sum_logprob!r} (d {one.sum_logprob - ref.sum_logprob:.3e}); no_speech_prob "
              f"{one.no_speech_prob!r} vs {ref.no_speech_prob!r} (d {one.no_speech_prob - ref.no_speech_prob:.3e})")
        assert one.language == -1
        assert one.tokens == ref.tokens
        assert one.sum_logprob == ref.sum_logprob
        assert one.no_speech_prob == ref.no_speech_prob


def test_beam5_matches_english_ref(en):
    """Beam search's first expansion is the combined step: ids equal the restated CTranslate2
    beam search (tests/english_ref.py on the fp16 oracle, from the GPU's own encoder output),
    and the golden's; no_speech_prob as in the greedy case."""
    encode_all(en)
    outs = en.eng.decode(3, cfg_ts(en, beam_size=5))
    orc = oracle(en)
    opts = odec.DecodeOptions(suppress_tokens=en.sup, max_length=1 + en.max_new)
    for i, (name, out) in enumerate(zip(en.names, outs)):
        r = eref.beam_from_encoder(orc, orc.cross_kv(en.eng.encoder_output(i)), en.st, opts=opts,
                                   beam=odec.BeamOptions(beam_size=5))
        ref_nsp = float(en.z[f"{name}/ts/no_speech_prob"])
        print(f"{name}: beam sum_logprob {out.sum_logprob:.5f} vs {r.sum_logprob:.5f}, nsp {out.no_speech_prob:.6f} "
              f"vs oracle {r.no_speech_prob:.6f} / golden {ref_nsp:.6f}")
        assert out.language == -1
        assert out.tokens == r.tokens, (name, out.tokens, r.tokens)
        assert out.tokens == en.z[f"{name}/ts/beam_ids"].tolist()
        assert abs(out.no_speech_prob - ref_nsp) <= NSP_TOL
        assert abs(out.sum_logprob - r.sum_logprob) <= lp_bound(len(r.tokens), r.sum_logprob)


def test_sampling_matches_draw_restatement(en):
    """temperature 0.8, best_of 3, fixed seed.  The rows of a window are decoder rows
    3 w .. 3 w + 2 and a draw depends on (seed, row, step, token) only, so the three rows of
    window 0 are replayed as three one-row windows of the same audio with their logits dumped:
    every pick equals english_ref's draw on the GPU's own logits (the existing sampling parity
    test's comparison), and the best_of call returns the tokens of the best of those rows."""
    T, seed = 0.8, 77
    nf = en.eng.log_mel(en.clips[:1])
    en.eng.encode([(0, 0, nf[0] - 1)])
    best = en.eng.decode(1, cfg_ts(en, temperature=T, best_of=3, seed=seed))[0]
    en.eng.encode([(0, 0, nf[0] - 1)] * 3)
    rows = en.eng.decode(3, cfg_ts(en, temperature=T, best_of=1, seed=seed), dump_steps=en.max_new + 1)
    opts = odec.DecodeOptions(suppress_tokens=en.sup, max_length=1 + en.max_new)
    for row, out in enumerate(rows):
        toks, _ = eref.replay_draws(out.logits, en.st, opts, T, seed, row, prompt_len=1)
        assert out.tokens == toks, row
        assert out.tokens[0] >= en.st.timestamp_begin
    assert len({tuple(o.tokens) for o in rows}) > 1    # the rows really draw differently

    def norm(o):
        return o.sum_logprob / max(1, len(o.tokens))
    k = max(range(3), key=lambda i: (norm(rows[i]), -i))
    assert best.tokens == rows[k].tokens
    # (a window's best_of rows share its cross-K/V, three windows each read their own: the sums
    # may differ in accumulation order, not more)
    assert abs(best.sum_logprob - rows[k].sum_logprob) <= 1e-4 * (len(best.tokens) + 1)
    assert abs(best.no_speech_prob - rows[k].no_speech_prob) <= 1e-5
    assert abs(best.no_speech_prob - float(en.z["chirp/ts/no_speech_prob"])) <= NSP_TOL


def _session_windows(e):
    out = []
    for i in range(7):
        pcm = e.clips[i % 3]
        n_prev = (0, 4, 0, 9, 223, 0, 2)[i]
        prefix = ([e.st.sot_prev] + prefix_tokens(n_prev)) if n_prev else None
        out.append(dict(tag=500 + i, pcm=pcm, seek=0, segment_size=len(pcm) // 160, language_token=None,
                        prefix=prefix, token_budget=3 + (5 * i) % 11))
    return out


def _alone(e, w, cfg):
    """The window on its own through osw_decode_windows, twice in one call so that a greedy
    decode takes the select kernel as every multi-row decode does."""
    e.eng.log_mel([w["pcm"]])
    e.eng.encode([(0, w["seek"], w["segment_size"])] * 2)
    c = dataclasses.replace(cfg, token_budget=(w["token_budget"],) * 2)
    return e.eng.decode(2, c, prefix=[w["prefix"]] * 2 if w["prefix"] else None)[0]


@pytest.mark.parametrize("beam", [1, 5])
def test_session_windows_equal_plain_decode(en, beam):
    cfg = DecodeConfig(suppress_tokens=en.sup, max_length=448, beam_size=beam)
    wins = _session_windows(en)
    en.eng.session_begin(cfg)
    got = {}
    try:
        en.eng.session_add(wins[:4])
        added, guard = False, 0
        while True:
            res, active, queued = en.eng.session_step(max_chunks=2, refill_min=1)
            got.update(res)
            if not added:
                en.eng.session_add(wins[4:])
                added = True
                continue
            if active == 0 and queued == 0:
                break
            guard += 1
            assert guard < 500
    finally:
        en.eng.session_end()
    assert sorted(got) == [w["tag"] for w in wins]
    for w in wins:
        r, g = _alone(en, w, cfg), got[w["tag"]]
        assert g.language == -1 and r.language == -1
        assert g.tokens == r.tokens, w["tag"]
        assert g.sum_logprob == r.sum_logprob and g.no_speech_prob == r.no_speech_prob, w["tag"]
        if not w["prefix"]:
            assert g.no_speech_prob > 0.1   # recorded at the combined step


def test_refill_equals_plain_decode(en):
    clips = [en.clips[i % 3] for i in range(9)]
    budgets = tuple(4 + (7 * i) % 13 for i in range(9))
    cfg = DecodeConfig(suppress_tokens=en.sup, max_length=64)
    got = en.eng.transcribe_refill(clips, dataclasses.replace(cfg, token_budget=budgets), refill_min=1)
    for i, g in enumerate(got):
        r = en.eng.transcribe_batch([clips[i]] * 2, dataclasses.replace(cfg, token_budget=(budgets[i],) * 2))[0]
        assert g.language == -1
        assert g.tokens == r.tokens and len(g.tokens) == budgets[i], i
        assert g.sum_logprob == r.sum_logprob and g.no_speech_prob == r.no_speech_prob, i


def test_decode_window_list_equals_encoding_those_windows(en):
    nf = en.eng.log_mel(en.clips)
    cfg = cfg_ts(en)
    en.eng.encode([(i, 0, nf[i] - 1) for i in (2, 0)])
    want = en.eng.decode(2, cfg)
    encode_all(en)
    got = en.eng.decode(2, cfg, windows=[2, 0])
    for g, r in zip(got, want):
        assert g.language == -1
        assert g.tokens == r.tokens
        assert g.sum_logprob == r.sum_logprob and g.no_speech_prob == r.no_speech_prob


@pytest.mark.parametrize("beam", [1, 5])
def test_confidences(en, beam):
    encode_all(en)
    off = en.eng.decode(3, cfg_ts(en, beam_size=beam))
    on = en.eng.decode(3, cfg_ts(en, beam_size=beam, confidences=True))
    try:
        for a, b in zip(on, off):
            assert a.tokens == b.tokens and a.sum_logprob == b.sum_logprob and a.no_speech_prob == b.no_speech_prob
            assert a.language_probs is None
            assert len(a.cum_logprobs) in (len(a.tokens), len(a.tokens) + 1) and len(a.cum_logprobs) >= 1
            assert np.float32(a.cum_logprobs[-1]).tobytes() == np.float32(a.sum_logprob).tobytes()
            assert len(a.token_logprobs) == len(a.tokens) and all(lp <= 0 for lp in a.token_logprobs)
        probs = np.zeros(en.st.n_langs, np.float32)
        rc = en.eng.lib.osw_get_language_probs(en.eng.ctx, 0, probs.ctypes.data_as(C.POINTER(C.c_float)), len(probs))
        assert rc == _lib.OSW_ESTATE
    finally:
        en.eng._set_confidences(False)


def test_language_queries_are_refused(en):
    encode_all(en)
    o, keep = en.eng._opts(cfg_ts(en), 3, None)
    probs = np.zeros((3, en.st.n_langs), np.float32)
    rc = en.eng.lib.osw_detect_language(en.eng.ctx, 3, C.byref(o), probs.ctypes.data_as(C.POINTER(C.c_float)), None)
    del keep
    assert rc == _lib.OSW_EINVAL
    with pytest.raises(ValueError):
        en.eng.detect_language(3)
    # the context still decodes
    assert en.eng.decode(3, cfg_ts(en))[0].language == -1


def test_alignment_with_the_short_forced_sequence(en):
    """[sot, no_timestamps, text..., eot]: M and the token probabilities against the restated
    reference (tools/make_english_golden.py), the tolerances of tests/test_gpu_align.py."""
    z = en.z
    toks = z["align/tokens"].tolist()
    nfr = int(z["align/num_frames"])
    nf = en.eng.log_mel(en.clips[:1])
    assert nf[0] - 1 == nfr
    en.eng.encode([(0, 0, nfr)])
    al = en.eng.align([AlignWindow(window=0, tokens=toks, num_frames=nfr, language=-1)])[0]
    M = en.eng.alignment_matrix(0)
    assert M.shape == z["align/M"].shape == (len(toks) + 1, nfr // 2)
    delta, tol = float(np.abs(M - z["align/M"]).max()), float(z["align/matrix_tol"])
    print(f"max |M_gpu - M_gold| {delta:.4g} (matrix_tol {tol:.4g})")
    assert delta <= tol
    ti, fi = align_ref.dtw(-M)
    np.testing.assert_array_equal(al.token_frame, align_ref.token_frames(ti, fi))
    c_gpu = align_ref.path_cost(-z["align/M"], ti, fi)
    c_gold = align_ref.path_cost(-z["align/M"], z["align/text_indices"], z["align/time_indices"])
    assert c_gpu - c_gold <= 2 * len(ti) * delta
    err = np.abs(np.log(al.token_prob.astype(np.float64)) - np.log(z["align/token_prob"])).max()
    print(f"max |d log token_prob| {err:.3e}")
    assert err <= LSM_TOL
    # one sentinel without the other is refused
    st = en.st
    t = np.ascontiguousarray(toks, dtype=np.int32)
    tf = np.zeros((1, len(toks) + 1), np.int32)
    tp = np.zeros((1, len(toks) + 1), np.float64)
    res = _lib.osw_align_result(token_frame=tf.ctypes.data_as(C.POINTER(C.c_int32)),
                                token_prob=tp.ctypes.data_as(C.POINTER(C.c_double)), stride=len(toks) + 1)
    for lang, task in ((-1, st.transcribe), (st.first_lang, -1)):
        a = (_lib.osw_align_window * 1)(_lib.osw_align_window(
            window=0, sot=st.sot, language=lang, task=task, no_timestamps=st.no_timestamps, eot=st.eot,
            tokens=t.ctypes.data_as(C.POINTER(C.c_int32)), n_tokens=len(toks), num_frames=nfr, median_filter_width=7))
        assert en.eng.lib.osw_align_windows(en.eng.ctx, 1, a, C.byref(res)) == _lib.OSW_EINVAL
    # the length limit is n + 3 <= n_text_ctx
    with pytest.raises(_lib.OswError):
        en.eng.align([AlignWindow(window=0, tokens=[1] * (en.d.n_text_ctx - 2), num_frames=nfr, language=-1)])
    ok = en.eng.align([AlignWindow(window=0, tokens=[1] * (en.d.n_text_ctx - 3), num_frames=nfr, language=-1)])[0]
    assert len(ok.token_frame) == en.d.n_text_ctx - 2


def test_backend_end_to_end(monkeypatch, tmp_path, caplog):
    """A transformers-layout English-only model directory through HipWhisperBackend: translate
    decodes as transcription, the language is "en", word timestamps are present when asked for."""
    import logging

    import tokfix
    from open_speech_amd.backend import HipWhisperBackend

    mid = tokfix.make_hf_model_dir(str(tmp_path / "tiny_en_hf"), D.TINY_EN_TEST)
    monkeypatch.setenv("STT_HIP_BEAM_SIZE", "1")
    monkeypatch.setenv("STT_HIP_MAX_BATCH", "2")
    monkeypatch.setenv("STT_HIP_GPUS", "0")
    monkeypatch.setenv("STT_HIP_LANES", "1")
    monkeypatch.delenv("STT_HIP_WORD_TIMESTAMPS", raising=False)
    b = HipWhisperBackend()
    b.load_model(mid)
    try:
        wav = synth.to_wav_bytes(synth.chirp_clip(41, 8.0))
        a = b.transcribe(wav, mid, response_format="verbose_json")
        with caplog.at_level(logging.WARNING):
            t = b.translate(wav, mid, response_format="verbose_json")
            f = b.transcribe(wav, mid, language="fr", response_format="verbose_json")
        w = b.transcribe(wav, mid, response_format="verbose_json", word_timestamps=True)
        det = b.detect_language(wav, mid)
    finally:
        b.unload_model(mid)
    assert sum(r.name.endswith("backend") and "English-only" in r.getMessage() for r in caplog.records) == 2
    assert a["language"] == "en" and t["language"] == "en" and f["language"] == "en"
    assert a["text"] and t["text"] == a["text"] and f["text"] == a["text"]
    assert [s["tokens"] for s in t["segments"]] == [s["tokens"] for s in a["segments"]]
    assert w["segments"] and all(s["words"] for s in w["segments"])
    for s in w["segments"]:
        assert "".join(x["word"] for x in s["words"]) == s["text"]
    assert det["language"] == "en" and det["language_probability"] == 1.0
