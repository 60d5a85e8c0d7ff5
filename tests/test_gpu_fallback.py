"""Temperature fallback on the GPU: the cross-attention kernels with a window map
(osw_debug_dec_xattn_windows), the decode of a list of the encoded windows
(osw_decode_window_list) against a decode after encoding just those windows, and
``transcribe_clips`` with a temperature ladder against ``tests/fallback_ref.py`` driven by direct
``engine.decode`` calls.  Everything here is an equality of bits except the one float64 case,
whose bound is ``attn_ref.decoder_tolerance``."""
import numpy as np
import pytest

import attn_ref as R
import fallback_ref as fr
from open_speech_amd import dims as D
from open_speech_amd import synth, weights
from open_speech_amd._lib import OswError
from open_speech_amd.engine import AlignWindow, DecodeConfig, WhisperEngine
from open_speech_amd.segments import TranscribeOptions, transcribe_clips
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens

pytestmark = pytest.mark.gpu

CLIPS = [(11, 30.0), (21, 30.0), (5, 8.4)]
MAPS = ([3, 1], [4], [2, 0, 4, 1, 3])


def bits(x):
    return np.asarray(x, dtype=np.float32).reshape(-1).view(np.uint32)


# --------------------------------------------------------------------------- 1. the kernels alone
def _dims(width):
    return D.WhisperDims(n_mels=80, n_audio_state=width, n_audio_head=width // 64, n_audio_layer=1,
                         n_text_state=width, n_text_head=width // 64, n_text_layer=1)


@pytest.fixture(scope="module")
def xeng():
    e = WhisperEngine(_dims(D.TINY_TEST.n_text_state), device=0, max_batch=5)
    yield e
    e.close()


_inputs = {}


def xattn_inputs(H, beam, ks):
    """``attn_ref.xattn_inputs(W=5, ...)``, computed once per shape and left unchanged."""
    key = (H, beam, ks)
    if key not in _inputs:
        _inputs[key] = R.xattn_inputs(5, H, beam, ks, seed=900 + 10 * beam + ks)
        for a in _inputs[key][:4]:
            if a is not None:
                a.setflags(write=False)
    return _inputs[key]


def rows_of(wmap, beam):
    return np.concatenate([np.arange(beam) + w * beam for w in wmap])


def check_map(eng, beam, ks, wmap, legacy=False):
    slabs, bias, K, V, _ = xattn_inputs(eng.dims.n_text_head, beam, ks)
    q = np.ascontiguousarray(slabs[:, rows_of(wmap, beam)])
    got = eng.debug_dec_xattn_windows(q, bias, K, V, wmap, beam=beam, legacy=legacy)
    want = eng.debug_dec_xattn(q, bias, K[wmap], V[wmap], beam=beam, legacy=legacy)
    assert np.isfinite(got).all()
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=f"beam={beam} ks={ks} map={wmap} legacy={legacy}")
    return q, got


# beam 1 with ks <= 8 and ks = 9: dec_xattn_chunk_kernel<1>; beam 5 / 8 with ks <= 8:
# dec_xattn_mfma_kernel<5 / 8>; beam 2 / 4 / 5 with ks = 9: dec_xattn_chunk_kernel<2 / 4 / 5>
PATHS = [(1, 3), (1, 8), (1, 9), (5, 3), (8, 5), (2, 9), (4, 9), (5, 9)]


@pytest.mark.parametrize("beam,ks", PATHS, ids=[f"beam{b}-ks{k}" for b, k in PATHS])
def test_xattn_window_map_equals_gathered_kv(xeng, beam, ks):
    for wmap in MAPS:
        check_map(xeng, beam, ks, wmap)


@pytest.mark.parametrize("beam,ks", [(1, 3), (5, 9), (2, 1)])
def test_xattn_window_map_legacy_kernel(xeng, beam, ks):
    for wmap in MAPS:
        check_map(xeng, beam, ks, wmap, legacy=True)


def test_xattn_window_map_at_turbo_head_count():
    """H = 20 (large-v3-turbo's decoder heads): (window, head) pairs are no multiple of the 8
    XCD groups for 1, 2 or 5 row groups."""
    eng = WhisperEngine(_dims(1280), device=0, max_batch=5)
    try:
        for beam, ks in ((1, 3), (5, 3), (5, 9)):
            for wmap in MAPS:
                check_map(eng, beam, ks, wmap)
    finally:
        eng.close()


def test_xattn_window_map_meets_the_float64_bound(xeng):
    beam, ks, wmap = 5, 3, [2, 0, 4, 1, 3]
    slabs, bias, K, V, _ = xattn_inputs(xeng.dims.n_text_head, beam, ks)
    q, got = check_map(xeng, beam, ks, wmap)
    ref = R.xattn_ref(q, bias, K[wmap], V[wmap], beam)
    tol, e32 = R.decoder_tolerance(ref, R.xattn_ref(q, bias, K[wmap], V[wmap], beam, np.float32, R.attend_f32), 1.0)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"mapped xattn beam={beam} ks={ks} map={wmap}: max |out - ref| = {err:.3e} (float32 numpy {e32:.3e}, "
          f"bound {tol:.3e})")
    assert err <= tol, (err, tol)


def test_xattn_window_map_rejects_bad_maps(xeng):
    slabs, bias, K, V, _ = xattn_inputs(xeng.dims.n_text_head, 1, 3)
    for wmap in ([5], [-1], [1, 1], [0, 3, 0], []):
        q = np.ascontiguousarray(slabs[:, :len(wmap)])
        with pytest.raises(OswError) as ei:
            xeng.debug_dec_xattn_windows(q, bias, K, V, wmap)
        assert ei.value.rc == -22, wmap
    # more row groups than K / V hold windows
    with pytest.raises(OswError) as ei:
        xeng.debug_dec_xattn_windows(np.ascontiguousarray(slabs[:, :3]), bias, K[:2], V[:2], [0, 1, 1])
    assert ei.value.rc == -22
    check_map(xeng, 1, 3, [4])      # the context is as good as before


# --------------------------------------------------------------------------- 2. list decode
@pytest.fixture(scope="module")
def tiny():
    d = D.TINY_TEST
    eng = WhisperEngine(d, device=0, max_batch=5)
    eng.load_weights(weights.random_weights(d, seed=1234, emb_std=0.5))
    tok = WhisperTokenizer(d.n_vocab)
    sup = get_suppressed_tokens(tok, [-1])
    pcm = [synth.chirp_clip(s, secs) for s, secs in CLIPS]
    yield d, eng, sup, tok, pcm
    eng.close()


def five_windows(nf):
    return [(0, 0, min(3000, nf[0] - 1)), (1, 0, min(3000, nf[1] - 1)), (2, 0, nf[2] - 1), (0, 1000, 2000),
            (1, 500, 1500)]


ST = D.SpecialTokens.for_vocab(D.TINY_TEST.n_vocab)
PREFIX = [[ST.sot_prev, 1000 + 7 * w, 2000 + w, 3000 + 11 * w] for w in range(5)]   # per encoded window
LANGS = [ST.first_lang + x for x in (0, 3, 7, 1, 20)]
BUDGETS = (30, 12, 9, 20, 17)
MODES = {
    "greedy": (dict(max_length=48), {}),
    "beam": (dict(max_length=40, beam_size=5), {}),
    "sampling": (dict(max_length=48, temperature=1.0, best_of=3, seed=12345), {}),
    "prefix": (dict(max_length=48), dict(prefix=PREFIX)),
    "languages": (dict(max_length=48), dict(languages=LANGS)),
}
LISTS = ([3, 1], [4], [0, 1, 2, 3, 4])


def pick(L, per_window):
    return {k: [v[w] for w in L] for k, v in per_window.items()}


def same_outputs(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.tokens == y.tokens, (what, i)
        assert bits(x.sum_logprob)[0] == bits(y.sum_logprob)[0], (what, i, x.sum_logprob, y.sum_logprob)
        assert bits(x.no_speech_prob)[0] == bits(y.no_speech_prob)[0], (what, i)
        assert x.language == y.language, (what, i)
        assert (x.cum_logprobs is None) == (y.cum_logprobs is None)
        if x.cum_logprobs is not None:
            np.testing.assert_array_equal(bits(x.cum_logprobs), bits(y.cum_logprobs), err_msg=f"{what} {i}")
            np.testing.assert_array_equal(bits(x.language_probs), bits(y.language_probs), err_msg=f"{what} {i}")


@pytest.fixture(scope="module")
def list_runs(tiny):
    """Everything decoded from the one 5-window encoding: the plain decode and the alignment of
    window 2 before and after all the list calls, and every mode's list decodes."""
    d, eng, sup, tok, pcm = tiny
    nf = eng.log_mel(pcm)
    wins = five_windows(nf)
    eng.encode(wins)
    plain_cfg = DecodeConfig(suppress_tokens=sup, max_length=48, token_budget=BUDGETS, confidences=True)
    before = eng.decode(5, plain_cfg)
    aw = AlignWindow(window=2, tokens=[t for t in before[2].tokens if t < ST.eot][:20], num_frames=wins[2][2],
                     language=before[2].language)
    assert aw.tokens
    al_before = eng.align([aw])[0]
    got = {}
    for mode, (kw, per_window) in MODES.items():
        for L in LISTS:
            cfg = DecodeConfig(suppress_tokens=sup, confidences=True, token_budget=tuple(BUDGETS[w] for w in L), **kw)
            got[mode, tuple(L)] = eng.decode(len(L), cfg, windows=L, **pick(L, per_window))
    det = eng.detect_language(5)
    after = eng.decode(5, plain_cfg)
    al_after = eng.align([aw])[0]
    return dict(wins=wins, before=before, after=after, al_before=al_before, al_after=al_after, got=got, det=det)


@pytest.mark.parametrize("mode", list(MODES))
def test_list_decode_equals_decode_of_just_those_windows(tiny, list_runs, mode):
    d, eng, sup, tok, pcm = tiny
    kw, per_window = MODES[mode]
    eng.log_mel(pcm)
    for L in LISTS:
        eng.encode([list_runs["wins"][w] for w in L])
        cfg = DecodeConfig(suppress_tokens=sup, confidences=True, token_budget=tuple(BUDGETS[w] for w in L), **kw)
        want = eng.decode(len(L), cfg, **pick(L, per_window))
        same_outputs(list_runs["got"][mode, tuple(L)], want, f"{mode} {L}")
        assert all(len(o.tokens) > 3 for o in want)
    if mode == "languages":
        assert [o.language for o in list_runs["got"][mode, (3, 1)]] == [LANGS[3], LANGS[1]]
    if mode == "sampling":
        # the draws are the seed's: another seed, another text (at temperature 1.0; at 0.7 these
        # weights' one-token loop leads by so much that every seed draws the same text)
        eng.encode([list_runs["wins"][w] for w in (3, 1)])
        other = eng.decode(2, DecodeConfig(suppress_tokens=sup, token_budget=(BUDGETS[3], BUDGETS[1]),
                                           **dict(kw, seed=54321)))
        assert [o.tokens for o in other] != [o.tokens for o in list_runs["got"][mode, (3, 1)]]


def test_list_decode_leaves_the_encoded_windows_alone(list_runs):
    same_outputs(list_runs["after"], list_runs["before"], "plain decode after the list calls")
    np.testing.assert_array_equal(list_runs["al_after"].token_frame, list_runs["al_before"].token_frame)
    np.testing.assert_array_equal(list_runs["al_after"].token_prob, list_runs["al_before"].token_prob)
    # the windows are told apart (the equalities above are not those of five equal windows)
    assert len({tuple(o.tokens) for o in list_runs["before"]}) == 5
    for w, o in enumerate(list_runs["before"]):   # detect_language still sees all five
        np.testing.assert_array_equal(bits(list_runs["det"][w]), bits(o.language_probs))


def test_list_decode_rejects_bad_lists(tiny):
    d, eng, sup, tok, pcm = tiny
    nf = eng.log_mel(pcm)
    eng.encode(five_windows(nf)[:3])
    cfg = DecodeConfig(suppress_tokens=sup, max_length=16)
    good = eng.decode(2, cfg, windows=[2, 0])
    for L in ([3], [-1], [1, 1], [0, 1, 2, 0], []):
        with pytest.raises(OswError) as ei:
            eng.decode(len(L), cfg, windows=L)
        assert ei.value.rc == -22, L
    eng.session_begin(cfg)
    try:
        with pytest.raises(OswError) as ei:
            eng.decode(1, cfg, windows=[0])
        assert ei.value.rc == -22
    finally:
        eng.session_end()
    eng.encode(five_windows(nf)[:3])
    same_outputs(eng.decode(2, cfg, windows=[2, 0]), good, "after the refusals")


# --------------------------------------------------------------------------- 3. / 4. end to end
class Recorder:
    """A thin wrapper that records every decode call and what it returned."""

    def __init__(self, eng):
        self.eng, self.calls, self.wins = eng, [], []
        self.max_batch, self.max_rows = eng.max_batch, eng.max_rows

    def log_mel(self, clips):
        return self.eng.log_mel(clips)

    def encode(self, wins):
        self.wins = list(wins)
        return self.eng.encode(wins)

    def align(self, windows):
        return self.eng.align(windows)

    def decode(self, n, cfg, **kw):
        outs = self.eng.decode(n, cfg, **kw)
        self.calls.append(dict(wins=list(self.wins), windows=kw.get("windows"), temperature=cfg.temperature,
                               seed=cfg.seed, outs=outs))
        return outs


def avg_logprob(o):
    return o.sum_logprob / (len(o.tokens) + 1)


def seg_tuple(sg):
    if isinstance(sg, dict):
        return (sg["seek"], sg["start"], sg["end"], list(sg["tokens"]), sg["temperature"], sg["avg_logprob"],
                sg["compression_ratio"], sg["no_speech_prob"])
    return (sg.seek, sg.start, sg.end, list(sg.tokens), sg.temperature, sg.avg_logprob, sg.compression_ratio,
            sg.no_speech_prob)


NEW_TOKENS = 20
BASE = dict(no_speech_threshold=None, compression_ratio_threshold=None, max_new_tokens=NEW_TOKENS, best_of=3, seed=77)


def test_ladder_equals_the_reference_on_direct_decodes(tiny):
    d, eng, sup, tok, pcm = tiny
    clip = pcm[0]
    rec = Recorder(eng)
    transcribe_clips(rec, [clip], TranscribeOptions(temperature=0.0, **BASE), tok, sup)
    first = avg_logprob(rec.calls[0]["outs"][0])
    opts = TranscribeOptions(temperature=(0.0, 0.4, 0.8), log_prob_threshold=first + 1e-3 * abs(first), **BASE)
    rec = Recorder(eng)
    got = transcribe_clips(rec, [clip], opts, tok, sup)[0]
    assert [c["windows"] for c in rec.calls[:2]] == [None, [0]]      # the first window did fall back

    # the reference, window by window, on direct engine.decode calls with the documented seeds
    nf = eng.log_mel([clip])
    calls = [0]

    def window_fn(seek, size):
        n_call = calls[0]
        calls[0] += 1

        def fn(k, t, prefix, language):
            eng.encode([(0, seek, size)])
            cfg = DecodeConfig(max_length=len(prefix) + 3 + NEW_TOKENS, suppress_tokens=sup, max_initial_timestamp_index=50,
                               beam_size=1 if t > 0 else opts.beam_size, temperature=t, best_of=opts.best_of,
                               seed=fr.attempt_seed(opts.seed, n_call, k))
            return eng.decode(1, cfg, prefix=[prefix] if prefix else None,
                              languages=None if language is None else [language])[0]
        return fn
    want = fr.transcribe_clip(window_fn, nf[0] - 1, opts, tok)
    assert [seg_tuple(s) for s in got.segments] == [seg_tuple(s) for s in want.segments]
    assert got.language == tok.language_code(want.language)
    assert sum(w["attempts"] for w in want.windows) == len(rec.calls)
    print("windows (seek, attempts, temperature):", [(w["seek"], w["attempts"], w["temperature"]) for w in want.windows])


def test_only_the_failing_clips_are_decoded_again(tiny):
    d, eng, sup, tok, pcm = tiny
    rec = Recorder(eng)
    plain = transcribe_clips(rec, pcm, TranscribeOptions(temperature=0.0, **BASE), tok, sup)
    plain_calls = rec.calls
    firsts = [avg_logprob(o) for o in plain_calls[0]["outs"]]
    assert len(firsts) == 3
    ordered = sorted(set(firsts))
    if len(ordered) < 2:
        pytest.skip(f"the three clips' avg_logprob at temperature 0 are not distinct: {firsts}")
    thr = (ordered[0] + ordered[1]) / 2
    opts = TranscribeOptions(temperature=(0.0, 0.4, 0.8), log_prob_threshold=thr, **BASE)
    rec = Recorder(eng)
    got = transcribe_clips(rec, pcm, opts, tok, sup)
    # every retry names exactly the windows whose result before it fell below the threshold
    expect, n_retry = None, 0
    for c in rec.calls:
        if c["windows"] is None:
            assert not expect
            idx = list(range(len(c["wins"])))
        else:
            idx = c["windows"]
            n_retry += 1
            assert idx == expect and c["temperature"] > 0
        expect = [i for i, o in zip(idx, c["outs"]) if avg_logprob(o) < thr] if c["temperature"] < 0.8 else []
    assert rec.calls[1]["windows"] == [i for i in range(3) if firsts[i] < thr] and n_retry >= 1
    # a clip all of whose windows pass is untouched; a clip whose first window fails carries a temperature
    worst = {}
    for c in plain_calls:
        for w, o in zip(c["wins"], c["outs"]):
            worst[w[0]] = min(worst.get(w[0], 0.0), avg_logprob(o))
    passing = [i for i in range(3) if worst[i] >= thr]
    failing = [i for i in range(3) if firsts[i] < thr]
    print(f"avg_logprob {firsts}, threshold {thr}: passing {passing}, failing {failing}, {n_retry} retry calls")
    assert failing
    for i in passing:
        assert [seg_tuple(s) for s in got[i].segments] == [seg_tuple(s) for s in plain[i].segments]
        assert got[i].language == plain[i].language
    for i in failing:
        assert all(s.temperature > 0 for s in got[i].segments if s.seek == 0)
        assert got[i].language == plain[i].language       # nothing is detected again
