"""Temperature fallback on the decode sessions (osw_session_retries / osw_session_retry): a held
window goes back to decoding in its own slot with ``best_of`` sampled rows, beside slots that go
on at temperature 0 (greedy, or beam search with five rows per slot).

Every comparison is exact (``==`` / ``assert_array_equal``) against the batch path on a second
engine of the same weights: a retried window equals ``decode`` of that window alone (``_alone``, as
in tests/test_gpu_session_align.py) at the retry's temperature, ``best_of``, seed, prefix, language
and token budget (ids, the bits of ``sum_logprob`` and ``no_speech_prob``, the language, and with
confidences on ``cum_logprobs`` / ``language_probs``), and every temperature-0 window equals its
decode alone.  Rows are independent in every decoder kernel and the Gumbel key depends only on
(seed, row in window, step, token), so there is no tolerance to state.  Random weights never emit
<|endoftext|>: the token budgets end the rows."""
import dataclasses

import numpy as np
import pytest

from open_speech_amd import dims as D
from open_speech_amd._lib import OSW_EINVAL, OSW_ESTATE, OswError
from test_gpu_session_align import _alone, _cfg, _engines, _window

pytestmark = pytest.mark.gpu


def _retry_cfg(cfg, T, best_of, seed):
    """The batch path's options for one attempt at T > 0: faster-whisper's sampling branch."""
    return dataclasses.replace(cfg, beam_size=1, temperature=T, best_of=best_of, seed=seed)


def _same(got, want, what):
    assert got.tokens == want.tokens, what
    assert got.sum_logprob == want.sum_logprob, what
    assert got.no_speech_prob == want.no_speech_prob, what
    assert got.language == want.language, what
    if want.cum_logprobs is not None:
        np.testing.assert_array_equal(got.cum_logprobs, want.cum_logprobs, err_msg=str(what))
        if want.language_probs is not None:
            np.testing.assert_array_equal(got.language_probs, want.language_probs, err_msg=str(what))
    else:
        assert got.cum_logprobs is None


def _check_t0(ref, cfg, w, got):
    _same(got, _alone(ref, w, cfg), (w["tag"], "temperature 0"))


def _check_retry(ref, cfg, w, got, T, best_of, seed, language):
    """`got` against the batch decode of the window alone at (T, best_of, seed), its language the
    one attempt 0 reported."""
    wl = dict(w, language_token=language if language >= 0 else None)
    _same(got, _alone(ref, wl, _retry_cfg(cfg, T, best_of, seed)), (w["tag"], T, seed))


def _step_until(eng, want_tags, limit=400):
    """Steps of one chunk until every tag of `want_tags` has been returned; {tag: out}, and the
    number of windows still decoding after the last step."""
    got, active = {}, 0
    for _ in range(limit):
        done, active, _ = eng.session_step(max_chunks=1)
        for t, out in done:
            assert t not in got
            got[t] = out
        if set(want_tags) <= set(got):
            return got, active
    raise AssertionError(f"windows {sorted(set(want_tags) - set(got))} did not finish")


# (2, 5): a beam session whose slots keep more rows than the beam (three parked rows at temperature 0)
CASES = [(1, 3, {}), (5, 3, {}), (5, 5, {}), (1, 5, {}), (5, 3, dict(repetition_penalty=1.3, no_repeat_ngram_size=3)),
         (2, 5, {})]


@pytest.mark.parametrize("beam,best_of,rules", CASES, ids=["b1-n3", "b5-n3", "b5-n5", "b1-n5", "b5-n3-rules", "b2-n5"])
def test_retry_beside_decoding_slots(beam, best_of, rules):
    """Four windows (prefixes of different lengths or none, detected and fixed languages, budgets
    40 / 16 / 4 / 9) in slots 0..3.  The three short ones finish while the long one decodes; each is
    retried at T = 1.0 with its own seed in the step that returned it, a fresh window joins in the
    same step as the first retries, and the long window is asserted to be still decoding then.
    Every result, retried or not, equals its decode alone; confidences are on."""
    d = D.TINY_TEST
    eng, ref = _engines(d, 5)
    try:
        cfg = dataclasses.replace(_cfg(d, beam), confidences=True, **rules)
        wins = [_window(d, 0, 200, 40, lang="detect", prefix=True), _window(d, 1, 200, 16, prefix=True),
                _window(d, 2, 200, 4), _window(d, 5, 200, 9, lang="detect")]
        fresh = _window(d, 4, 200, 6, prefix=True)
        by_tag = {w["tag"]: w for w in wins + [fresh]}
        long_tag = wins[0]["tag"]
        first, retried, seeds = {}, {}, {}
        eng.session_begin(cfg, hold=True, retries=best_of)
        try:
            eng.session_add(wins)
            added = False
            for _ in range(400):
                done, active, queued = eng.session_step(max_chunks=1)
                arm, release = [], []
                for t, out in done:
                    if t in first:                      # a retried window's second return
                        retried[t] = out
                        release.append(t)
                        continue
                    first[t] = out
                    if t in (long_tag, fresh["tag"]):
                        release.append(t)
                    else:
                        seeds[t] = 1000 + 17 * t
                        arm.append((t, 1.0, seeds[t], out.language))
                if arm:
                    assert long_tag not in first and active >= 1, "the long window still decodes beside the retries"
                    eng.session_retry(arm)
                    if not added:
                        eng.session_add([fresh])
                        added = True
                eng.session_release(release)
                if len(first) == 5 and len(retried) == 3:
                    break
            else:
                raise AssertionError("the session did not drain")
        finally:
            eng.session_end()
        assert sorted(retried) == sorted(w["tag"] for w in wins[1:])
        for t, w in by_tag.items():
            _check_t0(ref, cfg, w, first[t])
        for t, out in retried.items():
            _check_retry(ref, cfg, by_tag[t], out, 1.0, best_of, seeds[t], first[t].language)
    finally:
        eng.close()
        ref.close()


def test_twice_then_reuse():
    """The same held window retried at 0.6 and again at 1.0, each result exact; then released, and
    a new temperature-0 window admitted into that slot equals its decode alone (a row temperature
    that was not reset would sample it)."""
    d = D.TINY_TEST
    eng, ref = _engines(d, 2)
    try:
        cfg = dataclasses.replace(_cfg(d, 5), confidences=True)
        a, b, c = _window(d, 0, 600, 30, lang="detect"), _window(d, 1, 600, 5, prefix=True), _window(d, 2, 600, 7)
        eng.session_begin(cfg, hold=True, retries=3)
        try:
            eng.session_add([a, b])
            got, _ = _step_until(eng, [b["tag"]])
            out0 = got[b["tag"]]
            eng.session_retry([(b["tag"], 0.6, 11, out0.language)])
            got1, _ = _step_until(eng, [b["tag"]])
            eng.session_retry([(b["tag"], 1.0, 12, out0.language)])
            got2, _ = _step_until(eng, [b["tag"]])
            eng.session_release([b["tag"]])
            eng.session_add([c])
            rest = {**got, **got1, **got2}
            rest.pop(b["tag"])
            more, _ = _step_until(eng, {a["tag"], c["tag"]} - set(rest))
            rest.update(more)
        finally:
            eng.session_end()
        _check_t0(ref, cfg, b, out0)
        _check_retry(ref, cfg, b, got1[b["tag"]], 0.6, 3, 11, out0.language)
        _check_retry(ref, cfg, b, got2[b["tag"]], 1.0, 3, 12, out0.language)
        _check_t0(ref, cfg, a, rest[a["tag"]])
        _check_t0(ref, cfg, c, rest[c["tag"]])
    finally:
        eng.close()
        ref.close()


def test_seeds_matter():
    """At T = 1.0 another seed gives other ids for the same window, and two windows of different
    audio retried with the same seed differ; all three results are exact.  These weights are peaked
    (two or three candidates per step), so most seeds draw the greedy text: seeds 3 and 2 are a
    pair whose draws the batch path separates for the first window (3 starts [50379, 46892, ..],
    2 the greedy [50372, 12688, ..]), while the second window draws the greedy text with seed 3."""
    d = D.TINY_TEST
    eng, ref = _engines(d, 2)
    try:
        cfg = _cfg(d, 1)
        a, b = _window(d, 1, 700, 12), _window(d, 2, 700, 12)
        eng.session_begin(cfg, hold=True, retries=2)
        try:
            eng.session_add([a, b])
            t0, _ = _step_until(eng, [a["tag"], b["tag"]])
            eng.session_retry([(w["tag"], 1.0, 3, t0[w["tag"]].language) for w in (a, b)])
            s3, _ = _step_until(eng, [a["tag"], b["tag"]])
            eng.session_retry([(a["tag"], 1.0, 2, t0[a["tag"]].language)])
            s2, _ = _step_until(eng, [a["tag"]])
        finally:
            eng.session_end()
        assert s3[a["tag"]].tokens != s2[a["tag"]].tokens
        assert s3[a["tag"]].tokens != s3[b["tag"]].tokens
        for w in (a, b):
            _check_retry(ref, cfg, w, s3[w["tag"]], 1.0, 2, 3, t0[w["tag"]].language)
        _check_retry(ref, cfg, a, s2[a["tag"]], 1.0, 2, 2, t0[a["tag"]].language)
    finally:
        eng.close()
        ref.close()


def _refused(call, rc):
    with pytest.raises(OswError) as e:
        call()
    assert e.value.rc == rc, e.value


def test_refusals_leave_the_session_intact():
    """Every refusal of osw_session_retries / osw_session_retry, each followed by the next; after
    all of them a retry of the held window and the co-resident window are still exact."""
    d = D.TINY_TEST
    eng, ref = _engines(d, 2)
    try:
        cfg = _cfg(d, 5)
        a, b, q = _window(d, 0, 800, 36, prefix=True), _window(d, 2, 800, 4), _window(d, 1, 800, 5)
        # a session without retries, and one without hold
        eng.session_begin(cfg, hold=True)
        try:
            eng.session_add([b])
            got, _ = _step_until(eng, [b["tag"]])
            _refused(lambda: eng.session_retry([(b["tag"], 1.0, 1, got[b["tag"]].language)]), OSW_ESTATE)
            _refused(lambda: eng.session_retries(3), OSW_ESTATE)     # after the first add
        finally:
            eng.session_end()
        eng.session_begin(cfg)
        try:
            _refused(lambda: eng.session_retries(3), OSW_ESTATE)     # not a hold session
        finally:
            eng.session_end()
        _refused(lambda: eng.session_retries(3), OSW_ESTATE)         # no session
        eng.session_begin(cfg, hold=True)
        try:
            for n in (0, 6, -1):
                _refused(lambda: eng.session_retries(n), OSW_EINVAL)
            eng.session_retries(3)
            eng.session_add([a, b, q])                               # q waits for a slot
            got, active = _step_until(eng, [b["tag"]])
            assert active == 1
            lang = got[b["tag"]].language
            for bad in ([(4242, 1.0, 1, lang)],                      # unknown
                        [(a["tag"], 1.0, 1, lang)],                  # decoding
                        [(q["tag"], 1.0, 1, lang)],                  # queued
                        [(b["tag"], 1.0, 1, lang), (b["tag"], 1.0, 2, lang)],   # twice
                        [(b["tag"], 0.0, 1, lang)], [(b["tag"], -0.5, 1, lang)], [(b["tag"], float("nan"), 1, lang)],
                        [(b["tag"], float("inf"), 1, lang)]):
                _refused(lambda: eng.session_retry(bad), OSW_EINVAL)
            eng.session_retry([(b["tag"], 1.0, 9, lang)])
            again, _ = _step_until(eng, [b["tag"]])
            eng.session_release([b["tag"]])
            rest = {t: o for t, o in {**got, **again}.items() if t != b["tag"]}
            rest.update(_step_until(eng, {a["tag"], q["tag"]} - set(rest))[0])
        finally:
            eng.session_end()
        _check_t0(ref, cfg, b, got[b["tag"]])
        _check_retry(ref, cfg, b, again[b["tag"]], 1.0, 3, 9, lang)
        _check_t0(ref, cfg, a, rest[a["tag"]])
        _check_t0(ref, cfg, q, rest[q["tag"]])
    finally:
        eng.close()
        ref.close()


@pytest.mark.parametrize("which", ["tiny-en", "chunk5"])
def test_english_only_and_short_windows(which):
    """An English-only model with timestamps (the first sampled step is also the no-speech step,
    select.h sot_sample_step, here while sampling) and 5 s encoder windows: one retry each beside
    a decoding window, beam 5, exact."""
    d = D.TINY_EN_TEST if which == "tiny-en" else D.TINY_TEST.with_chunk_length(5)
    eng, ref = _engines(d, 2, seed=77)
    try:
        cfg = dataclasses.replace(_cfg(d, 5), confidences=True)
        a, b = _window(d, 0, 500, 24, prefix=True), _window(d, 1, 500, 5)
        eng.session_begin(cfg, hold=True, retries=3)
        try:
            eng.session_add([a, b])
            got, active = _step_until(eng, [b["tag"]])
            assert active == 1
            eng.session_retry([(b["tag"], 1.0, 31, None if got[b["tag"]].language < 0 else got[b["tag"]].language)])
            again, _ = _step_until(eng, [b["tag"]])
            eng.session_release([b["tag"]])
            rest = {**got, **again}
            rest.pop(b["tag"])
            if a["tag"] not in rest:
                rest.update(_step_until(eng, [a["tag"]])[0])
        finally:
            eng.session_end()
        _check_t0(ref, cfg, b, got[b["tag"]])
        _check_retry(ref, cfg, b, again[b["tag"]], 1.0, 3, 31, got[b["tag"]].language)
        _check_t0(ref, cfg, a, rest[a["tag"]])
    finally:
        eng.close()
        ref.close()


@pytest.mark.parametrize("knob,words", [("1", False), ("0", False), ("1", True)], ids=["lanes", "knob-off", "lanes-words"])
def test_backend_ladder_through_the_session_lanes(monkeypatch, tmp_path, knob, words):
    """Three clips (one of 47 s: two or more windows) as concurrent requests with the ladder
    (0.0, 0.4, 1.0), best_of 3 and length control through HipWhisperBackend's continuous lanes.  The
    log_prob_threshold sits between the two lowest temperature-0 avg_logprobs of a ladder-free run,
    so at least one window retries and at least one does not.  Each clip's ClipResult equals
    ``transcribe_clips(engine, [clip], opts)`` alone (with ``words``: the words too), and, without
    word timing, tests/fallback_ref.py's ``transcribe_clip`` driven by direct ``engine.decode`` calls
    with the documented seeds.  A recorder shows which path ran: the lane's ``session_retry`` and no
    batched ``decode`` (knob 1, the default), or the batched seek loop (STT_HIP_FALLBACK_SESSIONS=0)."""
    import fallback_ref as fr
    import tokfix
    from open_speech_amd import model_store, synth
    from open_speech_amd.backend import HipWhisperBackend
    from open_speech_amd.engine import DecodeConfig, WhisperEngine
    from open_speech_amd.segments import FRAME_SEC, TranscribeOptions, transcribe_clips

    d = D.MICRO_TEST
    mid = tokfix.make_hf_model_dir(str(tmp_path / "micro_hf"), d)
    for k, v in (("STT_HIP_BEAM_SIZE", "5"), ("STT_HIP_MAX_BATCH", "2"), ("STT_HIP_GPUS", "0"), ("STT_HIP_LANES", "1"),
                 ("STT_HIP_FALLBACK_SESSIONS", knob)):
        monkeypatch.setenv(k, v)
    for k in ("STT_HIP_WORD_TIMESTAMPS", "STT_HIP_WORD_SESSIONS", "STT_HIP_TEMPERATURE_INCREMENT_ON_FALLBACK"):
        monkeypatch.delenv(k, raising=False)
    clips = [synth.chirp_clip(61, 12.5), synth.chirp_clip(62, 47.0), synth.chirp_clip(63, 30.0)]
    tps = 1.5
    base = dict(beam_size=5, best_of=3, seed=77, tokens_per_second=tps, no_speech_threshold=None,
                compression_ratio_threshold=None, word_timestamps=words)
    src = model_store.resolve(mid, None)
    ref = WhisperEngine(src.dims, device=0, max_batch=2)
    try:
        heads = model_store.alignment_heads(src)
        if heads:
            ref.set_alignment_heads(heads)
        ref.load_weights(model_store.load_weights(src))
        b = HipWhisperBackend(length_control=tps)
        b.load_model(mid)
        try:
            m = b._models[mid]
            tok, sup = m.tokenizer, m.runner.suppress_for(TranscribeOptions(**base))
            # the ladder-free run that places the threshold (on the reference engine)
            plain = [transcribe_clips(ref, [c], TranscribeOptions(temperature=0.0, log_prob_threshold=None, **base),
                                      tok, sup)[0] for c in clips]
            avgs = sorted({s.avg_logprob for r in plain for s in r.segments})
            assert len(avgs) >= 2, avgs
            thr = (avgs[0] + avgs[1]) / 2
            opts = TranscribeOptions(temperature=(0.0, 0.4, 1.0), log_prob_threshold=thr, **base)
            calls = {"session_retry": [], "decode": 0}

            def retry_rec(self, entries, _orig=WhisperEngine.session_retry):
                calls["session_retry"].append([tuple(e) for e in entries])
                return _orig(self, entries)

            def decode_rec(self, *a, _orig=WhisperEngine.decode, **kw):
                if self is not ref:
                    calls["decode"] += 1
                return _orig(self, *a, **kw)
            monkeypatch.setattr(WhisperEngine, "session_retry", retry_rec)
            monkeypatch.setattr(WhisperEngine, "decode", decode_rec)
            futs = [m.runner.submit(c, opts) for c in clips]
            res = [f.result(timeout=120) for f in futs]
        finally:
            b.unload_model(mid)
        if knob == "1":
            assert len(calls["session_retry"]) >= 1 and calls["decode"] == 0, calls
        else:
            assert not calls["session_retry"] and calls["decode"] > 0, calls
        want = [transcribe_clips(ref, [c], opts, tok, sup)[0] for c in clips]
        temps = [s.temperature for r in want for s in r.segments]
        assert any(t > 0 for t in temps) and any(t == 0 for t in temps), temps
        for r, w in zip(res, want):
            assert r.segments == w.segments
            assert [s.words for s in r.segments] == [s.words for s in w.segments]
            assert (r.language, r.duration) == (w.language, w.duration)
            assert r == w
        if words:
            assert any(s.words for r in res for s in r.segments)
            return
        # the restatement, window by window, on direct engine.decode calls with the documented seeds
        from test_gpu_fallback import seg_tuple
        for clip, r in zip(clips, res):
            nf = ref.log_mel([clip])
            n_win = [0]

            def window_fn(seek, size):
                n = n_win[0]
                n_win[0] += 1

                def fn(k, t, prefix, language):
                    ref.encode([(0, seek, size)])
                    cfg = DecodeConfig(max_length=448, suppress_tokens=sup, max_initial_timestamp_index=50,
                                       beam_size=1 if t > 0 else opts.beam_size, temperature=t, best_of=opts.best_of,
                                       seed=fr.attempt_seed(opts.seed, n, k),
                                       token_budget=(int(np.ceil(tps * size * FRAME_SEC)) + 2,))
                    return ref.decode(1, cfg, prefix=[prefix] if prefix else None,
                                      languages=None if language is None else [language])[0]
                return fn
            tr = fr.transcribe_clip(window_fn, nf[0] - 1, opts, tok)
            assert [seg_tuple(s) for s in r.segments] == [seg_tuple(s) for s in tr.segments]
            assert r.language == tok.language_code(tr.language)
    finally:
        ref.close()
