"""Word timestamps on the decode sessions (osw_session_hold / osw_session_align / osw_session_release):
a window a step returns keeps its slot and cross-K/V, the alignment pass runs over the held slots
through a row -> slot map while the other slots go on decoding, and the slots are free afterwards.

Every comparison is exact (``assert_array_equal`` / ``==``) against the batched path on a second
engine of the same weights: the window's ``log_mel`` / ``encode`` / ``align`` on its own for
``token_frame``, ``token_prob`` and the alignment matrix, and ``_alone`` (as in
tests/test_gpu_session.py) for ids, ``sum_logprob``, ``no_speech_prob`` and the language.  The two
paths run the same kernels on the same row data, so there is no tolerance to state."""
import dataclasses

import numpy as np
import pytest

from open_speech_amd import dims as D
from open_speech_amd import synth, weights
from open_speech_amd._lib import OSW_EINVAL, OSW_ESTATE, OswError
from open_speech_amd.dims import SpecialTokens
from open_speech_amd.engine import AlignWindow, DecodeConfig, WhisperEngine
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens

pytestmark = pytest.mark.gpu


def _window(d, i, seed0, budget, lang="fixed", prefix=False):
    """Window i of tests/test_gpu_session.py::_windows' pattern (clips of 30, 12.5 and 47 s, seeks
    0 / 700 / 1500 into the 47 s ones), with the token budget and language given."""
    st = SpecialTokens.for_vocab(d.n_vocab)
    nf_max = 2 * d.n_audio_ctx
    secs = (30.0, 12.5, 47.0)[i % 3]
    pcm = synth.chirp_clip(seed0 + i, secs)
    nf = len(pcm) // 160 + 1
    seek = (0, 700, 1500)[(i // 3) % 3] if secs > 40 else 0
    size = min(nf_max, nf - 1 - seek)
    pre = [st.sot_prev] + [100 + (13 * i + 7 * j) % 300 for j in range(3 + i % 5)] if prefix else None
    language = None if (lang == "detect" or not st.multilingual) else st.first_lang + (i % 7)
    return dict(tag=1000 + i, pcm=pcm, seek=seek, segment_size=size, language_token=language, prefix=pre,
                token_budget=budget)


def _text(n, salt, eot):
    """n crafted text-token ids below <|endoftext|>."""
    return [(200 + 37 * j + 101 * salt) % (eot - 1) + 1 for j in range(n)]


def _alone(ref, w, cfg):
    """tests/test_gpu_session.py::_alone: the window decoded on its own (two rows, see there)."""
    ref.log_mel([w["pcm"]])
    ref.encode([(0, w["seek"], w["segment_size"])] * 2)
    c = dataclasses.replace(cfg, token_budget=(w["token_budget"],) * 2)
    return ref.decode(2, c, prefix=[w["prefix"]] * 2 if w["prefix"] else None, languages=[w["language_token"]] * 2)[0]


def _ref_align(ref, w, toks, language):
    """The batched path: the window's own log-mel and encoder output, then engine.align."""
    ref.log_mel([w["pcm"]])
    ref.encode([(0, w["seek"], w["segment_size"])])
    al = ref.align([AlignWindow(window=0, tokens=toks, num_frames=w["segment_size"], language=language)])[0]
    return al, ref.alignment_matrix(0)


def _engines(d, max_batch, seed=4321):
    w = weights.random_weights(d, seed=seed, emb_std=0.5)
    eng, ref = WhisperEngine(d, device=0, max_batch=max_batch), WhisperEngine(d, device=0, max_batch=2)
    eng.load_weights(w)
    ref.load_weights(w)
    return eng, ref


def _cfg(d, beam=1, max_length=64):
    return DecodeConfig(suppress_tokens=get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1]), max_length=max_length,
                        beam_size=beam)


def _aw(w, toks, out):
    return AlignWindow(window=-7, tokens=toks, num_frames=w["segment_size"], language=out.language)  # (window: ignored)


def _check_decoded(ref, cfg, w, got):
    r = _alone(ref, w, cfg)
    assert got.tokens == r.tokens, w["tag"]
    assert got.sum_logprob == r.sum_logprob, w["tag"]
    assert got.no_speech_prob == r.no_speech_prob, w["tag"]
    assert got.language == r.language, w["tag"]


def _check_aligned(ref, w, toks, out, al, M):
    ral, rM = _ref_align(ref, w, toks, out.language)
    assert len(al.token_prob) == len(toks) and len(al.token_frame) == len(toks) + 1
    np.testing.assert_array_equal(al.token_frame, ral.token_frame)
    np.testing.assert_array_equal(al.token_prob, ral.token_prob)
    np.testing.assert_array_equal(M, rM)


def _drive(eng, cfg, wins, text, more=None):
    """All of `wins` through a hold session; whatever a step returns is aligned in one call at
    once, window tag with text[tag].  Returns {tag: (out, alignment, M)} and the log of align
    calls [(tags, windows still decoding)].  more: {number of align calls so far: windows to add}."""
    by_tag = {w["tag"]: w for w in wins}
    got, calls = {}, []
    eng.session_begin(cfg, hold=True)
    try:
        eng.session_add(wins)
        for _ in range(2000):
            done, active, queued = eng.session_step(max_chunks=1)
            if done:
                als = eng.session_align([(t, _aw(by_tag[t], text[t], out)) for t, out in done])
                for i, ((t, out), al) in enumerate(zip(done, als)):
                    assert t not in got
                    got[t] = (out, al, eng.alignment_matrix(i))
                calls.append(([t for t, _ in done], active))
                if more and len(calls) in more:
                    add = more.pop(len(calls))
                    by_tag.update({w["tag"]: w for w in add})
                    eng.session_add(add)
                    continue
            if active == 0 and queued == 0 and not more:
                break
        else:
            raise AssertionError("the session did not drain")
    finally:
        eng.session_end()
    assert sorted(got) == sorted(by_tag)
    return got, calls


@pytest.mark.parametrize("beam", [1, 5])
def test_held_slots_align_exactly_while_slot_0_decodes(beam):
    """Four windows in slots 0..3 (budgets 40, 16, 4, 9): the windows of slots 2, 3 and 1 finish in
    different chunks while slot 0 still decodes, and each is aligned alone, so decoder row 0 of the
    pass reads the cross-K/V of slot 2, 3 or 1: a window map that is not the identity, beam 5
    with five decoder rows per slot.  Slots 2 and 3 force 17 tokens each (the same shape on
    another slot: the second call replays the first's graph with other data), slot 1 forces 40,
    slot 0 five.  The long window decodes across all of those calls and still equals its decode
    alone, as does every other window; every alignment equals the batched path's."""
    d = D.TINY_TEST
    eot = SpecialTokens.for_vocab(d.n_vocab).eot
    eng, ref = _engines(d, 4)
    try:
        cfg = _cfg(d, beam)
        wins = [_window(d, 0, 200, 40, lang="detect"), _window(d, 1, 200, 16, prefix=True), _window(d, 2, 200, 4),
                _window(d, 5, 200, 9, lang="detect")]
        text = {wins[0]["tag"]: _text(5, 0, eot), wins[1]["tag"]: _text(40, 1, eot), wins[2]["tag"]: _text(17, 2, eot),
                wins[3]["tag"]: _text(17, 3, eot)}
        got, calls = _drive(eng, cfg, wins, text)
        order = [t for tags, _ in calls for t in tags]
        assert order[-1] == wins[0]["tag"], order           # the long window finishes last ...
        beside = [tags for tags, active in calls if active >= 1 and wins[0]["tag"] not in tags]
        assert len(beside) >= 2, calls                      # ... after two or more align calls beside it
        assert all(len(tags) == 1 for tags in beside), calls  # each of one window: row 0 -> slot 1, 2 or 3
        for w in wins:
            out, al, M = got[w["tag"]]
            _check_decoded(ref, cfg, w, out)
            _check_aligned(ref, w, text[w["tag"]], out, al, M)
        assert len({len(o.tokens) for o, _, _ in got.values()}) >= 3
    finally:
        eng.close()
        ref.close()


def test_several_held_windows_in_one_call_one_without_text():
    """Three windows that finish in the same chunk (equal prompts and budgets) are aligned in one
    call with 17, 0 and 40 text tokens, then a second call aligns the fourth with a single token
    (another score stride).  The window without text comes back empty with an empty matrix, its slot
    is free again (a fifth window is admitted and decodes as alone), its neighbours are exact."""
    d = D.TINY_TEST
    eot = SpecialTokens.for_vocab(d.n_vocab).eot
    eng, ref = _engines(d, 4)
    try:
        cfg = _cfg(d)
        wins = [_window(d, 0, 300, 6), _window(d, 1, 300, 6), _window(d, 2, 300, 6), _window(d, 3, 300, 21)]
        extra = _window(d, 4, 300, 5)
        text = {wins[0]["tag"]: _text(17, 4, eot), wins[1]["tag"]: [], wins[2]["tag"]: _text(40, 5, eot),
                wins[3]["tag"]: _text(1, 6, eot), extra["tag"]: _text(5, 7, eot)}
        got, calls = _drive(eng, cfg, wins, text, more={1: [extra]})
        assert sorted(calls[0][0]) == [w["tag"] for w in wins[:3]] and calls[0][1] == 1, calls
        out, al, M = got[wins[1]["tag"]]
        assert al.token_frame.size == 0 and al.token_prob.size == 0 and M.size == 0
        for w in wins + [extra]:
            out, al, M = got[w["tag"]]
            _check_decoded(ref, cfg, w, out)
            if text[w["tag"]]:
                _check_aligned(ref, w, text[w["tag"]], out, al, M)
    finally:
        eng.close()
        ref.close()


def test_held_slots_are_not_reused():
    """max_batch 2, both slots held, a third window queued: the step returns at once with nothing
    done and the window still queued (admission is where a window's encoder runs, so it has not
    run), also when asked to admit only.  Aligning one held window frees its slot: the third is
    admitted there and decodes as alone, and the alignment of the other held window, taken after
    that admission's encoder ran, is still exact."""
    d = D.TINY_TEST
    eot = SpecialTokens.for_vocab(d.n_vocab).eot
    eng, ref = _engines(d, 2)
    try:
        cfg = _cfg(d)
        a, b, c = _window(d, 0, 400, 5), _window(d, 2, 400, 5), _window(d, 1, 400, 7)
        text = {a["tag"]: _text(17, 8, eot), b["tag"]: _text(5, 9, eot)}
        eng.session_begin(cfg, hold=True)
        try:
            eng.session_add([a, b, c])
            outs = {}
            for _ in range(50):
                done, active, queued = eng.session_step(max_chunks=1)
                outs.update(done)
                assert queued == 1
                if len(outs) == 2:
                    break
            assert sorted(outs) == [a["tag"], b["tag"]] and active == 0
            for chunks in (1, 0, 3):
                assert eng.session_step(max_chunks=chunks) == ([], 0, 1)
            al_b = eng.session_align([(b["tag"], _aw(b, text[b["tag"]], outs[b["tag"]]))])[0]
            M_b = eng.alignment_matrix(0)
            done, active, queued = eng.session_step(max_chunks=0)     # the third window's admission
            assert (done, active, queued) == ([], 1, 0)
            al_a = eng.session_align([(a["tag"], _aw(a, text[a["tag"]], outs[a["tag"]]))])[0]
            M_a = eng.alignment_matrix(0)
            for _ in range(50):
                done, active, queued = eng.session_step(max_chunks=1)
                if done:
                    break
            assert [t for t, _ in done] == [c["tag"]] and (active, queued) == (0, 0)
            out_c = done[0][1]
            eng.session_release([c["tag"]])
        finally:
            eng.session_end()
        _check_aligned(ref, b, text[b["tag"]], outs[b["tag"]], al_b, M_b)
        _check_aligned(ref, a, text[a["tag"]], outs[a["tag"]], al_a, M_a)
        for w, out in ((a, outs[a["tag"]]), (b, outs[b["tag"]]), (c, out_c)):
            _check_decoded(ref, cfg, w, out)
    finally:
        eng.close()
        ref.close()


@pytest.mark.parametrize("which", ["tiny-en", "chunk5"])
def test_english_only_and_short_windows(which):
    """An English-only model (forced sequence [sot, no_timestamps, ...]) and 5 s encoder windows
    (250 keys): three windows through two slots, one held while the other decodes."""
    d = D.TINY_EN_TEST if which == "tiny-en" else D.TINY_TEST.with_chunk_length(5)
    eot = SpecialTokens.for_vocab(d.n_vocab).eot
    eng, ref = _engines(d, 2, seed=77)
    try:
        cfg = _cfg(d)
        wins = [_window(d, 0, 500, 19), _window(d, 1, 500, 4), _window(d, 2, 500, 8)]
        text = {wins[0]["tag"]: _text(17, 10, eot), wins[1]["tag"]: _text(5, 11, eot), wins[2]["tag"]: _text(40, 12, eot)}
        got, calls = _drive(eng, cfg, wins, text)
        assert any(active >= 1 for _, active in calls), calls
        for w in wins:
            out, al, M = got[w["tag"]]
            _check_decoded(ref, cfg, w, out)
            _check_aligned(ref, w, text[w["tag"]], out, al, M)
            assert M.shape == (len(text[w["tag"]]) + 1, min(d.n_audio_ctx, w["segment_size"] // 2))
    finally:
        eng.close()
        ref.close()


def test_errors_leave_the_session_intact():
    d = D.TINY_TEST
    eot = SpecialTokens.for_vocab(d.n_vocab).eot
    eng, ref = _engines(d, 2)
    try:
        cfg = _cfg(d)
        a, b = _window(d, 0, 600, 4), _window(d, 1, 600, 14)
        text = _text(5, 13, eot)
        with pytest.raises(OswError) as e:          # no session
            eng.session_hold(True)
        assert e.value.rc == OSW_ESTATE
        eng.session_begin(cfg, hold=True)
        try:
            eng.session_add([a, b])
            with pytest.raises(OswError) as e:      # hold after an add
                eng.session_hold(True)
            assert e.value.rc == OSW_ESTATE
            with pytest.raises(OswError) as e:      # a tag that is queued, decoding or held is taken
                eng.session_add([dict(a)])
            assert e.value.rc == OSW_EINVAL
            outs = {}
            for _ in range(50):
                done, active, queued = eng.session_step(max_chunks=1)
                outs.update(done)
                if done:
                    break
            assert list(outs) == [a["tag"]] and active == 1
            good = (a["tag"], _aw(a, text, outs[a["tag"]]))
            for bad in ([(b["tag"], good[1])],                     # still decoding
                        [(424242, good[1])],                       # unknown
                        [good, good],                              # twice
                        [good, (b["tag"], good[1])],               # one held, one not: nothing is freed
                        [(a["tag"], _aw(a, [eot], outs[a["tag"]]))],                       # a token that is not text
                        [(a["tag"], _aw(a, [1] * (d.n_text_ctx - 4), outs[a["tag"]]))]):   # n + 5 > n_text_ctx
                with pytest.raises(OswError) as e:
                    eng.session_align(bad)
                assert e.value.rc == OSW_EINVAL, bad
            for bad in ([b["tag"]], [424242], [a["tag"], a["tag"]]):
                with pytest.raises(OswError) as e:
                    eng.session_release(bad)
                assert e.value.rc == OSW_EINVAL, bad
            with pytest.raises(OswError) as e:      # the batched entry stays shut while a session is open
                eng.align([AlignWindow(window=0, tokens=text, num_frames=a["segment_size"], language=outs[a["tag"]].language)])
            assert e.value.rc == OSW_EINVAL
            # the session goes on: the held window aligns exactly, the other finishes exactly
            al = eng.session_align([good])[0]
            M = eng.alignment_matrix(0)
            with pytest.raises(OswError):           # aligned once: no longer held
                eng.session_release([a["tag"]])
            for _ in range(50):
                done, active, queued = eng.session_step(max_chunks=1)
                outs.update(done)
                if done:
                    break
            assert sorted(outs) == [a["tag"], b["tag"]]
        finally:
            eng.session_end()                       # with b still held: clean
        _check_aligned(ref, a, text, outs[a["tag"]], al, M)
        _check_decoded(ref, cfg, a, outs[a["tag"]])
        _check_decoded(ref, cfg, b, outs[b["tag"]])
        # a session without hold hands its slots back at once, as before: three windows through
        # two slots with no align or release, and nothing is held
        wins = [_window(d, i, 700, 4 + 3 * i) for i in range(3)]
        eng.session_begin(cfg)
        try:
            eng.session_add(wins)
            outs = {}
            for _ in range(200):
                done, active, queued = eng.session_step(max_chunks=1)
                outs.update(done)
                for t, _ in done:
                    with pytest.raises(OswError):
                        eng.session_release([t])
                if active == 0 and queued == 0:
                    break
            assert sorted(outs) == [w["tag"] for w in wins]
        finally:
            eng.session_end()
        for w in wins:
            _check_decoded(ref, cfg, w, outs[w["tag"]])
        # and the context serves the batched path again
        _check_aligned(eng, a, text, outs[wins[0]["tag"]], *_ref_align(ref, a, text, outs[wins[0]["tag"]].language))
    finally:
        eng.close()
        ref.close()


@pytest.mark.parametrize("knob", ["1", "0"])
def test_backend_word_timestamps_through_the_session_lanes(monkeypatch, tmp_path, knob):
    """Three clips (one of 47 s: two or more windows) with word_timestamps through
    HipWhisperBackend's continuous lanes, length control on: the ClipResults equal
    transcribe_clips' on an engine of the same weights, segments and words compared with ==.
    A counter on session_align shows which path ran: the sessions (knob 1, the default) or the
    batched seek loop (STT_HIP_WORD_SESSIONS=0)."""
    import tokfix
    from open_speech_amd import model_store, segments
    from open_speech_amd.backend import HipWhisperBackend
    from open_speech_amd.segments import TranscribeOptions, transcribe_clips

    d = D.MICRO_TEST
    mid = tokfix.make_hf_model_dir(str(tmp_path / "micro_hf"), d)
    for k, v in (("STT_HIP_BEAM_SIZE", "5"), ("STT_HIP_MAX_BATCH", "2"), ("STT_HIP_GPUS", "0"), ("STT_HIP_LANES", "1"),
                 ("STT_HIP_WORD_SESSIONS", knob)):
        monkeypatch.setenv(k, v)
    monkeypatch.delenv("STT_HIP_WORD_TIMESTAMPS", raising=False)
    calls = {"session_align": 0, "align": 0}
    for name in calls:
        def counted(self, windows, _orig=getattr(WhisperEngine, name), _name=name):
            calls[_name] += 1
            return _orig(self, windows)
        monkeypatch.setattr(WhisperEngine, name, counted)
    clips = [synth.chirp_clip(61, 12.5), synth.chirp_clip(62, 47.0), synth.chirp_clip(63, 30.0)]
    planned = []    # content frames of the clip of every window either path plans

    def counting_plan(s, *a, _orig=segments._plan, **kw):
        planned.append(s.content_frames)
        return _orig(s, *a, **kw)
    monkeypatch.setattr(segments, "_plan", counting_plan)
    b = HipWhisperBackend(length_control=1.5)
    b.load_model(mid)
    try:
        m = b._models[mid]
        opts = TranscribeOptions(beam_size=5, tokens_per_second=1.5, word_timestamps=True)
        futs = [m.runner.submit(c, opts) for c in clips]
        res = [f.result(timeout=120) for f in futs]
        tok, sup = m.tokenizer, m.runner.suppress_for(opts)
    finally:
        b.unload_model(mid)
    assert planned.count(4700) >= 2, planned                 # the 47 s clip took two or more windows
    assert (calls["session_align"] > 0) == (knob == "1") and (calls["align"] > 0) == (knob == "0"), calls
    src = model_store.resolve(mid, None)
    ref = WhisperEngine(src.dims, device=0, max_batch=2)
    try:
        heads = model_store.alignment_heads(src)
        if heads:
            ref.set_alignment_heads(heads)
        ref.load_weights(model_store.load_weights(src))
        want = transcribe_clips(ref, clips, opts, tok, sup)
    finally:
        ref.close()
    assert any(s.words for r in res for s in r.segments)
    for r, w in zip(res, want):
        assert r.segments == w.segments
        assert [s.words for s in r.segments] == [s.words for s in w.segments]
        assert [s.seek for s in r.segments] == [s.seek for s in w.segments]
        assert (r.language, r.duration) == (w.language, w.duration)
