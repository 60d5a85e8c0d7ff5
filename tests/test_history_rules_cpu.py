"""repetition_penalty / no_repeat_ngram_size without a GPU: the numpy restatement the GPU
tests compare the kernel with is pinned to transformers' logits processors (0 ulp), and the
two options travel from the backend's keyword arguments / env knobs to the engine's
``DecodeConfig`` on the batched path and on the session path."""
import numpy as np
import pytest

import history_rules_ref as hr
from open_speech_amd.segments import TranscribeOptions, session_config, session_supported
from test_backend_cpu import MID, FakeEngine, wav

from open_speech_amd.backend import HipWhisperBackend


def _logits(rng, V):
    x = (rng.standard_normal(V) * 3).astype(np.float32)
    x[rng.integers(0, V, 6)] = 0.0
    x[1] = -0.0
    x[2] = -np.inf
    x[3] = np.float32(1e-41)   # subnormal
    x[4] = np.float32(-1e-41)
    return x


def _history(rng, V, n):
    # a few distinct ids, so duplicates and repeated n-grams occur (ids 1..4: the special values)
    pool = np.concatenate([np.arange(1, 5), rng.integers(0, V, 4)])
    return [int(t) for t in rng.choice(pool, n)] if n else []


def test_penalty_matches_transformers():
    torch = pytest.importorskip("torch")
    tf = pytest.importorskip("transformers")
    rng = np.random.default_rng(0)
    V = 97
    for p in (1.3, 2.0, 10.0, 0.5):
        for n in (0, 1, 2, 5, 40):
            x, h = _logits(rng, V), _history(rng, V, n)
            ref = tf.RepetitionPenaltyLogitsProcessor(penalty=p)(
                torch.tensor([h], dtype=torch.long).reshape(1, n), torch.from_numpy(x.copy())[None])[0].numpy()
            got = hr.history_rules(x, h, repetition_penalty=p)
            assert got.dtype == np.float32
            np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32), err_msg=f"p={p} n={n}")


@pytest.mark.parametrize("m", [1, 2, 3, 5])
def test_ngram_bans_match_transformers(m):
    torch = pytest.importorskip("torch")
    tf = pytest.importorskip("transformers")
    rng = np.random.default_rng(m)
    V = 97
    banned = 0
    for n in (0, m - 1, m, 40):
        for rep in range(4):
            x, h = _logits(rng, V), _history(rng, V, n)
            if rep % 2:   # periodic: the tail has occurred before whatever m is
                h = (h[:2 + rep // 2] * n)[:n]
            ids = torch.tensor([h], dtype=torch.long).reshape(1, n)
            ref = tf.NoRepeatNGramLogitsProcessor(m)(ids, torch.from_numpy(x.copy())[None])[0].numpy()
            got = hr.history_rules(x, h, no_repeat_ngram_size=m)
            np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32), err_msg=f"m={m} n={n}")
            banned += int(np.isneginf(got).sum() - np.isneginf(x).sum())
            # both rules: the penalty first, then the bans on the penalised row
            pen = tf.RepetitionPenaltyLogitsProcessor(penalty=1.3)(ids, torch.from_numpy(x.copy())[None])
            ref2 = tf.NoRepeatNGramLogitsProcessor(m)(ids, pen)[0].numpy()
            got2 = hr.history_rules(x, h, repetition_penalty=1.3, no_repeat_ngram_size=m)
            np.testing.assert_array_equal(got2.view(np.uint32), ref2.view(np.uint32), err_msg=f"both m={m} n={n}")
    assert banned > 0   # (the histories do repeat n-grams: the comparison is not vacuous)


def test_restatement_is_off_by_default_and_m1_bans_history():
    x = np.arange(-4, 4, dtype=np.float32)
    np.testing.assert_array_equal(hr.history_rules(x, [1, 2, 1]), x)
    y = hr.history_rules(x, [1, 6, 1], no_repeat_ngram_size=1)
    assert np.isneginf(y[[1, 6]]).all() and np.array_equal(np.delete(y, [1, 6]), np.delete(x, [1, 6]))
    assert hr.has_repeated_ngram([1, 2, 3, 1, 2], 2) and not hr.has_repeated_ngram([1, 2, 3, 1, 2], 3)


def test_options_key_and_validation():
    base = TranscribeOptions()
    assert base.repetition_penalty == 1.0 and base.no_repeat_ngram_size == 0
    assert TranscribeOptions().key() == base.key()
    assert TranscribeOptions(repetition_penalty=1.3).key() != base.key()
    assert TranscribeOptions(no_repeat_ngram_size=3).key() != base.key()
    assert TranscribeOptions(no_repeat_ngram_size=3).key() != TranscribeOptions(no_repeat_ngram_size=2).key()
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            TranscribeOptions(repetition_penalty=bad)
    with pytest.raises(ValueError):
        TranscribeOptions(no_repeat_ngram_size=-1)
    # requests with rules stay on the continuous path, and the session carries them
    o = TranscribeOptions(repetition_penalty=1.3, no_repeat_ngram_size=3)
    assert session_supported(o) == session_supported(base)
    cfg = session_config(o, ())
    assert (cfg.repetition_penalty, cfg.no_repeat_ngram_size) == (1.3, 3)
    cfg0 = session_config(base, ())
    assert (cfg0.repetition_penalty, cfg0.no_repeat_ngram_size) == (1.0, 0)


def test_decode_opts_binding_matches_header():
    """The two fields are appended after token_budget (x86-64 SysV layout of include/osw.h),
    zero-initialised, i.e. off."""
    import ctypes

    from open_speech_amd import _lib
    o = _lib.osw_decode_opts
    assert [n for n, _ in o._fields_][-3:] == ["token_budget", "repetition_penalty", "no_repeat_ngram_size"]
    assert (o.token_budget.offset, o.repetition_penalty.offset, o.no_repeat_ngram_size.offset) == (128, 136, 140)
    assert ctypes.sizeof(o) == 144
    assert (o().repetition_penalty, o().no_repeat_ngram_size) == (0.0, 0)


class RecordingEngine(FakeEngine):
    """The scripted stand-in engine, keeping every DecodeConfig it is given."""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.decode_cfgs, self.session_cfgs = [], []

    def decode(self, n, cfg, prefix=None, dump_steps=0, languages=None):
        self.decode_cfgs.append(cfg)
        return super().decode(n, cfg, prefix=prefix, dump_steps=dump_steps, languages=languages)

    def session_begin(self, cfg):
        self.session_cfgs.append(cfg)
        return super().session_begin(cfg)


def _run(monkeypatch, continuous, env=None, **kw):
    monkeypatch.setenv("STT_HIP_CONTINUOUS", "1" if continuous else "0")
    for k in ("STT_HIP_REPETITION_PENALTY", "STT_HIP_NO_REPEAT_NGRAM_SIZE"):
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    holder = []

    def factory(dims, gpu, mb):
        e = RecordingEngine(dims, gpu, mb)
        holder.append(e)
        return e
    b = HipWhisperBackend(engine_factory=factory)
    try:
        r = b.transcribe(wav(30.0), MID, response_format="verbose_json", **kw)
        assert r["segments"]
    finally:
        b.unload_model(MID)
    cfgs = [c for e in holder for c in (e.session_cfgs if continuous else e.decode_cfgs)]
    other = [c for e in holder for c in (e.decode_cfgs if continuous else e.session_cfgs)]
    assert cfgs and not other
    return {(c.repetition_penalty, c.no_repeat_ngram_size) for c in cfgs}


ENV = {"STT_HIP_REPETITION_PENALTY": "1.7", "STT_HIP_NO_REPEAT_NGRAM_SIZE": "4"}


@pytest.mark.parametrize("continuous", [False, True], ids=["batched", "session"])
def test_options_reach_the_engine(monkeypatch, continuous):
    assert _run(monkeypatch, continuous) == {(1.0, 0)}
    assert _run(monkeypatch, continuous, repetition_penalty=1.3, no_repeat_ngram_size=3) == {(1.3, 3)}
    assert _run(monkeypatch, continuous, env=ENV) == {(1.7, 4)}
    # keyword arguments win over the env knobs, each on its own
    assert _run(monkeypatch, continuous, env=ENV, repetition_penalty=1.3, no_repeat_ngram_size=3) == {(1.3, 3)}
    assert _run(monkeypatch, continuous, env=ENV, no_repeat_ngram_size=2) == {(1.7, 2)}
    assert _run(monkeypatch, continuous, env=ENV, repetition_penalty=1.0, no_repeat_ngram_size=0) == {(1.0, 0)}


def test_translate_takes_the_options(monkeypatch):
    monkeypatch.setenv("STT_HIP_CONTINUOUS", "0")
    holder = []

    def factory(dims, gpu, mb):
        e = RecordingEngine(dims, gpu, mb)
        holder.append(e)
        return e
    b = HipWhisperBackend(engine_factory=factory)
    try:
        b.translate(wav(30.0), MID, repetition_penalty=2.0, no_repeat_ngram_size=5)
        with pytest.raises(ValueError):
            b.transcribe(wav(30.0), MID, repetition_penalty=0.0)
    finally:
        b.unload_model(MID)
    cfgs = [c for e in holder for c in e.decode_cfgs]
    assert cfgs and all((c.task, c.repetition_penalty, c.no_repeat_ngram_size) == ("translate", 2.0, 5) for c in cfgs)
