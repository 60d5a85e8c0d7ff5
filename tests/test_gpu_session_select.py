"""The selection kernels of a retry session alone (select_retry_kernel<BEAM>, beam_update_kernel<5, true>;
csrc/decode.hip), one step at a time on crafted logits and state through osw_debug_select_step_rows:
three window slots whose rows take different paths in ONE launch.

  beam-5 session, 5 rows per slot: slot 0 decodes by beam search, slot 1 samples with best_of 3 (two
                                   parked rows), slot 2 samples with best_of 5
  greedy session, 3 rows per slot: slot 0 decodes greedily on its first row (two parked rows), slot 1
                                   samples with best_of 2 (one parked row), slot 2 with best_of 3

Expected, exactly (``assert_array_equal`` on every word): slot 0's rows as the existing
osw_debug_select_step in session mode leaves them when it runs that slot alone; each sampling slot's
armed rows as the existing batch-mode sampling step leaves them (the same temperature and seed,
``n_prefix = plen - tail``, rows 0 .. best_of-1 of one window): state words, ``cur_tok``, ``tokens``,
the step counters, ``lp_hist``, ``lang_probs``; the parked rows untouched; the arrival and ticket
counters all zero.  A second step on the outputs stays equal.  Both sides run on the GPU, through
the same device functions, so there is no tolerance to state.

The logits are the crafted families of tests/select_cases.py: exact ties, an all-NaN row, a row whose
allowed set is timestamps only (the first sampled step, at plen - 1, where in a beam session only
the prompt hypothesis of a BEAM slot expands while every armed row of a sampling slot samples), rows
at their token budget, rows reaching max_length, the <|startoftranscript|> step with a detected
language, and a prompt step."""
import dataclasses

import numpy as np
import pytest

import select_cases as sc
import select_ref as R
from open_speech_amd.engine import DecodeConfig, WhisperEngine

pytestmark = pytest.mark.gpu

V = 51865
MAX_LEN = 32
ROW_KEYS = ("pos", "state", "prompt", "cur_tok", "tokens", "budget", "lp_hist")


@pytest.fixture(scope="module")
def eng():
    e = WhisperEngine(sc.dims(V), device=0, max_batch=16)   # selection alone: no weights needed
    yield e
    e.close()


def _cfg(beam):
    return DecodeConfig(max_length=MAX_LEN, beam_size=beam, confidences=True)


def _rows(cfg, G, n_armed, kind, prefix, lang, budget, rng):
    """One slot as G single-row session windows of the same prompt (engine layout): rows [0, n_armed)
    where `kind` says, rows [n_armed, G) parked (done, at step 0)."""
    sr = R.SelectRef(sc.dims(V), dataclasses.replace(cfg, beam_size=1), "session")
    s = sr.st
    tb = s.timestamp_begin
    st = sr.initial_state(G, langs=[lang] * G, prefixes=[prefix] * G, budgets=[budget] * G)
    plen = int(st["state"]["plen"][0])
    known = lang if lang is not None else s.first_lang + 5
    for r in range(n_armed):
        if kind == "first":
            sr.set_history(st, r, [], 0.0, known)
        elif kind in ("mid", "budget"):
            sr.set_history(st, r, [tb + 3, 1000 + r], -1.0 - 0.25 * r, known)
        elif kind == "maxlen":
            n = MAX_LEN - plen - 1
            sr.set_history(st, r, [tb + 1] + [900 + 3 * i + r for i in range(n - 1)], -2.0 - r, known)
        elif kind == "sot":
            st["pos"][r] = plen - sr.tail
            st["cur_tok"][r] = s.sot
        else:
            assert kind == "prompt" and plen - sr.tail >= 1
    st["lp_hist"][:] = -np.cumsum(rng.uniform(0.05, 0.3, st["lp_hist"].shape), 1)
    st["state"]["done"][n_armed:] = 1
    out = R.to_engine(st)
    out.pop("lang_probs")
    return out, sr


def _logits(kind, n, G, rng, sr):
    """[G][V] logits of one sampling slot: row 0 with exact ties on top, row 1 all NaN, the others
    random with the timestamp mass winning on odd rows; parked rows hold values that would win."""
    s = sr.st
    tb = s.timestamp_begin
    x = (rng.standard_normal((G, V)) * 2.0).astype(np.float32)
    x[0, [tb + 7, tb + 8, 1500, 1501]] = 9.0
    if n > 1 and kind != "sot":
        x[1, :] = np.nan
    for r in range(2, n):
        if r % 2:
            x[r, tb + 4:tb + 400] += 6.0
    if kind == "sot":
        x[:, s.first_lang + 11] = 8.0
        x[1 % n, s.first_lang + 40] = 9.0      # (each row detects for itself; row 0 writes lang_probs)
        x[:, s.no_speech] = np.linspace(-1.0, 3.0, G)
    x[n:, 1234] = 50.0
    return x


def _join(slots, key):
    return np.concatenate([s[key] for s in slots])


def _session_state(cfg, slots, G, rng):
    """The three slots' rows as one retry-session state (beam: with identity ancestry and fresh
    bookkeeping for the sampling slots, slot 0's own for the beam slot)."""
    n_langs = R.SelectRef(sc.dims(V), cfg, "session").st.n_langs
    ctx = sc.dims(V).n_text_ctx
    st = {k: _join(slots, k) for k in ROW_KEYS}
    st["lang_probs"] = rng.uniform(0.0, 1.0, (len(slots), n_langs)).astype(np.float32)
    if cfg.beam_size > 1:
        rows = len(st["state"])
        st["anc"] = np.repeat(np.arange(rows, dtype=np.int32)[:, None], ctx, 1)
        st["anc"][:G] = slots[0]["anc"]
        st["bwin"] = np.concatenate([slots[0]["bwin"], np.zeros(len(slots) - 1, slots[0]["bwin"].dtype)])
        mt = st["tokens"].shape[1]
        st["best_tok"] = np.concatenate([slots[0]["best_tok"], np.zeros((len(slots) - 1, mt), np.int32)])
        st["best_lp"] = np.concatenate([slots[0]["best_lp"], np.zeros((len(slots) - 1, ctx), np.float32)])
    return st


def _beam_slot(cfg, rng):
    """Slot 0 of the beam session: tests/select_cases.py beam_long_history's window 1 (two tokens in,
    scrambled ancestry), with a prefix, and its logits."""
    sr = R.SelectRef(sc.dims(V), cfg, "session")
    s = sr.st
    st = sr.initial_state(1, langs=[s.first_lang + 1], prefixes=[[s.sot_prev, 7, 8]], budgets=[0])
    st["state"]["lang"][:] = s.first_lang + 1
    x = sc._floor(rng, 5, V, -30.0, -25.0)
    for k in range(5):
        sr.set_history(st, k, [s.timestamp_begin + 2, 200 + k], -1.0 - 0.5 * k)
        x[k, [1000 + k, 2000 + k]] = [6.0, 5.0 - 0.2 * k]
    st["anc"][:, :int(st["pos"][0])] = rng.integers(0, 5, (5, int(st["pos"][0])))
    st["lp_hist"][:] = -np.cumsum(rng.uniform(0.05, 0.3, st["lp_hist"].shape), 1)
    out = R.to_engine(st)
    out.pop("lang_probs")
    return out, x


def _as_batch(slot, n, lang_probs_row, sr):
    """Rows [0, n) of a sampling slot as one window of a batch decode with best_of = n."""
    plen = int(slot["state"]["plen"][0])
    state = slot["state"][:n].copy()
    state["plen"] = 0
    return dict(pos=slot["pos"][:1].copy(), state=state, prompt=slot["prompt"][:n, :plen].copy(),
                cur_tok=slot["cur_tok"][:n].copy(), tokens=slot["tokens"][:n, :max(1, MAX_LEN - plen)].copy(),
                budget=slot["budget"][:n].copy(), lp_hist=slot["lp_hist"][:n].copy(),
                lang_probs=lang_probs_row[None].copy()), plen - sr.tail


def _words(a):
    """Every word compared exactly, floats by their bits."""
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype.kind in "fV" else a


def _eq(got, want, what):
    np.testing.assert_array_equal(_words(got), _words(want), err_msg=what)


def _check_sampling(out, before, want, lo, n, G, slot, what):
    """Rows [lo, lo + G) of the session step `out` (input `before`): the armed rows equal the batch
    step `want`, the parked rows are untouched."""
    a = slice(lo, lo + n)
    plen = before["state"]["plen"][lo]
    st = out["state"][a].copy()
    assert (st["plen"] == plen).all(), what
    st["plen"] = 0
    _eq(st, want["state"], what + " state")
    _eq(out["cur_tok"][a], want["cur_tok"], what + " cur_tok")
    mtb = want["tokens"].shape[1]
    _eq(out["tokens"][a, :mtb], want["tokens"], what + " tokens")
    _eq(out["tokens"][a, mtb:], before["tokens"][a, mtb:], what + " tokens past the batch row")
    assert (out["pos"][a] == want["pos"][0]).all(), (what, out["pos"][a], want["pos"])
    _eq(out["lp_hist"][a], want["lp_hist"], what + " lp_hist")
    _eq(out["lang_probs"][slot], want["lang_probs"][0], what + " lang_probs")
    p = slice(lo + n, lo + G)
    for k in ("pos", "state", "cur_tok", "tokens", "lp_hist"):
        _eq(out[k][p], before[k][p], what + " parked " + k)


def _carry(out):
    return {k: v for k, v in out.items() if k not in ("counters", "logits")}


VARIANTS = {"first-mid": ("first", "mid"), "budget-maxlen": ("budget", "maxlen"), "sot-prompt": ("sot", "prompt")}


@pytest.mark.parametrize("variant", sorted(VARIANTS))
@pytest.mark.parametrize("beam", [5, 1])
def test_retry_session_step(eng, beam, variant):
    cfg = _cfg(beam)
    G = 5 if beam == 5 else 3
    armed = (0, 3, 5) if beam == 5 else (0, 2, 3)
    kinds = VARIANTS[variant]
    rng = np.random.default_rng([V, beam, sorted(VARIANTS).index(variant)])
    s0 = R.SelectRef(sc.dims(V), cfg, "session").st
    # slot 0: the session's temperature-0 mode
    if beam > 1:
        slot0, x0 = _beam_slot(cfg, rng)
    else:
        slot0, sr0 = _rows(cfg, G, 1, "mid", [s0.sot_prev, 7, 8], s0.first_lang + 1, 0, rng)
        x0 = (rng.standard_normal((G, V)) * 2.0).astype(np.float32)
        x0[1:, 1234] = 50.0
    # slots 1, 2: sampling, with their own prefixes, languages, budgets, temperatures and seeds
    specs = [dict(prefix=[s0.sot_prev, 11, 12, 13, 14], lang=None if kinds[0] == "sot" else s0.first_lang + 3,
                  budget=2 if kinds[0] == "budget" else 0, T=1.0, seed=12345),
             dict(prefix=[s0.sot_prev, 21], lang=s0.first_lang + 9, budget=0, T=0.7, seed=2 ** 63 + 11)]
    slots, xs, srs = [slot0], [x0], [None]
    for kind, n, sp in zip(kinds, armed[1:], specs):
        rows, sr = _rows(cfg, G, n, kind, sp["prefix"], sp["lang"], sp["budget"], rng)
        slots.append(rows)
        srs.append(sr)
        xs.append(_logits(kind, n, G, rng, sr))
    st = _session_state(cfg, slots, G, rng)
    rit = np.zeros(3 * G, np.float32)
    seeds = np.zeros(3 * G, np.uint64)
    for i, (n, sp) in enumerate(zip(armed[1:], specs), start=1):
        rit[i * G:i * G + n] = np.float32(1.0) / np.float32(sp["T"])
        seeds[i * G:i * G + n] = sp["seed"]

    # the references, each slot alone through the existing entry
    n0 = beam if beam > 1 else 1
    alone = {k: slot0[k][:n0].copy() for k in ROW_KEYS}
    alone["lang_probs"] = st["lang_probs"][:1].copy()
    if beam > 1:
        alone.update({k: slot0[k].copy() for k in ("anc", "bwin", "best_tok", "best_lp")})
    batch, cfgs, n_pres = [None], [None], [None]
    for i, (n, sp) in enumerate(zip(armed[1:], specs), start=1):
        b, n_pre = _as_batch(slots[i], n, st["lang_probs"][i], srs[i])
        batch.append(b)
        n_pres.append(n_pre)
        cfgs.append(dataclasses.replace(cfg, beam_size=1, temperature=sp["T"], best_of=n, seed=sp["seed"]))

    x = np.concatenate(xs)
    cur = st
    for step in range(2):
        if step == 1:   # the second step: fresh logits on everybody's outputs
            x = (rng.standard_normal((3 * G, V)) * 2.0).astype(np.float32)
        what = f"beam {beam} {variant} step {step}"
        out = eng.debug_select_step(cfg, {**cur, "logits": x}, "session", rows_per_slot=G, row_inv_temp=rit,
                                    row_seed=seeds)
        assert not out["counters"].any(), what
        want0 = eng.debug_select_step(dataclasses.replace(cfg, beam_size=beam), {**alone, "logits": x[:n0]}, "session")
        for k in want0:
            if k in ("counters", "logits"):
                continue
            rows_of = n0 if k in ROW_KEYS or k == "anc" else 1
            _eq(out[k][:rows_of], want0[k], f"{what} slot 0 {k}")
        for k in ("pos", "state", "cur_tok", "tokens", "lp_hist"):       # (greedy session: slot 0's parked rows)
            _eq(out[k][n0:G], cur[k][n0:G], f"{what} slot 0 parked {k}")
        for i, n in enumerate(armed[1:], start=1):
            want = eng.debug_select_step(cfgs[i], {**batch[i], "logits": x[i * G:i * G + n]}, "batch", n_pres[i])
            _check_sampling(out, cur, want, i * G, n, G, i, f"{what} slot {i}")
            batch[i] = _carry(want)
        if beam > 1:   # a sampling slot's ancestry and bookkeeping stay as they were
            for k in ("anc",):
                _eq(out[k][G:], cur[k][G:], f"{what} sampling slots' {k}")
            for k in ("bwin", "best_tok", "best_lp"):
                _eq(out[k][1:], cur[k][1:], f"{what} sampling slots' {k}")
        alone = _carry(want0)
        cur = _carry(out)
