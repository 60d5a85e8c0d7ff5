"""float64 reference of ONE token-selection step on physical decoder rows: what select_kernel and
beam_update_kernel (csrc/decode.hip, csrc/select.h) do to the row state, the histories, the
ancestry and the per-window beam bookkeeping, restated with the oracle's own pieces.

Greedy / sampling rows use ``oracle.decode.process_logits``, ``log_softmax``, ``sample_token``,
``detect_language`` and ``no_speech_prob``.  Beam windows follow the step of
``oracle.decode.beam_from_encoder`` line by line (score = float32(cumulative) + float32
log-softmax, lexsort by (-score, flat id), the ``sec`` replacement walk, ``_norm_score``, the three
stop conditions), restated over physical rows so that every row's state can be compared after
every step.  ``test_select_ref_cpu.py`` drives this step by step on a stub model and checks that it
reproduces ``greedy_from_encoder`` / ``beam_from_encoder`` exactly.

The state is the dict ``WhisperEngine.debug_select_step`` takes, with float64 in place of float32
(``SEL_REF`` / ``BEAM_REF`` records); ``to_engine`` converts.  Every comparison that decides an
outcome (argmax, the timestamp-mass rule, membership and order of the top 2K, the best-hypothesis
norm) is recorded in ``SelectRef.gaps``: it must be an exact tie of identical inputs or separated
by at least ``GAP``, else a float32 kernel and a float64 reference may legitimately disagree.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from open_speech_amd.dims import SpecialTokens
from open_speech_amd.engine import BEAM_WIN, SEL_STATE, DecodeConfig
from oracle import decode as odec

GAP = 1e-2     # 100x the floor of the float bound below
ATOL, RTOL = 1e-4, 1e-3   # test_gpu_confidences.py's per-token replay bound, on log values

SEL_REF = np.dtype([(n, "f8" if t.kind == "f" else t) for n, (t, _) in SEL_STATE.fields.items()])
BEAM_REF = np.dtype([(n, "f8" if t.kind == "f" else t) for n, (t, _) in BEAM_WIN.fields.items()])
PROMPT, SOT, SAMPLE, DONE = range(4)


def to_engine(state: dict) -> dict:
    out = {}
    for k, v in state.items():
        if k == "state":
            out[k] = _cast(v, SEL_STATE)
        elif k == "bwin":
            out[k] = _cast(v, BEAM_WIN)
        elif np.asarray(v).dtype.kind == "f":
            out[k] = np.asarray(v, np.float32)
        else:
            out[k] = np.array(v, np.int32)
    return out


def to_ref(state: dict) -> dict:
    out = {}
    for k, v in state.items():
        if k == "state":
            out[k] = _cast(v, SEL_REF)
        elif k == "bwin":
            out[k] = _cast(v, BEAM_REF)
        elif k == "logits":
            out[k] = np.asarray(v, np.float32)
        elif np.asarray(v).dtype.kind == "f":
            out[k] = np.asarray(v, np.float64)
        else:
            out[k] = np.array(v, np.int32)
    return out


def _cast(a, dt):
    a = np.asarray(a)
    out = np.zeros(a.shape, dt)
    for n in dt.names:
        out[n] = a[n]
    return out


class Gaps:
    """The smallest separation of the deciding comparisons seen so far."""

    def __init__(self):
        self.min = math.inf
        self.where = None
        self.count = 0

    def need(self, a: float, b: float, identical: bool, what: str) -> None:
        self.count += 1
        if a == b and identical:       # an exact tie of identical inputs: decided by the id order
            return
        g = abs(a - b) if np.isfinite(a) and np.isfinite(b) else math.inf
        if a == b:
            g = 0.0
        if g < self.min:
            self.min, self.where = g, what


class SelectRef:
    """The decode plan's numbers (csrc/plan.h DecodePlan) and one step over a state dict."""

    def __init__(self, dims, cfg: DecodeConfig, mode: str = "batch", n_prefix: int = 0):
        assert cfg.repetition_penalty in (0, 1.0) and cfg.no_repeat_ngram_size == 0, "history rules: history_rules_ref"
        self.dims, self.cfg, self.mode = dims, cfg, mode
        self.V, self.ctx = dims.n_vocab, dims.n_text_ctx
        self.st = st = SpecialTokens.for_vocab(self.V)
        self.english = not st.multilingual
        self.sampling = mode == "batch" and cfg.temperature > 0
        wide = max(1, cfg.beam_size)
        self.beam = 1 if (self.sampling or mode == "refill") else wide
        self.group = max(1, cfg.best_of) if self.sampling else self.beam
        self.inv_temp = np.float32(1.0) / np.float32(cfg.temperature) if self.sampling else np.float32(0)
        self.with_ts = not cfg.without_timestamps
        self.tail = (1 if self.english else 3) + (0 if self.with_ts else 1)
        self.n_pre = n_prefix if mode == "batch" else 0
        self.P = self.n_pre + self.tail
        self.max_len = min(cfg.max_length if cfg.max_length > 0 else self.ctx, self.ctx)
        assert self.P < self.max_len
        self.max_tok = max(1, self.max_len - self.P)
        self.pstride = self.ctx if mode == "session" else self.P
        self.pos_row = mode != "batch"
        patience = cfg.patience if cfg.patience > 0 else 1.0
        self.num_hyp = 1 if mode == "refill" else max(1, cfg.num_hypotheses)
        self.max_cand = 1 if mode == "refill" else max(1, int(math.floor(self.beam * patience + 0.5)))
        self.length_penalty = float(np.float32(cfg.length_penalty))
        self.sot_last = self.english and self.with_ts
        self.conf = cfg.confidences
        self.seed = int(cfg.seed) & 0xFFFFFFFFFFFFFFFF
        self.opts = odec.DecodeOptions(suppress_blank=cfg.suppress_blank, suppress_tokens=tuple(cfg.suppress_tokens),
                                       without_timestamps=cfg.without_timestamps,
                                       max_initial_timestamp_index=cfg.max_initial_timestamp_index,
                                       max_length=cfg.max_length)
        self.gaps = Gaps()
        self.finished = []   # beam: every registered hypothesis (window, tokens, raw score, normalised score)
        # a probe on which the mass rule never fires: its finite entries are the rule-allowed tokens
        self._probe = np.where(np.arange(self.V) < st.timestamp_begin, 0.0, -1e4)

    # ------------------------------------------------------------------ states
    def start_tokens(self, lang):
        """The start sequence with ``lang`` as its language token (None: the -1 placeholder)."""
        st = self.st
        e = [st.sot] if self.english else [st.sot, -1 if lang is None else lang,
                                           st.transcribe if self.cfg.task == "transcribe" else st.translate]
        return e + ([] if self.with_ts else [st.no_timestamps])

    def initial_state(self, windows: int, langs=None, prefixes=None, budgets=None) -> dict:
        """Rows at step 0 of their prompts, as decode() / session_rows_kernel leave them."""
        rows = windows * self.group
        s = dict(pos=np.zeros(rows if self.pos_row else 1, np.int32), state=np.zeros(rows, SEL_REF),
                 prompt=np.zeros((rows, self.pstride), np.int32), cur_tok=np.zeros(rows, np.int32),
                 tokens=np.zeros((rows, self.max_tok), np.int32))
        for r in range(rows):
            w = r // self.group
            pre = list(prefixes[w]) if prefixes else []
            assert self.mode != "refill" or not pre
            assert self.mode != "batch" or len(pre) == self.n_pre
            p = pre + self.start_tokens(langs[w] if langs else None)
            s["prompt"][r, :len(p)] = p
            s["cur_tok"][r] = p[0]
            if self.mode == "session":
                s["state"]["plen"][r] = len(p)
        if budgets is not None or self.mode == "session":
            s["budget"] = np.repeat(np.asarray(budgets if budgets is not None else [0] * windows, np.int32), self.group)
        if self.beam > 1:
            s["anc"] = np.repeat(np.arange(rows, dtype=np.int32)[:, None], self.ctx, 1)
            s["bwin"] = np.zeros(windows, BEAM_REF)
            s["best_tok"] = np.zeros((windows, self.max_tok), np.int32)
        if self.conf:
            s["lp_hist"] = np.zeros((rows, self.ctx))
            if self.beam > 1:
                s["best_lp"] = np.zeros((windows, self.ctx))
            if not self.english:
                s["lang_probs"] = np.zeros((windows, self.st.n_langs))
        return s

    def set_history(self, state: dict, r: int, hist, sum_lp: float = 0.0, lang: int | None = None) -> None:
        """Row r past its prompt with ``hist`` sampled: the state a decode would have left."""
        s = state["state"]
        pl = int(s["plen"][r]) or self.P
        n = len(hist)
        tb = self.st.timestamp_begin
        state["tokens"][r, :n] = hist
        ts = [t for t in hist if t >= tb]
        s["n_sampled"][r], s["sum_lp"][r] = n, sum_lp
        s["last"][r] = hist[-1] if n else 0
        s["penult"][r] = hist[-2] if n >= 2 else 0
        s["last_ts"][r] = ts[-1] if ts else 0
        if lang is not None:
            s["lang"][r] = lang
        state["cur_tok"][r] = hist[-1] if n else state["prompt"][r, pl - 1]
        if self.pos_row:
            state["pos"][r] = pl - 1 + n
        else:
            state["pos"][0] = pl - 1 + n
        if self.conf and "lp_hist" in state:
            s["n_lp"][r] = 0 if self.beam > 1 else n

    def fed(self, state: dict, r: int) -> tuple:
        """The tokens row r's decoder has consumed up to and including this step's input."""
        s = state["state"][r]
        pl = int(s["plen"]) or self.P
        step = int(state["pos"][r if self.pos_row else 0])
        p = [int(s["lang"]) if t < 0 else int(t) for t in state["prompt"][r, :pl]]
        seq = p + [int(t) for t in state["tokens"][r, :int(s["n_sampled"])]]
        return tuple(seq[:step + 1])

    # ------------------------------------------------------------------ one step
    def row_mode(self, s, step: int) -> int:
        pl = int(s["plen"]) or self.P
        if step < pl - 1:
            return SOT if step == pl - self.tail else PROMPT
        return DONE if s["done"] else SAMPLE

    def _rules(self, raw, hist, what):
        """(processed float64 logits, rule-allowed mask before the mass rule); records the mass
        rule's margin."""
        x = odec.process_logits(raw, hist, self.st, self.opts)
        allowed = np.isfinite(odec.process_logits(self._probe, hist, self.st, self.opts))
        if self.with_ts:
            tb = self.st.timestamp_begin
            r64 = raw.astype(np.float64)
            a_ts, a_tx = allowed[tb:], allowed[:tb]
            if a_ts.any() and a_tx.any() and np.isfinite(r64[:tb][a_tx]).any():
                self.gaps.need(odec.logsumexp(r64[tb:][a_ts]), float(np.max(r64[:tb][a_tx])), False, what + " mass rule")
        return x, allowed

    def _argmax(self, key, raw, what) -> int:
        """Lowest id of the maximum; records the margin to the runner-up (ties: identical inputs
        when the raw logits are the same bits)."""
        i = int(np.argmax(key))
        if key.size > 1:
            rest = key.copy()
            rest[i] = -np.inf
            j = int(np.argmax(rest))
            self.gaps.need(float(key[i]), float(key[j]), bool(raw[i] == raw[j]), what + " argmax")
        return i

    def step(self, state: dict, logits: np.ndarray) -> dict:
        """The state after one selection step on ``logits`` [rows][V] (float32 bits as uploaded)."""
        logits = np.asarray(logits, np.float32)
        new = {k: np.array(v, copy=True) for k, v in state.items() if k != "logits"}
        rows = len(state["state"])
        assert rows % self.group == 0 and logits.shape == (rows, self.V)
        for r in range(rows):
            step = int(state["pos"][r if self.pos_row else 0])
            mode = self.row_mode(state["state"][r], step)
            if mode == SAMPLE and self.beam > 1:
                continue
            self._row_step(state, new, r, step, mode, logits[r])
        if self.beam > 1:
            for w in range(rows // self.beam):
                self._window_step(state, new, w, logits)
        new["pos"] = state["pos"] + 1     # every row (window) advances its counter, whatever its mode
        return new

    def _row_step(self, old, new, r, step, mode, raw):
        st, s = self.st, new["state"]
        so = old["state"][r]
        pl = int(so["plen"]) or self.P
        if mode == PROMPT:
            nxt = int(old["prompt"][r, step + 1])
            new["cur_tok"][r] = int(so["lang"]) if nxt < 0 else nxt
            return
        if mode == DONE:
            new["cur_tok"][r] = st.eot
            return
        if mode == SOT:
            s["nsp"][r] = odec.no_speech_prob(raw, st)
            if self.conf and not self.english and r % self.group == 0:
                new["lang_probs"][r // self.group] = np.exp(odec.log_softmax(raw[st.first_lang:st.first_lang + st.n_langs]))
            nxt = int(old["prompt"][r, step + 1])
            if nxt < 0:
                lg = raw[st.first_lang:st.first_lang + st.n_langs]
                self._argmax(lg.astype(np.float64), lg, f"row {r} language")
                nxt = odec.detect_language(raw, st)
            s["lang"][r] = nxt
            new["cur_tok"][r] = nxt
            return
        n = int(so["n_sampled"])
        hist = [int(t) for t in old["tokens"][r, :n]]
        if self.sot_last and n == 0:
            s["nsp"][r] = odec.no_speech_prob(raw, st)
        x, allowed = self._rules(raw, hist, f"row {r}")
        if self.sampling:
            idx = np.nonzero(np.isfinite(x))[0]
            key = x[idx].astype(np.float32) * self.inv_temp + odec.gumbel_noise(self.seed, r, step, idx)
            self._argmax(key.astype(np.float64), np.arange(idx.size), f"row {r} draw")   # (no two keys are 'identical inputs')
            nxt = odec.sample_token(x, self.inv_temp, self.seed, r, step)
        else:
            nxt = self._argmax(x, raw, f"row {r}")
        lp = float(odec.log_softmax(x)[nxt])
        bud = int(old["budget"][r]) if "budget" in old else 0
        if bud > 0 and n >= bud:     # length control: <|endoftext|> under the rule-masked distribution, mass rule apart
            nxt = st.eot
            lp = float(raw[st.eot]) - odec.logsumexp(raw.astype(np.float64)[allowed])
        s["sum_lp"][r] = so["sum_lp"] + lp
        if self.conf and n < self.ctx:
            new["lp_hist"][r, n] = s["sum_lp"][r]
            s["n_lp"][r] = n + 1
        if nxt == st.eot:
            s["done"][r] = 1
        else:
            if n < self.max_tok:
                new["tokens"][r, n] = nxt
            s["n_sampled"][r] = n + 1
            s["penult"][r] = so["last"]
            s["last"][r] = nxt
            if nxt >= st.timestamp_begin:
                s["last_ts"][r] = nxt
            if pl + n + 1 >= self.max_len:
                s["done"][r] = 1
        new["cur_tok"][r] = nxt

    def _window_step(self, old, new, w, logits):
        st, K, V = self.st, self.beam, self.V
        r0 = w * K
        s0 = old["state"][r0]
        step = int(old["pos"][r0 if self.pos_row else 0])
        if self.row_mode(s0, step) != SAMPLE:
            return
        n = int(s0["n_sampled"])
        pl = int(s0["plen"]) or self.P
        first = step == pl - 1
        bud = int(old["budget"][r0]) if "budget" in old else 0
        is_last = pl + n + 1 >= self.max_len or (bud > 0 and n + 1 >= bud)
        ost = old["state"][r0:r0 + K].copy()
        if self.sot_last and first:
            ost["nsp"][0] = odec.no_speech_prob(logits[r0], st)   # every hypothesis descends from row 0
        # --- beam_from_encoder's step: scores, the top 2K, the replacement walk
        scores = []
        for k in range(1 if first else K):
            hist = [int(t) for t in old["tokens"][r0 + k, :n]]
            x, _ = self._rules(logits[r0 + k], hist, f"window {w} row {k}")
            lp = odec.log_softmax(x).astype(np.float32)
            scores.append(np.float32(ost["sum_lp"][k]) + lp)
        flat = np.concatenate(scores)
        f64 = flat.astype(np.float64)
        order = np.lexsort((np.arange(flat.size), -f64))[:2 * K + 1]
        for a, b in zip(order[:-1], order[1:]):   # membership (the 2K-th against the next) and order
            ka, kb = int(a) // V, int(b) // V
            ident = bool(logits[r0 + ka, int(a) % V] == logits[r0 + kb, int(b) % V]) and \
                (ka == kb or (ost["sum_lp"][ka] == ost["sum_lp"][kb] and
                              np.array_equal(logits[r0 + ka], logits[r0 + kb]) and
                              np.array_equal(old["tokens"][r0 + ka, :n], old["tokens"][r0 + kb, :n])))
            ident = ident or (f64[a] == -np.inf and f64[b] == -np.inf)
            self.gaps.need(float(f64[a]), float(f64[b]), ident, f"window {w} top-2K")
        cands = [(float(flat[i]), int(i) // V, int(i) % V) for i in order[:2 * K]]
        bw = new["bwin"]
        chosen, sec, top_fin = [], K, False
        for k in range(K):
            sc, q, tok = cands[k]
            nb = k
            if tok == st.eot or is_last:
                if k == 0:
                    top_fin = True
                ln = n + (0 if tok == st.eot else 1)
                norm = odec._norm_score(sc, ln, self.length_penalty)
                bw["n_hyp"][w] += 1
                toks = [int(t) for t in old["tokens"][r0 + q, :n]] + ([] if tok == st.eot else [tok])
                self.finished.append((w, toks, sc, norm))
                if bw["n_hyp"][w] > 1:   # (the same raw score and norm: the same hypothesis from identical rows)
                    self.gaps.need(float(norm), float(bw["best_norm"][w]), sc == bw["best_raw"][w],
                                   f"window {w} best norm")
                if bw["n_hyp"][w] == 1 or norm > bw["best_norm"][w]:
                    bw["best_norm"][w], bw["best_raw"][w], bw["best_len"][w] = norm, sc, min(ln, self.max_tok)
                    bt = new["best_tok"][w]
                    m = min(n, self.max_tok)
                    bt[:m] = old["tokens"][r0 + q, :m]
                    if tok != st.eot and n < self.max_tok:
                        bt[n] = tok
                    if self.conf:
                        bw["best_nlp"][w] = min(n + 1, self.ctx)
                        for j in range(min(n, self.ctx)):
                            row = int(old["anc"][r0 + q, pl + j]) if pl + j < step else r0 + q
                            new["best_lp"][w, j] = old["lp_hist"][row, j]
                        if n < self.ctx:
                            new["best_lp"][w, n] = sc
                for j in range(sec, 2 * K):
                    if cands[j][2] != st.eot:
                        nb, sec = j, j + 1
                        break
            chosen.append(cands[nb])
        fin = is_last or (top_fin and bw["n_hyp"][w] >= self.num_hyp) or bw["n_hyp"][w] >= self.max_cand
        bw["done"][w] = int(fin)
        ns = new["state"]
        if fin:
            for k in range(K):
                ns[r0 + k] = ost[k]
                ns["done"][r0 + k] = 1
                new["cur_tok"][r0 + k] = st.eot
            return
        for k, (sc, q, tok) in enumerate(chosen):
            r = r0 + k
            m = min(n, self.max_tok)
            new["tokens"][r, :m] = old["tokens"][r0 + q, :m]
            if n < self.max_tok:
                new["tokens"][r, n] = tok
            new["anc"][r, :step] = old["anc"][r0 + q, :step]
            new["anc"][r, step] = r0 + q
            ns[r] = ost[q]
            ns["n_sampled"][r] = n + 1
            ns["penult"][r] = ost["last"][q]
            ns["last"][r] = tok
            if tok >= st.timestamp_begin:
                ns["last_ts"][r] = tok
            ns["sum_lp"][r] = sc
            if self.conf and n < self.ctx:
                new["lp_hist"][r, n] = sc
            new["cur_tok"][r] = tok


# ---------------------------------------------------------------------- comparing
def bound_ratio(got, ref) -> float:
    """max |got - ref| / (ATOL + RTOL |ref|) over the entries; equal infinities agree, anything
    else non-finite is infinitely wrong."""
    got = np.asarray(got, np.float64).reshape(-1)
    ref = np.asarray(ref, np.float64).reshape(-1)
    assert got.shape == ref.shape
    same = (got == ref)
    fin = np.isfinite(got) & np.isfinite(ref)
    if (~same & ~fin).any():
        return math.inf
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - ref[fin]) / (ATOL + RTOL * np.abs(ref[fin]))))


def compare(got: dict, ref: dict, sr: SelectRef, what: str = "") -> float:
    """Discrete outputs exactly, floats within the bound; returns the worst ratio to the bound."""
    for k in ("pos", "cur_tok", "tokens", "anc", "best_tok"):
        if k in ref:
            g, r = np.asarray(got[k]), np.asarray(ref[k])
            assert np.array_equal(g, r), (what, k, np.argwhere(g != r)[:6].tolist(), g[g != r][:6], r[g != r][:6])
    worst = 0.0

    def flt(name, g, r, log=False):
        nonlocal worst
        if log:
            with np.errstate(divide="ignore"):
                g, r = np.log(np.asarray(g, np.float64)), np.log(np.asarray(r, np.float64))
        q = bound_ratio(g, r)
        assert q <= 1.0, (what, name, q, np.asarray(g).reshape(-1)[:8], np.asarray(r).reshape(-1)[:8])
        worst = max(worst, q)

    for rec, names in (("state", SEL_REF.names), ("bwin", BEAM_REF.names)):
        if rec not in ref:
            continue
        for n in names:
            g, r = got[rec][n], ref[rec][n]
            if ref[rec].dtype[n].kind == "f":
                flt(f"{rec}.{n}", g, r, log=(n == "nsp"))
            else:
                assert np.array_equal(g, r), (what, rec, n, g, r)
    for k in ("lp_hist", "best_lp"):
        if k in ref:
            flt(k, got[k], ref[k])
    if "lang_probs" in ref:
        flt("lang_probs", got["lang_probs"], ref["lang_probs"], log=True)
    if "counters" in got:
        assert not np.any(got["counters"]), (what, "arrival / ticket counters not left zeroed", got["counters"])
    return worst


# ---------------------------------------------------------------------- a stub model
def make_logits_fn(V: int, seed: int, st: SpecialTokens, n_peaks: int = 9, eot_after: int = 6,
                   ts_every: int = 3, spacing: float = 1.1, jitter: float = 0.7):
    """logits_fn(fed tokens) -> float32 [V]: a seeded function of the tokens consumed so far.
    A low floor, and a few peaks about ``spacing`` apart (text tokens, some timestamps, the language
    block, <|endoftext|> once ``eot_after`` tokens are in) so that the margins of a float64
    reference are wide; the scenario's CPU test asserts that they are."""
    tb = st.timestamp_begin

    def fn(fed: tuple) -> np.ndarray:
        h = np.random.SeedSequence([seed, len(fed)] + [int(t) + 1 for t in fed[-24:]])
        rng = np.random.default_rng(h)
        x = rng.uniform(-16.0, -11.0, V).astype(np.float32)
        text = rng.choice(st.eot, n_peaks, replace=False)
        ts = tb + rng.choice(V - tb, 4, replace=False)
        ts[0] = tb + min(V - tb - 1, 2 * len(fed) + int(rng.integers(0, 3)))   # one that moves forward
        lang = st.first_lang + rng.choice(st.n_langs, 3, replace=False)
        ids = np.concatenate([text, ts if len(fed) % ts_every == 0 else ts[:1], lang])
        vals = 9.0 - spacing * np.arange(ids.size) + rng.uniform(0.0, jitter, ids.size)
        x[ids] = rng.permutation(vals).astype(np.float32)
        x[st.no_speech] = np.float32(rng.uniform(-3.0, 3.0))
        if len(fed) > eot_after:
            x[st.eot] = np.float32(rng.uniform(4.0, 9.5))
        return x

    return fn


class StubOracle:
    """oracle.decode's model interface on a logits_fn: the cache is the list of tokens fed."""

    def __init__(self, logits_fn):
        self.fn = logits_fn

    def new_cache(self):
        return []

    def decoder_step(self, tok, pos, cache, xkv):
        assert pos == len(cache)
        cache.append(int(tok))
        return self.fn(tuple(cache))


def drive(sr: SelectRef, state: dict, logits_fn, steps: int, stepper, after=None) -> dict:
    """``steps`` selection steps: logits from ``logits_fn`` of what each row has been fed,
    ``stepper(state, logits)`` -> the next state; ``after(i, state, logits)`` sees each one."""
    for i in range(steps):
        rows = len(state["state"])
        cache = {}
        logits = np.empty((rows, sr.V), np.float32)
        for r in range(rows):
            f = sr.fed(state, r)
            if f not in cache:
                cache[f] = logits_fn(f)
            logits[r] = cache[f]
        state = stepper(state, logits)
        if after:
            after(i, state, logits)
    return state
