"""The inputs test_gpu_select.py feeds the selection kernels, built without a GPU so that
test_select_ref_cpu.py can run each through the float64 reference and assert its margins.

A scenario is a function returning a ``Case``: decode options, a mode, a crafted state and either
one logits array (a single step) or a ``logits_fn`` and a step count (a scripted run).  Geometry
the cases aim at (csrc/select.h, csrc/decode.hip): 16 vocabulary slices of per = ceil(V / 16) =
3242 entries, the last one shorter; 256 threads per slice, thread t holding entries lo + t + 256 i;
waves of 64 lanes; suppress-mask words of 32 tokens, the last one partial at V = 51865."""
from __future__ import annotations

import dataclasses

import numpy as np

import english_ref as er
import select_ref as R
from open_speech_amd import dims as D
from open_speech_amd.engine import DecodeConfig
from oracle import decode as odec

VOCABS = (51864, 51865, 51866)
SLICES = 16


def dims(V):
    return dataclasses.replace(D.MICRO_TEST, n_vocab=V)


def per(V):
    return -(-V // SLICES)


@dataclasses.dataclass
class Case:
    V: int
    cfg: DecodeConfig
    state: dict
    mode: str = "batch"
    n_prefix: int = 0
    logits: np.ndarray | None = None
    logits_fn: object = None
    steps: int = 1
    expect: object = None      # scripted runs: window -> (tokens, raw score) from oracle.decode on the stub

    def ref(self) -> R.SelectRef:
        return R.SelectRef(dims(self.V), self.cfg, self.mode, self.n_prefix)


def run_reference(case: Case):
    """(the SelectRef that ran, [(state entering step i, its logits) ..., (final state, None)])."""
    sr = case.ref()
    steps = []
    if case.logits is not None:
        steps.append((case.state, case.logits))
        steps.append((sr.step(case.state, case.logits), None))
        return sr, steps
    prev = [case.state]

    def stepper(state, logits):
        steps.append((state, logits))
        return sr.step(state, logits)

    final = R.drive(sr, prev[0], case.logits_fn, case.steps, stepper)
    steps.append((final, None))
    return sr, steps


def _floor(rng, rows, V, lo=-14.0, hi=-11.0):
    return rng.uniform(lo, hi, (rows, V)).astype(np.float32)


def _state(V, cfg, mode, windows, n_prefix=0, budgets=None, prefixes=None, lang=True):
    sr = R.SelectRef(dims(V), cfg, mode, n_prefix)
    langs = [sr.st.first_lang + 3] * windows if lang else None
    st = sr.initial_state(windows, langs=langs, budgets=budgets, prefixes=prefixes)
    if lang:
        st["state"]["lang"][:] = sr.st.first_lang + 3
    return sr, st


SCENARIOS = {}


def scenario(vocabs=VOCABS):
    def deco(fn):
        for V in vocabs:
            SCENARIOS[f"{fn.__name__}-{V}"] = (lambda V=V: fn(V))
        return fn
    return deco


# ====================================================================== greedy single steps
@scenario()
def first_step(V):
    """n == 0 with timestamps: text and timestamps past max_initial_timestamp are masked.  Row 0:
    the largest raw logit is a text token, a larger one sits at tb + 51, the winner is exactly
    tb + 50.  Row 1: the winner is tb itself.  Row 2: <|notimestamps|> and <|endoftext|> largest.
    (English-only: this is the combined <|startoftranscript|> step.)"""
    cfg = DecodeConfig(max_length=32, confidences=True)
    sr, st = _state(V, cfg, "refill", 3)
    tb = sr.st.timestamp_begin
    x = _floor(np.random.default_rng(V), 3, V)
    for r in range(3):
        sr.set_history(st, r, [])
    x[0, [1000, tb + 51, tb + 50, tb + 3]] = [10.0, 9.0, 8.0, 7.5]
    x[1, [0, V - 1, tb, tb + 50]] = [10.0, 9.5, 8.0, 7.0]
    x[2, [sr.st.no_timestamps, sr.st.eot, tb + 17, tb + 18]] = [10.0, 9.0, 3.0, 2.5]
    x[:, sr.st.no_speech] = [1.0, -2.0, 4.0]
    return Case(V, cfg, st, "refill", logits=x)


@scenario()
def first_step_no_max_initial(V):
    """max_initial_timestamp off (-1): the winner is the last token of the vocabulary."""
    cfg = DecodeConfig(max_length=32, max_initial_timestamp_index=None)
    sr, st = _state(V, cfg, "refill", 2)
    tb = sr.st.timestamp_begin
    x = _floor(np.random.default_rng(V + 1), 2, V)
    for r in range(2):
        sr.set_history(st, r, [])
    x[0, [77, V - 1, tb + 50]] = [10.0, 8.0, 7.0]
    x[1, [77, V - 2, tb + 51]] = [10.0, 7.0, 8.0]
    return Case(V, cfg, st, "refill", logits=x)


@scenario()
def suppress_blank(V):
    """No timestamps.  Row 0 (n == 0): blank and <|endoftext|> hold the largest logits and are
    masked.  Rows 1, 2 (n == 1): they are allowed again; row 2 ends."""
    cfg = DecodeConfig(max_length=32, without_timestamps=True)
    sr, st = _state(V, cfg, "refill", 3)
    x = _floor(np.random.default_rng(V + 2), 3, V)
    sr.set_history(st, 0, [])
    sr.set_history(st, 1, [500], -0.5)
    sr.set_history(st, 2, [501], -0.25)
    x[0, [sr.st.blank, sr.st.eot, 4000]] = [10.0, 9.0, 8.0]
    x[1, [sr.st.blank, sr.st.eot, 4000]] = [10.0, 9.0, 8.0]
    x[2, [sr.st.blank, sr.st.eot, 4000]] = [9.0, 10.0, 8.0]
    return Case(V, cfg, st, "refill", logits=x)


@scenario()
def timestamp_pairs(V):
    """The four (last is a timestamp, the one before is) combinations, T = tb + 20.
    0: [text, T]  T - 1 masked, T allowed (after a lone timestamp), text masked      -> T
    1: [text, T]  <|endoftext|> allowed where text is not                            -> eot
    2: [T-5, T]   every timestamp masked, text allowed                               -> text
    3: [T, text]  T masked, T + 1 allowed                                            -> T + 1
    4: [T, text]  T holds the largest logit and is masked, text beats the rest       -> text
    5: [text, text] no timestamp yet: tb itself is allowed                           -> tb
    6: [T]        a lone first timestamp: timestamps masked                          -> text
    7: [T, T, text, T+2] last_ts follows the history                                 -> T + 2"""
    cfg = DecodeConfig(max_length=32, confidences=True)
    sr, st = _state(V, cfg, "refill", 8)
    tb, eot = sr.st.timestamp_begin, sr.st.eot
    T = tb + 20
    x = _floor(np.random.default_rng(V + 3), 8, V)
    hists = [[300, T], [300, T], [T - 5, T], [T, 300], [T, 300], [300, 301], [T], [T, T, 300, T + 2]]
    for r, h in enumerate(hists):
        sr.set_history(st, r, h, -0.5 * r)
    x[0, [300, T - 1, T, eot]] = [12.0, 11.0, 10.0, 8.0]
    x[1, [300, T - 1, eot, T]] = [12.0, 11.0, 10.0, 8.0]
    x[2, [T + 1, T, 400]] = [12.0, 11.0, 10.0]
    x[3, [T, T + 1, 400]] = [12.0, 11.0, 9.0]
    x[4, [T, 400, T + 1]] = [12.0, 11.0, 4.0]
    x[5, [tb, 400]] = [11.0, 9.0]
    x[6, [T + 1, tb, 400, eot]] = [12.0, 11.5, 10.0, 9.0]
    x[7, [300, T + 1, T + 2, eot]] = [12.0, 11.0, 10.0, 8.0]
    return Case(V, cfg, st, "refill", logits=x)


@scenario()
def mass_rule(V):
    """300 equal timestamp logits c, each below the best text logit 10: their log-sum-exp is
    c + log 300.  Rows 0 / 1 straddle the threshold by 0.05: timestamps win (the pick is the best
    timestamp, its log-probability under the timestamps alone) / text wins.  Rows 2 / 3 the same
    with one timestamp 0.02 above the others, far from the first."""
    cfg = DecodeConfig(max_length=32, confidences=True)
    sr, st = _state(V, cfg, "refill", 4)
    tb = sr.st.timestamp_begin
    x = _floor(np.random.default_rng(V + 4), 4, V, -40.0, -35.0)
    ids = tb + 5 * np.arange(300)
    for r in range(4):
        sr.set_history(st, r, [300 + r], -1.0)
        c = 10.0 - np.log(300.0) + (0.05 if r % 2 == 0 else -0.05)
        x[r, ids] = np.float32(c)
        x[r, 2000 + r] = 10.0
        x[r, 2100] = 9.5
        if r >= 2:
            x[r, ids[211]] += np.float32(0.02)
    return Case(V, cfg, st, "refill", logits=x)


@scenario()
def extrema_and_ties(V):
    """Maxima at v = 0, at V - 1, at the last entry of slice 3 and the first of slice 4, and exact
    ties (the lowest id wins) between lanes, waves, the entries of one thread, a lower lane holding
    the higher id, slices, and the two ends of the vocabulary.  Rows 4, 5: the row's mass sits in
    the last entry of a slice / of the vocabulary, where the clamped loads land: counted twice, the
    pick's log-probability would move by log 2."""
    cfg = DecodeConfig(max_length=32, without_timestamps=True, suppress_blank=False, confidences=True)
    p = per(V)
    picks = [[0], [V - 1], [4 * p - 1], [4 * p], [7 * p - 1], [V - 1],
             [2 * p + 10, 2 * p + 11], [2 * p + 10, 2 * p + 74], [2 * p + 10, 2 * p + 266],
             [2 * p + 5 + 256, 2 * p + 3 + 512], [2 * p + 100, 9 * p + 1], [0, V - 1], [3 * p - 1, 3 * p]]
    sr, st = _state(V, cfg, "refill", len(picks))
    x = _floor(np.random.default_rng(V + 5), len(picks), V, -30.0, -25.0)
    for r, ids in enumerate(picks):
        sr.set_history(st, r, [600 + r], -0.125 * r)
        x[r, ids] = 6.0
        if r not in (4, 5):
            x[r, 12345] = 5.0
    return Case(V, cfg, st, "refill", logits=x)


@scenario()
def neg_inf(V):
    """-inf entries (what the history rules write).  Row 0: slice 7 is -inf throughout.  Row 1: a
    single finite entry in the whole row.  Row 2: the raw maximum is -inf-masked by the rules and
    every other entry of its slice is -inf."""
    cfg = DecodeConfig(max_length=32, without_timestamps=True, suppress_tokens=(9000,), confidences=True)
    p = per(V)
    sr, st = _state(V, cfg, "refill", 3)
    x = _floor(np.random.default_rng(V + 6), 3, V)
    for r in range(3):
        sr.set_history(st, r, [700 + r], -1.0)
    x[0, 7 * p:8 * p] = -np.inf
    x[0, [8 * p, 7 * p - 1]] = [5.0, 4.0]
    x[1, :] = -np.inf
    x[1, 5 * p + 300] = -3.0
    x[2, 2 * p:3 * p] = -np.inf
    x[2, [9000, 40000]] = [9.0, 3.0]
    assert 2 * p <= 9000 < 3 * p
    return Case(V, cfg, st, "refill", logits=x)


@scenario()
def suppress_mask_bits(V):
    """Suppressed ids at v % 32 in {0, 31}, in the first word, and in the last (partial) word of
    the mask; each holds a large logit, the winner is an unsuppressed neighbour."""
    last = (V - 1) // 32 * 32     # first id of the last mask word
    sup = (0, 31, 64, 95, 4095, 4096, last, V - 1)
    cfg = DecodeConfig(max_length=32, without_timestamps=True, suppress_blank=False, suppress_tokens=sup)
    sr, st = _state(V, cfg, "refill", 5)
    x = _floor(np.random.default_rng(V + 7), 5, V)
    for r in range(5):
        sr.set_history(st, r, [800 + r], -1.0)
    x[0, [0, 31, 1, 30, 32]] = [12.0, 11.0, 8.0, 9.0, 10.0]
    x[1, [64, 95, 63, 65, 94, 96]] = [12.0, 11.0, 7.0, 8.0, 9.0, 10.0]
    x[2, [4095, 4096, 4094, 4097]] = [12.0, 11.0, 9.0, 10.0]
    x[3, [V - 1, last, V - 2, last + 1, last - 1]] = [12.0, 11.0, 10.0, 9.0, 8.0]
    x[4, [V - 1, last, last - 1, V - 2]] = [12.0, 11.0, 10.0, 9.0]
    return Case(V, cfg, st, "refill", logits=x)


@scenario()
def ends_and_modes(V):
    """Refill rows at different counters and in different modes in one call, max_length 32:
    0: budget 3 reached -> <|endoftext|> with log-probability x[eot] - lse over the allowed tokens
    1: budget 2 reached where the timestamp mass would win (still lse over ALL allowed tokens)
    2: the pick reaches max_length: stored, and the row ends
    3: n_sampled == max_tok on a row not yet ended: the pick is not stored
    4: <|endoftext|> wins
    5: a finished row                  6: a row in its prompt (counter 0)
    7: budget 5 not reached"""
    cfg = DecodeConfig(max_length=32, confidences=True)
    bud = [3, 2, 0, 0, 0, 0, 0, 5]
    sr, st = _state(V, cfg, "refill", 8, budgets=bud)
    tb, eot = sr.st.timestamp_begin, sr.st.eot
    mt = sr.max_tok
    x = _floor(np.random.default_rng(V + 8), 8, V)
    full = [tb + 1] + [900 + i for i in range(mt - 1)]
    hists = [[tb + 1, 300, 301], [tb + 2, 300], full[:mt - 1], full, [tb + 1, 300], [tb + 1, 300, 302], None,
             [tb + 1, 300, 303]]
    for r, h in enumerate(hists):
        if h is not None:
            sr.set_history(st, r, h, -0.75 * r)
    st["state"]["done"][5] = 1
    if sr.english:    # (a one-token prompt has no prompt step: the combined first step instead)
        sr.set_history(st, 6, [])
        x[6, [tb + 5, tb + 6]] = [8.0, 7.0]
    else:
        st["pos"][6] = 1
    x[0, [400, eot]] = [10.0, 2.0]
    x[1, [tb + 10, tb + 11, 400, eot]] = [10.0, 9.5, 9.0, 1.0]
    x[2, [401, eot]] = [10.0, 3.0]
    x[3, [402, eot]] = [10.0, 3.0]
    x[4, [eot, 403]] = [10.0, 9.0]
    x[7, [404, eot]] = [10.0, 9.0]
    return Case(V, cfg, st, "refill", logits=x)


@scenario((51865, 51866))
def sot_step(V):
    """The <|startoftranscript|> step behind a 2-token prefix (batch mode, shared counter 2).
    Windows 0, 1 detect (-1 placeholder) with larger logits just outside the language block at
    first_lang - 1 and first_lang + n_langs; window 2 has its language given."""
    cfg = DecodeConfig(max_length=32, confidences=True)
    sr = R.SelectRef(dims(V), cfg, "batch", 2)
    s = sr.st
    st = sr.initial_state(3, langs=[None, None, s.first_lang + 9], prefixes=[[s.sot_prev, 1234]] * 3)
    st["pos"][0] = 2
    st["cur_tok"][:] = s.sot
    x = _floor(np.random.default_rng(V + 9), 3, V)
    x[:, [s.first_lang - 1, s.first_lang + s.n_langs]] = [12.0, 11.0]
    x[0, [s.first_lang, s.first_lang + s.n_langs - 1]] = [5.0, 6.0]
    x[1, [s.first_lang, s.first_lang + s.n_langs - 1, s.first_lang + 40]] = [6.0, 5.0, 5.5]
    x[2, s.first_lang + 1] = 7.0
    x[:, s.no_speech] = [3.0, -1.0, 9.0]
    return Case(V, cfg, st, "batch", n_prefix=2, logits=x)


@scenario((51865, 51866))
def sot_step_groups(V):
    """The same step with 5 rows per window (beam 5): only the first row of each window writes the
    window's language probabilities, every row detects for itself."""
    cfg = DecodeConfig(max_length=32, confidences=True, beam_size=5)
    sr = R.SelectRef(dims(V), cfg, "batch")
    s = sr.st
    st = sr.initial_state(2, langs=[None, None])
    rng = np.random.default_rng(V + 10)
    x = _floor(rng, 10, V)
    for r in range(10):
        x[r, s.first_lang + (7 * r) % s.n_langs] = 6.0 + 0.1 * r
        x[r, s.no_speech] = 0.5 * r - 2.0
    return Case(V, cfg, st, "batch", logits=x)


@scenario((51864,))
def english_steps(V):
    """English-only rows (refill).  Without timestamps: row 0 at its <|startoftranscript|> step
    (no-speech probability, next token <|notimestamps|>), row 1 sampling."""
    cfg = DecodeConfig(max_length=32, without_timestamps=True, confidences=True)
    sr, st = _state(V, cfg, "refill", 2, lang=False)
    x = _floor(np.random.default_rng(V + 11), 2, V)
    sr.set_history(st, 1, [])
    x[:, sr.st.no_speech] = [2.0, 5.0]
    x[1, [sr.st.blank, 77]] = [9.0, 8.0]
    return Case(V, cfg, st, "refill", logits=x)


def _sampling(V, seed, with_ts):
    """Sampling rows (temperature 0.8, best_of 4, 2 windows) two tokens in: the token is the
    oracle's Gumbel-max draw for (seed, row, step), its log-probability the untempered one."""
    cfg = DecodeConfig(max_length=32, temperature=0.8, best_of=4, seed=seed, without_timestamps=not with_ts,
                       confidences=True)
    sr, st = _state(V, cfg, "batch", 2)
    tb = sr.st.timestamp_begin
    rng = np.random.default_rng([V, seed])
    x = (rng.standard_normal((8, V)) * 2.0).astype(np.float32)
    for r in range(8):
        sr.set_history(st, r, [tb + 3, 1000 + r] if with_ts else [1000 + r, 2000 + r], -1.0 - r)
        if with_ts and r % 2:
            x[r, tb + 4:tb + 400] += 6.0      # the timestamp mass wins
    return Case(V, cfg, st, "batch", logits=x)


for _seed, _ts in ((0, False), (2, True), (2 ** 63 + 11, False), (3, True)):
    for _V in VOCABS:
        SCENARIOS[f"sampling-s{_seed % 1000}-{_V}"] = (lambda V=_V, s=_seed, t=_ts: _sampling(V, s, t))


# ====================================================================== beam single steps
def _beam_rows(sr, st, x, w, hist_fn, sums, lo_rows_peaks=True):
    """Window w: row k gets history hist_fn(k) and cumulative score sums[k]; rows after the first
    get two spaced text peaks so that their candidates are well ordered."""
    K = sr.beam
    for k in range(K):
        r = w * K + k
        sr.set_history(st, r, hist_fn(k), sums[k])
        if lo_rows_peaks and k:
            x[r, [200 + 10 * w + k, 300 + 10 * w + k]] = [3.0 - 0.3 * k, 1.0 - 0.3 * k]


@scenario()
def beam_first_step(V):
    """The first sampled step (beam 5, 3 windows, window 1 already finished): only row 0 of a
    window expands; rows 1 .. K-1 hold larger logits that must be ignored.  Window 2 ends at once
    with a zero-length hypothesis (<|endoftext|> on top) and length_penalty 1: norm -inf."""
    cfg = DecodeConfig(max_length=32, without_timestamps=True, suppress_blank=False, beam_size=5, confidences=True)
    sr, st = _state(V, cfg, "batch", 3)
    x = _floor(np.random.default_rng(V + 20), 15, V)
    for r in range(15):
        sr.set_history(st, r, [])
    p = per(V)
    for w in range(3):
        ids = [p * (3 * j + w) + 17 * j for j in range(5)] + [p * 15 + 5 + j for j in range(6)]
        x[5 * w, ids] = 8.0 - 0.4 * np.arange(11, dtype=np.float32)
        x[5 * w + 1:5 * w + 5, 1000:1010] = 20.0
    x[10, sr.st.eot] = 9.0
    st["state"]["done"][5:10] = 1
    st["bwin"]["done"][1] = 1
    return Case(V, cfg, st, "batch", logits=x)


def _paths(V, K, with_ts, which):
    """Candidate-list paths of beam_slice_body (K2 = 2K lists per slice), one window per path, the
    window's row 0 far ahead of the others (cumulative 0 against -50 - k) so that the window's top
    2K is the list of ONE slice of ONE row and shows what that path produced:
      rank   2K + 2 peaks 0.2 apart in lanes of wave 0: T = the 2K-th, |S| = 2K <= 64   -> wave 0 wave_rank
      pairs  100 tied maxima 7 ids apart: T = the tie, 64 < |S| = 100 <= 256     -> all-pairs rank
      pops   300 tied maxima 3 ids apart: |S| = 300 > 256                        -> block-wide pops
      empty  the slice is -inf but for 4 entries: every wave has fewer than 2K finite allowed
             entries, T = -inf                                                    -> block-wide pops
    List A (no timestamps, slice 5) or list B (timestamps on and their mass winning, the
    timestamps' slice 15; the other rows stay on list A: one window split between the lists)."""
    cfg = DecodeConfig(max_length=32, without_timestamps=not with_ts, suppress_blank=False, beam_size=K)
    sr, st = _state(V, cfg, "batch", len(which))
    tb = sr.st.timestamp_begin
    p = per(V)
    x = _floor(np.random.default_rng([V, K, with_ts]), len(which) * K, V)
    base = tb if with_ts else 5 * p
    lo, hi = (15 * p, V) if with_ts else (5 * p, 6 * p)
    assert lo <= base < hi
    K2 = 2 * K
    for w, path in enumerate(which):
        _beam_rows(sr, st, x, w, lambda k: [100 + k], [0.0] + [-50.0 - 1.37 * k for k in range(1, K)])
        r = w * K
        if path == "rank":
            i = np.arange(K2 + 2)   # distinct lanes of wave 0 (thread = (v - lo) % 256 < 64)
            ids = lo + 256 * ((7 if with_ts else 0) + i % 4) + 3 * i
            assert ids.min() >= base and ids.max() < hi
            x[r, ids] = 8.0 - 0.2 * i.astype(np.float32)
        elif path == "pairs":
            x[r, base + 7 * np.arange(100)] = 6.0
        elif path == "pops":
            x[r, base + 3 * np.arange(300)] = 5.0
        else:
            x[r, lo:hi] = -np.inf
            x[r, base + np.array([5, 70, 300, 1000])] = [9.0, 8.5, 8.0, 7.5]
            if not with_ts:   # the rest of the top 2K: spaced peaks of another slice
                x[r, 9 * p + 11 * np.arange(K2)] = 4.0 - 0.3 * np.arange(K2, dtype=np.float32)
    return Case(V, cfg, st, "batch", logits=x)


for _V in VOCABS:
    for _K in (2, 5, 6, 8):
        for _ts in (False, True):
            _n = "B" if _ts else "A"
            SCENARIOS[f"beam_paths{_n}-k{_K}-{_V}"] = (lambda V=_V, K=_K, t=_ts: _paths(V, K, t, ("rank", "pairs")
                                                                                        if K > 5 else ("rank", "pairs", "pops")))
            if _K in (5, 8):
                SCENARIOS[f"beam_paths{_n}-tail-k{_K}-{_V}"] = (
                    lambda V=_V, K=_K, t=_ts: _paths(V, K, t, ("empty", "pops") if K > 5 else ("empty",)))


@scenario()
def beam_one_per_slice(V):
    """Beam 8: the top 16 is one candidate from each of the 16 slices of row 3 (the first and the
    last entry of slices among them); beam 8 runs beam_update's KM = 8 instantiation."""
    cfg = DecodeConfig(max_length=32, without_timestamps=True, suppress_blank=False, beam_size=8, confidences=True)
    sr, st = _state(V, cfg, "batch", 2)
    p = per(V)
    x = _floor(np.random.default_rng(V + 22), 16, V)
    for w in range(2):
        _beam_rows(sr, st, x, w, lambda k: [100 + k, 150 + k], [-40.0 - k for k in range(8)])
        st["state"]["sum_lp"][8 * w + 3] = -1.0
    for w in range(2):
        ids = np.array([s * p + (0 if s % 3 == 0 else min(p, V - s * p) - 1 if s % 3 == 1 else 1000 + 64 * s)
                        for s in range(16)])
        x[8 * w + 3, ids] = 8.0 - 0.25 * np.random.default_rng(V + w).permutation(16).astype(np.float32)
    return Case(V, cfg, st, "batch", logits=x)


@scenario()
def beam_exact_ties(V):
    """Identical rows with identical cumulative scores (beam 5, 2 windows): equal scores across
    rows are ordered by flat id (row, then token), and two tokens of one row tie as well."""
    cfg = DecodeConfig(max_length=32, without_timestamps=True, suppress_blank=False, beam_size=5, confidences=True)
    sr, st = _state(V, cfg, "batch", 2)
    p = per(V)
    row = _floor(np.random.default_rng(V + 23), 1, V)[0]
    row[[3 * p + 9, 11 * p + 70]] = 7.0      # a tie within the row, across slices
    row[[40, 41]] = [6.0, 5.0]
    x = np.repeat(row[None], 10, 0)
    for r in range(10):
        sr.set_history(st, r, [100, 101], -2.5)
    x[5:, sr.st.eot] = 7.0       # window 1: <|endoftext|> ties with both, in every row: a three-way tie and the sec walk
    return Case(V, cfg, st, "batch", logits=x)


def _eot(V, K, patience, num_hyp, lp, eots, budget=None, last=False, n=2):
    """A window (beam K) whose row k holds two text tokens (6.0 and 5.0 - 0.2 k) and, for the rows
    in ``eots``, <|endoftext|> at the given logit, with cumulative scores -1 - 0.55 k: where
    <|endoftext|> lands in the top 2K is stated per scenario below (and follows from the
    reference).  Two children of one parent and dropped parents occur throughout.  ``last``:
    max_length is reached with this step; ``budget``: the window's token budget."""
    cfg = DecodeConfig(max_length=32, without_timestamps=True, suppress_blank=False, beam_size=K,
                       patience=patience, num_hypotheses=num_hyp, length_penalty=lp, confidences=True)
    if last:
        cfg = dataclasses.replace(cfg, max_length=R.SelectRef(dims(V), cfg, "batch").P + n + 1)
    sr, st = _state(V, cfg, "batch", 1, budgets=None if budget is None else [budget])
    eot = sr.st.eot
    x = _floor(np.random.default_rng([V, K, len(eots), n]), K, V, -30.0, -25.0)
    _beam_rows(sr, st, x, 0, lambda k: [100 + k] * n, [-1.0 - 0.55 * k for k in range(K)], lo_rows_peaks=False)
    for k in range(K):
        x[k, [1000 + k, 2000 + k]] = [6.0, 5.0 - 0.2 * k]
        if k in eots:
            x[k, eot] = eots[k]
    rng = np.random.default_rng(V)
    st["lp_hist"][:K, :n] = -np.cumsum(rng.uniform(0.05, 0.3, (K, n)), 1)
    return Case(V, cfg, st, "batch", logits=x)


for _V in VOCABS:
    # <|endoftext|> of row 0 on top (rank 0): the window ends at once (num_hypotheses 1)
    SCENARIOS[f"beam_eot-top-{_V}"] = lambda V=_V: _eot(V, 5, 1.0, 1, 1.0, {0: 6.6})
    # at ranks 1 and 3, patience 2, num_hypotheses 3, length_penalty 0: two hypotheses, replaced from ranks >= K
    SCENARIOS[f"beam_eot-several-{_V}"] = lambda V=_V: _eot(V, 5, 2.0, 3, 0.0, {1: 6.3, 2: 6.5})
    # every row's best is <|endoftext|>: patience 1 stops at 5 hypotheses although num_hypotheses is 3 ...
    SCENARIOS[f"beam_eot-patience-{_V}"] = lambda V=_V: _eot(V, 5, 1.0, 3, 1.0, {k: 7.5 for k in range(5)})
    # beam 2: <|endoftext|> at rank 2, inside the top 2K but beyond K: nothing finishes
    SCENARIOS[f"beam_eot-beyond-{_V}"] = lambda V=_V: _eot(V, 2, 1.0, 1, 1.0, {0: 5.5})
    SCENARIOS[f"beam_eot-k6-{_V}"] = lambda V=_V: _eot(V, 6, 2.0, 3, 1.0, {0: 6.6, 3: 6.4})
    # the last step by max_length and by the budget: every one of the top K finishes, whatever its token
    SCENARIOS[f"beam_last-length-{_V}"] = lambda V=_V: _eot(V, 5, 1.0, 1, 1.0, {1: 6.3, 2: 6.5}, last=True)
    SCENARIOS[f"beam_last-budget-{_V}"] = lambda V=_V: _eot(V, 5, 1.0, 1, 0.0, {2: 6.5}, budget=3)


@scenario()
def beam_long_history(V):
    """Session mode, beam 5, max_length 448: window 0 has 300 sampled tokens behind a 40-token
    prefix (positions past 256: the second half of the history / ancestry copies) and a scrambled
    ancestry; one hypothesis ends, so best_tok and best_lp gather along the ancestry.  Window 1 is
    2 tokens in, window 2 is still in its prompt: three counters in one launch."""
    cfg = DecodeConfig(max_length=448, without_timestamps=True, suppress_blank=False, beam_size=5, patience=2.0,
                       confidences=True)
    sr = R.SelectRef(dims(V), cfg, "session")
    s = sr.st
    rng = np.random.default_rng(V + 30)
    pre = [s.sot_prev] + [int(t) for t in rng.integers(0, 50000, 39)]
    st = sr.initial_state(3, langs=[s.first_lang + 1] * 3, prefixes=[pre, [], [s.sot_prev, 7, 8]], budgets=[0, 0, 0])
    st["state"]["lang"][:] = s.first_lang + 1
    x = _floor(rng, 15, V, -30.0, -25.0)
    for k in range(5):
        sr.set_history(st, k, [int(t) for t in rng.integers(0, 50000, 300)], -30.0 - 0.5 * k)
        sr.set_history(st, 5 + k, [100 + k, 200 + k], -1.0 - 0.5 * k)
        x[k, [1000 + k, 2000 + k]] = [6.0, 5.0 - 0.2 * k]
        x[5 + k, [1000 + k, 2000 + k]] = [6.0, 5.0 - 0.2 * k]
        x[k, s.eot] = 6.6 - 0.1 * k if k == 1 else -3.0
    step0 = int(st["pos"][0])
    st["anc"][:5, :step0] = rng.integers(0, 5, (5, step0))
    st["anc"][5:10, :int(st["pos"][5])] = rng.integers(5, 10, (5, int(st["pos"][5])))
    st["lp_hist"][:10] = -np.cumsum(rng.uniform(0.05, 0.3, (10, sr.ctx)), 1)
    return Case(V, cfg, st, "session", logits=x)


# ====================================================================== scripted runs
def _oracle(case_sr, fn, prev=()):
    st, sr = case_sr.st, case_sr
    if sr.beam > 1:
        bo = odec.BeamOptions(beam_size=sr.beam, patience=sr.cfg.patience, length_penalty=sr.cfg.length_penalty,
                              num_hypotheses=sr.cfg.num_hypotheses)
        f = er.beam_from_encoder if sr.english else odec.beam_from_encoder
        res = f(R.StubOracle(fn), None, st, prev_tokens=prev, opts=sr.opts, beam=bo)
    else:
        f = er.greedy_from_encoder if sr.english else odec.greedy_from_encoder
        res = f(R.StubOracle(fn), None, st, prev_tokens=prev, opts=sr.opts)
    return res.tokens, res.sum_logprob


def _scripted(V, cfg, mode, seed, steps, prevs=((),), budgets=None, **fn_kw):
    n_pre = len(prevs[0]) + 1 if (mode == "batch" and prevs[0]) else 0
    sr = R.SelectRef(dims(V), cfg, mode, n_pre)
    s = sr.st
    fn = R.make_logits_fn(V, seed, s, **fn_kw)
    prefixes = [([s.sot_prev] + list(p)) if p else [] for p in prevs]
    st = sr.initial_state(len(prevs), prefixes=prefixes if mode != "refill" else None, budgets=budgets)
    expect = None if sr.sampling else {w: _oracle(sr, fn, tuple(p)) for w, p in enumerate(prevs)}
    return Case(V, cfg, st, mode, n_prefix=n_pre, logits_fn=fn, steps=steps, expect=expect)


SCENARIOS["script-greedy-51865"] = lambda: _scripted(
    51865, DecodeConfig(max_length=36, confidences=True, suppress_tokens=(1, 31, 50000)), "batch", 11, 36)
SCENARIOS["script-greedy-refill-51864"] = lambda: _scripted(
    51864, DecodeConfig(max_length=30, confidences=True), "refill", 12, 30)
SCENARIOS["script-sampling-51866"] = lambda: _scripted(
    51866, DecodeConfig(max_length=28, temperature=0.6, best_of=3, seed=77, confidences=True), "batch", 13, 28,
    prevs=((), ()))
# Beam runs compare ~10 scores per window and step, so their stub has fewer, wider peaks, and the
# seeds are ones whose margins test_select_ref_cpu.py finds wide enough (most are not).
_BEAM_STUB = dict(n_peaks=3, spacing=2.3, jitter=1.3, eot_after=5)
SCENARIOS["script-beam5-batch-51865"] = lambda: _scripted(
    51865, DecodeConfig(max_length=30, beam_size=5, confidences=True), "batch", 105, 30, prevs=((3, 4),), **_BEAM_STUB)
SCENARIOS["script-beam5-session-51866"] = lambda: _scripted(
    51866, DecodeConfig(max_length=32, beam_size=5, patience=2.0, num_hypotheses=2, confidences=True), "session", 528, 32,
    prevs=((), (5, 6, 7)), **_BEAM_STUB)
