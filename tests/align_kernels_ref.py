"""Float64 references, error bounds and crafted inputs for the word-timestamp alignment kernels
of csrc/align.hip, one kernel at a time (numpy only: no GPU, no torch).

Used by tests/test_align_kernels_ref_cpu.py (the references pinned to torch / transformers, and
the conditions the inputs must meet) and tests/test_gpu_align_kernels.py (the kernels, through
osw_debug_align_post / _tail / _self_attn / _scores).  The derivations of the bounds are in the
docstring of tests/test_gpu_align_kernels.py; `U` is the fp32 unit roundoff 2^-24.
"""
from __future__ import annotations

import numpy as np

import align_ref

U = 2.0 ** -24
HD = 64
EXP_ULP = 1.0      # HIP math API documentation: expf, maximum error 1 ulp (= 2 U relative)
LOG_ULP = 1.0      # logf: 1 ulp
SLACK = 1.001      # second-order terms of the first-order bounds below
FILL = 0xFFFFFFFF  # the debug entries' 0xff fill, as a 32-bit word
NEG = -2000.0      # a score whose exp underflows to exactly 0 in fp32 and in float64


# =========================================================================== post-processing
def softmax_stats(scores):
    """[..., TK] -> [..., 2]: the row maximum and sum(exp(x - max)) over all TK keys, float64."""
    x = np.asarray(scores, np.float64)
    m = x.max(-1)
    return np.stack([m, np.exp(x - m[..., None]).sum(-1)], -1)


def probs(scores, stats):
    """softmax over all TK keys from given (max, sum) statistics, float64."""
    x = np.asarray(scores, np.float64)
    st = np.asarray(stats, np.float64)
    return np.exp(x - st[..., :1]) / st[..., 1:2]


def colstats_from_probs(p):
    """p [H][P][F] -> [H][F][2]: mean and population std over the positions."""
    p = np.asarray(p, np.float64)
    mean = p.mean(-2)
    with np.errstate(invalid="ignore"):
        std = np.sqrt(((p - mean[..., None, :]) ** 2).mean(-2))
    return np.stack([mean, std], -1)


def colstats(scores, stats, P, F):
    """scores [H][>=P][TK], stats [H][>=P][2] -> [H][F][2]: mean and population std over positions
    0 .. P-1 of the probabilities cropped to F frames after a softmax over all TK keys."""
    return colstats_from_probs(probs(np.asarray(scores)[:, :P], np.asarray(stats)[:, :P])[..., :F])


def matrix_from_probs(p, cs, head, width):
    """p [H][P][F], cs [H][F][2] -> M [P - head - 1][F]: standardise, median-filter along the frames
    (align_ref.median_filter), mean over the heads, rows head .. P-2."""
    p = np.asarray(p, np.float64)
    cs = np.asarray(cs, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        z = (p - cs[:, None, :, 0]) / cs[:, None, :, 1]
    z = align_ref.median_filter(z, width)
    return z.mean(0)[head:p.shape[1] - 1]


def matrix(scores, stats, cs, P, F, head, width):
    """M [P - head - 1][F] from the scores and given softmax / column statistics."""
    p = probs(np.asarray(scores)[:, :P], np.asarray(stats)[:, :P])[..., :F]
    return matrix_from_probs(p, np.asarray(cs)[:, :F], head, width)


def matrix_full(scores, P, F, head, width):
    """The whole chain in float64 from the scores alone."""
    st = softmax_stats(np.asarray(scores)[:, :P])
    return matrix(scores, st, colstats(scores, st, P, F), P, F, head, width)


# ---- bounds (test_gpu_align_kernels.py docstring)
def sum_depth(n):
    """Roundings on the longest path of block_sum over n terms: a thread's own ceil(n/256) - 1 adds,
    6 levels of the wave tree, 3 adds over the waves."""
    return max(0, (n + 255) // 256 - 1) + 9


def stats_sum_rel_bound(scores):
    """Relative bound on the fp32 sum of exp(x - max) of each row [..., n] -> [...]."""
    x = np.asarray(scores, np.float64)
    d = x.max(-1, keepdims=True) - x
    w = np.exp(-d)
    dbar = (w * d).sum(-1) / w.sum(-1)     # the rounding of x - m, weighted by the terms
    return (sum_depth(x.shape[-1]) + 2 * EXP_ULP + dbar) * U * SLACK


def prob_abs_bound(scores, stats):
    """|p_fp32 - p| per element for p = expf(x - m) / s from the given fp32 m and s: the rounding of
    x - m (|x - m| U in the exponent), expf, one division."""
    x = np.asarray(scores, np.float64)
    st = np.asarray(stats, np.float64)
    return probs(x, st) * (np.abs(x - st[..., :1]) + 2 * EXP_ULP + 1) * U * SLACK


def colstats_bounds(scores, stats, P, F):
    """(|mean error|, |std error|) [H][F] of the sequential fp32 column statistics."""
    x = np.asarray(scores, np.float64)[:, :P]
    st = np.asarray(stats, np.float64)[:, :P]
    p = probs(x, st)[..., :F]
    ep = prob_abs_bound(x, st)[..., :F]
    mean = p.mean(-2)
    tol_mean = (P * U * mean + ep.mean(-2)) * SLACK
    d = np.abs(p - mean[:, None, :])
    ss = (d * d).sum(-2)
    eta = ep + tol_mean[:, None, :] + U * d
    dss = (2 * d * (ep + U * d) + eta * eta).sum(-2) + (P + 1) * U * ss
    std = np.sqrt(ss / P)
    with np.errstate(invalid="ignore", divide="ignore"):
        tol_std = np.where(ss > 0, std * (0.5 * dss / ss + U) * SLACK, np.sqrt(dss / P))
    return tol_mean, tol_std


def _window_max(b, width):
    """max over each frame's median window (reflect padding) of b [..., F], NaNs ignored."""
    F = b.shape[-1]
    pad = width // 2
    b = np.where(np.isnan(b), 0.0, b)
    if F <= pad:
        return b
    pb = np.pad(b, [(0, 0)] * (b.ndim - 1) + [(pad, pad)], mode="reflect")
    return np.lib.stride_tricks.sliding_window_view(pb, width, axis=-1).max(-1)


def matrix_bound(scores, stats, cs, P, F, head, width, end_to_end=False):
    """Per-element bound [P - head - 1][F] on |M_fp32 - M| given the same stats and colstats.
    end_to_end: against the float64 chain from the scores alone (adds the statistics' own errors)."""
    x = np.asarray(scores, np.float64)[:, :P]
    st = np.asarray(stats, np.float64)[:, :P]
    cs = np.asarray(cs, np.float64)[:, :F]
    p = probs(x, st)[..., :F]
    ep = prob_abs_bound(x, st)[..., :F]
    mean, std = cs[:, None, :, 0], cs[:, None, :, 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        bz = (ep + 2 * U * (p + np.abs(mean))) / std * SLACK
        z = (p - mean) / std
        if end_to_end:
            tm, ts = colstats_bounds(scores, stats, P, F)
            rs = stats_sum_rel_bound(x)[..., None]
            tm = tm + (p * rs).mean(-2)                       # the sums' errors, through every p
            ts = ts + cs[..., 1] * rs.max()
            bz = bz + (p * rs + tm[:, None, :]) / std + np.abs(z) * ts[:, None, :] / std
    bz = np.where(np.isfinite(bz), bz, np.nan)
    bw = _window_max(bz, width).max(0)                       # over the window, then over the heads
    H = x.shape[0]
    head_mean = H * U * _window_max(np.where(np.isfinite(z), np.abs(z), 0.0), width).mean(0)  # H roundings
    return (bw + head_mean * SLACK)[head:P - 1]


# =========================================================================== tail
def tail_logprob(logits, eot, tok):
    """log softmax(logits[:eot])[tok] in float64."""
    x = np.asarray(logits, np.float64)[:eot]
    m = x.max()
    return float(np.asarray(logits, np.float64)[tok] - m - np.log(np.exp(x - m).sum()))


def tail_bound(logits, eot, tok):
    """|(lg[tok] - m) - logf(s)| error: the two subtractions, the relative error of s, logf."""
    x = np.asarray(logits, np.float64)[:eot]
    m = x.max()
    s = np.exp(x - m).sum()
    a = abs(float(np.asarray(logits, np.float64)[tok]) - m)
    res = a + np.log(s)
    return float((U * a + stats_sum_rel_bound(x) / SLACK + 2 * LOG_ULP * U * np.log(s) + U * res) * SLACK)


def tail_expected(pos, slot, length, head, forced, token_logprob, cur_tok, done, logits, eot):
    """What one launch_align_tail at `pos` leaves: (token_logprob, written mask, cur_tok, done)."""
    lp = np.array(token_logprob, np.float64)
    wr = np.zeros(lp.shape, bool)
    ct, dn = np.array(cur_tok), np.array(done)
    for r in range(len(slot)):
        L = int(length[r])
        if slot[r] < 0 or pos >= L:
            continue
        if head[r] <= pos <= L - 3:
            lp[slot[r], pos - head[r]] = tail_logprob(logits[r], eot, int(forced[r, pos + 1]))
            wr[slot[r], pos - head[r]] = True
        if pos + 1 < L:
            ct[r] = forced[r, pos + 1]
        else:
            dn[r] = 1
    return lp, wr, ct, dn


# =========================================================================== self-attention
def reduce_inorder(slabs, bias):
    """bias + slab 0 + slab 1 + ... in fp32, in index order (align_self_attn_kernel)."""
    v = np.array(bias, np.float32)
    v = np.broadcast_to(v, np.asarray(slabs).shape[1:]).copy()
    for s in np.asarray(slabs, np.float32):
        v = (v + s).astype(np.float32)
    return v


def self_attn(qkv_slabs, bias, kcache, vcache, pos, done):
    """One step of the forced pass's fp32 self-attention.  Returns (out float64 [rows][D] (NaN for
    done rows), kcache', vcache' fp32 with k and v of the live rows written at min(pos, ctx - 1))."""
    r = reduce_inorder(qkv_slabs, bias)
    rows, D3 = r.shape
    D = D3 // 3
    H = D // HD
    kc, vc = np.array(kcache, np.float32), np.array(vcache, np.float32)
    p = min(int(pos), kc.shape[2] - 1)
    out = np.full((rows, D), np.nan)
    for b in range(rows):
        if done[b]:
            continue
        kc[b, :, p] = r[b, D:2 * D].reshape(H, HD)
        vc[b, :, p] = r[b, 2 * D:].reshape(H, HD)
        for h in range(H):
            q = r[b, h * HD:(h + 1) * HD].astype(np.float64)
            s = kc[b, h, :p + 1].astype(np.float64) @ q * 0.125
            w = np.exp(s - s.max())
            out[b, h * HD:(h + 1) * HD] = (w @ vc[b, h, :p + 1].astype(np.float64)) / w.sum()
    return out, kc, vc


def self_attn_bound(qkv_slabs, bias, kcache, vcache, pos, done):
    """Per-element bound [rows][D] on |hi + lo - out| (NaN for done rows)."""
    r = reduce_inorder(qkv_slabs, bias).astype(np.float64)
    ref, kc, vc = self_attn(qkv_slabs, bias, kcache, vcache, pos, done)
    rows, D3 = r.shape
    D = D3 // 3
    H = D // HD
    p = min(int(pos), kc.shape[2] - 1)
    n = p + 1
    out = np.full((rows, D), np.nan)
    for b in range(rows):
        if done[b]:
            continue
        for h in range(H):
            q = r[b, h * HD:(h + 1) * HD]
            k = kc[b, h, :n].astype(np.float64)
            v = vc[b, h, :n].astype(np.float64)
            s = k @ q * 0.125
            ds = HD * U * (np.abs(k) @ np.abs(q)) * 0.125       # 64 sequential fmas
            d = s.max() - s
            w = np.exp(-d)
            e = ds + ds[np.argmax(s)] + U * d + 2 * EXP_ULP * U  # each weight, relative
            pw = w / w.sum()
            a = pw @ np.abs(v)
            # the weights' errors in numerator and denominator, the sum l, the 4-way P V sums, the division
            rel = 2 * e.max() + (sum_depth(n) + (n + 3) // 4 + 3 + 1) * U
            out[b, h * HD:(h + 1) * HD] = rel * a * SLACK
    return out + 2.0 ** -22 * np.abs(ref) + 2.0 ** -25          # the fp16 hi + lo pair


# =========================================================================== scores
def reduce_head(slabs, bias):
    """headreduce.h reduce_head in fp32 numpy: wave w sums slabs w, w+4, ... as pairs (s, s+4), then
    bias + (((w0 + w1) + w2) + w3), rounded to fp16."""
    f = np.float32
    part = np.asarray(slabs, f)
    ks = part.shape[0]
    red = []
    for w in range(4):
        v = np.zeros(part.shape[1:], f)
        s = w
        while s + 4 < ks:
            v = (v + (part[s] + part[s + 4]).astype(f)).astype(f)
            s += 8
        if s < ks:
            v = (v + part[s]).astype(f)
        red.append(v)
    r = np.zeros(part.shape[1:], f) if bias is None else np.broadcast_to(np.asarray(bias, f), part.shape[1:]).copy()
    r = (r + (((red[0] + red[1]).astype(f) + red[2]).astype(f) + red[3]).astype(f)).astype(f)
    return r.astype(np.float16)


def scores(q_slabs, bias, K, layer_heads, n_heads, pos, slot, length, scores_in):
    """One launch_align_scores: (scores float64, written mask, bound) from scores_in
    [slots][n_heads][pstride][T]."""
    q16 = reduce_head(q_slabs, bias).astype(np.float64)
    K = np.asarray(K, np.float64)
    out = np.array(scores_in, np.float64)
    wr = np.zeros(out.shape, bool)
    bound = np.zeros(out.shape)
    for b in range(q16.shape[0]):
        if slot[b] < 0 or pos >= length[b]:
            continue
        for h, hi in np.asarray(layer_heads).reshape(-1, 2):
            q = q16[b, h * HD:(h + 1) * HD]
            out[slot[b], hi, pos] = K[b, h] @ q * 0.125
            bound[slot[b], hi, pos] = HD * U * (np.abs(K[b, h]) @ np.abs(q)) * 0.125
            wr[slot[b], hi, pos] = True
    return out, wr, bound


# =========================================================================== crafted post cases
def _case(name, TK, slots, n_heads, sc, degenerate=False, **kw):
    """slots: (len, head, frames, width) per slot; sc fp32 [slots][heads][pstride][TK]."""
    return dict(name=name, TK=TK, slots=slots, n_heads=n_heads, scores=np.asarray(sc, np.float32),
                pstride=sc.shape[2], degenerate=degenerate, **kw)


HEAD_SCALES = (1.0, 3.0, 0.25, 6.0, 0.05, 2.0)   # heads of very different scale


def _random_scores(rng, slots, n_heads, TK, pstride, quantum=None):
    """Peaked rows: N(0, scale_h) noise, a peak of +4 .. +12 on one key per row, and for F < TK the
    largest scores (+14 .. +16) on keys >= F, so that cropping before the softmax changes every
    probability.  Rows p >= len hold NaN."""
    sc = np.full((len(slots), n_heads, pstride, TK), np.nan, np.float32)
    for s, (P, hd, F, W) in enumerate(slots):
        for h in range(n_heads):
            x = rng.standard_normal((P, TK)) * HEAD_SCALES[h % len(HEAD_SCALES)]
            x[np.arange(P), rng.integers(0, F, P)] += rng.uniform(4, 12, P)
            if F < TK:
                nb = min(3, TK - F)
                for i in range(P):
                    x[i, F + rng.choice(TK - F, nb, replace=False)] = x[i, :F].max() + rng.uniform(14, 16, nb)
            if quantum:
                x = np.round(x / quantum) * quantum
            sc[s, h, :P] = x
    return sc


def _pstride(slots):
    return max(16, (max(s[0] for s in slots) + 15) // 16 * 16)


def random_case(name, TK, slots, n_heads, seed, **kw):
    rng = np.random.default_rng(seed)
    ps = kw.pop("pstride", None) or _pstride(slots)
    return _case(name, TK, slots, n_heads, _random_scores(rng, slots, n_heads, TK, ps, kw.pop("quantum", None)), **kw)


WIDTHS = (1, 3, 5, 7, 9, 15)
TKS = (1, 7, 255, 256, 257, 300, 1500)
FS = (1, 2, 3, 4, 7, 255, 256, 257)


def post_cases():
    """Every single-launch case of the post-processing tests, by name."""
    cases = []
    seed = 100
    # each width at F = W/2 (unfiltered) and W/2 + 1 (the smallest filtered F), F < TK
    for W in WIDTHS:
        for F in (W // 2, W // 2 + 1):
            if F >= 1:
                seed += 1
                cases.append(random_case(f"w{W}_F{F}", 300, [(9, 3, F, W)], 2, seed))
    # F == TK over the TK list (TK 1: a softmax over one key, every column constant)
    for TK in TKS:
        seed += 1
        cases.append(random_case(f"tk{TK}_full", TK, [(12, 3, TK, 7)], 2, seed, degenerate=TK == 1))
    # F < TK over the F list (F <= 3 is unfiltered at width 7)
    for F in FS:
        seed += 1
        cases.append(random_case(f"tk300_F{F}", 300, [(10, 1, F, 7)], 1, seed))
    cases.append(random_case("tk1500_F257_w15", 1500, [(7, 3, 257, 15)], 2, 131))
    cases.append(random_case("heads6", 300, [(20, 3, 120, 7)], 6, 132))
    # exact ties inside a median window: duplicated columns
    c = random_case("ties", 64, [(12, 3, 40, 7)], 2, 133)
    c["scores"][..., 11] = c["scores"][..., 12] = c["scores"][..., 10]
    c["scores"][..., 21] = c["scores"][..., 20]
    c["scores"][..., 39] = c["scores"][..., 38] = c["scores"][..., 0]
    cases.append(c)
    cases.append(ramp_case())
    cases.append(peaked_case(False))
    cases.append(peaked_case(True))
    cases.append(random_case("long", 1500, [(448, 3, 1500, 7)], 2, 134))
    cases.extend(degenerate_cases())
    return cases


def ramp_case():
    """Every row's probability is strictly monotone along the frames (slope c_p, rising or falling),
    with a little noise: a reflect index that is off by one changes the first and last W/2
    outputs (checked on the reference in the CPU test)."""
    rng = np.random.default_rng(140)
    P, F, TK = 14, 48, 48
    c = np.linspace(-3.0, 3.0, P) + 0.2
    x = c[:, None] * np.arange(F)[None, :] / 8.0 + rng.standard_normal((P, F)) * 0.02
    sc = np.full((1, 2, 16, TK), np.nan, np.float32)
    sc[0, 0, :P] = x
    sc[0, 1, :P] = 0.5 * x[::-1] + rng.standard_normal((P, F)) * 0.02
    return _case("ramp", TK, [(P, 3, F, 9)], 2, sc)


def peaked_case(offset):
    """Score differences up to 60 within a row (exp still normal in fp32), on a grid of 1/64 so that
    adding 1e4 to a row is exact in fp32; offset: rows 2 and 5 of both heads carry the +1e4."""
    rng = np.random.default_rng(141)
    P, TK = 12, 300
    sc = np.full((1, 2, 16, TK), np.nan, np.float32)
    for h in range(2):
        x = rng.uniform(-8, 0, (P, TK))
        x[np.arange(P), rng.integers(0, TK, P)] = rng.uniform(20, 52, P)
        x[:, rng.integers(0, TK, 6)] += rng.uniform(0, 8, (P, 6))
        x = np.round(np.clip(x, -8, 52) * 64) / 64
        if offset:
            x[[2, 5]] += 1e4
        sc[0, h, :P] = x
    return _case("peaked_offset" if offset else "peaked", TK, [(P, 3, TK, 7)], 2, sc)


def nan_mask_case():
    """Exact zero-variance columns.  Head 0's scores are 0 or NEG (exp exactly 0), eight zeros per
    row, so every probability is exactly 0 or 2^-3 in fp32 and in float64, every column sum is
    exact, and a column on which all positions agree has mean == p and std == 0: 0/0 = NaN in the
    reference and in the kernel alike.  (Repeating an arbitrary score row does not do this: P
    copies of p do not sum to P p exactly, so the std is a rounding residue, not 0.)  The constant
    columns are {3}, {9, 10, 11}, {17 .. 20}, {26 .. 32}, so width-7 windows hold 0 to 7 NaNs;
    the other columns of head 0 vary over the positions; head 1 is an ordinary random head."""
    rng = np.random.default_rng(150)
    P, F, n1 = 12, 40, 8
    const = {3: 1, 9: 0, 10: 1, 11: 0, 17: 0, 18: 0, 19: 1, 20: 0}
    const.update({f: 0 for f in range(26, 33)})
    n_const1 = sum(const.values())
    free = [f for f in range(F) if f not in const]
    TK = F + n1
    bits = np.zeros((P, TK), bool)
    for f, b in const.items():
        bits[:, f] = bool(b)
    for i in range(P):
        k = int(rng.integers(1, n1 - n_const1))
        bits[i, rng.choice(free, k, replace=False)] = True
        bits[i, F:F + n1 - n_const1 - k] = True      # the rest of the eight, on cropped keys
    for f in free:                                    # no free column may be constant by accident
        if bits[:, f].all() or not bits[:, f].any():
            i = int(rng.integers(0, P))
            j = int(np.flatnonzero(bits[i, F:])[0]) + F if not bits[i, f] else int(np.flatnonzero(~bits[i, F:])[0]) + F
            bits[i, f], bits[i, j] = not bits[i, f], not bits[i, j]
    assert (bits.sum(1) == n1).all()
    sc = _random_scores(rng, [(P, 3, F, 7)], 2, TK, 16)
    sc[0, 0, :P] = np.where(bits, 0.0, NEG)
    return _case("nan_windows", TK, [(P, 3, F, 7)], 2, sc, degenerate=True, nan_columns=sorted(const))


def degenerate_cases():
    cases = [nan_mask_case()]
    # all scores equal over 256 keys: p = 2^-8 everywhere, every column has zero variance
    sc = np.full((1, 1, 16, 256), np.nan, np.float32)
    sc[0, 0, :8] = 1.5
    cases.append(_case("all_equal", 256, [(8, 3, 100, 7)], 1, sc, degenerate=True))
    # the same, at width 15 through the generic path with its +inf padding
    c = nan_mask_case()
    c["name"] = "nan_windows_w15"
    c["slots"] = [(12, 3, 40, 15)]
    cases.append(c)
    c = nan_mask_case()
    c["name"] = "nan_windows_w3"
    c["slots"] = [(12, 3, 40, 3)]
    cases.append(c)
    return cases


def multi_slot_cases():
    """Three slots per launch that differ in len (head + 3, exactly pstride, a non-multiple), head,
    frames and width; rows p >= len hold NaN."""
    a = [(4, 1, 5, 3), (16, 3, 64, 7), (11, 3, 2, 5)]
    b = [(6, 3, 300, 15), (32, 1, 17, 9), (21, 3, 8, 15)]
    return [random_case("multi16", 64, a, 2, 160, pstride=16), random_case("multi32", 300, b, 3, 161, pstride=32)]


def single_slot(case, s):
    """Slot s of a multi-slot case as a launch of its own (same pstride)."""
    return _case(f"{case['name']}[{s}]", case["TK"], [case["slots"][s]], case["n_heads"], case["scores"][s:s + 1])


def live_masks(case):
    """Boolean masks of the elements a launch must write: (stats, colstats, M)."""
    S, H, ps, TK = case["scores"].shape
    st = np.zeros((S, H, ps, 2), bool)
    cs = np.zeros((S, H, TK, 2), bool)
    M = np.zeros((S, ps, TK), bool)
    for s, (P, hd, F, W) in enumerate(case["slots"]):
        st[s, :, :P] = True
        cs[s, :, :F] = True
        M[s, :P - hd - 1, :F] = True
    return st, cs, M


# =========================================================================== crafted tail / attention / score inputs
TAIL_EOTS = (1, 5, 255, 256, 257, 1000)
TAIL_CTX = 24
TAIL_FILL_TOK = -7


def tail_case(eot, head):
    """Four rows over three slots: row 0 (slot 0, len 10) whose odd forced positions hold a token
    200 below the row maximum (eot >= 5), row 1 not aligned (slot -1), row 2 (slot 2) of len
    head + 3 (one text token), row 3 (slot 1, len 7).  Logits at indices >= eot sit 500 above
    everything else, the one at eot - 1 half a nat below the row maximum.  Launch it at every pos in TAIL_POSITIONS from the fill state."""
    rng = np.random.default_rng(1000 + 7 * eot + head)
    V, rows = eot + 7, 4
    logits = (rng.standard_normal((rows, V)) * 2).astype(np.float32)
    logits[:, eot:] = 500.0 + rng.uniform(0, 1, (rows, 7))
    forced = rng.integers(0, eot, (rows, TAIL_CTX)).astype(np.int32)
    if eot >= 5:
        logits[:, eot - 1] = logits[:, :eot - 1].max(1) - 0.5      # the last logit of the sum carries weight
        far = eot - 2
        forced[0, 1::2] = far
        logits[0, far] = logits[0, :eot].max() - 200.0
    slot = np.array([0, -1, 2, 1], np.int32)
    length = np.array([10, 10, head + 3, 7], np.int32)
    return dict(logits=logits, eot=eot, forced=forced, slot=slot, length=length,
                head=np.full(rows, head, np.int32), n_slots=3)


TAIL_POSITIONS = tuple(range(0, 11))


def tail_fill(case):
    """(token_logprob, cur_tok, done) before a launch: the 0xff pattern, a marker token, zeros."""
    lp = np.full((case["n_slots"], TAIL_CTX), FILL, np.uint32).view(np.float32)
    return lp, np.full(len(case["slot"]), TAIL_FILL_TOK, np.int32), np.zeros(len(case["slot"]), np.int32)


SELF_CTX = 448
SELF_POSITIONS = (0, 1, 3, 255, 256, 257, 447, 460)   # 460: past ctx - 1, clamped to 447


def order_slabs(target, ks, rng, big=(500.0, 4000.0)):
    """fp32 slabs [ks][...] whose sum is about `target` and depends on the order of the additions
    (ks >= 3): slab 1 carries +big and the last slab -big, so whatever is added while big is in the
    running sum is rounded to big's grid; slab 0 carries the target, the others small values."""
    t = np.asarray(target, np.float64)
    if ks == 1:
        return t[None].astype(np.float32)
    assert ks >= 3
    slabs = (rng.standard_normal((ks,) + t.shape) * 0.3).astype(np.float32)
    b = rng.uniform(big[0], big[1], t.shape).astype(np.float32)
    slabs[1], slabs[-1] = b, -b
    slabs[0] = t - slabs[2:-1].astype(np.float64).sum(0)
    return slabs


def self_attn_case(pos, H, ks):
    """Three rows: row 0 peaked (cached keys 0, 255, 256 and the new key score ~36 nats above the
    rest), row 1 done (must stay untouched), row 2 near-uniform.  Cache positions the step must
    not read (beyond min(pos, ctx - 1)) hold NaN."""
    rng = np.random.default_rng(2000 + 31 * pos + 7 * H + ks)
    rows, D, ctx = 3, H * HD, SELF_CTX
    p = min(pos, ctx - 1)
    kc = (rng.standard_normal((rows, H, ctx, HD)) * 0.3).astype(np.float32)
    vc = rng.uniform(-1, 1, (rows, H, ctx, HD)).astype(np.float32)
    tgt = rng.standard_normal((rows, 3 * D)) * 0.3
    for h in range(H):
        e = (rng.integers(0, 2, HD) * 2 - 1) / 8.0
        for key in (0, 255, 256):
            kc[0, h, key] += (6.0 * e).astype(np.float32)
        tgt[0, h * HD:(h + 1) * HD] += 48.0 * e
        tgt[0, D + h * HD:D + (h + 1) * HD] += 6.0 * e
    kc[:, :, p + 1:] = np.nan
    vc[:, :, p + 1:] = np.nan
    bias = rng.uniform(-1, 1, 3 * D).astype(np.float32)
    slabs = order_slabs(tgt - bias, ks, rng)
    return dict(slabs=slabs, bias=bias, kc=kc, vc=vc, pos=pos, done=np.array([0, 1, 0], np.int32))


SCORE_TS = (1, 255, 256, 257, 300)
SCORE_KS = (1, 4, 5, 9)
SCORE_PSTRIDE = 16
SCORE_LAYER_HEADS = ((4, 2), (0, 0))    # heads {4, 0} -> head_idx {2, 0} of n_heads 3; head_idx 1 keeps its fill


def scores_case(T, ks, with_bias, pos):
    """Four rows with H = 6: row 0 -> slot 1 with unit-vector keys (key j of every head is e_(j % 64),
    so each score is exactly q[j % 64] / 8), row 1 not aligned (slot -1), row 2 -> slot 0 with
    len == pos (pos >= len: untouched), row 3 -> slot 2 with random keys."""
    rng = np.random.default_rng(3000 + 13 * T + ks + 100 * pos + (1 if with_bias else 0))
    rows, H = 4, 6
    D = H * HD
    K = rng.uniform(-2, 2, (rows, H, T, HD)).astype(np.float16)
    K[0] = 0
    K[0, :, np.arange(T), np.arange(T) % HD] = 1.0
    q = rng.uniform(-30, 30, (rows, D))
    bias = rng.uniform(-1, 1, D).astype(np.float32) if with_bias else None
    slabs = order_slabs(q - (bias if with_bias else 0.0), ks, rng, big=(2.0 ** 17, 2.0 ** 19))   # big's grid ~ fp16's at |q| ~ 30
    slot = np.array([1, -1, 0, 2], np.int32)
    length = np.array([SCORE_PSTRIDE, SCORE_PSTRIDE, pos, SCORE_PSTRIDE], np.int32)
    sc = np.full((3, 3, SCORE_PSTRIDE, T), FILL, np.uint32).view(np.float32)
    return dict(slabs=slabs, bias=bias, K=K, layer_heads=np.array(SCORE_LAYER_HEADS, np.int32), n_heads=3, pos=pos,
                slot=slot, length=length, scores=sc)
