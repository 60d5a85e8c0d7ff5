"""Float64 references, crafted inputs and scheme emulations for the attention kernels.

Used by tests/test_attn_ref_cpu.py (generator conditions and the sensitivity of the bounds,
no GPU) and tests/test_gpu_attention.py (the kernels themselves, one launch per call
through osw_debug_enc_attn / osw_debug_dec_xattn / osw_debug_dec_self_attn).

The references are softmax(Q Kᵀ / 8) V in float64 from the same fp16 Q, K and V the kernels
get.  No rounding model is needed: the encoder kernel is handed Q, K and V directly, and the
decoder kernels reduce split-K slabs whose values are multiples of 2^-8 bounded by 64, so
every partial sum is exact in fp32 whatever the order, and each reduced q, k and v is built
to be an fp16 value (`split_slabs`).  What is left between a kernel and its reference is the
kernel's own arithmetic, which is what the bounds are derived for:

  encoder   |out - ref| <= 2^-9 max|V|: the fp16 P operand of the PV MFMA contributes at most
            2^-11 max|V| (relative 2^-11 per weight, the weights sum to 1), the fp16 output at
            most 2^-10 |out| (one half-even rounding with the fused fp32 normalisation), fp32
            accumulation noise on top: 2^-11 + 2^-10 + noise < 2^-9.
  decoder   the outputs are fp16 hi/lo pairs (~22 bits) of an fp32 evaluation with hardware
            exp: `decoder_tolerance` measures a plain float32 numpy evaluation of the same
            formula against the float64 reference on the same inputs and allows the GPU 8x
            that error (other summation order, v_exp_f32), floored at 1e-5 max|V|.

The emulations restate each kernel's scheme (key tiles / key chunks with partials and a merge,
clamped loads past the end) so the CPU tests can break it the ways a kernel could be broken
(no tail mask, no O rescale, merge without its exp factor) and show that the crafted inputs
push each break past the bound by orders of magnitude, while on near-uniform inputs, all the
suite had before, the same breaks vanish or move the output by a few percent of max|V|.
"""
from __future__ import annotations

import numpy as np

T_ENC = 1500
HD = 64
ENC_KB = 64                 # attn.hip: keys per tile
LOG2E = 1.4426950408889634
ENC_CS = 0.125 * LOG2E      # attn.hip: 1/sqrt(64) * log2(e), the base-2 score scale
XCH = 8                     # decode.h XCHUNKS
XPER = (T_ENC + XCH - 1) // XCH   # decode.hip: keys per cross-attention chunk (188; the last holds 184)
XKEYS = 192                 # decode.hip: key slots a chunk workgroup loads (clamped past the chunk's end)
ENC_MID_KEY = 700           # the mid key tied with key 1499 in the encoder inputs
# chunk edges of the cross-attention kernels (188-key chunks: 187 | 188, 1315 | 1316), the
# 192-key slot edges (191 | 192, 1343 | 1344) and both ends
X_MARKERS = (0, 187, 188, 191, 192, 1315, 1316, 1343, 1344, 1499)
SELF_NKEYS = (1, 2, 33, 255, 256, 257, 447, 448)


def _rng(seed):
    return np.random.default_rng(seed)


def _direction(rng):
    """A unit vector with entries +-1/8 (exact in fp16)."""
    return (rng.integers(0, 2, HD) * 2 - 1).astype(np.float64) / 8.0


def _orthogonal(e, rng):
    """A second +-1/8 unit vector orthogonal to e (half of the signs flipped)."""
    idx = rng.permutation(HD)[: HD // 2]
    f = e.copy()
    f[idx] = -f[idx]
    assert abs(f @ e) < 1e-12
    return f


# --------------------------------------------------------------------------- references
def softmax_attend(q, K, V):
    """float64 softmax(q Kᵀ / 8) V; q [..., 64], K and V [n][64]."""
    s = np.asarray(q, np.float64) @ np.asarray(K, np.float64).T * 0.125
    s -= s.max(-1, keepdims=True)
    p = np.exp(s)
    return (p @ np.asarray(V, np.float64)) / p.sum(-1, keepdims=True)


def enc_attn_ref(qkv):
    """qkv fp16 [3][nb][H][T][64] -> float64 [nb*T][H*64] (the kernel's output layout)."""
    _, nb, H, T, _ = qkv.shape
    out = np.empty((nb * T, H * HD), np.float64)
    for b in range(nb):
        for h in range(H):
            out[b * T:(b + 1) * T, h * HD:(h + 1) * HD] = softmax_attend(qkv[0, b, h], qkv[1, b, h], qkv[2, b, h])
    return out


def reduce_slabs(slabs, bias):
    """bias + the sum of the split-K slabs, exact (float64), as the fp16 value the kernels round to."""
    r = np.asarray(slabs, np.float64).sum(0)
    if bias is not None:
        r = r + np.asarray(bias, np.float64)
    r16 = r.astype(np.float16)
    assert np.array_equal(r16.astype(np.float64), r), "the reduced value must be an fp16 value"
    return r16


def xattn_ref(q_slabs, bias, K, V, beam, dtype=np.float64, attend=None):
    """q_slabs [ks][rows][D], K and V fp16 [W][H][1500][64] -> [rows][D]."""
    attend = attend or softmax_attend
    q = reduce_slabs(q_slabs, bias)
    rows, D = q.shape
    H = D // HD
    out = np.empty((rows, D), dtype)
    for r in range(rows):
        for h in range(H):
            out[r, h * HD:(h + 1) * HD] = attend(q[r, h * HD:(h + 1) * HD], K[r // beam, h], V[r // beam, h])
    return out


def self_attn_ref(qkv_slabs, bias, kcache, vcache, pos, ancestry=None, attend=None, dtype=np.float64):
    """One self-attention step.  Returns (out [rows][D], kcache', vcache'): the caches with fp16 k
    and v of each row written at its position, everything else untouched."""
    attend = attend or softmax_attend
    r16 = reduce_slabs(qkv_slabs, bias)
    rows, D3 = r16.shape
    D = D3 // 3
    H = D // HD
    posv = np.broadcast_to(np.asarray(pos, np.int64), (rows,))
    kc, vc = np.array(kcache, np.float16), np.array(vcache, np.float16)
    for r in range(rows):
        kc[r, :, posv[r]] = r16[r, D:2 * D].reshape(H, HD)
        vc[r, :, posv[r]] = r16[r, 2 * D:].reshape(H, HD)
    out = np.empty((rows, D), dtype)
    for r in range(rows):
        n = int(posv[r]) + 1
        src = np.full(n, r) if ancestry is None else np.append(np.asarray(ancestry)[r, :n - 1], r)
        for h in range(H):
            out[r, h * HD:(h + 1) * HD] = attend(r16[r, h * HD:(h + 1) * HD], kc[src, h, np.arange(n)],
                                                 vc[src, h, np.arange(n)])
    return out, kc, vc


def attend_f32(q, K, V):
    """The same formula evaluated in float32 throughout (numpy): the decoder bound's yardstick."""
    f = np.float32
    s = (np.asarray(q, f) @ np.asarray(K, f).T) * f(0.125)
    p = np.exp(s - s.max(-1, keepdims=True), dtype=f)
    return (p @ np.asarray(V, f)) / p.sum(-1, keepdims=True, dtype=f)


def decoder_tolerance(ref64, eval32, vmax):
    """(tolerance, float32 evaluation's error): 8x the error of the float32 numpy evaluation of
    the same inputs, floored at 1e-5 max|V|."""
    e32 = float(np.abs(np.asarray(eval32, np.float64) - ref64).max())
    return max(8.0 * e32, 1e-5 * float(vmax)), e32


def enc_tolerance(V):
    return 2.0 ** -9 * float(np.abs(np.asarray(V, np.float32)).max())


# --------------------------------------------------------------------------- crafted inputs
ENC_GAIN = 64.0


def enc_inputs(nb, H, seed=0):
    """qkv fp16 [3][nb][H][1500][64] with q = gamma_t e + noise, k = rho_u e + noise:
    rho ramps by +1 per 64-key tile (0 .. 23) with rho[700] = rho[1499] = 30, and the query
    gains gamma are spread over [-64, 64] in no order, so neighbouring queries (the lanes of
    one wave) climb at different rates.  Scores are gamma rho / 8: a positive gain raises the
    running max tile after tile and jumps at key 700's tile, a negative one peaks in tile 0."""
    rng = _rng(1000 + seed)
    qkv = np.empty((3, nb, H, T_ENC, HD), np.float16)
    rho = (np.arange(T_ENC) // ENC_KB).astype(np.float64)
    rho[ENC_MID_KEY] = rho[T_ENC - 1] = 30.0
    for b in range(nb):
        for h in range(H):
            e = _direction(rng)
            gamma = rng.uniform(-ENC_GAIN, ENC_GAIN, T_ENC)
            qkv[0, b, h] = gamma[:, None] * e + rng.uniform(-0.125, 0.125, (T_ENC, HD))
            qkv[1, b, h] = rho[:, None] * e + rng.uniform(-0.125, 0.125, (T_ENC, HD))
            qkv[2, b, h] = rng.uniform(-1.0, 1.0, (T_ENC, HD))
    return qkv


def uniform_enc_inputs(nb, H, seed=0):
    """Near-uniform attention, as the random-weight fixtures give: |q k / 8| stays below 0.9."""
    rng = _rng(2000 + seed)
    qkv = rng.uniform(-0.6, 0.6, (3, nb, H, T_ENC, HD)).astype(np.float16)
    qkv[2] = rng.uniform(-1.0, 1.0, qkv[2].shape).astype(np.float16)
    return qkv


def enc_trace(q, k):
    """The lazy running-max rule of enc_attn_kernel on the reference's own scores of one head
    (base-2 domain, float64).  Per query: raises after tile 0, the largest stale excess (a tile
    max above the kept running max), the largest jump of a raise after tile 0; and the number of
    (16-query group, tile) pairs whose lanes disagree on raising."""
    s2 = np.asarray(q, np.float64) @ np.asarray(k, np.float64).T * ENC_CS
    T = s2.shape[0]
    nkt = (s2.shape[1] + ENC_KB - 1) // ENC_KB
    mrun = np.full(T, -np.inf)
    raises = np.zeros(T, np.int64)
    stale = np.zeros(T)
    jump = np.zeros(T)
    disagree = 0
    for kt in range(nkt):
        mx = s2[:, kt * ENC_KB:(kt + 1) * ENC_KB].max(1)
        up = mx - mrun > 8.0
        if kt:
            raises += up
            stale = np.maximum(stale, np.where(up, 0.0, mx - mrun))
            jump = np.maximum(jump, np.where(up, mx - mrun, 0.0))
            pad = np.zeros((T + 15) // 16 * 16, bool)
            pad[:T] = up
            full = np.ones_like(pad)
            full[T:] = False
            g = pad.reshape(-1, 16).sum(1)
            n = full.reshape(-1, 16).sum(1)
            disagree += int(((g > 0) & (g < n)).sum())
        mrun = np.where(up, mx, mrun)
    return {"raises": raises, "stale": stale, "jump": jump, "disagree": disagree,
            "smax": float(np.abs(s2).max())}


def split_slabs(target, ks, rng, with_bias=True):
    """Split-K slabs [ks][...] and a bias whose exact sum is `target` (multiples of 2^-8 that are
    fp16 values, |target| <= 44): every slab value is a multiple of 2^-8 bounded by 64."""
    t = np.asarray(target, np.float64)
    assert np.array_equal(t * 256, np.round(t * 256)) and np.abs(t).max() <= 44.0
    assert np.array_equal(t.astype(np.float16).astype(np.float64), t)
    bias = np.round(rng.uniform(-1, 1, t.shape[-1]) * 256) / 256 if with_bias else None
    a = min(2.0, 18.0 / ks)   # the last slab takes the remainder: |it| <= 44 + 1 + a (ks - 1) < 64
    slabs = np.round(rng.uniform(-a, a, (ks,) + t.shape) * 256) / 256
    slabs[-1] = t - slabs[:-1].sum(0) - (bias if with_bias else 0.0)
    assert np.abs(slabs).max() <= 64.0
    return slabs.astype(np.float32), (bias.astype(np.float32) if with_bias else None)


def _q16(x):
    """Round to a multiple of 2^-8 that is also an fp16 value."""
    return (np.round(np.asarray(x, np.float64) * 256) / 256).astype(np.float16).astype(np.float64)


X_ROW_KINDS = ("markers", "low", "far", "uniform")


def xattn_inputs(W, H, beam, ks, seed=0, with_bias=True):
    """Cross-attention inputs.  K of a (window, head) is rho_u e + 5 f + noise (e, f orthonormal):
    rho = 4 at the marker keys X_MARKERS, -4 on chunk 3 (keys 564 .. 751), 0 elsewhere.  Row r's q
    is one of four kinds (r + head, cycling):
      markers  q = 320 e: the markers score 160 nats, near-tied, every other chunk's max lies
               >= 100 nats below (its merge factor underflows to 0);
      low      q = -320 e: chunk 3 alone carries the softmax, the markers sit at -160;
      far      q = -320 f: every score is near -200;
      uniform  q = noise: near-uniform weights (the baseline).
    Returns (q_slabs [ks][rows][D], bias [D] or None, K, V, kinds [rows][H])."""
    rng = _rng(3000 + seed)
    rows, D = W * beam, H * HD
    K = np.empty((W, H, T_ENC, HD), np.float16)
    V = rng.uniform(-1.0, 1.0, (W, H, T_ENC, HD)).astype(np.float16)
    rho = np.zeros(T_ENC)
    rho[3 * XPER:4 * XPER] = -4.0
    rho[list(X_MARKERS)] = 4.0
    q = np.empty((rows, D))
    kinds = np.empty((rows, H), dtype=object)
    for w in range(W):
        for h in range(H):
            e = _direction(rng)
            f = _orthogonal(e, rng)
            K[w, h] = rho[:, None] * e + 5.0 * f + rng.uniform(-1 / 64, 1 / 64, (T_ENC, HD))
            for b in range(beam):
                r = w * beam + b
                kind = X_ROW_KINDS[(r + h) % 4]
                kinds[r, h] = kind
                base = {"markers": 320.0 * e, "low": -320.0 * e, "far": -320.0 * f, "uniform": 0.0 * e}[kind]
                q[r, h * HD:(h + 1) * HD] = base + rng.uniform(-0.25, 0.25, HD)
    slabs, bias = split_slabs(_q16(q), ks, rng, with_bias)
    return slabs, bias, K, V, kinds


def uniform_xattn_inputs(W, H, beam, ks, seed=0):
    rng = _rng(4000 + seed)
    rows, D = W * beam, H * HD
    K = rng.uniform(-0.6, 0.6, (W, H, T_ENC, HD)).astype(np.float16)
    V = rng.uniform(-1.0, 1.0, (W, H, T_ENC, HD)).astype(np.float16)
    slabs, bias = split_slabs(_q16(rng.uniform(-0.6, 0.6, (rows, D))), ks, rng)
    return slabs, bias, K, V


def xattn_trace(q_slabs, bias, K, beam, kinds):
    """Structure of the crafted cross-attention inputs on the reference's own scores."""
    q = reduce_slabs(q_slabs, bias).astype(np.float64)
    rows, D = q.shape
    H = D // HD
    out = {"marker_min_weight": 1.0, "chunk_gap": 0.0, "low_chunk3_weight": 1.0, "far_max": -np.inf,
           "far_min": np.inf, "uniform_range": 0.0, "kinds": set()}
    mk = list(X_MARKERS)
    for r in range(rows):
        for h in range(H):
            s = q[r, h * HD:(h + 1) * HD] @ K[r // beam, h].astype(np.float64).T * 0.125
            p = np.exp(s - s.max())
            p /= p.sum()
            kind = kinds[r, h]
            out["kinds"].add(kind)
            cmax = np.array([s[c * XPER:(c + 1) * XPER].max() for c in range(XCH)])
            if kind == "markers":
                out["marker_min_weight"] = min(out["marker_min_weight"], float(p[mk].min()))
                out["chunk_gap"] = max(out["chunk_gap"], float(s.max() - cmax.min()))
            elif kind == "low":
                out["low_chunk3_weight"] = min(out["low_chunk3_weight"], float(p[3 * XPER:4 * XPER].sum()))
            elif kind == "far":
                out["far_max"] = max(out["far_max"], float(s.max()))
                out["far_min"] = min(out["far_min"], float(s.min()))
            else:
                out["uniform_range"] = max(out["uniform_range"], float(s.max() - s.min()))
    return out


def self_inputs(rows, H, ctx, pos, ks, seed=0, group=0):
    """Self-attention inputs for `rows` rows at positions pos (an int or one per row).  The cached K
    of a row is rho_p e + noise with rho = 6 at keys 0, 255, 256 (when cached) and 0 elsewhere; the
    new k (position pos) has rho = 6 as well, and q = 48 e + noise, so the row's softmax is
    shared by keys 0, 255, 256 and pos, near-tied (36 nats above the rest).  Every row has its own
    cache contents.  group > 0: an ancestry table that takes key p of row r from row
    (r + p + 1) % group of its group, so neighbouring keys come from different rows."""
    rng = _rng(5000 + seed)
    D = H * HD
    posv = np.broadcast_to(np.asarray(pos, np.int64), (rows,))
    kc = np.empty((rows, H, ctx, HD), np.float16)
    vc = rng.uniform(-1.0, 1.0, (rows, H, ctx, HD)).astype(np.float16)
    rho = np.zeros(ctx)
    rho[[p for p in (0, 255, 256) if p < ctx]] = 6.0
    tgt = np.empty((rows, 3 * D))
    # every row of a group shares its window's direction: a key gathered from a sibling row
    # still scores along the row's q
    for r in range(rows):
        g0 = r - r % group if group else r
        for h in range(H):
            e = _direction(_rng(7000 + 131 * seed + 17 * g0 + h))
            kc[r, h] = rho[:, None] * e + rng.uniform(-1 / 32, 1 / 32, (ctx, HD))
            sl = slice(h * HD, (h + 1) * HD)
            tgt[r, sl] = 48.0 * e + rng.uniform(-0.25, 0.25, HD)
            tgt[r, D:2 * D][sl] = 6.0 * e + rng.uniform(-1 / 32, 1 / 32, HD)
            tgt[r, 2 * D:][sl] = rng.uniform(-1.0, 1.0, HD)
    slabs, bias = split_slabs(_q16(tgt), ks, rng)
    anc = None
    if group:
        assert rows % group == 0
        anc = np.empty((rows, ctx), np.int32)
        for r in range(rows):
            g0 = r - r % group
            anc[r] = g0 + (r - g0 + np.arange(ctx) + 1) % group
    return slabs, bias, kc, vc, (posv.astype(np.int32) if np.ndim(pos) else int(pos)), anc


def self_trace(qkv_slabs, bias, kcache, pos, ancestry=None):
    """Smallest softmax weight of a peak key (0, 255, 256, pos, those below the row's length) and
    the peaks' total weight, on the reference's own scores; and how many distinct source rows the
    ancestry gives a row's keys."""
    r16 = reduce_slabs(qkv_slabs, bias).astype(np.float64)
    rows, D3 = r16.shape
    D = D3 // 3
    H = D // HD
    posv = np.broadcast_to(np.asarray(pos, np.int64), (rows,))
    wmin, wsum, nsrc = 1.0, 1.0, rows
    for r in range(rows):
        n = int(posv[r]) + 1
        src = np.full(n, r) if ancestry is None else np.append(np.asarray(ancestry)[r, :n - 1], r)
        if ancestry is not None and n > 1:
            nsrc = min(nsrc, len(set(src[:-1].tolist())))
        for h in range(H):
            kk = kcache[src, h, np.arange(n)].astype(np.float64)
            kk[n - 1] = r16[r, D + h * HD:D + (h + 1) * HD]
            s = kk @ r16[r, h * HD:(h + 1) * HD] * 0.125
            p = np.exp(s - s.max())
            p /= p.sum()
            peaks = sorted({k for k in (0, 255, 256, n - 1) if k < n})
            wmin = min(wmin, float(p[peaks].min()))
            wsum = min(wsum, float(p[peaks].sum()))
    return {"peak_min_weight": wmin, "peak_weight": wsum, "sources": nsrc}


# --------------------------------------------------------------------------- the structure, asserted
def check_enc_trace(qkv):
    """The structure every crafted encoder head must have (shared with the GPU tests)."""
    _, nb, H, _, _ = qkv.shape
    for b in range(nb):
        for h in range(H):
            t = enc_trace(qkv[0, b, h], qkv[1, b, h])
            assert (t["raises"] > 0).sum() >= 100, "queries whose max is raised after tile 0"
            assert (t["raises"] >= 10).sum() >= 1, "queries raised >= 10 times"
            assert ((t["stale"] > 4) & (t["stale"] <= 8)).sum() >= 100, "stale excess in (4, 8]"
            assert t["disagree"] >= 1, "lanes of one wave that disagree on raising"
            assert t["jump"].max() > 150, "a jump that flushes alpha to 0"
            assert t["smax"] < 400


def check_xattn_trace(slabs, bias, K, beam, kinds):
    t = xattn_trace(slabs, bias, K, beam, kinds)
    if "markers" in t["kinds"]:
        assert t["marker_min_weight"] >= 0.01, t    # the ten markers are near-tied
        assert t["chunk_gap"] >= 100, t             # a chunk whose max lies >= 100 nats below
    if "low" in t["kinds"]:
        assert t["low_chunk3_weight"] >= 0.999, t
    if "far" in t["kinds"]:
        assert -230 <= t["far_min"] and t["far_max"] <= -170, t
    if "uniform" in t["kinds"]:
        assert t["uniform_range"] <= 2.0, t
    return t


def check_self_trace(slabs, bias, kc, pos, anc=None, group=0):
    t = self_trace(slabs, bias, kc, pos, anc)
    assert t["peak_min_weight"] >= 0.1 and t["peak_weight"] >= 0.999, t
    if anc is not None:
        assert t["sources"] >= min(group, 2), t
    return t


# --------------------------------------------------------------------------- scheme emulations
def _h16(x):
    return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def enc_attn_emulate(q, k, v, lazy=True, tail_mask=True, rescale=True):
    """enc_attn_kernel's scheme for one head in float32: 64-key tiles with clamped loads past T,
    the running max on raw scores (lazy: raised only past 2^8), p = 2^(s cs - m cs) rounded to
    fp16 for P V, l and O rescaled by alpha, fp16 output.  tail_mask=False leaves the clamped
    duplicates of the last key in; rescale=False never multiplies O by alpha."""
    f = np.float32
    q, k, v = (np.asarray(a, f) for a in (q, k, v))
    T = k.shape[0]
    cs = f(ENC_CS)
    mrun = np.full(q.shape[0], -np.inf, f)
    lrun = np.zeros(q.shape[0], f)
    o = np.zeros((q.shape[0], HD), f)
    for kt in range((T + ENC_KB - 1) // ENC_KB):
        keys = np.minimum(kt * ENC_KB + np.arange(ENC_KB), T - 1)
        sc = q @ k[keys].T
        if tail_mask:
            sc[:, kt * ENC_KB + np.arange(ENC_KB) >= T] = -np.inf
        mnew = np.maximum(mrun, sc.max(1))
        if lazy:
            with np.errstate(invalid="ignore"):
                mnew = np.where((mnew - mrun) * cs <= f(8.0), mrun, mnew)
        with np.errstate(invalid="ignore"):
            alpha = np.where(np.isneginf(mrun), f(0), np.exp2((mrun - mnew) * cs, dtype=f))
        mrun = mnew
        p = np.exp2(sc * cs - (mnew * cs)[:, None], dtype=f)
        lrun = lrun * alpha + p.sum(1, dtype=f)
        if rescale:
            o = o * alpha[:, None]
        o = o + _h16(p) @ v[keys]
    return _h16(o / lrun[:, None])


def enc_attn_emulate_all(qkv, **kw):
    _, nb, H, T, _ = qkv.shape
    out = np.empty((nb * T, H * HD), np.float32)
    for b in range(nb):
        for h in range(H):
            out[b * T:(b + 1) * T, h * HD:(h + 1) * HD] = enc_attn_emulate(qkv[0, b, h], qkv[1, b, h], qkv[2, b, h], **kw)
    return out


def xattn_emulate(q, K, V, tail_mask=True, merge_factor=True):
    """The key-chunk scheme of dec_xattn_chunk_kernel / dec_xattn_mfma_kernel for one (row, head)
    in float32: 8 chunks of 188 keys (the last 184), each loaded into 192 slots clamped to the
    chunk's last key; per chunk m, l = sum exp(s - m), acc = sum exp(s - m) v; merged as
    sum e^(m_c - M) acc_c / sum e^(m_c - M) l_c.  tail_mask=False keeps the clamped slots;
    merge_factor=False merges without the e^(m_c - M) factors."""
    f = np.float32
    q, K, V = (np.asarray(a, f) for a in (q, K, V))
    T = K.shape[0]
    ms, ls, accs = [], [], []
    for c in range(XCH):
        k0 = c * XPER
        nk = min(T, k0 + XPER) - k0
        slot = np.arange(XKEYS)
        keys = k0 + np.minimum(slot, nk - 1)
        live = slot < nk if tail_mask else np.ones(XKEYS, bool)
        s = (K[keys] @ q) * f(0.125)
        m = s[live].max()
        p = np.where(live, np.exp(s - m, dtype=f), f(0))
        ms.append(m)
        ls.append(p.sum(dtype=f))
        accs.append(p @ V[keys])
    M = max(ms)
    e = [np.exp(f(m - M), dtype=f) if merge_factor else f(1) for m in ms]
    L = sum(l * x for l, x in zip(ls, e))
    O = sum(a * x for a, x in zip(accs, e))
    return O / L


def self_attend_emulate(q, K, V, tail_mask=True):
    """attend_one's scheme for one (row, head) in float32: 256-key blocks of 8 loads per lane, keys
    past n_keys clamped to the last key with p = 0.  tail_mask=False keeps them."""
    f = np.float32
    q, K, V = (np.asarray(a, f) for a in (q, K, V))
    n = K.shape[0]
    slot = np.arange((n + 255) // 256 * 256)
    keys = np.minimum(slot, n - 1)
    live = slot < n if tail_mask else np.ones(len(slot), bool)
    s = (K[keys] @ (q * f(0.125)))
    m = s[live].max()
    p = np.where(live, np.exp(s - m, dtype=f), f(0))
    return (p @ V[keys]) / p.sum(dtype=f)
