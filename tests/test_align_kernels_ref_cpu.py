"""tests/align_kernels_ref.py without a GPU: the float64 references pinned to torch and
transformers (so a reference cannot agree with a kernel by sharing its mistake), and the
conditions the crafted inputs of tests/test_gpu_align_kernels.py must meet to test anything."""
import numpy as np
import pytest

import align_kernels_ref as R
import align_ref

POST = R.post_cases()
MULTI = R.multi_slot_cases()
ALL_POST = POST + MULTI


def slot_ref(case, s):
    """(scores, fp32 stats, fp32 colstats, M, bound) of slot s on the reference alone."""
    P, hd, F, W = case["slots"][s]
    sc = case["scores"][s]
    st = R.softmax_stats(sc[:, :P]).astype(np.float32)
    cs = R.colstats(sc, st, P, F).astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        return sc, st, cs, R.matrix(sc, st, cs, P, F, hd, W), R.matrix_bound(sc, st, cs, P, F, hd, W)


# ------------------------------------------------------------------------------ pinned to upstream
@pytest.mark.parametrize("width", [1, 3, 7, 15])
def test_matrix_equals_torch_pipeline(width):
    torch = pytest.importorskip("torch")
    gw = pytest.importorskip("transformers.models.whisper.generation_whisper")
    rng = np.random.default_rng(width)
    for F in range(1, 10):
        for nan_cols in ((), (0,), tuple(range(0, F, 2)), tuple(range(F))):
            p = rng.uniform(0, 1, (3, 11, F))
            for f in nan_cols:
                p[:, :, f] = 0.25          # constant over the positions: 0/0 after standardising
            w = torch.from_numpy(p)
            std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
            w = gw._median_filter((w - mean) / std, width)
            want = w.mean(dim=0)[3:-1].numpy()
            cs = R.colstats_from_probs(p)
            np.testing.assert_allclose(cs[..., 0], mean[:, 0].numpy(), rtol=1e-14)
            got = R.matrix_from_probs(p, cs, 3, width)
            assert got.shape == want.shape == (7, F)
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12, equal_nan=True)
            assert not nan_cols or np.isnan(got).any() or width > 1
            assert len(nan_cols) < F or np.isnan(got).all()


def test_matrix_from_scores_equals_torch_softmax_pipeline():
    torch = pytest.importorskip("torch")
    gw = pytest.importorskip("transformers.models.whisper.generation_whisper")
    case = next(c for c in POST if c["name"] == "tk300_F255")
    P, hd, F, W = case["slots"][0]
    w = torch.from_numpy(case["scores"][0, :, :P].astype(np.float64)).softmax(dim=-1)[..., :F]
    std, mean = torch.std_mean(w, dim=-2, keepdim=True, unbiased=False)
    want = gw._median_filter((w - mean) / std, W).mean(dim=0)[hd:-1].numpy()
    np.testing.assert_allclose(R.matrix_full(case["scores"][0], P, F, hd, W), want, rtol=1e-9, atol=1e-11)


def test_tail_logprob_equals_torch_log_softmax():
    torch = pytest.importorskip("torch")
    for eot in R.TAIL_EOTS:
        c = R.tail_case(eot, 3)
        want = torch.log_softmax(torch.from_numpy(c["logits"][0, :eot].astype(np.float64)), -1).numpy()
        for tok in {0, eot - 1, int(c["forced"][0, 1])}:
            assert abs(R.tail_logprob(c["logits"][0], eot, tok) - want[tok]) <= 1e-12 * max(1.0, abs(want[tok]))


def test_self_attn_equals_torch_sdpa():
    torch = pytest.importorskip("torch")
    for pos, H, ks in ((0, 1, 1), (3, 6, 3), (257, 1, 3)):
        c = R.self_attn_case(pos, H, ks)
        out, kc, vc = R.self_attn(c["slabs"], c["bias"], c["kc"], c["vc"], pos, c["done"])
        r = R.reduce_inorder(c["slabs"], c["bias"]).astype(np.float64)
        D = 64 * H
        for b in (0, 2):
            q = torch.from_numpy(r[b, :D].reshape(H, 1, 64))
            k = torch.from_numpy(kc[b, :, :pos + 1].astype(np.float64))
            v = torch.from_numpy(vc[b, :, :pos + 1].astype(np.float64))
            want = torch.nn.functional.scaled_dot_product_attention(q, k, v).reshape(D).numpy()
            np.testing.assert_allclose(out[b], want, rtol=1e-10, atol=1e-12)
            np.testing.assert_array_equal(kc[b, :, pos].reshape(-1), R.reduce_inorder(c["slabs"], c["bias"])[b, D:2 * D])
        assert np.isnan(out[1]).all() and np.array_equal(kc[1].view(np.uint32), c["kc"][1].view(np.uint32))


# ------------------------------------------------------------------------------ conditions: post
@pytest.mark.parametrize("case", ALL_POST, ids=lambda c: c["name"])
def test_post_case_conditions(case):
    S, H, ps, TK = case["scores"].shape
    assert ps % 16 == 0 and len(case["slots"]) == S and H == case["n_heads"]
    for s, (P, hd, F, W) in enumerate(case["slots"]):
        assert hd in (1, 3) and hd + 2 <= P <= ps and 1 <= F <= TK and W % 2 == 1 and W <= 15
        sc, st, cs, M, bound = slot_ref(case, s)
        assert np.isnan(sc[:, P:]).all() and not np.isnan(sc[:, :P]).any()      # dead rows are NaN
        if case["degenerate"]:
            assert np.isnan(M).any()
            continue
        assert np.isfinite(M).all()
        # the bound must be far below the signal, and no column may be nearly constant
        assert bound.max() <= 1e-3 * M.std(), (bound.max(), M.std())
        assert (cs[..., 1] >= 1e-6 * cs[..., 0]).all()
        # exp stays normal in fp32
        assert (sc[:, :P].max(-1, keepdims=True) - sc[:, :P]).max() < 87
        if F < TK:
            # the largest scores sit at keys >= F: cropping before the softmax changes every probability
            assert (sc[:, :P, F:].max(-1) > sc[:, :P, :F].max(-1) + 10).all()
            crop = R.matrix_full(sc[..., :F], P, F, hd, W)
            d = np.abs(crop - M)      # (one key left: every probability 1, every column constant, NaN)
            assert np.isnan(d).all() or np.nanmax(d) > 1e3 * bound.max()


def test_post_cases_cover_the_issue_list():
    by = {c["name"]: c for c in POST}
    slots = [(c["TK"],) + tuple(s) for c in ALL_POST for s in c["slots"]]
    assert {t[0] for t in slots} >= set(R.TKS)
    for F in R.FS:
        assert any(tk > f == F for tk, _, _, f, _ in slots), F           # F < TK
    assert {tk for tk, _, _, f, _ in slots if f == tk} >= set(R.TKS)       # F == TK
    for W in R.WIDTHS:
        assert any(w == W and f == W // 2 + 1 for _, _, _, f, w in slots), W
        assert W == 1 or any(w == W and f == W // 2 for _, _, _, f, w in slots), W
    assert {c["n_heads"] for c in ALL_POST} >= {1, 2, 6}
    assert any(P == 448 and tk == 1500 for tk, P, _, _, _ in slots)
    for c in MULTI:
        ps = c["pstride"]
        lens = [s[0] for s in c["slots"]]
        assert ps in lens and any(P == hd + 3 for P, hd, _, _ in c["slots"]) and any(P % 16 for P in lens)
        assert {s[1] for s in c["slots"]} == {1, 3} and len({s[2] for s in c["slots"]}) == 3
        assert len({s[3] for s in c["slots"]}) >= 2
    assert {c["pstride"] for c in MULTI} == {16, 32}
    # heads of very different scale: a skipped head or a wrong divisor moves M past the bound
    assert by["heads6"]["n_heads"] == 6 and max(R.HEAD_SCALES) > 50 * min(R.HEAD_SCALES)


def test_post_ties_ramp_and_peaks():
    by = {c["name"]: c for c in POST}
    # ties: a median window that holds exactly equal values
    P, hd, F, W = by["ties"]["slots"][0]
    sc, st, cs, M, bound = slot_ref(by["ties"], 0)
    z = (R.probs(sc[:, :P], st)[..., :F] - cs[:, None, :, 0]) / cs[:, None, :, 1]
    assert np.array_equal(z[..., 10], z[..., 11]) and np.array_equal(z[..., 10], z[..., 12])
    assert np.array_equal(z[..., 0], z[..., 39])
    # ramp: reflect padding off by one (numpy's "symmetric") changes the first and last W/2 outputs
    P, hd, F, W = by["ramp"]["slots"][0]
    sc, st, cs, M, bound = slot_ref(by["ramp"], 0)
    z = (R.probs(sc[:, :P], st)[..., :F] - cs[:, None, :, 0]) / cs[:, None, :, 1]
    assert (np.diff(R.probs(sc[:, :P], st), axis=-1) != 0).all()
    pad = W // 2
    win = np.lib.stride_tricks.sliding_window_view(np.pad(z, [(0, 0), (0, 0), (pad, pad)], mode="symmetric"), W, axis=-1)
    off = np.sort(win, -1)[..., pad].mean(0)[hd:P - 1]
    d = np.abs(off - M)
    edge = np.r_[0:pad, F - pad:F]
    assert d[:, edge[:pad]].max() > 1e3 * bound.max() and d[:, edge[pad:]].max() > 1e3 * bound.max()
    assert (d[:, pad:F - pad] == 0).all()
    # peaks: differences up to about 60 within a row, and the offset rows are exact in fp32
    base, offc = by["peaked"]["scores"][0, :, :12], by["peaked_offset"]["scores"][0, :, :12]
    spread = (base.max(-1) - base.min(-1)).max()
    assert 55 <= spread <= 61
    assert np.array_equal(offc.astype(np.float64)[:, [2, 5]], base.astype(np.float64)[:, [2, 5]] + 1e4)
    assert np.array_equal(np.delete(offc, [2, 5], 1), np.delete(base, [2, 5], 1))


def test_nan_windows_hold_1_3_4_and_7_nans():
    case = next(c for c in POST if c["name"] == "nan_windows")
    P, hd, F, W = case["slots"][0]
    sc, st, cs, M, bound = slot_ref(case, 0)
    nan_col = np.zeros(F, bool)
    nan_col[case["nan_columns"]] = True
    assert np.array_equal(cs[0, :, 1] == 0, nan_col) and (cs[1, :, 1] > 0).all()
    pad = W // 2
    count = np.lib.stride_tricks.sliding_window_view(np.pad(nan_col, pad, mode="reflect"), W).sum(-1)
    assert set(count.tolist()) >= {0, 1, 3, 4, 7}
    # sorted NaN-last, the median is NaN from 4 NaNs of 7 on
    np.testing.assert_array_equal(np.isnan(M), np.broadcast_to(count >= 4, M.shape))
    # a compare-exchange network on fmin / fmax (which drop NaN) is finite there: the tests can tell
    with np.errstate(invalid="ignore"):
        z = (R.probs(sc[:, :P], st)[..., :F] - cs[:, None, :, 0]) / cs[:, None, :, 1]
    win = np.lib.stride_tricks.sliding_window_view(np.pad(z, [(0, 0), (0, 0), (pad, pad)], mode="reflect"), W, axis=-1).copy()
    for a in range(W):
        for b in range(W - 1 - a):
            lo, hi = np.fmin(win[..., b], win[..., b + 1]), np.fmax(win[..., b], win[..., b + 1])
            win[..., b], win[..., b + 1] = lo, hi
    assert np.isfinite(win[..., pad].mean(0)[hd:P - 1][:, count == 4]).all()


# ------------------------------------------------------------------------------ arithmetic mutants, on the reference
def test_reference_mutants_move_past_the_bounds():
    """The breaks a kernel could have, applied to the reference: each moves a crafted case past its
    bound by orders of magnitude."""
    by = {c["name"]: c for c in POST}
    P, hd, F, W = by["heads6"]["slots"][0]
    sc, st, cs, M, bound = slot_ref(by["heads6"], 0)
    p = R.probs(sc[:, :P], st)[..., :F]
    cs1 = cs.astype(np.float64).copy()
    cs1[..., 1] *= np.sqrt(P / (P - 1))                                   # the divisor P - 1
    assert np.abs(R.matrix_from_probs(p, cs1, hd, W) - M).max() > 1e3 * bound.max()
    z = align_ref.median_filter((p - cs[:, None, :, 0]) / cs[:, None, :, 1], W)
    assert np.abs(z.sum(0)[hd:P - 1] / 7 - M).max() > 1e3 * bound.max()   # the divisor n_heads + 1
    assert np.abs(z[1:].mean(0)[hd:P - 1] - M).max() > 1e3 * bound.max()  # a skipped head
    pad = W // 2
    zz = (p - cs[:, None, :, 0]) / cs[:, None, :, 1]
    win = np.lib.stride_tricks.sliding_window_view(np.pad(zz, [(0, 0), (0, 0), (pad, pad)], mode="reflect"), W, axis=-1)
    low = np.sort(win, -1)[..., pad - 1].mean(0)[hd:P - 1]               # the median index pad - 1
    assert np.abs(low - M).max() > 1e3 * bound.max()
    # tail: the loop bound eot - 1 drops the last logit, which the case makes the row's second largest
    for eot in R.TAIL_EOTS[1:]:
        c = R.tail_case(eot, 3)
        tok = int(c["forced"][0, 4])
        full, cut = R.tail_logprob(c["logits"][0], eot, tok), R.tail_logprob(c["logits"][0], eot - 1, tok)
        assert abs(full - cut) > 1e2 * R.tail_bound(c["logits"][0], eot, tok), eot
    # scores: 0.124 for 0.125
    c = R.scores_case(257, 5, True, 0)
    ref, wr, b = R.scores(c["slabs"], c["bias"], c["K"], c["layer_heads"], 3, 0, c["slot"], c["length"], c["scores"])
    assert (np.abs(ref[wr] * (1 - 0.124 / 0.125)) > 10 * b[wr]).mean() > 0.5


# ------------------------------------------------------------------------------ conditions: tail / attention / scores
@pytest.mark.parametrize("eot", R.TAIL_EOTS)
def test_tail_case_conditions(eot):
    for head in (1, 3):
        c = R.tail_case(eot, head)
        lg = c["logits"]
        assert lg.shape[1] == eot + 7 and (lg[:, eot:].min(1) > lg[:, :eot].max(1) + 400).all()
        assert (c["forced"] >= 0).all() and (c["forced"] < eot).all()
        assert -1 in c["slot"] and head + 3 in c["length"]
        seen = set()
        for pos in R.TAIL_POSITIONS:
            lp0, ct0, dn0 = R.tail_fill(c)
            lp, wr, ct, dn = R.tail_expected(pos, c["slot"], c["length"], c["head"], c["forced"], lp0, ct0, dn0, lg, eot)
            assert np.isfinite(lp[wr]).all()
            for r in range(4):
                L = int(c["length"][r])
                live = c["slot"][r] >= 0 and pos < L
                seen.add(("dead" if not live else "done" if pos == L - 1 else "prompt" if pos < head else
                          "last2" if pos == L - 2 else "text"))
                assert (ct[r] != R.TAIL_FILL_TOK) == (live and pos + 1 < L) and bool(dn[r]) == (live and pos == L - 1)
                if live:
                    assert wr[c["slot"][r]].sum() == (head <= pos <= L - 3)
            if eot >= 5 and wr[0].any() and pos % 2 == 0:
                assert lp[0][wr[0]][0] < -190                     # the forced token 200 below the maximum
        assert seen == {"dead", "done", "prompt", "last2", "text"}


def test_self_attn_case_conditions():
    assert set(R.SELF_POSITIONS) >= {0, 1, 3, 255, 256, 257, 447} and max(R.SELF_POSITIONS) > R.SELF_CTX - 1
    for pos, H, ks in ((257, 6, 3), (447, 1, 3), (460, 1, 1)):
        c = R.self_attn_case(pos, H, ks)
        p = min(pos, R.SELF_CTX - 1)
        assert c["done"].tolist() == [0, 1, 0]
        assert np.isnan(c["kc"][:, :, p + 1:]).all() and not np.isnan(c["kc"][:, :, :p + 1]).any()
        r = R.reduce_inorder(c["slabs"], c["bias"])
        if ks > 1:   # the fp32 sum depends on the order of the slabs
            assert (R.reduce_inorder(c["slabs"][::-1], c["bias"]) != r).mean() > 0.25
        out, kc, vc = R.self_attn(c["slabs"], c["bias"], c["kc"], c["vc"], pos, c["done"])
        D = 64 * H
        for b, peaked in ((0, True), (2, False)):
            for h in range(H):
                s = kc[b, h, :p + 1].astype(np.float64) @ r[b, h * 64:(h + 1) * 64].astype(np.float64) * 0.125
                w = np.exp(s - s.max())
                w /= w.sum()
                if peaked:
                    peaks = sorted({k for k in (0, 255, 256, p) if k <= p})
                    assert w[peaks].sum() > 0.999 and w[peaks].min() > 1e-3 and s.max() - np.median(s) > 20 or p < 3
                else:
                    assert s.max() - s.min() < 12
        bound = R.self_attn_bound(c["slabs"], c["bias"], c["kc"], c["vc"], pos, c["done"])
        # (the peaked row's scores are 36 nats: 64 sequential fmas over sum|k q| = 288 allow 5e-4)
        assert bound[0].max() < 1e-2 * out[0].std() and bound[2].max() < 1e-3 * out[2].std()


def test_scores_case_conditions():
    assert set(R.SCORE_TS) >= {1, 255, 256, 257, 300} and set(R.SCORE_KS) == {1, 4, 5, 9}
    for T, ks in ((257, 4), (300, 5), (255, 9)):
        c = R.scores_case(T, ks, True, 0)
        q = R.reduce_head(c["slabs"], c["bias"])
        plain = (np.asarray(c["bias"], np.float32) + c["slabs"].astype(np.float64).sum(0)).astype(np.float16)
        inorder = R.reduce_inorder(c["slabs"], c["bias"]).astype(np.float16)
        assert (q != inorder).mean() > 0.02 or (q != plain).mean() > 0.02   # the order of reduce_head shows in fp16
        ref, wr, b = R.scores(c["slabs"], c["bias"], c["K"], c["layer_heads"], 3, 0, c["slot"], c["length"], c["scores"])
        assert not wr[:, 1].any() and not wr[0].any() and wr[1, [0, 2], 0].all() and wr[2, [0, 2], 0].all()
        # unit-vector keys: each score of slot 1 is q[d] / 8 exactly
        d = np.arange(T) % 64
        np.testing.assert_array_equal(ref[1, 2, 0], q[0, 4 * 64 + d].astype(np.float64) / 8)
        np.testing.assert_array_equal(ref[1, 0, 0], q[0, d].astype(np.float64) / 8)
        assert b[wr].max() < 1e-4 * ref[2][wr[2]].std()
