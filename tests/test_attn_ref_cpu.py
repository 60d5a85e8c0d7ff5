"""The attention references, crafted inputs and bounds of tests/attn_ref.py, checked without a
GPU: each generator's structure on the reference's own scores (tests/test_gpu_attention.py
asserts the same traces on the inputs it launches), and the sensitivity of each bound: a numpy
restatement of each kernel's scheme, broken the ways a kernel could be, must leave the bound on
the crafted inputs by a wide margin, and on near-uniform inputs (all the suite had before) vanish
or shrink to a few percent of max|V|."""
import numpy as np
import pytest

import attn_ref as R


@pytest.fixture(scope="module")
def enc_case():
    qkv = R.enc_inputs(1, 2, seed=0)
    return qkv, R.enc_attn_ref(qkv), R.enc_tolerance(qkv[2])


@pytest.fixture(scope="module")
def enc_uniform_case():
    qkv = R.uniform_enc_inputs(1, 1, seed=0)
    return qkv, R.enc_attn_ref(qkv), R.enc_tolerance(qkv[2])


def test_enc_inputs_have_the_structure(enc_case):
    qkv, ref, _ = enc_case
    R.check_enc_trace(qkv)
    # key 1499 and the mid key are near-tied where they carry the softmax: both hold weight
    q, k = qkv[0, 0, 0].astype(np.float64), qkv[1, 0, 0].astype(np.float64)
    s = q @ k.T * 0.125
    p = np.exp(s - s.max(1, keepdims=True))
    p /= p.sum(1, keepdims=True)
    both = (p[:, R.ENC_MID_KEY] > 0.2) & (p[:, -1] > 0.2)
    assert both.sum() >= 300, both.sum()


def test_uniform_enc_inputs_are_what_the_suite_had(enc_uniform_case):
    qkv, _, _ = enc_uniform_case
    t = R.enc_trace(qkv[0, 0, 0], qkv[1, 0, 0])
    assert t["smax"] <= 0.9 * R.LOG2E and t["raises"].sum() == 0 and t["jump"].max() == 0


@pytest.mark.parametrize("lazy", [True, False])
def test_enc_emulation_meets_the_bound(enc_case, lazy):
    """The faithful emulation (fp16 P, fp32 sums, fp16 out) is inside 2^-9 max|V| on the crafted
    inputs: the bound is not so tight that a correct kernel would miss it."""
    qkv, ref, tol = enc_case
    err = np.abs(R.enc_attn_emulate_all(qkv, lazy=lazy) - ref).max()
    print(f"encoder emulation lazy={lazy}: max |err| {err:.3e} (bound {tol:.3e})")
    assert err <= tol


@pytest.mark.parametrize("broken", [dict(tail_mask=False), dict(rescale=False), dict(rescale=False, lazy=False)])
def test_enc_bound_catches_a_broken_scheme(enc_case, enc_uniform_case, broken):
    qkv, ref, tol = enc_case
    err = np.abs(R.enc_attn_emulate_all(qkv, **broken) - ref)
    assert err.max() > 10 * tol, (broken, err.max())
    if "tail_mask" in broken:
        # the unmasked duplicates of key 1499 move the queries tied between it and the mid key
        assert (err.max(1) > 0.05).sum() >= 300
    uq, uref, utol = enc_uniform_case
    uerr = np.abs(R.enc_attn_emulate_all(uq, **broken) - uref).max()
    if "tail_mask" in broken:
        # near-uniform weights: 36 duplicates among 1536 keys shift 2.3 % of the weight (e^0.9
        # times that at most) to v[1499]: a few percent of max|V|, above this bound too, and more
        # than 10x less than on the crafted inputs.  This break alone is NOT hidden from the old
        # suite: put into the oracle's attention on the tiny fixture (seed 1234, chirp_clip(3)) it
        # moves the encoder output by 3.7e-2 max / 6.9e-3 mean, against the 2e-2 / 2e-3 that
        # test_tiny_encoder_matches_oracle_and_golden allows: seen there at under 2x its bound,
        # here at over 200x.
        assert utol < uerr <= 0.05, uerr
        assert err.max() > 10 * uerr
    elif broken.get("lazy", True):
        assert uerr <= utol, uerr       # the max is never raised after tile 0: alpha is never used
    else:
        assert uerr <= 0.06 * err.max()  # eager: alpha = 2^-(a fraction of a bit) per tile


# --------------------------------------------------------------------------- cross-attention
@pytest.fixture(scope="module")
def x_case():
    slabs, bias, K, V, kinds = R.xattn_inputs(1, 2, 4, 3, seed=0)
    return slabs, bias, K, V, kinds, R.xattn_ref(slabs, bias, K, V, 4)


def test_xattn_inputs_have_the_structure(x_case):
    slabs, bias, K, V, kinds, _ = x_case
    t = R.check_xattn_trace(slabs, bias, K, 4, kinds)
    assert t["kinds"] == set(R.X_ROW_KINDS)
    assert np.abs(slabs).max() <= 64 and np.array_equal(slabs * 256, np.round(slabs * 256))
    # chunk edges as decode.hip cuts them: ceil(1500 / 8) = 188 keys, 184 in the last
    assert R.XPER == 188 and R.T_ENC - 7 * R.XPER == 184


def test_xattn_emulation_and_bound(x_case):
    slabs, bias, K, V, kinds, ref = x_case
    e32 = R.xattn_ref(slabs, bias, K, V, 4, np.float32, R.attend_f32)
    tol, err32 = R.decoder_tolerance(ref, e32, 1.0)
    emu = R.xattn_ref(slabs, bias, K, V, 4, np.float32, R.xattn_emulate)
    err = np.abs(emu - ref).max()
    print(f"cross-attention: float32 evaluation {err32:.3e}, chunk emulation {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    for broken in (dict(tail_mask=False), dict(merge_factor=False)):
        bad = R.xattn_ref(slabs, bias, K, V, 4, np.float32, lambda q, k, v: R.xattn_emulate(q, k, v, **broken))
        assert np.abs(bad - ref).max() > 100 * tol, broken


def test_xattn_breaks_hide_on_uniform_inputs():
    slabs, bias, K, V = R.uniform_xattn_inputs(1, 2, 2, 3)
    ref = R.xattn_ref(slabs, bias, K, V, 2)
    q = R.reduce_slabs(slabs, bias).astype(np.float64)
    assert np.abs(q[0, :64] @ K[0, 0].astype(np.float64).T).max() / 8 <= 0.9
    for broken in (dict(tail_mask=False), dict(merge_factor=False)):
        bad = R.xattn_ref(slabs, bias, K, V, 2, np.float32, lambda q, k, v: R.xattn_emulate(q, k, v, **broken))
        # 32 clamped slots among 1532, or chunk maxima within a nat of each other: a few percent of
        # max|V|, inside the 2e-2 of the end-to-end logits tests after the output projection
        assert np.abs(bad - ref).max() <= 2e-2, broken


# --------------------------------------------------------------------------- self-attention
def test_self_inputs_have_the_structure():
    pos = np.array(R.SELF_NKEYS) - 1
    slabs, bias, kc, vc, p, anc = R.self_inputs(8, 2, 448, pos, 3)
    R.check_self_trace(slabs, bias, kc, p)
    slabs, bias, kc, vc, p, anc = R.self_inputs(10, 2, 448, np.repeat([254, 447], 5), 3, group=5)
    t = R.check_self_trace(slabs, bias, kc, p, anc, 5)
    assert t["sources"] == 5     # every row of the group feeds keys to every other
    assert all(len(set(anc[r, :5].tolist())) == 5 for r in range(10))


def test_self_reference_and_bound():
    pos = np.array(R.SELF_NKEYS) - 1
    slabs, bias, kc, vc, p, _ = R.self_inputs(8, 2, 448, pos, 3)
    ref, kc2, vc2 = R.self_attn_ref(slabs, bias, kc, vc, p)
    e32, _, _ = R.self_attn_ref(slabs, bias, kc, vc, p, attend=R.attend_f32, dtype=np.float32)
    tol, err32 = R.decoder_tolerance(ref, e32, 1.0)
    emu, _, _ = R.self_attn_ref(slabs, bias, kc, vc, p, attend=R.self_attend_emulate, dtype=np.float32)
    err = np.abs(emu - ref).max()
    print(f"self-attention: float32 evaluation {err32:.3e}, emulation {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    bad, _, _ = R.self_attn_ref(slabs, bias, kc, vc, p, dtype=np.float32,
                                attend=lambda q, k, v: R.self_attend_emulate(q, k, v, tail_mask=False))
    assert np.abs(bad - ref).max() > 100 * tol
    # only the new position changed in the caches
    changed = (kc2 != kc) | (vc2 != vc)
    for r in range(8):
        changed[r, :, pos[r]] = False
    assert not changed.any()
    # n_keys = 1: the output is v itself
    r16 = R.reduce_slabs(slabs, bias)
    np.testing.assert_array_equal(ref[0], r16[0, 2 * 128:].astype(np.float64))
