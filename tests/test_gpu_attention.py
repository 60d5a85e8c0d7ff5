"""The attention kernels alone, one launch each on host data (osw_debug_enc_attn /
osw_debug_dec_xattn / osw_debug_dec_self_attn), against the float64 references of
tests/attn_ref.py on inputs whose softmax is far from uniform: the running max is raised
many times and by more than 2^150, key 1499 ties with a mid key (so a tail tile or tail chunk
that kept its clamped duplicates would move the output), chunk maxima lie 100+ nats apart.
The bounds are derived in attn_ref.py; tests/test_attn_ref_cpu.py shows what they catch.

Measured on an MI355X with max|V| = 1 (every test prints its figure): encoder lazy <= 5.96e-4,
eager 2.51e-4 (bound 1.95e-3); cross-attention <= 8.2e-6 (bounds 1.5e-5 .. 5.1e-5);
self-attention <= 2.8e-6 (bounds 1.0e-5 .. 2.0e-5).  DESIGN.md §2 has the record.
"""
import numpy as np
import pytest

import attn_ref as R
from open_speech_amd import dims as D
from open_speech_amd.engine import WhisperEngine

pytestmark = pytest.mark.gpu


def _dims(width):
    return D.WhisperDims(n_mels=80, n_audio_state=width, n_audio_head=width // 64, n_audio_layer=1,
                         n_text_state=width, n_text_head=width // 64, n_text_layer=1)


@pytest.fixture(scope="module", params=[128, 384], ids=["D128", "D384"])
def eng(request):
    e = WhisperEngine(_dims(request.param), device=0, max_batch=5)
    yield e
    e.close()


@pytest.fixture(scope="module")
def eng128():
    e = WhisperEngine(_dims(128), device=0, max_batch=1)
    yield e
    e.close()


# --------------------------------------------------------------------------- encoder
@pytest.fixture(scope="module")
def enc_small():
    qkv = R.enc_inputs(1, 2, seed=0)
    R.check_enc_trace(qkv)
    return qkv, R.enc_attn_ref(qkv), R.enc_tolerance(qkv[2])


def _enc_check(out, ref, tol, what):
    assert np.isfinite(out).all(), what
    err = float(np.abs(out.astype(np.float64) - ref).max())
    print(f"{what}: max |out - ref| = {err:.3e} (bound {tol:.3e})")
    assert err <= tol, (what, err, tol)


@pytest.mark.parametrize("nb,H,form", [(1, 2, None), (1, 3, "qb128"), (2, 3, "qb128"), (8, 6, None)],
                         ids=["1x2-auto", "1x3-qb128", "2x3-qb128", "8x6-auto"])
def test_enc_attn_matches_float64(eng128, enc_small, nb, H, form):
    """(1, 2) auto: 64-query workgroups; forced 128-query workgroups at (1, 3) (36 workgroups, not a
    multiple of the 8 XCDs the launch order is remapped over) and (2, 3); (8, 6) auto: 576 units of
    128 queries, the form the launcher picks for production batches."""
    if (nb, H) == (1, 2):
        qkv, ref, tol = enc_small
    else:
        qkv = R.enc_inputs(nb, H, seed=nb * 10 + H)
        R.check_enc_trace(qkv)
        ref, tol = R.enc_attn_ref(qkv), R.enc_tolerance(qkv[2])
    f = WhisperEngine.ATTN_AUTO if form is None else WhisperEngine.attn_form(qb128=True)
    _enc_check(eng128.debug_enc_attn(qkv, f), ref, tol, f"enc_attn {nb}x{H} {form or 'auto'}")


def test_enc_attn_forms(eng128, enc_small):
    """Every explicit form on the same inputs: 64- and 128-query workgroups, pipelined or not, give
    the same bits (as attn.hip claims); eager and lazy differ in rounding and each meets the bound."""
    qkv, ref, tol = enc_small
    for eager in (False, True):
        outs = {}
        for qb128 in (False, True):
            for pipe in (False, True):
                o = eng128.debug_enc_attn(qkv, WhisperEngine.attn_form(eager=eager, qb128=qb128, pipe=pipe))
                _enc_check(o, ref, tol, f"enc_attn eager={eager} qb128={qb128} pipe={pipe}")
                outs[qb128, pipe] = o
        np.testing.assert_array_equal(outs[False, False], outs[True, False], err_msg="64 vs 128 queries")
        np.testing.assert_array_equal(outs[False, False], outs[False, True], err_msg="pipelined vs not (64)")
        np.testing.assert_array_equal(outs[True, False], outs[True, True], err_msg="pipelined vs not (128)")
        if not eager:
            np.testing.assert_array_equal(outs[False, False], eng128.debug_enc_attn(qkv), err_msg="auto")


def test_enc_attn_rejects_bad_arguments(eng128, enc_small):
    from open_speech_amd._lib import OswError
    qkv = enc_small[0]
    for form in (2, 16, -1):
        with pytest.raises(OswError) as ei:
            eng128.debug_enc_attn(qkv, form)
        assert ei.value.rc == -22


# --------------------------------------------------------------------------- cross-attention
KS = (1, 3, 5, 9)


def _xattn_case(eng, W, beam, ks, seed, legacy=False, with_bias=True):
    H = eng.dims.n_text_head
    slabs, bias, K, V, kinds = R.xattn_inputs(W, H, beam, ks, seed=seed, with_bias=with_bias)
    R.check_xattn_trace(slabs, bias, K, beam, kinds)
    ref = R.xattn_ref(slabs, bias, K, V, beam)
    tol, e32 = R.decoder_tolerance(ref, R.xattn_ref(slabs, bias, K, V, beam, np.float32, R.attend_f32), 1.0)
    out = eng.debug_dec_xattn(slabs, bias, K, V, beam=beam, legacy=legacy)
    assert np.isfinite(out).all()
    err = float(np.abs(out.astype(np.float64) - ref).max())
    print(f"xattn D={eng.dims.n_text_state} W={W} beam={beam} ks={ks} legacy={legacy}: max |out - ref| = {err:.3e} "
          f"(float32 numpy {e32:.3e}, bound {tol:.3e})")
    assert err <= tol, (err, tol)
    return out


@pytest.mark.parametrize("W,beam", [(1, 1), (3, 1), (5, 1), (1, 5), (3, 5), (2, 2), (2, 4), (2, 8)])
def test_dec_xattn_matches_float64(eng, W, beam):
    """Greedy rows (dec_xattn_chunk_kernel<1>), beam rows with ks <= 8 (dec_xattn_mfma_kernel<5|8>)
    and with ks = 9 (dec_xattn_chunk_kernel<2|4|5|8>)."""
    for ks in KS:
        _xattn_case(eng, W, beam, ks, seed=100 * W + 10 * beam + ks)


@pytest.mark.parametrize("W,beam,ks,with_bias", [(2, 1, 3, True), (1, 5, 9, True), (2, 2, 1, False)])
def test_dec_xattn_legacy_kernel(eng, W, beam, ks, with_bias):
    _xattn_case(eng, W, beam, ks, seed=7, legacy=True, with_bias=with_bias)


def test_dec_xattn_without_bias(eng):
    _xattn_case(eng, 2, 1, 3, seed=8, with_bias=False)
    _xattn_case(eng, 1, 4, 3, seed=9, with_bias=False)


@pytest.mark.parametrize("beam,ks", [(1, 3), (5, 3), (4, 9)])
def test_dec_xattn_window_placement(eng, beam, ks):
    """The same window at another index of the batch gives the same bits (fixed-order merge, no
    dependence on the workgroup's XCD or arrival order)."""
    H = eng.dims.n_text_head
    slabs, bias, K, V, _ = R.xattn_inputs(3, H, beam, ks, seed=50 + beam)
    a = eng.debug_dec_xattn(slabs, bias, K, V, beam=beam)
    perm = [2, 0, 1]                      # window w of the second call is window perm[w] of the first
    rows = np.concatenate([np.arange(beam) + w * beam for w in perm])
    b = eng.debug_dec_xattn(slabs[:, rows], bias, K[perm], V[perm], beam=beam)
    np.testing.assert_array_equal(b, a[rows])
    one = eng.debug_dec_xattn(slabs[:, 2 * beam:], bias, K[2:], V[2:], beam=beam)
    np.testing.assert_array_equal(one, a[2 * beam:])


# --------------------------------------------------------------------------- self-attention
def _self_case(eng, rows, pos, ks, seed, group=0):
    H, ctx = eng.dims.n_text_head, eng.dims.n_text_ctx
    slabs, bias, kc, vc, p, anc = R.self_inputs(rows, H, ctx, pos, ks, seed=seed, group=group)
    R.check_self_trace(slabs, bias, kc, p, anc, group)
    ref, kc_ref, vc_ref = R.self_attn_ref(slabs, bias, kc, vc, p, anc)
    e32, _, _ = R.self_attn_ref(slabs, bias, kc, vc, p, anc, attend=R.attend_f32, dtype=np.float32)
    tol, err32 = R.decoder_tolerance(ref, e32, 1.0)
    out, kc2, vc2 = eng.debug_dec_self_attn(slabs, bias, kc, vc, p, anc, group or 1)
    assert np.isfinite(out).all()
    err = float(np.abs(out.astype(np.float64) - ref).max())
    print(f"self_attn D={eng.dims.n_text_state} rows={rows} group={group} ks={ks}: max |out - ref| = {err:.3e} "
          f"(float32 numpy {err32:.3e}, bound {tol:.3e})")
    assert err <= tol, (err, tol)
    # position pos of every row holds fp16 k and v; every other cache element is bit-unchanged
    np.testing.assert_array_equal(kc2.view(np.uint16), kc_ref.view(np.uint16))
    np.testing.assert_array_equal(vc2.view(np.uint16), vc_ref.view(np.uint16))
    posv = np.broadcast_to(np.asarray(p), (rows,))
    r16 = R.reduce_slabs(slabs, bias)
    Dm = H * 64
    for r in range(rows):
        np.testing.assert_array_equal(kc2[r, :, posv[r]].reshape(-1), r16[r, Dm:2 * Dm])
        np.testing.assert_array_equal(vc2[r, :, posv[r]].reshape(-1), r16[r, 2 * Dm:])


NK = np.array(R.SELF_NKEYS) - 1


def test_dec_self_attn_one_row(eng):
    """One row (V issued with K), a shared position: n_keys 1, 256 and 448."""
    for pos in (0, 255, 447):
        _self_case(eng, 1, pos, 3, seed=pos)


@pytest.mark.parametrize("rows,ks", [(8, 3), (8, 17), (9, 5)])
def test_dec_self_attn_rows(eng, rows, ks):
    """8 rows: V issued with K; 9 rows: V late.  Per-row positions over every n_keys at which the
    256-key blocks and their clamped tails change: 1, 2, 33, 255, 256, 257, 447, 448."""
    _self_case(eng, rows, np.resize(NK, rows), ks, seed=rows + ks)


@pytest.mark.parametrize("rows", [5, 10])
def test_dec_self_attn_gather(eng, rows):
    """Beam rows in groups of 5 (5 rows: V with K; 10 rows: V late): every key from another row of
    the group through the ancestry table; a group shares its position (257 and 448 keys)."""
    pos = np.repeat([256, 447], 5)[:rows]
    _self_case(eng, rows, pos, 3, seed=rows, group=5)


def test_dec_self_attn_rejects_bad_arguments(eng):
    from open_speech_amd._lib import OswError
    H, ctx = eng.dims.n_text_head, eng.dims.n_text_ctx
    slabs, bias, kc, vc, p, anc = R.self_inputs(5, H, ctx, 3, 1, group=5)
    bad = anc.copy()
    bad[0, 0] = 5
    for kw in (dict(pos=ctx), dict(anc=bad), dict(group=4)):
        with pytest.raises(OswError) as ei:
            eng.debug_dec_self_attn(slabs, bias, kc, vc, kw.get("pos", p), kw.get("anc", anc), kw.get("group", 5))
        assert ei.value.rc == -22
