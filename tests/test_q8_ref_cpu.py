"""Int8 decoder weights without a GPU: weights.quantize_rows, the int8 fragment layout, the float32
restatement and bound of tests/q8_ref.py (met by a faithful evaluation on every GPU case, missed
by >= 100x by three wrong ones), the CTranslate2 reader's keep_int8, and STT_COMPUTE_TYPE through
the backend with a recording engine factory."""
import numpy as np
import pytest

import dec_gemm_ref as R
import q8_ref as Q
from open_speech_amd import dims as D
from open_speech_amd import model_store, weights
from open_speech_amd.backend import HipWhisperBackend
from open_speech_amd.ct2 import canonical_to_ct2, ct2_to_canonical, read_model_bin, write_model_bin

F32, F16, F64 = np.float32, np.float16, np.float64


# --------------------------------------------------------------------------- quantize_rows
def test_quantize_rows_properties():
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((37, 192)) * rng.uniform(1e-3, 30, (37, 1))).astype(F32)
    w[11] = 0.0                      # a zero row
    w[12, 5] = -w[12].__abs__().max() * 2   # a negative row maximum
    qm = weights.quantize_rows(w)
    q, m = qm.q, qm.mult
    assert q.dtype == np.int8 and m.dtype == np.float32 and q.shape == w.shape and m.shape == (37,)
    assert np.abs(q.astype(np.int32)).max() <= 127
    # |w - q m| <= m / 2 per element (+ the float32 roundings of w * scale and of 1 / scale: 2 ulp of |w|)
    err = np.abs(w.astype(F64) - q.astype(F64) * m.astype(F64)[:, None])
    assert (err <= m.astype(F64)[:, None] / 2 + 2.0 ** -22 * np.abs(w)).all()
    # the row maximum maps to +-127
    nz = np.abs(w).max(1) > 0
    arg = np.abs(w).argmax(1)
    top = q[np.arange(37), arg]
    assert (np.abs(top[nz].astype(np.int32)) == 127).all()
    assert top[12] == -127
    # a zero row: q = 0, mult = 1
    assert not q[11].any() and m[11] == 1.0
    # quantising q * mult returns q (and the same multipliers up to their own rounding)
    again = weights.quantize_rows(qm.dequantize())
    assert np.array_equal(again.q, q)
    np.testing.assert_allclose(again.mult, m, rtol=2.0 ** -22)


def test_quantize_decoder_names_and_passthrough():
    d = D.MICRO_TEST
    w = weights.random_weights(d, seed=3)
    keep = weights.quantize_rows(np.asarray(w["dec.l0.o.w"], F32))
    w["dec.l0.o.w"] = keep
    out = weights.quantize_decoder(w, d)
    names = set(weights.q8_names(d))
    assert names == {"dec.tok"} | {f"dec.l{i}.{k}.w" for i in range(d.n_text_layer)
                                   for k in ("qkv", "o", "xq", "xo", "fc1", "fc2")}
    for n, v in out.items():
        assert isinstance(v, weights.QuantizedMatrix) == (n in names), n
    assert out["dec.l0.o.w"] is keep            # stored int8 is kept, not re-quantised
    assert out["dec.crosskv.w"] is w["dec.crosskv.w"] and out["enc.l0.fc1.w"] is w["enc.l0.fc1.w"]


# --------------------------------------------------------------------------- fragment layout
@pytest.mark.parametrize("N,K", [(384, 384), (1002, 384), (40, 128)])
def test_fragment_layout_is_a_bijection(N, K):
    """The // and % model of GemmArgs::Wq maps the padded [ceil(N/16)*16][K] index set one to one
    onto the padded buffer, 16 B per lane and 1 KB per (block, step pair)."""
    Np = (N + 15) // 16 * 16
    n, k = np.meshgrid(np.arange(Np), np.arange(K), indexing="ij")
    off = Q.frag_q8_offset(n, k, K).ravel()
    assert off.min() == 0 and off.max() == Q.frag_q8_bytes(N, K) - 1
    assert np.array_equal(np.sort(off), np.arange(Np * K))
    # a lane's 16 bytes: one column, 8 consecutive k of step 2j then 8 of step 2j + 1
    inv = np.empty(Np * K, np.int64)
    inv[off] = np.arange(Np * K)
    piece = inv.reshape(-1, 16)
    pn, pk = piece // K, piece % K
    assert (pn == pn[:, :1]).all()
    assert (pk[:, :8] == pk[:, :1] + np.arange(8)).all() and (pk[:, 8:] == pk[:, :1] + 32 + np.arange(8)).all()
    assert (pk[:, 0] % 64 < 32).all() and (pk[:, 0] % 8 == 0).all()
    # a wave's 64 lanes of one (block, pair): 16 columns x 64 k, 1 KB contiguous
    wave = inv.reshape(-1, 1024)
    assert ((wave // K) // 16 == (wave[:, :1] // K) // 16).all() and ((wave % K) // 64 == (wave[:, :1] % K) // 64).all()
    # the packed bytes: q + 128, and q = 0 past N
    q = np.random.default_rng(N).integers(-127, 128, (N, K)).astype(np.int8)
    buf = Q.pack_frag_q8(q)
    assert np.array_equal(buf[Q.frag_q8_offset(n[:N], k[:N], K)].astype(np.int16) - 128, q)
    if Np > N:
        assert (buf[Q.frag_q8_offset(n[N:], k[N:], K)] == 128).all()


# --------------------------------------------------------------------------- restatement and bound
CPU_ROWS = 5   # rows are independent: a few rows of each GPU case keep the vocabulary width quick


@pytest.mark.parametrize("fam", ["same-sign", "uniform"])
@pytest.mark.parametrize("form,N,K,rows", Q.GPU_CASES, ids=[f"f{c[0]}-{c[1]}x{c[2]}" for c in Q.GPU_CASES])
def test_restatement_meets_the_bound(fam, form, N, K, rows):
    """k32 steps, hi then lo, then one multiply, in float32: within G S + 2^-24 |ref| of the float64
    (hi + lo) (q mult)^T on every shape the GPU tests launch (the split of the largest row count)."""
    M = min(max(rows), CPU_ROWS)
    ks = Q.case_ksplit(form, max(rows), N, K)
    hi, lo, q, mult = Q.q8_inputs(fam, M, N, K, seed=N + K)
    _, C = Q.restate_q8(hi, lo, q, mult, ks)
    bound, ref = Q.q8_bound(hi, lo, q, mult)
    r = float((np.abs(C.astype(F64) - ref) / bound).max())
    print(f"restatement {fam} form {form} N {N} K {K} ks {ks}: worst |err| / bound = {r:.3f}")
    assert r <= 1


def test_exact_family_is_exact():
    hi, lo, q, mult = Q.q8_inputs("exact", 5, 384, 384, seed=768)
    R.assert_exact(hi, lo, q.astype(F16), 384)
    slabs, C = Q.restate_q8(hi, lo, q, mult, 3)
    want = Q.scale_slabs(R.gemm_ref_exact(hi, lo, q.astype(F16), 3), mult)
    assert np.array_equal(slabs, want)
    assert np.array_equal(C.astype(F64), Q.q8_ref(hi, lo, q, mult))


@pytest.mark.parametrize("wrong", ["neighbour", "dropped", "bias"])
def test_wrong_restatements_miss_by_100x(wrong):
    """A kernel that reads the multiplier of column n + 1, forgets the multiplier, or multiplies the
    bias too is >= 100 x outside the bound (rows whose multipliers differ between neighbours; a
    unit-scale bias)."""
    M, N, K = 5, 384, 384
    hi, lo, W = R.uniform_inputs(M, N, K, seed=21)
    qm = weights.quantize_rows(Q.varied_rows(W, seed=21))
    bias = np.random.default_rng(22).uniform(-1, 1, N).astype(F32)
    bound, ref = Q.q8_bound(hi, lo, qm.q, qm.mult)
    ref = ref + bias.astype(F64)
    _, good = Q.restate_q8(hi, lo, qm.q, qm.mult, 1, bias=bias)
    assert (np.abs(good.astype(F64) - ref) <= bound + 2.0 ** -24 * np.abs(ref)).all()   # (+ the bias add's rounding)
    _, bad = Q.restate_q8(hi, lo, qm.q, qm.mult, 1, bias=bias, wrong=wrong)
    r = float((np.abs(bad.astype(F64) - ref) / (bound + 2.0 ** -24 * np.abs(ref))).max())
    print(f"wrong restatement {wrong!r}: worst |err| / bound = {r:.0f}")
    assert r >= 100


def test_pow2_quantize_is_exact_in_fp16():
    d = D.TINY_TEST
    w = weights.random_weights(d, seed=1234, emb_std=0.5)
    for n in ("dec.tok", "dec.l0.qkv.w", "dec.l3.fc2.w"):
        q, mult, h = Q.pow2_quantize(np.asarray(w[n], F32))
        assert np.abs(q.astype(np.int32)).max() <= 127 and np.abs(q.astype(np.int32)).max(1).min() >= 32
        assert (np.log2(mult) == np.round(np.log2(mult))).all() and (mult >= 2.0 ** -14).all()
        assert np.array_equal(h.astype(F32), q.astype(F32) * mult[:, None])


# --------------------------------------------------------------------------- CTranslate2 reader
def int8_ct2_variables(w, d, all_linear=True):
    """canonical weights -> a CTranslate2 variable dict as an int8 conversion stores it: every
    linear weight and the embedding int8 with a per-row ``_scale`` (= 127 / max|row|)."""
    v, aliases = canonical_to_ct2(w, d)
    out = {}
    for name, arr in v.items():
        linear = name.endswith("/weight") and arr.ndim == 2 and ("linear_" in name or "embeddings" in name)
        if linear and (all_linear or name.startswith("decoder/")):
            qm = weights.quantize_rows(np.asarray(arr, F32))
            out[name] = qm.q
            out[name + "_scale"] = (F32(1.0) / qm.mult).astype(F32)
        else:
            out[name] = arr
    return out, aliases


def test_ct2_keep_int8(tmp_path):
    d = D.MICRO_TEST
    w = weights.random_weights(d, seed=9, emb_std=0.5)
    v, aliases = int8_ct2_variables(w, d)
    path = str(tmp_path / "model.bin")
    write_model_bin(path, v, aliases)
    rv, ra = read_model_bin(path)
    today = ct2_to_canonical(rv, ra, d)
    kept = ct2_to_canonical(rv, ra, d, keep_int8=True)
    assert set(today) == set(kept)
    names = set(weights.q8_names(d))
    kind = {"qkv": "self_attention/linear_0", "o": "self_attention/linear_1", "xq": "attention/linear_0",
            "xo": "attention/linear_2", "fc1": "ffn/linear_0", "fc2": "ffn/linear_1"}

    def ct2_name(n):
        if n == "dec.tok":
            return "decoder/embeddings/weight"
        _, layer, k, _ = n.split(".")
        return f"decoder/layer_{layer[1:]}/{kind[k]}/weight"

    for n in today:
        if n in names:
            # the file's exact bytes, and every row's multiplier is that row's 1 / scale
            qm, cn = kept[n], ct2_name(n)
            assert isinstance(qm, weights.QuantizedMatrix), n
            assert qm.q.dtype == np.int8 and qm.mult.dtype == np.float32
            assert qm.q.shape == v[cn].shape and qm.q.tobytes() == v[cn].tobytes(), n
            assert np.array_equal(qm.mult, F32(1.0) / v[cn + "_scale"]), n
            assert (qm.mult[1:] != qm.mult[:-1]).mean() > 0.5              # (neighbours do differ: a swap would show)
        else:                       # the encoder, the cross-K/V projection, every vector: dequantised as today
            assert not isinstance(kept[n], weights.QuantizedMatrix), n
            assert kept[n].dtype == today[n].dtype and np.array_equal(kept[n], today[n]), n
    # the default is byte for byte the reader without the argument
    again = ct2_to_canonical(rv, ra, d, keep_int8=False)
    for n in today:
        assert again[n].dtype == today[n].dtype and again[n].tobytes() == today[n].tobytes(), n
        assert today[n].dtype in (np.float16, np.float32)


def test_model_store_compute_type(tmp_path):
    """load_weights(src, compute_type): stored int8 kept, a float checkpoint quantised at load;
    float16, anything else and None give today's tensors."""
    d = D.MICRO_TEST
    w = weights.random_weights(d, seed=9, emb_std=0.5)
    q_dir, f_dir = tmp_path / "int8_ct2", tmp_path / "f16_ct2"
    for p, (v, a) in ((q_dir, int8_ct2_variables(w, d)), (f_dir, canonical_to_ct2(w, d))):
        p.mkdir()
        write_model_bin(str(p / "model.bin"), v, a)
    names = set(weights.q8_names(d))
    for p in (q_dir, f_dir):
        src = model_store.resolve(str(p))
        base = model_store.load_weights(src)
        for ct in (None, "float16", "default", "float32"):
            same = model_store.load_weights(src, ct)
            assert all(same[n].tobytes() == base[n].tobytes() for n in base)
        for ct in ("int8_float16", "int8", "INT8_FLOAT16"):
            got = model_store.load_weights(src, ct)
            assert {n for n, x in got.items() if isinstance(x, weights.QuantizedMatrix)} == names
            assert got["enc.l0.fc1.w"].tobytes() == base["enc.l0.fc1.w"].tobytes()
    stored = model_store.load_weights(model_store.resolve(str(q_dir)), "int8_float16")
    v, _ = read_model_bin(str(q_dir / "model.bin"))
    assert stored["dec.l0.fc1.w"].q.tobytes() == v["decoder/layer_0/ffn/linear_0/weight"].tobytes()
    assert model_store.load_weights(model_store.resolve("random:micro-test"), "int8_float16") is None


# --------------------------------------------------------------------------- backend
class RecordingEngine:
    """Records how the backend loads it; its lanes only ever idle (no request is sent)."""

    def __init__(self, dims, gpu, max_batch):
        self.dims, self.gpu, self.max_batch, self.calls = dims, gpu, max_batch, []

    def session_begin(self, cfg):
        pass

    def session_step(self, max_chunks=1, refill_min=1):
        return [], 0, 0

    def session_add(self, wins):
        raise AssertionError("no request is sent in these tests")

    def session_end(self):
        pass

    def load_weights(self, w):
        self.calls.append(("load_weights", w))

    def init_random(self, seed=0):
        self.calls.append(("init_random", seed))

    def close(self):
        pass


def _load(monkeypatch, mid, compute_type):
    engines = []

    def factory(dims, gpu, mb):
        engines.append(RecordingEngine(dims, gpu, mb))
        return engines[-1]
    if compute_type is None:
        monkeypatch.delenv("STT_COMPUTE_TYPE", raising=False)
    else:
        monkeypatch.setenv("STT_COMPUTE_TYPE", compute_type)
    monkeypatch.setenv("STT_HIP_GPUS", "0")
    monkeypatch.setenv("STT_HIP_LANES", "1")
    b = HipWhisperBackend(engine_factory=factory)
    b.load_model(mid)
    try:
        info = b.loaded_models()
    finally:
        b.unload_model(mid)
    assert len(engines) == 1 and len(info) == 1
    ct = info[0]["compute_type"] if isinstance(info[0], dict) else info[0].compute_type
    return engines[0].calls, ct


def test_backend_reads_stt_compute_type(monkeypatch, tmp_path):
    d = D.MICRO_TEST
    w = weights.random_weights(d, seed=9, emb_std=0.5)
    v, a = canonical_to_ct2(w, d)
    mdir = tmp_path / "micro_ct2"
    mdir.mkdir()
    write_model_bin(str(mdir / "model.bin"), v, a)
    names = set(weights.q8_names(d))

    calls, ct = _load(monkeypatch, str(mdir), "int8_float16")
    assert ct == "int8_float16" and [c[0] for c in calls] == ["load_weights"]
    got = calls[0][1]
    assert {n for n, x in got.items() if isinstance(x, weights.QuantizedMatrix)} == names

    calls8, ct8 = _load(monkeypatch, str(mdir), "int8")
    assert ct8 == "int8_float16" and isinstance(calls8[0][1]["dec.tok"], weights.QuantizedMatrix)

    base = model_store.load_weights(model_store.resolve(str(mdir)))
    for setting in (None, "float16"):
        calls, ct = _load(monkeypatch, str(mdir), setting)
        assert ct == "float16" and [c[0] for c in calls] == ["load_weights"]
        assert set(calls[0][1]) == set(base)
        assert all(calls[0][1][n].dtype == base[n].dtype and calls[0][1][n].tobytes() == base[n].tobytes() for n in base)

    # a model without weight files stays float16 and says so
    calls, ct = _load(monkeypatch, "random:micro-test", "int8_float16")
    assert ct == "float16" and [c[0] for c in calls] == ["init_random"]
