"""Model widths between the two the rest of the suite runs (384 and 1280): 256, and Whisper
base / small / medium (512, 768, 1024), whose LayerNorm instantiations (layernorm4_kernel<2|3|4>)
and GEMM shapes nothing else reaches; and the osw_create contract for the widths no kernel serves.

Per width: one encoder block and a 32-step greedy decode against the fp16-emulating oracle, at
the bounds of the tiny-dims parity tests, and the three decoder-step forms bit for bit.  The
weights are the varied-text kind (weights.text_positional, amplitude 80, seed 2): on the CPU the
oracle alone decodes 32 distinct ids at every width with a smallest top-2 margin of 0.72 (256),
2.4 (512), 3.5 (768) and 4.4 (1024), so every step is compared.
"""
import ctypes as C

import numpy as np
import pytest

from open_speech_amd import _lib
from open_speech_amd import dims as D
from open_speech_amd import synth, weights
from open_speech_amd.engine import DecodeConfig, WhisperEngine
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens

pytestmark = pytest.mark.gpu

SEED, TEXT_AMP, STEPS = 2, 80.0, 32


def _dims(width):
    return D.WhisperDims(n_mels=80, n_audio_state=width, n_audio_head=width // 64, n_audio_layer=1,
                         n_text_state=width, n_text_head=width // 64, n_text_layer=2)


@pytest.mark.parametrize("width", [640, 896, 1152])
def test_create_rejects_widths_without_kernels(width):
    """A multiple of 128 that launch_layernorm has no instantiation for: OSW_EINVAL from
    osw_create, before any allocation or launch."""
    d = _dims(width)
    lib = _lib.load()
    cd = _lib.osw_dims(d.n_mels, d.n_audio_ctx, d.n_audio_state, d.n_audio_head, d.n_audio_layer, d.n_vocab,
                       d.n_text_ctx, d.n_text_state, d.n_text_head, d.n_text_layer)
    ctx = C.c_void_p()
    assert lib.osw_create(C.byref(cd), 0, 1, C.byref(ctx)) == -22
    assert not ctx.value
    assert b"width" in lib.osw_last_error()
    with pytest.raises(_lib.OswError) as ei:
        WhisperEngine(d, device=0, max_batch=1)
    assert ei.value.rc == -22


@pytest.fixture(scope="module", params=[256, 512, 768, 1024])
def model(request):
    from oracle.model import WhisperOracle
    d = _dims(request.param)
    w = weights.random_weights(d, seed=SEED, text_pos=TEXT_AMP)
    eng = WhisperEngine(d, device=0, max_batch=12)
    eng.load_weights(w)
    yield d, eng, WhisperOracle(d, w, fp16=True)
    eng.close()


def test_encoder_layer_matches_oracle(model):
    d, eng, orc = model
    n = d.n_audio_ctx * d.n_audio_state
    x = weights.hash_uniform(77, 0, n, 1.0, 0.0).reshape(d.n_audio_ctx, d.n_audio_state)
    y = eng.encoder_layer(0, x)
    ref = orc.encoder_layer(0, x)
    err = np.abs(y - ref)
    print(f"width {d.n_audio_state}: encoder_layer max |err| {err.max():.3e} mean {err.mean():.3e}")
    # the bounds of test_tiny_encoder_matches_oracle_and_golden
    np.testing.assert_allclose(y, ref, atol=2e-2, rtol=0)
    assert err.mean() < 2e-3


def test_greedy_matches_oracle(model):
    from oracle import decode as odec
    d, eng, orc = model
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    eng.log_mel([synth.chirp_clip(3, 30.0)])
    eng.encode([(0, 0, 3000)])
    enc = eng.encoder_output(0)
    sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
    out = eng.decode(1, DecodeConfig(suppress_tokens=sup, max_length=3 + STEPS), dump_steps=4)[0]
    opts = odec.DecodeOptions(suppress_tokens=sup, max_length=3 + STEPS)
    r = odec.greedy_from_encoder(orc, orc.cross_kv(enc), st, opts=opts, keep_logits=STEPS)
    for i in range(4):
        e = np.abs(out.logits[i] - r.step_logits[i]).max()
        print(f"width {d.n_text_state}: step {i} logits max |err| {e:.3e}")
        np.testing.assert_allclose(out.logits[i], r.step_logits[i], atol=2e-2, rtol=0)
    # ids are compared while the oracle's own top-2 margin is clear (a near-tie may go either way)
    n_cmp = 0
    for i, lg in enumerate(r.step_logits):
        x = np.sort(odec.process_logits(lg, r.tokens[:i], st, opts))
        if x[-1] - x[-2] < 0.1:
            break
        n_cmp = i + 1
    assert n_cmp >= 24, n_cmp
    assert len(set(r.tokens[:n_cmp])) >= 16
    assert out.tokens[:n_cmp] == r.tokens[:n_cmp]
    assert out.language == r.language


def test_decoder_step_forms_bit_identical(model):
    """1, 3 and 12 rows (the three decoder-step forms, as the test of the same name at tiny dims)."""
    d, eng, _ = model
    sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
    cfg = DecodeConfig(suppress_tokens=sup, max_length=3 + STEPS)
    pcm = synth.chirp_clip(13, 30.0)
    got = {}
    for n in (1, 3, 12):
        eng.log_mel([pcm] * n)
        eng.encode([(i, 0, 3000) for i in range(n)])
        outs = eng.decode(n, cfg, dump_steps=6)
        for o in outs:
            assert o.tokens == outs[0].tokens
        got[n] = outs[-1]
    for n in (3, 12):
        assert got[n].tokens == got[1].tokens
        for i in range(len(got[1].logits)):
            np.testing.assert_array_equal(got[n].logits[i], got[1].logits[i], err_msg=f"rows {n} step {i}")
