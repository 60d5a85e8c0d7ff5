#!/usr/bin/env python3
"""English-only golden: tests/golden/tiny_en_model.npz (run on CPU; committed).

transformers' fp32 ``WhisperForConditionalGeneration`` at ``TINY_EN_TEST`` dims (the tiny-test
model with the 51864-id vocabulary of ``tiny.en`` ... ``medium.en``) with the hash-initialised
weights the GPU regenerates (``english_ref.golden_weights``: ``weights.random_weights(d, SEED,
text_pos=AMP)``, the ``text_positional`` table, so ids change every step and have margins, with
a <|nospeech|> row that makes no_speech_prob far from 0), stepped by the loops of
``tests/english_ref.py`` (start sequence ``(sot,)``; ``tests/test_english_only_cpu.py`` pins those
loops against transformers' own ``generate``).  Three short clips (chirp, tone, noise), per clip:

* ``ts``      greedy with timestamps, no previous text: ids, sum_logprob, no_speech_prob, the raw
              logits of the first sampled step (the <|startoftranscript|> step), beam-5 ids
* ``nots4``   greedy without timestamps after a 4-token previous-text prefix
* ``nots223`` the same after a 223-token prefix (the longest faster-whisper keeps)

and, for clip 0, the word-timestamp reference of the short forced sequence
``[sot, no_timestamps, text..., eot]``: M, the DTW path's token frames, the token probabilities
and ``matrix_tol`` measured as tools/make_align_golden.py measures it.

The tool records the minimum top-2 margin of the processed logits over EVERY greedy step of
every case and clip (the <|endoftext|> steps included) and refuses to write a golden whose
minimum is below 0.02 (20x the project's 1e-3 log-softmax bound).

    python tools/make_english_golden.py [--out tests/golden]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden as mg  # noqa: E402
from make_align_golden import TINY_NOISE, default_heads, window_mel  # noqa: E402

import english_ref as eref  # noqa: E402
import align_ref  # noqa: E402
from open_speech_amd import dims as D  # noqa: E402
from open_speech_amd import synth  # noqa: E402
from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens  # noqa: E402
from oracle import decode as odec  # noqa: E402

SEED = 21
AMP = 60.0
# english_ref.golden_weights: no_speech_prob far from 0 where <|startoftranscript|> ends the prompt
# (position 0, the combined step).  Position 0 is sampled only under the initial-timestamp rule, so
# <|nospeech|> itself is never picked.
NOSPEECH_MIX = 2.5
SOT_POSITIONS = (0,)
MIN_MARGIN = 0.02
MAX_NEW = 40          # sampled tokens per case at most (every case takes seconds on the GPU)
BEAM = 5
ALIGN_TOKENS = 24
NOISE_SEEDS = 8


def clips():
    return {"chirp": synth.chirp_clip(3, 6.0), "tone": synth.tone_clip(4.2), "noise": synth.noise_clip(5, 5.0)}


def prefix_tokens(n: int) -> list:
    """n distinct text ids (previous text)."""
    return [int((i * 97 + 13) % 50000) for i in range(n)]


def cases(st):
    """name -> (previous-text tokens, without_timestamps, max_length)"""
    out = {}
    for name, n_prev, nots in (("ts", 0, False), ("nots4", 4, True), ("nots223", 223, True)):
        prev = prefix_tokens(n_prev)
        plen = len(eref.prompt_tokens(st, prev, nots))
        out[name] = (prev, nots, plen + MAX_NEW)
    return out


def cross_probs(model, enc, forced, heads):
    with torch.no_grad():
        o = model(encoder_outputs=(enc,), decoder_input_ids=torch.tensor([forced]), output_attentions=True,
                  use_cache=False)
    cross = np.stack([o.cross_attentions[l][0, h].numpy() for l, h in heads])
    return o.logits[0].double().numpy(), cross


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden"))
    a = ap.parse_args()
    torch.manual_seed(0)
    d = D.TINY_EN_TEST
    st = D.SpecialTokens.for_vocab(d.n_vocab)
    assert not st.multilingual
    model = mg.build_model(d, eref.golden_weights(d, SEED, AMP, NOSPEECH_MIX, SOT_POSITIONS))
    sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
    store, margins_all = {}, []
    meta = {"generator": "tools/make_english_golden.py", "seed": SEED, "text_pos": AMP, "nospeech_mix": NOSPEECH_MIX,
            "sot_positions": list(SOT_POSITIONS), "max_new": MAX_NEW,
            "beam": BEAM, "clips": list(clips()), "cases": {}}
    encs = {}
    for cname, pcm in clips().items():
        mel = mg.fe_mel(pcm, d.n_mels)
        size = mel.shape[1] - 1
        with torch.no_grad():
            enc = model.model.encoder(input_features=torch.from_numpy(window_mel(mel, 0, size))[None]).last_hidden_state
        encs[cname] = (enc, size)
        stepper = mg._HFStepper(model, enc)
        for name, (prev, nots, max_len) in cases(st).items():
            opts = odec.DecodeOptions(suppress_tokens=sup, without_timestamps=nots, max_length=max_len)
            mr = []
            r = eref.greedy_from_encoder(stepper, None, st, prev_tokens=prev, opts=opts, keep_logits=1, margins=mr)
            margins_all.extend(mr)
            key = f"{cname}/{name}"
            store[key + "/ids"] = np.array(r.tokens, np.int32)
            store[key + "/sum_logprob"] = np.float64(r.sum_logprob)
            store[key + "/no_speech_prob"] = np.float64(r.no_speech_prob)
            store[key + "/margins"] = np.array(mr, np.float64)
            meta["cases"][key] = {"n_ids": len(r.tokens), "distinct": len(set(r.tokens)), "min_margin": min(mr),
                                  "max_length": max_len}
            print(key, "n", len(r.tokens), "distinct", len(set(r.tokens)), "min margin", round(min(mr), 4),
                  "nsp", r.no_speech_prob, "first", r.tokens[:6])
            if name == "ts":
                store[key + "/first_logits"] = r.step_logits[0].astype(np.float32)
                b = eref.beam_from_encoder(stepper, None, st, opts=opts, beam=odec.BeamOptions(beam_size=BEAM))
                store[key + "/beam_ids"] = np.array(b.tokens, np.int32)
                store[key + "/beam_sum_logprob"] = np.float64(b.sum_logprob)
                print(key, "beam n", len(b.tokens), "score", b.sum_logprob, "equal to greedy:", b.tokens == r.tokens)
    mm = float(min(margins_all))
    assert mm >= MIN_MARGIN, f"minimum top-2 margin {mm} over {len(margins_all)} steps is below {MIN_MARGIN}"
    meta["min_top2_margin"] = mm
    meta["steps_compared"] = len(margins_all)

    # word timestamps on clip 0: the short forced sequence
    enc, size = encs["chirp"]
    text = [int(t) for t in store["chirp/ts/ids"] if t < st.eot][:ALIGN_TOKENS]
    n = len(text)
    assert n >= 8
    forced = eref.forced_sequence(st, text)
    heads = default_heads(d)
    logits, cross = cross_probs(model, enc, forced, heads)
    M = eref.alignment_matrix(cross, n, size)
    ti, fi = align_ref.dtw(-M)
    dm = 0.0
    for s in range(NOISE_SEEDS):
        rng = np.random.default_rng(1000 + s)
        e2 = enc + torch.from_numpy(rng.uniform(-TINY_NOISE, TINY_NOISE, size=tuple(enc.shape)).astype(np.float32))
        dm = max(dm, float(np.abs(eref.alignment_matrix(cross_probs(model, e2, forced, heads)[1], n, size) - M).max()))
    store["align/tokens"] = np.array(text, np.int32)
    store["align/num_frames"] = np.int32(size)
    store["align/M"] = M
    store["align/token_frame"] = align_ref.token_frames(ti, fi).astype(np.int32)
    store["align/text_indices"] = ti.astype(np.int32)
    store["align/time_indices"] = fi.astype(np.int32)
    store["align/token_prob"] = eref.token_probs(logits, st, text)
    store["align/matrix_tol"] = np.float64(2 * dm)
    print("align: n", n, "M", M.shape, "matrix_tol", 2 * dm)

    path = os.path.join(a.out, "tiny_en_model.npz")
    np.savez_compressed(path, **store)
    print("wrote", path, os.path.getsize(path), "bytes; min top-2 margin", mm, "over", len(margins_all), "steps")
    assert os.path.getsize(path) < (1 << 20)
    with open(os.path.join(a.out, "tiny_en_model.json"), "w") as fh:
        json.dump(meta, fh, indent=1)


if __name__ == "__main__":
    main()
