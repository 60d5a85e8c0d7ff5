"""Reference loops for English-only Whisper models (``tiny.en`` ... ``medium.en``), test
infrastructure only.

``oracle/decode.py`` restates faster-whisper's loops for multilingual models, whose start
sequence is ``[sot, language, task]``.  faster-whisper's ``Tokenizer`` gives a model that is not
multilingual ``sot_sequence = (sot,)``: the prompt is ``[<|startofprev|>, prev..., sot]`` (plus
``<|notimestamps|>`` with ``without_timestamps``), ``no_speech_prob`` is
``softmax(raw logits at the sot position)[no_speech]`` whether or not ``sot`` ends the prompt,
and with timestamps the first sampled token comes from those same logits after the rules at
``n_sampled = 0``.  The loops below are ``oracle.decode``'s with that start sequence; the logits
rules, the log-softmax, the draw and the beam bookkeeping are the oracle's own functions.

The alignment part restates the forced pass of openai-whisper's ``find_alignment`` as
faster-whisper calls it for such a model: the forced sequence is
``[sot, no_timestamps, text..., eot]`` and the rows kept for the matrix are
``[no_timestamps, text...]`` (position 1 on, not 3 on).
"""
from __future__ import annotations

import copy

import numpy as np

from oracle.decode import (MODEL_MAX_LENGTH, BeamOptions, DecodeOptions, WindowResult, _norm_score, log_softmax,
                           process_logits, sample_token)

import align_ref


def golden_weights(d, seed: int, amp: float, nospeech_mix: float, sot_positions=(0,)) -> dict:
    """The weights of tests/golden/tiny_en_model.npz (tools/make_english_golden.py):
    ``weights.random_weights(d, seed, text_pos=amp)`` with the <|nospeech|> embedding row set to
    ``nospeech_mix`` times the sum of the text-target rows of the positions where the goldens'
    prompts hold <|startoftranscript|>.  With the tied output projection no_speech_prob is then
    far from 0 at those positions (plain random weights give about 1 / n_vocab, which a
    tolerance of 2e-3 cannot tell from a missing value)."""
    from open_speech_amd import weights
    from open_speech_amd.dims import SpecialTokens
    w = weights.random_weights(d, seed=seed, text_pos=amp)
    st = SpecialTokens.for_vocab(d.n_vocab)
    text, _ = weights.text_targets(d, seed)
    tok = w["dec.tok"].astype(np.float32)
    tok[st.no_speech] = nospeech_mix * sum(tok[int(text[p])] for p in sot_positions)
    w["dec.tok"] = tok.astype(w["dec.tok"].dtype)
    return w


def prompt_tokens(st, prev_tokens=(), without_timestamps: bool = False) -> list:
    """[<|startofprev|>, prev[-223:]..., sot(, no_timestamps)]"""
    p = []
    if len(prev_tokens):
        p.append(st.sot_prev)
        p.extend(int(t) for t in list(prev_tokens)[-(MODEL_MAX_LENGTH // 2 - 1):])
    p.append(st.sot)
    if without_timestamps:
        p.append(st.no_timestamps)
    return p


def _feed_prompt(oracle, xkv, st, prev_tokens, opts):
    """Feed the prompt; returns (cache, next position, logits after the last prompt token,
    no_speech_prob from the raw sot logits, prompt length)."""
    cache = oracle.new_cache()
    prompt = prompt_tokens(st, prev_tokens, opts.without_timestamps)
    nsp, lg = None, None
    for pos, t in enumerate(prompt):
        lg = oracle.decoder_step(t, pos, cache, xkv)
        if t == st.sot:
            nsp = float(np.exp(log_softmax(lg)[st.no_speech]))
    return cache, len(prompt), lg, nsp, len(prompt)


def greedy_from_encoder(oracle, xkv, st, *, prev_tokens=(), opts: DecodeOptions = DecodeOptions(),
                        keep_logits: int = 0, margins: list | None = None) -> WindowResult:
    """``margins``, if a list, receives the top-2 margin of the processed logits at every
    sampled step (the <|endoftext|> step included)."""
    cache, pos, lg, nsp, prompt_len = _feed_prompt(oracle, xkv, st, prev_tokens, opts)
    sampled, sum_lp, step_logits = [], 0.0, []
    while True:
        if keep_logits and len(step_logits) < keep_logits:
            step_logits.append(lg.copy())
        x = process_logits(lg, sampled, st, opts)
        nxt = int(np.argmax(x))
        if margins is not None:
            top = np.partition(x, -2)[-2:]
            margins.append(float(top[1] - top[0]))
        sum_lp += float(log_softmax(x)[nxt])
        if nxt == st.eot:
            break
        sampled.append(nxt)
        if prompt_len + len(sampled) >= opts.max_length:
            break
        lg = oracle.decoder_step(nxt, pos, cache, xkv)
        pos += 1
    return WindowResult(tokens=sampled, sum_logprob=sum_lp, no_speech_prob=nsp, language=-1, step_logits=step_logits)


def sample_from_encoder(oracle, xkv, st, *, temperature: float, seed: int, row: int, prev_tokens=(),
                        opts: DecodeOptions = DecodeOptions()) -> WindowResult:
    """One sampled row: every pick is the device's Gumbel-max draw (``oracle.decode.sample_token``
    at the row's decoder step), its log-probability under the rule-masked, untempered
    distribution."""
    cache, pos, lg, nsp, prompt_len = _feed_prompt(oracle, xkv, st, prev_tokens, opts)
    sampled, sum_lp = [], 0.0
    while True:
        x = process_logits(lg, sampled, st, opts)
        nxt = sample_token(x, 1.0 / temperature, seed, row, pos - 1)
        sum_lp += float(log_softmax(x)[nxt])
        if nxt == st.eot:
            break
        sampled.append(nxt)
        if prompt_len + len(sampled) >= opts.max_length:
            break
        lg = oracle.decoder_step(nxt, pos, cache, xkv)
        pos += 1
    return WindowResult(tokens=sampled, sum_logprob=sum_lp, no_speech_prob=nsp, language=-1)


def replay_draws(step_logits, st, opts: DecodeOptions, temperature: float, seed: int, row: int, prompt_len: int):
    """The draws of one sampled row replayed on given raw logits (``step_logits[i]``: the logits
    of the row's i-th sampled step, at decoder step ``prompt_len - 1 + i``): (tokens, sum_logprob)
    up to <|endoftext|>, max_length or the last logits given."""
    sampled, sum_lp = [], 0.0
    for i, lg in enumerate(step_logits):
        x = process_logits(np.asarray(lg), sampled, st, opts)
        nxt = sample_token(x, 1.0 / temperature, seed, row, prompt_len - 1 + i)
        sum_lp += float(log_softmax(x)[nxt])
        if nxt == st.eot:
            break
        sampled.append(nxt)
        if prompt_len + len(sampled) >= opts.max_length:
            break
    return sampled, sum_lp


def beam_from_encoder(oracle, xkv, st, *, prev_tokens=(), opts: DecodeOptions = DecodeOptions(),
                      beam: BeamOptions = BeamOptions()) -> WindowResult:
    """``oracle.decode.beam_from_encoder`` (the CTranslate2 BeamSearch restatement) from the
    English-only prompt."""
    cache, pos, lg, nsp, prompt_len = _feed_prompt(oracle, xkv, st, prev_tokens, opts)
    K = beam.beam_size
    V = lg.shape[0]
    max_cand = int(round(K * beam.patience))
    alive = [([], 0.0, cache, lg)]
    finished = []
    n = 0
    while True:
        is_last = prompt_len + n + 1 >= opts.max_length
        scores = []
        for seq, cum, _, logit in alive:
            lp = log_softmax(process_logits(logit, seq, st, opts)).astype(np.float32)
            scores.append(np.float32(cum) + lp)
        flat = np.concatenate(scores)
        order = np.lexsort((np.arange(flat.size), -flat.astype(np.float64)))[:2 * K]
        cands = [(float(flat[i]), int(i) // V, int(i) % V) for i in order]
        chosen, sec, top_fin = [], K, False
        for k in range(K):
            s, q, tok = cands[k]
            nb = k
            if tok == st.eot or is_last:
                if k == 0:
                    top_fin = True
                toks = list(alive[q][0]) + ([] if tok == st.eot else [tok])
                n_len = len(toks) + (1 if beam.length_counts_eot and tok == st.eot else 0)
                finished.append((_norm_score(s, n_len, beam.length_penalty), s, toks))
                for j in range(sec, 2 * K):
                    if cands[j][2] != st.eot:
                        nb, sec = j, j + 1
                        break
            chosen.append(cands[nb])
        if is_last or (top_fin and len(finished) >= beam.num_hypotheses) or len(finished) >= max_cand:
            break
        nxt = []
        for s, q, tok in chosen:
            seq, _, cch, _ = alive[q]
            c2 = copy.deepcopy(cch)
            nxt.append((list(seq) + [tok], s, c2, oracle.decoder_step(tok, pos, c2, xkv)))
        alive = nxt
        pos += 1
        n += 1
    best = finished[0]
    for f in finished[1:]:
        if f[0] > best[0]:
            best = f
    return WindowResult(tokens=best[2], sum_logprob=best[1], no_speech_prob=nsp, language=-1,
                        hypotheses=[(f[2], f[1], f[0]) for f in finished])


# ------------------------------------------------------------ word timestamps
ALIGN_HEAD = 1   # forced positions before <|notimestamps|>, the first row kept (multilingual: 3)


def forced_sequence(st, text_tokens) -> list:
    return [st.sot, st.no_timestamps] + [int(t) for t in text_tokens] + [st.eot]


def alignment_matrix(cross: np.ndarray, n: int, num_frames: int, width: int = 7) -> np.ndarray:
    """M [n + 1][F] from the alignment heads' cross-attention probabilities ``cross``
    [heads][n + 3][1500] of the forced pass: crop to F = num_frames // 2 frames, normalise per
    (head, frame) over all positions (population std), median filter along the frames, mean
    over the heads, rows 1 .. n + 1."""
    w = np.asarray(cross, dtype=np.float32)[..., : num_frames // 2]
    mean = w.mean(axis=-2, keepdims=True, dtype=np.float32)
    std = np.sqrt(((w - mean) ** 2).mean(axis=-2, keepdims=True, dtype=np.float32))
    w = align_ref.median_filter((w - mean) / std, width)
    return w.mean(axis=0, dtype=np.float32)[ALIGN_HEAD:n + ALIGN_HEAD + 1].astype(np.float32)


def token_probs(logits: np.ndarray, st, text_tokens) -> np.ndarray:
    """softmax(logits[1 + k][:eot])[t_k] of the forced pass's logits [n + 3][V]."""
    return np.array([float(np.exp(log_softmax(np.asarray(logits[ALIGN_HEAD + k][:st.eot]))[int(t)]))
                     for k, t in enumerate(text_tokens)])


# ------------------------------------------------------------ transformers as the pin
def hf_english_model(d, w):
    """transformers' fp32 ``WhisperForConditionalGeneration`` at dims ``d`` with the canonical
    weights ``w`` and the generation config of an ``.en`` checkpoint (``is_multilingual`` False,
    ``decoder_start_token_id`` = sot, ``begin_suppress_tokens`` [blank, eot],
    ``max_initial_timestamp_index`` 50)."""
    import torch
    from transformers import GenerationConfig, WhisperConfig, WhisperForConditionalGeneration

    from open_speech_amd import weights
    from open_speech_amd.dims import SpecialTokens
    from open_speech_amd.tokenizer import WhisperTokenizer, get_suppressed_tokens
    st = SpecialTokens.for_vocab(d.n_vocab)
    cfg = WhisperConfig(vocab_size=d.n_vocab, num_mel_bins=d.n_mels, encoder_layers=d.n_audio_layer,
                        encoder_attention_heads=d.n_audio_head, decoder_layers=d.n_text_layer,
                        decoder_attention_heads=d.n_text_head, d_model=d.n_audio_state,
                        encoder_ffn_dim=4 * d.n_audio_state, decoder_ffn_dim=4 * d.n_text_state,
                        max_source_positions=d.n_audio_ctx, max_target_positions=d.n_text_ctx,
                        pad_token_id=st.eot, bos_token_id=st.eot, eos_token_id=st.eot,
                        decoder_start_token_id=st.sot, attn_implementation="eager")
    model = WhisperForConditionalGeneration(cfg).eval()
    sd = {k: torch.from_numpy(v) for k, v in weights.to_hf_state_dict(w, d).items()}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not [m for m in missing if not m.endswith("k_proj.bias")] and not unexpected
    sup = get_suppressed_tokens(WhisperTokenizer(d.n_vocab), [-1])
    model.generation_config = GenerationConfig(
        is_multilingual=False, decoder_start_token_id=st.sot, no_timestamps_token_id=st.no_timestamps,
        prev_sot_token_id=st.sot_prev, begin_suppress_tokens=[st.blank, st.eot], suppress_tokens=list(sup),
        max_initial_timestamp_index=50, eos_token_id=st.eot, pad_token_id=st.eot, bos_token_id=st.eot,
        max_length=d.n_text_ctx)
    return model, sup


def hf_window_features(pcm, n_mels: int):
    """(input_features [1][n_mels][3000], content frames): transformers' extractor on
    faster-whisper's 160-sample-padded waveform, the window's frames zero padded to 30 s."""
    import torch
    from transformers import WhisperFeatureExtractor
    x = np.pad(np.asarray(pcm, np.float32) / 32768.0, (0, 160))
    mel = WhisperFeatureExtractor(feature_size=n_mels)._np_extract_fbank_features(x[None, :], "cpu")[0]
    size = mel.shape[1] - 1
    win = np.zeros((n_mels, 3000), np.float32)
    win[:, :size] = mel[:, :size]
    return torch.from_numpy(win)[None], size


class HFStepper:
    """``oracle.model.WhisperOracle``'s decoder-step interface over the transformers model."""

    def __init__(self, model, enc):
        self.model, self.enc = model, enc

    def new_cache(self):
        return {"past": None}

    def decoder_step(self, tok, pos, cache, xkv):
        import torch
        with torch.no_grad():
            o = self.model(encoder_outputs=(self.enc,), decoder_input_ids=torch.tensor([[int(tok)]]),
                           past_key_values=cache["past"], use_cache=True)
        cache["past"] = o.past_key_values
        return o.logits[0, -1].float().numpy()
