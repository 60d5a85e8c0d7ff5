"""Model id -> weights + dims + tokenizer, offline only.

Mirrors where the reference finds models (``src/backends/faster_whisper.py:93-208``:
``STT_MODEL_DIR`` or the HuggingFace hub cache, ``models--Org--Name`` dirs) and
what ``WhisperModel(model_id, ...)`` accepts (an id or a local directory).
Supported on-disk formats:

* a transformers Whisper checkpoint: ``config.json`` + ``model.safetensors``
  (e.g. ``openai/whisper-large-v3-turbo``), optional ``tokenizer.json``;
* ``random:<preset>[:<seed>]`` — deterministic random weights at a preset's dims
  (``large-v3-turbo``, ``tiny-test``, ``micro-test``) for benchmarking and tests.

* a CTranslate2 directory: ``model.bin`` (+ ``tokenizer.json``) — the format of the
  reference's default ``deepdml/faster-whisper-large-v3-turbo-ct2`` (``ct2.py``).

Nothing here downloads.
"""
from __future__ import annotations

import glob
import json
import os
from dataclasses import dataclass

import numpy as np

from .dims import PRESETS, WhisperDims
from .weights import dims_from_hf_config, from_hf_state_dict


@dataclass
class ModelSource:
    model_id: str
    dims: WhisperDims
    kind: str               # "random" | "hf" | "ct2"
    path: str | None = None
    seed: int = 0
    tokenizer_json: str | None = None


def cache_dirs(model_dir: str | None) -> list[str]:
    out = []
    if model_dir:
        out.append(model_dir)
    for env in ("HF_HUB_CACHE", "HUGGINGFACE_HUB_CACHE"):
        if os.environ.get(env):
            out.append(os.environ[env])
    out.append(os.path.join(os.path.expanduser("~"), ".cache", "huggingface", "hub"))
    return out


def _snapshot_dirs(model_id: str, model_dir: str | None) -> list[str]:
    cands = []
    if os.path.isdir(model_id):
        cands.append(model_id)
    safe = "models--" + model_id.replace("/", "--")
    for root in cache_dirs(model_dir):
        cands.extend(sorted(glob.glob(os.path.join(root, safe, "snapshots", "*"))))
        p = os.path.join(root, model_id.split("/")[-1])
        if os.path.isdir(p):
            cands.append(p)
    return cands


def resolve(model_id: str, model_dir: str | None = None, chunk_length: int | None = None) -> ModelSource:
    """``chunk_length`` (seconds, 1..30; None: the checkpoint's own window): the source's dims with
    ``n_audio_ctx = 50 * chunk_length``; the loaders crop the encoder positional table to it."""
    src = _resolve(model_id, model_dir)
    if chunk_length is not None:
        short = src.dims.with_chunk_length(chunk_length)
        if short.n_audio_ctx > src.dims.n_audio_ctx:
            raise ValueError(f"chunk_length {chunk_length} needs {short.n_audio_ctx} encoder positions; model "
                             f"{model_id!r} has {src.dims.n_audio_ctx}")
        src.dims = short
    return src


def _resolve(model_id: str, model_dir: str | None = None) -> ModelSource:
    if model_id.startswith("random:"):
        parts = model_id.split(":")
        preset = parts[1] if len(parts) > 1 else "large-v3-turbo"
        if preset not in PRESETS:
            raise ValueError(f"unknown preset {preset!r}; choose from {sorted(PRESETS)}")
        seed = int(parts[2]) if len(parts) > 2 else 0
        return ModelSource(model_id, PRESETS[preset], "random", seed=seed)
    for d in _snapshot_dirs(model_id, model_dir):
        cfg = os.path.join(d, "config.json")
        st = sorted(glob.glob(os.path.join(d, "model*.safetensors")))
        tok = os.path.join(d, "tokenizer.json")
        if os.path.exists(cfg) and st:
            with open(cfg) as fh:
                dims = dims_from_hf_config(json.load(fh))
            return ModelSource(model_id, dims, "hf", path=d, tokenizer_json=tok if os.path.exists(tok) else None)
        mb = os.path.join(d, "model.bin")
        if os.path.exists(mb):
            from .ct2 import dims_from_ct2, read_model_bin

            v, _ = read_model_bin(mb)
            return ModelSource(model_id, dims_from_ct2(v), "ct2", path=d,
                               tokenizer_json=tok if os.path.exists(tok) else None)
    raise FileNotFoundError(f"model {model_id!r} not found locally (searched {cache_dirs(model_dir)}); "
                            "this backend never downloads")


def alignment_heads(src: ModelSource) -> list | None:
    """The (layer, head) pairs word timing reads: ``alignment_heads`` of an HF checkpoint's
    ``generation_config.json`` or of a CTranslate2 directory's ``config.json`` (what
    CTranslate2's ``align`` uses [upstream]).  None: the engine's default, every head of the
    last ``n_text_layer // 2`` layers (random-weight models have no file to read)."""
    if not src.path:
        return None
    for name in ("generation_config.json", "config.json"):
        f = os.path.join(src.path, name)
        if not os.path.exists(f):
            continue
        try:
            with open(f) as fh:
                heads = json.load(fh).get("alignment_heads")
        except (OSError, ValueError, AttributeError):
            continue
        if heads:
            pairs = [(int(l), int(h)) for l, h in heads]
            if all(0 <= l < src.dims.n_text_layer and 0 <= h < src.dims.n_text_head for l, h in pairs):
                return pairs
    return None


INT8_COMPUTE_TYPES = ("int8_float16", "int8")


def int8_decoder(compute_type: str | None) -> bool:
    """Whether ``STT_COMPUTE_TYPE`` asks for int8 decoder weights.  ``int8`` means what
    ``int8_float16`` means here: the activations stay float16 pairs on this backend either way."""
    return (compute_type or "").strip().lower() in INT8_COMPUTE_TYPES


def load_weights(src: ModelSource, compute_type: str | None = None) -> dict | None:
    """Canonical weights for a resolved source (None for random init).  compute_type ``int8_float16``
    / ``int8``: the decoder matrices come back as ``weights.QuantizedMatrix`` — a CTranslate2 file's
    stored int8 as it is, float checkpoints quantised per row at load, as CTranslate2 does.  Anything
    else, or None: float16, exactly as before."""
    q8 = int8_decoder(compute_type)
    w = None
    if src.kind == "hf":
        w = load_hf_weights(src)
    elif src.kind == "ct2":
        from .ct2 import ct2_to_canonical, read_model_bin

        v, aliases = read_model_bin(os.path.join(src.path, "model.bin"))
        w = ct2_to_canonical(v, aliases, src.dims, keep_int8=True) if q8 else ct2_to_canonical(v, aliases, src.dims)
    if w is not None and q8:
        from .weights import quantize_decoder

        w = quantize_decoder(w, src.dims)
    return w


def load_hf_weights(src: ModelSource) -> dict:
    from safetensors.numpy import load_file

    sd = {}
    for f in sorted(glob.glob(os.path.join(src.path, "model*.safetensors"))):
        for k, v in load_file(f).items():
            sd[k] = v.astype(np.float32) if v.dtype != np.float32 else v
    if "model.decoder.embed_tokens.weight" not in sd:
        raise ValueError("not a Whisper checkpoint (no model.decoder.embed_tokens.weight)")
    return from_hf_state_dict(sd, src.dims)
