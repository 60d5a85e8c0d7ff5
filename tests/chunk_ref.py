"""References for the shorter encoder windows (faster-whisper's ``chunk_length``: nb_max_frames =
100 s mel frames, T = 50 s encoder positions, s = 1..30), restated with the window length as a
parameter where the 30 s references hard-code it:

* ``window_x1``: tests/mel_ref.py's ``window_x1`` (mel_window_kernel) with the frame count;
* ``enc_inputs`` / ``xattn_inputs``: peaked attention inputs in the style of tests/attn_ref.py at
  any T.  The encoder's marker key T - 1 ties with one mid key, so a tail tile that kept clamped
  duplicates of the last key would move the output; the cross-attention markers sit on both sides
  of every chunk edge ceil(T / 8) j;
* ``seek_loop``: oracle/seek.py's loop with ``nb_max_frames`` in place of 3000 (restated from
  faster-whisper's ``generate_segments``: ``segment_size = min(nb_max_frames, content_frames -
  seek)``, everything else unchanged).
"""
import numpy as np

import attn_ref as R
import mel_ref as M

HD = R.HD
XCH = R.XCH


def xper(T):
    """Keys per cross-attention chunk (decode.hip: per = ceil(T / XCH))."""
    return (T + XCH - 1) // XCH


def no_chunk_empty(T):
    """The last chunk's first key lies inside the window (what osw_create requires)."""
    return (XCH - 1) * xper(T) < T


def chunk_forms(T):
    """(keys per lane of the greedy kernel, key tiles per wave of the MFMA kernel) the launcher
    picks at T: ceil(per / 32), ceil(per / 64)."""
    per = xper(T)
    return (per + 31) // 32, (per + 63) // 64


# --------------------------------------------------------------------------- window packing
def window_x1(raw, gmax, seek, size, n_mels, n_fr):
    """mel_window_kernel for one window of n_fr frames -> fp16 bits [n_fr + 2][C1]."""
    nf = raw.shape[0]
    assert 0 <= seek < nf and size >= 1 and raw.shape[1] == n_mels
    seg = min(min(size, n_fr), nf - seek)
    out = np.zeros((n_fr + 2, M.c1_of(n_mels)), np.float16)
    out[1:1 + seg, :n_mels] = M._normalized(raw[seek:seek + seg], gmax).astype(np.float16)
    return out.view(np.uint16)


# --------------------------------------------------------------------------- attention inputs
def enc_mid_key(T):
    return T // 2 - 3


def enc_inputs(nb, H, T, seed=0):
    """attn_ref.enc_inputs at T keys: rho ramps by +1 per 64-key tile, rho[mid] = rho[T - 1] = 30,
    query gains spread over [-64, 64]."""
    rng = R._rng(1000 + 7 * T + seed)
    qkv = np.empty((3, nb, H, T, HD), np.float16)
    rho = (np.arange(T) // R.ENC_KB).astype(np.float64)
    rho[enc_mid_key(T)] = rho[T - 1] = 30.0
    for b in range(nb):
        for h in range(H):
            e = R._direction(rng)
            gamma = rng.uniform(-R.ENC_GAIN, R.ENC_GAIN, T)
            qkv[0, b, h] = gamma[:, None] * e + rng.uniform(-0.125, 0.125, (T, HD))
            qkv[1, b, h] = rho[:, None] * e + rng.uniform(-0.125, 0.125, (T, HD))
            qkv[2, b, h] = rng.uniform(-1.0, 1.0, (T, HD))
    return qkv


def x_markers(T):
    """Key 0, both sides of every chunk edge per * j (j = 1..7), and the last key."""
    per = xper(T)
    mk = {0, T - 1}
    for j in range(1, XCH):
        mk.update((per * j - 1, per * j))
    assert max(mk) == T - 1 and min(mk) == 0
    return sorted(mk)


def xattn_inputs(W, H, T, beam, ks, seed=0, with_bias=True):
    """attn_ref.xattn_inputs at T keys: rho = 4 at x_markers(T), -4 on the rest of chunk 3, 0
    elsewhere; the four row kinds of attn_ref.X_ROW_KINDS."""
    rng = R._rng(3000 + 11 * T + seed)
    rows, D = W * beam, H * HD
    per = xper(T)
    K = np.empty((W, H, T, HD), np.float16)
    V = rng.uniform(-1.0, 1.0, (W, H, T, HD)).astype(np.float16)
    rho = np.zeros(T)
    rho[3 * per:4 * per] = -4.0
    rho[x_markers(T)] = 4.0
    q = np.empty((rows, D))
    kinds = np.empty((rows, H), dtype=object)
    for w in range(W):
        for h in range(H):
            e = R._direction(rng)
            f = R._orthogonal(e, rng)
            K[w, h] = rho[:, None] * e + 5.0 * f + rng.uniform(-1 / 64, 1 / 64, (T, HD))
            for b in range(beam):
                r = w * beam + b
                kind = R.X_ROW_KINDS[(r + h) % 4]
                kinds[r, h] = kind
                base = {"markers": 320.0 * e, "low": -320.0 * e, "far": -320.0 * f, "uniform": 0.0 * e}[kind]
                q[r, h * HD:(h + 1) * HD] = base + rng.uniform(-0.25, 0.25, HD)
    slabs, bias = R.split_slabs(R._q16(q), ks, rng, with_bias)
    return slabs, bias, K, V, kinds


def marker_weights(q_slabs, bias, K, beam, kinds, T):
    """Smallest softmax weight of a marker key over the "markers" rows (float64): the markers must
    all carry weight, or a dropped or doubled edge key would not move the output."""
    q = R.reduce_slabs(q_slabs, bias).astype(np.float64)
    rows, D = q.shape
    lo = 1.0
    for r in range(rows):
        for h in range(D // HD):
            if kinds[r, h] != "markers":
                continue
            s = q[r, h * HD:(h + 1) * HD] @ K[r // beam, h].astype(np.float64).T * 0.125
            p = np.exp(s - s.max())
            lo = min(lo, float((p / p.sum())[x_markers(T)].min()))
    return lo


# --------------------------------------------------------------------------- seek loop
def seek_loop(decode_window, n_frames, st, decode_text, nb_max_frames, opts=None, initial_tokens=()):
    """oracle.seek.seek_loop with windows of nb_max_frames mel frames."""
    from oracle import seek as S
    opts = opts or S.SeekOptions()
    content = max(0, n_frames - 1)
    seek, all_tokens, reset_since, out = 0, list(initial_tokens), 0, []
    while seek < content:
        size = min(nb_max_frames, content - seek)
        prev = all_tokens[reset_since:]
        prompt = ([st.sot_prev] + prev[-(448 // 2 - 1):]) if prev else []
        tokens, sum_lp, nsp = decode_window(seek, size, prompt)
        w = S.Window(seek, size, prompt, list(tokens))
        out.append(w)
        avg = sum_lp / (len(tokens) + 1)
        if opts.no_speech_threshold is not None and nsp > opts.no_speech_threshold and not (
                opts.log_prob_threshold is not None and avg > opts.log_prob_threshold):
            w.skipped = True
            seek += size
            continue
        segs, new_seek = S.split_by_timestamps(list(tokens), st.timestamp_begin, seek * S.FRAME_SEC, size,
                                               size * S.FRAME_SEC, seek)
        for a, b, t in segs:
            if a == b or not decode_text(t).strip():
                continue
            all_tokens.extend(t)
            w.segments.append((a, b, list(t)))
        if not opts.condition_on_previous_text:
            reset_since = len(all_tokens)
        seek = new_seek
    return out
