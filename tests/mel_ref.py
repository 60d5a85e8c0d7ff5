"""References, inputs and float32 restatements for the log-mel front end (csrc/mel.hip):
mel_logmel_kernel with the host-built tables of setup_mel, the per-clip maximum, and the two
element-wise kernels behind osw_get_mel and the conv stem's operand X1.  Plain numpy, no GPU.
tests/test_gpu_mel.py runs the kernels against these (osw_debug_get_logmel / osw_debug_mel_windows);
tests/test_mel_ref_cpu.py shows that the bound below is met by a faithful float32 evaluation and
missed by each entry of MUTATIONS, a plausible kernel or table bug restated as one changed line.

Float64 reference per clip, from oracle/mel.py's definitions: x = pcm / 32768 padded by 160 zeros,
frame f = the reflect-centred 400 samples at hop 160 times the periodic Hann window (xw_f),
|X_f[k]| = |rfft(xw_f)|, S_f = sum_n |xw_f[n]|, the slaney bank F, E[f, m] = sum_k F[m, k] |X_f[k]|^2.
Everything here is time-major [frame][mel], as the kernel stores it.

Bound per element, in the energy domain.  With eps = 2^-24, d_f = S_f eps, Ec = max(E, 1e-10):
    B[f, m] = sum_k F[m, k] (2 |X_f[k]| d_f + d_f^2)     the DFT's error through the squaring
            + eps E[f, m]                                  the filter sum
            + 2 eps ln(10) |log10 Ec[f, m]| Ec[f, m]       log10f
and the kernel's raw log10 value v must satisfy |10^v - Ec| <= G B, for EVERY (frame, mel) element
of every case; a clamped element is 1e-10 on both sides.  Nothing is taken from the kernel's output:
G = 4 x G_MEASURED, the project's usual margin over a restatement, and G_MEASURED is the worst
|10^restated - Ec| / B of restate_logmel over the GPU tests' own cases (clips() x N_MELS), printed by
    python -m pytest tests/test_mel_ref_cpu.py -s -k measured

restate_logmel follows the kernel's arithmetic in float32: samples fetched through reflect_index
(the kernel's edge path; the interior path reads the same samples), the 16 x 25 factorisation
n = 25 n1 + n2, k = k1 + 16 k2, stage 1's fmaf chains over n1 with the float values of the W16 table
and the conjugate symmetry for k1 > 8, the tw400 twiddle, stage 2's plain multiply-adds over n2 with
the W25 values, re^2 + im^2, the fmaf filter sum over the sparse bank, float32 log10 of
max(s, 1e-10f).  (An fmaf is evaluated in float64 and rounded once more to float32: the product of
two float32 is exact there, and the double rounding moves a result by one ulp about once in 2^29.)
The compiler may contract stage 2's multiply-adds into FMAs; that is within G's factor of 4.

normalize() and window_x1() restate the two element-wise kernels bit for bit: float32
(max(x, gmax - 8) + 4) * 0.25, mel-major for osw_get_mel; the same value rounded to fp16 (to nearest
even, numpy's astype) in the [3002][C1] layout of X1, zero rows 0 and 3001, zero past the segment
and past n_mels.

Measured on an MI355X (every figure is printed by its test in tests/test_gpu_mel.py): worst
|err| / (G B) 0.330 at 80 mels and 0.290 at 128, both on the impulse train (|err| / B 1.57 and 1.38,
where the restatement has 1.18); maxima, osw_get_mel and every fp16 value of X1 bit-identical.  The
wrong restatements miss G B by >= 1000x on nearly every clip they can show on (the smallest: the
symmetric Hann window on the 1- and 2-sample clips, 7x).
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from oracle import mel as omel

F32, F64 = np.float32, np.float64
NFFT, HOP, NBIN, PAD = 400, 160, 201, 160
EPS = 2.0 ** -24
FLOOR = 1e-10
N_MELS = (80, 128)
X1_ROWS = 3002

MUTATIONS = ("reflect-off-by-one", "hann-symmetric", "fcnt-short")


def n_frames(n_samples):
    return (n_samples + PAD) // HOP


def c1_of(n_mels):
    return (n_mels + 63) // 64 * 64


def reflect_index(j, L):
    """mel.hip reflect_idx: position j of the reflect-extended signal of length L (period 2 (L - 1))."""
    j = np.asarray(j, np.int64)
    if L <= 1:
        return np.zeros_like(j)
    P = 2 * (L - 1)
    j = j % P                       # (C's % and `if (j < 0) j += P`: the same non-negative residue)
    return np.where(j < L, j, P - j)


# --------------------------------------------------------------------------- inputs
SIGNAL_SAMPLES = 2 * omel.SAMPLE_RATE
LENGTHS = (0, 1, 2, 39, 40, 41, 159, 160, 161, 199, 200, 201, 399, 400, 401, 2399, 2400, 2401, 2559, 2560, 2561,
           5159, 5160, 5161, 7719, 7720, 7721)


def _i16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def noise(n, amp, seed):
    """White noise, uniform in [-amp, amp] of full scale."""
    return _i16(np.random.default_rng([seed, n]).uniform(-amp, amp, n) * 32768.0)


def signal_clips():
    n = SIGNAL_SAMPLES
    t = np.arange(n) / omel.SAMPLE_RATE
    rng = np.random.default_rng(2024)
    imp = np.zeros(n)
    imp[::1777] = 32767
    return [
        ("noise-0.3", noise(n, 0.3, 1)),
        ("tone-440+floor-1e-4", _i16(32767 * np.sin(2 * np.pi * 440 * t) + rng.uniform(-1e-4, 1e-4, n) * 32768)),
        ("noise-decay", _i16(rng.uniform(-0.5, 0.5, n) * 32768 * np.exp(-6 * t))),
        ("square-50", _i16(32767 * np.where(np.sin(2 * np.pi * 50 * (t + 1e-6)) >= 0, 1.0, -1.0))),
        ("const-20000", np.full(n, 20000, np.int16)),
        ("const--32768", np.full(n, -32768, np.int16)),
        ("impulses-1777", _i16(imp)),
        ("ternary", rng.integers(-1, 2, n).astype(np.int16)),
        ("silence", np.zeros(n, np.int16)),
    ]


def length_clips():
    return [(f"len-{n}", noise(n, 0.5, 7)) for n in LENGTHS]


@lru_cache(maxsize=None)
def clips():
    """Every clip of the raw log-mel tests, (name, int16 pcm): the signal kinds, then the lengths."""
    out = signal_clips() + length_clips()
    for _, p in out:
        p.setflags(write=False)
    return tuple(out)


def calls(n_per_call=12):
    """clips() as a few ragged log_mel calls (index lists); the empty clip sits inside the first."""
    idx = list(range(len(clips())))
    out = [idx[i:i + n_per_call] for i in range(0, len(idx), n_per_call)]
    empty = [i for i, (_, p) in enumerate(clips()) if len(p) == 0]
    assert len(empty) == 1 and any(empty[0] in c[1:-1] for c in out)
    return out


# --------------------------------------------------------------------------- float64 reference
def frames_f64(pcm):
    """xw_f [n_frames][400]: padded by 160, reflect-centred, periodic Hann (oracle.mel.power_spectrum's
    frames without the one it drops)."""
    x = np.asarray(pcm, np.int16).astype(F64) / 32768.0
    xp = np.pad(np.pad(x, (0, PAD)), (NFFT // 2, NFFT // 2), mode="reflect")
    nf = n_frames(len(x))
    idx = np.arange(NFFT)[None, :] + HOP * np.arange(nf)[:, None]
    return xp[idx] * omel.hann_periodic()[None, :]


@dataclass
class Ref:
    E: np.ndarray      # [n_frames][n_mels] float64 mel energy
    Ec: np.ndarray     # max(E, 1e-10)
    B: np.ndarray      # the element bound (before G)


def reference(pcm, n_mels):
    xw = frames_f64(pcm)
    absX = np.abs(np.fft.rfft(xw, axis=1))                       # [nf][201]
    F = omel.mel_filters(n_mels)                                 # [n_mels][201]
    E = (absX ** 2) @ F.T
    Ec = np.maximum(E, FLOOR)
    d = (np.abs(xw).sum(1) * EPS)[:, None]
    B = (2 * absX * d + d * d) @ F.T + EPS * E + 2 * EPS * np.log(10.0) * np.abs(np.log10(Ec)) * Ec
    return Ref(E, Ec, B)


@lru_cache(maxsize=None)
def references(n_mels):
    """reference() of every clip of clips(), computed once and shared by the tests."""
    return tuple(reference(p, n_mels) for _, p in clips())


def ratio(raw, ref, G):
    """|10^raw - Ec| / (G B) per element (inf where raw is not finite)."""
    raw = np.asarray(raw)
    assert raw.dtype == F32 and raw.shape == ref.Ec.shape, (raw.dtype, raw.shape, ref.Ec.shape)
    r = np.abs(np.power(10.0, raw.astype(F64)) - ref.Ec) / (G * ref.B)
    r[~np.isfinite(raw)] = np.inf
    return r


# --------------------------------------------------------------------------- float32 restatement
def _fma(a, b, c):
    return (np.asarray(a, F64) * np.asarray(b, F64) + np.asarray(c, F64)).astype(F32)


@lru_cache(maxsize=None)
def tables(mut=None):
    """setup_mel's twiddle and window tables as float32: tw400 (re, im), the periodic Hann window."""
    a = 2.0 * np.pi * np.arange(NFFT) / 400.0
    hann = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(NFFT) / 399.0 if mut == "hann-symmetric" else a)
    return np.cos(a).astype(F32), (-np.sin(a)).astype(F32), hann.astype(F32)


@lru_cache(maxsize=None)
def sparse_bank(n_mels, mut=None):
    """setup_mel's flo / fcnt / foff / fw: per mel the contiguous run of bins with a positive weight."""
    F = omel.mel_filters(n_mels)
    lo, cnt, off, fw = [], [], [], []
    for m in range(n_mels):
        nz = np.flatnonzero(F[m] > 0)
        first, last = (int(nz[0]), int(nz[-1])) if nz.size else (0, 0)
        lo.append(first)
        cnt.append(last - first + 1 - (1 if mut == "fcnt-short" else 0))
        off.append(len(fw))
        fw.extend(F[m, first:last + 1].astype(F32))
    return np.array(lo), np.array(cnt), np.array(off), np.array(fw, F32)


def restate_logmel(pcm, n_mels, mut=None):
    """mel_logmel_kernel in float32 -> raw log10 mel [n_frames][n_mels] float32.  mut: one of MUTATIONS."""
    pcm = np.asarray(pcm, np.int16)
    N, nf = len(pcm), n_frames(len(pcm))
    twr, twi, hann = tables(mut)
    w16r, w16i = twr[25 * np.arange(16)], twi[25 * np.arange(16)]    # w16^j = w400^(25 j)
    w25r, w25i = twr[16 * np.arange(25)], twi[16 * np.arange(25)]    # w25^j = w400^(16 j)
    # samples: frame f, n at j = 160 f - 200 + n of the padded signal (length N + 160), reflected
    j = HOP * np.arange(nf)[:, None] - NFFT // 2 + np.arange(NFFT)[None, :]
    L = N + PAD
    jj = reflect_index(j, L)
    if mut == "reflect-off-by-one" and L > 1:
        P = 2 * (L - 1)
        jm = j % P
        jj = np.where(jm < L, jm, P - jm - 1)
    x = np.concatenate([pcm.astype(F32) * F32(1.0 / 32768.0), np.zeros(1, F32)])
    xs = x[np.where(jj < N, jj, N)]
    v = (xs * hann[None, :]).astype(F32).reshape(nf, 16, 25)         # [f][n1][n2]
    # stage 1: Y[k1] = sum_n1 v[n1] w16^(n1 k1) by fmaf chains (k1 <= 8), conjugates above, times w400^(n2 k1)
    Yr = np.zeros((nf, 25, 16), F32)
    Yi = np.zeros((nf, 25, 16), F32)
    for k1 in range(9):
        re = np.zeros((nf, 25), F32)
        im = np.zeros((nf, 25), F32)
        for n1 in range(16):
            re = _fma(v[:, n1], w16r[(n1 * k1) & 15], re)
            im = _fma(v[:, n1], w16i[(n1 * k1) & 15], im)
        Yr[:, :, k1], Yi[:, :, k1] = re, im
    for k1 in range(9, 16):
        Yr[:, :, k1], Yi[:, :, k1] = Yr[:, :, 16 - k1], -Yi[:, :, 16 - k1]
    t = np.arange(25)[:, None] * np.arange(16)[None, :]              # n2 k1 <= 360
    wr, wi = twr[t][None], twi[t][None]
    Zr = (Yr * wr).astype(F32) - (Yi * wi).astype(F32)               # [f][n2][k1]
    Zi = (Yr * wi).astype(F32) + (Yi * wr).astype(F32)
    # stage 2: X[k1 + 16 k2] = sum_n2 Z[n2][k1] w25^(n2 k2), plain float32 multiply-adds; power
    Pw = np.zeros((nf, 16 * 13), F32)
    for k2 in range(13):
        re = np.zeros((nf, 16), F32)
        im = np.zeros((nf, 16), F32)
        for n2 in range(25):
            cr, ci = w25r[(n2 * k2) % 25], w25i[(n2 * k2) % 25]
            re = re + ((Zr[:, n2] * cr).astype(F32) - (Zi[:, n2] * ci).astype(F32))
            im = im + ((Zr[:, n2] * ci).astype(F32) + (Zi[:, n2] * cr).astype(F32))
        Pw[:, 16 * k2:16 * k2 + 16] = (re * re).astype(F32) + (im * im).astype(F32)
    Pw = Pw[:, :NBIN]
    # stage 3: fmaf filter sum over the mel's run of bins, log10 of the clamped sum
    lo, cnt, off, fw = sparse_bank(n_mels, mut)
    out = np.empty((nf, n_mels), F32)
    for m in range(n_mels):
        s = np.zeros(nf, F32)
        for i in range(cnt[m]):
            s = _fma(fw[off[m] + i], Pw[:, lo[m] + i], s)
        out[:, m] = np.maximum(np.log10(np.maximum(s, F32(1e-10))), F32(-10.0))
    return out


# --------------------------------------------------------------------------- the element-wise kernels
def _normalized(raw, gmax):
    raw = np.asarray(raw)
    assert raw.dtype == F32
    floor_v = F32(gmax) - F32(8.0)
    return ((np.maximum(raw, floor_v) + F32(4.0)).astype(F32) * F32(0.25)).astype(F32)


def normalize(raw, gmax):
    """mel_normalize_kernel (osw_get_mel): raw [n_frames][n_mels] float32 -> [n_mels][n_frames] float32."""
    return np.ascontiguousarray(_normalized(raw, gmax).T)


def window_x1(raw, gmax, seek, size, n_mels, mut=None):
    """mel_window_kernel for one window -> fp16 bits [3002][C1].  mut "row-shift": t = r."""
    nf = raw.shape[0]
    assert 0 <= seek < nf and size >= 1 and raw.shape[1] == n_mels
    seg = min(min(size, 3000), nf - seek)
    out = np.zeros((X1_ROWS, c1_of(n_mels)), np.float16)
    r0 = 0 if mut == "row-shift" else 1
    out[r0:r0 + seg, :n_mels] = _normalized(raw[seek:seek + seg], gmax).astype(np.float16)
    return out.view(np.uint16)


# --------------------------------------------------------------------------- window-packing cases
WINDOW_CLIP_SAMPLES = (65 * omel.SAMPLE_RATE, omel.SAMPLE_RATE, 0)      # A (6501 frames), B (101), C (1)
A, B_, C_ = 0, 1, 2
WINDOW_CALLS_FIRST = [[(A, 0, 3000), (A, 3000, 3000), (A, 5000, 3000), (A, 6500, 3000)],
                      [(A, 1234, 500), (A, 0, 4000), (B_, 0, 3000), (B_, 100, 3000)]]
WINDOW_CALL_SECOND = [(C_, 0, 3000), (B_, 50, 7)]      # into the slots the first calls filled


def window_clips():
    return [noise(n, 0.5, 11 + i) for i, n in enumerate(WINDOW_CLIP_SAMPLES)]


# --------------------------------------------------------------------------- measured
def measure(n_mels_list=N_MELS):
    """-> (worst |10^restated - Ec| / B over clips() x n_mels, the case that set it)."""
    worst, where = 0.0, None
    for n_mels in n_mels_list:
        for name, pcm in clips():
            r = float(ratio(restate_logmel(pcm, n_mels), reference(pcm, n_mels), 1.0).max())
            if r > worst:
                worst, where = r, f"{name}, {n_mels} mels"
    return worst, where


G_MEASURED = 1.19
G_MEASURED_CASE = "impulses-1777, 128 mels"
G = 4 * G_MEASURED
