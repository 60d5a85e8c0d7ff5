"""What tests/mel_ref.py's bound catches, shown on the CPU: on every clip the GPU tests run, the
faithful float32 restatement of mel_logmel_kernel stays within G·B of the float64 reference (so
the reference alone satisfies the condition), each wrong restatement (mel_ref.MUTATIONS) misses it,
reflect_index equals numpy's reflect padding, the float64 pieces reproduce oracle.mel.log_mel_raw,
and the element-wise restatements equal loops written from the kernels' per-element definitions."""
import os
import re

import numpy as np
import pytest

import mel_ref as M
from oracle import mel as omel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = np.float32, np.float64


@pytest.mark.parametrize("N", M.LENGTHS)
def test_reflect_index_equals_numpy_pad(N):
    """Positions instead of samples: the padded signal is arange(N + 160), so every index is told apart
    (below 41 samples the 200-sample reflection wraps more than once)."""
    L = N + M.PAD
    want = np.pad(np.pad(np.arange(N), (0, M.PAD), mode="constant", constant_values=-1), 200, mode="reflect")
    pos = np.pad(np.arange(L), 200, mode="reflect")
    got = M.reflect_index(np.arange(-200, L + 200), L)
    assert np.array_equal(got, pos)
    assert np.array_equal(np.where(got < N, got, -1), want)


def test_reflect_index_degenerate():
    assert np.array_equal(M.reflect_index(np.arange(-5, 5), 1), np.zeros(10, np.int64))
    assert np.array_equal(M.reflect_index(np.arange(-3, 5), 2), [1, 0, 1, 0, 1, 0, 1, 0])


@pytest.mark.parametrize("n_mels", M.N_MELS)
def test_restatement_within_bound(n_mels):
    worst, where = 0.0, None
    for name, pcm in M.clips():
        ref = M.reference(pcm, n_mels)
        raw = M.restate_logmel(pcm, n_mels)
        assert raw.shape == (M.n_frames(len(pcm)), n_mels)
        r = float(M.ratio(raw, ref, M.G).max())
        if r > worst:
            worst, where = r, name
    print(f"{n_mels} mels: restatement worst |err| / (G B) = {worst:.3f} ({where})")
    assert worst <= 1


def test_measured_constant():
    worst, where = M.measure()
    print(f"G_MEASURED = {worst:.4f}  ({where})")
    assert worst <= M.G_MEASURED <= 1.05 * worst and where == M.G_MEASURED_CASE
    assert M.G == 4 * M.G_MEASURED


@pytest.mark.parametrize("n_mels", M.N_MELS)
def test_float64_pieces_reproduce_oracle(n_mels):
    for name, pcm in M.clips():
        ref = M.reference(pcm, n_mels)
        want = omel.log_mel_raw(omel.pcm16_to_float(pcm), n_mels).T
        assert want.shape == (omel.n_frames_for(len(pcm)), n_mels) == ref.E.shape, name
        np.testing.assert_allclose(np.log10(ref.Ec), want, rtol=0, atol=1e-12, err_msg=name)
        assert (ref.B > 0).all() and np.isfinite(ref.B).all(), name


def test_tables_equal_the_kernel_constants():
    """The W16 / W25 constants of mel.hip are the float values of tw400 at 25 j and 16 j, as the
    restatement takes them."""
    src = open(os.path.join(ROOT, "open-speech_amd", "csrc", "mel.hip")).read()
    consts = {m.group(1): np.array([float(v.strip().rstrip("f")) for v in m.group(2).split(",")], F32)
              for m in re.finditer(r"constexpr float (W\d+[RI])\[\d+\] = \{([^}]*)\}", src)}
    assert sorted(consts) == ["W16I", "W16R", "W25I", "W25R"]
    twr, twi, hann = M.tables()
    assert np.array_equal(consts["W16R"].view(np.uint32), twr[25 * np.arange(16)].view(np.uint32))
    assert np.array_equal(consts["W16I"].view(np.uint32), twi[25 * np.arange(16)].view(np.uint32))
    assert np.array_equal(consts["W25R"].view(np.uint32), twr[16 * np.arange(25)].view(np.uint32))
    assert np.array_equal(consts["W25I"].view(np.uint32), twi[16 * np.arange(25)].view(np.uint32))
    assert hann[0] == 0 and hann[200] == 1 and np.array_equal(hann[1:], hann[1:][::-1])


@pytest.mark.parametrize("n_mels", M.N_MELS)
def test_sparse_bank_is_the_bank(n_mels):
    lo, cnt, off, fw = M.sparse_bank(n_mels)
    F = omel.mel_filters(n_mels)
    dense = np.zeros_like(F)
    for m in range(n_mels):
        assert cnt[m] >= 1 and lo[m] + cnt[m] <= M.NBIN
        dense[m, lo[m]:lo[m] + cnt[m]] = fw[off[m]:off[m] + cnt[m]]
    assert np.array_equal(dense, F.astype(F32).astype(F64))
    assert off[-1] + cnt[-1] == fw.size


@pytest.mark.parametrize("mut", M.MUTATIONS)
def test_mutants_miss(mut):
    """Each wrong restatement misses G·B on the clips it can show on: the reflection on every clip's
    first frame (every short length included), the window and the filter run on every clip but the
    silent ones (where all three give 1e-10)."""
    quiet = {"silence", "len-0"}
    for n_mels in M.N_MELS:
        line = []
        for name, pcm in M.clips():
            r = float(M.ratio(M.restate_logmel(pcm, n_mels, mut), M.reference(pcm, n_mels), M.G).max())
            line.append(f"{name} {r:.3g}")
            if name in quiet:
                assert r <= 1, (mut, name)
            elif not (name.startswith("const") and mut == "reflect-off-by-one"):   # (a constant reflects onto itself)
                assert r > 1, (mut, name, n_mels, r)
        print(f"{mut}, {n_mels} mels: worst |err| / (G B) per clip: " + ", ".join(line))


def test_elementwise_restatements_against_loops():
    """normalize() and window_x1() against loops over the kernels' own per-element definitions."""
    rng = np.random.default_rng(5)
    n_mels, nf = 80, 57
    raw = rng.uniform(-10, 2, (nf, n_mels)).astype(F32)
    raw[3, 7] = F32(2.5)
    gmax = raw.max()
    floor_v = F32(gmax - F32(8))
    got = M.normalize(raw, gmax)
    assert got.dtype == F32 and got.shape == (n_mels, nf)
    for m in range(0, n_mels, 7):
        for t in range(nf):
            assert got[m, t] == F32(F32(max(raw[t, m], floor_v) + F32(4)) * F32(0.25))
    assert (raw < floor_v).any() and got.min() == F32(F32(floor_v + F32(4)) * F32(0.25))
    C1 = M.c1_of(n_mels)
    assert (C1, M.c1_of(128), M.c1_of(64), M.c1_of(65)) == (128, 128, 64, 128)
    for seek, size in ((0, 3000), (50, 7), (56, 3000), (10, 4000)):
        x1 = M.window_x1(raw, gmax, seek, size, n_mels)
        assert x1.shape == (3002, C1) and x1.dtype == np.uint16
        seg = min(size, nf - seek)
        want = np.zeros((3002, C1), np.float16)
        for r in range(1, 1 + seg):
            for c in range(n_mels):
                want[r, c] = np.float16(F32(F32(max(raw[seek + r - 1, c], floor_v) + F32(4)) * F32(0.25)))
        assert np.array_equal(x1, want.view(np.uint16)), (seek, size)
        assert not np.array_equal(M.window_x1(raw, gmax, seek, size, n_mels, "row-shift"), x1)


def test_case_lists():
    """The edges the GPU tests are there for, computed from the kernel's constants: lengths on both
    sides of the double-wrap threshold (41), of a frame being added (multiples of 160), of block 1's
    and block 2's switch from the edge path to the interior path (N = 2560 b + 2600), and partly
    filled last blocks."""
    L = M.LENGTHS
    assert {39, 40, 41} <= set(L) and {0, 1, 2} <= set(L)
    for n in (160, 200, 400, 2400, 2560, 5160, 7720):
        assert {n - 1, n, n + 1} <= set(L)
    # block b >= 1 takes the interior path from N = 2560 b + 2600 on: 5160 and 7720
    for b in (1, 2):
        n = 2560 * b + 2600
        j0 = 2560 * b - 200
        assert j0 + 2800 == n and {n - 1, n, n + 1} <= set(L)
    assert any(M.n_frames(n) % 16 for n in L) and any(M.n_frames(n) > 16 for n in L)
    assert [M.n_frames(n) for n in M.WINDOW_CLIP_SAMPLES] == [6501, 101, 1]
    names = [n for n, _ in M.clips()]
    assert len(names) == len(set(names)) == 9 + len(L)
    assert sum(len(c) for c in M.calls()) == len(names) and len(M.calls()) >= 2
    for batch in M.WINDOW_CALLS_FIRST + [M.WINDOW_CALL_SECOND]:
        assert 1 <= len(batch) <= 4
