"""The log-mel front end (csrc/mel.hip) kernel by kernel through osw_debug_get_logmel and
osw_debug_mel_windows, against tests/mel_ref.py: mel_logmel_kernel's raw log10 mel within G·B of the
float64 reference on every element (signal kinds, and lengths on both sides of every path switch);
the per-clip maximum and the two element-wise kernels bit for bit; the window packing's every fp16
value; refused windows; device-resident PCM with a non-zero first offset."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":      # the device-PCM child process: what tests/conftest.py does under pytest
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import osw_path
    osw_path.load()

import mel_ref as M
from open_speech_amd import _lib
from open_speech_amd import dims as D
from open_speech_amd.engine import WhisperEngine

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module", params=M.N_MELS)
def run(request):
    """One small engine per n_mels and, computed once, what the host-pointer log_mel calls of
    mel_ref.calls() left per clip: (frames, raw log-mel, maximum, osw_get_mel)."""
    n_mels = request.param
    d = D.WhisperDims(n_mels=n_mels, n_audio_state=128, n_audio_head=2, n_audio_layer=1, n_text_state=128,
                      n_text_head=2, n_text_layer=1)
    eng = WhisperEngine(d, device=0, max_batch=4)
    clips = M.clips()
    host = [None] * len(clips)
    for call in M.calls():
        nf = eng.log_mel([clips[i][1] for i in call])
        for k, i in enumerate(call):
            raw, mx = eng.debug_get_logmel(k)
            host[i] = (nf[k], raw, mx, eng.get_mel(k))
    yield n_mels, eng, host
    eng.close()


def test_raw_logmel_within_bound(run):
    n_mels, _, host = run
    worst, where = 0.0, None
    for (name, pcm), ref, (nf, raw, _, _) in zip(M.clips(), M.references(n_mels), host):
        assert nf == (len(pcm) + 160) // 160 and raw.shape == (nf, n_mels), name
        r = M.ratio(raw, ref, M.G)            # every (frame, mel) element; clamped ones are 1e-10 on both sides
        f, m = np.unravel_index(np.argmax(r), r.shape)
        print(f"{n_mels} mels {name}: worst |err| / (G B) = {r[f, m]:.3f} at frame {f} mel {m}")
        if r[f, m] > worst:
            worst, where = float(r[f, m]), name
    print(f"{n_mels} mels: worst |err| / (G B) = {worst:.3f} ({where}); |err| / B = {worst * M.G:.3f}, "
          f"the restatement's {M.G_MEASURED}")
    assert worst <= 1, (worst, where)


def test_clip_maximum_and_get_mel(run):
    """The ordered-int atomicMax gives the maximum of the clip's own raw values bit for bit (negative
    maxima included: -10 exactly for the silent clips), and osw_get_mel is the restated clamp and
    scaling of those raw values."""
    n_mels, _, host = run
    negative = 0
    for (name, pcm), (nf, raw, mx, mel) in zip(M.clips(), host):
        assert bits(np.float32(mx)) == bits(raw.max()), (name, mx, raw.max())
        if not pcm.any():
            assert mx == np.float32(-10.0) and (raw == np.float32(-10.0)).all(), name
        negative += bool(mx < 0)
        want = M.normalize(raw, mx)
        assert mel.shape == want.shape == (n_mels, nf)
        bad = int((bits(mel) != bits(want)).sum())
        assert bad == 0, (name, bad)
    print(f"{n_mels} mels: {len(host)} maxima and osw_get_mel bit-identical; {negative} negative maxima; "
          f"worst |err| / (G B) = 0 (exact)")
    assert negative >= 3


def test_window_packing(run):
    """mel_window_kernel alone: seek > 0, a clip's end inside the window, sizes below and above 3000,
    the border rows, the pad columns, and a second call into slots an earlier, larger call filled."""
    n_mels, eng, _ = run
    assert eng.log_mel(M.window_clips()) == [6501, 101, 1]
    raws = [eng.debug_get_logmel(i) for i in range(3)]
    C1 = M.c1_of(n_mels)
    total = 0
    for batch in M.WINDOW_CALLS_FIRST + [M.WINDOW_CALL_SECOND]:
        x1 = eng.debug_mel_windows(batch).view(np.uint16)
        assert x1.shape == (len(batch), 3002, C1)
        for w, (clip, seek, size) in enumerate(batch):
            raw, mx = raws[clip]
            want = M.window_x1(raw, mx, seek, size, n_mels)
            bad = int((x1[w] != want).sum())
            assert bad == 0, (clip, seek, size, bad)
            assert not x1[w, 0].any() and not x1[w, 3001].any() and not x1[w, :, n_mels:].any()
            total += want.size
    print(f"{n_mels} mels (C1 {C1}): {total} fp16 values bit-identical; worst |err| / (G B) = 0 (exact)")


def test_refused_windows(run):
    _, eng, _ = run
    nf = eng.log_mel(M.window_clips())
    for win, msg in (((1, nf[1], 3000), "window seek out of range"), ((0, 0, 0), "empty window"),
                     ((len(nf), 0, 3000), "window clip out of range")):
        for batch in ([win], [(0, 0, 3000), win]):        # alone, and behind a window that is fine
            with pytest.raises(_lib.OswError, match=msg) as e:
                eng.debug_mel_windows(batch)
            assert e.value.rc == _lib.OSW_EINVAL
    with pytest.raises(_lib.OswError, match="window count out of range"):
        eng.debug_mel_windows([(0, 0, 3000)] * 5)
    print("refused windows: 7 calls returned OSW_EINVAL; worst |err| / (G B): none computed")


def device_pcm_child():
    """Runs in a process of its own, torch first (as in bench.py: torch brings a HIP runtime of its
    own, which finds no GPU once the library's runtime has initialised the device in the same
    process).  The clips as one torch int16 device tensor behind 777 leading samples, so that
    offsets[0] = 777: raw log-mel and maxima must be bit-identical to the host-pointer call."""
    import torch
    torch.cuda.set_device(0)
    clips = M.clips()
    lead = M.noise(777, 0.9, 3)
    for n_mels in M.N_MELS:
        d = D.WhisperDims(n_mels=n_mels, n_audio_state=128, n_audio_head=2, n_audio_layer=1, n_text_state=128,
                          n_text_head=2, n_text_layer=1)
        eng = WhisperEngine(d, device=0, max_batch=4)
        worst = 0.0
        for call in M.calls():
            arrs = [clips[i][1] for i in call]
            nf_host = eng.log_mel(arrs)
            host = [eng.debug_get_logmel(k) for k in range(len(call))]
            offs = 777 + np.concatenate([[0], np.cumsum([len(a) for a in arrs])]).astype(np.int64)
            t = torch.from_numpy(np.concatenate([lead] + arrs)).to("cuda:0")
            torch.cuda.synchronize()
            assert eng.log_mel(None, on_device_ptr=t.data_ptr(), offsets=offs) == nf_host
            for k, i in enumerate(call):
                raw, mx = eng.debug_get_logmel(k)
                assert np.array_equal(bits(raw), bits(host[k][0])), clips[i][0]
                assert bits(np.float32(mx)) == bits(np.float32(host[k][1])), clips[i][0]
                worst = max(worst, float(M.ratio(raw, M.references(n_mels)[i], M.G).max()))
            del t
        eng.close()
        print(f"{n_mels} mels: device PCM at offset 777 bit-identical to the host calls; "
              f"worst |err| / (G B) = {worst:.3f}")
    print("DEVICE PCM OK")


def test_device_pcm_with_offset():
    """Device-resident PCM with offsets[0] != 0, what bench.py and distributed.py pass (src = pcm +
    offsets[0], offsets rebased): see device_pcm_child."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "DEVICE PCM OK" in out.stdout, out.stdout[-2000:] + out.stderr[-4000:]


if __name__ == "__main__":
    device_pcm_child()
