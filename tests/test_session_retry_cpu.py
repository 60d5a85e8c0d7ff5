"""What a retry session adds on the host (csrc/slots.h SlotTable::retry, csrc/plan.h DecodePlan with
retries): tests/cpp/session_retry_check.cpp, a stand-alone program with its own main, built with
AddressSanitizer + UBSan on the host side and run as a child process.  It checks the held ->
decoding transition and every refusal (a free, a decoding or an unknown tag, a duplicate) with the
table left untouched, ``stalled()`` with retried slots, a random walk against a model, the session
plan's ``group = max(beam, best_of)`` for (1,1), (1,3), (1,5), (5,3), (5,5), (2,5), and that the
decode-graph key of a retry session differs from the retry-free one, which is unchanged (see the
program's header).  No HIP call is made and nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not found")
def test_session_retry_check(tmp_path):
    exe = str(tmp_path / "session_retry_check")
    build = subprocess.run(
        [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
         "-Xarch_host", "-fno-sanitize-recover=undefined",
         "-I", os.path.join(ROOT, "open-speech_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
         os.path.join(ROOT, "tests", "cpp", "session_retry_check.cpp"), "-o", exe],
        capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert run.stdout.startswith("session retry ok:"), run.stdout
