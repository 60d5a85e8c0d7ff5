"""The decode plan (csrc/plan.h) on the host: tests/cpp/decode_plan_check.cpp, a stand-alone
program with its own main, built with AddressSanitizer + UBSan on the host side and run as a
child process.  It walks the option grid over the three decode modes and checks the SelParams
table per mode, the graph key's sensitivity and separation, the mask and the prompt-length check
(see the program's header).  No HIP call is made and nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not found")
def test_decode_plan_check(tmp_path):
    exe = str(tmp_path / "decode_plan_check")
    build = subprocess.run(
        [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
         "-Xarch_host", "-fno-sanitize-recover=undefined",
         "-I", os.path.join(ROOT, "open-speech_amd", "csrc"),
         os.path.join(ROOT, "tests", "cpp", "decode_plan_check.cpp"), "-o", exe],
        capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert run.stdout.startswith("decode plan ok:"), run.stdout
