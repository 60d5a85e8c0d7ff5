"""A decode session's window slots (csrc/slots.h) on the host: tests/cpp/session_slots_check.cpp, a
stand-alone program with its own main, built with AddressSanitizer + UBSan on the host side and
run as a child process.  It checks every transition of a slot (free, decoding, held) and every
refusal (align or release of a free or decoding slot, duplicate tags, hold after the first add)
with the table left untouched, that admission never picks a held slot, and that the
all-held-and-queued case is a step without work (see the program's header).  No HIP call is made
and nothing is loaded into this process."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.mark.skipif(HIPCC is None, reason="hipcc not found")
def test_session_slots_check(tmp_path):
    exe = str(tmp_path / "session_slots_check")
    build = subprocess.run(
        [HIPCC, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
         "-Xarch_host", "-fno-sanitize-recover=undefined",
         "-I", os.path.join(ROOT, "open-speech_amd", "csrc"),
         os.path.join(ROOT, "tests", "cpp", "session_slots_check.cpp"), "-o", exe],
        capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert run.stdout.startswith("session slots ok:"), run.stdout


def test_session_source_uses_the_slot_table():
    """session.hip keeps no slot bookkeeping of its own beside the table."""
    src = open(os.path.join(ROOT, "open-speech_amd", "csrc", "session.hip")).read()
    assert '#include "slots.h"' in src and "SlotTable slots" in src
    assert "slot_tag" not in src
    hdr = open(os.path.join(ROOT, "open-speech_amd", "csrc", "slots.h")).read()
    assert re.search(r"\bhip[A-Z_]|hip_runtime|ctx\.h|\bosw_ctx\s*\*", hdr) is None   # host only, no context
