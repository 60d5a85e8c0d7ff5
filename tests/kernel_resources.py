"""Per-kernel register, spill, occupancy and LDS numbers of a HIP source, from the compiler's own
resource remarks (hipcc -Rpass-analysis=kernel-resource-usage on a device-only gfx950 compile with
the Makefile's flags).  Shared by tools/kernel_resources_diff.py and tests/test_kernel_resources_cpu.py.
Numbers only: no instruction is looked at."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "open-speech_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
# open-speech_amd/csrc/Makefile's CXXFLAGS (without -Wall), device side only
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics",
         "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops", "--offload-device-only"]
FIELDS = {"VGPRs": "vgprs", "AGPRs": "agprs", "VGPRs Spill": "vgpr_spill", "SGPRs Spill": "sgpr_spill",
          "Occupancy [waves/SIMD]": "occupancy", "LDS Size [bytes/block]": "lds",
          "ScratchSize [bytes/lane]": "scratch"}
VGPR_GRANULE = 8   # registers are allocated to a wave in units of 8 (of 512 per SIMD lane)


def parse_remarks(text):
    """The remark stream -> {mangled kernel name: {field: int}} (fields: FIELDS' values)."""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = out.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][A-Za-z \[\]/]*?): (\d+)", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[FIELDS[m.group(1)]] = int(m.group(2))
    return out


def demangle(names):
    names = list(names)
    if not names:
        return {}
    filt = os.path.join(os.path.dirname(HIPCC), "..", "llvm", "bin", "llvm-cxxfilt")
    if not os.path.exists(filt):
        filt = "c++filt"
    res = subprocess.run([filt], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    return dict(zip(names, res.stdout.splitlines()))


def kernel_resources(src, cwd=CSRC, demangled=False):
    """Compile `src` (a path relative to cwd) and return its kernels' numbers, keyed by the mangled
    name, or by the demangled signature (demangled=True)."""
    with tempfile.TemporaryDirectory() as tmp:
        res = subprocess.run([HIPCC] + FLAGS + ["-c", src, "-o", os.path.join(tmp, "x.o"),
                                                "-Rpass-analysis=kernel-resource-usage"],
                             capture_output=True, text=True, cwd=cwd)
    if res.returncode != 0:
        raise RuntimeError(f"{src} did not compile:\n{res.stderr[-4000:]}")
    d = parse_remarks(res.stderr)
    if demangled:
        names = demangle(d)
        d = {names[k]: v for k, v in d.items()}
    return d


def allocated_vgprs(n):
    return -(-n // VGPR_GRANULE) * VGPR_GRANULE
