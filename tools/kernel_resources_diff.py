#!/usr/bin/env python3
"""Per-kernel VGPR / spill / occupancy / LDS of a HIP source against another version of it
(hipcc -Rpass-analysis=kernel-resource-usage; the parser is tests/kernel_resources.py); prints only
the kernels that differ.
usage: kernel_resources_diff.py OLD.hip NEW.hip  (paths relative to open-speech_amd/csrc)"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from kernel_resources import kernel_resources  # noqa: E402

a = kernel_resources(sys.argv[1])
b = kernel_resources(sys.argv[2])
for k in sorted(set(a) | set(b)):
    if a.get(k) != b.get(k):
        print(k[:90], a.get(k), '->', b.get(k))
