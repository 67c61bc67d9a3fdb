"""The shipped kernels carry no developer switches: an A/B experiment lives in its own working copy (tools/dev/ab_build.sh), not as
an #ifdef in premvos_amd/csrc.  The only conditionals left keep gfx950 builtins out of hipcc's host pass."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_only_device_compile_guards_in_kernel_sources():
    found = []
    for path in sorted(glob.glob(os.path.join(ROOT, "premvos_amd", "csrc", "*.hip"))):
        with open(path) as f:
            for line in f:
                if re.match(r"\s*#\s*if", line):
                    found.append((os.path.basename(path), line.split("//")[0].strip()))
    assert found == [("conv_bf16x3_s8.hip", "#if defined(__HIP_DEVICE_COMPILE__)"),
                     ("conv_pwdma_f32.hip", "#if defined(__HIP_DEVICE_COMPILE__)")], found
