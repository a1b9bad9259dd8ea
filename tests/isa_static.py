"""What the *_static tests share (no GPU): one kernel file compiled to gfx950 assembly with the flags of the build, and two readers of that
assembly -- the resource counts of a kernel's metadata and the opcodes of its body."""
import functools
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
RESOURCE_KEYS = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


@functools.lru_cache(maxsize=None)
def compile_asm(name):
    """the device assembly of csrc/<name>; compiled once per process"""
    r = subprocess.run([HIPCC, "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-S", "--cuda-device-only",
                        os.path.join(ROOT, "mkhe-kklss_amd", "csrc", name), "-o", "-"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-1500:]
    return r.stdout


def resources(asm, kernel):
    meta = [b for b in asm.split("- .agpr_count:")[1:] if kernel in b]
    assert len(meta) == 1, kernel
    return {k: int(re.search(r"\.%s:\s+(\d+)" % k, meta[0]).group(1)) for k in RESOURCE_KEYS}


def ops(asm, kernel):
    name = re.findall(r"^(\S*%s\S*):" % kernel, asm, re.M)
    assert len(name) == 1, name
    body = asm.split(name[0] + ":", 1)[1].split("s_endpgm", 1)[0]
    code = [l.strip() for l in body.splitlines() if l.strip() and not l.strip().startswith((";", ".", "//")) and not l.strip().endswith(":")]
    return [l.split()[0] for l in code]
