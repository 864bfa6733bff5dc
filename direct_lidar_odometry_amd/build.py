"""Build the HIP extension in-tree:  python -m direct_lidar_odometry_amd.build

Produces direct_lidar_odometry_amd/libngicp_hip.so for gfx950 (hipcc cross-compiles without a GPU).
-ffp-contract=off: FP32 squared distances must not be fused (the reference builds without -march,
/root/reference/CMakeLists.txt:14-15, so its distances are un-fused mul/add).
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libngicp_hip.so")
SOURCES = ["ngicp_api.hip", "ngicp_filters.hip"]
PUBLIC_HEADER = os.path.normpath(os.path.join(HERE, "..", "include", "ngicp.h"))
DEP_SUFFIXES = (".h", ".inc", ".hip")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-Wall", "-Wno-unused-function"]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


def dependencies() -> list[str]:
    """Every file the library is compiled from: what is on disk under csrc/ (a header nobody listed cannot leave a stale library
    behind), the public header, and this file for its flags."""
    found = [os.path.join(d, f) for d, _, files in os.walk(CSRC) for f in files if f.endswith(DEP_SUFFIXES)]
    return sorted(found) + [PUBLIC_HEADER, os.path.abspath(__file__)]


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    return any(os.path.getmtime(d) > t for d in dependencies())


def build(force: bool = False, verbose: bool = False, extra_flags: list[str] | None = None) -> str:
    if not force and not needs_build():
        return LIB
    tmp = f"{LIB}.{os.getpid()}.tmp"  # unique per process: several ranks may find the library stale at the same time
    cmd = [hipcc(), *FLAGS, *(extra_flags or []), *[os.path.join(CSRC, s) for s in SOURCES], "-o", tmp]
    if verbose:
        print(" ".join(cmd), flush=True)
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        sys.stderr.write(res.stdout + res.stderr)
        raise RuntimeError("hipcc failed")
    if verbose and res.stderr:
        sys.stderr.write(res.stderr)
    os.replace(tmp, LIB)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
