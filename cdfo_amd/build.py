"""Build libcdfo_hip.so (all HIP kernels + the C-ABI) in-tree for gfx950.

    python -m cdfo_amd.build [--force] [--dev]

hipcc cross-compiles without a GPU.  The .so lands in cdfo_amd/lib/ (git-ignored).  --dev builds the same sources with
-DCDFO_DEV_ABLATIONS (the kernels' developer ablations and timeline probes, wrong results by construction) into
cdfo_amd/lib/dev/libcdfo_hip.so; nothing loads that library unless CDFO_LIB_PATH names it.
"""
from __future__ import annotations

import concurrent.futures as cf
import glob
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libcdfo_hip.so")
DEV_LIB = os.path.join(LIBDIR, "dev", "libcdfo_hip.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "--offload-arch=gfx950", "-fPIC", "-std=c++17", "-ffp-contract=fast", "-Wall", "-Wno-unused-function"]


def _sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")))


def _deps_mtime():
    hdrs = glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(HERE, "..", "include", "*.h"))
    return max(os.path.getmtime(p) for p in hdrs)


def _compile(src: str, objdir: str, flags: list, force: bool) -> str:
    obj = os.path.join(objdir, os.path.basename(src)[:-4] + ".o")
    if (not force and os.path.exists(obj) and os.path.getmtime(obj) >= max(os.path.getmtime(src), _deps_mtime())):
        return obj
    cmd = [HIPCC, *flags, "-c", src, "-o", obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stdout}\n{r.stderr}")
    if r.stderr.strip():
        sys.stderr.write(r.stderr)
    return obj


def build(force: bool = False, jobs: int = 6, dev: bool = False) -> str:
    lib = DEV_LIB if dev else LIB
    objdir = os.path.join(os.path.dirname(lib), "obj")
    flags = FLAGS + ["-DCDFO_DEV_ABLATIONS"] if dev else FLAGS
    os.makedirs(objdir, exist_ok=True)
    srcs = _sources()
    with cf.ThreadPoolExecutor(max_workers=jobs) as ex:
        objs = list(ex.map(lambda s: _compile(s, objdir, flags, force), srcs))
    if force or not os.path.exists(lib) or any(os.path.getmtime(o) > os.path.getmtime(lib) for o in objs):
        cmd = [HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objs]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}\n{r.stderr}")
    return lib


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, dev="--dev" in sys.argv))
