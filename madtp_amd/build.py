"""Builds the C-ABI shared library (hand-written gfx950 kernels) in-tree with hipcc.

    python -m madtp_amd.build [--force]

hipcc cross-compiles for gfx950 without a GPU.  The .so is git-ignored but travels with the repo snapshot to
the GPU box, where it is loaded by madtp_amd.hip (ctypes)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIBDIR = os.path.join(HERE, "lib")
LIB = os.path.join(LIBDIR, "libmadtp_hip.so")
SOURCES = ["gemm.hip", "gemm_pp.hip", "attention.hip", "norm.hip", "prune.hip", "layers.hip", "lmhead.hip", "backward.hip", "retrieval.hip", "clip.hip", "eval.hip", "optim.hip", "image.hip", "augment.hip", "jpeg.hip", "search.hip", "jpeg_huff.hip", "search_coarse.hip", "lists.hip", "png.hip", "tokenmap.hip", "text.hip"]
INCLUDE = os.path.join("..", "..", "include")
# what is on disk, as paths from csrc/: a header nobody listed cannot leave a stale library
HEADERS = sorted(f for f in os.listdir(CSRC) if f.endswith(".h")) + \
    sorted(os.path.join(INCLUDE, f) for f in os.listdir(os.path.join(CSRC, INCLUDE)) if f.endswith(".h"))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", "hipcc"):
        if c and (os.path.isabs(c) and os.path.exists(c) or not os.path.isabs(c)):
            return c
    return "hipcc"


def needs_build():
    if not os.path.exists(LIB):
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, s) for s in SOURCES + HEADERS] + [os.path.abspath(__file__)]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=True):
    if not force and not needs_build():
        return LIB
    os.makedirs(LIBDIR, exist_ok=True)
    objs = []
    procs = []
    for s in SOURCES:
        o = os.path.join(LIBDIR, s.replace(".hip", ".o"))
        objs.append(o)
        cmd = [_hipcc()] + FLAGS + ["-c", os.path.join(CSRC, s), "-o", o]
        if verbose:
            print(" ".join(cmd), flush=True)
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise RuntimeError("hipcc failed: " + " ".join(cmd))
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
