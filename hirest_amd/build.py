"""Build libhirest_hip.so (the C-ABI library declared in include/hirest_hip.h) with hipcc for gfx950.

In-tree, explicit, no JIT cache: ``python -m hirest_amd.build`` (or ``__graft_entry__.build()``)
writes hirest_amd/lib/libhirest_hip.so, which travels to the GPU box with the repo snapshot.
hipcc cross-compiles gfx950 code objects without a GPU present.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_DIR = os.path.join(HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libhirest_hip.so")
SOURCES = ["gemm.hip", "joint_x3.hip", "attention.hip", "attention_long.hip","elementwise.hip", "score.hip", "tower.hip", "tower_f32.hip", "tower_x3.hip", "attention_x3.hip", "profile.hip", "joint.hip", "train.hip", "train_block.hip", "optim.hip", "optim_capturable.hip", "caption.hip", "preprocess.hip", "eval.hip", "cascade.hip", "jpeg.hip", "batch.hip", "bertscore.hip", "valid.hip", "audio.hip", "whisper_dec.hip", "whisper_align.hip", "whisper_prefill.hip", "whisper_enc_x3.hip"]
ARCH = "gfx950"
# attention's softmax only ever sees finite values (masked scores are -3e38, not -inf): dropping NaN handling removes
# the canonicalising v_max the compiler otherwise puts in front of every fmaxf on an MFMA result
EXTRA_FLAGS = {"attention.hip": ["-ffinite-math-only"],
               "attention_long.hip": ["-ffinite-math-only"],
               # Pillow-exact weight tables (host doubles) and the reference's (x/255-mean)/std: no fused multiply-adds
               "preprocess.hip": ["-ffp-contract=off"],
               # evaluate.py's double-precision interval arithmetic, operation for operation
               "eval.hip": ["-ffp-contract=off"],
               # the same bins (timeline_bins.h) between the cascade's stages
               "cascade.hip": ["-ffp-contract=off"],
               # numpy's linspace(0, n - 1, F) in double for the subsample rows
               "batch.hip": ["-ffp-contract=off"]}


def hipcc_path() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.isfile(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm >= 7.0 to build the gfx950 kernels)")


def _headers():
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + \
           [os.path.join(os.path.dirname(HERE), "include", "hirest_hip.h"), os.path.abspath(__file__)]


def _obj_stale(src: str, obj: str) -> bool:
    if not os.path.isfile(obj):
        return True
    t = os.path.getmtime(obj)
    return any(os.path.getmtime(d) > t for d in [src] + _headers())


def build(force: bool = False, verbose: bool = True) -> str:
    """Compile the stale objects (in parallel) and relink.  An object is stale when its source, any header or this
    file (the flags) is newer than it."""
    from concurrent.futures import ThreadPoolExecutor
    os.makedirs(LIB_DIR, exist_ok=True)
    objs, jobs = [], []
    for src in SOURCES:
        obj = os.path.join(LIB_DIR, src.replace(".hip", ".o"))
        objs.append(obj)
        if not force and not _obj_stale(os.path.join(CSRC, src), obj):
            continue
        cmd = [hipcc_path(), f"--offload-arch={ARCH}", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast"]
        cmd += EXTRA_FLAGS.get(src, [])
        cmd += ["-c", os.path.join(CSRC, src), "-o", obj]
        jobs.append(cmd)

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    if jobs:
        with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 1)) as ex:
            list(ex.map(run, jobs))
    if jobs or not os.path.isfile(LIB_PATH) or any(os.path.getmtime(o) > os.path.getmtime(LIB_PATH) for o in objs):
        run([hipcc_path(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB_PATH] + objs)
    return LIB_PATH


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
