"""Build the remaining compile-time variants of the kernel library and time them against the shipped build on one GPU.

    python tools/ab_variants.py            # builds lib/libtriforce_hip_<name>.so for every variant, then runs
                                           # tools/tune.py (cold-cache kernel timings) once per library

Each knob's shipped value is the measured winner; the variants are the losing sides, kept buildable for re-measurement
on new silicon / compilers.  The rejected variants of the attention kernels (load pipelines, P rounding, slab forms,
LDS-DMA selection ...) and of the skinny GEMM (prologue orders, tail walk, epilogue prefetch, in-flight depth, wave
counts ...) are no longer buildable: their measurements are in profiles/ (README.md there), their code in the history of
triforce_amd/csrc/attn.hip and triforce_amd/csrc/gemv.hip.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from triforce_amd.build import LIB_PATH, build_variant  # noqa: E402

VARIANTS = {"nopreload": ["!kernarg-preload"],       # built without -mllvm -amdgpu-kernarg-preload-count=14
            # round 6: the fully two-deep load loop of the decode attention forced onto the long streams
            # (tools/verify_bench.py <tag> with TRIFORCE_HIP_LIB set)
            "eagerall": ["TF_ATTN_EAGER_TILES=1000000"]}

if __name__ == "__main__":
    names = sys.argv[1:] or list(VARIANTS)
    libs = {"default": LIB_PATH}
    for n in names:
        libs[n] = build_variant(n, VARIANTS[n], verbose=False)
    for tag, lib in libs.items():
        env = dict(os.environ, TRIFORCE_HIP_LIB=lib)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "tune.py"), tag], env=env, capture_output=True,
                             text=True)
        line = [l for l in out.stdout.splitlines() if l.startswith("{")]
        print(json.dumps({"tag": tag, "result": json.loads(line[-1]) if line else out.stderr[-400:]}), flush=True)
