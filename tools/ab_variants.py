"""Build the remaining compile-time variants of the kernel library and time them against the shipped build on one GPU.

    python tools/ab_variants.py            # builds lib/libtriforce_hip_<name>.so for every variant, then runs
                                           # tools/tune.py (cold-cache kernel timings) once per library

Each knob's shipped value is the measured winner (profiles/r02_gemm_pipeline_ab.jsonl and the files named below); the
variants are the losing sides, kept buildable for re-measurement on new silicon / compilers.  The attention kernels'
rejected variants (load pipelines, P rounding, slab forms, LDS-DMA selection ...) are no longer buildable: their
measurements are in profiles/ (README.md there), their code in the history of triforce_amd/csrc/attn.hip.
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from triforce_amd.build import LIB_PATH, build_variant  # noqa: E402

VARIANTS = {"sgu8": ["SG_U=8"], "sgu2": ["SG_U=2"], "sgw8": ["SG_WAVES=8"],
            "reslate": ["TF_SG_RES_EARLY=0"],        # residual operands loaded at the GEMM's tail (tools/gemm_resid_ab.py)
            # round 4: the many-split in-launch attention merge off, the retrieval scorer's round-3 grid rule
            "bigmerge": ["FUSED_MERGE_BIG_SPLITS=64"], "rscoreceil": ["TF_RSCORE_CAP_CEIL=1"],
            "sgtail0": ["SG_TAIL_BATCH=0"],          # K-loop tail one chunk at a time (round 3)
            "sgprol0": ["SG_PROLOGUE_ORDER=0"],      # norm-GEMM prologue in round 3's load order (weights first, x after the fold)
            "sgprol1": ["SG_PROLOGUE_ORDER=1"],      # ... in round 4's first form (same order behind branches: the compiler threads it)
            "lnpre": ["SG_LN_PRE=1"],                # the first batch's norm weights prefetched with the prologue (+16 registers)
            "epilate0": ["SG_EPI_LATE=0"],           # plain GEMMs fetch their epilogue operands in front of the first weight batch
            "nopreload": ["!kernarg-preload"],       # built without -mllvm -amdgpu-kernarg-preload-count=14
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
