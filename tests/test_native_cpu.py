"""Host-side checks of header-only pieces of the kernels (plain C++ compiled with g++; no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_tree_mask_funnel_matches_the_per_key_rule(tmp_path):
    """tf_tree_vis8 (csrc/tree_mask.h, the funnel-shift form of the tree-attention mask read) against the
    per-key rule, exhaustively over tree offsets / alignments / lengths and random mask rows."""
    exe = tmp_path / "test_tree_mask"
    subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(ROOT, "tests", "native", "test_tree_mask.cpp"), "-o", str(exe)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    assert out.startswith("OK "), out


@pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")
def test_skinny_gemm_launch_rule_pins_the_shipped_forms(tmp_path):
    """sg_pick_form / sg_pick_ks (csrc/sg_rule.h, the launch rule csrc/gemv.hip dispatches) at the default knobs for
    every decode GEMM of the 7B / 13B configurations, whole and as a TP-8 rank's shard, at 1 / 8 / 16 / 17 / 32 rows,
    and the knob edges the GPU tests set through tf_sg_tune (keys 0, 3, 4)."""
    exe = tmp_path / "test_sg_rule"
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "test_sg_rule.cpp"),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK "), out.stdout
