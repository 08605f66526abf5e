"""The launch rule of the wide grouped-query decode attention and the presence of its entry point."""
import os
import re

import pytest


# 28 / 4, 64 / 8, 40 / 8 heads at 7 rows; tiny-gqa at 17; 28 / 4 at 9; then 28 rows (one pass already) and 72 (past four q-tiles)
@pytest.mark.parametrize("g,sq,want", [(7, 7, True), (8, 7, True), (5, 7, True), (2, 17, True), (7, 9, True),
                                       (4, 7, False), (8, 9, False)])
def test_gqa_wide_applies(g, sq, want):
    from triforce_amd import ops
    assert ops.gqa_wide_applies(g, sq) is want


def test_entry_point_declared_and_bound():
    from triforce_amd import hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "triforce_hip.h")).read()
    assert re.search(r"^int tf_attn_decode_gqa_wide_act\(", header, re.M)
    assert hip.SIGNATURES["tf_attn_decode_gqa_wide_act"] == hip.SIGNATURES["tf_attn_decode_gqa_act"]
