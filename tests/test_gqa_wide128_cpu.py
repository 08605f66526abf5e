"""The 128-row grouped-query decode attention: launch rule, knob, entry point and zoo config."""
import os
import re

import pytest

from triforce_amd import hip, ops
from triforce_amd.models import zoo


# 17 rows at 32 / 8, 28 / 4, 40 / 8 heads; 128 / 8 at 7; 65 and 128 rows; then 64, 49, 28 rows and 129 / 144 (past eight q-tiles)
@pytest.mark.parametrize("g,sq,want", [(4, 17, True), (7, 17, True), (5, 17, True), (16, 7, True), (13, 5, True), (16, 8, True),
                                       (8, 8, False), (7, 7, False), (4, 7, False), (43, 3, False), (16, 9, False)])
def test_gqa_wide128_applies(g, sq, want):
    assert ops.gqa_wide128_applies(g, sq) is want and not (want and ops.gqa_wide_applies(g, sq))


@pytest.mark.parametrize("env,want", [({}, (True, 64)), ({"TRIFORCE_GQA_WIDE": "1"}, (True, 64)),
                                      ({"TRIFORCE_GQA_WIDE": "0"}, (False, 64)), ({"TRIFORCE_GQA_WIDE": "128"}, (True, 128))])
def test_knob(env, want):
    assert ops._gqa_wide_knob(env) == want
    with pytest.raises(ValueError, match="TRIFORCE_GQA_WIDE"):
        ops._gqa_wide_knob({"TRIFORCE_GQA_WIDE": "64"})


def test_entry_point_declared_and_bound_and_tiny_gqa16_loads():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "triforce_hip.h")).read()
    assert re.search(r"^int tf_attn_decode_gqa_wide128_act\(", header, re.M) and \
        hip.SIGNATURES["tf_attn_decode_gqa_wide128_act"] == hip.SIGNATURES["tf_attn_decode_gqa_act"]
    c = zoo.config("tiny-gqa16")
    assert (c.num_attention_heads, c.num_key_value_heads, c.hidden_size // c.num_attention_heads) == (16, 1, 128)
    assert ops.gqa_wide128_applies(16, 7) and ops.gqa_wide128_applies(16, 8)
