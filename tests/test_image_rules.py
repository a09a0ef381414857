"""The argument rules of the image stages' older calls live in csrc/pt_plan.h, where csrc/pt_variants_check.cpp walks them — every
rule broken alone and together, the first in the header's order answering (tests/test_variants.py builds and runs that program,
plain and sanitized).  Here: each entry point's file asks the function the program walks, and states no rule of its own.  No GPU."""
import os
import re

import pytest

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "g.p.u-pathtracer_amd", "csrc")

# entry point: (its file, the call of the rules it makes, the piece of pt_variants_check.cpp that walks them)
MOVED = {
    "pt_render_aux": ("pt_aux.hip", "check_aux_call(f, p,", "check_aux_call(f, broken & 16 ? nullptr : &p"),
    "pt_denoise": ("pt_filter.hip", "check_denoise_call(dp,", "check_denoise_call(broken & 16 ? nullptr : &dp"),
    "pt_denoise_variance": ("pt_filter.hip", "check_denoise_variance_call(dp,", "check_denoise_variance_call(broken & 128 ? nullptr : &dp"),
    "pt_temporal": ("pt_temporal.hip", 'temporal_args(c, "pt_temporal", a, M)', '{TEMPORAL_COLOUR, "pt_temporal"}'),
    "pt_temporal_motion": ("pt_temporal.hip", 'temporal_args(c, "pt_temporal_motion", a, M)', '{TEMPORAL_MOTION, "pt_temporal_motion"}'),
    "pt_temporal_moments": ("pt_temporal.hip", 'temporal_args(c, "pt_temporal_moments", a, M)', '{TEMPORAL_MOMENTS, "pt_temporal_moments"}'),
    "pt_frame_error": ("pt_select.hip", "check_frame_error_call(moments_dev &&", "check_frame_error_call(!(broken & 1)"),
}


def entry_point(text, name):
    """The body of extern "C" int `name`(...)."""
    start = text.index('extern "C" int %s(' % name)
    nxt = text.find('extern "C"', start + 1)
    return text[start:nxt if nxt >= 0 else len(text)]


@pytest.mark.parametrize("name", list(MOVED))
def test_entry_point_asks_the_rules_the_check_program_walks(name):
    fname, asks, walked = MOVED[name]
    body = entry_point(open(os.path.join(CSRC, fname)).read(), name)
    assert asks in body, "the entry point asks pt_plan.h"
    assert body.index('"null ctx"') < body.index(asks), "null ctx stays first and outside the rules"
    assert len(re.findall(r"PT_ERR_INVALID|PT_ERR_UNSUPPORTED|PT_ERR_NO_SCENE", body)) == 1, "no rule of its own but null ctx"
    check = open(os.path.join(CSRC, "pt_variants_check.cpp")).read()
    assert walked in check, "the check program walks them"
    assert "first_answers(check_" in check


def test_the_reprojections_share_one_function():
    text = open(os.path.join(CSRC, "pt_temporal.hip")).read()
    assert text.count("check_temporal_call(") == 1 and "check_temporal_call(fn, a)" in text
    plan = open(os.path.join(CSRC, "pt_plan.h")).read()
    assert plan.count("inline Refusal check_temporal_call(const std::string& who, const TemporalCall& a)") == 1
    rules = plan[plan.index("inline Refusal check_aux_call("):plan.index("// ---- pt_closest_hits")]
    assert "*a." not in rules and "*b." not in rules and "[0]" not in rules, "device pointers are compared, never read"
