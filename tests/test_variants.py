"""The kernel families' variant words (csrc/pt_variants.h): every request the host can make of a launcher has an
instantiated kernel and every instantiated kernel has a request, checked on the host by csrc/pt_variants_check.cpp.  No GPU."""
import os
import re
import subprocess

import pytest

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PKG = os.path.join(ROOT, "g.p.u-pathtracer_amd")
CSRC = os.path.join(PKG, "csrc")

# kernels per family at the commit that introduced the words (hipcc's resource remarks, profiles/r22_variants_isa.txt)
KERNELS = {"k_trace_mega_bvh2": 90, "k_trace_persist_bvh2": 76, "k_render_rays": 19, "k_query_rays": 4, "k_wf_extend": 20, "k_wf_shade": 36,
           "k_wf_shade_last_any": 10, "k_wf_extend_packet_shade": 6}


@pytest.mark.parametrize("san", ["", "SAN=1"], ids=["plain", "sanitized"])
def test_variants_check_program(san):
    exe = os.path.join(CSRC, "pt_variants_check")
    build = subprocess.run(["make", "-B", "-C", PKG, "variants_check"] + ([san] if san else []), capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    assert ("-fsanitize=address,undefined" in build.stdout) == bool(san), build.stdout
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks hold" in run.stdout and "FAILED" not in run.stdout
    rows = {m.group(1): (int(m.group(2)), int(m.group(3)), int(m.group(4)))
            for m in re.finditer(r"^(\w+)\s+(\d+) requests,\s+(\d+) distinct words,\s+(\d+) kernels$", run.stdout, re.M)}
    assert set(rows) == set(KERNELS), run.stdout
    for family, (requests, words, kernels) in rows.items():
        assert kernels == KERNELS[family] and words == kernels and requests >= words, (family, run.stdout)


def test_the_library_includes_no_check_program():
    """The check program stays out of libptmi.so; the headers it checks are ones the kernels' objects depend on and are plain C++:
    they include nothing of the project but the C ABI's constants (the planner: and the variant words), and name no runtime call
    and no runtime type."""
    make = open(os.path.join(PKG, "Makefile"), encoding="utf-8").read()
    assert "pt_variants_check" not in re.search(r"^OBJS = (.*)$", make, re.M).group(1)
    includes = {"pt_variants.h": ["cstdint", "../../include/ptmi.h"],
                "pt_plan.h": ["algorithm", "climits", "cstdint", "string", "../../include/ptmi.h", "pt_variants.h"]}
    for header, expected in includes.items():
        assert re.search(r"^KHDR = .*csrc/%s\b" % re.escape(header), make, re.M), header
        assert re.search(r"^csrc/pt_variants_check: .*csrc/%s\b" % re.escape(header), make, re.M), header
        text = open(os.path.join(CSRC, header), encoding="utf-8").read()
        assert re.findall(r'#include [<"](.*)[>"]', text) == expected, header
        assert not re.search(r"\bhip[A-Z]\w*\(|\bhip\w+_t\b|__device__|__global__|\bfloat4\b|\bdim3\b", text), header
