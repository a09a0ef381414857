"""Ownership of device resources (csrc/pt_own.h): the rule that only the owners name the runtime's allocate /
free / create / destroy calls, and the owners themselves, exercised on the host over stubs of those calls.  No GPU."""
import os
import re
import subprocess

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
PKG = os.path.join(ROOT, "g.p.u-pathtracer_amd")
CSRC = os.path.join(PKG, "csrc")

RAW_CALLS = ("hipMalloc(", "hipFree(", "hipEventCreate", "hipEventDestroy(", "hipStreamCreate", "hipStreamDestroy(")
# pt_own.h holds the owners; pt_own_check.cpp is no part of the library: it DEFINES these calls, as the stubs the owners run over
ALLOWED = ("pt_own.h", "pt_own_check.cpp")


def test_only_the_owners_name_the_raw_calls():
    sources = sorted(f for f in os.listdir(CSRC) if re.search(r"\.(h|hip|cpp)$", f))
    assert "pt_own.h" in sources and "ptmi.hip" in sources and len(sources) >= 20, sources
    found = []
    for name in sources:
        text = open(os.path.join(CSRC, name), encoding="utf-8").read()
        for lineno, line in enumerate(text.splitlines(), 1):
            found += [(name, lineno, call) for call in RAW_CALLS if call in line]
    outside = [f for f in found if f[0] not in ALLOWED]
    assert not outside, f"raw runtime calls outside csrc/pt_own.h: {outside}"
    assert {call for name, _, call in found if name == "pt_own.h"} >= {"hipMalloc(", "hipFree(", "hipEventCreate", "hipEventDestroy(",
                                                                         "hipStreamCreate", "hipStreamDestroy("}


def test_the_library_includes_no_stub():
    """The check program stays out of libptmi.so and the owners' header includes nothing of the project."""
    make = open(os.path.join(PKG, "Makefile"), encoding="utf-8").read()
    objs = re.search(r"^OBJS = (.*)$", make, re.M).group(1)
    assert "pt_own_check" not in objs
    assert re.search(r"^KHDR = .*csrc/pt_own\.h", make, re.M)
    own = open(os.path.join(CSRC, "pt_own.h"), encoding="utf-8").read()
    assert re.findall(r'#include "(.*)"', own) == []


def test_own_check_program():
    build = subprocess.run(["make", "-C", PKG, "own_check"], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([os.path.join(CSRC, "pt_own_check")], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks hold" in run.stdout and "FAILED" not in run.stdout
