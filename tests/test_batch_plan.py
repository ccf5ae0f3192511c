"""The layout a mixed-size batch gets (csrc/s3dg_batch_plan.h: the pass over
the descriptors, the merge of its parts and plan_sub_batch), pinned on the CPU.

tests/capi/batch_plan_cases.cpp is compiled with g++ against that header alone
(no HIP, no library), fed generated descriptor sets and compared with
tests/golden/batch_plan_cases.json, which holds the generator parameters and
the plan each set got from the code before the plan became a function of its
own: uniform (run as a stream), the tile shift (0 = dense), the classes with
their object counts, tile shifts and records, the total records, the dense
span, the first object's granule and the majority zero class, or the error a
refused set reports.
"""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "capi", "batch_plan_cases.cpp")
with open(os.path.join(ROOT, "tests", "golden", "batch_plan_cases.json")) as f:
    CASES = json.load(f)["cases"]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """Every case's plan at every lead, from one run of the program."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path_factory.mktemp("batch_plan") / "batch_plan_cases")
    # no ROCm include path: the header must stand without HIP
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-o", exe, SRC])
    lines = [f"lead={lead} {c['spec']}" for c in CASES for lead in c["leads"]]
    out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    got = out.stdout.splitlines()
    assert len(got) == len(lines)
    return dict(zip(lines, got))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_plan(plans, case):
    assert len(case["expect"]) == len(case["leads"])
    for lead, want in zip(case["leads"], case["expect"]):
        assert plans[f"lead={lead} {case['spec']}"] == want, (case["name"], lead)


def test_cases_reach_every_branch():
    """The fixture itself: every kind of plan and every error is in it."""
    rows = [e.split() for c in CASES for e in c["expect"]]
    plans_ = [[int(x) for x in r] for r in rows if r[0] != "ERR"]
    assert any(p[0] == 1 for p in plans_)                               # a stream
    assert any(p[0] == 0 and p[1] == 0 and p[2] == 1 for p in plans_)   # dense
    assert any(p[2] == 2 and p[4] != p[7] for p in plans_)              # two classes, two tile sizes
    assert any(p[2] == 0 for p in plans_)                               # all empty
    assert {p[1] for p in plans_} >= {0, 1, 2, 3, 4, 5, 6}
    assert {p[12] for p in plans_} == {0, 1, 2}
    assert {p[11] for p in plans_} >= {0, 3, 7}
    msgs = {" ".join(r[2:]) for r in rows if r[0] == "ERR"}
    assert msgs == {"dst_off must be a multiple of 16", "need f_num < f_den", "object larger than 2^31 blocks"}
