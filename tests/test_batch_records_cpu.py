"""CPU: the batch fill's record rules (csrc/s3dg_batch_plan.h: lead, tile
count, tiled and dense record ranges, the own / whole-wave cut, the slot ->
block rule, the split rule; csrc/s3dg_prefix.h: the prefix parameters), the
functions the host's pass and the device's scan functor and k_batch_map share.

tests/capi/batch_records_sweep.cpp is compiled with g++ against those headers
alone (no HIP, no library), plain and under the address and undefined-behaviour
sanitizers.  Without arguments it sweeps generated descriptor sets (base
granule 0..7 with a sub-granule offset of 0 or 16, every tile and auto, split
0 / 2 / 16, aligned and 16-byte packed offsets, sizes around one, two, 16, 17
and 65 tiles, empties, three orders) and the prefix parameters, and asserts
coverage itself: every block in exactly one live slot, every record written by
exactly one object, the sums of the pass, the partition of two classes, the
merge of the pass's parts, the writer cut at 16 records, and slot = granule
modulo 8 (dense, tiles of 8 blocks and more) or modulo the tile (2 and 4
blocks).  With "cases" it does the same for the named lists of
tests/batch_record_cases.py and prints the plan each sub-batch got.
"""
import os
import shutil
import subprocess

import pytest

import batch_record_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "capi", "batch_records_sweep.cpp")


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def sweep(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path_factory.mktemp("batch_records") / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param else []
    # no ROCm include path: the headers must stand without HIP
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
                           "-o", exe, SRC])
    return exe


def test_sweep(sweep):
    out = subprocess.run([sweep], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = [line.split() for line in out.stdout.splitlines()]
    count = {r[0]: int(r[1]) for r in rows if r[0] != "shift"}
    assert count["subs"] > 40000 and count["merges"] > 15000 and count["prefix"] > 60000
    assert count["uniform"] >= 180 and count["dense"] > 1500 and count["two_class"] > 5000
    shifts = {int(r[1]): dict(zip(r[2::2], map(int, r[3::2]))) for r in rows if r[0] == "shift"}
    assert sorted(shifts) == [0, 1, 2, 3, 4, 5, 6]
    for sh, c in shifts.items():
        # (viii) objects of exactly 16 and 17 records at every shift, in the dense layout through gaps
        assert c["recs16"] > 0 and c["recs17"] > 0 and c["live"] > 1000000, (sh, c)
        # (vi) slot = granule modulo 8 everywhere but at 2- and 4-block tiles,
        # where the sweep asserts it modulo the tile and finds it broken modulo 8
        assert (c["off_mod8"] > 0) == (sh in (1, 2)), (sh, c)
    assert all(shifts[sh]["over64"] > 0 for sh in (0, 1, 2, 3, 4))   # the wave loop's second pass


@pytest.fixture(scope="module")
def plans(sweep):
    text = "".join(K.sweep_input(c) for c in K.CASES)
    out = subprocess.run([sweep, "cases"], input=text, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {}
    for line in out.stdout.splitlines():
        head, _, tail = line.partition(" | ")
        words = head.split()
        assert words[0] == "plan"
        got[words[1]] = (tuple(words[2:]), tuple(int(w.split("=")[1]) for w in tail.split()))
    assert sorted(got) == sorted(K.BY_NAME)
    return got


@pytest.mark.parametrize("name", [c.name for c in K.CASES])
def test_case_reaches_its_plan(plans, name):
    """The list passes every assertion of the sweep and runs as the plan it
    names; a map_paths list holds the 16-, 17- and over-64-record objects it is for."""
    plan, counts = plans[name]
    assert plan == K.BY_NAME[name].plan
    if name in K.MAP_COUNTS:
        assert counts == K.MAP_COUNTS[name]


def test_map_paths_are_all_counted():
    assert {n for n in K.GROUPS["map_paths"] if n != "one_record_t64"} == set(K.MAP_COUNTS)


def test_lists_hold_what_they_are_for():
    """The builders' own coverage: every lead two ways in every leads list, the
    tile edges, the tails; the dense gaps and sizes; the cuts' sizes."""
    for name in K.GROUPS["leads"]:
        c = K.BY_NAME[name]
        T = c.tile or 8
        seen = {(K.lead_of(c.shift, o[0]), o[0] % K.BLK) for o in c.objs}
        assert seen == {(g, sub) for g in range(8) for sub in (0, 4080)}, name
        assert c.shift % 16 == 0 and (("shift" in name) == (c.shift % K.BLK == 16 and c.shift >= K.BLK))
        edges = {(-(-o[1] // K.BLK) + K.lead_of(c.shift, o[0])) - m * T for o in c.objs for m in (1, 2)}
        assert {-1, 0, 1} <= edges
        assert {(o[1] - 1) % K.BLK + 1 for o in c.objs} >= {1, 16, 4095, 4096}
        assert {1, 16} <= {o[1] for o in c.objs}
    c = K.BY_NAME["dense_full_g5"]
    gaps = {((b[0] - a[0]) - -(-a[1] // K.BLK) * K.BLK) // K.BLK for a, b in zip(c.objs, c.objs[1:])}
    assert gaps >= set(K.GAPS) and {-(-o[1] // K.BLK) for o in c.objs} >= set(K.DENSE_BLOCKS)
    firsts = {(K.BY_NAME[n].shift // K.BLK, K.BY_NAME[n].objs[0][0] // K.BLK) for n in K.GROUPS["dense_front"]}
    assert firsts >= {(g, 0) for g in range(1, 8)} | {(0, g) for g in range(1, 8)}
    for n in (16383, 16384, 16385, 49153):
        c = K.BY_NAME[f"cuts_n{n}"]
        assert len(c.objs) == n and {o[1] for o in c.objs} == set(K.CUT_SIZES) and c.end < 100 * 10**6
        assert all(o[0] % 16 == 0 for o in c.objs)
    assert all(o[1] == 0 for o in K.BY_NAME["cuts_empty_middle"].objs[16384:49152])
    assert max(c.end for c in K.CASES if not c.name.startswith("cuts_")) <= 64 * K.MiB + 5 * K.BLK
