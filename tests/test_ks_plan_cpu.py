"""CPU: the plan of the uniform keystream launches (csrc/s3dg_ks_plan.h: lanes,
lane regions, the DG1 call's zero-split decisions, the half-length tail set,
the static and the persistent grid, the XCD remap, the queue quotas, fastmod)
without a GPU.  tests/capi/ks_plan_sweep.cpp asserts the plan's properties over
a sweep, compiled with g++ alone, plain and under the address and
undefined-behaviour sanitizers; tests/capi/ks_plan_table.cpp prints the plan
and tests/keystream_cases.py restates it: every line is equal.  Then every
case builder of tests/keystream_cases.py runs at 256 and 304 compute units,
so the coverage each asserts of its own list holds in this suite
(tests/test_gpu_keystream_edges.py runs the lists on a device)."""
import os
import shutil
import subprocess

import pytest

import keystream_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = (256, 304)
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]


def _run(tmp_path, name, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / name)
    # no ROCm include path: the plan header stands alone
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *(SAN if sanitize else []),
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", name + ".cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return out.stdout.splitlines()


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_sweep(tmp_path, sanitize):
    """lpc a power of two in [1, 1024]; span a multiple of D with lpc * span >=
    the chunk's draws; the regions of a chunk tile [8 z0, clen) exactly once
    and none passes clen; the lanes the rules give, a z0 tail's 64 among them;
    the remap a permutation; the quotas' sum and every queue unit distinct; A
    and A2 covering each chunk once; the split decisions; fastmod == %."""
    rows = dict(line.split("|", 1) for line in _run(tmp_path, "ks_plan_sweep", sanitize))
    assert int(rows["plans"]) > 500000


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_restatement_equals_the_header(tmp_path, sanitize):
    got, want = _run(tmp_path, "ks_plan_table", sanitize), K.table_lines()
    assert len(want) > 70000 and len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    assert {w.split()[0] for w in want} == {"lanes", "region", "call", "tail", "grid", "persist", "remap", "quota", "fastmod"}


def test_restated_ratio_is_the_library_s():
    import s3dlio_amd as S
    for comp in (1, 2, 3, 7, (3, 2), (20, 1), (100, 1), (256, 1), (65535, 32768)):
        fn, fd = K.ratio_of(comp)
        sn, sd = S.compress_ratio(comp)
        assert sn * fd == fn * sd and K.MIB * sn // sd == K.MIB * fn // fd, comp


@pytest.mark.parametrize("cus", CUS)
def test_k2_geometry_builder(cus):
    sizes = K.k2_geometry(cus)
    assert len(sizes) == 12 and all(c % 128 == 0 for c in sizes)
    for chunk in sizes + K.K2_BIG:
        for n in ((1,) if chunk in K.K2_BIG else (1, 3)):
            for D in K.DRAWS:
                cuts = K.k2_cuts(cus, chunk, n, D)
                assert cuts[-1] == chunk and 36 <= len(cuts) <= 106


@pytest.mark.parametrize("cus", CUS)
def test_split_ratio_builder(cus):
    R = K.split_ratios(cus)
    assert len(R) == 7 + 17 + 2
    for D in K.DRAWS:
        for comp in (3, (3, 2), K.compress_of(*R["lanes4"])):
            K.ragged_split(cus, 2 * K.MIB + 77, 1, comp, D)
            K.ragged_split(cus, 5 * K.MIB + 4093, 1, comp, D)
            K.ragged_split(cus, 2 * K.MIB + 1, 3, comp, D)


@pytest.mark.parametrize("cus", CUS)
def test_long_lane_builder(cus):
    sizes = {d: K.long_lanes(cus, d)[0] for d in (512, 1024, 2048)}
    assert [sizes[d] // K.MIB for d in (512, 1024, 2048)] == [cus, 2 * cus, 4 * cus]
    for d in (512, 1024):
        size, knob, comp = K.long_lanes(cus, d, True)
        assert size == sizes[d] and knob == d and comp == K.late_prefix()


@pytest.mark.parametrize("cus", CUS)
def test_persistent_builders(cus):
    n, L = K.persistent_dgen(cus, 1, 1, 16)
    assert n == 33 if cus == 256 else n > 33
    for D in K.DRAWS:
        for waves in (1, 2, 4):
            for xcd in (1, 4, 16):
                K.persistent_dgen(cus, 1, waves, xcd, D)
                for rem in (1, 7):
                    n, L = K.persistent_k2(cus, 1, waves, xcd, rem, D=D)
                    assert n * 65664 < 512 * K.MIB


@pytest.mark.parametrize("cus", CUS)
def test_half_tail_builder(cus):
    for D in K.DRAWS:
        for T in (1, 3, 32):
            for persist in (0, 1):
                for ragged in (False, True):
                    size, knob, L = K.half_tail_object(cus, 1, T, persist, ragged, D=D)
                    assert size <= max(cus, 256) * K.MIB and L["A2"]["nwg"] == 8 * T
        # an A2 set whose workgroups are no multiple of 8: 128 lanes per chunk, T = 3
        size, knob, L = K.half_tail_object(cus, 1, 3, 1, True, lpc=128, D=D)
        assert L["A2"]["nwg"] == 12 and L["grid"]


def test_far_blocks():
    assert K.FAR_BLOCKS * K.MIB < 1 << 63 and K.FAR_RANGES[-1][1] > K.FAR_BLOCKS
    assert K.far_seed(5, 7, 3) == 5 ^ K.PHI and K.far_seed(0, (1 << 32) - 2, 1 << 32) == ((1 << 32) - 2) * K.PHI % (1 << 64)
