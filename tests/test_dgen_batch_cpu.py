"""CPU: the DG1 batch surface without a GPU: the call's plan
(csrc/s3dg_dgen_batch_plan.h, compiled with g++ alone, plain and under the
address and undefined-behaviour sanitizers) over a sweep of descriptor lists,
the C entry points seen from a C program, the Python methods' bounds
checks, and the lists of tests/dgen_batch_cases.py: its restatement of the
plan against the header, line by line, and every builder's coverage."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3dlio_gpu.h")

# the contract's refusal texts (include/s3dlio_gpu.h) as the sweep prints them
REFUSALS = {
    "null_out": "null output",
    "null_out_empty": "null output",
    "null_descs": "null descriptor array",
    "null_dst": "dst_base must be 16-byte aligned",
    "odd_dst": "dst_base must be 16-byte aligned",
    "null_src": "src_base must be 16-byte aligned",
    "odd_src": "src_base must be 16-byte aligned",
    "odd_off": "object 2: dst_off must be a multiple of 16",
    "ratio": "object 1: need f_num < f_den",
    "f_den": "object 3: need f_num < f_den",
    "large": "object 0: object larger than 2^32 blocks",
    "far": "object 70000: need f_num < f_den",
    "grid": "more than 2^31 lanes in one launch",
}


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_sweep(tmp_path, sanitize):
    """tests/capi/dgen_batch_plan_sweep.cpp asserts the plan's properties
    itself: every byte of every object in exactly one lane region of exactly
    one launch, no region past its chunk's end, verify regions of whole
    granules, the records' seeds, prefixes and offsets.  Its refusal texts, each
    naming the first offender, are the C calls' (tests/test_gpu_dgen_batch.py
    meets the same texts on a device)."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    # no ROCm include path: the plan header needs the public header and its own neighbours only
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-I", os.path.dirname(HEADER), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "dgen_batch_plan_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = dict(line.split("|", 1) for line in out.stdout.splitlines())
    assert int(rows.pop("plans")) > 60000
    assert rows == REFUSALS


def test_refusal_texts_are_in_the_public_header():
    text = "".join(open(HEADER).read().replace(" * ", " ").split())
    for msg in set(REFUSALS.values()) - {"more than 2^31 lanes in one launch"}:
        msg = msg.split(": ", 1)[-1]
        if msg.endswith("_base must be 16-byte aligned"):
            assert '"dst_base/src_basemustbe16-bytealigned"' in text
        else:
            assert f'"{msg}"'.replace(" ", "") in text, msg


def test_c_program_sees_the_entry_points(tmp_path):
    """Both calls link from C; a null context is refused with a message before
    anything else, and the verify's outputs are written only on success."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    from s3dlio_amd._lib import LIB_PATH
    src = tmp_path / "db.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "s3dlio_gpu.h"
int main(void) {
    s3dg_obj_desc d = {0, 4096, 1, 1, 0, 1};
    s3dg_verify_result tot, per[1], was;
    memset(&tot, 0x5A, sizeof tot);
    memset(per, 0x5A, sizeof per);
    memset(&was, 0x5A, sizeof was);
    int rc = s3dg_dgen_fill_batch(NULL, (void *)16, &d, 1, NULL);
    if (rc != S3DG_EINVAL || strcmp(s3dg_last_error(), "null context")) return 2;
    rc = s3dg_verify_dgen_batch(NULL, (const void *)16, &d, 1, NULL, &tot, per);
    if (rc != S3DG_EINVAL || strcmp(s3dg_last_error(), "null context")) return 3;
    rc = s3dg_verify_dgen_batch(NULL, NULL, NULL, 0, NULL, NULL, NULL);
    if (rc != S3DG_EINVAL || strcmp(s3dg_last_error(), "null context")) return 4;
    if (memcmp(&tot, &was, sizeof tot) || memcmp(per, &was, sizeof was)) return 5;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "db"
    libdir = os.path.dirname(LIB_PATH)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                           "-L", libdir, "-ls3dlio_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out


class _FakeTensor:
    """What Context._dst asks of a tensor, without a device."""
    is_cuda = True

    class device:
        index = 0

    def __init__(self, nbytes):
        self._n = nbytes

    def data_ptr(self):
        return 4096

    def is_contiguous(self):
        return True

    def numel(self):
        return self._n

    def element_size(self):
        return 1


def test_python_bounds_checks():
    """The wrappers check every object against the buffer before any call: a
    context without a handle never reaches the library."""
    import s3dlio_amd as S
    from s3dlio_amd import _lib
    assert "s3dg_dgen_fill_batch" in _lib.SIGNATURES and "s3dg_verify_dgen_batch" in _lib.SIGNATURES
    ctx = S.Context.__new__(S.Context)
    ctx.device, ctx._h = 0, None
    t = _FakeTensor(1 << 20)
    arr, n, need = ctx._dgen_descs([(16, 100, 7, 2, 3), (4096, 0, 1, 1, 1), (1 << 19, 1 << 19, 2**64 + 5, 1, 1.5)])
    assert n == 3 and need == 1 << 20
    assert (arr[0].dst_off, arr[0].size, arr[0].entropy, arr[0].dedup, arr[0].f_num, arr[0].f_den) == (16, 100, 7, 2, 2, 3)
    assert arr[2].entropy == 5 and (arr[2].f_num, arr[2].f_den) == S.compress_ratio(1.5)
    assert ctx._dgen_descs(iter(()))[1:] == (0, 0)
    assert ctx._dgen_descs([(1 << 40, 0, 1, 1, 1)])[2] == 0          # an empty object reaches nothing
    over = [(16, 100, 1, 1, 1), ((1 << 20) - 100, 101, 2, 1, 1)]
    with pytest.raises(ValueError, match="writes 1048577 bytes, the tensor holds 1048576"):
        ctx.dgen_fill_batch(t, over)
    with pytest.raises(ValueError, match="reads 1048577 bytes, the tensor holds 1048576"):
        ctx.verify_dgen_batch(t, over)
    with pytest.raises(ValueError, match="reads"):
        ctx.verify_dgen_batch(t, over, per_object=False)
    for bad in ([(-16, 5, 1, 1, 1)], [(0, -1, 1, 1, 1)], [(0, 16, 1, 1, 1), (2**64, 1, 1, 1, 1)]):
        with pytest.raises(ValueError, match="64 unsigned bits"):
            ctx.dgen_fill_batch(t, bad)
    with pytest.raises(ValueError, match="beyond|writes"):
        ctx.dgen_fill_batch(t, [(2**64 - 16, 32, 1, 1, 1)])
    ctx._h = None                                                     # nothing for __del__ to close


# ---- the plan restated in Python, and the lists built from it --------------------------------

def _table_lines():
    """tests/capi/dgen_batch_lanes_table.cpp's output, from the restatement."""
    import dgen_batch_cases as K
    out = []
    lens = [1, 2, K.MIB, K.MIB + 1, 5 * K.MIB]
    for cls in K.RAGGED:
        C = 4096 << cls
        lens += [C // 2, C // 2 + 1, C - 1, C, C + 1]
    for ln in lens:
        out.append(f"class {ln} {K.chunk_class(ln)} {K.class_ceiling(K.chunk_class(ln))}")
    knobs = (0, 512, 4096, 131072)
    for cls in range(K.FULL + 1):
        for knob in knobs:
            for zeros in (0, 1):
                for draws in (16, 32, 64):
                    for verify in (0, 1):
                        for nchunks in (1, 67, 20000):
                            for cus in (1, 256, 304):
                                lpc, span = K.class_lanes(K.class_ceiling(cls), nchunks, cus, knob, bool(zeros), draws,
                                                          bool(verify))
                                out.append(f"lanes {cls} {knob} {zeros} {draws} {verify} {nchunks} {cus} {lpc} {span}")
    for cls in range(K.FULL + 1):
        C = K.class_ceiling(cls)
        lo = 0 if cls in (0, K.FULL) else C // 2
        for knob in knobs:
            for verify in (False, True):
                lpc, span = K.class_lanes(C, 67, 256, knob, False, 16, verify)
                for ln in (lo + 1, lo + 17, (lo + C) // 2 + 5, C - 1, C):
                    if cls == K.FULL and ln != C:
                        continue
                    for sub in range(lpc):
                        rb, rlen = K.lane_region(ln, span, sub)
                        out.append(f"region {ln} {span} {sub} {rb} {rlen}")
    return out


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_restatement_equals_the_header(tmp_path, sanitize):
    """tests/dgen_batch_cases.py restates the size classes, the lane plan (fill
    and verify, knob set and unset, with and without zero prefixes, every stage
    width) and the lane regions; tests/capi/dgen_batch_lanes_table.cpp prints
    the header's.  Every line is equal."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "table")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-I", os.path.dirname(HEADER), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "dgen_batch_lanes_table.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got, want = out.stdout.splitlines(), _table_lines()
    assert len(want) > 4320 and len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


def test_restated_ratio_is_the_library_s():
    import dgen_batch_cases as K
    import s3dlio_amd as S
    for comp in (0, 1, 2, 3, 7, (3, 2), 1.5):
        assert K.ratio(comp) == S.compress_ratio(comp), comp


def test_knob_lanes():
    """At the three knobs the builders target, a class of ceiling C has
    max(1, C / 8 / knob) lanes per chunk: lanes of C, 32 KiB and 4 KiB."""
    import dgen_batch_cases as K
    for cls in range(K.FULL + 1):
        C = K.class_ceiling(cls)
        assert [K.knob_lanes(cls, k)[1] for k in K.KNOBS] == [C, min(C, 32768), 4096]
    assert K.list_knob(2048) == 512 and all(K.list_knob(k) == k for k in K.KNOBS)


def test_builders_hold_their_coverage():
    """Every builder at every class and knob: each asserts its own coverage from
    the restated plan and the byte budget of its list (64 MiB of object bytes).
    Together every ragged class and the full class are launched at every knob."""
    import dgen_batch_cases as K
    for knob in K.KNOBS:
        launched = set()
        for cls in K.RAGGED:
            lists = [K.class_lengths(cls, knob), K.shared_wave(cls, knob)]
            if cls >= 1:
                lists.append(K.prefix_ends(cls, knob))
            for objs, total in lists:
                assert K.object_bytes(objs) <= K.BUDGET and total >= max(o[0] + o[1] for o in objs)
                assert len({o[2] for o in objs}) == len(objs)
                count, _ = K.class_counts(objs)
                assert count[cls] and not any(count[c] for c in K.RAGGED if c != cls)
                launched |= {c for c in range(K.FULL + 1) if count[c]}
            n = K.wave_objects(cls, knob)
            assert len(K.shared_wave(cls, knob)[0]) == (n + 3 if K.knob_lanes(cls, knob)[0] < 64 else 5)
        assert launched == set(range(K.FULL + 1)), knob
    objs, total = K.all_classes()
    assert K.object_bytes(objs) <= K.BUDGET and all(K.class_counts(objs)[0])
    for zeros in (True, False):
        objs, total = K.many_tiny(20000, zeros)
        assert len(objs) == 20000 and total < 3 << 20 and K.object_bytes(objs) <= K.BUDGET
        assert {o[4] for o in objs} == ({1, 2} if zeros else {1})
        assert [len(K.many_tiny(n, zeros)[0]) for n in (6500, 3)] == [6500, 3]


def test_class_lengths_hold_every_delta():
    """No list dropped a delta to meet the budget: around the last boundary it
    kept, every b + delta inside the class is a tail of the list."""
    import dgen_batch_cases as K
    for knob in K.KNOBS:
        for cls in K.RAGGED:
            objs, _ = K.class_lengths(cls, knob)
            tails = {o[1] % K.MIB for o in objs}
            C, lo = K.class_ceiling(cls), (0 if cls == 0 else K.class_ceiling(cls) // 2)
            b = K.boundaries(cls, knob)[-1]
            assert {b + d for d in K.DELTAS if lo < b + d <= min(C, K.MIB - 1)} <= tails, (cls, knob)
            assert {lo + 1, C - 1, min(C, K.MIB - 1)} <= tails
