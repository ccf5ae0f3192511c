"""CPU: TFRecord shards of records of any length framed, checked and indexed on
the device (s3dg_tfrecord_frame_var_batch, s3dg_tfrecord_check_var_batch,
s3dg_tfrecord_index_batch) without a GPU: the judges of
tests/tfrecord_var_restatement.py held to the oracle, the plan
(csrc/s3dg_tfrecord_var_plan.h, compiled with g++ alone, plain and as a
stand-alone program under the address and undefined-behaviour sanitizers), the
walk's rule against its Python restatement, the refusal that needs no device
from a C program and from Python, and the Python surface."""
import ctypes
import inspect
import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

from oracle.format_oracle import build_tfrecord_with_index

import tfrecord_var_restatement as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "s3dlio_gpu.h")
KiB = 1024


def test_the_judge_is_the_oracle_on_equal_lengths():
    """Before it judges anything else: frame() over equal lengths is
    build_tfrecord_with_index, stream and index."""
    for n, rs in ((1, 0), (3, 1), (5, 1023), (4, 1024), (3, 2100), (2, 32 * KiB + 17), (7, 0)):
        payload = bytes((i * 89 + 3) & 0xFF for i in range(n * rs))
        assert J.frame(payload, [rs] * n) == build_tfrecord_with_index(n, rs, payload), (n, rs)
    st, ix = J.frame(b"abcdefgh", [3, 0, 5])
    w = J.walk(st)
    assert w["records"] == 3 and w["status"] == 0 and w["trailing"] == 0 and w["bad_length_crc"] == 0
    assert np.frombuffer(ix, "<u8").reshape(-1, 2).tolist() == [list(e) for e in w["entries"]] == [[0, 19], [19, 16], [35, 21]]


def _build_sweep(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    # no ROCm include path: the plan header needs the public header and its own neighbours only
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-I", os.path.dirname(HEADER), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "tfrecord_var_plan_sweep.cpp")])
    return exe


def _named_lists():
    edges = [1024 * k + d for k in (1, 2) for d in (0, 1, 15, 16, 17, -1, -15, -16, -17)]
    return {"ramp": list(range(41)), "edges": edges, "mixed": [100, 3 * 32 * KiB + 1023] * 3,
            "zeros": [0, 0, 5, 0, 0, 0, 17, 0]}


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_sweep(tmp_path, sanitize):
    """tests/capi/tfrecord_var_plan_sweep.cpp asserts the plan's properties
    itself: one writer per stream byte, one reader per source byte, every
    wave's run covering each region once, the per-record fold against a
    bit-by-bit CRC at every alignment, the constants from the power table, the
    refusals.  The values it prints are CRC-32s of streams it framed through
    the plan from payloads this test rebuilds: they are the judge's streams'."""
    exe = _build_sweep(tmp_path, sanitize)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = dict(line.split("|", 1) for line in out.stdout.splitlines())
    assert int(rows.pop("lists")) > 80 and int(rows.pop("records")) > 7000 and int(rows.pop("regions")) > 9000
    named = _named_lists()
    assert set(rows) == {f"stream_{k}" for k in named}
    payload = bytes((i * 131 + 7) & 0xFF for i in range(400 * KiB))
    for name, lengths in named.items():
        stream, _ = J.frame(payload[:sum(lengths)], lengths)
        assert int(rows[f"stream_{name}"], 16) == zlib.crc32(stream), name


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_walk_rule_against_the_restatement(tmp_path, sanitize):
    """tfv_walk_host, the kernel's loop on the host, over the list of endings:
    empty streams, trailing 0-15 bytes, a truncated last record at every
    missing-byte count 1-20, length fields 2^32, 2^63 and 2^64 - 1,
    max_records of 0, exact and one short; and a flipped length-CRC byte,
    which is counted while the entries stay the reference's."""
    exe = _build_sweep(tmp_path, sanitize)
    cases = J.walk_endings()
    good, _ = J.frame(bytes(range(47)), [40, 0, 7])
    flipped = bytearray(good)
    flipped[56 + 9] ^= 0x10                      # record 1's length CRC
    cases.append(("flipped_length_crc", bytes(flipped), J.NONE))
    assert len({c[0] for c in cases}) == len(cases) == 45
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{name} {data.hex() or '-'} {cap}\n" for name, data, cap in cases))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = dict(line.split("|", 1) for line in out.stdout.splitlines())
    assert set(rows) == {f"walk_{c[0]}" for c in cases}
    seen = set()
    for name, data, cap in cases:
        w = J.walk(data, cap)
        c = 0
        for o, s in w["entries"]:
            c = (c * 31 + o % 1000003) & 0xFFFFFFFF
            c = (c * 31 + s % 1000003) & 0xFFFFFFFF
        first = -1 if w["first_bad_record"] is None else w["first_bad_record"]
        want = f'{w["records"]},{w["status"]},{w["stop_offset"]},{w["trailing"]},{w["bad_length_crc"]},{first},{c}'
        assert rows[f"walk_{name}"] == want, name
        seen.add(w["status"])
    assert seen == {0, 1, 2}
    # the restatement's own endings, spelled out once
    w = J.walk(good[:-5])
    assert (w["records"], w["status"], w["stop_offset"], w["trailing"]) == (2, 1, 72, 18)
    w = J.walk(good[:-12])
    assert (w["records"], w["status"], w["stop_offset"], w["trailing"]) == (2, 0, 72, 11)
    w = J.walk(good, 2)
    assert (w["records"], w["status"], w["stop_offset"], w["trailing"]) == (2, 2, 72, 23)
    assert J.walk(good, 3)["status"] == 0 and J.walk(good, 0)["status"] == 2 and J.walk(good[:11], 0)["status"] == 0
    w = J.walk(bytes(flipped))
    assert w["bad_length_crc"] == 1 and w["first_bad_record"] == 1 and w["entries"] == J.walk(good)["entries"]
    assert J.index_text(w["entries"]) == "0 56\n56 16\n72 23\n"


def test_c_program_sees_the_null_context_and_the_size(tmp_path):
    """A null context is S3DG_EINVAL "null context" for the three calls, before
    the descriptors or the outputs are looked at, n == 0 included;
    s3dg_tfrecord_var_size needs no context and refuses the overflow."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    from s3dlio_amd._lib import LIB_PATH
    src = tmp_path / "tfv.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "s3dlio_gpu.h"
#define MSG(text) (strcmp(s3dg_last_error(), text) == 0)
int main(void) {
    static uint8_t buf[1024] __attribute__((aligned(16)));
    const uint64_t lens[3] = {100, 0, 5};
    const s3dg_tfrecord_var_shard sh[2] = {{0, 512, 0, 2, 0}, {256, 768, 32, 1, 2}};
    const s3dg_tfrecord_stream st[1] = {{3, 100, 16, 4}};
    s3dg_tfrecord_result tot, per[2];
    s3dg_tfrecord_walk_result wr[1];
    uint64_t size = 7;
    memset(buf, 0xEE, sizeof buf);
    memset(&tot, 0xEE, sizeof tot);
    memset(per, 0xEE, sizeof per);
    memset(wr, 0xEE, sizeof wr);
    if (s3dg_tfrecord_frame_var_batch(NULL, buf, buf, buf, sh, 2, lens, 3, NULL) != S3DG_EINVAL || !MSG("null context")) return 1;
    if (s3dg_tfrecord_check_var_batch(NULL, buf, sh, 2, lens, 3, NULL, &tot, per) != S3DG_EINVAL || !MSG("null context")) return 2;
    if (s3dg_tfrecord_index_batch(NULL, buf, buf, st, 1, NULL, wr) != S3DG_EINVAL || !MSG("null context")) return 3;
    if (s3dg_tfrecord_frame_var_batch(NULL, NULL, NULL, NULL, NULL, 0, NULL, 0, NULL) != S3DG_EINVAL || !MSG("null context")) return 4;
    if (s3dg_tfrecord_check_var_batch(NULL, NULL, NULL, 0, NULL, 0, NULL, NULL, NULL) != S3DG_EINVAL || !MSG("null context")) return 5;
    if (s3dg_tfrecord_index_batch(NULL, NULL, NULL, NULL, 0, NULL, NULL) != S3DG_EINVAL || !MSG("null context")) return 6;
    for (size_t i = 0; i < sizeof buf; ++i) if (buf[i] != 0xEE) return 7;
    for (size_t i = 0; i < sizeof tot; ++i) if (((uint8_t *)&tot)[i] != 0xEE) return 8;
    for (size_t i = 0; i < sizeof per; ++i) if (((uint8_t *)per)[i] != 0xEE) return 9;
    for (size_t i = 0; i < sizeof wr; ++i) if (((uint8_t *)wr)[i] != 0xEE) return 10;
    if (s3dg_tfrecord_var_size(lens, 3, &size) != S3DG_OK || size != 48 + 105) return 11;
    if (s3dg_tfrecord_var_size(NULL, 0, &size) != S3DG_OK || size != 0) return 12;
    size = 7;
    {
        const uint64_t huge[2] = {UINT64_MAX - 40, 9};
        if (s3dg_tfrecord_var_size(huge, 2, &size) != S3DG_EINVAL || !MSG("sum(16 + length) overflows") || size != 7) return 13;
    }
    if (s3dg_tfrecord_var_size(NULL, 2, &size) != S3DG_EINVAL || !MSG("null lengths array")) return 14;
    if (s3dg_tfrecord_var_size(lens, 3, NULL) != S3DG_EINVAL || !MSG("null output")) return 15;
    if (sizeof(s3dg_tfrecord_var_shard) != 40 || sizeof(s3dg_tfrecord_stream) != 32 || sizeof(s3dg_tfrecord_walk_result) != 48) return 16;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "tfv"
    libdir = os.path.dirname(LIB_PATH)
    subprocess.check_call([gcc, "-std=gnu99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                           "-L", libdir, "-ls3dlio_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out


def test_python_sees_the_null_context():
    from s3dlio_amd import _lib
    sh = (_lib.TfrVarShard * 2)(_lib.TfrVarShard(0, 512, 0, 2, 0), _lib.TfrVarShard(256, 768, 32, 1, 2))
    lens = (_lib.c_u64 * 3)(100, 0, 5)
    st = (_lib.TfrStream * 1)(_lib.TfrStream(3, 100, 16, 4))
    tot = _lib.TfrRec(*([0xEEEE] * 7))
    wr = (_lib.TfrWalkRec * 1)(_lib.TfrWalkRec(*([0xEEEE] * 6)))
    for n in (2, 0):
        with pytest.raises(ValueError) as e:
            _lib.call("s3dg_tfrecord_frame_var_batch", None, 4096, 8192, None, sh, n, lens, 3, None)
        assert str(e.value) == "null context"
        with pytest.raises(ValueError) as e:
            _lib.call("s3dg_tfrecord_check_var_batch", None, 4096, sh, n, lens, 3, None, ctypes.byref(tot), None)
        assert str(e.value) == "null context"
        with pytest.raises(ValueError) as e:
            _lib.call("s3dg_tfrecord_index_batch", None, 4096, 8192, st, min(n, 1), None, wr)
        assert str(e.value) == "null context"
    assert [getattr(tot, f) for f, _ in _lib.TfrRec._fields_] == [0xEEEE] * 7
    assert [getattr(wr[0], f) for f, _ in _lib.TfrWalkRec._fields_] == [0xEEEE] * 6


def test_surface_exists():
    import s3dlio_amd as S
    from s3dlio_amd import _lib
    p = inspect.signature(S.Context.tfrecord_frame_var_batch).parameters
    assert list(p) == ["self", "src", "dst", "shards", "index", "stream"]
    assert p["index"].default is None and p["stream"].default is None
    p = inspect.signature(S.Context.tfrecord_check_var_batch).parameters
    assert list(p) == ["self", "src", "shards", "stream", "per_shard"]
    assert p["stream"].default is None and p["per_shard"].default is True
    p = inspect.signature(S.Context.tfrecord_index_batch).parameters
    assert list(p) == ["self", "src", "streams", "index", "stream"] and p["stream"].default is None
    p = inspect.signature(S.Context.tfrecord_scan).parameters
    assert list(p) == ["self", "src", "streams", "stream"] and p["stream"].default is None
    assert list(inspect.signature(S.tfrecord_var_size).parameters) == ["lengths"]
    assert list(inspect.signature(S.tfrecord_index_text).parameters) == ["entries"]
    for sym in ("s3dg_tfrecord_var_size", "s3dg_tfrecord_frame_var_batch", "s3dg_tfrecord_check_var_batch",
                "s3dg_tfrecord_index_batch"):
        assert hasattr(S.lib, sym)   # exported
        assert _lib.SIGNATURES[sym][0] is _lib.c_int
    assert ctypes.sizeof(_lib.TfrVarShard) == 40 and ctypes.sizeof(_lib.TfrStream) == 32 and ctypes.sizeof(_lib.TfrWalkRec) == 48
    assert [f for f, _ in _lib.TfrVarShard._fields_] == ["src_off", "dst_off", "idx_off", "records", "len0"]
    assert [f for f, _ in _lib.TfrStream._fields_] == ["off", "bytes", "idx_off", "max_records"]
    assert [f for f, _ in _lib.TfrWalkRec._fields_] == ["records", "status", "stop_offset", "trailing", "bad_length_crc",
                                                       "first_bad_record"]
    args = _lib.SIGNATURES["s3dg_tfrecord_frame_var_batch"][1]
    assert len(args) == 9 and args[4]._type_ is _lib.TfrVarShard and args[6]._type_ is _lib.c_u64 and args[7] is _lib.c_u64
    args = _lib.SIGNATURES["s3dg_tfrecord_check_var_batch"][1]
    assert len(args) == 9 and args[2]._type_ is _lib.TfrVarShard and args[7]._type_ is _lib.TfrRec
    args = _lib.SIGNATURES["s3dg_tfrecord_index_batch"][1]
    assert len(args) == 7 and args[3]._type_ is _lib.TfrStream and args[6]._type_ is _lib.TfrWalkRec
    # the size: any integer sequence or numpy array; the overflow is refused
    assert S.tfrecord_var_size([100, 0, 5]) == 48 + 105 and S.tfrecord_var_size([]) == 0
    assert S.tfrecord_var_size(np.array([7, 9], np.int32)) == 48 and S.tfrecord_var_size(range(4)) == 64 + 6
    assert S.tfrecord_var_size([150 * KiB] * 1000) == S.tfrecord_size(1000, 150 * KiB)
    with pytest.raises(ValueError) as e:
        S.tfrecord_var_size([2**64 - 41, 9])
    assert str(e.value) == "sum(16 + length) overflows"
    for bad in ([-1], [2**64], [1.5]):
        with pytest.raises(ValueError):
            S.tfrecord_var_size(bad)
    # the walk's result and the DALI text
    w = S.TfRecordWalk()
    assert w.ok and w.status == "complete" and w.first_bad_record is None and w.records == 0
    assert not S.TfRecordWalk(records=2, status="truncated", stop_offset=72, trailing=18).ok
    assert not S.TfRecordWalk(records=2, status="full").ok
    assert not S.TfRecordWalk(records=3, bad_length_crc=1, first_bad_record=1).ok
    r = _lib.TfrWalkRec(3, 2, 95, 12, 1, 2)
    assert S.TfRecordWalk._of(r) == S.TfRecordWalk(3, "full", 95, 12, 1, 2)
    assert S.TfRecordWalk._of(_lib.TfrWalkRec(0, 1, 0, 5, 0, 2**64 - 1)) == S.TfRecordWalk(0, "truncated", 0, 5, 0, None)
    entries = [(0, 56), (56, 16), (72, 23)]
    assert S.tfrecord_index_text(entries) == S.tfrecord_index_text(np.array(entries, np.uint64)) == J.index_text(entries)
    assert S.tfrecord_index_text([]) == "" and S.tfrecord_index_text([(2**63, 2**64 - 1)]) == f"{2**63} {2**64 - 1}\n"
