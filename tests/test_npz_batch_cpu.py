"""CPU: NPZ archives framed and checked on the device (s3dg_npz_frame_batch,
s3dg_npz_check_batch) without a GPU: the plan
(csrc/s3dg_npz_plan.h, compiled with g++ alone, plain and under the address and
undefined-behaviour sanitizers) with every refusal and its message, the refusal
that needs no device, and the helpers of the Python surface against the oracle."""
import ctypes
import os
import shutil
import subprocess

import pytest

from oracle import npz_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGION = 32 * 1024


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_plan_sweep(tmp_path, sanitize):
    """tests/capi/npz_plan_sweep.cpp asserts the plan's properties itself: one
    writer per archive byte, the member CRC from the regions' raws, the 2^32
    limits, every refusal with its message."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "npz_plan_sweep.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = dict(line.split("|", 1) for line in out.stdout.splitlines())
    assert int(rows.pop("refusals")) == 20   # every refusal of the header's list, with its message
    assert int(rows.pop("archives")) == 3 * 12 * 16 and int(rows.pop("members")) == 6 * 12 * 16 and int(rows.pop("regions")) > 900


def test_headers_and_sizes_match_the_oracle():
    import s3dlio_amd as S
    for shape, dtype in (([3, 4], "<f4"), ([7], "<i8"), ([300, 211, 1], "<f4"), ([], "<f8"), ([0], "|u1")):
        assert S.npy_header(shape, dtype) == O.npy_header(shape, dtype)
    for n in (0, 8, 99999, 10**9):
        h = S.npy_header_u1(n)
        assert len(h) % 16 == 0 and h.endswith(b"\n") and f"(%d,)" % n in h.decode("latin1")
    for shape, samples in (([5, 3], 2), ([0], 1), ([64, 64], 3)):
        members = [("x.npy", S.npy_header(shape, "<f4"), 0, 4 * shape[0] * (shape[1] if len(shape) > 1 else 1)),
                   ("y.npy", S.npy_header([samples], "<i8"), None, 8 * samples)]
        assert S.npz_archive_size(members) == S.npz_size(shape, "<f4", samples)
    assert S.npz_archive_size([("data.npy", S.npy_header_u1(100), 0, 100)], S.NPZ_STYLE_LEGACY) == \
        len(bytes(S.build_npz(100, 1, bytes(100))))


def test_null_context_and_sizes():
    """A null context is refused before anything else is looked at, n == 0
    included; s3dg_npz_archive_size needs no context."""
    from s3dlio_amd import _lib
    arr, marr = (_lib.NpzArchive * 1)(_lib.NpzArchive(0, 0, 1, 0, 0)), (_lib.NpzMember * 1)(_lib.NpzMember(0, 5, 0, 1, 1, 4))
    blob, tot = ctypes.create_string_buffer(64), _lib.NpzRec(*([0xEEEE] * 7))
    for n in (1, 0):
        for sym, args in (("s3dg_npz_frame_batch", (None, 4096, 8192, arr, n, marr, 1, blob, 64, None)),
                          ("s3dg_npz_check_batch", (None, 8192, arr, n, marr, 1, blob, 64, None, ctypes.byref(tot), None))):
            with pytest.raises(ValueError) as e:
                _lib.call(sym, *args)
            assert str(e.value) == "null context"
    assert [getattr(tot, f) for f, _ in _lib.NpzRec._fields_] == [0xEEEE] * 7
    out = _lib.c_u64(7)
    _lib.call("s3dg_npz_archive_size", marr, 1, ctypes.byref(out))
    assert out.value == 30 + 1 + 4 + 5 + 46 + 1 + 22
    big = (_lib.NpzMember * 2)(_lib.NpzMember(0, 2**63, 0, 1, 1, 4), _lib.NpzMember(0, 2**63, 0, 1, 1, 4))
    with pytest.raises(ValueError) as e:
        _lib.call("s3dg_npz_archive_size", big, 2, ctypes.byref(out))
    assert str(e.value) == "the archive's size overflows"
    assert ctypes.sizeof(_lib.NpzMember) == 32 and ctypes.sizeof(_lib.NpzArchive) == 32 and ctypes.sizeof(_lib.NpzRec) == 56
