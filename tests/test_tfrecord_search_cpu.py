"""CPU: s3dg_tfrecord_index_search_batch without a GPU: the
plan (csrc/s3dg_tfrecord_search_plan.h, compiled with g++ alone, plain and as a
stand-alone program under the address and undefined-behaviour sanitizers), the
search on the host over the list of endings against the Python restatement of
the walk, and the surface."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

import tfrecord_var_restatement as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[False, True], ids=["plain", "asan-ubsan"])
def sweep(request, tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no C++ compiler available")
    exe = str(tmp_path_factory.mktemp("tfs") / "sweep")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *extra,
                           "-I", os.path.join(ROOT, "s3dlio_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "capi", "tfrecord_search_plan_sweep.cpp")])
    return exe


def test_plan_sweep(sweep):
    """tests/capi/tfrecord_search_plan_sweep.cpp holds the search on the host to
    tfv_walk_host itself, call by call; here, that it ran what it says."""
    out = subprocess.run([sweep], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = {k: int(v) for k, v in (line.split("|") for line in out.stdout.splitlines())}
    assert rows["calls"] > 50 and rows["streams"] > 250 and rows["records"] > 50000 and rows["raw_steps"] > 500
    assert rows["nodes"] > rows["records"] - rows["raw_steps"]      # decoys and records behind max_records


def test_search_rule_against_the_restatement(sweep, tmp_path):
    """The search on the host over walk_endings(), each stream at a byte offset
    and flush against a copy of itself: the restatement's result and entries."""
    cases = J.walk_endings()
    path = tmp_path / "cases.txt"
    path.write_text("".join(f"{name} {data.hex() or '-'} {cap}\n" for name, data, cap in cases))
    out = subprocess.run([sweep, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    rows = dict(line.split("|", 1) for line in out.stdout.splitlines())
    assert set(rows) == {f"search_{c[0]}" for c in cases}
    for name, data, cap in cases:
        w = J.walk(data, cap)
        c = 0
        for o, s in w["entries"]:
            c = (c * 31 + o % 1000003) & 0xFFFFFFFF
            c = (c * 31 + s % 1000003) & 0xFFFFFFFF
        first = -1 if w["first_bad_record"] is None else w["first_bad_record"]
        assert rows[f"search_{name}"] == f'{w["records"]},{w["status"]},{w["stop_offset"]},{w["trailing"]},{w["bad_length_crc"]},{first},{c}', name


def test_surface_exists():
    import s3dlio_amd as S
    from s3dlio_amd import _lib
    sibling = inspect.signature(S.Context.tfrecord_index_batch)
    assert inspect.signature(S.Context.tfrecord_index_search_batch) == sibling
    assert inspect.signature(S.Context.tfrecord_scan).parameters.keys() == {"self", "src", "streams", "stream"}
    args = _lib.SIGNATURES["s3dg_tfrecord_index_search_batch"]
    assert args[0] is _lib.c_int and args[1] == _lib.SIGNATURES["s3dg_tfrecord_index_batch"][1]
    assert _lib.SIGNATURES["s3dg_tfrecord_index_search_timed"][1][:7] == args[1]
    for sym in ("s3dg_tfrecord_index_search_batch", "s3dg_tfrecord_index_search_timed", "s3dg_tfrecord_search_geometry"):
        assert hasattr(S.lib, sym)
    T, H = S.tfrecord_search_geometry()
    assert T >= 4096 and T & (T - 1) == 0 and H >= 2 and H & (H - 1) == 0
    with pytest.raises(ValueError) as e:
        _lib.call("s3dg_tfrecord_search_geometry", None, None)
    assert str(e.value) == "null output"
    # what needs no device is refused as the sibling refuses it, n == 0 included
    st = (_lib.TfrStream * 1)(_lib.TfrStream(3, 100, 16, 4))
    wr = (_lib.TfrWalkRec * 1)(_lib.TfrWalkRec(*([0xEEEE] * 6)))
    for n in (1, 0):
        msgs = []
        for sym in ("s3dg_tfrecord_index_batch", "s3dg_tfrecord_index_search_batch"):
            with pytest.raises(ValueError) as e:
                _lib.call(sym, None, 4096, 8192, st, n, None, wr)
            msgs.append(str(e.value))
        assert msgs == ["null context"] * 2
    assert [getattr(wr[0], f) for f, _ in _lib.TfrWalkRec._fields_] == [0xEEEE] * 6
    assert _lib.SIGNATURES["s3dg_tfrecord_index_search_timed"][1][7]._type_ is ctypes.c_float
