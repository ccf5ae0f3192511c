"""CPU: the host-side surface of payload verification (the read-side twins of
the fill calls).  No kernel runs here: argument checks, the empty-buffer
result, and the C entry point as a plain C program sees it."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "s3dlio_gpu.h")


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


def test_empty_buffer_is_clean(S):
    for buf in (b"", bytearray(0), np.zeros(0, np.uint8)):
        r = S.verify_controlled_data_seeded(buf, 2, 3, entropy=7)
        assert r.ok and r.first_offset is None
        assert (r.mismatched_bytes, r.mismatched_blocks) == (0, 0)
    assert S.VerifyResult().ok and not S.VerifyResult(1, 1, 0).ok


def test_read_only_buffer_is_accepted(S):
    """bytes passes the argument checks; what fails without a GPU is the GPU."""
    import torch
    if torch.cuda.is_available():
        assert isinstance(S.verify_controlled_data_seeded(b"\x00" * 4096, 1, 1), S.VerifyResult)
        return
    with pytest.raises(RuntimeError) as ei:
        S.verify_controlled_data_seeded(b"\x00" * 4096, 1, 1)
    assert not isinstance(ei.value, ValueError)


def test_non_contiguous_buffer_is_refused(S):
    a = np.zeros((8, 8), np.uint8)[:, ::2]
    with pytest.raises(ValueError, match="contiguous"):
        S.verify_controlled_data_seeded(a, 1, 1)


def test_wrong_base_block_size_is_refused(S):
    with pytest.raises(ValueError, match="4096"):
        S.verify_controlled_data_seeded(bytearray(4096), 1, 1, base_block=b"\x01" * 100)
    with pytest.raises(ValueError, match="4096"):   # checked even when there is nothing to verify
        S.verify_controlled_data_seeded(b"", 1, 1, base_block=b"\x01" * 100)


def test_verify_objects_refusals(S, tmp_path):
    uri = f"file://{tmp_path}/o"
    with pytest.raises(ValueError, match="dgen"):
        S.verify_objects([uri], 100, payload="dgen")
    # put_objects' default payload for a controlled config is DG1: refused the same way
    with pytest.raises(ValueError, match="dgen"):
        S.verify_objects([uri], 100, config=S.Config.new_with_defaults("RAW", 1, 100, 2, 2))
    with pytest.raises(ValueError, match="RAW"):
        S.verify_objects([uri], 100, config=S.Config.new_with_defaults("NPZ", 1, 100, 1, 1), payload="controlled")
    with pytest.raises(ValueError, match="file://"):
        S.verify_objects(["s3://bkt/o"], 100, payload="controlled")


def test_c_program_sees_the_host_entry_point(tmp_path):
    """Built as test_header_is_plain_c_and_links builds its program: an empty
    buffer is clean without a GPU, a null result pointer is S3DG_EINVAL with a
    message."""
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("gcc not available")
    from s3dlio_amd._lib import LIB_PATH
    src = tmp_path / "v.c"
    src.write_text(r'''
#include <stdio.h>
#include <string.h>
#include "s3dlio_gpu.h"
int main(void) {
    uint8_t buf[16] = {0};
    s3dg_verify_result r;
    memset(&r, 0x5A, sizeof r);
    if (sizeof r != 24) return 1;
    int rc = s3dlio_verify_controlled_data_seeded(buf, 0, 1, 1, 0, NULL, &r);
    if (rc != 0) return 2;
    if (r.mismatched_bytes != 0 || r.mismatched_blocks != 0 || r.first_offset != UINT64_MAX) return 3;
    rc = s3dlio_verify_controlled_data_seeded(buf, 0, 1, 1, 0, NULL, NULL);
    if (rc != S3DG_EINVAL) return 4;
    if (!s3dg_last_error()[0]) return 5;
    rc = s3dlio_verify_controlled_data_seeded(buf, 16, 1, 1, 0, NULL, NULL);
    if (rc != S3DG_EINVAL) return 6;
    printf("ok\n");
    return 0;
}
''')
    exe = tmp_path / "v"
    libdir = os.path.dirname(LIB_PATH)
    subprocess.check_call([gcc, "-std=c99", "-Wall", "-Werror", "-I", os.path.dirname(HEADER), str(src),
                           "-L", libdir, "-ls3dlio_amd", f"-Wl,-rpath,{libdir}", "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out
