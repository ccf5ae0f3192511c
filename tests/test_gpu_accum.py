"""GPU: what the three accumulating handles share (csrc/s3dg_accum.h behind
Measure, LzMeasure and Chunker): reset, close and the independence of streams.

Each case runs for all three kinds on the same small shapes and compares a
handle with another handle of its kind that was fed the same bytes the plain
way; what the results must be is the business of test_gpu_measure.py,
test_gpu_lz.py and test_gpu_chunks.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZE, STRIDE, N = 4096 + 16, 8192, 2     # two objects, each a block and a ragged one
KINDS = ["measure", "lz", "chunks"]


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def make(ctx, kind):
    if kind == "measure":
        return ctx.measurer(4096, hist=True)
    if kind == "lz":
        return ctx.lz_measurer(4096)
    return ctx.chunker(32, 64, 256)


def payload(torch, seed, n=N):
    """n objects at STRIDE: bytes of four values, so every kind finds something."""
    a = np.random.default_rng(seed).integers(0, 4, n * STRIDE, dtype=np.uint8)
    return torch.from_numpy(a).to("cuda:0")


def fresh(ctx, kind, adds):
    with make(ctx, kind) as h:
        for t, n in adds:
            h.add_stream(t, SIZE, n, STRIDE)
        return h.result()


@pytest.mark.parametrize("kind", KINDS)
def test_reset(torch, gpu_ctx, kind):
    """After reset() a handle is a fresh one, whether or not the adds before it
    were waited for."""
    a, b = payload(torch, 1), payload(torch, 2)
    torch.cuda.synchronize()
    want_a, want_b = fresh(gpu_ctx, kind, [(a, N)]), fresh(gpu_ctx, kind, [(b, N)])
    assert want_a != want_b and want_b.bytes == N * SIZE
    st = torch.cuda.Stream()
    with make(gpu_ctx, kind) as h:
        h.add_stream(a, SIZE, N, STRIDE, stream=st)
        assert h.result() == want_a
        h.reset()
        h.add_stream(b, SIZE, N, STRIDE, stream=st)
        assert h.result() == want_b
        h.add_stream(a, SIZE, N, STRIDE, stream=st)
        h.reset()                                  # the add may still be running
        h.add_stream(b, SIZE, N, STRIDE)
        assert h.result() == want_b
    st.synchronize()


@pytest.mark.parametrize("kind", KINDS)
def test_close(torch, gpu_ctx, kind):
    """close() twice is harmless; every call on a closed handle is refused by
    name; the context goes on working."""
    t = payload(torch, 3)
    torch.cuda.synchronize()
    want = fresh(gpu_ctx, kind, [(t, N)])
    h = make(gpu_ctx, kind)
    h.add_stream(t, SIZE, N, STRIDE)
    assert h.result() == want
    h.close()
    h.close()
    calls = [lambda: h.add(t, SIZE), lambda: h.add_stream(t, SIZE, N, STRIDE), h.result, h.reset]
    if kind == "chunks":
        calls += [h.time_passes, h.gear_table, h.pass_seconds]
    else:
        calls.append(lambda: h.add_range(t, SIZE, 0, 1))
    for f in calls:
        with pytest.raises(ValueError, match=f"null {kind} handle"):
            f()
    h.close()
    assert fresh(gpu_ctx, kind, [(t, N)]) == want


@pytest.mark.parametrize("kind", KINDS)
def test_stream_scratch_grows_beside_a_pending_add(torch, gpu_ctx, kind):
    """Stream 1's second add needs more scratch (records) than its first while
    stream 2's add is still queued: the same result as on one stream."""
    big, small, more = payload(torch, 4, 64), payload(torch, 5, 1), payload(torch, 6)
    torch.cuda.synchronize()
    adds = [(big, 64), (small, 1), (more, N)]
    want = fresh(gpu_ctx, kind, adds)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with make(gpu_ctx, kind) as h:
        for (t, n), st in zip(adds, (s2, s1, s1)):
            h.add_stream(t, SIZE, n, STRIDE, stream=st)
        assert h.result() == want
    assert want.bytes == (64 + 1 + N) * SIZE
    s1.synchronize()
    s2.synchronize()
