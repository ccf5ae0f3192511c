"""GPU: the batch fill's records at every lead, tile edge and map path: the
lists of tests/batch_record_cases.py (each proved on the CPU to reach the plan
it names, tests/test_batch_records_cpu.py) through Context.fill_batch.

One helper runs every list: the arena lies between a poisoned front guard and
a poisoned back guard of 64 KiB each, dst_base is `shift` bytes past a 32 KiB
boundary (so base itself contributes to every lead), and the WHOLE buffer,
guards and gaps included, is compared with a host image that holds the C
oracle's fill_controlled bytes of every object and poison everywhere else.
Every byte is exact; there is no tolerance.  verify_batch over the result must
be clean."""
import numpy as np
import pytest

import batch_record_cases as K
from oracle import oracle_py as P

pytestmark = pytest.mark.gpu

POISON = 0xAB
GUARD = 64 * K.KiB
ALIGN = 32 * K.KiB                       # leads are granules mod 8: 32 KiB
KEEP = 48 * K.MiB                        # host images of smaller arenas are kept for the reruns


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def base(golden_base):
    return np.frombuffer(golden_base, np.uint8)


@pytest.fixture(scope="module")
def wave_ctx(S, gpu_ctx):
    """One context per waves-per-block setting (the shared context stays as it is)."""
    ctxs = {w: S.Context(0, base_seed=S.DEFAULT_BASE_SEED, waves_per_block=w) for w in (1, 2, 4)}
    yield ctxs
    for c in ctxs.values():
        c.close()


@pytest.fixture(scope="module")
def arena_image(oracle, base):
    """The arena of a case as the fill must leave it: the oracle's bytes of
    every object in a field of poison.  Computed once per case and read-only."""
    kept = {}

    def image(case):
        if case.name in kept:
            return kept[case.name]
        a = np.full(case.end, POISON, np.uint8)
        for off, size, e, d, c in case.objs:
            if size:
                fn, fd = P.compress_ratio(c)
                a[off:off + size] = oracle.fill_controlled(size, d, fn, fd, e, base)
        a.setflags(write=False)
        if case.end <= KEEP:
            kept[case.name] = a
        return a
    return image


class Run:
    """A poisoned buffer around a case's arena, dst_base `shift` past a 32 KiB boundary."""

    def __init__(self, torch, case):
        self.case = case
        total = GUARD + ALIGN + case.shift + case.end + GUARD
        self.buf = torch.full((total,), POISON, dtype=torch.uint8, device="cuda:0")
        self.at = GUARD + (-(self.buf.data_ptr() + GUARD)) % ALIGN + case.shift
        assert case.shift % 16 == 0 and (self.buf.data_ptr() + self.at - case.shift) % ALIGN == 0
        self.dst = self.buf[self.at:]

    def fill(self, ctx, stream=None):
        c = self.case
        ctx.set_batch_tile(c.tile)
        ctx.set_batch_split(c.split)
        try:
            ctx.fill_batch(self.dst, c.objs, stream=stream)
        finally:
            ctx.set_batch_tile(0)
            ctx.set_batch_split(-1)

    def check(self, torch, arena_image):
        img = np.full(self.buf.numel(), POISON, np.uint8)
        img[self.at:self.at + self.case.end] = arena_image(self.case)
        want = torch.from_numpy(img).to("cuda:0")
        if not torch.equal(self.buf, want):
            bad = torch.nonzero(self.buf != want).flatten()
            first = int(bad[0]) - self.at
            raise AssertionError(f"{self.case.name}: {bad.numel()} bytes differ, the first at arena offset {first} "
                                 f"(front guard below 0, back guard from {self.case.end})")


def run_case(ctx, torch, arena_image, case, stream=None):
    r = Run(torch, case)
    r.fill(ctx, stream)
    torch.cuda.synchronize()
    r.check(torch, arena_image)
    return r


def lead7_object(case):
    """Index of the first non-empty object whose lead is 7."""
    return next(k for k, o in enumerate(case.objs) if o[1] and K.lead_of(case.shift, o[0]) == 7)


@pytest.mark.parametrize("name", [c.name for c in K.CASES])
def test_list_vs_oracle(gpu_ctx, torch, arena_image, name):
    """Every list under its knobs: the whole buffer against the host image,
    then verify_batch clean; in the leads lists one flipped byte in the last
    block of the object at lead 7 is named with its object index."""
    case = K.BY_NAME[name]
    r = run_case(gpu_ctx, torch, arena_image, case)
    gpu_ctx.set_batch_tile(case.tile if case.tile != 1 else 0)     # the verify has no dense layout
    try:
        res = gpu_ctx.verify_batch(r.dst, case.objs)
        assert res.ok and res.mismatches == () and res.objects == len(case.objs)
        if name in K.GROUPS["leads"]:
            k = lead7_object(case)
            off, size = case.objs[k][:2]
            r.dst[off + size - 1] ^= 0xFF
            res = gpu_ctx.verify_batch(r.dst, case.objs)
            assert res.total.mismatched_bytes == 1 and res.total.first_offset == off + size - 1
            assert [(j, v.mismatched_bytes, v.mismatched_blocks, v.first_offset) for j, v in res.mismatches] == \
                [(k, 1, 1, size - 1)]
    finally:
        gpu_ctx.set_batch_tile(0)


@pytest.mark.parametrize("name", K.GROUPS["leads"] + K.GROUPS["map_paths"])
def test_waves_and_prefetch(wave_ctx, torch, arena_image, name):
    """The leads and map_paths lists at 1, 2 and 4 waves per block, record
    prefetch off and 4 spans ahead (one_record_t64: the clamp to ntiles - 1)."""
    case = K.BY_NAME[name]
    for w, ctx in wave_ctx.items():
        for pf in (0, 4):
            ctx.set_batch_prefetch(pf)
            try:
                run_case(ctx, torch, arena_image, case)
            finally:
                ctx.set_batch_prefetch(-1)


def test_back_to_back_on_a_side_stream(gpu_ctx, torch, arena_image):
    """Two calls on one side stream without a sync between them, the larger
    first (two sub-batches, 16 385 descriptors), then a small one: the staging
    ring and the record maps are reused while the first fill may still run."""
    s = torch.cuda.Stream()
    big, small = Run(torch, K.BY_NAME["cuts_n16385"]), Run(torch, K.BY_NAME["leads_t2_shift"])
    s.wait_stream(torch.cuda.current_stream())
    big.fill(gpu_ctx, s)
    small.fill(gpu_ctx, s)
    torch.cuda.synchronize()
    big.check(torch, arena_image)
    small.check(torch, arena_image)
