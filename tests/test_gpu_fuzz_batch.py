"""GPU: the batch loop under seeded fuzz: fill, verify, measure and checksum
of one random descriptor list per seed (tests/batch_fuzz_cases.py draws it;
tests/test_batch_fuzz_cpu.py holds the draws to their checklist).

Per seed: Context.fill_batch and dgen_fill_batch write their objects into a
poisoned arena that already holds uploaded host payloads, and the whole arena,
gaps and guards included, must equal the C oracle's image.  verify_batch and
verify_dgen_batch over lists in any order, with repeats and sometimes one
descriptor with a wrong field, must give numpy's totals and per-object
records (`expected_verify`) on the clean arena and again after the drawn
corruption.  crc32_batch over the read list must give zlib.crc32 of the host
slices, and Measure, LzMeasure and Chunker must give their restatements and
the result of one add per span (tests/test_gpu_measure_batch.py's `check`).
Uniform seeds hold the stream calls against the batch calls as well.

Every value is exact.  A failure prints the case and names the call and the
first offending object, found by running that call one object at a time.
"""
import os
import zlib

import numpy as np
import pytest

import batch_fuzz_cases as C
import test_gpu_measure_batch as MB

pytestmark = pytest.mark.gpu
SOAK = max(1, int(os.environ.get("S3DG_FUZZ_SOAK", "1")))   # soak runs: seeds x SOAK


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


class Loop:
    """One case on the device."""

    def __init__(self, S, torch, ctx, oracle, base, case):
        self.S, self.torch, self.ctx, self.oracle, self.base, self.case = S, torch, ctx, oracle, base, case
        self.calls = {"controlled": (ctx.fill_batch, ctx.verify_batch, ctx.fill_stream, ctx.verify_stream),
                      "dg1": (ctx.dgen_fill_batch, ctx.verify_dgen_batch, ctx.dgen_fill_stream, ctx.verify_dgen_stream)}

    def fail(self, call, text):
        raise AssertionError(f"{call}: {text}\n{self.case.describe()}")

    def dev(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")

    def same_bytes(self, call, t, want):
        self.torch.cuda.synchronize()
        got = t.cpu().numpy()
        if not np.array_equal(got, want):
            bad = np.flatnonzero(got != want)
            p = int(bad[0])
            owner = [k for k, o in enumerate(self.case.writes) if o.off <= p < o.off + o.size]
            where = f"object {owner[0]} + {p - self.case.writes[owner[0]].off}" if owner else "a gap or guard byte"
            self.fail(call, f"{bad.size} bytes differ, first at {p} ({where}): got {got[p]:#04x}, want {want[p]:#04x}")
        return got

    # ---- steps 1 to 3 --------------------------------------------------------------------

    def fill(self):
        c = self.case
        t = self.dev(C.upload_image(c))
        for kind in C.GENERATED:
            self.calls[kind][0](t, [o.desc for o in c.of_kind(kind)])
        want = C.expected_image(c, self.oracle, self.base)
        self.same_bytes("fill_batch + dgen_fill_batch", t, want)
        return t, want

    def result(self, tot, per, n, per_object=True):
        V = self.S.VerifyResult
        return self.S.BatchVerifyResult(V(*tot), n, tuple((k, V(*r)) for k, r in sorted(per.items()))
                                        if per_object else None)

    def verify(self, t, image, state):
        for kind in C.GENERATED:
            call = self.calls[kind][1]
            descs = self.case.verify[kind]
            tot, per = C.expected_verify(image, self.case, kind, self.oracle, self.base)
            got = call(t, descs)
            if got != self.result(tot, per, len(descs)):
                for k, d in enumerate(descs):           # one by one: a miss names its descriptor
                    one = C.expected_verify(image, self.case, kind, self.oracle, self.base, descs=[d])
                    r = call(t, [d])
                    if r != self.result(*one, 1):
                        self.fail(f"{call.__name__} ({state})", f"descriptor {k} {d} alone gives {r}, want {one}")
                self.fail(f"{call.__name__} ({state})", f"every descriptor alone is right; the list gives {got}, want "
                                                        f"{tot} {per}")
            totals = call(t, descs, per_object=False)
            if totals != self.result(tot, per, len(descs), per_object=False):
                self.fail(f"{call.__name__} (per_object=False, {state})", f"{totals}, want {tot}")

    # ---- steps 5 and 6 -------------------------------------------------------------------

    def crc(self, t, host):
        c, torch = self.case, self.torch
        want = np.array([zlib.crc32(host[o:o + n].tobytes()) if n else 0 for o, n in c.reads], np.uint32)
        if c.seed % 2 == 0:
            got = self.ctx.crc32_batch(t, c.reads)
        else:
            out = torch.full((len(c.reads),), 0x6B6B6B6B, dtype=torch.int32, device="cuda:0")
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            try:
                assert self.ctx.crc32_batch(t, c.reads, stream=st, out=out) is None
                st.synchronize()
            finally:
                self.ctx.release_stream(st)
            got = out.cpu().numpy().view(np.uint32)
        if not np.array_equal(got, want):
            k = int(np.flatnonzero(got != want)[0])
            alone = self.ctx.crc32_batch(t, [c.reads[k]])[0]
            self.fail("crc32_batch", f"span {k} {c.reads[k]}: {got[k]:#010x}, want {want[k]:#010x}; alone {alone:#010x}")

    def kinds(self):
        c = self.case
        return [MB.measure_kind(c.measure_block, c.hist), MB.lz_kind(c.lz_block), MB.chunk_kind(c.chunk_params)]

    def measures(self, t, host):
        for kind in self.kinds():
            try:
                MB.check(self.S, self.ctx, kind, t, host, self.case.reads)
            except AssertionError:
                for k, span in enumerate(self.case.reads):       # one by one: a miss names its span
                    if span[1]:
                        got, want = MB.batch(self.ctx, kind, t, [span]), kind.judge(self.S, MB.live(host, [span]))
                        if got != want:
                            self.fail(f"{kind}.add_batch", f"span {k} {span} alone gives {got}, want {want}")
                got, want = MB.batch(self.ctx, kind, t, self.case.reads), kind.judge(self.S, MB.live(host, self.case.reads))
                self.fail(f"{kind}.add_batch", f"every span alone is right; the list gives {got}, the restatement "
                                               f"{want}, one add per span {MB.each(self.ctx, kind, t, self.case.reads)}")

    # ---- step 7 --------------------------------------------------------------------------

    def streams(self, t, clean, dirty):
        c, torch = self.case, self.torch
        u = self.dev(C.upload_image(c))
        for r in c.runs:
            self.calls[r.kind][2](u[r.start:], r.size, r.n, stride=r.stride, dedup=r.dedup, compress=r.compress,
                                  seed_base=r.seed_base, first_obj=r.first_obj)
        self.same_bytes("fill_stream + dgen_fill_stream", u, clean)
        for state, buf, image in (("clean", u, clean), ("corrupted", t, dirty)):
            for r in c.runs:
                call = self.calls[r.kind][3]
                got = call(buf[r.start:], r.size, r.n, stride=r.stride, dedup=r.dedup, compress=r.compress,
                           seed_base=r.seed_base, first_obj=r.first_obj)
                tot, _ = C.expected_verify(image, c, r.kind, self.oracle, self.base)
                want = self.S.VerifyResult(tot[0], tot[1], None if tot[2] is None else tot[2] - r.start)
                if got != want or self.calls[r.kind][1](buf, c.verify[r.kind], per_object=False).total != \
                        self.S.VerifyResult(*tot):
                    self.fail(f"{call.__name__} ({state})", f"{got}, want {want} (the batch totals from the run's start)")
        for kind in self.kinds():
            for r in c.runs:
                with kind.open(self.ctx) as h:
                    h.add_stream(t[r.start:], r.size, r.n, r.stride)
                    got = h.result()
                want = MB.batch(self.ctx, kind, t, r.spans)
                if got != want:
                    self.fail(f"{kind}.add_stream", f"{r}: {got}, add_batch over its spans {want}")

    def run(self):
        c, ctx = self.case, self.ctx
        try:
            ctx.set_waves_per_block(c.waves)
            ctx.set_batch_tile(c.tile)
            t, clean = self.fill()
            self.verify(t, clean, "clean")
            dirty = C.corrupted(clean, c)
            for pos, mask, _k, _mode in c.corrupt:
                t[pos] ^= mask
            self.verify(t, dirty, "corrupted")
            host = self.same_bytes("the verifies wrote to the arena, or the corruption went astray", t, dirty)
            self.crc(t, host)
            self.measures(t, host)
            if c.uniform:
                self.streams(t, clean, dirty)
            self.same_bytes("a read-only call wrote to the arena", t, dirty)
        finally:
            ctx.set_waves_per_block(0)
            ctx.set_batch_tile(0)


@pytest.mark.parametrize("seed", range(C.SEEDS * SOAK))
def test_fuzz_batch_loop(S, torch, gpu_ctx, oracle, base, seed):
    Loop(S, torch, gpu_ctx, oracle, base, C.draw(seed)).run()
