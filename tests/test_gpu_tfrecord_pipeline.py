"""GPU: the host protocol of the TFRecord calls (s3dg_tfrecord.cpp,
s3dg_tfrecord_var.cpp) used as it is meant to be:
calls enqueued back to back on a side stream that is still busy, so that both
of the stream's pinned tables are owned by uploads that have not happened when
the next call comes; the uniform, var and index calls and the two checks
interleaved over the same two tables; tables regrown while earlier calls are
queued; two threads on two streams.

The stream is kept busy by a blocker: torch.cuda._sleep where present, else
repeated device copies, sized from a timed sample to BLOCK_MS.  Every test
that relies on it asserts that the stream has not drained after the calls it
wants queued have returned, so none passes because the blocker was short.

Every value is exact.  The judges are tests/tfrecord_var_restatement.py's
through tests/tfrecord_fuzz_cases.py's Arena; whole arenas are compared
between poisoned guards, gaps included, and the source is held unchanged."""
import threading
import time

import numpy as np
import pytest

import tfrecord_fuzz_cases as F
import tfrecord_var_restatement as J
from test_gpu_tfrecord_var import Case as VarCase, call_rows

pytestmark = pytest.mark.gpu

KiB, MiB = 1 << 10, 1 << 20
POISON = F.POISON
BLOCK_MS = 250.0


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


_unit = {}


def _work(torch, units):
    """`units` of blocking work on the current stream."""
    if hasattr(torch.cuda, "_sleep"):
        torch.cuda._sleep(int(units * 1_000_000))
        return
    if "buf" not in _unit:
        _unit["buf"] = torch.zeros(2, 256 * MiB, dtype=torch.uint8, device="cuda:0")
    for _ in range(max(1, int(units))):
        _unit["buf"][1].copy_(_unit["buf"][0])


def block(torch, stream, ms=BLOCK_MS):
    """Keeps `stream` busy for about `ms` milliseconds; returns the two events
    around the blocker, for its measured duration after a sync."""
    with torch.cuda.stream(stream):
        if "ms" not in _unit:   # one unit of work, timed once (after a first one that pays for the start)
            _work(torch, 1)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            _work(torch, 4)
            b.record(stream)
            b.synchronize()
            _unit["ms"] = max(a.elapsed_time(b) / 4, 1e-3)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        _work(torch, ms / _unit["ms"])
        b.record(stream)
    return a, b


class Dev:
    """An Arena's tensors: the source uploaded, destination and index poisoned."""

    def __init__(self, torch, arena):
        self.torch, self.a = torch, arena
        self.src = torch.from_numpy(arena.src).to("cuda:0")
        self.dst = torch.full((len(arena.dst),), POISON, dtype=torch.uint8, device="cuda:0")
        self.idx = torch.full((len(arena.idx),), POISON, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

    def poison(self):
        self.dst.fill_(POISON)
        self.idx.fill_(POISON)
        self.torch.cuda.synchronize()

    def held(self, only=None):
        """Both arenas and the source are the judge's; with `only`, the shards
        not named are still poison."""
        a = self.a
        want_dst, want_idx = a.dst, a.idx
        if only is not None:
            want_dst, want_idx = np.full(len(a.dst), POISON, np.uint8), np.full(len(a.idx), POISON, np.uint8)
            for k in only:
                _, d, l, i = a.shards[k]
                want_dst[d:d + a.framed(k)] = a.dst[d:d + a.framed(k)]
                want_idx[i:i + 16 * len(l)] = a.idx[i:i + 16 * len(l)]
        got = self.dst.cpu().numpy()
        bad = np.flatnonzero(got != want_dst)
        assert bad.size == 0, (bad[:8], [a.record_at(int(p)) for p in bad[:2]], got[bad[:8]], want_dst[bad[:8]])
        got = self.idx.cpu().numpy()
        bad = np.flatnonzero(got != want_idx)
        assert bad.size == 0, (bad[:8], [a.index_owner(int(p)) for p in bad[:2]], got[bad[:8]], want_idx[bad[:8]])
        assert np.array_equal(self.src.cpu().numpy(), a.src)


def three_lists():
    """Three tables of a few hundred records each: uniform, var, uniform."""
    rng = np.random.default_rng(70)
    u1 = [[100 + 7 * k] * 30 for k in range(10)]                                   # shards 0-9
    v = [rng.integers(0, 3000, 120).tolist(), [], [0] * 4, rng.integers(0, 40, 200).tolist() + [40 * KiB + 3, 0, 70 * KiB]]
    u2 = [[1023] * 50, [0] * 20, [2049] * 100, [33 * KiB + 5] * 3, [16] * 80]       # shards 14-18
    return u1 + v + u2, list(range(0, 10)), list(range(10, 14)), list(range(14, 19))


def enqueue_three(ctx, d, ks1, ks2, ks3, stream, after_second=None):
    a = d.a
    ctx.tfrecord_frame_batch(d.src, d.dst, a.uniform(ks1), index=d.idx, stream=stream)
    ctx.tfrecord_frame_var_batch(d.src, d.dst, a.var(ks2), index=d.idx, stream=stream)
    if after_second:
        after_second()
    ctx.tfrecord_frame_batch(d.src, d.dst, a.uniform(ks3), index=d.idx, stream=stream)


def test_three_calls_behind_a_blocker(S, gpu_ctx, torch, capsys):
    """Two pinned tables, three calls in flight.  Both tables are warmed, then
    a blocker holds the side stream while a uniform, a var and a uniform frame
    call with three different tables are enqueued.  When the second has
    returned the stream has not drained: both tables belong to uploads that
    have not happened, and the third call has to wait for the first one's
    upload before it rebuilds that table.  After one sync all three calls'
    streams and indexes are the judge's.

    Measured on an MI355X: enqueueing the three calls on the idle stream took
    0.159 ms of host time (perf_counter), the blocker ran 249.3 ms (events):
    1500 times as long.  The test prints both and asserts the factor of ten."""
    lists, ks1, ks2, ks3 = three_lists()
    d = Dev(torch, F.Arena(lists, 70))
    stream = torch.cuda.Stream(device="cuda:0")
    try:
        enqueue_three(gpu_ctx, d, ks1, ks2, ks3, stream)       # warms both tables: nothing regrows below
        gpu_ctx.sync(stream)
        d.held()
        d.poison()
        t0 = time.perf_counter()
        enqueue_three(gpu_ctx, d, ks1, ks2, ks3, stream)       # the host time of the three calls, nothing in their way
        enqueue_ms = (time.perf_counter() - t0) * 1e3
        gpu_ctx.sync(stream)
        d.held()
        d.poison()
        drained = []
        ev = block(torch, stream)
        enqueue_three(gpu_ctx, d, ks1, ks2, ks3, stream, after_second=lambda: drained.append(stream.query()))
        gpu_ctx.sync(stream)
        blocker_ms = ev[0].elapsed_time(ev[1])
        with capsys.disabled():
            print(f"\n  three calls enqueued in {enqueue_ms:.3f} ms; the blocker ran {blocker_ms:.1f} ms")
        assert drained == [False]          # two uploads queued behind the blocker when the third call came
        assert blocker_ms >= 10 * enqueue_ms, (blocker_ms, enqueue_ms)
        d.held()
    finally:
        gpu_ctx.release_stream(stream)


def test_index_walk_between_frames(S, gpu_ctx, torch):
    """Behind a blocker: a uniform frame, a var frame, the index walk of both
    calls' streams (synchronous; it takes the first frame's table), a uniform
    frame.  The walk finds what the frames before it on the stream wrote: its
    entries, written to a second index arena, are the judge's."""
    lists, ks1, ks2, ks3 = three_lists()
    d = Dev(torch, F.Arena(lists, 71))
    a = d.a
    w_idx = torch.full_like(d.idx, POISON)
    stream = torch.cuda.Stream(device="cuda:0")
    try:
        enqueue_three(gpu_ctx, d, ks1, ks2, ks3, stream)
        gpu_ctx.sync(stream)
        d.poison()
        block(torch, stream)
        gpu_ctx.tfrecord_frame_batch(d.src, d.dst, a.uniform(ks1), index=d.idx, stream=stream)
        gpu_ctx.tfrecord_frame_var_batch(d.src, d.dst, a.var(ks2), index=d.idx, stream=stream)
        assert not stream.query()
        walks = gpu_ctx.tfrecord_index_batch(d.dst, a.spans(ks1 + ks2), w_idx, stream=stream)
        gpu_ctx.tfrecord_frame_batch(d.src, d.dst, a.uniform(ks3), index=d.idx, stream=stream)
        gpu_ctx.sync(stream)
        for k, w in zip(ks1 + ks2, walks):
            assert w.ok and w.records == len(lists[k]) and w.stop_offset == a.framed(k) and w.trailing == 0, (k, w)
        d.held()
        want = np.full(len(a.idx), POISON, np.uint8)
        for k in ks1 + ks2:
            i, n = a.shards[k][3], len(lists[k])
            want[i:i + 16 * n] = a.idx[i:i + 16 * n]
        assert np.array_equal(w_idx.cpu().numpy(), want)
    finally:
        gpu_ctx.release_stream(stream)


def test_checks_between_frames(S, gpu_ctx, torch):
    """Behind a blocker: frame, frame, the uniform check of the first, frame,
    the var check of everything framed so far.  Each check reads what the
    frames before it on the stream wrote, and is clean; each takes a table."""
    lists, ks1, ks2, ks3 = three_lists()
    d = Dev(torch, F.Arena(lists, 72))
    a = d.a
    stream = torch.cuda.Stream(device="cuda:0")
    try:
        enqueue_three(gpu_ctx, d, ks1, ks2, ks3, stream)
        gpu_ctx.sync(stream)
        d.poison()
        block(torch, stream)
        gpu_ctx.tfrecord_frame_batch(d.src, d.dst, a.uniform(ks1), index=d.idx, stream=stream)
        gpu_ctx.tfrecord_frame_var_batch(d.src, d.dst, a.var(ks2), index=d.idx, stream=stream)
        assert not stream.query()
        res = gpu_ctx.tfrecord_check_batch(d.dst, a.uniform(ks1), stream=stream)
        assert res.ok and res.records == sum(len(lists[k]) for k in ks1), res
        d.held(only=ks1 + ks2)
        block(torch, stream)
        gpu_ctx.tfrecord_frame_batch(d.src, d.dst, a.uniform(ks3), index=d.idx, stream=stream)
        assert not stream.query()
        everything = ks1 + ks2 + ks3
        res = gpu_ctx.tfrecord_check_var_batch(d.dst, a.var(everything), stream=stream)
        assert res.ok and res.records == sum(len(lists[k]) for k in everything) and res.shards == (), res
        gpu_ctx.tfrecord_frame_var_batch(d.src, d.dst, a.var(ks2), index=d.idx, stream=stream)
        gpu_ctx.sync(stream)
        d.held()
    finally:
        gpu_ctx.release_stream(stream)


def test_frame_of_the_previous_frame_s_output(S, gpu_ctx, torch):
    """A frame whose source is the stream the call before it writes: the
    framed shard is the payload, cut into records of other lengths.  Nothing
    but the stream's order makes the second call read framed bytes, not
    poison.  Behind a blocker, uniform then var and var then uniform."""
    rng = np.random.default_rng(73)
    inner = [[700] * 64, rng.integers(0, 5000, 90).tolist() + [0, 35 * KiB]]
    a = F.Arena(inner, 73)
    d = Dev(torch, a)
    outer, expect = [], []
    for k in (0, 1):
        framed = a.framed(k)
        if k == 0:   # the var stream of shard 0 framed again as records of one length
            rs = 179
            assert framed % rs == 0
            lens = [rs] * (framed // rs)
        else:
            cuts = np.sort(rng.integers(0, framed + 1, 150))
            lens = np.diff(np.concatenate(([0], cuts, [framed]))).tolist()
        outer.append(lens)
        expect.append(J.frame_np(a.dst[a.shards[k][1]:a.shards[k][1] + framed].tobytes(), lens))
    assert a.framed(0) == 64 * 716
    o = F.Arena(outer, 74, build=False)                  # its layout only: the sources are the inner streams
    want_dst, want_idx = np.full(o.sizes[1], POISON, np.uint8), np.full(o.sizes[2], POISON, np.uint8)
    for (_, d_off, _, i_off), (st, ix) in zip(o.shards, expect):
        want_dst[d_off:d_off + len(st)] = st
        want_idx[i_off:i_off + len(ix)] = ix
    o_dst = torch.full((o.sizes[1],), POISON, dtype=torch.uint8, device="cuda:0")
    o_idx = torch.full((o.sizes[2],), POISON, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    second = [(a.shards[k][1], o.shards[k][1], np.array(outer[k], np.uint64), o.shards[k][3]) for k in (0, 1)]
    stream = torch.cuda.Stream(device="cuda:0")
    try:
        block(torch, stream)
        gpu_ctx.tfrecord_frame_var_batch(d.src, d.dst, a.var([0]), index=d.idx, stream=stream)
        s, t, l, i = second[0]
        gpu_ctx.tfrecord_frame_batch(d.dst, o_dst, [(s, t, len(l), int(l[0]), i)], index=o_idx, stream=stream)
        gpu_ctx.tfrecord_frame_batch(d.src, d.dst, [(a.shards[1][0], a.shards[1][1], 0, 5, a.shards[1][3])], index=d.idx,
                                     stream=stream)                       # a call without records takes no table
        gpu_ctx.tfrecord_frame_var_batch(d.src, d.dst, a.var([1]), index=d.idx, stream=stream)
        gpu_ctx.tfrecord_frame_var_batch(d.dst, o_dst, [second[1]], index=o_idx, stream=stream)
        assert not stream.query()
        gpu_ctx.sync(stream)
        d.held()
        assert np.array_equal(o_dst.cpu().numpy(), want_dst) and np.array_equal(o_idx.cpu().numpy(), want_idx)
    finally:
        gpu_ctx.release_stream(stream)


def up256(n):
    return (n + 255) // 256 * 256


def var_table(lists):
    """(host bytes, device bytes) of a var call's table (s3dg_tfrecord_var_plan.h:
    powers, live + 1 shard entries, one entry per record and one per shard, 8
    bytes per long record; the device side adds 8 bytes per entry and 4 per
    region when there are long records)."""
    live = [l for l in lists if len(l)]
    ents = sum(len(l) for l in live) + len(live)
    regs = [F.regions(int(n)) for l in live for n in l]
    longs = sum(r > 1 for r in regs)
    host = F.up16(256 + 40 * (len(live) + 1)) + 16 * ents + 8 * longs
    return host, up256(up256(host) + 8 * ents) + (4 * sum(regs) if longs else 0)


def grown(need):
    return max(1 << 14, need + need // 4)


def test_regrow_in_flight(S, gpu_ctx, torch):
    """On a fresh stream, behind a blocker: a small call; a var call of more
    than 1100 records, whose table is past the 16 KiB a table starts with; a
    uniform call of more than 190 shards, past 16 KiB too, in the other
    table; a var call whose records of several regions make the device side
    of the second call's table too small by their raw CRCs; a small call
    again.  The sizes are asserted from the plan's layout.  All results are
    the judge's, and releasing the stream brings the context's stream states
    back to their number."""
    rng = np.random.default_rng(75)
    small1, small2 = [[5, 0, 300]], [[1025] * 3]
    many = [rng.integers(0, 200, 1150).tolist()]
    wide = [[17 + k % 5] * 2 for k in range(200)]
    long_ = [[int(x) for x in rng.integers(0, 64, 500)] + [33 * KiB + int(x) for x in rng.integers(0, 40 * KiB, 650)]]
    rng.shuffle(long_[0])
    lists = small1 + many + wide + long_ + small2
    k_small1, k_many, k_wide, k_long, k_small2 = [0], [1], list(range(2, 202)), [202], [203]
    host_many, dev_many = var_table(many)
    host_long, dev_long = var_table(long_)
    assert call_rows(long_) == call_rows(many) == F.REGION_ROWS
    assert len(many[0]) > 1100 and host_many > 1 << 14
    assert len(wide) > 190 and 88 * len(wide) > 1 << 14
    assert sum(F.regions(n) > 1 for n in long_[0]) == 650 and dev_long > grown(dev_many)          # the device side regrows
    assert dev_long - 4 * sum(F.regions(n) for n in long_[0]) <= grown(dev_many)                  # and by the raw CRCs alone
    d = Dev(torch, F.Arena(lists, 75))
    a = d.a
    stream = torch.cuda.Stream(device="cuda:0")
    gpu_ctx.release_stream(stream)   # torch hands streams out of a pool: whatever an earlier user of this one left
    before = gpu_ctx.stream_state_count()
    try:
        block(torch, stream)
        gpu_ctx.tfrecord_frame_var_batch(d.src, d.dst, a.var(k_small1), index=d.idx, stream=stream)
        assert not stream.query()
        gpu_ctx.tfrecord_frame_var_batch(d.src, d.dst, a.var(k_many), index=d.idx, stream=stream)
        gpu_ctx.tfrecord_frame_batch(d.src, d.dst, a.uniform(k_wide), index=d.idx, stream=stream)
        gpu_ctx.tfrecord_frame_var_batch(d.src, d.dst, a.var(k_long), index=d.idx, stream=stream)
        gpu_ctx.tfrecord_frame_batch(d.src, d.dst, a.uniform(k_small2), index=d.idx, stream=stream)
        gpu_ctx.sync(stream)
        assert gpu_ctx.stream_state_count() == before + 1
        d.held()
        assert gpu_ctx.tfrecord_check_var_batch(d.dst, a.var(list(range(len(lists)))), stream=stream).ok
    finally:
        gpu_ctx.release_stream(stream)
    assert gpu_ctx.stream_state_count() == before


def test_two_threads_two_streams_var(S, gpu_ctx, torch):
    """Two threads on two streams run the var frame, the var check and the
    index walk of different lists at once, four rounds each."""
    rng = np.random.default_rng(76)
    cases = [VarCase(torch, [rng.integers(0, 6000, 60).tolist() for _ in range(12)] + [[2, 70000, 0, 33 * KiB]], 76),
             VarCase(torch, [rng.integers(0, 130, 900).tolist(), [], [0] * 7, [3 * MiB + 1, 5]], 77)]
    streams = [torch.cuda.Stream(device="cuda:0") for _ in cases]
    errors = []

    def work(c, s):
        try:
            for _ in range(4):
                c.t_dst.fill_(POISON)
                c.t_idx.fill_(POISON)
                torch.cuda.synchronize()
                c.frame(gpu_ctx, torch, stream=s)
        except BaseException as e:   # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(c, s)) for c, s in zip(cases, streams)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for s in streams:
        gpu_ctx.release_stream(s)
    assert not errors, errors
