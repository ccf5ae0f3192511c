"""GPU: the TFRecord calls under seeded fuzz (cases from
tests/tfrecord_fuzz_cases.py, which tests/test_tfrecord_fuzz_cpu.py holds to
their checklist): one list of about 5000 records of every class per seed,
framed by three to five uniform and var calls enqueued back to back on a side
stream without a sync, each call twice; walked and scanned from its bytes
alone, whole and with spans cut short or extended; checked clean and after
one-bit flips.

Every value is exact.  The judges are tests/tfrecord_var_restatement.py's
frame and walk; whole arenas are compared between poisoned guards, gaps
included, and the source is held unchanged.  A failure prints the case
(describe()) and names the step, the call and the first offending shard and
record.  S3DG_FUZZ_SOAK=N runs N times the seeds."""
import ctypes
import os

import numpy as np
import pytest

import tfrecord_fuzz_cases as F
import tfrecord_var_restatement as J

pytestmark = pytest.mark.gpu
SOAK = max(1, int(os.environ.get("S3DG_FUZZ_SOAK", "1")))   # soak runs: seeds x SOAK
SEEDS = list(F.SEEDS) + [1000 + s for s in range(len(F.SEEDS) * (SOAK - 1))]
POISON = F.POISON
STATUS = ("complete", "truncated", "full")


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def fail(case, step, detail):
    raise AssertionError(f"{step}: {detail}\n{case.describe()}")


def call_of(case, k):
    return next(f"call {c} ({kind})" for c, (kind, ks) in enumerate(case.calls) if k in ks)


def same_arena(case, step, got, want, owner):
    """got == want byte for byte, or a failure naming the first differing
    byte's shard, record and call."""
    if np.array_equal(got, want):
        return
    bad = np.flatnonzero(got != want)
    k, i = owner(int(bad[0]))
    where = "before the first shard" if k is None else \
        f"{call_of(case, k)}, shard {k}, {'the gap behind it' if i is None else f'record {i}'}"
    fail(case, step, f"{bad.size} bytes differ, the first at {int(bad[0])}: {where}; "
                     f"got {got[bad[:8]].tolist()} want {want[bad[:8]].tolist()}")


def frame_raw(S, ctx, kind, a, ks, p_src, p_dst, p_idx, stream):
    """One frame call through the C ABI, its arrays overwritten as soon as it returns."""
    lib = S._lib
    if kind == "uniform":
        rows = a.uniform(ks)
        arr = (lib.TfrShard * len(rows))(*[lib.TfrShard(s, d, i, n, rs) for s, d, n, rs, i in rows])
        lib.call("s3dg_tfrecord_frame_batch", ctx._h, p_src, p_dst, p_idx, arr, len(rows), stream.cuda_stream)
    else:
        rows = a.var(ks)
        arr, len0 = (lib.TfrVarShard * len(rows))(), 0
        for j, (s, d, l, i) in enumerate(rows):
            arr[j] = lib.TfrVarShard(s, d, i, len(l), len0)
            len0 += len(l)
        lens = np.ascontiguousarray(np.concatenate([l for _, _, l, _ in rows]), dtype=np.uint64)
        lib.call("s3dg_tfrecord_frame_var_batch", ctx._h, p_src, p_dst, p_idx, arr, len(rows),
                 lens.ctypes.data_as(ctypes.POINTER(lib.c_u64)), len(lens), stream.cuda_stream)
        lens[:] = 2**64 - 1                                      # consumed before return
    ctypes.memset(arr, 0xFF, ctypes.sizeof(arr))


def held_walk(case, step, k, w, j):
    got = (w.records, w.status, w.stop_offset, w.trailing, w.bad_length_crc, w.first_bad_record)
    want = (j["records"], STATUS[j["status"]], j["stop_offset"], j["trailing"], j["bad_length_crc"], j["first_bad_record"])
    if got != want:
        fail(case, step, f"{call_of(case, k)}, shard {k}: walk {got}, the judge's {want}; first record off is {min(w.records, j['records'])}")


def flip_model(case):
    """{shard: {record: set of classes}} of the case's flips."""
    model = {}
    for k, i, off, bit, cls in case.flips:
        model.setdefault(k, {}).setdefault(i, set()).add(cls)
    return model


def held_check(case, step, res, model, records, per_shard=True):
    """The check's result is the model's, per shard and in total."""
    def counts(m):
        return (len(m),) + tuple(sum(cl in v for v in m.values()) for cl in range(3))
    total = tuple(map(sum, zip(*[counts(m) for m in model.values()]))) if model else (0, 0, 0, 0)
    first = (min(model), min(model[min(model)])) if model else (None, None)
    got = (res.records, res.bad_records, res.bad_length, res.bad_length_crc, res.bad_data_crc, res.first_shard, res.first_record)
    if got != (records,) + total + first:
        fail(case, step, f"totals {got}, the model's {(records,) + total + first}; the model's first bad is shard {first[0]} "
                         f"record {first[1]}")
    if not per_shard:
        if res.shards is not None:
            fail(case, step, "per_shard=False returned shards")
        return
    if [k for k, _ in res.shards] != sorted(model):
        off = sorted(set(k for k, _ in res.shards) ^ set(model))[0]
        fail(case, step, f"bad shards {[k for k, _ in res.shards]}, the model's {sorted(model)}: {call_of(case, off)}, "
                         f"shard {off}, record {min(model.get(off, {0: 0}))}")
    for k, r in res.shards:
        m = model[k]
        got = (r.records, r.bad_records, r.bad_length, r.bad_length_crc, r.bad_data_crc, r.first_shard, r.first_record)
        want = (len(case.lists[k]),) + counts(m) + (k, min(m))
        if got != want:
            fail(case, step, f"{call_of(case, k)}, shard {k}, record {min(m)}: {got}, the model's {want}")


@pytest.mark.parametrize("seed", SEEDS)
def test_fuzz(S, gpu_ctx, torch, seed):
    case = F.draw(seed)
    a = case.layout()
    n = len(a.shards)
    everything = list(range(n))
    records = sum(len(l) for l in case.lists)
    stream = torch.cuda.Stream(device="cuda:0")
    t_src = torch.from_numpy(a.src).to("cuda:0")
    t_dst, t_idx = (torch.full((len(x),), POISON, dtype=torch.uint8, device="cuda:0") for x in (a.dst, a.idx))
    v_dst, v_idx = torch.full_like(t_dst, POISON), torch.full_like(t_idx, POISON)
    torch.cuda.synchronize()   # source and poison are in place before the side stream writes
    try:
        # 1. frame: the calls back to back, each twice, nothing waited for
        for kind, ks in case.calls:
            for again in (False, True):
                if again and seed % 2:
                    frame_raw(S, gpu_ctx, kind, a, ks, t_src.data_ptr(), t_dst.data_ptr(), t_idx.data_ptr(), stream)
                elif kind == "uniform":
                    gpu_ctx.tfrecord_frame_batch(t_src, t_dst, a.uniform(ks), index=t_idx, stream=stream)
                else:
                    gpu_ctx.tfrecord_frame_var_batch(t_src, t_dst, a.var(ks), index=t_idx, stream=stream)
        # the whole list in one var call into a second arena: the uniform calls' shards among them
        gpu_ctx.tfrecord_frame_var_batch(t_src, v_dst, a.var(everything), index=v_idx, stream=stream)
        gpu_ctx.sync(stream)
        same_arena(case, "frame, destination", t_dst.cpu().numpy(), a.dst, a.record_at)
        same_arena(case, "frame, index", t_idx.cpu().numpy(), a.idx, a.index_owner)
        same_arena(case, "frame, the whole list in one var call, destination", v_dst.cpu().numpy(), a.dst, a.record_at)
        same_arena(case, "frame, the whole list in one var call, index", v_idx.cpu().numpy(), a.idx, a.index_owner)
        if not np.array_equal(t_src.cpu().numpy(), a.src):
            fail(case, "frame", "the source changed")

        # 2. walk and scan from the bytes alone; then with spans cut short and extended into the gap
        for delta in ({}, case.deltas):
            step = "walk" if not delta else "walk of changed spans"
            judged = [J.walk(a.dst[off:off + nbytes].tobytes(), cap) for off, nbytes, _, cap in a.spans(everything, delta)]
            want = np.full(len(a.idx), POISON, np.uint8)
            for (_, _, _, i_off), j in zip(a.shards, judged):
                e = np.array(j["entries"], "<u8").reshape(-1, 2)
                want[i_off:i_off + 16 * len(e)] = e.view(np.uint8).reshape(-1)
            if not delta and not np.array_equal(want, a.idx):
                fail(case, step, "the judge's walk is not the judge's index")
            w_idx = torch.full_like(t_idx, POISON)
            torch.cuda.synchronize()
            walks = gpu_ctx.tfrecord_index_batch(t_dst, a.spans(everything, delta), w_idx, stream=stream)
            for k, (w, j) in enumerate(zip(walks, judged)):
                held_walk(case, step, k, w, j)
            same_arena(case, step + ", index", w_idx.cpu().numpy(), want, a.index_owner)
            spans = [(off, nbytes) for off, nbytes, _, _ in a.spans(everything, delta)]
            walks, entries, res = gpu_ctx.tfrecord_scan(t_dst, spans, stream=stream)
            for k, (w, e, j) in enumerate(zip(walks, entries, judged)):
                full = J.walk(a.dst[spans[k][0]:spans[k][0] + spans[k][1]].tobytes())   # the scan's room is the span's
                held_walk(case, "scan, " + step, k, w, full)
                if e.tolist() != [list(x) for x in full["entries"]]:
                    fail(case, "scan, " + step, f"{call_of(case, k)}, shard {k}: the entries are not the judge's")
            held_check(case, "scan, " + step + ": the check covers the records found", res, {}, sum(w.records for w in walks))

        # 3. check: clean in both forms; then the model's counts after the flips
        for c, (kind, ks) in enumerate(case.calls):
            if kind == "uniform":
                res = gpu_ctx.tfrecord_check_batch(t_dst, a.uniform(ks), stream=stream)
                if not (res.ok and res.records == sum(len(case.lists[k]) for k in ks) and res.shards == ()):
                    fail(case, f"clean uniform check of call {c}", f"{res}; first shard {ks[res.first_shard or 0]}, "
                                                                   f"record {res.first_record}")
        held_check(case, "clean var check", gpu_ctx.tfrecord_check_var_batch(t_dst, a.var(everything), stream=stream), {}, records)
        hurt = a.dst.copy()
        for k, i, off, bit, _ in case.flips:
            l = case.lists[k]
            hurt[a.shards[k][1] + int(l[:i].sum()) + 16 * i + off] ^= 1 << bit
        t_hurt = torch.from_numpy(hurt).to("cuda:0")
        torch.cuda.synchronize()
        model = flip_model(case)
        held_check(case, "var check after the flips", gpu_ctx.tfrecord_check_var_batch(t_hurt, a.var(everything), stream=stream),
                   model, records)
        held_check(case, "var check after the flips, per_shard=False",
                   gpu_ctx.tfrecord_check_var_batch(t_hurt, a.var(everything), stream=stream, per_shard=False), model, records,
                   per_shard=False)
        if not np.array_equal(t_hurt.cpu().numpy(), hurt):
            fail(case, "check", "the check wrote to the stream")
    finally:
        gpu_ctx.release_stream(stream)
