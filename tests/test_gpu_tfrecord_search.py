"""GPU: Context.tfrecord_index_search_batch (s3dg_tfrecord_search.hip; DESIGN.md
§5.5.3) against the plain restatement of the walk, tests/tfrecord_var_restatement.py,
on the same bytes: every field of every result and every byte of a poisoned
index are equal, at the edges the search has of its own: the tile of its
candidate pass (T), the hop of its anchor walk (H), headers that only look like
headers, headers on the chain whose CRC is wrong, and neighbours in one call."""
import numpy as np
import pytest

import tfrecord_var_restatement as J
from test_gpu_tfrecord_var import POISON, held

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def geo(S):
    return S.tfrecord_search_geometry()


def rec(n, fill=0x11):
    """One framed record of n bytes of `fill` (the walk never reads a payload)."""
    return J.header(n) + bytes([fill]) * (n + 4)


def framed(rng, lens):
    return J.frame(rng.integers(0, 256, int(sum(lens)), dtype=np.uint8).tobytes(), lens)[0]


def search(ctx, torch, items, gaps=None, lead=0, order=None, twice=()):
    """items is [(bytes, max_records)], laid out from byte `lead` with gaps[k]
    poison bytes behind stream k, index slots in `order` with a poisoned entry
    between them, the streams of `twice` listed a second time.  Holds every
    result and the whole index to the judge; returns (walks, judges)."""
    gaps = gaps or [3] * len(items)
    spans, at = [], lead
    for (data, _), gap in zip(items, gaps):
        spans.append(at)
        at += len(data) + gap
    host = np.full(at + 16, POISON, np.uint8)
    for off, (data, _) in zip(spans, items):
        host[off:off + len(data)] = np.frombuffer(data, np.uint8)
    listed = list(range(len(items))) + list(twice)
    slots, io = {}, 16
    for m in (order or range(len(listed))):
        data, cap = items[listed[m]]
        slots[m] = io
        io += 16 * min(cap, len(data) // 16) + 16
    src = torch.from_numpy(host).to("cuda:0")
    idx = torch.full((io,), POISON, dtype=torch.uint8, device="cuda:0")
    walks = ctx.tfrecord_index_search_batch(src, [(spans[k], len(items[k][0]), slots[m], items[k][1]) for m, k in enumerate(listed)], idx)
    want = np.full(io, POISON, np.uint8)
    judges = [J.walk(*items[k]) for k in listed]
    for m, (w, j) in enumerate(zip(walks, judges)):
        held(w, j)
        e = np.array(j["entries"], "<u8").reshape(-1)
        want[slots[m]:slots[m] + 8 * len(e)] = e.view(np.uint8)
    assert np.array_equal(idx.cpu().numpy(), want)
    return walks, judges


@pytest.mark.parametrize("lead", range(16))
def test_endings(gpu_ctx, torch, lead):
    """walk_endings() in one call, every stream at `lead` (mod 16)."""
    cases = J.walk_endings()
    _, judges = search(gpu_ctx, torch, [(d, c) for _, d, c in cases], gaps=[-len(d) % 16 for _, d, _ in cases], lead=lead)
    assert {j["status"] for j in judges} == {0, 1, 2}


@pytest.mark.parametrize("lead", (0, 5))
def test_tile_edges(gpu_ctx, torch, geo, lead):
    """A true header at T - 12 (it ends at T) and at each of T - 11 .. T; streams
    of T, T - 1, T + 1 and 2 T + 5 bytes; zero-length records across the edge."""
    T = geo[0]
    items = [(rec(at - 16) + rec(33) + rec(0), J.NONE) for at in range(T - 12, T + 1)]
    items += [(rec(total - 48 - 7) + rec(0) + rec(7), J.NONE) for total in (T, T - 1, T + 1, 2 * T + 5)]
    items.append((rec(0) * (T // 16 + 9), J.NONE))
    assert [len(d) for d, _ in items[13:17]] == [T, T - 1, T + 1, 2 * T + 5]
    _, judges = search(gpu_ctx, torch, items, lead=lead)
    assert [j["entries"][1][0] for j in judges[:13]] == list(range(T - 12, T + 1)) and all(j["status"] == 0 for j in judges)


@pytest.mark.parametrize("hops,more", ((0, 0), (0, 1), (1, -1), (1, 0), (1, 1), (2, 0), (2, 1)))
def test_hop_edges(gpu_ctx, torch, geo, hops, more):
    """hops * H + more records of 0-48 bytes under every max_records around a
    hop and around the count, in one call; then every capped stream resumed at
    stop_offset until it is complete: the pieces' entries, their offsets
    rebased, are the one-shot's."""
    H = geo[1]
    count = hops * H + more
    rng = np.random.default_rng(count)
    data = framed(rng, rng.integers(0, 49, count).tolist())
    whole = np.array(J.walk(data)["entries"], "<u8").reshape(-1, 2)
    caps = sorted({c for c in (1, H - 1, H, H + 1, count - 1, count, count + 1) if c >= 0})
    search(gpu_ctx, torch, [(data, c) for c in caps])
    caps = [c for c in caps if c]
    src = torch.from_numpy(np.frombuffer(data + bytes(16), np.uint8).copy()).to("cuda:0")
    W = len(data) // 16 + 1                      # entries a slot can be asked to hold, and one that stays poison
    idx = torch.full((len(caps), W, 16), POISON, dtype=torch.uint8, device="cuda:0")
    at, done, live = [0] * len(caps), [0] * len(caps), list(range(len(caps)))
    base = np.zeros((len(caps), W), np.uint64)
    while live:
        walks = gpu_ctx.tfrecord_index_search_batch(
            src, [(at[m], len(data) - at[m], 16 * (W * m + done[m]), caps[m]) for m in live], idx)
        for m, w in zip(list(live), walks):
            assert (w.records, w.status) == (caps[m], "full") or w.status == "complete"
            if w.status == "complete":
                live.remove(m)
            base[m, done[m]:done[m] + w.records] = at[m]
            at[m] += w.stop_offset
            done[m] += w.records
    assert done == [count] * len(caps)
    got = idx.cpu().numpy()
    assert bool((got[:, count:] == POISON).all())
    e = got[:, :count].copy().view("<u8")
    e[:, :, 0] += base[:, :count]
    assert all(np.array_equal(e[m], whole) for m in range(len(caps)))


def test_decoys(gpu_ctx, torch):
    """Headers nobody reaches from byte 0: a framed stream of 5 records as a
    payload, ending inside it; the same as payload and footer, so that its
    last link lands on the next true header; a valid header one byte behind a
    true header and one ending a byte before the next; one in the last 12
    bytes of a stream and of a stream's last record."""
    inner = b"".join(rec(n, 0x22) for n in (3, 0, 9, 1, 5))
    more = rec(2) + rec(40) + rec(0)
    ends_inside = J.header(len(inner) + 7) + inner + bytes([0x11]) * 11 + more
    joins = J.header(len(inner) - 4) + inner + more
    around = (J.header(25) + b"\x33" + J.header(0) + b"\x44" * 3 + J.header(0) + b"\x44"
              + J.header(20) + b"\x55" + J.header(1) + b"\x66" * 11)
    last = rec(30) + J.header(0)
    last_in_record = J.header(8) + J.header(0)
    _, judges = search(gpu_ctx, torch, [(d, J.NONE) for d in (ends_inside, joins, around, last, last_in_record)])
    assert [(j["records"], j["status"]) for j in judges] == [(4, 0), (4, 0), (2, 0), (1, 1), (1, 0)]
    assert J.walk(joins[12:])["records"] == 5 + 3 and J.walk(ends_inside[12:])["records"] == 5   # the decoy chain joins the true one


def test_wrong_crcs_on_the_chain(gpu_ctx, torch, geo):
    """One flipped bit in the length CRC of record 0, a middle one, the last,
    two neighbours and record H (a break where an anchor starts); a flipped bit
    in a length, after which the chain runs through payload; and every CRC of a
    300-record stream."""
    H = geo[1]
    rng = np.random.default_rng(7)
    lens = rng.integers(0, 31, H + 40).tolist()
    data = framed(rng, lens)
    starts = [o for o, _ in J.walk(data)["entries"]]

    def flipped(records, byte=8):
        b = bytearray(data)
        for i in records:
            b[starts[i] + byte + i % 4 * (byte == 8)] ^= 1 << (i % 8)
        return bytes(b)
    items = [(flipped(r), J.NONE) for r in ([0], [H // 2], [H + 39], [H // 3, H // 3 + 1], [H])]
    items.append((flipped([1], byte=0), J.NONE))
    short = framed(rng, rng.integers(0, 31, 300).tolist())
    b = bytearray(short)
    for o, _ in J.walk(short)["entries"]:
        b[o + 11] ^= 0x80
    items += [(bytes(b), J.NONE), (bytes(b), 299)]
    _, judges = search(gpu_ctx, torch, items)
    assert [(j["bad_length_crc"], j["first_bad_record"]) for j in judges[:5]] == [(1, 0), (1, H // 2), (1, H + 39), (2, H // 3), (1, H)]
    assert judges[5]["entries"] != judges[0]["entries"] and judges[6]["bad_length_crc"] == 300 and judges[7]["status"] == 2


def test_many_streams(gpu_ctx, torch):
    """70 streams and one of them twice: empty ones, ones below 12 bytes,
    truncated and trailing ones, all flush against each other; every fifth
    ends with 11 bytes that, with its neighbour's first byte, are a header
    whose record would fit there; index slots in shuffled order."""
    rng = np.random.default_rng(11)
    items = []
    while len(items) < 70:
        k = len(items)
        data = b"" if k % 9 == 0 else framed(rng, rng.integers(0, 61, int(rng.integers(0, 40))).tolist())
        if k % 9 == 1:
            data = data[:int(rng.integers(0, 12))]
        if k % 7 == 2 and len(data) > 20:
            data = data[:len(data) - int(rng.integers(1, 20))]
        if k % 7 == 3:
            data += bytes([0x5A]) * int(rng.integers(0, 16))
        if k % 5 == 4:
            h = J.header(0x2A)
            items.append((data + h[:11], J.NONE))
            data = rec(h[11]) + rec(50) + rec(3)              # its first byte is the header's twelfth; 0x2A + 4 bytes follow
            assert J.walk(h[:11] + data)["entries"][0] == (0, 16 + 0x2A)
        items.append((data, int(rng.integers(0, 8)) if k % 11 == 5 else J.NONE))
    items = items[:70]
    order = rng.permutation(71).tolist()
    _, judges = search(gpu_ctx, torch, items, gaps=[0] * 70, lead=1, order=order, twice=(33,))
    assert {j["status"] for j in judges} == {0, 1, 2} and judges[33] == judges[70]


def test_larger_run(gpu_ctx, torch, geo):
    """200 000 records of log-uniform length 0-64 bytes: several tiles and
    hundreds of hops, complete and stopped at 123 457 records."""
    T, H = geo
    rng = np.random.default_rng(13)
    lens = (np.exp2(rng.uniform(0, np.log2(66), 200000)).astype(np.int64) - 1).clip(0, 64)
    out = bytearray()
    for n in lens.tolist():
        out += rec(n, 0x6B)
    assert len(out) > 4 * T and 200000 > 100 * H and lens.min() == 0 and lens.max() == 64
    walks, _ = search(gpu_ctx, torch, [(bytes(out), J.NONE), (bytes(out), 123457)], lead=3)
    assert (walks[0].records, walks[0].status, walks[1].records, walks[1].status) == (200000, "complete", 123457, "full")


def test_refusals_are_the_siblings(S, gpu_ctx, torch):
    """The same bad arguments give both calls the same message; n == 0 succeeds."""
    from s3dlio_amd import _lib
    src = torch.zeros(4096, dtype=torch.uint8, device="cuda:0")
    p = src.data_ptr()
    res = (_lib.TfrWalkRec * 2)()
    ok = [(0, 100, 0, 4), (100, 100, 64, 4)]
    bad = [(0, p, ok, 2, res), (p, 0, ok, 2, res), (p, p, ok, 2, None), (p, p, None, 2, res), (p, p + 8, ok, 2, res),
           (p, p, [(0, 100, 8, 4), ok[1]], 2, res), (p, p, [ok[0], (2**64 - 50, 100, 0, 4)], 2, res),
           (p, p, [ok[0], (0, 3200, 2**64 - 16, 200)], 2, res)]
    seen = set()
    for base, idx, streams, n, r in bad:
        arr = (_lib.TfrStream * 2)(*[_lib.TfrStream(*s) for s in streams]) if streams else None
        msgs = []
        for sym in ("s3dg_tfrecord_index_batch", "s3dg_tfrecord_index_search_batch"):
            with pytest.raises(ValueError) as e:
                _lib.call(sym, gpu_ctx._h, base, idx, arr, n, None, r)
            msgs.append(str(e.value))
        assert msgs[0] == msgs[1]
        seen.add(msgs[0])
    assert len(seen) == len(bad)
    _lib.call("s3dg_tfrecord_index_search_batch", gpu_ctx._h, None, None, None, 0, None, None)
    ms = (_lib.ctypes.c_float * 6)()
    arr = (_lib.TfrStream * 2)(*[_lib.TfrStream(*s) for s in ok])
    _lib.call("s3dg_tfrecord_index_search_timed", gpu_ctx._h, p, p + 2048, arr, 2, None, res, ms)
    assert all(m >= 0 for m in ms) and [(r.records, r.status, r.bad_length_crc) for r in res] == [(4, 2, 4)] * 2   # zeros: records of length 0
