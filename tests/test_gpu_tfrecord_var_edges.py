"""GPU: the device code of the var TFRecord calls at the edges its own loops
have (s3dg_tfrecord_var.hip): the row loop of
k_tfrecord_var_regions, which peels a record's first row when the record does
not start on a piece and so has its single-row, 4-row and 8-row steps one row
later than the uniform kernel's, in the frame form and in the check form
(which see the same record at different a); and k_tfrecord_walk with more
streams than the launch has waves, and along one chain of 20 000 records.

Every value is exact.  The judges are tests/tfrecord_var_restatement.py's;
whole arenas are compared between poisoned guards, as the Case of
tests/test_gpu_tfrecord_var.py does."""
import numpy as np
import pytest

import tfrecord_var_restatement as J
from test_gpu_tfrecord_var import DCRC, POISON, Case, call_rows, expect, held

pytestmark = pytest.mark.gpu

KiB = 1 << 10
ROWS = range(1, 19)
TAILS = (-17, -1, 0, 1, 15, 16, 17, 1008, 1023)


@pytest.fixture(scope="module")
def S():
    import s3dlio_amd
    return s3dlio_amd


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def rows_after_the_peel(a, n):
    """(whole rows of a record of n bytes whose first piece starts a bytes
    before it, rows left to the row loop once the first is peeled)."""
    nrows = (a + n) // KiB
    return nrows, nrows - (1 if a and nrows else 0)


def test_var_row_loop_edges(S, gpu_ctx, torch):
    """Records of r KiB + t, r in 1..18, t around a piece and a row, each as the
    second record of a shard whose first puts it at P mod 16 == 0 and at
    P mod 16 == 4: the frame form sees a = 0 and a = 4, the check form a = 12
    and a = 0.  All are one region.  Framed, parsed, checked clean and walked;
    then one flipped bit at every kind of site of one 13-row record whose
    check has a != 0 is reported as that record's data CRC and nothing else."""
    sizes = [r * KiB + t for r in ROWS for t in TAILS]
    lists = [[16 + p, n] for n in sizes for p in (0, 4)]
    assert call_rows(lists) == 32 and all(max(1, -(-((n + 15) // KiB) // 32)) == 1 for l in lists for n in l)
    for form, lead in (("frame", 0), ("check", 12)):
        left = {False: set(), True: set()}
        for first, n in lists:
            a = (lead + first) % 16
            nrows, rest = rows_after_the_peel(a, n)
            if a == 0 or nrows:                   # with a != 0, only where a first row is peeled
                left[a != 0].add(rest)
        assert left[False] == left[True] == set(range(19)), (form, left)
    c = Case(torch, lists, 80)
    shards = c.frame(gpu_ctx, torch)
    # the 13-row record with 63 whole tail pieces and 12 residual bytes, where the check has a = 12
    n = 13 * KiB + 1008
    k = lists.index([16, n])
    a = (12 + 16) % 16
    assert rows_after_the_peel(a, n) == (13, 12) and (a + n) % KiB == 63 * 16 + 12
    rec = shards[k][1] + 32                      # record 1 of shard k; its padded start is the record's own first byte
    sites = [q * KiB + 16 * ((5 * q + 3) % 64) + q % 16 for q in range(13)]          # one byte of each row
    sites += [12 + b for b in range(16 - a)]                                         # each byte of the masked first piece
    sites += [13 * KiB + 16 * p + 5 for p in range(63)]                              # one byte of each whole tail piece
    sites += [12 + n - 1 - b for b in range(12)]                                     # each residual byte
    assert len(set(sites)) == len(sites) == 13 + 4 + 63 + 12 and all(12 <= off < 12 + n for off in sites)
    for off in sites:
        c.t_dst[rec + off] ^= 1 << (off % 8)
        expect(gpu_ctx.tfrecord_check_var_batch(c.t_dst, shards), shards, k, 1, DCRC)
        c.t_dst[rec + off] ^= 1 << (off % 8)
    assert gpu_ctx.tfrecord_check_var_batch(c.t_dst, shards).ok


def test_walk_more_streams_than_waves(S, gpu_ctx, torch):
    """32 * CUs + 37 tiny streams in one call: the launch has at most 32 * CUs
    waves, so waves take a second stream and start it from fresh state.  0-3
    records of 0-40 bytes per stream at byte offsets of every residue mod 4; a
    fifth truncated, a fifth with trailing bytes, some capped, a few with a
    flipped length CRC.  Every result and the whole index arena are the
    judge's."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 32 * cus + 37
    assert n > 32 * cus
    rng = np.random.default_rng(81)
    counts = rng.integers(0, 4, n)
    payload = rng.integers(0, 256, 3 * 40, dtype=np.uint8).tobytes()
    datas, caps, spans, at = [], [], [], 1
    for k in range(n):
        lens = rng.integers(0, 41, int(counts[k])).tolist()
        data, _ = J.frame(payload[:sum(lens)], lens)
        if k % 5 == 1 and lens:
            data = data[:len(data) - int(rng.integers(1, min(20, 16 + lens[-1])))]
        elif k % 5 == 2:
            data += bytes(int(rng.integers(1, 12)))
        if k % 97 == 34 and len(data) > 9:
            data = data[:9] + bytes([data[9] ^ 1]) + data[10:]
        datas.append(data)
        caps.append(len(lens) // 2 if k % 7 == 3 else 4)
        at += (k - at) % 4                        # stream k at a byte offset of residue k mod 4
        spans.append((at, len(data)))
        at += len(data) + 5
    host = np.full(at + 16, POISON, np.uint8)
    for (off, m), data in zip(spans, datas):
        host[off:off + m] = np.frombuffer(data, np.uint8)
    assert {off % 4 for off, _ in spans} == {0, 1, 2, 3}
    src = torch.from_numpy(host).to("cuda:0")
    slot = 16 * 4
    idx = torch.full((16 + slot * n + 16,), POISON, dtype=torch.uint8, device="cuda:0")
    streams = [(off, m, 16 + slot * k, caps[k]) for k, (off, m) in enumerate(spans)]
    walks = gpu_ctx.tfrecord_index_batch(src, streams, idx)
    want = np.full(len(idx), POISON, np.uint8)
    statuses, flipped = set(), 0
    for k, (w, data) in enumerate(zip(walks, datas)):
        j = J.walk(data, caps[k])
        held(w, j)
        statuses.add(w.status)
        flipped += w.bad_length_crc
        e = np.array(j["entries"], "<u8").reshape(-1, 2)
        want[16 + slot * k:16 + slot * k + 16 * len(e)] = e.view(np.uint8).reshape(-1)
    assert statuses == {"complete", "truncated", "full"} and flipped >= 3
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(src.cpu().numpy(), host)


def test_walk_long_chain(S, gpu_ctx, torch):
    """One stream of 20 000 records of 0-9 bytes, so that headers land on every
    alignment: walked whole, then in pieces of at most 4999 records, each
    resumed where the one before stopped.  The pieces' entries, their offsets
    rebased, are the judge's."""
    rng = np.random.default_rng(82)
    lens = rng.integers(0, 10, 20000).tolist()
    data, index = J.frame(rng.integers(0, 256, sum(lens), dtype=np.uint8).tobytes(), lens)
    j = J.walk(data)
    assert j["records"] == 20000 and np.array(j["entries"], "<u8").tobytes() == index
    assert {pos % 16 for pos, _ in j["entries"]} == set(range(16))
    lead = 16
    host = np.full(lead + len(data) + 16, POISON, np.uint8)
    host[lead:lead + len(data)] = np.frombuffer(data, np.uint8)
    src = torch.from_numpy(host).to("cuda:0")
    want = np.full(16 + len(index) + 16, POISON, np.uint8)
    want[16:16 + len(index)] = np.frombuffer(index, np.uint8)
    idx = torch.full((len(want),), POISON, dtype=torch.uint8, device="cuda:0")
    w = gpu_ctx.tfrecord_index_batch(src, [(lead, len(data), 16, 20000)], idx)[0]
    held(w, j)
    assert w.ok and w.records == 20000
    assert np.array_equal(idx.cpu().numpy(), want)
    idx.fill_(POISON)
    at, done, pieces = 0, 0, []
    while True:
        w = gpu_ctx.tfrecord_index_batch(src, [(lead + at, len(data) - at, 16 + 16 * done, 4999)], idx)[0]
        held(w, J.walk(data[at:], 4999))
        pieces.append((w.records, w.status, at))
        if w.status != "full":
            break
        at += w.stop_offset
        done += w.records
    assert [(r, s) for r, s, _ in pieces] == [(4999, "full")] * 4 + [(4, "complete")]
    got = idx.cpu().numpy()
    assert bool((got[:16] == POISON).all()) and bool((got[16 + len(index):] == POISON).all())
    e = got[16:16 + len(index)].view("<u8").reshape(-1, 2).copy()
    for m, (_, _, base) in enumerate(pieces):
        e[4999 * m:4999 * (m + 1), 0] += np.uint64(base)
    assert e.tobytes() == index
