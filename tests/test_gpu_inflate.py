"""GPU: DEFLATE streams and NPZ archives with deflated members inflated on the
device (Context.inflate_batch, npz_zindex_batch, npz_zunpack_batch; DESIGN.md
§5.5.7).  Every comparison is exact, against zlib (wbits=-15), zipfile and
numpy; destinations lie between poisoned guards and are compared whole."""
import io
import random
import zipfile
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD, POISON = 64, 0xEE
RNG = np.random.default_rng(1951)


def up16(n):
    return (n + 15) & ~15


def rnd(n):
    return RNG.integers(0, 256, n, dtype=np.uint8).tobytes()


def raw(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, sync_every=None):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    if sync_every is None:
        return c.compress(data) + c.flush()
    parts = [c.compress(data[i:i + sync_every]) + c.flush(zlib.Z_SYNC_FLUSH) for i in range(0, len(data), sync_every)]
    return b"".join(parts) + c.flush()


def inflate(ctx, streams, outs, caps=None, wants=None, crcs=None, order=None):
    """One call over items order[j] -> stream index (default: each once), stream
    k at an odd offset, item j's place 16 bytes behind its predecessor's.
    Returns (result, destination, expected destination, places); the place of
    an item that is not "ok" is copied from the destination, so only the bytes
    around it are judged."""
    import torch
    order = list(range(len(streams))) if order is None else order
    offs, at = [], GUARD
    for k, s in enumerate(streams):
        offs.append(at + (k * 7 + 1) % 16)
        at = up16(offs[-1] + len(s)) + 16
    host = np.full(at + GUARD, POISON, np.uint8)
    for o, s in zip(offs, streams):
        host[o:o + len(s)] = np.frombuffer(s, np.uint8)
    items, places, at = [], [], GUARD
    for j, k in enumerate(order):
        cap = len(outs[k]) if caps is None or caps.get(j) is None else caps[j]
        items.append((offs[k], len(streams[k]), at, cap, None if wants is None else wants.get(j), None if crcs is None else crcs.get(j)))
        places.append((at, cap))
        at += up16(cap) + 16
    dst = torch.full((at + GUARD,), POISON, dtype=torch.uint8, device="cuda")
    res = ctx.inflate_batch(torch.from_numpy(host).cuda(), dst, items)
    got, exp = dst.cpu().numpy(), np.full(at + GUARD, POISON, np.uint8)
    for j, k in enumerate(order):
        pos, cap = places[j]
        if res.items[j].status == "ok":
            exp[pos:pos + len(outs[k])] = np.frombuffer(outs[k], np.uint8)
        else:
            exp[pos:pos + cap] = got[pos:pos + cap]
    return res, got, exp, places


def period(p, n):
    return (rnd(p) * (n // p + 1))[:n]


def fib_bytes():
    counts, data = [1, 1], bytearray()
    while len(counts) < 24:
        counts.append(counts[-1] + counts[-2])
    for v, c in enumerate(counts):
        data += bytes([v + 40]) * c
    random.Random(5).shuffle(data)
    return bytes(data)   # 121 392 bytes: Huffman-only codes run past the first-level table


GROUPS = {
    "shortest": lambda: [b"\x03\x00"] + [raw(rnd(n)) for n in (1, 15, 16, 17)],
    "stored": lambda: [raw(d, 0) for n in (0, 1, 65535, 65537) for d in (b"\x5a" * n, rnd(n))],
    "block_types": lambda: [raw(d, lv, st, sy) for d in (b"\x5a" * 5000, rnd(700), period(300, 5000))
                            for lv, st, sy in ((6, zlib.Z_FIXED, None), (1, 0, None), (9, 0, None), (6, 0, 100))],
    "batch_edges": lambda: [raw(d, 6, st) for n in (63, 64, 65) for d in (rnd(n), bytes(range(n))) for st in (0, zlib.Z_HUFFMAN_ONLY)],
    "ring_edges": lambda: [raw(period(1000, n)) for n in (32767, 32768, 32769, 65535, 65536, 65537, 200 * 1024)]
                          + [raw(rnd(40000) + period(77, 30000), 1)],
    "overlap": lambda: [raw(b"\x07" * 70000, 9)] + [raw(period(p, 3000), 9) for p in range(2, 21)],
    "long_codes": lambda: [raw(fib_bytes(), 6, zlib.Z_HUFFMAN_ONLY)],
}


@pytest.mark.parametrize("group", list(GROUPS))
def test_streams(gpu_ctx, group):
    streams = GROUPS[group]()
    outs = [zlib.decompress(s, -15) for s in streams]
    crcs = {j: zlib.crc32(o) for j, o in enumerate(outs)}
    res, got, exp, _ = inflate(gpu_ctx, streams, outs, wants={j: len(o) for j, o in enumerate(outs)}, crcs=crcs)
    assert [r.status for r in res.items] == ["ok"] * len(streams) and res.ok and res.first_item is None
    assert [(r.out_bytes, r.in_bytes) for r in res.items] == [(len(o), len(s)) for o, s in zip(outs, streams)]
    assert np.array_equal(got, exp)


class Bits:
    """A fixed-Huffman block written bit by bit (the only helper of its kind)."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()
        self.put(0b011, 3)   # final, fixed

    def put(self, v, n):     # n bits of v, least significant first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):    # a Huffman code, most significant bit first
        self.put(int(format(v, f"0{n}b")[::-1], 2), n)

    def sym(self, s):
        if s < 144: self.code(0x30 + s, 8)
        elif s < 256: self.code(0x190 + s - 144, 9)
        elif s < 280: self.code(s - 256, 7)
        else: self.code(0xC0 + s - 280, 8)

    def done(self):
        self.sym(256)
        self.put(0, 7)
        return bytes(self.out)


def test_far_match_and_refused_symbols(gpu_ctx):
    """Distance 32 768 with length 258, which zlib never emits; a distance one
    beyond the output's start, length symbol 286 and distance code 30, which
    zlib rejects too."""
    lits, far = rnd(32768), Bits()
    for b in lits:
        far.sym(b)
    far.sym(285), far.code(29, 5), far.put(8191, 13)
    beyond, len286, dist30 = Bits(), Bits(), Bits()
    beyond.sym(65), beyond.sym(66), beyond.sym(257), beyond.code(2, 5)        # length 3 at distance 3 behind 2 bytes
    len286.sym(65), len286.sym(286), len286.code(0, 5)
    dist30.sym(65), dist30.sym(257), dist30.code(30, 5)
    streams = [far.done(), beyond.done(), len286.done(), dist30.done()]
    outs = [lits + lits[:258], b"", b"", b""]
    assert zlib.decompress(streams[0], -15) == outs[0]
    for s in streams[1:]:
        with pytest.raises(zlib.error):
            zlib.decompress(s, -15)
    res, got, exp, _ = inflate(gpu_ctx, streams, outs, caps={1: 64, 2: 64, 3: 64})
    assert [r.status for r in res.items] == ["ok", "bad_stream", "bad_stream", "bad_stream"] and res.first_item == 1
    assert np.array_equal(got, exp)


def test_mixed_call(gpu_ctx):
    """300 items in any order, with repeats and shared sources; one place a
    byte short, one size a byte too many, one wrong CRC."""
    streams = [raw(d, lv) for lv in (0, 1, 6) for d in (rnd(333), period(9, 4000), b"", period(500, 40000), bytes(range(256)) * 3)]
    outs = [zlib.decompress(s, -15) for s in streams]
    order = [int(k) for k in RNG.integers(0, len(streams), 300)]
    order[100], order[200], order[250] = 3, 1, 4
    crcs = {j: zlib.crc32(outs[k]) for j, k in enumerate(order)}
    crcs[250] ^= 1
    res, got, exp, _ = inflate(gpu_ctx, streams, outs, caps={100: len(outs[3]) - 1}, wants={200: len(outs[1]) + 1}, crcs=crcs, order=order)
    status = ["ok"] * 300
    status[100], status[200] = "capacity", "size"
    assert [r.status for r in res.items] == status and res.status == "size"
    assert [j for j, r in enumerate(res.items) if r.bad_crc] == [250] and res.bad_crc == 1 and res.first_item == 100
    assert np.array_equal(got, exp)


@pytest.fixture(scope="module")
def small():
    data = bytes(random.Random(3).choices(b"etaoin shrdlu\n", weights=range(1, 15), k=420))
    s = raw(data, 9)
    assert 150 < len(s) < 260 and s[0] & 7 == 5   # one dynamic block, the final one
    return s, data


def test_prefix_cuts(gpu_ctx, small):
    s, data = small
    streams = [s[:n] for n in range(len(s))]
    res, got, exp, _ = inflate(gpu_ctx, streams, [data] * len(streams))
    assert {r.status for r in res.items} == {"truncated"} and res.status == "truncated"
    assert np.array_equal(got, exp)


def test_bit_flips(gpu_ctx, small):
    """Every single-bit flip: "ok" and zlib's bytes exactly where zlib reaches
    the stream's end within the place, some other status everywhere else."""
    s, data = small
    cap, streams, outs, ok = len(data) + 300, [], [], []
    for bit in range(8 * len(s)):
        f = bytearray(s)
        f[bit // 8] ^= 1 << (bit % 8)
        d = zlib.decompressobj(-15)
        try:
            o = d.decompress(bytes(f), cap + 1)
            ok.append(d.eof and len(o) <= cap)
        except zlib.error:
            o = b""
            ok.append(False)
        streams.append(bytes(f))
        outs.append(o if ok[-1] else b"")
    res, got, exp, _ = inflate(gpu_ctx, streams, outs, caps={j: cap for j in range(len(streams))})
    assert [r.status == "ok" for r in res.items] == ok and 0 < sum(ok) < len(ok)
    assert np.array_equal(got, exp)


def test_npz(gpu_ctx):
    import torch
    import s3dlio_amd as S
    arrays = {"a": RNG.standard_normal(3000).astype(np.float32), "b": np.arange(21, dtype=np.uint8).reshape(3, 7), "c": np.empty(0)}
    bio = io.BytesIO()
    np.savez_compressed(bio, **arrays)
    mixed = io.BytesIO()
    with zipfile.ZipFile(mixed, "w") as zf:
        zf.writestr("s0.bin", rnd(1000), zipfile.ZIP_STORED)
        zf.writestr("d1.bin", period(50, 70000), zipfile.ZIP_DEFLATED)
        zf.writestr("s2.bin", b"", zipfile.ZIP_STORED)
        zf.writestr("d3.bin", rnd(100) * 9, zipfile.ZIP_DEFLATED)
    blobs, offs = [bio.getvalue(), mixed.getvalue()], [GUARD, 0]
    offs[1] = up16(offs[0] + len(blobs[0])) + 16 + 5   # an odd byte offset
    host = np.full(offs[1] + len(blobs[1]) + GUARD, POISON, np.uint8)
    for o, b in zip(offs, blobs):
        host[o:o + len(b)] = np.frombuffer(b, np.uint8)
    infos = [zipfile.ZipFile(io.BytesIO(b)).infolist() for b in blobs]
    src, table = torch.from_numpy(host).cuda(), torch.full((3 * 256,), POISON, dtype=torch.uint8, device="cuda")
    walks = gpu_ctx.npz_zindex_batch(src, [(offs[0], len(blobs[0]), 0, 8), (offs[1], len(blobs[1]), 256, 8)], table)
    assert [(w.status, w.members) for w in walks] == [("complete", 3), ("complete", 4)]
    assert gpu_ctx.npz_index_batch(src, [(offs[0], len(blobs[0]), 512, 8)], table)[0].status == "unsupported"
    files = []
    for k, (blob, zis) in enumerate(zip(blobs, infos)):
        ents = S.npz_zentries(table, 256 * k, len(zis))
        assert [(e.local_off, e.name_len, e.flags, e.csize, e.usize, e.crc, e.method) for e in ents] == \
               [(z.header_offset, len(z.filename), z.flag_bits, z.compress_size, z.file_size, z.CRC, z.compress_type) for z in zis]
        assert walks[k].payload_bytes == sum(z.file_size for z in zis) and walks[k].packed_bytes == sum(up16(z.file_size) for z in zis)
        with zipfile.ZipFile(io.BytesIO(blob)) as zf:
            files.append([zf.read(z) for z in zis])
    assert np.array_equal(np.load(io.BytesIO(files[0][0])), arrays["a"])

    def unpack(takes, source=src, tab=table):
        at, rows = GUARD, []
        for k, first, count, cap in takes:
            span = sum(up16(len(f)) for f in files[k][first:first + count])
            rows.append((offs[k], len(blobs[k]), 256 * k, first, count, at, span if cap is None else cap))
            at += up16(span) + 16
        dst = torch.full((at + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        res = gpu_ctx.npz_zunpack_batch(source, tab, dst, rows)
        exp = np.full(at + GUARD, POISON, np.uint8)
        for (k, first, count, _), row, r in zip(takes, rows, res.takes):
            pos = row[5]
            for f in files[k][first:first + count] if r.status == "taken" else []:
                exp[pos:pos + len(f)] = np.frombuffer(f, np.uint8)
                pos += up16(len(f))
        return res, dst.cpu().numpy(), exp

    res, got, exp = unpack([(1, 0, 4, None), (0, 0, 3, None), (1, 1, 2, None), (0, 2, 1, None), (1, 1, 1, 69999)])
    assert [t.status for t in res.takes] == ["taken", "taken", "taken", "taken", "capacity"] and res.bad_crc == res.bad_stream == 0
    assert res.members == 10 and res.bytes == sum(map(len, files[1])) + sum(map(len, files[0])) + len(files[1][1]) + len(files[0][2])
    assert np.array_equal(got, exp)
    # one flipped bit in member 3's compressed data: that take and member only
    e3 = S.npz_zentries(table, 256, 4)[3]
    hurt = host.copy()
    hurt[offs[1] + e3.data_off + e3.csize // 2] ^= 0x10
    res, got, exp = unpack([(1, 0, 3, None), (1, 2, 2, None), (0, 0, 3, None)], source=torch.from_numpy(hurt).cuda())
    assert res.bad_crc + res.bad_stream == 1 and (res.first_take, res.first_member) == (1, 3)
    assert [t.bad_crc + t.bad_stream for t in res.takes] == [0, 1, 0]
    pos = GUARD + up16(sum(up16(len(f)) for f in files[1][:3])) + 16 + up16(len(files[1][2]))
    exp[pos:pos + up16(len(files[1][3]))] = got[pos:pos + up16(len(files[1][3]))]   # the hurt member's own place
    assert np.array_equal(got, exp)
    # a tampered entry: csize reaches past the archive
    bad = table.clone()
    bad[256 + 32 + 12:256 + 32 + 16] = torch.tensor([0xFF, 0xFF, 0xFF, 0x7F], dtype=torch.uint8, device="cuda")
    res, got, exp = unpack([(1, 0, 2, None), (0, 0, 3, None)], tab=bad)
    assert [t.status for t in res.takes] == ["table", "taken"] and res.status == "table"
    assert np.array_equal(got, exp)
