"""GPU: NPZ archives indexed from their bytes and unpacked by that index
(Context.npz_index_batch, Context.npz_unpack_batch).  Every
comparison is exact, against zipfile, zlib.crc32 and numpy.load; destinations
lie between poisoned guards and are compared whole."""
import io
import struct
import zipfile
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REGION = 32 * 1024        # the region of a small call: 32 rows of 1024 bytes
GUARD, POISON = 64, 0xEE
SIZES = (*range(71), 1023, 1024, 1025, REGION - 1, REGION, REGION + 1, 2 * REGION + 17, 3 * REGION + 5)


def up16(n):
    return (n + 15) & ~15


class Placed:
    """Archives (bytes) in one poisoned device buffer, archive k at a multiple
    of 16 plus residues[k], indexed in one call with room for `cap` members."""

    def __init__(self, ctx, blobs, residues=None, cap=8):
        import torch
        self.ctx, self.blobs, self.spans, at = ctx, blobs, [], GUARD
        for k, b in enumerate(blobs):
            off = at + (residues[k] if residues else 0)
            self.spans.append((off, len(b)))
            at = up16(off + len(b)) + 16
        host = np.full(at + GUARD, POISON, np.uint8)
        for (off, n), b in zip(self.spans, blobs):
            host[off:off + n] = np.frombuffer(b, np.uint8)
        self.src = torch.from_numpy(host).cuda()
        self.table = torch.full((32 * cap * len(blobs),), POISON, dtype=torch.uint8, device="cuda")
        self.tab_off = [32 * cap * k for k in range(len(blobs))]
        self.walks = ctx.npz_index_batch(self.src, [(off, n, t, cap) for (off, n), t in zip(self.spans, self.tab_off)], self.table)

    def entries(self, k):
        import s3dlio_amd as S
        return S.npz_entries(self.table, self.tab_off[k], self.walks[k].members)

    def unpack(self, picks, caps=None):
        """picks: (archive, first, count) per take, packed one behind the other
        16 bytes apart.  Returns (result, whole destination, expected destination)."""
        import torch
        takes, at, want = [], GUARD, []
        for t, (k, first, count) in enumerate(picks):
            ents = self.entries(k)[first:first + count]
            span = sum(up16(e.size) for e in ents)
            cap = span if caps is None or caps[t] is None else caps[t]
            takes.append((*self.spans[k], self.tab_off[k], first, count, at, cap))
            pos = at
            for e in ents:
                o = self.spans[k][0] + e.data_off
                want.append((t, pos, o, e.size))
                pos += up16(e.size)
            at += up16(span) + 16
        dst = torch.full((at + GUARD,), POISON, dtype=torch.uint8, device="cuda")
        res = self.ctx.npz_unpack_batch(self.src, self.table, dst, takes)
        exp, host = np.full(at + GUARD, POISON, np.uint8), self.src.cpu().numpy()
        for t, pos, o, size in want:
            if res.takes[t].status == "taken":
                exp[pos:pos + size] = host[o:o + size]
        return res, dst.cpu().numpy(), exp


def reference_entries(blob):
    """(local_off, name, flags, hdr_off, hdr_len, data_off, size, crc) per member from zipfile and the NPY preamble."""
    out = []
    with zipfile.ZipFile(io.BytesIO(blob)) as zf:
        for zi in zf.infolist():
            nl, xl = struct.unpack_from("<HH", blob, zi.header_offset + 26)
            at, stored, hl = zi.header_offset + 30 + nl + xl, zf.read(zi), 0
            if stored[:6] == b"\x93NUMPY":
                hl = 10 + struct.unpack_from("<H", stored, 8)[0] if stored[6] == 1 else 12 + struct.unpack_from("<I", stored, 8)[0]
            out.append((zi.header_offset, zi.filename.encode(), zi.flag_bits, at, hl, at + hl, zi.file_size - hl, zi.CRC))
    return out


def savez(compressed=False, **arrays):
    f = io.BytesIO()
    (np.savez_compressed if compressed else np.savez)(f, **arrays)
    return f.getvalue()


def stored_zip(payload, comment=b"", name="x.npy"):
    f = io.BytesIO()
    with zipfile.ZipFile(f, "w", zipfile.ZIP_STORED) as zf:
        zf.writestr(name, payload)
        zf.comment = comment
    return f.getvalue()


SAVED = (savez(a=np.arange(7, dtype="<f4"), b=np.arange(33, dtype="|u1"), c=np.array([-1, 2, 3], "<i8")),
         savez(z=np.array(5.0, "<f4"), e=np.zeros((0, 3), "<f4"), m=(np.arange(1000) % 251).astype("|u1")))


@pytest.fixture(scope="module")
def foreign(gpu_ctx):
    return Placed(gpu_ctx, [SAVED[k % 2] for k in range(32)], [k // 2 for k in range(32)])


def test_archives_nobody_framed_here(foreign, gpu_ctx):
    for k, w in enumerate(foreign.walks):
        ref = reference_entries(SAVED[k % 2])
        assert w.ok and w.members == w.members_total == 3 and w.bad_member is None
        assert [(e.local_off, e.flags, e.hdr_off, e.hdr_len, e.data_off, e.size, e.crc) for e in foreign.entries(k)] == \
            [(r[0], r[2], *r[3:]) for r in ref]
        assert w.payload_bytes == sum(r[6] for r in ref) and w.packed_bytes == sum(up16(r[6]) for r in ref)
    res, got, exp = foreign.unpack([(k, 0, 3) for k in range(32)])
    assert res.ok and res.members == 96 and np.array_equal(got, exp)
    at = GUARD   # the stated packed offsets against numpy.load
    for k in range(32):
        for name, arr in np.load(io.BytesIO(SAVED[k % 2])).items():
            assert got[at:at + arr.nbytes].tobytes() == arr.tobytes()
            at += up16(arr.nbytes)
        at += 16
    for k in (0, 31):
        off, n = foreign.spans[k]
        ref = reference_entries(SAVED[k % 2])
        assert gpu_ctx.npz_list(foreign.src, off, n) == [(r[1], SAVED[k % 2][r[3]:r[5]], r[6]) for r in ref]


@pytest.fixture(scope="module")
def framed(gpu_ctx):
    """npz_frame_batch's archives, copied back: one member per size with name
    lengths 1..16 in both styles, then the mixed cases."""
    import torch
    import s3dlio_amd as S
    rng = np.random.default_rng(11)
    src = rng.integers(0, 256, 4 * REGION + 4096, dtype=np.uint8)
    specs = [([("n" * (1 + k % 16), S.npy_header([s], "|u1"), 16 * (k % 9), s)], k % 2) for k, s in enumerate(SIZES)]
    specs += [([("zeros.npy", S.npy_header([50], "|u1"), None, 50), ("raw.bin", b"", 48, 777),
                ("w.npy", S.npy_header([REGION + 5], "|u1"), 64, REGION + 5)], 0),
              ([("p.npy", S.npy_header([3], "<i8"), 0, 24), ("q.npy", S.npy_header([1000], "|u1"), 16, 1000)], 1)]
    sizes = [S.npz_archive_size(m) for m, _ in specs]
    offs = np.concatenate([[0], np.cumsum([up16(n) for n in sizes])])
    dst = torch.zeros(int(offs[-1]), dtype=torch.uint8, device="cuda")
    gpu_ctx.npz_frame_batch(torch.from_numpy(src).cuda(), dst, [(int(o), m, st) for o, (m, st) in zip(offs, specs)])
    torch.cuda.synchronize()
    host = dst.cpu().numpy()
    blobs = [host[int(o):int(o) + n].tobytes() for o, n in zip(offs, sizes)]
    return Placed(gpu_ctx, blobs), specs, src


def test_the_loop(framed):
    placed, specs, src = framed
    assert all(w.ok and w.members == len(m) for w, (m, _) in zip(placed.walks, specs))
    assert {(placed.spans[k][0] + placed.entries(k)[0].data_off) % 16 for k in range(len(SIZES))} == set(range(16))
    n = len(SIZES)
    picks = [(k, 0, len(m)) for k, (m, _) in enumerate(specs)]            # every archive whole, two and more in one call
    picks += [(n, 2, 1), (n, 0, 1), (n, 2, 1), (n, 1, 2), (n + 1, 0, 0), (n + 1, 1, 1)]   # picks with repeats, a middle run, an empty take
    res, got, exp = placed.unpack(picks)
    assert res.ok and res.members == n + 5 + 6 and np.array_equal(got, exp)
    at = GUARD   # ... and the sources themselves
    for members, _ in specs:
        for _, _, so, size in members:
            assert got[at:at + size].tobytes() == (bytes(size) if so is None else src[so:so + size].tobytes())
            at += up16(size)
        at += 16


def flip(blob, byte, bit=0):
    b = bytearray(blob)
    b[byte] ^= 1 << bit
    return bytes(b)


def test_one_flipped_bit_per_place(gpu_ctx):
    import s3dlio_amd as S
    sa, sb = 1000, 3 * REGION + 5
    ha, hb = S.npy_header([sa], "|u1"), S.npy_header([sb], "|u1")
    pa, pb = bytes(range(256)) * 4, (np.arange(sb) % 253).astype(np.uint8).tobytes()
    f = io.BytesIO()
    with zipfile.ZipFile(f, "w", zipfile.ZIP_STORED) as zf:
        zf.writestr("a.npy", ha + pa[:sa])
        zf.writestr("bb.npy", hb + pb)
    good = f.getvalue()
    (la, _, _, fa, _, da, _, _), (_, _, _, fb, _, db, _, _) = reference_entries(good)
    with zipfile.ZipFile(io.BytesIO(good)) as zf:
        cd = zf.start_dir
    end = len(good) - 22
    places = [None, da + 500, db + 2 * REGION + 4000, fb + 30, la + 14, la + 30, la + 18, cd + 20, end + 10, end + 16]
    placed = Placed(gpu_ctx, [good if p is None else flip(good, p) for p in places], [k % 16 for k in range(len(places))])
    assert [(w.status, w.bad_member) for w in placed.walks] == \
        [("complete", None)] * 4 + [("local", 0)] * 3 + [("directory", 0), ("directory", None), ("directory", None)]
    res, got, exp = placed.unpack([(k, 0, 2) for k in range(4)])
    assert np.array_equal(got, exp)   # delivered as they stand
    assert [(t.status, t.bad_crc, t.first_member) for t in res.takes] == \
        [("taken", 0, None), ("taken", 1, 0), ("taken", 1, 1), ("taken", 1, 1)]
    assert (res.bad_crc, res.first_take, res.first_member, res.ok) == (3, 1, 0, False)


@pytest.mark.parametrize("comment", [b"", b"c", b"c" * 63, b"c" * 64, b"c" * 65, b"c" * 65535, b"PK\x05\x06" + bytes(30)],
                         ids=["0", "1", "63", "64", "65", "65535", "decoy"])
def test_end_record(gpu_ctx, comment):
    payload = b"\x93NUMPY\x01\x00\x06\x00{'x'}\n" + b"PK\x05\x06" + bytes(18) + b"tail"   # a decoy inside the payload too
    blob = stored_zip(payload, comment)
    placed = Placed(gpu_ctx, [blob, blob[:-1]], [5, 9])
    full, cut = placed.walks
    assert full.ok and full.members == 1 and cut.status == "no_end" and cut.members == cut.members_total == 0
    (e,), (r,) = placed.entries(0), reference_entries(stored_zip(payload))   # zipfile itself takes the comment's decoy
    assert (e.local_off, e.hdr_off, e.hdr_len, e.size, e.crc) == (r[0], r[3], 16, len(payload) - 16, zlib.crc32(payload))
    res, got, exp = placed.unpack([(0, 0, 1)])
    assert res.ok and np.array_equal(got, exp)


def test_other_cases(gpu_ctx):
    import torch
    placed = Placed(gpu_ctx, [savez(True, a=np.arange(100)), SAVED[0], SAVED[1]], [3, 0, 7], cap=2)
    assert [(w.status, w.members, w.members_total, w.bad_member) for w in placed.walks] == \
        [("unsupported", 0, 1, 0), ("capped", 2, 3, None), ("capped", 2, 3, None)]
    span = sum(up16(e.size) for e in placed.entries(1))
    res, got, exp = placed.unpack([(1, 0, 2), (1, 0, 2), (1, 0, 2)], caps=[None, span - 1, None])   # one byte short beside exact neighbours
    assert [(t.status, t.span, t.members) for t in res.takes] == [("taken", span, 2), ("capacity", span, 0), ("taken", span, 2)]
    assert res.status == "capacity" and np.array_equal(got, exp)
    raw = placed.table.cpu().numpy().copy()   # an entry whose size leaves the archive
    raw[placed.tab_off[2] + 32 + 20:placed.tab_off[2] + 32 + 24] = np.frombuffer(struct.pack("<I", len(SAVED[1])), np.uint8)
    placed.table.copy_(torch.from_numpy(raw))
    res, got, exp = placed.unpack([(1, 0, 2), (2, 0, 2), (1, 1, 1)])
    assert [t.status for t in res.takes] == ["taken", "table", "taken"] and np.array_equal(got, exp) and res.members == 3


def test_refusals(gpu_ctx, foreign):
    ps, pt, big = foreign.src.data_ptr(), foreign.table.data_ptr(), 2**64 - 1
    po, good = ps, (64, 64, 0, 0, 1, 0, 64)
    for args, msg in [((0, pt, po, [good]), "null base"), ((ps, 0, po, [good]), "null table"), ((ps, pt, 0, [good]), "null dst_base"),
                      ((ps, pt + 8, po, [good]), "table must be 16-byte aligned"),
                      ((ps, pt, po + 8, [good]), "dst_base must be 16-byte aligned"),
                      ((ps, pt, po, [good, (64, 64, 8, 0, 1, 0, 64)]), "take 1: tab_off must be a multiple of 16"),
                      ((ps, pt, po, [good, (64, 64, 0, 0, 1, 8, 64)]), "take 1: dst_off must be a multiple of 16"),
                      ((ps, pt, po, [(64, 64, 0, big, 2, 0, 64)]), "take 0: first + count overflows"),
                      ((ps, pt, po, [(big, 64, 0, 0, 1, 0, 64)]), "take 0: off + bytes overflows"),
                      ((ps, pt, po, [(64, 64, 0, 0, 1, big - 15, 64)]), "take 0: dst_off + dst_cap overflows"),
                      ((ps, pt, po, [(64, 64, 0, 0, 2**31, 0, 64)]), "take 0: more than 2^31 - 2 members in one call"),
                      ((ps, pt, po, [good, (64, 2**47, 0, 0, 1, 0, 2**47)]), "take 1: more than 2^46 archive bytes in one call")]:
        with pytest.raises(ValueError) as e:
            gpu_ctx.npz_unpack_batch(*args)
        assert str(e.value) == msg
    for args, msg in [((0, pt, [(64, 64, 0, 1)]), "null base"), ((ps, pt + 8, [(64, 64, 0, 1)]), "table must be 16-byte aligned"),
                      ((ps, pt, [(64, 64, 8, 1)]), "archive 0: tab_off must be a multiple of 16"),
                      ((ps, pt, [(64, 2**32, 0, 1)]), "archive 0: an archive of 2^32 bytes or more (no ZIP64)")]:
        with pytest.raises(ValueError) as e:
            gpu_ctx.npz_index_batch(args[0], args[2], args[1])
        assert str(e.value) == msg
    assert gpu_ctx.npz_unpack_batch(0, 0, 0, []).ok and gpu_ctx.npz_index_batch(0, [], 0) == []
