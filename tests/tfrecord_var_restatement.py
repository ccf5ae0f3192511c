"""Judges of the TFRecord calls for records of any length,
written from the format's definition with struct and zlib.crc32 alone:

  frame(payload, lengths)   write_raw_record applied record by record
                            (src/data_formats/tfrecord.rs:14-75): the stream
                            and its DALI index <offset, size>
  walk(data, max_records)   index_entries_from_bytes (src/tfrecord_index.rs:34-80)
                            with the device call's reporting: the silent break
                            below 12 bytes, the truncation offset, max_records

Neither knows anything of the library.  A not-a-test module: the test files
import it.
"""
import struct
import zlib

import numpy as np

MASK_DELTA = 0xA282EAD8
NONE = 2**64 - 1


def masked_crc(crc):
    return ((((crc >> 15) | (crc << 17)) & 0xFFFFFFFF) + MASK_DELTA) & 0xFFFFFFFF


def header(n):
    lb = struct.pack("<Q", n)
    return lb + struct.pack("<I", masked_crc(zlib.crc32(lb)))


def frame(payload, lengths):
    """(stream bytes, index bytes) of the records cut from `payload` back to back."""
    payload = bytes(payload)
    out, idx, at = [], [], 0
    pos = 0
    for n in lengths:
        n = int(n)
        d = payload[at:at + n]
        assert len(d) == n
        out.append(header(n) + d + struct.pack("<I", masked_crc(zlib.crc32(d))))
        idx.append(struct.pack("<QQ", pos, 16 + n))
        at += n
        pos += 16 + n
    return b"".join(out), b"".join(idx)


def frame_np(payload, lengths):
    """frame() as uint8 arrays."""
    st, ix = frame(payload, lengths)
    return np.frombuffer(st, np.uint8), np.frombuffer(ix, np.uint8)


def frame_equal_np(payload, records, rs):
    """frame_np for `records` records of rs bytes each, vectorised over the
    records: for fillers of hundreds of MiB.  Held to frame() by the tests."""
    out = np.empty((records, rs + 16), np.uint8)
    out[:, :12] = np.frombuffer(header(rs), np.uint8)
    data = payload[:records * rs].reshape(records, rs)
    out[:, 12:12 + rs] = data
    foot = np.array([masked_crc(zlib.crc32(data[i])) for i in range(records)], "<u4")
    out[:, 12 + rs:] = foot.view(np.uint8).reshape(records, 4)
    idx = np.empty((records, 2), "<u8")
    idx[:, 0] = np.arange(records, dtype=np.uint64) * np.uint64(rs + 16)
    idx[:, 1] = rs + 16
    return out.reshape(-1), idx.view(np.uint8).reshape(-1)


def walk(data, max_records=NONE):
    """dict(records, status, stop_offset, trailing, bad_length_crc,
    first_bad_record, entries) of a byte string, by the reference's rules:
      * fewer than 12 bytes left: stop silently (status 0);
      * else, with max_records entries written: status 2;
      * else a record whose 12 + len + 4 bytes do not fit: status 1 at its start;
      * the length CRC is looked at but never changes the index."""
    data = bytes(data)
    pos, entries, bad, first, status = 0, [], 0, None, 0
    while True:
        if pos + 12 > len(data):
            break
        if len(entries) == max_records:
            status = 2
            break
        (n,), (lc,) = struct.unpack_from("<Q", data, pos), struct.unpack_from("<I", data, pos + 8)
        if pos + 12 + n + 4 > len(data):   # Python integers: no overflow
            status = 1
            break
        if lc != masked_crc(zlib.crc32(data[pos:pos + 8])):
            bad += 1
            first = len(entries) if first is None else first
        entries.append((pos, 16 + n))
        pos += 16 + n
    return dict(records=len(entries), status=status, stop_offset=pos, trailing=len(data) - pos, bad_length_crc=bad,
                first_bad_record=first, entries=entries)


def index_text(entries):
    return "".join("%d %d\n" % (o, s) for o, s in entries)


def walk_endings(rng_seed=5):
    """The list of endings both the CPU sweep and the GPU test walk:
    (name, bytes, max_records).  Built from three framed records of lengths
    40, 0 and 7 with a fixed payload."""
    payload = bytes((i * 37 + 11) & 0xFF for i in range(47))
    good, _ = frame(payload, [40, 0, 7])
    cases = [("empty", b"", NONE)]
    for t in range(16):
        cases.append((f"trailing_{t}", good + bytes([0x5A] * t), NONE))
    for m in range(1, 21):
        cases.append((f"missing_{m}", good[:len(good) - m], NONE))
    for name, n in (("len_2^32", 1 << 32), ("len_2^63", 1 << 63), ("len_2^64-1", NONE)):
        cases.append((name, good + header(n) + bytes(20), NONE))
    cases.append(("max_0", good, 0))
    cases.append(("max_exact", good, 3))
    cases.append(("max_short", good, 2))
    cases.append(("max_0_short_stream", good[:11], 0))
    return cases
