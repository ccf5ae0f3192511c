// tfrecord_plan_sweep.cpp — s3dg_tfrecord_plan.h on its own (g++, no HIP).  The
// program walks shards the way the kernels do (tfr_find_region, tfr_region,
// tfr_region_span, the framing bytes, tfr_crc_one / tfr_crc_fold), on the host
// and byte by byte, over swept record sizes, record counts, region sizes and
// both forms (the frame form meets all 16 source alignments, the check form
// all 16 stream alignments), and asserts:
//   * every byte of a stream has exactly one writer, none outside it;
//   * every byte of the source has exactly one reader, and the bytes a wave
//     masks lie inside the shard;
//   * a region never spans two records, only a record's last region has a tail;
//   * the fold of the padded record's raw CRCs is the bit-by-bit CRC-32 of the
//     record's data, and the stream is the definition's;
//   * the refusals and their messages, the table's size and the two searches.
// It prints what tests/test_tfrecord_cpu.py compares with zlib.crc32.
#include <assert.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "s3dg_tfrecord_plan.h"

using namespace s3dg;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static const uint64_t kBase = 0x7000000000ull;
static uint64_t shards_walked = 0, records_folded = 0;

// bit by bit, from the definition: the judge
static uint32_t raw_bitwise(uint32_t reg, const uint8_t *p, uint64_t n) {
    for (uint64_t i = 0; i < n; ++i) {
        reg ^= p[i];
        for (int b = 0; b < 8; ++b) reg = (reg & 1) ? (reg >> 1) ^ 0xEDB88320u : reg >> 1;
    }
    return reg;
}
static uint32_t crc32_bitwise(const uint8_t *p, uint64_t n) { return ~raw_bitwise(0xFFFFFFFFu, p, n); }
static uint32_t masked(uint32_t c) { return (uint32_t)((((uint64_t)c >> 15) | ((uint64_t)c << 17)) + 0xA282EAD8ull); }

static void put32(std::vector<uint8_t> &v, uint32_t x) {
    for (int b = 0; b < 4; ++b) v.push_back((uint8_t)(x >> (8 * b)));
}
// build_tfrecord_with_index from its definition
static std::vector<uint8_t> reference_stream(const uint8_t *data, uint64_t records, uint64_t rs) {
    std::vector<uint8_t> out;
    for (uint64_t i = 0; i < records; ++i) {
        uint8_t lb[8];
        for (int b = 0; b < 8; ++b) lb[b] = (uint8_t)(rs >> (8 * b));
        out.insert(out.end(), lb, lb + 8);
        put32(out, masked(crc32_bitwise(lb, 8)));
        out.insert(out.end(), data + i * rs, data + (i + 1) * rs);
        put32(out, masked(crc32_bitwise(data + i * rs, rs)));
    }
    return out;
}

// One shard at the call region `rows`, walked as the kernels walk it.  frame:
// payload -> stream, with writers and readers counted; check: the stream is
// read back and every record's framing must compare equal.
static std::vector<uint8_t> walk(const std::vector<uint8_t> &payload, uint64_t records, uint64_t rs, uint32_t rows) {
    const s3dg_tfrecord_shard d{0, 0, 0, records, rs};
    TfrCounts C;
    std::string why;
    bool ok = tfr_check(true, kBase, kBase + (1ull << 40), 0, &d, 1, &C, &why);
    assert(ok && C.live == 1);
    C.rows = rows;   // the sweep's own region, whatever the call would pick
    TfrShard E;
    tfr_build(&d, 1, C, &E);
    assert(E.rows >= rows && E.rpr >= 1 && E.rpr <= kCrcBatchMaxRegions && E.k == 0 && E.reg0 == 0);
    assert(E.len_mcrc == tfr_len_mcrc(rs) && E.init == crcb_multmodp(crcb_x8n(rs), 0xFFFFFFFFu));
    uint64_t framed = 0;
    ok = tfr_size(records, rs, &framed);
    assert(ok && framed == records * (rs + 16));
    const std::vector<uint8_t> want = reference_stream(payload.data(), records, rs);
    assert(want.size() == framed);
    std::vector<uint8_t> stream(framed, 0xEE);
    for (int form = 0; form < 2; ++form) {
        const bool frame = form == 0;
        const std::vector<uint8_t> &in = frame ? payload : stream;
        std::vector<uint8_t> writers(framed, 0), readers(frame ? records * rs : 0, 0);
        std::vector<uint32_t> raw(E.rpr);
        for (uint64_t i = 0; i < records; ++i) {
            uint64_t next_lo = 0, a = 0, out = 0;
            for (uint32_t g = 0; g < E.rpr; ++g) {
                const uint64_t q = i * E.rpr + g;
                assert(tfr_find_region(&E, 1, q) == 0);
                const TfrRegion R = tfr_region(E, q, frame);
                assert(R.rec == i && R.g == g && R.a < 16 && R.tail < 1024 && R.nrows <= E.rows);
                assert(R.a == (frame ? (i * rs) % 16 : (12 + i * rs) % 16) && R.a == tfr_align(frame, i, rs));
                assert(R.out == i * (rs + 16) && R.data == (frame ? i * rs : R.out + 12));
                assert(R.data >= R.a && (R.data - R.a) % 16 == 0);       // the masked bytes lie inside the shard
                if (frame) assert((R.out + 12 - R.a) % 16 == 12);        // the stores are dword-aligned 16-byte ones
                assert(R.pad_lo == (uint64_t)g * E.rows * 1024);
                if (g + 1 < E.rpr) assert(R.nrows == E.rows && R.tail == 0);
                else assert(R.pad_lo + (uint64_t)R.nrows * 1024 + R.tail == R.a + rs);
                uint64_t lo, hi;
                tfr_region_span(R, &lo, &hi);
                assert(lo == next_lo && hi >= lo && hi <= rs);           // in order, inside the record
                next_lo = hi;
                // the wave's hash: the padded bytes, the first a of them zero
                std::vector<uint8_t> pad((uint64_t)R.nrows * 1024 + R.tail);
                for (uint64_t y = 0; y < pad.size(); ++y) {
                    const uint64_t py = R.pad_lo + y;
                    pad[y] = py < R.a ? 0 : in[R.data + (py - R.a)];
                }
                raw[g] = raw_bitwise(0, pad.data(), pad.size());
                for (uint64_t x = lo; x < hi; ++x) {
                    if (frame) {
                        ++readers[R.data + x];
                        ++writers[R.out + 12 + x];
                        stream[R.out + 12 + x] = in[R.data + x];
                    }
                }
                a = R.a;
                out = R.out;
            }
            assert(next_lo == rs);
            const uint32_t crc = E.rpr == 1 ? tfr_crc_one(raw[0], E.init) : tfr_crc_fold(raw.data(), E.rpr, E.rows, (uint32_t)a, rs, E.init);
            assert(crc == crc32_bitwise(in.data() + (frame ? i * rs : out + 12), rs));
            assert(tfr_masked(crc) == masked(crc));
            ++records_folded;
            for (uint32_t l = 0; l < 16; ++l) {
                const uint64_t at = out + tfr_framing_at(l, rs);
                const uint8_t b = (uint8_t)tfr_framing_byte(l, rs, E.len_mcrc, tfr_masked(crc));
                if (frame) {
                    ++writers[at];
                    stream[at] = b;
                } else {
                    assert(stream[at] == b);   // a clean stream compares equal
                }
            }
        }
        if (frame) {
            for (uint8_t w : writers) assert(w == 1);
            for (uint8_t r : readers) assert(r == 1);
            assert(stream == want);
        }
    }
    ++shards_walked;
    return stream;
}

static void expect_refusal(bool frame, uint64_t src, uint64_t dst, uint64_t idx, std::vector<s3dg_tfrecord_shard> v, const char *msg) {
    TfrCounts C;
    std::string why;
    const bool ok = tfr_check(frame, src, dst, idx, v.data(), v.size(), &C, &why);
    if (ok || why != msg) fprintf(stderr, "expected \"%s\", got %s \"%s\"\n", msg, ok ? "success" : "refusal", why.c_str());
    assert(!ok && why == msg);
}

int main() {
    static_assert(sizeof(TfrShard) == 88 && sizeof(s3dg_tfrecord_shard) == 40 && sizeof(s3dg_tfrecord_result) == 56, "layout");
    std::vector<uint8_t> payload(600 * 1024);
    for (uint8_t &b : payload) b = (uint8_t)(rnd() >> 32);
    // ---- every small size, enough records to meet all 16 alignments ---------------
    for (uint64_t rs = 0; rs <= 70; ++rs) walk(payload, 17, rs, 32);
    for (uint64_t rs = 1000; rs <= 1060; ++rs) walk(payload, 17, rs, 32);
    // ---- sizes around a row, a region and several regions, at several regions ------
    for (uint32_t rows : {1u, 2u, 3u, 5u, 32u}) {
        const uint64_t region = (uint64_t)rows * 1024;
        for (uint64_t m : {1ull, 2ull, 3ull}) {
            for (int d = -17; d <= 17; ++d) {
                const uint64_t rs = m * region + d;
                if (rs * 17 > payload.size()) continue;
                walk(payload, 17, rs, rows);
            }
            for (uint64_t d : {1024ull, 1025ull}) {
                if ((m * region + d) * 17 <= payload.size()) walk(payload, 17, m * region + d, rows);
                if (m * region > d && (m * region - d) * 17 <= payload.size()) walk(payload, 17, m * region - d, rows);
            }
        }
    }
    for (int k = 0; k < 60; ++k) walk(payload, 1 + rnd() % 20, rnd() % 20000, 1 + (uint32_t)(rnd() % 6));
    walk(payload, 0 + 1, 0, 32);
    {   // content the algebra could hide a slip behind
        std::vector<uint8_t> z(40 * 1024, 0), f(40 * 1024, 0xFF);
        for (uint64_t rs : {1ull, 15ull, 16ull, 1023ull, 2049ull}) {
            walk(z, 17, rs, 1);
            walk(f, 17, rs, 1);
        }
    }
    // ---- regions per record: the longest padded record decides, the cap doubles -------
    assert(tfr_shard_rpr(0, 32) == 1 && tfr_shard_rpr(32 * 1024 - 15, 32) == 1 && tfr_shard_rpr(32 * 1024 - 14, 32) == 1);
    assert(tfr_shard_rpr(32 * 1024 + 1024 - 15, 32) == 2 && tfr_shard_rpr(64ull << 20, 32) == 2048);
    assert(tfr_shard_rows(128ull << 20, 32) == 32 && tfr_shard_rpr(128ull << 20, 32) == 4096);
    assert(tfr_shard_rows((128ull << 20) + 1024 - 15, 32) == 64 && tfr_shard_rpr((128ull << 20) + 1024 - 15, 64) == 2049);
    assert(tfr_shard_rpr(kTfrMaxRecord, tfr_shard_rows(kTfrMaxRecord, 256)) <= kCrcBatchMaxRegions);
    // ---- a call: entries, prefixes, the two searches, the table's size ----------------
    {
        std::vector<s3dg_tfrecord_shard> v = {{0, 0, 0, 1000, 100},          {1 << 20, 1 << 21, 16000, 0, 77},
                                              {2 << 20, 3 << 21, 32000, 3, 70000}, {0, 5 << 21, 48000, 1000, 100},
                                              {4 << 20, 7 << 21, 64000, 5, 0},     {5 << 20, 9 << 21, 80000, 2, 40000}};
        TfrCounts C;
        std::string why;
        const bool ok = tfr_check(true, kBase, kBase + (1ull << 40), kBase + (1ull << 41), v.data(), v.size(), &C, &why);
        assert(ok && C.live == 5 && C.rows == 32 && C.total_rows == 3 * 68 + 2 * 39);
        assert(tfr_table_bytes(C) == 5 * 88 && tfr_raw_offset(C) % 256 == 0 && tfr_device_bytes(C) == tfr_raw_offset(C) + 4 * C.raw_slots);
        std::vector<TfrShard> e(C.live + 1, TfrShard{0xEEEE, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
        tfr_build(v.data(), v.size(), C, e.data());
        assert(e[C.live].src_off == 0xEEEE);
        assert(e[0].k == 0 && e[1].k == 2 && e[2].k == 3 && e[3].k == 4 && e[4].k == 5);
        assert(e[1].rpr == 3 && e[4].rpr == 2 && e[0].rpr == 1 && e[3].rpr == 1);
        assert(C.regions == 1000 + 9 + 1000 + 5 + 4 && C.long_records == 5 && C.raw_slots == 13);
        uint64_t reg = 0, lrec = 0, raw = 0;
        for (uint64_t j = 0; j < C.live; ++j) {
            assert(e[j].reg0 == reg && e[j].lrec0 == lrec && e[j].raw0 == raw);
            for (uint64_t q = 0; q < e[j].records * e[j].rpr; ++q) assert(tfr_find_region(e.data(), (uint32_t)C.live, reg + q) == j);
            if (e[j].rpr > 1) {
                for (uint64_t i = 0; i < e[j].records; ++i) assert(tfr_find_long(e.data(), (uint32_t)C.live, lrec + i) == j);
                lrec += e[j].records;
                raw += e[j].records * e[j].rpr;
            }
            reg += e[j].records * e[j].rpr;
        }
        // a million records are one entry
        const s3dg_tfrecord_shard big{0, 0, 0, 1000000, 150 * 1024};
        const bool ok2 = tfr_check(true, kBase, kBase + (1ull << 42), 0, &big, 1, &C, &why);
        assert(ok2 && tfr_table_bytes(C) == 88 && C.rows == 256 && C.regions == 1000000 && C.raw_slots == 0);
    }
    // ---- refusals, in order, with their messages ---------------------------------------
    const uint64_t S = kBase, D = kBase + (1ull << 40), I = kBase + (1ull << 41);
    {
        TfrCounts C;
        std::string why;
        bool ok = tfr_check(true, 0, 0, 0, nullptr, 0, &C, &why);
        assert(ok);
        const s3dg_tfrecord_shard odd{7, 9, 3, 0, 1ull << 60};   // no records: nothing is looked at
        ok = tfr_check(true, S, D, I, &odd, 1, &C, &why);
        assert(ok && C.live == 0 && C.regions == 0);
        uint64_t out = 0;
        assert(!tfr_size(1ull << 60, 16, &out) && !tfr_size(2, UINT64_MAX - 10, &out) && tfr_size(0, UINT64_MAX - 16, &out) && out == 0);
        assert(tfr_size(1ull << 58, 16, &out) && out == 1ull << 63);
    }
    const s3dg_tfrecord_shard good{16, 32, 48, 3, 100};
    {
        TfrCounts C;
        std::string why;
        const bool ok = tfr_check(true, S, D, I, nullptr, 2, &C, &why);
        assert(!ok && why == "null shard array");
    }
    expect_refusal(true, 0, D, I, {good}, "src_base must be a 16-byte aligned device pointer");
    expect_refusal(true, S + 8, D, I, {good}, "src_base must be a 16-byte aligned device pointer");
    expect_refusal(true, S, 0, I, {good}, "dst_base must be a 16-byte aligned device pointer");
    expect_refusal(true, S, D + 4, I, {good}, "dst_base must be a 16-byte aligned device pointer");
    expect_refusal(true, S, D, I + 1, {good}, "idx_base must be 16-byte aligned");
    expect_refusal(false, 0, 0, 0, {good}, "base must be a 16-byte aligned device pointer");
    expect_refusal(false, 0, D + 2, 0, {good}, "base must be a 16-byte aligned device pointer");
    expect_refusal(true, S, D, I, {good, {8, 32, 48, 3, 100}}, "shard 1: src_off must be a multiple of 16");
    expect_refusal(true, S, D, I, {good, good, {16, 33, 48, 3, 100}}, "shard 2: dst_off must be a multiple of 16");
    expect_refusal(true, S, D, I, {{16, 32, 40, 3, 100}}, "shard 0: idx_off must be a multiple of 16");
    expect_refusal(false, 0, D, 0, {{16, 40, 48, 3, 100}}, "shard 0: dst_off must be a multiple of 16");
    expect_refusal(true, S, D, I, {{16, 32, 48, 1, kTfrMaxRecord + 1}}, "shard 0: record_size larger than 2^31 blocks");
    expect_refusal(true, S, D, I, {{16, 32, 48, 1ull << 60, 16}}, "shard 0: records * (16 + record_size) overflows");
    expect_refusal(false, 0, D, 0, {{0, 32, 0, UINT64_MAX, 0}}, "shard 0: records * (16 + record_size) overflows");
    expect_refusal(true, S, D, I, {{16, 32, 48, 1ull << 43, 0}}, "shard 0: more than 2^46 framed bytes in one call");
    expect_refusal(true, S, D, I, {{16, 32, 48, 1ull << 42, 0}, {16, 64, 48, 1ull << 42, 0}}, "shard 1: more than 2^46 framed bytes in one call");
    expect_refusal(true, S, D, I, {{16, UINT64_MAX - 15, 48, 3, 100}}, "shard 0: dst_off + stream overflows");
    expect_refusal(true, S, D, I, {{UINT64_MAX - 15, 32, 48, 3, 100}}, "shard 0: src_off + payload overflows");
    expect_refusal(true, S, D, I, {{16, 32, UINT64_MAX - 15, 3, 100}}, "shard 0: idx_off + index overflows");
    // a shard's stream over its own source: any overlap, the in-place shift by 12 included
    expect_refusal(true, S, S, I, {{0, 0, 48, 3, 100}}, "shard 0: the stream overlaps its own source");
    expect_refusal(true, S, S, I, {{336, 0, 48, 3, 100}}, "shard 0: the stream overlaps its own source");
    expect_refusal(true, S, S, I, {{0, 288, 48, 3, 100}}, "shard 0: the stream overlaps its own source");
    {   // touching is fine; so is an index nobody asked for, and the check form never looks at src_off
        TfrCounts C;
        std::string why;
        const s3dg_tfrecord_shard a{352, 0, 7, 3, 100}, b{0, 304, 9, 3, 100};
        bool ok = tfr_check(true, S, S, 0, &a, 1, &C, &why);
        assert(ok);
        ok = tfr_check(true, S, S, 0, &b, 1, &C, &why);
        assert(ok);
        const s3dg_tfrecord_shard c{5, 32, 3, 3, 100};
        ok = tfr_check(false, 0, D, 0, &c, 1, &C, &why);
        assert(ok && C.live == 1 && C.regions == 3);
    }
    // ---- for the Python side: streams of payloads it can rebuild -------------------------
    const uint64_t shapes[][2] = {{1, 0}, {3, 1}, {5, 1023}, {4, 1024}, {3, 2100}, {2, 32 * 1024 + 17}, {2, 3 * 32 * 1024 + 1023}};
    for (const auto &sh : shapes) {
        std::vector<uint8_t> s(sh[0] * sh[1] + 1);
        for (uint64_t i = 0; i < sh[0] * sh[1]; ++i) s[i] = (uint8_t)(i * 131 + 7);
        const std::vector<uint8_t> stream = walk(s, sh[0], sh[1], 32);
        printf("stream_%llux%llu|%08x\n", (unsigned long long)sh[0], (unsigned long long)sh[1],
               crc32_bitwise(stream.data(), stream.size()));
    }
    printf("shards|%llu\nrecords|%llu\n", (unsigned long long)shards_walked, (unsigned long long)records_folded);
    return 0;
}
