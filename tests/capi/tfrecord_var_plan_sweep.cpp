// tfrecord_var_plan_sweep.cpp — s3dg_tfrecord_var_plan.h on its own (g++, no
// HIP).  The program walks lists of shards the way the kernels do (a wave's run
// of regions, one search, then steps; tfv_region; the framing bytes; the
// constants from the power table; tfr_crc_one / tfr_crc_fold), on the host and
// byte by byte, over swept length lists, region sizes, wave counts and both
// forms, and asserts:
//   * every byte of a stream has exactly one writer, none outside it, and every
//     byte of the source exactly one reader;
//   * the waves' runs, taken together, cover every region once;
//   * a record's CRC from its regions' raws is the bit-by-bit CRC-32 at every a;
//   * stream and index are the definition's;
//   * A^len (~0) from the power table, masked_crc(len), the restated region rule;
//   * the refusals and their messages, of the frame, the check and the walk.
// With a file of cases as argv[1] (lines "name hex max_records") it walks each
// with tfv_walk_host and prints the result.  It prints what
// tests/test_tfrecord_var_cpu.py compares with its own judges.
#include <assert.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "s3dg_tfrecord_var_plan.h"

using namespace s3dg;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

static const uint64_t kBase = 0x7000000000ull;
static uint64_t lists_walked = 0, records_folded = 0, regions_walked = 0;
static uint32_t g_pw[kTfvPowers];

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
static void put64(std::vector<uint8_t> &v, uint64_t x) {
    for (int b = 0; b < 8; ++b) v.push_back((uint8_t)(x >> (8 * b)));
}
// write_raw_record record by record, from its definition; and the index
static std::vector<uint8_t> reference_stream(const uint8_t *data, const std::vector<uint64_t> &lens, std::vector<uint8_t> *index) {
    std::vector<uint8_t> out;
    uint64_t at = 0;
    for (uint64_t len : lens) {
        if (index) {
            put64(*index, out.size());
            put64(*index, len + 16);
        }
        std::vector<uint8_t> lb;
        put64(lb, len);
        out.insert(out.end(), lb.begin(), lb.end());
        put32(out, masked(crc32_bitwise(lb.data(), 8)));
        out.insert(out.end(), data + at, data + at + len);
        put32(out, masked(crc32_bitwise(data + at, len)));
        at += len;
    }
    return out;
}

static uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

typedef std::vector<std::vector<uint64_t>> Lists;

// One call over `lists` (a shard each) at the call region `rows` with `waves`
// waves, walked as the kernels walk it.  Returns the streams, concatenated.
static std::vector<uint8_t> walk(const std::vector<uint8_t> &payload, const Lists &lists, uint32_t rows, uint64_t waves) {
    std::vector<s3dg_tfrecord_var_shard> sh;
    std::vector<uint64_t> lengths, sums;
    uint64_t so = 0, d_o = 16, io = 32;
    for (const auto &l : lists) {
        uint64_t sum = 0;
        for (uint64_t x : l) sum += x;
        sh.push_back(s3dg_tfrecord_var_shard{so, d_o, io, l.size(), lengths.size()});
        lengths.insert(lengths.end(), l.begin(), l.end());
        sums.push_back(sum);
        so += up16(sum) + 16;
        d_o += up16(sum + 16 * l.size()) + 16;
        io += 16 * l.size() + 16;
    }
    assert(so <= payload.size());
    std::vector<uint8_t> all;
    std::vector<uint8_t> arena(d_o, 0xEE), index(io, 0xEE);
    for (int form = 0; form < 2; ++form) {
        const bool frame = form == 0;
        TfvCounts C;
        std::string why;
        bool ok = tfv_check(frame, frame ? kBase : 0, kBase + (1ull << 40), frame ? kBase + (1ull << 41) : 0, sh.data(), sh.size(),
                            lengths.data(), lengths.size(), &C, &why);
        assert(ok);
        if (C.live == 0) continue;
        C.rows = rows;   // the sweep's own region, whatever the call would pick
        tfv_count_regions(sh.data(), sh.size(), lengths.data(), &C);
        std::vector<uint8_t> tab(tfv_table_bytes(C) + 16, 0xEE);
        tfv_build(sh.data(), sh.size(), lengths.data(), C, g_pw, tab.data());
        for (int q = 0; q < 16; ++q) assert(tab[tfv_table_bytes(C) + q] == 0xEE);
        assert(tfv_rec_offset(C) % 16 == 0 && tfv_const_offset(C) % 256 == 0 && tfv_raw_offset(C) % 256 == 0);
        assert(tfv_device_bytes(C) == tfv_raw_offset(C) + (C.long_records ? 4 * C.regions : 0));
        const TfvShard *E = reinterpret_cast<const TfvShard *>(tab.data() + kTfvShardOff);
        const TfvRec *rec = reinterpret_cast<const TfvRec *>(tab.data() + tfv_rec_offset(C));
        const uint64_t *longs = reinterpret_cast<const uint64_t *>(tab.data() + tfv_long_offset(C));
        assert(E[C.live].ent0 == C.ents && rec[C.ents - 1].reg0 == C.regions);
        const std::vector<uint8_t> &in = frame ? payload : arena;
        std::vector<uint8_t> writers(arena.size(), 0), iwriters(index.size(), 0), readers(frame ? payload.size() : 0, 0);
        std::vector<uint8_t> covered(C.regions, 0);
        std::vector<uint32_t> raw(C.regions, 0xEEEEEEEEu);
        auto finish = [&](const TfvShard &S, uint64_t i, uint64_t pre, uint64_t len, uint32_t crc) {
            const uint64_t out = S.dst_off + pre + 16 * i;
            assert(crc == crc32_bitwise(in.data() + (frame ? S.src_off + pre : out + 12), len));
            const uint32_t lm = tfv_len_mcrc(len);
            assert(lm == tfr_len_mcrc(len));
            ++records_folded;
            for (uint32_t l = 0; l < 16; ++l) {
                const uint64_t at = out + tfr_framing_at(l, len);
                const uint8_t b = (uint8_t)tfr_framing_byte(l, len, lm, tfr_masked(crc));
                if (frame) {
                    ++writers[at];
                    arena[at] = b;
                } else {
                    assert(arena[at] == b);   // a clean stream compares equal
                }
            }
            if (frame) {
                uint8_t *e = index.data() + S.idx_off + 16 * i;
                for (int q = 0; q < 16; ++q) ++iwriters[S.idx_off + 16 * i + q];
                const uint64_t v[2] = {pre + 16 * i, len + 16};
                memcpy(e, v, 16);
            }
        };
        const uint64_t per = tfv_run_len(C.regions, waves);
        for (uint64_t w = 0; w < waves; ++w) {
            uint64_t r, r_end;
            tfv_run(C.regions, per, w, &r, &r_end);
            assert(r <= r_end && r_end <= C.regions && r_end - r <= per);
            if (r >= r_end) continue;
            uint64_t j = tfv_find_rec(rec, C.ents, r);
            uint32_t si = tfv_find_shard(E, (uint32_t)C.live, j);
            assert(j + 1 < C.ents && rec[j].reg0 <= r && r < rec[j + 1].reg0 && E[si].ent0 <= j && j < E[si + 1].ent0 - 1);
            TfvRec cur = rec[j], nxt = rec[j + 1];
            TfvShard S = E[si];
            uint64_t e_end = E[si + 1].ent0;
            for (; r < r_end; ++r) {
                while (nxt.reg0 <= r) {
                    ++j;
                    cur = nxt;
                    assert(j + 1 < C.ents);
                    nxt = rec[j + 1];
                }
                while (e_end <= j) {
                    ++si;
                    assert(si < C.live);
                    S = E[si];
                    e_end = E[si + 1].ent0;
                }
                assert(j == tfv_find_rec(rec, C.ents, r) && si == tfv_find_shard(E, (uint32_t)C.live, j));
                assert(j + 1 < e_end);   // a record, never the entry behind a shard's last one
                const uint64_t i = j - S.ent0, len = nxt.pre - cur.pre;
                assert(len == lists[S.k][i] && S.src_off == sh[S.k].src_off);
                const uint32_t rpr = (uint32_t)(nxt.reg0 - cur.reg0), rr = tfv_rec_rows(len, rows);
                assert(rpr == tfv_rec_regions(len, rr) && rpr <= kCrcBatchMaxRegions);
                const uint32_t g = (uint32_t)(r - cur.reg0);
                const TfrRegion R = tfv_region(S, i, cur.pre, len, g, rpr, rr, frame);
                assert(R.rec == i && R.g == g && R.a < 16 && R.tail < 1024 && R.nrows <= rr);
                assert(R.a == (frame ? cur.pre % 16 : (12 + cur.pre) % 16));
                assert(R.out == S.dst_off + cur.pre + 16 * i && R.data == (frame ? S.src_off + cur.pre : R.out + 12));
                assert((R.data - R.a) % 16 == 0);
                assert(R.data - R.a >= (frame ? S.src_off : S.dst_off));   // the masked bytes lie inside the shard
                if (frame) assert((R.out + 12 - R.a) % 16 == 12);           // the stores are dword-aligned 16-byte ones
                if (g + 1 < rpr) assert(R.nrows == rr && R.tail == 0);
                else assert(R.pad_lo + (uint64_t)R.nrows * 1024 + R.tail == R.a + len);
                uint64_t lo, hi;
                tfr_region_span(R, &lo, &hi);
                assert(hi >= lo && hi <= len);
                if (g == 0) assert(lo == 0);
                if (g + 1 == rpr) assert(hi == len);
                std::vector<uint8_t> pad((uint64_t)R.nrows * 1024 + R.tail);
                for (uint64_t y = 0; y < pad.size(); ++y) {
                    const uint64_t py = R.pad_lo + y;
                    pad[y] = py < R.a ? 0 : in[R.data + (py - R.a)];
                }
                const uint32_t rw = raw_bitwise(0, pad.data(), pad.size());
                if (frame)
                    for (uint64_t x = lo; x < hi; ++x) {
                        ++readers[R.data + x];
                        ++writers[R.out + 12 + x];
                        arena[R.out + 12 + x] = in[R.data + x];
                    }
                ++covered[r];
                ++regions_walked;
                if (rpr == 1) finish(S, i, cur.pre, len, tfr_crc_one(rw, tfv_init(len, g_pw)));
                else raw[r] = rw;
            }
        }
        for (uint8_t c : covered) assert(c == 1);
        uint64_t nlong = 0;
        for (uint64_t t = 0; t < C.long_records; ++t) {
            const uint64_t j = longs[t];
            const TfvShard &S = E[tfv_find_shard(E, (uint32_t)C.live, j)];
            const TfvRec cur = rec[j], nxt = rec[j + 1];
            const uint64_t len = nxt.pre - cur.pre;
            const uint32_t rpr = (uint32_t)(nxt.reg0 - cur.reg0);
            assert(rpr > 1);
            const uint32_t a = (uint32_t)(((frame ? 0 : 12) + cur.pre) & 15);
            finish(S, j - S.ent0, cur.pre, len,
                   tfr_crc_fold(raw.data() + cur.reg0, rpr, tfv_rec_rows(len, rows), a, len, tfv_init(len, g_pw)));
            ++nlong;
        }
        assert(nlong == C.long_records);
        if (frame) {
            std::vector<uint8_t> wantw(arena.size(), 0), wantr(payload.size(), 0), wanti(index.size(), 0);
            for (size_t k = 0; k < lists.size(); ++k) {
                std::vector<uint8_t> ix;
                const std::vector<uint8_t> want = reference_stream(payload.data() + sh[k].src_off, lists[k], &ix);
                assert(want.size() == sums[k] + 16 * lists[k].size());
                if (lists[k].empty()) continue;
                assert(memcmp(arena.data() + sh[k].dst_off, want.data(), want.size()) == 0);
                assert(memcmp(index.data() + sh[k].idx_off, ix.data(), ix.size()) == 0);
                for (uint64_t x = 0; x < want.size(); ++x) wantw[sh[k].dst_off + x] = 1;
                for (uint64_t x = 0; x < sums[k]; ++x) wantr[sh[k].src_off + x] = 1;
                for (uint64_t x = 0; x < ix.size(); ++x) wanti[sh[k].idx_off + x] = 1;
                all.insert(all.end(), want.begin(), want.end());
                uint64_t sz = 0;
                ok = tfv_size(lists[k].data(), lists[k].size(), &sz);
                assert(ok && sz == want.size());
            }
            assert(writers == wantw && readers == wantr && iwriters == wanti);
            for (size_t x = 0; x < arena.size(); ++x) assert(wantw[x] || arena[x] == 0xEE);
        }
    }
    ++lists_walked;
    return all;
}

static void refuse(bool frame, uint64_t src, uint64_t dst, uint64_t idx, std::vector<s3dg_tfrecord_var_shard> v,
                   const std::vector<uint64_t> &lens, const char *msg, bool null_lengths = false) {
    TfvCounts C;
    std::string why;
    const bool ok = tfv_check(frame, src, dst, idx, v.data(), v.size(), null_lengths ? nullptr : lens.data(), lens.size(), &C, &why);
    if (ok || why != msg) fprintf(stderr, "expected \"%s\", got %s \"%s\"\n", msg, ok ? "success" : "refusal", why.c_str());
    assert(!ok && why == msg);
}
static void refuse_walk(uint64_t base, uint64_t idx, std::vector<s3dg_tfrecord_stream> v, bool results, const char *msg) {
    std::string why;
    const bool ok = tfv_walk_check(base, idx, v.data(), v.size(), results, &why);
    if (ok || why != msg) fprintf(stderr, "expected \"%s\", got %s \"%s\"\n", msg, ok ? "success" : "refusal", why.c_str());
    assert(!ok && why == msg);
}

static int walk_cases(const char *path) {
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream ss(line);
        std::string name, hex;
        unsigned long long cap = 0;
        ss >> name >> hex >> cap;
        if (hex == "-") hex.clear();
        std::vector<uint8_t> data(hex.size() / 2);
        for (size_t i = 0; i < data.size(); ++i) data[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
        // the stream at every dword alignment inside a poisoned buffer: the walk reads nothing outside it
        std::vector<uint64_t> ent(2 * (data.size() / 16 + 1), 0xEEEEEEEEEEEEEEEEull);
        const s3dg_tfrecord_walk_result R = tfv_walk_host(data.data(), data.size(), cap, ent.data());
        uint32_t c = 0;
        for (uint64_t k = 0; k < 2 * R.records; ++k) c = c * 31 + (uint32_t)(ent[k] % 1000003);
        for (uint64_t k = 2 * R.records; k < ent.size(); ++k) assert(ent[k] == 0xEEEEEEEEEEEEEEEEull);
        assert(R.trailing == data.size() - R.stop_offset && R.records <= cap);
        printf("walk_%s|%llu,%llu,%llu,%llu,%llu,%lld,%u\n", name.c_str(), (unsigned long long)R.records,
               (unsigned long long)R.status, (unsigned long long)R.stop_offset, (unsigned long long)R.trailing,
               (unsigned long long)R.bad_length_crc, R.first_bad_record == UINT64_MAX ? -1ll : (long long)R.first_bad_record, c);
    }
    return 0;
}

int main(int argc, char **argv) {
    static_assert(sizeof(s3dg_tfrecord_var_shard) == 40 && sizeof(s3dg_tfrecord_stream) == 32 &&
                      sizeof(s3dg_tfrecord_walk_result) == 48 && sizeof(TfvConst) == 8,
                  "layout");
    if (argc > 1) return walk_cases(argv[1]);
    tfv_powers(g_pw);
    std::vector<uint8_t> payload(900 * 1024);
    for (uint8_t &b : payload) b = (uint8_t)(rnd() >> 32);
    // ---- the constants -------------------------------------------------------------------
    for (uint64_t len = 0; len <= 4096; ++len) {
        assert(tfv_init(len, g_pw) == crcb_multmodp(crcb_x8n(len), 0xFFFFFFFFu));
        assert(tfv_len_mcrc(len) == tfr_len_mcrc(len));
    }
    for (int b = 0; b <= 43; ++b)
        for (uint64_t d : {0ull, 1ull, 4097ull}) {
            const uint64_t len = (1ull << b) + d;
            assert(tfv_init(len, g_pw) == crcb_multmodp(crcb_x8n(len), 0xFFFFFFFFu));
            assert(tfv_len_mcrc(len) == tfr_len_mcrc(len));
        }
    assert(tfv_len_mcrc(UINT64_MAX) == tfr_len_mcrc(UINT64_MAX) && tfv_len_mcrc(1ull << 63) == tfr_len_mcrc(1ull << 63));
    // ---- the restated region rule ----------------------------------------------------------
    for (uint32_t rows : {1u, 3u, 32u, 45u, 256u})
        for (uint64_t len : {0ull, 1ull, 1009ull, 1010ull, 32ull * 1024 - 15, 32ull * 1024 - 14, 33ull * 1024, 64ull << 20, 128ull << 20,
                             (128ull << 20) + 1024 - 15, 3ull << 30, (unsigned long long)kTfrMaxRecord}) {
            assert(tfv_rec_rows(len, rows) == crc_batch_obj_rows(len + 15, rows));
            assert(tfv_rec_regions(len, tfv_rec_rows(len, rows)) == crc_batch_obj_regions(len + 15, crc_batch_obj_rows(len + 15, rows)));
            assert(tfv_rec_rows(len, rows) == tfr_shard_rows(len, rows) && tfv_rec_regions(len, tfv_rec_rows(len, rows)) == tfr_shard_rpr(len, tfr_shard_rows(len, rows)));
        }
    // ---- every length 0..40 at every a: one call per a, a shard per length -------------------
    for (uint64_t a = 0; a < 16; ++a) {
        Lists L;
        for (uint64_t len = 0; len <= 40; ++len) L.push_back({a + 16, len, 3});
        walk(payload, L, 32, 1 + a);
    }
    {   // 0, 1, ..., 140 in order: the prefixes put records at every a
        std::vector<uint64_t> l;
        for (uint64_t k = 0; k <= 140; ++k) l.push_back(k);
        walk(payload, {l}, 32, 7);
    }
    // ---- lengths at 1024 k +- {0, 1, 15, 16, 17}; one and many regions mixed -----------------
    for (uint32_t rows : {1u, 2u, 3u})
        for (uint64_t a : {0ull, 5ull, 15ull}) {
            std::vector<uint64_t> l;
            if (a) l.push_back(a);
            for (uint64_t k = 1; k <= 4; ++k)
                for (int d : {0, 1, 15, 16, 17, -1, -15, -16, -17}) l.push_back(1024 * k + d);
            walk(payload, {l}, rows, 5);
            walk(payload, {l, {7}, l}, rows, 64);
        }
    for (uint32_t rows : {1u, 2u}) {
        walk(payload, {{100, 3 * rows * 1024 + 1023, 100, 3 * rows * 1024 + 1023, 100, 0, 9 * 1024ull + 1}}, rows, 3);
        walk(payload, {{5000, 3}, {}, {3, 5000, 0}, {0}}, rows, 4);
    }
    // ---- zero-length records first, last and in runs ------------------------------------------
    walk(payload, {{0, 0, 0, 5, 0, 0, 17, 0}, {0}, {0, 0}, {}, {1, 0, 0, 0, 1030, 0}}, 1, 2);
    walk(payload, {{0, 0, 0}}, 32, 1);
    walk(payload, {{}, {}}, 32, 1);
    // ---- random lists, any waves: every run covers its regions once --------------------------
    for (int k = 0; k < 40; ++k) {
        Lists L(1 + rnd() % 5);
        for (auto &l : L) {
            const uint64_t n = rnd() % 12;
            for (uint64_t i = 0; i < n; ++i) l.push_back(rnd() % 4 == 0 ? rnd() % 9000 : rnd() % 600);
        }
        walk(payload, L, 1 + (uint32_t)(rnd() % 3), 1 + rnd() % 40);
    }
    for (uint64_t nreg : {0ull, 1ull, 7ull, 8ull, 4096ull, 4097ull, 1000003ull})
        for (uint64_t waves : {1ull, 8ull, 4096ull, 4104ull}) {
            const uint64_t per = tfv_run_len(nreg, waves);
            uint64_t next = 0;
            for (uint64_t w = 0; w < waves; ++w) {
                uint64_t lo, hi;
                tfv_run(nreg, per, w, &lo, &hi);
                assert(lo == next && hi >= lo);
                next = hi;
            }
            assert(next == nreg);
        }
    // ---- a call's counts ---------------------------------------------------------------------
    {
        std::vector<uint64_t> lens(1000000, 2048);
        const s3dg_tfrecord_var_shard big{0, 0, 0, lens.size(), 0};
        TfvCounts C;
        std::string why;
        const bool ok = tfv_check(true, kBase, kBase + (1ull << 42), 0, &big, 1, lens.data(), lens.size(), &C, &why);
        assert(ok && C.live == 1 && C.ents == 1000001 && C.regions == 1000000 && C.long_records == 0 && C.rows == 256);
        assert(tfv_table_bytes(C) == 256 + 80 + 16 * 1000001ull);
    }
    // ---- refusals, in order, with their messages ------------------------------------------------
    const uint64_t S = kBase, D = kBase + (1ull << 40), I = kBase + (1ull << 41);
    const std::vector<uint64_t> lens = {100, 0, 7, 3000};
    const s3dg_tfrecord_var_shard good{16, 32, 48, 3, 1};
    {
        TfvCounts C;
        std::string why;
        bool ok = tfv_check(true, 0, 0, 0, nullptr, 0, nullptr, 0, &C, &why);
        assert(ok);
        const s3dg_tfrecord_var_shard odd{7, 9, 3, 0, 1ull << 60};   // no records: nothing is looked at
        ok = tfv_check(true, S, D, I, &odd, 1, nullptr, 0, &C, &why);
        assert(ok && C.live == 0 && C.regions == 0);
        ok = tfv_check(true, S, D, I, nullptr, 2, lens.data(), 4, &C, &why);
        assert(!ok && why == "null shard array");
        ok = tfv_check(true, S, D, I, &good, 1, lens.data(), 4, &C, &why);
        assert(ok && C.live == 1 && C.records == 3 && C.regions == 3);
        uint64_t out = 7;
        const uint64_t huge[2] = {UINT64_MAX - 40, 9};
        assert(!tfv_size(huge, 2, &out) && out == 7 && tfv_size(huge, 1, &out) && out == UINT64_MAX - 24);
        assert(!tfv_size(nullptr, 1ull << 60, &out) && tfv_size(nullptr, 0, &out) && out == 0);
    }
    refuse(true, 0, D, I, {good}, lens, "src_base must be a 16-byte aligned device pointer");
    refuse(true, S + 8, D, I, {good}, lens, "src_base must be a 16-byte aligned device pointer");
    refuse(true, S, 0, I, {good}, lens, "dst_base must be a 16-byte aligned device pointer");
    refuse(true, S, D, I + 1, {good}, lens, "idx_base must be 16-byte aligned");
    refuse(false, 0, 0, 0, {good}, lens, "base must be a 16-byte aligned device pointer");
    refuse(false, 0, D + 2, 0, {good}, lens, "base must be a 16-byte aligned device pointer");
    refuse(true, S, D, I, {good}, lens, "null lengths array", true);
    refuse(false, 0, D, 0, {good}, lens, "null lengths array", true);
    refuse(true, S, D, I, {good, {16, 32, 48, 3, 2}}, lens, "shard 1: len0 + records beyond the lengths");
    refuse(true, S, D, I, {{16, 32, 48, 1, 4}}, lens, "shard 0: len0 + records beyond the lengths");
    refuse(true, S, D, I, {{16, 32, 48, 2, UINT64_MAX}}, lens, "shard 0: len0 + records beyond the lengths");
    refuse(true, S, D, I, {good, {8, 32, 48, 3, 0}}, lens, "shard 1: src_off must be a multiple of 16");
    refuse(true, S, D, I, {good, good, {16, 33, 48, 3, 0}}, lens, "shard 2: dst_off must be a multiple of 16");
    refuse(true, S, D, I, {{16, 32, 40, 3, 0}}, lens, "shard 0: idx_off must be a multiple of 16");
    refuse(false, 0, D, 0, {{16, 40, 48, 3, 0}}, lens, "shard 0: dst_off must be a multiple of 16");
    refuse(true, S, D, I, {{16, 32, 48, 2, 0}}, {5, kTfrMaxRecord + 1}, "shard 0: a record longer than 2^31 blocks");
    refuse(true, S, D, I, {{16, 32, 48, 2, 0}}, {5, UINT64_MAX}, "shard 0: a record longer than 2^31 blocks");
    refuse(true, S, D, I, {{16, 32, 48, 9, 0}}, std::vector<uint64_t>(9, kTfrMaxRecord), "shard 0: more than 2^46 framed bytes in one call");
    refuse(true, S, S + (1ull << 50), I, {{16, 32, 48, 4, 0}, {16, 1ull << 47, 48, 4, 4}}, std::vector<uint64_t>(8, kTfrMaxRecord),
           "shard 1: more than 2^46 framed bytes in one call");
    refuse(true, S, D, I, {{16, UINT64_MAX - 15, 48, 3, 0}}, lens, "shard 0: dst_off + stream overflows");
    refuse(true, S, D, I, {{UINT64_MAX - 15, 32, 48, 3, 0}}, lens, "shard 0: src_off + payload overflows");
    refuse(true, S, D, I, {{16, 32, UINT64_MAX - 15, 3, 0}}, lens, "shard 0: idx_off + index overflows");
    refuse(true, S, S, I, {{0, 0, 48, 3, 0}}, lens, "shard 0: the stream overlaps its own source");
    refuse(true, S, S, I, {{0, 96, 48, 3, 0}}, lens, "shard 0: the stream overlaps its own source");
    {   // touching is fine; the check form never looks at src_off or idx_off
        TfvCounts C;
        std::string why;
        const s3dg_tfrecord_var_shard a{160, 0, 7, 3, 0}, c{5, 32, 3, 3, 0};
        bool ok = tfv_check(true, S, S, 0, &a, 1, lens.data(), 4, &C, &why);
        assert(ok);
        ok = tfv_check(false, 0, D, 0, &c, 1, lens.data(), 4, &C, &why);
        assert(ok && C.live == 1 && C.regions == 3);
    }
    // ---- the walk's refusals ----------------------------------------------------------------------
    {
        std::string why;
        bool ok = tfv_walk_check(0, 0, nullptr, 0, false, &why);
        assert(ok);
        const s3dg_tfrecord_stream any{5, 1000, 32, UINT64_MAX};   // any byte offset; max_records beyond what fits asks for no more
        ok = tfv_walk_check(S, I, &any, 1, true, &why);
        assert(ok && tfv_walk_cap(any) == 62);
    }
    const s3dg_tfrecord_stream st{5, 1000, 32, 10};
    refuse_walk(0, I, {st}, true, "null base");
    refuse_walk(S, 0, {st}, true, "null idx_base");
    refuse_walk(S, I, {st}, false, "null results");
    refuse_walk(S, I + 8, {st}, true, "idx_base must be 16-byte aligned");
    refuse_walk(S, I, {st, {5, 1000, 40, 10}}, true, "stream 1: idx_off must be a multiple of 16");
    refuse_walk(S, I, {{UINT64_MAX - 5, 1000, 32, 10}}, true, "stream 0: off + bytes overflows");
    refuse_walk(S, I, {{5, UINT64_MAX - 5, 32, 10}}, true, "stream 0: off + bytes overflows");
    refuse_walk(S, I, {{5, 1000, UINT64_MAX - 15, 10}}, true, "stream 0: idx_off + index overflows");
    {
        std::string why;
        const bool ok = tfv_walk_check(S, I, nullptr, 2, true, &why);
        assert(!ok && why == "null stream array");
    }
    // ---- the walk's step ---------------------------------------------------------------------------
    {
        uint64_t size = 7;
        assert(!tfv_walk_has_header(11) && tfv_walk_has_header(12));
        assert(tfv_walk_step(11, 0, &size) == kTfvWalkEnd && tfv_walk_step(12, 0, &size) == kTfvWalkTruncated && size == 7);
        assert(tfv_walk_step(15, 0, &size) == kTfvWalkTruncated && tfv_walk_step(16, 0, &size) == kTfvWalkRecord && size == 16);
        assert(tfv_walk_step(16, 1, &size) == kTfvWalkTruncated && tfv_walk_step(17, 1, &size) == kTfvWalkRecord && size == 17);
        assert(tfv_walk_step(1000, UINT64_MAX, &size) == kTfvWalkTruncated && tfv_walk_step(1000, UINT64_MAX - 15, &size) == kTfvWalkTruncated);
        assert(tfv_walk_step(UINT64_MAX, UINT64_MAX - 16, &size) == kTfvWalkRecord && size == UINT64_MAX);
    }
    // ---- for the Python side: streams of payloads it can rebuild ------------------------------------
    {
        std::vector<uint8_t> s(400 * 1024);
        for (uint64_t i = 0; i < s.size(); ++i) s[i] = (uint8_t)(i * 131 + 7);
        Lists ramp(1), edges(1), mixed(1), zeros = {{0, 0, 5, 0, 0, 0, 17, 0}};
        for (uint64_t k = 0; k <= 40; ++k) ramp[0].push_back(k);
        for (uint64_t k = 1; k <= 2; ++k)
            for (int d : {0, 1, 15, 16, 17, -1, -15, -16, -17}) edges[0].push_back(1024 * k + d);
        for (int k = 0; k < 3; ++k) {
            mixed[0].push_back(100);
            mixed[0].push_back(3 * 32 * 1024 + 1023);
        }
        const std::pair<const char *, Lists> named[] = {{"ramp", ramp}, {"edges", edges}, {"mixed", mixed}, {"zeros", zeros}};
        for (const auto &nl : named) {
            const std::vector<uint8_t> stream = walk(s, nl.second, 32, 9);
            printf("stream_%s|%08x\n", nl.first, crc32_bitwise(stream.data(), stream.size()));
        }
    }
    printf("lists|%llu\nrecords|%llu\nregions|%llu\n", (unsigned long long)lists_walked, (unsigned long long)records_folded,
           (unsigned long long)regions_walked);
    return 0;
}
