// tfrecord_search_plan_sweep.cpp — s3dg_tfrecord_search_plan.h on its own (g++,
// no HIP).  The program runs the search the way the kernels do (the bitmap and
// its two prefixes tile by tile, tfs_link per candidate, kTfsHopLog rounds of
// tfs_double, tfs_anchor_walk per stream, tfs_fill per anchor) on the host over
// crafted streams, several to a call, and holds every result field and every
// byte of a poisoned index to tfv_walk_host.  It also holds the length CRC from
// the byte tables to tfv_len_mcrc, and the workspace's parts to be disjoint.
// With a file of cases as argv[1] (lines "name hex max_records") it searches
// each and prints the result the way tfrecord_var_plan_sweep.cpp prints the
// walk's, for tests/test_tfrecord_search_cpu.py to compare with its judge.
#include <assert.h>
#include <stdio.h>
#include <string.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "s3dg_tfrecord_search_plan.h"

using namespace s3dg;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

typedef std::vector<uint8_t> Bytes;
static const uint8_t kPoison = 0xA7;
static uint32_t g_tab[kTfsCrcTabWords];
static uint64_t calls = 0, streams_searched = 0, records_found = 0, raw_steps = 0, nodes_linked = 0;

static void put_header(Bytes &v, uint64_t len, uint32_t flip = 0) {
    for (int b = 0; b < 8; ++b) v.push_back((uint8_t)(len >> (8 * b)));
    const uint32_t c = tfv_len_mcrc(len) ^ flip;
    for (int b = 0; b < 4; ++b) v.push_back((uint8_t)(c >> (8 * b)));
}
// A framed stream of these lengths with random payloads and footers; record i's length CRC flipped when bad[i].
static Bytes framed(const std::vector<uint64_t> &lens, const std::vector<bool> *bad = nullptr) {
    Bytes v;
    for (size_t i = 0; i < lens.size(); ++i) {
        put_header(v, lens[i], bad && (*bad)[i] ? 1u << (rnd() % 32) : 0);
        for (uint64_t j = 0; j < lens[i] + 4; ++j) v.push_back((uint8_t)rnd());
    }
    return v;
}

struct Call {
    Bytes arena;
    std::vector<s3dg_tfrecord_stream> st;
    uint64_t idx_bytes = 0;
    void add(const Bytes &data, uint64_t max_records, uint64_t gap) {
        s3dg_tfrecord_stream t{arena.size(), data.size(), idx_bytes, max_records};
        arena.insert(arena.end(), data.begin(), data.end());
        arena.insert(arena.end(), gap, kPoison);
        idx_bytes += 16 * tfv_walk_cap(t) + 16;   // a poisoned entry between neighbours
        st.push_back(t);
    }
};

// The device call on the host.  Returns the results; idx is the poisoned index.
static std::vector<s3dg_tfrecord_walk_result> search(const Call &C, Bytes *idx) {
    const uint64_t n = C.st.size();
    std::vector<uint64_t> tile0(n + 1);
    assert(tfs_tile_table(C.st.data(), n, tile0.data()));
    const uint64_t tiles = tile0[n];
    std::vector<uint64_t> bm(tiles * kTfsTileWords + 1, 0), tbase(tiles + 1, 0);
    std::vector<uint16_t> wpre(tiles * kTfsTileWords + 1, 0);
    const uint32_t K = tfs_crc_const();
    for (uint64_t g = 0; g < tiles; ++g) {   // k_tfs_candidates, a position at a time
        const uint64_t k = tfs_find_stream(tile0.data(), n, g);
        assert(tile0[k] <= g && g < tile0[k + 1]);
        const s3dg_tfrecord_stream Sd = C.st[k];
        const uint64_t tstart = (g - tile0[k]) * kTfsTile;
        uint32_t count = 0;
        for (uint32_t w = 0; w < kTfsTileWords; ++w) {
            uint64_t word = 0;
            for (uint32_t b = 0; b < 64; ++b) {
                const uint64_t pos = tstart + 64 * w + b;
                if (pos >= Sd.bytes || Sd.bytes - pos < kTfrHeader) continue;
                uint64_t len;
                uint32_t crc;
                tfs_header(C.arena.data() + Sd.off + pos, &len, &crc);
                if (tfs_fits(Sd.bytes - pos, len) && tfs_len_mcrc_tab(g_tab, K, len) == crc) word |= 1ull << b;
            }
            bm[g * kTfsTileWords + w] = word;
            wpre[g * kTfsTileWords + w] = (uint16_t)count;
            count += (uint32_t)__builtin_popcountll(word);
        }
        tbase[g] = count;
    }
    uint64_t nodes = 0;   // the exclusive sum
    for (uint64_t g = 0; g <= tiles; ++g) {
        const uint64_t c = tbase[g];
        tbase[g] = nodes;
        nodes += c;
    }
    assert(nodes <= kTfsMaxNodes);
    const TfsMap M{bm.data(), wpre.data(), tbase.data()};
    std::vector<TfsEnt> ent(nodes + 1);
    std::vector<uint32_t> next(nodes + 1);
    std::vector<TfsHop> hop[2] = {std::vector<TfsHop>(nodes + 1), std::vector<TfsHop>(nodes + 1)};
    std::vector<TfsAnchor> anch(nodes + 1, TfsAnchor{0, 0, 0});
    uint64_t seen = 0;
    for (uint64_t w = 0; w < tiles * kTfsTileWords; ++w) {   // k_tfs_link
        uint64_t word = bm[w];
        if (!word) continue;
        const uint64_t g = w / kTfsTileWords, k = tfs_find_stream(tile0.data(), n, g);
        const s3dg_tfrecord_stream Sd = C.st[k];
        const uint64_t p0 = (g - tile0[k]) * kTfsTile + (w % kTfsTileWords) * 64;
        uint32_t x = (uint32_t)(tbase[g] + wpre[w]);
        for (; word; word &= word - 1, ++x, ++seen) {
            const uint64_t pos = p0 + (uint32_t)__builtin_ctzll(word);
            assert(x == seen && tfs_node_at(M, tile0[k], pos) == x);   // node numbers count the candidates in order
            uint64_t len;
            uint32_t crc;
            tfs_header(C.arena.data() + Sd.off + pos, &len, &crc);
            ent[x] = TfsEnt{pos, len + kTfrFraming};
            next[x] = tfs_link(M, tile0[k], Sd.bytes, pos, len + kTfrFraming);
            assert(next[x] == kTfsNone || (next[x] > x && next[x] < tbase[tile0[k + 1]]));   // forward, inside its stream
            hop[0][x] = tfs_hop0(x, next[x]);
        }
    }
    assert(seen == nodes);
    int cur = 0;
    for (uint32_t r = 0; r < kTfsHopLog; ++r, cur ^= 1)   // k_tfs_double
        for (uint64_t x = 0; x < nodes; ++x) hop[cur ^ 1][x] = tfs_double(hop[cur].data(), (uint32_t)x, 1u << r);
    for (uint64_t x = 0; x < nodes; ++x) {   // a pair is what its many single links give
        uint32_t y = (uint32_t)x, s = 0;
        while (s < kTfsHop && next[y] != kTfsNone) y = next[y], ++s;
        assert(hop[cur][x].node == y && hop[cur][x].steps == s);
    }
    idx->assign(C.idx_bytes + 16, kPoison);
    std::vector<s3dg_tfrecord_walk_result> res(n);
    for (uint64_t k = 0; k < n; ++k)   // k_tfs_anchor
        res[k] = tfs_anchor_walk(C.arena.data() + C.st[k].off, C.st[k], M, tile0[k], ent.data(), next.data(), hop[cur].data(),
                                 anch.data(), idx->data(), true);
    for (uint64_t i = 0; i < nodes; ++i)   // k_tfs_fill
        if (anch[i].count) {
            assert(anch[i].count <= kTfsHop);
            tfs_fill(anch[i], ent.data(), next.data(), idx->data());
        }
    nodes_linked += nodes;
    return res;
}

static bool same(const s3dg_tfrecord_walk_result &a, const s3dg_tfrecord_walk_result &b) {
    return a.records == b.records && a.status == b.status && a.stop_offset == b.stop_offset && a.trailing == b.trailing &&
           a.bad_length_crc == b.bad_length_crc && a.first_bad_record == b.first_bad_record;
}

// The call against tfv_walk_host, stream by stream, index and poison included.
static void hold(const Call &C) {
    Bytes idx, want(C.idx_bytes + 16, kPoison);
    const std::vector<s3dg_tfrecord_walk_result> got = search(C, &idx);
    for (size_t k = 0; k < C.st.size(); ++k) {
        const s3dg_tfrecord_stream t = C.st[k];
        std::vector<uint64_t> e(2 * tfv_walk_cap(t) + 2);
        const s3dg_tfrecord_walk_result w = tfv_walk_host(C.arena.data() + t.off, t.bytes, t.max_records, e.data());
        assert(same(got[k], w));
        memcpy(want.data() + t.idx_off, e.data(), 16 * w.records);
        records_found += w.records;
        raw_steps += w.bad_length_crc;
    }
    assert(idx == want);
    ++calls;
    streams_searched += C.st.size();
}

static std::vector<uint64_t> random_lens(uint64_t count, uint64_t top) {
    std::vector<uint64_t> v(count);
    for (uint64_t &x : v) x = rnd() % (top + 1);
    return v;
}

static void sweep() {
    // the length CRC from the tables: short, wide and patterned lengths
    const uint32_t K = tfs_crc_const();
    for (uint64_t i = 0; i < 20000; ++i) {
        const uint64_t len = i < 5000 ? i : i < 10000 ? rnd() : i < 15000 ? rnd() >> (rnd() % 64) : 1ull << (i % 64);
        assert(tfs_len_mcrc_tab(g_tab, K, len) == tfv_len_mcrc(len));
    }
    // the workspaces: parts in order, 256-byte aligned, the last inside the whole
    for (uint64_t n : {1ull, 7ull, 1000ull})
        for (uint64_t tiles : {0ull, 1ull, 129ull}) {
            const TfsPlanA A = tfs_plan_a(n, tiles, 1000);
            assert(A.tile0_off >= n * 32 && A.upload_bytes == A.tile0_off + 8 * (n + 1) && A.res_off >= A.upload_bytes);
            assert(A.tbase_off >= A.res_off + 48 * n && A.bm_off >= A.tbase_off + 8 * (tiles + 1));
            assert(A.wpre_off >= A.bm_off + 8 * kTfsTileWords * tiles && A.tmp_off >= A.wpre_off + 2 * kTfsTileWords * tiles);
            assert(A.bytes >= A.tmp_off + 1000 && (A.res_off | A.tbase_off | A.bm_off | A.wpre_off | A.tmp_off) % 256 == 0);
            const TfsPlanB B = tfs_plan_b(tiles * 3);
            assert(B.anch_off >= 48 * tiles && B.hop_off[0] >= B.anch_off + 48 * tiles && B.hop_off[1] >= B.hop_off[0] + 24 * tiles);
            assert(B.next_off >= B.hop_off[1] + 24 * tiles && B.bytes >= B.next_off + 12 * tiles);
        }
    assert(tfs_tiles(0) == 0 && tfs_tiles(1) == 1 && tfs_tiles(kTfsTile) == 1 && tfs_tiles(kTfsTile + 1) == 2);
    // hop edges and max_records around them, resumed where a full walk stops
    for (uint64_t count : {0u, 1u, kTfsHop - 1, kTfsHop, kTfsHop + 1, 2 * kTfsHop, 2 * kTfsHop + 1}) {
        const Bytes data = framed(random_lens(count, 20));
        Call C;
        for (uint64_t cap : {(uint64_t)1, (uint64_t)kTfsHop - 1, (uint64_t)kTfsHop, (uint64_t)kTfsHop + 1, count - 1, count, count + 1,
                             UINT64_MAX})
            C.add(data, cap, rnd() % 3);
        hold(C);
    }
    // wrong CRCs on the chain: single, adjacent, at an anchor, every one; a length that leads into payload
    {
        const uint64_t count = kTfsHop + 40;
        const std::vector<uint64_t> lens = random_lens(count, 30);
        Call C;
        for (int variant = 0; variant < 6; ++variant) {
            std::vector<bool> bad(count, false);
            if (variant == 0) bad[0] = true;
            if (variant == 1) bad[count / 2] = bad[count / 2 + 1] = true;
            if (variant == 2) bad[count - 1] = true;
            if (variant == 3) bad[kTfsHop] = true;
            if (variant == 4) bad.assign(count, true);
            Bytes data = framed(lens, &bad);
            if (variant == 5) data[16 + lens[0]] ^= 4;   // record 1's length
            C.add(data, variant == 4 ? count - 3 : UINT64_MAX, 0);
        }
        hold(C);
    }
    // decoys: a framed stream inside a payload that ends inside it, one whose last link joins the true chain,
    // a header one byte before and one byte behind a true one, one at the last 12 bytes
    {
        const Bytes inner = framed({3, 0, 9, 1, 5});
        Bytes ends_inside, joins, around, last, last_in_record;
        put_header(ends_inside, inner.size() + 7);
        ends_inside.insert(ends_inside.end(), inner.begin(), inner.end());
        ends_inside.insert(ends_inside.end(), 7 + 4, 0x11);
        put_header(joins, inner.size() - 4);   // the inner stream is payload and footer: its chain ends at the next true header
        joins.insert(joins.end(), inner.begin(), inner.end());
        for (Bytes *v : {&ends_inside, &joins}) {
            const Bytes more = framed({2, 40, 0});
            v->insert(v->end(), more.begin(), more.end());
        }
        put_header(around, 25);                // payload and footer: a decoy a byte behind this header, one ending a byte before the next
        around.push_back(0x33);
        put_header(around, 0);
        around.insert(around.end(), 3, 0x44);
        put_header(around, 0);
        around.push_back(0x44);
        put_header(around, 20);
        around.push_back(0x55);
        put_header(around, 1);
        around.insert(around.end(), 7 + 4, 0x66);
        put_header(last, 30);
        last.insert(last.end(), 30 + 4, 0x77);
        put_header(last, 0);                   // 12 bytes, no footer: a header that does not fit
        put_header(last_in_record, 8);
        put_header(last_in_record, 0);         // the last record's payload and footer
        Call C;
        for (const Bytes *v : {&ends_inside, &joins, &around, &last, &last_in_record}) C.add(*v, UINT64_MAX, 0);
        hold(C);
    }
    // tile edges: a true header at each of T - 11 .. T, streams of T, T +- 1 and 2 T + 5 bytes, zero-length records across
    {
        Call C;
        for (uint64_t at = kTfsTile - 11; at <= kTfsTile; ++at) {
            Bytes data = framed({at - 16, 33, 0});
            C.add(data, UINT64_MAX, at % 2);   // some flush against the next stream
        }
        hold(C);
        Call D;
        for (uint64_t total : {(uint64_t)kTfsTile, (uint64_t)kTfsTile - 1, (uint64_t)kTfsTile + 1, (uint64_t)2 * kTfsTile + 5}) {
            Bytes data = framed({total - 48 - 7, 0, 7});
            assert(data.size() == total);
            D.add(data, UINT64_MAX, 0);
        }
        D.add(framed(std::vector<uint64_t>(kTfsTile / 16 + 9, 0)), UINT64_MAX, 0);
        hold(D);
    }
    // many streams flush against each other: empty, shorter than a header, truncated, trailing bytes, and pairs
    // whose last 11 bytes with the next stream's first byte would be a fitting header
    {
        Call C;
        for (int k = 0; k < 70; ++k) {
            Bytes data = k % 9 == 0 ? Bytes() : framed(random_lens(rnd() % 40, 60));
            if (k % 9 == 1) data.resize(rnd() % 12);
            if (k % 7 == 2 && data.size() > 20) data.resize(data.size() - 1 - rnd() % 19);
            if (k % 7 == 3) data.insert(data.end(), rnd() % 16, 0x5A);
            if (k % 5 == 4) {   // 11 bytes of a header of length 0x2A; the next stream's first byte is its twelfth
                Bytes h;
                put_header(h, 0x2A);
                data.insert(data.end(), h.begin(), h.begin() + 11);
                C.add(data, UINT64_MAX, 0);
                C.add(framed({h[11], 50, 3}), UINT64_MAX, 0);   // and 0x2A + 4 more bytes follow it
                continue;
            }
            C.add(data, k % 11 == 5 ? rnd() % 8 : UINT64_MAX, 0);
        }
        hold(C);
    }
    // seeded: random streams, some with a few bad CRCs, random caps
    for (int round = 0; round < 40; ++round) {
        Call C;
        const int ns = 1 + (int)(rnd() % 5);
        for (int k = 0; k < ns; ++k) {
            const uint64_t count = rnd() % (3 * kTfsHop);
            std::vector<bool> bad(count, false);
            for (uint64_t i = 0; i < count; ++i) bad[i] = rnd() % 200 == 0;
            Bytes data = framed(random_lens(count, rnd() % 2 ? 8 : 100), &bad);
            if (rnd() % 3 == 0 && data.size() > 30) data.resize(data.size() - rnd() % 30);
            C.add(data, rnd() % 2 ? UINT64_MAX : rnd() % (count + 2), rnd() % 4);
        }
        hold(C);
    }
}

int main(int argc, char **argv) {
    for (uint32_t e = 0; e < kTfsCrcTabWords; ++e) g_tab[e] = tfs_crc_tab_entry(e);
    if (argc > 1) {
        std::ifstream in(argv[1]);
        std::string line;
        while (std::getline(in, line)) {
            std::istringstream ls(line);
            std::string name, hex;
            unsigned long long cap;
            ls >> name >> hex >> cap;
            Bytes data;
            if (hex != "-")
                for (size_t i = 0; i + 1 < hex.size(); i += 2) data.push_back((uint8_t)std::stoul(hex.substr(i, 2), nullptr, 16));
            Call C;
            C.add(Bytes(3, kPoison), 0, 0);   // the stream under test at a byte offset, flush against its neighbours
            C.add(data, cap, 0);
            C.add(data, cap, 0);
            Bytes idx;
            const std::vector<s3dg_tfrecord_walk_result> res = search(C, &idx);
            hold(C);
            const s3dg_tfrecord_walk_result w = res[1];
            assert(same(w, res[2]));
            uint32_t c = 0;
            const uint64_t *e = reinterpret_cast<const uint64_t *>(idx.data() + C.st[1].idx_off);
            for (uint64_t i = 0; i < 2 * w.records; ++i) c = c * 31 + (uint32_t)(e[i] % 1000003);
            printf("search_%s|%llu,%llu,%llu,%llu,%llu,%lld,%u\n", name.c_str(), (unsigned long long)w.records,
                   (unsigned long long)w.status, (unsigned long long)w.stop_offset, (unsigned long long)w.trailing,
                   (unsigned long long)w.bad_length_crc, w.first_bad_record == UINT64_MAX ? -1ll : (long long)w.first_bad_record, c);
        }
        return 0;
    }
    sweep();
    printf("calls|%llu\nstreams|%llu\nrecords|%llu\nraw_steps|%llu\nnodes|%llu\n", (unsigned long long)calls,
           (unsigned long long)streams_searched, (unsigned long long)records_found, (unsigned long long)raw_steps,
           (unsigned long long)nodes_linked);
    return 0;
}
