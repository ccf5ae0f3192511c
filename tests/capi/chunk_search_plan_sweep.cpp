// The chunker's parallel cut walk (s3dg_chunk_search_plan.h) on the host: the
// records that nodes, links, doubling, the follow and the fill give for
// synthetic candidate bitmaps must be those of a literal restatement of
// chunk_walk (s3dg_chunks.hip), for several objects in one add.  "ok <adds>".
#include <stdio.h>

#include <vector>

#include "s3dg_chunk_search_plan.h"

using namespace s3dg;
typedef std::vector<uint64_t> V64;
struct Obj {
    uint64_t len;
    V64 bm;   // whole granules of words
};
static uint64_t rng = 88172645463325252ull;
static int fails = 0;
#define CHECK(c) do { if (!(c) && fails++ < 10) printf("line %d: %s\n", __LINE__, #c); } while (0)

// kind 0 empty, 1 full, 2 one bit at `at`, else a candidate every 2^kind positions on average
static Obj make(uint64_t len, int kind, uint64_t at) {
    Obj o{len, V64((len + 4095) / 4096 * 64, 0)};
    for (uint64_t p = 31; p < len; ++p) {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        if (kind == 1 || (kind == 2 && p == at) || (kind > 2 && (rng >> 33) % (1ull << kind) == 0)) o.bm[p >> 6] |= 1ull << (p & 63);
    }
    return o;
}

// chunk_walk, bit by bit: (offset, length) pairs appended to out, forced cuts added to *forced.
static void walk(const Obj &o, uint64_t mn, uint64_t mx, V64 *out, uint64_t *forced) {
    for (uint64_t s = 0, e; s < o.len; s = e + 1) {
        e = o.len - 1;
        const uint64_t lo = s + mn - 1, cap = s + mx - 1, hi = cap < e ? cap : e;
        if (lo < o.len) {
            uint64_t p = lo;
            while (p <= hi && !((o.bm[p >> 6] >> (p & 63)) & 1)) ++p;
            if (p > hi) *forced += cap < o.len;
            e = p <= hi ? p : hi;
        }
        out->push_back(s);
        out->push_back(e - s + 1);
    }
}

// One add of objs under (mn, avg, mx) with the threshold thr, step by step as the kernels run it.
static void run_add(const std::vector<Obj> &objs, uint64_t mn, uint64_t avg, uint64_t mx, uint64_t thr) {
    const uint64_t n = objs.size();
    V64 bm, gpre{0}, nb(n + 1, 0);
    std::vector<CsObj> obj(n);
    uint64_t slots = 0;
    for (uint64_t j = 0; j < n; ++j) {
        obj[j] = CsObj{objs[j].len, bm.size() / 64, 0, (uint32_t)slots, 0, 0, 0};
        slots += span_obj_slots(objs[j].len, mn);
        bm.insert(bm.end(), objs[j].bm.begin(), objs[j].bm.end());
        nb[j + 1] = nb[j] + cs_reserved(objs[j].len, thr, mn, avg);
    }
    const uint64_t granules = bm.size() / 64, nodes = nb[n];
    for (uint64_t w = 0; w < bm.size(); w += 64) {
        gpre.push_back(gpre.back());
        for (int l = 0; l < 64; ++l) gpre.back() += __builtin_popcountll(bm[w + l]);
    }
    const CsPlan C = cs_plan(0, n, granules, nodes, 0);
    for (uint64_t j = 0; j < n; ++j) obj[j] = cs_object(obj[j].len, obj[j].g0, obj[j].r0, nb[j], nb[j + 1] - nb[j], gpre.data());
    V64 off(nodes, 0xDEAD), roff(slots, ~0ull), rlen(slots, 0);
    std::vector<uint32_t> kf(nodes, 7);
    std::vector<CsHop> lvl((kCsHopLog + 1) * nodes);
    std::vector<CsAnchor> anch(C.anchors, CsAnchor{5, 5});
    for (uint64_t g = 0; g < granules; ++g) {                               // k_cs_nodes
        const CsObj &O = obj[cs_find_obj(obj.data(), n, &CsObj::g0, g)];
        CHECK(O.g0 <= g && g < O.g0 + (O.len + 4095) / 4096);
        uint64_t at = O.nb + kCsFirst + (gpre[g] - gpre[O.g0]);
        for (int l = 0; l < 64 && O.take; at += __builtin_popcountll(bm[g * 64 + l++]))
            cs_word_nodes(bm[g * 64 + l], (g - O.g0) * 4096 + l * 64, off.data() + at);
        CHECK(!O.take || at <= O.nb + kCsFirst + O.count);
    }
    for (uint64_t x = 0; x < nodes; ++x) {                                  // k_cs_link
        const CsObj &O = obj[cs_find_obj(obj.data(), n, &CsObj::nb, x)];
        const uint64_t local = x - O.nb;
        CHECK(O.nb <= x && local < cs_node_bound(O.len, mn, avg));
        lvl[x] = CsHop{(uint32_t)x, 0};
        kf[x] = 0;
        if (!O.take || local >= (uint64_t)O.count + kCsFirst) continue;
        if (local == kCsEnd) off[x] = O.len - 1;
        if (local == kCsRoot) off[x] = ~0ull;
        if (local == kCsEnd) continue;
        const CsView V{off.data(), gpre.data() + O.g0, O.nb, O.len, O.count};
        lvl[x].node = (uint32_t)O.nb + cs_link(V, off[x] + 1, mn, mx, &kf[x], &lvl[x].chunks);
        CHECK(lvl[x].node > x || lvl[x].node == O.nb + kCsEnd);
    }
    for (uint64_t r = 0; r < kCsHopLog; ++r)                                // k_cs_double
        for (uint64_t x = 0; x < nodes; ++x) lvl[(r + 1) * nodes + x] = cs_double(lvl.data() + r * nodes, (uint32_t)x);
    uint64_t forced = 0, want_forced = 0;
    std::vector<uint32_t> cnt(n, 0);
    for (uint64_t j = 0; j < n; ++j) {                                      // k_cs_follow
        const uint64_t a0 = cs_anchor_base(obj[j].nb, j), a1 = cs_anchor_base(nb[j + 1], j + 1);
        uint64_t hops = 0;
        CHECK(a1 <= C.anchors);
        if (obj[j].take) cnt[j] = cs_follow(obj[j], lvl.data() + kCsHopLog * nodes, anch.data() + a0, a1 - a0, true, &hops);
        for (uint64_t a = a0 + hops; a < a1; ++a) anch[a] = CsAnchor{kCsNone, 0};
    }
    for (uint64_t a = 0; a < C.anchors; ++a)                                // k_cs_fill
        for (uint32_t i = 0; i < kCsHop && anch[a].node != kCsNone; ++i) {
            CsRec R;
            if (!cs_fill_lane(lvl.data(), nodes, off.data(), kf.data(), anch[a], i, mx, &R)) continue;
            for (uint32_t k = 0; k < R.forced + (R.last != 0); ++k) {
                CHECK(roff[R.slot + k] == ~0ull);                           // every slot once
                roff[R.slot + k] = R.s + k * mx;
                rlen[R.slot + k] = k < R.forced ? mx : R.last;
            }
            forced += R.forced;
        }
    for (uint64_t j = 0; j < n; ++j) {
        const uint64_t count = gpre[obj[j].g0 + (objs[j].len + 4095) / 4096] - gpre[obj[j].g0];
        CHECK(obj[j].take == (thr && objs[j].len >= thr && count + kCsFirst <= cs_node_bound(objs[j].len, mn, avg)));
        if (!obj[j].take) continue;
        V64 want;
        walk(objs[j], mn, mx, &want, &want_forced);
        CHECK(cnt[j] == want.size() / 2);
        for (uint64_t k = 0; k < want.size() / 2 && k < cnt[j]; ++k)
            CHECK(roff[obj[j].r0 + k] == want[2 * k] && rlen[obj[j].r0 + k] == want[2 * k + 1]);
    }
    CHECK(forced == want_forced);
}

int main() {
    const uint64_t P[][3] = {{32, 64, 128}, {32, 64, 32}, {64, 256, 1024}, {100, 64, 100}, {40, 4096, 9000}, {33, 128, 70}};
    int adds = 0;
    for (const auto &p : P) {
        std::vector<Obj> all{make(300000, 6, 0), make(300000, 13, 0)};      // several hops; forced runs between sparse candidates
        for (uint64_t len : {1, 31, 32, 33, 127, 128, 129, 4095, 4096, 4097, 8191, 12288, 20000, 70001}) {
            for (int kind : {0, 1, 3, 5, 7, 10}) all.push_back(make(len, kind, 0));
            // single bits at word and granule edges, at the first chunk's skip edge and at max
            for (uint64_t at : V64{31, 63, 64, 4095, 4096, p[0] - 2, p[0] - 1, p[2] - 1, p[2], len - 1})
                if (at >= 31 && at < len) all.push_back(make(len, 2, at));
        }
        for (const Obj &o : all) run_add({o}, p[0], p[1], p[2], 1), ++adds;
        for (uint64_t thr : V64{1, 4096, 20000}) {                          // both walks in one add, dense objects in between
            std::vector<Obj> some;
            for (size_t k = adds % 7; k < all.size(); k += 5) some.push_back(all[k]);
            run_add(some, p[0], p[1], p[2], thr), ++adds;
        }
    }
    CHECK(cs_node_bound(1 << 20, 2048, 8192) == 512 + 1 + 256 + 64 && cs_reserved(99, 100, 32, 64) == 0);
    CHECK(cs_reserved(100, 0, 32, 64) == 0 && cs_reserved(100, 100, 32, 64) == 4 + 1 + 4 + 64);
    if (fails) return printf("%d checks failed\n", fails), 1;
    printf("ok %d\n", adds);
    return 0;
}
