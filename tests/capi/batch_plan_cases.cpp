// batch_plan_cases.cpp — prints the layout plan of generated descriptor sets
// (tests/test_batch_plan.py).  Host C++ only: it includes the library's
// s3dg_batch_plan.h and nothing of HIP.
//
// One case per input line, as key=value words:
//   lead=L             the batch's base address is granule L (mod 8)
//   tile=T dense=0|1 split=S    the knobs (forced tile shift, forced dense, split blocks)
//   gen=run n= size= stride= off0= estep=      object k: `size` bytes at off0 + k*stride,
//                                              entropy ent0 + k*estep (default 2^32)
//   gen=sizes n= lo= hi= seed= align=          packed at `align`, log-uniform sizes in
//                                              [lo, hi): lo << e plus a uniform remainder
//   ratio=a/b,c/d,...  compress (f_num/f_den) of object k: entry k mod the list's length
//   empty=E/P          objects with k mod E == P have size 0
//   swap=i:j           exchanges two descriptors (after everything above)
//   edit=k:field:v     sets (v) or adds to (+v) one field of descriptor k; may repeat
// Output per case: uniform tshift nclass, (count tshift recs) of both classes,
// recs span lead0 zclass; or "ERR code message" for a refused set.
#include "s3dg_batch_plan.h"

#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

using namespace s3dg;

static uint64_t rng_next(uint64_t &x) {   // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static uint64_t num(const std::string &s) { return strtoull(s.c_str(), nullptr, 0); }

static uint64_t *field(s3dg_obj_desc &o, const std::string &name, uint32_t **f32) {
    *f32 = nullptr;
    if (name == "dst_off") return &o.dst_off;
    if (name == "size") return &o.size;
    if (name == "dedup") return &o.dedup;
    if (name == "entropy") return &o.entropy;
    if (name == "f_num") *f32 = &o.f_num;
    if (name == "f_den") *f32 = &o.f_den;
    return nullptr;
}

// The descriptors, base address and knobs a case line describes.
static bool make_case(const std::string &line, std::vector<s3dg_obj_desc> &d, uintptr_t &base, BatchKnobs &K) {
    std::map<std::string, std::string> kv;
    std::vector<std::string> edits;
    std::istringstream in(line);
    for (std::string w; in >> w;) {
        const size_t eq = w.find('=');
        if (eq == std::string::npos) return false;
        if (w.substr(0, eq) == "edit") edits.push_back(w.substr(eq + 1));
        else kv[w.substr(0, eq)] = w.substr(eq + 1);
    }
    auto get = [&](const char *k, uint64_t def) { return kv.count(k) ? num(kv[k]) : def; };
    base = ((uintptr_t)1 << 40) + get("lead", 0) * kBlk;
    K.tile_shift = (uint32_t)get("tile", 0);
    K.force_dense = get("dense", 0) != 0;
    K.split_blocks = (uint32_t)get("split", 0);
    const uint64_t n = get("n", 0);
    d.assign(n, s3dg_obj_desc{});
    if (kv["gen"] == "run") {
        const uint64_t estep = get("estep", 1ull << 32);
        for (uint64_t k = 0; k < n; ++k) {
            d[k].dst_off = get("off0", 0) + k * get("stride", 0);
            d[k].size = get("size", 0);
            d[k].entropy = get("ent0", 1000) + k * estep;
        }
    } else if (kv["gen"] == "sizes") {
        uint64_t x = get("seed", 1), cur = 0;
        const uint64_t lo = get("lo", kBlk), hi = get("hi", kBlk), align = get("align", kBlk);
        uint32_t octaves = 0;
        while ((lo << (octaves + 1)) <= hi) ++octaves;
        for (uint64_t k = 0; k < n; ++k) {
            const uint64_t b = lo << (octaves ? rng_next(x) % octaves : 0);
            d[k].size = octaves ? b + rng_next(x) % b : b;
            d[k].dst_off = cur;
            d[k].entropy = rng_next(x);
            cur = (cur + d[k].size + align - 1) / align * align;
        }
    } else {
        return false;
    }
    std::vector<std::pair<uint32_t, uint32_t>> ratios;
    {
        std::istringstream rs(kv.count("ratio") ? kv["ratio"] : "0/1");
        for (std::string r; std::getline(rs, r, ',');) {
            const size_t sl = r.find('/');
            ratios.push_back({(uint32_t)num(r.substr(0, sl)), (uint32_t)num(r.substr(sl + 1))});
        }
    }
    for (uint64_t k = 0; k < n; ++k) {
        d[k].dedup = 1;
        d[k].f_num = ratios[k % ratios.size()].first;
        d[k].f_den = ratios[k % ratios.size()].second;
    }
    if (kv.count("empty")) {
        const size_t sl = kv["empty"].find('/');
        const uint64_t e = num(kv["empty"].substr(0, sl)), p = num(kv["empty"].substr(sl + 1));
        for (uint64_t k = 0; k < n; ++k)
            if (k % e == p) d[k].size = 0;
    }
    if (kv.count("swap")) {
        const size_t c = kv["swap"].find(':');
        const uint64_t i = num(kv["swap"].substr(0, c)), j = num(kv["swap"].substr(c + 1));
        if (i >= n || j >= n) return false;
        std::swap(d[i], d[j]);
    }
    for (const std::string &e : edits) {
        const size_t c1 = e.find(':'), c2 = e.find(':', c1 + 1);
        const uint64_t k = num(e.substr(0, c1));
        if (k >= n || c2 == std::string::npos) return false;
        std::string v = e.substr(c2 + 1);
        const bool add = v[0] == '+';
        if (add) v = v.substr(1);
        uint32_t *f32;
        uint64_t *f64 = field(d[k], e.substr(c1 + 1, c2 - c1 - 1), &f32);
        if (f64) *f64 = (add ? *f64 : 0) + num(v);
        else if (f32) *f32 = (add ? *f32 : 0) + (uint32_t)num(v);
        else return false;
    }
    return true;
}

static std::string plan_text(bool err, int code, const char *msg, const BatchPlan &B) {
    char buf[320];
    if (err) snprintf(buf, sizeof buf, "ERR %d %s", code, msg ? msg : "");
    else
        snprintf(buf, sizeof buf, "%d %u %d %llu %u %llu %llu %u %llu %llu %llu %llu %d", (int)B.uniform, B.tshift,
                 B.nclass, (unsigned long long)B.cls[0].count, B.cls[0].tshift, (unsigned long long)B.cls[0].recs,
                 (unsigned long long)B.cls[1].count, B.cls[1].tshift, (unsigned long long)B.cls[1].recs,
                 (unsigned long long)B.recs, (unsigned long long)B.span, (unsigned long long)B.lead0, B.zclass);
    return buf;
}

// The library's pass over one sub-batch: scanned in the parts the product
// cuts it into, merged, planned.
static std::string run_case(const std::vector<s3dg_obj_desc> &d, uintptr_t base, const BatchKnobs &K) {
    const uint64_t n = d.size();
    std::vector<s3dg_obj_desc> staged(n ? n : 1);
    const int parts = batch_parts(n);
    BatchScan part[kPrepParts];
    for (int q = 0; q < parts; ++q) {
        const uint64_t lo = batch_cut(0, n, q, parts), hi = batch_cut(0, n, q + 1, parts);
        batch_scan(d.data(), lo, hi, base, part[q], staged.data() + lo, K.split_blocks);
    }
    const BatchScan P = batch_scan_merge(part, parts);
    if (P.err) return plan_text(true, P.err, P.msg, BatchPlan{});
    return plan_text(false, 0, nullptr, plan_sub_batch(P, base, K));
}

int main() {
    for (std::string line; std::getline(std::cin, line);) {
        std::vector<s3dg_obj_desc> d;
        uintptr_t base;
        BatchKnobs K;
        if (!make_case(line, d, base, K)) {
            fprintf(stderr, "bad case: %s\n", line.c_str());
            return 2;
        }
        puts(run_case(d, base, K).c_str());
    }
    return 0;
}
