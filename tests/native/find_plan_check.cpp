// Stand-alone check of downpore_amd/csrc/dp_find_plan.h (tests/test_find_plan_cpu.py builds it plain and with ASan + UBSan, both
// with -ffp-contract=off): every rule of the find stage's plan against the same rule written out a second time in its simplest
// form - the literal numbers and expressions dp_overlap.hip had - and against explicit lists.  Prints "ok".  Arrays the header
// reads or writes have exactly the promised size, on the heap, so that a sanitizer sees a step too far.
#include <stdio.h>

#include <algorithm>
#include <memory>
#include <random>
#include <vector>

#include "dp_find_plan.h"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stdout, "FAILED line %d: %s\n", __LINE__, #c);    \
            return false;                                             \
        }                                                             \
    } while (0)

// ---- d_pbase: u64 [nq + 1] | u32 [nq + 1] | 8-byte states [nq], aligned as their types need, apart, inside the reservation
static bool pbase_one(uint32_t nq) {
    const dp_find_pbase b = dp_find_pbase_layout(nq);
    const uint64_t n = nq;
    CHECK(b.ibase % 8 == 0 && b.pbase % 4 == 0 && b.qstate % 8 == 0);
    CHECK(b.ibase + (n + 1) * 8 <= b.pbase);
    CHECK(b.pbase + (n + 1) * 4 <= b.qstate);
    CHECK(b.qstate + n * 8 <= b.bytes);
    return true;
}
static bool check_pbase() {
    for (uint32_t nq = 0; nq <= 4100; nq++) CHECK(pbase_one(nq));
    for (uint32_t nq : {65535u, 65536u, 65537u, 0xfffffffeu, 0xffffffffu}) CHECK(pbase_one(nq));
    return true;
}

// ---- the query meta block: 16 | 8 | 4 bytes a query
static bool check_qmeta() {
    for (uint32_t nq : {0u, 1u, 7u, 4100u, 65537u, 0xffffffffu}) {
        const dp_find_qmeta m = dp_find_qmeta_layout(nq);
        CHECK(m.words == (uint64_t)nq * 16 && m.qcnt == (uint64_t)nq * 24 && m.bytes == (uint64_t)nq * 28);
        CHECK(m.words % 8 == 0 && m.qcnt % 4 == 0);
    }
    return true;
}

// ---- cursor decode: every field from its own word
enum { F_PAIRS, F_SINTS, F_INTS, F_ERR, F_OVERFLOW, F_CHAINED, F_MARKED, F_LEFT0, F_LEFT1, F_LEFT2, F_LEFT3, F_ALG, F_N };
static void fields_of(const dp_find_report& r, uint64_t f[F_N]) {
    f[F_PAIRS] = r.tot_pairs, f[F_SINTS] = r.tot_sints, f[F_INTS] = r.ints, f[F_ERR] = r.err, f[F_OVERFLOW] = r.overflow;
    f[F_CHAINED] = r.chained, f[F_MARKED] = r.marked, f[F_ALG] = r.alg_bytes;
    for (int i = 0; i < 4; i++) f[F_LEFT0 + i] = r.left_open[i];
}
static int field_of_word(int w) {  // the layout, word by word; -1: a word the host does not read
    if (w >= 32) return F_ALG;
    switch (w) {
    case 0: return F_INTS;
    case 2: return F_ERR;
    case 3: return F_OVERFLOW;
    case 16: case 17: return F_PAIRS;
    case 18: case 19: return F_SINTS;
    case 20: return F_CHAINED;
    case 21: return F_MARKED;
    case 24: case 25: case 26: case 27: return F_LEFT0 + (w - 24);
    default: return -1;
    }
}
static bool check_decode() {
    CHECK(C_CURSOR_BYTES == 640);
    const int n_words = 160;
    std::unique_ptr<uint32_t[]> blk(new uint32_t[n_words]);
    for (int i = 0; i < n_words; i++) blk[i] = 0x01000193u * (uint32_t)(i + 1) + 7u;
    for (int i = 0; i < n_words; i++)
        for (int j = 0; j < i; j++) CHECK(blk[i] != blk[j]);
    const dp_find_report r = dp_find_decode(blk.get());
    auto w64 = [&](int i) { return (uint64_t)blk[i] | (uint64_t)blk[i + 1] << 32; };
    CHECK(r.ints == blk[0] && r.err == blk[2] && r.overflow == blk[3] && r.chained == blk[20] && r.marked == blk[21]);
    CHECK(r.tot_pairs == w64(16) && r.tot_sints == w64(18));
    for (int i = 0; i < 4; i++) CHECK(r.left_open[i] == blk[24 + i]);
    uint64_t sum = 0;
    for (int i = 0; i < 64; i++) sum += w64(32 + 2 * i);
    CHECK(r.alg_bytes == sum);
    CHECK(dp_find_open_ahead(r, 1) == blk[24] + blk[25] && dp_find_open_ahead(r, 2) == blk[26] + blk[27]);
    // a word that changes moves its own field and no other
    uint64_t f0[F_N], f1[F_N];
    fields_of(r, f0);
    for (int w = 0; w < n_words; w++) {
        blk[w] ^= 0x5a5a5a5au;
        fields_of(dp_find_decode(blk.get()), f1);
        blk[w] ^= 0x5a5a5a5au;
        for (int f = 0; f < F_N; f++) CHECK((f0[f] != f1[f]) == (f == field_of_word(w)));
    }
    return true;
}

// ---- capacities
static dp_find_report report(uint64_t pairs, uint64_t sints, uint32_t ints, uint32_t overflow) {
    dp_find_report r = {};
    r.tot_pairs = pairs, r.tot_sints = sints, r.ints = ints, r.overflow = overflow;
    return r;
}
static bool fits(const dp_find_report& r, const dp_find_caps& c) { return r.tot_pairs <= c.pair_cap && r.tot_sints <= c.sint_cap && r.ints <= c.int_cap; }
static bool check_caps() {
    dp_find_caps c = dp_find_caps_first(0, 0, 0);
    CHECK(c.want_pairs == 16384 && c.want_sints == 262144 && c.want_ints == 262144);
    c = dp_find_caps_first(16385, 262143, 1u << 20);
    CHECK(c.want_pairs == 16385 && c.want_sints == 262144 && c.want_ints == (1u << 20));
    c = dp_find_caps_first(1ull << 33, 1ull << 40, 1ull << 33);
    dp_find_caps_set(c);
    CHECK(c.pair_cap == 0xfffffff0u && c.sint_cap == 1ull << 40 && c.int_cap == 0xfffffff0u);
    c = dp_find_caps_first(0, 0, 0);
    dp_find_caps_set(c);
    CHECK(c.pair_cap == 16384 && c.sint_cap == 262144 && c.int_cap == 262144);
    const dp_find_caps first = c;
    // fits: nothing moves
    CHECK(dp_find_caps_check(report(16384, 262144, 262144, 0), c) == DP_FIND_FITS);
    CHECK(memcmp(&c, &first, sizeof c) == 0);
    // the three growth formulas
    CHECK(dp_find_caps_check(report(100000, 0, 0, 1), c) == DP_FIND_GROW);
    CHECK(c.want_pairs == 100000 + 50000 + 1024 && c.want_sints == first.want_sints && c.want_ints == first.want_ints);
    c = first;
    CHECK(dp_find_caps_check(report(0, 1000001, 0, 1), c) == DP_FIND_GROW);
    CHECK(c.want_sints == 1000001 + 500000 + 1024 && c.want_pairs == first.want_pairs && c.want_ints == first.want_ints);
    c = first;
    CHECK(dp_find_caps_check(report(0, 0, 300000, 1), c) == DP_FIND_GROW);  // twice the buffer is more
    CHECK(c.want_ints == 524288 && c.want_pairs == first.want_pairs && c.want_sints == first.want_sints);
    c = first;
    CHECK(dp_find_caps_check(report(0, 0, 2000000, 1), c) == DP_FIND_GROW);  // what was used and 1024 is more
    CHECK(c.want_ints == 2001024);
    c = first;
    CHECK(dp_find_caps_check(report(16385, 262145, 262145, 0), c) == DP_FIND_GROW);  // (all three at once; a total tells, flag or not)
    CHECK(c.want_pairs == 16385 + 8192 + 1024 && c.want_sints == 262145 + 131072 + 1024 && c.want_ints == 524288);
    // both refusals
    c = first;
    CHECK(dp_find_caps_check(report(0xfffffff1ull, 0, 0, 1), c) == DP_FIND_TOO_MANY_PAIRS);
    CHECK(dp_find_caps_check(report(1ull << 40, 0, 0, 0), c) == DP_FIND_TOO_MANY_PAIRS);
    CHECK(dp_find_caps_check(report(0xfffffff0ull, 0, 0, 1), c) == DP_FIND_GROW);
    CHECK(c.want_pairs == 0xfffffff0ull + 0x7ffffff8ull + 1024);
    c = first;
    CHECK(dp_find_caps_check(report(16384, 262144, 262144, 1), c) == DP_FIND_FLAG_ALONE);
    CHECK(memcmp(&c, &first, sizeof c) == 0);
    // one growth is enough: the stage is deterministic, so the second attempt reports the same totals
    std::mt19937_64 rng(12345);
    auto draw = [&](uint64_t top) {  // any magnitude up to top; the top itself and its neighbours now and then
        const unsigned kind = (unsigned)(rng() % 16);
        if (kind == 0) return top;
        if (kind == 1) return top - rng() % 3;
        const uint64_t v = rng() >> (rng() % 64);
        return v > top ? v % (top + 1) : v;
    };
    for (int it = 0; it < 50000; it++) {
        dp_find_caps k = dp_find_caps_first(draw(1ull << 33), draw(1ull << 41), draw(1ull << 33));
        dp_find_caps_set(k);
        const uint64_t pairs = draw(0xfffffff0ull), sints = draw(1ull << 42);
        const uint32_t ints = (uint32_t)draw(0xfffffff0ull);
        const bool fit = fits(report(pairs, sints, ints, 0), k);
        const dp_find_verdict v = dp_find_caps_check(report(pairs, sints, ints, fit ? 0 : 1), k);
        CHECK(v == (fit ? DP_FIND_FITS : DP_FIND_GROW));
        if (fit) continue;
        dp_find_caps_set(k);
        CHECK(fits(report(pairs, sints, ints, 0), k));
        CHECK(dp_find_caps_check(report(pairs, sints, ints, 0), k) == DP_FIND_FITS);
    }
    return true;
}

// ---- geometry: the expressions of dp_overlap.hip's chain_enqueue / dp_find_overlaps_impl / chain_finish before the header held them
static bool geometry_one(uint32_t nq, long pass_env, uint32_t open_ahead, int tier, uint32_t spec_blocks) {
    const dp_find_geom g = dp_find_geometry(nq, pass_env, open_ahead, tier, spec_blocks);
    int passes = pass_env >= 0 ? (int)pass_env : 3;
    if (pass_env < 0 && open_ahead < 2u) passes = 2;
    const uint32_t walk0_blocks = std::max<uint32_t>(1, std::min<uint32_t>(1024, (nq + 4 - 1) / 4));
    const uint32_t walk_blocks = std::min<uint32_t>(256, (nq + 4 - 1) / 4);
    const uint32_t final_blocks = passes > 0 ? std::min<uint32_t>(walk_blocks, 48) : walk_blocks;
    CHECK(g.passes == passes && g.slim_walk0 == (tier == 0 && passes > 0));
    CHECK(g.walk0_blocks == walk0_blocks && g.walk_blocks == walk_blocks && g.final_blocks == final_blocks);
    CHECK(g.spec_blocks == spec_blocks && g.resolve_blocks == std::min<uint32_t>(1024, (nq + 3) / 4));
    CHECK(g.prof_bytes == ((size_t)passes * spec_blocks * 4 + (size_t)walk0_blocks * 4) * 128);
    CHECK(g.prof_walk_slot == (uint32_t)(passes * spec_blocks * 4) && g.prof_stride == spec_blocks * 4);
    // what the printer walks: walk 0's slots, then every pass's - together every slot of the buffer, once
    CHECK(g.prof_bytes % DP_FIND_PROF_SLOT == 0);
    const size_t n_slots = g.prof_bytes / DP_FIND_PROF_SLOT;
    CHECK((size_t)passes * g.prof_stride + g.prof_walk_slots == n_slots);
    if (n_slots <= 4096 && (nq < 40 || nq % 101 == 0)) {
        std::vector<uint8_t> seen(n_slots, 0);
        for (int ps = -1; ps < g.passes; ps++) {
            const size_t first = ps < 0 ? g.prof_walk_slot : (size_t)ps * g.prof_stride, n = ps < 0 ? g.prof_walk_slots : g.prof_stride;
            for (size_t w = 0; w < n; w++) seen.at(first + w)++;
        }
        for (size_t s = 0; s < n_slots; s++) CHECK(seen[s] == 1);
    }
    return true;
}
static bool check_geometry() {
    std::vector<uint32_t> nqs;
    for (uint32_t nq = 0; nq <= 5000; nq++) nqs.push_back(nq);
    nqs.push_back(1u << 20);
    for (uint32_t nq : nqs)
        for (long pass_env = -1; pass_env <= 6; pass_env++)
            for (uint32_t open_ahead : {0u, 1u, 2u, ~0u}) {
                if (pass_env >= 0 && open_ahead != 1u && nq % 16 != 0) continue;  // (a set pass count does not look at it)
                for (int tier : {0, 2, 3})
                    for (uint32_t spec_blocks : {1u, 3u, 1024u}) CHECK(geometry_one(nq, pass_env, open_ahead, tier, spec_blocks));
            }
    CHECK(DP_FIND_MAX_PASSES == 6);
    return true;
}

// ---- the upload block and its minCount table
static bool extents_one(const std::vector<uint64_t>& q_off, uint32_t max_seeds, uint32_t mc_n, size_t off_bytes, size_t segs_bytes, size_t mc_bytes) {
    std::unique_ptr<uint64_t[]> q(new uint64_t[q_off.size()]);
    std::copy(q_off.begin(), q_off.end(), q.get());
    const dp_find_upload u = dp_find_upload_extents(q.get(), (uint32_t)q_off.size() - 1);
    CHECK(u.max_seeds == max_seeds && u.mc_n == mc_n);
    CHECK(u.off_bytes == off_bytes && u.segs_bytes == segs_bytes && u.mc_bytes == mc_bytes && u.bytes() == off_bytes + segs_bytes + mc_bytes);
    return true;
}
static bool check_upload() {
    CHECK(extents_one({0}, 0, 8, 8, 0, 32));                             // no query
    CHECK(extents_one({0, 2}, 1, 8, 16, 8, 32));                         // one seed: the table has its 8 entries
    CHECK(extents_one({0, 10, 10, 40}, 15, 16, 32, 160, 64));            // 5, 0 (an empty query) and 15 seeds
    CHECK(extents_one({0, 14, 28}, 7, 8, 24, 112, 32));                  // 7 seeds: n = 0..7
    CHECK(extents_one({0, 16}, 8, 9, 16, 64, 36));                       // 8 seeds: one entry more
    CHECK(extents_one({0, 4, 200004}, 100000, 100001, 24, 800016, 400004));
    return true;
}
static bool check_mincount() {
    const uint32_t n_max = 70000;
    for (double hf : {0.25, 0.1, 0.3, 0.05}) {
        std::unique_ptr<int32_t[]> mc(new int32_t[n_max + 1]);
        dp_find_mincount_table(hf, n_max + 1, mc.get());
        for (uint32_t n = 0; n <= n_max; n++) {
            if (hf == 0.25) CHECK(mc[n] == (int32_t)((n + 2) / 4));  // n / 4 + 1 / 2, exactly
            // the same expression, wider, rounded to double after the product and after the sum
            volatile long double prod_l = (long double)hf * (long double)n;
            volatile double prod = (double)prod_l;
            volatile long double sum_l = (long double)prod + 0.5L;
            volatile double sum = (double)sum_l;
            CHECK(mc[n] == (int32_t)sum);
        }
    }
    std::unique_ptr<int32_t[]> one(new int32_t[1]);  // (a table of one entry is one entry)
    dp_find_mincount_table(0.25, 1, one.get());
    CHECK(one[0] == 0);
    return true;
}

int main() {
    if (!check_pbase() || !check_qmeta() || !check_decode() || !check_caps() || !check_geometry() || !check_upload() || !check_mincount()) return 1;
    printf("ok\n");
    return 0;
}
