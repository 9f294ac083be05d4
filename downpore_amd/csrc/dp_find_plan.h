// The plan of the find stage (dp_overlap.hip: index query, then chaining) - every rule of its host side that is arithmetic: the
// layout of the cursor block through which the chaining kernels and the host talk, what a report means for the buffers' capacities,
// the grids of the chaining launches, and the layouts of the blocks the stage carves (d_pbase, the query meta block, the upload
// block with its minCount table).  Plain C++17, header only, no HIP: tests/native/find_plan_check.cpp holds it to the same rules
// written out a second time, with sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

// ---- the cursor block --------------------------------------------------------------------------------------------------------
// ctx->d_cursor on the device, ctx->h_cursor its pinned mirror: 32 words (cursor, flags, totals, counters) + 64 shards of the
// stage's algorithmic-byte count (one counter would be a thousand same-address atomics per kernel: 12 ns each, in a row).  The
// names are indices of 32-bit words.  Zero when an attempt starts.
#define DP_FIND_MAX_PASSES 6  // the largest DP_CHAIN_PASSES (dp_find_geometry clamps to it, dp_find_overlaps_impl reads the setting with it)
enum dp_find_cur {
    DP_CUR_INTS = 0,        // packed ints used (ma / mb); dp_fetch_overlaps' pack step counts here as well, once the stage is done
    DP_CUR_ERR = 2,         // error bits: 1 reduced buffer, 2 state pool, 4 results, 8 nodes
    DP_CUR_OVERFLOW = 3,    // a buffer was too small: the stage is repeated
    DP_CUR_OPEN = 8,        // [DP_CUR_OPEN + pass]: a query was still open when the pass started.  The walk writes pass 0's, the
                            // resolve step of pass p writes [DP_CUR_OPEN + 1 + p], the final walk reads [DP_CUR_OPEN + passes]
    DP_CUR_OPEN_WORDS = DP_FIND_MAX_PASSES + 1,
    DP_CUR_TOTALS = 16,     // two 64-bit totals (pair_scan_kernel), indexed by dp_find_tot
    DP_CUR_CHAINED = 20,    // final walk: pairs it chained
    DP_CUR_MARKED = 21,     // ... of them marked for the full layout by a slim pass
    DP_CUR_LEFT_OPEN = 24,  // [DP_CUR_LEFT_OPEN + 2 * pass + (q & 1)], pass 0 / 1: pairs left open by the pass's resolve step
    DP_CUR_LEFT_OPEN_WORDS = 4,
    DP_CUR_ALG = 32,        // 64-bit shards of the algorithmic bytes: shard q & (DP_CUR_ALG_SHARDS - 1)
    DP_CUR_ALG_SHARDS = 64,
    C_CURSOR_BYTES = (DP_CUR_ALG + 2 * DP_CUR_ALG_SHARDS) * 4,
};
enum dp_find_tot {  // the 64-bit words at DP_CUR_TOTALS
    DP_FIND_TOT_PAIRS = 0,  // (query, candidate) pairs of the round
    DP_FIND_TOT_SINTS = 1,  // ints of their scratch columns
    DP_FIND_TOT_WORDS = 2,
};
static_assert(DP_CUR_INTS < DP_CUR_ERR && DP_CUR_ERR < DP_CUR_OVERFLOW && DP_CUR_OVERFLOW < DP_CUR_OPEN, "cursor words overlap");
static_assert(DP_CUR_OPEN + DP_CUR_OPEN_WORDS <= DP_CUR_TOTALS, "the open flags of the largest pass count reach the totals");
static_assert(DP_CUR_OPEN + DP_CUR_OPEN_WORDS - 1 == 14, "pass 6: word 14");
static_assert(DP_CUR_TOTALS % 2 == 0 && DP_CUR_ALG % 2 == 0, "64-bit words of the cursor block are 8-byte aligned");
static_assert(DP_CUR_TOTALS + 2 * DP_FIND_TOT_WORDS <= DP_CUR_CHAINED && DP_CUR_CHAINED < DP_CUR_MARKED, "cursor words overlap");
static_assert(DP_CUR_MARKED < DP_CUR_LEFT_OPEN && DP_CUR_LEFT_OPEN + DP_CUR_LEFT_OPEN_WORDS <= DP_CUR_ALG, "cursor words overlap");
static_assert((DP_CUR_ALG_SHARDS & (DP_CUR_ALG_SHARDS - 1)) == 0, "shards are picked with a mask");
static_assert(C_CURSOR_BYTES == 640 && C_CURSOR_BYTES % 8 == 0, "the query kernel clears the block in 64-bit words");

// What an attempt reported: decoded once from the pinned mirror, after a wait.
struct dp_find_report {
    uint64_t tot_pairs, tot_sints;
    uint32_t ints, err, overflow, chained, marked;
    uint32_t left_open[DP_CUR_LEFT_OPEN_WORDS];
    uint64_t alg_bytes;  // sum of the shards
};
static inline dp_find_report dp_find_decode(const void* block /* C_CURSOR_BYTES */) {
    uint32_t w[DP_CUR_ALG];
    uint64_t tot[DP_FIND_TOT_WORDS], shard[DP_CUR_ALG_SHARDS];
    memcpy(w, block, sizeof w);
    memcpy(tot, (const uint8_t*)block + 4 * DP_CUR_TOTALS, sizeof tot);
    memcpy(shard, (const uint8_t*)block + 4 * DP_CUR_ALG, sizeof shard);
    dp_find_report r;
    r.tot_pairs = tot[DP_FIND_TOT_PAIRS];
    r.tot_sints = tot[DP_FIND_TOT_SINTS];
    r.ints = w[DP_CUR_INTS];
    r.err = w[DP_CUR_ERR];
    r.overflow = w[DP_CUR_OVERFLOW];
    r.chained = w[DP_CUR_CHAINED];
    r.marked = w[DP_CUR_MARKED];
    for (int i = 0; i < DP_CUR_LEFT_OPEN_WORDS; i++) r.left_open[i] = w[DP_CUR_LEFT_OPEN + i];
    r.alg_bytes = 0;
    for (int i = 0; i < DP_CUR_ALG_SHARDS; i++) r.alg_bytes += shard[i];
    return r;
}
// pairs left open ahead of pass 1 / pass 2 (by the resolve step of pass 0 / 1)
static inline uint32_t dp_find_open_ahead(const dp_find_report& r, int pass) { return r.left_open[2 * (pass - 1)] + r.left_open[2 * (pass - 1) + 1]; }

// ---- capacities --------------------------------------------------------------------------------------------------------------
// want_*: elements the buffers are reserved for (records and candidate lists; scratch columns sa / sb; packed chains ma / mb);
// *_cap: what the kernels are told, the 32-bit ones clamped.
#define DP_FIND_MAX_PAIRS 0xfffffff0ull
struct dp_find_caps {
    uint64_t want_pairs, want_sints, want_ints;
    uint32_t pair_cap, int_cap;
    uint64_t sint_cap;
};
// A stage's first attempt: what the buffers hold now (elements), at least a floor.
static inline dp_find_caps dp_find_caps_first(uint64_t mrec_elems, uint64_t sa_elems, uint64_t ma_elems) {
    dp_find_caps c = {};
    c.want_pairs = mrec_elems > (1u << 14) ? mrec_elems : (1u << 14);
    c.want_sints = sa_elems > (1u << 18) ? sa_elems : (1u << 18);
    c.want_ints = ma_elems > (1u << 18) ? ma_elems : (1u << 18);
    return c;
}
// Once the buffers are reserved for want_*: the capacities of the attempt.
static inline void dp_find_caps_set(dp_find_caps& c) {
    c.pair_cap = (uint32_t)(c.want_pairs < DP_FIND_MAX_PAIRS ? c.want_pairs : DP_FIND_MAX_PAIRS);
    c.sint_cap = c.want_sints;
    c.int_cap = (uint32_t)(c.want_ints < DP_FIND_MAX_PAIRS ? c.want_ints : DP_FIND_MAX_PAIRS);
}
enum dp_find_verdict {
    DP_FIND_FITS = 0,
    DP_FIND_GROW,            // a buffer was too small: want_* raised, run the attempt again (deterministic: the same totals)
    DP_FIND_TOO_MANY_PAIRS,  // more pairs than a 32-bit pair index holds
    DP_FIND_FLAG_ALONE,      // overflow flag without a total that exceeds a buffer
};
static inline dp_find_verdict dp_find_caps_check(const dp_find_report& r, dp_find_caps& c) {
    if (r.tot_pairs > DP_FIND_MAX_PAIRS) return DP_FIND_TOO_MANY_PAIRS;
    bool grow = false;
    if (r.tot_pairs > c.pair_cap) {
        c.want_pairs = r.tot_pairs + r.tot_pairs / 2 + 1024;
        grow = true;
    }
    if (r.tot_sints > c.sint_cap) {
        c.want_sints = r.tot_sints + r.tot_sints / 2 + 1024;
        grow = true;
    }
    if ((uint64_t)r.ints > c.int_cap) {
        c.want_ints = c.want_ints * 2 > (uint64_t)r.ints + 1024 ? c.want_ints * 2 : (uint64_t)r.ints + 1024;
        grow = true;
    }
    if (!grow && r.overflow) return DP_FIND_FLAG_ALONE;
    return grow ? DP_FIND_GROW : DP_FIND_FITS;
}

// ---- launch geometry ---------------------------------------------------------------------------------------------------------
#define DP_FIND_C_WAVES 4  // waves per workgroup of the kernels on the full layout (CWave)
#define DP_FIND_S_WAVES 4  // ... on the slim layout (CSlim)
#define DP_FIND_PROF_SLOT 128  // bytes of a wave's profile slot (16 64-bit words)
struct dp_find_geom {
    int passes;              // proposal passes (spec + resolve launches)
    bool slim_walk0;         // walk 0 on the slim layout (a forced tier, or no pass at all, is the full layout's business)
    uint32_t walk0_blocks;   // grid of walk 0 on the slim layout
    uint32_t walk_blocks;    // grid of a walk on the full layout (sizes the node pool, too)
    uint32_t final_blocks;   // grid of the final walk
    uint32_t spec_blocks;
    uint32_t resolve_blocks;
    uint32_t prof_stride;      // per-wave profile slots of one pass
    uint32_t prof_walk_slot;   // first slot of walk 0 (behind the passes')
    uint32_t prof_walk_slots;  // slots of walk 0
    size_t prof_bytes;         // all of them
};
// pass_env: DP_CHAIN_PASSES, < 0 = not set; open_ahead_2: pairs the context's previous stage left open ahead of pass 2
static inline dp_find_geom dp_find_geometry(uint32_t nq, long pass_env, uint32_t open_ahead_2, int tier, uint32_t spec_blocks) {
    dp_find_geom g = {};
    g.passes = pass_env >= 0 ? (int)(pass_env < DP_FIND_MAX_PASSES ? pass_env : DP_FIND_MAX_PASSES) : 3;
    // (round 6) the third pass is left out only when this context's previous stage left it next to nothing.  A threshold of 24 pairs - "at
    // k = 13 it sees ~18 short pairs, which the final walk chains as well" - saved two launches a round and cost more than it saved: the
    // final walk, one wave per QUERY, went from 13 to 53 us a launch under five slots (profiles/r06/k13_against_round5.txt).
    if (pass_env < 0 && open_ahead_2 < 2u) g.passes = 2;
    g.slim_walk0 = tier == 0 && g.passes > 0;
    const uint32_t w0 = (nq + DP_FIND_S_WAVES - 1) / DP_FIND_S_WAVES;
    g.walk0_blocks = w0 < 1 ? 1 : w0 > 1024 ? 1024 : w0;
    const uint32_t wf = (nq + DP_FIND_C_WAVES - 1) / DP_FIND_C_WAVES;
    g.walk_blocks = wf > 256 ? 256 : wf;
    // the final walk rarely has a query to do after the passes: a quarter of the workgroups (each wants 128 KB of a CU's LDS before it
    // can look whether there is anything to do) - a query that is still open finds a wave among 192
    g.final_blocks = g.passes > 0 ? (g.walk_blocks < 48 ? g.walk_blocks : 48) : g.walk_blocks;
    g.spec_blocks = spec_blocks;
    const uint32_t rb = (nq + 3) / 4;
    g.resolve_blocks = rb > 1024 ? 1024 : rb;
    g.prof_stride = spec_blocks * DP_FIND_S_WAVES;
    g.prof_walk_slot = (uint32_t)(g.passes * spec_blocks * DP_FIND_S_WAVES);
    g.prof_walk_slots = g.walk0_blocks * DP_FIND_S_WAVES;
    g.prof_bytes = ((size_t)g.passes * spec_blocks * DP_FIND_S_WAVES + (size_t)g.walk0_blocks * DP_FIND_S_WAVES) * DP_FIND_PROF_SLOT;
    return g;
}

// ---- the d_pbase block -------------------------------------------------------------------------------------------------------
// ibase u64 [nq + 1] (8-byte aligned first) | pbase u32 [nq + 1] (+ one word where that is odd) | qstate [nq], 8 bytes each
#define DP_FIND_QSTATE_BYTES 8
struct dp_find_pbase {
    size_t ibase, pbase, qstate;  // byte offsets
    size_t bytes;                 // to reserve
};
static inline dp_find_pbase dp_find_pbase_layout(uint32_t nq) {
    dp_find_pbase b;
    b.ibase = 0;
    b.pbase = ((size_t)nq + 1) * 8;
    b.qstate = b.pbase + ((size_t)nq + 1 + (((size_t)nq + 1) & 1)) * 4;
    b.bytes = ((size_t)nq + 1) * 4 + ((size_t)nq + 1) * 8 + (size_t)nq * DP_FIND_QSTATE_BYTES + (size_t)nq * 4 + 128;
    return b;
}

// ---- the query meta block ----------------------------------------------------------------------------------------------------
// What the query stage leaves per query, and the chaining stage's read-back brings to the host (ctx->d_qmeta / ctx->h_qm):
// meta u32 [nq][4] | posting words read u64 [nq] | candidate counts u32 [nq]
#define DP_QMETA_WORDS 4  // meta words of a query (query_body writes them); [2] bit 0: more than 65535 usable seeds
struct dp_find_qmeta {
    size_t words, qcnt;  // byte offsets (meta is at 0)
    size_t bytes;
};
static inline dp_find_qmeta dp_find_qmeta_layout(uint32_t nq) {
    dp_find_qmeta m;
    m.words = (size_t)nq * (DP_QMETA_WORDS * 4);
    m.qcnt = m.words + (size_t)nq * 8;
    m.bytes = m.qcnt + (size_t)nq * 4;
    return m;
}

// ---- the upload block --------------------------------------------------------------------------------------------------------
// What the host sends for the query stage, as it lies on both sides: query offsets u64 [nq + 1] | query segments i32 | minCount table i32 [mc_n]
struct dp_find_upload {
    uint32_t max_seeds;  // seeds of the largest query (two ints a seed)
    uint32_t mc_n;       // entries of the minCount table: one for every seed count that can occur, at least 8
    size_t off_bytes, segs_bytes, mc_bytes;
    size_t bytes() const { return off_bytes + segs_bytes + mc_bytes; }
};
static inline dp_find_upload dp_find_upload_extents(const uint64_t* q_off, uint32_t nq) {
    dp_find_upload u = {};
    for (uint32_t q = 0; q < nq; q++) {
        const uint32_t n = (uint32_t)((q_off[q + 1] - q_off[q]) / 2);
        if (n > u.max_seeds) u.max_seeds = n;
    }
    u.mc_n = u.max_seeds + 1 > 8 ? u.max_seeds + 1 : 8;
    u.off_bytes = ((size_t)nq + 1) * 8;
    u.segs_bytes = (size_t)(nq ? q_off[nq] : 0) * 4;
    u.mc_bytes = (size_t)u.mc_n * 4;
    return u;
}
// int(hitFraction*float64(n)+0.5) for every n that can occur (seeds/seeds.go:351, overlap/overlap.go:356), in IEEE double: product
// and sum are rounded to double one after the other (no contraction - the volatile intermediates, and -ffp-contract=off)
static inline void dp_find_mincount_table(double hf, uint32_t mc_n, int32_t* mc) {
    for (uint32_t n = 0; n < mc_n; n++) {
        volatile double prod = hf * (double)n;
        volatile double sum = prod + 0.5;
        mc[n] = (int32_t)sum;
    }
}

// ---- what the query stage hands on (dp_query_stage) ----------------------------------------------------------------------------
struct dp_query_out {
    int rc;  // DP_OK, or the error the context holds
    uint32_t* d_qmeta;
    uint64_t* d_words;
    uint32_t* d_qcnt;
    const int32_t* d_mc;
    uint32_t mc_n;
};
