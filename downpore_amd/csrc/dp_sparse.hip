// libdownpore_hip.so — the reference index of `map` in its sparse layout.  CDNA4 / gfx950 only.
//
// The dense layout (dp_overlap.hip) stores the chunk / seed relation twice as bit matrices, S x ceil(M/64) and M x ceil(S/64)
// words: it grows with the square of the reference while the relation itself is more than 99.9 % zeros.  Here the same
// relation is held as sorted id lists, 4 bytes per (chunk, seed) pair in each direction:
//   post_off uint64 [S + 1], post_ids uint32 [E]   per seed, the distinct chunks that hold it, ascending
//   set_off  uint64 [M + 1], set_ids  uint32 [E]   per chunk, its distinct seeds, ascending
//   pmeta    uint32 [S][4]                          {count, first word, last word, last + 1}: exactly what the dense build writes
// E is the number of distinct (chunk, seed) pairs, at most H = the sum of the chunks' seed counts.  Steady state:
// 8 E + 24 S + 24 M bytes (offsets, pmeta, the chunk views) <= 8 H + 32 (S + M).
//
// Build (set-up, once per run): every hit of the chunk scan's segments becomes a (seed, chunk) pair in chunk order; a stable radix
// sort by seed gives the posting rows (chunks ascending within a seed, repeats adjacent), a compaction drops the repeats; a second
// stable radix sort of the compacted pairs by chunk gives the seed-set rows (seeds ascending, as the input was seed-ordered).
// Row offsets are lower bounds into the sorted keys.
#include <algorithm>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "dp_common.h"

typedef uint64_t u64;

// one wave per chunk: its hits as (seed, chunk) pairs at the chunk's place in hit order
__global__ void sp_expand_kernel(const dp_seq_ref* __restrict__ refs, uint32_t n_seqs, const u64* __restrict__ hoff,
                                 const int32_t* __restrict__ segs, uint32_t* __restrict__ key, uint32_t* __restrict__ val) {
    const uint32_t waves = gridDim.x * (blockDim.x >> 6);
    const int lane = dp_lane();
    for (uint32_t c = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); c < n_seqs; c += waves) {
        const dp_seq_ref r = refs[c];
        const u64 o = hoff[c];
        for (uint32_t i = lane; i < r.n_seeds; i += 64) {
            key[o + i] = (uint32_t)segs[r.seg_off + 2 * (u64)i + 1];
            val[o + i] = c;
        }
    }
}

// flag[e] = 1 for the first of a run of equal (seed, chunk) pairs
__global__ void sp_first_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, u64 n, uint32_t* __restrict__ flag) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n) return;
    flag[e] = (e == 0 || key[e] != key[e - 1] || val[e] != val[e - 1]) ? 1u : 0u;
}

__global__ void sp_compact_kernel(const uint32_t* __restrict__ key, const uint32_t* __restrict__ val, const uint32_t* __restrict__ flag,
                                  const u64* __restrict__ pos, u64 n, uint32_t* __restrict__ okey, uint32_t* __restrict__ oval) {
    const u64 e = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n || !flag[e]) return;
    okey[pos[e]] = key[e];
    oval[pos[e]] = val[e];
}

// off[r] = first position of a key >= r in the ascending keys (r = 0 .. rows; off[rows] = n)
__global__ void sp_offsets_kernel(const uint32_t* __restrict__ keys, u64 n, uint32_t rows, u64* __restrict__ off) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > rows) return;
    u64 lo = 0, hi = n;
    while (lo < hi) {
        const u64 mid = (lo + hi) >> 1;
        if (keys[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    off[r] = lo;
}

// pmeta of every seed from its posting row: NewIntSet's {0, 1, 0, 1} when the row is empty
__global__ void sp_pmeta_kernel(const u64* __restrict__ off, const uint32_t* __restrict__ ids, uint32_t n_seeds, uint32_t* __restrict__ pmeta) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seeds) return;
    const u64 a = off[s], b = off[s + 1];
    uint4 m = make_uint4(0u, 1u, 0u, 1u);
    if (b > a) {
        const uint32_t first = ids[a] >> 6, last = ids[b - 1] >> 6;
        m = make_uint4((uint32_t)(b - a), first, last, last + 1);
    }
    *(uint4*)(pmeta + 4 * (size_t)s) = m;
}

static unsigned sp_bits(uint64_t n) {  // bits of the largest id below n
    unsigned b = 1;
    while (b < 32 && ((uint64_t)1 << b) < n) b++;
    return b;
}

uint64_t dp_index_sparse_bytes(const dp_ctx* ctx) {
    if (!ctx->index_sparse || ctx->index_src) return 0;
    const uint64_t S = ctx->n_seeds, M = ctx->n_seqs, E = ctx->sp_entries;
    return 8 * (S + 1) + 4 * E + 8 * (M + 1) + 4 * E + 16 * S + (uint64_t)sizeof(dp_seq_ref) * M;
}

extern "C" int dp_index_build_sparse(dp_ctx* ctx, const dp_seq_ref* seqs, uint32_t n_seqs) {
    if (!ctx || (n_seqs && !seqs)) return DP_ERR_ARG;
    if (!ctx->round_open) return dp_fail(ctx, DP_ERR_STATE, "dp_index_build_sparse before dp_round_begin");
    hipSetDevice(ctx->device);
    uint64_t H = 0, segEnd = 0;
    for (uint32_t i = 0; i < n_seqs; i++) {
        const uint64_t e = seqs[i].seg_off + 2ull * seqs[i].n_seeds + 1;
        if (e > ctx->n_segs) return dp_fail(ctx, DP_ERR_ARG, "dp_index_build_sparse: sequence view outside the scan output");
        segEnd = std::max(segEnd, e);
        H += seqs[i].n_seeds;
    }
    const uint32_t S = ctx->n_seeds;
    ctx->max_seq_seeds = 0;
    for (uint32_t i = 0; i < n_seqs; i++) ctx->max_seq_seeds = std::max(ctx->max_seq_seeds, seqs[i].n_seeds);
    ctx->n_seqs = n_seqs;
    ctx->W = std::max<uint32_t>(1, (n_seqs + 63) / 64);
    ctx->SW = std::max<uint32_t>(1, (S + 63) / 64);
    ctx->word_base = 0;
    ctx->global_n_seqs = 0;
    ctx->chunks_on_device = false;
    ctx->index_sparse = true;
    ctx->index_src = nullptr;
    ctx->sp_entries = 0;
    if (dev_reserve(ctx, ctx->d_seqrefs, (size_t)n_seqs * sizeof(dp_seq_ref) + 16)) return DP_ERR_HIP;
    if (dev_reserve(ctx, ctx->d_pmeta, (size_t)S * 16 + 16)) return DP_ERR_HIP;
    if (dev_reserve(ctx, ctx->d_sp_post_off, ((size_t)S + 1) * 8 + 64)) return DP_ERR_HIP;
    if (dev_reserve(ctx, ctx->d_sp_set_off, ((size_t)n_seqs + 1) * 8 + 64)) return DP_ERR_HIP;
    // the chunks' segments, out of the scan buffer that later window scans overwrite
    if (dev_reserve(ctx, ctx->d_sp_segs, (size_t)segEnd * 4 + 64)) return DP_ERR_HIP;
    if (segEnd) DP_HIP(hipMemcpyAsync(ctx->d_sp_segs.p, ctx->d_segs.p, (size_t)segEnd * 4, hipMemcpyDeviceToDevice, ctx->stream));
    if (n_seqs)
        DP_HIP(hipMemcpyAsync(ctx->d_seqrefs.p, dp_stage(ctx, seqs, (size_t)n_seqs * sizeof(dp_seq_ref)), (size_t)n_seqs * sizeof(dp_seq_ref),
                              hipMemcpyHostToDevice, ctx->stream));
    void *d_hoff = nullptr, *d_k0 = nullptr, *d_v0 = nullptr, *d_k1 = nullptr, *d_v1 = nullptr, *d_flag = nullptr, *d_pos = nullptr, *d_tmp = nullptr;
    auto cleanup = [&] {
        for (void* p : {d_hoff, d_k0, d_v0, d_k1, d_v1, d_flag, d_pos, d_tmp})
            if (p) dp_dev_free(p);
    };
#define SPB(x)                                                                   \
    do {                                                                         \
        hipError_t e_ = (x);                                                     \
        if (e_ != hipSuccess) {                                                  \
            (void)dp_stream_sync(ctx);                                           \
            cleanup();                                                           \
            return dp_fail(ctx, DP_ERR_HIP, "dp_index_build_sparse: " #x, e_);   \
        }                                                                        \
    } while (0)
    uint64_t E = 0;
    if (H) {
        std::vector<u64> hoff((size_t)n_seqs + 1, 0);
        for (uint32_t i = 0; i < n_seqs; i++) hoff[i + 1] = hoff[i] + seqs[i].n_seeds;
        SPB(dp_dev_malloc(&d_hoff, ((size_t)n_seqs + 1) * 8));
        SPB(dp_dev_malloc(&d_k0, (size_t)H * 4 + 64));
        SPB(dp_dev_malloc(&d_v0, (size_t)H * 4 + 64));
        SPB(dp_dev_malloc(&d_k1, (size_t)H * 4 + 64));
        SPB(dp_dev_malloc(&d_v1, (size_t)H * 4 + 64));
        SPB(dp_dev_malloc(&d_flag, (size_t)H * 4 + 64));
        SPB(dp_dev_malloc(&d_pos, (size_t)H * 8 + 64));
        SPB(hipMemcpyAsync(d_hoff, hoff.data(), ((size_t)n_seqs + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
        SPB(dp_stream_sync(ctx));  // (hoff is a local vector)
        hipLaunchKernelGGL(sp_expand_kernel, dim3(std::min<uint32_t>(4096, (n_seqs + 3) / 4)), dim3(256), 0, ctx->stream,
                           (const dp_seq_ref*)ctx->d_seqrefs.p, n_seqs, (const u64*)d_hoff, (const int32_t*)ctx->d_segs.p, (uint32_t*)d_k0,
                           (uint32_t*)d_v0);
        SPB(hipGetLastError());
        // 1. by seed (stable: chunks stay ascending within a seed)
        const unsigned sbits = sp_bits(S), cbits = sp_bits(n_seqs);
        size_t tb = 0, tb2 = 0, tb3 = 0;
        SPB(rocprim::radix_sort_pairs(nullptr, tb, (const uint32_t*)d_k0, (uint32_t*)d_k1, (const uint32_t*)d_v0, (uint32_t*)d_v1, (size_t)H, 0u,
                                      sbits, ctx->stream));
        SPB(rocprim::exclusive_scan(nullptr, tb2, (const uint32_t*)d_flag, (u64*)d_pos, (u64)0, (size_t)H, rocprim::plus<u64>(), ctx->stream));
        SPB(rocprim::radix_sort_pairs(nullptr, tb3, (const uint32_t*)d_v0, (uint32_t*)d_v1, (const uint32_t*)d_k0, (uint32_t*)d_k1, (size_t)H, 0u,
                                      cbits, ctx->stream));
        SPB(dp_dev_malloc(&d_tmp, std::max(tb, std::max(tb2, tb3)) + 64));
        SPB(rocprim::radix_sort_pairs(d_tmp, tb, (const uint32_t*)d_k0, (uint32_t*)d_k1, (const uint32_t*)d_v0, (uint32_t*)d_v1, (size_t)H, 0u,
                                      sbits, ctx->stream));
        // 2. drop repeated (seed, chunk) pairs: a chunk that holds a seed twice is one posting entry
        const uint32_t eb = (uint32_t)((H + 255) / 256);
        hipLaunchKernelGGL(sp_first_kernel, dim3(eb), dim3(256), 0, ctx->stream, (const uint32_t*)d_k1, (const uint32_t*)d_v1, (u64)H,
                           (uint32_t*)d_flag);
        SPB(hipGetLastError());
        SPB(rocprim::exclusive_scan(d_tmp, tb2, (const uint32_t*)d_flag, (u64*)d_pos, (u64)0, (size_t)H, rocprim::plus<u64>(), ctx->stream));
        u64 last[2] = {0, 0};
        uint32_t lastFlag = 0;
        SPB(hipMemcpyAsync(&last[0], (const u64*)d_pos + (H - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
        SPB(hipMemcpyAsync(&lastFlag, (const uint32_t*)d_flag + (H - 1), 4, hipMemcpyDeviceToHost, ctx->stream));
        SPB(dp_stream_sync(ctx));
        E = last[0] + lastFlag;
        // compacted pairs: seeds in d_k0, chunks in d_v0 (seed-major)
        hipLaunchKernelGGL(sp_compact_kernel, dim3(eb), dim3(256), 0, ctx->stream, (const uint32_t*)d_k1, (const uint32_t*)d_v1,
                           (const uint32_t*)d_flag, (const u64*)d_pos, (u64)H, (uint32_t*)d_k0, (uint32_t*)d_v0);
        SPB(hipGetLastError());
        if (dev_reserve(ctx, ctx->d_sp_post_ids, (size_t)E * 4 + 64) || dev_reserve(ctx, ctx->d_sp_set_ids, (size_t)E * 4 + 64)) {
            (void)dp_stream_sync(ctx);
            cleanup();
            return DP_ERR_HIP;
        }
        SPB(hipMemcpyAsync(ctx->d_sp_post_ids.p, d_v0, (size_t)E * 4, hipMemcpyDeviceToDevice, ctx->stream));
        hipLaunchKernelGGL(sp_offsets_kernel, dim3((S + 1 + 255) / 256), dim3(256), 0, ctx->stream, (const uint32_t*)d_k0, (u64)E, S,
                           (u64*)ctx->d_sp_post_off.p);
        SPB(hipGetLastError());
        // 3. by chunk (stable: seeds stay ascending within a chunk)
        SPB(rocprim::radix_sort_pairs(d_tmp, tb3, (const uint32_t*)d_v0, (uint32_t*)d_v1, (const uint32_t*)d_k0, (uint32_t*)ctx->d_sp_set_ids.p,
                                      (size_t)E, 0u, cbits, ctx->stream));
        hipLaunchKernelGGL(sp_offsets_kernel, dim3((n_seqs + 1 + 255) / 256), dim3(256), 0, ctx->stream, (const uint32_t*)d_v1, (u64)E, n_seqs,
                           (u64*)ctx->d_sp_set_off.p);
        SPB(hipGetLastError());
    } else {
        SPB(hipMemsetAsync(ctx->d_sp_post_off.p, 0, ((size_t)S + 1) * 8, ctx->stream));
        SPB(hipMemsetAsync(ctx->d_sp_set_off.p, 0, ((size_t)n_seqs + 1) * 8, ctx->stream));
        if (dev_reserve(ctx, ctx->d_sp_post_ids, 64) || dev_reserve(ctx, ctx->d_sp_set_ids, 64)) return DP_ERR_HIP;
    }
    if (S) {
        hipLaunchKernelGGL(sp_pmeta_kernel, dim3((S + 255) / 256), dim3(256), 0, ctx->stream, (const u64*)ctx->d_sp_post_off.p,
                           (const uint32_t*)ctx->d_sp_post_ids.p, S, (uint32_t*)ctx->d_pmeta.p);
        SPB(hipGetLastError());
    }
    SPB(dp_stream_sync(ctx));  // (the scratch goes back to the cache below)
#undef SPB
    cleanup();
    ctx->sp_entries = E;
    return DP_OK;
}

extern "C" int dp_index_borrow(dp_ctx* ctx, dp_ctx* src) {
    if (!ctx || !src) return ctx ? dp_fail(ctx, DP_ERR_ARG, "dp_index_borrow: bad arguments") : DP_ERR_ARG;
    if (ctx->owner != src || src->owner) return dp_fail(ctx, DP_ERR_ARG, "dp_index_borrow: the context was not made by dp_ctx_create_shared(src)");
    if (!src->index_sparse || src->index_src) return dp_fail(ctx, DP_ERR_STATE, "dp_index_borrow: the source holds no sparse index of its own");
    if (!ctx->round_open || ctx->n_seeds != src->n_seeds) return dp_fail(ctx, DP_ERR_STATE, "dp_index_borrow: the round's seeds differ from the source's");
    ctx->index_sparse = true;
    ctx->index_src = src;
    ctx->n_seqs = src->n_seqs;
    ctx->W = src->W;
    ctx->SW = src->SW;
    ctx->max_seq_seeds = src->max_seq_seeds;
    ctx->word_base = src->word_base;
    ctx->global_n_seqs = src->global_n_seqs;
    ctx->chunks_on_device = false;
    ctx->sp_entries = src->sp_entries;
    return DP_OK;
}

extern "C" int dp_index_info(dp_ctx* ctx, dp_index_info_t* out) {
    if (!ctx || !out) return ctx ? dp_fail(ctx, DP_ERR_ARG, "dp_index_info: bad arguments") : DP_ERR_ARG;
    memset(out, 0, sizeof(*out));
    for (int r = 0; r < 4; r++) out->queries[r] = ctx->map_regimes[r];
    out->n_seeds = ctx->n_seeds;
    out->n_seqs = ctx->n_seqs;
    if (ctx->index_sparse) {
        out->layout = DP_INDEX_SPARSE;
        out->borrowed = ctx->index_src ? 1u : 0u;
        out->device_bytes = dp_index_sparse_bytes(dp_index_of(ctx));
        out->entries = ctx->sp_entries;
        return DP_OK;
    }
    if (!ctx->d_pmeta.p || !ctx->W) return DP_OK;  // (no index yet)
    out->layout = DP_INDEX_DENSE;  // (entries stay 0: the bit matrices do not count them; the pmeta rows do)
    const uint64_t S = ctx->n_seeds;
    out->device_bytes = S * ctx->W * 8 + (uint64_t)ctx->n_seqs * ctx->SW * 8 + 16 * S + (uint64_t)sizeof(dp_seq_ref) * ctx->n_seqs;
    return DP_OK;
}

int dp_index_sparse_row(dp_ctx* ctx, int side, uint32_t row, uint64_t* words, uint32_t cap_words, uint32_t* n_words, uint32_t* count,
                        uint32_t* start, uint32_t* end) {
    const dp_ctx* ix = dp_index_of(ctx);
    hipSetDevice(ctx->device);
    const uint32_t nw = side == 0 ? ctx->W : ctx->SW;
    const DevBuf& offb = side == 0 ? ix->d_sp_post_off : ix->d_sp_set_off;
    const DevBuf& idb = side == 0 ? ix->d_sp_post_ids : ix->d_sp_set_ids;
    u64 o[2] = {0, 0};
    DP_HIP(hipMemcpyAsync(o, (const u64*)offb.p + row, 16, hipMemcpyDeviceToHost, ctx->stream));
    DP_HIP(dp_stream_sync(ctx));
    std::vector<uint32_t> ids((size_t)(o[1] - o[0]));
    if (!ids.empty()) {
        DP_HIP(hipMemcpyAsync(ids.data(), (const uint32_t*)idb.p + o[0], ids.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        DP_HIP(dp_stream_sync(ctx));
    }
    memset(words, 0, (size_t)nw * 8);
    for (uint32_t id : ids) {
        if (id >= 64ull * nw || (id >> 6) >= cap_words) return dp_fail(ctx, DP_ERR_STATE, "dp_index_sparse_row: id outside the row");
        words[id >> 6] |= 1ull << (id & 63);
    }
    if (n_words) *n_words = nw;
    if (side == 0) {
        uint32_t meta[4];
        DP_HIP(hipMemcpy(meta, (const uint32_t*)ix->d_pmeta.p + 4 * (size_t)row, 16, hipMemcpyDeviceToHost));
        if (count) *count = meta[0];
        if (start) *start = meta[1];
        if (end) *end = meta[2];
    }
    return DP_OK;
}

extern "C" int dp_device_memory(int device, uint64_t* free_bytes, uint64_t* total_bytes) {
    if (!free_bytes || !total_bytes) return DP_ERR_ARG;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return dp_fail(nullptr, DP_ERR_NODEVICE, "no HIP device (this library has no CPU fallback)", e);
    if (device < 0 || device >= n) return dp_fail(nullptr, DP_ERR_ARG, "device index out of range");
    hipSetDevice(device);
    size_t f = 0, t = 0;
    if ((e = hipMemGetInfo(&f, &t)) != hipSuccess) return dp_fail(nullptr, DP_ERR_HIP, "hipMemGetInfo", e);
    *free_bytes = (uint64_t)f + dp_dev_cached_bytes();  // (blocks the library has parked count as free)
    *total_bytes = (uint64_t)t;
    return DP_OK;
}
