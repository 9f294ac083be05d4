// libdownpore_hip.so — the edge stage of `trim`: findMatches / isNewFullMatch of trim/trim.go:326-428 for batches of read ends.
// CDNA4 / gfx950 only.
//
// One wave64 per 150-base read end:
//   1. the end's k-mers looked up in the adapter index's k-mer -> seed table (ShortKmers + GetSeedsFromKmers, sequence.go:482-504,
//      seeds.go:247-253) give its seed set - a bitset over seed ids in LDS - and its NewSeedSequence segments (seeds.go:33-50,
//      sequence.go:308-324) by ballot + prefix over the k-mer positions;
//   2. CountIntersection with every adapter row of the end's side, one adapter per lane, and the reference's gate
//      (trim: hits*10/size >= 2 || hits >= 3, :365-366; determine: hits >= size/2, :333-334); the passing adapters stay in adapter order;
//   3. SeedSequence.Match(adapter, adapterSet, edgeSet, minMatch, k) per passing adapter with the device functions map_kernel
//      uses (dp_match.h), then GetBasesCovered (seeds/sequence.go:830-858) and the start / end arithmetic of :397-410 on lane 0;
//   4. the barcode / ambiguity / best-identity state machine of :377-395 folded in adapter order, then dynamicMatch's return
//      order, so that one 24-byte record per end goes back (and counts[i]++ per reported match, :416).
// LDS per wave is sized from the longest uploaded adapter; the k-mer table sits in LDS when 4^k entries are <= 8 KB (k <= 6).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "dp_match.h"

#define TR_WAVES 4
#define TR_EDGE 150                  // edgeSize (trim.go:432,453)
#define TR_TCAP 152                  // seeds of an end: <= 150 - k + 1
#define TR_MAX_ADAPTER 512           // bases of the longest adapter the LDS working set is sized for (DP_TRIM_MAX_ADAPTER)
#define TR_MAX_SEEDS 16384           // distinct seeds of the adapter index (256 set words per end)
#define TR_NONE 0xffffu

struct TrimL {  // the working set dp_match.h's functions expect; the arrays live in the wave's slice of dynamic LDS
    int32_t* q;
    int32_t* t;
    uint16_t* qIdx;
    uint16_t* tIdx;
    int32_t* headChain;
    uint16_t* headLen;
    int32_t good[M_GOOD];
};

struct TrimGeom {
    int k;
    uint32_t n_front, n_back, SW, qcap;
    uint32_t table_bytes;  // bytes of the k-mer table copied into LDS (0: read through L2)
    uint32_t wave_words;   // 4-byte words of a wave's LDS slice
};
// a wave's slice: [set u64 x SW][eseg][t][q][headChain][tIdx][qIdx][headLen][codes]
static __host__ __device__ inline uint32_t tr_wave_words(uint32_t SW, uint32_t qcap) {
    return 2 * SW + (2 * TR_TCAP + 2) * 2 + (2 * qcap + 2) + (qcap + 2) + TR_TCAP / 2 + (qcap + 2) / 2 * 2 + TR_TCAP / 4 + 2;
}

// one thread per adapter: its seed-set row (row-major for Reduced's whitelist probes, transposed for the prefilter) and size
__global__ void trim_rows_kernel(const int32_t* __restrict__ segs, const uint32_t* __restrict__ seg_off, uint32_t nA, uint32_t SW,
                                 u64* __restrict__ rows, u64* __restrict__ rowsT, int32_t* __restrict__ size) {
    const uint32_t a = blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= nA) return;
    u64* row = rows + (size_t)a * SW;
    for (uint32_t i = seg_off[a] + 1; i < seg_off[a + 1]; i += 2) {
        const uint32_t s = (uint32_t)segs[i];
        row[s >> 6] |= 1ull << (s & 63);
    }
    int c = 0;
    for (uint32_t w = 0; w < SW; w++) {
        const u64 v = row[w];
        rowsT[(size_t)w * nA + a] = v;
        c += __popcll(v);
    }
    size[a] = c;
}

__device__ __forceinline__ int tr_seed_offset(const int32_t* seg, int index, int k) {  // GetSeedOffset (seeds/sequence.go:1239-1246)
    index = index * 2 + 1;
    int o = seg[0];
    for (int i = 2; i < index; i += 2) o += seg[i] + k;
    return o;
}
__device__ __forceinline__ int tr_seed_offset_from_end(const int32_t* seg, int n, int index, int k) {  // :1269-1276
    index = index * 2 + 1;
    int o = seg[n - 1];
    for (int i = n - 3; i > index; i -= 2) o += seg[i] + k;
    return o;
}

// errbits: 1 reduced sequence beyond its array, 2 chain pool, 4 good-chain list (dp_match.h)
__global__ __launch_bounds__(64 * TR_WAVES) void trim_edge_kernel(
    const uint8_t* __restrict__ ends, uint32_t n_ends, TrimGeom G, const uint16_t* __restrict__ table, const int32_t* __restrict__ asegs,
    const uint32_t* __restrict__ aoff, const int32_t* __restrict__ alen, const uint8_t* __restrict__ abar, const int32_t* __restrict__ asize,
    const u64* __restrict__ rows, const u64* __restrict__ rowsT, int mode, int min_match, int threshold, dp_trim_rec* __restrict__ recs,
    unsigned long long* __restrict__ counts, uint32_t* __restrict__ enabled, uint16_t* __restrict__ poolA, uint16_t* __restrict__ poolB,
    uint16_t* __restrict__ poolLen, uint32_t* __restrict__ errbits) {
    extern __shared__ __attribute__((aligned(16))) uint32_t tr_lds[];
    __shared__ TrimL sh[TR_WAVES];
    const int lane = dp_lane();
    const int wv = threadIdx.x >> 6;
    const int k = G.k;
    const uint32_t nA = G.n_front + G.n_back, SW = G.SW, qcap = G.qcap;
    // the k-mer table: in LDS when it was sized in (k <= 6), else through L2
    const uint16_t* tab = table;
    if (G.table_bytes) {
        uint16_t* lt = (uint16_t*)tr_lds;
        for (uint32_t i = threadIdx.x; i < G.table_bytes / 2; i += blockDim.x) lt[i] = table[i];
        tab = lt;
    }
    uint32_t* base = tr_lds + G.table_bytes / 4 + (size_t)wv * G.wave_words;
    u64* set = (u64*)base;
    int32_t* eseg = (int32_t*)(base + 2 * SW);
    uint8_t* codes;
    TrimL& L = sh[wv];
    {
        uint32_t* p = base + 2 * SW + (2 * TR_TCAP + 2);
        int32_t* t = (int32_t*)p;
        p += 2 * TR_TCAP + 2;
        int32_t* q = (int32_t*)p;
        p += 2 * qcap + 2;
        int32_t* hc = (int32_t*)p;
        p += qcap + 2;
        uint16_t* tI = (uint16_t*)p;
        p += TR_TCAP / 2;
        uint16_t* qI = (uint16_t*)p;
        p += (qcap + 2) / 2;
        uint16_t* hl = (uint16_t*)p;
        p += (qcap + 2) / 2;
        codes = (uint8_t*)p;
        if (lane == 0) {
            L.t = t;
            L.q = q;
            L.headChain = hc;
            L.tIdx = tI;
            L.qIdx = qI;
            L.headLen = hl;
        }
    }
    __syncthreads();
    const uint32_t gw = blockIdx.x * TR_WAVES + wv, waves = gridDim.x * TR_WAVES;
    MChainPool P;
    P.stride = qcap;
    P.a = poolA + (size_t)gw * M_CHAINS * qcap;
    P.b = poolB + (size_t)gw * M_CHAINS * qcap;
    uint16_t* chainLen = poolLen + (size_t)gw * M_CHAINS;
    const u64 below = (1ull << lane) - 1ull;
    const int nK = TR_EDGE - k + 1;
    uint32_t err = 0;
    for (uint32_t e = gw; e < n_ends; e += waves) {
        // ---- 1. the end's base codes, seed set and segments
        const uint8_t* src = ends + (size_t)e * TR_EDGE;
        for (int i = lane; i < TR_EDGE; i += 64) {
            const uint32_t b = src[i];
            codes[i] = (uint8_t)(((b >> 1) ^ ((b & 4) >> 2)) & 3);
        }
        for (uint32_t w = lane; w < SW; w += 64) set[w] = 0;
        __builtin_amdgcn_wave_barrier();
        int nE = 0, lastPos = -1;  // seeds so far, k-mer index of the last one
        for (int pb = 0; pb < nK; pb += 64) {
            const int p = pb + lane;
            uint32_t sid = TR_NONE;
            if (p < nK) {
                uint32_t km = 0;
                for (int j = 0; j < k; j++) km = (km << 2) | codes[p + j];
                sid = tab[km];
            }
            const bool is = sid != TR_NONE;
            if (is) atomicOr((uint32_t*)set + (sid >> 5), 1u << (sid & 31));
            const u64 m = __ballot(is);
            if (is) {
                const u64 mb = m & below;
                const int prev = mb ? pb + 63 - __builtin_clzll(mb) : lastPos;
                const int j = nE + __popcll(mb);
                eseg[2 * j] = p - (prev < 0 ? 0 : prev + k);  // kmerIndex - prev (sequence.go:316-318)
                eseg[2 * j + 1] = (int32_t)sid;
            }
            nE += __popcll(m);
            if (m) lastPos = pb + 63 - __builtin_clzll(m);
        }
        if (lane == 0) eseg[2 * nE] = TR_EDGE - (lastPos < 0 ? 0 : lastPos + k);  // len - prev (:323)
        __builtin_amdgcn_wave_barrier();
        const int eN = 2 * nE + 1;
        // ---- 2..4. the adapters of this end's side, in order
        const uint32_t side = e & 1u;
        const uint32_t a0 = side ? G.n_front : 0u, nSide = side ? G.n_back : G.n_front;
        int earliest = TR_EDGE, latest = 0, found = 0, bestMatch = 0, bestIdent = 0, barcoded = 0, ambiguous = 0;  // (lane 0's are the truth)
        for (uint32_t ab = 0; ab < nSide; ab += 64) {
            const uint32_t a = a0 + ab + lane;
            bool pass = false;
            if (ab + lane < nSide && !(mode == 1 && enabled[a])) {  // (:329-331 "we already know this is a good adapter")
                int hits = 0;
                for (uint32_t w = 0; w < SW; w++) hits += __popcll(set[w] & rowsT[(size_t)w * nA + a]);
                const int size = asize[a];
                pass = mode == 0 ? ((hits * 10) / size >= 2 || hits >= 3) : hits >= size / 2;
            }
            u64 pm = __ballot(pass);
            while (pm) {
                const int bit = __builtin_ctzll(pm);
                pm &= pm - 1;
                const uint32_t ai = a0 + ab + (uint32_t)bit;
                const int32_t* aSeg = asegs + aoff[ai];
                const int aN = (int)(aoff[ai + 1] - aoff[ai]);
                const int minHits = asize[ai] / 2;
                const int minMatch = mode == 0 ? min_match : minHits - 1;
                // Match (seeds/sequence.go:361-394): the end reduced to the adapter's seeds, the adapter to the end's
                const int nT = m_reduce_wave<uint16_t>(eseg, eN, (const u64*)(rows + (size_t)ai * SW), k, minMatch, L.t, L.tIdx, TR_TCAP, &err);
                const int nQ = nT < 0 ? -1 : m_reduce_wave<uint16_t>(aSeg, aN, (const u64*)set, k, minMatch, L.q, L.qIdx, (int)qcap, &err);
                int nGood = 0;
                if (nT >= 0 && nQ >= 0) nGood = m_dynamic_match_wave(L, 2 * nQ + 1, 2 * nT + 1, minMatch, k, P, chainLen, &err);
                if (lane == 0) {  // (lane 0 wrote the chains and reads them back itself)
                    for (int g = 0; g < nGood; g++) {
                        const int ch = L.good[g];
                        const int len = chainLen[ch];
                        if (len < (mode == 0 ? min_match : minHits)) continue;  // :374 / :342
                        const uint16_t* ca = P.A(ch);
                        const uint16_t* cb = P.B(ch);
                        // GetBasesCovered's countA (:830-858): SeqA = the adapter
                        int countA = len * k, prevA = L.qIdx[ca[0]];
                        for (int i = 1; i < len; i++) {
                            const int s = L.qIdx[ca[i]];
                            int d1 = aSeg[prevA * 2 + 2];
                            for (int j = prevA + 2; j <= s; j++) d1 += aSeg[j * 2] + k;
                            if (d1 < 0) countA += d1;
                            prevA = s;
                        }
                        const int identity = (countA * 100) / alen[ai];
                        if (mode == 1) {
                            if (identity >= threshold) enabled[ai] = 1u;  // :344-346
                            continue;
                        }
                        const bool isBarcode = abar[ai] != 0;
                        if (!barcoded && isBarcode) {  // :378-395
                            barcoded = 1;
                            bestIdent = identity;
                            bestMatch = (int)(ai - a0);
                        } else if (barcoded) {
                            if (isBarcode) {
                                const int delta = identity - bestIdent;
                                ambiguous = delta < 5 && delta > -5;
                                if (identity > bestIdent) {
                                    bestIdent = identity;
                                    bestMatch = (int)(ai - a0);
                                }
                            }
                        } else if (identity > bestIdent) {
                            bestIdent = identity;
                            bestMatch = (int)(ai - a0);
                        }
                        // :397-410 (both offsets are added, as the reference does)
                        int start = tr_seed_offset(eseg, L.tIdx[cb[0]], k) + tr_seed_offset(aSeg, L.qIdx[ca[0]], k);
                        int end = tr_seed_offset(eseg, L.tIdx[cb[len - 1]], k) + tr_seed_offset_from_end(aSeg, aN, L.qIdx[ca[len - 1]], k);
                        if (start < earliest) {
                            if (start < 0) start = 0;
                            earliest = start;
                        }
                        if (end > latest) {
                            if (end > TR_EDGE) end = TR_EDGE;
                            latest = end;
                        }
                        found = 1;
                        atomicAdd(&counts[ai], 1ull);  // :416
                    }
                }
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (lane == 0 && mode == 0) {
            dp_trim_rec r;
            r.earliest = earliest;
            r.latest = latest;
            r.found = found;
            r.best_match = bestMatch;
            r.ambiguous = ambiguous;
            r.best_ident = bestIdent;
            recs[e] = r;
        }
        __builtin_amdgcn_wave_barrier();
    }
    if (lane == 0 && err) atomicOr(errbits, err);
}

// ---------------------------------------------------------------------------------------------------------------
struct dp_trim {
    int device = 0, k = 0;
    uint32_t n_front = 0, n_back = 0, n_seeds = 0, SW = 0, qcap = 0, waves = 0;
    size_t lds_bytes = 0;
    TrimGeom G;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    void *d_table = nullptr, *d_segs = nullptr, *d_off = nullptr, *d_len = nullptr, *d_bar = nullptr, *d_size = nullptr, *d_rows = nullptr,
         *d_rowsT = nullptr, *d_counts = nullptr, *d_enabled = nullptr, *d_pool = nullptr, *d_err = nullptr, *d_ends = nullptr, *d_recs = nullptr;
    size_t ends_cap = 0;          // read ends the batch buffers hold
    std::vector<int32_t> pairs;   // the pair ids as uploaded (pairing is the host's rule, trim.go:471-485)
    std::string err;
};
static thread_local std::string g_trim_err;

static int tr_fail(dp_trim* t, int code, const std::string& what, hipError_t e = hipSuccess) {
    std::string s = what;
    if (e != hipSuccess) {
        s += ": ";
        s += hipGetErrorString(e);
    }
    if (t) t->err = s;
    g_trim_err = s;
    return code;
}

extern "C" const char* dp_trim_error(const dp_trim* t) { return t ? t->err.c_str() : g_trim_err.c_str(); }

extern "C" void dp_trim_release(dp_trim* t) {
    if (!t) return;
    hipSetDevice(t->device);
    if (t->stream) hipStreamSynchronize(t->stream);
    for (void* p : {t->d_table, t->d_segs, t->d_off, t->d_len, t->d_bar, t->d_size, t->d_rows, t->d_rowsT, t->d_counts, t->d_enabled, t->d_pool,
                    t->d_err, t->d_ends, t->d_recs})
        if (p) dp_dev_free(p);
    for (hipEvent_t e : t->ev)
        if (e) hipEventDestroy(e);
    if (t->stream) hipStreamDestroy(t->stream);
    delete t;
}

#define TR_HIP(call)                                                       \
    do {                                                                   \
        hipError_t e_ = (call);                                            \
        if (e_ != hipSuccess) {                                            \
            const int rc_ = tr_fail(t, DP_ERR_HIP, "dp_trim: " #call, e_); \
            if (own) dp_trim_release(t);                                   \
            return rc_;                                                    \
        }                                                                  \
    } while (0)

extern "C" int dp_trim_setup(int device, int k, const uint16_t* kmer_seed, uint32_t n_seeds, uint32_t n_front, uint32_t n_back,
                             const int32_t* segs, const uint64_t* seg_off, const int32_t* lengths, const uint8_t* is_barcode,
                             const int32_t* pair_ids, dp_trim** out) {
    if (out) *out = nullptr;
    if (!out || !kmer_seed || !segs || !seg_off || !lengths || !is_barcode) return tr_fail(nullptr, DP_ERR_ARG, "dp_trim_setup: null argument");
    if (k < 3 || k > 8) return tr_fail(nullptr, DP_ERR_ARG, "dp_trim_setup: k = " + std::to_string(k) + " is outside 3..8 (ShortKmers holds a k-mer in 16 bits)");
    const uint32_t nA = n_front + n_back;
    if (nA == 0) return tr_fail(nullptr, DP_ERR_ARG, "dp_trim_setup: no adapters");
    if (n_seeds == 0 || n_seeds > TR_MAX_SEEDS)
        return tr_fail(nullptr, DP_ERR_CAPACITY, "dp_trim_setup: " + std::to_string(n_seeds) + " distinct adapter seeds (limit " + std::to_string(TR_MAX_SEEDS) + ")");
    const size_t nK = (size_t)1 << (2 * k);
    for (size_t i = 0; i < nK; i++)
        if (kmer_seed[i] != TR_NONE && kmer_seed[i] >= n_seeds) return tr_fail(nullptr, DP_ERR_ARG, "dp_trim_setup: k-mer table entry beyond the seed count");
    int longest = 0;
    std::vector<uint32_t> off32(nA + 1);
    for (uint32_t a = 0; a <= nA; a++) {
        if (seg_off[a] > 0x7fffffffull || (a && seg_off[a] < seg_off[a - 1])) return tr_fail(nullptr, DP_ERR_ARG, "dp_trim_setup: segment offsets");
        off32[a] = (uint32_t)seg_off[a];
    }
    std::vector<uint64_t> seen((n_seeds + 63) / 64);
    for (uint32_t a = 0; a < nA; a++) {
        const uint32_t n = off32[a + 1] - off32[a];
        if (!(n & 1u)) return tr_fail(nullptr, DP_ERR_ARG, "dp_trim_setup: an adapter's segments are [gap, seed, ..., gap]");
        if (lengths[a] > TR_MAX_ADAPTER)
            return tr_fail(nullptr, DP_ERR_CAPACITY, "dp_trim_setup: adapter " + std::to_string(a) + " has " + std::to_string(lengths[a]) +
                                                         " bases; the longest adapter this build matches has " + std::to_string(TR_MAX_ADAPTER));
        std::fill(seen.begin(), seen.end(), 0);
        int distinct = 0;
        for (uint32_t i = off32[a] + 1; i < off32[a + 1]; i += 2) {
            if (segs[i] < 0 || (uint32_t)segs[i] >= n_seeds) return tr_fail(nullptr, DP_ERR_ARG, "dp_trim_setup: adapter seed beyond the seed count");
            uint64_t& w = seen[(uint32_t)segs[i] >> 6];
            distinct += !((w >> (segs[i] & 63)) & 1);
            w |= 1ull << (segs[i] & 63);
        }
        // (fewer than two distinct seeds: the reference divides by the set's size and chains with minMatch = size / 2 - 1 = -1)
        if (distinct < 2 || lengths[a] < k + 1)
            return tr_fail(nullptr, DP_ERR_ARG, "dp_trim_setup: adapter " + std::to_string(a) + " has fewer than two distinct " + std::to_string(k) + "-mers");
        if ((int)(n / 2) > TR_MAX_ADAPTER) return tr_fail(nullptr, DP_ERR_CAPACITY, "dp_trim_setup: adapter with more seeds than bases");
        longest = std::max(longest, (int)(n / 2));
    }
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || device < 0 || device >= nd) return tr_fail(nullptr, DP_ERR_NODEVICE, "dp_trim_setup: no usable GPU (there is no CPU fallback)");
    dp_trim* t = new dp_trim();
    const bool own = true;
    t->device = device;
    t->k = k;
    t->n_front = n_front;
    t->n_back = n_back;
    t->n_seeds = n_seeds;
    t->SW = (n_seeds + 63) / 64;
    t->qcap = std::max<uint32_t>(64u, ((uint32_t)longest + 31u) & ~31u);
    if (pair_ids) t->pairs.assign(pair_ids, pair_ids + nA);
    TR_HIP(hipSetDevice(device));
    TR_HIP(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    for (hipEvent_t& e : t->ev) TR_HIP(hipEventCreate(&e));
    const size_t nSegs = off32[nA];
    TR_HIP(dp_dev_malloc(&t->d_table, nK * 2 + 64));
    TR_HIP(dp_dev_malloc(&t->d_segs, nSegs * 4 + 64));
    TR_HIP(dp_dev_malloc(&t->d_off, ((size_t)nA + 1) * 4 + 64));
    TR_HIP(dp_dev_malloc(&t->d_len, (size_t)nA * 4 + 64));
    TR_HIP(dp_dev_malloc(&t->d_bar, (size_t)nA + 64));
    TR_HIP(dp_dev_malloc(&t->d_size, (size_t)nA * 4 + 64));
    TR_HIP(dp_dev_malloc(&t->d_rows, (size_t)nA * t->SW * 8 + 64));
    TR_HIP(dp_dev_malloc(&t->d_rowsT, (size_t)nA * t->SW * 8 + 64));
    TR_HIP(dp_dev_malloc(&t->d_counts, (size_t)nA * 8 + 64));
    TR_HIP(dp_dev_malloc(&t->d_enabled, (size_t)nA * 4 + 64));
    TR_HIP(dp_dev_malloc(&t->d_err, 64));
    TR_HIP(hipMemcpyAsync(t->d_table, kmer_seed, nK * 2, hipMemcpyHostToDevice, t->stream));
    TR_HIP(hipMemcpyAsync(t->d_segs, segs, nSegs * 4, hipMemcpyHostToDevice, t->stream));
    TR_HIP(hipMemcpyAsync(t->d_off, off32.data(), ((size_t)nA + 1) * 4, hipMemcpyHostToDevice, t->stream));
    TR_HIP(hipMemcpyAsync(t->d_len, lengths, (size_t)nA * 4, hipMemcpyHostToDevice, t->stream));
    TR_HIP(hipMemcpyAsync(t->d_bar, is_barcode, (size_t)nA, hipMemcpyHostToDevice, t->stream));
    TR_HIP(hipMemsetAsync(t->d_rows, 0, (size_t)nA * t->SW * 8, t->stream));
    TR_HIP(hipMemsetAsync(t->d_counts, 0, (size_t)nA * 8, t->stream));
    TR_HIP(hipMemsetAsync(t->d_enabled, 0, (size_t)nA * 4, t->stream));
    hipLaunchKernelGGL(trim_rows_kernel, dim3((nA + 63) / 64), dim3(64), 0, t->stream, (const int32_t*)t->d_segs, (const uint32_t*)t->d_off, nA, t->SW,
                       (u64*)t->d_rows, (u64*)t->d_rowsT, (int32_t*)t->d_size);
    TR_HIP(hipGetLastError());
    // the edge kernel's LDS: the table (k <= 6) + four wave slices sized from the longest adapter
    t->G.k = k;
    t->G.n_front = n_front;
    t->G.n_back = n_back;
    t->G.SW = t->SW;
    t->G.qcap = t->qcap;
    t->G.table_bytes = nK * 2 <= 8192 ? (uint32_t)(nK * 2) : 0u;
    t->G.wave_words = (tr_wave_words(t->SW, t->qcap) + 1u) & ~1u;
    t->lds_bytes = (size_t)t->G.table_bytes + (size_t)TR_WAVES * t->G.wave_words * 4;
    TR_HIP(hipFuncSetAttribute((const void*)trim_edge_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)t->lds_bytes));
    // chain pool (dp_match.h: M_CHAINS slots of qcap links per wave, two arrays): as many persistent waves as 1 GiB of it allows
    const size_t per_wave = (size_t)M_CHAINS * t->qcap * 4 + (size_t)M_CHAINS * 2;
    size_t waves = std::min<size_t>(2048, ((size_t)1 << 30) / per_wave);
    waves = std::max<size_t>(TR_WAVES, waves / TR_WAVES * TR_WAVES);
    t->waves = (uint32_t)waves;
    TR_HIP(dp_dev_malloc(&t->d_pool, waves * per_wave + 64));
    TR_HIP(hipStreamSynchronize(t->stream));
    *out = t;
    return DP_OK;
}

extern "C" int dp_trim_edges(dp_trim* t, const uint8_t* ends, uint32_t n_reads, int mode, int min_match, int threshold, dp_trim_rec* recs,
                             uint64_t* counts, uint8_t* enabled, double* times_ms) {
    if (!t) return tr_fail(nullptr, DP_ERR_ARG, "dp_trim_edges: null handle");
    const bool own = false;
    if ((mode != DP_TRIM_MODE_TRIM && mode != DP_TRIM_MODE_DETERMINE) || (n_reads && !ends) || (mode == DP_TRIM_MODE_TRIM && n_reads && !recs))
        return tr_fail(t, DP_ERR_ARG, "dp_trim_edges: bad arguments");
    if (mode == DP_TRIM_MODE_TRIM && min_match < 1) return tr_fail(t, DP_ERR_ARG, "dp_trim_edges: min_match < 1");
    if (n_reads > 0x3fffffffu) return tr_fail(t, DP_ERR_ARG, "dp_trim_edges: batch too large");
    TR_HIP(hipSetDevice(t->device));
    const uint32_t nA = t->n_front + t->n_back, n_ends = 2 * n_reads;
    if (times_ms) times_ms[0] = times_ms[1] = times_ms[2] = 0;
    if (n_ends) {
        if (n_ends > t->ends_cap) {
            if (t->d_ends) dp_dev_free(t->d_ends);
            if (t->d_recs) dp_dev_free(t->d_recs);
            t->d_ends = t->d_recs = nullptr;
            t->ends_cap = 0;
            const size_t cap = std::max<size_t>(n_ends, 1u << 16);
            TR_HIP(dp_dev_malloc(&t->d_ends, cap * TR_EDGE + 64));
            TR_HIP(dp_dev_malloc(&t->d_recs, cap * sizeof(dp_trim_rec) + 64));
            t->ends_cap = cap;
        }
        TR_HIP(hipMemsetAsync(t->d_err, 0, 64, t->stream));
        TR_HIP(hipEventRecord(t->ev[0], t->stream));
        TR_HIP(hipMemcpyAsync(t->d_ends, ends, (size_t)n_ends * TR_EDGE, hipMemcpyHostToDevice, t->stream));
        TR_HIP(hipEventRecord(t->ev[1], t->stream));
        const uint32_t blocks = std::min<uint32_t>(t->waves / TR_WAVES, (n_ends + TR_WAVES - 1) / TR_WAVES);
        const size_t poolElems = (size_t)t->waves * M_CHAINS * t->qcap;
        uint16_t* poolA = (uint16_t*)t->d_pool;
        hipLaunchKernelGGL(trim_edge_kernel, dim3(blocks), dim3(64 * TR_WAVES), t->lds_bytes, t->stream, (const uint8_t*)t->d_ends, n_ends, t->G,
                           (const uint16_t*)t->d_table, (const int32_t*)t->d_segs, (const uint32_t*)t->d_off, (const int32_t*)t->d_len,
                           (const uint8_t*)t->d_bar, (const int32_t*)t->d_size, (const u64*)t->d_rows, (const u64*)t->d_rowsT, mode, min_match,
                           threshold, (dp_trim_rec*)t->d_recs, (unsigned long long*)t->d_counts, (uint32_t*)t->d_enabled, poolA, poolA + poolElems,
                           poolA + 2 * poolElems, (uint32_t*)t->d_err);
        TR_HIP(hipGetLastError());
        TR_HIP(hipEventRecord(t->ev[2], t->stream));
        uint32_t errbits = 0;
        if (mode == DP_TRIM_MODE_TRIM) TR_HIP(hipMemcpyAsync(recs, t->d_recs, (size_t)n_ends * sizeof(dp_trim_rec), hipMemcpyDeviceToHost, t->stream));
        TR_HIP(hipMemcpyAsync(&errbits, t->d_err, 4, hipMemcpyDeviceToHost, t->stream));
        TR_HIP(hipEventRecord(t->ev[3], t->stream));
        TR_HIP(hipStreamSynchronize(t->stream));
        if (times_ms)
            for (int i = 0; i < 3; i++) {
                float ms = 0;
                if (hipEventElapsedTime(&ms, t->ev[i], t->ev[i + 1]) == hipSuccess) times_ms[i] = ms;
            }
        if (errbits) return tr_fail(t, DP_ERR_CAPACITY, "dp_trim_edges: chaining exceeded a device capacity (bits " + std::to_string(errbits) +
                                                            ": 1 reduced sequence, 2 chain pool, 4 good-chain list)");
    }
    if (counts) TR_HIP(hipMemcpy(counts, t->d_counts, (size_t)nA * 8, hipMemcpyDeviceToHost));
    if (enabled) {
        std::vector<uint32_t> en(nA);
        TR_HIP(hipMemcpy(en.data(), t->d_enabled, (size_t)nA * 4, hipMemcpyDeviceToHost));
        for (uint32_t a = 0; a < nA; a++) enabled[a] = en[a] ? 1 : 0;
    }
    return DP_OK;
}
