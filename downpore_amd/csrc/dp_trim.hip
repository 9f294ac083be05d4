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
#define TR_MAX_ADAPTER 512           // bases of the longest adapter the LDS working set is sized for
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
// The chaining working set for a target of tcap and a query of qcap reduced seeds, in 4-byte words from `base`: the one list of its
// fields.  Returns the words it takes; with L it also points L's arrays at them.
static __host__ __device__ inline uint32_t tr_chain_set(uint32_t tcap, uint32_t qcap, uint32_t* base = nullptr, TrimL* L = nullptr) {
    uint32_t w = 0;
#define TR_FIELD(name, words)                               \
    do {                                                    \
        if (L) L->name = (decltype(L->name))(base + w);     \
        w += (words);                                       \
    } while (0)
    TR_FIELD(t, 2 * tcap + 2);
    TR_FIELD(q, 2 * qcap + 2);
    TR_FIELD(headChain, qcap + 2);
    TR_FIELD(tIdx, tcap / 2);
    TR_FIELD(qIdx, (qcap + 2) / 2);
    TR_FIELD(headLen, (qcap + 2) / 2);
#undef TR_FIELD
    return w;
}
// a wave's slice in trim_edge_kernel: [set u64 x SW][eseg][the chaining working set][codes], and two words to spare
#define TR_ESEG_WORDS (2 * TR_TCAP + 2)
#define TR_CODE_WORDS (TR_TCAP / 4)
static inline uint32_t tr_wave_words(uint32_t SW, uint32_t qcap) { return 2 * SW + TR_ESEG_WORDS + tr_chain_set(TR_TCAP, qcap) + TR_CODE_WORDS + 2; }

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

// NewSeedSequence's segment emission (seeds.go:33-50, sequence.go:308-324) for the 64 k-mer positions pb .. pb + 63: the lane's
// position pb + lane holds seed `sid` (TR_NONE: none).  The seed that is the j-th of the sequence gets its [gap, seed] at seg[2 j]
// when j < cap; nE (seeds so far) and lastPos (k-mer index of the last one, -1: none yet) advance.  POS: int for a read end, 64 bits
// for a chunk of any length.
template <typename POS>
__device__ __forceinline__ void tr_scan_step(uint32_t sid, POS pb, int k, uint32_t& nE, POS& lastPos, int32_t* seg, uint32_t cap) {
    const bool is = sid != TR_NONE;
    const u64 m = __ballot(is);
    if (is) {
        const u64 mb = m & ((1ull << dp_lane()) - 1ull);
        const POS prev = mb ? pb + 63 - __builtin_clzll(mb) : lastPos;
        const uint32_t j = nE + (uint32_t)__popcll(mb);
        if (j < cap) {
            seg[2 * (size_t)j] = (int32_t)(pb + dp_lane() - (prev < 0 ? 0 : prev + k));  // kmerIndex - prev (sequence.go:316-318)
            seg[2 * (size_t)j + 1] = (int32_t)sid;
        }
    }
    nE += (uint32_t)__popcll(m);
    if (m) lastPos = pb + 63 - __builtin_clzll(m);
}

// GetBasesCovered's countA (seeds/sequence.go:830-858) of a chain of len links: SeqA = the adapter, ca = its links into the reduced adapter
__device__ __forceinline__ int tr_count_a(const int32_t* aSeg, const uint16_t* qIdx, const uint16_t* ca, int len, int k) {
    int countA = len * k, prevA = qIdx[ca[0]];
    for (int i = 1; i < len; i++) {
        const int s = qIdx[ca[i]];
        int d1 = aSeg[prevA * 2 + 2];
        for (int j = prevA + 2; j <= s; j++) d1 += aSeg[j * 2] + k;
        if (d1 < 0) countA += d1;
        prevA = s;
    }
    return countA;
}

// wave gw's part of the chain pool (dp_match.h): M_CHAINS slots of qcap links in each of two arrays, and the chains' lengths
__device__ __forceinline__ MChainPool tr_wave_pool(uint32_t gw, uint32_t qcap, uint16_t* poolA, uint16_t* poolB, uint16_t* poolLen, uint16_t** chainLen) {
    MChainPool P;
    P.stride = qcap;
    P.a = poolA + (size_t)gw * M_CHAINS * qcap;
    P.b = poolB + (size_t)gw * M_CHAINS * qcap;
    *chainLen = poolLen + (size_t)gw * M_CHAINS;
    return P;
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
    uint32_t* chain = base + 2 * SW + TR_ESEG_WORDS;
    TrimL& L = sh[wv];
    uint8_t* codes = (uint8_t*)(chain + tr_chain_set(TR_TCAP, qcap, chain, lane == 0 ? &L : nullptr));
    __syncthreads();
    const uint32_t gw = blockIdx.x * TR_WAVES + wv, waves = gridDim.x * TR_WAVES;
    uint16_t* chainLen;
    const MChainPool P = tr_wave_pool(gw, qcap, poolA, poolB, poolLen, &chainLen);
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
        uint32_t nE = 0;
        int lastPos = -1;
        for (int pb = 0; pb < nK; pb += 64) {
            const int p = pb + lane;
            uint32_t sid = TR_NONE;
            if (p < nK) {
                uint32_t km = 0;
                for (int j = 0; j < k; j++) km = (km << 2) | codes[p + j];
                sid = tab[km];
            }
            if (sid != TR_NONE) atomicOr((uint32_t*)set + (sid >> 5), 1u << (sid & 31));
            tr_scan_step(sid, pb, k, nE, lastPos, eseg, TR_TCAP);
        }
        if (lane == 0) eseg[2 * nE] = TR_EDGE - (lastPos < 0 ? 0 : lastPos + k);  // len - prev (:323)
        __builtin_amdgcn_wave_barrier();
        const int eN = 2 * (int)nE + 1;
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
                        const int identity = (tr_count_a(aSeg, L.qIdx, ca, len, k) * 100) / alen[ai];
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
// the device buffers of a handle: the adapter index (set-up), the edge stage's batch, the middle stage's chunks, pairs and records
enum TrBuf { TB_TABLE, TB_SEGS, TB_OFF, TB_LEN, TB_BAR, TB_SIZE, TB_ROWS, TB_ROWST, TB_COUNTS, TB_ENABLED, TB_POOL, TB_ERR, TB_ENDS, TB_RECS,
             TB_CBASES, TB_COFF, TB_CCOUNT, TB_CSEGOFF, TB_PAIRS, TB_MRECS, TB_MOVER, TB_MCNT, TB_SPANS, TB_N };
struct dp_trim {
    int device = 0, k = 0;
    uint32_t n_front = 0, n_back = 0, n_seeds = 0, SW = 0, qcap = 0, waves = 0;
    size_t lds_bytes = 0;
    TrimGeom G;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    DevBuf buf[TB_N];             // the handle's device memory (tr_reserve)
    template <typename T>
    T* dev(TrBuf b) const { return (T*)buf[b].p; }
    std::vector<int32_t> pairs;   // the pair ids as uploaded (pairing is the host's rule, trim.go:471-485)
    std::string err;
    // ---- the middle stage (dp_trim_scan_chunks / dp_trim_search)
    dp_ctx* ctx = nullptr;             // the context whose index build and query stage (SeedIndex.Matches) the search drives
    std::vector<uint32_t> seed_kmers;  // seed id -> k-mer (dp_round_begin)
    std::vector<int32_t> h_fsegs;      // the front adapters' segments and offsets as dp_query_candidates takes them
    std::vector<uint64_t> h_foff;
    std::vector<int32_t> h_alen;
    uint32_t n_chunks = 0;
    std::vector<uint32_t> c_count;     // seeds per scanned chunk
    std::vector<uint64_t> c_segoff;    // [n_chunks + 1] offsets of the chunks' segments in the context's scan buffer
    std::vector<dp_trim_mid_rec> m_recs;
    std::vector<uint32_t> m_over;
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

// A buffer that holds `bytes`: one that is too small is freed and replaced by one of `grown` bytes (the caller's head room; 0: bytes)
// and 64 of pad.  The contents do not survive.
static hipError_t tr_reserve(dp_trim* t, TrBuf which, size_t bytes, size_t grown = 0) {
    DevBuf& b = t->buf[which];
    if (b.p && bytes <= b.cap) return hipSuccess;
    if (b.p) dp_dev_free(b.p);
    b.p = nullptr;
    b.cap = 0;
    grown = std::max(grown, bytes);
    const hipError_t e = dp_dev_malloc(&b.p, grown + 64);
    if (e == hipSuccess) b.cap = grown;
    return e;
}
// elapsed ms between ev[i] and ev[i + 1], or 0
static double tr_ms(const dp_trim* t, int i) {
    float ms = 0;
    return hipEventElapsedTime(&ms, t->ev[i], t->ev[i + 1]) == hipSuccess ? ms : 0;
}

extern "C" const char* dp_trim_error(const dp_trim* t) { return t ? t->err.c_str() : g_trim_err.c_str(); }

extern "C" void dp_trim_release(dp_trim* t) {
    if (!t) return;
    hipSetDevice(t->device);
    if (t->stream) hipStreamSynchronize(t->stream);
    for (DevBuf& b : t->buf)
        if (b.p) dp_dev_free(b.p);
    if (t->ctx) dp_ctx_destroy(t->ctx);
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
    t->seed_kmers.assign(n_seeds, 0);
    for (size_t i = 0; i < nK; i++)
        if (kmer_seed[i] != TR_NONE) t->seed_kmers[kmer_seed[i]] = (uint32_t)i;
    t->h_fsegs.assign(segs, segs + off32[n_front]);
    t->h_foff.assign(seg_off, seg_off + n_front + 1);
    t->h_alen.assign(lengths, lengths + nA);
    TR_HIP(hipSetDevice(device));
    TR_HIP(hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking));
    for (hipEvent_t& e : t->ev) TR_HIP(hipEventCreate(&e));
    const size_t nSegs = off32[nA];
    TR_HIP(tr_reserve(t, TB_TABLE, nK * 2));
    TR_HIP(tr_reserve(t, TB_SEGS, nSegs * 4));
    TR_HIP(tr_reserve(t, TB_OFF, ((size_t)nA + 1) * 4));
    TR_HIP(tr_reserve(t, TB_LEN, (size_t)nA * 4));
    TR_HIP(tr_reserve(t, TB_BAR, (size_t)nA));
    TR_HIP(tr_reserve(t, TB_SIZE, (size_t)nA * 4));
    TR_HIP(tr_reserve(t, TB_ROWS, (size_t)nA * t->SW * 8));
    TR_HIP(tr_reserve(t, TB_ROWST, (size_t)nA * t->SW * 8));
    TR_HIP(tr_reserve(t, TB_COUNTS, (size_t)nA * 8));
    TR_HIP(tr_reserve(t, TB_ENABLED, (size_t)nA * 4));
    TR_HIP(tr_reserve(t, TB_ERR, 64));
    TR_HIP(hipMemcpyAsync(t->buf[TB_TABLE].p, kmer_seed, nK * 2, hipMemcpyHostToDevice, t->stream));
    TR_HIP(hipMemcpyAsync(t->buf[TB_SEGS].p, segs, nSegs * 4, hipMemcpyHostToDevice, t->stream));
    TR_HIP(hipMemcpyAsync(t->buf[TB_OFF].p, off32.data(), ((size_t)nA + 1) * 4, hipMemcpyHostToDevice, t->stream));
    TR_HIP(hipMemcpyAsync(t->buf[TB_LEN].p, lengths, (size_t)nA * 4, hipMemcpyHostToDevice, t->stream));
    TR_HIP(hipMemcpyAsync(t->buf[TB_BAR].p, is_barcode, (size_t)nA, hipMemcpyHostToDevice, t->stream));
    TR_HIP(hipMemsetAsync(t->buf[TB_ROWS].p, 0, (size_t)nA * t->SW * 8, t->stream));
    TR_HIP(hipMemsetAsync(t->buf[TB_COUNTS].p, 0, (size_t)nA * 8, t->stream));
    TR_HIP(hipMemsetAsync(t->buf[TB_ENABLED].p, 0, (size_t)nA * 4, t->stream));
    hipLaunchKernelGGL(trim_rows_kernel, dim3((nA + 63) / 64), dim3(64), 0, t->stream, t->dev<const int32_t>(TB_SEGS), t->dev<const uint32_t>(TB_OFF), nA, t->SW,
                       t->dev<u64>(TB_ROWS), t->dev<u64>(TB_ROWST), t->dev<int32_t>(TB_SIZE));
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
    TR_HIP(tr_reserve(t, TB_POOL, waves * per_wave));
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
        const size_t cap = std::max<size_t>(n_ends, 1u << 16);  // read ends the batch buffers hold once they grow
        TR_HIP(tr_reserve(t, TB_ENDS, (size_t)n_ends * TR_EDGE, cap * TR_EDGE));
        TR_HIP(tr_reserve(t, TB_RECS, (size_t)n_ends * sizeof(dp_trim_rec), cap * sizeof(dp_trim_rec)));
        TR_HIP(hipMemsetAsync(t->buf[TB_ERR].p, 0, 64, t->stream));
        TR_HIP(hipEventRecord(t->ev[0], t->stream));
        TR_HIP(hipMemcpyAsync(t->buf[TB_ENDS].p, ends, (size_t)n_ends * TR_EDGE, hipMemcpyHostToDevice, t->stream));
        TR_HIP(hipEventRecord(t->ev[1], t->stream));
        const uint32_t blocks = std::min<uint32_t>(t->waves / TR_WAVES, (n_ends + TR_WAVES - 1) / TR_WAVES);
        const size_t poolElems = (size_t)t->waves * M_CHAINS * t->qcap;
        uint16_t* poolA = t->dev<uint16_t>(TB_POOL);
        hipLaunchKernelGGL(trim_edge_kernel, dim3(blocks), dim3(64 * TR_WAVES), t->lds_bytes, t->stream, t->dev<const uint8_t>(TB_ENDS), n_ends, t->G,
                           t->dev<const uint16_t>(TB_TABLE), t->dev<const int32_t>(TB_SEGS), t->dev<const uint32_t>(TB_OFF), t->dev<const int32_t>(TB_LEN),
                           t->dev<const uint8_t>(TB_BAR), t->dev<const int32_t>(TB_SIZE), t->dev<const u64>(TB_ROWS), t->dev<const u64>(TB_ROWST), mode, min_match,
                           threshold, t->dev<dp_trim_rec>(TB_RECS), t->dev<unsigned long long>(TB_COUNTS), t->dev<uint32_t>(TB_ENABLED), poolA, poolA + poolElems,
                           poolA + 2 * poolElems, t->dev<uint32_t>(TB_ERR));
        TR_HIP(hipGetLastError());
        TR_HIP(hipEventRecord(t->ev[2], t->stream));
        uint32_t errbits = 0;
        if (mode == DP_TRIM_MODE_TRIM) TR_HIP(hipMemcpyAsync(recs, t->buf[TB_RECS].p, (size_t)n_ends * sizeof(dp_trim_rec), hipMemcpyDeviceToHost, t->stream));
        TR_HIP(hipMemcpyAsync(&errbits, t->buf[TB_ERR].p, 4, hipMemcpyDeviceToHost, t->stream));
        TR_HIP(hipEventRecord(t->ev[3], t->stream));
        TR_HIP(hipStreamSynchronize(t->stream));
        if (times_ms)
            for (int i = 0; i < 3; i++) times_ms[i] = tr_ms(t, i);
        if (errbits) return tr_fail(t, DP_ERR_CAPACITY, "dp_trim_edges: chaining exceeded a device capacity (bits " + std::to_string(errbits) +
                                                            ": 1 reduced sequence, 2 chain pool, 4 good-chain list)");
    }
    if (counts) TR_HIP(hipMemcpy(counts, t->buf[TB_COUNTS].p, (size_t)nA * 8, hipMemcpyDeviceToHost));
    if (enabled) {
        std::vector<uint32_t> en(nA);
        TR_HIP(hipMemcpy(en.data(), t->buf[TB_ENABLED].p, (size_t)nA * 4, hipMemcpyDeviceToHost));
        for (uint32_t a = 0; a < nA; a++) enabled[a] = en[a] ? 1 : 0;
    }
    return DP_OK;
}


// ---- the middle stage: chunk scan, chunk index, candidates and the (front adapter, chunk) matching -----------------------------------
// Trim's second half (trim/trim.go:151-217) and findSplit's search (:519-530).  The centres of the edge-trimmed reads arrive as
// chunks of ASCII bases; chunk_scan_kernel is step 1 of trim_edge_kernel for a chunk of any length (NewSeedSequence, seeds.go:33-50:
// one wave per chunk, ballot + prefix over 64 k-mer positions at a time), first counting, then writing [gap, seed, ..., gap] into the
// scan buffer of a dp_ctx the handle owns.  That context's dense index build (seed-set rows, posting matrix, pmeta) and its query
// stage - the exact GetSharedIDs emulation behind dp_query_candidates - give Matches(ad, 0.2) for every front adapter;
// trim_mid_kernel then runs Match for every (candidate chunk, front adapter) pair.
#define MID_TCAP 1024  // reduced seeds of a chunk a wave's LDS slice holds; a pair beyond it is listed for the host's exact Match

template <bool WRITE>
__global__ __launch_bounds__(256) void chunk_scan_kernel(const uint8_t* __restrict__ bases, const uint64_t* __restrict__ off, uint32_t n_chunks, int k,
                                                         const uint16_t* __restrict__ table, uint32_t* __restrict__ counts,
                                                         const uint64_t* __restrict__ segoff, int32_t* __restrict__ segs) {
    const int lane = dp_lane();
    const uint32_t gw = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t c = gw; c < n_chunks; c += waves) {
        const uint8_t* src = bases + off[c];
        const long long len = (long long)(off[c + 1] - off[c]);
        const long long nK = len - k + 1;
        const uint32_t cap = WRITE ? counts[c] : 0u;
        int32_t* seg = WRITE ? segs + segoff[c] : nullptr;
        uint32_t nE = 0;
        long long lastPos = -1;
        for (long long pb = 0; pb < nK; pb += 64) {
            const long long p = pb + lane;
            uint32_t sid = TR_NONE;
            if (p < nK) {
                uint32_t km = 0;
                for (int j = 0; j < k; j++) {
                    const uint32_t b = src[p + j];
                    km = (km << 2) | (((b >> 1) ^ ((b & 4) >> 2)) & 3);
                }
                sid = table[km];
            }
            if (WRITE) tr_scan_step(sid, pb, k, nE, lastPos, seg, cap);
            else nE += (uint32_t)__popcll(__ballot(sid != TR_NONE));  // the counting pass
        }
        if (lane == 0) {
            if (WRITE) {
                if (nE == cap) seg[2 * (size_t)nE] = (int32_t)(len - (lastPos < 0 ? 0 : lastPos + k));  // len - prev (:323)
            } else {
                counts[c] = nE;
            }
        }
    }
}

struct MidGeom {
    int k;
    uint32_t SW, SWc, qcap, wave_words, n_pairs, rec_cap;
    int threshold;
};

// One wave per (chunk, front adapter) pair, pairs in chunk-major order so that the waves of a workgroup read one chunk's segments
// together.  cnt[0] = records appended, cnt[1] = pairs listed for the host.
__global__ __launch_bounds__(64 * TR_WAVES) void trim_mid_kernel(
    const uint2* __restrict__ pairs, MidGeom G, const dp_seq_ref* __restrict__ refs, const int32_t* __restrict__ csegs, const u64* __restrict__ csets,
    const int32_t* __restrict__ asegs, const uint32_t* __restrict__ aoff, const int32_t* __restrict__ alen, const u64* __restrict__ rows,
    dp_trim_mid_rec* __restrict__ recs, uint32_t* __restrict__ over, uint32_t* __restrict__ cnt, uint16_t* __restrict__ poolA,
    uint16_t* __restrict__ poolB, uint16_t* __restrict__ poolLen) {
    extern __shared__ __attribute__((aligned(16))) uint32_t tr_lds[];
    __shared__ TrimL sh[TR_WAVES];
    const int lane = dp_lane();
    const int wv = threadIdx.x >> 6;
    const int k = G.k;
    const uint32_t qcap = G.qcap;
    TrimL& L = sh[wv];
    tr_chain_set(MID_TCAP, qcap, tr_lds + (size_t)wv * G.wave_words, lane == 0 ? &L : nullptr);
    __syncthreads();
    const uint32_t gw = blockIdx.x * TR_WAVES + wv, waves = gridDim.x * TR_WAVES;
    uint16_t* chainLen;
    const MChainPool P = tr_wave_pool(gw, qcap, poolA, poolB, poolLen, &chainLen);
    for (uint32_t pi = gw; pi < G.n_pairs; pi += waves) {
        const uint2 pr = pairs[pi];  // x = indexed chunk, y = front adapter
        const dp_seq_ref ref = refs[pr.x];
        const int32_t* cSeg = csegs + ref.seg_off;
        const int cN = 2 * (int)ref.n_seeds + 1;
        const uint32_t ai = pr.y;
        const int32_t* aSeg = asegs + aoff[ai];
        const int aN = (int)(aoff[ai + 1] - aoff[ai]);
        const int minMatch = (aN / 2) / 5;  // ad.GetNumSeeds() / 5 (trim.go:519)
        uint32_t err = ref.n_seeds > 0xffffu ? 1u : 0u;  // (seed indices travel in 16 bits)
        int nGood = 0;
        if (!err) {
            // Match (seeds/sequence.go:361-394): the chunk reduced to the adapter's seeds, the adapter to the chunk's
            const int nT = m_reduce_wave<uint16_t>(cSeg, cN, (const u64*)(rows + (size_t)ai * G.SW), k, minMatch, L.t, L.tIdx, MID_TCAP, &err);
            const int nQ = nT < 0 ? -1 : m_reduce_wave<uint16_t>(aSeg, aN, (const u64*)(csets + (size_t)pr.x * G.SWc), k, minMatch, L.q, L.qIdx, (int)qcap, &err);
            if (nT >= 0 && nQ >= 0) nGood = m_dynamic_match_wave(L, 2 * nQ + 1, 2 * nT + 1, minMatch, k, P, chainLen, &err);
        }
        err = (uint32_t)__builtin_amdgcn_readfirstlane((int)err);
        if (lane == 0) {
            if (err) {
                over[atomicAdd(&cnt[1], 1u)] = pi;  // (the list holds every pair)
            } else {
                for (int g = 0; g < nGood; g++) {
                    const int ch = L.good[g];
                    const int len = chainLen[ch];
                    const uint16_t* ca = P.A(ch);
                    const uint16_t* cb = P.B(ch);
                    const int countA = tr_count_a(aSeg, L.qIdx, ca, len, k);
                    if ((countA * 100) / alen[ai] < G.threshold) continue;  // trim.go:528
                    const uint32_t at = atomicAdd(&cnt[0], 1u);
                    if (at < G.rec_cap) {
                        dp_trim_mid_rec r;
                        r.adapter = (int32_t)ai;
                        r.chunk = (int32_t)pr.x;
                        r.ordinal = g;
                        r.start_rel = tr_seed_offset(cSeg, L.tIdx[cb[0]], k) - tr_seed_offset(aSeg, L.qIdx[ca[0]], k);  // :541
                        r.covered = countA;
                        r.chain_len = len;
                        recs[at] = r;
                    }
                }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}

#define TR_CTX(call)                                                                                            \
    do {                                                                                                        \
        const int rc_ = (call);                                                                                 \
        if (rc_ != DP_OK) return tr_fail(t, rc_, std::string("dp_trim: " #call ": ") + dp_last_error(t->ctx)); \
    } while (0)

static int tr_mid_ctx(dp_trim* t) {
    if (t->k < 4) return tr_fail(t, DP_ERR_ARG, "dp_trim: the middle stage needs k >= 4 (the chunk index is a dp_ctx round index)");
    if (!t->ctx) {
        const int rc = dp_ctx_create(t->device, &t->ctx);
        if (rc != DP_OK) return tr_fail(t, rc, std::string("dp_trim: dp_ctx_create: ") + dp_last_error(nullptr));
        TR_CTX(dp_round_begin(t->ctx, t->k, t->seed_kmers.data(), t->n_seeds));
    }
    return DP_OK;
}

extern "C" int dp_trim_scan_chunks(dp_trim* t, const uint8_t* bases, const uint64_t* off, uint32_t n_chunks, uint32_t* n_seeds_out,
                                   double* times_ms) {
    if (!t) return tr_fail(nullptr, DP_ERR_ARG, "dp_trim_scan_chunks: null handle");
    const bool own = false;
    if (n_chunks && (!bases || !off)) return tr_fail(t, DP_ERR_ARG, "dp_trim_scan_chunks: bad arguments");
    for (uint32_t c = 0; c < n_chunks; c++)
        if (off[c + 1] < off[c]) return tr_fail(t, DP_ERR_ARG, "dp_trim_scan_chunks: chunk offsets must ascend");
    if (int rc = tr_mid_ctx(t)) return rc;
    TR_HIP(hipSetDevice(t->device));
    if (times_ms) times_ms[0] = times_ms[1] = 0;
    t->n_chunks = 0;
    t->c_count.assign(n_chunks, 0);
    t->c_segoff.assign((size_t)n_chunks + 1, 0);
    t->ctx->n_segs = 0;
    if (!n_chunks) return DP_OK;
    hipStream_t st = t->ctx->stream;
    const size_t nb = off[n_chunks] - off[0];
    TR_HIP(tr_reserve(t, TB_CBASES, nb, nb + nb / 4));
    const size_t cap = (size_t)n_chunks + n_chunks / 4 + 1024;  // chunks the three per-chunk arrays hold once they grow
    TR_HIP(tr_reserve(t, TB_COFF, ((size_t)n_chunks + 1) * 8, (cap + 1) * 8));
    TR_HIP(tr_reserve(t, TB_CCOUNT, (size_t)n_chunks * 4, cap * 4));
    TR_HIP(tr_reserve(t, TB_CSEGOFF, ((size_t)n_chunks + 1) * 8, (cap + 1) * 8));
    std::vector<uint64_t> rel((size_t)n_chunks + 1);
    for (uint32_t c = 0; c <= n_chunks; c++) rel[c] = off[c] - off[0];
    TR_HIP(hipEventRecord(t->ev[0], st));
    TR_HIP(hipMemcpyAsync(t->buf[TB_CBASES].p, bases + off[0], nb, hipMemcpyHostToDevice, st));
    TR_HIP(hipMemcpyAsync(t->buf[TB_COFF].p, rel.data(), ((size_t)n_chunks + 1) * 8, hipMemcpyHostToDevice, st));
    TR_HIP(hipEventRecord(t->ev[1], st));
    const uint32_t blocks = std::min<uint32_t>(4096, (n_chunks + 3) / 4);
    hipLaunchKernelGGL(chunk_scan_kernel<false>, dim3(blocks), dim3(256), 0, st, t->dev<const uint8_t>(TB_CBASES), t->dev<const uint64_t>(TB_COFF), n_chunks, t->k,
                       t->dev<const uint16_t>(TB_TABLE), t->dev<uint32_t>(TB_CCOUNT), (const uint64_t*)nullptr, (int32_t*)nullptr);
    TR_HIP(hipGetLastError());
    TR_HIP(hipMemcpyAsync(t->c_count.data(), t->buf[TB_CCOUNT].p, (size_t)n_chunks * 4, hipMemcpyDeviceToHost, st));
    TR_HIP(hipStreamSynchronize(st));
    for (uint32_t c = 0; c < n_chunks; c++) t->c_segoff[c + 1] = t->c_segoff[c] + 2ull * t->c_count[c] + 1;
    const uint64_t total = t->c_segoff[n_chunks];
    if (dev_reserve(t->ctx, t->ctx->d_segs, (size_t)total * 4 + 64)) return tr_fail(t, DP_ERR_HIP, std::string("dp_trim_scan_chunks: ") + dp_last_error(t->ctx));
    TR_HIP(hipMemcpyAsync(t->buf[TB_CSEGOFF].p, t->c_segoff.data(), ((size_t)n_chunks + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(chunk_scan_kernel<true>, dim3(blocks), dim3(256), 0, st, t->dev<const uint8_t>(TB_CBASES), t->dev<const uint64_t>(TB_COFF), n_chunks, t->k,
                       t->dev<const uint16_t>(TB_TABLE), t->dev<uint32_t>(TB_CCOUNT), t->dev<const uint64_t>(TB_CSEGOFF), (int32_t*)t->ctx->d_segs.p);
    TR_HIP(hipGetLastError());
    TR_HIP(hipEventRecord(t->ev[2], st));
    TR_HIP(hipStreamSynchronize(st));
    t->ctx->n_segs = total;
    t->n_chunks = n_chunks;
    if (times_ms)
        for (int i = 0; i < 2; i++) times_ms[i] = tr_ms(t, i);
    if (n_seeds_out) memcpy(n_seeds_out, t->c_count.data(), (size_t)n_chunks * 4);
    return DP_OK;
}

extern "C" int dp_trim_chunk_segments(dp_trim* t, uint32_t chunk, int32_t* out, uint64_t cap, uint64_t* n) {
    if (!t || !n) return tr_fail(t, DP_ERR_ARG, "dp_trim_chunk_segments: bad arguments");
    const bool own = false;
    if (chunk >= t->n_chunks) return tr_fail(t, DP_ERR_ARG, "dp_trim_chunk_segments: no such chunk in the last scan");
    *n = t->c_segoff[chunk + 1] - t->c_segoff[chunk];
    if (!out || cap < *n) return DP_OK;
    TR_HIP(hipSetDevice(t->device));
    TR_HIP(hipMemcpy(out, (const int32_t*)t->ctx->d_segs.p + t->c_segoff[chunk], (size_t)*n * 4, hipMemcpyDeviceToHost));
    return DP_OK;
}

extern "C" int dp_trim_search(dp_trim* t, const uint32_t* sel, uint32_t n_sel, int mid_threshold, dp_trim_mid_batch* out) {
    if (!t || !out) return tr_fail(t, DP_ERR_ARG, "dp_trim_search: bad arguments");
    const bool own = false;
    memset(out, 0, sizeof(*out));
    t->m_recs.clear();
    t->m_over.clear();
    if (n_sel && !sel) return tr_fail(t, DP_ERR_ARG, "dp_trim_search: bad arguments");
    if (!n_sel || !t->n_front) return DP_OK;
    if (!t->ctx || !t->n_chunks) return tr_fail(t, DP_ERR_STATE, "dp_trim_search before dp_trim_scan_chunks");
    TR_HIP(hipSetDevice(t->device));
    hipStream_t st = t->ctx->stream;
    std::vector<dp_seq_ref> refs(n_sel);
    for (uint32_t i = 0; i < n_sel; i++) {
        if (sel[i] >= t->n_chunks || (i && sel[i] <= sel[i - 1])) return tr_fail(t, DP_ERR_ARG, "dp_trim_search: the chunks must be ascending ids of the last scan");
        refs[i].seg_off = t->c_segoff[sel[i]];
        refs[i].n_seeds = t->c_count[sel[i]];
        refs[i].reserved = 0;
    }
    // AddSequence + IndexSequences, then Matches(ad, 0.2) of every front adapter (trim.go:187, :520)
    TR_HIP(hipEventRecord(t->ev[0], st));
    TR_CTX(dp_index_build(t->ctx, refs.data(), n_sel));
    TR_HIP(hipEventRecord(t->ev[1], st));
    dp_candidate_batch cb;
    TR_CTX(dp_query_candidates(t->ctx, t->h_fsegs.data(), t->h_foff.data(), t->n_front, 0.2, &cb));
    TR_HIP(hipEventRecord(t->ev[2], st));
    for (uint32_t a = 0; a < t->n_front; a++)
        if (cb.meta[3 * a + 2]) return tr_fail(t, DP_ERR_CAPACITY, "dp_trim_search: front adapter " + std::to_string(a) + " exceeds a capacity of the index query");
    const uint64_t n_pairs64 = cb.cand_off[t->n_front];
    if (n_pairs64 > 0x7fffffffull) return tr_fail(t, DP_ERR_CAPACITY, "dp_trim_search: more than 2^31 candidate pairs in one batch");
    const uint32_t n_pairs = (uint32_t)n_pairs64;
    out->n_pairs = n_pairs;
    if (n_pairs) {
        // chunk-major pair list: a counting sort of the per-adapter candidate lists by chunk
        std::vector<uint32_t> start((size_t)n_sel + 1, 0);
        for (uint64_t i = 0; i < n_pairs64; i++) start[cb.cand[i] + 1]++;
        for (uint32_t i = 0; i < n_sel; i++) start[i + 1] += start[i];
        std::vector<uint2> pairs(n_pairs);
        for (uint32_t a = 0; a < t->n_front; a++)
            for (uint64_t i = cb.cand_off[a]; i < cb.cand_off[a + 1]; i++) pairs[start[cb.cand[i]]++] = make_uint2(cb.cand[i], a);
        const size_t cap = (size_t)n_pairs + n_pairs / 4 + 1024;  // pairs the list and the overflow list hold once they grow
        TR_HIP(tr_reserve(t, TB_PAIRS, (size_t)n_pairs * 8, cap * 8));
        TR_HIP(tr_reserve(t, TB_MOVER, (size_t)n_pairs * 4, cap * 4));
        TR_HIP(tr_reserve(t, TB_MCNT, 64));
        TR_HIP(hipMemcpyAsync(t->buf[TB_PAIRS].p, pairs.data(), (size_t)n_pairs * 8, hipMemcpyHostToDevice, st));
        MidGeom G;
        G.k = t->k;
        G.SW = t->SW;
        G.SWc = t->ctx->SW;
        G.qcap = t->qcap;
        G.wave_words = (tr_chain_set(MID_TCAP, t->qcap) + 2 + 1u) & ~1u;  // (a wave's slice: the working set and two words to spare)
        G.n_pairs = n_pairs;
        G.threshold = mid_threshold;
        const size_t lds = (size_t)TR_WAVES * G.wave_words * 4;
        TR_HIP(hipFuncSetAttribute((const void*)trim_mid_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        // the record buffer is sized from a guess - nearly every pair emits nothing - and the launch repeated when it was too small
        size_t rec_cap = (size_t)dp_env_long("DP_TRIM_MID_REC_CAP", (long)std::max<size_t>(1024, n_pairs / 64), 1);
        const uint32_t blocks = std::min<uint32_t>(t->waves / TR_WAVES, (n_pairs + TR_WAVES - 1) / TR_WAVES);
        const size_t poolElems = (size_t)t->waves * M_CHAINS * t->qcap;
        uint16_t* poolA = t->dev<uint16_t>(TB_POOL);
        TR_HIP(hipEventRecord(t->ev[2], st));
        for (;;) {
            TR_HIP(tr_reserve(t, TB_MRECS, rec_cap * sizeof(dp_trim_mid_rec)));
            G.rec_cap = (uint32_t)std::min<size_t>(rec_cap, 0x7fffffffu);
            TR_HIP(hipMemsetAsync(t->buf[TB_MCNT].p, 0, 64, st));
            hipLaunchKernelGGL(trim_mid_kernel, dim3(blocks), dim3(64 * TR_WAVES), lds, st, t->dev<const uint2>(TB_PAIRS), G, (const dp_seq_ref*)t->ctx->d_seqrefs.p,
                               (const int32_t*)t->ctx->d_segs.p, (const u64*)t->ctx->d_seedsets.p, t->dev<const int32_t>(TB_SEGS), t->dev<const uint32_t>(TB_OFF),
                               t->dev<const int32_t>(TB_LEN), t->dev<const u64>(TB_ROWS), t->dev<dp_trim_mid_rec>(TB_MRECS), t->dev<uint32_t>(TB_MOVER), t->dev<uint32_t>(TB_MCNT), poolA,
                               poolA + poolElems, poolA + 2 * poolElems);
            TR_HIP(hipGetLastError());
            uint32_t cnt[2] = {0, 0};
            TR_HIP(hipMemcpyAsync(cnt, t->buf[TB_MCNT].p, 8, hipMemcpyDeviceToHost, st));
            TR_HIP(hipStreamSynchronize(st));
            out->launches++;
            if (cnt[0] > G.rec_cap) {
                rec_cap = (size_t)cnt[0] + cnt[0] / 8 + 16;
                continue;
            }
            t->m_recs.resize(cnt[0]);
            t->m_over.resize(std::min<uint32_t>(cnt[1], n_pairs));
            if (cnt[0]) TR_HIP(hipMemcpyAsync(t->m_recs.data(), t->buf[TB_MRECS].p, (size_t)cnt[0] * sizeof(dp_trim_mid_rec), hipMemcpyDeviceToHost, st));
            if (!t->m_over.empty()) TR_HIP(hipMemcpyAsync(t->m_over.data(), t->buf[TB_MOVER].p, t->m_over.size() * 4, hipMemcpyDeviceToHost, st));
            TR_HIP(hipEventRecord(t->ev[3], st));
            TR_HIP(hipStreamSynchronize(st));
            break;
        }
        // records name the caller's chunk ids; the overflow list becomes (chunk, adapter) pairs
        for (dp_trim_mid_rec& r : t->m_recs) r.chunk = (int32_t)sel[r.chunk];
        std::vector<uint32_t> ov;
        for (uint32_t pi : t->m_over) {
            ov.push_back(sel[pairs[pi].x]);
            ov.push_back(pairs[pi].y);
        }
        t->m_over.swap(ov);
        std::sort(t->m_recs.begin(), t->m_recs.end(), [](const dp_trim_mid_rec& a, const dp_trim_mid_rec& b) {
            if (a.adapter != b.adapter) return a.adapter < b.adapter;
            if (a.chunk != b.chunk) return a.chunk < b.chunk;
            return a.ordinal < b.ordinal;
        });
    }
    out->n_recs = (uint32_t)t->m_recs.size();
    out->recs = t->m_recs.data();
    out->n_overflow = (uint32_t)(t->m_over.size() / 2);
    out->overflow = t->m_over.data();
    out->index_ms = tr_ms(t, 0);
    out->query_ms = tr_ms(t, 1);
    if (n_pairs) out->kernel_ms = tr_ms(t, 2);
    return DP_OK;
}


// ---- both stages on reads a context holds resident (`overlap -trim true`) --------------------------------------------------------------
// The ends buffer and the chunk bases the two scan kernels read are spelled on the device from the context's 2-bit reads, so that what
// crosses the link is a table of read ids or spans.  unpack_spans_kernel: one thread per 16 bytes of the destination.  Span i is, with
// `ends_reads`, end i & 1 of read ends_reads[i >> 1] at i * 150 (the dense layout trim_edge_kernel reads: its spans start unaligned);
// else spans[i] at doff[i].  A 16-byte group inside one span takes its 32 bits from at most two source dwords - the second one only when
// the group's last base lies in it, so never past the read's padded end - and is stored at once; a group that straddles spans, or the
// buffer's tail, goes base by base.  Traffic per base: 0.25 bytes read, 1 written.
__global__ __launch_bounds__(256) void unpack_spans_kernel(const uint32_t* __restrict__ packed, const uint64_t* __restrict__ boff, const uint32_t* __restrict__ rlen,
                                                           const uint32_t* __restrict__ ends_reads, const dp_read_span* __restrict__ spans,
                                                           const uint64_t* __restrict__ doff, uint32_t n_spans, uint64_t total, uint8_t* __restrict__ dst) {
    const uint64_t pos0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * 16;
    if (pos0 >= total) return;
    const uint8_t* src;
    uint64_t lo, hi;  // the span's bytes of dst
    uint32_t start;
    auto load = [&](uint32_t i) {
        uint32_t r;
        if (ends_reads) {
            r = ends_reads[i >> 1];
            start = (i & 1u) ? rlen[r] - TR_EDGE : 0u;
            lo = (uint64_t)i * TR_EDGE;
            hi = lo + TR_EDGE;
        } else {
            r = spans[i].read;
            start = spans[i].start;
            lo = doff[i];
            hi = doff[i + 1];
        }
        src = (const uint8_t*)packed + boff[r];
    };
    uint32_t i;
    if (ends_reads) {
        i = (uint32_t)(pos0 / TR_EDGE);
    } else {  // the last span with doff[i] <= pos0 (empty spans before it share its offset)
        uint32_t a = 0, b = n_spans;
        while (b - a > 1) {
            const uint32_t mid = (a + b) >> 1;
            if (doff[mid] <= pos0) a = mid;
            else b = mid;
        }
        i = a;
    }
    load(i);
    if (pos0 + 16 <= hi) {
        const uint32_t p = start + (uint32_t)(pos0 - lo);
        const uint32_t* w = (const uint32_t*)src + (p >> 4);
        u64 v = w[0];
        if (p & 15u) v |= (u64)w[1] << 32;
        uint32_t o[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint32_t q = (p & 15u) + j;  // base q of the two dwords: byte q / 4, first base in the byte's top bits
            const uint32_t c = (uint32_t)(v >> (8 * (q >> 2) + 6 - 2 * (q & 3u))) & 3u;
            o[j >> 2] |= ((0x54474341u >> (8 * c)) & 0xffu) << (8 * (j & 3));  // "ACGT"[c]
        }
        *(uint4*)(dst + pos0) = make_uint4(o[0], o[1], o[2], o[3]);
    } else {
        const uint64_t end = pos0 + 16 < total ? pos0 + 16 : total;
        for (uint64_t pos = pos0; pos < end; pos++) {
            while (pos >= hi) load(++i);  // (pos < total: a span that holds it follows)
            const uint32_t p = start + (uint32_t)(pos - lo);
            const uint32_t c = (src[p >> 2] >> (6 - 2 * (p & 3u))) & 3u;
            dst[pos] = (uint8_t)((0x54474341u >> (8 * c)) & 0xffu);
        }
    }
}

// doff[0 .. n] = the prefix of the spans' lengths (TB_COFF as chunk_scan_kernel reads it), by one workgroup: a slice per thread
__global__ __launch_bounds__(1024) void span_offsets_kernel(const dp_read_span* __restrict__ spans, uint32_t n, uint64_t* __restrict__ doff) {
    __shared__ u64 part[1024];
    const uint32_t tid = threadIdx.x, per = (n + 1023u) / 1024u;
    const uint32_t lo = min(n, tid * per), hi = min(n, lo + per);
    u64 s = 0;
    for (uint32_t i = lo; i < hi; i++) s += spans[i].len;
    part[tid] = s;
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {
        const u64 v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    u64 run = part[tid] - s;
    for (uint32_t i = lo; i < hi; i++) {
        doff[i] = run;
        run += spans[i].len;
    }
    if (tid == 1023) doff[n] = part[1023];
}

// what both resident calls check first, and the order they set up: `st` - the stream the unpack kernel runs on - waits for what is
// queued on the context's stream (its upload) through an event of the handle's
static int tr_resident_begin(dp_trim* t, dp_ctx* ctx, hipStream_t st, const char* who) {
    const bool own = false;
    if (!ctx) return tr_fail(t, DP_ERR_ARG, std::string(who) + ": null context");
    if (ctx->device != t->device) return tr_fail(t, DP_ERR_ARG, std::string(who) + ": the handle and the context are on different devices");
    if (dp_reads_stale(ctx, who) != 0) return tr_fail(t, DP_ERR_STATE, dp_last_error(ctx));  // (a borrower that has not seen its owner's new read set)
    {
        std::lock_guard<std::mutex> lk(ctx->upload_mu);
        if (ctx->upload) return tr_fail(t, DP_ERR_STATE, std::string(who) + ": an upload of dp_reads_upload_rc_begin is pending on the context");
    }
    TR_HIP(hipSetDevice(t->device));
    TR_HIP(hipEventRecord(t->ev[0], ctx->stream));
    TR_HIP(hipStreamWaitEvent(st, t->ev[0], 0));
    return DP_OK;
}

extern "C" int dp_trim_edges_resident(dp_trim* t, dp_ctx* ctx, const uint32_t* reads, uint32_t n_reads, int mode, int min_match, int threshold,
                                      dp_trim_rec* recs, uint64_t* counts, uint8_t* enabled, double* times_ms) {
    if (!t) return tr_fail(nullptr, DP_ERR_ARG, "dp_trim_edges_resident: null handle");
    const bool own = false;
    if ((mode != DP_TRIM_MODE_TRIM && mode != DP_TRIM_MODE_DETERMINE) || (n_reads && !reads) || (mode == DP_TRIM_MODE_TRIM && n_reads && !recs))
        return tr_fail(t, DP_ERR_ARG, "dp_trim_edges_resident: bad arguments");
    if (mode == DP_TRIM_MODE_TRIM && min_match < 1) return tr_fail(t, DP_ERR_ARG, "dp_trim_edges_resident: min_match < 1");
    if (n_reads > 0x3fffffffu) return tr_fail(t, DP_ERR_ARG, "dp_trim_edges_resident: batch too large");
    if (int rc = tr_resident_begin(t, ctx, t->stream, "dp_trim_edges_resident")) return rc;
    for (uint32_t i = 0; i < n_reads; i++)
        if (reads[i] >= ctx->n_reads || ctx->h_len[reads[i]] < 200u)
            return tr_fail(t, DP_ERR_ARG, "dp_trim_edges_resident: read " + std::to_string(reads[i]) + " is not a resident read of 200 bases or more");
    const uint32_t nA = t->n_front + t->n_back, n_ends = 2 * n_reads;
    if (times_ms) times_ms[0] = times_ms[1] = times_ms[2] = 0;
    if (n_ends) {
        const size_t cap = std::max<size_t>(n_ends, 1u << 16);  // read ends the batch buffers hold once they grow
        TR_HIP(tr_reserve(t, TB_ENDS, (size_t)n_ends * TR_EDGE, cap * TR_EDGE));
        TR_HIP(tr_reserve(t, TB_RECS, (size_t)n_ends * sizeof(dp_trim_rec), cap * sizeof(dp_trim_rec)));
        TR_HIP(tr_reserve(t, TB_SPANS, (size_t)n_reads * 4, cap * 2));
        TR_HIP(hipMemsetAsync(t->buf[TB_ERR].p, 0, 64, t->stream));
        TR_HIP(hipEventRecord(t->ev[0], t->stream));
        TR_HIP(hipMemcpyAsync(t->buf[TB_SPANS].p, reads, (size_t)n_reads * 4, hipMemcpyHostToDevice, t->stream));
        const uint64_t total = (uint64_t)n_ends * TR_EDGE;
        hipLaunchKernelGGL(unpack_spans_kernel, dim3((uint32_t)((total + 4095) / 4096)), dim3(256), 0, t->stream, (const uint32_t*)ctx->d_packed.p,
                           (const uint64_t*)ctx->d_boff.p, (const uint32_t*)ctx->d_len.p, t->dev<const uint32_t>(TB_SPANS), (const dp_read_span*)nullptr,
                           (const uint64_t*)nullptr, n_ends, total, t->dev<uint8_t>(TB_ENDS));
        TR_HIP(hipGetLastError());
        TR_HIP(hipEventRecord(t->ev[1], t->stream));
        const uint32_t blocks = std::min<uint32_t>(t->waves / TR_WAVES, (n_ends + TR_WAVES - 1) / TR_WAVES);
        const size_t poolElems = (size_t)t->waves * M_CHAINS * t->qcap;
        uint16_t* poolA = t->dev<uint16_t>(TB_POOL);
        hipLaunchKernelGGL(trim_edge_kernel, dim3(blocks), dim3(64 * TR_WAVES), t->lds_bytes, t->stream, t->dev<const uint8_t>(TB_ENDS), n_ends, t->G,
                           t->dev<const uint16_t>(TB_TABLE), t->dev<const int32_t>(TB_SEGS), t->dev<const uint32_t>(TB_OFF), t->dev<const int32_t>(TB_LEN),
                           t->dev<const uint8_t>(TB_BAR), t->dev<const int32_t>(TB_SIZE), t->dev<const u64>(TB_ROWS), t->dev<const u64>(TB_ROWST), mode, min_match,
                           threshold, t->dev<dp_trim_rec>(TB_RECS), t->dev<unsigned long long>(TB_COUNTS), t->dev<uint32_t>(TB_ENABLED), poolA, poolA + poolElems,
                           poolA + 2 * poolElems, t->dev<uint32_t>(TB_ERR));
        TR_HIP(hipGetLastError());
        TR_HIP(hipEventRecord(t->ev[2], t->stream));
        uint32_t errbits = 0;
        if (mode == DP_TRIM_MODE_TRIM) TR_HIP(hipMemcpyAsync(recs, t->buf[TB_RECS].p, (size_t)n_ends * sizeof(dp_trim_rec), hipMemcpyDeviceToHost, t->stream));
        TR_HIP(hipMemcpyAsync(&errbits, t->buf[TB_ERR].p, 4, hipMemcpyDeviceToHost, t->stream));
        TR_HIP(hipEventRecord(t->ev[3], t->stream));
        TR_HIP(hipStreamSynchronize(t->stream));
        if (times_ms)
            for (int i = 0; i < 3; i++) times_ms[i] = tr_ms(t, i);
        if (errbits) return tr_fail(t, DP_ERR_CAPACITY, "dp_trim_edges_resident: chaining exceeded a device capacity (bits " + std::to_string(errbits) +
                                                            ": 1 reduced sequence, 2 chain pool, 4 good-chain list)");
    }
    if (counts) TR_HIP(hipMemcpy(counts, t->buf[TB_COUNTS].p, (size_t)nA * 8, hipMemcpyDeviceToHost));
    if (enabled) {
        std::vector<uint32_t> en(nA);
        TR_HIP(hipMemcpy(en.data(), t->buf[TB_ENABLED].p, (size_t)nA * 4, hipMemcpyDeviceToHost));
        for (uint32_t a = 0; a < nA; a++) enabled[a] = en[a] ? 1 : 0;
    }
    return DP_OK;
}

extern "C" int dp_trim_scan_chunks_resident(dp_trim* t, dp_ctx* ctx, const dp_read_span* spans, uint32_t n_chunks, uint32_t* n_seeds_out,
                                            double* times_ms) {
    if (!t) return tr_fail(nullptr, DP_ERR_ARG, "dp_trim_scan_chunks_resident: null handle");
    const bool own = false;
    if (n_chunks && !spans) return tr_fail(t, DP_ERR_ARG, "dp_trim_scan_chunks_resident: bad arguments");
    if (int rc = tr_mid_ctx(t)) return rc;
    hipStream_t st = t->ctx->stream;
    if (int rc = tr_resident_begin(t, ctx, st, "dp_trim_scan_chunks_resident")) return rc;
    uint64_t nb = 0;
    for (uint32_t c = 0; c < n_chunks; c++) {
        if (spans[c].read >= ctx->n_reads || (uint64_t)spans[c].start + spans[c].len > ctx->h_len[spans[c].read])
            return tr_fail(t, DP_ERR_ARG, "dp_trim_scan_chunks_resident: span " + std::to_string(c) + " lies outside its read");
        nb += spans[c].len;
    }
    if (times_ms) times_ms[0] = times_ms[1] = 0;
    t->n_chunks = 0;
    t->c_count.assign(n_chunks, 0);
    t->c_segoff.assign((size_t)n_chunks + 1, 0);
    t->ctx->n_segs = 0;
    if (!n_chunks) return DP_OK;
    TR_HIP(tr_reserve(t, TB_CBASES, nb, nb + nb / 4));
    const size_t cap = (size_t)n_chunks + n_chunks / 4 + 1024;  // chunks the per-chunk arrays hold once they grow
    TR_HIP(tr_reserve(t, TB_COFF, ((size_t)n_chunks + 1) * 8, (cap + 1) * 8));
    TR_HIP(tr_reserve(t, TB_CCOUNT, (size_t)n_chunks * 4, cap * 4));
    TR_HIP(tr_reserve(t, TB_CSEGOFF, ((size_t)n_chunks + 1) * 8, (cap + 1) * 8));
    TR_HIP(tr_reserve(t, TB_SPANS, (size_t)n_chunks * sizeof(dp_read_span), cap * sizeof(dp_read_span)));
    TR_HIP(hipEventRecord(t->ev[0], st));
    TR_HIP(hipMemcpyAsync(t->buf[TB_SPANS].p, spans, (size_t)n_chunks * sizeof(dp_read_span), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(span_offsets_kernel, dim3(1), dim3(1024), 0, st, t->dev<const dp_read_span>(TB_SPANS), n_chunks, t->dev<uint64_t>(TB_COFF));
    TR_HIP(hipGetLastError());
    if (nb) {
        hipLaunchKernelGGL(unpack_spans_kernel, dim3((uint32_t)((nb + 4095) / 4096)), dim3(256), 0, st, (const uint32_t*)ctx->d_packed.p, (const uint64_t*)ctx->d_boff.p,
                           (const uint32_t*)ctx->d_len.p, (const uint32_t*)nullptr, t->dev<const dp_read_span>(TB_SPANS), t->dev<const uint64_t>(TB_COFF), n_chunks, nb,
                           t->dev<uint8_t>(TB_CBASES));
        TR_HIP(hipGetLastError());
    }
    TR_HIP(hipEventRecord(t->ev[1], st));
    const uint32_t blocks = std::min<uint32_t>(4096, (n_chunks + 3) / 4);
    hipLaunchKernelGGL(chunk_scan_kernel<false>, dim3(blocks), dim3(256), 0, st, t->dev<const uint8_t>(TB_CBASES), t->dev<const uint64_t>(TB_COFF), n_chunks, t->k,
                       t->dev<const uint16_t>(TB_TABLE), t->dev<uint32_t>(TB_CCOUNT), (const uint64_t*)nullptr, (int32_t*)nullptr);
    TR_HIP(hipGetLastError());
    TR_HIP(hipMemcpyAsync(t->c_count.data(), t->buf[TB_CCOUNT].p, (size_t)n_chunks * 4, hipMemcpyDeviceToHost, st));
    TR_HIP(hipStreamSynchronize(st));
    for (uint32_t c = 0; c < n_chunks; c++) t->c_segoff[c + 1] = t->c_segoff[c] + 2ull * t->c_count[c] + 1;
    const uint64_t total = t->c_segoff[n_chunks];
    if (dev_reserve(t->ctx, t->ctx->d_segs, (size_t)total * 4 + 64)) return tr_fail(t, DP_ERR_HIP, std::string("dp_trim_scan_chunks_resident: ") + dp_last_error(t->ctx));
    TR_HIP(hipMemcpyAsync(t->buf[TB_CSEGOFF].p, t->c_segoff.data(), ((size_t)n_chunks + 1) * 8, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(chunk_scan_kernel<true>, dim3(blocks), dim3(256), 0, st, t->dev<const uint8_t>(TB_CBASES), t->dev<const uint64_t>(TB_COFF), n_chunks, t->k,
                       t->dev<const uint16_t>(TB_TABLE), t->dev<uint32_t>(TB_CCOUNT), t->dev<const uint64_t>(TB_CSEGOFF), (int32_t*)t->ctx->d_segs.p);
    TR_HIP(hipGetLastError());
    TR_HIP(hipEventRecord(t->ev[2], st));
    TR_HIP(hipStreamSynchronize(st));
    t->ctx->n_segs = total;
    t->n_chunks = n_chunks;
    if (times_ms)
        for (int i = 0; i < 2; i++) times_ms[i] = tr_ms(t, i);
    if (n_seeds_out) memcpy(n_seeds_out, t->c_count.data(), (size_t)n_chunks * 4);
    return DP_OK;
}
