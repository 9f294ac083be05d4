// The arithmetic of `downpore map` that decides what the device is asked to do (host_map.cpp: runMap and its workers), as plain
// functions on numbers, strings and the ABI's plain structs: the 32-bit limits, the circular join chunks, the packed upload's layout,
// the chunk schedule, a Mapper batch's layout and device ids (a trimmed batch's raw ids too), a window request's scan items and the reverse strand's fix-up, the shards' seed-window merge and the dense
// index estimate.  No device call, no environment, no thread: tests/native/map_plan_check.cpp holds every function here to the
// oracle's Mapper, to rules written out a second time or to brute force, without a GPU.
#pragma once
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "dph.hpp"

namespace dph {

// ---- limits.  Positions in the reference travel as 32-bit signed ints (chunk offsets, the reverse strand, the PAF's target fields):
// a longer sequence is refused before anything is packed or allocated on the device.  Seed windows and chunks are numbered in 32 bits.
// Closed-form counts of one run's seed windows and chunks (the chunk count is an upper bound: it books a join chunk for every
// sequence of a circular reference, and the schedule gives none to a sequence shorter than query_size).  false: the parameters
// make no schedule to count (seed_rate <= 0 or chunk_size * 10 <= query_size).
inline bool mapCountBounds(const MapParams& p, const std::vector<i64>& refLens, unsigned long long& nWin, unsigned long long& nChk) {
    nWin = nChk = 0;
    if (!(p.seedRate > 0 && p.chunkSize * 10 > p.querySize)) return false;
    const i64 step = p.chunkSize * 10 - p.querySize;
    for (size_t c = 0; c < refLens.size(); c++) {
        const i64 L = refLens[c];
        if (L > p.seedRate) nWin += (unsigned long long)((L - 1) / p.seedRate);
        for (i64 j = 0; j < 10; j++)
            if (j * p.chunkSize < L - p.chunkSize / 2) nChk += (unsigned long long)((L - p.chunkSize / 2 - j * p.chunkSize + step - 1) / step);
        nChk += p.circular ? 1 : 0;
    }
    return true;
}
// 0, or DP_ERR_ARG with the refusal's text; names[c] is sequence c's name (used with -all_sequences only)
inline int mapCheckLimits(const MapParams& p, const std::vector<i64>& refLens, const std::vector<std::string>& names, std::string& error) {
    for (size_t c = 0; c < refLens.size(); c++)
        if (refLens[c] > (i64)0x7fffffff) {
            error = p.allSequences ? "map: the reference sequence " + names[c] + " is " + std::to_string((long long)refLens[c]) +
                                         " bases long; at most 2147483647 are supported"
                                   : "map: the reference sequence is " + std::to_string((long long)refLens[c]) +
                                         " bases long; at most 2147483647 are supported";
            return DP_ERR_ARG;
        }
    unsigned long long nWin = 0, nChk = 0;
    if (mapCountBounds(p, refLens, nWin, nChk) && (nWin > 0xffffffffull || nChk > 0xffffffffull)) {
        error = "map: the reference has " + std::to_string(nWin) + " seed windows and " + std::to_string(nChk) +
                " chunks; fewer than 4294967296 of each are supported";
        return DP_ERR_ARG;
    }
    return 0;
}

// ---- circular join chunks (mapping.go:93-95): the last query_size bases of a sequence followed by its first query_size.  Without
// -all_sequences the one sequence has a slot of its own even when it is empty; with it only the sequences that are long enough
// have one, and the others leave a line for stderr (the reference would slice out of range).
struct MapJoins {
    std::vector<std::string> joins;
    std::vector<int> joinOf;  // a sequence's join chunk among `joins`, -1: none
    std::string notes;
    uint32_t firstPaired = 0;  // device reads before the (forward, reverse complement) pairs: the sequences and their join chunks
};
inline MapJoins mapJoinChunks(const MapParams& p, const std::vector<i64>& refLens, const std::vector<const char*>& seqs,
                              const std::vector<std::string>& names) {
    const size_t T = refLens.size();
    MapJoins J;
    J.joinOf.assign(T, -1);
    for (size_t c = 0; c < T; c++) {
        const char* ref = seqs[c];
        const i64 refLen = refLens[c];
        if (!p.allSequences) {  // (a slot of its own even when it is empty)
            J.joinOf[c] = 0;
            J.joins.push_back(p.circular ? std::string(ref + (refLen - p.querySize), (size_t)p.querySize) + std::string(ref, (size_t)p.querySize) : std::string());
        } else if (p.circular && refLen >= p.querySize) {
            J.joinOf[c] = (int)J.joins.size();
            J.joins.push_back(std::string(ref + (refLen - p.querySize), (size_t)p.querySize) + std::string(ref, (size_t)p.querySize));
        } else if (p.circular) {  // (the reference would slice out of range, mapping.go:93-95)
            J.notes += "Sequence " + names[c] + " (" + std::to_string((long long)refLen) + " bases) is shorter than query_size " +
                       std::to_string((long long)p.querySize) + ": no circular join chunk\n";
        }
    }
    J.firstPaired = (uint32_t)(T + J.joins.size());
    return J;
}

// ---- the packed upload's layout: 2 bits per base, every device read on a 16-byte boundary.  Untrimmed the head comes first
// ([sequences | join chunks | reads]: sequence c is device read c, join j is T + j, read r is firstPaired + r); with a trim the
// raw reads come first, so that the trim's id lists and spans name raw read r as device read r (read r, sequence c at nReads + c,
// join j at nReads + T + j).  readOff: the read set's nReads + 1 offsets.
struct MapPacked {
    std::vector<uint32_t> plens;  // bases per device read as uploaded
    std::vector<uint64_t> poff;   // byte offset of each in the pinned block, and the block's size
    size_t headAt = 0, readsAt = 0;  // device ids of the first sequence / read as uploaded
};
inline MapPacked mapPackedLayout(const std::vector<i64>& refLens, const std::vector<std::string>& joins, const i64* readOff, size_t nReads,
                                 bool readsFirst) {
    const size_t T = refLens.size(), firstPaired = T + joins.size(), n = firstPaired + nReads;
    MapPacked P;
    P.headAt = readsFirst ? nReads : 0;
    P.readsAt = readsFirst ? 0 : firstPaired;
    P.plens.resize(n);
    P.poff.assign(n + 1, 0);
    for (size_t c = 0; c < T; c++) P.plens[P.headAt + c] = (uint32_t)refLens[c];
    for (size_t j = 0; j < joins.size(); j++) P.plens[P.headAt + T + j] = (uint32_t)joins[j].size();
    for (size_t r = 0; r < nReads; r++) P.plens[P.readsAt + r] = (uint32_t)(readOff[r + 1] - readOff[r]);
    for (size_t r = 0; r < n; r++) P.poff[r + 1] = P.poff[r] + ((((uint64_t)P.plens[r] + 3) / 4 + 15) & ~(uint64_t)15);
    return P;
}

// ---- a Mapper's batch (host_map.cpp: Mapper).  The head - sequences and join chunks, the device reads [0, firstPaired) - went up when
// the mapper was opened and stays; a batch's pinned block holds the batch alone, in the same host layout (read r at the sum of the
// 16-byte-rounded packed sizes before it), and dp_reads_replace_tail_packed_rc puts it behind the head as pairs: the forward strand of
// batch read r is device read firstPaired + 2 r, its reverse complement the next - the ids an upload of head + batch in one go gives.
inline MapPacked mapBatchLayout(const i64* readOff, size_t nReads) {
    return mapPackedLayout(std::vector<i64>(), std::vector<std::string>(), readOff, nReads, false);
}
inline uint32_t mapBatchReadId(uint32_t firstPaired, uint32_t read, bool reverse) { return firstPaired + 2 * read + (reverse ? 1u : 0u); }
// A batch that is trimmed first goes behind the head raw and unpaired (dp_reads_replace_tail_packed): raw read r is device read
// base + r with base = firstPaired, and that is the id the trim's resident calls and dp_reads_respan_tail_rc are given - the eligible
// reads' id list, the middle stage's chunk spans, and the spans trimmedReadSet cut from the raw reads.  Starts and lengths stay.
inline uint32_t mapTailId(uint32_t base, uint32_t read) { return base + read; }
inline std::vector<uint32_t> mapTailIds(const std::vector<uint32_t>& reads, uint32_t base) {
    std::vector<uint32_t> ids(reads.size());
    for (size_t i = 0; i < reads.size(); i++) ids[i] = mapTailId(base, reads[i]);
    return ids;
}
inline std::vector<dp_read_span> mapTailSpans(const std::vector<dp_read_span>& cut, uint32_t base) {
    std::vector<dp_read_span> spans(cut);
    for (dp_read_span& sp : spans) sp.read = mapTailId(base, sp.read);
    return spans;
}

// ---- chunk schedule mapping.go:79-96, canonical generation order; sequence after sequence, the chunk ids running on.  Sequence sq
// is device read sq, its join chunk device read T + joinOf[sq].
struct MapSchedule {
    std::vector<dp_scan_item> items;
    std::vector<std::pair<i64, i64>> meta;  // offset, inset per chunk, within its reference sequence
    std::vector<int> chunkRef;              // its reference sequence
};
inline MapSchedule mapChunkSchedule(const MapParams& p, const std::vector<i64>& refLens, const MapJoins& J) {
    const size_t T = refLens.size();
    const int k = p.k;
    MapSchedule S;
    for (size_t sq = 0; sq < T; sq++) {
        const i64 refLen = refLens[sq];
        for (i64 j = 0; j < 10; j++) {
            const i64 start = j * p.chunkSize, step = p.chunkSize * 10 - p.querySize;
            for (i64 i = start; i < refLen - p.chunkSize / 2; i += step) {
                i64 end = i + p.chunkSize;
                if (i >= refLen) end = refLen;
                if (end > refLen) end = refLen;  // SubSequence clamps
                dp_scan_item it;
                it.read = (uint32_t)sq;
                it.start = (uint32_t)i;
                it.n_kmers = (uint32_t)std::max<i64>(0, (end - i) - k + 1);
                it.min_seeds = 0;
                S.items.push_back(it);
                S.meta.push_back({i, refLen - (end - 1)});  // SubSequence: offset+start, inset + length - (end-1)
                S.chunkRef.push_back((int)sq);
            }
        }
        if (p.circular && J.joinOf[sq] >= 0) {
            // Append(...) is a fresh top-level sequence of 2*edge bases: len%4==0 loses its last 4 k-mers (asm:88-96)
            const i64 jl = (i64)J.joins[(size_t)J.joinOf[sq]].size();
            i64 nk = jl - k + 1;
            if (jl % 4 == 0) nk -= 4;
            dp_scan_item it;
            it.read = (uint32_t)(T + (size_t)J.joinOf[sq]);
            it.start = 0;
            it.n_kmers = (uint32_t)std::max<i64>(0, nk);
            it.min_seeds = 0;
            S.items.push_back(it);
            S.meta.push_back({refLen - p.querySize, refLen - (p.querySize - 1)});  // offset of the first part, inset of the second
            S.chunkRef.push_back((int)sq);
        }
    }
    return S;
}

// ---- the (forward, reverse complement) scan items of the window [a, b) of read `read` (L bases; device reads firstPaired + 2 read
// and the next).  whole: the top-level read itself, not a view of it.
inline void mapWindowItems(uint32_t firstPaired, uint32_t read, i64 L, i64 a, i64 b, bool whole, int k, dp_scan_item& f, dp_scan_item& r) {
    const uint32_t fr = mapBatchReadId(firstPaired, read, false), rr = mapBatchReadId(firstPaired, read, true);
    const i64 wl = b - a;
    f.read = fr;
    r.read = rr;
    f.min_seeds = r.min_seeds = 0;
    const i64 nk = wl - k + 1;
    if (whole && (L % 4) == 0) {
        // top-level query with finalLen == 0: the forward scan loses 4 k-mers; its ReverseComplement() has
        // firstLen == 0 and the scan starts 4 bases in (sequence.go:196, asm:109-132) — fixed up by mapFixReverseWhole
        f.start = 0;
        f.n_kmers = (uint32_t)std::max<i64>(0, nk - 4);
        r.start = 4;
        r.n_kmers = (uint32_t)std::max<i64>(0, nk - 4);
    } else {
        f.start = (uint32_t)a;
        f.n_kmers = (uint32_t)std::max<i64>(0, nk);
        r.start = (uint32_t)(L - b);
        r.n_kmers = (uint32_t)std::max<i64>(0, nk);
    }
}
inline bool mapReverseNeedsFix(bool reverseSide, bool whole, i64 L) { return reverseSide && whole && (L % 4) == 0; }
// The reverse strand of a whole read with L % 4 == 0, scanned from base 4 as mapWindowItems asks: in the reference's scan k-mer index 0
// duplicates the k-mer at base 4 and every later index is shifted by one (the firstLen == 0 quirk).  Rewrites the segments
// [gap, seed, ..., gap] that are the tail of `segs` from `base` on, in place.
inline void mapFixReverseWhole(std::vector<int32_t>& segs, size_t base, int k) {
    int32_t* sg = segs.data() + base;
    const size_t n = segs.size() - base;
    if (n >= 3 && sg[0] == 0) {  // the duplicated k-mer is a seed: it appears twice, 1-k apart
        std::vector<int32_t> fix;
        fix.push_back(0);
        fix.push_back(sg[1]);
        fix.push_back(1 - k);
        fix.insert(fix.end(), sg + 1, sg + n);
        segs.resize(base);
        segs.insert(segs.end(), fix.begin(), fix.end());
    } else {
        sg[0] += 1;  // all indices shift by one (no hits: the single gap counts the extra k-mer too)
    }
}

// ---- a sharded index's per-seed windows {count, first word, last word, last + 1} over the 64-chunk words of the WHOLE index, from
// every shard's own (include/downpore_hip.h, dp_index_set_global).  Shards hold whole words: shard s starts at word c0 / 64.
inline uint32_t mapChunksPerShard(uint32_t nChunks, uint32_t nShards) { return ((nChunks + nShards - 1) / nShards + 63) / 64 * 64; }
inline void mapGlobalWindowsInit(std::vector<uint32_t>& global, uint32_t S) {
    global.resize((size_t)S * 4);
    for (uint32_t i = 0; i < S; i++) {  // NewIntSet(): count 0, start 1, end 0 (last + 1 = 1)
        global[4 * (size_t)i + 0] = 0;
        global[4 * (size_t)i + 1] = 1;
        global[4 * (size_t)i + 2] = 0;
        global[4 * (size_t)i + 3] = 1;
    }
}
inline void mapGlobalWindowsMerge(std::vector<uint32_t>& global, const std::vector<uint32_t>& local, uint32_t S, uint32_t wordBase) {
    for (uint32_t i = 0; i < S; i++) {
        const uint32_t cnt = local[4 * (size_t)i];
        if (!cnt) continue;
        uint32_t* g = &global[4 * (size_t)i];
        const uint32_t st = local[4 * (size_t)i + 1] + wordBase, en = local[4 * (size_t)i + 2] + wordBase;
        if (g[0] == 0) {
            g[1] = st;
            g[2] = en;
        } else {
            g[1] = std::min(g[1], st);
            g[2] = std::max(g[2], en);
        }
        g[0] += cnt;
        g[3] = g[2] + 1;
    }
}

// ---- the reference index's layout.  Dense: S x ceil(M/64) + M x ceil(S/64) words per context or shard; the estimate sums them per
// device over every context / shard this run would build there.  Sparse (id lists, ~8 bytes per seed hit) when the estimate exceeds
// a device's free memory less an eighth of its total: a run that close could already fail in its later allocations.
inline uint64_t mapDenseBytes(uint64_t S, uint64_t m) { return S * ((m + 63) / 64) * 8 + m * ((S + 63) / 64) * 8; }
// dense bytes per device, devices in the order they are first used: the shards dealt round robin over `devs`, or (one context
// per mapper thread) nThreads whole indexes on `device`
inline std::vector<std::pair<int, uint64_t>> mapDenseEstimate(uint64_t S, uint32_t nChunks, int nShards, uint32_t perShard, const std::vector<int>& devs,
                                                              int device, size_t nThreads) {
    std::vector<std::pair<int, uint64_t>> perDev;  // device, dense bytes
    auto addDev = [&](int d, uint64_t b) {
        for (auto& pd : perDev)
            if (pd.first == d) return (void)(pd.second += b);
        perDev.push_back({d, b});
    };
    if (nShards > 1) {
        size_t i = 0;
        for (uint32_t c0 = 0; c0 < nChunks; c0 += perShard, i++) addDev(devs[i % devs.size()], mapDenseBytes(S, std::min(nChunks, c0 + perShard) - c0));
    } else {
        addDev(device, (uint64_t)nThreads * mapDenseBytes(S, nChunks));
    }
    return perDev;
}
inline bool mapDenseOver(uint64_t bytes, uint64_t freeBytes, uint64_t totalBytes) { return bytes + totalBytes / 8 > freeBytes; }
// mem[i] = (free, total) of perDev[i]'s device.  true: the dense layout is over on some device; *dTotal the estimate's sum
inline bool mapDenseOverAny(const std::vector<std::pair<int, uint64_t>>& perDev, const std::vector<std::pair<uint64_t, uint64_t>>& mem, uint64_t* dTotal) {
    bool over = false;
    *dTotal = 0;
    for (size_t i = 0; i < perDev.size(); i++) {
        *dTotal += perDev[i].second;
        if (mapDenseOver(perDev[i].second, mem[i].first, mem[i].second)) over = true;
    }
    return over;
}

}  // namespace dph
