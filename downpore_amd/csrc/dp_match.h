// Seed-space chaining on one wave, shared by the kernels that run SeedSequence.Match (seeds/sequence.go:361-394) on the device:
// map_kernel (dp_map.hip), trim_edge_kernel and trim_mid_kernel (dp_trim.hip).  Reduced (:85-123), dynamicMatch (:401-471), extendChain (:476-576)
// and the set membership tests they use.  The working set type LT supplies q / t (reduced query / target segments), qIdx / tIdx,
// headChain / headLen and good[M_GOOD]; chain storage is an HBM pool of M_CHAINS fixed-stride slots per wave (MChainPool).
#pragma once
#include "dp_common.h"

typedef uint64_t u64;

#define M_CHAINS 1024     // chains that may be started per candidate (pool slots per wave)
#define M_GOOD 512

__device__ __forceinline__ bool m_contains(const u64* __restrict__ set, int32_t x) { return (set[x >> 6] >> (x & 63)) & 1ull; }
// a sorted id list (the sparse index's seed-set rows, the windows' seed lists): membership by binary search
struct MList {
    const uint32_t* ids;
    uint32_t n;
};
__device__ __forceinline__ bool m_has(const u64* __restrict__ set, int32_t x) { return m_contains(set, x); }
__device__ __forceinline__ bool m_has(const MList& l, int32_t x) {
    uint32_t lo = 0, hi = l.n;
    while (lo < hi) {
        const uint32_t m = (lo + hi) >> 1;
        if (l.ids[m] < (uint32_t)x) lo = m + 1;
        else hi = m;
    }
    return lo < l.n && l.ids[lo] == (uint32_t)x;
}

// SeedSequence.Reduced (seeds/sequence.go:85-123).  Returns the number of reduced seeds or -1 if < minSeeds.
// err bit 1: LDS capacity.
template <typename IDX>
__device__ int m_reduce(const int32_t* __restrict__ seg, int n, const u64* __restrict__ whitelist, int k, int minSeeds,
                        int32_t* out, IDX* index, int cap, uint32_t* err) {
    int count = 0, prev = -1;
    for (int i = 1; i < n; i += 2) {
        const int next = seg[i];
        if (next != prev && m_contains(whitelist, next)) {
            count++;
            prev = next;
        }
    }
    if (count < minSeeds) return -1;
    if (count > cap) {
        *err |= 1;
        return -1;
    }
    int offset = seg[0];
    prev = -1;
    int j = 0;
    for (int i = 1; i < n; i += 2) {
        const int seed = seg[i];
        if (prev != seed && m_contains(whitelist, seed)) {
            out[j] = offset;
            out[j + 1] = seed;
            index[j / 2] = (IDX)(i / 2);
            j += 2;
            offset = seg[i + 1];
            prev = seed;
        } else {
            offset += seg[i + 1] + k;
        }
    }
    out[j] = offset;
    return count;
}

// The same on the whole wave: lane i takes seed base + i of every 64-seed piece; its whitelist probe is one of 64 in flight (on one
// lane the probes of a 250-seed chunk were 2 x 250 dependent global loads - half a millisecond per candidate).  A seed is kept when
// it is whitelisted and differs from the last KEPT seed; a whitelisted seed is dropped only when it equals the last kept one, which
// then stays what it was - so "differs from the previous whitelisted seed" decides, and all lanes decide at once.  The gap written
// before kept seed a (previous kept seed p, or -1) is sum_{t=p+1..a} gap_t + k (a - p - 1): prefix sums of the gaps.
template <typename IDX, class SET>
__device__ int m_reduce_wave(const int32_t* __restrict__ seg, int n, SET whitelist, int k, int minSeeds, int32_t* out,
                             IDX* index, int cap, uint32_t* err) {
    const int lane = dp_lane();
    const u64 below = (1ull << lane) - 1ull;
    const int nS = n >> 1;
    int kept = 0, carrySeed = -1, prevKept = -1;  // seeds kept so far, last whitelisted seed, index of the last kept seed
    long long gRun = 0, gPrevKept = 0;            // sum of gap_0 .. gap_{base-1}, prefix sum at the last kept seed
    bool over = false;
    for (int base = 0; base < nS; base += 64) {
        const int sI = base + lane;
        const bool valid = sI < nS;
        const int seed = valid ? seg[2 * sI + 1] : -1;
        const int gap = valid ? seg[2 * sI] : 0;
        const bool c = valid && m_has(whitelist, seed);
        const u64 cmask = __ballot(c);
        const u64 cb = cmask & below;
        const int srcC = cb ? 63 - __builtin_clzll(cb) : 0;
        const int fromC = __shfl(seed, srcC, 64);
        const int prevC = cb ? fromC : carrySeed;
        const bool keep = c && seed != prevC;
        const u64 kmask = __ballot(keep);
        const long long G = gRun + (long long)wave_incl_sum(gap);  // inclusive prefix sum of the gaps up to this seed
        // the previous kept seed: in this piece (a lane below), or carried over
        const u64 kb = kmask & below;
        const int srcK = kb ? 63 - __builtin_clzll(kb) : 0;
        const long long gFrom = __shfl((long long)G, srcK, 64);
        const int pIdx = kb ? base + srcK : prevKept;
        const long long gP = kb ? gFrom : gPrevKept;
        if (keep) {
            const int j = kept + __popcll(kb);
            if (j < cap) {
                out[2 * j] = (int32_t)(G - gP + (long long)k * (sI - pIdx - 1));
                out[2 * j + 1] = seed;
                index[j] = (IDX)sI;
            } else {
                over = true;
            }
        }
        kept += __popcll(kmask);
        if (cmask) carrySeed = __shfl(seed, 63 - __builtin_clzll(cmask), 64);
        if (kmask) {
            const int lk = 63 - __builtin_clzll(kmask);
            prevKept = base + lk;
            gPrevKept = __shfl((long long)G, lk, 64);
        }
        gRun = __shfl((long long)G, 63, 64);
    }
    if (kept < minSeeds) return -1;
    if (__ballot(over) || kept > cap) {
        *err |= 1;
        return -1;
    }
    if (lane == 0) {  // final gap: everything after the last kept seed
        const long long gEnd = gRun + (long long)seg[2 * nS];
        out[2 * kept] = (int32_t)(gEnd - gPrevKept + (long long)k * (nS - 1 - prevKept));
    }
    __builtin_amdgcn_wave_barrier();
    return kept;
}

struct MChainPool {
    uint16_t* a;  // [M_CHAINS][stride]: stride = the reduced query's capacity (M_QMAX, or the BIG variant's)
    uint16_t* b;
    uint32_t stride;
    __device__ __forceinline__ uint16_t* A(int c) const { return a + (size_t)c * stride; }
    __device__ __forceinline__ uint16_t* B(int c) const { return b + (size_t)c * stride; }
};

// extendChain (seeds/sequence.go:476-576); a = reduced query, b = reduced target.  Returns the chain's final length.
template <class LT>
__device__ int m_extend(LT& L, int an, int bn, int aIndex, int bIndex, int k, int cur, int curLen, const MChainPool& P) {
    const int32_t* as = L.q;
    const int32_t* bs = L.t;
    uint16_t* ca = P.A(cur);
    uint16_t* cb = P.B(cur);
    int offsetA = as[aIndex + 1], offsetB = bs[bIndex + 1];
    aIndex += 2;
    bIndex += 2;
    while (aIndex < an && bIndex < bn) {
        int aSeedIndex = aIndex / 2;
        int minBOffset, maxBOffset;
        if (offsetA < 0) {
            minBOffset = -k;
            maxBOffset = 0;
        } else {
            minBOffset = (offsetA * 2) / 3 - k;
            maxBOffset = (offsetA * 3) / 2 + k;
        }
        while (maxBOffset < offsetB) {
            offsetA += as[aIndex + 1] + k;
            aIndex += 2;
            if (aIndex >= an) return curLen;
            aSeedIndex = aIndex / 2;
            minBOffset = (offsetA * 2) / 3 - k;
            maxBOffset = (offsetA * 3) / 2 + k;
        }
        while (offsetB < minBOffset) {
            offsetB += bs[bIndex + 1] + k;
            bIndex += 2;
            if (bIndex >= bn) return curLen;
        }
        const int oldBIndex = bIndex, oldBOffset = offsetB;
        bool matched = false;
        const int seedA = as[aIndex];
        while (offsetB <= maxBOffset) {
            if (seedA == bs[bIndex]) {
                const int hc = L.headChain[aSeedIndex];
                if (hc >= 0) {
                    const int hl = L.headLen[aSeedIndex];
                    if (bIndex / 2 == (int)P.B(hc)[hl - 1] && hl > curLen) return curLen;  // they have a better chain already
                }
                ca[curLen] = (uint16_t)aSeedIndex;
                cb[curLen] = (uint16_t)(bIndex / 2);
                curLen++;
                L.headChain[aSeedIndex] = cur;
                L.headLen[aSeedIndex] = (uint16_t)curLen;
                offsetA = as[aIndex + 1];
                offsetB = bs[bIndex + 1];
                aIndex += 2;
                bIndex += 2;
                matched = true;
                break;
            } else {
                offsetB += bs[bIndex + 1] + k;
                bIndex += 2;
                if (bIndex >= bn) break;
            }
        }
        if (!matched) {
            offsetA += as[aIndex + 1] + k;
            aIndex += 2;
            offsetB = oldBOffset;
            bIndex = oldBIndex;
        }
    }
    return curLen;
}

// dynamicMatch (seeds/sequence.go:401-471).  seq = reduced target (L.t, sn ints), query = reduced query (L.q, qn ints).
// Fills L.good with chain slots (in the reference's allGoodChains order) and their lengths in goodLen; returns count.
// err bit 2: chain pool exhausted, bit 4: good list overflow.
template <class LT>
__device__ int m_dynamic_match(LT& L, int qn, int sn, int minMatch, int k, const MChainPool& P, uint16_t* chainLen,
                               uint32_t* err) {
    if (minMatch == 0) minMatch = 1;
    const int nq = qn / 2;
    for (int i = 0; i < nq; i++) L.headChain[i] = -1;
    int nChains = 0, nGood = 0;
    const int32_t* qs = L.q;
    const int32_t* ss = L.t;
    for (int qIndex = 1; qIndex < qn - minMatch * 2 + 2; qIndex += 2) {
        if (qs[qIndex - 1] < 0 && qIndex > 1 && qs[qIndex + 1] < 0 && qs[qIndex] == qs[qIndex - 2] && qs[qIndex] == qs[qIndex + 2])
            continue;
        const int qsi = qIndex / 2;
        if (L.headChain[qsi] >= 0) continue;
        int prevSeed = -1;
        for (int i = 1; i < sn - minMatch * 2 + 2; i += 2) {
            const int nextSeed = ss[i];
            const int hc = L.headChain[qsi];
            if (nextSeed == qs[qIndex] && nextSeed != prevSeed && (hc < 0 || (int)P.B(hc)[L.headLen[qsi] - 1] != i / 2)) {
                if (nChains >= M_CHAINS) {
                    *err |= 2;
                    return nGood;
                }
                const int c = nChains++;
                P.A(c)[0] = (uint16_t)qsi;
                P.B(c)[0] = (uint16_t)(i / 2);
                L.headChain[qsi] = c;
                L.headLen[qsi] = 1;
                const int len = m_extend(L, qn, sn, qIndex, i, k, c, 1, P);
                chainLen[c] = (uint16_t)len;
                if (len >= minMatch) {
                    const int nextLength = (len * 2) / 3;
                    if (nextLength > minMatch) {
                        minMatch = nextLength;
                        for (int j = nGood - 1; j >= 0; j--) {
                            if ((int)chainLen[L.good[j]] < nextLength) {
                                L.good[j] = L.good[nGood - 1];
                                nGood--;
                            }
                        }
                    }
                    if (nGood >= M_GOOD) {
                        *err |= 4;
                        return nGood;
                    }
                    L.good[nGood++] = c;
                    int remaining = 0;
                    for (int x = 0; x < nq; x++) remaining += L.headChain[x] < 0;
                    if (remaining < len) return nGood;
                }
            }
            prevSeed = nextSeed;
        }
    }
    return nGood;
}

// dynamicMatch with the whole wave (round 4).  The reference's loop nest is "for every query seed that heads no chain yet: for
// every target seed: equal?" - |q| x |t| probes (125 x 250 for a 250-seed reference chunk) of which a handful are hits; on one lane
// that scan WAS map_kernel's time (1.24 ms per launch).  Here the 64 lanes probe 64 target seeds at once (equal to the query seed
// and not a repeat of the target seed in front of it: both are facts of positions, not of the walk's state), and lane 0 handles
// the hits in ascending order exactly as the one-lane loop does - the head-chain test at the moment of the hit, extendChain, the
// 2 len / 3 ratchet (which also shortens both loops' bounds), the "fewer open query seeds than this chain is long" exit.  What
// lane 0 decides (chain count, good count, minMatch, stop) is broadcast after every hit, so every lane runs the same loops.
template <class LT>
__device__ int m_dynamic_match_wave(LT& L, int qn, int sn, int minMatch, int k, const MChainPool& P, uint16_t* chainLen,
                                    uint32_t* err) {
    const int lane = dp_lane();
    if (minMatch == 0) minMatch = 1;
    const int nq = qn / 2, nsT = sn / 2;
    for (int i = lane; i < nq; i += 64) L.headChain[i] = -1;
    __builtin_amdgcn_wave_barrier();
    int nChains = 0, nGood = 0;
    const int32_t* qs = L.q;
    const int32_t* ss = L.t;
    for (int qIndex = 1; qIndex < qn - minMatch * 2 + 2; qIndex += 2) {
        if (qs[qIndex - 1] < 0 && qIndex > 1 && qs[qIndex + 1] < 0 && qs[qIndex] == qs[qIndex - 2] && qs[qIndex] == qs[qIndex + 2])
            continue;
        const int qsi = qIndex / 2;
        if (L.headChain[qsi] >= 0) continue;
        const int qseed = qs[qIndex];
        for (int tb = 0; 2 * tb + 1 < sn - minMatch * 2 + 2; tb += 64) {
            const int t = tb + lane, i = 2 * t + 1;
            bool hit = false;
            if (t < nsT && i < sn - minMatch * 2 + 2) {
                const int sd = ss[i];
                hit = sd == qseed && (t == 0 || ss[i - 2] != sd);  // (prevSeed of the reference's scan = the target seed in front)
            }
            unsigned long long m = __ballot(hit);
            while (m) {
                const int j = __builtin_ctzll(m);
                m &= m - 1;
                const int ti = 2 * (tb + j) + 1;
                if (ti >= sn - minMatch * 2 + 2) break;  // (a ratchet inside this stretch moved the bound in front of the hit)
                int stop = 0;
                if (lane == 0) {
                    const int hc = L.headChain[qsi];
                    if (hc < 0 || (int)P.B(hc)[L.headLen[qsi] - 1] != ti / 2) {
                        if (nChains >= M_CHAINS) {
                            *err |= 2;
                            stop = 1;
                        } else {
                            const int c = nChains++;
                            P.A(c)[0] = (uint16_t)qsi;
                            P.B(c)[0] = (uint16_t)(ti / 2);
                            L.headChain[qsi] = c;
                            L.headLen[qsi] = 1;
                            const int len = m_extend(L, qn, sn, qIndex, ti, k, c, 1, P);
                            chainLen[c] = (uint16_t)len;
                            if (len >= minMatch) {
                                const int nextLength = (len * 2) / 3;
                                if (nextLength > minMatch) {
                                    minMatch = nextLength;
                                    for (int g = nGood - 1; g >= 0; g--) {
                                        if ((int)chainLen[L.good[g]] < nextLength) {
                                            L.good[g] = L.good[nGood - 1];
                                            nGood--;
                                        }
                                    }
                                }
                                if (nGood >= M_GOOD) {
                                    *err |= 4;
                                    stop = 1;
                                } else {
                                    L.good[nGood++] = c;
                                    int remaining = 0;
                                    for (int x = 0; x < nq; x++) remaining += L.headChain[x] < 0;
                                    if (remaining < len) stop = 1;
                                }
                            }
                        }
                    }
                }
                __builtin_amdgcn_wave_barrier();
                nChains = __builtin_amdgcn_readfirstlane(nChains);
                nGood = __builtin_amdgcn_readfirstlane(nGood);
                minMatch = __builtin_amdgcn_readfirstlane(minMatch);
                stop = __builtin_amdgcn_readfirstlane(stop);
                if (stop) return nGood;
            }
        }
    }
    return nGood;
}
