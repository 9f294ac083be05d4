// The test bench of libdownpore_host.so (dph_testhooks.h, version node DPH_TEST): host logic on bare numbers and flat arrays,
// self-tests and helpers that only files under tests/ call.  None of it is on the pipeline's path; the boundary's entry points
// are in host_capi.cpp.
#include <unistd.h>

#include <algorithm>
#include <cstring>

#include "dph_handles.hpp"
#include "dph_testhooks.h"
#include "host_util.hpp"

using namespace dph;

extern "C" {

// "name\tACGT...\n" per read, bases spelled from their 2-bit codes: lets tests compare this reader with the oracle's
const char* dph_reads_dump(void* h, int64_t* n) {
    static thread_local std::string out;
    out.clear();
    ReadSet& s = ((ReadsH*)h)->set;
    for (size_t i = 0; i < s.size(); i++) {
        out += s.names[i];
        out += '\t';
        const char* b = s.seq(i);
        for (i64 j = 0; j < s.length(i); j++) out += "ACGT"[baseCode((unsigned char)b[j])];
        if (const uint8_t* q = s.quality(i)) {  // FASTQ: the stored quality bytes (phred - 33), two hex digits each
            out += '\t';
            for (i64 j = 0; j < s.length(i); j++) {
                out += "0123456789abcdef"[q[j] >> 4];
                out += "0123456789abcdef"[q[j] & 15];
            }
        }
        out += '\n';
    }
    *n = (int64_t)out.size();
    return out.data();
}

// ---- test hooks: three decision rules of the host side on bare numbers, held to answers worked by hand from the reference's Go
// text (tests/golden/hand/, tests/test_hand_known_answers.py) - not part of the pipeline's boundary
int dph_hand_is_consistent(const int64_t* left5, const int64_t* right4, int circular, int64_t ref_len) {
    return dph::handIsConsistent((const dph::i64*)left5, (const dph::i64*)right4, circular != 0, (dph::i64)ref_len) ? 1 : 0;
}
int dph_hand_remove_dominated(const int64_t* maps3, int n, int64_t query_len, int* kept) {
    return dph::handRemoveDominated((const dph::i64*)maps3, n, (dph::i64)query_len, kept);
}
void dph_hand_trim_indices(int upto, const int32_t* match_a, const int64_t* off, int n_matches, int min_match, int length, int* out2) {
    std::vector<dph::SeedMatch> store((size_t)n_matches);
    std::vector<dph::SeedMatch*> ms;
    for (int i = 0; i < n_matches; i++) {
        store[(size_t)i].MatchA.assign(match_a + off[i], match_a + off[i + 1]);
        ms.push_back(&store[(size_t)i]);
    }
    dph::trimBestIndices(upto, ms, min_match, length, &out2[0], &out2[1]);
}

int dph_hand_add_seeds(const char* bases, int64_t len, int k, int num_seeds, const double* values, uint32_t* seed_map, int cap) {
    dph::SeedIndex ix(k);
    ix.addSeeds(bases, (dph::i64)len, num_seeds, dph::ValueView(values));
    if ((int)ix.seedMap.size() > cap) return -1;
    for (size_t i = 0; i < ix.seedMap.size(); i++) seed_map[i] = (uint32_t)ix.seedMap[i];
    return (int)ix.seedMap.size();
}
int dph_hand_bases_covered(const int32_t* a_seg, int a_n, const int32_t* b_seg, int b_n, const int32_t* match_a, const int32_t* match_b, int n,
                           int k, int64_t* out2) {
    dph::SeedSeq A, B;
    A.seg = a_seg;
    A.n = a_n;
    B.seg = b_seg;
    B.n = b_n;
    dph::SeedMatch m;
    m.SeqA = &A;
    m.SeqB = &B;
    m.MatchA.assign(match_a, match_a + n);
    m.MatchB.assign(match_b, match_b + n);
    dph::i64 a = 0, b = 0;
    bool panic = false;
    dph::matchBasesCovered(m, k, &a, &b, &panic);
    out2[0] = a;
    out2[1] = b;
    return panic ? 1 : 0;
}
int dph_hand_consensus(const int32_t* segs, const int64_t* off, int n_seqs, int k, int32_t* cons_out, int64_t cons_cap, int64_t* cons_n,
                       int* kept, int64_t* out_counts, int32_t* out_a, int32_t* out_b, int64_t cap, int64_t* n_matches) {
    dph::Arena ar;
    std::vector<dph::SeedSeq> store((size_t)n_seqs);
    std::vector<dph::SeedSeq*> seqs;
    for (int i = 0; i < n_seqs; i++) {
        store[(size_t)i].seg = segs + off[i];
        store[(size_t)i].n = (int)(off[i + 1] - off[i]);
        store[(size_t)i].id = i;
        seqs.push_back(&store[(size_t)i]);
    }
    std::vector<dph::SeedMatch*> ms;
    dph::SeedSeq* cons = dph::multiAlignerConsensus(ar, seqs, k, ms);
    if (!cons || cons->n > cons_cap) return -1;
    for (int i = 0; i < cons->n; i++) cons_out[i] = cons->seg[i];
    *cons_n = cons->n;
    *n_matches = (int64_t)ms.size();
    int64_t at = 0;
    for (size_t j = 0; j < ms.size(); j++) {
        kept[j] = ms[j]->SeqB ? ms[j]->SeqB->id : -1;
        out_counts[j] = (int64_t)ms[j]->MatchA.size();
        for (size_t x = 0; x < ms[j]->MatchA.size(); x++) {
            if (at >= cap) return -1;
            out_a[at] = ms[j]->MatchA[x];
            out_b[at] = ms[j]->MatchB[x];
            at++;
        }
    }
    return 0;
}
void dph_pack_bases(const char* bases, int64_t n, uint8_t* out, int scalar_only) { dph::packBases(bases, (size_t)n, out, scalar_only != 0); }
long dph_test_coroutines(int n_tasks, int yields) { return dph::coroSelfTest(n_tasks, yields); }

// host-logic test hook: the value table (commands/overlap.go:55-92) from a k-mer histogram; counts is overwritten with the
// merged forward + reverse-complement counts like the reference's in-place loop
void dph_values_from_counts(uint64_t* counts, int k, double* out) {
    std::vector<uint64_t> c(counts, counts + ((size_t)1 << (2 * k)));
    std::vector<double> v = kmerValuesFromCounts(c, k);
    memcpy(out, v.data(), v.size() * sizeof(double));
    memcpy(counts, c.data(), c.size() * sizeof(uint64_t));
}

}  // extern "C"

// ---- host-logic test hook (no GPU needed): ignore flags that arrive while the planner thread holds a finished plan in
// its hands (set DP_TUNE=plan_delay_us).  A commit flags one read below the next plan's firstIn and one of that plan's own
// query reads; the plan must be thrown away and recomputed.  Returns 0 = the plan handed out is current, 1 = stale plan,
// <0 = the scenario could not be set up.
extern "C" int dph_selftest_planner_flags(void* readsH, int k, int64_t seedBatchSize, const double* values) {
    ReadSet& reads = ((ReadsH*)readsH)->set;
    OverlapParams p;
    p.k = k;
    p.seedBatchSize = seedBatchSize;
    Planner pl(reads, p, values, true, nullptr);
    std::shared_ptr<const RoundPlan> p0 = pl.get(0);  // the thread goes on with plan 1 (prefetch depth)
    if (!p0 || p0->empty || p0->firstOut <= 1 || p0->firstOut >= (i64)reads.size()) return -1;
    const long delay = dp_tune("plan_delay_us", 0);
    if (delay <= 0) return -2;
    usleep((useconds_t)(delay / 2));  // plan 1 is computed by now and sits in the hook's sleep
    const int small = 0, big = (int)p0->firstOut;  // big = first query read of plan 1
    pl.applyIgnores({small, big}, 0);
    pl.dropBefore(1, p0->firstOut);
    std::shared_ptr<const RoundPlan> p1 = pl.get(1);
    if (!p1 || p1->firstIn != p0->firstOut) return -3;
    for (const auto& w : p1->windows)
        if ((int)w.read == big || (int)w.read == small) return 1;
    return 0;
}

// ---- host-logic test hook (no GPU needed): the whole plan chain of a read set three ways - the general PrepareQueries path
// (no window cache), the window-cache path with one planner lane, and with `lanes` lanes that start plans from guesses of
// where their predecessors end - with the same commits in all three (every `flagEvery`-th round flags two reads ahead of the
// chain, as a final check would).  The window cache's producer selects on the host here (WindowCache with ctx == nullptr).
// Returns 0 = all chains equal, r + 1 = they differ in round r, < 0 = set-up problem; *nRounds = plans of the chain.
extern "C" int dph_selftest_planner_lanes(void* readsH, int k, int64_t seedBatchSize, const double* values, int lanes, int flagEvery,
                                          int64_t* nRounds) {
    ReadSet& reads = ((ReadsH*)readsH)->set;
    OverlapParams p;
    p.k = k;
    p.seedBatchSize = seedBatchSize;
    struct Rec {
        i64 firstIn, firstOut;
        std::vector<Overlapper::Window> windows;
        std::vector<uint32_t> seedMap;
        bool empty;
    };
    auto chain = [&](bool useCache, int nLanes, std::vector<Rec>& out) -> int {
        std::fill(reads.ignore.begin(), reads.ignore.end(), 0);
        std::unique_ptr<WindowCache> wc;
        if (useCache) wc.reset(new WindowCache(nullptr, reads, p.overlapSize, k, p.numSeeds, ValueView(values)));
        Planner pl(reads, p, ValueView(values), true, nullptr, wc.get());
        pl.setLanes(nLanes);
        for (i64 r = 0;; r++) {
            std::shared_ptr<const RoundPlan> pp = pl.get(r);
            if (!pp) return -1;
            if (pp->failed) return -2;
            out.push_back({pp->firstIn, pp->firstOut, pp->windows, pp->seedMap, pp->empty});
            if (pp->empty) break;
            if (r > 100000) return -3;
            std::vector<int> flags;
            if (flagEvery > 0 && r % flagEvery == flagEvery - 1) {  // one read a little ahead of the chain, one far ahead
                const i64 a = pp->firstOut + 3, b = pp->firstOut + 40;
                if (a < (i64)reads.size()) flags.push_back((int)a);
                if (b < (i64)reads.size()) flags.push_back((int)b);
            }
            pl.applyIgnores(flags, r);
            pl.dropBefore(r + 1, pp->firstOut);
        }
        return 0;
    };
    std::vector<Rec> a, b, c;
    if (int rc = chain(false, 1, a)) return rc;
    if (int rc = chain(true, 1, b)) return rc - 10;
    if (int rc = chain(true, lanes, c)) return rc - 20;
    std::fill(reads.ignore.begin(), reads.ignore.end(), 0);
    if (nRounds) *nRounds = (int64_t)a.size();
    auto same = [](const Rec& x, const Rec& y) {
        if (x.firstIn != y.firstIn || x.firstOut != y.firstOut || x.empty != y.empty || x.seedMap != y.seedMap || x.windows.size() != y.windows.size()) return false;
        for (size_t i = 0; i < x.windows.size(); i++)
            if (x.windows[i].read != y.windows[i].read || x.windows[i].start != y.windows[i].start || x.windows[i].len != y.windows[i].len) return false;
        return true;
    };
    for (size_t r = 0; r < std::max(a.size(), std::max(b.size(), c.size())); r++) {
        if (r >= a.size() || r >= b.size() || r >= c.size()) return (int)r + 1;
        if (!same(a[r], b[r]) || !same(a[r], c[r])) return (int)r + 1;
    }
    return 0;
}

// ---- test hook: SeedIndex::touchesSeed on evaluated k-mers, every instruction-set variant the CPU has against the scalar one.
// Fills res[w] (w < nWindows; windows of `stride` k-mers) with the scalar answers; returns the number of disagreements, and
// sets *isaMask to the variants that ran (bit 1 AVX2, bit 2 AVX-512).
extern "C" int dph_selftest_touch(int k, const uint32_t* seeds, int64_t nSeeds, const uint32_t* kmers, int64_t nWindows, int64_t stride,
                                  uint8_t* res, int* isaMask) {
    SeedIndex ix(k, 21);
    for (int64_t i = 0; i < nSeeds; i++) ix.addSeedKmer(seeds[i]);
    int bad = 0, mask = 0;
    if (__builtin_cpu_supports("avx2")) mask |= 2;
    if (__builtin_cpu_supports("avx512f")) mask |= 4;
    for (int64_t w = 0; w < nWindows; w++) {
        const uint32_t* km = kmers + w * stride;
        const bool a = ix.touchesSeedWith(0, km, (uint32_t)stride);
        res[w] = a ? 1 : 0;
        if ((mask & 2) && ix.touchesSeedWith(1, km, (uint32_t)stride) != a) bad++;
        if ((mask & 4) && ix.touchesSeedWith(2, km, (uint32_t)stride) != a) bad++;
        if (ix.touchesSeed(km, (uint32_t)stride) != a) bad++;
    }
    if (isaMask) *isaMask = mask;
    return bad;
}

// ---- host-logic test hook (no GPU needed): finalCheckWorker over externally supplied matches ----------------------
// Queries and indexed sequences come as flat arrays in the reference's segment layout; matches as (query index,
// target index, MatchA, MatchB).  Returns the PAF text of the round and applies SetIgnore to `reads`.
extern "C" const char* dph_finalcheck(void* readsH, int k, int64_t overlapSize, const uint32_t* seedKmers, int64_t nSeeds,
                                      const int32_t* qSegs, const int64_t* qOff, const int64_t* qId, const int64_t* qSeqId,
                                      const int64_t* qLen, const int64_t* qOffset, const int64_t* qInset, int64_t nQ,
                                      const int32_t* iSegs, const int64_t* iOff, const int64_t* iId, const int64_t* iLen,
                                      const int64_t* iOffset, const int64_t* iInset, int64_t nI, const int64_t* mQuery,
                                      const int64_t* mTarget, const int64_t* mOff, const int32_t* mA, const int32_t* mB,
                                      int64_t nM, int64_t numQuerySeqs, int64_t* outLen, int64_t* outStats) {
    static thread_local std::string paf;
    ReadSet& reads = ((ReadsH*)readsH)->set;
    SeedIndex index(k);
    for (int64_t i = 0; i < nSeeds; i++) index.addSeedKmer(seedKmers[i]);
    index.buildRcTable();
    Arena& ar = index.arena;
    std::vector<SeedSeq*> qs, is;
    for (int64_t q = 0; q < nQ; q++) {
        SeedSeq* s = ar.make();
        s->seg = qSegs + qOff[q];
        s->n = (int)(qOff[q + 1] - qOff[q]);
        s->id = (int)qSeqId[q];
        s->length = qLen[q];
        s->offset = qOffset[q];
        s->inset = qInset[q];
        s->rc = (q & 1) != 0;
        qs.push_back(s);
    }
    for (int64_t q = 0; q + 1 < nQ; q += 2) qs[(size_t)q + 1]->reverseComplement = qs[(size_t)q];  // rc query -> fwd (sequence.go:157)
    for (int64_t i = 0; i < nI; i++) {
        SeedSeq* root = ar.make();
        root->length = reads.length((size_t)iId[i]);
        root->id = (int)iId[i];
        SeedSeq* s = ar.make();
        s->seg = iSegs + iOff[i];
        s->n = (int)(iOff[i + 1] - iOff[i]);
        s->id = (int)iId[i];
        s->length = iLen[i];
        s->offset = iOffset[i];
        s->inset = iInset[i];
        s->parent = root;
        is.push_back(s);
    }
    std::vector<std::unique_ptr<SeedMatch>> matches;
    for (int64_t m = 0; m < nM; m++) {
        std::unique_ptr<SeedMatch> sm(new SeedMatch());
        sm->MatchA.assign(mA + mOff[m], mA + mOff[m + 1]);
        sm->MatchB.assign(mB + mOff[m], mB + mOff[m + 1]);
        sm->SeqA = qs[(size_t)mQuery[m]];
        sm->SeqB = is[(size_t)mTarget[m]];
        sm->QueryID = (int)qId[mQuery[m]];
        sm->ReverseComplementQuery = (mQuery[m] & 1) != 0;
        matches.push_back(std::move(sm));
    }
    FinalCheckStats fs;
    paf.clear();
    finalCheck(ar, index, reads, matches, numQuerySeqs, overlapSize, paf, fs);
    if (outStats) {
        outStats[0] = fs.badBack;
        outStats[1] = fs.emptyMatch;
        outStats[2] = (int64_t)fs.lines;
    }
    *outLen = (int64_t)paf.size();
    return paf.data();
}

// test hook: the host's exact Match of one (chunk, front adapter) pair - what the pairs beyond the kernel's working set are given
// to - with the identity test of trim.go:527-530; out = six int32 per passing match (adapter and chunk as passed in); returns their number
extern "C" int64_t dph_hand_trim_match(const int32_t* chunk_segs, int n_chunk, const int32_t* adapter_segs, int n_adapter, int adapter_len, int n_seeds,
                                       int k, int threshold, int adapter, int chunk, int32_t* out, int64_t cap) {
    std::vector<TrimMidRec> recs;
    trimHostMatch(chunk_segs, n_chunk, adapter_segs, n_adapter, adapter_len, n_seeds, k, threshold, adapter, chunk, recs);
    for (size_t i = 0; i < recs.size() && (int64_t)i < cap; i++) memcpy(out + 6 * i, &recs[i], sizeof(TrimMidRec));
    return (int64_t)recs.size();
}

// ---- host-logic test hook (no GPU needed): the plan chain of a round-parallel run of `world` ranks whose planners each compute
// only the plans of their own rounds (Planner::setOwnership) and guess where the rounds in between end.  Every simulated rank has
// its own copy of the read set (its own flags), its own window cache (host producer) and planner; the driver plays the commit:
// round r's plan comes from its owner, is accepted iff it starts at the committed firstSequence (what OverlapRun::resultValid
// checks) - otherwise every rank is told the truth (dropBefore) and the owner is asked again - and is then committed on every
// rank (flags of every `flagEvery`-th round + dropBefore).  The accepted chain must equal the one a single dense planner walks.
// Returns 0 = equal, r + 1 = differs in round r, < 0 = set-up problem / a round that never became valid; *nRounds = plans of the
// chain, *nRedone = plans that had to be asked for again because their guess did not hold.
extern "C" int dph_selftest_planner_sparse(void* readsH, int k, int64_t seedBatchSize, const double* values, int world, int flagEvery,
                                           int64_t* nRounds, int64_t* nRedone) {
    ReadSet& reads = ((ReadsH*)readsH)->set;
    OverlapParams p;
    p.k = k;
    p.seedBatchSize = seedBatchSize;
    struct Rec {
        i64 firstIn, firstOut;
        std::vector<Overlapper::Window> windows;
        std::vector<uint32_t> seedMap;
        bool empty;
    };
    auto flagsOf = [&](i64 r, i64 firstOut, size_t n) {
        std::vector<int> flags;
        if (flagEvery > 0 && r % flagEvery == flagEvery - 1) {
            const i64 a = firstOut + 3, b = firstOut + 40;
            if (a < (i64)n) flags.push_back((int)a);
            if (b < (i64)n) flags.push_back((int)b);
        }
        return flags;
    };
    std::vector<Rec> ref, got;
    {
        std::fill(reads.ignore.begin(), reads.ignore.end(), 0);
        WindowCache wc(nullptr, reads, p.overlapSize, k, p.numSeeds, ValueView(values));
        Planner pl(reads, p, ValueView(values), true, nullptr, &wc);
        for (i64 r = 0;; r++) {
            std::shared_ptr<const RoundPlan> pp = pl.get(r);
            if (!pp || pp->failed) return -1;
            ref.push_back({pp->firstIn, pp->firstOut, pp->windows, pp->seedMap, pp->empty});
            if (pp->empty) break;
            if (r > 100000) return -3;
            pl.applyIgnores(flagsOf(r, pp->firstOut, reads.size()), r);
            pl.dropBefore(r + 1, pp->firstOut);
        }
        std::fill(reads.ignore.begin(), reads.ignore.end(), 0);
    }
    i64 redone = 0;
    {
        std::vector<std::unique_ptr<ReadSet>> rs;
        std::vector<std::unique_ptr<WindowCache>> wcs;
        std::vector<std::unique_ptr<Planner>> pls;
        for (int w = 0; w < world; w++) {
            rs.emplace_back(new ReadSet(reads));
            wcs.emplace_back(new WindowCache(nullptr, *rs[w], p.overlapSize, k, p.numSeeds, ValueView(values)));
            pls.emplace_back(new Planner(*rs[w], p, ValueView(values), true, nullptr, wcs[w].get()));
            pls[w]->setLanes(3);
            pls[w]->setOwnership(w, world);
            if (!pls[w]->sparse()) return -4;
        }
        i64 firstSequence = 0;
        // (the executor slots of a rank ask for the plans of rounds well ahead of the commit point - that is what makes them
        // speculative: here every round's plan is fetched from its owner 2 * world rounds before its turn)
        std::map<i64, std::pair<std::shared_ptr<const RoundPlan>, i64>> ahead;  // plan, commit point when it was fetched
        std::vector<i64> flagRound(reads.size(), -1);                            // round whose commit flagged the read
        bool ended = false;
        for (i64 r = 0;; r++) {
            Planner& owner = *pls[(size_t)(r % world)];
            for (i64 j = r; j <= r + 2 * world && !ended; j++) {
                if (ahead.count(j)) continue;
                std::shared_ptr<const RoundPlan> q = pls[(size_t)(j % world)]->get(j);
                if (!q || q->failed) return -5;
                ahead[j] = {q, r};
                if (q->empty) break;  // (what lies behind an "end of input" - real or guessed - is asked for once it is settled)
            }
            std::shared_ptr<const RoundPlan> pp = ahead.count(r) ? ahead[r].first : owner.get(r);
            i64 snap = ahead.count(r) ? ahead[r].second : r;
            ahead.erase(r);
            for (int attempt = 0;; attempt++) {
                if (!pp || pp->failed) return -5;
                // OverlapRun::resultValid / emptyResultValid: the plan starts at the committed firstSequence and none of its query
                // reads was flagged by a round committed since it was made
                bool valid = pp->empty ? (pp->round == r && pp->firstIn == firstSequence) : pp->firstIn == firstSequence;
                for (size_t i = 0; valid && i < pp->windows.size(); i++)
                    if (flagRound[pp->windows[i].read] >= snap) valid = false;
                if (valid) break;
                snap = r;
                if (attempt >= 3) return -6;
                redone++;
                // the commit point has reached r and the plan does not start there: every rank knows where r starts (dropBefore
                // of the last commit), the owner plans the round again
                pp = owner.get(r);
            }
            ended = pp->empty;
            got.push_back({pp->firstIn, pp->firstOut, pp->windows, pp->seedMap, pp->empty});
            if (pp->empty) break;
            if (r > 100000) return -3;
            firstSequence = pp->firstOut;
            const std::vector<int> flags = flagsOf(r, pp->firstOut, reads.size());
            for (int id : flags)
                if (flagRound[(size_t)id] < 0) flagRound[(size_t)id] = r;
            for (auto& q : pls) {
                q->applyIgnores(flags, r);
                q->dropBefore(r + 1, firstSequence);
            }
        }
    }
    if (nRounds) *nRounds = (int64_t)ref.size();
    if (nRedone) *nRedone = redone;
    auto same = [](const Rec& x, const Rec& y) {
        if (x.firstIn != y.firstIn || x.firstOut != y.firstOut || x.empty != y.empty || x.seedMap != y.seedMap || x.windows.size() != y.windows.size()) return false;
        for (size_t i = 0; i < x.windows.size(); i++)
            if (x.windows[i].read != y.windows[i].read || x.windows[i].start != y.windows[i].start || x.windows[i].len != y.windows[i].len) return false;
        return true;
    };
    for (size_t r = 0; r < std::max(ref.size(), got.size()); r++) {
        if (r >= ref.size() || r >= got.size()) return (int)r + 1;
        if (!same(ref[r], got[r])) return (int)r + 1;
    }
    return 0;
}
