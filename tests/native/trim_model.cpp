// TEST INFRASTRUCTURE ONLY: the checker of the `trim` edge stage.  A line-by-line C++ restatement of trim/trim.go (setupIndex,
// DetermineAdapters, isNewFullMatch, findMatches, checkAdapterWorker, trimWorker, PrintStats), seeds/seeds.go (NewAllSeedSequence,
// GetSeedsFromKmers), sequence/sequence.go (ShortKmers) and sequence/seqio.go (Write, Demultiplex) on the oracle's own types
// (oracle/oracle.hpp: PackedSeq views, IntSet, SeedIndex::newSeedSequence, ssMatch, smGetBasesCovered).  It shares no source with
// downpore_amd/csrc/host/host_trim.cpp or dp_trim.hip.  Built on demand by tests/trim_model.py against oracle/_build/liboracle.so.
//
// Canonical semantics: one worker (reads in file order); log lines without timestamps; the middle-adapter search (Trim's second half)
// is not restated; with seenCount == 0, where the reference divides by zero, PrintStats says "no reads long enough to trim".
// A FASTQ read whose quality line did not match its length is written with an empty quality line.
//
// mutation (tests of the hand cases only): 1 = `delta < 5` of trim.go:386 becomes `delta <= 5`; 2 = the `+` of :397 becomes `-`.
#include <cstring>
#include <fstream>
#include <map>
#include <string>
#include <vector>

#include "oracle.hpp"

using namespace dpo;

namespace {

struct Params {
    int k = 6;
    i64 checkReads = 10000;
    int threshold = 90, extraEdgeTrim = 5;
    bool tagAdapters = true, requirePairs = false, determine = true;
    int verbosity = 1, mutation = 0;
};

struct Rec {
    int32_t earliest, latest, found, bestMatch, ambiguous, bestIdent;
};

// sequence/sequence.go:482-504 ShortKmers on a packed view
std::vector<uint16_t> shortKmers(const PackedSeq& s, int k, bool collapse) {
    const i64 length = s.length - k + 1;
    std::vector<uint16_t> kmers((size_t)std::max<i64>(length, 1));
    i64 v = s.kmerAt(0, k);
    i64 mask = 0;
    for (int i = 0; i < k; i++) mask = (mask << 2) | 3;
    i64 prev = 0;
    size_t index = 0;
    for (i64 i = k; i < s.length; i++) {
        if (!collapse || v != prev || index == 0) {
            kmers[index] = (uint16_t)v;
            prev = v;
            index++;
        }
        v = s.nextKmer(v, mask, i);
    }
    kmers[index] = (uint16_t)v;
    index++;
    kmers.resize(index);
    return kmers;
}

// seeds/seeds.go:247-253
void getSeedsFromKmers(const SeedIndex& g, const std::vector<uint16_t>& kmers, IntSet& seedSet) {
    for (uint16_t k : kmers)
        if (g.kmers[k]) seedSet.add((u64)g.kmerMap[k]);
}

// seeds/seeds.go:204-237
SeedSequence* newAllSeedSequence(SeedIndex& g, const PackedSeq& seq) {
    const int k = g.seedSize;
    i64 mask = 0;
    for (int i = 0; i < k; i++) mask = (mask << 2) | 3;
    auto segments = std::make_shared<std::vector<i64>>();
    i64 prev = 0;
    i64 kmer = seq.kmerAt(0, k) >> 2;
    i64 kmerIndex = 0;
    for (i64 i = k - 1; i < seq.length; i++) {
        kmer = seq.nextKmer(kmer, mask, i);
        g.addSeedKmer(kmer);  // the `if !g.kmers[kmer] {...}` block :217-226
        segments->push_back(kmerIndex - prev);
        segments->push_back((i64)g.kmerMap[(size_t)kmer]);
        prev = kmerIndex + k;
        kmerIndex++;
    }
    segments->push_back(0);
    SeedSequence* s = g.arena.make();
    s->store = segments;
    s->lo = 0;
    s->n = segments->size();
    s->length = seq.length;
    s->id = seq.id;
    s->name = std::make_shared<std::string>(seq.getName());
    s->offset = seq.offset;
    s->inset = seq.inset;
    return s;
}

bool hasPrefix(const std::string& s, const char* p) { return s.compare(0, strlen(p), p) == 0; }

struct Trimmer {  // trim.go:13-40
    std::vector<PackedSeq> originalFront, originalBack;
    std::vector<SeedSequence*> frontAdapters, backAdapters;
    std::vector<IntSet> frontAdapterSets, backAdapterSets;
    std::vector<int> pairsFront, pairsBack;
    std::unique_ptr<SeedIndex> index;
    Params p;
    std::vector<i64> frontCounts, backCounts;
    i64 noCount = 0, seenCount = 0;
    std::string err;

    void log(const std::string& s) { err += s + "\n"; }

    void setupIndex() {  // :57-99
        frontAdapters.clear();
        frontAdapterSets.clear();
        backAdapters.clear();
        backAdapterSets.clear();
        index.reset(new SeedIndex(p.k));
        for (const PackedSeq& s : originalFront) {
            frontAdapters.push_back(newAllSeedSequence(*index, s));
            IntSet set;
            getSeedsFromKmers(*index, shortKmers(s, p.k, true), set);
            frontAdapterSets.push_back(set);
        }
        for (const PackedSeq& s : originalBack) {
            backAdapters.push_back(newAllSeedSequence(*index, s));
            IntSet set;
            getSeedsFromKmers(*index, shortKmers(s, p.k, true), set);
            backAdapterSets.push_back(set);
        }
        frontCounts.assign(originalFront.size(), 0);
        backCounts.assign(originalBack.size(), 0);
        int pairID = 1;
        pairsFront.assign(originalFront.size(), 0);
        pairsBack.assign(originalBack.size(), -1);
        for (size_t i = 0; i < originalFront.size(); i++) {
            const std::string name = originalFront[i].getName();
            pairsFront[i] = -1;
            for (size_t j = 0; j < originalBack.size(); j++)
                if (originalBack[j].getName() == name) {
                    pairsFront[i] = pairID;
                    pairsBack[j] = pairID;
                    pairID++;
                    break;
                }
        }
    }

    // :326-352
    void isNewFullMatch(const IntSet& kmerSet, const PackedSeq& seq, int threshold, std::vector<SeedSequence*>& adapters,
                        std::vector<IntSet>& adapterSets, std::vector<uint8_t>& enabled, size_t base) {
        SeedSequence* seedSeq = nullptr;
        for (size_t i = 0; i < adapterSets.size(); i++) {
            const IntSet& adapter = adapterSets[i];
            if (enabled[base + i]) continue;
            const i64 hits = (i64)kmerSet.countIntersection(adapter);
            const i64 minHits = (i64)adapter.size() / 2;
            if (hits >= minHits) {
                if (!seedSeq) seedSeq = index->newSeedSequence(seq);
                std::vector<SeedMatch> ms = ssMatch(index->arena, seedSeq, adapters[i], &adapter, &kmerSet, minHits - 1, p.k);
                for (const SeedMatch& m : ms)
                    if ((i64)m.MatchA.size() >= minHits) {
                        i64 identity = 0, b = 0;
                        smGetBasesCovered(m, p.k, &identity, &b);
                        if ((identity * 100) / adapters[i]->length >= threshold) enabled[base + i] = 1;
                    }
            }
        }
    }

    // :354-428, returning its variables as they stand before the `if ambiguous` of :423
    Rec findMatches(const IntSet& kmerSet, const PackedSeq& seq, std::vector<SeedSequence*>& adapters, std::vector<IntSet>& adapterSets,
                    std::vector<i64>& counts) {
        SeedSequence* seedSeq = nullptr;
        i64 earliest = seq.length;
        i64 latest = 0;
        bool found = false;
        i64 bestMatch = 0, bestIdent = 0;
        bool barcoded = false, ambiguous = false;
        for (size_t i = 0; i < adapterSets.size(); i++) {
            const IntSet& adapter = adapterSets[i];
            const i64 hits = (i64)kmerSet.countIntersection(adapter);
            const i64 fraction = (hits * 10) / (i64)adapter.size();
            if (fraction >= 2 || hits >= 3) {
                if (!seedSeq) seedSeq = index->newSeedSequence(seq);
                std::vector<SeedMatch> ms = ssMatch(index->arena, seedSeq, adapters[i], &adapter, &kmerSet, 3, p.k);
                for (const SeedMatch& m : ms) {
                    if (m.MatchA.size() >= 3) {
                        i64 identity = 0, b = 0;
                        smGetBasesCovered(m, p.k, &identity, &b);
                        identity = (identity * 100) / adapters[i]->length;
                        const bool isBarcode = hasPrefix(*adapters[i]->name, "Barcode");
                        if (!barcoded && isBarcode) {
                            barcoded = true;
                            bestIdent = identity;
                            bestMatch = (i64)i;
                        } else if (barcoded) {
                            if (isBarcode) {
                                const i64 delta = identity - bestIdent;
                                ambiguous = (p.mutation == 1 ? delta <= 5 : delta < 5) && delta > -5;
                                if (identity > bestIdent) {
                                    bestIdent = identity;
                                    bestMatch = (i64)i;
                                }
                            }
                        } else if (identity > bestIdent) {
                            bestIdent = identity;
                            bestMatch = (i64)i;
                        }
                        const i64 aOff = adapters[i]->getSeedOffset(m.MatchA[0], p.k);
                        i64 start = seedSeq->getSeedOffset(m.MatchB[0], p.k) + (p.mutation == 2 ? -aOff : aOff);  // :397
                        i64 end = seedSeq->getSeedOffset(m.MatchB.back(), p.k) + adapters[i]->getSeedOffsetFromEnd(m.MatchA.back(), p.k);
                        if (start < earliest) {
                            if (start < 0) start = 0;
                            earliest = start;
                        }
                        if (end > latest) {
                            if (end > seq.length) end = seq.length;
                            latest = end;
                        }
                        found = true;
                        counts[i]++;
                    }
                }
            }
        }
        return Rec{(int32_t)earliest, (int32_t)latest, found ? 1 : 0, (int32_t)bestMatch, ambiguous ? 1 : 0, (int32_t)bestIdent};
    }
};

struct Model {
    FastaSet reads;
    Trimmer t;
    std::vector<uint8_t> enabled;      // over the adapters as loaded (front then back); empty: no determination
    std::vector<int32_t> eligible;     // reads the workers do not skip (:434 / :455)
    std::vector<Rec> recs;             // two per eligible read
    std::vector<i64> frontTrim, backTrim;
    std::vector<int32_t> table, ints;
    std::string out, adapters, index;
    bool failed = false;
};

const int edgeSize = 150;

void kmerSetOf(Trimmer& t, const PackedSeq& edge, IntSet& kmerSet) {  // :439-441 / :460-463
    kmerSet.clear();
    getSeedsFromKmers(*t.index, shortKmers(edge, t.p.k, true), kmerSet);
}

// DetermineAdapters (:272-324).  enabledIn != nullptr: the flags come from the caller instead of checkAdapterWorker.
void determineAdapters(Model& m, const uint8_t* enabledIn) {
    Trimmer& t = m.t;
    const size_t nF = t.frontAdapters.size(), nB = t.backAdapters.size();
    m.enabled.assign(nF + nB, 0);
    if (enabledIn) {
        m.enabled.assign(enabledIn, enabledIn + nF + nB);
    } else {
        // GetNSequencesFrom(0, numReads) + checkAdapterWorker (:430-449)
        IntSet kmerSet;
        const size_t n = (size_t)std::max<i64>(0, std::min<i64>(t.p.checkReads, (i64)m.reads.size()));
        for (size_t r = 0; r < n; r++) {
            const PackedSeq seq = m.reads.served(r);
            if (seq.length < edgeSize + 50) continue;
            const PackedSeq frontSeq = seq.subSequence(0, edgeSize);
            const PackedSeq backSeq = seq.subSequence(seq.length - edgeSize, seq.length);
            kmerSetOf(t, frontSeq, kmerSet);
            t.isNewFullMatch(kmerSet, frontSeq, t.p.threshold, t.frontAdapters, t.frontAdapterSets, m.enabled, 0);
            kmerSetOf(t, backSeq, kmerSet);
            t.isNewFullMatch(kmerSet, backSeq, t.p.threshold, t.backAdapters, t.backAdapterSets, m.enabled, nF);
        }
    }
    for (int side = 0; side < 2; side++) {  // :285-303, :304-322
        std::vector<PackedSeq>& original = side ? t.originalBack : t.originalFront;
        const uint8_t* en = m.enabled.data() + (side ? nF : 0);
        const size_t n = side ? nB : nF;
        size_t count = 0;
        for (size_t i = 0; i < n; i++) count += en[i] ? 1 : 0;
        if (t.p.verbosity > 0)
            t.log(std::to_string(count) + " / " + std::to_string(n) + (side ? " back" : " front") + " adapters identified with high identity matches.");
        for (size_t i = n; i-- > 0;) {
            if (en[i]) {
                if (t.p.verbosity > 0) t.log(" - " + original[i].getName());
            } else {
                original[i] = original[original.size() - 1];
                original.pop_back();
            }
        }
    }
    t.setupIndex();
}

// trimWorker (:451-513); recsIn / countsIn != nullptr: findMatches' results come from the caller
void trimAll(Model& m, const Rec* recsIn, const i64* countsIn) {
    Trimmer& t = m.t;
    const size_t n = m.reads.size();
    m.frontTrim.assign(n, 0);
    m.backTrim.assign(n, 0);
    m.table.assign(n * 5, 0);
    for (size_t r = 0; r < n; r++) m.table[5 * r + 3] = m.table[5 * r + 4] = -1;
    if (t.p.verbosity > 0) t.log("Trimming ends and indexing all sequences against " + std::to_string(t.frontAdapters.size()) + " adapters...");  // :141
    if (countsIn) {
        for (size_t i = 0; i < t.frontCounts.size(); i++) t.frontCounts[i] = countsIn[i];
        for (size_t i = 0; i < t.backCounts.size(); i++) t.backCounts[i] = countsIn[t.frontCounts.size() + i];
    }
    IntSet kmerSet;
    size_t slot = 0;
    for (size_t r = 0; r < n; r++) {
        const PackedSeq seq = m.reads.served(r);
        if (seq.length < edgeSize + 50) continue;
        Rec f, b;
        if (recsIn) {
            f = recsIn[2 * slot];
            b = recsIn[2 * slot + 1];
        } else {
            const PackedSeq frontSeq = seq.subSequence(0, edgeSize);
            const PackedSeq backSeq = seq.subSequence(seq.length - edgeSize, seq.length);
            kmerSetOf(t, frontSeq, kmerSet);
            f = t.findMatches(kmerSet, frontSeq, t.frontAdapters, t.frontAdapterSets, t.frontCounts);
            kmerSetOf(t, backSeq, kmerSet);
            b = t.findMatches(kmerSet, backSeq, t.backAdapters, t.backAdapterSets, t.backCounts);
        }
        slot++;
        m.eligible.push_back((int32_t)r);
        m.recs.push_back(f);
        m.recs.push_back(b);
        // :423-427 "trim, but pretend we didn't see an adapter"
        i64 start = f.latest;
        bool foundStart = f.ambiguous ? false : f.found != 0;
        i64 matchIndex = f.ambiguous ? 0 : f.bestMatch;
        i64 end = b.earliest;
        bool foundEnd = b.ambiguous ? false : b.found != 0;
        i64 backMatchIndex = b.ambiguous ? 0 : b.bestMatch;
        if (t.p.requirePairs) {  // :471-485
            int fp = -1, bp = -1;
            if (foundStart) fp = t.pairsFront[(size_t)matchIndex];
            if (foundEnd) bp = t.pairsBack[(size_t)backMatchIndex];
            if (fp != bp) {
                foundStart = false;
                foundEnd = false;
            }
        }
        t.seenCount++;
        if (!foundStart) t.noCount++;
        start += t.p.extraEdgeTrim;
        end = edgeSize - end + t.p.extraEdgeTrim;
        if (start + end + 10 >= seq.length) {
            m.reads.ignore[r] = 1;
        } else {
            if (foundStart) {
                m.frontTrim[r] = start;
                if (t.p.tagAdapters) m.reads.names[r] = *t.frontAdapters[(size_t)matchIndex]->name + "_" + m.reads.names[r];
            } else if (end > start && start > 0) {
                m.frontTrim[r] = start;
            }
            if (foundEnd || (end > start && end < seq.length)) m.backTrim[r] = end;
        }
        m.table[5 * r + 3] = foundStart ? (int32_t)matchIndex : -1;
        m.table[5 * r + 4] = foundEnd ? (int32_t)backMatchIndex : -1;
    }
    for (size_t r = 0; r < n; r++) {
        m.table[5 * r] = (int32_t)m.frontTrim[r];
        m.table[5 * r + 1] = (int32_t)m.backTrim[r];
        m.table[5 * r + 2] = m.reads.ignore[r];
    }
}

// PrintStats (:260-268) + commands/trim.go:44
void printStats(Model& m) {
    Trimmer& t = m.t;
    if (t.seenCount == 0) {
        t.log("no reads long enough to trim");
        m.failed = true;
        return;
    }
    for (size_t i = 0; i < t.frontCounts.size(); i++)
        t.log("Front adapter: " + t.originalFront[i].getName() + " \t " + std::to_string((t.frontCounts[i] * 100) / t.seenCount) + " %");
    for (size_t i = 0; i < t.backCounts.size(); i++)
        t.log("Back adapter: " + t.originalBack[i].getName() + " \t " + std::to_string((t.backCounts[i] * 100) / t.seenCount) + " %");
    t.log(std::to_string((t.noCount * 100) / t.seenCount) + " % with no adapters found.");
    t.log("Writing trimmed sequences...");
}

// what GetSequences serves once trims are set (seqio.go:149-186): the trimmed stretch re-read as a top-level sequence, and its
// quality bytes from the same stretch of the quality line
std::string recordText(const Model& m, size_t r, const std::string& name) {
    const PackedSeq& c = m.reads.cached[r];
    const i64 ft = m.frontTrim[r], n = c.length - m.frontTrim[r] - m.backTrim[r];
    const PackedSeq seq = newPackedSequence((i64)r, c.str().substr((size_t)ft, (size_t)n), nullptr);
    std::string s;
    if (m.reads.isFastq) {  // fastqWriter :415-435
        std::string q;
        if (c.qual)
            for (i64 j = 0; j < n; j++) q += (char)(uint8_t)((*c.qual)[c.qlo + (size_t)(ft + j)] + 33);
        s = "@" + name + "\n" + seq.str() + "\n+\n" + q + "\n";
    } else {  // fastaWriter :401-414
        s = ">" + name + "\n" + seq.str() + "\n";
    }
    return s;
}

void writeAll(Model& m) {  // Write(os.Stdout, true) :438-458, one worker
    m.out.clear();
    for (size_t r = 0; r < m.reads.size(); r++)
        if (!m.reads.ignore[r]) m.out += recordText(m, r, m.reads.names[r]);
}

Model* load(const char* readsPath, const char* frontPath, const char* backPath, const int64_t* params) {
    Model* m = new Model();
    Params& p = m->t.p;
    p.k = (int)params[0];
    p.checkReads = params[1];
    p.threshold = (int)params[2];
    p.extraEdgeTrim = (int)params[3];
    p.tagAdapters = params[4] != 0;
    p.requirePairs = params[5] != 0;
    p.determine = params[6] != 0;
    p.verbosity = (int)params[7];
    p.mutation = (int)params[8];
    // LoadTrimmer (:102-116) and commands/trim.go:35
    m->t.originalFront = FastaSet::fromFile(frontPath, 0, false).cached;
    m->t.originalBack = FastaSet::fromFile(backPath, 0, false).cached;
    m->reads = FastaSet::fromFile(readsPath, 50, false);
    m->t.setupIndex();
    return m;
}

void finish(Model* m, const Rec* recsIn, const i64* countsIn) {
    trimAll(*m, recsIn, countsIn);
    printStats(*m);
    if (!m->failed) writeAll(*m);
    Trimmer& t = m->t;
    for (size_t i = 0; i < t.originalFront.size(); i++) m->adapters += "F\t" + t.originalFront[i].getName() + "\t" + std::to_string(t.frontCounts[i]) + "\n";
    for (size_t i = 0; i < t.originalBack.size(); i++) m->adapters += "B\t" + t.originalBack[i].getName() + "\t" + std::to_string(t.backCounts[i]) + "\n";
}

}  // namespace

extern "C" {

// params[9] = k, check_reads, adapter_threshold, extra_end_trim, tag_adapters, require_pairs, determine_adapters, verbosity, mutation
void* tm_run(const char* readsPath, const char* frontPath, const char* backPath, const int64_t* params) {
    Model* m = load(readsPath, frontPath, backPath, params);
    if (m->t.p.determine) determineAdapters(*m, nullptr);
    finish(m, nullptr, nullptr);
    return m;
}

// the same with the matching stage's results supplied: enabled (may be null) over the adapters as loaded; recs = six int32 per end,
// two per read of 200 bases and more; counts per adapter of the lists after determination
void* tm_run_with_records(const char* readsPath, const char* frontPath, const char* backPath, const int64_t* params, const uint8_t* enabled,
                          const int32_t* recs, const int64_t* counts) {
    Model* m = load(readsPath, frontPath, backPath, params);
    if (enabled) determineAdapters(*m, enabled);
    finish(m, (const Rec*)recs, (const i64*)counts);
    return m;
}

// DetermineAdapters alone: afterwards which = 3 gives the flags and which = 2 of tm_text the compacted adapter order
void* tm_determine(const char* readsPath, const char* frontPath, const char* backPath, const int64_t* params) {
    Model* m = load(readsPath, frontPath, backPath, params);
    determineAdapters(*m, nullptr);
    Trimmer& t = m->t;
    for (size_t i = 0; i < t.originalFront.size(); i++) m->adapters += "F\t" + t.originalFront[i].getName() + "\t0\n";
    for (size_t i = 0; i < t.originalBack.size(); i++) m->adapters += "B\t" + t.originalBack[i].getName() + "\t0\n";
    return m;
}

void tm_free(void* h) { delete (Model*)h; }
int tm_failed(void* h) { return ((Model*)h)->failed ? 1 : 0; }

// which: 0 output, 1 log lines, 2 adapters ("F|B <tab> name <tab> matches") after determination
const char* tm_text(void* h, int which, int64_t* n) {
    Model* m = (Model*)h;
    const std::string& s = which == 0 ? m->out : which == 1 ? m->t.err : m->adapters;
    *n = (int64_t)s.size();
    return s.data();
}

// which: 0 per-read table (5 per read), 1 edge records (6 per end), 2 counts (front then back), 3 determine flags, 4 eligible reads,
// 5 k-mer -> seed table (4^k, -1 none), 6 adapter segments (concatenated), 7 their offsets (n + 1), 8 pairs (front then back)
const int32_t* tm_ints(void* h, int which, int64_t* n) {
    Model* m = (Model*)h;
    Trimmer& t = m->t;
    std::vector<int32_t>& v = m->ints;
    v.clear();
    if (which == 0) v = m->table;
    else if (which == 1)
        for (const Rec& r : m->recs) v.insert(v.end(), {r.earliest, r.latest, r.found, r.bestMatch, r.ambiguous, r.bestIdent});
    else if (which == 2) {
        for (i64 c : t.frontCounts) v.push_back((int32_t)c);
        for (i64 c : t.backCounts) v.push_back((int32_t)c);
    } else if (which == 3) v.assign(m->enabled.begin(), m->enabled.end());
    else if (which == 4) v = m->eligible;
    else if (which == 5)
        for (size_t i = 0; i < t.index->kmers.size(); i++) v.push_back(t.index->kmers[i] ? t.index->kmerMap[i] : -1);
    else if (which == 6 || which == 7) {
        int32_t off = 0;
        if (which == 7) v.push_back(0);
        for (const auto* list : {&t.frontAdapters, &t.backAdapters})
            for (const SeedSequence* s : *list) {
                if (which == 6)
                    for (size_t i = 0; i < s->n; i++) v.push_back((int32_t)s->seg()[i]);
                off += (int32_t)s->n;
                if (which == 7) v.push_back(off);
            }
    } else if (which == 8) {
        v.assign(t.pairsFront.begin(), t.pairsFront.end());
        v.insert(v.end(), t.pairsBack.begin(), t.pairsBack.end());
    }
    *n = (int64_t)v.size();
    return v.data();
}

// Demultiplex (seqio.go:460-523) into dir; returns the number of files (they replace existing ones)
int tm_demultiplex(void* h, const char* dir) {
    Model* m = (Model*)h;
    std::map<std::string, std::string> partitions;
    std::vector<std::string> order;
    const char* ext = m->reads.isFastq ? ".fastq" : ".fasta";
    for (size_t r = 0; r < m->reads.size(); r++) {
        if (m->reads.ignore[r]) continue;
        const std::string n = m->reads.names[r];
        if (!hasPrefix(n, "Barcode")) continue;
        const size_t pos = n.find('_');
        if (pos != std::string::npos) {
            const std::string label = n.substr(0, pos);
            if (!partitions.count(label)) order.push_back(label);
            partitions[label] += recordText(*m, r, n.substr(pos + 1));  // SetName(id, n[pos+1:]) then the writer with fullNames
        }
    }
    for (const std::string& label : order) {
        std::ofstream f(std::string(dir) + "/" + label + ext, std::ios::binary | std::ios::trunc);
        f << partitions[label];
    }
    return (int)order.size();
}
}
