// MODEL of `map -all_sequences` — test infrastructure only (tests/map_multi_model.py compiles it on demand against liboracle.so).
//
// The mapper of mapping/mapping.go built over the sequence set R_0 .. R_{T-1} (the top-level sequences of the reference file, in
// file order, lengths L_c) instead of over its first sequence, written on the oracle's types (SeedIndex, PackedSeq, SeedSequence,
// ssMatch, goSort).  The rules, each marked [n] where it is applied:
//   [1] value table: every sequence of the file (commands/map.go:45-71), as it is.
//   [2] seeds: AddSingleSeeds(R_c) for c = 0 .. T-1 on ONE SeedIndex (seed ids in order of addition; a window adds nothing when a k-mer
//       of its count region is a seed already, whichever sequence added it; L_c <= seed_rate: no window).
//   [3] chunks, for c in order: the ten passes of mapping.go:79-91 over R_c, then (circular) R_c's join chunk (:93-95); chunk ids run
//       on; every chunk remembers c, its offset / inset are relative to R_c; L_c < query_size: no join chunk and one stderr line;
//       L_c <= chunk_size / 2: no regular chunk; IndexSequences once.
//   [4] performMapping: m.reference.Len() (:530-531, :570-571) is L_c of the candidate chunk's sequence; Mapping gains ref = c; the
//       de-duplication (:590-607) sorts by (ref, Start) and removes a pair only when the refs agree as well.
//   [5] isConsistent: false first when the refs differ; its reference length is L_ref; matchPairs' combined mapping takes ra.ref.
//       findSplitPoint, mapNext, Map and removeDominated are textually the oracle's.
//   [6] AsString: columns 6, 7 and the circular mappedLength correction use the mapping's sequence.
//   [7] output: reads in file order, a read's lines in Map's order, the four counts per read over all its lines.
// With all_sequences = 0 only R_0 is used: the oracle's runMap.  Zero chunks in total: every read is unmapped.
// Mutations (tests prove the cases can tell them): 1 = isConsistent ignores ref, 2 = L_0 is used for every sequence's End.
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "oracle.hpp"

using namespace dpo;

namespace {

struct MM : Mapping {
    int ref = 0;
};
inline int refOf(const Mapping* m) { return static_cast<const MM*>(m)->ref; }

struct MultiMapper {
    SeedIndex index;
    std::vector<PackedSeq> refs;
    std::vector<int> chunkRef;
    i64 edgeSize;
    bool circular;
    int mutation;
    std::string notes;
    std::vector<std::unique_ptr<MM>> pool;

    MM* mk() {
        pool.emplace_back(new MM());
        return pool.back().get();
    }
    i64 lenOf(int c) const { return refs[(size_t)c].length; }

    MultiMapper(const std::vector<PackedSeq>& rs, bool circ, int k, const double* values, i64 seedRate, i64 edge, i64 chunkSize, int mut)
        : index(k), refs(rs), edgeSize(edge), circular(circ), mutation(mut) {
        for (const PackedSeq& r : refs) index.addSingleSeeds(r, seedRate, values);  // [2]
        i64 ind = 0;
        auto addChunk = [&](const PackedSeq& piece, int c) {
            SeedSequence* s = index.newSeedSequence(piece);
            s->id = ind++;
            index.addSequence(s);
            chunkRef.push_back(c);
        };
        for (size_t c = 0; c < refs.size(); c++) {  // [3]
            const PackedSeq& reference = refs[c];
            for (i64 j = 0; j < 10; j++) {
                const i64 start = j * chunkSize, step = chunkSize * 10 - edgeSize;
                for (i64 i = start; i < reference.length - chunkSize / 2; i += step) {
                    i64 end = i + chunkSize;
                    if (i >= reference.length) end = reference.length;
                    addChunk(reference.subSequence(i, end), (int)c);
                }
            }
            if (!circular) continue;
            if (reference.length < edgeSize) {
                notes += "Sequence " + reference.getName() + " (" + std::to_string(reference.length) + " bases) is shorter than query_size " +
                         std::to_string(edgeSize) + ": no circular join chunk\n";
                continue;
            }
            addChunk(reference.subSequence(reference.length - edgeSize, reference.length).append(0, reference.subSequence(0, edgeSize)), (int)c);
        }
        index.indexSequences();
    }

    std::string asString(const Mapping& m) const {  // [6]
        const PackedSeq& reference = refs[(size_t)refOf(&m)];
        i64 mappedLength = m.End - m.Start;
        if (circular && mappedLength < 0) mappedLength = reference.length - m.Start + m.End;
        return m.Query->getName() + "\t" + std::to_string(m.Query->length) + "\t" + std::to_string(m.QueryOffset) + "\t" +
               std::to_string(m.Query->length - m.QueryInset) + "\t" + (m.RC ? "-" : "+") + "\t" + reference.getName() + "\t" +
               std::to_string(reference.length) + "\t" + std::to_string(m.Start) + "\t" + std::to_string(m.End) + "\t" + std::to_string(m.ids) +
               "\t" + std::to_string(mappedLength) + "\t255";
    }

    bool isConsistent(const Mapping* left, const Mapping* right) const {  // [5]
        if (mutation != 1 && refOf(left) != refOf(right)) return false;
        return mappingsConsistent(left, left->Query->length, right, circular, lenOf(refOf(left)));
    }

    void matchPairs(std::vector<Mapping*>& openA, std::vector<Mapping*>& openB, std::vector<Mapping*>& matched, bool& matchedNil) {
        matched.clear();
        matchedNil = true;
        for (i64 i = (i64)openA.size() - 1; i >= 0; i--) {
            Mapping* ra = openA[(size_t)i];
            for (i64 j = (i64)openB.size() - 1; j >= 0; j--) {
                Mapping* rb = openB[(size_t)j];
                if (isConsistent(ra, rb)) {
                    const i64 qOffset = ra->QueryOffset, qInset = rb->QueryInset;
                    if (ra->RC) std::swap(ra, rb);
                    MM* combined = mk();
                    combined->Start = ra->Start;
                    combined->End = rb->End;
                    combined->Query = ra->Query;
                    combined->QueryOffset = qOffset;
                    combined->QueryInset = qInset;
                    combined->RC = ra->RC;
                    combined->ids = ra->ids + rb->ids;
                    combined->ref = refOf(ra);  // [5]
                    matchedNil = false;
                    matched.push_back(combined);
                    openA[(size_t)i] = openA.back();
                    openA.pop_back();
                    openB[(size_t)j] = openB.back();
                    openB.pop_back();
                    break;
                }
            }
        }
    }

    void findSplitPoint(const PackedSeq& query, std::vector<Mapping*>& openA, std::vector<Mapping*>& openB, i64 left, i64 right) {
        while (right - left >= edgeSize) {
            const i64 start = (right + left - edgeSize) / 2, end = start + edgeSize;
            std::vector<Mapping*> mid = performMapping(query.subSequence(start, end));
            i64 newLeft = left, newRight = right, afterA = 0, afterB = 0;
            for (Mapping* mm : mid) {
                mm->Query = &query;
                for (Mapping* ma : openA) {
                    if (isConsistent(ma, mm)) {
                        ma->QueryInset = mm->QueryInset;
                        ma->ids += mm->ids;
                        if (ma->RC) ma->Start = mm->Start;
                        else ma->End = mm->End;
                        const i64 midMatched = query.length - mm->QueryInset - mm->QueryOffset;
                        if (midMatched > afterA) afterA = midMatched;
                        if (query.length - mm->QueryInset > newLeft) newLeft = query.length - mm->QueryInset;
                        break;
                    }
                }
                if (afterA < (edgeSize * 2) / 3) {
                    for (Mapping* mb : openB) {
                        if (isConsistent(mm, mb)) {
                            mb->QueryOffset = mm->QueryOffset;
                            mb->ids += mm->ids;
                            if (mb->RC) mb->End = mm->End;
                            else mb->Start = mm->Start;
                            const i64 midMatched = query.length - mm->QueryInset - mm->QueryOffset;
                            if (midMatched > afterB) afterB = midMatched;
                            if (mm->QueryOffset < newRight) newRight = mm->QueryOffset;
                            break;
                        }
                    }
                }
            }
            if (afterA > 0 && afterB > 0) {
                std::vector<Mapping*> empty;
                if (newLeft - left > edgeSize * 2) findSplitPoint(query, openA, empty, newLeft - edgeSize * 2, newLeft - edgeSize);
                if (right - newRight > edgeSize * 2) findSplitPoint(query, empty, openB, newRight + edgeSize, newRight + edgeSize * 2);
                return;
            }
            if (afterA == 0 && afterB == 0) {
                std::vector<Mapping*> empty;
                if (!openA.empty()) findSplitPoint(query, openA, empty, left, start);
                if (!openB.empty()) findSplitPoint(query, empty, openB, end, right);
                return;
            }
            left = newLeft;
            right = newRight;
        }
    }

    static void updateQuery(std::vector<Mapping*>& ms, const PackedSeq* q) {
        for (Mapping* m : ms) m->Query = q;
    }
    static void appendAll(std::vector<Mapping*>& dst, const std::vector<Mapping*>& src) { dst.insert(dst.end(), src.begin(), src.end()); }
    std::vector<Mapping*> mapped(const PackedSeq& window, const PackedSeq& query) {  // performMapping, removeDominated, updateQuery
        std::vector<Mapping*> r = removeDominated(performMapping(window), nullptr, query.length);
        updateQuery(r, &query);
        return r;
    }

    // mapNext :305-383 (Go's aliasing slices as value copies, as in the oracle)
    void mapNext(const PackedSeq& query, std::vector<Mapping*>& openA, std::vector<Mapping*>& openB, std::vector<Mapping*>& newA,
                 std::vector<Mapping*>& newB, std::vector<Mapping*>& matched, bool& matchedNil) {
        std::vector<Mapping*> extended;
        bool extNil;
        const i64 e = edgeSize, L = query.length;
        if (L < e * 4) {
            newA = mapped(query.subSequence(e, L - e), query);
            matchPairs(openA, newA, extended, extNil);
            if (!extNil) {
                std::vector<Mapping*> t = newA;
                appendAll(t, extended);
                openA = t;
            } else {
                appendAll(openA, newA);
            }
            matchPairs(openA, openB, matched, matchedNil);
            newA = openA;
            newB = openB;
            if (matchedNil) return;
            newA.clear();
            newB.clear();
            return;
        }
        newA = mapped(query.subSequence(e, e * 2), query);
        matchPairs(openA, newA, extended, extNil);
        appendAll(openA, newA);
        if (!extNil) appendAll(openA, extended);
        newB = mapped(query.subSequence(L - e * 2, L - e), query);
        {
            std::vector<Mapping*> a = newB, b = openB;
            matchPairs(a, b, extended, extNil);
            openB = a;
            newB = b;
        }
        appendAll(openB, newB);
        if (!extNil) appendAll(openB, extended);
        {
            std::vector<Mapping*> a = openA, b = openB;
            matchPairs(a, b, matched, matchedNil);
            newA = a;
            newB = b;
        }
        if (!matchedNil) return;
        if (L > e * 5) {
            openA = mapped(query.subSequence(e * 2, e * 3), query);
            {
                std::vector<Mapping*> a = newA, b = openA;
                matchPairs(a, b, extended, extNil);
                openA = a;
                newA = b;
            }
            if (!extNil) appendAll(openA, extended);
            appendAll(openA, newA);
        }
        if (L > e * 6) {
            openB = mapped(query.subSequence(L - e * 3, L - e * 2), query);
            {
                std::vector<Mapping*> a = openB, b = newB;
                matchPairs(a, b, extended, extNil);
                openB = a;
                newB = b;
            }
            if (!extNil) appendAll(openB, extended);
            appendAll(openB, newB);
        } else {
            openB = newB;
        }
        if (L > e * 5) {
            std::vector<Mapping*> a = openA, b = openB;
            matchPairs(a, b, matched, matchedNil);
            newA = a;
            newB = b;
        }
    }

    std::vector<Mapping*> map(const PackedSeq& query) {  // :430-487
        std::vector<Mapping*> results;
        if (query.length <= edgeSize * 2) return mapped(query, query);
        std::vector<Mapping*> openA = performMapping(query.subSequence(0, edgeSize));
        std::vector<Mapping*> openB = performMapping(query.subSequence(query.length - edgeSize, query.length));
        openA = removeDominated(openA, nullptr, query.length);
        openB = removeDominated(openB, nullptr, query.length);
        updateQuery(openA, &query);
        updateQuery(openB, &query);
        std::vector<Mapping*> matched;
        bool matchedNil;
        matchPairs(openA, openB, matched, matchedNil);
        if (!matchedNil) return matched;
        if (query.length < edgeSize * 3) {
            results = openA;
            appendAll(results, openB);
            return results;
        }
        std::vector<Mapping*> nA, nB;
        mapNext(query, openA, openB, nA, nB, matched, matchedNil);
        openA = nA;
        openB = nB;
        if (!matchedNil) return matched;
        i64 left = edgeSize * 2, right = query.length - edgeSize * 2;
        for (Mapping* a : openA)
            if (a->QueryInset > left) left = a->QueryInset;
        left = query.length - right;  // sic (:461)
        for (Mapping* b : openB)
            if (b->QueryOffset < right) right = b->QueryOffset;
        findSplitPoint(query, openA, openB, left, right);
        const i64 size = query.length - edgeSize;
        for (i64 i = (i64)openA.size() - 1; i >= 0; i--)
            if (openA[(size_t)i]->QueryInset >= size) {
                openA[(size_t)i] = openA.back();
                openA.pop_back();
            }
        for (i64 i = (i64)openB.size() - 1; i >= 0; i--)
            if (openB[(size_t)i]->QueryOffset >= size) {
                openB[(size_t)i] = openB.back();
                openB.pop_back();
            }
        results = openA;
        appendAll(results, openB);
        return results;
    }

    // performMapping :489-611; one strand of it (s = 0 forward, 1 reverse complement)
    void strand(int s, SeedSequence* q, const std::vector<u64>& candidates, IntSet& seedSet, i64& minOwn, i64* minOther, std::vector<Mapping*>& results) {
        const int k = index.seedSize;
        for (u64 idx : candidates) {
            const IntSet& matchSet = index.seedSets[(size_t)idx];
            if (matchSet.countIntersectionTo(seedSet, minOwn) < (u64)minOwn) continue;
            SeedSequence* match = index.sequences[(size_t)idx];
            const int c = chunkRef[(size_t)idx];
            const i64 refLen = lenOf(mutation == 2 ? 0 : c);  // [4]
            std::vector<SeedMatch> seedMatches = ssMatch(index.arena, match, q, &seedSet, &matchSet, minOwn, k);
            for (auto& sm : seedMatches) {
                i64 start = match->offset + match->getSeedOffset(sm.MatchB[0], k);
                const i64 end = refLen - match->inset - match->getSeedOffsetFromEnd(sm.MatchB.back(), k);
                if (circular && start > refLen) start -= refLen;
                i64 first = q->getSeedOffset(sm.MatchA[0], k), last = q->getSeedOffsetFromEnd(sm.MatchA.back(), k);
                if (first + last > (q->length * 2) / 3) continue;
                first += q->offset;
                last += q->inset;
                i64 ca, ids;
                if (!smGetBasesCovered(sm, k, &ca, &ids)) throw std::runtime_error("model: performMapping GetBasesCovered (reference would panic)");
                MM* mp = mk();
                mp->Start = start;
                mp->End = end;
                mp->QueryOffset = s == 0 ? first : last;  // (offsets and insets of the reverse-complement query are swapped, :569-580)
                mp->QueryInset = s == 0 ? last : first;
                mp->RC = s == 1;
                mp->ids = ids;
                mp->ref = c;
                results.push_back(mp);
                const i64 limit = ((i64)sm.MatchA.size() * 4) / 5;
                if (limit > minOwn) minOwn = limit;
                if (minOther && limit > *minOther) *minOther = limit;
            }
        }
    }
    std::vector<Mapping*> performMapping(const PackedSeq& query) {
        SeedSequence* seedQuery = index.newSeedSequence(query);
        SeedSequence* rcQuery = index.newSeedSequence(query.reverseComplement());
        i64 minMatches = std::max<i64>(5, seedQuery->numSeeds() / 5), minRCMatches = std::max<i64>(5, rcQuery->numSeeds() / 5);
        const std::vector<u64> fwd = index.matches(seedQuery, 0.25), rc = index.matches(rcQuery, 0.25);
        std::vector<Mapping*> results;
        i64 maxSeed = 0;
        for (i64 i = 0; i < seedQuery->numSeeds(); i++) maxSeed = std::max(maxSeed, seedQuery->getSeed(i));
        IntSet seedSet(maxSeed + 1);
        for (i64 i = 0; i < seedQuery->numSeeds(); i++) seedSet.add((u64)seedQuery->getSeed(i));
        strand(0, seedQuery, fwd, seedSet, minMatches, &minRCMatches, results);
        seedSet.clear();
        for (i64 i = 0; i < rcQuery->numSeeds(); i++) seedSet.add((u64)rcQuery->getSeed(i));
        strand(1, rcQuery, rc, seedSet, minRCMatches, nullptr, results);
        if (results.size() > 1) {  // [4]
            goSort(results, [](Mapping* a, Mapping* b) { return refOf(a) != refOf(b) ? refOf(a) < refOf(b) : a->Start < b->Start; });
            for (i64 i = (i64)results.size() - 1; i > 0; i--) {
                Mapping* ra = results[(size_t)(i - 1)];
                Mapping* rb = results[(size_t)i];
                if (refOf(ra) == refOf(rb) && ra->RC == rb->RC && rb->Start < ra->End) {
                    if (ra->End - ra->Start > rb->End - rb->Start) {
                        results[(size_t)i] = results.back();
                        results.pop_back();
                    } else {
                        results[(size_t)(i - 1)] = results[(size_t)i];
                        results[(size_t)i] = results.back();
                        results.pop_back();
                    }
                }
            }
        }
        return results;
    }
};

struct Result {
    std::string paf, err, error;
};

// params: circular, k, query_size, min_length (unused: the read set is loaded with it), chunk_size, seed_rate, all_sequences, mutation
void run(FastaSet& refSet, FastaSet& reads, const int64_t* p, Result& res) {
    if (refSet.size() == 0) throw std::runtime_error("model: empty reference");
    const int k = (int)p[1];
    std::vector<u64> counts = kmerOccurrences(refSet.cached, k);  // [1]
    std::vector<double> values = kmerValues(counts, k);
    res.err += "K-mer counting complete. Preparing to start indexing and querying...\n";
    std::vector<PackedSeq> refs(refSet.cached.begin(), p[6] ? refSet.cached.end() : refSet.cached.begin() + 1);
    MultiMapper mapper(refs, p[0] != 0, k, values.data(), p[5], p[2], p[4], (int)p[7]);
    res.err += mapper.notes;
    i64 unmapped = 0, mapped = 0, multiple = 0, total = 0;
    const size_t arenaBase = mapper.index.arena.seqs.size();
    for (size_t id = 0; id < reads.size(); id++) {  // [7]
        const PackedSeq& q = reads.cached[id];
        std::vector<Mapping*> maps;
        if (!mapper.chunkRef.empty()) maps = mapper.map(q);
        for (Mapping* m : maps) res.paf += mapper.asString(*m) + "\n";
        if (maps.size() == 1) mapped++;
        else if (maps.size() > 1) multiple++;
        else unmapped++;
        total += (i64)maps.size();
        mapper.index.arena.seqs.resize(arenaBase);
        mapper.pool.clear();
    }
    char line[160];
    snprintf(line, sizeof line, "Uniquely mapped: %lld\nMultiple mappings: %lld\ntotal: %lld\nUnmapped: %lld\n", (long long)mapped,
             (long long)multiple, (long long)total, (long long)unmapped);
    res.err += line;
}

FastaSet fromArrays(const char* bases, const int64_t* off, int64_t n, int64_t minLen) {
    std::vector<std::string> names, seqs;
    char nm[32];
    for (int64_t i = 0; i < n; i++) {
        snprintf(nm, sizeof nm, "r%07lld", (long long)i);
        names.push_back(nm);
        seqs.emplace_back(bases + off[i], (size_t)(off[i + 1] - off[i]));
    }
    return FastaSet::fromReads(names, seqs, minLen, false);
}

}  // namespace

extern "C" {
void* mmm_run(const char* refBases, const int64_t* refOff, int64_t nRef, const char* readBases, const int64_t* readOff, int64_t nReads,
              const int64_t* params) {
    Result* r = new Result();
    try {
        FastaSet ref = fromArrays(refBases, refOff, nRef, 0), reads = fromArrays(readBases, readOff, nReads, params[3]);
        run(ref, reads, params, *r);
    } catch (const std::exception& e) {
        r->error = e.what();
    }
    return r;
}
void* mmm_run_files(const char* refPath, const char* readsPath, const int64_t* params) {
    Result* r = new Result();
    try {
        FastaSet ref = FastaSet::fromFile(refPath, 0, false), reads = FastaSet::fromFile(readsPath, params[3], false);
        if (!ref.error.empty() || !reads.error.empty()) throw std::runtime_error(ref.error + reads.error);
        run(ref, reads, params, *r);
    } catch (const std::exception& e) {
        r->error = e.what();
    }
    return r;
}
void mmm_free(void* h) { delete (Result*)h; }
const char* mmm_text(void* h, int which, int64_t* n) {
    Result* r = (Result*)h;
    const std::string& s = which == 0 ? r->paf : which == 1 ? r->err : r->error;
    *n = (int64_t)s.size();
    return s.data();
}
}
