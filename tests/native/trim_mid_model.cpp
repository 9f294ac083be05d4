// TEST INFRASTRUCTURE ONLY: the checker of `trim`'s middle-adapter stage.  A line-by-line C++ restatement of the second half of
// Trimmer.Trim (trim/trim.go:151-256) and of findSplit (:515-591) on the oracle's own types (PackedSeq::subSequence,
// SeedIndex::newSeedSequence / addSequence / indexSequences / matches, ssMatch, smGetBasesCovered, IntSet), together with the parts of
// sequence/seqio.go the stage leans on (the re-read of trimmed reads :138-187, GetSequencesByID :302-323, AddSequence :396-399,
// sendExtras :81-104, the writers :401-435, Demultiplex :460-523).  It chains after the edge model, whose translation unit it includes
// unchanged, and shares no source with downpore_amd/csrc/host/host_trim.cpp or dp_trim.hip.
//
// Canonical semantics: one worker; front adapters in list order, each to completion; within an adapter the chunks in
// the order Matches returns them; within a pair the matches in Match's return order.  himem = false.  Deliberate differences from the
// reference: chunk_size <= 100 is refused (its chunk loop never ends); the `continue` of :536 that leaves the lock held is not
// restated (its condition cannot occur); a right half whose bStart is negative - SubSequence would slice out of range - is skipped,
// counted and named in one log line.
//
// mutation (hand cases only): 1 = the `<` of :543 becomes `<=`; 2 = the `- frontTrim` of :579 is dropped.
#include "trim_model.cpp"

namespace {

struct MidParams {
    i64 chunkSize = 5000;
    int midThreshold = 85, extraMidTrim = 100;
    bool keepSplits = true;
    i64 flushSeeds = 300000000;
    int mutation = 0;
};

struct SequenceSplit {  // trim.go:42-46
    i64 id, aEnd, bStart;
};

struct MidRec {  // one applied match
    int32_t adapter, chunk, ordinal, startRel, covered, chainLen;
};

struct Extra {
    std::string name, text;  // the record as the writer prints it, without its name line
};

struct MidModel {
    Model* m = nullptr;
    MidParams p;
    std::string error;
    std::vector<int32_t> plan;        // per planned chunk: read, start, end, remainder, seeds, indexed
    std::vector<i64> chunkOfIndex;    // index position of the current batch -> planned chunk
    std::vector<int32_t> segs, segOff;
    std::vector<MidRec> recs;
    std::vector<int32_t> splitsOut;   // per entry of ids with a live split: read, aEnd, bStart, kept (bit 0 left, bit 1 right)
    std::vector<Extra> extras;
    std::vector<PackedSeq> served;    // what the second GetSequences() serves, per read (length 0: ignored then)
    std::vector<std::unique_ptr<SequenceSplit>> splits;
    std::vector<i64> ids;
    i64 batches = 0, outOfRange = 0, candidatePairs = 0, indexedChunks = 0;
    std::vector<int32_t> ints;
    std::string out;
    // the matching stage's results supplied by the caller (hand cases): per planned chunk its seed count, and the matches that pass
    // the identity test, in canonical order
    const int32_t* seedCountsIn = nullptr;
    const MidRec* recsIn = nullptr;
    int64_t nRecsIn = 0;
    std::vector<SeedSequence*> chunkSeq;  // planned chunk -> its seed sequence while its batch is open
    std::vector<int32_t> candidates;      // (front adapter, planned chunk) per candidate pair, in the order searched
};

// what GetSequences serves once trims are set (seqio.go:149-186): the trimmed stretch re-read as a top-level sequence with the same
// stretch of the quality line
PackedSeq reread(const Model& m, size_t r) {
    const PackedSeq& c = m.reads.cached[r];
    const i64 ft = m.frontTrim[r], n = c.length - m.frontTrim[r] - m.backTrim[r];
    PackedSeq seq = newPackedSequence((i64)r, c.str().substr((size_t)ft, (size_t)n), nullptr);
    if (m.reads.isFastq && c.qual) {
        seq.qual = std::make_shared<std::vector<uint8_t>>(c.qual->begin() + (long)(c.qlo + (size_t)ft), c.qual->begin() + (long)(c.qlo + (size_t)(ft + n)));
        seq.qlo = 0;
    }
    return seq;
}

std::string bodyText(const Model& m, const PackedSeq& s) {  // fastaWriter / fastqWriter (:401-435) after the name line
    if (!m.reads.isFastq) return s.str() + "\n";
    std::string q;
    if (s.qual)
        for (i64 j = 0; j < s.length; j++) q += (char)(uint8_t)((*s.qual)[s.qlo + (size_t)j] + 33);
    return s.str() + "\n+\n" + q + "\n";
}

// the body of findSplit's loop over the matches (trim.go:527-586) for one match of front adapter ai in `target`
void applyMatch(MidModel& mm, size_t ai, SeedSequence* target, i64 planChunk, int32_t ordinal, i64 startRel, i64 identity, i64 chainLen) {
    Trimmer& t = mm.m->t;
    Model& m = *mm.m;
    SeedSequence* ad = t.frontAdapters[ai];
    const i64 minSeqLength = 500;
    {
        {
            if ((identity * 100) / ad->length < mm.p.midThreshold) return;  // :528
            const i64 id = target->id;                                      // :533
            const i64 frontTrim = m.frontTrim[(size_t)id];                  // :538
            const i64 backTrim = m.backTrim[(size_t)id];                    // :539
            const i64 start = target->offset + startRel;                    // :541
            const i64 seqLen = target->offset + target->length + target->inset - backTrim;  // :542
            mm.recs.push_back(MidRec{(int32_t)ai, (int32_t)planChunk, ordinal, (int32_t)startRel, (int32_t)identity, (int32_t)chainLen});
            std::unique_ptr<SequenceSplit>& split = mm.splits[(size_t)id];
            if (mm.p.mutation == 1 ? start <= minSeqLength + frontTrim : start < minSeqLength + frontTrim) {  // :543 just crop the front off
                const i64 newTrim = start + ad->length + mm.p.extraMidTrim;  // :544
                if (newTrim + minSeqLength < seqLen) {
                    if (newTrim > frontTrim) {
                        m.frontTrim[(size_t)id] = newTrim;  // SetFrontTrim :547
                        if (split) {                        // :548-551
                            split->aEnd -= (newTrim - frontTrim);
                            split->bStart -= (newTrim - frontTrim);
                        }
                    }
                    if (t.p.tagAdapters) m.reads.names[(size_t)id] = *ad->name + "_" + m.reads.names[(size_t)id];  // :553-555
                } else {
                    split.reset();                   // :557
                    m.reads.ignore[(size_t)id] = 1;  // :558
                }
            } else if (start + minSeqLength + ad->length > seqLen) {  // :560 crop off the tail
                const i64 newTrim = seqLen - start + mm.p.extraMidTrim;
                if (newTrim > backTrim) m.backTrim[(size_t)id] = newTrim;
            } else {
                if (split) {  // :568-574
                    if (split->aEnd > start - mm.p.extraMidTrim - frontTrim) split->aEnd = start - mm.p.extraMidTrim - frontTrim;
                    if (split->bStart < start + ad->length + mm.p.extraMidTrim - frontTrim) split->bStart = start + ad->length + mm.p.extraMidTrim - frontTrim;
                } else {  // :579-583
                    const i64 ft = mm.p.mutation == 2 ? 0 : frontTrim;
                    split.reset(new SequenceSplit{id, start - mm.p.extraMidTrim - ft, start + ad->length + mm.p.extraMidTrim - ft});
                    mm.ids.push_back(id);
                }
            }
        }
    }
}

// findSplit (trim.go:515-591) for front adapter ai over the current index
void findSplit(MidModel& mm, size_t ai) {
    Trimmer& t = mm.m->t;
    SeedSequence* ad = t.frontAdapters[ai];
    if (mm.recsIn) {  // the caller's matches of this adapter in the chunks of the open batch, in the order given
        for (int64_t x = 0; x < mm.nRecsIn; x++) {
            const MidRec& r = mm.recsIn[x];
            if ((size_t)r.adapter != ai || r.chunk < 0 || (size_t)r.chunk >= mm.chunkSeq.size() || !mm.chunkSeq[(size_t)r.chunk]) continue;
            applyMatch(mm, ai, mm.chunkSeq[(size_t)r.chunk], r.chunk, r.ordinal, r.startRel, r.covered, r.chainLen);
        }
        return;
    }
    const IntSet* adSet = &t.frontAdapterSets[ai];
    const i64 minMatch = ad->numSeeds() / 5;                           // :519
    const std::vector<u64> ms = t.index->matches(ad, 0.2);             // :520
    mm.candidatePairs += (i64)ms.size();
    for (u64 index : ms) {
        mm.candidates.push_back((int32_t)ai);
        mm.candidates.push_back((int32_t)mm.chunkOfIndex[(size_t)index]);
        SeedSequence* target = t.index->sequences[(size_t)index];     // :522
        const IntSet* targetSet = &t.index->seedSets[(size_t)index];  // :523
        std::vector<SeedMatch> matches = ssMatch(t.index->arena, target, ad, adSet, targetSet, minMatch, t.p.k);  // :524
        int32_t ordinal = -1;
        for (const SeedMatch& match : matches) {
            ordinal++;
            i64 identity = 0, b = 0;
            smGetBasesCovered(match, t.p.k, &identity, &b);  // :527
            applyMatch(mm, ai, target, mm.chunkOfIndex[(size_t)index], ordinal,
                       target->getSeedOffset(match.MatchB[0], t.p.k) - ad->getSeedOffset(match.MatchA[0], t.p.k), identity, (i64)match.MatchA.size());
        }
    }
}

void searchBatch(MidModel& mm, i64 totalBases) {  // :187-198 / :207-216
    Trimmer& t = mm.m->t;
    t.index->indexSequences();
    mm.batches++;
    if (t.p.verbosity > 0)
        t.log("Searching " + std::to_string(totalBases / 1000000) + " MB of sequences for splitting based on " + std::to_string(t.frontAdapters.size()) + " adapters");
    for (size_t i = 0; i < t.frontAdapters.size(); i++) findSplit(mm, i);
}

// the second half of Trim (trim.go:151-256)
void trimMiddle(MidModel& mm) {
    Model& m = *mm.m;
    Trimmer& t = m.t;
    const size_t n = m.reads.size();
    const i64 longestAdapter = 100, edgeSize = 150, minSeeds = 4;  // :153-155
    i64 totalCount = 0, totalBases = 0;
    mm.splits.clear();
    mm.splits.resize(n + 1);  // :159
    mm.served.assign(n, PackedSeq());
    for (size_t r = 0; r < n; r++) {  // ss = seqs.GetSequences() :152
        if (m.reads.ignore[r]) continue;
        mm.served[r] = reread(m, r);
        const PackedSeq& seq = mm.served[r];
        totalBases += seq.length - edgeSize * 2;  // :164
        for (i64 i = edgeSize; i < seq.length - edgeSize - longestAdapter; i += mm.p.chunkSize - longestAdapter) {  // :165
            bool remainder = false;
            i64 endPoint;
            if (i > seq.length - (mm.p.chunkSize * 3) / 2 - edgeSize) {  // :166 add the entire remainder
                remainder = true;
                endPoint = seq.length - edgeSize;
            } else {  // :173-177
                endPoint = i + mm.p.chunkSize;
                if (endPoint >= seq.length - edgeSize) endPoint = seq.length - edgeSize;
            }
            SeedSequence* seedSeq = t.index->newSeedSequence(seq.subSequence(i, endPoint));
            const i64 numSeeds = mm.seedCountsIn ? mm.seedCountsIn[mm.plan.size() / 6] : seedSeq->numSeeds();
            totalCount += numSeeds;
            const bool indexed = remainder || numSeeds >= minSeeds;  // :170 / :180-182
            mm.chunkSeq.push_back(indexed ? seedSeq : nullptr);
            if (indexed) {
                mm.chunkOfIndex.push_back((i64)mm.plan.size() / 6);
                t.index->addSequence(seedSeq);
                mm.indexedChunks++;
            }
            mm.plan.insert(mm.plan.end(), {(int32_t)r, (int32_t)i, (int32_t)endPoint, remainder ? 1 : 0, (int32_t)numSeeds, indexed ? 1 : 0});
            mm.segOff.push_back((int32_t)mm.segs.size());
            for (size_t x = 0; x < seedSeq->n; x++) mm.segs.push_back((int32_t)seedSeq->seg()[x]);
            if (remainder) break;  // :171
        }
        if (totalCount > mm.p.flushSeeds) {  // :186
            searchBatch(mm, totalBases);
            totalCount = 0;
            totalBases = 0;
            t.setupIndex();  // :202 (also zeroes frontCounts / backCounts)
            mm.chunkOfIndex.clear();
            std::fill(mm.chunkSeq.begin(), mm.chunkSeq.end(), nullptr);
        }
    }
    mm.segOff.push_back((int32_t)mm.segs.size());
    if (totalCount > 0) searchBatch(mm, totalBases);  // :206-217
    if (t.p.verbosity > 0) t.log(std::to_string(mm.ids.size()) + " sequences require splitting");  // :218-220
    // :222-226 GetSequencesByID: the reads of ids re-read with the trims as they stand now, whatever their ignore flag
    for (i64 id : mm.ids) {  // :227
        SequenceSplit* split = mm.splits[(size_t)id].get();
        if (!split) continue;
        const PackedSeq seq = reread(m, (size_t)id);
        int kept = 0;
        if (mm.p.keepSplits) {
            std::string report = "Splitting read " + std::to_string(split->id) + " into";  // :234
            if (split->aEnd > edgeSize) {
                mm.extras.push_back(Extra{m.reads.names[(size_t)id] + "_(left)", bodyText(m, seq.subSequence(0, split->aEnd))});  // :237
                report += ": 0 - " + std::to_string(split->aEnd) + " and ";
                kept |= 1;
            } else {
                report += " ignored short left hand side and ";
            }
            if (seq.length - split->bStart > edgeSize) {
                if (split->bStart < 0) {  // (SubSequence would slice out of range: skipped and counted)
                    mm.outOfRange++;
                    t.log("Skipping the right hand side of read " + std::to_string(split->id) + ": its start " + std::to_string(split->bStart) + " is out of range");
                    report += " out of range right hand side";
                } else {
                    mm.extras.push_back(Extra{m.reads.names[(size_t)id] + "_(right)", bodyText(m, seq.subSequence(split->bStart, seq.length))});  // :243
                    report += std::to_string(split->bStart) + " - " + std::to_string(seq.length);
                    kept |= 2;
                }
            } else {
                report += " ignored short right hand side";
            }
            if (t.p.verbosity > 1) {  // :248-253
                t.log(report);
                if (split->aEnd >= 0 && split->bStart < seq.length && split->bStart - split->aEnd - mm.p.extraMidTrim * 2 <= longestAdapter)
                    t.log(seq.subSequence(split->aEnd + mm.p.extraMidTrim, split->bStart - mm.p.extraMidTrim).str());
            }
        }
        mm.splitsOut.insert(mm.splitsOut.end(), {(int32_t)id, (int32_t)split->aEnd, (int32_t)split->bStart, kept});
        m.reads.ignore[(size_t)split->id] = 1;  // :255
    }
    for (size_t r = 0; r < n; r++) {
        m.table[5 * r] = (int32_t)m.frontTrim[r];
        m.table[5 * r + 1] = (int32_t)m.backTrim[r];
        m.table[5 * r + 2] = m.reads.ignore[r];
    }
}

void finishMid(MidModel& mm, const Rec* recsIn, const i64* countsIn) {
    Model* m = mm.m;
    trimAll(*m, recsIn, countsIn);
    trimMiddle(mm);
    printStats(*m);
    if (!m->failed) {
        writeAll(*m);  // the file's reads, then the extras in the order added (sendExtras)
        for (const Extra& e : mm.extras) m->out += (m->reads.isFastq ? "@" : ">") + e.name + "\n" + e.text;
    }
    Trimmer& t = m->t;
    for (size_t i = 0; i < t.originalFront.size(); i++) m->adapters += "F\t" + t.originalFront[i].getName() + "\t" + std::to_string(t.frontCounts[i]) + "\n";
    for (size_t i = 0; i < t.originalBack.size(); i++) m->adapters += "B\t" + t.originalBack[i].getName() + "\t" + std::to_string(t.backCounts[i]) + "\n";
}

}  // namespace

extern "C" {

// params[15] = the edge model's nine, then chunk_size, middle_threshold, extra_middle_trim, discard_middle, flush_seeds, mid mutation.
// enabled / recs / counts as tm_run_with_records takes them, or all null: the edge model computes them itself.  seedCounts (per planned
// chunk) and midRecs (six int32 per passing match, canonical order), or null: the model scans and matches itself.
void* tmm_run(const char* readsPath, const char* frontPath, const char* backPath, const int64_t* params, const uint8_t* enabled,
              const int32_t* recs, const int64_t* counts, const int32_t* seedCounts, const int32_t* midRecs, int64_t nMidRecs) {
    MidModel* mm = new MidModel();
    mm->seedCountsIn = seedCounts;
    mm->recsIn = seedCounts ? (const MidRec*)midRecs : nullptr;
    mm->nRecsIn = nMidRecs;
    mm->p.chunkSize = params[9];
    mm->p.midThreshold = (int)params[10];
    mm->p.extraMidTrim = (int)params[11];
    mm->p.keepSplits = params[12] == 0;
    mm->p.flushSeeds = params[13];
    mm->p.mutation = (int)params[14];
    mm->m = load(readsPath, frontPath, backPath, params);
    if (mm->p.chunkSize <= 100) {
        mm->error = "trim: -chunk_size must be larger than 100";
        return mm;
    }
    if (recs) {
        if (enabled) determineAdapters(*mm->m, enabled);
    } else if (mm->m->t.p.determine) {
        determineAdapters(*mm->m, nullptr);
    }
    finishMid(*mm, (const Rec*)recs, (const i64*)counts);
    return mm;
}

void tmm_free(void* h) {
    MidModel* mm = (MidModel*)h;
    delete mm->m;
    delete mm;
}
void* tmm_edge(void* h) { return ((MidModel*)h)->m; }  // the edge model's handle, for tm_text / tm_ints / tm_demultiplex... of this library
const char* tmm_error(void* h) { return ((MidModel*)h)->error.c_str(); }
int tmm_failed(void* h) { return ((MidModel*)h)->m->failed ? 1 : 0; }

// which: 0 output, 1 log lines, 2 adapters, 3 extras' names (one per line)
const char* tmm_text(void* h, int which, int64_t* n) {
    MidModel* mm = (MidModel*)h;
    if (which == 3) {
        mm->out.clear();
        for (const Extra& e : mm->extras) mm->out += e.name + "\n";
        *n = (int64_t)mm->out.size();
        return mm->out.data();
    }
    return tm_text(mm->m, which, n);
}

// which: 0 table (5 per read), 1 chunk plan (6 per chunk: read, start, end, remainder, seeds, indexed), 2 applied records (6 each:
// adapter, chunk, ordinal, start_rel, covered, chain length), 3 splits (4 each: read, aEnd, bStart, kept halves), 4 counters (batches,
// out-of-range halves, candidate pairs, indexed chunks, front adapters), 5 chunk segments, 6 their offsets, 7 edge records, 8 edge
// counts, 9 determine flags, 10 candidate pairs (front adapter, chunk)
const int32_t* tmm_ints(void* h, int which, int64_t* n) {
    MidModel* mm = (MidModel*)h;
    std::vector<int32_t>& v = mm->ints;
    v.clear();
    if (which == 0) v = mm->m->table;
    else if (which == 1) v = mm->plan;
    else if (which == 2)
        for (const MidRec& r : mm->recs) v.insert(v.end(), {r.adapter, r.chunk, r.ordinal, r.startRel, r.covered, r.chainLen});
    else if (which == 3) v = mm->splitsOut;
    else if (which == 4)
        v = {(int32_t)mm->batches, (int32_t)mm->outOfRange, (int32_t)mm->candidatePairs, (int32_t)mm->indexedChunks, (int32_t)mm->m->t.frontAdapters.size()};
    else if (which == 5) v = mm->segs;
    else if (which == 6) v = mm->segOff;
    else if (which == 7) return tm_ints(mm->m, 1, n);
    else if (which == 8) return tm_ints(mm->m, 2, n);
    else if (which == 9) return tm_ints(mm->m, 3, n);
    else if (which == 10) v = mm->candidates;
    *n = (int64_t)v.size();
    return v.data();
}

// the chunk loop of trim.go:165-184 for one trimmed length: out[3 * i ..] = start, end, remainder; returns the number of chunks
int64_t tmm_chunk_plan(int64_t length, int64_t chunkSize, int32_t* out, int64_t cap) {
    const i64 longestAdapter = 100, edgeSize = 150;
    int64_t count = 0;
    for (i64 i = edgeSize; i < length - edgeSize - longestAdapter; i += chunkSize - longestAdapter) {
        i64 endPoint;
        bool remainder = false;
        if (i > length - (chunkSize * 3) / 2 - edgeSize) {
            endPoint = length - edgeSize;
            remainder = true;
        } else {
            endPoint = i + chunkSize;
            if (endPoint >= length - edgeSize) endPoint = length - edgeSize;
        }
        if (count < cap) {
            out[3 * count] = (int32_t)i;
            out[3 * count + 1] = (int32_t)endPoint;
            out[3 * count + 2] = remainder ? 1 : 0;
        }
        count++;
        if (remainder) break;
    }
    return count;
}

// Demultiplex (seqio.go:460-523) into dir, the extras after the file's reads; returns the number of files
int tmm_demultiplex(void* h, const char* dir) {
    MidModel* mm = (MidModel*)h;
    Model* m = mm->m;
    std::map<std::string, std::string> partitions;
    std::vector<std::string> order;
    const char* ext = m->reads.isFastq ? ".fastq" : ".fasta";
    auto send = [&](const std::string& n, const std::string& body) {
        if (!hasPrefix(n, "Barcode")) return;
        const size_t pos = n.find('_');
        if (pos == std::string::npos) return;
        const std::string label = n.substr(0, pos);
        if (!partitions.count(label)) order.push_back(label);
        partitions[label] += (m->reads.isFastq ? "@" : ">") + n.substr(pos + 1) + "\n" + body;
    };
    for (size_t r = 0; r < m->reads.size(); r++)
        if (!m->reads.ignore[r]) send(m->reads.names[r], bodyText(*m, reread(*m, r)));
    for (const Extra& e : mm->extras) send(e.name, e.text);
    for (const std::string& label : order) {
        std::ofstream f(std::string(dir) + "/" + label + ext, std::ios::binary | std::ios::trunc);
        f << partitions[label];
    }
    return (int)order.size();
}
}
