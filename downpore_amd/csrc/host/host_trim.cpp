// trim.Trimmer, edge stage (trim/trim.go:13-132, 259-513; commands/trim.go:32-50): adapter determination, end trimming, tagging,
// pairing, stats, the trimmed FASTA / FASTQ writer and demultiplexing (sequence/seqio.go:375-523).  The matching itself - findMatches
// and isNewFullMatch for every read end - runs on the device (dp_trim_edges); what stays here is the sequential logic around it.
// The middle stage (Trim's second half and findSplit, :151-257, :515-591): the chunk plan, the flush batches, findSplit's rules over
// the matches a matching stage reports, the halves of split reads (AddSequence, sendExtras: seqio.go:81-104, 396-399).
//
// Canonical semantics where the reference depends on goroutine scheduling: one worker, so reads are judged and written in file order;
// in the middle stage front adapters in list order, each to completion, within an adapter the chunks in ascending index order, within
// a pair the matches in Match's return order.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "host_util.hpp"
#include "map_plan.hpp"

namespace dph {

namespace {
const int kEdgeSize = 150;        // edgeSize: the bases of a read end that are searched (trim.go:432,453)
const int kMinEdgeLength = 200;   // a shorter read keeps its ends (:434 / :455)
const i64 kLongestAdapter = 100;  // longestAdapter (:153)
const i64 kMinSeeds = 4;          // minSeeds: a chunk with fewer is not indexed (:155)
const i64 kMinSeqLength = 500;    // minSeqLength of findSplit (:517)

void logLine(std::string& err, const std::string& s) {  // log.Println without the timestamp (the CLI adds it)
    err += s;
    err += '\n';
}
bool isBarcodeName(const std::string& n) { return n.compare(0, 7, "Barcode") == 0; }  // strings.HasPrefix(name, "Barcode") :377

// a ReadSet holding the chosen adapters of another one, in the given order
ReadSet pickAdapters(const ReadSet& src, const std::vector<size_t>& order) {
    ReadSet out;
    out.off.push_back(0);
    for (size_t i : order) {
        out.names.push_back(src.names[i]);
        out.bases.append(src.seq(i), (size_t)src.length(i));
        out.off.push_back((i64)out.bases.size());
        out.ignore.push_back(0);
    }
    return out;
}

// DetermineAdapters' report and compaction for one side (trim.go:285-303 / :304-322): walking backwards, an adapter without a good
// match is overwritten by the list's last element, which reorders the survivors
std::vector<size_t> compactAdapters(const ReadSet& set, const uint8_t* enabled, const char* side, int verbosity, std::string& errText) {
    const size_t n = set.size();
    size_t count = 0;
    for (size_t i = 0; i < n; i++) count += enabled[i] ? 1 : 0;
    if (verbosity > 0)
        logLine(errText, std::to_string(count) + " / " + std::to_string(n) + " " + side + " adapters identified with high identity matches.");
    std::vector<size_t> order(n);
    for (size_t i = 0; i < n; i++) order[i] = i;
    for (size_t i = n; i-- > 0;) {
        if (enabled[i]) {
            if (verbosity > 0) logLine(errText, " - " + set.names[order[i]]);
        } else {
            order[i] = order.back();
            order.pop_back();
        }
    }
    return order;
}

struct EdgeBatch {
    std::vector<uint32_t> reads;  // eligible reads (>= 200 bases, :434 / :455), in read order
    std::vector<uint8_t> ends;    // 2 x 150 ASCII bases per eligible read
};
void eligibleReads(const ReadSet& reads, size_t lo, size_t hi, std::vector<uint32_t>& out) {
    out.clear();
    for (size_t r = lo; r < hi; r++)
        if (reads.length(r) >= kMinEdgeLength) out.push_back((uint32_t)r);
}
void extractEnds(const ReadSet& reads, size_t lo, size_t hi, EdgeBatch& b) {
    eligibleReads(reads, lo, hi, b.reads);
    b.ends.resize(b.reads.size() * 2 * kEdgeSize);
    for (size_t i = 0; i < b.reads.size(); i++) {
        const size_t r = b.reads[i];
        memcpy(b.ends.data() + i * 2 * kEdgeSize, reads.seq(r), kEdgeSize);
        memcpy(b.ends.data() + i * 2 * kEdgeSize + kEdgeSize, reads.seq(r) + reads.length(r) - kEdgeSize, kEdgeSize);
    }
}

// One edge call over the reads [lo, hi): their ends extracted here and sent, or - with `resident`, a context that holds `reads` - spelled on
// the device from the packed reads, the eligible reads' ids being all that goes up.  `up` receives the bytes sent.
int edgeCall(dp_trim* h, dp_ctx* resident, uint32_t base, const ReadSet& reads, size_t lo, size_t hi, EdgeBatch& b, int mode, int minMatch, int threshold,
             dp_trim_rec* recs, uint64_t* counts, uint8_t* enabled, double* tms, double* up) {
    if (resident) {
        *up = 4.0 * (double)b.reads.size();
        if (base) {  // (the context holds host read r as device read base + r)
            const std::vector<uint32_t> ids = mapTailIds(b.reads, base);
            return dp_trim_edges_resident(h, resident, ids.data(), (uint32_t)ids.size(), mode, minMatch, threshold, recs, counts, enabled, tms);
        }
        return dp_trim_edges_resident(h, resident, b.reads.data(), (uint32_t)b.reads.size(), mode, minMatch, threshold, recs, counts, enabled, tms);
    }
    *up = (double)b.ends.size();
    return dp_trim_edges(h, b.ends.data(), (uint32_t)b.reads.size(), mode, minMatch, threshold, recs, counts, enabled, tms);
}
// the batch of reads [lo, hi): with `resident` only the list of the eligible ones
void edgeBatch(const ReadSet& reads, size_t lo, size_t hi, bool resident, EdgeBatch& b) {
    if (resident) eligibleReads(reads, lo, hi, b.reads);
    else extractEnds(reads, lo, hi, b);
}

// trimWorker's arithmetic on the device's records (trim.go:464-510): frontTrim / backTrim / ignore of the reads, their names after
// tagging, seen / none, the table's adapter columns, and the adapters with their counts
bool applyEdgeRecords(ReadSet& reads, const ReadSet& front, const ReadSet& back, const TrimIndex& ix, const TrimParams& p, const std::vector<uint32_t>& eligible,
                      const dp_trim_rec* recs, const uint64_t* counts, TrimResult& res, std::string& error) {
    const size_t n = reads.size();
    reads.frontTrim.assign(n, 0);
    reads.backTrim.assign(n, 0);
    std::fill(reads.ignore.begin(), reads.ignore.end(), 0);
    res.names = reads.names;
    res.table.assign(n * 5, 0);
    for (size_t r = 0; r < n; r++) res.table[5 * r + 3] = res.table[5 * r + 4] = -1;
    res.seen = res.none = 0;
    for (size_t i = 0; i < eligible.size(); i++) {
        const size_t r = eligible[i];
        const dp_trim_rec& f = recs[2 * i];
        const dp_trim_rec& b = recs[2 * i + 1];
        // findMatches' return (:423-427): an ambiguous barcode trims, but pretends no adapter was seen
        int start = f.latest, matchIndex = f.ambiguous ? 0 : f.best_match;
        bool foundStart = !f.ambiguous && f.found;
        int end = b.earliest, backMatchIndex = b.ambiguous ? 0 : b.best_match;
        bool foundEnd = !b.ambiguous && b.found;
        if ((foundStart && (matchIndex < 0 || (size_t)matchIndex >= front.size())) || (foundEnd && (backMatchIndex < 0 || (size_t)backMatchIndex >= back.size()))) {
            error = "trim: an edge record names an adapter beyond the list";
            return false;
        }
        if (p.requirePairs) {  // :471-485
            const int fp = foundStart ? ix.pairs[matchIndex] : -1;
            const int bp = foundEnd ? ix.pairs[front.size() + backMatchIndex] : -1;
            if (fp != bp) foundStart = foundEnd = false;
        }
        res.seen++;
        if (!foundStart) res.none++;
        const i64 len = reads.length(r);
        start += p.extraEdgeTrim;
        end = kEdgeSize - end + p.extraEdgeTrim;
        if ((i64)start + end + 10 >= len) {  // :495
            reads.ignore[r] = 1;
        } else {
            if (foundStart) {
                reads.frontTrim[r] = start;
                if (p.tagAdapters) res.names[r] = front.names[matchIndex] + "_" + res.names[r];
            } else if (end > start && start > 0) {
                reads.frontTrim[r] = start;  // trim off ambiguous adapters too
            }
            if (foundEnd || (end > start && end < len)) reads.backTrim[r] = end;
        }
        res.table[5 * r + 3] = foundStart ? matchIndex : -1;
        res.table[5 * r + 4] = foundEnd ? backMatchIndex : -1;
    }
    res.frontNames = front.names;
    res.backNames = back.names;
    res.counts.assign(counts, counts + front.size() + back.size());
    return true;
}

// the table's trim columns, from the reads as the stages left them
void fillTable(const ReadSet& reads, TrimResult& res) {
    for (size_t r = 0; r < reads.size(); r++) {
        res.table[5 * r] = reads.frontTrim[r];
        res.table[5 * r + 1] = reads.backTrim[r];
        res.table[5 * r + 2] = reads.ignore[r];
    }
}

// a half of a split read as the writers print it (seqio.go:401-435): extras follow the file's reads in the order added (sendExtras)
void writeExtras(const ReadSet& reads, const TrimResult& res, const std::vector<std::string>& names, const std::vector<uint8_t>* keep, std::string& out) {
    for (size_t e = 0; e < res.extraNames.size(); e++) {
        if (keep && !(*keep)[e]) continue;
        out += reads.isFastq ? '@' : '>';
        out += names[e];
        out += '\n';
        out += res.extraBases[e];
        out += '\n';
        if (reads.isFastq) {
            out += "+\n";
            out += res.extraQuals[e];
            out += '\n';
        }
    }
}

// PrintStats (trim.go:260-268) and Write (seqio.go:401-458)
int reportAndWrite(const ReadSet& reads, const ReadSet& front, const ReadSet& back, TrimResult& res, std::string& error, bool write = true) {
    // PrintStats: with seenCount == 0 the reference divides by zero
    if (res.seen == 0) {
        logLine(res.errText, "no reads long enough to trim");
        error = "trim: no reads long enough to trim (the ends are searched in reads of 200 bases and more)";
        return -2;
    }
    for (size_t i = 0; i < front.size(); i++)
        logLine(res.errText, "Front adapter: " + front.names[i] + " \t " + std::to_string((i64)(res.counts[i] * 100) / res.seen) + " %");
    for (size_t i = 0; i < back.size(); i++)
        logLine(res.errText, "Back adapter: " + back.names[i] + " \t " + std::to_string((i64)(res.counts[front.size() + i] * 100) / res.seen) + " %");
    logLine(res.errText, std::to_string((res.none * 100) / res.seen) + " % with no adapters found.");
    res.out.clear();
    if (!write) return 0;  // (the reads stay on the device: trimmedReadSet)
    logLine(res.errText, "Writing trimmed sequences...");  // commands/trim.go:44
    const double t1 = now();
    trimWrite(reads, res.names, nullptr, res.out);
    writeExtras(reads, res, res.extraNames, nullptr, res.out);
    res.t_write = now() - t1;
    return 0;
}

// ---- the middle stage -----------------------------------------------------------------------------------------------------------
struct MidSplit {  // sequenceSplit (trim.go:42-46); live = the pointer is not nil
    bool live = false;
    i64 aEnd = 0, bStart = 0;
};

struct MidBatchRange {
    size_t lo, hi;  // planned chunks [lo, hi)
    i64 totalBases;
};
struct MidPlan {
    std::vector<TrimChunk> plan;
    std::vector<i64> servedLen;       // -1: the read was ignored when the second pass began
    std::vector<size_t> firstChunk;   // [reads + 1]
    std::vector<MidBatchRange> batches;
};
const uint32_t kNoBatch = 0xffffffffu;

// the plan over what the second GetSequences() serves: the non-ignored reads with their edge trims applied (seqio.go:138-187)
bool midBuildPlan(const ReadSet& reads, const TrimParams& p, MidPlan& mp, std::string& error) {
    if (p.chunkSize <= kLongestAdapter) {
        error = "trim: -chunk_size must be larger than 100 (the chunks advance by chunk_size - 100 bases)";
        return false;
    }
    const size_t n = reads.size();
    mp.servedLen.assign(n, -1);
    mp.firstChunk.assign(n + 1, 0);
    for (size_t r = 0; r < n; r++) {
        mp.firstChunk[r] = mp.plan.size();
        if (reads.ignore[r]) continue;
        mp.servedLen[r] = reads.length(r) - reads.frontTrim[r] - reads.backTrim[r];
        trimChunkPlan(mp.servedLen[r], p.chunkSize, (uint32_t)r, mp.plan);
    }
    mp.firstChunk[n] = mp.plan.size();
    return true;
}
// the flush batches (:186-203, :206): a batch ends after the READ that takes totalCount over the threshold; returns "a flush happened"
bool midCutBatches(const TrimParams& p, const int32_t* seedCounts, MidPlan& mp) {
    bool flushed = false;
    i64 totalCount = 0, totalBases = 0;
    size_t lo = 0;
    mp.batches.clear();
    for (size_t r = 0; r + 1 < mp.firstChunk.size(); r++) {
        if (mp.servedLen[r] < 0) continue;
        totalBases += mp.servedLen[r] - kEdgeSize * 2;  // :164
        for (size_t c = mp.firstChunk[r]; c < mp.firstChunk[r + 1]; c++) totalCount += seedCounts[c];
        if (totalCount > p.flushSeeds) {
            mp.batches.push_back(MidBatchRange{lo, mp.firstChunk[r + 1], totalBases});
            lo = mp.firstChunk[r + 1];
            totalCount = totalBases = 0;
            flushed = true;
        }
    }
    if (totalCount > 0) mp.batches.push_back(MidBatchRange{lo, mp.plan.size(), totalBases});
    return flushed;
}

// the plan table of the result (six int32 per chunk) and the batch every chunk is searched in (kNoBatch: never)
std::vector<uint32_t> midPlanTable(const MidPlan& mp, const int32_t* seedCounts, TrimResult& res) {
    res.midChunks = (i64)mp.plan.size();
    res.midBatches = (i64)mp.batches.size();
    res.plan.resize(mp.plan.size() * 6);
    for (size_t c = 0; c < mp.plan.size(); c++) {
        const i64 seeds = seedCounts[c];
        res.midSeeds += seeds;
        const bool indexed = mp.plan[c].remainder || seeds >= kMinSeeds;
        const int32_t row[6] = {(int32_t)mp.plan[c].read, mp.plan[c].start, mp.plan[c].end, mp.plan[c].remainder, (int32_t)seeds, indexed ? 1 : 0};
        std::copy(row, row + 6, res.plan.begin() + 6 * (long)c);
    }
    // (chunks behind the last batch - a tail whose seeds sum to 0 - are never searched)
    std::vector<uint32_t> batchOf(mp.plan.size(), kNoBatch);
    for (size_t b = 0; b < mp.batches.size(); b++)
        for (size_t c = mp.batches[b].lo; c < mp.batches[b].hi; c++) batchOf[c] = (uint32_t)b;
    return batchOf;
}

// findSplit's rules (trim.go:527-586) over the records in canonical order - batch, adapter, chunk, ordinal: crops go into the reads'
// trims, the splits into `splits` (one per read) and, in the order made, `ids`
bool midFindSplits(ReadSet& reads, const ReadSet& front, const TrimParams& p, const MidPlan& mp, const std::vector<uint32_t>& batchOf, const TrimMidInput& in,
                   TrimResult& res, std::vector<MidSplit>& splits, std::vector<i64>& ids, std::string& error) {
    std::vector<TrimMidRec> recs;
    for (size_t i = 0; i < in.nRecs; i++) {
        const TrimMidRec& r = in.recs[i];
        if (r.adapter < 0 || (size_t)r.adapter >= front.size() || r.chunk < 0 || (size_t)r.chunk >= mp.plan.size()) {
            error = "trim: a middle record names an adapter or a chunk beyond the lists";
            return false;
        }
        if (batchOf[(size_t)r.chunk] == kNoBatch || !res.plan[6 * (size_t)r.chunk + 5]) {
            error = "trim: a middle record names a chunk that was not indexed";
            return false;
        }
        recs.push_back(r);
    }
    std::stable_sort(recs.begin(), recs.end(), [&](const TrimMidRec& a, const TrimMidRec& b) {
        const uint32_t ba = batchOf[(size_t)a.chunk], bb = batchOf[(size_t)b.chunk];
        if (ba != bb) return ba < bb;
        if (a.adapter != b.adapter) return a.adapter < b.adapter;
        if (a.chunk != b.chunk) return a.chunk < b.chunk;
        return a.ordinal < b.ordinal;
    });
    size_t at = 0;
    for (size_t b = 0; b < mp.batches.size(); b++) {
        if (p.verbosity > 0)
            logLine(res.errText, "Searching " + std::to_string(mp.batches[b].totalBases / 1000000) + " MB of sequences for splitting based on " +
                                     std::to_string(front.size()) + " adapters");
        for (; at < recs.size() && batchOf[(size_t)recs[at].chunk] == b; at++) {
            const TrimMidRec& m = recs[at];
            const i64 adLen = front.length((size_t)m.adapter);
            if (((i64)m.covered * 100) / adLen < p.middleThreshold) continue;  // :528
            res.applied.insert(res.applied.end(), {m.adapter, m.chunk, m.ordinal, m.startRel, m.covered, m.chainLen});
            const TrimChunk& c = mp.plan[(size_t)m.chunk];
            const size_t id = c.read;
            const i64 frontTrim = reads.frontTrim[id], backTrim = reads.backTrim[id];  // :538-539
            // the chunk is SubSequence(start, end) of the served read: offset = start, Len = end - start, and - `end--` comes before
            // the inset is taken (sequence.go:353-370) - inset = served length - end + 1
            const i64 start = (i64)c.start + m.startRel;           // :541
            const i64 seqLen = mp.servedLen[id] + 1 - backTrim;    // :542
            MidSplit& split = splits[id];
            if (start < kMinSeqLength + frontTrim) {  // :543 just crop the front off
                const i64 newTrim = start + adLen + p.extraMiddleTrim;
                if (newTrim + kMinSeqLength < seqLen) {
                    if (newTrim > frontTrim) {
                        reads.frontTrim[id] = (int32_t)newTrim;
                        if (split.live) {  // update the existing split
                            split.aEnd -= newTrim - frontTrim;
                            split.bStart -= newTrim - frontTrim;
                        }
                    }
                    if (p.tagAdapters) res.names[id] = front.names[(size_t)m.adapter] + "_" + res.names[id];
                } else {
                    split.live = false;  // in case of existing split that is no longer valid
                    reads.ignore[id] = 1;
                }
            } else if (start + kMinSeqLength + adLen > seqLen) {  // :560 crop off the tail
                const i64 newTrim = seqLen - start + p.extraMiddleTrim;
                if (newTrim > backTrim) reads.backTrim[id] = (int32_t)newTrim;
            } else if (split.live) {  // :568-574
                split.aEnd = std::min(split.aEnd, start - p.extraMiddleTrim - frontTrim);
                split.bStart = std::max(split.bStart, start + adLen + p.extraMiddleTrim - frontTrim);
            } else {  // :579-583
                split.live = true;
                split.aEnd = start - p.extraMiddleTrim - frontTrim;
                split.bStart = start + adLen + p.extraMiddleTrim - frontTrim;
                ids.push_back((i64)id);  // (an id whose split was dropped and made again is listed twice, as in the reference)
            }
        }
    }
    res.midRecords = (i64)res.applied.size() / 6;
    return true;
}

// trim.go:222-256 over the reads re-read with the trims as they stand now: the halves of the split reads become extras
void midEmitHalves(ReadSet& reads, const TrimParams& p, const std::vector<MidSplit>& splits, const std::vector<i64>& ids, TrimResult& res) {
    auto bases = [&](size_t id, i64 lo, i64 hi) {
        std::string t((size_t)(hi - lo), 'A');
        const char* s = reads.seq(id) + reads.frontTrim[id] + lo;
        for (i64 j = 0; j < hi - lo; j++) t[(size_t)j] = "ACGT"[baseCode((unsigned char)s[j])];
        return t;
    };
    auto quals = [&](size_t id, i64 lo, i64 hi) {
        std::string t;
        if (const uint8_t* q = reads.isFastq ? reads.quality(id) : nullptr)
            for (i64 j = lo; j < hi; j++) t += (char)(uint8_t)(q[reads.frontTrim[id] + j] + 33);
        return t;
    };
    for (i64 idv : ids) {
        const size_t id = (size_t)idv;
        const MidSplit& split = splits[id];
        if (!split.live) continue;
        const i64 len = reads.length(id) - reads.frontTrim[id] - reads.backTrim[id];
        int kept = 0;
        if (!p.discardMiddle) {
            std::string report = "Splitting read " + std::to_string(id) + " into";
            if (split.aEnd > kEdgeSize) {
                const i64 e = std::min(split.aEnd, len);  // SubSequence clamps its end (:354-356)
                res.extraNames.push_back(res.names[id] + "_(left)");
                res.extraBases.push_back(bases(id, 0, e));
                res.extraQuals.push_back(quals(id, 0, e));
                res.extraSpans.push_back(dp_read_span{(uint32_t)id, (uint32_t)reads.frontTrim[id], (uint32_t)e});
                report += ": 0 - " + std::to_string(split.aEnd) + " and ";
                kept |= 1;
            } else {
                report += " ignored short left hand side and ";
            }
            if (len - split.bStart > kEdgeSize) {
                if (split.bStart < 0) {  // SubSequence would slice out of range (the reference panics or reads past its bytes)
                    res.midOutOfRange++;
                    logLine(res.errText, "Skipping the right hand side of read " + std::to_string(id) + ": its start " + std::to_string(split.bStart) + " is out of range");
                    report += " out of range right hand side";
                } else {
                    res.extraNames.push_back(res.names[id] + "_(right)");
                    res.extraBases.push_back(bases(id, split.bStart, len));
                    res.extraQuals.push_back(quals(id, split.bStart, len));
                    res.extraSpans.push_back(dp_read_span{(uint32_t)id, (uint32_t)(reads.frontTrim[id] + split.bStart), (uint32_t)(len - split.bStart)});
                    report += std::to_string(split.bStart) + " - " + std::to_string(len);
                    kept |= 2;
                }
            } else {
                report += " ignored short right hand side";
            }
            if (p.verbosity > 1) {
                logLine(res.errText, report);
                if (split.aEnd >= 0 && split.bStart < len && split.bStart - split.aEnd - (i64)p.extraMiddleTrim * 2 <= kLongestAdapter)
                    logLine(res.errText, bases(id, split.aEnd + p.extraMiddleTrim, std::min(split.bStart - p.extraMiddleTrim, len)));
            }
        }
        res.splits.insert(res.splits.end(), {(int32_t)id, (int32_t)split.aEnd, (int32_t)split.bStart, kept});
        reads.ignore[id] = 1;  // :255
    }
}

// The middle stage's sequential half over the plan `mp` of the edge-trimmed reads and the matching stage's results: crops, splits and
// extras.  setupIndex() after a flush zeroes frontCounts / backCounts (trim.go:78-79, :202), so the stats lines then print zeros.
bool trimMiddle(ReadSet& reads, const ReadSet& front, const TrimParams& p, MidPlan& mp, const TrimMidInput& in, TrimResult& res, std::string& error) {
    if (in.nChunks != mp.plan.size()) {
        error = "trim: " + std::to_string(in.nChunks) + " seed counts for " + std::to_string(mp.plan.size()) + " planned chunks";
        return false;
    }
    const bool flushed = midCutBatches(p, in.seedCounts, mp);
    const std::vector<uint32_t> batchOf = midPlanTable(mp, in.seedCounts, res);
    std::vector<MidSplit> splits(reads.size() + 1);
    std::vector<i64> ids;
    if (!midFindSplits(reads, front, p, mp, batchOf, in, res, splits, ids, error)) return false;
    if (p.verbosity > 0) logLine(res.errText, std::to_string(ids.size()) + " sequences require splitting");  // :218-220
    midEmitHalves(reads, p, splits, ids, res);
    if (flushed) std::fill(res.counts.begin(), res.counts.end(), 0);
    return true;
}

// ---- SeedSequence.Match on the host (seeds/sequence.go:85-123, 361-576), for the pairs the device lists as beyond its working set --
// Reduced (:85-123): the seeds of `seg` that are in the whitelist and differ from the seed kept before them; index = their positions
int hostReduced(const int32_t* seg, int n, const std::vector<uint64_t>& wl, int k, int minSeeds, std::vector<int32_t>& out, std::vector<int>& index) {
    auto has = [&](int x) { return (wl[(size_t)x >> 6] >> (x & 63)) & 1ull; };
    int count = 0, prev = -1;
    for (int i = 1; i < n; i += 2) {
        const int next = seg[i];
        if (next != prev && has(next)) {
            count++;
            prev = next;
        }
    }
    if (count < minSeeds) return -1;
    out.assign((size_t)count * 2 + 1, 0);
    index.assign((size_t)count, 0);
    int offset = seg[0], j = 0;
    prev = -1;
    for (int i = 1; i < n; i += 2) {
        const int seed = seg[i];
        if (prev != seed && has(seed)) {
            out[(size_t)j] = offset;
            out[(size_t)j + 1] = seed;
            index[(size_t)j / 2] = i / 2;
            j += 2;
            offset = seg[i + 1];
            prev = seed;
        } else {
            offset += seg[i + 1] + k;
        }
    }
    out[(size_t)j] = offset;
    return count;
}
struct HostChains {
    std::vector<std::vector<int>> a, b;  // chain -> seed indices of the reduced query / target
    std::vector<int> headChain, headLen;
};
// extendChain (:476-576); as = reduced query, bs = reduced target
void hostExtend(HostChains& C, const std::vector<int32_t>& as, const std::vector<int32_t>& bs, int aIndex, int bIndex, int k, int cur) {
    const int an = (int)as.size(), bn = (int)bs.size();
    std::vector<int>&ca = C.a[(size_t)cur], &cb = C.b[(size_t)cur];
    int offsetA = as[(size_t)aIndex + 1], offsetB = bs[(size_t)bIndex + 1];
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
            offsetA += as[(size_t)aIndex + 1] + k;
            aIndex += 2;
            if (aIndex >= an) return;
            aSeedIndex = aIndex / 2;
            minBOffset = (offsetA * 2) / 3 - k;
            maxBOffset = (offsetA * 3) / 2 + k;
        }
        while (offsetB < minBOffset) {
            offsetB += bs[(size_t)bIndex + 1] + k;
            bIndex += 2;
            if (bIndex >= bn) return;
        }
        const int oldBIndex = bIndex, oldBOffset = offsetB;
        bool matched = false;
        const int seedA = as[(size_t)aIndex];
        while (offsetB <= maxBOffset) {
            if (seedA == bs[(size_t)bIndex]) {
                const int hc = C.headChain[(size_t)aSeedIndex];
                if (hc >= 0) {
                    const int hl = C.headLen[(size_t)aSeedIndex];
                    if (bIndex / 2 == C.b[(size_t)hc][(size_t)hl - 1] && hl > (int)ca.size()) return;  // they have a better chain already
                }
                ca.push_back(aSeedIndex);
                cb.push_back(bIndex / 2);
                C.headChain[(size_t)aSeedIndex] = cur;
                C.headLen[(size_t)aSeedIndex] = (int)ca.size();
                offsetA = as[(size_t)aIndex + 1];
                offsetB = bs[(size_t)bIndex + 1];
                aIndex += 2;
                bIndex += 2;
                matched = true;
                break;
            }
            offsetB += bs[(size_t)bIndex + 1] + k;
            bIndex += 2;
            if (bIndex >= bn) break;
        }
        if (!matched) {
            offsetA += as[(size_t)aIndex + 1] + k;
            aIndex += 2;
            offsetB = oldBOffset;
            bIndex = oldBIndex;
        }
    }
}
// dynamicMatch (:401-471): the good chains in the reference's return order
std::vector<int> hostDynamicMatch(HostChains& C, const std::vector<int32_t>& qs, const std::vector<int32_t>& ss, int minMatch, int k) {
    if (minMatch == 0) minMatch = 1;
    const int qn = (int)qs.size(), sn = (int)ss.size(), nq = qn / 2;
    C.headChain.assign((size_t)nq, -1);
    C.headLen.assign((size_t)nq, 0);
    std::vector<int> good;
    for (int qIndex = 1; qIndex < qn - minMatch * 2 + 2; qIndex += 2) {
        if (qs[(size_t)qIndex - 1] < 0 && qIndex > 1 && qs[(size_t)qIndex + 1] < 0 && qs[(size_t)qIndex] == qs[(size_t)qIndex - 2] && qs[(size_t)qIndex] == qs[(size_t)qIndex + 2])
            continue;
        const int qsi = qIndex / 2;
        if (C.headChain[(size_t)qsi] >= 0) continue;
        int prevSeed = -1;
        for (int i = 1; i < sn - minMatch * 2 + 2; i += 2) {
            const int nextSeed = ss[(size_t)i];
            const int hc = C.headChain[(size_t)qsi];
            if (nextSeed == qs[(size_t)qIndex] && nextSeed != prevSeed && (hc < 0 || C.b[(size_t)hc][(size_t)C.headLen[(size_t)qsi] - 1] != i / 2)) {
                const int c = (int)C.a.size();
                C.a.push_back({qsi});
                C.b.push_back({i / 2});
                C.headChain[(size_t)qsi] = c;
                C.headLen[(size_t)qsi] = 1;
                hostExtend(C, qs, ss, qIndex, i, k, c);
                const int len = (int)C.a[(size_t)c].size();
                if (len >= minMatch) {
                    const int nextLength = (len * 2) / 3;
                    if (nextLength > minMatch) {
                        minMatch = nextLength;
                        for (int j = (int)good.size() - 1; j >= 0; j--)
                            if ((int)C.a[(size_t)good[(size_t)j]].size() < nextLength) {
                                good[(size_t)j] = good.back();
                                good.pop_back();
                            }
                    }
                    good.push_back(c);
                    int remaining = 0;
                    for (int x = 0; x < nq; x++) remaining += C.headChain[(size_t)x] < 0;
                    if (remaining < len) return good;
                }
            }
            prevSeed = nextSeed;
        }
    }
    return good;
}
// a device call's outcome: false with the handle's (h == nullptr: the set-up's) error text
bool devOk(bool ok, const dp_trim* h, std::string& error) {
    if (!ok) error = std::string("trim: ") + dp_trim_error(h);
    return ok;
}
typedef std::unique_ptr<dp_trim, void (*)(dp_trim*)> TrimDev;
TrimDev setupDevice(const TrimIndex& ix, int device, std::string& error) {
    dp_trim* h = nullptr;
    const int rc = dp_trim_setup(device, ix.k, ix.kmerSeed.data(), ix.nSeeds, ix.nFront, ix.nBack, ix.segs.data(), ix.segOff.data(), ix.lengths.data(),
                                 ix.isBarcode.data(), ix.pairs.data(), &h);
    devOk(rc == 0 && h, nullptr, error);
    return TrimDev(h, dp_trim_release);
}

// the middle stage's device half over the plan `mp`: scan every planned chunk for its seed count, cut the flush batches, then per batch
// scan -> index -> candidates -> matching kernel, and the host's Match for the pairs the kernel listed
bool midDevice(dp_trim* h, dp_ctx* resident, uint32_t base, const ReadSet& reads, const TrimIndex& ix, const TrimParams& p, MidPlan& mp, std::vector<int32_t>& seedCounts,
               std::vector<TrimMidRec>& recs, TrimResult& res, std::string& error) {
    const size_t nC = mp.plan.size();
    seedCounts.assign(nC, 0);
    recs.clear();
    if (!nC || !ix.nFront) return true;
    std::vector<uint8_t> bases;
    std::vector<uint64_t> off;
    std::vector<uint32_t> cnt;
    std::vector<dp_read_span> spans;
    double tms[2];
    // chunks [lo, hi) cut from the trimmed reads and scanned in one call; their segments stay on the device.  With `resident` the chunks
    // are named as spans of the reads that context holds (host read r is its read base + r), in the coordinates of the uploaded read.
    auto scan = [&](size_t lo, size_t hi) -> bool {
        cnt.assign(hi - lo, 0);
        if (resident) {
            spans.clear();
            for (size_t c = lo; c < hi; c++) {
                const TrimChunk& ch = mp.plan[c];
                spans.push_back(dp_read_span{mapTailId(base, ch.read), (uint32_t)(reads.frontTrim[ch.read] + ch.start), (uint32_t)(ch.end - ch.start)});
            }
            if (!devOk(dp_trim_scan_chunks_resident(h, resident, spans.data(), (uint32_t)spans.size(), cnt.data(), tms) == 0, h, error)) return false;
            res.bytes_up += (double)(spans.size() * sizeof(dp_read_span));
        } else {
            off.assign(1, 0);
            for (size_t c = lo; c < hi; c++) off.push_back(off.back() + (uint64_t)(mp.plan[c].end - mp.plan[c].start));
            bases.resize((size_t)off.back() + 1);
            for (size_t c = lo; c < hi; c++) {
                const TrimChunk& ch = mp.plan[c];
                memcpy(bases.data() + off[c - lo], reads.seq(ch.read) + reads.frontTrim[ch.read] + ch.start, (size_t)(ch.end - ch.start));
            }
            if (!devOk(dp_trim_scan_chunks(h, bases.data(), off.data(), (uint32_t)(hi - lo), cnt.data(), tms) == 0, h, error)) return false;
            res.bytes_up += (double)off.back();
        }
        res.mid_upload_ms += tms[0];
        res.mid_scan_ms += tms[1];
        for (size_t c = lo; c < hi; c++) seedCounts[c] = (int32_t)cnt[c - lo];
        return true;
    };
    const uint64_t groupBases = (uint64_t)1 << 28;  // (bytes of chunk bases on the device per scan, whichever way they get there)
    size_t scannedLo = 0, scannedHi = 0;  // what the device holds segments of
    for (size_t lo = 0; lo < nC;) {
        size_t hi = lo;
        uint64_t b = 0;
        while (hi < nC && (hi == lo || b + (uint64_t)(mp.plan[hi].end - mp.plan[hi].start) <= groupBases)) b += (uint64_t)(mp.plan[hi].end - mp.plan[hi].start), hi++;
        if (!scan(lo, hi)) return false;
        scannedLo = lo;
        scannedHi = hi;
        lo = hi;
    }
    midCutBatches(p, seedCounts.data(), mp);
    std::vector<uint32_t> sel;
    std::vector<int32_t> cseg;
    for (const MidBatchRange& bt : mp.batches) {
        if (bt.lo != scannedLo || bt.hi != scannedHi) {
            if (!scan(bt.lo, bt.hi)) return false;
            scannedLo = bt.lo;
            scannedHi = bt.hi;
        }
        sel.clear();
        for (size_t c = bt.lo; c < bt.hi; c++)
            if (mp.plan[c].remainder || seedCounts[c] >= kMinSeeds) sel.push_back((uint32_t)(c - bt.lo));
        dp_trim_mid_batch mb;
        if (!devOk(dp_trim_search(h, sel.data(), (uint32_t)sel.size(), p.middleThreshold, &mb) == 0, h, error)) return false;
        res.midPairs += mb.n_pairs;
        res.midOverflowPairs += mb.n_overflow;
        res.mid_index_ms += mb.index_ms;
        res.mid_query_ms += mb.query_ms;
        res.mid_kernel_ms += mb.kernel_ms;
        res.bytes_down += (double)mb.n_recs * sizeof(dp_trim_mid_rec);
        static_assert(sizeof(dp_trim_mid_rec) == sizeof(TrimMidRec), "device and host records are the same six int32");
        for (uint32_t i = 0; i < mb.n_recs; i++) {
            const dp_trim_mid_rec& r = mb.recs[i];
            recs.push_back(TrimMidRec{r.adapter, (int32_t)(r.chunk + (int32_t)bt.lo), r.ordinal, r.start_rel, r.covered, r.chain_len});
        }
        const std::vector<uint32_t> over(mb.overflow, mb.overflow + 2 * (size_t)mb.n_overflow);  // (the handle's arrays go with its next call)
        for (size_t i = 0; i < over.size(); i += 2) {
            const uint32_t c = over[i], a = over[i + 1];
            uint64_t n = 0;
            cseg.resize(2 * (size_t)seedCounts[bt.lo + c] + 1);
            if (!devOk(dp_trim_chunk_segments(h, c, cseg.data(), cseg.size(), &n) == 0 && n == cseg.size(), h, error)) return false;
            trimHostMatch(cseg.data(), (int)cseg.size(), ix.segs.data() + ix.segOff[a], (int)(ix.segOff[a + 1] - ix.segOff[a]), ix.lengths[a], (int)ix.nSeeds, ix.k,
                          p.middleThreshold, (int32_t)a, (int32_t)(bt.lo + c), recs);
        }
    }
    return true;
}

// Demultiplex's bookkeeping for one name (seqio.go:460-523): a name that starts with "Barcode" loses its label, which is found in or
// added to `labels`; returns the label's index, -1 for a name without one
int demuxLabel(std::string& name, std::vector<std::string>& labels) {
    if (!isBarcodeName(name)) return -1;
    const size_t pos = name.find('_');
    if (pos == std::string::npos) return -1;
    const std::string label = name.substr(0, pos);
    size_t li = 0;
    while (li < labels.size() && labels[li] != label) li++;
    if (li == labels.size()) labels.push_back(label);
    name = name.substr(pos + 1);
    return (int)li;
}
}  // namespace

// setupIndex (trim.go:57-99): NewAllSeedSequence of every front, then every back adapter (seeds/seeds.go:204-237) - seed ids in order
// of first occurrence - and pairsFront / pairsBack by name
bool trimBuildIndex(const ReadSet& front, const ReadSet& back, int k, TrimIndex& ix, std::string& error) {
    if (k < 3 || k > 8) {
        error = "trim: k = " + std::to_string(k) + " is outside 3..8 (ShortKmers holds a k-mer in 16 bits)";
        return false;
    }
    ix = TrimIndex();
    ix.k = k;
    ix.nFront = (uint32_t)front.size();
    ix.nBack = (uint32_t)back.size();
    ix.kmerSeed.assign((size_t)1 << (2 * k), (uint16_t)0xffff);
    ix.segOff.push_back(0);
    const uint32_t mask = (uint32_t)(((size_t)1 << (2 * k)) - 1);
    for (const ReadSet* set : {&front, &back}) {
        for (size_t a = 0; a < set->size(); a++) {
            const char* s = set->seq(a);
            const i64 len = set->length(a);
            int prev = 0, kmerIndex = 0;
            uint32_t kmer = 0;
            for (i64 i = 0; i < k - 1 && i < len; i++) kmer = (kmer << 2) | baseCode((unsigned char)s[i]);  // KmerAt(0, k) >> 2 (:212)
            for (i64 i = k - 1; i < len; i++) {
                kmer = ((kmer << 2) | baseCode((unsigned char)s[i])) & mask;
                if (ix.kmerSeed[kmer] == 0xffff) {  // :217-226
                    if (ix.nSeeds >= 0xffff) {
                        error = "trim: more than 65534 distinct adapter k-mers";
                        return false;
                    }
                    ix.kmerSeed[kmer] = (uint16_t)ix.nSeeds++;
                }
                ix.segs.push_back(kmerIndex - prev);
                ix.segs.push_back((int32_t)ix.kmerSeed[kmer]);
                prev = kmerIndex + k;
                kmerIndex++;
            }
            ix.segs.push_back(0);  // :233
            ix.segOff.push_back((uint64_t)ix.segs.size());
            ix.lengths.push_back((int32_t)len);
            ix.isBarcode.push_back(isBarcodeName(set->names[a]) ? 1 : 0);
        }
    }
    // :81-98
    int pairID = 1;
    ix.pairs.assign(front.size() + back.size(), -1);
    for (size_t i = 0; i < front.size(); i++)
        for (size_t j = 0; j < back.size(); j++)
            if (back.names[j] == front.names[i]) {
                ix.pairs[i] = pairID;
                ix.pairs[front.size() + j] = pairID;
                pairID++;
                break;
            }
    return true;
}

// the chunk loop of trim.go:165-184 for a served (edge-trimmed) read of `length` bases
void trimChunkPlan(i64 length, i64 chunkSize, uint32_t read, std::vector<TrimChunk>& out) {
    for (i64 i = kEdgeSize; i < length - kEdgeSize - kLongestAdapter; i += chunkSize - kLongestAdapter) {
        if (i > length - (chunkSize * 3) / 2 - kEdgeSize) {  // add the entire remainder
            out.push_back(TrimChunk{read, (int32_t)i, (int32_t)(length - kEdgeSize), 1});
            break;
        }
        const i64 endPoint = std::min<i64>(i + chunkSize, length - kEdgeSize);
        out.push_back(TrimChunk{read, (int32_t)i, (int32_t)endPoint, 0});
    }
}

// Match(ad, adSet, chunkSet, minMatch, k) of one (chunk, front adapter) pair and the identity test of trim.go:527-530
void trimHostMatch(const int32_t* cSeg, int cN, const int32_t* aSeg, int aN, int adLen, int nSeeds, int k, int threshold, int32_t adapter, int32_t chunk,
                   std::vector<TrimMidRec>& out) {
    std::vector<uint64_t> aSet(((size_t)nSeeds + 63) / 64, 0), cSet(aSet.size(), 0);
    for (int i = 1; i < aN; i += 2) aSet[(size_t)aSeg[i] >> 6] |= 1ull << (aSeg[i] & 63);
    for (int i = 1; i < cN; i += 2) cSet[(size_t)cSeg[i] >> 6] |= 1ull << (cSeg[i] & 63);
    const int minMatch = (aN / 2) / 5;
    std::vector<int32_t> t, q;
    std::vector<int> tIdx, qIdx;
    if (hostReduced(cSeg, cN, aSet, k, minMatch, t, tIdx) < 0) return;
    if (hostReduced(aSeg, aN, cSet, k, minMatch, q, qIdx) < 0) return;
    HostChains C;
    const std::vector<int> good = hostDynamicMatch(C, q, t, minMatch, k);
    auto seedOffset = [&](const int32_t* seg, int index) {  // GetSeedOffset (seeds/sequence.go:1239-1246)
        index = index * 2 + 1;
        int o = seg[0];
        for (int i = 2; i < index; i += 2) o += seg[i] + k;
        return o;
    };
    for (size_t g = 0; g < good.size(); g++) {
        const std::vector<int>&ca = C.a[(size_t)good[g]], &cb = C.b[(size_t)good[g]];
        const int len = (int)ca.size();
        int countA = len * k, prevA = qIdx[(size_t)ca[0]];  // GetBasesCovered's countA (:830-858)
        for (int i = 1; i < len; i++) {
            const int s = qIdx[(size_t)ca[(size_t)i]];
            int d1 = aSeg[prevA * 2 + 2];
            for (int j = prevA + 2; j <= s; j++) d1 += aSeg[j * 2] + k;
            if (d1 < 0) countA += d1;
            prevA = s;
        }
        if ((countA * 100) / adLen < threshold) continue;
        out.push_back(TrimMidRec{adapter, chunk, (int32_t)g, seedOffset(cSeg, tIdx[(size_t)cb[0]]) - seedOffset(aSeg, qIdx[(size_t)ca[0]]), countA, len});
    }
}
// fastaWriter / fastqWriter with fullNames (seqio.go:401-435) over the non-ignored reads in file order; keep (may be null) selects reads
void trimWrite(const ReadSet& reads, const std::vector<std::string>& names, const std::vector<uint8_t>* keep, std::string& out) {
    for (size_t r = 0; r < reads.size(); r++) {
        if (reads.ignore[r] || (keep && !(*keep)[r])) continue;
        const i64 ft = reads.frontTrim.empty() ? 0 : reads.frontTrim[r], bt = reads.backTrim.empty() ? 0 : reads.backTrim[r];
        const i64 n = reads.length(r) - ft - bt;
        const char* s = reads.seq(r) + ft;
        out += reads.isFastq ? '@' : '>';
        out += names[r];
        out += '\n';
        const size_t at = out.size();
        out.resize(at + (size_t)n);
        for (i64 j = 0; j < n; j++) out[at + j] = "ACGT"[baseCode((unsigned char)s[j])];  // packedSequence.String (sequence.go:242-276)
        out += '\n';
        if (reads.isFastq) {
            out += "+\n";
            if (const uint8_t* q = reads.quality(r))  // (a read whose quality line did not match its length carries none: an empty line)
                for (i64 j = 0; j < n; j++) out += (char)(uint8_t)(q[ft + j] + 33);
            out += '\n';
        }
    }
}

// Demultiplex (seqio.go:460-523): reads whose name starts with "Barcode" go to <label><ext> with the label cut off their name; a file
// that exists is replaced (the reference opens without truncating and leaves the tail of a longer old file in place)
int trimDemultiplex(const ReadSet& reads, const TrimResult& res, const std::string& dir, std::string& error) {
    // labels in the order first seen: over the reads, then over the halves of split reads that follow them (sendExtras)
    std::vector<std::string> labels;
    std::vector<std::string> names = res.names, extraNames = res.extraNames;
    std::vector<int> labelOf(reads.size(), -1), extraLabelOf(extraNames.size(), -1);
    for (size_t r = 0; r < reads.size(); r++)
        if (!reads.ignore[r]) labelOf[r] = demuxLabel(names[r], labels);
    for (size_t e = 0; e < extraNames.size(); e++) extraLabelOf[e] = demuxLabel(extraNames[e], labels);
    const char* ext = reads.isFastq ? ".fastq" : ".fasta";
    std::vector<uint8_t> keep(reads.size()), keepExtra(extraNames.size());
    for (size_t li = 0; li < labels.size(); li++) {
        const std::string path = dir + "/" + labels[li] + ext;
        for (size_t r = 0; r < reads.size(); r++) keep[r] = labelOf[r] == (int)li;
        for (size_t e = 0; e < extraNames.size(); e++) keepExtra[e] = extraLabelOf[e] == (int)li;
        std::string text;
        trimWrite(reads, names, &keep, text);
        writeExtras(reads, res, extraNames, &keepExtra, text);
        const int fd = open(path.c_str(), O_CREAT | O_WRONLY | O_TRUNC, 0755);
        if (fd < 0) {
            error = "Unable to open file for writing:" + path;
            return -1;
        }
        size_t done = 0;
        while (done < text.size()) {
            const ssize_t w = write(fd, text.data() + done, text.size() - done);
            if (w <= 0) {
                close(fd);
                error = "write failed: " + path;
                return -1;
            }
            done += (size_t)w;
        }
        close(fd);
    }
    return (int)labels.size();
}

// The device-free half: DetermineAdapters' compaction from caller-supplied flags (enabled == nullptr: none ran), then trimWorker,
// PrintStats and Write from caller-supplied edge records of the eligible reads (in read order) and per-adapter match counts, both
// in the order of the COMPACTED adapter lists; with mid and p.middle, the middle stage's sequential half over its matching results too.
int applyTrim(ReadSet& reads, const ReadSet& front0, const ReadSet& back0, const TrimParams& p, const uint8_t* enabled, const dp_trim_rec* recs,
              size_t nRecReads, const uint64_t* counts, const TrimMidInput* mid, TrimResult& res, std::string& error) {
    res = TrimResult();
    ReadSet front = front0, back = back0;
    if (enabled) {
        front = pickAdapters(front0, compactAdapters(front0, enabled, "front", p.verbosity, res.errText));
        back = pickAdapters(back0, compactAdapters(back0, enabled + front0.size(), "back", p.verbosity, res.errText));
    }
    TrimIndex ix;
    if (!trimBuildIndex(front, back, p.k, ix, error)) return -1;
    if (p.verbosity > 0) logLine(res.errText, "Trimming ends and indexing all sequences against " + std::to_string(front.size()) + " adapters...");
    std::vector<uint32_t> eligible;
    eligibleReads(reads, 0, reads.size(), eligible);
    if (eligible.size() != nRecReads) {
        error = "trim: " + std::to_string(nRecReads) + " edge record pairs for " + std::to_string(eligible.size()) + " reads of 200 bases and more";
        return -1;
    }
    const double t0 = now();
    if (!applyEdgeRecords(reads, front, back, ix, p, eligible, recs, counts, res, error)) return -1;
    if (mid && p.middle) {
        MidPlan mp;
        if (!midBuildPlan(reads, p, mp, error) || !trimMiddle(reads, front, p, mp, *mid, res, error)) return -1;
    }
    fillTable(reads, res);
    res.t_apply = now() - t0;
    return reportAndWrite(reads, front, back, res, error);
}

int runTrim(ReadSet& reads, const ReadSet& front0, const ReadSet& back0, const TrimParams& p, int device, TrimResult& res, std::string& error,
            dp_ctx* resident, uint32_t residentBase) {
    res = TrimResult();
    TrimIndex ix;
    if (!trimBuildIndex(front0, back0, p.k, ix, error)) return -1;
    ReadSet front = front0, back = back0;
    const size_t batchReads = (size_t)1 << 17;  // 39 MB of ends per call
    EdgeBatch eb;
    double tms[3];
    if (p.determineAdapters) {  // DetermineAdapters (:272-324) over the first check_reads reads
        const double t0 = now();
        const size_t nCheck = (size_t)std::max<i64>(0, std::min<i64>(p.checkReads, (i64)reads.size()));
        std::vector<uint8_t> enabled(front0.size() + back0.size(), 0);
        if (!enabled.empty()) {
            const TrimDev h = setupDevice(ix, device, error);
            if (!h) return kTrimDeviceFailed;
            for (size_t lo = 0; lo < nCheck; lo += batchReads) {
                const size_t hi = std::min(nCheck, lo + batchReads);
                double up;
                edgeBatch(reads, lo, hi, resident != nullptr, eb);
                if (!devOk(edgeCall(h.get(), resident, residentBase, reads, lo, hi, eb, DP_TRIM_MODE_DETERMINE, 0, p.adapterThreshold, nullptr, nullptr, enabled.data(), tms, &up) == 0,
                           h.get(), error))
                    return kTrimDeviceFailed;
                res.k_determine_ms += tms[1];
            }
        }
        front = pickAdapters(front0, compactAdapters(front0, enabled.data(), "front", p.verbosity, res.errText));
        back = pickAdapters(back0, compactAdapters(back0, enabled.data() + front0.size(), "back", p.verbosity, res.errText));
        if (!trimBuildIndex(front, back, p.k, ix, error)) return -1;  // setupIndex() :323
        res.t_determine = now() - t0;
    }
    if (p.verbosity > 0) logLine(res.errText, "Trimming ends and indexing all sequences against " + std::to_string(front.size()) + " adapters...");
    const size_t nA = front.size() + back.size();
    std::vector<uint32_t> eligible;
    std::vector<dp_trim_rec> recs;
    std::vector<uint64_t> counts(nA, 0);
    TrimDev h(nullptr, dp_trim_release);
    if (nA) {
        h = setupDevice(ix, device, error);
        if (!h) return kTrimDeviceFailed;
    }
    for (size_t lo = 0; lo < reads.size(); lo += batchReads) {
        const double t0 = now();
        const size_t hi = std::min(reads.size(), lo + batchReads);
        edgeBatch(reads, lo, hi, resident != nullptr, eb);
        res.t_extract += now() - t0;
        const size_t at = eligible.size();
        eligible.insert(eligible.end(), eb.reads.begin(), eb.reads.end());
        recs.resize(2 * eligible.size(), dp_trim_rec{kEdgeSize, 0, 0, 0, 0, 0});  // (no adapters at all: what findMatches returns)
        if (h && !eb.reads.empty()) {
            double up;
            if (!devOk(edgeCall(h.get(), resident, residentBase, reads, lo, hi, eb, DP_TRIM_MODE_TRIM, 3, 0, recs.data() + 2 * at, counts.data(), nullptr, tms, &up) == 0, h.get(), error))
                return kTrimDeviceFailed;
            res.upload_ms += tms[0];
            res.kernel_ms += tms[1];
            res.download_ms += tms[2];
            res.bytes_up += up;
            res.bytes_down += (double)(2 * eb.reads.size() * sizeof(dp_trim_rec));
        }
    }
    const double t0 = now();
    if (!applyEdgeRecords(reads, front, back, ix, p, eligible, recs.data(), counts.data(), res, error)) return -1;
    if (p.middle && h) {  // the matching results are made once the edge trims stand
        MidPlan mp;
        std::vector<int32_t> seedCounts;
        std::vector<TrimMidRec> midRecs;
        if (!midBuildPlan(reads, p, mp, error)) return -1;
        if (!midDevice(h.get(), resident, residentBase, reads, ix, p, mp, seedCounts, midRecs, res, error)) return kTrimDeviceFailed;
        TrimMidInput mid;
        mid.seedCounts = seedCounts.data();
        mid.nChunks = seedCounts.size();
        mid.recs = midRecs.data();
        mid.nRecs = midRecs.size();
        if (!trimMiddle(reads, front, p, mp, mid, res, error)) return -1;
    }
    fillTable(reads, res);
    res.t_apply = now() - t0;
    h.reset();
    return reportAndWrite(reads, front, back, res, error, resident == nullptr);
}

// The read set `trim`'s output would give when read back (rules 3 and 4 of DESIGN.md 4.8), without the text: the non-ignored reads in
// file order under their names after tagging, bases [front trim, length - back trim), then the halves of split reads in the order
// added; every record spelled "ACGT"[code] with its quality bytes as trimWrite / writeExtras print them, and kept as
// ReadSet::addLine keeps a written line of n bases: iff n + 1 >= minLen (a record of no bases is dropped).  spans[i] names record i of
// `out` in the coordinates of `raw`, the read set the trim ran on.
void trimmedReadSet(const ReadSet& raw, const TrimResult& res, i64 minLen, bool himem, ReadSet& out, std::vector<dp_read_span>& spans) {
    out = ReadSet();
    out.himem = himem;
    out.off.push_back(0);
    spans.clear();
    std::string line, ql;
    auto add = [&](const std::string& name, const dp_read_span& sp) {
        if (sp.len == 0) return;
        out.isFastq = raw.isFastq;  // (the written file's first line would begin with '@')
        const char* s = raw.seq(sp.read) + sp.start;
        line.resize((size_t)sp.len + 1);
        for (uint32_t j = 0; j < sp.len; j++) line[j] = "ACGT"[baseCode((unsigned char)s[j])];
        line[sp.len] = '\n';
        const uint8_t* q = raw.isFastq ? raw.quality(sp.read) : nullptr;
        ql.clear();
        if (q)
            for (uint32_t j = 0; j < sp.len; j++) ql += (char)(uint8_t)(q[sp.start + j] + 33);
        ql += '\n';
        const size_t before = out.size();
        out.addLine(name, line.data(), line.size(), minLen, raw.isFastq ? ql.data() : nullptr, raw.isFastq ? ql.size() : 0);
        if (out.size() != before) spans.push_back(sp);
    };
    for (size_t r = 0; r < raw.size(); r++) {
        const int32_t* row = res.table.data() + 5 * r;
        if (row[2]) continue;
        add(res.names[r], dp_read_span{(uint32_t)r, (uint32_t)row[0], (uint32_t)(raw.length(r) - row[0] - row[1])});
    }
    for (size_t e = 0; e < res.extraSpans.size(); e++) add(res.extraNames[e], res.extraSpans[e]);
    if (out.isFastq) {
        out.qual.resize(out.bases.size(), 0);
        out.hasQual.resize(out.names.size(), 0);
    }
}

}  // namespace dph
