// trim.Trimmer, edge stage (trim/trim.go:13-132, 259-513; commands/trim.go:32-50): adapter determination, end trimming, tagging,
// pairing, stats, the trimmed FASTA / FASTQ writer and demultiplexing (sequence/seqio.go:375-523).  The matching itself - findMatches
// and isNewFullMatch for every read end - runs on the device (dp_trim_edges); what stays here is the sequential logic around it.
// The search for adapters in the middle of reads (Trim's second half and findSplit, :151-257, :515-591) is not part of this build.
//
// Canonical semantics where the reference depends on goroutine scheduling: one worker, so reads are judged and written in file order.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include "host_util.hpp"

namespace dph {

namespace {
const int kEdgeSize = 150;  // trim.go:432,453

void logLine(std::string& err, const std::string& s) {  // log.Println without the timestamp (the CLI adds it)
    err += s;
    err += '\n';
}
bool isBarcodeName(const std::string& n) { return n.compare(0, 7, "Barcode") == 0; }  // strings.HasPrefix(name, "Barcode") :377
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

namespace {
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
void extractEnds(const ReadSet& reads, size_t lo, size_t hi, EdgeBatch& b) {
    b.reads.clear();
    for (size_t r = lo; r < hi; r++)
        if (reads.length(r) >= kEdgeSize + 50) b.reads.push_back((uint32_t)r);
    b.ends.resize(b.reads.size() * 2 * kEdgeSize);
    for (size_t i = 0; i < b.reads.size(); i++) {
        const size_t r = b.reads[i];
        memcpy(b.ends.data() + i * 2 * kEdgeSize, reads.seq(r), kEdgeSize);
        memcpy(b.ends.data() + i * 2 * kEdgeSize + kEdgeSize, reads.seq(r) + reads.length(r) - kEdgeSize, kEdgeSize);
    }
}

// trimWorker's arithmetic on the device's records (trim.go:464-510), PrintStats (:260-268) and Write (seqio.go:401-458)
int finishTrim(ReadSet& reads, const ReadSet& front, const ReadSet& back, const TrimIndex& ix, const TrimParams& p, const std::vector<uint32_t>& eligible,
               const dp_trim_rec* recs, const uint64_t* counts, TrimResult& res, std::string& error) {
    const double t0 = now();
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
            return -1;
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
    for (size_t r = 0; r < n; r++) {
        res.table[5 * r] = reads.frontTrim[r];
        res.table[5 * r + 1] = reads.backTrim[r];
        res.table[5 * r + 2] = reads.ignore[r];
    }
    res.frontNames = front.names;
    res.backNames = back.names;
    res.counts.assign(counts, counts + front.size() + back.size());
    res.t_apply = now() - t0;
    // PrintStats: with seenCount == 0 the reference divides by zero
    if (res.seen == 0) {
        logLine(res.errText, "no reads long enough to trim");
        error = "trim: no reads long enough to trim (the ends are searched in reads of 200 bases and more)";
        return -2;
    }
    for (size_t i = 0; i < front.size(); i++)
        logLine(res.errText, "Front adapter: " + front.names[i] + " \t " + std::to_string((i64)(counts[i] * 100) / res.seen) + " %");
    for (size_t i = 0; i < back.size(); i++)
        logLine(res.errText, "Back adapter: " + back.names[i] + " \t " + std::to_string((i64)(counts[front.size() + i] * 100) / res.seen) + " %");
    logLine(res.errText, std::to_string((res.none * 100) / res.seen) + " % with no adapters found.");
    logLine(res.errText, "Writing trimmed sequences...");  // commands/trim.go:44
    const double t1 = now();
    res.out.clear();
    trimWrite(reads, res.names, nullptr, res.out);
    res.t_write = now() - t1;
    return 0;
}

#define TRIM_DEV(call, h)                                     \
    do {                                                      \
        if ((call) != 0) {                                    \
            error = std::string("trim: ") + dp_trim_error(h); \
            if (h) dp_trim_release(h);                        \
            return -1;                                        \
        }                                                     \
    } while (0)

dp_trim* setupDevice(const TrimIndex& ix, int device) {
    dp_trim* h = nullptr;
    dp_trim_setup(device, ix.k, ix.kmerSeed.data(), ix.nSeeds, ix.nFront, ix.nBack, ix.segs.data(), ix.segOff.data(), ix.lengths.data(),
                  ix.isBarcode.data(), ix.pairs.data(), &h);
    return h;
}
}  // namespace

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
    std::vector<std::string> labels;
    std::vector<std::vector<uint8_t>> keep;
    std::vector<std::string> names = res.names;
    for (size_t r = 0; r < reads.size(); r++) {
        if (reads.ignore[r]) continue;
        const std::string n = names[r];
        if (!isBarcodeName(n)) continue;
        const size_t pos = n.find('_');
        if (pos == std::string::npos) continue;
        const std::string label = n.substr(0, pos);
        size_t li = 0;
        while (li < labels.size() && labels[li] != label) li++;
        if (li == labels.size()) {
            labels.push_back(label);
            keep.emplace_back(reads.size(), 0);
        }
        names[r] = n.substr(pos + 1);
        keep[li][r] = 1;
    }
    const char* ext = reads.isFastq ? ".fastq" : ".fasta";
    for (size_t li = 0; li < labels.size(); li++) {
        const std::string path = dir + "/" + labels[li] + ext;
        std::string text;
        trimWrite(reads, names, &keep[li], text);
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
// in the order of the COMPACTED adapter lists.
int applyTrim(ReadSet& reads, const ReadSet& front0, const ReadSet& back0, const TrimParams& p, const uint8_t* enabled, const dp_trim_rec* recs,
              size_t nRecReads, const uint64_t* counts, TrimResult& res, std::string& error) {
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
    for (size_t r = 0; r < reads.size(); r++)
        if (reads.length(r) >= kEdgeSize + 50) eligible.push_back((uint32_t)r);
    if (eligible.size() != nRecReads) {
        error = "trim: " + std::to_string(nRecReads) + " edge record pairs for " + std::to_string(eligible.size()) + " reads of 200 bases and more";
        return -1;
    }
    return finishTrim(reads, front, back, ix, p, eligible, recs, counts, res, error);
}

int runTrim(ReadSet& reads, const ReadSet& front0, const ReadSet& back0, const TrimParams& p, int device, TrimResult& res, std::string& error) {
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
            dp_trim* h = setupDevice(ix, device);
            TRIM_DEV(h ? 0 : 1, h);
            for (size_t lo = 0; lo < nCheck; lo += batchReads) {
                extractEnds(reads, lo, std::min(nCheck, lo + batchReads), eb);
                TRIM_DEV(dp_trim_edges(h, eb.ends.data(), (uint32_t)eb.reads.size(), DP_TRIM_MODE_DETERMINE, 0, p.adapterThreshold, nullptr, nullptr,
                                       enabled.data(), tms),
                         h);
                res.k_determine_ms += tms[1];
            }
            dp_trim_release(h);
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
    dp_trim* h = nullptr;
    if (nA) {
        h = setupDevice(ix, device);
        TRIM_DEV(h ? 0 : 1, h);
    }
    for (size_t lo = 0; lo < reads.size(); lo += batchReads) {
        const double t0 = now();
        extractEnds(reads, lo, std::min(reads.size(), lo + batchReads), eb);
        res.t_extract += now() - t0;
        const size_t at = eligible.size();
        eligible.insert(eligible.end(), eb.reads.begin(), eb.reads.end());
        recs.resize(2 * eligible.size(), dp_trim_rec{kEdgeSize, 0, 0, 0, 0, 0});  // (no adapters at all: what findMatches returns)
        if (h && !eb.reads.empty()) {
            TRIM_DEV(dp_trim_edges(h, eb.ends.data(), (uint32_t)eb.reads.size(), DP_TRIM_MODE_TRIM, 3, 0, recs.data() + 2 * at, counts.data(), nullptr, tms), h);
            res.upload_ms += tms[0];
            res.kernel_ms += tms[1];
            res.download_ms += tms[2];
            res.bytes_up += (double)eb.ends.size();
            res.bytes_down += (double)(2 * eb.reads.size() * sizeof(dp_trim_rec));
        }
    }
    if (h) dp_trim_release(h);
    return finishTrim(reads, front, back, ix, p, eligible, recs.data(), counts.data(), res, error);
}

}  // namespace dph
