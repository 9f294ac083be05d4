// The boundary of libdownpore_host.so and nothing else: every entry point include/downpore_host.h declares (read sets, `overlap`
// round by round with the multi-GPU exchanges, `map`, `trim`).  A Go command, bench.py and the Python drivers come in here.  The
// entry points that only tests call are in host_testhooks.cpp (dph_testhooks.h).
#include <atomic>
#include <algorithm>
#include <cstring>

#include "downpore_host.h"
#include "dph_handles.hpp"
#include "host_util.hpp"

using namespace dph;

namespace {
struct OverlapH {
    OverlapRun run;
    dp_ctx* ctx = nullptr;
    dp_comm* comm = nullptr;
    dp_ctx* xctx = nullptr;           // round-parallel mode: the context (own stream) the result exchange runs on
    std::vector<dp_comm*> slotComms;  // scan-shard with executor slots: one communicator per slot
    ReadSet* reads = nullptr;
    ReadsH* trimmed = nullptr;        // dph_overlap_open_trim: the trimmed read set the job runs on (owned; `reads` points into it)
    int textRoot = -1;                // dph_overlap_text_root: >= 0 = a superstep gathers the rounds' PAF text to that rank only
    bool keepText = true;             // dph_overlap_keep_text(0): gathered rounds of other ranks are committed without their PAF text
    double tCtx = 0, tUpload = 0, tInit = 0;
    std::string err;
    // PAF of every committed round so far.  Kept as one chunk per commit and joined only when somebody asks for the
    // whole text: appending to one growing std::string re-copied up to 128 MB at every doubling (20-30 ms stalls of the
    // committing thread at rounds ~80, ~165, ~330 of a config-2 job).
    // (round 4: a step's text is MOVED in - it is the buffer a formatter thread filled, never copied, never freed before the job
    // ends: copying 400 KB per round into fresh memory and freeing the original was an mmap + munmap pair per round on the
    // committing thread)
    std::vector<std::string> pafChunks;
    std::string allPafJoined;
    std::string lastStepCopy;  // text of the last step once allPaf() has folded the chunks away
    bool lastStepHasText = false, lastStepInChunks = false;
    void addPaf(std::string& s) {  // takes s's buffer; s is empty afterwards
        lastStepHasText = !s.empty();
        lastStepInChunks = lastStepHasText;
        if (lastStepHasText) {
            pafChunks.push_back(std::move(s));
            s.clear();
        }
    }
    const std::string& lastStepText() const {
        static const std::string none;
        if (!lastStepHasText) return none;
        return lastStepInChunks ? pafChunks.back() : lastStepCopy;
    }
    const std::string& allPaf() {
        if (!pafChunks.empty()) {
            size_t n = allPafJoined.size();
            for (const std::string& c : pafChunks) n += c.size();
            allPafJoined.reserve(n);
            for (const std::string& c : pafChunks) allPafJoined += c;
            if (lastStepHasText && lastStepInChunks) {
                lastStepCopy = pafChunks.back();
                lastStepInChunks = false;
            }
            pafChunks.clear();
        }
        return allPafJoined;
    }
};
thread_local std::string g_err;
}  // namespace

extern "C" {

const char* dph_last_error(void* h) { return h ? ((OverlapH*)h)->err.c_str() : g_err.c_str(); }

void* dph_reads_from_arrays(const char* bases, const int64_t* off, int64_t n, int64_t minLen, int himem) {
    return new ReadsH{ReadSet::fromArrays(bases, off, (size_t)n, minLen, himem != 0)};
}
// bases + raw FASTQ quality characters at the same offsets: the set behaves as if it had been read from a FASTQ file
void* dph_reads_from_arrays_q(const char* bases, const char* quals, const int64_t* off, int64_t n, int64_t minLen, int himem) {
    return new ReadsH{ReadSet::fromArrays(bases, off, (size_t)n, minLen, himem != 0, quals)};
}
void* dph_reads_from_fasta(const char* path, int64_t minLen, int himem) {
    ReadsH* h = new ReadsH();
    if (!ReadSet::fromFile(path, minLen, himem != 0, h->set, g_err)) {
        delete h;
        return nullptr;
    }
    return h;
}
void dph_reads_free(void* h) { delete (ReadsH*)h; }
int64_t dph_reads_count(void* h) { return (int64_t)((ReadsH*)h)->set.size(); }
void dph_reads_get_ignore(void* h, uint8_t* out) {
    auto& ig = ((ReadsH*)h)->set.ignore;
    memcpy(out, ig.data(), ig.size());
}
void dph_reads_reset_ignore(void* h) {
    auto& ig = ((ReadsH*)h)->set.ignore;
    std::fill(ig.begin(), ig.end(), 0);
}
int64_t dph_reads_total_bases(void* h) { return (int64_t)((ReadsH*)h)->set.bases.size(); }

static OverlapParams paramsFrom(const int64_t* params, double minHits) {
    OverlapParams p;
    p.overlapSize = params[0];
    p.k = (int)params[1];
    p.numSeeds = (int)params[2];
    p.seedBatchSize = params[3];
    p.chunkSize = params[4];
    p.queryBatchSize = params[5];
    p.himem = (params[6] & 1) != 0;
    p.queryType = (int)(params[6] >> 8) ? (int)(params[6] >> 8) : 1;  // bits 8.. of the himem word: overlap.Query* flags
    p.minHits = minHits;
    return p;
}

// The command in two halves, so that a caller can keep the reads resident and run (or time) whole jobs on them:
// dph_overlap_open = device context + the reads uploaded and packed; dph_overlap_init = everything `downpore overlap`
// does between "Counting all k-mers" and its first round (value table, k-mer position index, executor slots, planner);
// dph_overlap_reset = back to the state after dph_overlap_open (the job's resident tables are released).
void* dph_overlap_open(void* reads, int device) {
    OverlapH* h = new OverlapH();
    ReadSet& rs = ((ReadsH*)reads)->set;
    h->reads = &rs;
    const double tc0 = now();
    int rc = dp_ctx_create(device, &h->ctx);
    if (rc != 0) {
        g_err = dp_last_error(nullptr);
        delete h;
        return nullptr;
    }
    const double tc1 = now();
    rc = dp_reads_upload(h->ctx, (const uint8_t*)rs.bases.data(), rs.off.data(), (uint32_t)rs.size());
    h->tCtx = tc1 - tc0;
    h->tUpload = now() - tc1;
    if (g_prof.on) fprintf(stderr, "[setup] context %.1f ms, upload + pack %.1f ms\n", 1e3 * h->tCtx, 1e3 * h->tUpload);
    if (rc == 0 && rs.isFastq && !rs.qual.empty()) {
        // FASTQ: the selection kernels weight values by the quality bytes (seeds.go:99-101).  Once per read set, here - the bytes
        // belong to the reads, not to a job, and dp_quality_upload refuses a context that already lends its reads to others
        // (the contexts a reset() keeps for the handle's next job do)
        rc = dp_quality_upload(h->ctx, (const uint8_t*)rs.qual.data(), rs.off.data(), rs.hasQual.data(), (uint32_t)rs.size());
        if (rc == 0) h->run.qualityCtx = h->ctx;
    }
    if (rc != 0) {
        g_err = dp_last_error(h->ctx);
        dp_ctx_destroy(h->ctx);
        delete h;
        return nullptr;
    }
    return h;
}
// params: overlapSize,k,numSeeds,seedBatchSize,chunkSize,queryBatchSize,himem,nSlots
int dph_overlap_init(void* hh, const int64_t* params, double minHits, const double* valuesOrNull) {
    OverlapH* h = (OverlapH*)hh;
    const double t0 = now();
    int rc = h->run.init(h->ctx, h->reads, paramsFrom(params, minHits), valuesOrNull, (int)params[7]);
    h->tInit = now() - t0;
    if (rc != 0) h->err = h->run.error.empty() ? dp_last_error(h->ctx) : h->run.error;
    return rc;
}
int dph_overlap_reset(void* hh) {
    OverlapH* h = (OverlapH*)hh;
    h->run.shutdown(true);  // (the slots' and the planner's contexts serve the handle's next job)
    TextJobBuffers::giveTexts(h->pafChunks);  // (the rounds' text buffers serve the next job's rounds)
    h->pafChunks.clear();
    h->allPafJoined.clear();
    h->lastStepCopy.clear();
    h->lastStepHasText = h->lastStepInChunks = false;
    std::fill(h->reads->ignore.begin(), h->reads->ignore.end(), 0);
    int rc = dp_scan_release(h->ctx);
    if (rc != 0) h->err = dp_last_error(h->ctx);
    return rc;
}
// out: seconds spent creating the context, uploading + packing the reads, and in the last dph_overlap_init
void dph_overlap_setup_times(void* hh, double* out) {
    OverlapH* h = (OverlapH*)hh;
    out[0] = h->tCtx;
    out[1] = h->tUpload;
    out[2] = h->tInit;
}
void* dph_overlap_create(void* reads, int device, const int64_t* params, double minHits, const double* valuesOrNull) {
    void* hh = dph_overlap_open(reads, device);
    if (!hh) return nullptr;
    if (dph_overlap_init(hh, params, minHits, valuesOrNull) != 0) {
        OverlapH* h = (OverlapH*)hh;
        g_err = h->err;
        h->run.shutdown();
        dp_ctx_destroy(h->ctx);
        delete h;
        return nullptr;
    }
    return hh;
}
void dph_overlap_destroy(void* hh) {
    OverlapH* h = (OverlapH*)hh;
    if (!h) return;
    h->run.shutdown();
    if (h->ctx) dp_kindex_set_comm(h->ctx, nullptr);
    if (h->comm) dp_comm_destroy(h->comm);
    for (dp_comm* c : h->slotComms) dp_comm_destroy(c);
    if (h->xctx) dp_ctx_destroy(h->xctx);
    dp_ctx_destroy(h->ctx);
    delete h->trimmed;
    delete h;
}
void dph_overlap_set_shard(void* hh, int64_t lo, int64_t hi) {
    OverlapH* h = (OverlapH*)hh;
    h->run.shardLo = (size_t)lo;
    h->run.shardHi = (size_t)hi;
}
const double* dph_overlap_values(void* hh, int64_t* n) {
    OverlapH* h = (OverlapH*)hh;
    const double* v = h->run.fullValues();
    *n = (int64_t)h->run.values.size();
    return v;
}
// 1 = a round was prepared and the local shard scanned; 0 = no more rounds; <0 error
int dph_overlap_round_scan(void* hh) {
    OverlapH* h = (OverlapH*)hh;
    int rc = h->run.roundPrepareAndScan();
    if (rc < 0) h->err = h->run.error;
    return rc;
}
void dph_overlap_local(void* hh, const uint32_t** read, const uint32_t** nseeds, const uint64_t** segoff,
                       const int32_t** segs, uint64_t* n, uint64_t* nsegs) {
    Survivors& s = ((OverlapH*)hh)->run.local();
    *read = s.read.data();
    *nseeds = s.n_seeds.data();
    *segoff = s.seg_off.data();
    *segs = s.segData();
    *n = s.read.size();
    *nsegs = s.segCount();
}
// survivors == all ranks' lists concatenated in rank order (read ids ascending); read == NULL: use the local list
int dph_overlap_round_finish(void* hh, const uint32_t* read, const uint32_t* nseeds, const int32_t* segs, uint64_t n) {
    OverlapH* h = (OverlapH*)hh;
    int rc;
    if (!read) {
        rc = h->run.roundFinish(h->run.local());
    } else {
        Survivors all;
        all.read.assign(read, read + n);
        all.n_seeds.assign(nseeds, nseeds + n);
        all.seg_off.assign(1, 0);
        uint64_t pos = 0;
        for (uint64_t i = 0; i < n; i++) {
            pos += 2ull * nseeds[i] + 1;
            all.seg_off.push_back(pos);
        }
        all.segsView = segs;  // the caller's gathered array outlives the call
        all.segsViewLen = pos;
        rc = h->run.roundFinish(all);
    }
    if (rc < 0) h->err = h->run.error;
    else h->addPaf(h->run.paf);
    return rc;
}
// ---- multi-GPU with the exchange inside the library (dp_comm): RCCL across processes, or in-process peers
int dph_comm_unique_id(uint8_t* id128) { return dp_comm_unique_id(id128); }
int dph_overlap_comm_init(void* hh, int nRanks, int rank, const uint8_t* id128) {
    OverlapH* h = (OverlapH*)hh;
    dp_kindex_set_comm(h->ctx, nullptr);
    if (h->comm) dp_comm_destroy(h->comm);
    h->comm = nullptr;
    int rc = dp_comm_init(h->ctx, nRanks, rank, id128, &h->comm);
    if (rc != 0) h->err = dp_last_error(h->ctx);
    h->run.comm = h->comm;
    // (round 5: with a communicator in place the job's k-mer position index is built in shares, one per rank, and all-gathered over it)
    if (rc == 0) dp_kindex_set_comm(h->ctx, h->comm);
    return rc;
}
int dph_overlap_comm_init_local(void** handles, int n) {
    std::vector<dp_ctx*> ctxs;
    for (int i = 0; i < n; i++) ctxs.push_back(((OverlapH*)handles[i])->ctx);
    std::vector<dp_comm*> comms((size_t)n, nullptr);
    int rc = dp_comm_init_local(ctxs.data(), n, comms.data());
    if (rc != 0) return rc;
    for (int i = 0; i < n; i++) {
        OverlapH* h = (OverlapH*)handles[i];
        dp_kindex_set_comm(h->ctx, nullptr);
        if (h->comm) dp_comm_destroy(h->comm);
        h->comm = comms[(size_t)i];
        h->run.comm = h->comm;
        dp_kindex_set_comm(h->ctx, h->comm);
    }
    return 0;
}
// One communicator per executor slot (ids = nSlots x 128 bytes, made by rank 0 with dph_comm_unique_id and handed to every
// rank in the same order).  Call before dph_overlap_init: the slots pick their communicators up when they are created.
int dph_overlap_comm_init_slots(void* hh, int nRanks, int rank, const uint8_t* ids, int nSlots) {
    OverlapH* h = (OverlapH*)hh;
    if (!h->comm) dp_kindex_set_comm(h->ctx, nullptr);
    for (dp_comm* c : h->slotComms) dp_comm_destroy(c);
    h->slotComms.clear();
    for (int i = 0; i < nSlots; i++) {
        dp_comm* c = nullptr;
        int rc = dp_comm_init(h->ctx, nRanks, rank, ids + (size_t)i * 128, &c);
        if (rc != 0) {
            h->err = dp_last_error(h->ctx);
            return rc;
        }
        h->slotComms.push_back(c);
    }
    h->run.slotComms = h->slotComms;
    for (size_t i = 0; i < h->run.slots.size() && i < h->slotComms.size(); i++) h->run.slots[i]->comm = h->slotComms[i];
    if (!h->comm && !h->slotComms.empty()) dp_kindex_set_comm(h->ctx, h->slotComms[0]);  // (the index is built in shares over slot 0's)
    return 0;
}
int dph_overlap_comm_init_local_slots(void** handles, int n, int nSlots) {
    std::vector<dp_ctx*> ctxs;
    for (int i = 0; i < n; i++) ctxs.push_back(((OverlapH*)handles[i])->ctx);
    for (int i = 0; i < n; i++) {
        OverlapH* h = (OverlapH*)handles[i];
        if (!h->comm) dp_kindex_set_comm(h->ctx, nullptr);
        for (dp_comm* c : h->slotComms) dp_comm_destroy(c);
        h->slotComms.clear();
    }
    for (int s = 0; s < nSlots; s++) {
        std::vector<dp_comm*> comms((size_t)n, nullptr);
        int rc = dp_comm_init_local(ctxs.data(), n, comms.data());
        if (rc != 0) return rc;
        for (int i = 0; i < n; i++) ((OverlapH*)handles[i])->slotComms.push_back(comms[(size_t)i]);
    }
    for (int i = 0; i < n; i++) {
        OverlapH* h = (OverlapH*)handles[i];
        h->run.slotComms = h->slotComms;
        for (size_t j = 0; j < h->run.slots.size() && j < h->slotComms.size(); j++) h->run.slots[j]->comm = h->slotComms[j];
        if (!h->comm && !h->slotComms.empty()) dp_kindex_set_comm(h->ctx, h->slotComms[0]);
    }
    return 0;
}
// the next slots.size() rounds of this rank, executed concurrently and committed in order (collective: every rank calls it,
// from its own thread / process): rounds committed, 0 = finished, <0 error
int dph_overlap_rounds_sharded(void* hh) {
    OverlapH* h = (OverlapH*)hh;
    int rc = h->run.roundsShardedBatch();
    if (rc < 0) h->err = h->run.error;
    else h->addPaf(h->run.paf);
    return rc;
}
// one whole round of this rank (collective: every rank calls it, from its own thread / process): 1 ran, 0 finished
int dph_overlap_round_sharded(void* hh) {
    OverlapH* h = (OverlapH*)hh;
    int rc = h->run.roundSharded();
    if (rc < 0) h->err = h->run.error;
    else h->addPaf(h->run.paf);
    return rc;
}

const char* dph_overlap_round_paf(void* hh, int64_t* n) {
    OverlapH* h = (OverlapH*)hh;
    const std::string& t = h->lastStepText();
    *n = (int64_t)t.size();
    return t.data();
}
const char* dph_overlap_all_paf(void* hh, int64_t* n) {
    OverlapH* h = (OverlapH*)hh;
    const std::string& all = h->allPaf();
    *n = (int64_t)all.size();
    return all.data();
}
const char* dph_overlap_errtext(void* hh, int64_t* n) {
    OverlapH* h = (OverlapH*)hh;
    *n = (int64_t)h->run.errText.size();
    return h->run.errText.data();
}
// out[0..] t_prepare,t_scan,t_index,t_query,t_consensus,k_scan_ms,k_query_ms,k_chain_ms,scan_bases,scan_items,
// scan_bytes,query_bytes,n_queries,n_indexed,n_hits,n_matches,n_paf,n_seeds,round,badBack,emptyMatch,k_count_ms,
// k_write_ms,count_bytes,k_cons_ms,idx_rounds,idx_hits,chain_bytes
static void statsOut(OverlapH* h, const RoundStats& s, double* out);
void dph_overlap_stats(void* hh, double* out) { statsOut((OverlapH*)hh, ((OverlapH*)hh)->run.last, out); }
// the same fields summed over every committed round of the job
void dph_overlap_stats_total(void* hh, double* out) { statsOut((OverlapH*)hh, ((OverlapH*)hh)->run.total, out); }
static void statsOut(OverlapH* h, const RoundStats& s, double* out) {
    double v[] = {s.t_prepare, s.t_scan, s.t_index, s.t_query, s.t_consensus, s.k_scan_ms, s.k_query_ms, s.k_chain_ms,
                  (double)s.scan_bases, (double)s.scan_items, (double)s.scan_bytes, (double)s.query_bytes, (double)s.n_queries,
                  (double)s.n_indexed, (double)s.n_hits, (double)s.n_matches, (double)s.n_paf, (double)s.n_seeds,
                  (double)h->run.round, (double)h->run.badBack, (double)h->run.emptyMatch, s.k_count_ms, s.k_write_ms,
                  (double)s.count_bytes, s.k_cons_ms, (double)s.idx_rounds, (double)s.idx_hits, (double)s.chain_bytes, (double)s.timed_rounds, (double)s.gang_members, (double)s.cons_bytes, s.k_index_ms};
    static_assert(sizeof v == DPH_OVERLAP_STATS * sizeof(double), "dph_overlap_stats writes out[DPH_OVERLAP_STATS]");
    memcpy(out, v, sizeof v);
}
void* dph_overlap_ctx(void* hh) { return ((OverlapH*)hh)->ctx; }

// ---- whole round on this process (planner thread prefetches the next query batches): 1 ran, 0 finished, <0 error
int dph_overlap_step(void* hh) {
    OverlapH* h = (OverlapH*)hh;
    int rc = h->run.step();
    if (rc < 0) h->err = h->run.error;
    else {
        const double t0 = now();
        h->addPaf(h->run.paf);
        g_prof.commitKeepUs += (long long)((now() - t0) * 1e6);
    }
    return rc;
}
// step() stops committing at round n (tests that compare the first n rounds with a fixture); -1 lifts the limit
void dph_overlap_set_round_limit(void* hh, int64_t n) { ((OverlapH*)hh)->run.roundLimit = n; }
int64_t dph_overlap_round(void* hh) { return ((OverlapH*)hh)->run.round; }
void dph_profile_print() { profilePrint(); }
// Buffers the library keeps between jobs so that a handle's next job need not map and zero-fill them again (PAF text strings and
// record arrays: up to 512 MB; window-cache chunks: up to 16 x 11.5 MB; the map command's staging block: ~400 MB at config 3)
// go back to the allocator.  Safe at any time (a running job simply allocates again); returns the bytes released.
int64_t dph_release_caches() {
    return (int64_t)(TextJobBuffers::releaseAll() + WindowCache::releaseSpares() + releaseMapStaging()) + dp_release_device_caches();  // (round 5: + the device library's parked blocks)
}
// process-wide planner counters (tests): 0 plans computed, 1 computed plans thrown away (stale flags, or started from a wrong
// guess of where the plan before them ends), 2 finished plans erased by a commit's flags
int64_t dph_planner_counter(int which) {
    // 0 plans computed, 1 thrown away, 2 erased by flags, 3 rounds executed, 4 rejected at the commit, 5 committed, 6 microseconds in
    // plan computes (wall), 7 slots' microseconds waiting for a plan (planComputes etc. count since the process started)
    switch (which) {
        case 0: return g_prof.planComputes.load();
        case 1: return g_prof.planDiscarded.load();
        case 2: return g_prof.planErased.load();
        case 3: return g_prof.executed.load();
        case 4: return g_prof.rejected.load();
        case 5: return g_prof.committed.load();
        case 6: return g_prof.planUs.load();
        case 7: return g_prof.getWaitUs.load();
        case 8: return g_prof.commitWaitUs.load();   // the committing thread (whoever calls dph_overlap_step): waiting for the next round in order,
        case 9: return g_prof.commitTextUs.load();   // ... joining its text,
        case 10: return g_prof.commitStateUs.load();  // ... flags + planner bookkeeping,
        case 11: return g_prof.commitKeepUs.load();   // ... keeping the step's text for dph_overlap_all_paf
        case 12: return g_prof.formatUs.load();       // formatter threads: time in TextJob::format, all threads together
        case 13: return g_prof.textWaitUs.load();
        case 14: return g_prof.planLanes.load();     // lanes of the planner that was given lanes last (not a sum: bench.py reports it as is)     // the committing thread's share of `text` spent waiting for a formatter thread
        default: return -1;
    }
}
int64_t dph_overlap_step_lines(void* hh) { return ((OverlapH*)hh)->run.pafLines; }  // PAF lines of the last step
// discards the executor pipeline's in-flight rounds (they are re-executed): a timed region then starts from an empty pipeline
void dph_overlap_drain(void* hh) { ((OverlapH*)hh)->run.drain(); }

// ---- round-parallel mode: a rank executes ONE round speculatively and serialises the result; every rank then commits
// the gathered results in round order with the speculation check (OverlapRun::commitResults).
static void putv(std::string& b, const void* p, size_t n) { b.append((const char*)p, n); }
// text (may be null): the record's PAF text goes there instead of into the record (hdr[17] = 1, hdr[7] still says how long it is):
// the control part - a few KB per round - is all-gathered, the text travels to the printing rank alone (dp_gather_blobs)
static void serialise(RoundResult& res, std::string& blob, std::string* text = nullptr) {
    res.takeText();  // (the PAF text may still be with a formatter thread)
    int64_t hdr[18] = {res.round, res.empty ? 1 : 0, res.firstIn, res.firstOut, res.numQuerySeqs, (int64_t)res.ignores.size(),
                       (int64_t)res.indexedReads.size(), (int64_t)res.paf.size(), res.fs.badBack, res.fs.emptyMatch,
                       (int64_t)res.fs.lines, (int64_t)res.fs.hits, (int64_t)res.fs.qHits, 0, res.snapshot,
                       (int64_t)res.queryReads.size(), res.planRound, text ? 1 : 0};
    int64_t total = (int64_t)(sizeof hdr + sizeof(RoundStats) + res.ignores.size() * sizeof(int) + res.indexedReads.size() * 4 +
                              (text ? 0 : res.paf.size()) + res.queryReads.size() * 4);
    hdr[13] = total;
    putv(blob, hdr, sizeof hdr);
    putv(blob, &res.st, sizeof(RoundStats));
    putv(blob, res.ignores.data(), res.ignores.size() * sizeof(int));
    putv(blob, res.indexedReads.data(), res.indexedReads.size() * 4);
    if (text)
        text->append(res.paf);
    else
        putv(blob, res.paf.data(), res.paf.size());
    putv(blob, res.queryReads.data(), res.queryReads.size() * 4);
}
// Executes rounds first, first+1, ... (one per executor slot of this process, concurrently) and returns their
// serialised results back to back (each record carries its own length in hdr[13]).
const uint8_t* dph_overlap_exec_round(void* hh, int64_t first, uint64_t* n) {
    OverlapH* h = (OverlapH*)hh;
    static thread_local std::string blob;
    std::vector<i64> rounds;
    for (size_t i = 0; i < h->run.slots.size(); i++) rounds.push_back(first + (i64)i);
    std::vector<RoundResult> outs;
    int rc = h->run.executeRounds(rounds, outs);
    if (rc < 0) {
        h->err = h->run.error;
        *n = 0;
        return nullptr;
    }
    blob.clear();
    for (RoundResult& r : outs) serialise(r, blob);
    *n = blob.size();
    return (const uint8_t*)blob.data();
}
int dph_overlap_slots(void* hh) { return (int)((OverlapH*)hh)->run.slots.size(); }
// blobs: concatenation; sizes[i] bytes each.  Returns the number of rounds committed (0..count) or <0.
// textSizes (may be null): per rank, the bytes of text its records announce but do not carry (hdr[17] = 1); the records' own
// lengths go to textLen in the order the records appear
static void deserialise(const uint8_t* blobs, const uint64_t* sizes, int count, std::vector<RoundResult>& rs, bool keepText = true,
                        std::vector<uint64_t>* textSizes = nullptr, std::vector<uint64_t>* textLen = nullptr) {
    uint64_t totalBytes = 0;
    for (int i = 0; i < count; i++) totalBytes += sizes[i];
    const uint8_t* q = blobs;
    const uint8_t* end = blobs + totalBytes;
    if (textSizes) textSizes->assign((size_t)count, 0);
    int rankOf = 0;
    uint64_t rankEnd = count ? sizes[0] : 0;
    while (q < end) {
        while (rankOf + 1 < count && (uint64_t)(q - blobs) >= rankEnd) rankEnd += sizes[++rankOf];
        const uint8_t* rec = q;
        int64_t hdr[18];
        memcpy(hdr, q, sizeof hdr);
        q += sizeof hdr;
        RoundResult r;
        r.round = hdr[0];
        r.empty = hdr[1] != 0;
        r.firstIn = hdr[2];
        r.firstOut = hdr[3];
        r.numQuerySeqs = hdr[4];
        memcpy(&r.st, q, sizeof(RoundStats));
        q += sizeof(RoundStats);
        r.ignores.assign((const int*)q, (const int*)q + hdr[5]);
        q += hdr[5] * sizeof(int);
        r.indexedReads.assign((const uint32_t*)q, (const uint32_t*)q + hdr[6]);
        q += hdr[6] * 4;
        if (hdr[17]) {  // the text travels on its own
            if (textSizes) (*textSizes)[(size_t)rankOf] += (uint64_t)hdr[7];
            if (textLen) textLen->push_back((uint64_t)hdr[7]);
        } else {
            if (keepText) r.paf.assign((const char*)q, (size_t)hdr[7]);  // (a rank that prints nothing keeps the counts, not the text)
            q += hdr[7];
            if (textLen) textLen->push_back(0);
        }
        r.snapshot = hdr[14];
        r.planRound = hdr[16];
        r.queryReads.assign((const uint32_t*)q, (const uint32_t*)q + hdr[15]);
        r.fs.badBack = hdr[8];
        r.fs.emptyMatch = hdr[9];
        r.fs.lines = (uint64_t)hdr[10];
        r.fs.hits = (uint64_t)hdr[11];
        r.fs.qHits = (uint64_t)hdr[12];
        rs.push_back(std::move(r));
        q = rec + hdr[13];
    }
}

// ---- pipelined round-parallel mode: rank `rank` of `world` owns the rounds r % world == rank
void dph_overlap_set_ranks(void* hh, int rank, int world) { ((OverlapH*)hh)->run.setRanks(rank, world); }
// serialised results of this rank's contribution to the current superstep: its next owned round (blocks until its executor
// pipeline has it) and up to max_rounds - 1 finished owned rounds after it, back to back (each record carries its length)
const uint8_t* dph_overlap_wait_owned_many(void* hh, int max_rounds, uint64_t* n) {
    OverlapH* h = (OverlapH*)hh;
    static thread_local std::string blob;
    std::vector<RoundResult> res;
    int rc = h->run.waitOwned(res, max_rounds);
    if (rc != 0) {
        h->err = h->run.error;
        *n = 0;
        return nullptr;
    }
    blob.clear();
    for (RoundResult& r : res) serialise(r, blob);
    *n = blob.size();
    return (const uint8_t*)blob.data();
}
const uint8_t* dph_overlap_wait_owned(void* hh, uint64_t* n) { return dph_overlap_wait_owned_many(hh, 1, n); }
int dph_overlap_commit_gathered(void* hh, const uint8_t* blobs, const uint64_t* sizes, int count) {
    OverlapH* h = (OverlapH*)hh;
    std::vector<RoundResult> rs;
    deserialise(blobs, sizes, count, rs, h->keepText);
    int c = h->run.commitGathered(rs);
    if (c >= 0) h->addPaf(h->run.paf);
    return c;
}

// One superstep of the round-parallel layout with the exchange inside the library (dp_allgather_blobs on the communicator of
// dph_overlap_comm_init / _comm_init_local): this rank's next owned round and up to max_rounds - 1 finished ones after it,
// all-gathered, committed in round order on every rank.  Collective.  Returns the rounds committed (0 = the superstep's first
// round was rejected and is executed again; call dph_overlap_done to learn whether the command is finished), < 0 on error.
int dph_overlap_superstep(void* hh, int max_rounds) {
    OverlapH* h = (OverlapH*)hh;
    if (!h->comm) {
        h->err = "dph_overlap_superstep without a communicator (dph_overlap_comm_init)";
        return -1;
    }
    if (!h->xctx && dp_ctx_create_shared(h->ctx, &h->xctx) != 0) {
        h->err = dp_last_error(nullptr);
        return -1;
    }
    std::vector<RoundResult> res;
    int rc = h->run.waitOwned(res, max_rounds);
    if (rc != 0) {
        h->err = h->run.error;
        dp_comm_abort(h->comm);  // (the peers must not wait for this rank's contribution)
        return rc < 0 ? rc : -1;
    }
    static thread_local std::string blob, text;
    blob.clear();
    text.clear();
    const bool split = h->textRoot >= 0;
    for (RoundResult& r : res) serialise(r, blob, split ? &text : nullptr);
    const uint8_t* all = nullptr;
    const uint64_t* sizes = nullptr;
    rc = dp_allgather_blobs(h->comm, h->xctx, (const uint8_t*)blob.data(), blob.size(), &all, &sizes);
    if (rc != 0) {
        h->err = dp_last_error(h->xctx);
        return rc;
    }
    std::vector<RoundResult> rs;
    std::vector<uint64_t> textSizes, textLen;
    deserialise(all, sizes, dp_comm_size(h->comm), rs, h->keepText, &textSizes, &textLen);
    if (split) {
        // the rounds' text: to the printing rank alone.  Every rank knows every rank's text length from the control records.
        const uint8_t* allText = nullptr;
        rc = dp_gather_blobs(h->comm, h->xctx, (const uint8_t*)text.data(), text.size(), textSizes.data(), h->textRoot, &allText);
        if (rc != 0) {
            h->err = dp_last_error(h->xctx);
            return rc;
        }
        if (allText && h->keepText) {
            const char* t = (const char*)allText;
            for (size_t i = 0; i < rs.size(); i++) {
                rs[i].paf.assign(t, (size_t)textLen[i]);
                t += textLen[i];
            }
        }
    }
    const int c = h->run.commitGathered(rs);
    if (c >= 0) h->addPaf(h->run.paf);
    return c;
}

int dph_overlap_commit_blobs(void* hh, const uint8_t* blobs, const uint64_t* sizes, int count) {
    OverlapH* h = (OverlapH*)hh;
    std::vector<RoundResult> rs;
    deserialise(blobs, sizes, count, rs, h->keepText);
    std::sort(rs.begin(), rs.end(), [](const RoundResult& a, const RoundResult& b) { return a.round < b.round; });
    int c = h->run.commitResults(rs);
    if (c >= 0) h->addPaf(h->run.paf);
    return c;
}
int dph_overlap_done(void* hh) { return ((OverlapH*)hh)->run.done ? 1 : 0; }
// Multi-rank runs: a rank that does not print the PAF (every rank but the one that writes the output) need not keep the other
// ranks' text - the gathered rounds are committed with their counts, flags and read lists, the text is dropped as it arrives
// (at 8 ranks every rank would otherwise copy all 235 MB of a config-2 job's PAF three times).  keep != 0 (default): as before.
void dph_overlap_keep_text(void* hh, int keep) { ((OverlapH*)hh)->keepText = keep != 0; }
// dph_overlap_superstep: root >= 0 = the rounds' PAF text is gathered to rank `root` alone (dp_gather_blobs) and only their control
// records - a few KB per round - are all-gathered; every rank of the job must say the same.  -1 (default): text and control records
// travel together to every rank, as before (what a caller needs that reads the PAF on every rank).
void dph_overlap_text_root(void* hh, int root) { ((OverlapH*)hh)->textRoot = root; }

}  // extern "C"

// ---- `downpore map` ------------------------------------------------------------------------------------------------
// params: circular,k,querySize,minLength,chunkSize,seedRate[,index layout[,all sequences]].  Returns a handle holding paf/err text, or NULL.
namespace {
struct MapH {
    std::string paf, err;
    MapStats st;
};
}  // namespace
namespace {
// the parameter block of dph_map_run_ex and dph_map_run_trim (6, 7 or 8 values); false with g_err set, before any device call
bool mapParamsFrom(const char* who, bool handles, const int64_t* params, int n_params, MapParams& p) {
    if (!handles || !params || n_params < 6 || n_params > 8) {
        g_err = std::string(who) + ": bad arguments (6, 7 or 8 parameters)";
        return false;
    }
    if (n_params >= 7 && (params[6] < 0 || params[6] > 2)) {
        g_err = std::string(who) + ": index layout " + std::to_string((long long)params[6]) + " (0 = auto, 1 = dense, 2 = sparse)";
        return false;
    }
    if (n_params == 8 && params[7] != 0 && params[7] != 1) {
        g_err = std::string(who) + ": all sequences " + std::to_string((long long)params[7]) + " (0 = the first sequence of the reference, 1 = all of them)";
        return false;
    }
    p.indexLayout = n_params >= 7 ? (int)params[6] : 0;
    p.allSequences = n_params == 8 && params[7] == 1;
    p.circular = params[0] != 0;
    p.k = (int)params[1];
    p.querySize = params[2];
    p.minLength = params[3];
    p.chunkSize = params[4];
    p.seedRate = params[5];
    return true;
}
}  // namespace
extern "C" void* dph_map_run_ex(void* refH, void* readsH, const int64_t* params, int n_params, int device) {
    MapParams p;
    if (!mapParamsFrom("dph_map_run_ex", refH && readsH, params, n_params, p)) return nullptr;
    MapH* h = new MapH();
    std::string error;
    int rc = runMap(((ReadsH*)refH)->set, ((ReadsH*)readsH)->set, p, device, h->paf, h->err, &h->st, error);
    if (rc != 0) {
        g_err = error;
        delete h;
        return nullptr;
    }
    return h;
}
extern "C" void* dph_map_run(void* refH, void* readsH, const int64_t* params, int device) {
    return dph_map_run_ex(refH, readsH, params, 6, device);
}
extern "C" void dph_map_free(void* h) { delete (MapH*)h; }
extern "C" const char* dph_map_paf(void* h, int64_t* n) {
    *n = (int64_t)((MapH*)h)->paf.size();
    return ((MapH*)h)->paf.data();
}
extern "C" const char* dph_map_errtext(void* h, int64_t* n) {
    *n = (int64_t)((MapH*)h)->err.size();
    return ((MapH*)h)->err.data();
}
// ---- a mapper: dph_map_run_ex's reference side once, its read side per batch
namespace {
struct MapperH {
    Mapper* m = nullptr;
    std::atomic<bool> busy{false};
    ~MapperH() {
        if (m) mapperClose(m);
    }
};
}  // namespace
extern "C" void* dph_mapper_open(void* refH, const int64_t* params, int n_params, int device) {
    MapParams p;
    if (!mapParamsFrom("dph_mapper_open", refH != nullptr, params, n_params, p)) return nullptr;
    std::string error;
    int rc = 0;
    Mapper* m = mapperOpen(((ReadsH*)refH)->set, p, device, error, &rc);
    if (!m) {
        g_err = error;
        return nullptr;
    }
    MapperH* h = new MapperH();
    h->m = m;
    return h;
}
extern "C" void* dph_mapper_map(void* mapperH, void* readsH) {
    MapperH* mh = (MapperH*)mapperH;
    if (!mh || !readsH) {
        g_err = "dph_mapper_map: bad arguments";
        return nullptr;
    }
    if (mh->busy.exchange(true)) {
        g_err = "dph_mapper_map: DP_ERR_STATE: another call is mapping on this mapper (one batch at a time per mapper)";
        return nullptr;
    }
    MapH* h = new MapH();
    std::string error;
    const int rc = mapperMap(mh->m, ((ReadsH*)readsH)->set, h->paf, h->err, &h->st, error);
    mh->busy.store(false);
    if (rc != 0) {
        g_err = error;
        delete h;
        return nullptr;
    }
    return h;
}
extern "C" void dph_mapper_close(void* mapperH) { delete (MapperH*)mapperH; }

// out: n_chunks,n_seeds,n_windows,n_chains,n_batches,k_scan_ms,k_map_ms
extern "C" void dph_map_stats(void* h, double* out) {
    const MapStats& s = ((MapH*)h)->st;
    double v[] = {(double)s.n_chunks, (double)s.n_seeds, (double)s.n_windows, (double)s.n_chains, (double)s.n_batches, s.k_scan_ms,
                  s.k_map_ms, s.t_setup_s, s.t_scan_s, s.t_chain_s, s.t_host_s, s.map_bytes, s.scan_bytes};
    static_assert(sizeof v == DPH_MAP_STATS * sizeof(double), "dph_map_stats writes out[DPH_MAP_STATS]");
    memcpy(out, v, sizeof v);
}

// out: layout, index bytes, dense estimate, device total memory, seed hits, contexts that built an index, queries per regime (4)
extern "C" int dph_map_index_info(void* h, int64_t* out, int cap) {
    const MapStats& s = ((MapH*)h)->st;
    const int64_t v[] = {s.index_layout, s.index_bytes, s.dense_estimate, s.device_total, s.hits, s.index_builds,
                         s.regimes[0], s.regimes[1], s.regimes[2], s.regimes[3]};
    const int n = std::max(0, std::min(cap, (int)(sizeof v / sizeof v[0])));
    memcpy(out, v, (size_t)n * sizeof(int64_t));
    return n;
}

// ---- `downpore trim`, edge stage -----------------------------------------------------------------------------------
// params: k, check_reads, adapter_threshold, extra_end_trim, tag_adapters, require_pairs, determine_adapters, verbosity
namespace {
struct TrimH {
    ReadSet* reads = nullptr;
    TrimResult res;
    std::string adapters;
};
bool trimParamsFrom(const int64_t* params, int n, TrimParams& p) {
    if (!params || (n != 8 && n != 14)) return false;
    if (n == 14) {  // the middle stage's six follow the edge stage's eight
        p.middle = params[8] != 0;
        p.chunkSize = params[9];
        p.middleThreshold = (int)params[10];
        p.extraMiddleTrim = (int)params[11];
        p.discardMiddle = params[12] != 0;
        p.flushSeeds = params[13];
    }
    p.k = (int)params[0];
    p.checkReads = params[1];
    p.adapterThreshold = (int)params[2];
    p.extraEdgeTrim = (int)params[3];
    p.tagAdapters = params[4] != 0;
    p.requirePairs = params[5] != 0;
    p.determineAdapters = params[6] != 0;
    p.verbosity = (int)params[7];
    return true;
}
}  // namespace
extern "C" void* dph_trim_run(void* readsH, void* frontH, void* backH, const int64_t* params, int n_params, int device) {
    TrimParams p;
    if (!readsH || !frontH || !backH || !trimParamsFrom(params, n_params, p)) {
        g_err = "dph_trim_run: bad arguments (8 parameters, or 14 with the middle stage's)";
        return nullptr;
    }
    TrimH* h = new TrimH();
    h->reads = &((ReadsH*)readsH)->set;
    std::string error;
    if (runTrim(*h->reads, ((ReadsH*)frontH)->set, ((ReadsH*)backH)->set, p, device, h->res, error) != 0) {
        g_err = error;
        delete h;
        return nullptr;
    }
    return h;
}
extern "C" void* dph_trim_apply(void* readsH, void* frontH, void* backH, const int64_t* params, int n_params, const uint8_t* enabled,
                                const int32_t* recs, int64_t n_rec_reads, const uint64_t* counts) {
    TrimParams p;
    if (!readsH || !frontH || !backH || !trimParamsFrom(params, n_params, p) || n_rec_reads < 0 || (n_rec_reads && !recs) || !counts) {
        g_err = "dph_trim_apply: bad arguments (8 parameters)";
        return nullptr;
    }
    static_assert(sizeof(dp_trim_rec) == 6 * sizeof(int32_t), "edge records are six int32");
    TrimH* h = new TrimH();
    h->reads = &((ReadsH*)readsH)->set;
    std::string error;
    if (applyTrim(*h->reads, ((ReadsH*)frontH)->set, ((ReadsH*)backH)->set, p, enabled, (const dp_trim_rec*)recs, (size_t)n_rec_reads, counts, nullptr,
                  h->res, error) != 0) {
        g_err = error;
        delete h;
        return nullptr;
    }
    return h;
}
// dph_trim_apply with the middle stage (params[14], middle != 0): seed_counts[n_chunks] per planned chunk and mid_recs = six int32 per
// match that passed the identity test (adapter, chunk, ordinal, start_rel, covered, chain length), in any order
extern "C" void* dph_trim_apply_mid(void* readsH, void* frontH, void* backH, const int64_t* params, int n_params, const uint8_t* enabled,
                                    const int32_t* recs, int64_t n_rec_reads, const uint64_t* counts, const int32_t* seed_counts, int64_t n_chunks,
                                    const int32_t* mid_recs, int64_t n_mid_recs) {
    TrimParams p;
    if (!readsH || !frontH || !backH || !trimParamsFrom(params, n_params, p) || n_params != 14 || n_rec_reads < 0 || (n_rec_reads && !recs) || !counts ||
        n_chunks < 0 || (n_chunks && !seed_counts) || n_mid_recs < 0 || (n_mid_recs && !mid_recs)) {
        g_err = "dph_trim_apply_mid: bad arguments (14 parameters)";
        return nullptr;
    }
    static_assert(sizeof(TrimMidRec) == 6 * sizeof(int32_t), "middle records are six int32");
    TrimH* h = new TrimH();
    h->reads = &((ReadsH*)readsH)->set;
    std::string error;
    TrimMidInput mid;
    mid.seedCounts = seed_counts;
    mid.nChunks = (size_t)n_chunks;
    mid.recs = (const TrimMidRec*)mid_recs;
    mid.nRecs = (size_t)n_mid_recs;
    if (applyTrim(*h->reads, ((ReadsH*)frontH)->set, ((ReadsH*)backH)->set, p, enabled, (const dp_trim_rec*)recs, (size_t)n_rec_reads, counts, &mid,
                  h->res, error) != 0) {
        g_err = error;
        delete h;
        return nullptr;
    }
    return h;
}
// the chunk loop of trim.go:165-184 for one served length: out[3 i ..] = start, end, is-remainder; returns the number of chunks, -1: chunk_size <= 100
extern "C" int64_t dph_trim_chunk_plan(int64_t length, int64_t chunk_size, int32_t* out, int64_t cap) {
    if (chunk_size <= 100) {
        g_err = "trim: -chunk_size must be larger than 100 (the chunks advance by chunk_size - 100 bases)";
        return -1;
    }
    std::vector<TrimChunk> plan;
    trimChunkPlan(length, chunk_size, 0, plan);
    for (size_t i = 0; i < plan.size() && (int64_t)i < cap; i++) {
        out[3 * i] = plan[i].start;
        out[3 * i + 1] = plan[i].end;
        out[3 * i + 2] = plan[i].remainder;
    }
    return (int64_t)plan.size();
}
// which: 0 the chunk plan (6 per chunk: read, start, end, remainder, seeds, indexed), 1 the splits (4 each: read, aEnd, bStart, kept
// halves), 2 the applied records (6 each); returns the number of int32 (out may be NULL)
extern "C" int64_t dph_trim_mid_ints(void* h, int which, int32_t* out, int64_t cap) {
    const TrimResult& r = ((TrimH*)h)->res;
    const std::vector<int32_t>& v = which == 0 ? r.plan : which == 1 ? r.splits : r.applied;
    if (out) memcpy(out, v.data(), (size_t)std::min<int64_t>(cap, (int64_t)v.size()) * sizeof(int32_t));
    return (int64_t)v.size();
}
// the names of the halves added for split reads, one per line, in the order added (their sequences close dph_trim_output's text)
extern "C" const char* dph_trim_extras(void* h, int64_t* n) {
    TrimH* t = (TrimH*)h;
    t->adapters.clear();
    for (const std::string& s : t->res.extraNames) t->adapters += s + "\n";
    *n = (int64_t)t->adapters.size();
    return t->adapters.data();
}
// out[DPH_TRIM_MID_STATS]: chunks, seeds, batches, candidate pairs, records applied, overflow pairs, out-of-range halves, upload / scan / index / query /
// kernel ms
extern "C" void dph_trim_mid_stats(void* h, double* out) {
    const TrimResult& r = ((TrimH*)h)->res;
    const double v[] = {(double)r.midChunks, (double)r.midSeeds, (double)r.midBatches, (double)r.midPairs, (double)r.midRecords, (double)r.midOverflowPairs,
                          (double)r.midOutOfRange, r.mid_upload_ms, r.mid_scan_ms, r.mid_index_ms, r.mid_query_ms, r.mid_kernel_ms};
    static_assert(sizeof v == DPH_TRIM_MID_STATS * sizeof(double), "dph_trim_mid_stats writes out[DPH_TRIM_MID_STATS]");
    memcpy(out, v, sizeof v);
}
extern "C" void dph_trim_free(void* h) { delete (TrimH*)h; }
// the read set the run's output gives when it is read back with minimum length min_len (ReadSet::addLine's rule), without the text: a
// reads handle of the caller's (dph_reads_free).  Needs no device: works on the handles of dph_trim_apply / _apply_mid too.
extern "C" void* dph_trim_reads(void* h, int64_t min_len, int himem) {
    TrimH* t = (TrimH*)h;
    if (!t || !t->reads) {
        g_err = "dph_trim_reads: bad arguments";
        return nullptr;
    }
    ReadsH* out = new ReadsH();
    std::vector<dp_read_span> spans;
    trimmedReadSet(*t->reads, t->res, min_len, himem != 0, out->set, spans);
    return out;
}
// `overlap -trim true`: the reads go up once, both trim stages run on the resident copy, the trimmed read set (min_len: overlap_size) is cut
// from it on the device and the handle that comes back runs the job on it.  *trim_out: the trim run's handle (log, table, stats).
extern "C" void* dph_overlap_open_trim(void* reads, void* front, void* back, const int64_t* trim_params, int n_params, int64_t min_len, int device,
                                       void** trim_out) {
    if (trim_out) *trim_out = nullptr;
    TrimParams p;
    if (!reads || !front || !back || !trim_out || !trimParamsFrom(trim_params, n_params, p)) {
        g_err = "dph_overlap_open_trim: bad arguments (8 trim parameters, or 14 with the middle stage's)";
        return nullptr;
    }
    ReadSet& raw = ((ReadsH*)reads)->set;
    OverlapH* h = new OverlapH();
    TrimH* th = new TrimH();
    th->reads = &raw;
    auto fail = [&](const std::string& why) -> void* {
        g_err = why;
        if (h->ctx) dp_ctx_destroy(h->ctx);
        delete h->trimmed;
        delete h;
        delete th;
        return nullptr;
    };
    const double tc0 = now();
    if (dp_ctx_create(device, &h->ctx) != 0) return fail(dp_last_error(nullptr));
    const double tc1 = now();
    if (dp_reads_upload(h->ctx, (const uint8_t*)raw.bases.data(), raw.off.data(), (uint32_t)raw.size()) != 0) return fail(dp_last_error(h->ctx));
    const double tc2 = now();
    std::string error;
    if (runTrim(raw, ((ReadsH*)front)->set, ((ReadsH*)back)->set, p, device, th->res, error, h->ctx) != 0) return fail(error);
    const double tc3 = now();
    h->trimmed = new ReadsH();
    std::vector<dp_read_span> spans;
    trimmedReadSet(raw, th->res, min_len, raw.himem, h->trimmed->set, spans);
    ReadSet& rs = h->trimmed->set;
    const double tc4 = now();
    int rc = dp_reads_respan(h->ctx, spans.data(), (uint32_t)spans.size());
    if (rc == 0 && rs.isFastq && !rs.qual.empty()) {
        rc = dp_quality_upload(h->ctx, (const uint8_t*)rs.qual.data(), rs.off.data(), rs.hasQual.data(), (uint32_t)rs.size());
        if (rc == 0) h->run.qualityCtx = h->ctx;
    }
    if (rc != 0) return fail(dp_last_error(h->ctx));
    h->reads = &rs;
    h->tCtx = tc1 - tc0;
    h->tUpload = (tc2 - tc1) + (now() - tc4);
    if (g_prof.on)
        fprintf(stderr, "[setup] context %.1f ms, upload + pack %.1f ms, trim on resident reads %.1f ms, trimmed read set %.1f ms, respan %.1f ms\n", 1e3 * h->tCtx,
                1e3 * (tc2 - tc1), 1e3 * (tc3 - tc2), 1e3 * (tc4 - tc3), 1e3 * (now() - tc4));
    *trim_out = th;
    return h;
}
// the read set a handle's jobs run on: the caller's for dph_overlap_open, the handle's own trimmed one for dph_overlap_open_trim (valid
// while the handle lives; not to be freed)
extern "C" void* dph_overlap_reads(void* hh) {
    OverlapH* h = (OverlapH*)hh;
    return h->trimmed;
}
// `map` with the trim in front: the raw reads go up once, packed; the trim runs on the resident copy; the trimmed read set (minimum length
// params[3]) is cut from it on the device with its reverse strands, and the run goes on as dph_map_run_ex does on that set.  *trim_out: the
// trim run's handle, as dph_overlap_open_trim gives it.
extern "C" void* dph_map_run_trim(void* refH, void* readsH, void* frontH, void* backH, const int64_t* trim_params, int n_trim, const int64_t* params,
                                  int n_params, int device, void** trim_out) {
    if (trim_out) *trim_out = nullptr;
    MapTrim mt;
    if (!refH || !readsH || !frontH || !backH || !trim_out || !trimParamsFrom(trim_params, n_trim, mt.params)) {
        g_err = "dph_map_run_trim: bad arguments (8 trim parameters, or 14 with the middle stage's)";
        return nullptr;
    }
    MapParams p;
    if (!mapParamsFrom("dph_map_run_trim", true, params, n_params, p)) return nullptr;
    MapH* h = new MapH();
    TrimH* th = new TrimH();
    th->reads = &((ReadsH*)readsH)->set;
    mt.raw = th->reads;
    mt.front = &((ReadsH*)frontH)->set;
    mt.back = &((ReadsH*)backH)->set;
    mt.res = &th->res;
    std::string error;
    if (runMap(((ReadsH*)refH)->set, *mt.raw, p, device, h->paf, h->err, &h->st, error, &mt) != 0) {
        g_err = error;
        delete h;
        delete th;
        return nullptr;
    }
    *trim_out = th;
    return h;
}
// dph_mapper_map with the trim in front, per batch: the raw reads go behind the mapper's resident head once, packed; both trim stages run on
// that copy; the trimmed read set (the mapper's minimum length) is cut from it on the device with its reverse strands and mapped.
// *trim_out: the trim run's handle, as dph_map_run_trim gives it.
extern "C" void* dph_mapper_map_trim(void* mapperH, void* readsH, void* frontH, void* backH, const int64_t* trim_params, int n_trim, void** trim_out) {
    if (trim_out) *trim_out = nullptr;
    MapperH* mh = (MapperH*)mapperH;
    MapTrim mt;
    if (!mh || !readsH || !frontH || !backH || !trim_out || !trimParamsFrom(trim_params, n_trim, mt.params)) {
        g_err = "dph_mapper_map_trim: bad arguments (8 trim parameters, or 14 with the middle stage's)";
        return nullptr;
    }
    if (mh->busy.exchange(true)) {
        g_err = "dph_mapper_map_trim: DP_ERR_STATE: another call is mapping on this mapper (one batch at a time per mapper)";
        return nullptr;
    }
    MapH* h = new MapH();
    TrimH* th = new TrimH();
    th->reads = &((ReadsH*)readsH)->set;
    mt.raw = th->reads;
    mt.front = &((ReadsH*)frontH)->set;
    mt.back = &((ReadsH*)backH)->set;
    mt.res = &th->res;
    std::string error;
    const int rc = mapperMap(mh->m, mt, h->paf, h->err, &h->st, error);
    mh->busy.store(false);
    if (rc != 0) {
        g_err = error;
        delete h;
        delete th;
        return nullptr;
    }
    *trim_out = th;
    return h;
}
// dph_mapper_map (no trim arguments) or dph_mapper_map_trim with NM and cg tags behind every line of the batch: align_params[0] = max_edits.
extern "C" void* dph_mapper_map_align(void* mapperH, void* readsH, void* frontH, void* backH, const int64_t* trim_params, int n_trim, void** trim_out,
                                      const int64_t* align_params, int n_align) {
    if (trim_out) *trim_out = nullptr;
    MapperH* mh = (MapperH*)mapperH;
    const bool noTrim = !frontH && !backH && !trim_params && n_trim == 0;
    MapTrim mt;
    if (!mh || !readsH || !align_params || n_align != 1 || (!noTrim && (!frontH || !backH || !trim_out || !trimParamsFrom(trim_params, n_trim, mt.params)))) {
        g_err = "dph_mapper_map_align: bad arguments (no trim: front, back and trim_params NULL and n_trim 0, else 8 or 14 trim parameters; one align parameter)";
        return nullptr;
    }
    if (align_params[0] < 1 || align_params[0] > 32768) {
        g_err = "dph_mapper_map_align: bad arguments: max_edits " + std::to_string((long long)align_params[0]) + " (1 .. 32768)";
        return nullptr;
    }
    if (mh->busy.exchange(true)) {
        g_err = "dph_mapper_map_align: DP_ERR_STATE: another call is mapping on this mapper (one batch at a time per mapper)";
        return nullptr;
    }
    MapH* h = new MapH();
    TrimH* th = noTrim ? nullptr : new TrimH();
    if (th) {
        th->reads = &((ReadsH*)readsH)->set;
        mt.raw = th->reads;
        mt.front = &((ReadsH*)frontH)->set;
        mt.back = &((ReadsH*)backH)->set;
        mt.res = &th->res;
    }
    std::string error;
    const int rc = mapperMapAlign(mh->m, &((ReadsH*)readsH)->set, th ? &mt : nullptr, align_params[0], h->paf, h->err, &h->st, error);
    mh->busy.store(false);
    if (rc != 0) {
        g_err = error;
        delete h;
        delete th;
        return nullptr;
    }
    if (th) *trim_out = th;
    return h;
}
// out: lines, aligned, over max_edits, out of range, DP cells computed, band doublings, kernel microseconds, trace-back bytes
extern "C" int dph_map_align_info(void* h, int64_t* out, int cap) {
    const MapStats& s = ((MapH*)h)->st;
    const int n = std::max(0, std::min(cap, 8));
    for (int i = 0; i < n; i++) out[i] = s.align[i];
    return n;
}
extern "C" const char* dph_trim_output(void* h, int64_t* n) {
    *n = (int64_t)((TrimH*)h)->res.out.size();
    return ((TrimH*)h)->res.out.data();
}
extern "C" const char* dph_trim_errtext(void* h, int64_t* n) {
    *n = (int64_t)((TrimH*)h)->res.errText.size();
    return ((TrimH*)h)->res.errText.data();
}
extern "C" int64_t dph_trim_table(void* h, int32_t* out, int64_t cap_reads) {
    const std::vector<int32_t>& t = ((TrimH*)h)->res.table;
    const int64_t n = std::min<int64_t>(cap_reads, (int64_t)t.size() / 5);
    if (out && n > 0) memcpy(out, t.data(), (size_t)n * 5 * sizeof(int32_t));
    return (int64_t)t.size() / 5;
}
// "F\tname\tcount\n" per front adapter, then "B\t..." per back adapter, in the trimmer's order after determination
extern "C" const char* dph_trim_adapters(void* h, int64_t* n) {
    TrimH* t = (TrimH*)h;
    t->adapters.clear();
    const TrimResult& r = t->res;
    for (size_t i = 0; i < r.frontNames.size(); i++) t->adapters += "F\t" + r.frontNames[i] + "\t" + std::to_string(r.counts[i]) + "\n";
    for (size_t i = 0; i < r.backNames.size(); i++)
        t->adapters += "B\t" + r.backNames[i] + "\t" + std::to_string(r.counts[r.frontNames.size() + i]) + "\n";
    *n = (int64_t)t->adapters.size();
    return t->adapters.data();
}
// out[DPH_TRIM_STATS]: seen, none, reads, front adapters, back adapters, determine s, end extraction s, upload ms, kernel ms, download ms,
// host apply s, write s, determine kernel ms, bytes up, bytes down, 0
extern "C" void dph_trim_stats(void* h, double* out) {
    const TrimH* t = (const TrimH*)h;
    const TrimResult& r = t->res;
    const double v[] = {(double)r.seen, (double)r.none, (double)t->reads->size(), (double)r.frontNames.size(), (double)r.backNames.size(),
                          r.t_determine, r.t_extract, r.upload_ms, r.kernel_ms, r.download_ms, r.t_apply, r.t_write, r.k_determine_ms,
                          r.bytes_up, r.bytes_down, 0.0};
    static_assert(sizeof v == DPH_TRIM_STATS * sizeof(double), "dph_trim_stats writes out[DPH_TRIM_STATS]");
    memcpy(out, v, sizeof v);
}
extern "C" int dph_trim_demultiplex(void* h, const char* dir) {
    TrimH* t = (TrimH*)h;
    std::string error;
    const int rc = trimDemultiplex(*t->reads, t->res, dir ? dir : ".", error);
    if (rc < 0) g_err = error;
    return rc;
}
// setupIndex as dp_trim_setup takes it.  kmer_seed[4^k]; segs[seg_cap]; seg_off[n + 1]; lengths, is_barcode, pairs[n] with
// n = front + back adapters.  Returns the number of seeds, or -1 (dph_last_error(NULL)); seg_cap too small: -2 - seg_off[n] ints are needed.
extern "C" int64_t dph_trim_index(void* frontH, void* backH, int k, uint16_t* kmer_seed, int32_t* segs, int64_t seg_cap, uint64_t* seg_off,
                                  int32_t* lengths, uint8_t* is_barcode, int32_t* pairs) {
    TrimIndex ix;
    std::string error;
    if (!frontH || !backH || !trimBuildIndex(((ReadsH*)frontH)->set, ((ReadsH*)backH)->set, k, ix, error)) {
        g_err = error.empty() ? "dph_trim_index: bad arguments" : error;
        return -1;
    }
    const size_t n = ix.lengths.size();
    memcpy(seg_off, ix.segOff.data(), (n + 1) * sizeof(uint64_t));
    if ((int64_t)ix.segs.size() > seg_cap) return -2;
    memcpy(kmer_seed, ix.kmerSeed.data(), ix.kmerSeed.size() * 2);
    memcpy(segs, ix.segs.data(), ix.segs.size() * 4);
    memcpy(lengths, ix.lengths.data(), n * 4);
    memcpy(is_barcode, ix.isBarcode.data(), n);
    memcpy(pairs, ix.pairs.data(), n * 4);
    return (int64_t)ix.nSeeds;
}
