/*
 * downpore_host.h — C ABI of libdownpore_host.so: the whole `downpore overlap` / `downpore map` pipeline above the kernels of
 * libdownpore_hip.so (include/downpore_hip.h).
 *
 * downpore_hip.h is the boundary of the kernels: one call per batched body of overlap.Overlapper / seeds.SeedIndex /
 * mapping.Mapper.  A host that drives those calls one synchronous round at a time gets the kernels, not the throughput: the
 * reference's own command loop (commands/overlap.go:119-195: PrepareQueries -> AddSequences -> FindOverlaps -> finalCheckWorker,
 * round after round) leaves the GPU idle between dependent launches.  What bench.py measures (BENCH_r*.json) is the pipeline in
 * this library: a planner that runs the PrepareQueries chain ahead on speculative lanes, a window cache that selects every edge
 * window's seeds on the device once, executor slots that run rounds concurrently and commit
 * them in order with a speculation check, consensus + PAF numbers on the device, text on formatter threads.  This header is
 * that pipeline's boundary: a Go `commands/overlap.go` that calls dph_overlap_open / _init / _step / _round_paf (cgo,
 * INTEGRATION.md, integration/commands/gpu_overlap.go) prints the reference's PAF at the measured rate.
 *
 * Conventions: plain pointers and sizes; handles are opaque; int results are 0 / a count on success and negative on failure
 * (dph_last_error gives the text); returned text / byte pointers belong to the handle and stay valid until the next call of the
 * same function on it.  One caller thread per handle (the library runs its own threads behind it).  No CPU fallback: the calls
 * fail without a GPU.
 *
 * Everything declared here is exported under the version node DPH.  What the library exports for its own tests alone (version node
 * DPH_TEST) is declared in downpore_amd/csrc/host/dph_testhooks.h, not here: no embedder calls it.
 */
#ifndef DOWNPORE_HOST_H
#define DOWNPORE_HOST_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPH_API __attribute__((visibility("default")))

/* h: an overlap handle, or NULL for the calling thread's last failed constructor (reads / open / create / map_run) */
DPH_API const char* dph_last_error(void* h);

/* ---- read sets: sequence.NewFastaSequenceSet (sequence/seqio.go:45-300) --------------------------------------------------
 * One-line FASTA / FASTQ records; a line is a sequence iff its first byte is in ['A','T'], kept iff len(line incl. '\n') >=
 * min_len; ids = file order; himem != 0 = the cache the commands use (later passes serve SubSequence views, seqio.go:111-118).
 * from_arrays: read r = bases[off[r] .. off[r+1]) (ASCII), n reads; _q: raw FASTQ quality characters at the same offsets. */
DPH_API void* dph_reads_from_arrays(const char* bases, const int64_t* off, int64_t n, int64_t min_len, int himem);
DPH_API void* dph_reads_from_arrays_q(const char* bases, const char* quals, const int64_t* off, int64_t n, int64_t min_len, int himem);
DPH_API void* dph_reads_from_fasta(const char* path, int64_t min_len, int himem);
DPH_API void dph_reads_free(void* reads);
DPH_API int64_t dph_reads_count(void* reads);
DPH_API int64_t dph_reads_total_bases(void* reads);
/* SetIgnore flags (seqio.go:375) as the last job left them: out[n reads] */
DPH_API void dph_reads_get_ignore(void* reads, uint8_t* out);
DPH_API void dph_reads_reset_ignore(void* reads);

/* ---- `downpore overlap` (commands/overlap.go:96-233) -----------------------------------------------------------------------
 * dph_overlap_open   device context on HIP device `device`; the reads are uploaded and packed (and stay resident for every job
 *                    on this handle); FASTQ qualities travel with them.
 * dph_overlap_init   everything the command does between "Counting all k-mers" and its first round: k-mer position index,
 *                    value table (on the device unless `values` - 4^k doubles, the -seed_values table - is given), executor
 *                    slots, planner, window cache.  params[8] = overlap_size, k, num_seeds, seed_batch_size, chunk_size,
 *                    query_batch_size, himem | query_type << 8 (overlap.QueryEdges 1 = the overlap command, QueryCentre 2,
 *                    QueryAll 4, + WeightEdges 8; overlap/overlap.go:18-21), executor slots (rounds in flight; 8 = what bench.py
 *                    uses).  min_hits = -min_hits.
 * dph_overlap_step   commits the next finished round(s) in round order; returns how many (0 = the command is finished).  The
 *                    PAF lines of exactly those rounds: dph_overlap_round_paf (dph_overlap_step_lines of them); every line so
 *                    far: dph_overlap_all_paf; the reference's stderr lines: dph_overlap_errtext.
 * dph_overlap_reset  ends the job, keeps the handle, the resident reads and the executor contexts: dph_overlap_init starts the
 *                    next job (other k, other parameters).  dph_overlap_create = open + init. */
DPH_API void* dph_overlap_open(void* reads, int device);
/* dph_overlap_open_trim   `overlap -trim true`: dph_overlap_open of the read set `downpore trim` would write for `reads` (loaded with
 *                    min_len 50), without the file: the reads go up once, the trim (params as dph_trim_run takes them) runs on the resident
 *                    copy, the trimmed read set - kept as a written record of n bases is kept by a reader with minimum length min_len:
 *                    n + 1 >= min_len - is cut from it on the device (dp_reads_respan) and its qualities follow.  The handle owns
 *                    that read set (dph_overlap_reads: a reads handle valid while the overlap handle lives, NULL for a handle of
 *                    dph_overlap_open); *trim_out receives the trim run's handle (log, table, stats; no output text; dph_trim_free). */
DPH_API void* dph_overlap_open_trim(void* reads, void* front, void* back, const int64_t* trim_params, int n_params, int64_t min_len, int device,
                                    void** trim_out);
DPH_API void* dph_overlap_reads(void* h);
DPH_API int dph_overlap_init(void* h, const int64_t* params, double min_hits, const double* values);
DPH_API int dph_overlap_reset(void* h);
DPH_API void* dph_overlap_create(void* reads, int device, const int64_t* params, double min_hits, const double* values);
DPH_API void dph_overlap_destroy(void* h);
DPH_API int dph_overlap_step(void* h);
DPH_API int64_t dph_overlap_step_lines(void* h);
DPH_API const char* dph_overlap_round_paf(void* h, int64_t* n);
DPH_API const char* dph_overlap_all_paf(void* h, int64_t* n);
DPH_API const char* dph_overlap_errtext(void* h, int64_t* n);
/* multi-rank runs: keep == 0 on a rank that does not print the PAF - gathered rounds are committed with their counts, flags and read
 * lists, their text is dropped as it arrives (default: kept on every rank) */
DPH_API void dph_overlap_keep_text(void* h, int keep);
DPH_API int dph_overlap_done(void* h);
DPH_API int64_t dph_overlap_round(void* h);                     /* rounds committed so far */
DPH_API void dph_overlap_set_round_limit(void* h, int64_t n);   /* dph_overlap_step commits no round >= n (-1: no limit) */
DPH_API void dph_overlap_drain(void* h);                        /* drops the rounds in flight (they are executed again) */
DPH_API int dph_overlap_slots(void* h);
/* the job's k-mer value table (4^k doubles, commands/overlap.go:55-93) */
DPH_API const double* dph_overlap_values(void* h, int64_t* n);
/* the device context of the handle (a dp_ctx* of downpore_hip.h) */
DPH_API void* dph_overlap_ctx(void* h);
/* out[3]: seconds spent creating the context, uploading + packing the reads, in the last dph_overlap_init */
DPH_API void dph_overlap_setup_times(void* h, double* out);
/* statistics of the last committed round / summed over the job: out[DPH_OVERLAP_STATS] doubles in the order of
 * downpore_amd/overlap.py STAT_FIELDS (host seconds per phase, kernel milliseconds, algorithmic bytes, counts) */
#define DPH_OVERLAP_STATS 32
DPH_API void dph_overlap_stats(void* h, double* out);
DPH_API void dph_overlap_stats_total(void* h, double* out);

/* ---- multi-GPU: one handle per GPU (process, or thread of one process) ---------------------------------------------------------
 * scan-shard (reads partitioned, survivors' seed index all-gathered): every rank runs every round on its read
 * range [lo, hi); the survivors are exchanged inside the library (dp_comm: RCCL over xGMI, or peer copies between the handles
 * of one process).  dph_comm_unique_id on rank 0, the 128 bytes to every rank, dph_overlap_comm_init (one communicator) or
 * _comm_init_slots (one per executor slot: ids = n_slots x 128 bytes) BEFORE dph_overlap_init; then dph_overlap_set_shard and
 * dph_overlap_round_sharded (one round) / dph_overlap_rounds_sharded (one round per slot, concurrently) - collective calls.
 * dph_overlap_round_scan / _local / _round_finish: the same round in two halves with the exchange left to the caller.
 * round-parallel (reads + index on every GPU, rounds dealt to the ranks): dph_overlap_set_ranks, then per superstep
 * dph_overlap_wait_owned_many (this rank's finished rounds, serialised) -> the caller all-gathers the blobs ->
 * dph_overlap_commit_gathered on every rank (commits the valid prefix in round order; rejected rounds are executed again).
 * dph_overlap_exec_round / dph_overlap_commit_blobs: the batch-synchronous form of the same. */
DPH_API int dph_comm_unique_id(uint8_t* id128);
DPH_API int dph_overlap_comm_init(void* h, int n_ranks, int rank, const uint8_t* id128);
DPH_API int dph_overlap_comm_init_slots(void* h, int n_ranks, int rank, const uint8_t* ids, int n_slots);
DPH_API int dph_overlap_comm_init_local(void** handles, int n);
DPH_API int dph_overlap_comm_init_local_slots(void** handles, int n, int n_slots);
DPH_API void dph_overlap_set_shard(void* h, int64_t lo, int64_t hi);
DPH_API int dph_overlap_round_sharded(void* h);
DPH_API int dph_overlap_rounds_sharded(void* h);
DPH_API int dph_overlap_round_scan(void* h);
DPH_API void dph_overlap_local(void* h, const uint32_t** read, const uint32_t** n_seeds, const uint64_t** seg_off, const int32_t** segs,
                               uint64_t* n, uint64_t* n_segs);
DPH_API int dph_overlap_round_finish(void* h, const uint32_t* read, const uint32_t* n_seeds, const int32_t* segs, uint64_t n);
DPH_API void dph_overlap_set_ranks(void* h, int rank, int world);
DPH_API const uint8_t* dph_overlap_wait_owned(void* h, uint64_t* n);
DPH_API const uint8_t* dph_overlap_wait_owned_many(void* h, int max_rounds, uint64_t* n);
DPH_API int dph_overlap_commit_gathered(void* h, const uint8_t* blobs, const uint64_t* sizes, int count);
/* the same superstep with the exchange inside the library (dp_allgather_blobs on the communicator of dph_overlap_comm_init):
 * rounds committed; 0 = the superstep's first round was rejected and runs again (or the command is finished: dph_overlap_done) */
DPH_API int dph_overlap_superstep(void* h, int max_rounds);
/* root >= 0: a superstep gathers the rounds' PAF text to rank `root` alone (the rank that prints: commands/overlap.go:225-228 prints
 * in one process) and all-gathers only the rounds' control records (flags, read lists, counts: a few KB per round); every rank of
 * the job must pass the same root, before the first superstep.  -1 (the default): text and control travel together to every rank. */
DPH_API void dph_overlap_text_root(void* h, int root);
DPH_API const uint8_t* dph_overlap_exec_round(void* h, int64_t first_round, uint64_t* n);
DPH_API int dph_overlap_commit_blobs(void* h, const uint8_t* blobs, const uint64_t* sizes, int count);

/* ---- `downpore map` (commands/map.go:33-116, mapping/mapping.go) -------------------------------------------------------------
 * The whole command: reference = first sequence of `ref` (a read set opened with himem = 0), reads top-level.  params[6] =
 * circular, k, query_size, min_length, chunk_size, seed_rate.  DP_MAP_SHARDS / DP_MAP_DEVICES in the environment spread the
 * reference index over several contexts / GPUs (BASELINE config 5).  Returns a handle holding the PAF (read order) and the
 * reference's stderr lines, or NULL.  dph_map_stats: out[DPH_MAP_STATS] = chunks, seeds, windows, chains, batches, scan kernel ms, map
 * kernel ms, seconds of set-up / window scans / dp_map_windows / host, algorithmic bytes of the map kernels (index query +
 * prefilter + chaining) and of the window scans (packed bases). */
DPH_API void* dph_map_run(void* ref, void* reads, const int64_t* params, int device);
/* dph_map_run with n_params = 6 (the same), 7 or 8: params[6] = the reference index's layout, 0 = auto, 1 = dense, 2 = sparse
 * (dp_index_build_sparse; mapper threads then borrow the one index).  Auto takes sparse when the dense estimate - S ceil(M/64) 8 +
 * M ceil(S/64) 8 bytes summed over the contexts / shards the run builds on a device - exceeds that device's free memory less an
 * eighth of its total.  Both layouts print the same PAF.  Another layout value is refused before any device call.  A reference
 * sequence longer than 2^31 - 1 bases is refused (with its length in the error) before anything is allocated.
 * params[7] (n_params = 8) = 1: map against EVERY sequence of `ref` in file order, 0 (the default): against the first one only;
 * another value is refused before any device call.  The seeds are chosen for one sequence after the other on one index, the chunk
 * ids run on from sequence to sequence (ten passes, then the circular join chunk of a sequence of at least query_size bases; a
 * shorter one gets none and one stderr line says so), a chunk's positions are relative to its own sequence, mappings on two
 * sequences are never joined or de-duplicated against each other, and columns 6 - 9 of a PAF line are its sequence's name, length
 * and positions.  Both index layouts and DP_MAP_SHARDS work as they are (they cut by chunk id).  A sequence longer than 2^31 - 1
 * bases (the error names it) and 2^32 or more seed windows or chunks in total are refused before anything is allocated; a
 * reference without any chunk leaves every read unmapped.  With one sequence in `ref` the output is that of params[7] = 0. */
DPH_API void* dph_map_run_ex(void* ref, void* reads, const int64_t* params, int n_params, int device);
/* dph_map_run_trim   `trim` in front of `map` on one upload.  reads: the raw read set, loaded with trim's minimum length 50; front / back
 *                    and trim_params[n_trim] (8, or 14 with the middle stage) as dph_trim_run and dph_overlap_open_trim take them;
 *                    params[n_params] (6, 7 or 8) as dph_map_run_ex takes them.  The PAF of the handle that comes back is byte for
 *                    byte what dph_map_run_ex gives on the read set `downpore trim` would write for `reads`, read back with minimum
 *                    length params[3] (dph_trim_reads' rule: a record of n bases is kept iff n + 1 >= min_len and n > 0; the halves of
 *                    split reads follow the file's reads; names as tagged); dph_map_errtext is map's own text over that set.
 *                    The bases cross the link once, 2-bit packed: the device read set goes up as [raw reads | reference sequences |
 *                    join chunks] without pairs, both trim stages run on that copy (ids and spans go up), and one dp_reads_respan_rc
 *                    makes map's own set from it - reference sequences and join chunks, then (forward, reverse complement) of every
 *                    trimmed read.  From there the run is dph_map_run_ex's: shards (DP_MAP_SHARDS / DP_MAP_DEVICES), both index
 *                    layouts, all sequences.  The packed upload is the only one here: DP_TUNE=map_async_upload and
 *                    DP_TUNE=map_ascii_upload are not consulted.
 *                    *trim_out receives the trim run's handle, on `device` like the context: its log without the line about writing,
 *                    table and stats, no output text; dph_trim_reads works on it; dph_trim_free frees it.  The raw read set must
 *                    outlive it; the run overwrites its ignore flags and trims.  NULL on failure (dph_last_error(NULL)), with
 *                    *trim_out = NULL and nothing left behind. */
DPH_API void* dph_map_run_trim(void* ref, void* reads, void* front, void* back, const int64_t* trim_params, int n_trim,
                               const int64_t* params, int n_params, int device, void** trim_out);
DPH_API void dph_map_free(void* m);
DPH_API const char* dph_map_paf(void* m, int64_t* n);
DPH_API const char* dph_map_errtext(void* m, int64_t* n);
#define DPH_MAP_STATS 13
DPH_API void dph_map_stats(void* m, double* out);
/* The run's reference index: out[0..9] = layout (1 dense, 2 sparse), device bytes of the indexes built, the dense estimate D, the
 * device's total memory, H (seed hits in chunks), contexts that built an index, then the queries by regime: 4/8-ladder (minCount
 * <= 12), 16-ladder (13 .. 24), exact count (> 24), more than 512 sets.  Writes at most cap values; returns how many it wrote. */
DPH_API int dph_map_index_info(void* m, int64_t* out, int cap);
/* A mapper: the reference side of dph_map_run_ex done once, batches of reads mapped against it one after the other (the reference
 * program's NewMapper, then MapWorker over a stream of reads).
 * dph_mapper_open   params[n_params] as dph_map_run_ex takes them.  The reference sequences and join chunks go up, the value table, the
 *                   seeds, the chunk scan and the reference index are made, and stay until dph_mapper_close.  `ref` must outlive the
 *                   mapper.  DP_MAP_SHARDS > 1 and DP_TUNE=map_ascii_upload / map_async_upload are refused by name (they stay with
 *                   the one-shot call), as is everything dph_map_run_ex refuses about its parameters.  NULL on failure
 *                   (dph_last_error(NULL)).
 * dph_mapper_map    maps `reads` and returns a handle of dph_map_run_ex's kind (dph_map_paf, dph_map_errtext, dph_map_stats,
 *                   dph_map_index_info, dph_map_free): PAF and stderr text are byte for byte what dph_map_run_ex gives for (ref, reads).
 *                   Only the batch crosses the link; it replaces the previous batch behind the resident head.  Stats: chunks and
 *                   seeds are the mapper's, the set-up seconds are this batch's time before its loops, the index bytes and builds
 *                   are the mapper's totals so far (they grow only when a batch is the first to use more threads).  One call at a
 *                   time per mapper: a second, concurrent one returns NULL (state error) at once.  After a batch has failed with a
 *                   device error the mapper is broken and every later call returns that first error without touching the device; a
 *                   batch refused for its arguments leaves it usable.  The handle is independent of the mapper and of `reads`.
 * dph_mapper_map_trim  dph_mapper_map with `trim` in front of it, per batch: reads is the raw read set (loaded with trim's minimum
 *                   length 50); front / back, trim_params[n_trim] and *trim_out are as dph_map_run_trim documents them; the result
 *                   handle is of dph_mapper_map's kind, and its PAF and stderr text are byte for byte dph_map_run_trim's for (ref,
 *                   reads, front, back, trim_params) with the mapper's parameters.  The batch crosses the link once, 2-bit packed: it
 *                   goes behind the resident head unpaired (dp_reads_replace_tail_packed), both trim stages run on that copy under
 *                   the ids behind the head, and dp_reads_respan_tail_rc cuts the trimmed set (minimum length: the mapper's
 *                   params[3]) from it with its reverse strands; the head is not touched.  Adapters are determined per batch.  Bad
 *                   arguments return NULL with a text that starts "dph_mapper_map_trim: bad arguments" and leave the mapper
 *                   usable; so does a trim that fails for its parameters or its input (k outside 3..8, chunk_size <= 100 with the
 *                   middle stage, no read long enough), whether or not the raw batch had gone up.  A device error breaks the mapper
 *                   as in dph_mapper_map.  *trim_out = NULL on every failure.
 * dph_mapper_map_align  dph_mapper_map, or dph_mapper_map_trim, with the base-level alignment of every PAF line of the batch behind its
 *                   column 12: "\tNM:i:<edit distance>\tcg:Z:<CIGAR>" (what `minimap2 -c` prints; M covers matches and mismatches).
 *                   front == back == trim_params == NULL and n_trim == 0 (trim_out is then not written beyond a NULL) mean no trim;
 *                   otherwise those arguments and *trim_out are exactly dph_mapper_map_trim's.  align_params[0] = max_edits (1 ..
 *                   32768; 4096 is the usual choice), n_align == 1.  The rule, per line: the query is columns 3 - 4 of
 *                   the read ('-': their reverse complement), the target End - Start bases from Start (plus the sequence's length when
 *                   the mapper is circular and that is negative; positions wrap on a circular mapper); NM is the unit-cost edit distance
 *                   of the two, the CIGAR the canonical walk dp_align_spans documents (gaps go to the left end of a tie).  A line whose
 *                   coordinates lie outside its read or sequence, or whose spans exceed 2^20 bases, gets no tags (out of range), as
 *                   does a line whose NM exceeds max_edits.  Columns 1 - 12, the order of the lines, the stderr text and dph_map_stats
 *                   are dph_mapper_map's (dph_mapper_map_trim's), byte for byte.  The alignment runs on the device (dp_align_spans)
 *                   over the reads and reference the mapper holds there anyway.  Bad arguments (a max_edits outside its range among
 *                   them) return NULL with a text that starts "dph_mapper_map_align: bad arguments" and leave the mapper usable; a
 *                   device error breaks it, as in dph_mapper_map.
 * dph_map_align_info  out[0..7] of a map handle = PAF lines, lines aligned, lines over max_edits, lines out of range, DP cells
 *                   computed, band doublings, kernel microseconds, trace-back bytes written; all zero for a handle made without
 *                   alignment.  Writes at most cap values; returns how many it wrote.
 * dph_mapper_close  gives everything back: worker contexts, then the main context, then the pinned block.  NULL is ignored. */
DPH_API void* dph_mapper_open(void* ref, const int64_t* params, int n_params, int device);
DPH_API void* dph_mapper_map(void* mapper, void* reads);
DPH_API void* dph_mapper_map_trim(void* mapper, void* reads, void* front, void* back, const int64_t* trim_params, int n_trim, void** trim_out);
DPH_API void* dph_mapper_map_align(void* mapper, void* reads, void* front, void* back, const int64_t* trim_params, int n_trim, void** trim_out,
                                   const int64_t* align_params, int n_align);
DPH_API int dph_map_align_info(void* m, int64_t* out, int cap);
DPH_API void dph_mapper_close(void* mapper);

/* ---- `downpore trim`, edge stage (commands/trim.go:32-50, trim/trim.go:272-513, sequence/seqio.go:375-523) --------------------
 * reads: a read set loaded with min_len 50 (commands/trim.go:35); front / back: the adapter files loaded with min_len 0.  The read
 * set must outlive the handle; a run overwrites its ignore flags and trims.
 * params[8] = k, check_reads, adapter_threshold, extra_end_trim, tag_adapters, require_pairs, determine_adapters, verbosity.
 * dph_trim_run: adapter determination, end trimming and the writer on HIP device `device`; NULL on failure - k outside 3..8, an
 * adapter beyond the device's limits, no read of 200 bases ("no reads long enough to trim").
 * dph_trim_apply: the same outputs without a device, from what a caller that drives dp_trim_edges itself has in hand: enabled (NULL:
 * no determination ran) = the determine flags over the front then the back adapters as loaded; recs = six int32 (dp_trim_rec) per
 * end, two ends per read of 200 bases and more in read order, and counts = matches per adapter - both in the order of the adapter
 * lists AFTER determination (the backwards swap-remove of trim.go:294-322).
 * dph_trim_output: the trimmed FASTA / FASTQ text; dph_trim_errtext: the reference's log lines without their timestamps.
 * dph_trim_table: int32[reads][5] = front_trim, back_trim, ignore, front adapter index or -1, back adapter index or -1; returns the
 * number of reads.  dph_trim_adapters: "F|B <tab> name <tab> matches" lines, the adapters after determination in the trimmer's order.
 * dph_trim_stats: out[DPH_TRIM_STATS] = seen, none, reads, front adapters, back adapters, determination s, end extraction s, upload ms, kernel
 * ms, download ms, host apply s, write s, determination kernel ms, bytes up, bytes down, 0.
 * dph_trim_demultiplex: <dir>/<label>.fasta|.fastq per barcode label (seqio.go:460-523); returns the number of files or < 0.
 * dph_trim_index: setupIndex (trim.go:57-99) in the layout dp_trim_setup takes - kmer_seed[4^k], segs[seg_cap], seg_off[n + 1],
 * lengths / is_barcode / pairs[n], n = front + back adapters; returns the number of seeds, -1 on error, -2 when seg_cap is below the
 * seg_off[n] ints needed. */
DPH_API void* dph_trim_run(void* reads, void* front, void* back, const int64_t* params, int n_params, int device);
DPH_API void* dph_trim_apply(void* reads, void* front, void* back, const int64_t* params, int n_params, const uint8_t* enabled,
                             const int32_t* recs, int64_t n_rec_reads, const uint64_t* counts);
DPH_API void dph_trim_free(void* t);
/* the read set the run's output gives when read back with minimum length min_len, without the text (a new reads handle; no device needed) */
DPH_API void* dph_trim_reads(void* t, int64_t min_len, int himem);
DPH_API const char* dph_trim_output(void* t, int64_t* n);
DPH_API const char* dph_trim_errtext(void* t, int64_t* n);
DPH_API int64_t dph_trim_table(void* t, int32_t* out, int64_t cap_reads);
DPH_API const char* dph_trim_adapters(void* t, int64_t* n);
#define DPH_TRIM_STATS 16
DPH_API void dph_trim_stats(void* t, double* out);
DPH_API int dph_trim_demultiplex(void* t, const char* dir);
DPH_API int64_t dph_trim_index(void* front, void* back, int k, uint16_t* kmer_seed, int32_t* segs, int64_t seg_cap, uint64_t* seg_off,
                               int32_t* lengths, uint8_t* is_barcode, int32_t* pairs);

/* ---- `downpore trim`, middle stage (trim/trim.go:151-256, 515-591; sequence/seqio.go:81-104, 302-323, 396-399) ----------------
 * The search for front adapters in the middle of reads: every edge-trimmed read's centre is cut into chunks (dph_trim_chunk_plan:
 * out[3 i ..] = start, end, is-remainder of the chunks of one served length, in the coordinates of the trimmed read; -1 when
 * chunk_size <= 100, where the reference's loop does not end), the chunks are scanned for adapter seeds and matched against every
 * front adapter, and findSplit's rules crop the front, crop the tail or split the read; the halves of split reads follow the file's
 * reads in the output as <name>_(left) / <name>_(right).
 * params[14] = the edge stage's eight, then middle (0: off, exactly the eight-parameter behaviour), chunk_size, middle_threshold,
 * extra_middle_trim, discard_middle, flush_seeds (the reference's 300000000: a batch of chunks is searched after the read that takes
 * the batch's seed count over it; after such a flush PrintStats reports the edge counts as 0, as the reference does).
 * dph_trim_apply_mid: dph_trim_apply with the middle stage's device results supplied: seed_counts[n_chunks] = seeds of every planned
 * chunk (reads in file order, chunks in position order) and mid_recs = six int32 per match that passed the identity test - front
 * adapter, chunk (position in the plan), ordinal of the match within the pair, GetSeedOffset(MatchB[0]) - ad.GetSeedOffset(MatchA[0]),
 * bases covered, chain length - in any order: they are applied batch by batch, adapter by adapter, in chunk and ordinal order.
 * dph_trim_mid_ints: which = 0 the plan (read, start, end, remainder, seeds, indexed per chunk), 1 the splits (read, aEnd, bStart,
 * kept halves: bit 0 left, bit 1 right), 2 the records applied; returns the number of int32.  dph_trim_extras: the halves' names,
 * one per line.  dph_trim_mid_stats: out[DPH_TRIM_MID_STATS] = chunks, seeds, batches, candidate pairs, records applied, overflow pairs,
 * out-of-range halves (a right half whose start is negative is skipped, counted and named in the log), upload / scan / index /
 * query / kernel ms. */
DPH_API void* dph_trim_apply_mid(void* reads, void* front, void* back, const int64_t* params, int n_params, const uint8_t* enabled,
                                 const int32_t* recs, int64_t n_rec_reads, const uint64_t* counts, const int32_t* seed_counts,
                                 int64_t n_chunks, const int32_t* mid_recs, int64_t n_mid_recs);
DPH_API int64_t dph_trim_chunk_plan(int64_t length, int64_t chunk_size, int32_t* out, int64_t cap);
DPH_API int64_t dph_trim_mid_ints(void* t, int which, int32_t* out, int64_t cap);
DPH_API const char* dph_trim_extras(void* t, int64_t* n);
#define DPH_TRIM_MID_STATS 12
DPH_API void dph_trim_mid_stats(void* t, double* out);

/* ---- process-wide: profile, pipeline counters, kept buffers ------------------------------------------------------------------ */
DPH_API void dph_profile_print(void);
/* process-wide pipeline counters since the process started: 0 plans computed, 1 thrown away, 2 erased by a commit's flags, 3 rounds
   executed, 4 rejected at the commit, 5 committed, 6 us in plan computes (wall, all lanes), 7 us the slots waited for plans,
   8 us the committing thread (the caller of dph_overlap_step) waited for the next round in order, 9 us it spent on a round's text
   (13: of which waiting for a formatter thread), 10 us on flags + planner bookkeeping, 11 us keeping the step's text,
   12 us the formatter threads spent formatting (all threads together), 14 the planner's lanes at the moment (a state, not a sum);
   -1 for any other index */
DPH_API int64_t dph_planner_counter(int which);
/* The library keeps some host buffers between jobs (process-wide, shared by all handles, surviving dph_overlap_destroy): PAF text
 * strings and record arrays of finished rounds (at most 512 MB), window-cache chunks (at most 16 x 11.5 MB), the staging block of
 * the last `map` command (reference + reads, ~400 MB at BASELINE config 3).  A long-lived embedder calls this after its last job
 * (or whenever it wants the memory back; a running job simply allocates again).  Returns the bytes released. */
DPH_API int64_t dph_release_caches(void);

#ifdef __cplusplus
}
#endif
#endif /* DOWNPORE_HOST_H */
