/*
 * dph_testhooks.h — the test bench of libdownpore_host.so: sixteen C entry points that only files under tests/ call.  They are
 * NOT part of the pipeline's boundary (include/downpore_host.h), which is why this header does not live under include/: host
 * logic that runs without a GPU (decision rules on bare numbers, planner and ISA self-tests, a finalCheckWorker replay) and a few
 * helpers the tests compare with the oracle.  The library exports them under a version node of their own (DPH_TEST in
 * exports_host.map; the boundary is DPH), their bodies are in host_testhooks.cpp.  Conventions as in downpore_host.h.
 */
#ifndef DPH_TESTHOOKS_H
#define DPH_TESTHOOKS_H

#include "downpore_host.h" /* DPH_API, the reads handles */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- helpers only tests use ---------------------------------------------------------------------------------------------------
 * dph_reads_dump          "name <tab> ACGT..." per read (FASTQ: <tab> the stored quality bytes, two hex digits each): this reader
 *                          against the oracle's
 * dph_values_from_counts  the value table (commands/overlap.go:55-92) from a k-mer histogram; counts is overwritten with the
 *                          merged forward + reverse-complement counts like the reference's in-place loop */
DPH_API const char* dph_reads_dump(void* reads, int64_t* n);
DPH_API void dph_values_from_counts(uint64_t* counts, int k, double* out);
/* packBytes of a whole read as `map` hands its reads to the device (sequence/sequence.go:59-93); out: ceil(n / 4) bytes; scalar_only:
   without the AVX2 path */
DPH_API void dph_pack_bases(const char* bases, int64_t n, uint8_t* out, int scalar_only);
/* finalCheckWorker (commands/overlap.go:197-233) over externally supplied queries, indexed sequences and matches (flat arrays
 * in the reference's segment layout): returns the round's PAF text and applies SetIgnore to `reads` */
DPH_API const char* dph_finalcheck(void* reads, int k, int64_t overlap_size, const uint32_t* seed_kmers, int64_t n_seeds,
                                   const int32_t* q_segs, const int64_t* q_off, const int64_t* q_id, const int64_t* q_seq_id,
                                   const int64_t* q_len, const int64_t* q_offset, const int64_t* q_inset, int64_t n_q,
                                   const int32_t* i_segs, const int64_t* i_off, const int64_t* i_id, const int64_t* i_len,
                                   const int64_t* i_offset, const int64_t* i_inset, int64_t n_i, const int64_t* m_query,
                                   const int64_t* m_target, const int64_t* m_off, const int32_t* m_a, const int32_t* m_b,
                                   int64_t n_m, int64_t num_query_seqs, int64_t* out_len, int64_t* out_stats);

/* ---- hand-worked rules: decision rules of the host side on bare numbers, held by tests/test_hand_known_answers.py
 * to answers worked by hand from the reference's Go text (the files under tests/golden/hand).
 * dph_hand_is_consistent   mapping.isConsistent (mapping/mapping.go:131-160): left5 = {RC, Query.Len(), QueryInset, Start, End},
 *                          right4 = {RC, QueryOffset, Start, End}
 * dph_hand_remove_dominated  removeDominated (mapping.go:387-428): maps3 = n x {QueryOffset, QueryInset, ids}; kept[] = the survivors'
 *                          indices in the order the function returns them; returns their number
 * dph_hand_trim_indices    step 1 of trimToBestSeed (overlap/combine.go:24-58): match i's MatchA = match_a[off[i] .. off[i + 1]);
 *                          out2 = {bestIndex, backIndex}
 */
DPH_API int dph_hand_is_consistent(const int64_t* left5, const int64_t* right4, int circular, int64_t ref_len);
DPH_API int dph_hand_remove_dominated(const int64_t* maps3, int n, int64_t query_len, int* kept);
DPH_API void dph_hand_trim_indices(int upto, const int32_t* match_a, const int64_t* off, int n_matches, int min_match, int length, int* out2);
/* SeedIndex.AddSeeds (seeds/seeds.go:62-156) of one top-level sequence into an empty index, as the planner's host selection does it: the index's
   seedMap (k-mers in seed-id order); returns their number, -1 when cap is too small */
DPH_API int dph_hand_add_seeds(const char* bases, int64_t len, int k, int num_seeds, const double* values, uint32_t* seed_map, int cap);
/* SeedMatch.GetBasesCovered (seeds/sequence.go:830-858: the PAF line's tenth column) on raw segment arrays and matched seed indices;
   out2 = {countA, countB}; returns 1 where the reference would panic */
DPH_API int dph_hand_bases_covered(const int32_t* a_seg, int a_n, const int32_t* b_seg, int b_n, const int32_t* match_a, const int32_t* match_b, int n,
                                   int k, int64_t* out2);
/* multiAligner.Consensus of the host's consensus path (seeds/alignment.go:23-268) on raw segment arrays: sequence i = segs[off[i] .. off[i + 1]);
   the consensus' segments, the indices of the sequences whose match was kept (>= 3 pairs) in the order returned, their pairs */
DPH_API int dph_hand_consensus(const int32_t* segs, const int64_t* off, int n_seqs, int k, int32_t* cons_out, int64_t cons_cap, int64_t* cons_n,
                               int* kept, int64_t* out_counts, int32_t* out_a, int32_t* out_b, int64_t cap, int64_t* n_matches);
/* `downpore trim`, middle stage: the exact host Match that the (chunk, front adapter) pairs beyond the matching kernel's working set are
 * given to, with the identity test; segments as [gap, seed, ..., gap]; out = six int32 per passing match; returns their number */
DPH_API int64_t dph_hand_trim_match(const int32_t* chunk_segs, int n_chunk, const int32_t* adapter_segs, int n_adapter, int adapter_len,
                                    int n_seeds, int k, int threshold, int adapter, int chunk, int32_t* out, int64_t cap);

/* ---- self-tests --------------------------------------------------------------------------------------------------------------
 * dph_test_coroutines     the mapper's read tasks are stackful coroutines (host/host_coro.hpp): n_tasks of them on recycled stacks,
 *                          each resumed `yields` times; returns the sum of id x yields over the tasks, -1 if a frame came back damaged.
 */
DPH_API long dph_test_coroutines(int n_tasks, int yields);
DPH_API int dph_selftest_planner_flags(void* reads, int k, int64_t seed_batch_size, const double* values);
DPH_API int dph_selftest_planner_lanes(void* reads, int k, int64_t seed_batch_size, const double* values, int lanes, int flag_every,
                                       int64_t* n_rounds);
/* the plan chain of a round-parallel run of `world` ranks whose planners compute only their own rounds' plans and guess the rest
 * (Planner::setOwnership), played against a commit that accepts a plan iff it starts at the committed firstSequence */
DPH_API int dph_selftest_planner_sparse(void* reads, int k, int64_t seed_batch_size, const double* values, int world, int flag_every,
                                        int64_t* n_rounds, int64_t* n_redone);
DPH_API int dph_selftest_touch(int k, const uint32_t* seeds, int64_t n_seeds, const uint32_t* kmers, int64_t n_windows, int64_t stride,
                               uint8_t* res, int* isa_mask);

#ifdef __cplusplus
}
#endif
#endif /* DPH_TESTHOOKS_H */
