// The chunk parameters for which chunkWorker's walk (overlap/overlap.go:253-318) is bounded - what chunk_kernel and chunk_cap_of
// (dp_overlap.hip) rely on, and what decides on the host side whether the device may chunk at all.  Plain C++, header only: both
// libraries include it, so that the library's refusal and the host's choice of path cannot drift apart.
#pragma once
#include <stdint.h>

// Every turn of the walk's loop has to move its first seed forward:
//  - a chunk of seedCount >= min_seeds seeds is followed by a back-up of at most five seeds: min_seeds >= 6 moves on by
//    min_seeds - 5 >= 1 seeds (the step chunk_cap_of divides by);
//  - the forward count stops at 100 seeds, so min_seeds > 100 would send every stretch into the branch for too few seeds;
//  - that branch (overlap.go:302-313) backs up by bases alone, with no limit in seeds - but it starts from the length the forward
//    count reached (lengthInBases is not reset there), which is >= chunk_size: with overlap / 2 <= chunk_size it backs up nothing
//    and moves on by the seeds counted, at least one.
// Outside this set a read can be made on which the walk never ends (five seeds 100 bases apart and min_seeds = 5 suffice).
static inline bool dp_chunk_walk_bounded(int64_t chunk_size, int64_t overlap, int64_t min_seeds) {
    return chunk_size >= 1 && min_seeds >= 6 && min_seeds <= 100 && overlap / 2 <= chunk_size;
}
