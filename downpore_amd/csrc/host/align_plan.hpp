// The arithmetic between a finished mapping and its base-level alignment (host_map.cpp: MapRun::alignMappings), as
// plain functions on numbers and the ABI's plain structs: which bases of which resident reads a PAF line's query and target are
// (strand flip, circular wrap), when a line is out of range and gets no tags, and the text of the tags from the device's run words.
// No device call, no environment, no thread: tests/native/align_plan_check.cpp holds every function here without a GPU.
#pragma once
#include <cstdint>
#include <string>

#include "downpore_hip.h"

namespace dph {

const int64_t kAlignMaxSpan = (int64_t)1 << 20;  // longest query or target span the device aligns
const int64_t kAlignMaxEditsDefault = 4096, kAlignMaxEditsLimit = 32768;

// what retireTasks keeps of a mapping (Mapping, host_map.cpp): the PAF line's columns 2 - 5, 8 and 9 and its reference sequence
struct AlignLine {
    int64_t L = 0;                        // query length (column 2)
    int64_t queryOffset = 0, queryInset = 0;
    int64_t start = 0, end = 0;           // columns 8 and 9
    bool rc = false;
    int ref = 0;
};
// the line's two spans: query bases [qOff, qOff + qLen) of the strand's resident read, target bases tOff + j (mod Lr on a circular
// mapper), j < tLen, of the reference sequence
struct AlignSpan {
    int64_t qOff = 0, qLen = 0, tOff = 0, tLen = 0;
};

// Columns 3 and 4 are forward-read coordinates on both strands (mapping.go:574-580): qs = QueryOffset, qe = L - QueryInset.  On '-' the
// query is the reverse complement of read[qs, qe), which is rc_read[L - qe, L - qs) of the resident reverse strand.  The target is
// End - Start bases from Start, plus Lr when the mapper is circular and that is negative (AsString's mappedLength).
// false: the line is out of range (it keeps its columns and gets no tags) - coordinates outside the read are the reference's own
// arithmetic.
inline bool alignSpanOf(const AlignLine& ln, int64_t Lr, bool circular, AlignSpan& s) {
    const int64_t qs = ln.queryOffset, qe = ln.L - ln.queryInset;
    int64_t tl = ln.end - ln.start;
    if (circular && tl < 0) tl += Lr;
    if (qs < 0 || qe > ln.L || qs >= qe) return false;
    if (tl < 1 || tl > Lr) return false;
    if (ln.start < 0) return false;
    if (circular ? ln.start > Lr : ln.end > Lr) return false;
    if (qe - qs > kAlignMaxSpan || tl > kAlignMaxSpan) return false;
    s.qOff = ln.rc ? ln.L - qe : qs;
    s.qLen = qe - qs;
    s.tOff = ln.start;
    s.tLen = tl;
    return true;
}

// the device's item: a mapper holds read r of the batch as the pair (firstPaired + 2 r, its reverse strand) and reference sequence c
// as device read c
inline dp_align_item alignItemOf(const AlignSpan& s, uint32_t firstPaired, uint32_t read, bool rc, int ref) {
    dp_align_item it;
    it.q_read = firstPaired + 2 * read + (rc ? 1u : 0u);
    it.q_off = (uint32_t)s.qOff;
    it.q_len = (uint32_t)s.qLen;
    it.t_read = (uint32_t)ref;
    it.t_off = (uint32_t)s.tOff;
    it.t_len = (uint32_t)s.tLen;
    return it;
}

// run words (len << 2 | op; 0 M, 1 I, 2 D) -> "12M1I3D"
inline std::string alignCigarText(const uint32_t* runs, uint32_t n) {
    std::string s;
    for (uint32_t i = 0; i < n; i++) {
        s += std::to_string(runs[i] >> 2);
        s += "MID?"[runs[i] & 3u];
    }
    return s;
}
// what goes behind column 12
inline std::string alignTags(int32_t nm, const uint32_t* runs, uint32_t n) {
    return "\tNM:i:" + std::to_string(nm) + "\tcg:Z:" + alignCigarText(runs, n);
}
// bases a run array consumes on either side: its M + I and its M + D
inline void alignConsumed(const uint32_t* runs, uint32_t n, int64_t& query, int64_t& target) {
    query = target = 0;
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t op = runs[i] & 3u;
        const int64_t len = runs[i] >> 2;
        if (op != 2) query += len;
        if (op != 1) target += len;
    }
}

}  // namespace dph
