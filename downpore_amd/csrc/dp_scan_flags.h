// Host bookkeeping of the reads' ignore flags for dp_scan_reads (dp_scan.hip): the shadow copy of the flags as the device holds
// them, and the two sums a round reports - bases examined and reads scanned over the non-ignored reads of the view.  Plain C++,
// header only, no HIP: tests/native/scan_flags_check.cpp runs it against a brute-force recount, with sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

// What the sums are taken over: the reads [lo, hi), and how many of a read's bases a scan examines (top_level, k).
struct dp_flag_view {
    uint32_t lo, hi;
    int top_level, k;
};
static inline bool dp_flag_view_same(const dp_flag_view& a, const dp_flag_view& b) {
    return a.lo == b.lo && a.hi == b.hi && a.top_level == b.top_level && a.k == b.k;
}
struct dp_flag_sums {
    uint64_t bases;  // bases examined: every k-mer's, so k - 1 more than the k-mers of a read that has any
    uint32_t reads;
};

// Bases a scan examines of a read of `len` bases: all of it, or nothing where it holds no k-mer; a top-level sequence whose length
// is a multiple of four has four k-mers fewer (finalLen == 0, sequence/asm_amd64.s:88-96 - as make_read_items_kernel has it).
static inline uint64_t dp_flag_bases_of(uint32_t len, const dp_flag_view& v) {
    int64_t n = (int64_t)len - v.k + 1;
    if (v.top_level && (len & 3u) == 0) n -= 4;
    return n > 0 ? (uint64_t)n + v.k - 1 : 0ull;
}

// Brings `shadow` (shadow_bytes >= n_reads rounded up to 8; what lies behind n_reads is and stays zero) up to date with the caller's
// `flags` and returns the view's sums.  !same_view - another view than `sums` was taken over, or a shadow that is not valid -
// everything once: the flags are copied and the sums recounted.  same_view: the shadow is compared with the flags eight bytes at a
// time and `sums` adjusted by the reads of the view whose flag went between zero and non-zero.  The caller's array may change under
// either loop: every byte of it is read ONCE, and what was read is what the shadow gets (and, from there, the device) and what the
// sums count - the commit's speculation check covers flags set after a round's snapshot.
static inline dp_flag_sums dp_scan_flags_update(uint8_t* shadow, size_t shadow_bytes, const uint8_t* flags, uint32_t n_reads,
                                                const uint32_t* len, const dp_flag_view& v, bool same_view, dp_flag_sums sums) {
    if (!same_view) {
        memcpy(shadow, flags, n_reads);
        memset(shadow + n_reads, 0, shadow_bytes - n_reads);
        sums = dp_flag_sums{0, 0};
        for (uint32_t r = v.lo; r < v.hi; r++) {
            if (shadow[r]) continue;
            sums.bases += dp_flag_bases_of(len[r], v);
            sums.reads++;
        }
        return sums;
    }
    // the reads r0 .. r0 + n - 1 (n <= 8), whose flags as just read are the bytes of now_w
    auto take_word = [&](uint32_t r0, uint32_t n, uint64_t now_w) {
        uint64_t old_w = 0;
        memcpy(&old_w, shadow + r0, n);
        if (now_w == old_w) return;
        for (uint32_t r = r0; r < r0 + n; r++) {
            const uint8_t now = (uint8_t)(now_w >> (8 * (r - r0)));
            if (now == shadow[r]) continue;
            if (r >= v.lo && r < v.hi && (now != 0) != (shadow[r] != 0)) {
                const uint64_t b = dp_flag_bases_of(len[r], v);
                if (now) sums.bases -= b, sums.reads--;
                else sums.bases += b, sums.reads++;
            }
            shadow[r] = now;
        }
    };
    const uint32_t full = n_reads & ~7u;
    for (uint32_t r0 = 0; r0 < full; r0 += 8) {
        uint64_t now_w;
        memcpy(&now_w, flags + r0, 8);
        take_word(r0, 8, now_w);
    }
    if (full < n_reads) {  // a partial last word
        uint64_t now_w = 0;
        memcpy(&now_w, flags + full, n_reads - full);
        take_word(full, n_reads - full, now_w);
    }
    return sums;
}
