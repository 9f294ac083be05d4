// Stand-alone check of downpore_amd/csrc/dp_scan_flags.h (tests/test_scan_flags_cpu.py builds it plain and with ASan + UBSan):
// the shadow of the ignore flags and the two sums dp_scan_reads reports, against a brute-force recount after every step.
// Prints "ok".  Every array has exactly the size the header is promised, on the heap, so that a sanitizer sees a step too far.
#include <stdio.h>

#include <memory>
#include <random>
#include <vector>

#include "dp_scan_flags.h"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stdout, "FAILED line %d: %s\n", __LINE__, #c);    \
            return false;                                             \
        }                                                             \
    } while (0)

// the recount: k-mers counted one start position at a time
static uint64_t bases_examined(uint32_t len, int k, int top_level) {
    int64_t kmers = 0;
    for (int64_t p = 0; p + k <= (int64_t)len; p++) kmers++;
    if (top_level && len % 4 == 0) kmers -= 4;
    return kmers > 0 ? (uint64_t)kmers + (uint64_t)k - 1 : 0;
}
static dp_flag_sums recount(const uint8_t* flags, const uint32_t* len, const dp_flag_view& v) {
    dp_flag_sums s = {0, 0};
    for (uint32_t r = v.lo; r < v.hi; r++)
        if (!flags[r]) s.bases += bases_examined(len[r], v.k, v.top_level), s.reads++;
    return s;
}

// what a context keeps between two calls, and a call's flags step as dp_scan.hip makes it
struct Book {
    uint32_t n_reads;
    size_t shadow_bytes;
    std::unique_ptr<uint32_t[]> len;
    std::unique_ptr<uint8_t[]> shadow, flags;  // flags: the caller's array
    bool valid = false;
    dp_flag_view view = {0, 0, 0, 0};
    dp_flag_sums sums = {0, 0};

    explicit Book(uint32_t n) : n_reads(n), shadow_bytes((((size_t)n + 7) & ~(size_t)7) + 64), len(new uint32_t[n]), shadow(new uint8_t[shadow_bytes]), flags(new uint8_t[n]) {
        memset(shadow.get(), 0xee, shadow_bytes);  // (a fresh pinned block holds anything)
        memset(flags.get(), 0, n);
        for (uint32_t r = 0; r < n; r++) len[r] = 3000 + r;
    }
    bool step(const dp_flag_view& v, bool expect_same) {
        const bool same = valid && dp_flag_view_same(view, v);
        CHECK(same == expect_same);
        sums = dp_scan_flags_update(shadow.get(), shadow_bytes, flags.get(), n_reads, len.get(), v, same, sums);
        valid = true;
        view = v;
        CHECK(n_reads == 0 || memcmp(shadow.get(), flags.get(), n_reads) == 0);
        for (size_t i = n_reads; i < shadow_bytes; i++) CHECK(shadow[i] == 0);
        const dp_flag_sums want = recount(flags.get(), len.get(), v);
        CHECK(sums.bases == want.bases && sums.reads == want.reads);
        return true;
    }
};

// the cases the header's comment names, one at a time, on 43 reads (a partial last word) and a sub-range
static bool named_cases() {
    Book b(43);
    const int k = 10;
    b.len[6] = 5;  // shorter than k: no k-mer, no base
    b.len[7] = 9;
    b.len[8] = 10;  // exactly one k-mer
    const dp_flag_view sub = {5, 30, 0, k};
    CHECK(dp_flag_bases_of(5, sub) == 0 && dp_flag_bases_of(9, sub) == 0 && dp_flag_bases_of(10, sub) == 10 && dp_flag_bases_of(3000, sub) == 3000);
    CHECK(b.step(sub, false));
    CHECK(b.sums.reads == 25);
    const dp_flag_sums s0 = b.sums;
    // 0 -> 1 inside the range, and changes outside it (before, behind, in the partial last word)
    b.flags[12] = 1, b.flags[2] = 1, b.flags[31] = 1, b.flags[42] = 1;
    CHECK(b.step(sub, true));
    CHECK(b.sums.reads == s0.reads - 1 && b.sums.bases == s0.bases - 3012);
    // 1 -> 2: the sums stay, the shadow takes the 2
    b.flags[12] = 2, b.flags[42] = 2;
    const dp_flag_sums s1 = b.sums;
    CHECK(b.step(sub, true));
    CHECK(b.sums.reads == s1.reads && b.sums.bases == s1.bases && b.shadow[12] == 2 && b.shadow[42] == 2);
    // 2 -> 0 and 1 -> 0
    b.flags[12] = 0, b.flags[2] = 0;
    CHECK(b.step(sub, true));
    CHECK(b.sums.reads == s0.reads && b.sums.bases == s0.bases);
    // the read without a k-mer: a read less, no base less
    b.flags[6] = 1;
    CHECK(b.step(sub, true));
    CHECK(b.sums.reads == s0.reads - 1 && b.sums.bases == s0.bases);
    // nothing changed
    CHECK(b.step(sub, true));
    // lo == hi, then the whole range: view changes, recounted
    CHECK(b.step(dp_flag_view{17, 17, 0, k}, false));
    CHECK(b.sums.reads == 0 && b.sums.bases == 0);
    b.flags[17] = 1;
    CHECK(b.step(dp_flag_view{17, 17, 0, k}, true));
    CHECK(b.sums.reads == 0 && b.sums.bases == 0);
    CHECK(b.step(dp_flag_view{0, 43, 0, k}, false));
    // another k alone is another view
    CHECK(b.step(dp_flag_view{0, 43, 0, k + 1}, false));
    // an invalidated shadow (a call that left before its launch; a pinned block that grew): everything once
    b.flags[20] = 1;
    b.valid = false;
    memset(b.shadow.get(), 0xee, b.shadow_bytes);
    CHECK(b.step(dp_flag_view{0, 43, 0, k + 1}, false));
    return true;
}

// top_level: a length that is a multiple of four has four k-mers fewer; lengths 0, 1, 2 and 3 mod 4, and reads that end up without a k-mer
static bool top_level_cases() {
    const int k = 10;
    const dp_flag_view top = {0, 8, 1, k}, plain = {0, 8, 0, k};
    CHECK(dp_flag_bases_of(3000, top) == 2996 && dp_flag_bases_of(3001, top) == 3001 && dp_flag_bases_of(3002, top) == 3002 &&
          dp_flag_bases_of(3003, top) == 3003 && dp_flag_bases_of(3000, plain) == 3000);
    CHECK(dp_flag_bases_of(12, top) == 0 && dp_flag_bases_of(12, plain) == 12 && dp_flag_bases_of(16, top) == 12 && dp_flag_bases_of(0, top) == 0);
    Book b(8);
    const uint32_t lens[8] = {3000, 3001, 3002, 3003, 12, 13, 16, 0};
    for (int r = 0; r < 8; r++) b.len[r] = lens[r];
    CHECK(b.step(plain, false));
    CHECK(b.step(top, false));
    for (int r = 0; r < 8; r++) {
        b.flags[r] = 1;
        CHECK(b.step(top, true));
    }
    for (int r = 7; r >= 0; r--) {
        b.flags[r] = 0;
        CHECK(b.step(top, true));
    }
    return true;
}

// seeded random sequences of flag arrays, views and invalidations
static bool random_sequences(uint32_t n, uint32_t seed) {
    std::mt19937 rng(seed);
    auto below = [&](uint32_t m) { return m ? (uint32_t)(rng() % m) : 0u; };
    Book b(n);
    for (uint32_t r = 0; r < n; r++) b.len[r] = below(3) ? 2990 + below(24) : below(24);
    dp_flag_view v = {0, n, 0, 10};
    CHECK(b.step(v, false));
    for (int it = 0; it < 200; it++) {
        const uint32_t changes = below(4) ? below(5) : below(n + 1);
        for (uint32_t c = 0; c < changes && n; c++) b.flags[below(n)] = (uint8_t)(below(3) ? below(3) : below(256));
        bool same = true;
        const uint32_t what = below(10);
        if (what == 0) {  // another view
            const uint32_t lo = below(n + 1), hi = lo + below(n - lo + 1);
            const dp_flag_view w = {lo, hi, (int)below(2), 4 + (int)below(12)};
            same = dp_flag_view_same(v, w);
            v = w;
        } else if (what == 1) {
            b.valid = same = false;
            memset(b.shadow.get(), 0xee, b.shadow_bytes);
        }
        CHECK(b.step(v, same));
    }
    return true;
}

int main() {
    if (!named_cases() || !top_level_cases()) return 1;
    const uint32_t sizes[] = {0, 1, 7, 8, 9, 43, 64, 1000};
    for (uint32_t n : sizes)
        for (uint32_t seed = 1; seed <= 4; seed++)
            if (!random_sequences(n, 1000 * n + seed)) {
                fprintf(stdout, "(n_reads %u, seed %u)\n", n, 1000 * n + seed);
                return 1;
            }
    printf("ok\n");
    return 0;
}
