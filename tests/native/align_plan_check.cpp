// align_plan.hpp (downpore_amd/csrc/host) by itself, without a GPU: the strand flip, the circular wrap, every out-of-range clause on
// both sides of its boundary, the device item and the text of the tags.  Built plain and under ASan + UBSan by
// tests/test_align_plan_cpu.py; prints "ok" or the first failed check.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "align_plan.hpp"

using namespace dph;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
            return 1;                                                        \
        }                                                                    \
    } while (0)

static AlignLine line(int64_t L, int64_t qOffset, int64_t qInset, int64_t start, int64_t end, bool rc, int ref = 0) {
    AlignLine ln;
    ln.L = L, ln.queryOffset = qOffset, ln.queryInset = qInset, ln.start = start, ln.end = end, ln.rc = rc, ln.ref = ref;
    return ln;
}

// the rule written out a second time, on strings: the query's bases from the forward read / the target's from the sequence
static std::string revComp(const std::string& s) {
    std::string r(s.rbegin(), s.rend());
    for (char& c : r) c = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A';
    return r;
}

int main() {
    AlignSpan s;
    // ---- strand flip, on both sides of L % 4 (the packed layout's byte boundary plays no part in the arithmetic: L = 8, 9, 10, 11)
    for (int64_t L = 8; L <= 11; L++) {
        std::string read;
        for (int64_t i = 0; i < L; i++) read += "ACGT"[(i * 7 + L) % 4];
        const std::string rc = revComp(read);
        for (int64_t qs = 0; qs < L; qs++)
            for (int64_t qe = qs + 1; qe <= L; qe++) {
                CHECK(alignSpanOf(line(L, qs, L - qe, 0, qe - qs, false), 100, true, s));
                CHECK(s.qOff == qs && s.qLen == qe - qs);
                CHECK(read.substr((size_t)s.qOff, (size_t)s.qLen) == read.substr((size_t)qs, (size_t)(qe - qs)));
                CHECK(alignSpanOf(line(L, qs, L - qe, 0, qe - qs, true), 100, true, s));
                CHECK(s.qOff == L - qe && s.qLen == qe - qs);
                // the reverse complement of read[qs, qe) is rc_read[L - qe, L - qs)
                CHECK(rc.substr((size_t)s.qOff, (size_t)s.qLen) == revComp(read.substr((size_t)qs, (size_t)(qe - qs))));
            }
    }
    // ---- the target: End - Start, plus Lr when circular and negative
    const int64_t Lr = 1000;
    CHECK(alignSpanOf(line(50, 0, 0, 100, 150, false), Lr, true, s) && s.tOff == 100 && s.tLen == 50);
    CHECK(alignSpanOf(line(50, 0, 0, 100, 150, false), Lr, false, s) && s.tOff == 100 && s.tLen == 50);
    // wrap at Start = Lr - 1: one base before the end, the rest from 0
    CHECK(alignSpanOf(line(50, 0, 0, Lr - 1, 49, false), Lr, true, s) && s.tOff == Lr - 1 && s.tLen == 50);
    CHECK(!alignSpanOf(line(50, 0, 0, Lr - 1, 49, false), Lr, false, s));  // (linear: the length is negative)
    // Start = Lr (the reference's start == Len() quirk): the modulo makes it base 0
    CHECK(alignSpanOf(line(50, 0, 0, Lr, 50, false), Lr, true, s) && s.tOff == Lr && s.tLen == 50);
    CHECK(!alignSpanOf(line(50, 0, 0, Lr + 1, 51, false), Lr, true, s));  // Start > Lr
    CHECK(!alignSpanOf(line(50, 0, 0, Lr, Lr + 50, false), Lr, false, s));  // linear: End > Lr
    // End = 0: the target ends with the sequence's last base
    CHECK(alignSpanOf(line(50, 0, 0, Lr - 50, 0, false), Lr, true, s) && s.tOff == Lr - 50 && s.tLen == 50);
    CHECK(!alignSpanOf(line(50, 0, 0, Lr - 50, 0, false), Lr, false, s));
    CHECK(alignSpanOf(line(50, 0, 0, Lr - 50, Lr, false), Lr, false, s) && s.tLen == 50);  // linear: End = Lr is the last legal one
    // ---- every out-of-range clause, on both sides of its boundary
    CHECK(alignSpanOf(line(50, 0, 0, 0, 50, false), Lr, true, s));        // qs = 0
    CHECK(!alignSpanOf(line(50, -1, 0, 0, 50, false), Lr, true, s));      // qs < 0
    CHECK(alignSpanOf(line(50, 10, 0, 0, 40, false), Lr, true, s));       // qe = L
    CHECK(!alignSpanOf(line(50, 10, -1, 0, 40, false), Lr, true, s));     // qe > L
    CHECK(alignSpanOf(line(50, 24, 25, 0, 1, false), Lr, true, s) && s.qLen == 1);  // qs = qe - 1
    CHECK(!alignSpanOf(line(50, 25, 25, 0, 1, false), Lr, true, s));      // qs = qe
    CHECK(!alignSpanOf(line(50, 26, 25, 0, 1, false), Lr, true, s));      // qs > qe
    CHECK(alignSpanOf(line(50, 0, 0, 10, 11, false), Lr, true, s) && s.tLen == 1);  // tl = 1
    CHECK(!alignSpanOf(line(50, 0, 0, 10, 10, false), Lr, true, s));      // tl = 0
    CHECK(!alignSpanOf(line(50, 0, 0, 10, 10, false), Lr, false, s));
    CHECK(alignSpanOf(line(50, 0, 0, 0, Lr, false), Lr, true, s) && s.tLen == Lr);  // tl = Lr
    CHECK(!alignSpanOf(line(50, 0, 0, 0, Lr + 1, false), Lr, true, s));   // tl > Lr
    CHECK(alignSpanOf(line(50, 0, 0, 0, 50, false), Lr, false, s));       // Start = 0
    CHECK(!alignSpanOf(line(50, 0, 0, -1, 49, false), Lr, false, s));     // Start < 0
    CHECK(!alignSpanOf(line(50, 0, 0, -1, 49, false), Lr, true, s));
    {
        const int64_t big = kAlignMaxSpan, bigLr = 4 * kAlignMaxSpan;
        CHECK(alignSpanOf(line(big, 0, 0, 0, 50, false), bigLr, true, s) && s.qLen == big);  // qe - qs = 2^20
        CHECK(!alignSpanOf(line(big + 1, 0, 0, 0, 50, false), bigLr, true, s));
        CHECK(alignSpanOf(line(50, 0, 0, 7, 7 + big, false), bigLr, true, s) && s.tLen == big);  // tl = 2^20
        CHECK(!alignSpanOf(line(50, 0, 0, 7, 8 + big, false), bigLr, true, s));
    }
    // ---- the device item: forward read firstPaired + 2 r, reverse strand + 1, reference sequence c
    CHECK(alignSpanOf(line(40, 5, 7, Lr - 3, 20, true, 2), Lr, true, s));
    {
        const dp_align_item it = alignItemOf(s, 6, 11, true, 2);
        CHECK(it.q_read == 6 + 22 + 1 && it.q_off == 7 && it.q_len == 28 && it.t_read == 2 && it.t_off == (uint32_t)(Lr - 3) && it.t_len == 23);
        const dp_align_item fw = alignItemOf(s, 6, 11, false, 0);
        CHECK(fw.q_read == 28 && fw.t_read == 0);
    }
    // ---- run words to text
    {
        const std::vector<uint32_t> runs = {1u << 2 | 2u, 3u << 2 | 0u, 12u << 2 | 1u, 1048576u << 2 | 0u};
        CHECK(alignCigarText(runs.data(), (uint32_t)runs.size()) == "1D3M12I1048576M");
        CHECK(alignCigarText(nullptr, 0) == "");
        CHECK(alignTags(17, runs.data(), 2) == "\tNM:i:17\tcg:Z:1D3M");
        CHECK(alignTags(0, runs.data() + 1, 1) == "\tNM:i:0\tcg:Z:3M");
        int64_t q = 0, t = 0;
        alignConsumed(runs.data(), 3, q, t);
        CHECK(q == 15 && t == 4);
    }
    printf("ok\n");
    return 0;
}
