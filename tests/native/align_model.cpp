// Model of the alignment rule of DESIGN.md 4.9 (NM and the canonical CIGAR), written from the rule alone: the full (m + 1) x (n + 1)
// matrix of unit-cost edit distances, two bits per cell for the move the walk takes there, and the walk back from (m, n).  No band,
// no device, nothing of the product's code.  tests/align_model.py compiles and loads it.
//
//   D[i][0] = i, D[0][j] = j, D[i][j] = min(D[i-1][j-1] + (Q[i-1] != T[j-1]), D[i-1][j] + 1, D[i][j-1] + 1)
//   at (i, j) the walk takes the first that applies: M if i, j > 0 and D[i-1][j-1] + (Q[i-1] != T[j-1]) == D[i][j];
//   else I (consumes the query) if i > 0 and D[i-1][j] + 1 == D[i][j]; else D.  Equal moves are merged into runs.
//
// mutation 1 prefers I over M, mutation 2 tests D before I: two wrong walks the hand-worked cases must tell from the right one.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace {
enum { OP_M = 0, OP_I = 1, OP_D = 2 };

int64_t alignModel(const uint8_t* q, int64_t m, const uint8_t* t, int64_t n, int mutation, std::string& cigar) {
    const int64_t cols = n + 1;
    std::vector<uint8_t> moves((size_t)(((m + 1) * cols + 3) / 4), 0);
    auto setMove = [&](int64_t i, int64_t j, int op) { moves[(size_t)((i * cols + j) >> 2)] |= (uint8_t)(op << (((i * cols + j) & 3) << 1)); };
    auto getMove = [&](int64_t i, int64_t j) { return (moves[(size_t)((i * cols + j) >> 2)] >> (((i * cols + j) & 3) << 1)) & 3; };
    std::vector<int64_t> prev((size_t)cols), cur((size_t)cols);
    for (int64_t j = 0; j <= n; j++) {
        prev[(size_t)j] = j;
        setMove(0, j, OP_D);
    }
    for (int64_t i = 1; i <= m; i++) {
        cur[0] = i;
        setMove(i, 0, OP_I);
        for (int64_t j = 1; j <= n; j++) {
            const int64_t dg = prev[(size_t)(j - 1)] + (q[i - 1] != t[j - 1] ? 1 : 0), up = prev[(size_t)j] + 1, lf = cur[(size_t)(j - 1)] + 1;
            const int64_t d = std::min(dg, std::min(up, lf));
            cur[(size_t)j] = d;
            int op;
            if (mutation == 1) op = up == d ? OP_I : dg == d ? OP_M : OP_D;
            else if (mutation == 2) op = dg == d ? OP_M : lf == d ? OP_D : OP_I;
            else op = dg == d ? OP_M : up == d ? OP_I : OP_D;
            setMove(i, j, op);
        }
        prev.swap(cur);
    }
    const int64_t nm = prev[(size_t)n];
    // the walk, last run first
    std::vector<std::pair<int, int64_t>> runs;
    for (int64_t i = m, j = n; i > 0 || j > 0;) {
        const int op = getMove(i, j);
        if (!runs.empty() && runs.back().first == op) runs.back().second++;
        else runs.emplace_back(op, 1);
        if (op == OP_M) i--, j--;
        else if (op == OP_I) i--;
        else j--;
    }
    cigar.clear();
    for (size_t r = runs.size(); r-- > 0;) {
        cigar += std::to_string((long long)runs[r].second);
        cigar += "MID"[runs[r].first];
    }
    return nm;
}
}  // namespace

// q, t: one code per byte (any values; equal bytes match).  The CIGAR's text goes to cigar[0 .. cap) when it fits; *cigar_len is its length.
extern "C" int64_t alm_align(const uint8_t* q, int64_t m, const uint8_t* t, int64_t n, int mutation, char* cigar, int64_t cap, int64_t* cigar_len) {
    std::string s;
    const int64_t nm = alignModel(q, m, t, n, mutation, s);
    *cigar_len = (int64_t)s.size();
    if ((int64_t)s.size() <= cap) memcpy(cigar, s.data(), s.size());
    return nm;
}
