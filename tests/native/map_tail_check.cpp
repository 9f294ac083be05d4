// A Mapper batch's layout arithmetic (downpore_amd/csrc/host/map_plan.hpp: mapBatchLayout, mapBatchReadId) held to brute force and to
// mapPackedLayout of head + batch, without a GPU: what dp_reads_replace_tail_packed_rc is given for a batch must be what an upload of
// the head and the batch in one go would have been given for the batch's part.  Prints "ok", or the first difference and exits 1.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "map_plan.hpp"

using namespace dph;

namespace {
int fails = 0;
#define CHECK(cond, ...)                    \
    do {                                    \
        if (!(cond)) {                      \
            fprintf(stderr, __VA_ARGS__);   \
            fprintf(stderr, "\n");          \
            if (++fails > 20) exit(1);      \
        }                                   \
    } while (0)

// the host layout written out a second time: a read's packed bytes, rounded up to 16, one after the other
uint64_t bruteOffset(const std::vector<i64>& lens, size_t r) {
    uint64_t o = 0;
    for (size_t i = 0; i < r; i++) {
        uint64_t bytes = 0;
        for (i64 b = 0; b < lens[i]; b += 4) bytes++;
        while (bytes % 16) bytes++;
        o += bytes;
    }
    return o;
}

void oneCase(const std::vector<i64>& refLens, const std::vector<std::string>& joins, const std::vector<i64>& lens, const char* what) {
    std::vector<i64> off(1, 100);  // (a read set's offsets need not start at 0)
    for (i64 l : lens) off.push_back(off.back() + l);
    const size_t n = lens.size(), firstPaired = refLens.size() + joins.size();
    const MapPacked B = mapBatchLayout(off.data(), n);
    CHECK(B.headAt == 0 && B.readsAt == 0, "%s: a batch block starts with its first read", what);
    CHECK(B.plens.size() == n && B.poff.size() == n + 1, "%s: %zu reads, %zu lengths, %zu offsets", what, n, B.plens.size(), B.poff.size());
    for (size_t r = 0; r < n; r++) {
        CHECK((i64)B.plens[r] == lens[r], "%s: length of read %zu", what, r);
        CHECK(B.poff[r] == bruteOffset(lens, r), "%s: offset of read %zu is %llu, brute force %llu", what, r, (unsigned long long)B.poff[r], (unsigned long long)bruteOffset(lens, r));
        CHECK(B.poff[r] % 16 == 0, "%s: read %zu not on a 16-byte boundary", what, r);
    }
    CHECK(B.poff[n] == bruteOffset(lens, n), "%s: block size", what);
    // against the one-go layout of head + batch: the batch's part of it, moved to the block's start
    const MapPacked P = mapPackedLayout(refLens, joins, off.data(), n, false);
    CHECK(P.readsAt == firstPaired && P.plens.size() == firstPaired + n, "%s: one-go layout", what);
    for (size_t r = 0; r <= n; r++)
        CHECK(P.poff[firstPaired + r] - P.poff[firstPaired] == B.poff[r], "%s: read %zu sits %llu bytes behind the head in one go, %llu in the batch block", what, r,
              (unsigned long long)(P.poff[firstPaired + r] - P.poff[firstPaired]), (unsigned long long)B.poff[r]);
    for (size_t r = 0; r < n; r++) CHECK(P.plens[firstPaired + r] == B.plens[r], "%s: one-go length of read %zu", what, r);
    // device ids: the device set of an upload with first_paired = firstPaired, listed by brute force
    std::vector<std::pair<uint32_t, bool>> dev;  // device read -> (batch read, reverse)
    for (size_t h = 0; h < firstPaired; h++) dev.push_back({0xffffffffu, false});
    for (size_t r = 0; r < n; r++) {
        dev.push_back({(uint32_t)r, false});
        dev.push_back({(uint32_t)r, true});
    }
    for (size_t r = 0; r < n; r++)
        for (int s = 0; s < 2; s++) {
            const uint32_t id = mapBatchReadId((uint32_t)firstPaired, (uint32_t)r, s != 0);
            CHECK(id < dev.size() && dev[id].first == (uint32_t)r && dev[id].second == (s != 0), "%s: device id of read %zu strand %d", what, r, s);
        }
    // ... and they are the ids a window request names (mapWindowItems)
    for (size_t r = 0; r < n; r++) {
        if (lens[r] < 12) continue;
        dp_scan_item f, v;
        mapWindowItems((uint32_t)firstPaired, (uint32_t)r, lens[r], 0, lens[r], true, 11, f, v);
        CHECK(f.read == mapBatchReadId((uint32_t)firstPaired, (uint32_t)r, false) && v.read == f.read + 1, "%s: window items of read %zu", what, r);
    }
}
}  // namespace

int main() {
    const std::vector<i64> edge = {1, 3, 4, 15, 16, 17, 63, 64, 65, 0, 66, 127, 128, 129, 1000, 1001, 1002, 1003};
    oneCase({}, {}, {}, "nothing at all");
    oneCase({5000}, {std::string(2000, 'A')}, {}, "empty batch");
    oneCase({5000}, {std::string()}, edge, "edge lengths, empty join slot");
    oneCase({5000, 7, 63}, {std::string(2000, 'C'), std::string(2000, 'G')}, edge, "edge lengths, three sequences");
    std::vector<i64> mod16;
    for (i64 l = 64; l < 64 + 64; l++) mod16.push_back(l);  // every length % 16 (and % 64), byte sizes on both sides of a 16-byte step
    oneCase({12345}, {std::string(2000, 'T')}, mod16, "all residues");
    std::mt19937_64 rng(7);
    for (int it = 0; it < 200; it++) {
        std::vector<i64> refLens(1 + rng() % 4), lens(rng() % 40);
        for (i64& l : refLens) l = (i64)(rng() % 30000);
        for (i64& l : lens) l = (i64)(rng() % (it % 2 ? 70 : 20000));
        std::vector<std::string> joins(rng() % (refLens.size() + 1), std::string((size_t)(rng() % 3000), 'A'));
        oneCase(refLens, joins, lens, "random");
    }
    {  // the largest length the device call takes
        const std::vector<i64> big = {0x7fffffff, 1};
        oneCase({1}, {}, big, "2^31 - 1 bases");
    }
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
