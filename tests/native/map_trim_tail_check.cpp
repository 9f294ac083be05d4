// The arithmetic a Mapper's trimmed batch adds (downpore_amd/csrc/host/map_plan.hpp: mapTailId, mapTailIds, mapTailSpans), without a GPU.
// The raw batch goes behind the head unpaired, so raw read r is device read base + r: the trim's id lists and the spans handed to
// dp_reads_respan_tail_rc are the host's with `read` moved by the head's size and nothing else.  Held to the rule written out a second
// time - the device set listed by brute force - and to the identity spans[i].read - keep == cut[i].read for shuffled and repeated
// reads; and the ids of the pairs the respan leaves behind are the ones a window request names.  Prints "ok", or the first difference
// and exits 1.
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

void oneCase(const std::vector<i64>& refLens, const std::vector<std::string>& joins, size_t nRaw, const std::vector<dp_read_span>& cut, const char* what) {
    const uint32_t keep = (uint32_t)(refLens.size() + joins.size());
    // the device set after dp_reads_replace_tail_packed, listed by brute force: the head, then every raw read once
    std::vector<long> dev;  // device read -> raw read, -1 for a read of the head
    for (size_t c = 0; c < refLens.size(); c++) dev.push_back(-1);
    for (size_t j = 0; j < joins.size(); j++) dev.push_back(-1);
    for (size_t r = 0; r < nRaw; r++) dev.push_back((long)r);
    std::vector<uint32_t> reads;
    for (size_t r = 0; r < nRaw; r += 1 + r % 3) reads.push_back((uint32_t)r);  // an id list with gaps, as the eligible reads are
    const std::vector<uint32_t> ids = mapTailIds(reads, keep);
    CHECK(ids.size() == reads.size(), "%s: %zu ids for %zu reads", what, ids.size(), reads.size());
    for (size_t i = 0; i < ids.size(); i++) {
        CHECK(ids[i] < dev.size() && dev[ids[i]] == (long)reads[i], "%s: id %zu names device read %u, which is not raw read %u", what, i, ids[i], reads[i]);
        CHECK(ids[i] == mapTailId(keep, reads[i]) && ids[i] >= keep, "%s: id %zu", what, i);
    }
    if (keep == 0) CHECK(ids == reads, "%s: no head, no offset", what);
    const std::vector<dp_read_span> spans = mapTailSpans(cut, keep);
    CHECK(spans.size() == cut.size(), "%s: %zu spans for %zu cuts", what, spans.size(), cut.size());
    for (size_t i = 0; i < spans.size(); i++) {
        CHECK(spans[i].read >= keep && spans[i].read - keep == cut[i].read, "%s: span %zu names read %u, cut %u, keep %u", what, i, spans[i].read, cut[i].read, keep);
        CHECK(spans[i].read < dev.size() && dev[spans[i].read] == (long)cut[i].read, "%s: span %zu is not a span of raw read %u", what, i, cut[i].read);
        CHECK(spans[i].start == cut[i].start && spans[i].len == cut[i].len, "%s: span %zu moved within its read", what, i);
    }
    // the device set after dp_reads_respan_tail_rc, by brute force: the head, then (span, reverse) per cut - the ids the mapper's
    // threads ask for (mapBatchReadId of trimmed read i)
    std::vector<std::pair<long, bool>> after;
    for (uint32_t h = 0; h < keep; h++) after.push_back({-1, false});
    for (size_t i = 0; i < cut.size(); i++) {
        after.push_back({(long)i, false});
        after.push_back({(long)i, true});
    }
    for (size_t i = 0; i < cut.size(); i++)
        for (int s = 0; s < 2; s++) {
            const uint32_t id = mapBatchReadId(keep, (uint32_t)i, s != 0);
            CHECK(id < after.size() && after[id].first == (long)i && after[id].second == (s != 0), "%s: device id of trimmed read %zu strand %d", what, i, s);
        }
}
}  // namespace

int main() {
    oneCase({}, {}, 0, {}, "nothing at all");
    oneCase({5000}, {std::string(2000, 'A')}, 0, {}, "empty batch");
    oneCase({}, {}, 4, {{3, 0, 5}, {0, 1, 2}}, "no head");
    oneCase({5000}, {std::string()}, 5, {{4, 10, 100}, {4, 10, 100}, {0, 0, 1}, {4, 0, 7}, {2, 3, 0}}, "one read three times, out of order");
    std::mt19937_64 rng(11);
    for (int it = 0; it < 300; it++) {
        std::vector<i64> refLens(rng() % 5);
        for (i64& l : refLens) l = (i64)(rng() % 30000);
        std::vector<std::string> joins(rng() % (refLens.size() + 1), std::string((size_t)(rng() % 3000), 'A'));
        const size_t nRaw = rng() % 60;
        std::vector<dp_read_span> cut;
        if (nRaw) {
            // the order trimmedReadSet gives - reads in file order, then the halves of split reads - then shuffled, with repeats
            for (size_t r = 0; r < nRaw; r++)
                if (rng() % 4) cut.push_back(dp_read_span{(uint32_t)r, (uint32_t)(rng() % 100), (uint32_t)(rng() % 5000)});
            for (int e = 0; e < (int)(rng() % 6); e++) cut.push_back(dp_read_span{(uint32_t)(rng() % nRaw), (uint32_t)(rng() % 100), (uint32_t)(rng() % 5000)});
            if (it % 2)
                for (size_t i = cut.size(); i > 1; i--) std::swap(cut[i - 1], cut[rng() % i]);
            if (it % 3 == 0 && !cut.empty()) cut.push_back(cut[rng() % cut.size()]);
        }
        oneCase(refLens, joins, nRaw, cut, "random");
    }
    {  // ids near the top of the 32-bit range the device call takes
        const uint32_t keep = 3;
        const std::vector<uint32_t> top = {0x7ffffff0u, 0x7ffffffbu};
        const std::vector<uint32_t> ids = mapTailIds(top, keep);
        CHECK(ids[0] == 0x7ffffff3u && ids[1] == 0x7ffffffeu, "large ids");
    }
    if (fails) return 1;
    printf("ok\n");
    return 0;
}
