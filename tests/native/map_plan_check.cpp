// Stand-alone check of downpore_amd/csrc/host/map_plan.hpp (tests/test_map_plan_cpu.py builds and runs it, plain and under ASan + UBSan;
// it links the oracle library).  Test infrastructure only.  Every function of the header is held to something that is not the header:
// the oracle's Mapper, a rule written out a second time here, explicit lists, or brute force.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <set>
#include <string>
#include <vector>

#include "map_plan.hpp"
#include "oracle.hpp"

using dph::i64;

namespace {

[[noreturn]] void fail(const char* what, const std::string& detail) {
    fprintf(stderr, "map_plan_check: %s: %s\n", what, detail.c_str());
    exit(1);
}
#define CHECK(cond, detail) \
    do {                    \
        if (!(cond)) fail(#cond, detail); \
    } while (0)

uint64_t rngState = 0x9e3779b97f4a7c15ull;
uint32_t rnd() {
    rngState = rngState * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rngState >> 33);
}
std::string randomBases(i64 n) {
    std::string s((size_t)n, 'A');
    for (char& c : s) c = "ACGT"[rnd() & 3];
    return s;
}

const int K = 11;
std::vector<double> g_values;  // any value table will do: the seeds chosen do not move a chunk

dph::MapParams params(i64 querySize, bool circular, bool all) {
    dph::MapParams p;
    p.k = K;
    p.chunkSize = 100;
    p.querySize = querySize;
    p.seedRate = 40;
    p.circular = circular;
    p.allSequences = all;
    return p;
}

// the schedule loop of mapping.go:79-91 counted, without making anything
unsigned long long countChunksByWalking(const dph::MapParams& p, const std::vector<i64>& lens, bool joinForEvery) {
    unsigned long long n = 0;
    for (i64 L : lens) {
        for (i64 j = 0; j < 10; j++)
            for (i64 i = j * p.chunkSize; i < L - p.chunkSize / 2; i += p.chunkSize * 10 - p.querySize) n++;
        if (p.circular && (joinForEvery || L >= p.querySize)) n++;
    }
    return n;
}

// ---- chunk schedule against the oracle's Mapper: one Mapper per sequence, the ids running on
void checkSchedule(const std::vector<i64>& lens, i64 querySize, bool circular, bool all, const std::string& wantNotes) {
    const dph::MapParams p = params(querySize, circular, all);
    const std::string tag = "lens[0]=" + std::to_string(lens[0]) + " n=" + std::to_string(lens.size()) + " q=" + std::to_string(querySize) + " circ=" + std::to_string(circular);
    std::vector<std::string> seqs, names;
    std::vector<const char*> ptrs;
    for (size_t c = 0; c < lens.size(); c++) {
        seqs.push_back(randomBases(lens[c]));
        names.push_back("s" + std::to_string(c));
    }
    for (const std::string& s : seqs) ptrs.push_back(s.data());
    const dph::MapJoins J = dph::mapJoinChunks(p, lens, ptrs, names);
    const dph::MapSchedule S = dph::mapChunkSchedule(p, lens, J);
    CHECK(J.notes == wantNotes, tag + " notes: " + J.notes);
    CHECK(J.firstPaired == lens.size() + J.joins.size(), tag);
    CHECK(S.items.size() == S.meta.size() && S.items.size() == S.chunkRef.size(), tag);

    size_t at = 0, nJoins = 0;
    const size_t T = lens.size();
    for (size_t c = 0; c < T; c++) {
        const bool hasJoin = circular && (!all || lens[c] >= querySize);
        if (all) CHECK(J.joinOf[c] == (hasJoin ? (int)nJoins : -1), tag + " joinOf");
        else CHECK(J.joinOf[c] == 0 && J.joins.size() == 1, tag + " joinOf (one sequence)");
        if (hasJoin) {  // the last query_size bases, then the first
            const std::string want = seqs[c].substr((size_t)(lens[c] - querySize)) + seqs[c].substr(0, (size_t)querySize);
            CHECK(J.joins[(size_t)J.joinOf[c]] == want, tag + " join chunk's bases");
        }
        const dpo::PackedSeq ref = dpo::newPackedSequence((i64)c, seqs[c], std::make_shared<std::string>(names[c]));
        dpo::Mapper m(ref, hasJoin, K, g_values.data(), p.seedRate, querySize, p.chunkSize);
        const size_t n = m.index.sequences.size();
        CHECK(at + n <= S.items.size(), tag + " fewer chunks than the oracle: " + std::to_string(S.items.size()));
        for (size_t i = 0; i < n; i++, at++) {
            const dpo::SeedSequence* q = m.index.sequences[i];
            const dp_scan_item& it = S.items[at];
            const bool isJoin = hasJoin && i + 1 == n;
            const std::string ctag = tag + " seq " + std::to_string(c) + " chunk " + std::to_string(i);
            CHECK(S.chunkRef[at] == (int)c, ctag + " chunkRef");
            CHECK(S.meta[at].first == q->offset, ctag + " offset " + std::to_string(S.meta[at].first) + " oracle " + std::to_string(q->offset));
            CHECK(S.meta[at].second == q->inset, ctag + " inset " + std::to_string(S.meta[at].second) + " oracle " + std::to_string(q->inset));
            const bool losesFour = isJoin && q->length % 4 == 0;
            CHECK((i64)it.n_kmers + K + (losesFour ? 3 : -1) == q->length, ctag + " n_kmers " + std::to_string(it.n_kmers) + " oracle length " + std::to_string(q->length));
            CHECK(it.min_seeds == 0, ctag);
            if (isJoin) CHECK(it.read == T + nJoins && it.start == 0, ctag + " join chunk's device read");
            else CHECK(it.read == c && (i64)it.start == q->offset, ctag + " device read and start");
        }
        if (hasJoin) nJoins++;
    }
    CHECK(at == S.items.size(), tag + " more chunks than the oracle: " + std::to_string(S.items.size()) + " against " + std::to_string(at));
    CHECK(nJoins == (all ? J.joins.size() : (circular ? 1u : 0u)), tag + " joins");

    // the closed-form count of the limits check: never below the schedule, equal when every sequence has its join chunk (or none has)
    unsigned long long nWin = 0, nChk = 0;
    CHECK(dph::mapCountBounds(p, lens, nWin, nChk), tag);
    CHECK(nChk >= S.items.size(), tag + " closed form below the schedule");
    bool everyJoin = true;
    for (i64 L : lens) everyJoin = everyJoin && (!all || L >= querySize);
    if (everyJoin || !circular) CHECK(nChk == S.items.size(), tag + " closed form " + std::to_string(nChk) + " schedule " + std::to_string(S.items.size()));
    CHECK(countChunksByWalking(p, lens, !all) == S.items.size(), tag + " walked count");
    unsigned long long wantWin = 0;  // AddSingleSeeds' loop, seeds.go:160: i = 0; i < len - seedRate; i += seedRate
    for (i64 L : lens)
        for (i64 i = 0; i < L - p.seedRate; i += p.seedRate) wantWin++;
    CHECK(nWin == wantWin, tag + " seed windows");
}

void scheduleCases() {
    const i64 lens[] = {30, 49, 50, 51, 99, 100, 101, 979, 980, 981, 2100};
    for (i64 q : {20, 21})
        for (int circ = 0; circ < 2; circ++) {
            for (i64 L : lens) checkSchedule({L}, q, circ != 0, false, "");
            // -all_sequences: the middle sequence is shorter than query_size - no join chunk, one line for stderr
            const std::string note = "Sequence s1 (15 bases) is shorter than query_size " + std::string(q == 20 ? "20" : "21") + ": no circular join chunk\n";
            checkSchedule({230, 15, 981}, q, circ != 0, true, circ ? note : "");
            checkSchedule({101, 2100, 51}, q, circ != 0, true, "");
        }
}

// ---- the two refusals, one below each
void limitCases() {
    const std::vector<std::string> names = {"a", "b", "c"};
    std::string err;
    dph::MapParams p;  // the command's defaults
    CHECK(dph::mapCheckLimits(p, {(i64)1 << 31}, names, err) == DP_ERR_ARG, "2^31 bases accepted");
    CHECK(err == "map: the reference sequence is 2147483648 bases long; at most 2147483647 are supported", err);
    err.clear();
    CHECK(dph::mapCheckLimits(p, {((i64)1 << 31) - 1}, names, err) == 0 && err.empty(), "2^31 - 1 bases refused: " + err);
    p.allSequences = true;
    CHECK(dph::mapCheckLimits(p, {5000, (i64)1 << 31}, names, err) == DP_ERR_ARG, "2^31 bases accepted (-all_sequences)");
    CHECK(err == "map: the reference sequence b is 2147483648 bases long; at most 2147483647 are supported", err);
    // seed windows: seed_rate 1 makes len - 1 windows per sequence: 2 (2^31 - 2) + 4 = 2^32 is one too many
    p.seedRate = 1;
    const i64 big = ((i64)1 << 31) - 1;
    const unsigned long long nChk = countChunksByWalking(p, {big, big, 5}, false);
    err.clear();
    CHECK(dph::mapCheckLimits(p, {big, big, 5}, names, err) == DP_ERR_ARG, "2^32 seed windows accepted");
    CHECK(err == "map: the reference has 4294967296 seed windows and " + std::to_string(nChk + 1) + " chunks; fewer than 4294967296 of each are supported", err);
    err.clear();
    CHECK(dph::mapCheckLimits(p, {big, big, 4}, names, err) == 0 && err.empty(), "2^32 - 1 seed windows refused: " + err);
    // chunks: chunk_size 1, query_size 9 give a step of 1, so pass j of a sequence makes len - j chunks (chunk_size / 2 = 0)
    dph::MapParams c;
    c.chunkSize = 1;
    c.querySize = 9;
    c.circular = false;
    c.allSequences = true;
    c.seedRate = 1 << 30;
    // 10 L - 45 chunks per sequence of L bases: 429496734 bases make 2^32 - 1 of them
    const i64 L0 = 429496734;
    unsigned long long w = 0, k0 = 0;
    CHECK(dph::mapCountBounds(c, {L0}, w, k0) && k0 == 4294967295ull, "chunk count of the step-1 schedule: " + std::to_string(k0));
    CHECK(dph::mapCheckLimits(c, {L0}, names, err) == 0 && err.empty(), "2^32 - 1 chunks refused: " + err);
    c.circular = true;  // (the closed form books one join chunk more)
    CHECK(dph::mapCheckLimits(c, {L0}, names, err) == DP_ERR_ARG, "2^32 chunks accepted");
    CHECK(err == "map: the reference has 0 seed windows and 4294967296 chunks; fewer than 4294967296 of each are supported", err);
}

// ---- packed layout, both orders
void packedCases() {
    const std::vector<i64> refLens = {30, 101, 64};
    const std::vector<std::string> joins = {std::string(40, 'A'), std::string(42, 'C')};
    const std::vector<i64> readLens = {1, 4, 5, 63, 64, 65, 127, 128, 129, 3000, 0, 17};
    std::vector<i64> off(1, 7);  // (a read set's offsets need not start at 0)
    for (i64 l : readLens) off.push_back(off.back() + l);
    const size_t T = refLens.size(), nReads = readLens.size(), firstPaired = T + joins.size();
    for (int readsFirst = 0; readsFirst < 2; readsFirst++) {
        const dph::MapPacked P = dph::mapPackedLayout(refLens, joins, off.data(), nReads, readsFirst != 0);
        const std::string tag = readsFirst ? "reads first" : "head first";
        CHECK(P.plens.size() == firstPaired + nReads && P.poff.size() == P.plens.size() + 1, tag);
        CHECK(P.poff[0] == 0, tag);
        for (size_t r = 0; r < P.plens.size(); r++) {
            CHECK(P.poff[r] % 16 == 0 && P.poff[r + 1] % 16 == 0, tag + " offset not on a 16-byte boundary");
            CHECK(P.poff[r + 1] >= P.poff[r] && P.poff[r + 1] - P.poff[r] >= ((uint64_t)P.plens[r] + 3) / 4, tag + " a read does not fit its slot");
            CHECK(P.poff[r + 1] - P.poff[r] < ((uint64_t)P.plens[r] + 3) / 4 + 16, tag + " a slot wider than its read needs");
        }
        // the device ids the rest of the run uses
        const size_t headAt = readsFirst ? nReads : 0, readsAt = readsFirst ? 0 : firstPaired;
        CHECK(P.headAt == headAt && P.readsAt == readsAt, tag + " headAt / readsAt");
        for (size_t c = 0; c < T; c++) CHECK(P.plens[headAt + c] == (uint32_t)refLens[c], tag + " sequence id");
        for (size_t j = 0; j < joins.size(); j++) CHECK(P.plens[headAt + T + j] == joins[j].size(), tag + " join id");
        for (size_t r = 0; r < nReads; r++) CHECK(P.plens[readsAt + r] == (uint32_t)readLens[r], tag + " read id");
    }
}

// ---- window items: the two rules, written out here
void windowCases() {
    const uint32_t firstPaired = 5, read = 3;
    for (i64 L = 44; L <= 52; L++)
        for (i64 a = 0; a <= L; a++)
            for (i64 b = a; b <= L; b++)
                for (int whole = 0; whole < 2; whole++) {
                    if (whole && !(a == 0 && b == L)) continue;
                    dp_scan_item f, r;
                    dph::mapWindowItems(firstPaired, read, L, a, b, whole != 0, K, f, r);
                    const std::string tag = "L=" + std::to_string(L) + " [" + std::to_string(a) + "," + std::to_string(b) + ") whole=" + std::to_string(whole);
                    CHECK(f.read == 11 && r.read == 12 && f.min_seeds == 0 && r.min_seeds == 0, tag);
                    const i64 nk = (b - a) - K + 1;  // k-mers of b - a bases
                    if (whole && L % 4 == 0) {       // the whole read: four k-mers fewer, the reverse strand from base 4
                        const uint32_t want = (uint32_t)(nk - 4 > 0 ? nk - 4 : 0);
                        CHECK(f.start == 0 && r.start == 4 && f.n_kmers == want && r.n_kmers == want, tag + " whole-read rule");
                    } else {  // the plain window, and its mirror image on the reverse strand
                        const uint32_t want = (uint32_t)(nk > 0 ? nk : 0);
                        CHECK(f.start == (uint32_t)a && f.n_kmers == want && r.n_kmers == want, tag + " plain rule");
                        CHECK((i64)r.start + (b - a) == L - a, tag + " the reverse window's last base");
                    }
                    CHECK(dph::mapReverseNeedsFix(true, whole != 0, L) == (whole && L % 4 == 0), tag);
                    CHECK(!dph::mapReverseNeedsFix(false, whole != 0, L), tag);
                }
}

// ---- reverse-strand fix-up against a re-encoding from explicit lists
typedef std::vector<std::pair<i64, int32_t>> Seeds;  // (k-mer index, seed)
std::vector<int32_t> encode(const Seeds& s, int32_t lastGap) {
    std::vector<int32_t> seg;
    for (size_t i = 0; i < s.size(); i++) {
        seg.push_back((int32_t)(i == 0 ? s[0].first : s[i].first - s[i - 1].first - K));
        seg.push_back(s[i].second);
    }
    seg.push_back(lastGap);
    return seg;
}
Seeds decode(const std::vector<int32_t>& seg) {
    Seeds s;
    i64 at = 0;
    for (size_t i = 0; i + 1 < seg.size(); i += 2) {
        at = i == 0 ? seg[0] : at + seg[i] + K;
        s.push_back({at, seg[i + 1]});
    }
    return s;
}
void fixCase(const Seeds& scanned, int32_t lastGap, const char* what) {
    const std::vector<int32_t> before = {7, 99, 3};  // another window's segments in front: they stay
    std::vector<int32_t> segs = before;
    const std::vector<int32_t> enc = encode(scanned, lastGap);
    CHECK(decode(enc) == scanned, what);
    segs.insert(segs.end(), enc.begin(), enc.end());
    dph::mapFixReverseWhole(segs, before.size(), K);
    std::vector<int32_t> want;
    if (scanned.empty()) {
        want = {lastGap + 1};  // no seed: the one gap counts every k-mer, and there is one more
    } else {
        Seeds moved;
        if (scanned[0].first == 0) moved.push_back({0, scanned[0].second});  // k-mer 0 is the k-mer at base 4 once more
        for (const auto& s : scanned) moved.push_back({s.first + 1, s.second});
        want = encode(moved, lastGap);
    }
    CHECK(std::vector<int32_t>(segs.begin(), segs.begin() + 3) == before, what);
    CHECK(std::vector<int32_t>(segs.begin() + 3, segs.end()) == want, what);
}
void fixCases() {
    fixCase({}, 30, "no seed at all");
    fixCase({}, 0, "no seed, no k-mer");
    fixCase({{0, 5}, {K + 2, 6}, {2 * K + 9, 5}}, 4, "first seed at index 0");
    fixCase({{0, 5}, {3, 6}}, 0, "first seed at index 0, the next overlapping it");
    fixCase({{1, 5}, {K + 4, 8}}, 2, "first seed at index 1");
    fixCase({{0, 9}}, 12, "a single seed at index 0");
    fixCase({{6, 9}}, 0, "a single seed further in");
}

// ---- shard merge against brute force: per shard and seed a count and an explicit set of the shard's own 64-chunk words
void mergeCases() {
    struct Held {
        uint32_t count;
        std::set<uint32_t> words;
    };
    const uint32_t S = 5, wordBase[3] = {0, 2, 4};  // shards of 128 chunks
    CHECK(dph::mapChunksPerShard(300, 3) == 128 && dph::mapChunksPerShard(64, 1) == 64 && dph::mapChunksPerShard(65, 1) == 128 && dph::mapChunksPerShard(1, 2) == 64, "chunks per shard");
    // seed 0 in none, 1 in the middle shard only, 2 in all, 3 only in the last, 4 in the first and the last
    const Held held[3][5] = {
        {{0, {}}, {0, {}}, {3, {0, 1}}, {0, {}}, {1, {1}}},
        {{0, {}}, {7, {0, 1}}, {1, {1}}, {0, {}}, {0, {}}},
        {{0, {}}, {0, {}}, {2, {0}}, {4, {1}}, {9, {0, 1}}},
    };
    std::vector<uint32_t> global;
    dph::mapGlobalWindowsInit(global, S);
    CHECK(global.size() == 4 * S, "init size");
    for (int sh = 0; sh < 3; sh++) {
        std::vector<uint32_t> local;
        for (uint32_t i = 0; i < S; i++) {
            const Held& h = held[sh][i];
            if (h.words.empty()) local.insert(local.end(), {0u, 1u, 0u, 1u});
            else local.insert(local.end(), {h.count, *h.words.begin(), *h.words.rbegin(), *h.words.rbegin() + 1});
        }
        dph::mapGlobalWindowsMerge(global, local, S, wordBase[sh]);
    }
    for (uint32_t i = 0; i < S; i++) {
        uint32_t count = 0;
        std::set<uint32_t> words;
        for (int sh = 0; sh < 3; sh++) {
            count += held[sh][i].count;
            for (uint32_t w : held[sh][i].words) words.insert(w + wordBase[sh]);
        }
        const uint32_t* g = &global[4 * i];
        const std::string tag = "seed " + std::to_string(i);
        if (words.empty()) CHECK(g[0] == 0 && g[1] == 1 && g[2] == 0 && g[3] == 1, tag + " in no shard");
        else CHECK(g[0] == count && g[1] == *words.begin() && g[2] == *words.rbegin() && g[3] == *words.rbegin() + 1, tag);
    }
}

// ---- dense estimate and layout choice
uint64_t denseByHand(uint64_t S, uint64_t m) {  // S rows of ceil(m / 64) words and m rows of ceil(S / 64) words, 8 bytes each
    return 8 * (S * ((m + 63) / 64) + m * ((S + 63) / 64));
}
void layoutCases() {
    CHECK(dph::mapDenseBytes(1000, 300) == denseByHand(1000, 300) && dph::mapDenseBytes(1000, 300) == 8 * (1000 * 5 + 300 * 16), "dense bytes");
    // 300 chunks in shards of 128, 128, 44 dealt over devices 2, 0, 2
    const auto perDev = dph::mapDenseEstimate(1000, 300, 3, 128, {2, 0}, 7, 0);
    CHECK(perDev.size() == 2 && perDev[0].first == 2 && perDev[1].first == 0, "devices in the order of first use");
    CHECK(perDev[0].second == denseByHand(1000, 128) + denseByHand(1000, 44) && perDev[1].second == denseByHand(1000, 128), "bytes per device");
    const auto one = dph::mapDenseEstimate(1000, 300, 1, 320, {2, 0}, 7, 6);  // not sharded: a whole index per mapper thread on the run's device
    CHECK(one.size() == 1 && one[0].first == 7 && one[0].second == 6 * denseByHand(1000, 300), "unsharded estimate");
    // over exactly where bytes + total / 8 > free
    const uint64_t total = 1000003, bytes = 500000, edge = bytes + total / 8;
    CHECK(!dph::mapDenseOver(bytes, edge, total), "over at the edge");
    CHECK(dph::mapDenseOver(bytes, edge - 1, total), "not over one byte below");
    CHECK(dph::mapDenseOver(bytes + 1, edge, total), "not over one byte above");
    CHECK(!dph::mapDenseOver(bytes - 1, edge - 1, total), "over with both one less");
    uint64_t dTotal = 0;
    const std::vector<std::pair<int, uint64_t>> two = {{0, bytes}, {1, bytes}};
    CHECK(dph::mapDenseOverAny(two, {{edge, total}, {edge - 1, total}}, &dTotal) && dTotal == 2 * bytes, "only the second device over");
    CHECK(!dph::mapDenseOverAny(two, {{edge, total}, {edge, total}}, &dTotal) && dTotal == 2 * bytes, "no device over");
    CHECK(dph::mapDenseOverAny(two, {{edge - 1, total}, {edge, total}}, &dTotal), "only the first device over");
}

}  // namespace

int main() {
    g_values.resize((size_t)1 << (2 * K));
    for (double& v : g_values) v = 1.0 + (rnd() % 1000);
    scheduleCases();
    limitCases();
    packedCases();
    windowCases();
    fixCases();
    mergeCases();
    layoutCases();
    puts("ok");
    return 0;
}
