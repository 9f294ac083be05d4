// Product host side of `downpore map` (mapping/mapping.go, commands/map.go:33-116) above the C ABI.
//
// mapping.Mapper.Map is adaptive per read (ends -> one/two steps in -> binary split search), every step being a
// performMapping of one window.  To batch windows of MANY reads into each GPU call while keeping Map()'s control flow
// written exactly as the reference's sequential code, each read's Map() runs as a stackful coroutine (host_coro.hpp):
// performMapping() files a window request and yields; when every live coroutine is waiting, the scheduler scans all
// requested windows (dp_scan), runs the candidate/chaining stage (dp_map_windows) and resumes the coroutines with
// their chains.  Results are emitted in read order (the canonical single-worker order).
#include <algorithm>
#include <cstdio>
#include <cstring>

#include <chrono>

#include "dph.hpp"
#include "host_util.hpp"
#include "align_plan.hpp"
#include "map_plan.hpp"

#define DPH_CORO_IMPLEMENTATION  // (the switch routine itself lives in this translation unit)
#include "host_coro.hpp"

namespace dph {

namespace {

struct Mapping {  // mapping/mapping.go:11-20
    i64 queryLen = 0;  // Query.Len() of the sequence updateQuery() attached (the whole read)
    bool hasQuery = false;
    i64 Start = 0, End = 0, QueryOffset = 0, QueryInset = 0;
    bool RC = false;
    i64 ids = 0;
    int ref = 0;  // the reference sequence of the chunk the chain was found in (`-all_sequences`; 0 otherwise)
};

// Go sort.Sort stand-in (DESIGN.md canonical semantics): insertion sort <= 12 elements, stable sort above.
template <class T, class Less>
void goSort(std::vector<T>& v, Less less) {
    if (v.size() <= 12) {
        for (size_t i = 1; i < v.size(); i++)
            for (size_t j = i; j > 0 && less(v[j], v[j - 1]); j--) std::swap(v[j], v[j - 1]);
    } else {
        std::stable_sort(v.begin(), v.end(), less);
    }
}

struct Chunk {  // an indexed reference chunk (seeds.SeedSequence of a reference.SubSequence)
    const int32_t* seg = nullptr;
    int n = 0;
    i64 offset = 0, inset = 0;  // within its reference sequence
    int ref = 0;                // which reference sequence it was cut from
};

struct WindowReq {
    uint32_t read = 0;  // index into the read set
    i64 a = 0, b = 0;   // view [a, b) of the top-level read
    bool whole = false; // the top-level read itself (len <= 2*edge)
};

struct WindowResult {
    // forward / reverse-complement seed sequences of the window and the chains the GPU kept
    std::vector<int32_t> seg[2];
    struct ChainRef {
        uint32_t target;
        std::vector<int32_t> a, b;
    };
    std::vector<ChainRef> chains[2];
};

struct Task;

struct Sched {
    CoroPoint main;  // the scheduler's own stack while a coroutine runs
};

// What is the same for every mapper thread: built once by the run and shared const (chunks[i].seg point into chunkSegs, so it is
// never copied)
struct MapIndex {
    int k = 11;
    i64 edgeSize = 1000;
    bool circular = true;
    std::vector<i64> refLens;  // the reference sequences mapped against: the first of the file, or all of them in file order
    std::vector<std::string> refNames;
    std::vector<Chunk> chunks;
    std::vector<int32_t> chunkSegs;  // host copy of the chunk scan
    MapIndex() = default;
    MapIndex(const MapIndex&) = delete;
    MapIndex& operator=(const MapIndex&) = delete;
};

// One thread's mapper: the shared index, the context its windows go to and the scheduler its read tasks switch back to
struct MapperImpl {
    const MapIndex& ix;
    dp_ctx* ctx = nullptr;
    Sched sched;
    explicit MapperImpl(const MapIndex& index) : ix(index) {}

    bool isConsistent(const Mapping* l, const Mapping* r) const;
    void matchPairs(std::vector<Mapping*>& openA, std::vector<Mapping*>& openB, std::vector<Mapping*>& matched, bool& matchedNil,
                    Task& t);
    void findSplitPoint(Task& t, std::vector<Mapping*>& openA, std::vector<Mapping*>& openB, i64 left, i64 right);
    void mapNext(Task& t, std::vector<Mapping*>& openA, std::vector<Mapping*>& openB, std::vector<Mapping*>& newA,
                 std::vector<Mapping*>& newB, std::vector<Mapping*>& matched, bool& matchedNil);
    std::vector<Mapping*> map(Task& t);
    std::vector<Mapping*> performMapping(Task& t, i64 a, i64 b, bool whole);
    std::string asString(const Mapping& m, const std::string& qname, i64 qlen) const;
};

struct Task {
    CoroPoint at;           // where the coroutine stands while it is switched out
    char* stack = nullptr;  // from the scheduler's stack pool (uninitialised memory, reused by later reads)
    uint32_t read = 0;
    i64 L = 0;
    bool done = false, waiting = false;
    WindowReq req;
    WindowResult res;
    std::vector<std::unique_ptr<Mapping>> pool;
    std::vector<Mapping*> results;
    MapperImpl* m = nullptr;
    Mapping* mk() {
        pool.emplace_back(new Mapping());
        return pool.back().get();
    }
};

// first frame of every coroutine: never returns (the last switch leaves it for good)
void coroTrampoline(void* arg) {
    Task* t = (Task*)arg;
    t->results = t->m->map(*t);
    t->done = true;
    coroSwitch(t->at, t->m->sched.main, true);
}

// ---- mapping.go:131-160
bool MapperImpl::isConsistent(const Mapping* left, const Mapping* right) const {
    if (left->ref != right->ref) return false;  // positions on two reference sequences have no distance
    if (left->RC != right->RC) return false;
    const i64 expectedDistance = right->QueryOffset - left->queryLen + left->QueryInset;
    i64 distance = !left->RC ? right->Start - left->End : left->Start - right->End;
    if (ix.circular && distance < -50) distance += ix.refLens[(size_t)left->ref];
    if (distance < 50 && expectedDistance < 50 && distance > -50) return true;
    if (distance < 500) return (expectedDistance < (distance * 3) / 2 && expectedDistance > (distance * 2) / 3);
    if (distance > 5000) return (expectedDistance < (distance * 10) / 9 && expectedDistance > (distance * 9) / 10);
    double ratio = (double)(distance - 500) / 4500.0;
    ratio = 3.0 / 2.0 + ratio * (10.0 / 9.0 - 3.0 / 2.0);
    return distance < (i64)((double)expectedDistance * ratio) && distance > (i64)((double)expectedDistance / ratio);
}

// ---- removeDominated mapping.go:387-428 (open and extended are the same slice at every call site)
std::vector<Mapping*> removeDominated(std::vector<Mapping*> open, i64 queryLen) {
    if (open.empty()) return open;
    goSort(open, [](Mapping* a, Mapping* b) { return a->QueryOffset < b->QueryOffset; });
    const std::vector<Mapping*>& extended = open;
    size_t j = 0;
    std::vector<uint8_t> toRemove(open.size(), 0);
    for (size_t i = 0; i < open.size(); i++) {
        Mapping* next = open[i];
        while (j < extended.size() && queryLen - extended[j]->QueryInset < next->QueryOffset) j++;
        if (j == extended.size()) return open;
        bool dominated = false;
        for (size_t kk = j; !dominated && kk < extended.size() && extended[kk]->QueryOffset < queryLen - next->QueryInset; kk++) {
            if (extended[kk]->ids * 4 > next->ids * 5) {
                i64 start = next->QueryOffset;
                if (extended[kk]->QueryOffset > start) start = extended[kk]->QueryOffset;
                i64 end = queryLen - next->QueryInset;
                if (extended[kk]->QueryInset > next->QueryInset) end = queryLen - extended[kk]->QueryInset;
                dominated = ((end - start) * 10 > (queryLen - next->QueryOffset - next->QueryInset) * 9);
            }
        }
        toRemove[i] = dominated;
    }
    i64 last = (i64)open.size() - 1;
    for (i64 i = last; i >= 0; i--)
        if (toRemove[(size_t)i]) {
            open[(size_t)i] = open[(size_t)last];
            last--;
        }
    open.resize((size_t)(last + 1));
    return open;
}

void updateQuery(std::vector<Mapping*>& ms, i64 len) {
    for (Mapping* m : ms) {
        m->queryLen = len;
        m->hasQuery = true;
    }
}
void appendAll(std::vector<Mapping*>& d, const std::vector<Mapping*>& s) { d.insert(d.end(), s.begin(), s.end()); }

// ---- matchPairs mapping.go:174-203
void MapperImpl::matchPairs(std::vector<Mapping*>& openA, std::vector<Mapping*>& openB, std::vector<Mapping*>& matched,
                            bool& matchedNil, Task& t) {
    matched.clear();
    matchedNil = true;
    for (i64 i = (i64)openA.size() - 1; i >= 0; i--) {
        Mapping* ra = openA[(size_t)i];
        for (i64 j = (i64)openB.size() - 1; j >= 0; j--) {
            Mapping* rb = openB[(size_t)j];
            if (isConsistent(ra, rb)) {
                const i64 qOffset = ra->QueryOffset, qInset = rb->QueryInset;
                if (ra->RC) std::swap(ra, rb);
                Mapping* c = t.mk();
                c->Start = ra->Start;
                c->End = rb->End;
                c->queryLen = ra->queryLen;
                c->hasQuery = ra->hasQuery;
                c->QueryOffset = qOffset;
                c->QueryInset = qInset;
                c->RC = ra->RC;
                c->ids = ra->ids + rb->ids;
                c->ref = ra->ref;
                matchedNil = false;
                matched.push_back(c);
                openA[(size_t)i] = openA.back();
                openA.pop_back();
                openB[(size_t)j] = openB.back();
                openB.pop_back();
                break;
            }
        }
    }
}

// ---- findSplitPoint mapping.go:207-288
void MapperImpl::findSplitPoint(Task& t, std::vector<Mapping*>& openA, std::vector<Mapping*>& openB, i64 left, i64 right) {
    const i64 qLen = t.L, edgeSize = ix.edgeSize;
    while (right - left >= edgeSize) {
        const i64 start = (right + left - edgeSize) / 2, end = start + edgeSize;
        std::vector<Mapping*> mid = performMapping(t, start, end, false);
        i64 newLeft = left, newRight = right, afterA = 0, afterB = 0;
        for (Mapping* mm : mid) {
            mm->queryLen = qLen;
            mm->hasQuery = true;
            for (Mapping* ma : openA) {
                if (isConsistent(ma, mm)) {
                    ma->QueryInset = mm->QueryInset;
                    ma->ids += mm->ids;
                    if (ma->RC) ma->Start = mm->Start;
                    else ma->End = mm->End;
                    const i64 midMatched = qLen - mm->QueryInset - mm->QueryOffset;
                    if (midMatched > afterA) afterA = midMatched;
                    if (qLen - mm->QueryInset > newLeft) newLeft = qLen - mm->QueryInset;
                    break;
                }
            }
            if (afterA < (edgeSize * 2) / 3) {
                for (Mapping* mb : openB) {
                    if (isConsistent(mm, mb)) {
                        mb->QueryOffset = mm->QueryOffset;
                        mb->ids += mm->ids;
                        if (mb->RC) mb->End = mm->End;
                        else mb->Start = mm->Start;
                        const i64 midMatched = qLen - mm->QueryInset - mm->QueryOffset;
                        if (midMatched > afterB) afterB = midMatched;
                        if (mm->QueryOffset < newRight) newRight = mm->QueryOffset;
                        break;
                    }
                }
            }
        }
        if (afterA > 0 && afterB > 0) {
            std::vector<Mapping*> empty;
            if (newLeft - left > edgeSize * 2) findSplitPoint(t, openA, empty, newLeft - edgeSize * 2, newLeft - edgeSize);
            if (right - newRight > edgeSize * 2) findSplitPoint(t, empty, openB, newRight + edgeSize, newRight + edgeSize * 2);
            return;
        }
        if (afterA == 0 && afterB == 0) {
            std::vector<Mapping*> empty;
            if (!openA.empty()) findSplitPoint(t, openA, empty, left, start);
            if (!openB.empty()) findSplitPoint(t, empty, openB, end, right);
            return;
        }
        left = newLeft;
        right = newRight;
    }
}

// ---- mapNext mapping.go:305-383 (Go slice aliasing reproduced with value copies, cf. oracle/mapping.cpp notes)
void MapperImpl::mapNext(Task& t, std::vector<Mapping*>& openA, std::vector<Mapping*>& openB, std::vector<Mapping*>& newA,
                         std::vector<Mapping*>& newB, std::vector<Mapping*>& matched, bool& matchedNil) {
    const i64 qLen = t.L, edgeSize = ix.edgeSize;
    std::vector<Mapping*> extended;
    bool extNil;
    if (qLen < edgeSize * 4) {
        newA = removeDominated(performMapping(t, edgeSize, qLen - edgeSize, false), qLen);
        updateQuery(newA, qLen);
        matchPairs(openA, newA, extended, extNil, t);
        if (!extNil) {
            std::vector<Mapping*> tmp = newA;
            appendAll(tmp, extended);
            openA = tmp;
        } else {
            appendAll(openA, newA);
        }
        matchPairs(openA, openB, matched, matchedNil, t);
        newA = openA;
        newB = openB;
        if (matchedNil) return;
        newA.clear();
        newB.clear();
        return;
    }
    newA = removeDominated(performMapping(t, edgeSize, edgeSize * 2, false), qLen);
    updateQuery(newA, qLen);
    matchPairs(openA, newA, extended, extNil, t);
    appendAll(openA, newA);
    if (!extNil) appendAll(openA, extended);
    newB = removeDominated(performMapping(t, qLen - edgeSize * 2, qLen - edgeSize, false), qLen);
    updateQuery(newB, qLen);
    {
        std::vector<Mapping*> a = newB, b = openB;
        matchPairs(a, b, extended, extNil, t);
        openB = a;
        newB = b;
    }
    appendAll(openB, newB);
    if (!extNil) appendAll(openB, extended);
    {
        std::vector<Mapping*> a = openA, b = openB;
        matchPairs(a, b, matched, matchedNil, t);
        newA = a;
        newB = b;
    }
    if (matchedNil) {
        if (qLen > edgeSize * 5) {
            openA = removeDominated(performMapping(t, edgeSize * 2, edgeSize * 3, false), qLen);
            updateQuery(openA, qLen);
            {
                std::vector<Mapping*> a = newA, b = openA;
                matchPairs(a, b, extended, extNil, t);
                openA = a;
                newA = b;
            }
            if (!extNil) appendAll(openA, extended);
            appendAll(openA, newA);
        }
        if (qLen > edgeSize * 6) {
            openB = removeDominated(performMapping(t, qLen - edgeSize * 3, qLen - edgeSize * 2, false), qLen);
            updateQuery(openB, qLen);
            {
                std::vector<Mapping*> a = openB, b = newB;
                matchPairs(a, b, extended, extNil, t);
                openB = a;
                newB = b;
            }
            if (!extNil) appendAll(openB, extended);
            appendAll(openB, newB);
        } else {
            openB = newB;
        }
        if (qLen > edgeSize * 5) {
            std::vector<Mapping*> a = openA, b = openB;
            matchPairs(a, b, matched, matchedNil, t);
            newA = a;
            newB = b;
        }
    }
}

// ---- Map mapping.go:430-487
std::vector<Mapping*> MapperImpl::map(Task& t) {
    const i64 qLen = t.L, edgeSize = ix.edgeSize;
    std::vector<Mapping*> results;
    if (qLen <= edgeSize * 2) {
        results = removeDominated(performMapping(t, 0, qLen, true), qLen);
        updateQuery(results, qLen);
        return results;
    }
    std::vector<Mapping*> openA = performMapping(t, 0, edgeSize, false);           // mapEnds :164-172
    std::vector<Mapping*> openB = performMapping(t, qLen - edgeSize, qLen, false);
    openA = removeDominated(openA, qLen);
    openB = removeDominated(openB, qLen);
    updateQuery(openA, qLen);
    updateQuery(openB, qLen);
    std::vector<Mapping*> matched;
    bool matchedNil;
    matchPairs(openA, openB, matched, matchedNil, t);
    if (!matchedNil) return matched;
    if (qLen < edgeSize * 3) {
        results = openA;
        appendAll(results, openB);
        return results;
    }
    std::vector<Mapping*> nA, nB;
    mapNext(t, openA, openB, nA, nB, matched, matchedNil);
    openA = nA;
    openB = nB;
    if (!matchedNil) return matched;
    i64 left = edgeSize * 2, right = qLen - edgeSize * 2;
    for (Mapping* a : openA)
        if (a->QueryInset > left) left = a->QueryInset;
    left = qLen - right;  // sic (:461)
    for (Mapping* b : openB)
        if (b->QueryOffset < right) right = b->QueryOffset;
    findSplitPoint(t, openA, openB, left, right);
    const i64 size = qLen - edgeSize;
    for (i64 i = (i64)openA.size() - 1; i >= 0; i--)
        if (openA[(size_t)i]->QueryInset >= size) {
            openA[(size_t)i] = openA.back();
            openA.pop_back();
        }
    for (i64 i = (i64)openB.size() - 1; i >= 0; i--)
        if (openB[(size_t)i]->QueryOffset >= size) {
            openB[(size_t)i] = openB.back();
            openB.pop_back();
        }
    results = openA;
    appendAll(results, openB);
    return results;
}

i64 segSeedOffset(const int32_t* seg, int index, int k) {
    index = index * 2 + 1;
    i64 o = seg[0];
    for (int i = 2; i < index; i += 2) o += seg[i] + k;
    return o;
}
i64 segSeedOffsetFromEnd(const int32_t* seg, int n, int index, int k) {
    index = index * 2 + 1;
    i64 o = seg[n - 1];
    for (int i = n - 3; i > index; i -= 2) o += seg[i] + k;
    return o;
}
// GetBasesCovered second return (target side), seeds/sequence.go:830-858
i64 basesCoveredB(const int32_t* sb, const std::vector<int32_t>& mb, int k) {
    i64 countB = (i64)mb.size() * k;
    int prevB = mb[0];
    for (size_t i = 1; i < mb.size(); i++) {
        const int s2 = mb[i];
        i64 d2 = sb[prevB * 2 + 2];
        for (int j = prevB + 2; j <= s2; j++) d2 += sb[j * 2] + k;
        if (d2 < 0) countB += d2;
        prevB = s2;
    }
    return countB;
}

// ---- performMapping mapping.go:489-611: the window is sent to the GPU batch; this coroutine resumes with the chains.
std::vector<Mapping*> MapperImpl::performMapping(Task& t, i64 a, i64 b, bool whole) {
    if (b > t.L) b = t.L;  // SubSequence clamps end (sequence.go:354)
    t.req.read = t.read;
    t.req.a = a;
    t.req.b = b;
    t.req.whole = whole;
    t.waiting = true;
    coroSwitch(t.at, sched.main);  // yield until the batch has been processed
    t.waiting = false;
    const WindowResult& R = t.res;
    const int k = ix.k;
    const bool circular = ix.circular;
    const i64 qlen = b - a;
    // view metadata: SubSequence of a top-level read (offset a, inset L-(b-1)); the RC view swaps them (sequence.go:196)
    i64 vOffset = whole ? 0 : a, vInset = whole ? 0 : t.L - (b - 1);
    std::vector<Mapping*> results;
    for (int s = 0; s < 2; s++) {
        const int32_t* qseg = R.seg[s].data();
        const int qn = (int)R.seg[s].size();
        const i64 sqOffset = s == 0 ? vOffset : vInset, sqInset = s == 0 ? vInset : vOffset;
        for (const auto& ch : R.chains[s]) {
            const Chunk& c = ix.chunks[ch.target];
            const i64 refLen = ix.refLens[(size_t)c.ref];
            i64 start = c.offset + segSeedOffset(c.seg, ch.b[0], k);
            const i64 end = refLen - c.inset - segSeedOffsetFromEnd(c.seg, c.n, ch.b.back(), k);
            if (circular && start > refLen) start -= refLen;
            Mapping* mp = t.mk();
            if (s == 0) {
                i64 qOffset = segSeedOffset(qseg, ch.a[0], k) + sqOffset;
                i64 qInset = segSeedOffsetFromEnd(qseg, qn, ch.a.back(), k) + sqInset;
                mp->QueryOffset = qOffset;
                mp->QueryInset = qInset;
            } else {  // offsets/insets are swapped: they are based on the reverse-complement query (:569-580)
                i64 qInset = segSeedOffset(qseg, ch.a[0], k) + sqOffset;
                i64 qOffset = segSeedOffsetFromEnd(qseg, qn, ch.a.back(), k) + sqInset;
                mp->QueryOffset = qOffset;
                mp->QueryInset = qInset;
            }
            mp->Start = start;
            mp->End = end;
            mp->RC = s == 1;
            mp->ids = basesCoveredB(c.seg, ch.b, k);
            mp->ref = c.ref;
            results.push_back(mp);
        }
    }
    (void)qlen;
    if (results.size() > 1) {  // :590-608
        goSort(results, [](Mapping* x, Mapping* y) { return x->ref != y->ref ? x->ref < y->ref : x->Start < y->Start; });
        for (i64 i = (i64)results.size() - 1; i > 0; i--) {
            Mapping* ra = results[(size_t)(i - 1)];
            Mapping* rb = results[(size_t)i];
            if (ra->ref == rb->ref && ra->RC == rb->RC && rb->Start < ra->End) {
                if (ra->End - ra->Start > rb->End - rb->Start) {
                    results[(size_t)i] = results.back();
                    results.pop_back();
                } else {
                    results[(size_t)(i - 1)] = results[(size_t)i];
                    results[(size_t)i] = results.back();
                    results.pop_back();
                }
            }
        }
    }
    return results;
}

// ---- AsString mapping.go:112-122
std::string MapperImpl::asString(const Mapping& m, const std::string& qname, i64 qlen) const {
    const i64 refLen = ix.refLens[(size_t)m.ref];
    i64 mappedLength = m.End - m.Start;
    if (ix.circular && mappedLength < 0) mappedLength = refLen - m.Start + m.End;
    char buf[512];
    snprintf(buf, sizeof buf, "\t%lld\t%lld\t%lld\t%s\t", (long long)qlen, (long long)m.QueryOffset, (long long)(qlen - m.QueryInset),
             m.RC ? "-" : "+");
    std::string s = qname + buf + ix.refNames[(size_t)m.ref];
    snprintf(buf, sizeof buf, "\t%lld\t%lld\t%lld\t%lld\t%lld\t255", (long long)refLen, (long long)m.Start, (long long)m.End,
             (long long)m.ids, (long long)mappedLength);
    return s + buf;
}


}  // namespace

// ---- test hooks: the mapper's two decision rules on bare numbers (tests/test_hand_known_answers.py: answers worked from the Go text)
// l = {RC, Query.Len(), QueryInset, Start, End}, r = {RC, QueryOffset, Start, End}
bool handIsConsistent(const i64* l, const i64* r, bool circular, i64 refLen) {
    MapIndex ix;
    ix.circular = circular;
    ix.refLens.assign(1, refLen);
    MapperImpl m(ix);
    Mapping L, R;
    L.RC = l[0] != 0;
    L.queryLen = l[1];
    L.hasQuery = true;
    L.QueryInset = l[2];
    L.Start = l[3];
    L.End = l[4];
    R.RC = r[0] != 0;
    R.QueryOffset = r[1];
    R.Start = r[2];
    R.End = r[3];
    return m.isConsistent(&L, &R);
}
// maps = n x {QueryOffset, QueryInset, ids}; kept[] = indices of the survivors in the order removeDominated returns them
int handRemoveDominated(const i64* maps, int n, i64 queryLen, int* kept) {
    std::vector<Mapping> store((size_t)n);
    std::vector<Mapping*> open;
    for (int i = 0; i < n; i++) {
        store[(size_t)i].QueryOffset = maps[3 * i];
        store[(size_t)i].QueryInset = maps[3 * i + 1];
        store[(size_t)i].ids = maps[3 * i + 2];
        open.push_back(&store[(size_t)i]);
    }
    std::vector<Mapping*> out = removeDominated(open, queryLen);
    for (size_t i = 0; i < out.size(); i++) kept[i] = (int)(out[i] - store.data());
    return (int)out.size();
}

// ---------------------------------------------------------------------------------------------------------------
// commands/map.go:33-116 + NewMapper mapping.go:67-109

// the staging block [reference | join chunk | all reads] of the last map command of this process, kept for the next one
namespace {
std::mutex g_stagingMu;
std::unique_ptr<char[]> g_staging;
size_t g_stagingCap = 0;
std::unique_ptr<char[]> stagingTake(size_t need, size_t* cap) {
    {
        std::lock_guard<std::mutex> lk(g_stagingMu);
        if (g_staging && g_stagingCap >= need) {
            *cap = g_stagingCap;
            g_stagingCap = 0;
            return std::move(g_staging);
        }
    }
    *cap = need;
    return std::unique_ptr<char[]>(new char[need]);
}
void stagingPut(std::unique_ptr<char[]> p, size_t cap) {
    std::lock_guard<std::mutex> lk(g_stagingMu);
    if (cap > g_stagingCap) {  // (the smaller of two blocks goes: its munmap is the caller's 40 ms, once)
        g_staging = std::move(p);
        g_stagingCap = cap;
    }
}
}  // namespace
size_t releaseMapStaging() {
    std::lock_guard<std::mutex> lk(g_stagingMu);
    const size_t freed = g_staging ? g_stagingCap : 0;
    g_staging.reset();
    g_stagingCap = 0;
    return freed;
}

namespace {

double wallNow() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- owners: everything a run holds that has to be given back.  MapRun declares one of each, in the order that makes a plain
// `return rc` correct on every way out of runMap (see there)
struct PinnedBlock {  // the packed reads' pinned block
    uint8_t* p = nullptr;
    size_t cap = 0;
    bool reserve(size_t bytes) {  // (a Mapper keeps the block from batch to batch while it is large enough)
        if (p && bytes <= cap) return true;
        if (p) dp_host_free(p);
        p = (uint8_t*)dp_host_alloc(bytes);
        cap = p ? bytes : 0;
        return p != nullptr;
    }
    ~PinnedBlock() {
        if (p) dp_host_free(p);
    }
};
struct ThreadJoiner {
    std::thread t;
    void join() {
        if (t.joinable()) t.join();
    }
    ~ThreadJoiner() { join(); }
};
struct CtxOwner {
    dp_ctx* c = nullptr;
    void destroy() {
        if (c) dp_ctx_destroy(c);
        c = nullptr;
    }
    ~CtxOwner() { destroy(); }
};
// DP_MAP_SHARDS=N: shard s holds the chunks [c0, c1) (c0 a multiple of 64) on a context of its own
struct Shard {
    dp_ctx* ctx = nullptr;
    uint32_t c0 = 0, c1 = 0;
};
struct ShardCtxs {
    std::vector<Shard> v;
    ~ShardCtxs() {
        for (Shard& sh : v)
            if (sh.ctx) dp_ctx_destroy(sh.ctx);
    }
};
struct WorkerCtxs {  // the contexts of the mapper threads after the first (which works on the main context); slot 0 stays empty
    std::vector<dp_ctx*> v;
    void destroy() {
        for (dp_ctx*& c : v) {
            if (c) dp_ctx_destroy(c);
            c = nullptr;
        }
    }
    ~WorkerCtxs() { destroy(); }
};
// The ASCII paths' staging block.  Giving 400 MB of staging back to the system is 40 ms of munmap - round 3's profile had booked it
// as "AddSingleSeeds (waited for)" - and on a thread of its own it holds the address-space lock against this one's allocations just
// as long: the block is kept for the process's next map command instead, which then also finds its pages touched.  Before it
// changes hands the upload's thread has read its last byte (the wait) and the thread that fills it has written its last (on a way
// out before the upload step that thread may still run: it is joined here, ahead of its own joiner).
struct StagingBlock {
    std::unique_ptr<char[]> p;
    size_t cap = 0;
    CtxOwner& ctx;
    ThreadJoiner& writer;
    StagingBlock(CtxOwner& c, ThreadJoiner& w) : ctx(c), writer(w) {}
    ~StagingBlock() {
        if (ctx.c) (void)dp_reads_upload_wait(ctx.c, 0xffffffffu);
        writer.join();
        if (p) stagingPut(std::move(p), cap);
    }
};

struct LoopStats {  // what one mapper thread reports
    MapStats st;
    double tScan = 0, tChain = 0, wall = 0;
    int rc = 0;
    std::string error;
};

// One map command: what its steps share.  runMap calls the steps in order; a step that fails has put the text into `error` (of
// the context that failed, while it still exists) and returns its code.
struct MapRun {
    // ---- what the caller gave.  upSet: the reads that go up.  Without a trim they are the reads that are mapped; with one they are
    // the raw reads, and the set that is mapped (trimmedSet) is made from them once the trim has run on the device's copy
    const ReadSet& refSet;
    const ReadSet* upSetP;  // (a Mapper binds its batches one after the other: bindBatch)
    const MapParams& p;
    const int device;
    std::string& paf;
    std::string& errText;
    MapStats* const stats;
    std::string& error;
    MapTrim* const trim;
    ReadSet trimmedSet;
    const ReadSet* readsP;
    const ReadSet& upSet() const { return *upSetP; }
    const ReadSet& reads() const { return *readsP; }
    const int k;
    // the sequences mapped against: the first of the reference file (commands/map.go:34-36) or, with -all_sequences, every top-level
    // sequence of it in file order (one seed index, chunk ids running on from sequence to sequence)
    const size_t T;
    const bool prof;
    double tRun0;  // (of the run, or of a Mapper's batch)
    double tMark, tLoop0 = 0;
    // ---- layout of the device read set (map_plan.hpp)
    std::vector<i64> refLens;
    MapJoins J;
    size_t head = 0, readBytes = 0;  // ASCII paths: bytes of [reference | join chunks] and of the reads in the staging block
    bool asyncUpload = false, packedUpload = false, packScalar = false;
    MapPacked P;
    std::vector<i64> off;  // ASCII paths: offsets into the staging block
    // ---- seeds, chunks and the reference index
    std::vector<double> values;
    SeedIndex index;
    dp_single_seed_batch ssb;  // (host arrays of the main context)
    bool deviceSeeds = false;
    MapSchedule sched;
    dp_seedseq_batch sb;  // the chunk scan (host arrays of the main context)
    std::vector<dp_seq_ref> refs;
    MapIndex M;
    int nShards = 1;
    std::vector<int> devs;
    uint32_t perShard = 0;
    bool sparseIndex = false;
    std::mutex infoMu;  // the mapper threads add their index's bytes to *stats
    // ---- a Mapper (below): this run's reference side stays, batches of reads come and go
    bool mapperMode = false;  // worker contexts are kept from batch to batch, the index estimate counts the most threads a batch may use
    bool noChunks = false;    // no sequence is long enough for a chunk: every batch is "all unmapped" without a device call
    std::string refText;      // the stderr lines of the reference side, in front of every batch's counts
    int64_t regimesSeen[4] = {0, 0, 0, 0};  // the contexts count their queries for as long as they live: a batch reports what it added
    // ---- what the mapper threads leave
    size_t nThreads = 1;
    std::vector<std::string> out;  // per read, in read order, whoever mapped it
    std::vector<int> nmaps;
    std::vector<LoopStats> lstats;
    // ---- base-level alignment of a Mapper's batch (alignMappings): off unless the batch asked for it
    bool alignOn = false;
    uint32_t maxEdits = (uint32_t)kAlignMaxEditsDefault;
    std::vector<std::vector<AlignLine>> lines;  // per read, the mappings behind out[r]'s lines in their order
    // ---- the owners, declared in the reverse of the order they must go in (everything above outlives them all):
    PinnedBlock pinned;     // 7. freed last: the packing thread writes it
    ThreadJoiner concat;    // 6. the packing / concatenating thread (it touches no context)
    CtxOwner ctx;           // 5. the main context, after everything that uses it or memory it owns:
    ThreadJoiner seedWalk;  // 4. with device seeds the walk reads ssb's arrays, which are host memory of the main context
    StagingBlock staging;   // 3. dp_reads_upload_wait(ctx, 0xffffffff), then the block goes back to stagingPut
    ShardCtxs shards;       // 2. the shard contexts
    WorkerCtxs workers;     // 1. go first: they share the main context's reads and may borrow its sparse index

    MapRun(const ReadSet& refSet_, const ReadSet& upSet_, const MapParams& p_, int device_, std::string& paf_, std::string& errText_,
           MapStats* stats_, std::string& error_, MapTrim* trim_)
        : refSet(refSet_), upSetP(&upSet_), p(p_), device(device_), paf(paf_), errText(errText_), stats(stats_), error(error_), trim(trim_),
          readsP(trim_ ? &trimmedSet : &upSet_), k(p_.k), T(p_.allSequences ? refSet_.size() : std::min<size_t>(1, refSet_.size())),
          prof(dp_profile_on()), tRun0(wallNow()), tMark(tRun0), off(1, 0), index(p_.k), staging(ctx, concat) {
        memset(&ssb, 0, sizeof ssb);
        memset(&sb, 0, sizeof sb);
    }
    void mark(const char* what) {
        if (!prof) return;
        const double t = wallNow();
        fprintf(stderr, "[map setup] %-28s %.1f ms\n", what, 1e3 * (t - tMark));
        tMark = t;
    }
    int failed(dp_ctx* c, int rc) {  // the text of the context that failed, taken while it exists
        error = dp_last_error(c);
        return rc;
    }
    size_t plannedThreads(size_t nReads) const;
    int64_t indexBytes(dp_ctx* c, uint64_t m) const;
    int buildIndexOn(dp_ctx* c, const dp_seq_ref* r, uint32_t n);

    int check();
    void layoutAndStage();
    void packOrConcatenate();
    int allocBlocks();
    int openContext();
    int startSeedWalk();
    void walkCandidates();
    void walkOnHost();
    int uploadReads();
    int trimAndRespan();
    int scanChunks();
    int chooseIndexLayout();
    int buildIndex();
    int buildShard(Shard& sh, std::vector<uint32_t>& global, std::vector<uint32_t>& local);
    int runWorkers();
    void collectStats();
    void packReads(const std::vector<uint64_t>& poff, size_t readsAt);
    void unmappedBatch();
    // the steps of a Mapper's batch
    void bindBatch(const ReadSet& batch, bool trimmed = false);
    int packBatch();
    int refreshWorkers();
    int replaceTail();
    int replaceTailTrimmed(MapTrim& t);
    int alignMappings();
    void writeText();
    void writeCounts(i64 mapped, i64 multiple, i64 total, i64 unmapped);
};

// ---- checks: what is refused before anything is packed or allocated on the device
int MapRun::check() {
    if (refSet.size() == 0) {
        error = "empty reference";
        return -1;
    }
    refLens.resize(T);
    for (size_t c = 0; c < T; c++) refLens[c] = refSet.length(c);
    if (int rc = mapCheckLimits(p, refLens, refSet.names, error)) return rc;
    if (trim) {  // what the trim refuses about its adapters and k
        TrimIndex ix;
        if (!trimBuildIndex(*trim->front, *trim->back, trim->params.k, ix, error)) return DP_ERR_ARG;
    }
    if (p.indexLayout < 0 || p.indexLayout > 2) {
        error = "map: reference index layout " + std::to_string(p.indexLayout) + " (0 = auto, 1 = dense, 2 = sparse)";
        return DP_ERR_ARG;
    }
    return 0;
}

// ---- device read set: [0] reference, [1] circular join chunk, then (forward, reverse complement) of every read; with
// -all_sequences [0 .. T) the reference sequences, then the join chunk of every sequence that has one, then the reads.
// The reads cross PCIe the way the reference holds them - 2 bits per base (sequence.packedSequence) - packed here by
// the worker pool straight into a pinned block in the device's own layout (every read on a 16-byte boundary) and put in place by
// dp_reads_upload_packed_rc, which also makes the reverse strands: 100 MB instead of 400 at config 3, one copy instead of three
// (staging, pinned ring, link).  DP_TUNE=map_ascii_upload=1: the ASCII path (it is what map_async_upload uses): one staging buffer
// [reference | join chunk | all reads].  With a trim the packed path is the only one and neither key is consulted: the device set is
// then [raw reads | reference sequences | join chunks] without pairs, so that the trim's id lists and spans name raw read r as device
// read r, and dp_reads_respan_rc makes map's order and the reverse strands from it afterwards.
void MapRun::layoutAndStage() {
    std::vector<const char*> seqs(T);
    for (size_t c = 0; c < T; c++) seqs[c] = refSet.seq(c);
    J = mapJoinChunks(p, refLens, seqs, refSet.names);
    for (size_t c = 0; c < T; c++) head += (size_t)refLens[c];
    for (const std::string& j : J.joins) head += j.size();
    readBytes = !trim && reads().size() ? (size_t)(reads().off[reads().size()] - reads().off[0]) : 0;
    asyncUpload = !trim && dp_tune("map_async_upload", 0) != 0;
    packedUpload = trim || (!asyncUpload && !dp_tune("map_ascii_upload", 0));
    packScalar = dp_tune("pack_scalar", 0) != 0;  // (tests: the packer without its AVX2 path)
}
int MapRun::allocBlocks() {
    if (!packedUpload) {
        staging.p = stagingTake(head + readBytes + 1, &staging.cap);
        return 0;
    }
    P = mapPackedLayout(refLens, J.joins, upSet().off.data(), upSet().size(), trim != nullptr);
    if (!pinned.reserve((size_t)P.poff.back() + 64)) {
        error = "dp_host_alloc: no pinned memory for the packed reads";
        return DP_ERR_HIP;
    }
    return 0;
}
// the reads packed into the pinned block by the worker pool, read r at poff[readsAt + r]
void MapRun::packReads(const std::vector<uint64_t>& poff, size_t readsAt) {
    // pieces of about 2 M bases: whole reads
    std::vector<size_t> cut(1, 0);
    i64 acc = 0;
    for (size_t r = 0; r < upSet().size(); r++) {
        acc += upSet().length(r);
        if (acc >= ((i64)2 << 20)) {
            cut.push_back(r + 1);
            acc = 0;
        }
    }
    if (cut.back() != upSet().size()) cut.push_back(upSet().size());
    parallelFor(cut.size() - 1, [&](size_t i) {
        for (size_t r = cut[i]; r < cut[i + 1]; r++) packBases(upSet().seq(r), (size_t)upSet().length(r), pinned.p + poff[readsAt + r], packScalar);
    });
}
// The host staging copy is made by a thread of its own while the device computes the reference's k-mer table
void MapRun::packOrConcatenate() {
    if (packedUpload) {
        for (size_t c = 0; c < T; c++) packBases(refSet.seq(c), (size_t)refLens[c], pinned.p + P.poff[P.headAt + c], packScalar);
        for (size_t j = 0; j < J.joins.size(); j++) packBases(J.joins[j].data(), J.joins[j].size(), pinned.p + P.poff[P.headAt + T + j], packScalar);
        packReads(P.poff, P.readsAt);
        return;
    }
    // the reads are one contiguous block of the read set, copied (and its pages first touched) by the worker pool in 4 MiB pieces
    for (size_t c = 0; c < T; c++) {
        memcpy(staging.p.get() + off.back(), refSet.seq(c), (size_t)refLens[c]);
        off.push_back(off.back() + refLens[c]);
    }
    for (const std::string& j : J.joins) {
        memcpy(staging.p.get() + off.back(), j.data(), j.size());
        off.push_back(off.back() + (i64)j.size());
    }
    const char* src = reads().size() ? reads().seq(0) : nullptr;
    const size_t piece = (size_t)4 << 20, nPieces = (readBytes + piece - 1) / piece;
    char* dst = staging.p.get() + head;
    parallelFor(nPieces, [&](size_t i) {
        const size_t b = i * piece, e = std::min(readBytes, b + piece);
        memcpy(dst + b, src + b, e - b);
    });
    const i64 shift = (i64)head - (reads().size() ? reads().off[0] : 0);
    for (size_t r = 0; r < reads().size(); r++) off.push_back(reads().off[r + 1] + shift);
}

// ---- context, reference upload, and the value table from every sequence of the reference file (map.go:45-71)
int MapRun::openContext() {
    if (dp_ctx_create(device, &ctx.c) != 0) {
        error = dp_last_error(nullptr);
        return DP_ERR_NODEVICE;
    }
    mark("context");
    int rc = dp_reads_upload(ctx.c, (const uint8_t*)refSet.bases.data(), refSet.off.data(), (uint32_t)refSet.size());
    if (rc) return failed(ctx.c, rc);
    values.resize((size_t)1 << (2 * k));
    rc = dp_kmer_values(ctx.c, k, values.data());  // KmerOccurrences + value table + 1 % cut on the GPU
    if (rc) return failed(ctx.c, rc);
    mark("reference upload + value table");
    errText += "K-mer counting complete. Preparing to start indexing and querying...\n";
    errText += J.notes;
    return 0;
}

// ---- AddSingleSeeds seeds/seeds.go:160-200 on the (top-level) reference, host, sequential - on a thread of its own while
// this one waits for the concatenated reads and the device uploads and packs them (neither needs the seeds).
// Everything about a window that does not depend on the seeds added before it - its best k-mer, and which k-mers of
// its count region are the best of ANY window (only those can ever be seeds) - comes from the device for all windows at once
// (dp_single_seed_candidates: the reference and the value table are resident right now); the thread then walks the
// windows in order and probes five or six candidates per window instead of seed_rate k-mers (3.9 s -> 0.1 s per 375 Mb of
// reference).  DP_TUNE=map_seeds_host=1: the whole walk on the host.
// -all_sequences: AddSingleSeeds for one sequence after the other on the ONE index; the device numbers the windows of all sequences
// in sequence order and "best of any window" is over all of them (dp_single_seed_candidates_multi), so the walk is the same.
int MapRun::startSeedWalk() {
    if (!dp_tune("map_seeds_host", 0)) {  // (tests: AddSingleSeeds walked on the host)
        if (p.allSequences) {
            dp_single_seed_multi_batch mb;
            if (int rc = dp_single_seed_candidates_multi(ctx.c, 0, (uint32_t)T, k, p.seedRate, &mb)) return failed(ctx.c, rc);
            ssb.n_windows = mb.n_windows;
            ssb.best = mb.best;
            ssb.cand_off = mb.cand_off;
            ssb.cand = mb.cand;
        } else {
            if (int rc = dp_single_seed_candidates(ctx.c, 0, k, p.seedRate, &ssb)) return failed(ctx.c, rc);
        }
        deviceSeeds = true;
        mark("single-seed candidates (device)");
    }
    seedWalk.t = std::thread([this] { deviceSeeds ? walkCandidates() : walkOnHost(); });
    return 0;
}
void MapRun::walkCandidates() {
    const double ts0 = wallNow();
    for (uint32_t w = 0; w < ssb.n_windows; w++) {
        bool any = false;
        for (uint32_t c = ssb.cand_off[w]; c < ssb.cand_off[w + 1] && !any; c++) any = index.isSeed(ssb.cand[c]);
        if (!any) index.addSeedKmer(ssb.best[w]);
    }
    if (prof)
        fprintf(stderr, "[map setup] single-seed walk: %u windows, %u candidates, %zu seeds, %.1f ms on its thread\n", ssb.n_windows,
                ssb.cand_off[ssb.n_windows], index.seedMap.size(), 1e3 * (wallNow() - ts0));
}
void MapRun::walkOnHost() {
    const uint32_t mask = (uint32_t)(((uint64_t)1 << (2 * k)) - 1);
    for (size_t sq = 0; sq < T; sq++) {  // (one sequence after the other on the one index)
        const char* ref = refSet.seq(sq);
        const i64 refLen = refLens[sq];
        const int finalLen = (int)(refLen % 4);  // top-level sequence: 0 when len%4 == 0 (sequence.go:70,88)
        const i64 skipBack = 4 - finalLen;
        auto code = [&](i64 pos) -> uint32_t { return pos < refLen ? baseCode((unsigned char)ref[pos]) : 0u; };  // zero padding
        auto kmerAt = [&](i64 pos) {
            uint32_t v = 0;
            for (int j = 0; j < k; j++) v = (v << 2) | code(pos + j);
            return v;
        };
        for (i64 i = 0; i < refLen - p.seedRate; i += p.seedRate) {
            // CountKmersBetween(i, i+seedRate, 1, ...) == 0 ?  (sequence.go:332-337 + asm:81-203: whole bytes only,
            // parent's skipBack, do-while group loop)
            const i64 startB = (i + 3) / 4, endB = (i + p.seedRate) / 4;
            const i64 nb = endB - startB;
            const i64 nk = 4 * (nb - 1) - skipBack - k + 1;
            i64 groups = (nk & ~(i64)3) / 4;
            if (groups < 1) groups = 1;
            const i64 P = 4 + 4 * groups + (nk & 3);
            bool any = false;
            {
                const i64 p0 = startB * 4;
                uint32_t km = kmerAt(p0);
                for (i64 j = 0; j < P; j++) {
                    if (j) km = ((km << 2) | code(p0 + j + k - 1)) & mask;
                    if (index.isSeed(km)) {
                        any = true;
                        break;
                    }
                }
            }
            if (!any) {
                const i64 end = i + p.seedRate;
                uint32_t km = kmerAt(i);
                double bestValue = values[km];
                uint32_t best = km;
                for (i64 j = i + k; j < end; j++) {
                    km = ((km << 2) | code(j)) & mask;
                    const double v = values[km];
                    if (v > bestValue) {
                        bestValue = v;
                        best = km;
                    }
                }
                index.addSeedKmer(best);
            }
        }
    }
}

// ---- read upload.  Device ids: 0 reference, 1 join chunk, then (forward, reverse complement) per read; the reverse strands are
// made on the device.
// DP_TUNE=map_async_upload=1: the reads travel while they are mapped (dp_reads_upload_rc_begin: this call returns when the
// reference and the join chunk are packed; the mapper threads wait for "reads below n are packed" block by block).  Built, parity
// tested and left OFF: set-up 14.5 -> 8 ms and the best run 56.0 -> 54.4 ms, but the runs of a process spread 55 - 107 ms where
// they were 56 - 65 (means of 12 runs 69 / 77 against 62 / 69 ms, profiles/r05/map_threads_and_reads_in_flight.txt): the upload's
// copy threads and the link compete with six mapper threads for the same host cores and queues.
int MapRun::uploadReads() {
    concat.join();
    mark("concatenate reads (waited for)");
    const uint32_t firstPaired = J.firstPaired;
    const int rc = packedUpload  ? dp_reads_upload_packed_rc(ctx.c, pinned.p, P.plens.data(), (uint32_t)P.plens.size(), trim ? (uint32_t)P.plens.size() : firstPaired)
                   : asyncUpload ? dp_reads_upload_rc_begin(ctx.c, (const uint8_t*)staging.p.get(), off.data(), (uint32_t)(off.size() - 1), firstPaired, firstPaired)
                                 : dp_reads_upload_rc(ctx.c, (const uint8_t*)staging.p.get(), off.data(), (uint32_t)(off.size() - 1), firstPaired);
    if (rc) return failed(ctx.c, rc);
    mark(trim ? "packed upload (raw reads)" : packedUpload ? "packed upload + reverse strands" : asyncUpload ? "upload begun (reference packed)" : "upload + pack (both strands)");
    return 0;
}

// ---- the trim on the device's copy, the trimmed read set on the host, and the device set cut and paired from the raw one: the
// reference sequences and join chunks first, whole and unpaired, then every trimmed read with its reverse strand
int MapRun::trimAndRespan() {
    std::string trimError;
    if (runTrim(*trim->raw, *trim->front, *trim->back, trim->params, device, *trim->res, trimError, ctx.c) != 0) {
        error = trimError;
        return -1;
    }
    mark("trim on resident reads");
    std::vector<dp_read_span> cut;
    trimmedReadSet(*trim->raw, *trim->res, p.minLength, trim->raw->himem, trimmedSet, cut);
    mark("trimmed read set");
    std::vector<dp_read_span> order;
    order.reserve((size_t)J.firstPaired + cut.size());
    for (size_t c = 0; c < T; c++) order.push_back(dp_read_span{(uint32_t)(P.headAt + c), 0u, (uint32_t)refLens[c]});
    for (size_t j = 0; j < J.joins.size(); j++) order.push_back(dp_read_span{(uint32_t)(P.headAt + T + j), 0u, (uint32_t)J.joins[j].size()});
    order.insert(order.end(), cut.begin(), cut.end());
    if (int rc = dp_reads_respan_rc(ctx.c, order.data(), (uint32_t)order.size(), J.firstPaired)) return failed(ctx.c, rc);
    mark("respan + reverse strands");
    return 0;
}

// ---- chunk scan: the schedule's chunks (map_plan.hpp) scanned with the seeds of the walk, which is waited for here; their segments
// copied to the host for the mapper threads and the shards.  An empty schedule is left to runMap
int MapRun::scanChunks() {
    seedWalk.join();
    mark("AddSingleSeeds (waited for)");
    M.k = k;
    M.edgeSize = p.querySize;
    M.circular = p.circular;
    M.refLens = refLens;
    M.refNames.assign(refSet.names.begin(), refSet.names.begin() + (i64)T);
    sched = mapChunkSchedule(p, refLens, J);
    if (sched.items.empty()) return 0;
    int rc = dp_round_begin(ctx.c, k, index.seedMap.data(), (uint32_t)index.seedMap.size());
    if (rc) return failed(ctx.c, rc);
    rc = dp_scan(ctx.c, sched.items.data(), (uint32_t)sched.items.size(), &sb);
    if (rc) return failed(ctx.c, rc);
    const size_t n = sched.items.size();
    M.chunkSegs.assign(sb.segs, sb.segs + sb.n_segs);
    refs.resize(n);
    M.chunks.resize(n);
    for (size_t i = 0; i < n; i++) {
        refs[i].seg_off = sb.seg_off[i];
        refs[i].n_seeds = sb.n_seeds[i];
        refs[i].reserved = 0;
        M.chunks[i].seg = M.chunkSegs.data() + sb.seg_off[i];
        M.chunks[i].n = (int)(sb.seg_off[i + 1] - sb.seg_off[i]);
        M.chunks[i].offset = sched.meta[i].first;
        M.chunks[i].inset = sched.meta[i].second;
        M.chunks[i].ref = sched.chunkRef[i];
    }
    return 0;
}

// mapper threads (each with a context of its own) when the index is not sharded
size_t MapRun::plannedThreads(size_t nReads) const {
    const size_t n = (size_t)dp_env_long("DP_MAP_THREADS", hostThreads() >= 16 ? 8 : hostThreads() >= 12 ? 6 : hostThreads() >= 8 ? 4 : 3, 1);
    // (fewer reads than that per thread are not worth a context; the key is a test hook)
    const size_t perThread = (size_t)std::max(1L, dp_tune("map_min_reads_per_thread", 2048));
    return std::min(n, std::max<size_t>(1, nReads / perThread));
}
// device bytes of an index of m chunks as dp_index_info counts them (the dense one without asking the device: its build is still queued)
int64_t MapRun::indexBytes(dp_ctx* c, uint64_t m) const {
    const uint64_t S64 = index.seedMap.size();
    if (!sparseIndex) return (int64_t)(mapDenseBytes(S64, m) + 16 * S64 + (uint64_t)sizeof(dp_seq_ref) * m);
    dp_index_info_t ii;
    return dp_index_info(c, &ii) == 0 ? (int64_t)ii.device_bytes : 0;
}

// ---- the reference index's layout (map_plan.hpp: the dense estimate per device against that device's memory), and where it goes:
// DP_MAP_SHARDS=N: the reference index spread over N contexts (DP_MAP_DEVICES=0,1,..: their GPUs, round robin; default all on this
// one) - what BASELINE config 5 does with a 3 Gb reference on 8 GPUs.  With the sparse layout the mapper threads' contexts borrow
// the one index instead of building their own.
int MapRun::chooseIndexLayout() {
    nShards = (int)dp_env_long("DP_MAP_SHARDS", 1, 1, INT_MAX);
    if (const char* e = dp_env_str("DP_MAP_DEVICES")) {
        for (const char* q = e; *q;) {
            devs.push_back(atoi(q));
            while (*q && *q != ',') q++;
            if (*q == ',') q++;
        }
    }
    if (devs.empty()) devs.push_back(device);
    const uint32_t nChunksAll = (uint32_t)sched.items.size();
    perShard = mapChunksPerShard(nChunksAll, (uint32_t)nShards);  // whole 64-chunk words
    sparseIndex = p.indexLayout == 2;
    const std::vector<std::pair<int, uint64_t>> perDev =
        mapDenseEstimate(index.seedMap.size(), nChunksAll, nShards, perShard, devs, device, nShards > 1 ? 0 : plannedThreads(mapperMode ? ~(size_t)0 : reads().size()));
    std::vector<std::pair<uint64_t, uint64_t>> mem(perDev.size());  // free, total
    for (size_t i = 0; i < perDev.size(); i++) {
        if (int rc = dp_device_memory(perDev[i].first, &mem[i].first, &mem[i].second)) return failed(ctx.c, rc);
        if (perDev[i].first == device && stats) stats->device_total = (int64_t)mem[i].second;
    }
    uint64_t dTotal = 0;
    const bool over = mapDenseOverAny(perDev, mem, &dTotal);
    if (p.indexLayout == 0) sparseIndex = over;
    if (stats) {
        stats->dense_estimate = (int64_t)dTotal;
        stats->index_layout = sparseIndex ? 2 : 1;
        for (const dp_seq_ref& r : refs) stats->hits += r.n_seeds;
    }
    if (prof) fprintf(stderr, "[map setup] reference index: dense estimate %.3f GB over %zu device(s) -> %s\n", dTotal / 1e9, perDev.size(), sparseIndex ? "sparse" : "dense");
    return 0;
}

// ---- index build: on the main context, or shard after shard.  Shard s holds the chunks [c0, c1): their segments (imported from the
// chunk scan), posting and seed-set words.  The sets' global windows are combined here once (map_plan.hpp; include/downpore_hip.h,
// dp_index_set_global).
int MapRun::buildIndexOn(dp_ctx* c, const dp_seq_ref* r, uint32_t n) {
    const auto tb0 = std::chrono::steady_clock::now();
    const int rc = sparseIndex ? dp_index_build_sparse(c, r, n) : dp_index_build(c, r, n);
    if (prof) fprintf(stderr, "[map setup] %s index of %u chunks built in %.1f ms\n", sparseIndex ? "sparse" : "dense", n,
                      1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - tb0).count());
    if (rc == 0 && stats) {
        stats->index_bytes += indexBytes(c, n);
        stats->index_builds++;
    }
    return rc;
}
int MapRun::buildShard(Shard& sh, std::vector<uint32_t>& global, std::vector<uint32_t>& local) {
    const uint32_t S = (uint32_t)index.seedMap.size();
    dp_ctx* sc = sh.ctx;
    int rc = dp_round_begin(sc, k, index.seedMap.data(), S);
    if (rc) return failed(sc, rc);
    const uint64_t s0 = sb.seg_off[sh.c0], s1 = sb.seg_off[sh.c1];
    rc = dp_scan_import_segments(sc, M.chunkSegs.data() + s0, s1 - s0);
    if (rc) return failed(sc, rc);
    std::vector<dp_seq_ref> lrefs(refs.begin() + sh.c0, refs.begin() + sh.c1);
    for (dp_seq_ref& r : lrefs) r.seg_off -= s0;
    rc = buildIndexOn(sc, lrefs.data(), (uint32_t)lrefs.size());
    if (rc) return failed(sc, rc);
    rc = dp_index_meta(sc, local.data(), S);
    if (rc) return failed(sc, rc);
    mapGlobalWindowsMerge(global, local, S, sh.c0 / 64);
    return 0;
}
int MapRun::buildIndex() {
    if (nShards > 1) {
        const uint32_t nChunks = (uint32_t)sched.items.size(), S = (uint32_t)index.seedMap.size();
        std::vector<uint32_t> global, local((size_t)S * 4);
        mapGlobalWindowsInit(global, S);
        for (uint32_t c0 = 0; c0 < nChunks; c0 += perShard) {
            Shard sh;
            sh.c0 = c0;
            sh.c1 = std::min(nChunks, c0 + perShard);
            if (dp_ctx_create(devs[shards.v.size() % devs.size()], &sh.ctx) != 0) {
                error = dp_last_error(nullptr);
                return DP_ERR_NODEVICE;
            }
            shards.v.push_back(sh);
            if (int rc = buildShard(shards.v.back(), global, local)) return rc;
        }
        for (Shard& sh : shards.v)
            if (int rc = dp_index_set_global(sh.ctx, global.data(), S, sh.c0 / 64, nChunks)) return failed(sh.ctx, rc);
    } else {
        if (int rc = buildIndexOn(ctx.c, refs.data(), (uint32_t)refs.size())) return failed(ctx.c, rc);
    }
    // dp_scan below reuses the device scan buffer: keep the chunk segments in a dedicated import
    // (dp_index_build references the device-resident scan output, so windows must not overwrite it)
    if (stats) stats->n_chunks = sched.items.size(), stats->n_seeds = index.seedMap.size();
    mark("round begin + chunk scan + index");
    return 0;
}

// ---- One mapper thread: coroutines + batched windows.  Every thread runs this loop on a context of its own (the packed reads are
// shared, the reference index - half a megabyte of chunk segments at E. coli scale - is built once per context), so one thread's
// mapper control flow (mapEnds / mapNext / findSplitPoint of its reads in flight) runs while another thread's windows are on the
// GPU.  (mapping.go:613-619 MapWorker: the reference does the same with goroutines.)
// The reads are dealt in blocks of 1 024: thread t takes blocks t, t + nT, ... - so that every thread finds its first block on the
// device a fraction of a millisecond into the upload (contiguous shares would leave the last thread waiting for five sixths of it).
// Output is per read, in read order, whoever mapped it.
struct MapWorker {
    static constexpr size_t BL = 1024, stackBytes = 256 * 1024;  // (a coroutine's stack is 256 KiB of address space, touched pages only)
    MapRun& R;
    const size_t tIdx, nT;
    LoopStats& ls;
    MapperImpl M;
    size_t inflight = 0;  // reads in flight = windows per dp_map_windows call
    std::vector<std::unique_ptr<Task>> live;
    // coroutine stacks: allocated once (never zero-filled) and recycled — 50 k reads x 256 KiB of fresh zeroed vectors
    // used to be most of the run time
    std::vector<std::unique_ptr<char[]>> stackStore;
    std::vector<char*> freeStacks;
    size_t myCount = 0, nextSeq = 0, waitedBelow = 0;
    // a batch: the live tasks' window requests as scan items (forward, reverse complement), then their segments
    std::vector<dp_scan_item> witems;
    std::vector<int32_t> wsegs;
    std::vector<uint64_t> woff;
    std::vector<uint32_t> wlen;
    double tStart = 0, tItems = 0, tScanCopy = 0, tResume = 0;  // the loop's phases, for the profile line

    MapWorker(MapRun& run, size_t t, size_t n) : R(run), tIdx(t), nT(n), ls(run.lstats[t]), M(run.M) {}
    int failed(dp_ctx* c, int rc) {
        ls.error = dp_last_error(c);
        ls.rc = rc;
        return rc;
    }
    size_t readOf(size_t seq) const { return ((seq / BL) * nT + tIdx) * BL + seq % BL; }
    void run();
    int openContext(double tt0);
    int loop();
    int startTasks();
    void retireTasks();
    void windowItems();
    int scanWindows();
    void takeChains(const dp_chain_batch& cb, uint32_t chunkBase);
    int chainWindows();
};

void MapWorker::run() {
    const double tt0 = wallNow();
    M.ctx = R.ctx.c;
    if (tIdx > 0 && R.workers.v[tIdx]) M.ctx = R.workers.v[tIdx];  // (a Mapper's context of an earlier batch, refreshed by replaceTail)
    else if (tIdx > 0 && openContext(tt0) != 0) return;
    const double tt1 = wallNow();
    loop();
    if (R.prof)
        fprintf(stderr, "[map thread %zu] context + index %.1f ms, loop %.1f (its own clock %.1f), from the loops' start to this thread's end %.1f\n", tIdx, 1e3 * (tt1 - tt0),
                1e3 * (wallNow() - tt1), 1e3 * ls.wall, 1e3 * (wallNow() - R.tLoop0));
}
// a context of its own: shared packed reads, the same seeds, the reference index from the run's chunk scan
int MapWorker::openContext(double tt0) {
    dp_ctx*& tc = R.workers.v[tIdx];
    int rc = dp_ctx_create_shared(R.ctx.c, &tc);
    const double ta = wallNow();
    if (rc == 0) rc = dp_round_begin(tc, R.k, R.index.seedMap.data(), (uint32_t)R.index.seedMap.size());
    const double tb = wallNow();
    if (rc == 0 && !R.sparseIndex) rc = dp_scan_import_segments(tc, R.M.chunkSegs.data(), R.M.chunkSegs.size());
    const double tc0 = wallNow();
    if (rc == 0 && R.sparseIndex) rc = dp_index_borrow(tc, R.ctx.c);  // (the one sparse index, read-only)
    else if (rc == 0) rc = dp_index_build(tc, R.refs.data(), (uint32_t)R.refs.size());
    if (rc == 0 && !R.sparseIndex && R.stats) {
        std::lock_guard<std::mutex> lk(R.infoMu);
        R.stats->index_bytes += R.indexBytes(tc, R.refs.size());
        R.stats->index_builds++;
    }
    if (R.prof) fprintf(stderr, "[map thread %zu] context %.2f ms, round begin %.2f, import %.2f, index %.2f\n", tIdx, 1e3 * (ta - tt0), 1e3 * (tb - ta), 1e3 * (tc0 - tb), 1e3 * (wallNow() - tc0));
    if (rc != 0) {
        ls.rc = rc;
        ls.error = tc ? dp_last_error(tc) : dp_last_error(nullptr);
        return rc;
    }
    M.ctx = tc;
    return 0;
}

// Reads in flight per thread (DP_MAP_INFLIGHT: another number).
// Measured at config 3 (profiles/r05/map_threads_and_reads_in_flight.txt): 3 threads x 1 365 reads = 120 launches, 20.7 ms of
// map_kernel, loops of 60 - 70 ms; 4 x 2 730 = 64 launches, 14.5 ms, loops of 41 - 46 ms; 8 192 and more per thread: fewer launches
// still (10.6 ms of kernels) but the threads' control flow no longer fits their caches and runs less beside the GPU's work
// and once a context's teardown no longer cost 5 ms, more threads paid: 6 x 2 730 = 78 launches, 18 ms of kernels, a run of 58 - 60 ms
// (856 k reads/s) against 64 - 70 ms with 4 x 2 730 and 61 - 70 with 8 x 2 048
// once a context no longer costs a thread 4 ms: 8 x 2 048 runs 46 - 47 ms where 6 x 2 730 runs 50 - 51 (three alternations on
// one box, profiles/r06/map_threads_sweep.txt)
int MapWorker::loop() {
    const double tl0 = wallNow();
    inflight = nT >= 8 ? 2048 : std::max<size_t>(2730, 10922 / nT);
    inflight = (size_t)dp_env_long("DP_MAP_INFLIGHT", (long)inflight, 64);
    const size_t nReads = R.reads().size();
    for (size_t blk = tIdx; blk * BL < nReads; blk += nT) myCount += std::min(BL, nReads - blk * BL);
    while (nextSeq < myCount || !live.empty()) {
        const double t0 = wallNow();
        if (int rc = startTasks()) return rc;
        retireTasks();
        const double t1 = wallNow();
        tStart += t1 - t0;  // new tasks up to their first window + finished ones retired
        if (live.empty()) continue;
        windowItems();
        const double t2 = wallNow();
        tItems += t2 - t1;
        if (int rc = scanWindows()) return rc;
        const double t3 = wallNow();
        tScanCopy += t3 - t2;  // scan call + copying its segments out
        if (int rc = chainWindows()) return rc;
        const double t4 = wallNow();
        ls.tChain += t4 - t3;
        for (auto& tk : live) coroSwitch(M.sched.main, tk->at);  // distribute and resume
        tResume += wallNow() - t4;  // performMapping's tail + the mapper's control flow up to the next window
    }
    if (R.prof)
        fprintf(stderr, "[map loop] thread %zu of %zu: start/retire + upload waits %.1f ms, items %.1f, scan+copy %.1f (scan call %.1f), map call %.1f, resume %.1f\n", tIdx, nT,
                1e3 * tStart, 1e3 * tItems, 1e3 * tScanCopy, 1e3 * ls.tScan, 1e3 * ls.tChain, 1e3 * tResume);
    ls.wall = wallNow() - tl0;
    return 0;
}
// new read tasks up to `inflight`, each run to its first window request (or completion)
int MapWorker::startTasks() {
    const size_t nReads = R.reads().size();
    while (live.size() < inflight && nextSeq < myCount) {
        const size_t nextRead = readOf(nextSeq);
        if (nextRead >= waitedBelow) {  // (the block may still be on its way to the device: dp_reads_upload_rc_begin)
            const size_t upto = std::min(nReads, (nextRead / BL + 1) * BL);
            // the main context owns the reads: the threads ask it how far their upload has come (the host reads before them: the
            // reference and its join chunks)
            if (int rc = dp_reads_upload_wait(R.ctx.c, (uint32_t)(R.J.firstPaired + upto))) return failed(M.ctx, rc);
            waitedBelow = upto;
        }
        std::unique_ptr<Task> t(new Task());
        t->m = &M;
        t->read = (uint32_t)nextRead;
        t->L = R.reads().length(nextRead);
        if (freeStacks.empty()) {
            stackStore.emplace_back(new char[stackBytes]);
            freeStacks.push_back(stackStore.back().get());
        }
        t->stack = freeStacks.back();
        freeStacks.pop_back();
        coroStart(t->at, t->stack, stackBytes, &coroTrampoline, t.get());
        nextSeq++;
        coroSwitch(M.sched.main, t->at);
        live.push_back(std::move(t));
    }
    return 0;
}
void MapWorker::retireTasks() {
    for (size_t i = 0; i < live.size();) {
        if (live[i]->done) {
            Task& t = *live[i];
            std::string& o = R.out[t.read];
            for (Mapping* mm : t.results) o += M.asString(*mm, R.reads().names[t.read], t.L) + "\n";
            if (R.alignOn)  // what the alignment needs of each line: its spans are worked out once every read has retired
                for (Mapping* mm : t.results) {
                    AlignLine ln;
                    ln.L = t.L, ln.queryOffset = mm->QueryOffset, ln.queryInset = mm->QueryInset;
                    ln.start = mm->Start, ln.end = mm->End, ln.rc = mm->RC, ln.ref = mm->ref;
                    R.lines[t.read].push_back(ln);
                }
            R.nmaps[t.read] = (int)t.results.size();
            coroRelease(t.at);
            freeStacks.push_back(t.stack);
            live[i] = std::move(live.back());
            live.pop_back();
        } else {
            i++;
        }
    }
}
void MapWorker::windowItems() {
    witems.clear();
    for (auto& tk : live) {
        const WindowReq& q = tk->req;
        dp_scan_item f, r;
        mapWindowItems(R.J.firstPaired, q.read, tk->L, q.a, q.b, q.whole, R.k, f, r);
        witems.push_back(f);
        witems.push_back(r);
    }
}
// scan the requested windows and hand every task its two seed sequences
int MapWorker::scanWindows() {
    dp_seedseq_batch wb;
    const double ts0 = wallNow();
    if (int rc = dp_scan(M.ctx, witems.data(), (uint32_t)witems.size(), &wb)) return failed(M.ctx, rc);
    ls.tScan += wallNow() - ts0;
    ls.st.k_scan_ms += wb.kernel_ms, ls.st.n_windows += witems.size() / 2;
    for (const dp_scan_item& wi : witems) ls.st.scan_bytes += (double)((wi.n_kmers + 3) / 4);  // packed bases of the window, both strands
    wsegs.clear();
    woff.assign(1, 0);
    wlen.clear();
    for (size_t w = 0; w < witems.size(); w++) {
        Task& t = *live[w / 2];
        const size_t base = wsegs.size();
        wsegs.insert(wsegs.end(), wb.segs + wb.seg_off[w], wb.segs + wb.seg_off[w + 1]);
        if (mapReverseNeedsFix((w & 1) != 0, t.req.whole, t.L)) mapFixReverseWhole(wsegs, base, R.k);
        woff.push_back(wsegs.size());
        wlen.push_back((uint32_t)(t.req.b - t.req.a));
    }
    for (auto& tk : live) {
        tk->res.seg[0].clear();
        tk->res.seg[1].clear();
        tk->res.chains[0].clear();
        tk->res.chains[1].clear();
    }
    for (size_t w = 0; w < witems.size(); w++)
        live[w / 2]->res.seg[w & 1].assign(wsegs.begin() + (i64)woff[w], wsegs.begin() + (i64)woff[w + 1]);
    return 0;
}
void MapWorker::takeChains(const dp_chain_batch& cb, uint32_t chunkBase) {
    for (uint32_t c = 0; c < cb.n_chains; c++) {
        const uint32_t w = cb.window[c];
        WindowResult::ChainRef cr;
        cr.target = cb.target[c] + chunkBase;
        cr.a.assign(cb.match_a + cb.off[c], cb.match_a + cb.off[c + 1]);
        cr.b.assign(cb.match_b + cb.off[c], cb.match_b + cb.off[c + 1]);
        live[w / 2]->res.chains[w & 1].push_back(std::move(cr));
    }
    ls.st.k_map_ms += cb.kernel_ms, ls.st.n_chains += cb.n_chains, ls.st.map_bytes += cb.alg_bytes;
}
// the candidate / chaining stage of the batch: on this thread's context, or shard after shard
int MapWorker::chainWindows() {
    const uint32_t nW = (uint32_t)witems.size();
    if (R.shards.v.empty()) {
        // the window scan has reused the device scan buffer the dense index's chunk segments lived in: they are imported again
        // before the map stage (the sparse index holds its own copy of the chunk segments)
        if (!R.sparseIndex)
            if (int rc = dp_scan_import_segments(M.ctx, R.M.chunkSegs.data(), R.M.chunkSegs.size())) return failed(M.ctx, rc);
        dp_chain_batch cb;
        if (int rc = dp_map_windows(M.ctx, wsegs.data(), woff.data(), wlen.data(), nW, R.k, &cb)) return failed(M.ctx, rc);
        takeChains(cb, 0);
    } else {
        // candidates of a window in ascending chunk id = shard after shard; forward strand over all shards first, its
        // ratchet raises the reverse threshold too (mapping.go:543-549): the thresholds travel with the batch
        std::vector<int32_t> thr(witems.size(), -1);
        for (int phase = 0; phase < 2; phase++)
            for (Shard& sh : R.shards.v) {
                dp_chain_batch cb;
                if (int rc = dp_map_windows_shard(sh.ctx, wsegs.data(), woff.data(), wlen.data(), nW, R.k, phase, thr.data(), &cb)) return failed(sh.ctx, rc);
                takeChains(cb, sh.c0);
            }
    }
    ls.st.n_batches++;
    return 0;
}

// ---- Map every read: the reads are dealt to a few host threads; the first works on the main context
int MapRun::runWorkers() {
    tLoop0 = wallNow();
    if (stats) stats->t_setup_s = tLoop0 - tRun0;
    out.assign(reads().size(), std::string());
    nmaps.assign(reads().size(), 0);
    lines.assign(alignOn ? reads().size() : 0, std::vector<AlignLine>());
    nThreads = shards.v.empty() ? plannedThreads(reads().size()) : 1;
    lstats.assign(nThreads, LoopStats());
    if (workers.v.size() < nThreads) workers.v.resize(nThreads, nullptr);  // (a Mapper's contexts of earlier batches stay in their slots)
    {
        std::vector<std::unique_ptr<MapWorker>> ws;
        for (size_t t = 0; t < nThreads; t++) ws.emplace_back(new MapWorker(*this, t, nThreads));
        std::vector<std::thread> th;
        for (size_t t = 0; t < nThreads; t++) th.emplace_back([&ws, t] { ws[t]->run(); });
        for (auto& t : th) t.join();
    }
    if (stats) {  // queries per regime: every thread's context, or one shard (every shard answers every window)
        std::vector<dp_ctx*> qc;
        if (shards.v.empty()) {
            qc = workers.v;
            qc[0] = ctx.c;
        } else {
            qc.push_back(shards.v[0].ctx);
        }
        for (dp_ctx* c : qc) {
            dp_index_info_t ii;
            if (c && dp_index_info(c, &ii) == 0)
                for (int r = 0; r < 4; r++) stats->regimes[r] += (int64_t)ii.queries[r];
        }
        for (int r = 0; r < 4; r++) {  // (what earlier batches of a Mapper have already reported)
            stats->regimes[r] -= regimesSeen[r];
            regimesSeen[r] += stats->regimes[r];
        }
    }
    const double tJoin = wallNow();
    if (!mapperMode) workers.destroy();
    if (prof) fprintf(stderr, "[map end] threads joined at %.1f ms after the loops' start, their contexts destroyed in %.1f\n", 1e3 * (tJoin - tLoop0), 1e3 * (wallNow() - tJoin));
    for (size_t t = 0; t < nThreads; t++)
        if (lstats[t].rc != 0) {
            error = lstats[t].error;
            return lstats[t].rc;
        }
    return 0;
}

void MapRun::collectStats() {
    if (!stats) return;
    double tScan = 0, tChain = 0;
    for (const LoopStats& ls : lstats) {
        stats->k_scan_ms += ls.st.k_scan_ms;
        stats->k_map_ms += ls.st.k_map_ms;
        stats->map_bytes += ls.st.map_bytes;
        stats->scan_bytes += ls.st.scan_bytes;
        stats->n_windows += ls.st.n_windows;
        stats->n_chains += ls.st.n_chains;
        stats->n_batches += ls.st.n_batches;
        tScan += ls.tScan / (double)nThreads;   // (means over the threads, which run side by side)
        tChain += ls.tChain / (double)nThreads;
    }
    stats->t_scan_s = tScan;
    stats->t_chain_s = tChain;
    stats->t_host_s = (wallNow() - tLoop0) - tScan - tChain;
}

// ---- NM and cg tags behind every line of the batch.  The mappings are finished and both strands of every read and the
// reference sequences are resident: each line's spans (align_plan.hpp) become one item of dp_align_spans on the main context - forward
// read firstPaired + 2 r, its reverse strand + 1, reference sequence c - and the tags go behind the line's column 12.  A line out of
// range or over max_edits keeps its twelve columns and is counted.
int MapRun::alignMappings() {
    const double t0 = wallNow();
    std::vector<dp_align_item> items;
    std::vector<int64_t> itemOf;  // per line in (read, line) order: its item, -1 = out of range
    i64 nLines = 0, outOfRange = 0, aligned = 0, over = 0;
    for (size_t r = 0; r < lines.size(); r++)
        for (const AlignLine& ln : lines[r]) {
            nLines++;
            AlignSpan sp;
            if (!alignSpanOf(ln, refLens[(size_t)ln.ref], p.circular, sp)) {
                outOfRange++;
                itemOf.push_back(-1);
                continue;
            }
            itemOf.push_back((int64_t)items.size());
            items.push_back(alignItemOf(sp, J.firstPaired, (uint32_t)r, ln.rc, ln.ref));
        }
    dp_align_batch ab;
    memset(&ab, 0, sizeof ab);
    if (!items.empty())
        if (int rc = dp_align_spans(ctx.c, items.data(), (uint32_t)items.size(), maxEdits, p.circular ? 1 : 0, &ab)) return failed(ctx.c, rc);
    size_t at = 0;
    std::string tagged;
    for (size_t r = 0; r < lines.size(); r++) {
        if (lines[r].empty()) continue;
        tagged.clear();
        size_t b = 0;
        for (size_t li = 0; li < lines[r].size(); li++, at++) {
            const size_t e = out[r].find('\n', b);
            tagged.append(out[r], b, e - b);
            if (itemOf[at] >= 0) {
                const dp_align_rec& rec = ab.recs[itemOf[at]];
                if (rec.nm >= 0) {
                    tagged += alignTags(rec.nm, ab.runs + rec.run_off, rec.n_runs);
                    aligned++;
                } else {
                    over++;
                }
            }
            tagged += '\n';
            b = e + 1;
        }
        out[r].swap(tagged);
    }
    if (stats) {
        const int64_t v[8] = {nLines, aligned, over, outOfRange, (int64_t)ab.cells, (int64_t)ab.doublings, (int64_t)(1e3 * ab.kernel_ms), (int64_t)ab.tb_bytes};
        for (int i = 0; i < 8; i++) stats->align[i] = v[i];
    }
    if (prof) fprintf(stderr, "[map align] %lld lines, %zu items, %.1f ms (kernels %.1f ms)\n", (long long)nLines, items.size(), 1e3 * (wallNow() - t0), ab.kernel_ms);
    return 0;
}

void MapRun::writeCounts(i64 mapped, i64 multiple, i64 total, i64 unmapped) {
    char line[160];
    snprintf(line, sizeof line, "Uniquely mapped: %lld\nMultiple mappings: %lld\ntotal: %lld\nUnmapped: %lld\n", (long long)mapped,
             (long long)multiple, (long long)total, (long long)unmapped);
    errText += line;
}
void MapRun::unmappedBatch() {
    if (stats) stats->n_seeds = index.seedMap.size(), stats->t_setup_s = wallNow() - tRun0;
    writeCounts(0, 0, 0, (i64)reads().size());
}
void MapRun::writeText() {
    i64 unmapped = 0, mapped = 0, multiple = 0, total = 0;
    for (size_t r = 0; r < reads().size(); r++) {
        paf += out[r];
        if (nmaps[r] > 0) {
            if (nmaps[r] == 1) mapped++;
            else multiple++;
            total += nmaps[r];
        } else {
            unmapped++;
        }
    }
    writeCounts(mapped, multiple, total, unmapped);
}

}  // namespace

// The whole `map` command as its steps in order.  MapRun's owners make every `return rc` below complete: they go in the order worker
// contexts, shard contexts, upload wait + staging block, seed-walk thread, main context, packing thread, pinned block.
int runMap(const ReadSet& refSet, const ReadSet& upSet, const MapParams& p, int device, std::string& paf, std::string& errText,
           MapStats* stats, std::string& error, MapTrim* trim) {
    MapRun R(refSet, upSet, p, device, paf, errText, stats, error, trim);
    int rc;
    if ((rc = R.check())) return rc;
    R.layoutAndStage();
    if ((rc = R.allocBlocks())) return rc;
    R.concat.t = std::thread([&R] { R.packOrConcatenate(); });
    if ((rc = R.openContext())) return rc;
    if ((rc = R.startSeedWalk())) return rc;
    if ((rc = R.uploadReads())) return rc;
    if (trim && (rc = R.trimAndRespan())) return rc;
    if ((rc = R.scanChunks())) return rc;
    if (R.sched.items.empty()) {  // no sequence is long enough for a chunk: an empty index matches nothing, every read is unmapped
        R.unmappedBatch();
        return 0;
    }
    if ((rc = R.chooseIndexLayout())) return rc;
    if ((rc = R.buildIndex())) return rc;
    if ((rc = R.runWorkers())) return rc;
    R.collectStats();
    const double tText0 = wallNow();
    R.writeText();
    const double tEnd0 = wallNow();
    R.ctx.destroy();  // (before the timing line: the owners would do it just as well)
    if (R.prof) fprintf(stderr, "[map end] text joined in %.1f ms, context destroyed in %.1f, whole run %.1f\n", 1e3 * (tEnd0 - tText0), 1e3 * (wallNow() - tEnd0), 1e3 * (wallNow() - R.tRun0));
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------
// A Mapper: the reference program's NewMapper once, then MapWorker over batch after batch of reads.  It is a MapRun whose steps are
// regrouped, none copied: open runs the steps that look at the reference alone (with an empty read set, so the one upload carries the
// head only), and a batch runs the steps that look at the reads.  What stays from batch to batch: the main context with the head, the
// value table, the seed index, the schedule and chunk scan, the layout choice, the index, the pinned block, and every worker context
// a batch's thread plan has asked for so far (its round, import and dense build or borrow are done once, when it is opened).  What a
// batch owns: its read set's binding, the packed batch in the pinned block, the tail replace and the workers' refreshes, the loops,
// and its paf / stderr / stats.  A batch that is trimmed first (mapperMap with a MapTrim) has replaceTailTrimmed in replaceTail's place:
// the raw batch behind the head unpaired, runTrim on it, and the trimmed set cut from the raw tail with its reverse strands.
// The owners are MapRun's and go in MapRun's order when the mapper is closed.
void MapRun::bindBatch(const ReadSet& batch, bool trimmed) {
    upSetP = &batch;
    readsP = trimmed ? &trimmedSet : &batch;  // (a trimmed batch goes up raw and is mapped as trimmedReadSet gives it)
    tRun0 = tMark = wallNow();
    paf.clear();
    errText = refText;
    error.clear();
    // the reference side's figures stay (chunks, seeds, index layout / bytes / builds, hits); what the loops count starts again
    stats->n_windows = stats->n_chains = stats->n_batches = 0;
    stats->k_scan_ms = stats->k_map_ms = stats->map_bytes = stats->scan_bytes = 0;
    stats->t_setup_s = stats->t_scan_s = stats->t_chain_s = stats->t_host_s = 0;
    for (int64_t& r : stats->regimes) r = 0;
    for (int64_t& a : stats->align) a = 0;
}
// the batch packed into the pinned block, put behind the head on the device, and the worker contexts told about it
int MapRun::packBatch() {
    P = mapBatchLayout(upSet().off.data(), upSet().size());
    if (!pinned.reserve((size_t)P.poff.back() + 64)) {
        error = "dp_host_alloc: no pinned memory for the packed reads";
        return DP_ERR_HIP;
    }
    packReads(P.poff, 0);
    mark("pack the batch");
    return 0;
}
int MapRun::refreshWorkers() {
    for (dp_ctx* wc : workers.v)
        if (wc)
            if (int rc = dp_ctx_refresh_shared(wc)) return failed(wc, rc);
    return 0;
}
int MapRun::replaceTail() {
    if (int rc = packBatch()) return rc;
    if (int rc = dp_reads_replace_tail_packed_rc(ctx.c, J.firstPaired, pinned.p, P.plens.data(), (uint32_t)P.plens.size())) return failed(ctx.c, rc);
    if (int rc = refreshWorkers()) return rc;
    mark("tail replace + refreshes");
    return 0;
}
// A batch that is trimmed first: the raw reads go behind the head unpaired (raw read r is device read firstPaired + r), the trim runs
// on that copy, and the trimmed set with its reverse strands is cut from the raw tail in place of it - the ids replaceTail gives.
// DP_ERR_ARG: the trim failed for its parameters or its input; whatever the tail holds then, the next batch replaces it.
int MapRun::replaceTailTrimmed(MapTrim& t) {
    if (int rc = packBatch()) return rc;
    const uint32_t base = J.firstPaired;
    if (int rc = dp_reads_replace_tail_packed(ctx.c, base, pinned.p, P.plens.data(), (uint32_t)P.plens.size())) return failed(ctx.c, rc);
    mark("tail replace (raw reads)");
    std::string trimError;
    if (int rc = runTrim(*t.raw, *t.front, *t.back, t.params, device, *t.res, trimError, ctx.c, base)) {
        error = trimError;
        return rc == kTrimDeviceFailed ? DP_ERR_HIP : DP_ERR_ARG;
    }
    mark("trim on resident reads");
    std::vector<dp_read_span> cut;
    trimmedReadSet(*t.raw, *t.res, p.minLength, t.raw->himem, trimmedSet, cut);
    mark("trimmed read set");
    const std::vector<dp_read_span> spans = mapTailSpans(cut, base);
    if (int rc = dp_reads_respan_tail_rc(ctx.c, base, spans.data(), (uint32_t)spans.size())) return failed(ctx.c, rc);
    if (int rc = refreshWorkers()) return rc;
    mark("respan + reverse strands + refreshes");
    return 0;
}

struct Mapper {
    const MapParams p;  // (MapRun holds references to these: they are declared before it)
    ReadSet none;       // the read set of the open: the head goes up alone
    std::string paf, errText, error;
    MapStats st;
    MapRun R;
    int brokenRc = 0;  // the first device error: every later batch returns it without touching the device
    std::string brokenText;
    Mapper(const ReadSet& refSet, const MapParams& p_, int device) : p(p_), R(refSet, none, p, device, paf, errText, &st, error, nullptr) {
        R.mapperMode = true;
    }
};

Mapper* mapperOpen(const ReadSet& refSet, const MapParams& p, int device, std::string& error, int* rcOut) {
    int rc = 0;
    auto fail = [&](int code, const std::string& text) {
        error = text;
        if (rcOut) *rcOut = code;
        return (Mapper*)nullptr;
    };
    if (dp_env_long("DP_MAP_SHARDS", 1, 1, INT_MAX) > 1) return fail(DP_ERR_ARG, "mapper: DP_MAP_SHARDS > 1 is not supported by a mapper (use the one-shot map call)");
    for (const char* key : {"map_ascii_upload", "map_async_upload"})
        if (dp_tune(key, 0) != 0) return fail(DP_ERR_ARG, std::string("mapper: DP_TUNE=") + key + " is not supported by a mapper (use the one-shot map call)");
    std::unique_ptr<Mapper> m(new Mapper(refSet, p, device));
    MapRun& R = m->R;
    auto failRun = [&](int code) { return fail(code, m->error); };  // (the owners give everything back, in MapRun's order)
    if ((rc = R.check())) return failRun(rc);
    R.layoutAndStage();
    if ((rc = R.allocBlocks())) return failRun(rc);
    R.concat.t = std::thread([&R] { R.packOrConcatenate(); });
    if ((rc = R.openContext())) return failRun(rc);
    if ((rc = R.startSeedWalk())) return failRun(rc);
    if ((rc = R.uploadReads())) return failRun(rc);
    if ((rc = R.scanChunks())) return failRun(rc);
    R.noChunks = R.sched.items.empty();
    if (!R.noChunks) {
        if ((rc = R.chooseIndexLayout())) return failRun(rc);
        if ((rc = R.buildIndex())) return failRun(rc);
    } else {
        m->st.n_seeds = R.index.seedMap.size();
    }
    R.refText = m->errText;
    if (rcOut) *rcOut = 0;
    return m.release();
}

namespace {
// one batch: trim == nullptr maps `reads` as they are; with a trim `reads` is the raw set (trim->raw)
int mapperBatch(Mapper* m, const ReadSet& reads, MapTrim* trim, const int64_t* maxEdits, std::string& paf, std::string& errText, MapStats* stats,
                std::string& error) {
    if (m->brokenRc) {
        error = m->brokenText;
        return m->brokenRc;
    }
    if (maxEdits && (*maxEdits < 1 || *maxEdits > kAlignMaxEditsLimit)) {  // (refused before the batch touches anything)
        error = "map align: max_edits " + std::to_string((long long)*maxEdits) + " (1 .. 32768)";
        return DP_ERR_ARG;
    }
    MapRun& R = m->R;
    R.alignOn = maxEdits != nullptr;
    R.maxEdits = maxEdits ? (uint32_t)*maxEdits : (uint32_t)kAlignMaxEditsDefault;
    R.bindBatch(reads, trim != nullptr);
    int rc = 0;
    if (R.noChunks) {  // (the trim still runs: its result is the caller's, and the counts are of the trimmed set)
        if (!trim || (rc = R.replaceTailTrimmed(*trim)) == 0) R.unmappedBatch();
    } else {
        if ((rc = trim ? R.replaceTailTrimmed(*trim) : R.replaceTail()) == 0 && (rc = R.runWorkers()) == 0) {
            R.collectStats();
            if (!R.alignOn || (rc = R.alignMappings()) == 0) R.writeText();
        }
    }
    R.upSetP = R.readsP = &m->none;  // (the batch's read set is the caller's: nothing of it is held beyond this call)
    R.trimmedSet = ReadSet();
    R.lines.clear();
    if (rc) {
        error = m->error;
        if (rc != DP_ERR_ARG) {  // a batch refused for its arguments (or its trim's) leaves nothing the next batch does not replace; anything else leaves the device state unknown
            m->brokenRc = rc;
            m->brokenText = error;
        }
        return rc;
    }
    paf.swap(m->paf);
    errText.swap(m->errText);
    if (stats) *stats = m->st;
    return 0;
}
}  // namespace
int mapperMap(Mapper* m, const ReadSet& reads, std::string& paf, std::string& errText, MapStats* stats, std::string& error) {
    return mapperBatch(m, reads, nullptr, nullptr, paf, errText, stats, error);
}
int mapperMap(Mapper* m, MapTrim& trim, std::string& paf, std::string& errText, MapStats* stats, std::string& error) {
    return mapperBatch(m, *trim.raw, &trim, nullptr, paf, errText, stats, error);
}
int mapperMapAlign(Mapper* m, const ReadSet* reads, MapTrim* trim, int64_t maxEdits, std::string& paf, std::string& errText, MapStats* stats,
                   std::string& error) {
    return mapperBatch(m, trim ? *trim->raw : *reads, trim, &maxEdits, paf, errText, stats, error);
}

void mapperClose(Mapper* m) { delete m; }

// ---- self-test of the coroutine switch (dph_testhooks.h: dph_test_coroutines): n_tasks coroutines on recycled stacks, every one adds
// its number `yields` times with a switch back to the caller in between and touches its stack deeply; returns the sum (-1: a task
// was resumed with a damaged frame).  What the mapper does with its read tasks, without a GPU - and under the sanitizer builds.
namespace {
struct CoroTestTask {
    CoroPoint at, *main = nullptr;
    int id = 0, yields = 0;
    long sum = 0;
    bool done = false, bad = false;
};
void coroTestBody(void* arg) {
    CoroTestTask* t = (CoroTestTask*)arg;
    volatile char pad[8192];
    for (int y = 0; y < t->yields; y++) {
        for (size_t i = 0; i < sizeof(pad); i += 64) pad[i] = (char)(t->id + y);
        coroSwitch(t->at, *t->main);
        for (size_t i = 0; i < sizeof(pad); i += 64)
            if (pad[i] != (char)(t->id + y)) t->bad = true;
        t->sum += t->id;
    }
    t->done = true;
    coroSwitch(t->at, *t->main, true);
}
}  // namespace
long coroSelfTest(int nTasks, int yields) {
    const size_t stackBytes = (size_t)64 << 10;
    CoroPoint main;
    std::vector<std::unique_ptr<char[]>> store;
    std::vector<char*> freeStacks;
    long sum = 0;
    const int wave = 7;  // tasks alive at a time: stacks are reused by later tasks
    for (int base = 0; base < nTasks; base += wave) {
        std::vector<std::unique_ptr<CoroTestTask>> live;
        std::vector<char*> mine;
        for (int i = base; i < std::min(nTasks, base + wave); i++) {
            if (freeStacks.empty()) {
                store.emplace_back(new char[stackBytes]);
                freeStacks.push_back(store.back().get());
            }
            live.emplace_back(new CoroTestTask());
            CoroTestTask& t = *live.back();
            t.main = &main;
            t.id = i + 1;
            t.yields = yields;
            mine.push_back(freeStacks.back());
            freeStacks.pop_back();
            coroStart(t.at, mine.back(), stackBytes, &coroTestBody, &t);
            coroSwitch(main, t.at);
        }
        for (bool any = true; any;) {
            any = false;
            for (auto& t : live)
                if (!t->done) {
                    coroSwitch(main, t->at);
                    any = true;
                }
        }
        for (size_t i = 0; i < live.size(); i++) {
            if (live[i]->bad) return -1;
            sum += live[i]->sum;
            coroRelease(live[i]->at);
            freeStacks.push_back(mine[i]);
        }
    }
    return sum;
}

}  // namespace dph
