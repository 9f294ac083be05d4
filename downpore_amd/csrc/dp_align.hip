// Base-level alignment of spans of the resident read set: unit-cost edit distance (NM) and the canonical CIGAR of DESIGN.md 4.9.
//
// One wave per pair, row by row over a band of diagonals d = j - i in [dlo, dlo + 64 C): lane l owns the C diagonals from dlo + l C on,
// so a row's state - the previous row's values on those diagonals - is private to the lane (LDS, or device memory for bands too wide
// for it).  A cell takes its diagonal neighbour from the lane's own cell of the previous row, its upper neighbour from the next
// diagonal (the lane's next cell, or the first cell of lane l + 1: one shuffle per row), and its left neighbour from the row itself:
// D[i][j] = min over j' <= j of V[j'] + (j - j'), V = min(diagonal, upper + 1) - a running minimum inside the lane and one shifted
// min-scan over the 64 lanes.  Two bits per cell (the move rule 7 takes at that cell) go to the trace-back buffer; a second kernel,
// one thread per pair, walks them back from (m, n) and writes the runs.
//
// The band (Ukkonen).  A path from (0, 0) to (m, n) starts on diagonal 0 and ends on diagonal n - m; a gap moves it by one diagonal.
// One that leaves the diagonals [min(0, n - m) - w, max(0, n - m) + w] therefore costs more than |m - n| + 2 w.  So when the banded
// result s satisfies s <= |m - n| + 2 w, every optimal path of the full matrix lies inside the band: s is NM, every cell on an optimal
// path has its full-matrix value in the band, and every other cell has at least its full-matrix value.  The walk of rule 7 visits only
// cells on optimal paths and accepts only neighbours on optimal paths (values <= NM), and a neighbour the full matrix refuses is refused
// here too (its banded value is no smaller): the banded walk is the full matrix's walk, move for move.  While s fails the test the half
// width doubles (from 64); once |m - n| + 2 w >= max_edits a failing s proves NM > max_edits.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "dp_common.h"

namespace {

constexpr int32_t AL_INF = 1 << 29;
constexpr uint32_t AL_MAX_SPAN = 1u << 20, AL_W0 = 64, AL_MAX_EDITS = 32768;
constexpr uint32_t AL_LDS_MAX_C = 128;  // 2 arrays x 64 lanes x C x 4 bytes = 64 KiB at C = 128

struct AlJob {                 // one attempt at one pair
    uint64_t q_byte, t_byte;   // where the two reads start in the packed block
    uint64_t tb_off;           // bytes into the trace-back buffer: rows 1 .. m of 16 C bytes
    uint64_t row_off;          // device-memory tier: ints into the row scratch (2 x 64 C)
    uint32_t q_off, t_off, t_rlen, m, n;
    int32_t dlo;               // lowest diagonal of the band
    uint32_t C, item;
};

struct AlTrace {               // a pair whose attempt succeeded: where its runs go
    uint32_t job, cap;
    uint64_t run_off;
};

__device__ __forceinline__ uint32_t al_code(const uint32_t word, const uint32_t g) {  // base g of its 16-base word (first base in a byte's top bits)
    return (word >> ((((g >> 2) & 3u) << 3) + 6u - ((g & 3u) << 1))) & 3u;
}

template <bool LDS>
__global__ __launch_bounds__(64) void align_forward_kernel(const uint8_t* __restrict__ packed, const AlJob* __restrict__ jobs, const int circular,
                                                           uint8_t* __restrict__ tb, int32_t* __restrict__ scratch, int32_t* __restrict__ nm_out) {
    extern __shared__ int32_t al_lds[];
    const AlJob J = jobs[blockIdx.x];
    const int lane = (int)threadIdx.x, C = (int)J.C, m = (int)J.m, n = (int)J.n;
    int32_t* const P = LDS ? al_lds : scratch + J.row_off;  // [C][64]: the previous row on this lane's diagonals
    int32_t* const X = P + 64 * C;                           // [C][64]: the row without what reaches it from the lanes below, bit 31 = mismatch
    const uint32_t* const tw = (const uint32_t*)(packed + J.t_byte);
    const uint8_t* const qb = packed + J.q_byte;
    const int b0 = lane * C;
    for (int c = 0; c < C; c++) {  // row 0: D[0][j] = j
        const int j = J.dlo + b0 + c;
        P[c * 64 + lane] = (j >= 0 && j <= n) ? j : AL_INF;
    }
    for (int i = 1; i <= m; i++) {  // (m rows of C cells per lane: every loop here is bounded by the job)
        const uint32_t qg = J.q_off + (uint32_t)(i - 1);
        const uint32_t qc = ((uint32_t)qb[qg >> 2] >> (6u - ((qg & 3u) << 1))) & 3u;
        const int j0 = i + J.dlo + b0;  // column of this lane's first cell
        int32_t pc = P[lane];
        int32_t pnext = __shfl_down(pc, 1, 64);  // the first diagonal of the next lane, previous row
        if (lane == 63) pnext = AL_INF;
        const int32_t p0 = pc;
        uint32_t curw = 0xffffffffu, word = 0;
        int32_t run = AL_INF;
        for (int c = 0; c < C; c++) {
            const int32_t pn = c + 1 < C ? P[(c + 1) * 64 + lane] : pnext;
            const int j = j0 + c;
            int32_t v = AL_INF;
            uint32_t sub = 0;
            if (j == 0) {
                v = i;
            } else if (j > 0 && j <= n) {
                uint32_t g = J.t_off + (uint32_t)(j - 1);
                if (circular && g >= J.t_rlen) g -= J.t_rlen;  // (t_off <= t_rlen and j - 1 < t_rlen: once is enough)
                if ((g >> 4) != curw) {
                    curw = g >> 4;
                    word = tw[curw];
                }
                sub = al_code(word, g) != qc ? 1u : 0u;
                v = min(pc + (int32_t)sub, pn + 1);
            }
            run = min(min(v, run + 1), AL_INF);
            X[c * 64 + lane] = (int32_t)((uint32_t)run | (sub << 31));
            pc = pn;
        }
        // what reaches a lane from the lanes below it: E[l] = min over l' <= l of (last cell of l') + (l - l') C
        int32_t E = run;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int32_t t = __shfl_up(E, d, 64);
            if (lane >= d) E = min(E, t + d * C);
        }
        int32_t carry = __shfl_up(E, 1, 64);
        if (lane == 0) carry = AL_INF;
        carry = min(carry, AL_INF);
        uint8_t* const row = tb + J.tb_off + (uint64_t)(i - 1) * (uint64_t)(16 * C);
        pc = p0;
        uint32_t bits = 0;
        for (int c = 0; c < C; c++) {
            const uint32_t xv = (uint32_t)X[c * 64 + lane];
            const int32_t sub = (int32_t)(xv >> 31);
            const int32_t pn = c + 1 < C ? P[(c + 1) * 64 + lane] : pnext;
            const int j = j0 + c;
            int32_t D = min((int32_t)(xv & 0x7fffffffu), carry + c + 1);
            if (j < 0 || j > n) D = AL_INF;
            // rule 7 at this cell: M before I before D
            const uint32_t dir = (j >= 1 && pc + sub == D) ? 0u : (pn + 1 == D ? 1u : 2u);
            P[c * 64 + lane] = D;
            bits |= dir << ((c & 3) << 1);
            if ((c & 3) == 3) {
                row[(c >> 2) * 64 + lane] = (uint8_t)bits;
                bits = 0;
            }
            pc = pn;
        }
    }
    const int be = n - m - J.dlo;  // the end cell's diagonal
    if (be / C == lane) nm_out[blockIdx.x] = P[(be % C) * 64 + lane];
}

// One thread per pair: the walk of rule 7 from (m, n), runs written last first and then turned round.  At most m + n steps.
__global__ void align_trace_kernel(const AlJob* __restrict__ jobs, const AlTrace* __restrict__ sel, const uint32_t n_sel, const uint8_t* __restrict__ tb,
                                   uint32_t* __restrict__ runs, uint32_t* __restrict__ n_runs, uint32_t* __restrict__ err) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_sel) return;
    const AlTrace S = sel[t];
    const AlJob J = jobs[S.job];
    const int C = (int)J.C;
    uint32_t* const out = runs + S.run_off;
    int i = (int)J.m, j = (int)J.n;
    uint32_t k = 0, cur = 3, len = 0;
    bool bad = false;
    const uint32_t steps = J.m + J.n;
    for (uint32_t s = 0; s < steps && (i > 0 || j > 0); s++) {
        uint32_t op;
        if (i == 0) {
            op = 2;
        } else if (j == 0) {
            op = 1;
        } else {
            const int b = j - i - J.dlo;
            if (b < 0 || b >= 64 * C) {
                bad = true;
                break;
            }
            const int c = b % C, l = b / C;
            op = ((uint32_t)tb[J.tb_off + (uint64_t)(i - 1) * (uint64_t)(16 * C) + (uint64_t)((c >> 2) * 64 + l)] >> ((c & 3) << 1)) & 3u;
        }
        if (op == cur) {
            len++;
        } else {
            if (len) {
                if (k < S.cap) out[k] = len << 2 | cur;
                k++;
            }
            cur = op;
            len = 1;
        }
        if (op == 0) i--, j--;
        else if (op == 1) i--;
        else j--;
    }
    if (len) {
        if (k < S.cap) out[k] = len << 2 | cur;
        k++;
    }
    if (bad || k > S.cap || i != 0 || j != 0) {
        atomicOr(err, 1u);
        n_runs[t] = 0;
        return;
    }
    for (uint32_t a = 0, b = k - 1; a < b; a++, b--) {
        const uint32_t x = out[a];
        out[a] = out[b];
        out[b] = x;
    }
    n_runs[t] = k;
}

uint32_t al_cells_per_lane(uint32_t m, uint32_t n, uint32_t w, int32_t* dlo) {
    const int64_t delta = (int64_t)n - (int64_t)m;
    const int64_t lo = std::max<int64_t>(std::min<int64_t>(0, delta) - w, -(int64_t)m), hi = std::min<int64_t>(std::max<int64_t>(0, delta) + w, n);
    *dlo = (int32_t)lo;
    const uint32_t W = (uint32_t)(hi - lo + 1);
    return ((W + 63) / 64 + 3) & ~3u;  // a multiple of 4: four cells' moves make a byte of the trace-back
}

struct AlBufs {  // a group's device blocks, given back on every way out
    void* p[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    ~AlBufs() {
        for (void* q : p)
            if (q) dp_dev_free(q);
    }
};

}  // namespace

struct AlignState {
    std::vector<dp_align_rec> recs;
    std::vector<uint32_t> runs;
    hipEvent_t ev[2] = {nullptr, nullptr};
};

void dp_align_state_free(dp_ctx* ctx) {
    if (!ctx->align_state) return;
    for (hipEvent_t e : ctx->align_state->ev)
        if (e) hipEventDestroy(e);
    delete ctx->align_state;
    ctx->align_state = nullptr;
}

extern "C" int dp_align_spans(dp_ctx* ctx, const dp_align_item* items, uint32_t n, uint32_t max_edits, int circular, dp_align_batch* out) {
    if (!ctx) return DP_ERR_ARG;
    if (!out || (n && !items)) return dp_fail(ctx, DP_ERR_ARG, "dp_align_spans: bad arguments");
    if (max_edits < 1 || max_edits > AL_MAX_EDITS) return dp_fail(ctx, DP_ERR_ARG, "dp_align_spans: max_edits outside 1 .. 32768");
    if (int rc = dp_reads_stale(ctx, "dp_align_spans")) return rc;
    {
        std::lock_guard<std::mutex> lk(ctx->upload_mu);
        if (ctx->upload) return dp_fail(ctx, DP_ERR_STATE, "dp_align_spans: an upload of dp_reads_upload_rc_begin is pending on the context");
    }
    for (uint32_t x = 0; x < n; x++) {
        const dp_align_item& it = items[x];
        bool ok = it.q_read < ctx->n_reads && it.t_read < ctx->n_reads && it.q_len >= 1 && it.t_len >= 1 && it.q_len <= AL_MAX_SPAN && it.t_len <= AL_MAX_SPAN;
        if (ok) {
            const uint64_t ql = ctx->h_len[it.q_read], tl = ctx->h_len[it.t_read];
            ok = (uint64_t)it.q_off + it.q_len <= ql && (circular ? (it.t_off <= tl && it.t_len <= tl) : (uint64_t)it.t_off + it.t_len <= tl);
        }
        if (!ok) {
            const std::string msg = "dp_align_spans: item " + std::to_string(x) + " lies outside its reads or the span limit of 2^20 bases";
            return dp_fail(ctx, DP_ERR_ARG, msg.c_str());
        }
    }
    hipSetDevice(ctx->device);
    if (!ctx->align_state) {
        ctx->align_state = new AlignState();
        for (hipEvent_t& e : ctx->align_state->ev) DP_HIP(hipEventCreate(&e));
    }
    AlignState& S = *ctx->align_state;
    S.recs.assign(n, dp_align_rec{-1, 0u, 0ull});
    S.runs.clear();
    memset(out, 0, sizeof *out);
    out->n = n;

    // the attempts still to make: (item, half width).  A pair whose lengths alone differ by more than the cap is over it without a cell.
    std::vector<std::pair<uint32_t, uint32_t>> pending, next;
    for (uint32_t x = 0; x < n; x++) {
        const int64_t delta = (int64_t)items[x].t_len - (int64_t)items[x].q_len;
        if (std::llabs(delta) <= (int64_t)max_edits) pending.emplace_back(x, AL_W0);
    }
    size_t freeB = 0, totalB = 0;
    DP_HIP(hipMemGetInfo(&freeB, &totalB));
    const uint64_t budget = std::min<uint64_t>((uint64_t)(freeB + dp_dev_cached_bytes()) / 2, (uint64_t)16 << 30);

    std::vector<AlJob> jobs;
    std::vector<uint32_t> width;  // the half width of jobs[x]
    std::vector<int32_t> nm;
    std::vector<AlTrace> sel;
    std::vector<uint32_t> nruns, gruns;
    double kernel_ms = 0;
    while (!pending.empty()) {
        // ---- a group: attempts in order until the trace-back and row scratch reach the budget (one attempt always goes)
        jobs.clear();
        width.clear();
        uint64_t tbBytes = 0, rowInts = 0;
        size_t taken = 0;
        for (; taken < pending.size(); taken++) {
            const dp_align_item& it = items[pending[taken].first];
            AlJob J;
            J.C = al_cells_per_lane(it.q_len, it.t_len, pending[taken].second, &J.dlo);
            const uint64_t tbNeed = (uint64_t)16 * J.C * it.q_len, rowNeed = J.C > AL_LDS_MAX_C ? (uint64_t)128 * J.C : 0;
            if (taken && tbBytes + tbNeed + 4 * (rowInts + rowNeed) > budget) break;
            J.q_byte = ctx->h_boff[it.q_read];
            J.t_byte = ctx->h_boff[it.t_read];
            J.tb_off = tbBytes;
            J.row_off = rowInts;
            J.q_off = it.q_off;
            J.t_off = it.t_off;
            J.t_rlen = ctx->h_len[it.t_read];
            J.m = it.q_len;
            J.n = it.t_len;
            J.item = pending[taken].first;
            tbBytes += tbNeed;
            rowInts += rowNeed;
            jobs.push_back(J);
            width.push_back(pending[taken].second);
            out->cells += (uint64_t)64 * J.C * it.q_len;
        }
        next.assign(pending.begin() + (int64_t)taken, pending.end());
        out->tb_bytes += tbBytes;
        // the jobs by class of C (a launch's LDS is sized for its class): 4, 8, 16, 32, 64, 128, then the device-memory tier
        std::vector<uint32_t> order(jobs.size());
        for (uint32_t x = 0; x < order.size(); x++) order[x] = x;
        auto klass = [](uint32_t C) {
            int k = 0;
            for (uint32_t cap = 4; cap < C && k < 6; cap <<= 1) k++;
            return C > AL_LDS_MAX_C ? 6 : k;
        };
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return klass(jobs[a].C) < klass(jobs[b].C); });
        {
            std::vector<AlJob> sj(jobs.size());
            std::vector<uint32_t> sw(jobs.size());
            for (size_t x = 0; x < order.size(); x++) sj[x] = jobs[order[x]], sw[x] = width[order[x]];
            jobs.swap(sj);
            width.swap(sw);
        }
        const uint32_t nJ = (uint32_t)jobs.size();
        AlBufs B;  // 0 trace-back, 1 jobs, 2 nm, 3 row scratch, 4 trace list + run counts + error word, 5 runs
        DP_HIP(dp_dev_malloc(&B.p[0], std::max<uint64_t>(tbBytes, 64)));
        DP_HIP(dp_dev_malloc(&B.p[1], (size_t)nJ * sizeof(AlJob)));
        DP_HIP(dp_dev_malloc(&B.p[2], (size_t)nJ * 4));
        if (rowInts) DP_HIP(dp_dev_malloc(&B.p[3], rowInts * 4));
        DP_HIP(hipMemcpyAsync(B.p[1], jobs.data(), (size_t)nJ * sizeof(AlJob), hipMemcpyHostToDevice, ctx->stream));
        DP_HIP(hipEventRecord(S.ev[0], ctx->stream));
        for (uint32_t a = 0; a < nJ;) {
            uint32_t b = a;
            const int kl = klass(jobs[a].C);
            while (b < nJ && klass(jobs[b].C) == kl) b++;
            if (kl < 6) {
                const size_t lds = (size_t)512 * ((size_t)4 << kl);
                hipLaunchKernelGGL(align_forward_kernel<true>, dim3(b - a), dim3(64), lds, ctx->stream, (const uint8_t*)ctx->d_packed.p, (const AlJob*)B.p[1] + a,
                                   circular ? 1 : 0, (uint8_t*)B.p[0], (int32_t*)nullptr, (int32_t*)B.p[2] + a);
            } else {
                hipLaunchKernelGGL(align_forward_kernel<false>, dim3(b - a), dim3(64), 0, ctx->stream, (const uint8_t*)ctx->d_packed.p, (const AlJob*)B.p[1] + a,
                                   circular ? 1 : 0, (uint8_t*)B.p[0], (int32_t*)B.p[3], (int32_t*)B.p[2] + a);
            }
            DP_HIP(hipGetLastError());
            a = b;
        }
        DP_HIP(hipEventRecord(S.ev[1], ctx->stream));
        nm.resize(nJ);
        DP_HIP(hipMemcpyAsync(nm.data(), B.p[2], (size_t)nJ * 4, hipMemcpyDeviceToHost, ctx->stream));
        DP_HIP(dp_stream_sync(ctx));
        float ms = 0;
        if (hipEventElapsedTime(&ms, S.ev[0], S.ev[1]) == hipSuccess) kernel_ms += ms;
        // ---- what each attempt proved
        sel.clear();
        uint64_t runCap = 0;
        for (uint32_t x = 0; x < nJ; x++) {
            const AlJob& J = jobs[x];
            const int64_t lim = std::llabs((int64_t)J.n - (int64_t)J.m) + 2 * (int64_t)width[x], s = nm[x];
            if (s <= lim) {  // every optimal path lies inside the band: s is NM
                if (s > (int64_t)max_edits) continue;
                S.recs[J.item].nm = (int32_t)s;
                sel.push_back(AlTrace{x, (uint32_t)(2 * s + 1), runCap});  // (gap runs hold an edit each, M runs lie between them)
                runCap += (uint64_t)(2 * s + 1);
            } else if (lim < (int64_t)max_edits) {
                next.emplace_back(J.item, width[x] * 2);
                out->doublings++;
            }  // else NM > |m - n| + 2 w >= max_edits: over the cap
        }
        if (!sel.empty()) {
            const uint32_t nS = (uint32_t)sel.size();
            const size_t selBytes = (size_t)nS * sizeof(AlTrace), cntAt = (selBytes + 15) & ~(size_t)15;
            DP_HIP(dp_dev_malloc(&B.p[4], cntAt + (size_t)nS * 4 + 16));
            DP_HIP(dp_dev_malloc(&B.p[5], runCap * 4));
            uint32_t* const d_cnt = (uint32_t*)((uint8_t*)B.p[4] + cntAt);
            DP_HIP(hipMemcpyAsync(B.p[4], sel.data(), selBytes, hipMemcpyHostToDevice, ctx->stream));
            DP_HIP(hipMemsetAsync(d_cnt + nS, 0, 4, ctx->stream));
            DP_HIP(hipEventRecord(S.ev[0], ctx->stream));
            hipLaunchKernelGGL(align_trace_kernel, dim3((nS + 63) / 64), dim3(64), 0, ctx->stream, (const AlJob*)B.p[1], (const AlTrace*)B.p[4], nS,
                               (const uint8_t*)B.p[0], (uint32_t*)B.p[5], d_cnt, d_cnt + nS);
            DP_HIP(hipGetLastError());
            DP_HIP(hipEventRecord(S.ev[1], ctx->stream));
            nruns.resize((size_t)nS + 1);
            gruns.resize(runCap);
            DP_HIP(hipMemcpyAsync(nruns.data(), d_cnt, ((size_t)nS + 1) * 4, hipMemcpyDeviceToHost, ctx->stream));
            DP_HIP(hipMemcpyAsync(gruns.data(), B.p[5], runCap * 4, hipMemcpyDeviceToHost, ctx->stream));
            DP_HIP(dp_stream_sync(ctx));
            if (hipEventElapsedTime(&ms, S.ev[0], S.ev[1]) == hipSuccess) kernel_ms += ms;
            if (nruns[nS]) return dp_fail(ctx, DP_ERR_HIP, "dp_align_spans: the trace-back left its band (device state inconsistent)");
            for (uint32_t t = 0; t < nS; t++) {
                dp_align_rec& r = S.recs[jobs[sel[t].job].item];
                r.n_runs = nruns[t];
                r.run_off = S.runs.size();
                S.runs.insert(S.runs.end(), gruns.begin() + (int64_t)sel[t].run_off, gruns.begin() + (int64_t)(sel[t].run_off + nruns[t]));
            }
        }
        pending.swap(next);
    }
    out->recs = S.recs.data();
    out->runs = S.runs.data();
    out->n_runs = S.runs.size();
    out->kernel_ms = kernel_ms;
    return DP_OK;
}
