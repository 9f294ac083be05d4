// Every run-time setting of the two libraries and the CLI: one table and the only getenv() of the source tree.
// (plain C++17, header only: libdownpore_hip.so and libdownpore_host.so each carry their own copy of the small cache below, which
// parses DP_TUNE / DP_DEBUG again whenever the variable's text has changed)
//
// When a setting is read - the table's third column, and the only three answers there are:
//   CALL     by the call that uses it, every time: tests and experiments switch these between two calls of one process
//   CREATE   once, when the object that uses it is created - the dp_ctx, the overlap or map job, the planner - and kept in that
//            object: the ones consulted many times per round.  A change takes effect with the next context / job
//   PROCESS  once per process, where a process-wide pool is first sized or a process-wide hook is installed
// No setting lives in a function-local static except the PROCESS ones.  Asking for a name that is not in the table aborts.
#pragma once
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <set>
#include <string>

namespace dp_env {
enum Kind { VAR, TUNE, DEBUG };
enum When { CALL, CREATE, PROCESS };
struct Setting {
    Kind kind;
    const char* name;
    When when;
    const char* meaning;
};
inline constexpr Setting kSettings[] = {
    // ---- variables of their own
    {VAR, "DP_TUNE", CALL, "key=value,...: the keys below"},
    {VAR, "DP_DEBUG", CALL, "a,b,...: the tokens below"},
    {VAR, "DP_SCAN_INDEX", CALL, "0/1: forbid / force the resident k-mer position index (default: from 1 Gbase up)"},
    {VAR, "DP_KINDEX_SHARD", CALL, "0/1/force: index built in shares over the communicator never / also over RCCL / also with one rank"},
    {VAR, "DP_KINDEX_WIDE", CALL, "set: index entries of eight bytes throughout"},
    {VAR, "DP_KINDEX_MAX_K", CALL, "n: no index above k = n (at most 14)"},
    {VAR, "DP_KB_MIN_PBITS", CALL, "n: a floor for the index's position bits, at most 32 (tests reach every entry format on small inputs)"},
    {VAR, "DP_KX_BINS_CAP", CALL, "n: capacity of a bin, at least 16 (tests: bins that overflow)"},
    {VAR, "DP_KX_ONESHOT", CALL, "0: count, wait, fill instead of the index step in one go"},
    {VAR, "DP_KX_DENSE", CALL, "0/1: the dense regime's kernels never / always"},
    {VAR, "DP_INDEX_FILL_ROWS", CALL, "0/1: bit matrices by atomics / seed-set rows in LDS + transpose (default: by size)"},
    {VAR, "DP_CHAIN_PASSES", CALL, "n: proposal passes of the chaining stage, 0..6 (default 3; 0 = the serial walk alone)"},
    {VAR, "DP_CHAIN_TIER", CALL, "2/3: the LDS / the one-lane tier for every pair (tests)"},
    {VAR, "DP_CHAIN_PERFECT", CALL, "0: no perfect-chain shortcut"},
    {VAR, "DP_CHAIN_PACK", CALL, "1: chains always packed for a host consumer"},
    {VAR, "DP_CONS_LAYOUTS", CALL, "words nosmall,eager,huge,nohuge: which LDS layouts of the consensus kernel run when (tests)"},
    {VAR, "DP_TRIM_MIDDLE", CALL, "set and not 0: CLI trim and overlap -trim run the middle stage"},
    {VAR, "DP_TRIM_MID_REC_CAP", CALL, "n: first capacity of dp_trim_search's record buffer, at least 1 (tests: the repeat on overflow)"},
    {VAR, "DP_DEVICE_CONSENSUS", CALL, "0: BuildConsensus on the host; 1: where the host builds it, its seed-space alignment on the device"},
    {VAR, "DP_DEVICE_CHUNK", CALL, "0: chunkWorker on the host"},
    {VAR, "DPH_PRECHAIN", CALL, "0/1: the chunk stage behind the un-waited scan never / always (default: up to three slots)"},
    {VAR, "DP_WINDOW_CACHE", CREATE, "0: per-plan dp_select_seeds calls instead of the window cache"},
    {VAR, "DP_EXEC_SLOTS", CREATE, "n: executor slots of the CLI's overlap job (default 8)"},
    {VAR, "DP_HOST_THREADS", PROCESS, "n: size of the worker pool = the CPU budget everything else is derived from (default: cgroup quota)"},
    {VAR, "DPH_PLAN_LANES", CREATE, "n: planner lanes, 1..8, and no adaptive growth"},
    {VAR, "DPH_TEXT_THREADS", CREATE, "n: formatter threads, 1..16"},
    {VAR, "DP_MAP_THREADS", CREATE, "n: host threads a map job deals its reads to"},
    {VAR, "DP_MAP_INFLIGHT", CREATE, "n: reads each of them keeps in flight, at least 64"},
    {VAR, "DP_MAP_SHARDS", CREATE, "n: reference index of a map job in n shards"},
    {VAR, "DP_MAP_DEVICES", CREATE, "a,b,...: the devices that hold them"},
    {VAR, "DP_DEV_CACHE_MB", PROCESS, "n: device bytes that may stay parked after the context that owned the reads (default 16384)"},
    {VAR, "DP_PIN_CACHE_MB", PROCESS, "n: pinned host bytes that may stay parked (default 2048)"},
    {VAR, "DP_KERNEL_TIMING", PROCESS, "n: timing events around every n-th round of a context (default 8, 0 = never); the initial value dp_set_kernel_timing overrides"},
    {VAR, "DP_SPIN_SYNC", CREATE, "0/1: host threads poll / busy-wait for their context's stream (default: dp_set_stream_wait)"},
    {VAR, "DPH_PROFILE", CREATE, "set: host pipeline counters and set-up marks on stderr"},
    // ---- DP_TUNE keys: numbers that experiments vary
    {TUNE, "spec_blocks", CALL, "workgroups of the chaining stage's proposal passes (default 1024)"},
    {TUNE, "scan_wg_per_cu", CALL, "persistent scan workgroups per CU, 1..2 (default 2)"},
    {TUNE, "query_split", CALL, "workgroups per query of the query kernel, up to 16 (default 0 = one, which also clears its own rows)"},
    {TUNE, "upload_threads", PROCESS, "helper threads of the shared pinned upload ring, 0..16 (default 4)"},
    {TUNE, "sync_poll_us", CREATE, "sleep between two polls of a waiting host thread (default 20; 0 = blocking wait)"},
    {TUNE, "kb_b1", CALL, "first-digit bits of the sorted index build, 6..10"},
    {TUNE, "plan_depth", CREATE, "plans computed beyond the highest round asked for, at least 1 (default 6)"},
    {TUNE, "issue_window", CREATE, "rounds issued beyond the slots' own, at least 0 (default 10)"},
    {TUNE, "text_pool_mb", PROCESS, "cap of the process-wide pool of PAF text strings (default 512)"},
    {TUNE, "pin_workers", PROCESS, "1/2: pool workers pinned one per physical core / within NUMA node 0"},
    {TUNE, "map_min_reads_per_thread", CREATE, "reads below which a map job starts no further thread (default 2048)"},
    {TUNE, "map_async_upload", CREATE, "1: a map job's reads travel while the first ones are mapped"},
    {TUNE, "map_ascii_upload", CREATE, "1: the mapper sends its reads as ASCII and the device packs them"},
    // ---- DP_TUNE keys: test hooks
    {TUNE, "kindex_atomic", CALL, "1: the count -> offsets -> atomic scatter build of the position index"},
    {TUNE, "map_one_lane", CALL, "1: dynamicMatch on one lane"},
    {TUNE, "map_seeds_host", CREATE, "1: AddSingleSeeds walked on the host"},
    {TUNE, "pack_scalar", CREATE, "1: the host's packer without its AVX2 path"},
    {TUNE, "host_values", CREATE, "1: k-mer histogram on the GPU, value table on the host"},
    {TUNE, "host_select", CREATE, "1: the speculative seed selection on host threads"},
    {TUNE, "no_planner_thread", CREATE, "1: plans computed on the calling thread"},
    {TUNE, "no_query_prestage", CALL, "1: dp_find_overlaps uploads the queries itself"},
    {TUNE, "no_shard_queries", CALL, "1: every rank of a scan-shard job does every query window"},
    {TUNE, "touch_isa", PROCESS, "0/1/2: the touch test in scalar / AVX2 / AVX-512 code (only what the CPU has), chosen at its first use"},
    {TUNE, "cons_flag_every", CALL, "n: every n-th window of the device consensus goes to the host path"},
    {TUNE, "plan_delay_us", CREATE, "sleep after every plan: flags arrive after the plan has read them"},
    {TUNE, "fail_begin_rank", CALL, "r: rank r's round fails before it reaches any exchange"},
    {TUNE, "comm_fail_rank", CALL, "r: rank r fails before it meets its peers"},
    {TUNE, "query_debug", CALL, "debug bits handed to the query kernel"},
    {TUNE, "scan_debug", CALL, "debug bits handed to the scan kernels"},
    // ---- DP_DEBUG tokens: diagnosis output, no change of behaviour
    {DEBUG, "alloc", CALL, "one line per growth of a buffer (read where a buffer grows, not per round)"},
    {DEBUG, "kx_bins", CREATE, "how full the index step's bins are (waits for the stream)"},
    {DEBUG, "kx_oneshot", CREATE, "every one-go index step that had to be repeated"},
    {DEBUG, "cons", CREATE, "per-window records of the consensus kernel"},
    {DEBUG, "cons_why", CREATE, "why a window was left to the host path"},
    {DEBUG, "chain_prof", CREATE, "the chaining stage's per-wave phase timers (make PROF=1)"},
    {DEBUG, "chain_paths", CALL, "the chaining stage records which kernel and which path made every pair final (tests: dp_debug_chain_paths)"},
    {DEBUG, "map_prof", CREATE, "the map kernel's phase timers (make PROF=1)"},
    {DEBUG, "planner", CREATE, "plans as they are computed and fetched"},
    {DEBUG, "start", CREATE, "a job's first twelve rounds, in ms since the end of its set-up"},
    {DEBUG, "slow", CREATE, "every round that took its slot more than 3 ms, with where the time went"},
    {DEBUG, "exchange", CREATE, "the slots' turns at a scan-shard job's exchanges"},
    {DEBUG, "segv", PROCESS, "a crashing host thread prints its frames (handlers installed when the library is loaded)"},
    {DEBUG, "sample_prof", PROCESS, "wall-clock sampling of the pipeline's threads (installed when the library is loaded)"},
};

inline bool known(Kind kind, const char* name) {
    for (const Setting& s : kSettings)
        if (s.kind == kind && strcmp(s.name, name) == 0) return true;
    return false;
}
inline void require(Kind kind, const char* name) {  // a name the table does not have is a mistake in the code, not in the environment
    if (known(kind, name)) return;
    fprintf(stderr, "dp_env: \"%s\" is not in the table of settings (dp_env.h)\n", name);
    abort();
}

// DP_TUNE / DP_DEBUG: "a,b=3,,c=" -> a = "1", b = "3", c = "" (empty tokens dropped); keys the table does not have are named
// in one line on stderr, once per distinct text of the variable
struct Tokens {
    Tokens(const char* v, Kind k) : var(v), kind(k) {}
    const char* const var;
    const Kind kind;
    std::mutex mu;
    std::string text;
    bool parsed = false;
    std::map<std::string, std::string> m;
    std::set<std::string> warned;
    const std::map<std::string, std::string>& get() {  // (call with mu held)
        const char* e = getenv(var);
        if (!e) e = "";
        if (parsed && text == e) return m;
        text = e;
        parsed = true;
        m.clear();
        std::string unknown;
        for (size_t at = 0; at <= text.size();) {
            size_t end = text.find(',', at);
            if (end == std::string::npos) end = text.size();
            const std::string tok = text.substr(at, end - at);
            const size_t eq = tok.find('=');
            const std::string key = tok.substr(0, eq);
            at = end + 1;
            if (tok.empty()) continue;
            m[key] = eq == std::string::npos ? "1" : tok.substr(eq + 1);
            if (!known(kind, key.c_str())) unknown += (unknown.empty() ? "" : ", ") + key;
        }
        if (!unknown.empty() && warned.insert(text).second) fprintf(stderr, "%s: unknown (ignored): %s\n", var, unknown.c_str());
        return m;
    }
};
}  // namespace dp_env

// a variable's text, or null when it is not set
inline const char* dp_env_str(const char* name) {
    dp_env::require(dp_env::VAR, name);
    return getenv(name);
}
// a number: dflt as it is when the variable is not set, else its value brought into [lo, hi]
inline long dp_env_long(const char* name, long dflt, long lo = LONG_MIN, long hi = LONG_MAX) {
    const char* e = dp_env_str(name);
    return e ? (atol(e) < lo ? lo : atol(e) > hi ? hi : atol(e)) : dflt;
}
// the 0/1 switches: -1 not set, 0 / 1 the text starts with that digit, 2 any other text (which the call sites treat as they
// always have: "off unless 1" where 1 forces something, "on unless 0" where 0 forbids it)
inline int dp_env_tristate(const char* name) {
    const char* e = dp_env_str(name);
    return !e ? -1 : e[0] == '0' ? 0 : e[0] == '1' ? 1 : 2;
}
// is `word` one of the comma-separated words of the variable?
inline bool dp_env_has_word(const char* name, const char* word) {
    const char* e = dp_env_str(name);
    const size_t n = strlen(word);
    for (const char* p = e; p && *p;) {
        const char* end = strchr(p, ',');
        const size_t len = end ? (size_t)(end - p) : strlen(p);
        if (len == n && memcmp(p, word, n) == 0) return true;
        p += len + (end ? 1 : 0);
    }
    return false;
}
// DP_DEBUG=a,b,c: diagnosis output of the named parts (no change of behaviour)
inline bool dp_debug(const char* what) {
    dp_env::require(dp_env::DEBUG, what);
    static dp_env::Tokens t("DP_DEBUG", dp_env::DEBUG);
    std::lock_guard<std::mutex> lk(t.mu);
    return t.get().count(what) != 0;
}
// DP_TUNE=key=value,...: the numbers experiments vary and the hooks tests use (the defaults are what the measurements chose)
inline long dp_tune(const char* key, long dflt) {
    dp_env::require(dp_env::TUNE, key);
    static dp_env::Tokens t("DP_TUNE", dp_env::TUNE);
    std::lock_guard<std::mutex> lk(t.mu);
    const auto& m = t.get();
    const auto it = m.find(key);
    return it == m.end() ? dflt : atol(it->second.c_str());
}

// ---- the settings several call sites share
inline bool dp_device_consensus_on() { return dp_env_tristate("DP_DEVICE_CONSENSUS") != 0; }  // DP_DEVICE_CONSENSUS=0: on the host
inline bool dp_profile_on() { return dp_env_str("DPH_PROFILE") != nullptr; }
struct dp_wait_mode {    // how a host thread waits for its context's stream (dp_stream_sync, kx_wait_done)
    int spin = -1;       // DP_SPIN_SYNC: 1 busy-wait, 0 poll, -1 what dp_set_stream_wait chose
    long poll_ns = 0;    // DP_TUNE=sync_poll_us, in ns
};
inline dp_wait_mode dp_wait_mode_read() {
    const int t = dp_env_tristate("DP_SPIN_SYNC");
    return dp_wait_mode{t < 0 ? -1 : t == 1 ? 1 : 0, dp_tune("sync_poll_us", 20) * 1000L};
}
