// `downpore` command-line front end of the product: same commands, flag names, defaults, aliases, stderr lines and
// PAF columns as the reference for the path in scope (downpore.go:34-92; commands/overlap.go:22-29; commands/map.go:17-22;
// commands/trim.go:16-50).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>

#include "host_util.hpp"

using namespace dph;

static bool parseBool(const std::string& a) { return a == "1" || (!a.empty() && (a[0] == 'T' || a[0] == 't')); }
static i64 parseInt(const std::string& a, bool& ok) {
    char* e = nullptr;
    long long v = strtoll(a.c_str(), &e, 10);
    if (a.empty() || *e) {
        fprintf(stderr, "Invalid integer argument value:%s\n", a.c_str());
        ok = false;
    }
    return v;
}

static void printLog(const std::string& text);
static bool trimMiddleFromEnv() {  // the middle stage is in force with DP_TRIM_MIDDLE=1
    const char* midEnv = dp_env_str("DP_TRIM_MIDDLE");
    return midEnv && midEnv[0] && strcmp(midEnv, "0") != 0;
}
static const char* const kNoMiddleNotice =
    "downpore trim: the search for adapters in the middle of reads is not part of this build; reads are end-trimmed only\n";
static const char* const kNoAdapterLists =
    "downpore trim: -front_adapters and -back_adapters are required (the adapter lists are not shipped with this build)\n";

static int runOverlap(ArgTable& t) {
    bool ok = true;
    OverlapParams p;
    p.overlapSize = parseInt(t.args["overlap_size"], ok);
    p.numSeeds = (int)parseInt(t.args["num_seeds"], ok);
    p.seedBatchSize = parseInt(t.args["seed_batch_size"], ok);
    p.queryBatchSize = parseInt(t.args["query_batch_size"], ok);
    p.chunkSize = parseInt(t.args["chunk_size"], ok);
    p.numWorkers = (int)parseInt(t.args["num_workers"], ok);
    p.k = (int)parseInt(t.args["k"], ok);
    p.minHits = atof(t.args["min_hits"].c_str());
    p.himem = parseBool(t.args["himem"]);
    if (!ok) return 1;
    if (!t.args["seed_values"].empty()) {
        fprintf(stderr, "seed_values files are not supported by this build (out of scope, SURVEY #16)\n");
        return 1;
    }
    // -trim true: `downpore trim` with its default flags in front, on the reads the device holds anyway, instead of through a file
    const bool trim = parseBool(t.args["trim"]);
    TrimParams tp;
    if (trim) {
        if (t.args["front_adapters"].empty() || t.args["back_adapters"].empty()) {
            fputs(kNoAdapterLists, stderr);
            return 1;
        }
        tp.middle = trimMiddleFromEnv();
        if (!tp.middle) fputs(kNoMiddleNotice, stderr);
    }
    ReadSet reads, raw, front, back;
    std::string err;
    const bool prof = dp_profile_on();
    double tm = now();
    auto mark = [&](const char* what) {
        if (!prof) return;
        const double tn = now();
        fprintf(stderr, "[cli] %-24s %.1f ms\n", what, 1e3 * (tn - tm));
        tm = tn;
    };
    if (trim ? !ReadSet::fromFile(t.args["front_adapters"], 0, false, front, err) || !ReadSet::fromFile(t.args["back_adapters"], 0, false, back, err) ||
                   !ReadSet::fromFile(t.args["input"], 50, p.himem, raw, err)
             : !ReadSet::fromFile(t.args["input"], p.overlapSize, p.himem, reads, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 1;
    }
    mark("read input");
    dp_ctx* ctx = nullptr;
    if (dp_ctx_create(0, &ctx) != 0) {
        fprintf(stderr, "downpore: %s\n", dp_last_error(nullptr));
        return 2;
    }
    const ReadSet& up = trim ? raw : reads;
    int rc = dp_reads_upload(ctx, (const uint8_t*)up.bases.data(), up.off.data(), (uint32_t)up.size());
    if (trim && rc == 0) {
        mark("upload + pack");
        TrimResult res;
        std::string error;
        const int trc = runTrim(raw, front, back, tp, 0, res, error, ctx);
        printLog(res.errText);
        if (trc != 0) {
            fprintf(stderr, "downpore: %s\n", error.c_str());
            return 2;
        }
        mark("trim (resident reads)");
        std::vector<dp_read_span> spans;
        trimmedReadSet(raw, res, p.overlapSize, p.himem, reads, spans);
        raw = ReadSet();
        mark("trimmed read set");
        rc = dp_reads_respan(ctx, spans.data(), (uint32_t)spans.size());
        mark("respan");
    }
    OverlapRun run;
    if (rc == 0) rc = run.init(ctx, &reads, p, nullptr, (int)dp_env_long("DP_EXEC_SLOTS", 8));
    if (rc != 0) {
        fprintf(stderr, "downpore: %s\n", run.error.empty() ? dp_last_error(ctx) : run.error.c_str());
        return 2;
    }
    mark("set-up (device)");
    size_t shown = 0;
    for (;;) {
        rc = run.step();
        if (rc == 0) break;
        if (rc < 0) {
            fprintf(stderr, "downpore: %s\n", run.error.c_str());
            return 2;
        }
        fwrite(run.paf.data(), 1, run.paf.size(), stdout);
        fwrite(run.errText.data() + shown, 1, run.errText.size() - shown, stderr);
        shown = run.errText.size();
    }
    fwrite(run.errText.data() + shown, 1, run.errText.size() - shown, stderr);
    mark("rounds + output");
    fprintf(stderr, "[downpore_amd] rounds=%lld bad_back_suppressed=%lld empty_match_panics_avoided=%lld\n", (long long)run.round,
            (long long)run.badBack, (long long)run.emptyMatch);
    run.shutdown();
    dp_ctx_destroy(ctx);
    return 0;
}

// log.Println's default prefix ("2006/01/02 15:04:05 ") in front of every line of a run's log text
static void printLog(const std::string& text) {
    char stamp[32];
    const time_t t = time(nullptr);
    struct tm tmv;
    localtime_r(&t, &tmv);
    strftime(stamp, sizeof stamp, "%Y/%m/%d %H:%M:%S ", &tmv);
    size_t at = 0;
    while (at < text.size()) {
        size_t e = text.find('\n', at);
        if (e == std::string::npos) e = text.size();
        fprintf(stderr, "%s%.*s\n", stamp, (int)(e - at), text.data() + at);
        at = e + 1;
    }
}

static int runTrimCommand(ArgTable& t) {  // commands/trim.go:32-50
    bool ok = true;
    TrimParams p;
    p.k = (int)parseInt(t.args["k"], ok);
    p.checkReads = parseInt(t.args["check_reads"], ok);
    p.adapterThreshold = (int)parseInt(t.args["adapter_threshold"], ok);
    p.extraEdgeTrim = (int)parseInt(t.args["extra_end_trim"], ok);
    p.verbosity = (int)parseInt(t.args["verbosity"], ok);
    p.tagAdapters = parseBool(t.args["tag_adapters"]);
    p.requirePairs = parseBool(t.args["require_pairs"]);
    p.determineAdapters = parseBool(t.args["determine_adapters"]);
    // the flags of the search for adapters in the middle of reads: in force with DP_TRIM_MIDDLE=1, else parsed and accepted
    p.middle = trimMiddleFromEnv();
    p.chunkSize = parseInt(t.args["chunk_size"], ok);
    p.middleThreshold = (int)parseInt(t.args["middle_threshold"], ok);
    p.extraMiddleTrim = (int)parseInt(t.args["extra_middle_trim"], ok);
    p.discardMiddle = parseBool(t.args["discard_middle"]);
    parseInt(t.args["num_workers"], ok);  // (changes nothing in the result)
    if (!ok) return 1;
    if (p.middle && p.chunkSize <= 100) {
        fprintf(stderr, "downpore trim: -chunk_size must be larger than 100 (the chunks advance by chunk_size - 100 bases)\n");
        return 1;
    }
    if (t.args["front_adapters"].empty() || t.args["back_adapters"].empty()) {
        fputs(kNoAdapterLists, stderr);
        return 1;
    }
    if (!p.middle) fputs(kNoMiddleNotice, stderr);
    ReadSet front, back, reads;
    std::string err;
    if (!ReadSet::fromFile(t.args["front_adapters"], 0, false, front, err) || !ReadSet::fromFile(t.args["back_adapters"], 0, false, back, err) ||
        !ReadSet::fromFile(t.args["input"], 50, parseBool(t.args["himem"]), reads, err)) {
        fprintf(stderr, "%s\n", err.c_str());
        return 1;
    }
    TrimResult res;
    std::string error;
    const int rc = runTrim(reads, front, back, p, 0, res, error);
    printLog(res.errText);
    if (rc != 0) {
        fprintf(stderr, "downpore: %s\n", error.c_str());
        return 2;
    }
    if (!t.args["demultiplex"].empty()) {
        if (trimDemultiplex(reads, res, t.args["demultiplex"], error) < 0) {
            fprintf(stderr, "downpore: %s\n", error.c_str());
            return 2;
        }
    } else {
        fwrite(res.out.data(), 1, res.out.size(), stdout);
    }
    return 0;
}

int main(int argc, char** argv) {
    setenv("GPU_MAX_HW_QUEUES", "8", 0);  // one hardware queue per executor slot's stream (the runtime's default is 4)
    ArgTable ov, mp, tr;
    ov.make({"overlap_size", "k", "num_seeds", "seed_batch_size", "chunk_size", "query_batch_size", "min_hits", "num_workers",
             "input", "seed_values", "himem", "trim", "front_adapters", "back_adapters"},
            {"1000", "10", "15", "10000", "10000", "20000", "0.25", "4", "", "", "true", "false", "", ""},
            {"Size of overlap to search for in bases", "Number of bases in each seed",
             "Minimum number of seeds to generate for each overlap query", "Maximum total unique seeds to use in each query batch",
             "Size to chop long reads into for querying against, in bases",
             "Maximum number of queries per batch (if max seeds not reached)", "Minimum proportion of seeds that must match each query",
             "Number of worker threads to spawn", "Fasta/fastq input file", "File containing values to use during seed selection.",
             "Whether to cache all reads in memory", "Whether to trim adapters off the reads first, as the trim command does with its default flags",
             "Fasta/fastq file containing front adapters (with -trim)", "Fasta/fastq file containing back adapters (with -trim)"});
    mp.make({"input", "reference", "circular", "k", "query_size", "min_length", "chunk_size", "seed_rate", "num_workers", "all_sequences"},
            {"", "", "true", "11", "1000", "500", "10000", "40", "4", "false"},
            {"Fasta/fastq input file", "A fasta file containing a reference sequence to align against",
             "Whether the reference genome is circular", "Length of seeds in bases", "The number of bases to query at a time",
             "The minimum sequence size to generate queries from", "The number of bases for reference index chunks",
             "The maximum number of bases between seeds in the reference", "The number of worker process to use for mapping",
             "Whether to map against every sequence of the reference file, not only the first"});
    tr.make({"input", "k", "chunk_size", "middle_threshold", "discard_middle", "check_reads", "adapter_threshold", "extra_end_trim",
             "extra_middle_trim", "tag_adapters", "verbosity", "front_adapters", "back_adapters", "num_workers", "himem", "demultiplex",
             "require_pairs", "determine_adapters"},
            {"", "6", "5000", "85", "false", "10000", "90", "5", "100", "true", "1", "", "", "4", "false", "", "false", "true"},
            {"Fasta/fastq/gzip input file", "k-mer size to use when matching adapters", "Split long reads into chunks of this size when indexing",
             "% identity for matching adapters that split reads", "Whether to keep halves of split reads",
             "Number of reads to use to determine which adapters are present", "% identity required at check_adapters stage",
             "Number of bases to remove around adapters at read edges", "Number of bases to remove around read-splitting adapters",
             "Whether to add adapter names to output sequence names", "Level (0-2) of output to stderr", "Fasta/fastq file containing front adapters",
             "Fasta/fastq file containing back adapters", "Number of threads to use", "Whether to cache all reads in memory",
             "A path to demultiplex to, otherwise write sequences to stdout", "Whether front/back adapters with the same name must appear together",
             "Whether to use a fixed set of adapters or to search for those present"});
    if (argc == 1) {
        printf("Available commands:\n help <command> Describe the command and its arguments\n overlap\n map\n trim\n");
        return 0;
    }
    std::string cmd = argv[1];
    if (cmd == "help") {
        ArgTable* t = argc > 2 && !strcmp(argv[2], "overlap") ? &ov : argc > 2 && !strcmp(argv[2], "map") ? &mp : argc > 2 && !strcmp(argv[2], "trim") ? &tr : nullptr;
        if (!t) {
            printf("Usage: downpore help <command>\nTo see a list of available commands just run downpore\n");
            return 0;
        }
        for (size_t i = 0; i < t->names.size(); i++) {
            auto a = t->alias.find(t->names[i]);
            printf("-%s  %s  %s  (default:%s)\n", t->names[i].c_str(), a != t->alias.end() ? ("-" + a->second).c_str() : "",
                   t->descriptions[i].c_str(), t->defaults[i].c_str());
        }
        return 0;
    }
    std::string err;
    if (cmd == "overlap") {
        if (!ov.parse(argc, argv, err)) {
            fprintf(stderr, "%s\n", err.c_str());
            return 1;
        }
        return runOverlap(ov);
    }
    if (cmd == "map") {
        if (!mp.parse(argc, argv, err)) {
            fprintf(stderr, "%s\n", err.c_str());
            return 1;
        }
        bool ok = true;
        MapParams p;
        p.k = (int)parseInt(mp.args["k"], ok);
        p.numWorkers = (int)parseInt(mp.args["num_workers"], ok);
        p.minLength = parseInt(mp.args["min_length"], ok);
        p.circular = parseBool(mp.args["circular"]);
        p.querySize = parseInt(mp.args["query_size"], ok);
        p.chunkSize = parseInt(mp.args["chunk_size"], ok);
        p.seedRate = parseInt(mp.args["seed_rate"], ok);
        p.allSequences = parseBool(mp.args["all_sequences"]);
        if (!ok) return 1;
        ReadSet ref, reads;
        if (!ReadSet::fromFile(mp.args["reference"], 0, false, ref, err) || !ReadSet::fromFile(mp.args["input"], p.minLength, false, reads, err)) {
            fprintf(stderr, "%s\n", err.c_str());
            return 1;
        }
        std::string paf, errText, error;
        int rc = runMap(ref, reads, p, 0, paf, errText, nullptr, error);
        if (rc != 0) {
            fprintf(stderr, "downpore: %s\n", error.c_str());
            return 2;
        }
        fwrite(paf.data(), 1, paf.size(), stdout);
        fwrite(errText.data(), 1, errText.size(), stderr);
        return 0;
    }
    if (cmd == "trim") {
        if (!tr.parse(argc, argv, err)) {
            fprintf(stderr, "%s\n", err.c_str());
            return 1;
        }
        return runTrimCommand(tr);
    }
    printf("Available commands:\n help <command> Describe the command and its arguments\n");
    return 0;
}
