// Stand-alone check of downpore_amd/csrc/dp_env.h (tests/test_env_settings.py builds it plain, with ASan + UBSan and with TSan).
// `env_check` runs every case and prints "ok"; `env_check --unknown-name` asks for a name the table does not have and must die.
#include <fcntl.h>
#include <sys/wait.h>
#include <unistd.h>

#include <atomic>
#include <string>
#include <thread>

#include "dp_env.h"

#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            fprintf(stdout, "FAILED line %d: %s\n", __LINE__, #c);    \
            return 1;                                                 \
        }                                                             \
    } while (0)

// runs fn with stderr going to a file of its own and returns what it wrote
template <class F>
static std::string captured(F fn) {
    char path[] = "/tmp/env_check_XXXXXX";
    const int fd = mkstemp(path);
    fflush(stderr);
    const int saved = dup(2);
    dup2(fd, 2);
    fn();
    fflush(stderr);
    dup2(saved, 2);
    close(saved);
    std::string s;
    char buf[512];
    lseek(fd, 0, SEEK_SET);
    for (ssize_t n; (n = read(fd, buf, sizeof buf)) > 0;) s.append(buf, (size_t)n);
    close(fd);
    unlink(path);
    return s;
}
static size_t count(const std::string& s, const std::string& what) {
    size_t n = 0;
    for (size_t at = s.find(what); at != std::string::npos; at = s.find(what, at + 1)) n++;
    return n;
}

int main(int argc, char** argv) {
    if (argc > 1 && std::string(argv[1]) == "--unknown-name") return (int)dp_tune("no_such_key", 0);

    // ---- DP_TUNE / DP_DEBUG: unset, empty, and the shapes a token can have
    unsetenv("DP_TUNE");
    unsetenv("DP_DEBUG");
    CHECK(dp_tune("spec_blocks", 7) == 7);
    CHECK(!dp_debug("kx_bins"));
    setenv("DP_TUNE", "", 1);
    setenv("DP_DEBUG", "", 1);
    CHECK(dp_tune("spec_blocks", 7) == 7);
    CHECK(!dp_debug("kx_bins"));
    setenv("DP_TUNE", "host_select,spec_blocks=3,,kb_b1=", 1);  // a -> 1, b=3 -> 3, an empty token, c= -> 0
    CHECK(dp_tune("host_select", 0) == 1);
    CHECK(dp_tune("spec_blocks", 7) == 3);
    CHECK(dp_tune("kb_b1", 8) == 0);
    CHECK(dp_tune("query_split", 5) == 5);
    setenv("DP_DEBUG", "kx_bins,,cons=", 1);
    CHECK(dp_debug("kx_bins") && dp_debug("cons") && !dp_debug("alloc"));
    // ---- a value that changes between two reads
    setenv("DP_TUNE", "spec_blocks=9", 1);
    CHECK(dp_tune("spec_blocks", 7) == 9);
    CHECK(dp_tune("host_select", 0) == 0);
    unsetenv("DP_TUNE");
    CHECK(dp_tune("spec_blocks", 7) == 7);
    setenv("DP_DEBUG", "alloc", 1);
    CHECK(dp_debug("alloc") && !dp_debug("kx_bins"));

    // ---- string, long (default as it is, the variable's value clamped), tristate, word list
    unsetenv("DP_MAP_DEVICES");
    CHECK(dp_env_str("DP_MAP_DEVICES") == nullptr);
    setenv("DP_MAP_DEVICES", "0,2", 1);
    CHECK(std::string(dp_env_str("DP_MAP_DEVICES")) == "0,2");
    unsetenv("DPH_PLAN_LANES");
    CHECK(dp_env_long("DPH_PLAN_LANES", 0, 1, 8) == 0);  // (the default is not clamped)
    CHECK(dp_env_long("DPH_PLAN_LANES", 5) == 5);
    setenv("DPH_PLAN_LANES", "3", 1);
    CHECK(dp_env_long("DPH_PLAN_LANES", 0, 1, 8) == 3);
    setenv("DPH_PLAN_LANES", "40", 1);
    CHECK(dp_env_long("DPH_PLAN_LANES", 0, 1, 8) == 8);
    CHECK(dp_env_long("DPH_PLAN_LANES", 0) == 40);
    setenv("DPH_PLAN_LANES", "-2", 1);
    CHECK(dp_env_long("DPH_PLAN_LANES", 0, 1, 8) == 1);
    CHECK(dp_env_long("DPH_PLAN_LANES", 0, 1) == 1);
    CHECK(dp_env_long("DPH_PLAN_LANES", 0, LONG_MIN, 8) == -2);
    setenv("DPH_PLAN_LANES", "", 1);
    CHECK(dp_env_long("DPH_PLAN_LANES", 5, 1, 8) == 1);  // (set and empty reads as 0, as atoi always did)
    unsetenv("DP_KX_DENSE");
    CHECK(dp_env_tristate("DP_KX_DENSE") == -1);
    setenv("DP_KX_DENSE", "0", 1);
    CHECK(dp_env_tristate("DP_KX_DENSE") == 0);
    setenv("DP_KX_DENSE", "1", 1);
    CHECK(dp_env_tristate("DP_KX_DENSE") == 1);
    setenv("DP_KX_DENSE", "yes", 1);
    CHECK(dp_env_tristate("DP_KX_DENSE") == 2);
    setenv("DP_KX_DENSE", "", 1);
    CHECK(dp_env_tristate("DP_KX_DENSE") == 2);
    unsetenv("DP_CONS_LAYOUTS");
    CHECK(!dp_env_has_word("DP_CONS_LAYOUTS", "huge"));
    setenv("DP_CONS_LAYOUTS", "nosmall,nohuge", 1);
    CHECK(dp_env_has_word("DP_CONS_LAYOUTS", "nosmall") && dp_env_has_word("DP_CONS_LAYOUTS", "nohuge"));
    CHECK(!dp_env_has_word("DP_CONS_LAYOUTS", "huge") && !dp_env_has_word("DP_CONS_LAYOUTS", "eager") && !dp_env_has_word("DP_CONS_LAYOUTS", "no"));
    setenv("DP_CONS_LAYOUTS", "huge", 1);
    CHECK(dp_env_has_word("DP_CONS_LAYOUTS", "huge") && !dp_env_has_word("DP_CONS_LAYOUTS", "nohuge"));
    // ---- the shared helpers
    unsetenv("DP_DEVICE_CONSENSUS");
    CHECK(dp_device_consensus_on());
    setenv("DP_DEVICE_CONSENSUS", "0", 1);
    CHECK(!dp_device_consensus_on());
    unsetenv("DPH_PROFILE");
    CHECK(!dp_profile_on());
    setenv("DPH_PROFILE", "", 1);
    CHECK(dp_profile_on());
    unsetenv("DP_SPIN_SYNC");
    setenv("DP_TUNE", "sync_poll_us=5", 1);
    CHECK(dp_wait_mode_read().spin == -1 && dp_wait_mode_read().poll_ns == 5000);
    setenv("DP_SPIN_SYNC", "1", 1);
    unsetenv("DP_TUNE");
    CHECK(dp_wait_mode_read().spin == 1 && dp_wait_mode_read().poll_ns == 20000);
    setenv("DP_SPIN_SYNC", "x", 1);
    CHECK(dp_wait_mode_read().spin == 0);

    // ---- a key the table does not have: one line that names it, once per distinct text of the variable
    {
        const std::string w = captured([] {
            setenv("DP_TUNE", "spec_blocks=2,spec_blokcs=4,cons_flag_evry=2", 1);
            for (int i = 0; i < 3; i++) (void)dp_tune("spec_blocks", 0);
            (void)dp_tune("kb_b1", 0);
        });
        CHECK(count(w, "\n") == 1 && count(w, "DP_TUNE") == 1 && count(w, "spec_blokcs") == 1 && count(w, "cons_flag_evry") == 1);
        CHECK(dp_tune("spec_blocks", 0) == 2);
        const std::string w2 = captured([] {
            setenv("DP_TUNE", "old_name=1", 1);
            (void)dp_tune("spec_blocks", 0);
            (void)dp_tune("spec_blocks", 0);
        });
        CHECK(count(w2, "\n") == 1 && count(w2, "old_name") == 1 && count(w2, "spec_blokcs") == 0);
        const std::string w3 = captured([] {
            setenv("DP_TUNE", "spec_blocks=2", 1);
            (void)dp_tune("spec_blocks", 0);
            setenv("DP_TUNE", "old_name=1", 1);  // a text that has had its line already
            (void)dp_tune("spec_blocks", 0);
            setenv("DP_DEBUG", "kx_bins,plannner", 1);
            (void)dp_debug("kx_bins");
            (void)dp_debug("planner");
        });
        CHECK(count(w3, "\n") == 1 && count(w3, "DP_DEBUG") == 1 && count(w3, "plannner") == 1);
    }

    // ---- two threads read while a third alternates the text: the cache behind dp_tune / dp_debug is what is under test.  (Every
    // text has been the variable's value before the threads start - setenv keeps the strings it has made and uses them again, so
    // only which of them the variable points to changes: a string made while somebody calls getenv is a race the C library itself
    // leaves open, and not this header's)
    {
        for (int i = 1; i >= 0; i--) {
            setenv("DP_TUNE", i & 1 ? "spec_blocks=2,kb_b1=6" : "spec_blocks=1", 1);
            setenv("DP_DEBUG", i & 1 ? "kx_bins,cons" : "kx_bins", 1);
        }
        std::atomic<bool> stop{false};
        std::atomic<int> bad{0};
        auto reader = [&] {
            while (!stop.load()) {
                const long v = dp_tune("spec_blocks", 7);
                if (v != 1 && v != 2) bad++;
                const long b1 = dp_tune("kb_b1", 8);
                if (b1 != 8 && b1 != 6) bad++;
                if (!dp_debug("kx_bins")) bad++;
            }
        };
        std::thread a(reader), b(reader);
        for (int i = 0; i < 2000; i++) {
            setenv("DP_TUNE", i & 1 ? "spec_blocks=2,kb_b1=6" : "spec_blocks=1", 1);
            setenv("DP_DEBUG", i & 1 ? "kx_bins,cons" : "kx_bins", 1);
        }
        stop = true;
        a.join();
        b.join();
        CHECK(bad.load() == 0);
    }

    // ---- a name the table does not have is a mistake in the code: the child dies and says which name
    {
        const std::string cmd = std::string(argv[0]) + " --unknown-name 2>&1";
        FILE* p = popen(cmd.c_str(), "r");
        CHECK(p != nullptr);
        std::string out;
        char buf[256];
        while (fgets(buf, sizeof buf, p)) out += buf;
        const int st = pclose(p);
        CHECK(st != 0);  // (the shell reports the child's SIGABRT as 134)
        CHECK(out.find("no_such_key") != std::string::npos);
    }
    printf("ok\n");
    return 0;
}
