// csrc/knobs.h on the CPU: the table, the loader, the three text knobs and the publication of snapshots.  Its own main;
// no HIP, no other header of the project.  tests/test_knobs_host.py builds and runs it plain, with the address and
// undefined-behaviour sanitizers, and with the thread sanitizer (the last group of checks is what that build is for).
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <thread>
#include <vector>

#include "knobs.h"

using namespace sageicp;

static long g_checks = 0;
#define CHECK(cond)                                                               \
    do {                                                                          \
        ++g_checks;                                                               \
        if (!(cond)) {                                                            \
            std::printf("knobs_check: FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                         \
        }                                                                         \
    } while (0)

static int clamped(const KnobDesc &d, int v) { return v < d.lo ? d.lo : (v > d.hi ? d.hi : v); }

static void clear_environment() {
    for (const KnobDesc &d : kKnobTable) unsetenv(d.name);
}

// the table itself: every name once, every field once, a default inside its own clamp
static void check_table() {
    std::set<std::string> names;
    std::set<const IntKnob *> fields;
    const Knobs probe;
    for (const KnobDesc &d : kKnobTable) {
        CHECK(std::strncmp(d.name, "SAGEICP_", 8) == 0);
        CHECK(names.insert(d.name).second);
        CHECK((d.field != nullptr) != (d.parse != nullptr));
        if (!d.field) continue;
        CHECK(fields.insert(&(probe.*d.field)).second);
        CHECK(d.lo <= d.hi);
        if (d.has_default) CHECK(clamped(d, d.dflt) == d.dflt);
    }
    CHECK(names.size() == 49);
    CHECK(fields.size() == 45);
}

// unset -> get(d) is d and get() the table's default; set -> the value inside the clamp; unset again
static void check_integers() {
    clear_environment();
    const Knobs &empty = reload_knobs();
    for (const KnobDesc &d : kKnobTable) {
        if (!d.field) continue;
        const IntKnob &f = empty.*d.field;
        CHECK(!f.set);
        CHECK(f.get(12345) == 12345 && f.get(-7) == -7);
        if (d.has_default) CHECK(f.get() == d.dflt);
    }
    const char *texts[] = {"0", "1", "-1", "2", "3", "4", "5", "9", "17", "-40", "2147483647", "-2147483648", "12abc", "abc", "", " 7"};
    for (const char *t : texts) {
        for (const KnobDesc &d : kKnobTable)
            if (d.field) setenv(d.name, t, 1);
        const Knobs &k = reload_knobs();
        for (const KnobDesc &d : kKnobTable) {
            if (!d.field) continue;
            const IntKnob &f = k.*d.field;
            CHECK(f.set);
            CHECK(f.get() == clamped(d, std::atoi(t)));       // (non-numeric text: atoi's answer)
            CHECK(f.get(12345) == f.get());
        }
    }
    // the clamps the call sites used to spell, on values that decide
    setenv("SAGEICP_LW", "7", 1);
    setenv("SAGEICP_LOOP_PRIO", "-2", 1);
    setenv("SAGEICP_LOOP_DEAL", "3", 1);
    setenv("SAGEICP_DEPTH", "100", 1);
    setenv("SAGEICP_ACC_SHIFT", "5", 1);
    setenv("SAGEICP_LOOP_COOLDOWN", "-1", 1);
    setenv("SAGEICP_LOOP_TIMEOUT_MS", "0", 1);
    setenv("SAGEICP_MAX_ITER", "0", 1);
    setenv("SAGEICP_SORT_FROM", "-3", 1);
    setenv("SAGEICP_LOOP_COUNT_TIMEOUT_RANK", "-5", 1);
    {
        const Knobs &k = reload_knobs();
        CHECK(k.lw.get() == 4 && k.loop_prio.get() == 0 && k.loop_deal.get() == 2 && k.depth.get() == 8);
        CHECK(k.acc_shift.get() == 2 && k.loop_cooldown.get() == 0 && k.loop_timeout_ms.get() == 1);
        CHECK(k.max_iter.get(500) == 1 && k.sort_from.get(16384) == 0 && k.loop_count_timeout_rank.get() == -5);
    }
    setenv("SAGEICP_LW", "-3", 1);                            // negative: not forced, like unset
    CHECK(reload_knobs().lw.get() == -1);
    clear_environment();
    const Knobs &again = reload_knobs();
    for (const KnobDesc &d : kKnobTable)
        if (d.field) CHECK(!(again.*d.field).set && (again.*d.field).get(77) == 77);
    CHECK(again == empty);
}

// SAGEICP_DEVICES as sageicp_map_create read it before the table existed
static std::vector<int> devices_by_strtol(const char *list) {
    std::vector<int> devs;
    for (const char *q = list; *q;) {
        char *end = nullptr;
        const long v = std::strtol(q, &end, 10);
        if (end == q) break;
        devs.push_back(static_cast<int>(v));
        q = (*end == ',') ? end + 1 : end;
    }
    return devs;
}

static void check_text_knobs() {
    clear_environment();
    {
        const Knobs &k = reload_knobs();
        CHECK(k.n_devices == 0 && !k.cu_share_set && k.cu_share_i == 0 && k.cu_share_k == 1);
        CHECK(k.map_archive_max_rows == 0 && k.size_classes);
    }
    const char *lists[] = {"0,1,2", "3", "", "1,x", "0,1,2,3,4,5,6,7", " 2, 5", "1,,2", "4;5", "-1,2"};
    for (const char *l : lists) {
        setenv("SAGEICP_DEVICES", l, 1);
        const Knobs &k = reload_knobs();
        const std::vector<int> want = devices_by_strtol(l);
        CHECK(k.n_devices == static_cast<int>(want.size()));
        for (int i = 0; i < k.n_devices; ++i) CHECK(k.devices[i] == want[i]);
    }
    {
        // a list longer than the array: cut at its size, still more than the eight that sageicp_map_set_devices takes
        std::string many;
        for (int i = 0; i < 40; ++i) many += (i ? "," : "") + std::to_string(i);
        setenv("SAGEICP_DEVICES", many.c_str(), 1);
        const Knobs &k = reload_knobs();
        CHECK(k.n_devices == kMaxKnobDevices && kMaxKnobDevices > 8);
        for (int i = 0; i < k.n_devices; ++i) CHECK(k.devices[i] == i);
    }
    struct Share {
        const char *text;
        bool ok;
        int i, k;
    };
    const Share shares[] = {{"1/2", true, 1, 2}, {"0/1", true, 0, 1}, {"15/16", true, 15, 16}, {"2/2", false, 0, 1},
                            {"0/17", false, 0, 1}, {"-1/4", false, 0, 1}, {"1", false, 0, 1}, {"a/b", false, 0, 1},
                            {"", false, 0, 1}, {"1/0", false, 0, 1}};
    for (const Share &s : shares) {
        setenv("SAGEICP_CU_SHARE", s.text, 1);
        const Knobs &k = reload_knobs();
        CHECK(k.cu_share_set == s.ok && k.cu_share_i == s.i && k.cu_share_k == s.k);
    }
    setenv("SAGEICP_MAP_ARCHIVE_MAX_ROWS", "0", 1);
    CHECK(reload_knobs().map_archive_max_rows == 0);
    setenv("SAGEICP_MAP_ARCHIVE_MAX_ROWS", "4294967296", 1);
    CHECK(reload_knobs().map_archive_max_rows == 4294967296ull);
    setenv("SAGEICP_MAP_ARCHIVE_MAX_ROWS", "-5", 1);
    CHECK(reload_knobs().map_archive_max_rows == 0);
    setenv("SAGEICP_MAP_ARCHIVE_MAX_ROWS", "12rows", 1);
    CHECK(reload_knobs().map_archive_max_rows == 12);
    // off only for a value that begins with '0' (the rule HostMap::configure had)
    const std::pair<const char *, bool> classes[] = {{"0", false}, {"00", false}, {"01", false}, {"1", true}, {"", true}, {"x", true}, {" 0", true}};
    for (const auto &c : classes) {
        setenv("SAGEICP_SIZE_CLASSES", c.first, 1);
        CHECK(reload_knobs().size_classes == c.second);
    }
    clear_environment();
}

// a reference outlives a reload; an unchanged environment publishes nothing
static void check_snapshots() {
    clear_environment();
    setenv("SAGEICP_LOOP", "0", 1);
    setenv("SAGEICP_DEVICES", "0,1", 1);
    const Knobs &before = reload_knobs();
    CHECK(&knobs() == &before && &reload_knobs() == &before && &knobs() == &before);
    setenv("SAGEICP_LOOP", "2", 1);
    setenv("SAGEICP_DEVICES", "3", 1);
    const Knobs &after = reload_knobs();
    CHECK(&after != &before && &knobs() == &after);
    CHECK(before.loop.get() == 0 && before.n_devices == 2 && before.devices[1] == 1);
    CHECK(after.loop.get() == 2 && after.n_devices == 1 && after.devices[0] == 3);
    for (int i = 0; i < 100; ++i) {            // (the store grows: the first references stay where they are)
        setenv("SAGEICP_DEPTH", std::to_string(1 + i % 8).c_str(), 1);
        (void)reload_knobs();
    }
    CHECK(before.loop.get() == 0 && before.n_devices == 2 && after.loop.get() == 2 && after.devices[0] == 3);
    clear_environment();
}

// Eight readers beside a reloading main thread.  Phase 1: the environment does not change while they run.  Phase 2:
// it changes between joins only (setenv beside getenv is a race of the C library's).  A reader sees the three fields of
// ONE load: depth, prio and deal are always set from the same number.
static void check_threads() {
    clear_environment();
    auto set_all = [](int v) {
        setenv("SAGEICP_DEPTH", std::to_string(1 + v).c_str(), 1);
        setenv("SAGEICP_LOOP_PRIO", std::to_string(v % 4).c_str(), 1);
        setenv("SAGEICP_LOOP_DEAL", std::to_string(v % 3).c_str(), 1);
    };
    std::atomic<long> bad{0}, reads{0};
    auto reader = [&](int a, int c) {       // every read is the load of a or the load of c
        long b = 0;
        for (int i = 0; i < 100000; ++i) {
            const Knobs &k = knobs();
            const int v = k.depth.get() - 1;
            if ((v != a && v != c) || k.loop_prio.get() != v % 4 || k.loop_deal.get() != v % 3) ++b;
        }
        bad += b;
        reads += 100000;
    };
    set_all(5);
    (void)reload_knobs();
    {
        std::vector<std::thread> th;
        for (int t = 0; t < 8; ++t) th.emplace_back(reader, 5, 5);
        const Knobs *first = &knobs();
        for (int i = 0; i < 1000; ++i) CHECK(&reload_knobs() == first);
        for (auto &t : th) t.join();
    }
    for (int v = 0; v < 8; ++v) {
        set_all(v);                            // (nobody reads the environment now)
        std::vector<std::thread> th;
        for (int t = 0; t < 8; ++t) th.emplace_back(reader, v == 0 ? 5 : v - 1, v);   // the last load (phase 1's 5 at first) or this one
        (void)reload_knobs();
        for (auto &t : th) t.join();
        CHECK(knobs().depth.get() == 1 + v);
    }
    CHECK(bad.load() == 0);
    CHECK(reads.load() == 9 * 8 * 100000L);
    clear_environment();
}

int main() {
    check_table();
    check_integers();
    check_text_knobs();
    check_snapshots();
    check_threads();
    std::printf("knobs_check: OK %ld\n", g_checks);
    return 0;
}
