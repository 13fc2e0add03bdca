// Stand-alone host program for csrc/options.h (plain g++, no HIP), built by tests/test_options.py with -fsanitize=address,undefined
// and with -fsanitize=thread: the interning table under concurrent use, its errors, and its behaviour at capacity.
// Exit status 0 and "ok" on success; the first failed check prints its line and exits 1.
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <string>
#include <thread>
#include <vector>

#include "options.h"

using namespace admmnet;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "options_model.cpp:%d: %s\n", __LINE__, #cond); \
            exit(1);                                                     \
        }                                                                \
    } while (0)

constexpr int kSets = 64, kInterners = 8, kResolvers = 4, kRounds = 20;

// set i: ADMMNET_SPECTRAL_ITERS = 100 + i, ADMMNET_EIG = ql on odd i; `flip` gives the other order and another spelling
static int32_t intern_set(int i, bool flip, char *err, size_t err_len) {
    const std::string iters = (flip ? "0" : "") + std::to_string(100 + i);   // atoi reads "0107" as 107
    const char *eig = (i & 1) ? "ql" : (flip ? "dc" : "no");                 // anything but "ql" is the default solver
    const char *n0[] = {"ADMMNET_SPECTRAL_ITERS", "ADMMNET_EIG"}, *v0[] = {iters.c_str(), eig};
    const char *n1[] = {"ADMMNET_EIG", "ADMMNET_SPECTRAL_ITERS"}, *v1[] = {eig, iters.c_str()};
    return flip ? options_intern(n1, v1, 2, err, err_len) : options_intern(n0, v0, 2, err, err_len);
}

static void check_set(int i, const Switches *s) {
    const Switches &d = switches();
    CHECK(s != nullptr);
    CHECK(s->spectral_iters == 100 + i && s->eig_ql == (bool)(i & 1));
    CHECK(s->spectral == d.spectral && s->spectral_tol == d.spectral_tol && s->pn_split == d.pn_split && s->dc_blocks == d.dc_blocks &&
          s->lean == d.lean && s->arrow == d.arrow && s->tr_occ3 == d.tr_occ3 && s->pad_min_set == d.pad_min_set);
}

int main() {
    char err[256] = "";
    // ---- 1. eight threads intern overlapping sets while four resolve what has been published ------------------------------------
    static std::atomic<int32_t> published[kSets];
    static int32_t seen[kInterners][kSets];
    std::atomic<bool> done{false};
    std::vector<std::thread> th;
    for (int t = 0; t < kInterners; ++t)
        th.emplace_back([t] {
            char e[256];
            for (int r = 0; r < kRounds; ++r)
                for (int j = 0; j < kSets; ++j) {
                    const int i = (j * (2 * t + 1) + 7 * t + r) % kSets;   // every thread walks the sets in its own order
                    const int32_t h = intern_set(i, (t + r) & 1, e, sizeof(e));
                    CHECK(h >= 1 && h <= kSets);
                    CHECK(seen[t][i] == 0 || seen[t][i] == h);
                    seen[t][i] = h;
                    check_set(i, options_resolve(h));
                    published[i].store(h, std::memory_order_release);
                }
        });
    std::vector<std::thread> rs;
    for (int t = 0; t < kResolvers; ++t)
        rs.emplace_back([&done] {
            while (!done.load(std::memory_order_acquire))
                for (int i = 0; i < kSets; ++i) {
                    const int32_t h = published[i].load(std::memory_order_acquire);
                    if (h) check_set(i, options_resolve(h));
                    CHECK(options_resolve(kOptionsCapacity + 1 + i) == nullptr && options_resolve(-1 - i) == nullptr);
                    CHECK(options_resolve(0) == &switches());
                }
        });
    for (auto &t : th) t.join();
    done.store(true, std::memory_order_release);
    for (auto &t : rs) t.join();
    std::vector<bool> used(kSets + 1, false);
    for (int i = 0; i < kSets; ++i) {
        for (int t = 0; t < kInterners; ++t) CHECK(seen[t][i] == seen[0][i]);   // one handle per distinct set across threads
        CHECK(!used[seen[0][i]]);                                              // and one set per handle
        used[seen[0][i]] = true;
    }
    CHECK(options_table().count.load() == kSets);

    // ---- 2. what is not a set ---------------------------------------------------------------------------------------------------
    CHECK(options_intern(nullptr, nullptr, 0, err, sizeof(err)) == 0);
    {
        const Switches &d = switches();   // pairs that restate the defaults change nothing: handle 0
        const std::string it = std::to_string(d.spectral_iters);
        const char *n[] = {"ADMMNET_SPECTRAL", "ADMMNET_SPECTRAL_ITERS"}, *v[] = {d.spectral ? "1" : "0", it.c_str()};
        CHECK(options_intern(n, v, 2, err, sizeof(err)) == 0);
    }
    {
        const char *n[] = {"ADMMNET_SPECTRAL", "ADMMNET_NO_SUCH_SWITCH"}, *v[] = {"0", "1"};
        CHECK(options_intern(n, v, 2, err, sizeof(err)) == -1 && strstr(err, "ADMMNET_NO_SUCH_SWITCH"));
        const char *n2[] = {"ADMMNET_SPECTRAL", nullptr};
        CHECK(options_intern(n2, v, 2, err, sizeof(err)) == -1 && strstr(err, "name 1 is NULL"));
        const char *v2[] = {nullptr, "1"};
        CHECK(options_intern(n, v2, 2, err, sizeof(err)) == -1 && strstr(err, "ADMMNET_SPECTRAL"));
        CHECK(options_intern(nullptr, v, 2, err, sizeof(err)) == -1 && options_intern(n, nullptr, 2, err, sizeof(err)) == -1);
        CHECK(options_intern(n, v, -1, err, sizeof(err)) == -1);
        CHECK(options_table().count.load() == kSets);   // none of them left an entry
    }
    {   // of two pairs with one name the later wins
        const char *n[] = {"ADMMNET_SPECTRAL_ITERS", "ADMMNET_SPECTRAL_ITERS"}, *v[] = {"3", "100"};
        CHECK(options_intern(n, v, 2, err, sizeof(err)) == seen[0][0]);
    }

    // ---- 3. capacity: the table fills to kOptionsCapacity entries, then refuses new sets and still serves the old ------------------
    for (int j = kSets; j < kOptionsCapacity; ++j) {
        const std::string it = std::to_string(10000 + j);
        const char *n[] = {"ADMMNET_SPECTRAL_ITERS"}, *v[] = {it.c_str()};
        CHECK(options_intern(n, v, 1, err, sizeof(err)) == j + 1);
    }
    CHECK(options_table().count.load() == kOptionsCapacity);
    for (int j = 0; j < 8; ++j) {
        const std::string it = std::to_string(20000 + j);
        const char *n[] = {"ADMMNET_SPECTRAL_ITERS"}, *v[] = {it.c_str()};
        CHECK(options_intern(n, v, 1, err, sizeof(err)) == -1 && strstr(err, "full"));
    }
    CHECK(options_table().count.load() == kOptionsCapacity);
    CHECK(options_resolve(kOptionsCapacity) && options_resolve(kOptionsCapacity)->spectral_iters == 10000 + kOptionsCapacity - 1);
    CHECK(options_resolve(kOptionsCapacity + 1) == nullptr);
    for (int i = 0; i < kSets; ++i) CHECK(intern_set(i, i & 1, err, sizeof(err)) == seen[0][i]);
    CHECK(options_intern(nullptr, nullptr, 0, err, sizeof(err)) == 0);
    char buf[2048];
    const int64_t len = options_describe(*options_resolve(seen[0][1]), buf, sizeof(buf));
    CHECK(len > 0 && len < (int64_t)sizeof(buf) && strstr(buf, "ADMMNET_SPECTRAL_ITERS 101\n") && strstr(buf, "ADMMNET_EIG 1\n"));
    char tiny[8];
    CHECK(options_describe(switches(), tiny, sizeof(tiny)) == options_describe(switches(), buf, sizeof(buf)) && strlen(tiny) == 7);
    printf("ok\n");
    return 0;
}
