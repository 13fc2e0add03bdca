// options.h -- option sets: the Switches of one model instead of one process.  An option set is the process defaults
// (route.h switches(): the environment) overridden by (name, value) pairs in the environment's own names and syntax; the
// table below interns the RESOLVED Switches and hands out a small integer handle, which admmnet_cfg carries in reserved[0].
// Handle 0 is the process defaults.  Plain C++17 without a HIP include: tests/host_model/options_model.cpp compiles it with g++
// under the address, undefined-behaviour and thread sanitizers (tests/test_options.py).
#pragma once
#include <stdio.h>

#include <atomic>
#include <mutex>

#include "route.h"

namespace admmnet {

constexpr int kOptionsCapacity = 4096;   // distinct option sets per process (besides the defaults)

// A switch added to Switches (route.h) joins builtin_switches() and the parser there, and same_switches() and options_describe()
// here: a field missing from same_switches() would make two different sets share a handle.  The size pins the field list.
static_assert(sizeof(Switches) == 60, "Switches changed: extend same_switches() and options_describe(), then update this size");

inline bool same_switches(const Switches &a, const Switches &b) {   // field by field (the struct has padding); tol by its bits
    return a.spectral == b.spectral && a.spectral_fused == b.spectral_fused && !memcmp(&a.spectral_tol, &b.spectral_tol, sizeof(float)) &&
           a.spectral_iters == b.spectral_iters && a.sf_fold == b.sf_fold && a.prep_gather == b.prep_gather && a.sf_smallwg == b.sf_smallwg && a.sf_timing == b.sf_timing &&
           a.eig_ql == b.eig_ql && a.arrow == b.arrow && a.arrow_fused == b.arrow_fused && a.arrow_onekernel == b.arrow_onekernel && a.ar_timing == b.ar_timing &&
           a.lean == b.lean && a.fuse_back == b.fuse_back && a.br_timing == b.br_timing && a.tridiag_lds == b.tridiag_lds &&
           a.tridiag_sweep == b.tridiag_sweep && a.back_q == b.back_q && a.rebuild_tiles == b.rebuild_tiles &&
           a.pad_min_set == b.pad_min_set && a.pad_min == b.pad_min && a.two_streams == b.two_streams && a.one_stream == b.one_stream && a.tr_occ3 == b.tr_occ3 &&
           a.tr_pad_lds == b.tr_pad_lds && a.pn_split == b.pn_split && a.pn_timing == b.pn_timing && a.dc_occ == b.dc_occ &&
           a.dc_blocks == b.dc_blocks && a.dc_poison == b.dc_poison && a.dc_timing == b.dc_timing;
}

// Append-only: entry i (handle i + 1) is written once, under the lock, before `count` is published past it with release order;
// a reader that saw count > i with acquire order reads a finished entry, and nothing ever changes it afterwards.
struct OptionsTable {
    std::mutex mu;
    std::atomic<int32_t> count{0};
    Switches entry[kOptionsCapacity];
};
inline OptionsTable &options_table() { static OptionsTable t; return t; }

// The Switches of a handle: 0 = the process defaults, 1 .. count = an interned set, anything else = nullptr (never issued).
// The pointer stays valid, and what it points to unchanged, for the life of the process.
inline const Switches *options_resolve(int32_t handle) {
    if (handle == 0) return &switches();
    OptionsTable &t = options_table();
    if (handle < 0 || handle > t.count.load(std::memory_order_acquire)) return nullptr;
    return &t.entry[handle - 1];
}

// Interns the Switches `s`: 0 if it equals the process defaults, the handle of an equal entry, a new handle, or -1 when the
// table is full.
inline int32_t options_intern_switches(const Switches &s) {
    if (same_switches(s, *options_resolve(0))) return 0;
    OptionsTable &t = options_table();
    std::lock_guard<std::mutex> lk(t.mu);
    const int32_t n = t.count.load(std::memory_order_relaxed);
    for (int32_t i = 0; i < n; ++i)
        if (same_switches(s, t.entry[i])) return i + 1;
    if (n >= kOptionsCapacity) return -1;
    t.entry[n] = s;
    t.count.store(n + 1, std::memory_order_release);
    return n + 1;
}

// The process defaults overridden by `count` (name, value) pairs (a later pair of the same name wins).  Returns the handle
// (>= 0), or -1 with the reason in err: a null pointer, a name the parser of route.h never asks for, or a full table.
inline int32_t options_intern(const char *const *names, const char *const *values, int32_t count, char *err, size_t err_len) {
    if (count < 0 || (count > 0 && (!names || !values))) {
        snprintf(err, err_len, "options: %s", count < 0 ? "negative count" : "names or values is NULL");
        return -1;
    }
    for (int32_t i = 0; i < count; ++i)
        if (!names[i] || !values[i]) {
            snprintf(err, err_len, "options: %s %d is NULL%s%s", names[i] ? "value" : "name", i, names[i] ? " for " : "",
                     names[i] ? names[i] : "");
            return -1;
        }
    // the names the parser asks for are the names that exist: a pair it never looked up is unknown
    constexpr int kMaxPairs = 256;
    if (count > kMaxPairs) {
        snprintf(err, err_len, "options: %d pairs (at most %d)", count, kMaxPairs);
        return -1;
    }
    bool asked[kMaxPairs] = {};
    const auto lookup = [&](const char *name) -> const char * {
        const char *v = nullptr;
        for (int32_t i = 0; i < count; ++i)
            if (!strcmp(names[i], name)) asked[i] = true, v = values[i];
        return v;
    };
    const Switches s = switches_from_env(*options_resolve(0), lookup);
    for (int32_t i = 0; i < count; ++i)
        if (!asked[i]) {
            snprintf(err, err_len, "options: unknown name \"%s\"", names[i]);
            return -1;
        }
    const int32_t h = options_intern_switches(s);
    if (h < 0) snprintf(err, err_len, "options: the table is full (%d distinct sets)", kOptionsCapacity);
    return h;
}

// "name value" lines, one per switch, in the form tests/host_model/route_model prints its switches.  Returns the length of the
// whole text without the terminator (as snprintf: the text is cut to len - 1 characters when the buffer is smaller).
inline int64_t options_describe(const Switches &s, char *buf, size_t len) {
    return snprintf(buf, len,
                    "ADMMNET_SPECTRAL %d\nADMMNET_SPECTRAL_FUSED %d\nADMMNET_SPECTRAL_TOL %.9g\nADMMNET_SPECTRAL_ITERS %d\n"
                    "ADMMNET_SF_FOLD %d\nADMMNET_SF_SMALLWG %d\nADMMNET_SF_TIMING %d\nADMMNET_EIG %d\n"
                    "ADMMNET_ARROW %d\nADMMNET_ARROW_FUSED %d\nADMMNET_AR_TIMING %d\nADMMNET_LEAN %d\nADMMNET_FUSE_BACK %d\n"
                    "ADMMNET_BR_TIMING %d\nADMMNET_TRIDIAG %d\nADMMNET_TRIDIAG_BIG %d\nADMMNET_BACK %d\nADMMNET_REBUILD %d\n"
                    "ADMMNET_PAD_MIN %d\nADMMNET_STREAMS %d\nADMMNET_TR_OCC %d\nADMMNET_TR_PAD_LDS %d\nADMMNET_PN_SPLIT %d\n"
                    "ADMMNET_PN_TIMING %d\nADMMNET_DC_OCC %d\nADMMNET_DC_BLOCKS %d\nADMMNET_DC_POISON %d\nADMMNET_DC_TIMING %d\n",
                    s.spectral, s.spectral_fused, (double)s.spectral_tol, s.spectral_iters, s.sf_fold, s.sf_smallwg, s.sf_timing, s.eig_ql,   // (ADMMNET_SF_FOLD and ADMMNET_ARROW_FUSED 1 also where they were set to 2)
                    s.arrow, s.arrow_fused, s.ar_timing, s.lean, s.fuse_back, s.br_timing, s.tridiag_lds, s.tridiag_sweep, s.back_q,
                    s.rebuild_tiles, s.pad_min_set ? s.pad_min : -1000, s.two_streams, s.tr_occ3, s.tr_pad_lds, s.pn_split, s.pn_timing,
                    s.dc_occ, s.dc_blocks, s.dc_poison, s.dc_timing);
}

}  // namespace admmnet
