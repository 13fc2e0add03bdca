// set_model.cpp -- csrc/set_core.h (and the search of csrc/score_core.h) on the host, with the wave of csrc/loss_set.hip emulated:
// 64 "lanes" in arrays, every __shfl a plain index, the xor-butterfly argmin a loop under the same order (sc_better).  A
// stand-alone program (its own main): tests/test_set_loss.py builds it with -fsanitize=address,undefined and runs it.
//   set_model            checks the search on random signals of every size pair up to 6 x 6 against the least value of the
//                        DEFINITION over all assignments (brute force), the shape of every assignment, and the options; prints "ok"
//   set_model FILE       reads signals (one per line: Lmax Lt n sx sy period_tau period_f w_conf, then tau, f, conf of the slots
//                        and tau, f of the Lt targets) and prints per signal: nonfinite, assign[Lmax], loss_b, match_b, conf_b
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "set_core.h"

using namespace admmnet;

#define CHECK(cond, ...)                                 \
    do {                                                 \
        if (!(cond)) {                                   \
            std::fprintf(stderr, "FAILED %s:%d: ", __FILE__, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);           \
            std::fprintf(stderr, "\n");                  \
            std::exit(1);                                \
        }                                                \
    } while (0)

struct Signal {
    int Lmax, Lt;
    long long n_raw;
    double opts[SET_OPTS];
    std::vector<double> tau, f, conf, t_tau, t_f;
};

struct Result {
    bool nonfinite, outside;
    std::vector<int> assign;
    double v[3];
};

// the body of ls_set_kernel for one signal
static Result emu_set(const Signal &s) {
    const int Lmax = s.Lmax;
    Result r;
    const int n = sc_clamp_count(s.n_raw, s.Lt, &r.outside);
    double s_tau[SC_MAX] = {}, s_f[SC_MAX] = {}, s_conf[SC_MAX] = {}, t_tau[SC_MAX] = {}, t_f[SC_MAX] = {};
    r.nonfinite = false;
    for (int l = 0; l < SC_MAX; ++l) {
        if (l < Lmax) s_tau[l] = s.tau[l], s_f[l] = s.f[l], s_conf[l] = s.conf[l];
        if (l < n) t_tau[l] = s.t_tau[l], t_f[l] = s.t_f[l];
        r.nonfinite = r.nonfinite || !(sc_finite(s_tau[l]) && sc_finite(s_f[l]) && sc_finite(s_conf[l]) && sc_finite(t_tau[l]) &&
                                       sc_finite(t_f[l]));
    }
    r.assign.assign(Lmax, -1);
    r.v[0] = r.v[1] = r.v[2] = 0.0;
    if (r.nonfinite) return r;
    const ScoreOpt o = set_score_opt(s.opts);
    const double w_conf = s.opts[4], wl = w_conf / (double)Lmax;
    double term[SC_MAX];
    for (int l = 0; l < SC_MAX; ++l) term[l] = set_term(wl, s_conf[l]);
    const bool rows_slots = Lmax <= n;
    const double *r_tau = rows_slots ? s_tau : t_tau, *r_f = rows_slots ? s_f : t_f;
    const int nrows = rows_slots ? Lmax : n;
    ScCol col[SC_MAX];
    double u[SC_MAX] = {};
    for (int l = 0; l < SC_MAX; ++l)
        sc_col_init(col[l], rows_slots ? t_tau[l] : s_tau[l], rows_slots ? t_f[l] : s_f[l], rows_slots ? l < n : l < Lmax);
    for (int root = 0; root < nrows; ++root) {
        bool in_tree[SC_MAX] = {};
        for (int l = 0; l < SC_MAX; ++l) sc_col_begin(col[l]);
        in_tree[root] = true;
        int cur = root, j0 = -1, step = 0;
        for (;; ++step) {
            CHECK(step <= SC_MAX, "a search longer than the columns there are");
            for (int l = 0; l < SC_MAX; ++l)
                set_relax(col[l], rows_slots, r_tau[cur], r_f[cur], u[cur], j0, rows_slots ? term[cur] : term[l], n, o);
            double key = sc_key(col[0]);
            int arg = 0;
            for (int l = 1; l < SC_MAX; ++l)
                if (sc_better(key, arg, sc_key(col[l]), l)) {
                    key = sc_key(col[l]);
                    arg = l;
                }
            CHECK(sc_finite(key), "no free column left");
            for (int l = 0; l < SC_MAX; ++l) sc_shift(col[l], u[l], in_tree[l], key);
            col[arg].used = true;
            j0 = arg;
            cur = col[arg].p;
            if (cur < 0) break;
            in_tree[cur] = true;
        }
        for (step = 0; j0 >= 0; ++step) {
            CHECK(step <= SC_MAX, "a path longer than the columns there are");
            const int before = col[j0].way;
            col[j0].p = before < 0 ? root : col[before].p;
            j0 = before;
        }
    }
    int pairs = 0;
    for (int l = 0; l < SC_MAX; ++l) {
        if (col[l].p < 0) continue;
        CHECK(col[l].live && col[l].p < nrows, "column %d holds row %d", l, col[l].p);
        const int slot = rows_slots ? col[l].p : l, target = rows_slots ? l : col[l].p;
        CHECK(slot < Lmax && target < n && r.assign[slot] < 0, "pair (%d, %d)", slot, target);
        r.assign[slot] = target;
        ++pairs;
    }
    CHECK(pairs == std::min(Lmax, n), "%d pairs matched, expected %d", pairs, std::min(Lmax, n));
    std::vector<int> seen;
    for (int a : r.assign)
        if (a >= 0) seen.push_back(a);
    std::sort(seen.begin(), seen.end());
    CHECK(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "a target on two slots");
    double sum_d2 = 0.0, sum_c = 0.0;
    for (int i = 0; i < Lmax; ++i) {
        const int a = r.assign[i];
        if (a >= 0) sum_d2 += sc_delta(s_tau[i], s_f[i], t_tau[a], t_f[a], o).d2;
        sum_c += set_conf_sq(s_conf[i], a >= 0);
    }
    set_values(sum_d2, sum_c, n, Lmax, w_conf, r.v);
    return r;
}

// the least value of the definition over all assignments: slot by slot, a free target or none, k = min(Lmax, n) matched
static double brute(const Signal &s, int n, int slot, std::vector<char> &taken, int matched, double sum_d2, double sum_c) {
    const ScoreOpt o = set_score_opt(s.opts);
    const int k = std::min(s.Lmax, n);
    if (slot == s.Lmax)
        return matched == k ? sum_d2 / (double)std::max(n, 1) + s.opts[4] * sum_c / (double)s.Lmax : INFINITY;
    double best = INFINITY;
    if (s.Lmax - slot - 1 >= k - matched)   // leave this slot out
        best = brute(s, n, slot + 1, taken, matched, sum_d2, sum_c + s.conf[slot] * s.conf[slot]);
    for (int j = 0; j < n && matched < k; ++j) {
        if (taken[j]) continue;
        taken[j] = 1;
        const double e = s.conf[slot] - 1.0;
        best = std::min(best, brute(s, n, slot + 1, taken, matched + 1,
                                    sum_d2 + sc_delta(s.tau[slot], s.f[slot], s.t_tau[j], s.t_f[j], o).d2, sum_c + e * e));
        taken[j] = 0;
    }
    return best;
}

static Signal draw(std::mt19937_64 &g, int Lmax, int Lt, int n, const double *opts) {
    std::uniform_real_distribution<double> ut(0.0, 1.0), uf(-0.5, 0.5);
    std::normal_distribution<double> nz(0.0, 0.03);
    Signal s;
    s.Lmax = Lmax, s.Lt = Lt, s.n_raw = n;
    std::copy(opts, opts + SET_OPTS, s.opts);
    for (int j = 0; j < Lt; ++j) s.t_tau.push_back((double)(float)ut(g)), s.t_f.push_back((double)(float)uf(g));
    for (int i = 0; i < Lmax; ++i) {
        const bool copy = i < Lt && ut(g) < 0.8;
        s.tau.push_back((double)(float)(copy ? s.t_tau[i] + nz(g) : ut(g)));
        s.f.push_back((double)(float)(copy ? s.t_f[i] + nz(g) : uf(g)));
        s.conf.push_back((double)(float)ut(g));
    }
    return s;
}

static int self_check() {
    std::mt19937_64 g(20260301);
    const double plain[SET_OPTS] = {1, 1, 0, 0, 0.1, 0}, scaled[SET_OPTS] = {16, 10, 1, 1, 5, 0}, w0[SET_OPTS] = {1, 1, 0, 1, 0, 0};
    for (const double *opts : {plain, scaled, w0})
        for (int Lmax = 1; Lmax <= 6; ++Lmax)
            for (int Lt = 1; Lt <= 6; ++Lt)
                for (int rep = 0; rep < 12; ++rep) {
                    const int n = rep % (Lt + 1);
                    const Signal s = draw(g, Lmax, Lt, n, opts);
                    const Result r = emu_set(s);
                    std::vector<char> taken(Lt, 0);
                    const double want = brute(s, n, 0, taken, 0, 0.0, 0.0);
                    CHECK(!r.nonfinite && std::fabs(r.v[0] - want) <= 1e-12 * std::fabs(want) + 1e-300,
                          "loss %.17g, the least value of the definition is %.17g (Lmax=%d, Lt=%d, n=%d)", r.v[0], want, Lmax, Lt, n);
                }
    const int big[][3] = {{64, 64, 64}, {64, 3, 3}, {3, 64, 64}, {33, 17, 9}};
    for (const auto &b : big) {
        const Result r = emu_set(draw(g, b[0], b[1], b[2], plain));   // (the shape of the assignment is checked inside)
        CHECK(!r.nonfinite && r.v[0] >= 0.0, "large sizes");
    }
    // n = 0: nothing matched, the loss is the confidences' own
    {
        Signal s = draw(g, 3, 2, 0, plain);
        const Result r = emu_set(s);
        double c2 = 0;
        for (double c : s.conf) c2 += c * c;
        CHECK(r.assign == std::vector<int>(3, -1) && r.v[1] == 0.0 && std::fabs(r.v[0] - 0.1 * c2 / 3) < 1e-15, "n = 0");
        s.n_raw = -4;
        CHECK(emu_set(s).outside && emu_set(s).v[0] == r.v[0], "L_true below the range is held to 0");
        s.n_raw = 7;
        CHECK(emu_set(s).outside && emu_set(s).assign != r.assign, "L_true above the range is held to Lt");
    }
    // a value that is no number inside the first n counts, past n it does not
    {
        Signal s = draw(g, 2, 3, 2, plain);
        s.t_tau[2] = NAN;
        CHECK(!emu_set(s).nonfinite, "a NaN truth past n");
        s.t_f[1] = NAN;
        CHECK(emu_set(s).nonfinite && emu_set(s).assign == std::vector<int>(2, -1) && emu_set(s).v[0] == 0.0, "a NaN truth inside n");
        s.t_f[1] = 0.0;
        s.conf[1] = INFINITY;
        CHECK(emu_set(s).nonfinite, "an infinite confidence");
    }
    {
        const double bad1[SET_OPTS] = {0, 1, 0, 0, 0.1, 0}, bad2[SET_OPTS] = {1, 1, -1, 0, 0.1, 0}, bad3[SET_OPTS] = {1, 1, 0, 0, -0.1, 0},
                     bad4[SET_OPTS] = {1, 1, 0, 0, 0.1, NAN}, bad5[SET_OPTS] = {1, INFINITY, 0, 0, 0.1, 0};
        CHECK(set_opts_ok(plain) && set_opts_ok(scaled) && set_opts_ok(w0), "good options");
        CHECK(!set_opts_ok(bad1) && !set_opts_ok(bad2) && !set_opts_ok(bad3) && !set_opts_ok(bad4) && !set_opts_ok(bad5), "bad options");
    }
    CHECK(set_grad_coord(1.5, 2.0, 0.25, 3, 4) == 1.5 * 2.0 * 4.0 * 0.25 / 12.0, "g_tau");
    CHECK(set_grad_conf(0.5, 0.75, true, 2, 4) == 0.5 * 2.0 * -0.25 / 8.0 && set_grad_conf(0.5, 0.75, false, 2, 4) == 0.5 * 2.0 * 0.75 / 8.0,
          "g_conf");
    std::puts("ok");
    return 0;
}

int main(int argc, char **argv) {
    if (argc < 2) return self_check();
    FILE *in = std::fopen(argv[1], "r");
    CHECK(in, "cannot open %s", argv[1]);
    for (;;) {
        Signal s;
        if (std::fscanf(in, "%d %d %lld", &s.Lmax, &s.Lt, &s.n_raw) != 3) break;
        CHECK(s.Lmax >= 1 && s.Lmax <= SC_MAX && s.Lt >= 1 && s.Lt <= SC_MAX, "sizes %d, %d", s.Lmax, s.Lt);
        s.opts[5] = 0.0;
        for (int i = 0; i < 5; ++i) CHECK(std::fscanf(in, "%lf", &s.opts[i]) == 1, "options");
        CHECK(set_opts_ok(s.opts), "options refused");
        auto read = [&](std::vector<double> &v, int count) {
            v.resize(count);
            for (double &x : v) CHECK(std::fscanf(in, "%lf", &x) == 1, "a value");
        };
        read(s.tau, s.Lmax), read(s.f, s.Lmax), read(s.conf, s.Lmax), read(s.t_tau, s.Lt), read(s.t_f, s.Lt);
        const Result r = emu_set(s);
        std::printf("%d", (int)r.nonfinite);
        for (int a : r.assign) std::printf(" %d", a);
        std::printf(" %.17g %.17g %.17g\n", r.v[0], r.v[1], r.v[2]);
    }
    std::fclose(in);
    return 0;
}
