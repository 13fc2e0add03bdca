// score_model.cpp -- csrc/score_core.h on the host, with the wave of csrc/score.hip emulated: 64 "lanes" in arrays, every
// __shfl a plain index, the xor-butterfly argmin a loop under the same order (sc_better).  A stand-alone program (its own main):
// tests/test_metrics.py builds it with -fsanitize=address,undefined and runs it.  It checks, on random signals of every size
// pair up to 7 x 7 and a few up to 64 x 64,
//   * the cost of the assignment found == the least cost over ALL assignments (brute force, min(ne, nt) <= 7) to 1e-12 relative,
//     == the cost of a plain O(n^3) serial Hungarian method above that;
//   * the assignment is injective, within the live rows and columns, and matches min(ne, nt) pairs;
//   * the wrap, the clamp, the truncation example and the chain that a greedy matcher fails.
// Prints "ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

#include "score_core.h"

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
    std::vector<double> e_tau, e_f;   // Le rows, NaN = absent
    std::vector<double> t_tau, t_f;   // the first nt are the targets
};

struct Result {
    std::vector<int> match;   // per target: the estimate that hit it, -1
    double stats[SC_STATS];
    int ne, nt;
};

// the body of sc_match_kernel for one signal
static Result emu_match(const Signal &s, const ScoreOpt &o) {
    const int Le = (int)s.e_tau.size(), nt = (int)s.t_tau.size();
    bool e_live[SC_MAX] = {}, t_live[SC_MAX] = {};
    double e_tau[SC_MAX] = {}, e_f[SC_MAX] = {}, t_tau[SC_MAX] = {}, t_f[SC_MAX] = {};
    int ne = 0;
    for (int l = 0; l < SC_MAX; ++l) {
        if (l < Le) {
            e_tau[l] = s.e_tau[l];
            e_f[l] = s.e_f[l];
            e_live[l] = sc_finite(e_tau[l]) && sc_finite(e_f[l]);
            ne += e_live[l];
        }
        if (l < nt) {
            t_tau[l] = s.t_tau[l];
            t_f[l] = s.t_f[l];
            t_live[l] = true;
        }
    }
    const bool rows_est = ne <= nt;
    const double *r_tau = rows_est ? e_tau : t_tau, *r_f = rows_est ? e_f : t_f;
    const bool *r_live = rows_est ? e_live : t_live;
    ScCol col[SC_MAX];
    double u[SC_MAX] = {};
    for (int l = 0; l < SC_MAX; ++l)
        sc_col_init(col[l], rows_est ? t_tau[l] : e_tau[l], rows_est ? t_f[l] : e_f[l], rows_est ? t_live[l] : e_live[l]);
    for (int root = 0; root < SC_MAX; ++root) {
        if (!r_live[root]) continue;
        bool in_tree[SC_MAX] = {};
        for (int l = 0; l < SC_MAX; ++l) sc_col_begin(col[l]);
        in_tree[root] = true;
        int cur = root, j0 = -1, step = 0;
        for (;; ++step) {
            CHECK(step <= SC_MAX, "a search longer than the columns there are");
            for (int l = 0; l < SC_MAX; ++l) sc_relax(col[l], r_tau[cur], r_f[cur], u[cur], j0, o);
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
    Result r;
    r.ne = ne;
    r.nt = nt;
    r.match.assign(nt, -1);
    double n_hit = 0, s_tau = 0, s_f = 0, s_d2 = 0;
    for (int l = 0; l < SC_MAX; ++l) {
        if (!col[l].live || col[l].p < 0) continue;
        const int p = col[l].p;
        CHECK(p < SC_MAX && r_live[p], "column %d holds row %d that does not exist", l, p);
        const ScDelta d = sc_delta(r_tau[p], r_f[p], col[l].tau, col[l].f, o);
        if (!sc_hit(d.d2, o.c2)) continue;
        n_hit += 1;
        s_tau += d.dtau * d.dtau;
        s_f += d.df * d.df;
        s_d2 += d.d2;
        const int truth = rows_est ? l : p, est = rows_est ? p : l;
        CHECK(truth < nt && est < Le, "pair (%d, %d) outside the signal", est, truth);
        CHECK(r.match[truth] < 0, "target %d matched twice", truth);
        r.match[truth] = est;
    }
    int assigned = 0;
    std::vector<int> seen;
    for (int l = 0; l < SC_MAX; ++l)
        if (col[l].p >= 0) {
            ++assigned;
            CHECK(col[l].live, "a row on a column that does not exist");
            seen.push_back(col[l].p);
        }
    std::sort(seen.begin(), seen.end());
    CHECK(std::adjacent_find(seen.begin(), seen.end()) == seen.end(), "a row on two columns");
    CHECK(assigned == std::min(ne, nt), "%d pairs matched, expected %d", assigned, std::min(ne, nt));
    sc_stats(ne, nt, n_hit, s_tau, s_f, s_d2, o.c2, r.stats);
    return r;
}

static std::vector<std::vector<double>> cost_matrix(const Signal &s, const ScoreOpt &o, std::vector<int> &live) {
    live.clear();
    for (size_t i = 0; i < s.e_tau.size(); ++i)
        if (sc_finite(s.e_tau[i]) && sc_finite(s.e_f[i])) live.push_back((int)i);
    std::vector<std::vector<double>> C(live.size(), std::vector<double>(s.t_tau.size()));
    for (size_t a = 0; a < live.size(); ++a)
        for (size_t j = 0; j < s.t_tau.size(); ++j)
            C[a][j] = sc_cost(sc_delta(s.e_tau[live[a]], s.e_f[live[a]], s.t_tau[j], s.t_f[j], o).d2, o.c2);
    return C;
}

// least cost over all assignments of the smaller side into the larger
static double brute(const std::vector<std::vector<double>> &C) {
    const int n = (int)C.size(), m = n ? (int)C[0].size() : 0;
    if (n == 0 || m == 0) return 0.0;
    const bool tr = n > m;
    const int rows = tr ? m : n, cols = tr ? n : m;
    std::vector<int> idx(cols);
    std::iota(idx.begin(), idx.end(), 0);
    double best = INFINITY;
    do {
        double c = 0;
        for (int i = 0; i < rows; ++i) c += tr ? C[idx[i]][i] : C[i][idx[i]];
        best = std::min(best, c);
        std::reverse(idx.begin() + rows, idx.end());   // skip the orders of the unused tail
    } while (std::next_permutation(idx.begin(), idx.end()));
    return best;
}

// the textbook serial Hungarian method, rows <= columns
static double serial(const std::vector<std::vector<double>> &C0) {
    int n = (int)C0.size(), m = n ? (int)C0[0].size() : 0;
    if (n == 0 || m == 0) return 0.0;
    std::vector<std::vector<double>> C = C0;
    if (n > m) {
        C.assign(m, std::vector<double>(n));
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < m; ++j) C[j][i] = C0[i][j];
        std::swap(n, m);
    }
    std::vector<double> u(n + 1), v(m + 1);
    std::vector<int> p(m + 1), way(m + 1);
    for (int i = 1; i <= n; ++i) {
        p[0] = i;
        int j0 = 0;
        std::vector<double> minv(m + 1, INFINITY);
        std::vector<char> used(m + 1, 0);
        do {
            used[j0] = 1;
            const int i0 = p[j0];
            double delta = INFINITY;
            int j1 = 0;
            for (int j = 1; j <= m; ++j)
                if (!used[j]) {
                    const double cur = C[i0 - 1][j - 1] - u[i0] - v[j];
                    if (cur < minv[j]) minv[j] = cur, way[j] = j0;
                    if (minv[j] < delta) delta = minv[j], j1 = j;
                }
            for (int j = 0; j <= m; ++j)
                if (used[j])
                    u[p[j]] += delta, v[j] -= delta;
                else
                    minv[j] -= delta;
            j0 = j1;
        } while (p[j0] != 0);
        do {
            const int j1 = way[j0];
            p[j0] = p[j1];
            j0 = j1;
        } while (j0);
    }
    double c = 0;
    for (int j = 1; j <= m; ++j)
        if (p[j]) c += C[p[j] - 1][j - 1];
    return c;
}

static Signal draw(std::mt19937_64 &g, int Le, int nt, bool absent) {
    std::uniform_real_distribution<double> ut(0.1, 0.9), uf(-0.4, 0.4), u01(0.0, 1.0);
    std::normal_distribution<double> nz(0.0, 0.03);
    Signal s;
    for (int j = 0; j < nt; ++j) {
        s.t_tau.push_back((double)(float)ut(g));
        s.t_f.push_back((double)(float)uf(g));
    }
    std::vector<int> order(nt);
    std::iota(order.begin(), order.end(), 0);
    std::shuffle(order.begin(), order.end(), g);
    for (int i = 0; i < Le; ++i) {
        if (i < nt && u01(g) < 0.8) {   // a noisy copy of a target, else a stray
            s.e_tau.push_back(s.t_tau[order[i]] + nz(g));
            s.e_f.push_back(s.t_f[order[i]] + nz(g));
        } else {
            s.e_tau.push_back(ut(g));
            s.e_f.push_back(uf(g));
        }
        if (absent && u01(g) < 0.2) s.e_tau.back() = NAN;
    }
    std::vector<int> rows(Le);
    std::iota(rows.begin(), rows.end(), 0);
    std::shuffle(rows.begin(), rows.end(), g);
    Signal t = s;
    for (int i = 0; i < Le; ++i) t.e_tau[i] = s.e_tau[rows[i]], t.e_f[i] = s.e_f[rows[i]];
    return t;
}

static void check_signal(const Signal &s, const ScoreOpt &o, bool small) {
    const Result r = emu_match(s, o);
    std::vector<int> live;
    const auto C = cost_matrix(s, o, live);
    const double want = small ? brute(C) : serial(C), got = r.stats[7];
    CHECK(std::fabs(got - want) <= 1e-12 * std::fabs(want) + 1e-300,
          "cost %.17g, the optimum is %.17g (ne=%d, nt=%d)", got, want, r.ne, r.nt);
    CHECK(r.stats[0] + r.stats[1] == r.nt && r.stats[0] + r.stats[2] == r.ne, "counts do not add up");
}

int main() {
    std::mt19937_64 g(20260104);
    const ScoreOpt o = {1.0, 1.0, 0.1 * 0.1, 0.0, 0.0};
    for (int Le = 1; Le <= 7; ++Le)
        for (int nt = 1; nt <= 7; ++nt)
            for (int rep = 0; rep < 40; ++rep) check_signal(draw(g, Le, nt, rep % 4 == 3), o, true);
    const ScoreOpt scaled = {10.0, 7.0, 1.0, 1.0, 1.0};
    for (int rep = 0; rep < 200; ++rep) check_signal(draw(g, 1 + rep % 6, 1 + (rep / 6) % 6, false), scaled, true);
    const int big[][2] = {{8, 8}, {17, 33}, {33, 17}, {64, 3}, {3, 64}, {64, 64}, {63, 64}, {64, 63}};
    for (const auto &b : big)
        for (int rep = 0; rep < 6; ++rep) check_signal(draw(g, b[0], b[1], rep == 5), o, false);

    // no estimate, no target
    {
        Signal s;
        s.e_tau = {NAN, 0.3};
        s.e_f = {0.1, INFINITY};
        s.t_tau = {0.3, 0.5};
        s.t_f = {0.1, 0.2};
        const Result r = emu_match(s, o);
        CHECK(r.ne == 0 && r.stats[0] == 0 && r.stats[1] == 2 && r.stats[2] == 0 && r.stats[6] == o.c2 && r.stats[7] == 0, "all absent");
        s.t_tau.clear();
        s.t_f.clear();
        s.e_tau = {0.2};
        s.e_f = {0.0};
        const Result q = emu_match(s, o);
        CHECK(q.nt == 0 && q.stats[2] == 1 && q.stats[6] == 0.5 * o.c2, "no target");
    }
    // the chain: identity is optimal, a nearest-neighbour matcher pairs estimate j with target j + 1
    for (int m : {3, 8, 64}) {
        Signal s;
        for (int j = 0; j < m; ++j) {
            s.t_tau.push_back((double)(float)(0.1 + 0.01 * j));
            s.t_f.push_back(0.0);
            s.e_tau.push_back(s.t_tau.back() + 0.006);
            s.e_f.push_back(0.0);
        }
        const ScoreOpt wide = {1.0, 1.0, 100.0, 0.0, 0.0};
        const Result r = emu_match(s, wide);
        for (int j = 0; j < m; ++j) CHECK(r.match[j] == j, "chain m=%d: target %d got %d", m, j, r.match[j]);
        CHECK(std::fabs(r.stats[7] - 3.6e-5 * m) < 1e-9, "chain cost %.12g", r.stats[7]);
    }
    // the truncation is inside the solve
    {
        Signal s;
        s.e_tau = {0.26, 0.33};
        s.t_tau = {(double)0.20f, (double)0.27f};
        s.e_f = {0.0, 0.0};
        s.t_f = {0.0, 0.0};
        const Result a = emu_match(s, ScoreOpt{1.0, 1.0, 100.0, 0.0, 0.0});
        CHECK(a.match[0] == 0 && a.match[1] == 1, "untruncated: (0,0), (1,1)");
        const Result b = emu_match(s, ScoreOpt{1.0, 1.0, 0.05 * 0.05, 0.0, 0.0});
        CHECK(b.match[0] == -1 && b.match[1] == 0 && b.stats[0] == 1, "truncated: the one hit is estimate 0 on target 1");
        CHECK(std::fabs(b.stats[7] - 0.0026) < 1e-8, "truncated cost %.12g", b.stats[7]);
    }
    // wrap and clamp
    CHECK(std::fabs(sc_wrap(0.01 - 0.98, 1.0) - 0.03) < 1e-15 && sc_wrap(-0.97, 0.0) == -0.97, "wrap");
    CHECK(sc_wrap(0.5, 1.0) == -0.5 && sc_wrap(-0.5, 1.0) == -0.5 && sc_wrap(0.25, 1.0) == 0.25, "wrap edges");
    {
        bool out;
        CHECK(sc_clamp_count(-3, 5, &out) == 0 && out, "clamp below");
        CHECK(sc_clamp_count(9, 5, &out) == 5 && out, "clamp above");
        CHECK(sc_clamp_count(5, 5, &out) == 5 && !out, "clamp inside");
        CHECK(sc_clamp_count(INT64_MAX, 64, &out) == 64 && out && sc_clamp_count(INT64_MIN, 64, &out) == 0 && out, "clamp extremes");
    }
    {
        const double good[5] = {1, 1, 0.1, 0, 1}, bad1[5] = {0, 1, 0.1, 0, 0}, bad2[5] = {1, 1, NAN, 0, 0}, bad3[5] = {1, 1, 1, -1, 0};
        CHECK(sc_opts_ok(good) && !sc_opts_ok(bad1) && !sc_opts_ok(bad2) && !sc_opts_ok(bad3), "options");
    }
    // huge finite coordinates: d^2 overflows, the pair costs c^2 and is no hit
    {
        Signal s;
        s.e_tau = {1e308};
        s.e_f = {0.0};
        s.t_tau = {-3e38};
        s.t_f = {0.0};
        const Result r = emu_match(s, ScoreOpt{1e10, 1.0, 0.01, 0.0, 0.0});
        CHECK(r.match[0] == -1 && r.stats[7] == 0.01, "huge coordinates");
    }
    std::puts("ok");
    return 0;
}
