// host_par.h -- the workgroup of csrc/scene_wg.h's ScenePar<THREADS> emulated on the host, for the models of the scene kernels
// (refine_model.cpp, order_model.cpp, cfar_model.cpp, relax_model.cpp): the threads are a loop over the items, a sum adds every
// thread's items in index order, then the lanes of a wave in the butterfly's pairing, then the waves in order; the best item is
// kept per thread in index order, then among the lanes in the butterfly's pairing, then among the waves.  The ONE host statement
// of that order: a model instantiates it with the thread constant of its kernel.
#pragma once

template <int THREADS>
struct HostPar {
    template <class F>
    void each(int count, F fn) {
        for (int item = 0; item < count; ++item) fn(item);
    }

    static double fold(double *v) {   // v[THREADS]: lanes by the butterfly, waves in order
        double total = 0.0;
        for (int w = 0; w < THREADS / 64; ++w) {
            double *lane = v + 64 * w;
            for (int o = 32; o > 0; o >>= 1)
                for (int i = 0; i < o; ++i) lane[i] += lane[i + o];
            total = w == 0 ? lane[0] : total + lane[0];
        }
        return total;
    }

    template <class F>
    double sum(int count, F fn) {
        double v[THREADS];
        for (int t = 0; t < THREADS; ++t) {
            v[t] = 0.0;
            for (int item = t; item < count; item += THREADS) v[t] += fn(item);
        }
        return fold(v);
    }

    template <int N, class F>
    void sums(int count, F fn, double (&out)[N]) {
        static double acc[THREADS][N];
        for (int t = 0; t < THREADS; ++t) {
            for (int n = 0; n < N; ++n) acc[t][n] = 0.0;
            for (int item = t; item < count; item += THREADS) fn(item, acc[t]);
        }
        for (int n = 0; n < N; ++n) {
            double v[THREADS];
            for (int t = 0; t < THREADS; ++t) v[t] = acc[t][n];
            out[n] = fold(v);
        }
    }

    static bool better(double ov, int oi, double bv, int bi) { return ov > bv || (ov == bv && oi < bi); }

    template <class F>
    int best(int count, F fn) {
        double bv[THREADS];
        int bi[THREADS];
        for (int t = 0; t < THREADS; ++t) {
            bv[t] = -1.0;
            bi[t] = -1;
            for (int item = t; item < count; item += THREADS) {
                const double v = fn(item);
                if (v > bv[t]) {
                    bv[t] = v;
                    bi[t] = item;
                }
            }
        }
        double top = -1.0;
        int at = -1;
        for (int w = 0; w < THREADS / 64; ++w) {
            double *v = bv + 64 * w;
            int *k = bi + 64 * w;
            for (int o = 32; o > 0; o >>= 1)
                for (int i = 0; i < o; ++i)
                    if (better(v[i + o], k[i + o], v[i], k[i])) {
                        v[i] = v[i + o];
                        k[i] = k[i + o];
                    }
            if (w == 0 || better(v[0], k[0], top, at)) {
                top = v[0];
                at = k[0];
            }
        }
        return top >= 0.0 ? at : -1;
    }
};
