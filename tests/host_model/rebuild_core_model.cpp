// Host (CPU) entry points of admm_net_amd/csrc/rebuild_core.h -- TEST HARNESS.
// The eigenvalue map in float and in double and the lower-triangle tile decode, exactly the functions the kernels inline.
//   g++ -O2 -shared -fPIC -I admm_net_amd/csrc tests/host_model/rebuild_core_model.cpp -o tests/host_model/librebuild_core_model.so
#include "rebuild_core.h"

using namespace admmnet;

extern "C" {

// vn: w1[16] b1[16] w2[16] b2[1]; thr already sigmoid-ed
void eig_map_f32(int m, const float *lam, float thr, const float *vn, float *out) {
    for (int i = 0; i < m; ++i) out[i] = eig_map(lam[i], thr, vn);
}

void eig_map_f64_host(int m, const double *lam, double thr, const float *vn, double *out) {
    for (int i = 0; i < m; ++i) out[i] = eig_map_f64(lam[i], thr, vn);
}

void tri_tiles(int m, int *IJ) {
    for (int t = 0; t < m; ++t) tri_tile(t, IJ[2 * t], IJ[2 * t + 1]);
}
}
