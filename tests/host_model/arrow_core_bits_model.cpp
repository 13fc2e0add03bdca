// Host (CPU) view of the arrowhead solver core's intermediate results -- TEST HARNESS.
// The phases of tests/host_model/arrow_fused_model.cpp up to zeta-hat, returning what the eigenvectors are built from: the
// origin pole and tau of every root and zeta-hat of every surviving pole (tests/test_arrow_core_bits_host.py holds their bits).
// With the pole arrays of arrow_core.h (ADMMNET_ARROW_POLES) the roots run through that form, as on the device; against a
// header without them through the (d, z) form, which is how the recorded bits were taken.
//   g++ -O2 -shared -fPIC -I admm_net_amd/csrc tests/host_model/arrow_core_bits_model.cpp -o tests/host_model/libarrow_core_bits_model.so
#include <algorithm>
#include <cmath>
#include <vector>

#include "arrow_core.h"

using namespace admmnet;

extern "C" {

// C = [[diag h, z], [z^H, alpha]], z[D] interleaved complex.  org_out[D + 1], tau_out[D + 1], zhat_out[D]: the first k + 1 and k
// entries are written, the rest left as they are.  Returns k.
int arrow_core_bits(int D, float alpha, const float *z_ri, const float *h, int *org_out, float *tau_out, float *zhat_out) {
    std::vector<float> zeta(D);
    for (int i = 0; i < D; ++i) zeta[i] = std::sqrt(z_ri[2 * i] * z_ri[2 * i] + z_ri[2 * i + 1] * z_ri[2 * i + 1]);
    std::vector<int> perm(D);
    for (int i = 0; i < D; ++i) {
        int r = 0;
        for (int q = 0; q < D; ++q) r += (h[q] < h[i]) || (h[q] == h[i] && q < i);
        perm[r] = i;
    }
    std::vector<float> ds(D), zs(D), dl(D), zl(D);
    std::vector<int> src(D);
    std::vector<DcRot> rot(D);
    float dmax = std::fabs(alpha), zmax = 0.f;
    for (int p = 0; p < D; ++p) {
        ds[p] = h[perm[p]];
        zs[p] = zeta[perm[p]];
        dmax = std::max(dmax, std::fabs(ds[p]));
        zmax = std::max(zmax, zs[p]);
    }
    int k = 0, nrot = 0;
    deflate_scan_tol(D, 1.0f, dmax, zmax, ds.data(), zs.data(), dl.data(), zl.data(), src.data(), rot.data(), k, nrot);
    if (k == 0) return 0;
    float zn2 = 0.f;
    for (int i = 0; i < k; ++i) zn2 += zl[i] * zl[i];
    const float znorm = std::sqrt(zn2);
    std::vector<float> lamd(k + 1);
#if defined(ADMMNET_ARROW_POLES)
    std::vector<float> zz(k), dR(k), zzR(k);
    for (int i = 0; i < k; ++i) arrow_poles_fill(k, i, dl.data(), zl.data(), zz.data(), dR.data(), zzR.data());
    const ArrowPoles poles{dl.data(), zz.data(), dR.data(), zzR.data()};
#endif
    for (int j = 0; j <= k; ++j) {
#if defined(ADMMNET_ARROW_POLES)
        arrow_root(k, j, alpha, znorm, poles, org_out[j], tau_out[j]);
#else
        arrow_root(k, j, alpha, znorm, dl.data(), zl.data(), org_out[j], tau_out[j]);
#endif
        lamd[j] = dl[org_out[j]];
    }
    for (int i = 0; i < k; ++i) zhat_out[i] = arrow_zhat(k, i, dl.data(), lamd.data(), tau_out);
    return k;
}
}
