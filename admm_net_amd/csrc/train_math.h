// train_math.h -- arithmetic shared by the training kernels (train_small.hip, train_hlayer.hip, train_head.hip).  The
// activations and their derivatives are softplus_f, sigmoid_f, dsoftplus_f and dsigmoid_f of eig_core.h.
#pragma once
#include "common.h"

namespace admmnet {

// sum_{i < len} w[i * stride] x[i], x in LDS, four interleaved partial sums
__device__ __forceinline__ float dot4(const float *__restrict__ w, int stride, const float *x, int len) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    int i = 0;
    for (; i + 3 < len; i += 4) {
        a0 = fmaf(w[(int64_t)i * stride], x[i], a0);
        a1 = fmaf(w[(int64_t)(i + 1) * stride], x[i + 1], a1);
        a2 = fmaf(w[(int64_t)(i + 2) * stride], x[i + 2], a2);
        a3 = fmaf(w[(int64_t)(i + 3) * stride], x[i + 3], a3);
    }
    for (; i < len; ++i) a0 = fmaf(w[(int64_t)i * stride], x[i], a0);
    return (a0 + a1) + (a2 + a3);
}

}  // namespace admmnet
