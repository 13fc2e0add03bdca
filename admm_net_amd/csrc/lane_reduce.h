// lane_reduce.h -- the eigensolver kernels' float lane exchanges and packed complex arithmetic, each defined once:
//   * DPP lane reads (dpp_get) and the sums built on them: no LDS traffic, no barrier;
//   * sums across the four 16-lane rows of a wave by v_permlane16_swap / v_permlane32_swap;
//   * complex multiply-adds on (re, im) register pairs in two v_pk_fma_f32.
// Users: tridiag_reg.hip, tridiag_big.hip, tridiag_panel.hip, wy_apply.hip, spectral_fused.hip (sums and products),
// dc.hip, arrow.hip (the lane-pair read).  Every file is its own translation unit and compiles this header under its own
// flags (build.py: tridiag_reg.hip and tridiag_panel.hip without the SLP vectoriser, which re-packs the DPP adds).
//
// THE RULES that keep this code correct -- stated here only, the kernels refer to this block:
//   1. The swaps are inline asm, never the compiler's __builtin_amdgcn_permlane16/32_swap: with identical operands it
//      folds the two results into one and the sums come out wrong (the hidden-copy workaround still failed the n = 257
//      test).
//   2. Every asm block of swaps opens and closes with `s_nop 1`: the hazard recogniser does not see inside inline asm, so
//      the block itself keeps the distance between the VALU write of its operands, the swaps and the VALU reads after.
//      The blocks are volatile; two values that are to overlap go through ONE block (rows_sum2, quad_rows_sum2, wave_sum4).
//   3. For the same reason a value that a DPP / lane instruction reads next must come out of a compiler-emitted VALU op,
//      never out of the asm products below: the LAST term of a sum of products that feeds a lane sum is written in
//      plain C++ (pk_cfma_open).
#pragma once
#include "common.h"

namespace admmnet {

// ---- DPP lane reads -------------------------------------------------------------------------------------------------
// CTRL 0x121/2/4/8 = row_ror:1/2/4/8 (rotate inside each row of 16 lanes), 0x140 / 0x141 = row_mirror / row_half_mirror,
// 0x142 / 0x143 = row_bcast:15 / row_bcast:31 (last lane of a row -> next row(s)), below 0x100 = quad_perm.
template <int CTRL, int ROWMASK = 0xF>
__device__ __forceinline__ float dpp_get(float x) {
    return __builtin_bit_cast(float,
                              __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), CTRL, ROWMASK, 0xF, false));
}
// x of the neighbouring lane l ^ 1 (quad_perm [1, 0, 3, 2]), and x + that
__device__ __forceinline__ float pair_get(float x) { return dpp_get<0xB1>(x); }
__device__ __forceinline__ float pair_sum(float x) { return x + pair_get(x); }
// sum over the 16 lanes of a DPP row; every lane of the row receives the total
__device__ __forceinline__ float row16_sum(float x) {
    x += dpp_get<0x128>(x);
    x += dpp_get<0x124>(x);
    x += dpp_get<0x122>(x);
    x += dpp_get<0x121>(x);
    return x;
}
// stage-wise row sum of NA - A0 complex values: the chains interleave, so no DPP hazard stalls
template <int NA, int A0>
__device__ __forceinline__ void row16_sum_all(f32x2 (&acc)[NA]) {
#pragma unroll
    for (int a = A0; a < NA; ++a) { acc[a].x += dpp_get<0x128>(acc[a].x); acc[a].y += dpp_get<0x128>(acc[a].y); }
#pragma unroll
    for (int a = A0; a < NA; ++a) { acc[a].x += dpp_get<0x124>(acc[a].x); acc[a].y += dpp_get<0x124>(acc[a].y); }
#pragma unroll
    for (int a = A0; a < NA; ++a) { acc[a].x += dpp_get<0x122>(acc[a].x); acc[a].y += dpp_get<0x122>(acc[a].y); }
#pragma unroll
    for (int a = A0; a < NA; ++a) { acc[a].x += dpp_get<0x121>(acc[a].x); acc[a].y += dpp_get<0x121>(acc[a].y); }
}
// One step of the transposing butterfly sum: this lane keeps `lo` (hi lanes: `hi`), its DPP partner sends the value it
// does not keep; returns kept + received.
template <int CTRL>
__device__ __forceinline__ float keep_add(bool hi_lane, float lo, float hi) {
    const float keep = hi_lane ? hi : lo, send = hi_lane ? lo : hi;
    return keep + dpp_get<CTRL>(send);
}
// sum over the whole wave as a wave-UNIFORM value (row totals chained through row_bcast, then a readlane)
__device__ __forceinline__ float wave_sum_dpp(float x) {
    x = row16_sum(x);
    x += dpp_get<0x142, 0xA>(x);   // rows 1, 3 += row 0, 2
    x += dpp_get<0x143, 0xC>(x);   // rows 2, 3 += rows 0 + 1
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}
// two such sums at once: the chains interleave
__device__ __forceinline__ void wave_sum_dpp2(float &x, float &y) {
    x += dpp_get<0x128>(x); y += dpp_get<0x128>(y);
    x += dpp_get<0x124>(x); y += dpp_get<0x124>(y);
    x += dpp_get<0x122>(x); y += dpp_get<0x122>(y);
    x += dpp_get<0x121>(x); y += dpp_get<0x121>(y);
    x += dpp_get<0x142, 0xA>(x); y += dpp_get<0x142, 0xA>(y);
    x += dpp_get<0x143, 0xC>(x); y += dpp_get<0x143, 0xC>(y);
    x = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
    y = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, y), 63));
}

// ---- sums across the rows of the wave (rules 1 and 2) -----------------------------------------------------------------
// x + (x of the partner row, 0 <-> 1, 2 <-> 3).  v_permlane16_swap (gfx950) exchanges the odd rows of the first operand
// with the even rows of the second, instead of a ds_bpermute round trip through the LDS pipeline:
// (a, b) = (x, x) -> a = [x0 x0 x2 x2], b = [x1 x1 x3 x3]
__device__ __forceinline__ float swap16_sum(float x) {
    float a = x, b = x;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    return a + b;
}
// x + (x of the lane 32 away): v_permlane32_swap exchanges the upper half of the first operand with the lower half of
// the second
__device__ __forceinline__ float swap32_sum(float x) {
    float a = x, b = x;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 1" : "+v"(a), "+v"(b));
    return a + b;
}
// sum over the four rows, lane by lane (x of lanes l, l ^ 16, l ^ 32, l ^ 48): every lane gets it
__device__ __forceinline__ float rows_sum(float x) { return swap32_sum(swap16_sum(x)); }
// the same for two values at once (re / im)
__device__ __forceinline__ void rows_sum2(float &x, float &y) {
    float a = x, b = x, c = y, d = y;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\tv_permlane16_swap_b32 %2, %3\n\ts_nop 1"
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    x = a + b;
    y = c + d;
    a = x;
    b = x;
    c = y;
    d = y;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\tv_permlane32_swap_b32 %2, %3\n\ts_nop 1"
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    x = a + b;
    y = c + d;
}
// all-reduce over the 32 lanes of a half wave, and over all 64 (every lane gets the sum; wave_sum_dpp is the uniform one)
__device__ __forceinline__ float row32_sum(float x) { return swap16_sum(row16_sum(x)); }
__device__ __forceinline__ float wave_sum_swap(float x) { return rows_sum(row16_sum(x)); }
// Two quadruples (re / im) of per-lane partial vectors, each value to be summed over the four rows of the wave, reduced
// together: 3 swaps + 3 adds per quadruple instead of 8 + 8.  Result: row 0 holds the total of x[0], row 1 of x[2],
// row 2 of x[1], row 3 of x[3].
__device__ __forceinline__ void quad_rows_sum2(const float (&x)[4], const float (&y)[4], float &tx, float &ty) {
    float x0 = x[0], x1 = x[1], x2 = x[2], x3 = x[3], y0 = y[0], y1 = y[1], y2 = y[2], y3 = y[3];
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\tv_permlane32_swap_b32 %2, %3\n\t"
                 "v_permlane32_swap_b32 %4, %5\n\tv_permlane32_swap_b32 %6, %7\n\ts_nop 1"
                 : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(y0), "+v"(y1), "+v"(y2), "+v"(y3));
    float a = x0 + x1, b = x2 + x3, c = y0 + y1, d = y2 + y3;
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\tv_permlane16_swap_b32 %2, %3\n\ts_nop 1"
                 : "+v"(a), "+v"(b), "+v"(c), "+v"(d));
    tx = a + b;
    ty = c + d;
}
// Four wave-wide sums for the price of ~one: returns t with t(row 0) = sum a, t(row 1) = sum b, t(row 2) = sum c,
// t(row 3) = sum d (every lane of a row holds the sum).
__device__ __forceinline__ float wave_sum4(float a, float b, float c, float d) {
    // halves: lanes 0..31 keep (a, b), lanes 32..63 keep (c, d)
    float a2 = a, c2 = c, b2 = b, d2 = d;
    asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\tv_permlane32_swap_b32 %2, %3\n\ts_nop 1"
                 : "+v"(a2), "+v"(c2), "+v"(b2), "+v"(d2));
    float x = a2 + c2, y = b2 + d2;   // x: [a lo+hi | c lo+hi], y: [b | d]
    asm volatile("s_nop 1\n\tv_permlane16_swap_b32 %0, %1\n\ts_nop 1" : "+v"(x), "+v"(y));
    return row16_sum(x + y);          // rows: a, b, c, d
}

// ---- packed complex arithmetic on (re, im) register pairs (f32x2, common.h) -----------------------------------------
// A complex multiply-add in TWO packed instructions (the scalar form takes four): f32 vector peak on gfx950 needs
// v_pk_fma_f32, and the skinny phases are bound by the VALU issue of ONE wave per SIMD (a wave64 instruction holds the
// 16-lane SIMD for 4 cycles).
__device__ __forceinline__ f32x2 pk2(float2 a) { return f32x2{a.x, a.y}; }
__device__ __forceinline__ float2 unpk2(f32x2 a) { return make_float2(a.x, a.y); }
// (-v.y, v.x) = i v and (v.y, -v.x) = -i v: formed once per vector element for pk_cfma_open and reused across a whole
// block row / column
__device__ __forceinline__ f32x2 rot(f32x2 v) { return f32x2{-v.y, v.x}; }
__device__ __forceinline__ f32x2 rotc(f32x2 v) { return f32x2{v.y, -v.x}; }
// The open form is plain C++ that hipcc turns into one v_pk_fma_f32 per half (op_sel broadcasts, no shuffles) given the
// rotated operand, which says which product it is: use it where rule 3 asks for a compiler-emitted op.
//   bj = rot(b):   acc + a b        = fma(a.xx, (b.x, b.y), acc), then fma(a.yy, (-b.y, b.x), .)
//   bj = rotc(b):  acc + conj(a) b  = fma(a.xx, (b.x, b.y), acc), then fma(a.yy, (b.y, -b.x), .)
__device__ __forceinline__ f32x2 pk_cfma_open(f32x2 acc, f32x2 a, f32x2 b, f32x2 bj) {
    acc = __builtin_elementwise_fma(a.xx, b, acc);
    return __builtin_elementwise_fma(a.yy, bj, acc);
}
// The asm forms fold the rotation into the operand selects (op_sel picks the real / imaginary half of each operand pair)
// and the negate bits (neg_lo / neg_hi) of the second instruction: the compiler folds the broadcast of the first product
// but materialises the swapped, negated operand of the second (v_mov + v_xor per use).
__device__ __forceinline__ f32x2 pk_cfma(f32x2 acc, f32x2 a, f32x2 b) {        // acc + a b
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]\n\t"
        "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"
        : "+v"(acc)
        : "v"(a), "v"(b));
    return acc;
}
__device__ __forceinline__ f32x2 pk_cfma_conj(f32x2 acc, f32x2 a, f32x2 b) {   // acc + conj(a) b (= acc + b conj(a))
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1]\n\t"
        "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_hi:[0,1,0]"
        : "+v"(acc)
        : "v"(a), "v"(b));
    return acc;
}
__device__ __forceinline__ f32x2 pk_cmul(f32x2 a, f32x2 b) {                   // a b (no accumulator to clear first)
    f32x2 acc;
    asm("v_pk_mul_f32 %0, %1, %2 op_sel_hi:[0,1]\n\t"
        "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[0,1,0]"
        : "=&v"(acc)
        : "v"(a), "v"(b));
    return acc;
}
// acc - conj(a) b (= acc - b conj(a)): pk_cfma_conj with the broadcast operand negated (neg_lo / neg_hi on src0)
__device__ __forceinline__ f32x2 pk_cfms_conj(f32x2 acc, f32x2 a, f32x2 b) {
    asm("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[0,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"
        "v_pk_fma_f32 %0, %1, %2, %0 op_sel:[1,1,0] op_sel_hi:[1,0,1] neg_lo:[1,0,0] neg_hi:[1,1,0]"
        : "+v"(acc)
        : "v"(a), "v"(b));
    return acc;
}
}  // namespace admmnet
