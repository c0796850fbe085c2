// The sixteen-rows-per-wave layout of the row-local kernels (acm_conv_agg16.hip, acm_conv_local16.hip, acm_conv_aggw.hip) and the
// part of the ACM head that they share: lane (g, m) of a wave holds columns 16 t + 4 g + r (t, r = 0..3) of row m as
// f32x4 D[c][t], so a whole row sits in the four lanes m, m + 16, m + 32, m + 48.  Everything here is inlined into its kernel.
// A block moved here only where every kernel kept its registers, scratch, LDS and occupancy (profiles/r08_rows16_head_resources.txt):
// the forward's epi16_body and the blocks of K3 behind the head (post-op undone, mix backward, the channel pass, the slab) did not
// and stay written out in their kernels -- a change of the head arithmetic below has to be repeated in epi16_body.
#pragma once
#include "acm_conv_device.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// floats of the head-parameter partial vector of three channels: [d att_vec | d gamma | d beta][c][col] | d att_mix[c][j]
constexpr int ROWS16_NPG = 3 * 3 * 64 + 9;

// sum over the four lanes that hold one row (lanes m, m + 16, m + 32, m + 48); result in all four
__device__ __forceinline__ float row4_sum(float v) { return acm_cross_row_sum(v); }

// sum over the 16 lanes of a row for 16 values per lane, leaving value i's total in lane i (m = i): a reduce-scatter of four
// DPP exchange steps (partner = 15 - m, 7 - m within the half, m ^ 2, m ^ 1; each lane keeps the half of the values its
// own lane bit selects and adds the partner's copy of them) -- 45 instructions, where sixteen all-reduces cost 64 and
// sixteen per-lane accumulators would pin 48 registers per kernel.
__device__ __forceinline__ float row_reduce_scatter16(const float (&v)[16], int m) {
    const bool b3 = (m & 8) != 0, b2 = (m & 4) != 0, b1 = (m & 2) != 0, b0 = (m & 1) != 0;
    float a[8], b[4], c[2];
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = (b3 ? v[i + 8] : v[i]) + acm_dpp<0x140>(b3 ? v[i] : v[i + 8]);       // row_mirror
#pragma unroll
    for (int i = 0; i < 4; ++i) b[i] = (b2 ? a[i + 4] : a[i]) + acm_dpp<0x141>(b2 ? a[i] : a[i + 4]);       // row_half_mirror
#pragma unroll
    for (int i = 0; i < 2; ++i) c[i] = (b1 ? b[i + 2] : b[i]) + acm_dpp<0x4E>(b1 ? b[i] : b[i + 2]);        // quad_perm [2,3,0,1]
    return (b0 ? c[1] : c[0]) + acm_dpp<0xB1>(b0 ? c[0] : c[1]);                                            // quad_perm [1,0,3,2]
}

// Stages the head parameters of a K3 kernel of `nthreads` threads: hl = [att_vec | gamma | beta][c][col] (gamma = 1, beta = 0
// without LayerNorm), ul[c][col] = u_c = att_vec_c (.) gamma_c, and per lane c0_c = sum_col beta_c v_c, c1_c = mean_col(u_c).
// The caller's barrier publishes hl and ul.
template <int NC, bool LN, class P>
__device__ __forceinline__ void rows16_stage_head_params(const P& p, int nthreads, int lane, float* hl, float* ul, float (&c0)[NC],
                                                         float (&c1)[NC]) {
    for (int idx = threadIdx.x; idx < 3 * NC * 64; idx += nthreads) {
        const int arr = idx / (NC * 64), c = (idx / 64) % NC, col = idx & 63;
        float v;
        if (arr == 0) v = p.att_vec[c][col];
        else if (LN) v = arr == 1 ? p.ln_weight[c][col] : p.ln_bias[c][col];
        else v = arr == 1 ? 1.f : 0.f;
        hl[idx] = v;
    }
    if (threadIdx.x < NC * 64) {
        const int c = threadIdx.x >> 6, col = threadIdx.x & 63;
        float u = p.att_vec[c][col];
        if (LN) u *= p.ln_weight[c][col];
        ul[threadIdx.x] = u;
    }
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        float u = p.att_vec[c][lane];
        c0[c] = LN ? acm_group_sum<64>(p.ln_bias[c][lane] * u) : 0.f;
        if (LN) u *= p.ln_weight[c][lane];
        c1[c] = acm_group_sum<64>(u) * (1.0f / 64.0f);
    }
}

// The head of row m: clamps D in place (channels L, H at lo_a, the MLP channel at lo_m, the structure channel at 0), then
// mean_c, rstd_c (0 and 1 without LayerNorm), gsig_c = sigmoid(s_c) and al = softmax(gsig att_mix / NC).  LayerNorm is folded
// into the attention vector: with d = H - mean,
//   s_c = sum_col (d * rstd * gamma + beta) * v = rstd * sum_col d * u_c + c0_c,   u_c = gamma_c (.) att_vec_c in LDS at ul.
// gq: the caller's acm_opaque(g) -- u depends on the lane only, and hoisted out of the row loop it would pin 48 .. 144 registers.
template <int NC, bool LN>
__device__ __forceinline__ void rows16_head(f32x4 (&D)[NC][4], const float* ul, int gq, const float (&c0)[NC], const float (&mixm)[NC * NC],
                                            float lo_a, float lo_m, float (&mean)[NC], float (&rstd)[NC], float (&gsig)[NC],
                                            float (&al)[NC]) {
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const float lo = c < 2 ? lo_a : (c == 2 ? lo_m : 0.f);
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) D[c][t][r] = fmaxf(D[c][t][r], lo);
        float dot = 0.f;
        if (LN) {
            float s = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) s += (D[c][t][0] + D[c][t][1]) + (D[c][t][2] + D[c][t][3]);
            const float mu = row4_sum(s) * (1.0f / 64.0f);
            float q = 0.f;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(ul + c * 64 + 16 * t + 4 * gq);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float d = D[c][t][r] - mu;
                    q = fmaf(d, d, q);
                    dot = fmaf(d, u[r], dot);
                }
            }
            mean[c] = mu;
            rstd[c] = acm_rsqrt(row4_sum(q) * (1.0f / 64.0f) + ACM_LN_EPS);
            dot = fmaf(rstd[c], row4_sum(dot), c0[c]);
        } else {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const f32x4 u = *reinterpret_cast<const f32x4*>(ul + c * 64 + 16 * t + 4 * gq);
#pragma unroll
                for (int r = 0; r < 4; ++r) dot = fmaf(D[c][t][r], u[r], dot);
            }
            mean[c] = 0.f;
            rstd[c] = 1.f;
            dot = row4_sum(dot);
        }
        gsig[c] = acm_rcp(1.0f + acm_exp(-dot));
    }
    float lg[NC], mx = -INFINITY, den = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        float a = 0.f;
#pragma unroll
        for (int c = 0; c < NC; ++c) a = fmaf(gsig[c], mixm[c * NC + j], a);
        lg[j] = a * (1.0f / NC);
        mx = fmaxf(mx, lg[j]);
    }
#pragma unroll
    for (int j = 0; j < NC; ++j) {
        lg[j] = acm_exp(lg[j] - mx);
        den += lg[j];
    }
    const float inv = acm_rcp(den);
#pragma unroll
    for (int j = 0; j < NC; ++j) al[j] = lg[j] * inv;
}

}  // namespace
