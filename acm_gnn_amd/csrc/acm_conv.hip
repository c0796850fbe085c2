// Forward of the literal ACM layer for gfx950 (MI355X):
//   K2  acm_conv_fwd       one CSR pass over A_low -> all graph channels + adaptive mixing
//       acm_conv_head_fwd  the row-local head alone, behind products the caller has made
//       acm_conv_fwd_tail  output layer + loss + row-local backward in one row pass
// The gathers are those of acm_gather_device.h; the backward (K3, K4) is acm_conv_bwd.hip.
#include "acm_gather_device.h"

struct EpiFwd {
    static constexpr bool kFusedHead = true;
    using Args = acm_conv_fwd_t;
    template <class L, int NG>
    static __device__ __forceinline__ void apply(const Args& p, int row, const L& lay, int F,
                                                 const float (&acc)[NG][L::NV]) {
        constexpr int NV = L::NV;
        float H[4][NV], hn[4][NV], xhat[4][NV], pre[3][NV];
        const float dg = (NG == 3) ? p.deg[row] : 0.f;
        const float rs = p.row_scale ? p.row_scale[row] : 1.f;      // pattern-only operator: A_low = D^-1 P
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = lay.col(i);
            const bool ok = col < F;
            const float zh = ok ? p.s_high[(long)row * p.ld_s_high + col] : 0.f;
            const float zi = ok ? p.s_mlp[(long)row * p.ld_s_mlp + col] : 0.f;
            const float p0 = rs * acc[0][i];
            const float p1 = zh - rs * acc[1][i];
            pre[0][i] = p0;
            pre[1][i] = p1;
            H[0][i] = p.relu_after ? fmaxf(p0, 0.f) : p0;
            H[1][i] = p.relu_after ? fmaxf(p1, 0.f) : p1;
            H[2][i] = p.relu_mlp ? fmaxf(zi, 0.f) : zi;
            if (NG == 3) {
                const float ss = ok ? p.s_struc[(long)row * p.ld_s_struc + col] : 0.f;
                const float p3 = dg * (rs * acc[NG - 1][i]) - ss;
                pre[2][i] = p3;
                H[3][i] = fmaxf(p3, 0.f);
            } else {
                pre[2][i] = 0.f;
                H[3][i] = 0.f;
            }
            if (!ok) {
                H[0][i] = H[1][i] = H[2][i] = H[3][i] = 0.f;
            }
        }
        HeadOut ho;
        const HeadParams hp = acm_head_params(p);
        acm_head<L, NG + 1>(lay, F, p.layernorm, hp, H, hn, xhat, ho);
        const bool st = Owns<L>::lane_stores(lay);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int col = lay.col(i);
            if (col < F && st) {
                float o = ho.alpha[0] * H[0][i] + ho.alpha[1] * H[1][i] + ho.alpha[2] * H[2][i];
                if (NG == 3) o += ho.alpha[3] * H[3][i];
                o *= p.scale;
                if (p.post_relu) o = fmaxf(o, 0.f);
                if (p.post_scale) o *= p.post_scale[(long)row * p.ld_post_scale + col];
                if (p.post_drop.p > 0.f) o *= acm_drop1(acm_drop_ctx(p.post_drop), row, col);
                p.out[(long)row * p.ld_out + col] = o;
                float* pr = p.pre + (long)row * p.ld_pre;
                pr[col] = pre[0][i];
                pr[F + col] = pre[1][i];
                if (NG == 3) pr[2 * F + col] = pre[2][i];
            }
        }
        if (lay.leader()) {
            float4 a4 = make_float4(ho.alpha[0], ho.alpha[1], ho.alpha[2], ho.alpha[3]);
            *reinterpret_cast<float4*>(p.att + (long)row * 4) = a4;
        }
    }
};

// Narrow layers (F <= 8), phase 1 of the fused forward: the raw neighbour sums go to the `pre` buffer; phase 2
// (conv_fwd_rows_kernel) finishes every row with one THREAD per row.  In the narrow gather the whole row sits
// in one lane, so running EpiFwd there leaves 31 of 32 lanes idle through the head's exp / rsqrt chains
// (~40 us of the 110 us F = 2 forward on the twitch graph).
struct EpiRaw {
    static constexpr bool kFusedHead = false;
    using Args = acm_conv_fwd_t;
    template <class L, int NG>
    static __device__ __forceinline__ void apply(const Args& p, int row, const L& lay, int F,
                                                 const float (&acc)[NG][L::NV]) {
        if (!Owns<L>::lane_stores(lay)) return;
        float* pr = p.pre + (long)row * p.ld_pre;
#pragma unroll
        for (int i = 0; i < L::NV; ++i) {
            const int col = lay.col(i);
            if (col < F) {
#pragma unroll
                for (int c = 0; c < NG; ++c) pr[c * F + col] = acc[c][i];
            }
        }
    }
};

template <int FP, int NG>
__global__ __launch_bounds__(256) void conv_fwd_rows_kernel(acm_conv_fwd_t p, int n_rows, CsrView csr,
                                                            const float* __restrict__ partial, int row_blocks) {
    const int F = p.f_out;
    float acc[NG][FP];
    if ((int)blockIdx.x >= row_blocks) {
        // tail blocks: the long rows, whose work items left partial sums in the slots -- a 16-lane group per row,
        // lanes over the slots (slot order within a lane, fixed DPP tree across lanes), then the same head.  This is
        // the fix-up pass of the gather folded into this launch (the two parts do not depend on each other).
        const int m = threadIdx.x & 15;
        const int w = ((int)blockIdx.x - row_blocks) * 16 + (threadIdx.x >> 4);
        if (w >= csr.n_long) return;
        const AcmLongRow lr = csr.long_rows[w];
#pragma unroll
        for (int c = 0; c < NG; ++c)
#pragma unroll
            for (int f = 0; f < FP; ++f) acc[c][f] = 0.f;
        for (int s = lr.slot_begin + m; s < lr.slot_end; s += 16) {
            const float* ps = partial + (long)s * (NG * F);
#pragma unroll
            for (int c = 0; c < NG; ++c)
#pragma unroll
                for (int f = 0; f < FP; ++f)
                    if (f < F) acc[c][f] += ps[c * F + f];
        }
#pragma unroll
        for (int c = 0; c < NG; ++c)
#pragma unroll
            for (int f = 0; f < FP; ++f) acc[c][f] = acm_group_sum<16>(acc[c][f]);
        const LaySerial<FP> lay{m == 0};
        EpiFwd::apply<LaySerial<FP>, NG>(p, lr.row, lay, F, acc);
        return;
    }
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= n_rows) return;
    if (csr.long_index && csr.long_index[row] >= 0) return;      // done by a tail block
    const float* pr = p.pre + (long)row * p.ld_pre;
#pragma unroll
    for (int c = 0; c < NG; ++c)
#pragma unroll
        for (int f = 0; f < FP; ++f) acc[c][f] = (f < F) ? pr[c * F + f] : 0.f;
    const LaySerial<FP> lay{true};
    EpiFwd::apply<LaySerial<FP>, NG>(p, row, lay, F, acc);     // overwrites this row of `pre` with the final values
}

// The row-local head of a wide three-channel layer as a kernel of its own (acm_conv_head_fwd): the channels' pre-activations
// come from products the caller has already made -- pre_L = g_low[row], pre_H = s_high[row] - g_high[row], Z_I = s_mlp[row]
// (the aggregate-first form for wide inputs: functional._AcmAggWide) -- so there is nothing to gather: a 16-lane group takes a
// row (four rows per wave, 16-byte loads), EpiFwd does the rest exactly as behind a gather.
__global__ __launch_bounds__(256) void conv_head_rows_kernel(acm_conv_fwd_t p, int n_rows) {
    const int lane = threadIdx.x & 63, m = lane & 15;
    const int row = ((int)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4 + (lane >> 4);
    if (row >= n_rows) return;                          // (whole 16-lane groups leave: the group sums stay complete)
    constexpr int F = 64;
    // EpiFwd::apply for NG = 2 with 16-byte loads and stores (the arithmetic, statement for statement, is the same)
    const float4 a = *reinterpret_cast<const float4*>(p.g_low + (long)row * p.ld_g_low + 4 * m);
    const float4 b = *reinterpret_cast<const float4*>(p.g_high + (long)row * p.ld_g_high + 4 * m);
    const float4 zh4 = *reinterpret_cast<const float4*>(p.s_high + (long)row * p.ld_s_high + 4 * m);
    const float4 zi4 = *reinterpret_cast<const float4*>(p.s_mlp + (long)row * p.ld_s_mlp + 4 * m);
    const float aa[4] = {a.x, a.y, a.z, a.w}, bb[4] = {b.x, b.y, b.z, b.w};
    const float zh[4] = {zh4.x, zh4.y, zh4.z, zh4.w}, zi[4] = {zi4.x, zi4.y, zi4.z, zi4.w};
    float H[4][4], hn[4][4], xhat[4][4], pre[2][4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float p0 = 1.f * aa[i];
        const float p1 = zh[i] - 1.f * bb[i];
        pre[0][i] = p0, pre[1][i] = p1;
        H[0][i] = p.relu_after ? fmaxf(p0, 0.f) : p0;
        H[1][i] = p.relu_after ? fmaxf(p1, 0.f) : p1;
        H[2][i] = p.relu_mlp ? fmaxf(zi[i], 0.f) : zi[i];
        H[3][i] = 0.f;
    }
    const LayRow16 lay{lane};
    HeadOut ho;
    const HeadParams hp = acm_head_params(p);
    acm_head<LayRow16, 3>(lay, F, p.layernorm, hp, H, hn, xhat, ho);
    float o[4];
    const AcmDropCtx dc = acm_drop_ctx(p.post_drop);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int col = 4 * m + i;
        float v = ho.alpha[0] * H[0][i] + ho.alpha[1] * H[1][i] + ho.alpha[2] * H[2][i];
        v *= p.scale;
        if (p.post_relu) v = fmaxf(v, 0.f);
        if (p.post_scale) v *= p.post_scale[(long)row * p.ld_post_scale + col];
        if (p.post_drop.p > 0.f) v *= acm_drop1(dc, row, col);
        o[i] = v;
    }
    *reinterpret_cast<float4*>(p.out + (long)row * p.ld_out + 4 * m) = make_float4(o[0], o[1], o[2], o[3]);
    float* pr = p.pre + (long)row * p.ld_pre + 4 * m;
    *reinterpret_cast<float4*>(pr) = make_float4(pre[0][0], pre[0][1], pre[0][2], pre[0][3]);
    *reinterpret_cast<float4*>(pr + F) = make_float4(pre[1][0], pre[1][1], pre[1][2], pre[1][3]);
    if (m == 0) *reinterpret_cast<float4*>(p.att + (long)row * 4) = make_float4(ho.alpha[0], ho.alpha[1], ho.alpha[2], ho.alpha[3]);
}

extern "C" int acm_conv_head_fwd(int64_t n_rows, const acm_conv_fwd_t* p, acm_stream_t stream) {
    ACM_REQUIRE(p, ACM_EINVAL, "acm_conv_head_fwd: NULL argument");
    ACM_REQUIRE(n_rows >= 0 && n_rows < INT32_MAX, ACM_ESHAPE, "acm_conv_head_fwd: bad row count");
    ACM_REQUIRE(p->f_out == 64 && p->n_channels == 3 && !p->gather_bf16 && !p->row_scale && !p->deg, ACM_EUNSUPPORTED,
                "acm_conv_head_fwd: three fp32 channels of 64 columns, no row scale (got F %d, k %d)", p->f_out, p->n_channels);
    ACM_REQUIRE(p->g_low && p->g_high && p->s_high && p->s_mlp && p->out && p->pre && p->att && p->att_mix, ACM_EINVAL,
                "acm_conv_head_fwd: NULL pointer in the parameter block");
    const uintptr_t bits = (uintptr_t)p->g_low | (uintptr_t)p->g_high | (uintptr_t)p->s_high | (uintptr_t)p->s_mlp | (uintptr_t)p->out |
                           (uintptr_t)p->pre | (uintptr_t)p->att;
    ACM_REQUIRE((p->ld_g_low | p->ld_g_high | p->ld_s_high | p->ld_s_mlp | p->ld_out | p->ld_pre) % 4 == 0 && (bits & 15) == 0,
                ACM_EUNSUPPORTED, "acm_conv_head_fwd: every row (inputs, out, pre, att) must be 16-byte aligned");
    if (n_rows == 0) return ACM_OK;
    hipLaunchKernelGGL(conv_head_rows_kernel, dim3((unsigned)((n_rows + 15) / 16)), dim3(256), 0, (hipStream_t)stream, *p, (int)n_rows);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_conv_fwd(const acm_csr_t* a, const acm_conv_fwd_t* p, void* workspace,
                            size_t workspace_bytes, acm_stream_t stream) {
    ACM_REQUIRE(a && p, ACM_EINVAL, "acm_conv_fwd: NULL argument");
    const int F = p->f_out, k = p->n_channels;
    ACM_REQUIRE(F > 0 && (k == 3 || k == 4), ACM_ESHAPE, "acm_conv_fwd: f_out %d n_channels %d", F, k);
    ACM_REQUIRE(p->g_low && p->g_high && p->s_high && p->s_mlp && p->out && p->pre && p->att &&
                    p->att_mix, ACM_EINVAL, "acm_conv_fwd: NULL tensor pointer");
    for (int c = 0; c < k; ++c) {
        ACM_REQUIRE(p->att_vec[c], ACM_EINVAL, "acm_conv_fwd: att_vec[%d] is NULL", c);
        ACM_REQUIRE(!p->layernorm || (p->ln_weight[c] && p->ln_bias[c]), ACM_EINVAL,
                    "acm_conv_fwd: layernorm parameters of channel %d are NULL", c);
    }
    ACM_REQUIRE(p->ld_out >= F && p->ld_pre >= (k - 1) * F, ACM_ESHAPE,
                "acm_conv_fwd: ld_out %lld / ld_pre %lld too small", (long long)p->ld_out,
                (long long)p->ld_pre);
    ACM_REQUIRE(((uintptr_t)p->att) % 16 == 0, ACM_EINVAL, "acm_conv_fwd: att must be 16-byte aligned");
    ACM_REQUIRE(k == 3 || (p->g_struc && p->s_struc && p->deg), ACM_EINVAL,
                "acm_conv_fwd: structure channel pointers are NULL");
    const GatherSrc g = {{p->g_low, p->g_high, k == 4 ? p->g_struc : nullptr}, {p->ld_g_low, p->ld_g_high, k == 4 ? p->ld_g_struc : 0}};
    hipStream_t s = (hipStream_t)stream;
    if (F > 8)
        return acm_pick([&](auto kc) {
            return launch_gather<kc() - 1, EpiFwd>(a, g, F, *p, workspace, workspace_bytes, s, "acm_conv_fwd", nullptr, p->gather_bf16 != 0);
        }, acm_k_of(k));
    // narrow layers, two phases: gather raw sums into `pre`, then one thread per row
    ACM_REQUIRE(!p->gather_bf16, ACM_EUNSUPPORTED, "acm_conv_fwd: bf16 operands need F > 8");
    const int st = acm_pick([&](auto kc) {
        return launch_gather<kc() - 1, EpiRaw>(a, g, F, *p, workspace, workspace_bytes, s, "acm_conv_fwd", nullptr, false, true);
    }, acm_k_of(k));
    if (st != ACM_OK || a->n_rows == 0) return st;
    const int grid = (int)((a->n_rows + 255) / 256), n = (int)a->n_rows;
    CsrView cv = acm_view(a);
    const float* part = (const float*)workspace;
    const bool done = narrow_finishes_long_rows(a);     // the gather left complete raw sums for every row
    if (done) cv.long_index = nullptr;
    const int tail = done ? 0 : (int)((a->n_long + 15) / 16);
    acm_pick([&](auto fp, auto kc) {
        hipLaunchKernelGGL((conv_fwd_rows_kernel<fp(), kc() - 1>), dim3(grid + tail), dim3(256), 0, s, *p, n, cv, part, grid);
        return ACM_OK;
    }, acm_fp_of(F), acm_k_of(k));
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

// ================================================================== output layer + loss + K3 in one row pass
// One thread per row, three steps that hand their results to each other through the row's own few bytes of global
// memory (written and read back by the same thread): the head of the narrow forward, the masked NLL of its logits, the
// row-local backward with that gradient.  Block-level reductions: loss partial, K3 parameter partials.
// ROWS (acm_conv_fwd_tail_rows): `keep` marks the rows that carry weight in the loss.  A thread whose row is not kept loads
// nothing and computes nothing: it stores zeros to every per-row output (logits, pre, att, dlogits, G_L, G_H, G_I -- G_H is
// the self term of the transposed gather and G_I feeds the hidden layer's projection backward, so neither may be stale) and
// enters both block reductions with zero accumulators.  Thread <-> row and block <-> 256 rows stay what they are, so the
// partials of a block are the sums they were with the dropped rows' zero terms left out.
template <int FP, int NG, bool ROWS = false>
__global__ __launch_bounds__(256) void conv_tail_rows_kernel(acm_conv_fwd_t pf, acm_loss_t pl, acm_conv_bwd_local_t pb,
                                                             int n_rows, float* __restrict__ loss_partial,
                                                             float* __restrict__ k3_partial, const uint8_t* __restrict__ keep) {
    extern __shared__ float lds[];
    __shared__ float red[256];
    constexpr int K = NG + 1;
    const int F = pf.f_out;
    const int npg = 3 * K * F + K * K;
    const int row = blockIdx.x * 256 + threadIdx.x;
    const bool active = row < n_rows;
    const LaySerial<FP> lay{true};
    ParamAcc<LaySerial<FP>> pa;
    pa.zero();
    float term = 0.f;
    if (ROWS && active && !keep[row]) {
        for (int f = 0; f < F; ++f) {
            pf.out[(long)row * pf.ld_out + f] = 0.f;
            pl.dlogits[(long)row * pl.ld_dlogits + f] = 0.f;
            pb.g_low[(long)row * pb.ld_g_low + f] = 0.f;
            pb.g_high[(long)row * pb.ld_g_high + f] = 0.f;
            pb.g_mlp[(long)row * pb.ld_g_mlp + f] = 0.f;
            for (int c = 0; c < NG; ++c) pf.pre[(long)row * pf.ld_pre + c * F + f] = 0.f;
        }
        *reinterpret_cast<float4*>(pf.att + (long)row * 4) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else if (active) {
        float acc[NG][FP];
        const float* pr = pf.pre + (long)row * pf.ld_pre;
#pragma unroll
        for (int c = 0; c < NG; ++c)
#pragma unroll
            for (int f = 0; f < FP; ++f) acc[c][f] = (f < F) ? pr[c * F + f] : 0.f;
        EpiFwd::apply<LaySerial<FP>, NG>(pf, row, lay, F, acc);
        term = acm_nll_row(F, pf.out + (long)row * pf.ld_out, (int)pl.labels[row], pl.row_weight[row],
                           pl.dlogits + (long)row * pl.ld_dlogits);
        conv_bwd_row<LaySerial<FP>, K>(pb, row, true, lay, pa);      // LaySerial: no cross-lane step, divergence is fine
    }
    red[threadIdx.x] = term;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_partial[blockIdx.x] = red[0];
    bwd_local_block_reduce<LaySerial<FP>, 64, K>(pa, lay, F, lds, k3_partial + (long)blockIdx.x * npg);
}

// The same for 4 < F <= 8 with EIGHT LANES PER ROW (LayPacked<8>: one column per lane, eight rows per wave): the
// thread-per-row form above holds three channels x 8 columns of every stage in registers (169 VGPRs, 3 waves/SIMD) and
// walks a row's head, loss and backward as one serial chain -- 50 us for the 169 k rows of the arXiv-year-shaped graph.
// Here a lane reads back only what it wrote itself (its own logit, its own dlogit), the row-wise max / sums of the loss are
// 8-lane DPP reductions.
__device__ __forceinline__ float acm_group8_max(float v) {
    v = fmaxf(v, acm_dpp<0xB1>(v));      // quad_perm [1,0,3,2]
    v = fmaxf(v, acm_dpp<0x4E>(v));      // quad_perm [2,3,0,1]
    return fmaxf(v, acm_dpp<0x141>(v));  // row_half_mirror
}

template <int NG>
__global__ __launch_bounds__(256) void conv_tail_packed8_kernel(acm_conv_fwd_t pf, acm_loss_t pl, acm_conv_bwd_local_t pb,
                                                                int n_rows, float* __restrict__ loss_partial,
                                                                float* __restrict__ k3_partial) {
    extern __shared__ float lds[];
    __shared__ float red[256];
    constexpr int K = NG + 1;
    using L = LayPacked<8>;
    const int F = pf.f_out;
    const int npg = 3 * K * F + K * K;
    const int lane = threadIdx.x & 63, col = lane & 7;
    const int row = blockIdx.x * 32 + (threadIdx.x >> 3);
    const bool active = row < n_rows;
    const int rr = active ? row : 0;
    const L lay{lane};
    ParamAcc<L> pa;
    pa.zero();
    float term = 0.f;
    {
        float acc[NG][1];
        const float* pr = pf.pre + (long)rr * pf.ld_pre;
#pragma unroll
        for (int c = 0; c < NG; ++c) acc[c][0] = (col < F) ? pr[c * F + col] : 0.f;
        if (active) EpiFwd::apply<L, NG>(pf, rr, lay, F, acc);          // every lane of an active row takes part
        // masked NLL of the row's logits: the lane's own logit back from memory (it wrote it), the rest by reduction
        const bool mine = active && col < F;
        const float z = mine ? pf.out[(long)rr * pf.ld_out + col] : -INFINITY;
        const float wi = active ? pl.row_weight[rr] : 0.f;
        const int yi = active ? (int)pl.labels[rr] : 0;
        const float m = acm_group8_max(z);
        const float e = mine ? expf(z - m) : 0.f;
        const float ssum = acm_group_sum<8>(e);
        const float zy = acm_group_sum<8>((mine && col == yi) ? z : 0.f);
        if (mine) pl.dlogits[(long)rr * pl.ld_dlogits + col] = (wi == 0.f) ? 0.f : wi * (e / ssum - (col == yi ? 1.f : 0.f));
        if (active && col == 0 && wi != 0.f) term = wi * (m + logf(ssum) - zy);
        conv_bwd_row<L, K>(pb, rr, active, lay, pa);
    }
    red[threadIdx.x] = term;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if ((int)threadIdx.x < m) red[threadIdx.x] += red[threadIdx.x + m];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss_partial[blockIdx.x] = red[0];
    bwd_local_block_reduce<L, 8, K>(pa, lay, F, lds, k3_partial + (long)blockIdx.x * npg);
}

extern "C" int acm_conv_fwd_tail_workspace_bytes(int64_t n_rows, int f_out, int n_channels, size_t* bytes) {
    ACM_REQUIRE(bytes, ACM_EINVAL, "acm_conv_fwd_tail_workspace_bytes: NULL argument");
    ACM_REQUIRE(n_rows >= 0 && f_out > 0 && f_out <= 8 && n_channels == 3, ACM_EUNSUPPORTED,
                "acm_conv_fwd_tail: f_out %d n_channels %d (needs f_out <= 8, three channels)", f_out, n_channels);
    const int64_t rows_per_block = f_out > 4 ? 32 : 256;         // 4 < F <= 8: eight lanes per row
    const int64_t nblk = (n_rows + rows_per_block - 1) / rows_per_block > 0 ? (n_rows + rows_per_block - 1) / rows_per_block : 1;
    *bytes = (size_t)nblk * (size_t)(1 + 3 * n_channels * f_out + n_channels * n_channels) * sizeof(float);
    return ACM_OK;
}

// rows: over the operator's loss-row attachment (acm_conv_fwd_tail_rows)
static int conv_fwd_tail(const acm_csr_t* a, const acm_conv_fwd_t* p, const acm_loss_t* l,
                         const acm_conv_bwd_local_t* b, void* workspace, size_t workspace_bytes,
                         void* tail_workspace, size_t tail_workspace_bytes, acm_stream_t stream, bool rows) {
    ACM_REQUIRE(a && p && l && b, ACM_EINVAL, "acm_conv_fwd_tail: NULL argument");
    const int F = p->f_out, k = p->n_channels;
    const AcmLossRows* lr = rows ? a->loss_rows : nullptr;
    if (rows) {
        ACM_REQUIRE(lr, ACM_EUNSUPPORTED, "acm_conv_fwd_tail_rows: the operator has no loss-row list (acm_csr_build_loss_rows)");
        ACM_REQUIRE(F <= 4, ACM_EUNSUPPORTED, "acm_conv_fwd_tail_rows: f_out %d (the thread-per-row tail: f_out <= 4)", F);
    }
    size_t need = 0;
    int st = acm_conv_fwd_tail_workspace_bytes(a->n_rows, F, k, &need);
    if (st != ACM_OK) return st;
    ACM_REQUIRE(l->n_classes == F && b->f_out == F && b->n_channels == k, ACM_EUNSUPPORTED,
                "acm_conv_fwd_tail: the layer's f_out must be the number of classes");
    ACM_REQUIRE(!p->post_relu && !p->post_scale && p->post_drop.p == 0.f && !b->post_relu && !b->post_scale &&
                    b->post_drop.p == 0.f && !p->gather_bf16, ACM_EUNSUPPORTED,
                "acm_conv_fwd_tail: post-ops / bf16 operands are not part of the fused tail");
    ACM_REQUIRE((rows ? lr->n_long : a->n_long) == 0 || narrow_finishes_long_rows(a), ACM_EUNSUPPORTED,
                "acm_conv_fwd_tail: this graph's narrow gather leaves partial sums of long rows");
    ACM_REQUIRE(p->g_low && p->g_high && p->s_high && p->s_mlp && p->out && p->pre && p->att && p->att_mix &&
                    l->labels && l->row_weight && l->loss && l->dlogits && b->att_mix && b->g_low && b->g_high &&
                    b->g_mlp && b->d_att_mix, ACM_EINVAL, "acm_conv_fwd_tail: NULL tensor pointer");
    ACM_REQUIRE(b->grad_out == l->dlogits && b->ld_grad_out == l->ld_dlogits && b->pre == p->pre &&
                    b->ld_pre == p->ld_pre && b->s_mlp == p->s_mlp && b->ld_s_mlp == p->ld_s_mlp, ACM_EINVAL,
                "acm_conv_fwd_tail: bwd must read what fwd / loss write (grad_out = dlogits, pre, s_mlp)");
    ACM_REQUIRE(p->ld_out >= F && p->ld_pre >= (k - 1) * F && l->ld_dlogits >= F && ((uintptr_t)p->att) % 16 == 0,
                ACM_ESHAPE, "acm_conv_fwd_tail: leading dimensions / alignment");
    for (int c = 0; c < k; ++c) {
        ACM_REQUIRE(p->att_vec[c] && b->att_vec[c], ACM_EINVAL, "acm_conv_fwd_tail: att_vec[%d] is NULL", c);
        ACM_REQUIRE(!p->layernorm || (p->ln_weight[c] && p->ln_bias[c] && b->ln_weight[c] && b->ln_bias[c]), ACM_EINVAL,
                    "acm_conv_fwd_tail: layernorm parameters of channel %d are NULL", c);
    }
    ACM_REQUIRE(tail_workspace && tail_workspace_bytes >= need, ACM_ENOMEM,
                "acm_conv_fwd_tail: tail workspace %zu B < required %zu B", tail_workspace_bytes, need);
    if (a->n_rows == 0) return ACM_OK;
    hipStream_t s = (hipStream_t)stream;
    GatherSrc g = {{p->g_low, p->g_high, nullptr}, {p->ld_g_low, p->ld_g_high, 0}};
    if (rows) {
        // the attachment's list in place of the handle's: same column ids, same values, its own items and slot count
        GatherOverride over = {acm_view(a), lr->n_slots};
        over.view.items = lr->items;
        over.view.n_items = (int)lr->n_items;
        over.view.long_rows = lr->long_rows;
        over.view.long_index = lr->long_index;
        over.view.n_long = (int)lr->n_long;
        over.view.n_windows = (int)lr->n_windows;
        over.view.n_multi = (int)lr->n_multi;
        st = launch_gather<2, EpiRaw>(a, g, F, *p, workspace, workspace_bytes, s, "acm_conv_fwd_tail_rows", nullptr, false, true, &over);
    } else {
        st = launch_gather<2, EpiRaw>(a, g, F, *p, workspace, workspace_bytes, s, "acm_conv_fwd_tail", nullptr, false, true);
    }
    if (st != ACM_OK) return st;
    const bool packed = F > 4;             // eight lanes per row (conv_tail_packed8_kernel)
    const int n = (int)a->n_rows, nblk = packed ? (n + 31) / 32 : (n + 255) / 256;
    const int npg = 3 * k * F + k * k;
    float* loss_partial = (float*)tail_workspace;
    float* k3_partial = loss_partial + nblk;
    const size_t lds = (size_t)4 * npg * sizeof(float);
    acm_pick([&](auto fp) {
        if constexpr (fp() == 8)
            hipLaunchKernelGGL((conv_tail_packed8_kernel<2>), dim3(nblk), dim3(256), lds, s, *p, *l, *b, n, loss_partial, k3_partial);
        else if (rows)
            hipLaunchKernelGGL((conv_tail_rows_kernel<fp(), 2, true>), dim3(nblk), dim3(256), lds, s, *p, *l, *b, n, loss_partial, k3_partial,
                               (const uint8_t*)lr->keep);
        else
            hipLaunchKernelGGL((conv_tail_rows_kernel<fp(), 2>), dim3(nblk), dim3(256), lds, s, *p, *l, *b, n, loss_partial, k3_partial,
                               (const uint8_t*)nullptr);
        return ACM_OK;
    }, acm_fp_of(F));
    ACM_CHECK_HIP(hipGetLastError());
    const acm_reduce_seg_t seg = {loss_partial, nblk, 1, 0, 1, l->loss, 1, 0, 0, 0};
    st = acm_reduce_emit(b->defer, &seg, 1, s);
    if (st != ACM_OK) return st;
    return acm_bwd_local_reduce(b, k3_partial, nblk, s);
}

extern "C" int acm_conv_fwd_tail(const acm_csr_t* a, const acm_conv_fwd_t* p, const acm_loss_t* l,
                                 const acm_conv_bwd_local_t* b, void* workspace, size_t workspace_bytes,
                                 void* tail_workspace, size_t tail_workspace_bytes, acm_stream_t stream) {
    return conv_fwd_tail(a, p, l, b, workspace, workspace_bytes, tail_workspace, tail_workspace_bytes, stream, false);
}

extern "C" int acm_conv_fwd_tail_rows(const acm_csr_t* a, const acm_conv_fwd_t* p, const acm_loss_t* l,
                                      const acm_conv_bwd_local_t* b, void* workspace, size_t workspace_bytes,
                                      void* tail_workspace, size_t tail_workspace_bytes, acm_stream_t stream) {
    return conv_fwd_tail(a, p, l, b, workspace, workspace_bytes, tail_workspace, tail_workspace_bytes, stream, true);
}
