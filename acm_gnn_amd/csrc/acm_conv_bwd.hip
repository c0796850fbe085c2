// Backward of the literal ACM layer for gfx950 (MI355X):
//   K3  acm_conv_bwd_local row-local backward of the mixing head (+ parameter-gradient reduction)
//   K4  acm_conv_bwd_spmm  transposed SpMM with the high-pass / structure identities folded in
#include "acm_gather_device.h"

struct EpiBwd {
    static constexpr bool kFusedHead = false;
    using Args = acm_conv_bwd_spmm_t;
    template <class L, int NG>
    static __device__ __forceinline__ void apply(const Args& p, int row, const L& lay, int F,
                                                 const float (&acc)[NG][L::NV]) {
        if (!Owns<L>::lane_stores(lay)) return;
        const float idg = (NG == 3 && p.inv_deg) ? p.inv_deg[row] : 1.f;
        const float ssc = p.self_scale ? p.self_scale[row] : 1.f;   // pattern-only: s_high holds D^-1 G_H
#pragma unroll
        for (int i = 0; i < L::NV; ++i) {
            const int col = lay.col(i);
            if (col >= F) continue;
            float dl = acc[0][i];
            float dh = ssc * p.s_high[(long)row * p.ld_s_high + col] - acc[1][i];
            if (p.mask_low) dl = (p.mask_low[(long)row * p.ld_mask_low + col] > 0.f) ? dl : 0.f;
            if (p.mask_high) dh = (p.mask_high[(long)row * p.ld_mask_high + col] > 0.f) ? dh : 0.f;
            p.dz_low[(long)row * p.ld_dz_low + col] = dl;
            p.dz_high[(long)row * p.ld_dz_high + col] = dh;
            if (NG == 3)
                p.d_struc[(long)row * p.ld_d_struc + col] =
                    acc[NG - 1][i] - p.s_struc[(long)row * p.ld_s_struc + col] * idg;
        }
    }
};

// The three outputs of K4 do not depend on each other, so the wide backward can run ONE CHANNEL PER PASS: a pass then
// gathers 64-column rows (256 B, two cache lines per neighbour) of a table whose hot part -- the hub rows -- is half as
// large as that of the [G_L | G_H] rows, more of it stays in the 4 MB L2 of an XCD, and the single-channel passes take the
// vector form (scripts/probe_wide.py: 2 x 270 us against 610 us for the 128-column gather on the twitch-shaped graph).
struct EpiBwdLow {
    static constexpr bool kFusedHead = false;
    using Args = acm_conv_bwd_spmm_t;
    template <class L, int NG>
    static __device__ __forceinline__ void apply(const Args& p, int row, const L& lay, int F, const float (&acc)[NG][L::NV]) {
        if (!Owns<L>::lane_stores(lay)) return;
#pragma unroll
        for (int i = 0; i < L::NV; ++i) {
            const int col = lay.col(i);
            if (col >= F) continue;
            float dl = acc[0][i];
            if (p.mask_low) dl = (p.mask_low[(long)row * p.ld_mask_low + col] > 0.f) ? dl : 0.f;
            p.dz_low[(long)row * p.ld_dz_low + col] = dl;
        }
    }
};
struct EpiBwdHigh {
    static constexpr bool kFusedHead = false;
    using Args = acm_conv_bwd_spmm_t;
    template <class L, int NG>
    static __device__ __forceinline__ void apply(const Args& p, int row, const L& lay, int F, const float (&acc)[NG][L::NV]) {
        if (!Owns<L>::lane_stores(lay)) return;
        const float ssc = p.self_scale ? p.self_scale[row] : 1.f;
#pragma unroll
        for (int i = 0; i < L::NV; ++i) {
            const int col = lay.col(i);
            if (col >= F) continue;
            float dh = ssc * p.s_high[(long)row * p.ld_s_high + col] - acc[0][i];
            if (p.mask_high) dh = (p.mask_high[(long)row * p.ld_mask_high + col] > 0.f) ? dh : 0.f;
            p.dz_high[(long)row * p.ld_dz_high + col] = dh;
        }
    }
};
struct EpiBwdStruc {
    static constexpr bool kFusedHead = false;
    using Args = acm_conv_bwd_spmm_t;
    template <class L, int NG>
    static __device__ __forceinline__ void apply(const Args& p, int row, const L& lay, int F, const float (&acc)[NG][L::NV]) {
        if (!Owns<L>::lane_stores(lay)) return;
        const float idg = p.inv_deg ? p.inv_deg[row] : 1.f;
#pragma unroll
        for (int i = 0; i < L::NV; ++i) {
            const int col = lay.col(i);
            if (col < F) p.d_struc[(long)row * p.ld_d_struc + col] = acc[0][i] - p.s_struc[(long)row * p.ld_s_struc + col] * idg;
        }
    }
};

// Whether K4 runs one channel per pass.
// wide layers on graphs whose gathered tables exceed the L2: one channel per pass (see EpiBwdLow)
// (acm_tuning_t.bwd_split = 1 / 0 force either form, for tests and A/B measurements)
// Measured (profiles/r02_wide_kernels.jsonl): twitch-shaped (mean degree 82) 640 -> 613 us, with the structure channel
// 1004 -> 899, Penn94-shaped (66) 121 -> 106; arXiv-year-shaped (15) 160 -> 190: short rows pay the per-item cost of
// every pass, so the split needs a mean degree of K4_SPLIT_MIN_ROW.
// bf16 tables (gather_bf16): [G_L | G_H] of a neighbour are 2 x 128 bytes -- what ONE fp32 channel is -- so the fused pass
// keeps the hot set of a single fp32 pass and saves the second walk over the operator (twitch-shaped, F = 64: 430 us in
// two passes, 387 us fused; fp32: 619 us in two passes)
constexpr int K4_SPLIT_MIN_ROW = 32;
static bool conv_bwd_splits(int64_t n_rows, int64_t n_cols, int64_t nnz, int F, bool b16, int want_split) {
    const bool big = (size_t)n_cols * (size_t)F * sizeof(float) > GATHER_L2_BYTES && nnz >= K4_SPLIT_MIN_ROW * n_rows;
    const bool split = want_split == 0 ? false : (want_split == 1 ? true : (big && !b16));
    return F > 8 && F <= 256 && split;
}

// The host-only query of the chooser (acm_hip.h): the same choose_gather_form / choose_gather_fixup / conv_bwd_splits the launches
// call, on sizes and addresses the caller states.  Nothing is dereferenced.
static_assert(GatherForm::NARROW == ACM_GATHER_NARROW && GatherForm::PAIR3 == ACM_GATHER_PAIR3 && GatherForm::VEC16 == ACM_GATHER_VEC16 &&
                  GatherForm::VEC == ACM_GATHER_VEC && GatherForm::PAIR_BF16 == ACM_GATHER_PAIR_BF16 &&
                  GatherForm::PAIR_F32 == ACM_GATHER_PAIR_F32 && GatherForm::WIDE == ACM_GATHER_WIDE,
              "acm_hip.h states the kinds");
static_assert(FIXUP_NONE == ACM_FIXUP_NONE && FIXUP_NARROW == ACM_FIXUP_NARROW && FIXUP_WINDOWS == ACM_FIXUP_WINDOWS &&
                  FIXUP_WIDE == ACM_FIXUP_WIDE, "acm_hip.h states the fix-ups");
extern "C" int acm_gather_form(const acm_gather_query_t* q, acm_gather_form_t* out) {
    ACM_REQUIRE(q && out, ACM_EINVAL, "acm_gather_form: NULL argument");
    const int NG = q->n_gathered, F = q->width;
    ACM_REQUIRE(NG >= 1 && NG <= 3 && F > 0 && q->n_rows >= 0 && q->n_cols >= 0 && q->nnz >= 0 && q->n_long >= 0 && q->n_multi >= 0,
                ACM_ESHAPE, "acm_gather_form: n_gathered %d width %d", NG, F);
    ACM_REQUIRE(F <= 256, ACM_EUNSUPPORTED, "acm_gather_form: F = %d > 256 columns per channel", F);
    const bool b16 = q->bf16 != 0;
    ACM_REQUIRE(!b16 || (F > 8 && F <= 64 && F % 2 == 0), ACM_EUNSUPPORTED,
                "acm_gather_form: bf16 gathered operands are implemented for even 8 < F <= 64");
    static const int32_t some_index = 0;              // (the chooser asks whether the handle has a long index, not what it holds)
    GatherSrc g = {{nullptr, nullptr, nullptr}, {0, 0, 0}};
    for (int c = 0; c < NG; ++c) {
        g.p[c] = reinterpret_cast<const float*>((uintptr_t)q->table[c]);
        g.ld[c] = (long)q->ld[c];
    }
    const GatherForm f = choose_gather_form(q->n_rows, q->n_cols, q->nnz, q->n_long, q->has_long_index ? &some_index : nullptr, g, NG, F,
                                            b16, acm_tuning().wide_form, q->fused_head != 0);
    out->kind = (int32_t)f.kind;
    out->lanes = f.lanes;
    out->vecmask = f.vecmask;
    out->merged = f.merged ? 1 : 0;
    out->f_arg = gather_form_f_arg(f, F);
    out->fixup = (int32_t)choose_gather_fixup(F, q->n_rows, q->nnz, q->n_long, q->n_multi);
    out->k4_split = conv_bwd_splits(q->n_rows, q->n_cols, q->nnz, F, b16, acm_tuning().bwd_split) ? 1 : 0;
    return ACM_OK;
}

extern "C" int acm_conv_bwd_spmm(const acm_csr_t* at, const acm_conv_bwd_spmm_t* p, void* workspace,
                                 size_t workspace_bytes, acm_stream_t stream) {
    ACM_REQUIRE(at && p, ACM_EINVAL, "acm_conv_bwd_spmm: NULL argument");
    const int F = p->f_out;
    ACM_REQUIRE(F > 0, ACM_ESHAPE, "acm_conv_bwd_spmm: f_out %d", F);
    ACM_REQUIRE(p->g_low && p->g_high && p->s_high && p->dz_low && p->dz_high, ACM_EINVAL,
                "acm_conv_bwd_spmm: NULL tensor pointer");
    if (p->g_struc) ACM_REQUIRE(p->s_struc && p->d_struc, ACM_EINVAL, "acm_conv_bwd_spmm: structure channel pointers are NULL");
    const bool b16 = p->gather_bf16 != 0;             // launch_gather checks the shape (even 8 < F <= 64) and alignment
    if (conv_bwd_splits(at->n_rows, at->n_cols, at->nnz, F, b16, acm_tuning().bwd_split)) {
        hipStream_t s = (hipStream_t)stream;
        GatherSrc gl = {{p->g_low, nullptr, nullptr}, {p->ld_g_low, 0, 0}};
        int st = launch_gather<1, EpiBwdLow>(at, gl, F, *p, workspace, workspace_bytes, s, "acm_conv_bwd_spmm", nullptr, b16);
        if (st != ACM_OK) return st;
        GatherSrc gh = {{p->g_high, nullptr, nullptr}, {p->ld_g_high, 0, 0}};
        st = launch_gather<1, EpiBwdHigh>(at, gh, F, *p, workspace, workspace_bytes, s, "acm_conv_bwd_spmm", nullptr, b16);
        if (st != ACM_OK || !p->g_struc) return st;
        GatherSrc gs = {{p->g_struc, nullptr, nullptr}, {p->ld_g_struc, 0, 0}};
        return launch_gather<1, EpiBwdStruc>(at, gs, F, *p, workspace, workspace_bytes, s, "acm_conv_bwd_spmm", nullptr, b16);
    }
    if (p->g_struc) {
        GatherSrc g = {{p->g_low, p->g_high, p->g_struc}, {p->ld_g_low, p->ld_g_high, p->ld_g_struc}};
        return launch_gather<3, EpiBwd>(at, g, F, *p, workspace, workspace_bytes, (hipStream_t)stream,
                                        "acm_conv_bwd_spmm", nullptr, b16);
    }
    GatherSrc g = {{p->g_low, p->g_high, nullptr}, {p->ld_g_low, p->ld_g_high, 0}};
    return launch_gather<2, EpiBwd>(at, g, F, *p, workspace, workspace_bytes, (hipStream_t)stream,
                                    "acm_conv_bwd_spmm", nullptr, b16);
}

// ================================================================== K3: row-local backward
// K3, one launch: rows -> accumulators -> bwd_local_block_reduce -> partial[block][npg].
template <class L, int RPW /* rows per wave */, int K>
__global__ __launch_bounds__(256) void conv_bwd_local_kernel(acm_conv_bwd_local_t p, int n_rows,
                                                             float* __restrict__ partial) {
    extern __shared__ float lds[];
    constexpr int k = K;
    const int F = p.f_out;
    const int npg = 3 * k * F + k * k;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    L lay{lane};
    ParamAcc<L> pa;
    pa.zero();
    const int rows_per_block = 4 * RPW;
    for (int r0 = blockIdx.x * rows_per_block; r0 < n_rows; r0 += gridDim.x * rows_per_block) {
        const int row = r0 + wv * RPW + (RPW > 1 ? lane / (64 / RPW) : 0);
        conv_bwd_row<L, K>(p, row < n_rows ? row : 0, row < n_rows, lay, pa);
    }
    bwd_local_block_reduce<L, RPW, K>(pa, lay, F, lds, partial + (long)blockIdx.x * npg);
}

// K3 for 16 < F <= 64: four rows per wave (16 lanes x 4 columns), head parameters in LDS, two passes per
// row (scalars, then one channel at a time).  Same partial-vector layout as conv_bwd_local_kernel, so the
// same reduce kernel finishes the job.  (The one-row-per-wave version spent 270-370 us here on the
// twitch-sized graph: every lane recomputed the row scalars and the compiler parked the loop-invariant
// parameter loads in ~36 VGPRs.)
template <int K>
__global__ __launch_bounds__(256) void conv_bwd_local_grouped_kernel(acm_conv_bwd_local_t p, int n_rows,
                                                                     float* __restrict__ partial) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m = lane & 15, g = lane >> 4;
    const int F = p.f_out;
    const int npg = 3 * K * F + K * K;
    float* hlds = lds;                                   // 3 * K * 64 floats, dead after the row loop
    stage_head_params<K>(hlds, p.att_vec, p.ln_weight, p.ln_bias, p.layernorm, F);
    __syncthreads();
    float pA[K][4], pS[K], dmix1 = 0.f, mixm[K * K];     // head-parameter accumulators (see row_channel_backward)
    const int qc = (m < K * K ? m : 0) / K, qj = (m < K * K ? m : 0) % K;    // the att_mix element this lane accumulates
#pragma unroll
    for (int c = 0; c < K; ++c) {
        pS[c] = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) pA[c][i] = 0.f;
    }
#pragma unroll
    for (int q = 0; q < K * K; ++q) {
        mixm[q] = p.att_mix[q];
    }
    const bool ln = p.layernorm != 0;
    for (int r0 = (blockIdx.x * 4 + wv) * 4; r0 < n_rows; r0 += gridDim.x * 16) {
        const int row = r0 + g;
        const bool active = row < n_rows;
        const long rr = active ? row : 0;
        // 32-bit element offsets from the (uniform) base pointers: one VGPR per array instead of a
        // loop-carried 64-bit pointer per access (the host checks n_rows * ld < 2^31)
        const unsigned urow = (unsigned)rr;
        const int mm = acm_opaque(m);             // see acm_opaque(): keeps the LDS parameter reads in the loop
        float H[K][4], dO[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int col = m + 16 * i;
            const bool ok = active && col < F;
            const unsigned cc = ok ? (unsigned)col : 0u;          // clamped: loads stay unconditional (no exec branches)
            const unsigned o_pre = urow * (unsigned)p.ld_pre + cc;
            const float p0 = p.pre[o_pre], p1 = p.pre[o_pre + F];
            const float zi = p.s_mlp[urow * (unsigned)p.ld_s_mlp + cc];
            const float go = p.grad_out[urow * (unsigned)p.ld_grad_out + cc];
            H[0][i] = ok ? (p.relu_after ? fmaxf(p0, 0.f) : p0) : 0.f;
            H[1][i] = ok ? (p.relu_after ? fmaxf(p1, 0.f) : p1) : 0.f;
            H[2][i] = ok ? (p.relu_mlp ? fmaxf(zi, 0.f) : zi) : 0.f;
            if (K == 4) H[K - 1][i] = ok ? fmaxf(p.pre[o_pre + 2 * F], 0.f) : 0.f;
            dO[i] = ok ? go : 0.f;
        }
        RowHead<K> rh;
        row_head<K>(hlds, mixm, mm, F, ln, H, rh);
        row_post_backward<K>(p, rh, H, active, rr, m, F, dO);
        float ds[K];
        row_head_backward_scalars<K>(rh, mixm, p.scale, H, dO, ds, qc, qj, dmix1);
        const float dg = (K == 4 && active && p.deg) ? p.deg[rr] : 1.f;
        const float gsc = (active && p.g_scale) ? p.g_scale[rr] : 1.f;
#pragma unroll
        for (int c = 0; c < K; ++c) {
            const bool relu_c = (c < 2) ? (p.relu_after != 0) : (c == 2 ? p.relu_mlp != 0 : true);
            float G[4];
            row_channel_backward<K>(hlds, c, mm, F, ln, p.scale, rh, ds[c], H[c], dO, pA[c], pS[c], G);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int col = m + 16 * i;
                if (!(active && col < F)) continue;
                const float gv = (!relu_c || H[c][i] > 0.f) ? G[i] : 0.f;
                if (c == 0) p.g_low[urow * (unsigned)p.ld_g_low + col] = gsc * gv;
                if (c == 1) p.g_high[urow * (unsigned)p.ld_g_high + col] = gsc * gv;
                if (c == 2) p.g_mlp[urow * (unsigned)p.ld_g_mlp + col] = gv;
                if (c == 3) p.g_struc[urow * (unsigned)p.ld_g_struc + col] = dg * gv;
            }
        }
    }
    float dv[K][4], dgam[K][4], dbet[K][4];
#pragma unroll
    for (int c = 0; c < K; ++c) {
#pragma unroll
        for (int i = 0; i < 4; ++i) pA[c][i] = acm_cross_row_sum(pA[c][i]);
        pS[c] = acm_cross_row_sum(pS[c]);
        row_param_grads<K>(hlds, c, m, pA[c], pS[c], dv[c], dgam[c], dbet[c]);      // hlds is still intact here
    }
    dmix1 = acm_cross_row_sum(dmix1);
    __syncthreads();
    float* slab = lds + wv * npg;
    if (g == 0) {
#pragma unroll
        for (int c = 0; c < K; ++c)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int col = m + 16 * i;
                if (col < F) {
                    slab[(0 * K + c) * F + col] = dv[c][i];
                    slab[(1 * K + c) * F + col] = dgam[c][i];
                    slab[(2 * K + c) * F + col] = dbet[c][i];
                }
            }
    }
    if (g == 0 && m < K * K) slab[3 * K * F + m] = dmix1;
    __syncthreads();
    for (int q = threadIdx.x; q < npg; q += 256)
        partial[(long)blockIdx.x * npg + q] = (lds[q] + lds[npg + q]) + (lds[2 * npg + q] + lds[3 * npg + q]);
}

namespace {
int bwd_local_blocks(int64_t n_rows, int rows_per_block) {
    int64_t nb = (n_rows + rows_per_block - 1) / rows_per_block;
    if (nb > 1024) nb = 1024;
    if (nb < 1) nb = 1;
    return (int)nb;
}

int bwd_rows_per_wave(int F) { return F > 64 ? 1 : (F > 16 ? 4 : (F > 8 ? 4 : (F > 4 ? 8 : (F > 2 ? 16 : 32)))); }
}  // namespace

// Second phase of K3: the [d att_vec | d ln_weight | d ln_bias] (k x F each) | d att_mix (k x k) columns of the
// per-block partials go to up to 3k + 1 destinations.
int acm_bwd_local_reduce(const acm_conv_bwd_local_t* p, const float* partial, int nblk, hipStream_t st) {
    const int F = p->f_out, k = p->n_channels, npg = 3 * k * F + k * k;
    acm_reduce_seg_t segs[13];
    int n = 0;
    for (int which = 0; which < 3; ++which)
        for (int c = 0; c < k; ++c) {
            float* dst = which == 0 ? p->d_att_vec[c] : (which == 1 ? p->d_ln_weight[c] : p->d_ln_bias[c]);
            if (dst) segs[n++] = {partial, nblk, npg, (which * k + c) * F, F, dst, F, 0, 0, 0};
        }
    segs[n++] = {partial, nblk, npg, 3 * k * F, k * k, p->d_att_mix, k * k, 0, 0, 0};
    return acm_reduce_emit(p->defer, segs, n, st);
}

extern "C" int acm_conv_bwd_local_workspace_bytes(int64_t n_rows, int f_out, int n_channels, size_t* bytes) {
    ACM_REQUIRE(bytes, ACM_EINVAL, "acm_conv_bwd_local_workspace_bytes: NULL argument");
    ACM_REQUIRE(f_out > 0 && (n_channels == 3 || n_channels == 4), ACM_ESHAPE,
                "acm_conv_bwd_local_workspace_bytes: f_out %d n_channels %d", f_out, n_channels);
    const int npg = 3 * n_channels * f_out + n_channels * n_channels;
    *bytes = (size_t)bwd_local_blocks(n_rows, 4 * bwd_rows_per_wave(f_out)) * npg * sizeof(float);
    return ACM_OK;
}

extern "C" int acm_conv_bwd_local(int64_t n_rows, const acm_conv_bwd_local_t* p, void* workspace,
                                  size_t workspace_bytes, acm_stream_t stream) {
    ACM_REQUIRE(p, ACM_EINVAL, "acm_conv_bwd_local: NULL argument");
    const int F = p->f_out, k = p->n_channels;
    ACM_REQUIRE(F > 0 && F <= 256 && (k == 3 || k == 4), (F > 256 ? ACM_EUNSUPPORTED : ACM_ESHAPE),
                "acm_conv_bwd_local: f_out %d n_channels %d", F, k);
    ACM_REQUIRE(p->grad_out && p->pre && p->s_mlp && p->att_mix && p->g_low && p->g_high && p->g_mlp &&
                    p->d_att_mix, ACM_EINVAL, "acm_conv_bwd_local: NULL tensor pointer");
    ACM_REQUIRE(k == 3 || p->g_struc, ACM_EINVAL,
                "acm_conv_bwd_local: structure channel pointers are NULL");
    for (int c = 0; c < k; ++c) {
        ACM_REQUIRE(p->att_vec[c] && p->d_att_vec[c], ACM_EINVAL, "acm_conv_bwd_local: att_vec[%d] NULL", c);
        ACM_REQUIRE(!p->layernorm || (p->ln_weight[c] && p->ln_bias[c] && p->d_ln_weight[c] && p->d_ln_bias[c]),
                    ACM_EINVAL, "acm_conv_bwd_local: layernorm pointers of channel %d NULL", c);
    }
    size_t need = 0;
    acm_conv_bwd_local_workspace_bytes(n_rows, F, k, &need);
    ACM_REQUIRE(workspace && workspace_bytes >= need, ACM_ENOMEM,
                "acm_conv_bwd_local: workspace %zu B < required %zu B", workspace_bytes, need);
    const int npg = 3 * k * F + k * k;
    const int rpw = bwd_rows_per_wave(F);
    const int nblk = bwd_local_blocks(n_rows, 4 * rpw);
    size_t lds = (size_t)4 * npg * sizeof(float);
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)workspace;
    if (F == 64 && k == 3) {                      // sixteen rows per wave, 16-byte accesses (acm_conv_local16.hip)
        const int nb16 = acm_bwd_local16(p, n_rows, partial, nblk, st);
        if (nb16 < 0) return -nb16;
        if (nb16 > 0) return acm_bwd_local_reduce(p, partial, nb16, st);
    }
    if (F > 16 && F <= 64) {                      // 4-rows-per-wave lean kernel
        const int64_t max_ld = p->ld_pre > p->ld_grad_out ? p->ld_pre : p->ld_grad_out;
        ACM_REQUIRE(n_rows * (max_ld > p->ld_g_mlp ? max_ld : p->ld_g_mlp) < (int64_t)INT32_MAX, ACM_EUNSUPPORTED,
                    "acm_conv_bwd_local: rows x leading dimension exceeds 2^31");
        const size_t hl = (size_t)3 * k * 64 * sizeof(float);
        if (hl > lds) lds = hl;
        acm_pick([&](auto kc) {
            hipLaunchKernelGGL((conv_bwd_local_grouped_kernel<kc()>), dim3(nblk), dim3(256), lds, st, *p, (int)n_rows, partial);
            return ACM_OK;
        }, acm_k_of(k));
        ACM_CHECK_HIP(hipGetLastError());
        return acm_bwd_local_reduce(p, partial, nblk, st);
    }
    auto launch = [&](auto lay, auto rpw) {
        acm_pick([&](auto kc) {
            hipLaunchKernelGGL((conv_bwd_local_kernel<decltype(lay), rpw(), kc()>), dim3(nblk), dim3(256), lds, st, *p, (int)n_rows, partial);
            return ACM_OK;
        }, acm_k_of(k));
    };
    if (F > 128) launch(LayWide<4>{}, acm_int<1>{});
    else if (F > 64) launch(LayWide<2>{}, acm_int<1>{});
    else if (F > 8) launch(LayPacked<16>{}, acm_int<4>{});
    else if (F > 4) launch(LayPacked<8>{}, acm_int<8>{});
    else if (F > 2) launch(LayPacked<4>{}, acm_int<16>{});
    else launch(LayPacked<2>{}, acm_int<32>{});
    ACM_CHECK_HIP(hipGetLastError());
    return acm_bwd_local_reduce(p, partial, nblk, st);
}
