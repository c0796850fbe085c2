// acm_gcn_fwd / acm_gcn_bwd: the graph side of a ONE-channel layer -- the GCN / SGC baselines of the synthetic study
// (synthetic-experiments/baseline_models/layers.py:122-124, models.py:29-33) -- as two epilogues of the gather family
// (acm_gather_device.h).  Neither epilogue is linear, so a row longer than `chunk` gets it ONCE, on the combined sum: the
// fix-up kernels of the family (and the narrow gather's in-LDS combine) call Epi::apply after adding the pieces in slot order.
//
//   EpiGcnFwd   Y = drop(relu?(row_scale * (A Z))), mask regenerated from acm_dropout_t (global row, column, tag, step), and
//               optionally Z_next = Y W_next for f_next <= 8: the row is in registers, one dot product per output column,
//               reduced over the lanes that share the row (layout's rsum: DPP / permlane, no LDS).  W_next (at most
//               256 x 8 floats) is read through the cache: the epilogue runs under divergent control flow in the narrow and
//               fix-up kernels (one group of a wave finishes a row while its neighbours do not), where a workgroup barrier
//               -- which staging it in LDS needs -- is not allowed.
//   EpiGcnBwd   dZ = A^T dY for a narrow dY (the output layer), then row-locally the backward of the layer below:
//               G[r, :] = (dZ[r] W2^T) * keep_scale [H[r, :] > 0]   and the partial sums of dW2 = H^T dZ.
//               Every 8 / 16 / 32-lane group of the narrow gather owns one slab of the partial buffer: it adds the rows it
//               finishes into it in its own program order (item -> group is a static assignment), the slabs are summed by
//               the deferred-reduction pass in a fixed order -- deterministic, no float atomics.
#include "acm_gather_device.h"

namespace {

struct EpiGcnFwd {
    static constexpr bool kFusedHead = false;
    // More than 8 columns only.  In the narrow gather this parameter block stayed in scalar registers across the persistent
    // loop: SGPR spills and a wave per SIMD less than EpiPlain's instantiations.  acm_gcn_fwd answers a plain narrow product with
    // acm_spmm's own kernels and refuses a narrow one with a post-op (the caller composes it).
    static constexpr bool kWideOnly = true;
    struct Args {
        float* y;
        long ldy;
        int relu, col0;               // col0: first column of this block of <= 256 (the mask is a function of the global column)
        const float* row_scale;       // implicit form A = diag(row_scale) P (NULL = 1)
        acm_dropout_t drop;
        const float* w_next;          // [width, f_next], NULL / f_next = 0: none
        long ld_w;
        int f_next;
        float* z_next;
        long ld_zn;
    };
    template <class L, int NG>
    static __device__ __forceinline__ void apply(const Args& a, int row, const L& lay, int F, const float (&acc)[NG][L::NV]) {
        const float os = a.row_scale ? a.row_scale[row] : 1.f;
        const AcmDropCtx dc = acm_drop_ctx(a.drop);
        const bool stores = Owns<L>::lane_stores(lay);
        float v[L::NV];
#pragma unroll
        for (int i = 0; i < L::NV; ++i) {
            const int col = lay.col(i);
            const bool ok = col < F;
            float t = os * acc[0][i];
            if (a.relu) t = fmaxf(t, 0.f);
            if (dc.on && ok) t *= acm_drop1(dc, row, a.col0 + col);
            v[i] = ok ? t : 0.f;                 // (columns beyond F: whatever the block fetch left there)
            if (ok && stores) a.y[(long)row * a.ldy + col] = t;
        }
        if (a.f_next > 0) {
            for (int j = 0; j < a.f_next; ++j) {          // uniform trip count
                float part = 0.f;
#pragma unroll
                for (int i = 0; i < L::NV; ++i) {
                    const int col = lay.col(i);
                    if (col < F) part = fmaf(v[i], a.w_next[(long)(a.col0 + col) * a.ld_w + j], part);
                }
                const float t = lay.rsum(part);
                if (stores && lay.leader()) a.z_next[(long)row * a.ld_zn + j] = t;
            }
        }
    }
};

// What EpiGcnBwd needs, in DEVICE memory (the head of the call's workspace, written by gcn_bwd_prepare_kernel, which also
// zeroes the slabs): as kernel arguments these 21 dwords stayed in scalar registers across the persistent gather loop -- SGPR
// spills, and a wave per SIMD less than EpiPlain's instantiations.  The epilogue reads them where it runs.
struct GcnBwdRec {
    const float* h;               // stored forward output of the layer below [n_rows, hidden]: both masks are read off it
    long ldh;
    const float* w2;              // [hidden, F]
    long ldw2;
    float keep_scale;
    int relu, hidden;
    float* g;
    long ldg;
    float* dz;                    // optional
    long lddz;
    float* part;                  // dW2 partial sums: [group of 32 elements][slab][32], element = h * F + c
    long group_stride;            // floats between two groups of 32 elements (= slabs * 32)
};

struct EpiGcnBwd {
    struct Args {
        const GcnBwdRec* rec;
        int gs, slab_base;            // lanes per gather group of THIS launch; its first slab
    };
    template <class L, int NG>
    static __device__ __forceinline__ void apply(const Args& k, int row, const L&, int F, const float (&acc)[NG][L::NV]) {
        // every lane of the group holds the whole row dZ[row] (LaySerial); lane gl takes the hidden columns gl, gl + gs, ...
        const GcnBwdRec a = *k.rec;
        const int tid = blockIdx.x * 256 + threadIdx.x;
        const int gl = tid % k.gs;
        float* ps = a.part + (long)(k.slab_base + tid / k.gs) * 32;
        if (gl == 0 && a.dz) {
#pragma unroll
            for (int c = 0; c < L::NV; ++c)
                if (c < F) a.dz[(long)row * a.lddz + c] = acc[0][c];
        }
        for (int hc = gl; hc < a.hidden; hc += k.gs) {
            const float hv = a.h[(long)row * a.ldh + hc];
            float dh = 0.f;
#pragma unroll
            for (int c = 0; c < L::NV; ++c)
                if (c < F) dh = fmaf(acc[0][c], a.w2[(long)hc * a.ldw2 + c], dh);
            // acm_bias_act_bwd's rule: kept and active iff H > 0; without a ReLU a dropped element is an exact zero
            float gv = dh;
            if (a.relu) gv = hv > 0.f ? dh * a.keep_scale : 0.f;
            else if (a.keep_scale != 1.f) gv = hv != 0.f ? dh * a.keep_scale : 0.f;
            a.g[(long)row * a.ldg + hc] = gv;
#pragma unroll
            for (int c = 0; c < L::NV; ++c)
                if (c < F) {
                    const int q = hc * F + c;
                    float* p = ps + (long)(q >> 5) * a.group_stride + (q & 31);
                    *p = fmaf(hv, acc[0][c], *p);       // this lane alone ever touches the address: program order
                }
        }
    }
};

__global__ __launch_bounds__(256) void gcn_bwd_prepare_kernel(GcnBwdRec r, GcnBwdRec* dst, float4* slabs, long n4) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *dst = r;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < n4; q += (long)gridDim.x * 256) slabs[q] = make_float4(0.f, 0.f, 0.f, 0.f);
}

constexpr size_t GCN_BWD_REC_BYTES = 256;     // the record's place in the workspace (keeps the slabs 16-byte aligned)
constexpr int GCN_BWD_MAX_BLOCKS = 256;       // gather blocks of acm_gcn_bwd: every group owns a slab the second phase reads
constexpr int GCN_BWD_MAX_HIDDEN = 256;       // bounds the slabs: at most 64 groups x (256 x 32 + fix-up) slabs x 128 B

struct GcnBwdPlan {
    int gs, grid, fix_blocks;                 // lanes per item, gather blocks, fix-up blocks (16 groups each)
    long slabs, groups;                       // slabs of the dW2 partial buffer; groups of 32 elements
    size_t gather_bytes, partial_bytes;
};

GcnBwdPlan gcn_bwd_plan(const acm_csr* a, int width, int hidden) {
    GcnBwdPlan p;
    p.gs = narrow_lanes(a->n_rows, a->nnz);
    // 5..8 columns with sixteen lanes per item: that instantiation (the in-LDS combine keeps the row and the epilogue's dot
    // products live together: 70 VGPRs, 103 SGPRs) would run 7 waves per SIMD where EpiPlain's runs 8; thirty-two lanes keep 8
    if (acm_fp(width) == 8 && p.gs == 16) p.gs = 32;
    const int gpb = 256 / p.gs;
    long grid = (a->n_items + gpb - 1) / gpb;
    if (grid > GCN_BWD_MAX_BLOCKS) grid = GCN_BWD_MAX_BLOCKS;
    if (grid < 1) grid = 1;
    p.grid = (int)grid;
    // sixteen lanes per item: the gather finishes the long rows itself, except the rows of several windows
    const bool fix = p.gs == ACM_WINDOW ? a->n_multi > 0 : a->n_long > 0;
    p.fix_blocks = fix ? (int)((a->n_long + 15) / 16) : 0;
    p.slabs = (long)p.grid * gpb + (long)p.fix_blocks * 16;
    p.groups = ((long)hidden * width + 31) / 32;
    p.gather_bytes = (((size_t)a->n_slots * (size_t)width * sizeof(float)) + 255) / 256 * 256;
    p.partial_bytes = (size_t)p.groups * (size_t)p.slabs * 32 * sizeof(float);
    return p;
}

int check_drop(const acm_dropout_t& d, const char* who) {
    ACM_REQUIRE(d.p == 0.f || (d.p > 0.f && d.p < 1.f && d.step), ACM_EINVAL, "%s: bad dropout spec", who);
    return ACM_OK;
}

}  // namespace

extern "C" int acm_gcn_fwd(const acm_csr_t* a, const acm_gcn_fwd_t* p, void* workspace, size_t workspace_bytes,
                           acm_stream_t stream) {
    ACM_REQUIRE(p, ACM_EINVAL, "acm_gcn_fwd: NULL parameter block");
    ACM_REQUIRE(p->width > 0 && p->ld_z >= p->width && p->ld_y >= p->width, ACM_ESHAPE,
                "acm_gcn_fwd: width %d ld_z %lld ld_y %lld", p->width, (long long)p->ld_z, (long long)p->ld_y);
    ACM_REQUIRE(p->f_next >= 0 && p->f_next <= 8, ACM_EUNSUPPORTED, "acm_gcn_fwd: f_next %d (the fused projection takes 0..8 columns)",
                p->f_next);
    ACM_REQUIRE(p->f_next == 0 || p->width <= 256, ACM_EUNSUPPORTED, "acm_gcn_fwd: the fused projection needs width <= 256 (got %d)",
                p->width);
    ACM_REQUIRE(p->f_next == 0 || (p->ld_w_next >= p->f_next && p->ld_z_next >= p->f_next), ACM_ESHAPE,
                "acm_gcn_fwd: ld_w_next %lld ld_z_next %lld below f_next %d", (long long)p->ld_w_next, (long long)p->ld_z_next, p->f_next);
    ACM_REQUIRE(a && p->z && p->y && (p->f_next == 0 || (p->w_next && p->z_next)), ACM_EINVAL, "acm_gcn_fwd: NULL argument");
    const int st = check_drop(p->drop, "acm_gcn_fwd");
    if (st != ACM_OK) return st;
    if (!p->relu && p->drop.p == 0.f && p->f_next == 0) {  // no post-op: acm_spmm_ex itself (the same kernels, any width)
        const acm_spmm_opts_t o = {nullptr, p->row_scale, nullptr, 0, nullptr, 0, 0};
        return acm_spmm_internal(a, p->z, p->ld_z, p->width, p->y, p->ld_y, &o, workspace, workspace_bytes, stream, nullptr);
    }
    ACM_REQUIRE(p->width > 8, ACM_EUNSUPPORTED, "acm_gcn_fwd: a post-op (ReLU / dropout / next projection) needs more than 8 columns "
                "(got %d): compose acm_spmm_ex + acm_bias_act + acm_gemm", p->width);
    int wd = 0;
    for (int c0 = 0; c0 < p->width; c0 += wd) {           // column blocks of <= 256, none of 8 columns or fewer
        const int left = p->width - c0;
        wd = left <= 256 ? left : (left - 256 <= 8 ? 128 : 256);
        const GatherSrc g = {{p->z + c0, nullptr, nullptr}, {(long)p->ld_z, 0, 0}};
        const EpiGcnFwd::Args ea = {p->y + c0, (long)p->ld_y, p->relu, c0, p->row_scale, p->drop,
                                    p->f_next ? p->w_next : nullptr, (long)p->ld_w_next, p->f_next, p->z_next, (long)p->ld_z_next};
        const int rc = launch_gather<1, EpiGcnFwd>(a, g, wd, ea, workspace, workspace_bytes, (hipStream_t)stream, "acm_gcn_fwd");
        if (rc != ACM_OK) return rc;
    }
    return ACM_OK;
}

static int gcn_bwd_check(const acm_gcn_bwd_t* p) {
    ACM_REQUIRE(p, ACM_EINVAL, "acm_gcn_bwd: NULL parameter block");
    ACM_REQUIRE(p->width >= 1 && p->width <= 8, ACM_EUNSUPPORTED,
                "acm_gcn_bwd: width %d (a narrow dY of 1..8 columns; wider layers compose acm_spmm_ex and the GEMMs)", p->width);
    ACM_REQUIRE(p->hidden >= 1 && p->hidden <= GCN_BWD_MAX_HIDDEN, ACM_EUNSUPPORTED, "acm_gcn_bwd: hidden %d (1..%d)", p->hidden,
                GCN_BWD_MAX_HIDDEN);
    return ACM_OK;
}

extern "C" int acm_gcn_bwd_workspace_bytes(const acm_csr_t* a_t, int width, int hidden, size_t* bytes) {
    const acm_gcn_bwd_t shape = {width, hidden};
    const int st = gcn_bwd_check(&shape);
    if (st != ACM_OK) return st;
    ACM_REQUIRE(a_t && bytes, ACM_EINVAL, "acm_gcn_bwd_workspace_bytes: NULL argument");
    const GcnBwdPlan pl = gcn_bwd_plan(a_t, width, hidden);
    *bytes = pl.gather_bytes + GCN_BWD_REC_BYTES + pl.partial_bytes;
    return ACM_OK;
}

extern "C" int acm_gcn_bwd(const acm_csr_t* a, const acm_gcn_bwd_t* p, void* workspace, size_t workspace_bytes,
                           acm_stream_t stream) {
    int st = gcn_bwd_check(p);
    if (st != ACM_OK) return st;
    ACM_REQUIRE(p->ld_dy >= p->width && p->ld_h >= p->hidden && p->ld_g >= p->hidden && p->ld_w2 >= p->width &&
                    p->ld_dw2 >= p->width && (!p->dz || p->ld_dz >= p->width) && p->keep_scale >= 1.f, ACM_ESHAPE,
                "acm_gcn_bwd: leading dimensions (ld_dy %lld ld_h %lld ld_g %lld ld_w2 %lld ld_dw2 %lld ld_dz %lld) / keep_scale",
                (long long)p->ld_dy, (long long)p->ld_h, (long long)p->ld_g, (long long)p->ld_w2, (long long)p->ld_dw2,
                (long long)p->ld_dz);
    ACM_REQUIRE(a && p->dy && p->h && p->w2 && p->g && p->d_w2, ACM_EINVAL, "acm_gcn_bwd: NULL argument");
    const int F = p->width;
    const GcnBwdPlan pl = gcn_bwd_plan(a, F, p->hidden);
    const size_t need = pl.gather_bytes + GCN_BWD_REC_BYTES + pl.partial_bytes;
    ACM_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace) % 16 == 0, ACM_ENOMEM,
                "acm_gcn_bwd: workspace %zu B < required %zu B (or not 16-byte aligned)", workspace_bytes, need);
    static_assert(sizeof(GcnBwdRec) <= GCN_BWD_REC_BYTES, "record slot");
    hipStream_t s = (hipStream_t)stream;
    float* partial = (float*)workspace;
    GcnBwdRec* rec = (GcnBwdRec*)((char*)workspace + pl.gather_bytes);
    float* slabs = (float*)((char*)rec + GCN_BWD_REC_BYTES);
    {   // one launch: the parameter record and the zeroed slabs
        const GcnBwdRec r = {p->h, (long)p->ld_h, p->w2, (long)p->ld_w2, p->keep_scale, p->relu, p->hidden, p->g, (long)p->ld_g,
                             p->dz, (long)p->ld_dz, slabs, pl.slabs * 32};
        const long n4 = (long)(pl.partial_bytes / 16);
        long blocks = (n4 + 255) / 256;
        blocks = blocks < 1 ? 1 : (blocks > 1024 ? 1024 : blocks);
        hipLaunchKernelGGL(gcn_bwd_prepare_kernel, dim3((unsigned)blocks), dim3(256), 0, s, r, rec, (float4*)slabs, n4);
        ACM_CHECK_HIP(hipGetLastError());
    }
    if (a->n_items > 0) {
        const CsrView v = acm_view(a);
        const GatherSrc g = {{p->dy, nullptr, nullptr}, {(long)p->ld_dy, 0, 0}};
        const GatherForm form = choose_gather_form(a->n_rows, a->n_cols, a->nnz, a->n_long, a->long_index, g, 1, F, false, 0, false);
        EpiGcnBwd::Args ea = {rec, pl.gs, 0};
        const int rc = acm_pick([&](auto fp, auto gs) {
            constexpr int FP = decltype(fp)::value, GS = decltype(gs)::value;
            if constexpr (!(FP == 8 && GS == 16))          // (never chosen: gcn_bwd_plan)
                hipLaunchKernelGGL((spmm_narrow_kernel<FP, 1, GS, false, EpiGcnBwd>), dim3(pl.grid), dim3(256), 0, s, v, g, F,
                                   form.vecmask, ea, partial);
            return ACM_OK;
        }, acm_fp_of(F), acm_lanes_of(pl.gs));
        ACM_REQUIRE(rc == ACM_OK, ACM_EUNSUPPORTED, "acm_gcn_bwd: no narrow gather for %d lanes per item", pl.gs);
        ACM_CHECK_HIP(hipGetLastError());
        if (pl.fix_blocks) {                      // the long rows the gather left in partial slots: groups of sixteen lanes
            ea.gs = 16;
            ea.slab_base = pl.grid * (256 / pl.gs);
            const bool windows = pl.gs == ACM_WINDOW;
            acm_pick([&](auto fp) {
                if (windows)
                    hipLaunchKernelGGL((spmm_fixup_windows_kernel<fp(), 1, EpiGcnBwd>), dim3(pl.fix_blocks), dim3(256), 0, s, v, F, ea, partial);
                else
                    hipLaunchKernelGGL((spmm_fixup_narrow_kernel<fp(), 1, EpiGcnBwd>), dim3(pl.fix_blocks), dim3(256), 0, s, v, F, ea, partial);
                return ACM_OK;
            }, acm_fp_of(F));
            ACM_CHECK_HIP(hipGetLastError());
        }
    }
    const int len = p->hidden * F;
    const acm_reduce_seg_t seg = {slabs, (int)pl.slabs, 32, 0, len, p->d_w2, F, 0, p->ld_dw2, 0, (int)(pl.slabs * 32), 0};
    return acm_reduce_emit(p->defer, &seg, 1, s);
}
