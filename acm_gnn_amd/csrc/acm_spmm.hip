// acm_spmm / acm_spmm_v / acm_spmm_ex: plain CSR x dense (k-hop chains, tests); acm_spmm_internal: the same for callers
// inside the library; acm_cast_bf16: the bf16 table of a gathered operand.
#include "acm_gather_device.h"

struct EpiPlain {
    static constexpr bool kFusedHead = false;
    struct Args {
        float* y;
        long ldy;
        int relu;
        const float* sub;         // optional: y = out_scale[row] * acc - sub_scale[row] * sub[row][col]
        long ld_sub;
        const float* sub_scale;   // optional (NULL = 1)
        const float* out_scale;   // optional (NULL = 1)
    };
    template <class L, int NG>
    static __device__ __forceinline__ void apply(const Args& a, int row, const L& lay, int F,
                                                 const float (&acc)[NG][L::NV]) {
        if (!Owns<L>::lane_stores(lay)) return;
        const float os = a.out_scale ? a.out_scale[row] : 1.f;
#pragma unroll
        for (int i = 0; i < L::NV; ++i) {
            const int col = lay.col(i);
            if (col < F) {
                float v = os * acc[0][i];
                if (a.sub) v -= (a.sub_scale ? a.sub_scale[row] : 1.f) * a.sub[(long)row * a.ld_sub + col];
                a.y[(long)row * a.ldy + col] = a.relu ? fmaxf(v, 0.f) : v;
            }
        }
    }
};

__global__ __launch_bounds__(256) void cast_bf16_kernel(long n_rows, int n_cols, const float* __restrict__ src, long ld_src,
                                                        unsigned short* __restrict__ dst, long ld_dst) {
    const long total = n_rows * n_cols;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; q < total; q += (long)gridDim.x * 256) {
        const long r = q / n_cols;
        const int c = (int)(q - r * n_cols);
        unsigned b = __float_as_uint(src[r * ld_src + c]);
        if ((b & 0x7FFFFFFFu) > 0x7F800000u)
            b |= 0x00400000u;                            // NaN stays NaN (quiet, same sign): the carry below would make inf or 0 of some
        else
            b += 0x7FFFu + ((b >> 16) & 1u);             // round to nearest even
        dst[r * ld_dst + c] = (unsigned short)(b >> 16);
    }
}

extern "C" int acm_cast_bf16(int64_t n_rows, int64_t n_cols, const float* src, int64_t ld_src, uint16_t* dst,
                             int64_t ld_dst, acm_stream_t stream) {
    ACM_REQUIRE(src && dst, ACM_EINVAL, "acm_cast_bf16: NULL pointer");
    ACM_REQUIRE(n_rows >= 0 && n_cols >= 0 && n_cols < INT32_MAX && ld_src >= n_cols && ld_dst >= n_cols, ACM_ESHAPE,
                "acm_cast_bf16: bad sizes");
    if (n_rows == 0 || n_cols == 0) return ACM_OK;
    long blocks = (n_rows * n_cols + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(cast_bf16_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long)n_rows,
                       (int)n_cols, src, (long)ld_src, dst, (long)ld_dst);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_spmm_ex(const acm_csr_t* a, const void* G, int64_t ldg, int width, float* Y, int64_t ldy,
                           const acm_spmm_opts_t* o, void* workspace, size_t workspace_bytes, acm_stream_t stream) {
    return acm_spmm_internal(a, G, ldg, width, Y, ldy, o, workspace, workspace_bytes, stream, nullptr);
}

// *defer_fixup (in): leave the partial sums of the long rows in the workspace slots (width <= 256) for the caller's
// next kernel to add (acm_conv_agg_fwd's epilogue); (out): false when the gather finished those rows itself (the narrow
// kernel with 16 lanes per item) or the width rules it out -- Y is complete then.
int acm_spmm_internal(const acm_csr* a, const void* G, int64_t ldg, int width, float* Y, int64_t ldy,
                      const acm_spmm_opts_t* o, void* workspace, size_t workspace_bytes, acm_stream_t stream,
                      bool* defer_fixup) {
    bool defer = defer_fixup && *defer_fixup && a && width <= 256 && !(width <= 8 && narrow_finishes_long_rows(a));
    if (defer_fixup) *defer_fixup = defer;
    static const acm_spmm_opts_t none = {nullptr, nullptr, nullptr, 0, nullptr, 0, 0};
    if (!o) o = &none;
    ACM_REQUIRE(a && G && Y, ACM_EINVAL, "acm_spmm: NULL argument");
    ACM_REQUIRE(width > 0 && ldg >= width && ldy >= width && (!o->sub || o->ld_sub >= width), ACM_ESHAPE,
                "acm_spmm: width %d ldg %lld ldy %lld ld_sub %lld", width, (long long)ldg, (long long)ldy,
                (long long)o->ld_sub);
    ACM_REQUIRE(!o->g_bf16 || width <= 256, ACM_EUNSUPPORTED, "acm_spmm: bf16 operands are one column block wide");
    for (int c0 = 0; c0 < width; c0 += 256) {  // column blocks of <= 256
        const int wd = width - c0 < 256 ? width - c0 : 256;
        GatherSrc g = {{reinterpret_cast<const float*>(G) + (o->g_bf16 ? 0 : c0), nullptr, nullptr}, {ldg, 0, 0}};
        EpiPlain::Args ea = {Y + c0, ldy, o->relu, o->sub ? o->sub + c0 : nullptr, o->ld_sub, o->sub_scale, o->row_scale};
        int st = launch_gather<1, EpiPlain>(a, g, wd, ea, workspace, workspace_bytes, (hipStream_t)stream, "acm_spmm",
                                            o->vals, o->g_bf16 != 0, defer);
        if (st != ACM_OK) return st;
    }
    return ACM_OK;
}

extern "C" int acm_spmm_v(const acm_csr_t* a, const float* vals, const float* G, int64_t ldg, int width, float* Y,
                          int64_t ldy, int relu, void* workspace, size_t workspace_bytes, acm_stream_t stream) {
    const acm_spmm_opts_t o = {vals, nullptr, nullptr, 0, nullptr, relu, 0};
    return acm_spmm_ex(a, G, ldg, width, Y, ldy, &o, workspace, workspace_bytes, stream);
}

extern "C" int acm_spmm(const acm_csr_t* a, const float* G, int64_t ldg, int width, float* Y,
                        int64_t ldy, void* workspace, size_t workspace_bytes, acm_stream_t stream) {
    return acm_spmm_ex(a, G, ldg, width, Y, ldy, nullptr, workspace, workspace_bytes, stream);
}
