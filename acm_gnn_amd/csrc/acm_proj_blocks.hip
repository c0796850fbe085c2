// The projection of a layer whose input is a list of column blocks [x | H_0 | ... | H_{J-1}] (ACM-Snowball,
// ACM-Geometric/models.py:57-64) without the concatenation: Z = act(Z * accumulate + sum_j H_j W[r_j : r_j + w_j, :]) over the
// dense blocks H_j (the feature block's product -- acm_spmm_v for CSR features -- is in Z already), and its backward
// dH_j = dZ W[r_j : r_j + w_j, :]^T, dW[r_j : r_j + w_j, :] = H_j^T dZ (gfx950, wave64, fp32).
//
// W = [W_L | W_H | W_I] is never packed: the kernels walk the "product columns" p = c * F + q (channel c, column q) and
// read W_c[., q]; Z and dZ keep channel c at column c * f_block (the layout of the CSR route of the literal layer), so p maps
// to column (p / F) * f_block + p % F.  Everything runs on v_mfma_f32_16x16x4_f32 (a k-ordered fmaf chain per element):
//   forward   a wave owns two 16-row tiles and every product column (<= 12 tiles of 16); a block's weight rows W[r_j ...]
//             sit in LDS as [k][p]; a lane loads four consecutive k of its row at once (k = 16 c + 4 g + s at step s of lane
//             group g -- the B operand is read at the same k, so the chain's order is fixed, only not ascending)
//   backward  per dense block: the weight rows transposed in LDS as [p][i]; dH on the same tile product (K = the product
//             columns); dW = H_j^T dZ with the rows as the contraction index, operands straight from memory, accumulated in
//             registers over the 64-row groups a workgroup walks, then ONE slab per workgroup in groups of 32 elements
//             (acm_reduce_seg_t.elem_stride) and the fixed-order second phase of acm_reduce.hip.  No atomics.
#include "acm_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int PB_FWD_ROWS = 128;            // rows per workgroup of the forward: 4 waves x 2 tiles x 16
constexpr int PB_BWD_ROWS = 64;             // rows per group of the backward: 4 waves x 16
constexpr int PB_BWD_MAX_BLOCKS = 256;      // workgroups (= slabs) of the backward
constexpr int PB_FWD_LDS = 64 * 196;        // [k <= 64][p <= 192 (+ 4: lane groups land on different banks)]
constexpr int PB_BWD_LDS = 192 * 68;        // [p <= 192][i <= 64 (+ 4)]

__device__ __forceinline__ int pb_zcol(int p, int f, int fb) {
    const int c = p / f;
    return c * fb + (p - c * f);
}

__device__ __forceinline__ float pb_weight(const acm_proj_blocks_t& p, int row, int pc) {
    const int c = pc / p.f, q = pc - c * p.f;
    const float* W = c == 0 ? p.w_low : (c == 1 ? p.w_high : p.w_mlp);
    return W[(long)row * p.ldw + q];
}

template <int TMAX>
__global__ __launch_bounds__(256) void proj_blocks_fwd_kernel(acm_proj_blocks_t p, int n_rows, float* __restrict__ Z, long ldz,
                                                              int accumulate, int relu) {
    __shared__ __attribute__((aligned(16))) float ws[PB_FWD_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, g = lane >> 4;
    const int f = p.f, fb = p.f_block, P = 3 * f, T = (P + 15) >> 4, NP = T * 16, SW = NP + 4;
    const long r0 = (long)blockIdx.x * PB_FWD_ROWS + wave * 32;
    int zc[TMAX];                                // this lane's column of Z per product-column tile (-1: none)
#pragma unroll
    for (int t = 0; t < TMAX; ++t) zc[t] = (16 * t + m < P) ? pb_zcol(16 * t + m, f, fb) : -1;
    f32x4 acc[2][TMAX];
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = r0 + rt * 16 + 4 * g + r;
                acc[rt][t][r] = (accumulate && zc[t] >= 0 && row < n_rows) ? Z[row * ldz + zc[t]] : 0.f;
            }
    for (int j = 0; j < p.n_blocks; ++j) {
        const int w = p.width[j], kr = (w + 15) & ~15, wrow = p.row0[j];
        __syncthreads();                         // (the previous block's weights are done with)
        for (int e = threadIdx.x; e < kr * NP; e += 256) {
            const int k = e / NP, pc = e - k * NP;
            ws[k * SW + pc] = (k < w && pc < P) ? pb_weight(p, wrow + k, pc) : 0.f;
        }
        __syncthreads();
        const float* __restrict__ H = p.h[j];
        const long ldh = p.ld_h[j];
        const bool vec = ((uintptr_t)H & 15) == 0 && (ldh & 3) == 0;
        for (int c0 = 0; c0 < w; c0 += 16) {
            const int kb = c0 + 4 * g;           // this lane's four consecutive k (w % 4 == 0: all four or none)
            float a[2][4];
#pragma unroll
            for (int rt = 0; rt < 2; ++rt) {
                const long row = r0 + rt * 16 + m;
                if (row < n_rows && kb < w) {
                    if (vec) {
                        const float4 v = *reinterpret_cast<const float4*>(H + row * ldh + kb);
                        a[rt][0] = v.x, a[rt][1] = v.y, a[rt][2] = v.z, a[rt][3] = v.w;
                    } else {
#pragma unroll
                        for (int s = 0; s < 4; ++s) a[rt][s] = H[row * ldh + kb + s];
                    }
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s) a[rt][s] = 0.f;
                }
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int t = 0; t < TMAX; ++t)
                    if (t < T) {
                        const float b = ws[(kb + s) * SW + 16 * t + m];
                        acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0][s], b, acc[0][t], 0, 0, 0);
                        acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1][s], b, acc[1][t], 0, 0, 0);
                    }
        }
    }
    // C/D fragment: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
    for (int rt = 0; rt < 2; ++rt)
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long row = r0 + rt * 16 + 4 * g + r;
                if (zc[t] >= 0 && row < n_rows) {
                    const float v = acc[rt][t][r];
                    Z[row * ldz + zc[t]] = relu ? fmaxf(v, 0.f) : v;
                }
            }
    if (!accumulate && fb != f) {                // the pad columns of the two gathered channels: zeros, as acm_spmm_v leaves them
        const int half = fb - f, npad = 2 * half;
        for (int e = lane; e < 32 * npad; e += 64) {
            const int rr = e / npad, i = e - rr * npad;
            const long row = r0 + rr;
            if (row < n_rows) Z[row * ldz + (i < half ? f + i : fb + f + (i - half))] = 0.f;
        }
    }
}

__global__ __launch_bounds__(256) void proj_blocks_bwd_kernel(acm_proj_blocks_t p, int n_rows, const float* __restrict__ dZ,
                                                              long lddz, float* __restrict__ partial, int n_groups) {
    __shared__ __attribute__((aligned(16))) float wt[PB_BWD_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, g = lane >> 4;
    const int f = p.f, fb = p.f_block, P = 3 * f, T = (P + 15) >> 4, KP = T * 16;
    const int nblk = gridDim.x;
    const bool dz_vec = fb == f && ((uintptr_t)dZ & 15) == 0 && (lddz & 3) == 0;
    int zc[3];                                   // this lane's column of dZ for the product-column tiles wave, wave + 4, wave + 8
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int pc = 16 * (wave + 4 * u) + m;
        zc[u] = pc < P ? pb_zcol(pc, f, fb) : -1;
    }
    long base = 0;                               // first float of block j's slab region
    for (int j = 0; j < p.n_blocks; ++j) {
        const int w = p.width[j], MT = (w + 15) >> 4, wrow = p.row0[j];
        const float* __restrict__ H = p.h[j];
        const long ldh = p.ld_h[j];
        float* __restrict__ dH = p.d_h[j];
        const long lddh = p.ld_dh[j];
        __syncthreads();
        for (int e = threadIdx.x; e < MT * 16 * KP; e += 256) {      // wt[p][i] = W[r_j + i][p]
            const int i = e / KP, pc = e - i * KP;
            wt[pc * 68 + i] = (i < w && pc < P) ? pb_weight(p, wrow + i, pc) : 0.f;
        }
        __syncthreads();
        f32x4 dw[4][3];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int u = 0; u < 3; ++u) dw[mt][u] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int grp = blockIdx.x; grp < n_groups; grp += nblk) {
            const long rbase = (long)grp * PB_BWD_ROWS;
            if (dH) {                            // dH_j rows [rbase + 16 wave, + 16): K = the product columns
                f32x4 acc[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) acc[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
                const long row = rbase + 16 * wave + m;
                for (int c0 = 0; c0 < KP; c0 += 16) {
                    const int kb = c0 + 4 * g;
                    float a[4];
                    if (row < n_rows && dz_vec && kb + 3 < P) {
                        const float4 v = *reinterpret_cast<const float4*>(dZ + row * lddz + kb);
                        a[0] = v.x, a[1] = v.y, a[2] = v.z, a[3] = v.w;
                    } else {
#pragma unroll
                        for (int s = 0; s < 4; ++s)
                            a[s] = (row < n_rows && kb + s < P) ? dZ[row * lddz + pb_zcol(kb + s, f, fb)] : 0.f;
                    }
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int t = 0; t < 4; ++t)
                            if (t < MT)
                                acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], wt[(kb + s) * 68 + 16 * t + m], acc[t], 0, 0, 0);
                }
#pragma unroll
                for (int t = 0; t < 4; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const long orow = rbase + 16 * wave + 4 * g + r;
                        if (16 * t + m < w && orow < n_rows) dH[orow * lddh + 16 * t + m] = acc[t][r];
                    }
            }
            // dW rows of this block: A[i][row] = H_j[row][i], B[row][p] = dZ[row][p]; this wave's product-column tiles
            for (int c0 = 0; c0 < PB_BWD_ROWS; c0 += 4) {
                const long row = rbase + c0 + g;
                const bool in = row < n_rows;
                float a[4], b[3];
#pragma unroll
                for (int mt = 0; mt < 4; ++mt) a[mt] = (in && 16 * mt + m < w) ? H[row * ldh + 16 * mt + m] : 0.f;
#pragma unroll
                for (int u = 0; u < 3; ++u) b[u] = (in && zc[u] >= 0) ? dZ[row * lddz + zc[u]] : 0.f;
#pragma unroll
                for (int mt = 0; mt < 4; ++mt)
                    if (mt < MT) {
#pragma unroll
                        for (int u = 0; u < 3; ++u)
                            if (wave + 4 * u < T) dw[mt][u] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[mt], b[u], dw[mt][u], 0, 0, 0);
                    }
            }
        }
        // this workgroup's slab of block j, in groups of 32 elements: region[q / 32][workgroup][q % 32], q = i * P + p
        float* __restrict__ region = partial + base;
#pragma unroll
        for (int mt = 0; mt < 4; ++mt)
#pragma unroll
            for (int u = 0; u < 3; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * mt + 4 * g + r, pc = 16 * (wave + 4 * u) + m;
                    if (i < w && pc < P) {
                        const long q = (long)i * P + pc;
                        region[((q >> 5) * nblk + blockIdx.x) * 32 + (q & 31)] = dw[mt][u][r];
                    }
                }
        base += (long)nblk * (((long)w * P + 31) / 32 * 32);
    }
}

int pb_check(const acm_proj_blocks_t* p, const char* who) {
    ACM_REQUIRE(p && p->w_low && p->w_high && p->w_mlp, ACM_EINVAL, "%s: NULL argument", who);
    ACM_REQUIRE(p->n_blocks >= 0 && p->f >= 1 && p->f_block >= p->f && p->ldw >= p->f, ACM_ESHAPE, "%s: bad sizes", who);
    ACM_REQUIRE(p->n_blocks <= ACM_PROJ_BLOCKS_MAX && p->f <= 64, ACM_EUNSUPPORTED,
                "%s: %d blocks, F = %d (at most %d blocks, F <= 64; compose it from acm_gemm otherwise)", who, p->n_blocks, p->f,
                ACM_PROJ_BLOCKS_MAX);
    for (int j = 0; j < p->n_blocks; ++j) {
        ACM_REQUIRE(p->h[j] && p->row0[j] >= 0 && p->width[j] >= 1 && p->ld_h[j] >= p->width[j] &&
                        (int64_t)p->row0[j] + p->width[j] <= p->f_in, ACM_ESHAPE,
                    "%s: block %d: NULL pointer, bad sizes or rows beyond the weights' %d", who, j, p->f_in);
        ACM_REQUIRE(p->width[j] % 4 == 0 && p->width[j] <= 64, ACM_EUNSUPPORTED,
                    "%s: block %d is %d columns wide (multiples of 4 up to 64; compose it from acm_gemm otherwise)", who, j,
                    p->width[j]);
    }
    return ACM_OK;
}

int pb_bwd_blocks(int64_t n_rows) {
    int64_t nb = (n_rows + PB_BWD_ROWS - 1) / PB_BWD_ROWS;
    if (nb > PB_BWD_MAX_BLOCKS) nb = PB_BWD_MAX_BLOCKS;
    return nb < 1 ? 1 : (int)nb;
}

}  // namespace

extern "C" int acm_proj_blocks_fwd(int64_t n_rows, const acm_proj_blocks_t* p, float* Z, int64_t ldz, int accumulate, int relu,
                                   acm_stream_t stream) {
    const int st = pb_check(p, "acm_proj_blocks_fwd");
    if (st != ACM_OK) return st;
    ACM_REQUIRE(Z, ACM_EINVAL, "acm_proj_blocks_fwd: NULL pointer");
    ACM_REQUIRE(n_rows >= 0 && n_rows < INT32_MAX && ldz >= 2 * (int64_t)p->f_block + p->f, ACM_ESHAPE,
                "acm_proj_blocks_fwd: bad sizes / leading dimensions");
    if (n_rows == 0) return ACM_OK;
    hipStream_t s = (hipStream_t)stream;
    const int nblk = (int)((n_rows + PB_FWD_ROWS - 1) / PB_FWD_ROWS);
    const int tiles = (3 * p->f + 15) / 16;
    const int rc = acm_pick([&](auto T) {
        hipLaunchKernelGGL((proj_blocks_fwd_kernel<T()>), dim3(nblk), dim3(256), 0, s, *p, (int)n_rows, Z, (long)ldz, accumulate, relu);
        return ACM_OK;
    }, acm_one_of<3, 6, 12>(tiles <= 3 ? 3 : (tiles <= 6 ? 6 : (tiles <= 12 ? 12 : tiles))));
    ACM_REQUIRE(rc == ACM_OK, ACM_EUNSUPPORTED, "acm_proj_blocks_fwd: no kernel for %d column tiles", tiles);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_proj_blocks_bwd_workspace_bytes(int64_t n_rows, const acm_proj_blocks_t* p, size_t* bytes) {
    ACM_REQUIRE(bytes, ACM_EINVAL, "acm_proj_blocks_bwd_workspace_bytes: NULL argument");
    const int st = pb_check(p, "acm_proj_blocks_bwd");
    if (st != ACM_OK) return st;
    ACM_REQUIRE(n_rows >= 0 && n_rows < INT32_MAX, ACM_ESHAPE, "acm_proj_blocks_bwd_workspace_bytes: bad sizes");
    size_t per_block = 0;
    for (int j = 0; j < p->n_blocks; ++j) per_block += ((size_t)p->width[j] * 3 * p->f + 31) / 32 * 32;       // whole groups of 32
    *bytes = (size_t)pb_bwd_blocks(n_rows) * per_block * sizeof(float);
    return ACM_OK;
}

extern "C" int acm_proj_blocks_bwd(int64_t n_rows, const acm_proj_blocks_t* p, const float* dZ, int64_t lddz, float* dW,
                                   int64_t lddw, int64_t dw_col_block, int64_t dw_block_stride, void* workspace,
                                   size_t workspace_bytes, acm_reduce_list_t* defer, acm_stream_t stream) {
    size_t need = 0;
    const int st = acm_proj_blocks_bwd_workspace_bytes(n_rows, p, &need);
    if (st != ACM_OK) return st;
    const int P = 3 * p->f;
    ACM_REQUIRE(dZ && dW, ACM_EINVAL, "acm_proj_blocks_bwd: NULL pointer");
    ACM_REQUIRE(lddz >= 2 * (int64_t)p->f_block + p->f && dw_col_block >= 0 &&
                    lddw >= (dw_col_block ? (dw_col_block < P ? dw_col_block : P) : P), ACM_ESHAPE,
                "acm_proj_blocks_bwd: bad sizes / leading dimensions");
    for (int j = 0; j < p->n_blocks; ++j)
        ACM_REQUIRE(!p->d_h[j] || p->ld_dh[j] >= p->width[j], ACM_ESHAPE, "acm_proj_blocks_bwd: block %d: bad leading dimension", j);
    if (p->n_blocks == 0) return ACM_OK;
    ACM_REQUIRE(workspace && workspace_bytes >= need, ACM_ENOMEM, "acm_proj_blocks_bwd: workspace %zu B < required %zu B",
                workspace_bytes, need);
    ACM_REQUIRE(((uintptr_t)workspace & 15) == 0, ACM_EINVAL, "acm_proj_blocks_bwd: the workspace must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float* partial = (float*)workspace;
    const int nblk = pb_bwd_blocks(n_rows);
    const int n_groups = (int)((n_rows + PB_BWD_ROWS - 1) / PB_BWD_ROWS);
    hipLaunchKernelGGL(proj_blocks_bwd_kernel, dim3(nblk), dim3(256), 0, s, *p, (int)n_rows, dZ, (long)lddz, partial, n_groups);
    ACM_CHECK_HIP(hipGetLastError());
    // dW[r_j + i][p] = sum_b region_j[(i * P + p) / 32][b][(i * P + p) % 32], optionally in the column-block layout of dW
    acm_reduce_seg_t segs[ACM_PROJ_BLOCKS_MAX];
    long base = 0;
    for (int j = 0; j < p->n_blocks; ++j) {
        const long len = (long)p->width[j] * P;
        const acm_reduce_seg_t seg = {partial + base, nblk, 32, 0, (int32_t)len, dW + (long)p->row0[j] * lddw, P,
                                      (int32_t)dw_col_block, lddw, dw_block_stride, nblk * 32, 0};
        segs[j] = seg;
        base += (long)nblk * ((len + 31) / 32 * 32);
    }
    return acm_reduce_emit(defer, segs, p->n_blocks, s);
}
