// BatchNorm1d between the Linears of a deep mlpX stack (ACM-Pytorch/models/layers.py:245-285: lin -> relu -> bn -> dropout,
// ACM-Pytorch/models/models.py:37-41,150-152), folded into the Linears on both sides of it:
//   acm_bnorm_stats      column statistics of H = relu(...) [n, f] -> (mu, r, a, c) and the running buffers
//   acm_bnorm_fold_centred       W' = W diag(a), b' = b + W beta: the next Linear reads H - 1 mu^T, subtracted where its product
//                        stages H (acm_linear_fwd_shift); Z = a * (H - mu) + beta is never written
//   acm_bnorm_param_bwd_centred  dW, d_beta, d_gamma of that pair from the f x f matrices M_c = G^T (H - 1 mu^T) (acm_gemm_shift)
//                        and s = colsum(G)
//   acm_bnorm_fold / acm_bnorm_param_bwd  the same pair for products on H itself (b' = b + W c, M = G^T H): the first form of the
//                        stack, kept for callers of the C ABI
// The package takes the CENTRED pair: on a column whose mean is far above its spread (a unit that is always on) a * H + c and
// M a + s c cancel all but the digits the statistics kernel took care to keep.
//   acm_bnorm_bwd        the one row-local pass of the backward: G_i = [H > 0] a (dZ - d_beta / n - xhat d_gamma / n) and
//                        its column sums (or, without statistics, the stack's output epilogue read off Y as acm_bias_act_bwd does)
// Row-major matrices of f <= 256 columns.  The 256 threads of a block are (row slice, column group): f / V threads share a
// row (V = 4 floats per thread where f, the pitches and the addresses allow 16-byte accesses; V = 1 otherwise), 256 / (f / V)
// rows are in flight per pass, a block owns a contiguous stripe of rows.  Every sum has a fixed order: same bits every run.
#include <initializer_list>

#include "acm_common.h"

namespace {

constexpr int BN_ROWS = 8;         // rows a thread takes per step: one group, merged into its running triple (Chan)

long bn_rows_per_block(int64_t n_rows) {
    long r = (long)((n_rows + 1023) / 1024);
    if (r < 32) r = 32;
    return (r + 7) & ~7L;
}
int bn_blocks(int64_t n_rows) {
    const long rpb = bn_rows_per_block(n_rows);
    const long b = (long)((n_rows + rpb - 1) / rpb);
    return (int)(b < 1 ? 1 : b);
}
bool bn_vec4(int f, std::initializer_list<const void*> ptrs, std::initializer_list<int64_t> lds) {
    if (f % 4) return false;
    for (const void* p : ptrs)
        if (((uintptr_t)p) % 16) return false;
    for (int64_t ld : lds)
        if (ld % 4) return false;
    return true;
}

template <int V>
struct Vec;
template <>
struct Vec<4> {
    static __device__ __forceinline__ void load(float (&d)[4], const float* p) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
    }
    static __device__ __forceinline__ void store(float* p, const float (&d)[4]) {
        *reinterpret_cast<float4*>(p) = make_float4(d[0], d[1], d[2], d[3]);
    }
};
template <>
struct Vec<1> {
    static __device__ __forceinline__ void load(float (&d)[1], const float* p) { d[0] = *p; }
    static __device__ __forceinline__ void store(float* p, const float (&d)[1]) { *p = d[0]; }
};

// (count, mean, M2) <- merge with (cb, mb, m2b), cb > 0 (Chan et al.): no sum of squares of the raw values anywhere -- a column
// of post-ReLU activations with mean >> spread keeps its digits
__device__ __forceinline__ void bn_merge(float& ca, float& ma, float& m2a, float cb, float mb, float m2b) {
    const float tot = ca + cb, w = cb / tot, d = mb - ma;
    ma = fmaf(d, w, ma);
    m2a += m2b + d * d * ca * w;
    ca = tot;
}

// Phase 1: block b -> (mean, M2) per column of its stripe [b * rows_per_block, ...); the count is the stripe's length.
// partial: [block][2][f]
template <int V>
__global__ __launch_bounds__(256) void bn_stats_partial_kernel(long n_rows, int f, const float* __restrict__ h, long ldh,
                                                               long rows_per_block, float* __restrict__ partial) {
    __shared__ float s_cnt[256], s_mean[256 * V], s_m2[256 * V];
    const int tpr = f / V, rpp = 256 / tpr;
    const int rr = threadIdx.x / tpr, q = threadIdx.x - rr * tpr;
    const long r0 = (long)blockIdx.x * rows_per_block;
    const long r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    float cnt = 0.f, mean[V], m2[V];
#pragma unroll
    for (int v = 0; v < V; ++v) mean[v] = 0.f, m2[v] = 0.f;
    if (rr < rpp) {
        for (long r = r0 + rr; r < r1; r += (long)rpp * BN_ROWS) {
            float x[BN_ROWS][V];
            int k = 0;
#pragma unroll
            for (int u = 0; u < BN_ROWS; ++u) {
                const long ru = r + (long)u * rpp;
                const bool in = ru < r1;                 // (a prefix of the group: the rows ascend)
                Vec<V>::load(x[u], h + (in ? ru : r) * ldh + q * V);
                k += in ? 1 : 0;
            }
            const float kf = (float)k, inv_k = 1.f / kf;
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float sum = 0.f;
#pragma unroll
                for (int u = 0; u < BN_ROWS; ++u) sum += u < k ? x[u][v] : 0.f;
                const float gm = sum * inv_k;
                float gm2 = 0.f;
#pragma unroll
                for (int u = 0; u < BN_ROWS; ++u) {
                    const float d = x[u][v] - gm;
                    gm2 += u < k ? d * d : 0.f;
                }
                float c = cnt;
                bn_merge(c, mean[v], m2[v], kf, gm, gm2);
            }
            cnt += kf;
        }
    }
    s_cnt[threadIdx.x] = cnt;
#pragma unroll
    for (int v = 0; v < V; ++v) s_mean[threadIdx.x * V + v] = mean[v], s_m2[threadIdx.x * V + v] = m2[v];
    __syncthreads();
    if ((int)threadIdx.x < tpr) {                        // the row slices of a column group, in slice order
        for (int s = 1; s < rpp; ++s) {
            const int t = s * tpr + q;
            const float cb = s_cnt[t];
            if (cb > 0.f) {
#pragma unroll
                for (int v = 0; v < V; ++v) {
                    float c = cnt;
                    bn_merge(c, mean[v], m2[v], cb, s_mean[t * V + v], s_m2[t * V + v]);
                }
                cnt += cb;
            }
        }
        float* dst = partial + (long)blockIdx.x * 2 * f + q * V;
        Vec<V>::store(dst, mean);
        Vec<V>::store(dst + f, m2);
    }
}

struct BnFinal {
    const float* gamma;
    const float* beta;
    float eps, momentum;
    float* running_mean;
    float* running_var;
    long long* num_batches;
    float* stats;              // [4][f]: mu, r = 1 / sqrt(var + eps), a = gamma r, c = beta - mu a
};

// Phase 2: one block per 32 columns, 8 slices of blocks per column (slice s: blocks s, s + 8, ... in order), the slices in
// order; then the derived vectors and the running buffers (momentum update, unbiased variance, the batch counter).
__global__ __launch_bounds__(256) void bn_stats_final_kernel(long n_rows, int f, const float* __restrict__ partial, int nblk,
                                                             long rows_per_block, BnFinal p) {
    __shared__ float s_cnt[256], s_mean[256], s_m2[256];
    const int lane = threadIdx.x & 31, sl = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + lane;
    float cnt = 0.f, mean = 0.f, m2 = 0.f;
    if (c < f) {
        for (int b = sl; b < nblk; b += 8) {
            const long r0 = (long)b * rows_per_block;
            const long r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
            const float* src = partial + (long)b * 2 * f + c;
            bn_merge(cnt, mean, m2, (float)(r1 - r0), src[0], src[f]);
        }
    }
    s_cnt[threadIdx.x] = cnt, s_mean[threadIdx.x] = mean, s_m2[threadIdx.x] = m2;
    __syncthreads();
    if (sl == 0 && c < f) {
        for (int s = 1; s < 8; ++s) {
            const int t = s * 32 + lane;
            if (s_cnt[t] > 0.f) bn_merge(cnt, mean, m2, s_cnt[t], s_mean[t], s_m2[t]);
        }
        const float nf = (float)n_rows;
        const float var = m2 / nf;                           // biased: what normalises the batch
        const float r = 1.f / sqrtf(var + p.eps);
        const float a = p.gamma[c] * r;
        p.stats[c] = mean, p.stats[f + c] = r, p.stats[2 * f + c] = a, p.stats[3 * f + c] = p.beta[c] - mean * a;
        if (p.running_mean) p.running_mean[c] = (1.f - p.momentum) * p.running_mean[c] + p.momentum * mean;
        if (p.running_var) p.running_var[c] = (1.f - p.momentum) * p.running_var[c] + p.momentum * (m2 / (nf - 1.f));
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.num_batches) p.num_batches[0] += 1;
}

// Evaluation: the running statistics take the batch's place; nothing of size n is read and no buffer changes.
__global__ __launch_bounds__(256) void bn_stats_eval_kernel(int f, BnFinal p) {
    const int c = threadIdx.x;
    if (c < f) {
        const float mean = p.running_mean[c];
        const float r = 1.f / sqrtf(p.running_var[c] + p.eps);
        const float a = p.gamma[c] * r;
        p.stats[c] = mean, p.stats[f + c] = r, p.stats[2 * f + c] = a, p.stats[3 * f + c] = p.beta[c] - mean * a;
    }
}

// Block o: row o of W' = W diag(a) and b'[o] = b[o] + sum_k W[o, k] beta[k] (binary tree over the 256 threads); beta NULL: the
// uncentred form, c[k] = stats row 3 in beta's place
__global__ __launch_bounds__(256) void bn_fold_kernel(int f_in, const float* __restrict__ w, long ldw, const float* __restrict__ bias,
                                                      const float* __restrict__ beta, const float* __restrict__ stats,
                                                      float* __restrict__ wf, long ldwf, float* __restrict__ bias_f) {
    __shared__ float red[256];
    const int o = blockIdx.x, k = threadIdx.x;
    float t = 0.f;
    if (k < f_in) {
        const float wv = w[(long)o * ldw + k];
        wf[(long)o * ldwf + k] = wv * stats[2 * f_in + k];
        t = wv * (beta ? beta[k] : stats[3 * f_in + k]);
    }
    red[k] = t;
    __syncthreads();
    for (int m = 128; m >= 1; m >>= 1) {
        if (k < m) red[k] += red[k + m];
        __syncthreads();
    }
    if (k == 0) bias_f[o] = (bias ? bias[o] : 0.f) + red[0];
}

// Thread = input column k of the Linear behind the BatchNorm, rows o in order, M = M_c = G^T (H - 1 mu^T):
//   dW[o, k] = M[o, k] a[k] + s[o] beta[k]     d_beta[k] = sum_o s[o] W[o, k]     d_gamma[k] = r[k] sum_o W[o, k] M[o, k]
// beta NULL: the uncentred form, M = G^T H:  dW = M a + s c,  d_gamma[k] = r[k] (sum_o W[o, k] M[o, k] - mu[k] d_beta[k])
__global__ __launch_bounds__(64) void bn_param_bwd_kernel(int f_out, int f_in, const float* __restrict__ m, long ldm,
                                                          const float* __restrict__ s, const float* __restrict__ w, long ldw,
                                                          const float* __restrict__ beta, const float* __restrict__ stats,
                                                          float* __restrict__ dw, long lddw, float* __restrict__ d_beta,
                                                          float* __restrict__ d_gamma) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= f_in) return;
    const float r = stats[f_in + k], a = stats[2 * f_in + k], bt = beta ? beta[k] : stats[3 * f_in + k];
    float db = 0.f, q = 0.f;
    for (int o = 0; o < f_out; ++o) {
        const float mv = m[(long)o * ldm + k], wv = w[(long)o * ldw + k], so = s[o];
        dw[(long)o * lddw + k] = fmaf(mv, a, so * bt);
        db = fmaf(so, wv, db);
        q = fmaf(wv, mv, q);
    }
    d_beta[k] = db;
    d_gamma[k] = beta ? r * q : r * (q - stats[k] * db);
}

struct BnBwd {
    const float* stats;        // NULL: the output epilogue (keep_scale / relu, masks read off H = Y)
    const float* d_beta;
    const float* d_gamma;
    float inv_n, keep_scale;
    int relu;
};

// G may be dZ itself: an element is read and written by the same thread.
// partial: [group of 32 columns][block][32]
template <int V>
__global__ __launch_bounds__(256) void bn_bwd_kernel(long n_rows, int f, const float* dz, long lddz, const float* __restrict__ h,
                                                     long ldh, BnBwd p, float* g, long ldg, long rows_per_block,
                                                     float* __restrict__ partial) {
    __shared__ float s_acc[256 * V];
    const int tpr = f / V, rpp = 256 / tpr;
    const int rr = threadIdx.x / tpr, q = threadIdx.x - rr * tpr;
    const long r0 = (long)blockIdx.x * rows_per_block;
    const long r1 = r0 + rows_per_block < n_rows ? r0 + rows_per_block : n_rows;
    float acc[V], a[V], mu[V], k1[V], k2[V];
#pragma unroll
    for (int v = 0; v < V; ++v) acc[v] = 0.f, a[v] = 0.f, mu[v] = 0.f, k1[v] = 0.f, k2[v] = 0.f;
    if (rr < rpp) {
        if (p.stats) {
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const int c = q * V + v;
                mu[v] = p.stats[c], a[v] = p.stats[2 * f + c];
                k1[v] = p.d_beta[c] * p.inv_n;
                k2[v] = p.stats[f + c] * p.d_gamma[c] * p.inv_n;
            }
        }
        for (long r = r0 + rr; r < r1; r += rpp) {
            float dv[V], hv[V], gv[V];
            Vec<V>::load(dv, dz + r * lddz + q * V);
            Vec<V>::load(hv, h + r * ldh + q * V);
#pragma unroll
            for (int v = 0; v < V; ++v) {
                float t;
                if (p.stats) t = hv[v] > 0.f ? a[v] * (dv[v] - k1[v] - (hv[v] - mu[v]) * k2[v]) : 0.f;
                else if (p.relu) t = hv[v] > 0.f ? dv[v] * p.keep_scale : 0.f;
                else if (p.keep_scale != 1.f) t = hv[v] != 0.f ? dv[v] * p.keep_scale : 0.f;
                else t = dv[v];
                gv[v] = t;
                acc[v] += t;
            }
            Vec<V>::store(g + r * ldg + q * V, gv);
        }
    }
#pragma unroll
    for (int v = 0; v < V; ++v) s_acc[threadIdx.x * V + v] = acc[v];
    __syncthreads();
    if ((int)threadIdx.x < tpr) {
        const long gstride = (long)gridDim.x * 32;
        for (int s = 1; s < rpp; ++s) {
#pragma unroll
            for (int v = 0; v < V; ++v) acc[v] += s_acc[(s * tpr + q) * V + v];
        }
#pragma unroll
        for (int v = 0; v < V; ++v) {
            const int c = q * V + v;
            partial[(long)(c >> 5) * gstride + (long)blockIdx.x * 32 + (c & 31)] = acc[v];
        }
    }
}

}  // namespace

extern "C" int acm_bnorm_stats_workspace_bytes(int64_t n_rows, int f, size_t* bytes) {
    ACM_REQUIRE(bytes, ACM_EINVAL, "acm_bnorm_stats_workspace_bytes: NULL argument");
    ACM_REQUIRE(n_rows >= 0 && f >= 1 && f <= 256, ACM_EUNSUPPORTED, "acm_bnorm_stats: f %d outside 1..256", f);
    *bytes = (size_t)bn_blocks(n_rows) * 2 * (size_t)f * sizeof(float);
    return ACM_OK;
}

extern "C" int acm_bnorm_stats(int64_t n_rows, int f, const float* H, int64_t ldh, const float* gamma, const float* beta, float eps,
                               float momentum, int train, float* running_mean, float* running_var, int64_t* num_batches,
                               float* stats, void* workspace, size_t workspace_bytes, acm_stream_t stream) {
    ACM_REQUIRE(gamma && beta && stats, ACM_EINVAL, "acm_bnorm_stats: NULL argument");
    ACM_REQUIRE(f >= 1 && f <= 256, ACM_EUNSUPPORTED, "acm_bnorm_stats: f %d outside 1..256", f);
    ACM_REQUIRE(eps > 0.f, ACM_EINVAL, "acm_bnorm_stats: eps must be positive");
    hipStream_t s = (hipStream_t)stream;
    const BnFinal fin = {gamma, beta, eps, momentum, running_mean, running_var, (long long*)num_batches, stats};
    if (!train) {
        ACM_REQUIRE(running_mean && running_var, ACM_EINVAL, "acm_bnorm_stats: evaluation needs the running statistics");
        hipLaunchKernelGGL(bn_stats_eval_kernel, dim3(1), dim3(256), 0, s, f, fin);
        ACM_CHECK_HIP(hipGetLastError());
        return ACM_OK;
    }
    ACM_REQUIRE(H, ACM_EINVAL, "acm_bnorm_stats: NULL argument");
    ACM_REQUIRE(n_rows >= 2, ACM_ESHAPE, "acm_bnorm_stats: batch statistics need more than one row (%lld)", (long long)n_rows);
    ACM_REQUIRE(ldh >= f, ACM_ESHAPE, "acm_bnorm_stats: ldh %lld < f %d", (long long)ldh, f);
    ACM_REQUIRE(momentum >= 0.f && momentum <= 1.f, ACM_EINVAL, "acm_bnorm_stats: momentum outside 0..1");
    size_t need = 0;
    const int st = acm_bnorm_stats_workspace_bytes(n_rows, f, &need);
    if (st != ACM_OK) return st;
    ACM_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace) % 16 == 0, ACM_ENOMEM,
                "acm_bnorm_stats: workspace %zu B < required %zu B (or not 16-byte aligned)", workspace_bytes, need);
    const int nblk = bn_blocks(n_rows);
    const long rpb = bn_rows_per_block(n_rows);
    float* partial = (float*)workspace;
    if (bn_vec4(f, {H}, {ldh}))
        hipLaunchKernelGGL(bn_stats_partial_kernel<4>, dim3(nblk), dim3(256), 0, s, (long)n_rows, f, H, (long)ldh, rpb, partial);
    else
        hipLaunchKernelGGL(bn_stats_partial_kernel<1>, dim3(nblk), dim3(256), 0, s, (long)n_rows, f, H, (long)ldh, rpb, partial);
    ACM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3((f + 31) / 32), dim3(256), 0, s, (long)n_rows, f, partial, nblk, rpb, fin);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

static int bn_fold(int f_out, int f_in, const float* W, int64_t ldw, const float* bias, const float* beta, const float* stats,
                   float* W_folded, int64_t ldwf, float* bias_folded, acm_stream_t stream) {
    ACM_REQUIRE(W && stats && W_folded && bias_folded, ACM_EINVAL, "acm_bnorm_fold: NULL argument");
    ACM_REQUIRE(f_in >= 1 && f_in <= 256 && f_out >= 1 && f_out <= 256, ACM_EUNSUPPORTED, "acm_bnorm_fold: %d x %d outside 1..256", f_out,
                f_in);
    ACM_REQUIRE(ldw >= f_in && ldwf >= f_in, ACM_ESHAPE, "acm_bnorm_fold: leading dimension too small");
    hipLaunchKernelGGL(bn_fold_kernel, dim3(f_out), dim3(256), 0, (hipStream_t)stream, f_in, W, (long)ldw, bias, beta, stats,
                       W_folded, (long)ldwf, bias_folded);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_bnorm_fold(int f_out, int f_in, const float* W, int64_t ldw, const float* bias, const float* stats, float* W_folded,
                              int64_t ldwf, float* bias_folded, acm_stream_t stream) {
    return bn_fold(f_out, f_in, W, ldw, bias, nullptr, stats, W_folded, ldwf, bias_folded, stream);
}

extern "C" int acm_bnorm_fold_centred(int f_out, int f_in, const float* W, int64_t ldw, const float* bias, const float* beta,
                                      const float* stats, float* W_folded, int64_t ldwf, float* bias_folded, acm_stream_t stream) {
    ACM_REQUIRE(beta, ACM_EINVAL, "acm_bnorm_fold_centred: NULL argument");
    return bn_fold(f_out, f_in, W, ldw, bias, beta, stats, W_folded, ldwf, bias_folded, stream);
}

static int bn_param_bwd(int f_out, int f_in, const float* M, int64_t ldm, const float* s, const float* W, int64_t ldw, const float* beta,
                        const float* stats, float* dW, int64_t lddw, float* d_beta, float* d_gamma, acm_stream_t stream) {
    ACM_REQUIRE(M && s && W && stats && dW && d_beta && d_gamma, ACM_EINVAL, "acm_bnorm_param_bwd: NULL argument");
    ACM_REQUIRE(f_in >= 1 && f_in <= 256 && f_out >= 1 && f_out <= 256, ACM_EUNSUPPORTED, "acm_bnorm_param_bwd: %d x %d outside 1..256",
                f_out, f_in);
    ACM_REQUIRE(ldm >= f_in && ldw >= f_in && lddw >= f_in, ACM_ESHAPE, "acm_bnorm_param_bwd: leading dimension too small");
    hipLaunchKernelGGL(bn_param_bwd_kernel, dim3((f_in + 63) / 64), dim3(64), 0, (hipStream_t)stream, f_out, f_in, M, (long)ldm, s, W,
                       (long)ldw, beta, stats, dW, (long)lddw, d_beta, d_gamma);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_bnorm_param_bwd(int f_out, int f_in, const float* M, int64_t ldm, const float* s, const float* W, int64_t ldw,
                                   const float* stats, float* dW, int64_t lddw, float* d_beta, float* d_gamma, acm_stream_t stream) {
    return bn_param_bwd(f_out, f_in, M, ldm, s, W, ldw, nullptr, stats, dW, lddw, d_beta, d_gamma, stream);
}

extern "C" int acm_bnorm_param_bwd_centred(int f_out, int f_in, const float* M, int64_t ldm, const float* s, const float* W, int64_t ldw,
                                           const float* beta, const float* stats, float* dW, int64_t lddw, float* d_beta, float* d_gamma,
                                           acm_stream_t stream) {
    ACM_REQUIRE(beta, ACM_EINVAL, "acm_bnorm_param_bwd_centred: NULL argument");
    return bn_param_bwd(f_out, f_in, M, ldm, s, W, ldw, beta, stats, dW, lddw, d_beta, d_gamma, stream);
}

extern "C" int acm_bnorm_bwd_workspace_bytes(int64_t n_rows, int f, size_t* bytes) {
    ACM_REQUIRE(bytes, ACM_EINVAL, "acm_bnorm_bwd_workspace_bytes: NULL argument");
    ACM_REQUIRE(n_rows >= 0 && f >= 1 && f <= 256, ACM_EUNSUPPORTED, "acm_bnorm_bwd: f %d outside 1..256", f);
    *bytes = (size_t)((f + 31) / 32) * (size_t)bn_blocks(n_rows) * 32 * sizeof(float);
    return ACM_OK;
}

extern "C" int acm_bnorm_bwd(int64_t n_rows, int f, const float* dZ, int64_t lddz, const float* H, int64_t ldh, const float* stats,
                             const float* d_beta, const float* d_gamma, float keep_scale, int relu, float* G, int64_t ldg,
                             float* d_bias, void* workspace, size_t workspace_bytes, acm_reduce_list_t* defer, acm_stream_t stream) {
    ACM_REQUIRE(dZ && H && G && d_bias, ACM_EINVAL, "acm_bnorm_bwd: NULL argument");
    ACM_REQUIRE(!stats || (d_beta && d_gamma), ACM_EINVAL, "acm_bnorm_bwd: statistics without d_beta / d_gamma");
    size_t need = 0;
    const int st = acm_bnorm_bwd_workspace_bytes(n_rows, f, &need);
    if (st != ACM_OK) return st;
    ACM_REQUIRE(n_rows >= 1, ACM_ESHAPE, "acm_bnorm_bwd: no rows");
    ACM_REQUIRE(lddz >= f && ldh >= f && ldg >= f && keep_scale >= 1.f, ACM_ESHAPE, "acm_bnorm_bwd: leading dimensions / scale");
    ACM_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace) % 16 == 0, ACM_ENOMEM,
                "acm_bnorm_bwd: workspace %zu B < required %zu B (or not 16-byte aligned)", workspace_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    const int nblk = bn_blocks(n_rows);
    const long rpb = bn_rows_per_block(n_rows);
    float* partial = (float*)workspace;
    const BnBwd p = {stats, d_beta, d_gamma, 1.f / (float)n_rows, keep_scale, relu};
    if (bn_vec4(f, {dZ, H, G}, {lddz, ldh, ldg}))
        hipLaunchKernelGGL(bn_bwd_kernel<4>, dim3(nblk), dim3(256), 0, s, (long)n_rows, f, dZ, (long)lddz, H, (long)ldh, p, G, (long)ldg,
                           rpb, partial);
    else
        hipLaunchKernelGGL(bn_bwd_kernel<1>, dim3(nblk), dim3(256), 0, s, (long)n_rows, f, dZ, (long)lddz, H, (long)ldh, p, G, (long)ldg,
                           rpb, partial);
    ACM_CHECK_HIP(hipGetLastError());
    const acm_reduce_seg_t seg = {partial, nblk, 32, 0, f, d_bias, f, 0, 0, 0, nblk * 32, 0};
    return acm_reduce_emit(defer, &seg, 1, s);
}
