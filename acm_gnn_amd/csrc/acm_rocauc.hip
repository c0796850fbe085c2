// ROC-AUC of up to eight index sets from eval-mode logits, in exact integers (gfx950).
//
//   acm_rocauc_scores   s_i = softmax(z_i)[1], one thread per row, the row maximum subtracted first
//   (the caller sorts the n scores once, ascending, and hands back the sorted scores and the int64 order)
//   acm_rocauc          four launches over the SORTED positions, tiles of 1024 (256 threads x 4 consecutive positions):
//     1. flags + tile counts   position j -> row r = order[j] -> one 16-bit record: bit k = "negative member of set k",
//                              bit 8 + k = "positive member of set k"; per tile and set the number of negatives
//     2. scan of tile counts   one block per set: exclusive prefix of the tile counts; zeroes the result, writes nneg
//     3. apply                 negpre[k][j] = negatives of set k at sorted positions < j, for j = 0 .. n
//     4. statistic             every positive finds the bounds [lo, hi) of its tie group (neighbour compare first, binary
//                              search in the sorted scores otherwise) and adds negpre[lo] + negpre[hi] = 2 #less + #equal;
//                              64-bit integer sums per wave, per block, then integer atomics: any order gives the same
//                              bits.  The block that arrives last turns the triples into float64 AUCs.
// No kernel waits for another block; nothing is allocated; the arrival counter is zeroed by launch 2 of the same call.
#include <math.h>

#include "acm_common.h"

namespace {

constexpr int AUC_MAX_SETS = 8;
constexpr int AUC_TILE = 1024;            // sorted positions per block
constexpr int AUC_PER_THREAD = 4;

__global__ __launch_bounds__(256) void rocauc_scores_kernel(int n, int C, const float* __restrict__ z, long ldz,
                                                            float* __restrict__ scores) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float* zi = z + i * ldz;
        float m = zi[0];
        for (int c = 1; c < C; ++c) m = fmaxf(m, zi[c]);
        float se = 0.f;
        for (int c = 0; c < C; ++c) se += expf(zi[c] - m);
        scores[i] = expf(zi[1] - m) / se;
    }
}

struct AucWs {
    unsigned short* flags;      // [n + 1] (+ padding)
    int* tile_pre;              // [k][nblk]: tile counts, then their exclusive prefix
    int* negpre;                // [k][n + 1]
    int* arrive;                // one counter
    size_t bytes;
};

inline size_t auc_align(size_t b) { return (b + 15) & ~(size_t)15; }

inline long auc_tiles(int64_t n) { return (long)(n / AUC_TILE) + 1; }            // covers positions 0 .. n

inline AucWs auc_layout(void* base, int64_t n, int k) {
    const size_t nblk = (size_t)auc_tiles(n);
    const size_t o_flags = 0;
    const size_t o_tiles = o_flags + auc_align((size_t)(n + 1) * sizeof(unsigned short));
    const size_t o_pre = o_tiles + auc_align((size_t)k * nblk * sizeof(int));
    const size_t o_arrive = o_pre + auc_align((size_t)k * (size_t)(n + 1) * sizeof(int));
    AucWs w = {nullptr, nullptr, nullptr, nullptr, o_arrive + 16};
    if (base) {
        char* p = (char*)base;
        w.flags = (unsigned short*)(p + o_flags);
        w.tile_pre = (int*)(p + o_tiles);
        w.negpre = (int*)(p + o_pre);
        w.arrive = (int*)(p + o_arrive);
    }
    return w;
}

// Inclusive scan of one int per thread over the block's 256 threads (Hillis-Steele in LDS); returns the thread's
// inclusive value, *total = the block's sum.  Ends with a barrier, so `buf` can be reused right away.
__device__ __forceinline__ int auc_block_scan(int v, int* buf, int* total) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int add = t >= d ? buf[t - d] : 0;
        __syncthreads();
        buf[t] += add;
        __syncthreads();
    }
    const int inc = buf[t];
    *total = buf[255];
    __syncthreads();
    return inc;
}

__global__ __launch_bounds__(256) void rocauc_flags_kernel(long n, int S, const int64_t* __restrict__ order,
                                                           const int64_t* __restrict__ y, const float* __restrict__ w, long ldw,
                                                           unsigned short* __restrict__ flags, int* __restrict__ tile_cnt,
                                                           long nblk) {
    __shared__ int cnt[AUC_MAX_SETS];
    if (threadIdx.x < AUC_MAX_SETS) cnt[threadIdx.x] = 0;
    __syncthreads();
    int mine[AUC_MAX_SETS];
#pragma unroll
    for (int s = 0; s < AUC_MAX_SETS; ++s) mine[s] = 0;
    const long j0 = (long)blockIdx.x * AUC_TILE + (long)threadIdx.x * AUC_PER_THREAD;
#pragma unroll
    for (int q = 0; q < AUC_PER_THREAD; ++q) {
        const long j = j0 + q;
        if (j > n) break;
        unsigned f = 0;
        if (j < n) {
            const int64_t r = order[j];
            if (r >= 0 && r < n) {                         // (an order that is no permutation reads nothing out of range)
                const int64_t yi = y[r];
                if (yi == 0 || yi == 1) {
#pragma unroll
                    for (int s = 0; s < AUC_MAX_SETS; ++s) {
                        if (s < S && w[(long)s * ldw + r] != 0.f) {
                            f |= 1u << (s + (yi == 1 ? 8 : 0));
                            mine[s] += yi == 0;
                        }
                    }
                }
            }
        }
        flags[j] = (unsigned short)f;
    }
#pragma unroll
    for (int s = 0; s < AUC_MAX_SETS; ++s)
        if (s < S && mine[s]) atomicAdd(&cnt[s], mine[s]);              // LDS integer adds: order-free
    __syncthreads();
    if ((int)threadIdx.x < S) tile_cnt[(long)threadIdx.x * nblk + blockIdx.x] = cnt[threadIdx.x];
}

__global__ __launch_bounds__(256) void rocauc_scan_kernel(long nblk, int* __restrict__ tile_pre, long long* __restrict__ out,
                                                          int* __restrict__ arrive) {
    __shared__ int buf[256];
    const int s = blockIdx.x;
    int* row = tile_pre + (long)s * nblk;
    int carry = 0;
    for (long b0 = 0; b0 < nblk; b0 += 256) {
        const long b = b0 + threadIdx.x;
        const int v = b < nblk ? row[b] : 0;
        int total;
        const int inc = auc_block_scan(v, buf, &total);
        if (b < nblk) row[b] = carry + inc - v;
        carry += total;
    }
    if (threadIdx.x == 0) {
        out[3 * s + 0] = 0;
        out[3 * s + 1] = 0;
        out[3 * s + 2] = carry;                     // nneg
        if (s == 0) *arrive = 0;
    }
}

__global__ __launch_bounds__(256) void rocauc_apply_kernel(long n, int S, const unsigned short* __restrict__ flags,
                                                           const int* __restrict__ tile_pre, long nblk, int* __restrict__ negpre) {
    __shared__ int buf[256];
    const long j0 = (long)blockIdx.x * AUC_TILE + (long)threadIdx.x * AUC_PER_THREAD;
    unsigned f[AUC_PER_THREAD];
#pragma unroll
    for (int q = 0; q < AUC_PER_THREAD; ++q) f[q] = j0 + q <= n ? flags[j0 + q] : 0u;
    for (int s = 0; s < S; ++s) {
        int mine = 0;
#pragma unroll
        for (int q = 0; q < AUC_PER_THREAD; ++q) mine += (f[q] >> s) & 1u;
        int total;
        int run = tile_pre[(long)s * nblk + blockIdx.x] + auc_block_scan(mine, buf, &total) - mine;
        int* dst = negpre + (long)s * (n + 1);
#pragma unroll
        for (int q = 0; q < AUC_PER_THREAD; ++q) {
            if (j0 + q <= n) dst[j0 + q] = run;
            run += (f[q] >> s) & 1u;
        }
    }
}

// first index in [lo, hi) whose score is >= v (UPPER = false) or > v (UPPER = true); hi if none.  Always inside [lo, hi].
template <bool UPPER>
__device__ __forceinline__ long auc_bound(const float* __restrict__ a, long lo, long hi, float v) {
    while (lo < hi) {
        const long mid = lo + ((hi - lo) >> 1);
        const float x = a[mid];
        const bool left = UPPER ? !(x > v) : (x < v);        // "the answer lies to the right of mid"
        if (left) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ long long auc_wave_sum(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(256) void rocauc_stat_kernel(long n, int S, const float* __restrict__ sorted,
                                                          const unsigned short* __restrict__ flags,
                                                          const int* __restrict__ negpre, long long* __restrict__ out,
                                                          double* __restrict__ auc, int* __restrict__ arrive) {
    __shared__ unsigned long long acc[AUC_MAX_SETS][2];
    __shared__ int last;
    if (threadIdx.x < 2 * AUC_MAX_SETS) acc[threadIdx.x >> 1][threadIdx.x & 1] = 0ull;
    __syncthreads();
    long long u2[AUC_MAX_SETS], np[AUC_MAX_SETS];
#pragma unroll
    for (int s = 0; s < AUC_MAX_SETS; ++s) u2[s] = 0, np[s] = 0;
    const long j0 = (long)blockIdx.x * AUC_TILE + (long)threadIdx.x * AUC_PER_THREAD;
#pragma unroll
    for (int q = 0; q < AUC_PER_THREAD; ++q) {
        const long j = j0 + q;
        if (j >= n) break;
        const unsigned pos = flags[j] >> 8;
        if (!pos) continue;
        const float v = sorted[j];
        // the tie group [lo, hi) of position j: almost always j alone -- one compare with each neighbour settles it
        const long lo = (j == 0 || sorted[j - 1] < v) ? j : auc_bound<false>(sorted, 0, j, v);
        const long hi = (j + 1 == n || sorted[j + 1] > v) ? j + 1 : auc_bound<true>(sorted, j + 1, n, v);
#pragma unroll
        for (int s = 0; s < AUC_MAX_SETS; ++s) {
            if (s < S && ((pos >> s) & 1u)) {
                const int* pre = negpre + (long)s * (n + 1);
                u2[s] += (long long)pre[lo] + (long long)pre[hi];
                np[s] += 1;
            }
        }
    }
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int s = 0; s < AUC_MAX_SETS; ++s) {
        if (s < S) {                                     // (S is uniform)
            const long long a = auc_wave_sum(u2[s]), b = auc_wave_sum(np[s]);
            if (lane == 0 && b) {
                atomicAdd(&acc[s][0], (unsigned long long)a);
                atomicAdd(&acc[s][1], (unsigned long long)b);
            }
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * S) {
        const unsigned long long v = acc[threadIdx.x >> 1][threadIdx.x & 1];
        if (v) atomicAdd((unsigned long long*)out + 3 * (threadIdx.x >> 1) + (threadIdx.x & 1), v);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const int old = __hip_atomic_fetch_add(arrive, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = old == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!last || !auc) return;
    __threadfence();
    if ((int)threadIdx.x < S) {
        const long long* o = out + 3 * threadIdx.x;
        const double u = (double)__hip_atomic_load(o + 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double p = (double)__hip_atomic_load(o + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double q = (double)__hip_atomic_load(o + 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const double den = 2.0 * p * q;
        auc[threadIdx.x] = den > 0.0 ? u / den : (double)NAN;
    }
}

int scores_blocks(int64_t n) {
    int64_t nb = (n + 255) / 256;
    if (nb > 4096) nb = 4096;
    if (nb < 1) nb = 1;
    return (int)nb;
}

}  // namespace

extern "C" int acm_rocauc_scores(int64_t n_rows, int n_classes, const float* logits, int64_t ld_logits, float* scores,
                                 acm_stream_t stream) {
    ACM_REQUIRE(logits && scores, ACM_EINVAL, "acm_rocauc_scores: NULL pointer");
    ACM_REQUIRE(n_rows >= 0 && n_rows < INT32_MAX && n_classes >= 2, ACM_ESHAPE, "acm_rocauc_scores: bad sizes (column 1 is the score)");
    ACM_REQUIRE(n_classes <= 64, ACM_EUNSUPPORTED, "acm_rocauc_scores: %d classes > 64", n_classes);
    ACM_REQUIRE(ld_logits >= n_classes, ACM_ESHAPE, "acm_rocauc_scores: leading dimension too small");
    if (n_rows == 0) return ACM_OK;
    hipLaunchKernelGGL(rocauc_scores_kernel, dim3(scores_blocks(n_rows)), dim3(256), 0, (hipStream_t)stream, (int)n_rows,
                       n_classes, logits, (long)ld_logits, scores);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_rocauc_workspace_bytes(int64_t n_rows, int n_sets, size_t* bytes) {
    ACM_REQUIRE(bytes, ACM_EINVAL, "acm_rocauc_workspace_bytes: NULL argument");
    ACM_REQUIRE(n_rows >= 0 && n_rows < INT32_MAX && n_sets >= 1 && n_sets <= AUC_MAX_SETS, ACM_ESHAPE,
                "acm_rocauc_workspace_bytes: bad sizes");
    *bytes = auc_layout(nullptr, n_rows, n_sets).bytes;
    return ACM_OK;
}

extern "C" int acm_rocauc(int64_t n_rows, const float* sorted_scores, const int64_t* order, const int64_t* labels,
                          const float* weights, int64_t ld_weights, int n_sets, int64_t* counts, double* auc,
                          void* workspace, size_t workspace_bytes, acm_stream_t stream) {
    ACM_REQUIRE(sorted_scores && order && labels && weights && counts, ACM_EINVAL, "acm_rocauc: NULL pointer");   // (auc may be NULL)
    ACM_REQUIRE(n_sets >= 1 && n_sets <= AUC_MAX_SETS, ACM_ESHAPE, "acm_rocauc: %d index sets (1..%d)", n_sets, AUC_MAX_SETS);
    ACM_REQUIRE(n_rows >= 0 && n_rows < INT32_MAX && ld_weights >= n_rows, ACM_ESHAPE, "acm_rocauc: bad sizes");
    const AucWs ws = auc_layout(workspace, n_rows, n_sets);
    ACM_REQUIRE(workspace && workspace_bytes >= ws.bytes, ACM_ENOMEM, "acm_rocauc: workspace %zu B < required %zu B",
                workspace_bytes, ws.bytes);
    ACM_REQUIRE(((uintptr_t)workspace & 7) == 0, ACM_EINVAL, "acm_rocauc: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long nblk = auc_tiles(n_rows);
    const long n = (long)n_rows;
    hipLaunchKernelGGL(rocauc_flags_kernel, dim3((unsigned)nblk), dim3(256), 0, st, n, n_sets, order, labels, weights,
                       (long)ld_weights, ws.flags, ws.tile_pre, nblk);
    ACM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(rocauc_scan_kernel, dim3(n_sets), dim3(256), 0, st, nblk, ws.tile_pre, (long long*)counts, ws.arrive);
    ACM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(rocauc_apply_kernel, dim3((unsigned)nblk), dim3(256), 0, st, n, n_sets, ws.flags, ws.tile_pre, nblk,
                       ws.negpre);
    ACM_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(rocauc_stat_kernel, dim3((unsigned)nblk), dim3(256), 0, st, n, n_sets, sorted_scores, ws.flags, ws.negpre,
                       (long long*)counts, auc, ws.arrive);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}
