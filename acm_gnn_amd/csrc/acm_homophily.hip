// Homophily measures on the device (gfx950): the label census of a CSR pattern and aggregation homophily.
//
// The reference's synthetic-experiments/homophily.py forms dense n x n matrices (label @ label.T at :16, A.nonzero() at
// :31/:44/:97, (A X)(A X)^T at :115-117).  Here:
//
//   acm_homophily_census   three launches over the stored pattern, exact integers (homophily.py:8-19 edge, :40-60 node,
//                          :63-87 compatibility matrix, :90-111 class homophily)
//     1. prep     one byte per node: its class, 255 = unlabeled (negative or >= C); zeroes M, the per-row counters and the
//                 arrival counter.  Every later label lookup is one byte from a table smaller than an XCD's L2 (168 KB at
//                 twitch-gamer size, 1.6 MB at pokec size) instead of 8 B of int64 per edge.
//     2. edges    a 16-lane group per work item of the handle's own list (a row, or a piece of a long row), four items per
//                 wave at a time.  The row's class is group-uniform: 64 column ids per step (four coalesced 64 B loads per
//                 group, issued together), their byte labels, and either per-lane counters per class summed over the group
//                 once per item (C <= 8) or an LDS integer add per counted entry; the block's C x C histogram goes
//                 into M with 64-bit integer atomics.  Per-row counters: a plain store for a whole row, integer atomics for
//                 the pieces of a split row.
//     3. finish   one thread per row: cls, iso, n_labeled, n_deg in integers and node_sum = sum row_same / row_deg in
//                 float64 -- per thread in row order, a fixed shuffle tree per wave, per-block partials, and the block
//                 that arrives last adds the partials in block order (the acm_eval_metrics pattern): the same bits on
//                 every run.
//   acm_class_means        mu_k = mean of Z_u over y_u = k (the column mean that replaces
//                          mean(inner_prod[:, labels == k], 1), homophily.py:122-123): a wave owns a tile of rows and 64
//                          columns, lane = column, one private fp32 accumulator per class in LDS, rows in order; tiles are
//                          added in tile order in float64.  No float atomics.
//   acm_class_score        W[v][k] = Z_v . mu_k on v_mfma_f32_16x16x4_f32, sixteen rows per wave (mu staged in LDS), first
//                          arg-max over the classes that have a member, compared with the row's label
//                          (homophily.py:124); hits and scored rows are integer atomics.
#include <limits.h>
#include <math.h>

#include "acm_common.h"

namespace {

constexpr int HOM_MAX_C = 64;
constexpr int HOM_UNLABELED = 255;
constexpr int HOM_BALLOT_C = 8;           // up to here: per-lane counters per class instead of LDS adds
constexpr int HOM_FIN_BLOCKS = 256;       // finish: at most one partial per thread of the last block
constexpr int HOM_MEANS_MAX_TILES = 2048;
constexpr int HOM_SCORE_MAX_F = 256;

typedef float f32x4 __attribute__((ext_vector_type(4)));

inline size_t hom_align(size_t b) { return (b + 15) & ~(size_t)15; }

// ------------------------------------------------------------------------------------------------ census
struct HomWs {
    unsigned char* lab8;     // [n_cols]
    int* row_same;           // [n_rows] (used when the caller passes no array of its own)
    int* row_deg;            // [n_rows]
    int* row_off;            // [n_rows]: stored off-diagonal entries of a labeled row, whatever the neighbours' labels
    double* part_sum;        // [HOM_FIN_BLOCKS]
    int* part_cnt;           // [HOM_FIN_BLOCKS][2 C + 2]
    int* arrive;
    size_t bytes;
};

inline HomWs hom_layout(void* base, int64_t n_rows, int64_t n_cols, int C) {
    const size_t o_lab = 0;
    const size_t o_same = o_lab + hom_align((size_t)n_cols);
    const size_t o_deg = o_same + hom_align((size_t)n_rows * sizeof(int));
    const size_t o_off = o_deg + hom_align((size_t)n_rows * sizeof(int));
    const size_t o_psum = o_off + hom_align((size_t)n_rows * sizeof(int));
    const size_t o_pcnt = o_psum + hom_align((size_t)HOM_FIN_BLOCKS * sizeof(double));
    const size_t o_arrive = o_pcnt + hom_align((size_t)HOM_FIN_BLOCKS * (2 * C + 2) * sizeof(int));
    HomWs w = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, o_arrive + 16};
    if (base) {
        char* p = (char*)base;
        w.lab8 = (unsigned char*)(p + o_lab);
        w.row_same = (int*)(p + o_same);
        w.row_deg = (int*)(p + o_deg);
        w.row_off = (int*)(p + o_off);
        w.part_sum = (double*)(p + o_psum);
        w.part_cnt = (int*)(p + o_pcnt);
        w.arrive = (int*)(p + o_arrive);
    }
    return w;
}

__global__ __launch_bounds__(256) void hom_prep_kernel(long n_rows, long n_cols, int C, const int64_t* __restrict__ labels,
                                                       unsigned char* __restrict__ lab8, int* __restrict__ row_same,
                                                       int* __restrict__ row_deg, int* __restrict__ row_off,
                                                       long long* __restrict__ M, int* __restrict__ arrive) {
    const long total = n_cols > n_rows ? n_cols : n_rows;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        if (i < n_cols) {
            const int64_t y = labels[i];
            lab8[i] = (y >= 0 && y < C) ? (unsigned char)y : (unsigned char)HOM_UNLABELED;   // a label never becomes an index outside [0, C)
        }
        if (i < n_rows) row_same[i] = 0, row_deg[i] = 0, row_off[i] = 0;
    }
    if (blockIdx.x == 0) {
        for (int t = threadIdx.x; t < C * C; t += 256) M[t] = 0;
        if (threadIdx.x == 0) *arrive = 0;
    }
}

// sum over the 16 lanes of a group (xor 8, 4, 2, 1 never leave it); every lane of the group must be active
__device__ __forceinline__ int hom_group_sum(int v) {
#pragma unroll
    for (int d = 8; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// A 16-lane group per work item, four items per wave at a time: an item is a chain of dependent round trips (descriptor,
// the row's label, column ids, their labels), so what hides it is more items in flight, not wider ones.  A step takes 64
// entries of the item -- four id loads per lane issued together, then their four byte labels.  SMALL (C <= 8): per-lane
// counters per class, summed over the group once per item; otherwise one LDS integer add per counted entry.
template <bool SMALL>
__global__ __launch_bounds__(256) void hom_edges_kernel(const AcmItem* __restrict__ items, long n_items,
                                                        const int32_t* __restrict__ indices, long row_offset, long n_cols, int C,
                                                        const unsigned char* __restrict__ lab8, int* __restrict__ row_same,
                                                        int* __restrict__ row_deg, int* __restrict__ row_off,
                                                        unsigned long long* __restrict__ M) {
    extern __shared__ int hist[];             // [C][C]
    for (int t = threadIdx.x; t < C * C; t += 256) hist[t] = 0;
    __syncthreads();
    const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15;
    for (long it = (long)blockIdx.x * 16 + grp; it < n_items; it += (long)gridDim.x * 16) {
        const AcmItem item = items[it];                              // group-uniform, and so is all control flow below
        if (item.begin >= item.end) continue;                        // (an empty row keeps the zeros of the prep launch)
        const long self = row_offset + item.row;
        const int a = lab8[self];
        if (a == HOM_UNLABELED) continue;
        int same = 0, deg = 0, off = 0;
        int cnt[HOM_BALLOT_C];
#pragma unroll
        for (int c = 0; c < HOM_BALLOT_C; ++c) cnt[c] = 0;
        for (int p0 = item.begin; p0 < item.end; p0 += 64) {
            long j[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int p = p0 + 16 * u + gl;
                j[u] = p < item.end ? (long)indices[p] : -1;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const bool offd = j[u] >= 0 && j[u] != self && j[u] < n_cols;
                const int b = offd ? (int)lab8[j[u]] : HOM_UNLABELED;
                const bool valid = b != HOM_UNLABELED;
                off += offd, deg += valid, same += valid && b == a;
                if (SMALL) {
#pragma unroll
                    for (int c = 0; c < HOM_BALLOT_C; ++c) cnt[c] += b == c;
                } else if (valid) {
                    atomicAdd(&hist[a * C + b], 1);                  // LDS integer add: order-free
                }
            }
        }
        same = hom_group_sum(same), deg = hom_group_sum(deg), off = hom_group_sum(off);
        if (SMALL) {
#pragma unroll
            for (int c = 0; c < HOM_BALLOT_C; ++c) {
                if (c < C) {                                         // (C is uniform)
                    const int v = hom_group_sum(cnt[c]);
                    if (gl == 0 && v) atomicAdd(&hist[a * C + c], v);
                }
            }
        }
        if (gl == 0) {
            if (item.slot < 0) {                                     // the whole row: its only writer
                row_same[item.row] = same, row_deg[item.row] = deg, row_off[item.row] = off;
            } else {                                                 // a piece of a split row
                if (same) atomicAdd(&row_same[item.row], same);
                if (deg) atomicAdd(&row_deg[item.row], deg);
                if (off) atomicAdd(&row_off[item.row], off);
            }
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < C * C; t += 256) {
        const int v = hist[t];
        if (v) atomicAdd(M + t, (unsigned long long)v);
    }
}

__device__ __forceinline__ double hom_wave_sum(double v) {            // a fixed tree: the same bits on every run
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__global__ __launch_bounds__(256) void hom_finish_kernel(long n_rows, long row_offset, int C, const unsigned char* __restrict__ lab8,
                                                         const int* __restrict__ row_same, const int* __restrict__ row_deg,
                                                         const int* __restrict__ row_off, double* __restrict__ part_sum,
                                                         int* __restrict__ part_cnt, int* __restrict__ arrive,
                                                         long long* __restrict__ tail /* counts + C*C */, double* __restrict__ node_sum) {
    __shared__ int cnt[2 * HOM_MAX_C + 2];     // cls[C], iso[C], n_labeled, n_deg
    __shared__ double red[4];
    __shared__ int last;
    const int nslot = 2 * C + 2;
    if ((int)threadIdx.x < nslot) cnt[threadIdx.x] = 0;
    __syncthreads();
    double ns = 0.0;
    int nl = 0, nd = 0;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n_rows; i += (long)gridDim.x * 256) {
        const int a = lab8[row_offset + i];
        if (a == HOM_UNLABELED) continue;
        nl += 1;
        atomicAdd(&cnt[a], 1);
        if (row_off[i] == 0) atomicAdd(&cnt[C + a], 1);
        const int d = row_deg[i];
        if (d > 0) {
            nd += 1;
            ns += (double)row_same[i] / (double)d;
        }
    }
    if (nl) atomicAdd(&cnt[2 * C], nl);
    if (nd) atomicAdd(&cnt[2 * C + 1], nd);
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    ns = hom_wave_sum(ns);
    if (lane == 0) red[wv] = ns;
    __syncthreads();
    if ((int)threadIdx.x < nslot)
        __hip_atomic_store(part_cnt + (long)blockIdx.x * nslot + threadIdx.x, cnt[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (threadIdx.x == 0)
        __hip_atomic_store((long long*)part_sum + blockIdx.x, __double_as_longlong((red[0] + red[1]) + (red[2] + red[3])),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence();
        const int old = __hip_atomic_fetch_add(arrive, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        last = old == (int)gridDim.x - 1;
    }
    __syncthreads();
    if (!last) return;
    __threadfence();
    if ((int)threadIdx.x < nslot) {
        long long s = 0;
        for (int b = 0; b < (int)gridDim.x; ++b)
            s += __hip_atomic_load(part_cnt + (long)b * nslot + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        tail[threadIdx.x] = s;
    }
    double v = 0.0;                            // thread b takes block b's sum (gridDim.x <= 256), then the same fixed tree
    if (threadIdx.x < gridDim.x)
        v = __longlong_as_double(__hip_atomic_load((long long*)part_sum + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    v = hom_wave_sum(v);
    __syncthreads();
    if (lane == 0) red[wv] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        *node_sum = (red[0] + red[1]) + (red[2] + red[3]);
        __hip_atomic_store(arrive, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ------------------------------------------------------------------------------------------------ class means
inline int means_tile_rows(int64_t n) {
    int64_t t = (n + HOM_MEANS_MAX_TILES - 1) / HOM_MEANS_MAX_TILES;
    t = (t + 63) / 64 * 64;
    return (int)(t < 128 ? 128 : t);
}

struct MeansWs {
    float* part;             // [tiles][C][F]
    int* part_cnt;           // [tiles][C]
    long tiles;
    size_t bytes;
};

inline MeansWs means_layout(void* base, int64_t n, int F, int C) {
    const int rows = means_tile_rows(n);
    const long tiles = (long)((n + rows - 1) / rows);
    const size_t o_part = 0;
    const size_t o_cnt = o_part + hom_align((size_t)tiles * C * F * sizeof(float));
    MeansWs w = {nullptr, nullptr, tiles, o_cnt + hom_align((size_t)tiles * C * sizeof(int)) + 16};
    if (base) {
        w.part = (float*)((char*)base + o_part);
        w.part_cnt = (int*)((char*)base + o_cnt);
    }
    return w;
}

// two waves per block, a wave = one tile of rows x 64 columns (blockIdx.y = column slab); the wave's accumulators are its own
// LDS region (no barrier: a wave's LDS accesses are ordered)
__global__ __launch_bounds__(128) void means_tile_kernel(long n, int F, int C, const float* __restrict__ Z, long ldz,
                                                         const int64_t* __restrict__ y, int tile_rows, long tiles,
                                                         float* __restrict__ part, int* __restrict__ part_cnt) {
    extern __shared__ float acc[];             // [2][C][64] floats, then [2][C] ints
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long tile = (long)blockIdx.x * 2 + wv;
    if (tile >= tiles) return;
    float* my = acc + (long)wv * C * 64;
    int* mycnt = (int*)(acc + 2L * C * 64) + wv * C;
    for (int c = 0; c < C; ++c) my[c * 64 + lane] = 0.f;
    if (lane < C) mycnt[lane] = 0;
    const int col = blockIdx.y * 64 + lane;
    const long r0 = tile * tile_rows;
    const long r1 = r0 + tile_rows < n ? r0 + tile_rows : n;
#pragma unroll 4
    for (long r = r0; r < r1; ++r) {
        const int64_t yy = y[r];                                     // wave-uniform
        const float z = col < F ? Z[r * ldz + col] : 0.f;
        if (yy < 0 || yy >= C) continue;
        my[(int)yy * 64 + lane] += z;                                // rows in order: a fixed fp32 sum
        if (lane == 0) mycnt[yy] += 1;
    }
    if (col < F)
        for (int c = 0; c < C; ++c) part[(tile * C + c) * F + col] = my[c * 64 + lane];
    if (blockIdx.y == 0 && lane < C) part_cnt[tile * C + lane] = mycnt[lane];
}

__global__ __launch_bounds__(256) void means_finish_kernel(int F, int C, long tiles, const float* __restrict__ part,
                                                           const int* __restrict__ part_cnt, float* __restrict__ mu, long ld_mu,
                                                           long long* __restrict__ class_count) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= C * F) return;
    const int c = idx / F, f = idx - c * F;
    double s = 0.0;
    long long k = 0;
    for (long t = 0; t < tiles; ++t) {                               // tile order, float64
        s += (double)part[(t * C + c) * F + f];
        k += part_cnt[t * C + c];
    }
    mu[(long)c * ld_mu + f] = k > 0 ? (float)(s / (double)k) : 0.f;
    if (f == 0) class_count[c] = k;
}

// ------------------------------------------------------------------------------------------------ score
// LDS copy of mu for the MFMA's A operand: row = class (T * 16 of them, zero rows beyond C), Fp = F rounded up to 16 columns
// (zeros beyond F).  A lane reads four consecutive floats of its class row per step; rows are padded by four floats, or --
// where Fp is a multiple of 64, 256 included, so that 64 x 256 floats stay within 64 KB -- the 16-byte pieces of a row are
// XOR-swizzled with the row index inside each 64-float block.
__device__ __forceinline__ int score_lds_at(int c, int f, int FS, bool swz) {
    return c * FS + (swz ? (f ^ ((c & 15) << 2)) : f);
}

template <int T>
__global__ __launch_bounds__(256) void score_kernel(long n, int F, int C, const float* __restrict__ Z, long ldz,
                                                    const float* __restrict__ mu, long ld_mu,
                                                    const long long* __restrict__ class_count, const int64_t* __restrict__ y,
                                                    unsigned char* __restrict__ row_hit, unsigned long long* __restrict__ out,
                                                    int vec4) {
    extern __shared__ float smu[];
    const int Fp = (F + 15) & ~15;
    const bool swz = (Fp & 63) == 0;
    const int FS = swz ? Fp : Fp + 4;
    for (int idx = threadIdx.x; idx < T * 16 * Fp; idx += 256) {
        const int c = idx / Fp, f = idx - c * Fp;
        smu[score_lds_at(c, f, FS, swz)] = (c < C && f < F) ? mu[(long)c * ld_mu + f] : 0.f;
    }
    __syncthreads();
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = lane & 15, q = lane >> 4;
    // the classes this lane's MFMA results belong to: 16 t + 4 q + r; bit 4 t + r = "has a member"
    unsigned okmask = 0;
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 16 * t + 4 * q + r;
            if (c < C && class_count[c] > 0) okmask |= 1u << (4 * t + r);
        }
    int hits = 0, scored = 0;
    for (long g = (long)blockIdx.x * 4 + wv; g * 16 < n; g += (long)gridDim.x * 4) {
        const long row = g * 16 + m;
        const bool rin = row < n;
        const float* zr = Z + (rin ? row : 0) * ldz;
        f32x4 D[T];
#pragma unroll
        for (int t = 0; t < T; ++t) D[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j < Fp / 16; ++j) {
            const int f0 = 16 * j + 4 * q;
            float z[4];
            if (vec4) {                                              // uniform: F, ld and the base allow 16-byte loads
                const f32x4 v = (rin && f0 < F) ? *(const f32x4*)(zr + f0) : (f32x4){0.f, 0.f, 0.f, 0.f};
                z[0] = v[0], z[1] = v[1], z[2] = v[2], z[3] = v[3];
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) z[s] = (rin && f0 + s < F) ? zr[f0 + s] : 0.f;
            }
#pragma unroll
            for (int t = 0; t < T; ++t) {
                const f32x4 a = *(const f32x4*)(smu + score_lds_at(16 * t + m, f0, FS, swz));
#pragma unroll
                for (int s = 0; s < 4; ++s) D[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], z[s], D[t], 0, 0, 0);
            }
        }
        // D[t][r] = W[row m][class 16 t + 4 q + r]: first arg-max inside the lane (classes ascend), then over the four lanes
        // of the row (lane ^ 16, lane ^ 32); a class without a member scores -inf and is never chosen
        float best = -INFINITY;
        int arg = 4 * q;
#pragma unroll
        for (int t = 0; t < T; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float w = (okmask >> (4 * t + r)) & 1u ? D[t][r] : -INFINITY;
                if (w > best) best = w, arg = 16 * t + 4 * q + r;
            }
#pragma unroll
        for (int d = 16; d <= 32; d <<= 1) {
            const float ob = __shfl_xor(best, d, 64);
            const int oa = __shfl_xor(arg, d, 64);
            if (ob > best || (ob == best && oa < arg)) best = ob, arg = oa;
        }
        if (q == 0 && rin) {
            const int64_t yy = y[row];
            const bool labeled = yy >= 0 && yy < C;
            const bool hit = labeled && (int64_t)arg == yy;
            if (row_hit) row_hit[row] = hit ? 1 : 0;
            hits += hit, scored += labeled;
        }
    }
    int hs = hits, sc = scored;                // per-lane counts -> one pair of integer atomics per wave
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) hs += __shfl_xor(hs, d, 64), sc += __shfl_xor(sc, d, 64);
    if (lane == 0) {
        if (hs) atomicAdd(out + 0, (unsigned long long)hs);
        if (sc) atomicAdd(out + 1, (unsigned long long)sc);
    }
}

inline int hom_blocks(int64_t work, int per_block, int cap) {
    int64_t nb = (work + per_block - 1) / per_block;
    if (nb > cap) nb = cap;
    if (nb < 1) nb = 1;
    return (int)nb;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int acm_homophily_workspace_bytes(int64_t n_rows, int64_t n_cols, int n_classes, size_t* bytes) {
    ACM_REQUIRE(bytes, ACM_EINVAL, "acm_homophily_workspace_bytes: NULL argument");
    ACM_REQUIRE(n_classes >= 2 && n_rows >= 0 && n_cols >= 0 && n_rows < INT32_MAX && n_cols < INT32_MAX, ACM_ESHAPE,
                "acm_homophily_workspace_bytes: bad sizes (n_classes >= 2)");
    ACM_REQUIRE(n_classes <= HOM_MAX_C, ACM_EUNSUPPORTED, "acm_homophily_workspace_bytes: %d classes > %d", n_classes, HOM_MAX_C);
    *bytes = hom_layout(nullptr, n_rows, n_cols, n_classes).bytes;
    return ACM_OK;
}

extern "C" int acm_homophily_census(const acm_csr_t* a, const int64_t* labels, int64_t row_offset, int n_classes,
                                    int64_t* counts, double* node_sum, int32_t* row_same, int32_t* row_deg,
                                    void* workspace, size_t workspace_bytes, acm_stream_t stream) {
    ACM_REQUIRE(n_classes >= 2, ACM_ESHAPE, "acm_homophily_census: %d classes (2..%d)", n_classes, HOM_MAX_C);
    ACM_REQUIRE(n_classes <= HOM_MAX_C, ACM_EUNSUPPORTED, "acm_homophily_census: %d classes > %d", n_classes, HOM_MAX_C);
    ACM_REQUIRE(a && labels && counts && node_sum, ACM_EINVAL, "acm_homophily_census: NULL pointer");   // (row_same / row_deg may be NULL)
    ACM_REQUIRE(row_offset >= 0 && row_offset + a->n_rows <= a->n_cols, ACM_ESHAPE,
                "acm_homophily_census: rows [%lld, %lld) are no columns of an operator with %lld columns", (long long)row_offset,
                (long long)(row_offset + a->n_rows), (long long)a->n_cols);
    const HomWs ws = hom_layout(workspace, a->n_rows, a->n_cols, n_classes);
    ACM_REQUIRE(workspace && workspace_bytes >= ws.bytes, ACM_ENOMEM, "acm_homophily_census: workspace %zu B < required %zu B",
                workspace_bytes, ws.bytes);
    ACM_REQUIRE(((uintptr_t)workspace & 7) == 0, ACM_EINVAL, "acm_homophily_census: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int C = n_classes;
    const long n_rows = (long)a->n_rows, n_cols = (long)a->n_cols;
    int* rs = row_same ? row_same : ws.row_same;
    int* rd = row_deg ? row_deg : ws.row_deg;
    long long* M = (long long*)counts;
    hipLaunchKernelGGL(hom_prep_kernel, dim3(hom_blocks(n_cols > n_rows ? n_cols : n_rows, 256, 4096)), dim3(256), 0, st, n_rows,
                       n_cols, C, labels, ws.lab8, rs, rd, ws.row_off, M, ws.arrive);
    ACM_CHECK_HIP(hipGetLastError());
    if (a->n_items > 0) {
        const int nb = hom_blocks(a->n_items, 64, 2048);             // a 16-lane group takes about four items
        const size_t lds = (size_t)C * C * sizeof(int);
        if (C <= HOM_BALLOT_C)
            hipLaunchKernelGGL(hom_edges_kernel<true>, dim3(nb), dim3(256), lds, st, a->items, (long)a->n_items, a->indices,
                               (long)row_offset, n_cols, C, ws.lab8, rs, rd, ws.row_off, (unsigned long long*)M);
        else
            hipLaunchKernelGGL(hom_edges_kernel<false>, dim3(nb), dim3(256), lds, st, a->items, (long)a->n_items, a->indices,
                               (long)row_offset, n_cols, C, ws.lab8, rs, rd, ws.row_off, (unsigned long long*)M);
        ACM_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(hom_finish_kernel, dim3(hom_blocks(n_rows, 256, HOM_FIN_BLOCKS)), dim3(256), 0, st, n_rows, (long)row_offset,
                       C, ws.lab8, rs, rd, ws.row_off, ws.part_sum, ws.part_cnt, ws.arrive, M + (long)C * C, node_sum);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_class_means_workspace_bytes(int64_t n_rows, int n_features, int n_classes, size_t* bytes) {
    ACM_REQUIRE(bytes, ACM_EINVAL, "acm_class_means_workspace_bytes: NULL argument");
    ACM_REQUIRE(n_classes >= 2 && n_rows >= 0 && n_rows < INT32_MAX && n_features >= 1, ACM_ESHAPE,
                "acm_class_means_workspace_bytes: bad sizes (n_classes >= 2, n_features >= 1)");
    ACM_REQUIRE(n_classes <= HOM_MAX_C, ACM_EUNSUPPORTED, "acm_class_means_workspace_bytes: %d classes > %d", n_classes, HOM_MAX_C);
    *bytes = means_layout(nullptr, n_rows, n_features, n_classes).bytes;
    return ACM_OK;
}

extern "C" int acm_class_means(int64_t n_rows, int n_features, int n_classes, const float* z, int64_t ld_z,
                               const int64_t* labels, float* mu, int64_t ld_mu, int64_t* class_count, void* workspace,
                               size_t workspace_bytes, acm_stream_t stream) {
    ACM_REQUIRE(z && labels && mu && class_count, ACM_EINVAL, "acm_class_means: NULL pointer");
    ACM_REQUIRE(n_classes >= 2 && n_rows >= 0 && n_rows < INT32_MAX && n_features >= 1, ACM_ESHAPE,
                "acm_class_means: bad sizes (n_classes >= 2, n_features >= 1)");
    ACM_REQUIRE(n_classes <= HOM_MAX_C, ACM_EUNSUPPORTED, "acm_class_means: %d classes > %d", n_classes, HOM_MAX_C);
    ACM_REQUIRE(ld_z >= n_features && ld_mu >= n_features, ACM_ESHAPE, "acm_class_means: leading dimension too small");
    const MeansWs ws = means_layout(workspace, n_rows, n_features, n_classes);
    ACM_REQUIRE(workspace && workspace_bytes >= ws.bytes, ACM_ENOMEM, "acm_class_means: workspace %zu B < required %zu B",
                workspace_bytes, ws.bytes);
    ACM_REQUIRE(((uintptr_t)workspace & 7) == 0, ACM_EINVAL, "acm_class_means: workspace must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const int F = n_features, C = n_classes;
    if (ws.tiles > 0) {
        const size_t lds = 2 * (size_t)C * 64 * sizeof(float) + 2 * (size_t)C * sizeof(int);
        hipLaunchKernelGGL(means_tile_kernel, dim3((unsigned)((ws.tiles + 1) / 2), (unsigned)((F + 63) / 64)), dim3(128), lds, st,
                           (long)n_rows, F, C, z, (long)ld_z, labels, means_tile_rows(n_rows), ws.tiles, ws.part, ws.part_cnt);
        ACM_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(means_finish_kernel, dim3((unsigned)((C * F + 255) / 256)), dim3(256), 0, st, F, C, ws.tiles, ws.part,
                       ws.part_cnt, mu, (long)ld_mu, (long long*)class_count);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_class_score(int64_t n_rows, int n_features, int n_classes, const float* z, int64_t ld_z, const float* mu,
                               int64_t ld_mu, const int64_t* class_count, const int64_t* labels, uint8_t* row_hit,
                               int64_t* counts, acm_stream_t stream) {
    ACM_REQUIRE(z && mu && class_count && labels && counts, ACM_EINVAL, "acm_class_score: NULL pointer");   // (row_hit may be NULL)
    ACM_REQUIRE(n_classes >= 2 && n_rows >= 0 && n_rows < INT32_MAX && n_features >= 1, ACM_ESHAPE,
                "acm_class_score: bad sizes (n_classes >= 2, n_features >= 1)");
    ACM_REQUIRE(n_classes <= HOM_MAX_C, ACM_EUNSUPPORTED, "acm_class_score: %d classes > %d", n_classes, HOM_MAX_C);
    ACM_REQUIRE(n_features <= HOM_SCORE_MAX_F, ACM_EUNSUPPORTED,
                "acm_class_score: %d features > %d (form W = Z mu^T with acm_gemm and score W against the identity)", n_features,
                HOM_SCORE_MAX_F);
    ACM_REQUIRE(ld_z >= n_features && ld_mu >= n_features, ACM_ESHAPE, "acm_class_score: leading dimension too small");
    hipStream_t st = (hipStream_t)stream;
    ACM_CHECK_HIP(hipMemsetAsync(counts, 0, 2 * sizeof(int64_t), st));
    if (n_rows == 0) return ACM_OK;
    const int F = n_features, C = n_classes;
    const int T = (C + 15) / 16;
    const int Fp = (F + 15) & ~15;
    const int FS = (Fp & 63) == 0 ? Fp : Fp + 4;
    const size_t lds = (size_t)T * 16 * FS * sizeof(float);           // <= 64 x 256 x 4 B = 64 KB
    const int nb = hom_blocks(n_rows, 64, lds > 16384 ? 512 : 2048);
    const int vec4 = (F % 4 == 0) && (ld_z % 4 == 0) && (((uintptr_t)z & 15) == 0);
    const int rc = acm_pick([&](auto TT) {
        hipLaunchKernelGGL(score_kernel<TT()>, dim3(nb), dim3(256), lds, st, (long)n_rows, F, C, z, (long)ld_z, mu, (long)ld_mu,
                           (const long long*)class_count, labels, (unsigned char*)row_hit, (unsigned long long*)counts, vec4);
        return ACM_OK;
    }, acm_one_of<1, 2, 3, 4>(T));
    ACM_REQUIRE(rc == ACM_OK, ACM_EUNSUPPORTED, "acm_class_score: no score_kernel for %d class tiles", T);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}
