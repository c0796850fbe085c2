// Synthetic homophily-controlled graphs and uniform features, written as CSR on the device (contract: include/acm_hip.h,
// "synthetic graphs").  Every random number is an acm_philox7 word addressed by (seed, graph index, stream tag, row or call
// number, block): nothing depends on the grid, the block size, the launch order or the order atomics arrive in.
//   regular   one wave per row: two Floyd samples held in registers (ballot membership test), the row sorted by rank in
//             LDS and stored as d contiguous ids
//   random    draw (64-bit value -> slot -> key), [torch stable sort], mark first occurrences, rank them in draw order
//             (three-phase scan over 4096-draw chunks), select rank < M, emit both directions + integer block counts
#include "acm_common.h"

namespace {

constexpr int SYN_MAX_C = 64;
constexpr int SYN_MAX_D = ACM_SYNTH_MAX_DEGREE;   // 256 = 64 lanes x the four words of one Philox call
constexpr int SYN_CHUNK = 4096;                   // draws per block of the scan: 256 threads x 16 flag bytes
constexpr long long SYN_INVALID = INT64_MAX;
constexpr unsigned SYN_TAG_REG_INTRA = 0x5301, SYN_TAG_REG_INTER = 0x5302, SYN_TAG_PAIR = 0x5303, SYN_TAG_RECT = 0x5304,
                   SYN_TAG_UNIFORM = 0x5305, SYN_TAG_RANGE = 0x5306;

__device__ __forceinline__ AcmDropCtx syn_ctx(unsigned long long seed, unsigned long long graph_index, unsigned tag) {
    AcmDropCtx c;
    c.k0 = (unsigned)seed, c.k1 = (unsigned)(seed >> 32);
    c.c2 = (unsigned)graph_index, c.c3 = (unsigned)(graph_index >> 32);
    c.tag16 = tag << 16;
    c.thresh = 0, c.inv_keep = 1.f, c.row_offset = 0, c.on = true;
    return c;
}

// ------------------------------------------------------------------------------------------------ regular
// Floyd: k distinct of [0, m) for one row, by one wave.  Lane l draws the Philox call with block l = words 4 l .. 4 l + 3;
// step s uses word s.  The chosen set lives in registers: entry s in lane s & 63, register s >> 6, -1 elsewhere.
__device__ __forceinline__ void syn_floyd(const AcmDropCtx& cx, long row, int k, unsigned m, int lane, int (&c)[4]) {
    c[0] = c[1] = c[2] = c[3] = -1;
    if (k == 0) return;
    unsigned w[4];
    acm_philox7(cx, row, lane, w);
    for (int s = 0; s < k; ++s) {                                   // (k is wave-uniform)
        const unsigned t = m - (unsigned)k + (unsigned)s;
        const int ws = s & 3;
        const unsigned mine = ws == 0 ? w[0] : (ws == 1 ? w[1] : (ws == 2 ? w[2] : w[3]));
        const unsigned word = (unsigned)__builtin_amdgcn_readlane((int)mine, __builtin_amdgcn_readfirstlane(s >> 2));
        const int r = (int)(((unsigned long long)word * ((unsigned long long)t + 1ull)) >> 32);
        const bool hit = c[0] == r || c[1] == r || c[2] == r || c[3] == r;
        const int v = __ballot(hit) != 0ull ? (int)t : r;
        if (lane == (s & 63)) {
            const int q = s >> 6;
            if (q == 0) c[0] = v;
            else if (q == 1) c[1] = v;
            else if (q == 2) c[2] = v;
            else c[3] = v;
        }
    }
}

__global__ __launch_bounds__(256) void syn_regular_kernel(int C, long npc, int k_in, int k_out, unsigned long long seed,
                                                          unsigned long long graph_index, long row_begin, long row_end,
                                                          int* __restrict__ out) {
    __shared__ int raw[4][SYN_MAX_D];
    __shared__ int srt[4][SYN_MAX_D];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const long j = row_begin + (long)blockIdx.x * 4 + wv;
    const bool live = j < row_end;
    const long jj = live ? j : row_begin;                           // an idle wave repeats a row and stores nothing
    const long cls = jj / npc, base = cls * npc, n = (long)C * npc;
    const int jl = (int)(jj - base);
    int a[4], b[4];
    syn_floyd(syn_ctx(seed, graph_index, SYN_TAG_REG_INTRA), jj, k_in, (unsigned)(npc - 1), lane, a);
    syn_floyd(syn_ctx(seed, graph_index, SYN_TAG_REG_INTER), jj, k_out, (unsigned)(n - npc), lane, b);
    const int d = k_in + k_out;                                     // <= SYN_MAX_D
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int s = q * 64 + lane;
        if (s < k_in) raw[wv][s] = (int)base + a[q] + (a[q] >= jl ? 1 : 0);          // own block without j
        if (s < k_out) raw[wv][k_in + s] = b[q] + ((long)b[q] >= base ? (int)npc : 0);   // every node outside the block
    }
    __syncthreads();
    for (int e = lane; e < d; e += 64) {                            // the ids are distinct: rank = ids below mine
        const int v = raw[wv][e];
        int rank = 0;
        for (int u = 0; u < d; ++u) rank += raw[wv][u] < v ? 1 : 0;
        srt[wv][rank] = v;
    }
    __syncthreads();
    if (live)
        for (int e = lane; e < d; e += 64) out[(j - row_begin) * d + e] = srt[wv][e];
}

// ------------------------------------------------------------------------------------------------ uniform features
typedef float syn_f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void syn_uniform_kernel(long n_rows, long F, long F4, unsigned long long seed,
                                                          unsigned long long graph_index, long row_begin,
                                                          float* __restrict__ out, long ld, int vec4) {
    const AcmDropCtx cx = syn_ctx(seed, graph_index, SYN_TAG_UNIFORM);
    const long total = n_rows * F4;
    for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
        const long r = idx / F4, blk = idx - r * F4;
        unsigned w[4];
        acm_philox7(cx, row_begin + r, (int)blk, w);
        float v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (float)(w[i] >> 8) * 0x1p-24f;
        float* dst = out + r * ld + 4 * blk;
        if (vec4)
            *(syn_f32x4*)dst = (syn_f32x4){v[0], v[1], v[2], v[3]};
        else
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (4 * blk + i < F) dst[i] = v[i];
    }
}

// ------------------------------------------------------------------------------------------------ streams of keys
// call q of segment g (row field q, block field block_first + g) gives draws 2 q and 2 q + 1: v = w[2p] << 32 | w[2p + 1]
__global__ __launch_bounds__(256) void syn_draw_kernel(int kind, long a, long b, int block_first, unsigned long long seed,
                                                       unsigned long long graph_index, long T, long long* __restrict__ keys) {
    const int seg = blockIdx.y;
    const unsigned tag = kind == ACM_SYNTH_PAIR ? SYN_TAG_PAIR : (kind == ACM_SYNTH_RECT ? SYN_TAG_RECT : SYN_TAG_RANGE);
    const AcmDropCtx cx = syn_ctx(seed, graph_index, tag);
    const unsigned long long R = kind == ACM_SYNTH_PAIR ? (unsigned long long)a * a : (unsigned long long)a * b;
    long long* dst = keys + (long)seg * T;
    for (long q = (long)blockIdx.x * 256 + threadIdx.x; 2 * q < T; q += (long)gridDim.x * 256) {
        unsigned w[4];
        acm_philox7(cx, q, block_first + seg, w);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const long t = 2 * q + p;
            if (t >= T) break;
            const unsigned long long v = ((unsigned long long)w[2 * p] << 32) | w[2 * p + 1];
            const unsigned long long slot = __umul64hi(v, R);       // < R
            long long key = (long long)slot;
            if (kind == ACM_SYNTH_PAIR) {
                const long long x = (long long)(slot / (unsigned long long)a), y = (long long)slot - x * a;
                key = x == y ? SYN_INVALID : (x < y ? x * a + y : y * a + x);
            }
            dst[t] = key;
        }
    }
}

// sorted position p (stable sort: equal keys keep their draw order) -> flag of the draw it came from
__global__ __launch_bounds__(256) void syn_mark_kernel(long T, long Tpad, const long long* __restrict__ sorted_keys,
                                                       const long long* __restrict__ perm, unsigned char* __restrict__ flags) {
    const int seg = blockIdx.y;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= T) return;
    const long long* sk = sorted_keys + (long)seg * T;
    const long long k = sk[p];
    const bool first = k != SYN_INVALID && (p == 0 || sk[p - 1] != k);
    const long long d = perm[(long)seg * T + p];
    if ((unsigned long long)d < (unsigned long long)T) flags[(long)seg * Tpad + d] = first ? 1 : 0;
}

__device__ __forceinline__ int syn_popc16(const uint4 f) { return __popc(f.x) + __popc(f.y) + __popc(f.z) + __popc(f.w); }

__global__ __launch_bounds__(256) void syn_count_kernel(long Tpad, long nblk, const unsigned char* __restrict__ flags,
                                                        long long* __restrict__ bsum) {
    __shared__ int red[4];
    const int seg = blockIdx.y;
    const uint4 f = *(const uint4*)(flags + (long)seg * Tpad + (long)blockIdx.x * SYN_CHUNK + threadIdx.x * 16);
    int c = syn_popc16(f);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) bsum[(long)seg * nblk + blockIdx.x] = (long long)red[0] + red[1] + red[2] + red[3];
}

// one block per segment: chunk sums -> exclusive prefixes (in place), found = min(distinct, M, cap), status bits
__global__ __launch_bounds__(256) void syn_scan_kernel(long nblk, long long* __restrict__ bsum, const long long* __restrict__ M,
                                                       long cap, long long* __restrict__ found, int* __restrict__ status) {
    __shared__ long long tsum[256];
    const int seg = blockIdx.x;
    long long* bs = bsum + (long)seg * nblk;
    const long per = (nblk + 255) / 256;
    const long b0 = (long)threadIdx.x * per, b1 = b0 + per < nblk ? b0 + per : nblk;
    long long s = 0;
    for (long i = b0; i < b1; ++i) s += bs[i];
    tsum[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int i = 0; i < 256; ++i) {
            const long long v = tsum[i];
            tsum[i] = run;
            run += v;
        }
        long long want = M[seg] > 0 ? M[seg] : 0;
        int bits = 0;
        if (run < want) bits |= ACM_SYNTH_SHORT;
        if (want > cap) bits |= ACM_SYNTH_OVER, want = cap;
        found[seg] = run < want ? run : want;
        if (bits) atomicOr(status, bits);
    }
    __syncthreads();
    long long run = tsum[threadIdx.x];
    for (long i = b0; i < b1; ++i) {
        const long long v = bs[i];
        bs[i] = run;
        run += v;
    }
}

__global__ __launch_bounds__(256) void syn_select_kernel(long T, long Tpad, long nblk, const unsigned char* __restrict__ flags,
                                                         const long long* __restrict__ bpre, const long long* __restrict__ keys,
                                                         const long long* __restrict__ M, long cap, long long* __restrict__ out) {
    __shared__ int wsum[4];
    const int seg = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const long t0 = (long)blockIdx.x * SYN_CHUNK + threadIdx.x * 16;
    const uint4 f = *(const uint4*)(flags + (long)seg * Tpad + t0);
    const int c = syn_popc16(f);
    int inc = c;                                                     // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    long long rank = bpre[(long)seg * nblk + blockIdx.x] + (inc - c);
    for (int u = 0; u < wv; ++u) rank += wsum[u];
    long long lim = M[seg] > 0 ? M[seg] : 0;
    if (lim > cap) lim = cap;
    if (c == 0 || rank >= lim) return;
    const unsigned words[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        if ((words[i >> 2] >> (8 * (i & 3))) & 0xFFu) {
            const long t = t0 + i;
            if (rank < lim && t < T) out[(long)seg * cap + rank] = keys[(long)seg * T + t];
            ++rank;
        }
    }
}

// selected key r of class cls -> the entries (row, col) and (col, row) as row * n + col; the rest of the region = INVALID
__global__ __launch_bounds__(256) void syn_emit_kernel(int kind, int C, long npc, int cls_first, const long long* __restrict__ sel,
                                                       const long long* __restrict__ found, long cap,
                                                       long long* __restrict__ edges, unsigned long long* __restrict__ B) {
    __shared__ int hist[SYN_MAX_C];
    const int seg = blockIdx.y, cls = cls_first + seg;
    const long n = (long)C * npc;
    if ((int)threadIdx.x < C) hist[threadIdx.x] = 0;
    __syncthreads();
    long long nf = found[seg];
    if (nf > cap) nf = cap;
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r < cap) {
        long long e0 = SYN_INVALID, e1 = SYN_INVALID;
        if (r < nf) {
            const long long key = sel[(long)seg * cap + r];
            long long row, col;
            if (kind == ACM_SYNTH_PAIR) {
                const long long x = key / npc, y = key - x * npc;
                row = cls * npc + x, col = cls * npc + y;
            } else {
                const long long W = (long long)(C - 1 - cls) * npc;
                const long long x = key / W, y = key - x * W;
                row = cls * npc + x, col = (cls + 1) * npc + y;
                const long long dest = cls + 1 + y / npc;
                if (dest >= 0 && dest < C) atomicAdd(&hist[dest], 1);
            }
            e0 = row * n + col, e1 = col * n + row;
        }
        long long* dst = edges + ((long)seg * cap + r) * 2;
        dst[0] = e0, dst[1] = e1;
    }
    __syncthreads();
    if (kind == ACM_SYNTH_PAIR) {
        if (blockIdx.x == 0 && threadIdx.x == 0) B[(long)cls * C + cls] = 2ull * (unsigned long long)nf;
    } else if ((int)threadIdx.x < C && hist[threadIdx.x] > 0) {           // integer adds: the same sums in any order
        atomicAdd(B + (long)cls * C + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
        atomicAdd(B + (long)threadIdx.x * C + cls, (unsigned long long)hist[threadIdx.x]);
    }
}

__global__ void syn_inter_count_kernel(int C, int cls, double t_edges, const long long* __restrict__ B, long long* __restrict__ m) {
    long long e = 0;
    for (int k = 0; k < cls; ++k) e += B[(long)k * C + cls];         // edges the earlier classes placed into this block
    const double want = rint(t_edges - (double)e) + 1.0;             // round-half-even, like Python's round
    *m = want > 0.0 ? (long long)want : 0;
}

inline size_t syn_align(size_t b) { return (b + 255) & ~(size_t)255; }
inline long syn_nblk(int64_t T) { return (long)((T + SYN_CHUNK - 1) / SYN_CHUNK); }
inline int syn_grid(int64_t work, int per_block, int cap) {
    int64_t nb = (work + per_block - 1) / per_block;
    if (nb > cap) nb = cap;
    return (int)(nb < 1 ? 1 : nb);
}
inline bool syn_shape_ok(int n_classes, int64_t npc) {
    return n_classes >= 2 && npc >= 1 && npc < INT32_MAX && (int64_t)n_classes * npc < INT32_MAX;
}

}  // namespace

// ================================================================================================ C ABI
extern "C" int acm_synth_regular(int n_classes, int64_t nodes_per_class, int64_t degree_intra, int64_t degree_inter, uint64_t seed,
                                 uint64_t graph_index, int64_t row_begin, int64_t row_end, int32_t* indices, acm_stream_t stream) {
    ACM_REQUIRE(indices, ACM_EINVAL, "acm_synth_regular: NULL pointer");
    ACM_REQUIRE(syn_shape_ok(n_classes, nodes_per_class), ACM_ESHAPE,
                "acm_synth_regular: bad sizes (n_classes >= 2, nodes_per_class >= 1, fewer than 2^31 nodes)");
    const int64_t npc = nodes_per_class, n = (int64_t)n_classes * npc;
    ACM_REQUIRE(degree_intra >= 0 && degree_intra <= npc - 1 && degree_inter >= 0 && degree_inter <= n - npc, ACM_ESHAPE,
                "acm_synth_regular: degrees %lld / %lld need 0 <= intra <= %lld and 0 <= inter <= %lld", (long long)degree_intra,
                (long long)degree_inter, (long long)(npc - 1), (long long)(n - npc));
    ACM_REQUIRE(row_begin >= 0 && row_begin <= row_end && row_end <= n, ACM_ESHAPE,
                "acm_synth_regular: rows [%lld, %lld) of %lld", (long long)row_begin, (long long)row_end, (long long)n);
    ACM_REQUIRE(n_classes <= SYN_MAX_C, ACM_EUNSUPPORTED, "acm_synth_regular: %d classes > %d", n_classes, SYN_MAX_C);
    ACM_REQUIRE(degree_intra + degree_inter <= SYN_MAX_D, ACM_EUNSUPPORTED, "acm_synth_regular: degree %lld > %d",
                (long long)(degree_intra + degree_inter), SYN_MAX_D);
    const int64_t rows = row_end - row_begin;
    if (rows == 0 || degree_intra + degree_inter == 0) return ACM_OK;
    hipLaunchKernelGGL(syn_regular_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, n_classes, (long)npc,
                       (int)degree_intra, (int)degree_inter, (unsigned long long)seed, (unsigned long long)graph_index,
                       (long)row_begin, (long)row_end, indices);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_synth_uniform(int64_t n_rows, int64_t n_features, uint64_t seed, uint64_t graph_index, int64_t row_begin,
                                 float* out, int64_t ld_out, acm_stream_t stream) {
    ACM_REQUIRE(out, ACM_EINVAL, "acm_synth_uniform: NULL pointer");
    ACM_REQUIRE(n_rows >= 0 && n_features >= 1 && row_begin >= 0 && row_begin + n_rows <= (int64_t)UINT32_MAX && ld_out >= n_features,
                ACM_ESHAPE, "acm_synth_uniform: bad sizes (n_features >= 1, ld_out >= n_features, rows below 2^32)");
    ACM_REQUIRE(n_features <= ACM_SYNTH_MAX_FEATURES, ACM_EUNSUPPORTED, "acm_synth_uniform: %lld features > %d",
                (long long)n_features, ACM_SYNTH_MAX_FEATURES);
    if (n_rows == 0) return ACM_OK;
    const int64_t F4 = (n_features + 3) / 4;
    const int vec4 = (n_features % 4 == 0) && (ld_out % 4 == 0) && (((uintptr_t)out & 15) == 0);
    hipLaunchKernelGGL(syn_uniform_kernel, dim3(syn_grid(n_rows * F4, 256, 8192)), dim3(256), 0, (hipStream_t)stream, (long)n_rows,
                       (long)n_features, (long)F4, (unsigned long long)seed, (unsigned long long)graph_index, (long)row_begin, out,
                       (long)ld_out, vec4);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_synth_random_plan(int n_classes, int64_t nodes_per_class, int64_t degree_intra, double edge_homo, int64_t* plan) {
    ACM_REQUIRE(plan, ACM_EINVAL, "acm_synth_random_plan: NULL pointer");
    ACM_REQUIRE(syn_shape_ok(n_classes, nodes_per_class) && nodes_per_class >= 2, ACM_ESHAPE,
                "acm_synth_random_plan: bad sizes (n_classes >= 2, nodes_per_class >= 2, fewer than 2^31 nodes)");
    ACM_REQUIRE(n_classes <= SYN_MAX_C, ACM_EUNSUPPORTED, "acm_synth_random_plan: %d classes > %d", n_classes, SYN_MAX_C);
    const int64_t npc = nodes_per_class;
    ACM_REQUIRE(degree_intra >= 0 && degree_intra <= npc - 1, ACM_ESHAPE, "acm_synth_random_plan: degree_intra %lld outside [0, %lld]",
                (long long)degree_intra, (long long)(npc - 1));
    const int64_t S = degree_intra * npc;                            // <= the npc (npc - 1) ordered pairs of a block
    ACM_REQUIRE(S % 2 == 0, ACM_ESHAPE, "acm_synth_random_plan: degree_intra * nodes_per_class = %lld must be even", (long long)S);
    ACM_REQUIRE(edge_homo > 0.0 && edge_homo <= 1.0, ACM_ESHAPE, "acm_synth_random_plan: edge_homo %g outside (0, 1]", edge_homo);
    const double T = (double)S * (1.0 - edge_homo) / edge_homo;
    const double slots = (double)npc * (double)npc * (double)(n_classes - 1);
    const double want = rint(T) + 1.0;
    ACM_REQUIRE(want <= slots, ACM_ESHAPE, "acm_synth_random_plan: %.0f inter-class edges for %.0f slots of class 0", want, slots);
    plan[0] = S / 2;
    plan[1] = (int64_t)want;                                         // no class asks for more: e_i >= 0
    return ACM_OK;
}

extern "C" int acm_synth_draw(int kind, int64_t a, int64_t b, int block_first, int n_segments, uint64_t seed, uint64_t graph_index,
                              int64_t n_draws, int64_t* keys, acm_stream_t stream) {
    ACM_REQUIRE(keys, ACM_EINVAL, "acm_synth_draw: NULL pointer");
    ACM_REQUIRE(kind == ACM_SYNTH_PAIR || kind == ACM_SYNTH_RECT || kind == ACM_SYNTH_RANGE, ACM_EINVAL, "acm_synth_draw: kind %d", kind);
    ACM_REQUIRE(a >= 1 && a < INT32_MAX && b >= 1 && b < INT32_MAX && n_draws >= 0 && n_draws < INT32_MAX && n_segments >= 1 &&
                    block_first >= 0,
                ACM_ESHAPE, "acm_synth_draw: bad sizes (1 <= a, b < 2^31, 0 <= n_draws < 2^31, n_segments >= 1)");
    ACM_REQUIRE((int64_t)block_first + n_segments <= 65535, ACM_EUNSUPPORTED, "acm_synth_draw: block field %lld > 65534",
                (long long)block_first + n_segments - 1);
    if (n_draws == 0) return ACM_OK;
    hipLaunchKernelGGL(syn_draw_kernel, dim3(syn_grid((n_draws + 1) / 2, 256, 4096), (unsigned)n_segments), dim3(256), 0,
                       (hipStream_t)stream, kind, (long)a, (long)b, block_first, (unsigned long long)seed,
                       (unsigned long long)graph_index, (long)n_draws, (long long*)keys);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_synth_select_workspace_bytes(int n_segments, int64_t n_draws, size_t* bytes) {
    ACM_REQUIRE(bytes, ACM_EINVAL, "acm_synth_select_workspace_bytes: NULL argument");
    ACM_REQUIRE(n_segments >= 1 && n_draws >= 0 && n_draws < INT32_MAX, ACM_ESHAPE,
                "acm_synth_select_workspace_bytes: bad sizes (n_segments >= 1, 0 <= n_draws < 2^31)");
    ACM_REQUIRE(n_segments <= 65535, ACM_EUNSUPPORTED, "acm_synth_select_workspace_bytes: %d segments > 65535", n_segments);
    const long nblk = syn_nblk(n_draws);
    *bytes = syn_align((size_t)n_segments * nblk * SYN_CHUNK) + syn_align((size_t)n_segments * nblk * sizeof(long long)) + 256;
    return ACM_OK;
}

extern "C" int acm_synth_select(int n_segments, int64_t n_draws, const int64_t* keys, const int64_t* sorted_keys, const int64_t* perm,
                                const int64_t* m, int64_t out_cap, int64_t* out, int64_t* found, int32_t* status, void* workspace,
                                size_t workspace_bytes, acm_stream_t stream) {
    ACM_REQUIRE(keys && sorted_keys && perm && m && out && found && status, ACM_EINVAL, "acm_synth_select: NULL pointer");
    ACM_REQUIRE(n_segments >= 1 && n_draws >= 0 && n_draws < INT32_MAX && out_cap >= 0, ACM_ESHAPE,
                "acm_synth_select: bad sizes (n_segments >= 1, 0 <= n_draws < 2^31, out_cap >= 0)");
    ACM_REQUIRE(n_segments <= 65535, ACM_EUNSUPPORTED, "acm_synth_select: %d segments > 65535", n_segments);
    size_t need = 0;
    acm_synth_select_workspace_bytes(n_segments, n_draws, &need);
    ACM_REQUIRE(workspace && workspace_bytes >= need, ACM_ENOMEM, "acm_synth_select: workspace %zu B < required %zu B", workspace_bytes,
                need);
    ACM_REQUIRE(((uintptr_t)workspace & 15) == 0, ACM_EINVAL, "acm_synth_select: workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const long T = (long)n_draws, nblk = syn_nblk(n_draws), Tpad = nblk * SYN_CHUNK;
    unsigned char* flags = (unsigned char*)workspace;
    long long* bsum = (long long*)((char*)workspace + syn_align((size_t)n_segments * Tpad));
    const dim3 per_chunk((unsigned)nblk, (unsigned)n_segments);
    if (T > 0) {
        ACM_CHECK_HIP(hipMemsetAsync(flags, 0, (size_t)n_segments * Tpad, st));
        hipLaunchKernelGGL(syn_mark_kernel, dim3((unsigned)((T + 255) / 256), (unsigned)n_segments), dim3(256), 0, st, T, Tpad,
                           (const long long*)sorted_keys, (const long long*)perm, flags);
        ACM_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(syn_count_kernel, per_chunk, dim3(256), 0, st, Tpad, nblk, flags, bsum);
        ACM_CHECK_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(syn_scan_kernel, dim3((unsigned)n_segments), dim3(256), 0, st, nblk, bsum, (const long long*)m, (long)out_cap,
                       (long long*)found, status);
    ACM_CHECK_HIP(hipGetLastError());
    if (T > 0 && out_cap > 0) {
        hipLaunchKernelGGL(syn_select_kernel, per_chunk, dim3(256), 0, st, T, Tpad, nblk, flags, bsum, (const long long*)keys,
                           (const long long*)m, (long)out_cap, (long long*)out);
        ACM_CHECK_HIP(hipGetLastError());
    }
    return ACM_OK;
}

extern "C" int acm_synth_inter_count(int n_classes, int cls, double t_edges, const int64_t* block_counts, int64_t* m_out,
                                     acm_stream_t stream) {
    ACM_REQUIRE(block_counts && m_out, ACM_EINVAL, "acm_synth_inter_count: NULL pointer");
    ACM_REQUIRE(n_classes >= 2 && cls >= 0 && cls < n_classes - 1 && t_edges >= 0.0 && t_edges < 9.0e18, ACM_ESHAPE,
                "acm_synth_inter_count: class %d of %d (every class but the last), t_edges >= 0", cls, n_classes);
    ACM_REQUIRE(n_classes <= SYN_MAX_C, ACM_EUNSUPPORTED, "acm_synth_inter_count: %d classes > %d", n_classes, SYN_MAX_C);
    hipLaunchKernelGGL(syn_inter_count_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, n_classes, cls, t_edges,
                       (const long long*)block_counts, (long long*)m_out);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_synth_emit(int kind, int n_classes, int64_t nodes_per_class, int class_first, int n_segments, const int64_t* selected,
                              const int64_t* found, int64_t cap, int64_t* edge_keys, int64_t* block_counts, acm_stream_t stream) {
    ACM_REQUIRE(selected && found && edge_keys && block_counts, ACM_EINVAL, "acm_synth_emit: NULL pointer");
    ACM_REQUIRE(kind == ACM_SYNTH_PAIR || kind == ACM_SYNTH_RECT, ACM_EINVAL, "acm_synth_emit: kind %d", kind);
    ACM_REQUIRE(syn_shape_ok(n_classes, nodes_per_class) && cap >= 0 && cap < INT32_MAX && class_first >= 0 && n_segments >= 1 &&
                    class_first + n_segments <= n_classes - (kind == ACM_SYNTH_RECT ? 1 : 0),
                ACM_ESHAPE, "acm_synth_emit: bad sizes (classes [%d, %d) of %d)", class_first, class_first + n_segments, n_classes);
    ACM_REQUIRE(n_classes <= SYN_MAX_C, ACM_EUNSUPPORTED, "acm_synth_emit: %d classes > %d", n_classes, SYN_MAX_C);
    if (cap == 0) return ACM_OK;
    hipLaunchKernelGGL(syn_emit_kernel, dim3((unsigned)((cap + 255) / 256), (unsigned)n_segments), dim3(256), 0, (hipStream_t)stream, kind,
                       n_classes, (long)nodes_per_class, class_first, (const long long*)selected, (const long long*)found, (long)cap,
                       (long long*)edge_keys, (unsigned long long*)block_counts);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}
