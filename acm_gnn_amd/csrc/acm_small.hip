// The whole training step of the two-layer ACM model on a SMALL graph in six launches (acm_small_step, ABI 25) -- SEVEN for
// ACM-GCN++ (acm_small_step_t::residual: launch 0 writes the residual Linear's weight transposed, launches 1, 2, 4 and 6 carry
// the branch under `bool RES`; its evaluation pass is four launches, not three).
//
// Reference: one step of ACM-Pytorch/models/models.py:100-166 (dropout -> GraphConvolution -> relu -> dropout ->
// GraphConvolution), utils.py:547-574 (log_softmax + nll_loss on the training rows, backward, optimizer.step) --
// layers.py:154-232 / ACM-Geometric/layers.py:78-116 per layer -- ~250 ATen launches there, 17-18 launches on this
// library's general path, whose kernels are sized for graphs 100x larger.  Cora (2 708 nodes), Chameleon (2 277),
// Squirrel (5 201): every table of the step fits one XCD's L2, a launch costs >= 5 us whatever it does, and these
// graphs are trained for thousands of epochs x 10 splits (ACM-Pytorch/train.py:95-139).  So: ONE launch per dependency
// level of the step (a level ends where the next one needs rows of OTHER nodes), everything row-local folded into the
// gather that produces its input, every update applied where its gradient becomes final.
//
// Layout conventions (wave = 64 lanes = four 16-lane groups g, lane m of a group).  The hidden width F is a template
// parameter of every launch but the third, given as V = F / 16, the columns a lane owns: V = 4 (F = 64) and V = 2 (F = 32)
// are instantiated; acm_small_step_t::hidden chooses.
//   * wide rows (F columns): lane (g, m) owns columns V m .. V m + V - 1 -- one 4 V-byte load per lane and row.  In a GATHER
//     group g takes every fourth neighbour (one wave instruction fetches four 4 F-byte rows); in ROW MATH group g owns
//     channel g (low, high, identity, structure): the per-channel LayerNorm / attention sums are 16-lane DPP sums, the 4
//     (or 3) channels run side by side, per-row scalars travel through v_readlane.
//   * narrow rows (<= 8 columns per channel): tables of 16-byte blocks [L 8 | H 8 | S 8]; lane (e, q) fetches block q of
//     the neighbour in slot e (eight neighbours per wave instruction); row math runs with lane c = column c.
//   * long rows: the handle's work items (acm_csr.cpp: build_items) cut them into pieces; a piece leaves its partial sums
//     in its slot (write-through stores), arrives at the row's counter, and the LAST piece to arrive adds the slots in slot
//     order and runs the row's epilogue -- no second launch, no float atomics, deterministic.  A slot is SLOT_PITCH floats
//     whatever the width: a wide piece uses 3 F of them, a narrow one 24.
#include <algorithm>
#include <vector>

#include "acm_common.h"
#include "acm_small_batch_host.h"
#include "acm_adam_device.h"

namespace {

typedef float f4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
// a lane's V consecutive columns of a wide row
template <int V> struct vec_of;
template <> struct vec_of<4> { typedef f4 type; };
template <> struct vec_of<2> { typedef f2 type; };
template <int V> using fv = typename vec_of<V>::type;

constexpr int F_MAX = 64;             // the widest hidden width: sizes the workspace for every width
constexpr int SLOT_PITCH = 3 * F_MAX; // floats of a long row's slot
constexpr int SLOT_PITCH_RES = 4 * F_MAX;  // ... of a residual plan's (launches 1 and 6 carry a fourth sum there: R, dW_X)
// The residual branch's two tensors (acm_small_step_t::res) ride behind the roles of layer 1 on the device: t[0][SR_RES_W],
// t[0][SR_RES_B] -- step factors, step counters and the reducing blocks' updates treat them like every other role.
constexpr int DEV_ROLES = ACM_SMALL_ROLES + 2;
constexpr int SR_RES_W = ACM_SMALL_ROLES, SR_RES_B = ACM_SMALL_ROLES + 1;
constexpr int TR = 32;                // launch 0's tile: TR x TR elements of W_X through LDS
constexpr int C8 = 8;                 // padded class count
constexpr int WAVES = 8;              // per workgroup of the gather phases (two per SIMD: the second hides the first's latency chain)
constexpr int MAX_WG = 512;           // workgroups of the phases that leave per-workgroup partial sums (launches 3, 4): beyond that a
                                      // wave loops over work items (Squirrel: 875 -> 512 workgroups, launch 4 56 -> 47 us)
constexpr int MAX_WG_WIDE = 2048;     // ... of the wide gather phases (launches 2, 5): one work item per wave up to 16384 items (a
                                      // wave's item is a chain of ~2 000 dependent instructions; more waves, not longer loops, hide it)
constexpr int RED_EL = 8;             // elements of the partial-sum vectors per reducing block of the last launch (x 32 producer lanes)
// dW2 [3][F][8] | dv1 [4][F] | dgamma1 | dbeta1 | dmix1 [4][4] | with the residual: db_X [F]
constexpr int part4_of(int f, bool res = false) { return 3 * f * C8 + 3 * 4 * f + 16 + (res ? f : 0); }
constexpr int PART3 = 3 * 4 * C8 + 16 + 1;              // dv2 [4][8] | dgamma2 | dbeta2 | dmix2 | loss
constexpr int PART3_PITCH = 128;
                                                        // (= a long row's record of launch 4: the row's terms in the layout of a partial)

struct SmallTensor {
    float* p;
    float* g;
    float* m;
    float* v;
    float* step;
};

struct ItemView {
    const AcmItem* items;
    int n_items;
    const AcmLongRow* long_rows;
    const int32_t* long_index;
    const int32_t* indices;
};

struct SmallDev {
    int n, f_in, C, k, relu_before, layernorm, train, update;
    float scale;
    SmallTensor t[2][DEV_ROLES];
    ItemView graph, x, xt;
    const float* x_vals;
    const int32_t* xt_src_pos;
    const float* row_scale;
    const int64_t* labels;
    const float* row_weight;
    float* loss;
    float* logits;
    float *att1, *att2;
    // workspace
    float *Z1, *H1, *ST1, *OUT1, *T2, *Z2I, *G2, *DZ2, *G1, *DZ1, *slots, *part3, *part4, *W2T, *FACT;
    int64_t* latch;                  // the dropout counter as launch 1 found it: what launches 2-6 draw their masks with
    float *long3, *long4;            // [n_long][PART3_PITCH] / [n_long][LONG4]: the parameter-gradient terms of the long rows
    int n_long;
    const float* xt_vals;
    int* counters;
    int nwg3, nwg4;                  // producer workgroups of the two partial-sum buffers
    acm_dropout_t drop_in, drop_hidden;
    AdamScalars hp;
    int64_t* also_advance;
    int* arrive;
    // the residual branch (ACM-GCN++; all unused without it)
    int residual;
    float *WXT, *R, *XX, *DR;        // W_X^T [f_in, F] | x_d W_X^T [n, F] | xX [n, F] | dR [n, F]
    acm_dropout_t drop_res;
};

// A sub-struct of the step's block as a value.  The block is either a kernel argument (generic reference) or an entry of the
// batch table seen through the constant address space (scalar loads for uniform fields); functions that take a sub-struct by
// generic reference get a copy made here, word by word -- small structs without indexing, so the copies dissolve into the
// loads of the fields that are used.
#define ACM_CONST_AS __attribute__((address_space(4)))
template <class T>
__device__ __forceinline__ T take(const T& v) { return v; }
template <class T>
__device__ __forceinline__ T take(const ACM_CONST_AS T& v) {
    static_assert(sizeof(T) % 4 == 0 && sizeof(T) <= 64, "take: a small struct of whole words");
    typedef uint32_t __attribute__((may_alias)) word_t;
    T out;
    const ACM_CONST_AS word_t* s = reinterpret_cast<const ACM_CONST_AS word_t*>(&v);
    word_t* o = reinterpret_cast<word_t*>(&out);
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; ++i) o[i] = s[i];
    return out;
}

// the V-wide forms (ldv<4> .. are the 16-byte ld4 .. of the narrow rows, whose blocks are four floats at every width)
template <int V> __device__ __forceinline__ fv<V> ldv(const float* p) { return *reinterpret_cast<const fv<V>*>(p); }
template <int V> __device__ __forceinline__ void stv(float* p, fv<V> v) { *reinterpret_cast<fv<V>*>(p) = v; }
template <int V> __device__ __forceinline__ fv<V> zerov() {
    if constexpr (V == 4) return f4{0.f, 0.f, 0.f, 0.f};
    else return f2{0.f, 0.f};
}
__device__ __forceinline__ f4 reluv(f4 v) { return f4{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f), fmaxf(v.z, 0.f), fmaxf(v.w, 0.f)}; }
__device__ __forceinline__ f2 reluv(f2 v) { return f2{fmaxf(v.x, 0.f), fmaxf(v.y, 0.f)}; }
__device__ __forceinline__ float hsumv(f4 v) { return (v.x + v.y) + (v.z + v.w); }
__device__ __forceinline__ float hsumv(f2 v) { return v.x + v.y; }
template <class T>
__device__ __forceinline__ T selv(int g, T a, T b, T c, T d) { return g == 0 ? a : (g == 1 ? b : (g == 2 ? c : d)); }
__device__ __forceinline__ f4 xsumv(f4 v) {      // over the four 16-lane groups
    return f4{acm_cross_row_sum(v.x), acm_cross_row_sum(v.y), acm_cross_row_sum(v.z), acm_cross_row_sum(v.w)};
}
__device__ __forceinline__ f2 xsumv(f2 v) { return f2{acm_cross_row_sum(v.x), acm_cross_row_sum(v.y)}; }
// v where the element of `gate` is positive, else 0 (a ReLU's or a dropout mask's backward)
__device__ __forceinline__ f4 wherev(f4 gate, f4 v) {
    return f4{gate.x > 0.f ? v.x : 0.f, gate.y > 0.f ? v.y : 0.f, gate.z > 0.f ? v.z : 0.f, gate.w > 0.f ? v.w : 0.f};
}
__device__ __forceinline__ f2 wherev(f2 gate, f2 v) { return f2{gate.x > 0.f ? v.x : 0.f, gate.y > 0.f ? v.y : 0.f}; }
__device__ __forceinline__ f4 ld4(const float* p) { return ldv<4>(p); }
__device__ __forceinline__ void st4(float* p, f4 v) { stv<4>(p, v); }
__device__ __forceinline__ f4 zero4() { return zerov<4>(); }
__device__ __forceinline__ f4 relu4(f4 v) { return reluv(v); }
__device__ __forceinline__ float bcast_f(float v, int u) { return __int_as_float(acm_row_bcast(__float_as_int(v), u)); }

// slot traffic crosses workgroups (and XCDs: each has its own L2): write-through stores, cache-bypassing loads
__device__ __forceinline__ void st_coherent(float* p, float v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ float ld_coherent(const float* p) {
    return __hip_atomic_load(const_cast<float*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_coherent(float* p, f4 v) {
    st_coherent(p, v.x), st_coherent(p + 1, v.y), st_coherent(p + 2, v.z), st_coherent(p + 3, v.w);
}
__device__ __forceinline__ void st_coherent(float* p, f2 v) { st_coherent(p, v.x), st_coherent(p + 1, v.y); }
template <int V> __device__ __forceinline__ fv<V> ldv_coherent(const float* p) {
    if constexpr (V == 4) return f4{ld_coherent(p), ld_coherent(p + 1), ld_coherent(p + 2), ld_coherent(p + 3)};
    else return f2{ld_coherent(p), ld_coherent(p + 1)};
}
__device__ __forceinline__ void st4_coherent(float* p, f4 v) { st_coherent(p, v); }
__device__ __forceinline__ f4 ld4_coherent(const float* p) { return ldv_coherent<4>(p); }

// ------------------------------------------------------------------------------------------------ wide gather
// acc[c] += sum over the entries [begin, end) of an id list of  w(pos) * T_c[id(pos), V m .. V m + V - 1];  group g of the wave
// takes the entries 4u + g.  The ids are loaded TRANSPOSED (lane (g, u) holds the id step u needs in group g), so a step
// is one row-broadcast DPP move per lane, no LDS crossbar.  Entries past `end` read row `safe` with weight 0.
// NA: the arrays' length (3; 4 where a residual plan gathers a fourth table), deduced.
template <int V, int NCH, int RELU_MASK, int NA, class W>
__device__ __forceinline__ void wide_gather(const int32_t* __restrict__ ids, int begin, int end, const float* const (&tab)[NA],
                                            const int (&ld)[NA], int safe, W&& weight, fv<V> (&acc)[NA]) {
    const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15;
    int id = safe;
    float w = 0.f;
    if (begin + 4 * m + g < end) id = ids[begin + 4 * m + g], w = weight(begin + 4 * m + g);
    for (int k0 = begin; k0 < end; k0 += 64) {
        // the NEXT chunk's ids travel while this chunk's rows do (one dependent round trip less per 64 entries)
        const int npos = k0 + 64 + 4 * m + g;
        int nid = safe;
        float nw = 0.f;
        if (npos < end) nid = ids[npos], nw = weight(npos);
        const int steps = (min(end - k0, 64) + 3) >> 2;              // uniform
        // CNT steps (x NCH rows) requested before the first is consumed: a step is a dependent L2 round trip, and with one
        // item per wave nothing else hides it
#define ACM_WG_BLOCK(U0, CNT)                                                                   \
        {                                                                                       \
            fv<V> v[CNT][NCH];                                                                  \
            float ww[CNT];                                                                      \
            _Pragma("unroll") for (int s = 0; s < CNT; ++s) {                                   \
                const int j = acm_row_bcast(id, U0 + s);                                        \
                ww[s] = bcast_f(w, U0 + s);                                                     \
                _Pragma("unroll") for (int c = 0; c < NCH; ++c)                                 \
                    v[s][c] = ldv<V>(tab[c] + (long)j * ld[c] + V * m);                         \
            }                                                                                   \
            _Pragma("unroll") for (int s = 0; s < CNT; ++s)                                     \
                _Pragma("unroll") for (int c = 0; c < NCH; ++c) {                               \
                    fv<V> x = v[s][c];                                                          \
                    if ((RELU_MASK >> c) & 1) x = reluv(x);                                     \
                    acc[c] += ww[s] * x;                                                        \
                }                                                                               \
        }
        if constexpr (NCH == 4) {
            // four tables: four steps (sixteen rows) in flight -- eight would hold 128 registers of rows at F = 64
            ACM_WG_BLOCK(0, 4)
            if (steps > 4) ACM_WG_BLOCK(4, 4)
            if (steps > 8) ACM_WG_BLOCK(8, 4)
            if (steps > 12) ACM_WG_BLOCK(12, 4)
        } else if (steps <= 4) {
            ACM_WG_BLOCK(0, 4)
        } else if (steps <= 8) {
            ACM_WG_BLOCK(0, 8)
        } else {
            ACM_WG_BLOCK(0, 8)
            if (steps <= 12) {
                ACM_WG_BLOCK(8, 4)
            } else {
                ACM_WG_BLOCK(8, 8)
            }
        }
#undef ACM_WG_BLOCK
        id = nid, w = nw;
    }
}

// The item loop of a wide phase: every wave takes the items wave, wave + n_waves, ...; `gather(item, acc)` fills the lane's
// partial sums, `epi(row, acc)` runs once per ROW with the complete sums (in every group).
// `pre(row)`: the loads of the row's epilogue that depend on nothing but the row number, requested BEFORE the gather (they
// travel while the item -> ids -> rows chain runs; with one item per wave that chain is the kernel's duration).
template <int V, int NCH, class Pre, class Gather, class Epi>
__device__ __forceinline__ void wide_items(const ItemView& iv, float* slots, int* counters, int wave, int n_waves, Pre&& pre,
                                           Gather&& gather, Epi&& epi) {
    const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15;
    for (int it = wave; it < iv.n_items; it += n_waves) {
        AcmItem item = iv.items[it];
        item.row = acm_uniform(item.row), item.begin = acm_uniform(item.begin), item.end = acm_uniform(item.end), item.slot = acm_uniform(item.slot);
        auto pf = pre(item.row);
        constexpr int F = 16 * V;
        constexpr int NA = NCH > 3 ? NCH : 3;                        // four sums (and slots of four) in a residual plan's launches 1 and 6
        constexpr int PITCH = NCH > 3 ? SLOT_PITCH_RES : SLOT_PITCH;
        fv<V> acc[NA];
#pragma unroll
        for (int c = 0; c < NA; ++c) acc[c] = zerov<V>();
        gather(item, acc);
#pragma unroll
        for (int c = 0; c < NCH; ++c) acc[c] = xsumv(acc[c]);
        if (item.slot >= 0) {                                        // a piece of a long row (uniform branch)
            float* sp = slots + (long)item.slot * PITCH;
            if (g < NCH) st_coherent(sp + g * F + V * m, selv(g, acc[0], acc[1], acc[2], acc[NA - 1]));
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const int li = iv.long_index[item.row];
            const AcmLongRow lr = iv.long_rows[li];
            int old = 0;
            if (lane == 0) old = __hip_atomic_fetch_add(counters + li, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            old = __builtin_amdgcn_readfirstlane(old);
            if (old != lr.slot_end - lr.slot_begin - 1) continue;    // another piece will finish the row
            if (lane == 0) __hip_atomic_store(counters + li, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
            for (int c = 0; c < NA; ++c) acc[c] = zerov<V>();
            for (int q = lr.slot_begin; q < lr.slot_end; ++q) {
                const float* qp = slots + (long)q * PITCH + V * m;
#pragma unroll
                for (int c = 0; c < NCH; ++c) acc[c] += ldv_coherent<V>(qp + c * F);
            }
        }
        epi(item.row, acc, pf);
    }
}

// ------------------------------------------------------------------------------------------------ narrow gather
// Rows of NQ 16-byte blocks (NQ = 4: [L 8 | H 8], 6: + [S 8]); lane = 8 e + q fetches block q of the neighbour in slot e.
// Returns in EVERY lane (e, q) block q of the row sum.  `relu01`: ReLU on the gathered L / H blocks (ACMII).
template <int NQ>
__device__ __forceinline__ f4 narrow_gather(const int32_t* __restrict__ ids, int begin, int end, const float* __restrict__ tab,
                                            int ld, int safe, bool relu01) {
    const int lane = threadIdx.x & 63, q = lane & 7, base = lane & ~7;
    const int qq = q < NQ ? q : NQ - 1;                  // idle lanes repeat the last block (unconditional loads: a guarded load
    const bool relu = relu01 && q < 4;                   // makes the compiler wait for every one before the next)
    f4 acc = zero4();
    int id = safe;
    float w = 0.f;
    if (begin + 8 * q + (lane >> 3) < end) id = ids[begin + 8 * q + (lane >> 3)], w = 1.f;
    for (int k0 = begin; k0 < end; k0 += 64) {
        const int npos = k0 + 64 + 8 * q + (lane >> 3);       // the next chunk's ids, requested before this chunk's rows
        int nid = safe;
        float nw = 0.f;
        if (npos < end) nid = ids[npos], nw = 1.f;
        const int steps = (min(end - k0, 64) + 7) >> 3;
        f4 v[8];
        float ww[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (u < steps || u < 2) {                    // (uniform; two steps always: most rows of a small graph end there)
                const int j = __shfl(id, base + u);
                ww[u] = __shfl(w, base + u);
                v[u] = ld4(tab + (long)j * ld + 4 * qq);
            } else {
                v[u] = zero4(), ww[u] = 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            f4 x = v[u];
            if (relu) x = relu4(x);
            acc += ww[u] * x;
        }
        id = nid, w = nw;
    }
    if (q >= NQ) acc = zero4();
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) {
        acc.x += __shfl_xor(acc.x, off);
        acc.y += __shfl_xor(acc.y, off);
        acc.z += __shfl_xor(acc.z, off);
        acc.w += __shfl_xor(acc.w, off);
    }
    return acc;
}

// The epilogue also receives the row's long-row index (-1: a whole row).  WHICH wave finishes a long row depends on the
// arrival order, so a finisher must not add the row's parameter-gradient terms to its own running sums (the sums of the
// workgroups would differ from run to run in the last bit): it leaves them in the row's own record (SmallDev::long3 / long4).
template <int NQ, class Pre, class Gather, class Epi>
__device__ __forceinline__ void narrow_items(const ItemView& iv, float* slots, int* counters, int wave, int n_waves, Pre&& pre,
                                             Gather&& gather, Epi&& epi) {
    const int lane = threadIdx.x & 63, q = lane & 7;
    for (int it = wave; it < iv.n_items; it += n_waves) {
        AcmItem item = iv.items[it];
        item.row = acm_uniform(item.row), item.begin = acm_uniform(item.begin), item.end = acm_uniform(item.end), item.slot = acm_uniform(item.slot);
        auto pf = pre(item.row);
        f4 acc = gather(item);
        int li = -1;
        if (item.slot >= 0) {
            float* sp = slots + (long)item.slot * SLOT_PITCH;
            if (lane < 8 && q < NQ) st4_coherent(sp + 4 * q, acc);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            li = iv.long_index[item.row];
            const AcmLongRow lr = iv.long_rows[li];
            int old = 0;
            if (lane == 0) old = __hip_atomic_fetch_add(counters + li, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            old = __builtin_amdgcn_readfirstlane(old);
            if (old != lr.slot_end - lr.slot_begin - 1) continue;
            if (lane == 0) __hip_atomic_store(counters + li, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            acc = zero4();
            if (q < NQ)
                for (int s = lr.slot_begin; s < lr.slot_end; ++s) acc += ld4_coherent(slots + (long)s * SLOT_PITCH + 4 * q);
        }
        epi(item.row, acc, pf, li);
    }
}

// column c = lane & 7 of channel block `blk` (0: L, 1: H, 2: S) out of the per-lane 16-byte blocks of a narrow row
__device__ __forceinline__ float narrow_pick(f4 acc, int blk) {
    const int lane = threadIdx.x & 63, c = lane & 7, src = 2 * blk + (c >> 2);
    const float x0 = __shfl(acc.x, src), x1 = __shfl(acc.y, src), x2 = __shfl(acc.z, src), x3 = __shfl(acc.w, src);
    const int el = c & 3;
    return el == 0 ? x0 : (el == 1 ? x1 : (el == 2 ? x2 : x3));
}
__device__ __forceinline__ float gsum8(float v) { return acm_group_sum<8>(v); }
__device__ __forceinline__ float gmax8(float v) {
    v = fmaxf(v, __shfl_xor(v, 1));
    v = fmaxf(v, __shfl_xor(v, 2));
    return fmaxf(v, __shfl_xor(v, 4));
}

// ------------------------------------------------------------------------------------------------ Adam in an epilogue
// The update of a lane's V consecutive elements of tensor T at I, whose gradient G has just become final; PF holds the
// elements and their moments as loaded before the gather (pp / mm / vv), FC the tensor's two step factors (V is the
// enclosing template's).  Two branches with the vector's components NAMED, as the 64-wide code had them: with the components
// subscripted in one V-sized loop (`PF.pp[r]`, `po[r] = pp[r]`) -- in this macro or in an inlined function, both were tried
// -- the 64-wide small_finish and small_conv1_bwd<FOUR, .> take 170 registers instead of 168 and run two waves per SIMD
// instead of three.  A further width is a further branch.
#define ACM_SMALL_ADAM_LANE(T, I, PF, G, AF, FC)                                                                                     \
    if constexpr (V == 4) {                                                                                                          \
        float pp[4] = {PF.pp.x, PF.pp.y, PF.pp.z, PF.pp.w}, mm[4] = {PF.mm.x, PF.mm.y, PF.mm.z, PF.mm.w};                            \
        float vv[4] = {PF.vv.x, PF.vv.y, PF.vv.z, PF.vv.w};                                                                          \
        const float gg[4] = {G.x, G.y, G.z, G.w};                                                                                    \
        _Pragma("unroll") for (int r = 0; r < 4; ++r)                                                                                \
            adam_one(pp[r], gg[r], mm[r], vv[r], AF.decay_eff, AF.wd, AF.decoupled, AF.w1, AF.b2, AF.w2, FC[0], FC[1], AF.eps);      \
        st4(T.p + I, f4{pp[0], pp[1], pp[2], pp[3]}), st4(T.m + I, f4{mm[0], mm[1], mm[2], mm[3]});                                  \
        st4(T.v + I, f4{vv[0], vv[1], vv[2], vv[3]});                                                                                \
    } else {                                                                                                                         \
        float pp[2] = {PF.pp.x, PF.pp.y}, mm[2] = {PF.mm.x, PF.mm.y}, vv[2] = {PF.vv.x, PF.vv.y};                                    \
        const float gg[2] = {G.x, G.y};                                                                                              \
        _Pragma("unroll") for (int r = 0; r < 2; ++r)                                                                                \
            adam_one(pp[r], gg[r], mm[r], vv[r], AF.decay_eff, AF.wd, AF.decoupled, AF.w1, AF.b2, AF.w2, FC[0], FC[1], AF.eps);      \
        stv<2>(T.p + I, f2{pp[0], pp[1]}), stv<2>(T.m + I, f2{mm[0], mm[1]}), stv<2>(T.v + I, f2{vv[0], vv[1]});                     \
    }

// What the later launches of the step read as tables, written by the first workgroup of launch 1 (both change every step):
//   W2T  [idx = ch * 8 + c][col < F]: layer 2's weights, classes padded to 8 -- a lane's V columns of one output are one
//        load, for the forward projection (launch 2) and for dH = dZ2 W2^T (launch 4) alike
//   FACT [layer * DEV_ROLES + role][2]: the step-dependent Adam factors of every tensor (double-precision pow: once, not per block)
template <int V, class D>
__device__ __forceinline__ void write_tables(const D& d) {
    constexpr int F = 16 * V;
    if (blockIdx.x != 0) return;
    for (int e = threadIdx.x; e < 3 * F * C8; e += blockDim.x) {
        const int idx = e / F, col = e % F, ch = idx >> 3, c = idx & 7;
        d.W2T[e] = c < d.C ? d.t[1][ACM_SR_W_LOW + ch].p[col * d.C + c] : 0.f;
    }
    if ((int)threadIdx.x < 2 * DEV_ROLES && d.update) {
        const SmallTensor t = take(d.t[threadIdx.x / DEV_ROLES][threadIdx.x % DEV_ROLES]);
        if (t.p && t.step) acm_adam_step_factors(take(d.hp), t.step[0], d.FACT[2 * threadIdx.x], d.FACT[2 * threadIdx.x + 1]);
    }
    // the dropout counter of THIS step: the later launches draw their masks with this copy, so the last launch may advance
    // the live counter whenever it likes (no arrival barrier over its ~900 blocks: their atomics on one address were 10 us)
    if (threadIdx.x == 0) d.latch[0] = d.drop_hidden.step ? d.drop_hidden.step[0] : (d.drop_in.step ? d.drop_in.step[0] : 0);
}

// ------------------------------------------------------------------------------------------------ launch 1: Z1 = drop(X) Wcat
// ------------------------------------------------------------------------------------------------ launch 0 (residual plans): W_X^T
// mlpX.lins[0] is an nn.Linear: its weight is [F, f_in], the transpose of the [f_in, F] tables launch 1 gathers by feature id.
// WXT[j, c] = W_X[c, j], a TR x TR tile per workgroup through LDS (rows of W_X read along j, rows of WXT written along c).
// Rebuilt on every call: the optimizer, a keep-best restore and load_state_dict all rewrite the parameter through its pointer.
__global__ __launch_bounds__(256) void small_wxt_kernel(const float* __restrict__ w, float* __restrict__ wxt, int f_in, int F) {
    __shared__ float tile[TR][TR + 1];
    const int tx = threadIdx.x & (TR - 1), ty = threadIdx.x / TR;          // 32 x 8 threads
    const int j0 = (int)blockIdx.x * TR, c0 = (int)blockIdx.y * TR;
    for (int r = ty; r < TR; r += 256 / TR)
        tile[r][tx] = (c0 + r < F && j0 + tx < f_in) ? w[(long)(c0 + r) * f_in + j0 + tx] : 0.f;
    __syncthreads();
    for (int r = ty; r < TR; r += 256 / TR)
        if (j0 + r < f_in && c0 + tx < F) wxt[(long)(j0 + r) * F + c0 + tx] = tile[tx][r];
}

// RES: a fourth sum R = drop(X) W_X^T beside the three channels (the same dropped values, items and long-row machinery);
// group 3, idle in the store without it, stores R to its own [n, F] buffer -- Z1 keeps its 3 F pitch.
template <int V, bool RES, class D>
__device__ __forceinline__ void small_proj1_body(const D& d, int n_wg) {
    constexpr int F = 16 * V;
    write_tables<V>(d);
    const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15;
    const int wave = (int)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = n_wg * 4;
    const AcmDropCtx dc = acm_drop_ctx(take(d.drop_in));
    const float* __restrict__ xv = d.x_vals;
    if constexpr (RES) {
        const float* tab[4] = {d.t[0][ACM_SR_W_LOW].p, d.t[0][ACM_SR_W_HIGH].p, d.t[0][ACM_SR_W_MLP].p, d.WXT};
        const int ld[4] = {F, F, F, F};
        wide_items<V, 4>(
            take(d.x), d.slots, d.counters, wave, n_waves, [](int) { return 0; },
            [&](const AcmItem& item, fv<V>(&acc)[4]) {
                wide_gather<V, 4, 0>(d.x.indices, item.begin, item.end, tab, ld, 0,
                                     [&](int pos) { return xv[pos] * acm_drop1(dc, pos, 0); }, acc);
            },
            [&](int row, fv<V>(&acc)[4], int) {
                if (g < 3) stv<V>(d.Z1 + (long)row * (3 * F) + g * F + V * m, selv(g, acc[0], acc[1], acc[2], acc[2]));
                else stv<V>(d.R + (long)row * F + V * m, acc[3]);
                if (d.k == 4 && g == 3 && m < C8) d.T2[(long)row * 24 + 16 + m] = m < d.C ? d.t[1][ACM_SR_STRUC].p[(long)row * d.C + m] : 0.f;
            });
        return;
    }
    const float* tab[3] = {d.t[0][ACM_SR_W_LOW].p, d.t[0][ACM_SR_W_HIGH].p, d.t[0][ACM_SR_W_MLP].p};
    const int ld[3] = {F, F, F};
    wide_items<V, 3>(
        take(d.x), d.slots, d.counters, wave, n_waves, [](int) { return 0; },
        [&](const AcmItem& item, fv<V>(&acc)[3]) {
            wide_gather<V, 3, 0>(d.x.indices, item.begin, item.end, tab, ld, 0,
                                 [&](int pos) { return xv[pos] * acm_drop1(dc, pos, 0); }, acc);
        },
        [&](int row, fv<V>(&acc)[3], int) {
            if (g < 3) stv<V>(d.Z1 + (long)row * (3 * F) + g * F + V * m, selv(g, acc[0], acc[1], acc[2], acc[2]));
            // the structure parameter of layer 2 as a block of the narrow table (refreshed every step: it is a parameter)
            if (d.k == 4 && g == 3 && m < C8) d.T2[(long)row * 24 + 16 + m] = m < d.C ? d.t[1][ACM_SR_STRUC].p[(long)row * d.C + m] : 0.f;
        });
}

// ------------------------------------------------------------------------------------------------ launch 2: layer 1 forward
// per-row math of a WIDE layer (F columns), group g = channel g.  `acc` = complete gathered sums (in every group).
template <int V, bool RES>
struct Pre2 {
    float rs;
    fv<V> own;
};
template <int V>
struct Pre2<V, true> {
    float rs;
    fv<V> own, r;                                        // r: the row of R = drop(X) W_X^T (launch 1)
};
// RES: xX = drop_res(relu(R[row] + b_X)), element (row, column) with tag 2, is stored and joins `out` in layer 2's projection
// (models.py:160-163: the layer after sees drop(relu(fea1)) + xX); OUT1 keeps the pure `out`.
template <int V, bool FOUR, bool VARIANT, bool RES, class D>
__device__ __forceinline__ void small_conv1_fwd_body(const D& d, const float* z1, int n_wg) {
    constexpr int F = 16 * V;
    typedef fv<V> vt;
    const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15;
    const int wave = (int)blockIdx.x * WAVES + (threadIdx.x >> 6), n_waves = n_wg * WAVES;
    constexpr int NCH = FOUR ? 3 : 2;
    constexpr int K = FOUR ? 4 : 3;
    const AcmDropCtx dh = acm_drop_ctx(take(d.drop_hidden));
    AcmDropCtx dr = dh;
    vt bx = zerov<V>();
    if constexpr (RES) dr = acm_drop_ctx(take(d.drop_res)), bx = ldv<V>(d.t[0][SR_RES_B].p + V * m);
    const float* tab[3] = {z1, z1 + F, FOUR ? d.t[0][ACM_SR_STRUC].p : z1};
    const int ld[3] = {3 * F, 3 * F, F};
    const bool act = g < K;
    // this lane's channel parameters (columns V m .. V m + V - 1) and its share of layer 2's weights: output idx = g + 4t
    const vt av = act ? ldv<V>(d.t[0][ACM_SR_V_LOW + g].p + V * m) : zerov<V>();
    vt gam = zerov<V>(), bet = zerov<V>();
    if (d.layernorm && act) gam = ldv<V>(d.t[0][ACM_SR_LNW_LOW + g].p + V * m), bet = ldv<V>(d.t[0][ACM_SR_LNB_LOW + g].p + V * m);
    float mix[K][K];
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = 0; b < K; ++b) mix[a][b] = d.t[0][ACM_SR_MIX].p[a * K + b];
    vt w2t[6];
#pragma unroll
    for (int t = 0; t < 6; ++t) w2t[t] = ldv<V>(d.W2T + (g + 4 * t) * F + V * m);
    // the row's own terms: group 1 its Z_H row, group 2 its Z_I row, group 3 its struc_low row
    const float* own_base = g == 1 ? z1 + F : (g == 2 ? z1 + 2 * F : (FOUR ? d.t[0][ACM_SR_STRUC].p : z1));
    const int own_ld = (g == 1 || g == 2) ? 3 * F : F;
    wide_items<V, NCH>(
        take(d.graph), d.slots, d.counters, wave, n_waves,
        [&](int row) {
            Pre2<V, RES> pf;
            pf.rs = d.row_scale[row];
            pf.own = (g == 0 || (!FOUR && g == 3)) ? zerov<V>() : ldv<V>(own_base + (long)row * own_ld + V * m);
            if constexpr (RES) pf.r = ldv<V>(d.R + (long)row * F + V * m);
            return pf;
        },
        [&](const AcmItem& item, vt(&acc)[3]) {
            wide_gather<V, NCH, VARIANT ? 3 : 0>(d.graph.indices, item.begin, item.end, tab, ld, item.row, [](int) { return 1.f; }, acc);
        },
        [&](int row, vt(&acc)[3], const Pre2<V, RES>& pf) {
            const float rs = pf.rs;
            const vt own = pf.own;
            vt h;
            if (VARIANT) h = selv(g, rs * acc[0], reluv(own) - rs * acc[1], reluv(own), reluv(acc[2] - own));
            else h = selv(g, reluv(rs * acc[0]), reluv(own - rs * acc[1]), reluv(own), reluv(acc[2] - own));
            if (!act) h = zerov<V>();
            float mean = 0.f, rstd = 1.f;
            vt hn = h;
            if (d.layernorm) {
                mean = acm_group_sum<16>(hsumv(h)) * (1.0f / F);
                const vt dd = h - mean;
                const float var = acm_group_sum<16>(hsumv(dd * dd)) * (1.0f / F);
                rstd = 1.0f / sqrtf(var + ACM_LN_EPS);
                hn = dd * rstd * gam + bet;
            }
            const float logit = acm_group_sum<16>(hsumv(hn * av));
            const float sg = 1.0f / (1.0f + expf(-logit));
            float sig[K], tt[K], al[K];
#pragma unroll
            for (int c = 0; c < K; ++c) sig[c] = acm_lane_f(sg, 16 * c);
            float mx = -INFINITY;
#pragma unroll
            for (int b = 0; b < K; ++b) {
                float s = 0.f;
#pragma unroll
                for (int a = 0; a < K; ++a) s += sig[a] * mix[a][b];
                tt[b] = s / (float)K;
                mx = fmaxf(mx, tt[b]);
            }
            float den = 0.f;
#pragma unroll
            for (int b = 0; b < K; ++b) al[b] = expf(tt[b] - mx), den += al[b];
#pragma unroll
            for (int b = 0; b < K; ++b) al[b] /= den;
            const float my_al = g == 0 ? al[0] : (g == 1 ? al[1] : (g == 2 ? al[2] : (K == 4 ? al[K - 1] : 0.f)));
            vt out = d.scale * xsumv(my_al * h);
            // the caller's dropout(relu(.)) between the layers (models.py:70): element (row, column) of an [n, F] activation
            out = reluv(out);
            if (dh.on) {
#pragma unroll
                for (int r = 0; r < V; ++r) out[r] *= acm_drop1(dh, row, V * m + r);
            }
            if (g == 0) stv<V>(d.OUT1 + (long)row * F + V * m, out);
            vt in2 = out;                                  // what layer 2 projects
            if constexpr (RES) {
                vt xx = reluv(pf.r + bx);
                if (dr.on) {
#pragma unroll
                    for (int r = 0; r < V; ++r) xx[r] *= acm_drop1(dr, row, V * m + r);
                }
                if (g == 1) stv<V>(d.XX + (long)row * F + V * m, xx);
                in2 = out + xx;
            }
            if (act) stv<V>(d.H1 + (long)row * (4 * F) + g * F + V * m, h);
            if (m == 0 && act) {
                float* st = d.ST1 + (long)row * 16;
                st[g] = mean, st[4 + g] = rstd, st[8 + g] = sg, st[12 + g] = my_al;
                d.att1[(long)row * 4 + g] = my_al;
            }
            // layer 2's projection of this row: output idx = ch * 8 + c, group g takes idx = g, g + 4, ...
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const int idx = g + 4 * t, ch = idx >> 3, c = idx & 7;
                const float s = acm_group_sum<16>(hsumv(in2 * w2t[t]));
                if (m == 0 && c < d.C) {
                    if (ch < 2) d.T2[(long)row * 24 + ch * 8 + c] = s;
                    else d.Z2I[(long)row * C8 + c] = s;
                }
            }
        });
}

// ------------------------------------------------------------------------------------------------ launch 3: layer 2 forward + loss + K3
struct Pre3 {
    float rs, zH, zI, sS, w;
    int y;
};
template <bool FOUR, class D>
__device__ __forceinline__ void small_conv2_fwd_body(const D& d, int n_wg) {
    __shared__ float red[WAVES][PART3_PITCH];
    const int lane = threadIdx.x & 63, c = lane & 7, wv = threadIdx.x >> 6;
    const int wave = (int)blockIdx.x * WAVES + wv, n_waves = n_wg * WAVES;
    constexpr int NQ = FOUR ? 6 : 4;
    constexpr int K = FOUR ? 4 : 3;
    const int C = d.C;
    const bool valid = c < C;
    const float invC = 1.0f / (float)C;
    const bool variant = d.relu_before != 0;
    float av[K], gam[K], bet[K];
#pragma unroll
    for (int ch = 0; ch < K; ++ch) {
        av[ch] = valid ? d.t[1][ACM_SR_V_LOW + ch].p[c] : 0.f;
        gam[ch] = (valid && d.layernorm) ? d.t[1][ACM_SR_LNW_LOW + ch].p[c] : 0.f;
        bet[ch] = (valid && d.layernorm) ? d.t[1][ACM_SR_LNB_LOW + ch].p[c] : 0.f;
    }
    float mix[K][K];
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = 0; b < K; ++b) mix[a][b] = d.t[1][ACM_SR_MIX].p[a * K + b];
    float a_dv[K], a_dg[K], a_db[K], a_dm[K][K], a_loss = 0.f;
#pragma unroll
    for (int ch = 0; ch < K; ++ch) {
        a_dv[ch] = a_dg[ch] = a_db[ch] = 0.f;
#pragma unroll
        for (int b = 0; b < K; ++b) a_dm[ch][b] = 0.f;
    }
    narrow_items<NQ>(
        take(d.graph), d.slots, d.counters, wave, n_waves,
        [&](int row) {
            Pre3 pf;
            pf.rs = d.row_scale[row];
            pf.zH = d.T2[(long)row * 24 + 8 + c], pf.zI = d.Z2I[(long)row * C8 + c];
            pf.sS = FOUR ? d.T2[(long)row * 24 + 16 + c] : 0.f;
            pf.w = d.train ? d.row_weight[row] : 0.f;
            pf.y = d.train ? (int)d.labels[row] : 0;
            return pf;
        },
        [&](const AcmItem& item) { return narrow_gather<NQ>(d.graph.indices, item.begin, item.end, d.T2, 24, item.row, variant); },
        [&](int row, f4 acc, const Pre3& pf, int li) {
            const float rs = pf.rs;
            const float aL = narrow_pick(acc, 0), aH = narrow_pick(acc, 1), aS = FOUR ? narrow_pick(acc, 2) : 0.f;
            const float zH = pf.zH, zI = pf.zI;
            float h[K];
            if (variant) h[0] = rs * aL, h[1] = fmaxf(zH, 0.f) - rs * aH;
            else h[0] = fmaxf(rs * aL, 0.f), h[1] = fmaxf(zH - rs * aH, 0.f);
            h[2] = fmaxf(zI, 0.f);
            if (FOUR) h[K - 1] = fmaxf(aS - pf.sS, 0.f);
            float xh[K], hn[K], rstd[K], sig[K], tt[K], al[K];
#pragma unroll
            for (int ch = 0; ch < K; ++ch) {
                if (!valid) h[ch] = 0.f;
                xh[ch] = 0.f, rstd[ch] = 1.f, hn[ch] = h[ch];
                if (d.layernorm) {
                    const float mean = gsum8(h[ch]) * invC;
                    const float dd = valid ? h[ch] - mean : 0.f;
                    const float var = gsum8(dd * dd) * invC;
                    rstd[ch] = 1.0f / sqrtf(var + ACM_LN_EPS);
                    xh[ch] = dd * rstd[ch];
                    hn[ch] = valid ? xh[ch] * gam[ch] + bet[ch] : 0.f;
                }
                const float logit = gsum8(hn[ch] * av[ch]);
                sig[ch] = 1.0f / (1.0f + expf(-logit));
            }
            float mx = -INFINITY;
#pragma unroll
            for (int b = 0; b < K; ++b) {
                float s = 0.f;
#pragma unroll
                for (int a = 0; a < K; ++a) s += sig[a] * mix[a][b];
                tt[b] = s / (float)K;
                mx = fmaxf(mx, tt[b]);
            }
            float den = 0.f;
#pragma unroll
            for (int b = 0; b < K; ++b) al[b] = expf(tt[b] - mx), den += al[b];
            float z = 0.f;
#pragma unroll
            for (int b = 0; b < K; ++b) al[b] /= den, z += al[b] * h[b];
            z *= d.scale;
            if (lane < 8 && valid) d.logits[(long)row * C + c] = z;
            if (lane < K) d.att2[(long)row * 4 + lane] = lane == 0 ? al[0] : (lane == 1 ? al[1] : (lane == 2 ? al[2] : al[K - 1]));
            if (!d.train) return;
            // masked NLL of the row and its gradient (acm_nll_row)
            const float w = pf.w;
            float dl = 0.f, r_loss = 0.f;
            float r_dv[K], r_dg[K], r_db[K], r_dm[K][K];        // this row's terms of the parameter gradients
            if (w != 0.f) {
                const float mz = gmax8(valid ? z : -INFINITY);
                const float ex = valid ? expf(z - mz) : 0.f;
                const float s = gsum8(ex);
                const int y = pf.y;
                const float zy = __shfl(z, (lane & ~7) + y);
                r_loss = w * ((mz + logf(s)) - zy);
                dl = valid ? w * (ex * (1.0f / s) - (c == y ? 1.f : 0.f)) : 0.f;
            }
            // row-local backward of the layer (no post-op on an output layer)
            float dal[K], dot = 0.f;
#pragma unroll
            for (int ch = 0; ch < K; ++ch) dal[ch] = d.scale * gsum8(dl * h[ch]), dot += al[ch] * dal[ch];
            float dt[K];
#pragma unroll
            for (int ch = 0; ch < K; ++ch) dt[ch] = al[ch] * (dal[ch] - dot);
            float gch[K];
#pragma unroll
            for (int ch = 0; ch < K; ++ch) {
                float dsig = 0.f;
#pragma unroll
                for (int b = 0; b < K; ++b) {
                    dsig += dt[b] * mix[ch][b];
                    r_dm[ch][b] = sig[ch] * dt[b] / (float)K;
                }
                dsig /= (float)K;
                const float dlg = dsig * sig[ch] * (1.0f - sig[ch]);
                r_dv[ch] = dlg * hn[ch];
                r_dg[ch] = r_db[ch] = 0.f;
                const float dhn = dlg * av[ch];
                float dln = dhn;
                if (d.layernorm) {
                    r_dg[ch] = dhn * xh[ch];
                    r_db[ch] = valid ? dhn : 0.f;
                    const float u = dhn * gam[ch];
                    const float s1 = gsum8(u) * invC, s2 = gsum8(u * xh[ch]) * invC;
                    dln = valid ? rstd[ch] * (u - s1 - xh[ch] * s2) : 0.f;
                }
                const float dh = d.scale * al[ch] * dl + dln;
                const bool relu_here = !(variant && ch < 2);
                gch[ch] = (relu_here && !(h[ch] > 0.f)) ? 0.f : dh;
            }
            if (lane < 8) {
                float* gp = d.G2 + (long)row * 24;
                gp[c] = rs * gch[0], gp[8 + c] = rs * gch[1];
                if (FOUR) gp[16 + c] = gch[K - 1];
                float* dz = d.DZ2 + (long)row * 24;
                dz[8 + c] = gch[1], dz[16 + c] = gch[2];
            }
            if (li < 0) {
                a_loss += r_loss;
#pragma unroll
                for (int ch = 0; ch < K; ++ch) {
                    a_dv[ch] += r_dv[ch], a_dg[ch] += r_dg[ch], a_db[ch] += r_db[ch];
#pragma unroll
                    for (int b = 0; b < K; ++b) a_dm[ch][b] += r_dm[ch][b];
                }
            } else {                                      // the finisher of a long row: its terms go to the row's own record
                float* rec = d.long3 + (long)li * PART3_PITCH;
                if (lane < 8) {
#pragma unroll
                    for (int ch = 0; ch < 4; ++ch) {
                        const bool on = ch < K;
                        rec[ch * 8 + c] = on ? r_dv[on ? ch : 0] : 0.f, rec[32 + ch * 8 + c] = on ? r_dg[on ? ch : 0] : 0.f;
                        rec[64 + ch * 8 + c] = on ? r_db[on ? ch : 0] : 0.f;
                    }
                }
                if (lane == 0) {
#pragma unroll
                    for (int a = 0; a < 4; ++a)
#pragma unroll
                        for (int b = 0; b < 4; ++b) rec[96 + a * 4 + b] = (a < K && b < K) ? r_dm[a < K ? a : 0][b < K ? b : 0] : 0.f;
                    rec[112] = r_loss;
                }
            }
        });
    if (!d.train) return;
    // per-workgroup partial sums: waves in order through LDS (deterministic)
    if (lane < 8) {
#pragma unroll
        for (int ch = 0; ch < K; ++ch) red[wv][ch * 8 + c] = a_dv[ch], red[wv][32 + ch * 8 + c] = a_dg[ch], red[wv][64 + ch * 8 + c] = a_db[ch];
        if (!FOUR) red[wv][24 + c] = red[wv][56 + c] = red[wv][88 + c] = 0.f;
    }
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) red[wv][96 + a * 4 + b] = (a < K && b < K) ? a_dm[a < K ? a : 0][b < K ? b : 0] : 0.f;
        red[wv][112] = a_loss;
    }
    __syncthreads();
    if (threadIdx.x < PART3) {
        float s = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) s += red[w][threadIdx.x];
        d.part3[(long)blockIdx.x * PART3_PITCH + threadIdx.x] = s;
    }
}

// ------------------------------------------------------------------------------------------------ launch 4: layer 2 backward gather + dH + layer 1 K3
template <int V>
struct Pre4 {
    float rs, gH, dzI, zL, zH, gS, sp, sm, sv;
    fv<V> o, h;
    float mean, rstd, sa[8];
};
// RES: the layer's real input is o + xX (dW2 takes it); dmix stays on the pure o; dR = the gradient through the residual's
// dropout and ReLU goes to its own [n, F] buffer (launch 6's fourth table) and db_X = sum over rows of dR joins the partial
// sums (the last F elements of a partial / a long row's record).
template <int V, bool FOUR, bool RES, class D>
__device__ __forceinline__ void small_conv2_bwd_body(const D& d, const float* z1, int n_wg) {
    constexpr int F = 16 * V, PART4 = part4_of(F, RES), LONG4 = PART4, DBX = part4_of(F);   // DBX: where db_X starts
    typedef fv<V> vt;
    __shared__ __attribute__((aligned(16))) float red[WAVES / 2][PART4];  // the waves' sums side by side (two rounds: 37 KB at F = 64)
    __shared__ __attribute__((aligned(16))) float w2s[3 * F * C8];        // W2T [idx][col]: 24 rows of F, read by every row's dH
    // RES: db_X's running sum per wave, in LDS (the 64-wide kernel has no four registers left for it: 256 without the residual)
    __shared__ __attribute__((aligned(16))) float dbx[RES ? WAVES : 1][F];
    for (int e = 4 * threadIdx.x; e < 3 * F * C8; e += 4 * 64 * WAVES) st4(w2s + e, ld4(d.W2T + e));
    if constexpr (RES) {
        if (threadIdx.x < WAVES * F / 4) st4(&dbx[0][0] + 4 * threadIdx.x, zero4());
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15, c = lane & 7, wv = threadIdx.x >> 6;
    const int wave = (int)blockIdx.x * WAVES + wv, n_waves = n_wg * WAVES;
    constexpr int NQ = FOUR ? 6 : 4;
    constexpr int K = FOUR ? 4 : 3;
    const int C = d.C;
    const bool variant = d.relu_before != 0;
    const AcmDropCtx dh = acm_drop_ctx(take(d.drop_hidden));
    const float inv_keep = dh.on ? dh.inv_keep : 1.f;
    float inv_keep_res = 1.f;
    if constexpr (RES) inv_keep_res = d.drop_res.p > 0.f ? 1.0f / (1.0f - d.drop_res.p) : 1.f;    // (acm_drop_ctx's own expression)
    const bool act = g < K;
    const vt av = act ? ldv<V>(d.t[0][ACM_SR_V_LOW + g].p + V * m) : zerov<V>();
    vt gam = zerov<V>();
    if (d.layernorm && act) gam = ldv<V>(d.t[0][ACM_SR_LNW_LOW + g].p + V * m);
    vt bet = zerov<V>();
    if (d.layernorm && act) bet = ldv<V>(d.t[0][ACM_SR_LNB_LOW + g].p + V * m);
    float mix[K][K];
#pragma unroll
    for (int a = 0; a < K; ++a)
#pragma unroll
        for (int b = 0; b < K; ++b) mix[a][b] = d.t[0][ACM_SR_MIX].p[a * K + b];
    const AdamFactors af(take(d.hp));
    const SmallTensor ts2 = take(d.t[1][ACM_SR_STRUC]);
    const bool s2_lane = FOUR && lane < 8 && c < C;
    vt a_w2[6];
#pragma unroll
    for (int t = 0; t < 6; ++t) a_w2[t] = zerov<V>();
    vt a_dv = zerov<V>(), a_dg = zerov<V>(), a_db = zerov<V>();
    float a_dm = 0.f;                                 // d(mix): lane L < 16 holds element (L >> 2, L & 3)
    narrow_items<NQ>(
        take(d.graph), d.slots, d.counters, wave, n_waves,
        [&](int row) {                                   // everything the row's epilogue reads that is not a gathered sum
            Pre4<V> pf;
            pf.rs = d.row_scale[row];
            const float* dzp = d.DZ2 + (long)row * 24;
            pf.gH = dzp[8 + c], pf.dzI = dzp[16 + c];
            pf.zL = variant ? d.T2[(long)row * 24 + c] : 1.f, pf.zH = variant ? d.T2[(long)row * 24 + 8 + c] : 1.f;
            pf.gS = FOUR ? d.G2[(long)row * 24 + 16 + c] : 0.f;
            pf.sp = pf.sm = pf.sv = 0.f;
            if (s2_lane && d.update) {
                const long i = (long)row * C + c;
                pf.sp = ts2.p[i], pf.sm = ts2.m[i], pf.sv = ts2.v[i];
            }
            pf.o = ldv<V>(d.OUT1 + (long)row * F + V * m);
            pf.h = act ? ldv<V>(d.H1 + (long)row * (4 * F) + g * F + V * m) : zerov<V>();
            const float* st = d.ST1 + (long)row * 16;
            pf.mean = st[g], pf.rstd = st[4 + g];
#pragma unroll
            for (int q = 0; q < 8; ++q) pf.sa[q] = st[8 + q];         // sigmoid and alpha of the four channels (wave-uniform)
            return pf;
        },
        [&](const AcmItem& item) { return narrow_gather<NQ>(d.graph.indices, item.begin, item.end, d.G2, 24, item.row, false); },
        [&](int row, f4 acc, const Pre4<V>& pf, int li) {
            const float aL = narrow_pick(acc, 0), aH = narrow_pick(acc, 1), aS = FOUR ? narrow_pick(acc, 2) : 0.f;
            float dzL = aL, dzH = pf.gH - aH;
            const float dzI = pf.dzI;
            if (variant) {
                if (!(pf.zL > 0.f)) dzL = 0.f;
                if (!(pf.zH > 0.f)) dzH = 0.f;
            }
            if (s2_lane) {                                // dS2 = P G_S - G_S: final here, the parameter row is updated in place
                const float ds = aS - pf.gS;
                const long i = (long)row * C + c;
                if (ts2.g) ts2.g[i] = ds;
                if (d.update) {
                    float pp = pf.sp, mm = pf.sm, vv = pf.sv;
                    const float* fc = d.FACT + 2 * (DEV_ROLES + ACM_SR_STRUC);
                    adam_one(pp, ds, mm, vv, af.decay_eff, af.wd, af.decoupled, af.w1, af.b2, af.w2, fc[0], fc[1], af.eps);
                    ts2.p[i] = pp, ts2.m[i] = mm, ts2.v[i] = vv;
                }
            }
            // dZ2 of this row as wave-uniform values, idx = ch * 8 + c
            float dz[24];
#pragma unroll
            for (int cc = 0; cc < 8; ++cc) {
                dz[cc] = acm_lane_f(dzL, cc);
                dz[8 + cc] = acm_lane_f(dzH, cc);
                dz[16 + cc] = acm_lane_f(dzI, cc);
            }
            const vt o = pf.o;
            // the layer's input: with the residual o + xX (xX requested here, not before the gather: it travels while dH is
            // formed from LDS, and the 64-wide kernel has no registers to hold it through the gather)
            vt xx = zerov<V>();
            if constexpr (RES) xx = ldv<V>(d.XX + (long)row * F + V * m);
            // dH = dZ2 Wcat2^T (columns V m .. V m + V - 1) and dWcat2 += H^T dZ2 (group g: idx = g, g + 4, ...)
            // (W2T from LDS, staged once per workgroup: as global loads its 24 rows were three dependent round trips per row)
            vt dH0 = zerov<V>(), dH1 = zerov<V>();
#pragma unroll
            for (int q = 0; q < 24; q += 2) dH0 += dz[q] * ldv<V>(w2s + q * F + V * m), dH1 += dz[q + 1] * ldv<V>(w2s + (q + 1) * F + V * m);
            const vt dH = dH0 + dH1;
            vt in2 = o, dmix_r = o;
            if constexpr (RES) {
                // Everything that reads o, xX or dH on its own first, then their sum in o's place: the 64-wide kernel is at
                // its 256 registers without the residual.
                dmix_r = wherev(o, dH * inv_keep);
                // through the residual's dropout(relu(.)), as dmix through the layer's
                const vt r_dbx = wherev(xx, dH * inv_keep_res);
                if (g == 1) stv<V>(d.DR + (long)row * F + V * m, r_dbx);
                if (li < 0) {
                    if (g == 0) stv<V>(dbx[wv] + V * m, ldv<V>(dbx[wv] + V * m) + r_dbx);      // (a wave's own slice: no barrier)
                } else if (g == 0) stv<V>(d.long4 + (long)li * LONG4 + DBX + V * m, r_dbx);
                in2 = o + xx;
            }
            if (li < 0) {
#pragma unroll
                for (int t = 0; t < 6; ++t) {
                    const float zz = g == 0 ? dz[4 * t] : (g == 1 ? dz[4 * t + 1] : (g == 2 ? dz[4 * t + 2] : dz[4 * t + 3]));
                    a_w2[t] += zz * in2;
                }
            } else {                                      // a long row: its dW2 term goes to the row's own record
                float* rec = d.long4 + (long)li * LONG4;
#pragma unroll
                for (int t = 0; t < 6; ++t) {
                    const int idx = g + 4 * t, ch = idx >> 3, cc = idx & 7;
                    const float zz = g == 0 ? dz[4 * t] : (g == 1 ? dz[4 * t + 1] : (g == 2 ? dz[4 * t + 2] : dz[4 * t + 3]));
                    float* rp = rec + ch * (F * C8) + (V * m) * C8 + cc;
#pragma unroll
                    for (int r = 0; r < V; ++r) rp[r * C8] = zz * in2[r];
                }
            }
            // through dropout(relu(.)): the forward's output is non-zero exactly where both let the element pass
            vt dmix;
            if constexpr (RES) dmix = dmix_r;
            else dmix = wherev(o, dH * inv_keep);
            // row-local backward of layer 1, channel g in group g
            const float rs = pf.rs;
            const vt h = pf.h;
            float sig[K], al[K];
#pragma unroll
            for (int ch = 0; ch < K; ++ch) sig[ch] = pf.sa[ch], al[ch] = pf.sa[4 + ch];
            const float mean = pf.mean, rstd = pf.rstd;
            const float dal_mine = d.scale * acm_group_sum<16>(hsumv(dmix * h));
            float dal[K], dot = 0.f;
#pragma unroll
            for (int ch = 0; ch < K; ++ch) dal[ch] = acm_lane_f(dal_mine, 16 * ch), dot += al[ch] * dal[ch];
            float dt[K], dlg[K];
#pragma unroll
            for (int ch = 0; ch < K; ++ch) dt[ch] = al[ch] * (dal[ch] - dot);
#pragma unroll
            for (int ch = 0; ch < K; ++ch) {
                float dsig = 0.f;
#pragma unroll
                for (int b = 0; b < K; ++b) dsig += dt[b] * mix[ch][b];
                dsig /= (float)K;
                dlg[ch] = dsig * sig[ch] * (1.0f - sig[ch]);
            }
            float r_dm = 0.f;
            {
                const int ma = (lane >> 2) & 3, mb = lane & 3;
                const float sa = ma == 0 ? sig[0] : (ma == 1 ? sig[1] : (ma == 2 ? sig[2] : sig[K - 1]));
                const float tb = mb == 0 ? dt[0] : (mb == 1 ? dt[1] : (mb == 2 ? dt[2] : dt[K - 1]));
                if (ma < K && mb < K) r_dm = sa * tb / (float)K;
            }
            const float my_dl = g == 0 ? dlg[0] : (g == 1 ? dlg[1] : (g == 2 ? dlg[2] : (K == 4 ? dlg[K - 1] : 0.f)));
            const float my_al = g == 0 ? al[0] : (g == 1 ? al[1] : (g == 2 ? al[2] : (K == 4 ? al[K - 1] : 0.f)));
            vt xh = zerov<V>(), hn = h;
            if (d.layernorm) xh = (h - mean) * rstd, hn = xh * gam + bet;
            const vt r_dv = my_dl * hn;
            const vt dhn = my_dl * av;
            vt dln = dhn, r_dg = zerov<V>(), r_db = zerov<V>();
            if (d.layernorm) {
                r_dg = dhn * xh;
                r_db = dhn;
                const vt u = dhn * gam;
                const float s1 = acm_group_sum<16>(hsumv(u)) * (1.0f / F), s2 = acm_group_sum<16>(hsumv(u * xh)) * (1.0f / F);
                dln = rstd * (u - s1 - xh * s2);
            }
            vt dhc = (d.scale * my_al) * dmix + dln;
            const bool relu_here = !(variant && g < 2);
            if (relu_here) dhc = wherev(h, dhc);
            float* g1 = d.G1 + (long)row * (3 * F) + V * m;
            float* dz1 = d.DZ1 + (long)row * (3 * F) + V * m;
            if (g == 0) stv<V>(g1, rs * dhc);
            if (g == 1) stv<V>(g1 + F, rs * dhc), stv<V>(dz1 + F, dhc);
            if (g == 2) stv<V>(dz1 + 2 * F, dhc);
            if (FOUR && g == 3) stv<V>(g1 + 2 * F, dhc);
            if (li < 0) {
                a_dv += r_dv, a_dg += r_dg, a_db += r_db, a_dm += r_dm;
            } else {                                      // the finisher of a long row: its terms go to the row's own record
                float* rec = d.long4 + (long)li * LONG4 + 3 * F * C8;
                const vt zv = zerov<V>();
                stv<V>(rec + g * F + V * m, act ? r_dv : zv), stv<V>(rec + 4 * F + g * F + V * m, act ? r_dg : zv);
                stv<V>(rec + 8 * F + g * F + V * m, act ? r_db : zv);
                if (lane < 16) rec[12 * F + lane] = r_dm;
            }
        });
    // per-workgroup partial sums: waves 0-3 leave their sums in a slice each, waves 4-7 add theirs on top, then every thread
    // adds the four slices of its elements -- a fixed order of additions (deterministic), two barriers
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        if ((wv >> 2) == round) {
            float* mine = red[wv & 3];
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const int idx = g + 4 * t, ch = idx >> 3, cc = idx & 7;
                float* rp = mine + ch * (F * C8) + (V * m) * C8 + cc;
#pragma unroll
                for (int r = 0; r < V; ++r) {
                    if (round == 0) rp[r * C8] = a_w2[t][r];
                    else rp[r * C8] += a_w2[t][r];
                }
            }
            float* r1 = mine + 3 * F * C8 + g * F + V * m;
            const vt zv = zerov<V>();
            const vt v0 = act ? a_dv : zv, v1 = act ? a_dg : zv, v2 = act ? a_db : zv;
            if (round == 0) stv<V>(r1, v0), stv<V>(r1 + 4 * F, v1), stv<V>(r1 + 8 * F, v2);
            else stv<V>(r1, ldv<V>(r1) + v0), stv<V>(r1 + 4 * F, ldv<V>(r1 + 4 * F) + v1), stv<V>(r1 + 8 * F, ldv<V>(r1 + 8 * F) + v2);
            if (lane < 16) {
                float* rm = mine + 3 * F * C8 + 12 * F + lane;
                if (round == 0) rm[0] = a_dm;
                else rm[0] += a_dm;
            }
            if constexpr (RES) {
                if (g == 0) {
                    float* rx = mine + DBX + V * m;
                    const vt a_dbx = ldv<V>(dbx[wv] + V * m);
                    if (round == 0) stv<V>(rx, a_dbx);
                    else stv<V>(rx, ldv<V>(rx) + a_dbx);
                }
            }
        }
        __syncthreads();
    }
    for (int e = threadIdx.x; e < PART4; e += 64 * WAVES)
        d.part4[(long)blockIdx.x * PART4 + e] = (red[0][e] + red[1][e]) + (red[2][e] + red[3][e]);
}

// ------------------------------------------------------------------------------------------------ launch 5: layer 1 backward gather
template <int V>
struct Pre5 {
    fv<V> a, b, pp, mm, vv;
};
template <int V, bool FOUR, bool VARIANT, class D>
__device__ __forceinline__ void small_conv1_bwd_body(const D& d, const float* z1, int n_wg) {
    constexpr int F = 16 * V;
    typedef fv<V> vt;
    const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15;
    const int wave = (int)blockIdx.x * WAVES + (threadIdx.x >> 6), n_waves = n_wg * WAVES;
    constexpr int NCH = FOUR ? 3 : 2;
    const float* tab[3] = {d.G1, d.G1 + F, d.G1 + 2 * F};
    const int ld[3] = {3 * F, 3 * F, 3 * F};
    const AdamFactors af(take(d.hp));
    const SmallTensor ts = take(d.t[0][ACM_SR_STRUC]);
    wide_items<V, NCH>(
        take(d.graph), d.slots, d.counters, wave, n_waves,
        [&](int row) {
            // group 0: the ReLU mask of Z_L (ACMII); group 1: its direct term dZ_H and the mask of Z_H; group 3: G_S of the row
            // and the parameter row with its moments
            Pre5<V> pf;
            pf.a = pf.b = pf.pp = pf.mm = pf.vv = zerov<V>();
            const float* zr = z1 + (long)row * (3 * F) + V * m;
            if (g == 0 && VARIANT) pf.b = ldv<V>(zr);
            if (g == 1) {
                pf.a = ldv<V>(d.DZ1 + (long)row * (3 * F) + F + V * m);
                if (VARIANT) pf.b = ldv<V>(zr + F);
            }
            if (FOUR && g == 3) {
                pf.a = ldv<V>(d.G1 + (long)row * (3 * F) + 2 * F + V * m);
                if (d.update) {
                    const long i = (long)row * F + V * m;
                    pf.pp = ldv<V>(ts.p + i), pf.mm = ldv<V>(ts.m + i), pf.vv = ldv<V>(ts.v + i);
                }
            }
            return pf;
        },
        [&](const AcmItem& item, vt(&acc)[3]) {
            wide_gather<V, NCH, 0>(d.graph.indices, item.begin, item.end, tab, ld, item.row, [](int) { return 1.f; }, acc);
        },
        [&](int row, vt(&acc)[3], const Pre5<V>& pf) {
            float* dz1 = d.DZ1 + (long)row * (3 * F) + V * m;
            if (g == 0 || g == 1) {
                vt dz = g == 0 ? acc[0] : pf.a - acc[1];
                if (VARIANT) dz = wherev(pf.b, dz);
                stv<V>(dz1 + g * F, dz);
            } else if (FOUR && g == 3) {                   // dS = P G_S - G_S: final, the parameter row is updated in place
                const vt ds = acc[2] - pf.a;
                const long i = (long)row * F + V * m;
                if (ts.g) stv<V>(ts.g + i, ds);
                if (d.update) {
                    const float* fc = d.FACT + 2 * ACM_SR_STRUC;
                    ACM_SMALL_ADAM_LANE(ts, i, pf, ds, af, fc)
                }
            }
        });
}

// ------------------------------------------------------------------------------------------------ launch 6: dW1, every other sum, the updates
// blocks [0, item_blocks): dW1 = drop(X)^T dZ1 by feature row (the transposed feature handle's items) + its update;
// blocks behind: RED_EL elements of the two partial-sum vectors per block (sum over the producer workgroups and the long
// rows' records, then the update).  The first block advances the step counters.
// RES: the feature-row blocks take dR as a fourth table, dW_X[:, j] = sum_i x_d[i, j] dR[i, :], and update W_X in the Linear's
// own layout (element (c, j) at c f_in + j: strided scalar accesses, group 3's); the reducing blocks apply b_X from the
// partial sums' last F elements.
template <int V, bool RES, class D>
__device__ __forceinline__ void small_finish_body(const D& d, int item_blocks, int red_blocks) {
    constexpr int F = 16 * V, PART4 = part4_of(F, RES), LONG4 = PART4;
    typedef fv<V> vt;
    __shared__ float red8[256 / RED_EL][RED_EL];
    const float* __restrict__ fact = d.FACT;              // step factors of every tensor (launch 1 wrote them)
    const AdamFactors af(take(d.hp));
    auto apply = [&](int layer, int role, long i, float gsum) {
        const SmallTensor t = take(d.t[layer][role]);
        if (!t.p) return;
        if (t.g) t.g[i] = gsum;
        if (!d.update) return;
        const float* s = fact + 2 * (layer * DEV_ROLES + role);
        float pp = t.p[i], mm = t.m[i], vv = t.v[i];
        adam_one(pp, gsum, mm, vv, af.decay_eff, af.wd, af.decoupled, af.w1, af.b2, af.w2, s[0], s[1], af.eps);
        t.p[i] = pp, t.m[i] = mm, t.v[i] = vv;
    };
    const int blk = (int)blockIdx.x;
    if (blk < item_blocks) {
        const int lane = threadIdx.x & 63, g = lane >> 4, m = lane & 15;
        const int wave = blk * 4 + (threadIdx.x >> 6), n_waves = item_blocks * 4;
        const AcmDropCtx dc = acm_drop_ctx(take(d.drop_in));
        constexpr int NT = RES ? 4 : 3;
        const float* tab[NT] = {d.DZ1, d.DZ1 + F, d.DZ1 + 2 * F};
        int ld[NT] = {3 * F, 3 * F, 3 * F};
        if constexpr (RES) tab[3] = d.DR, ld[3] = F;
        const int(&ldc)[NT] = ld;
        const float* __restrict__ xv = d.x_vals;
        const float* __restrict__ xtv = d.xt_vals;
        const int32_t* __restrict__ sp = d.xt_src_pos;
        const long f_in = d.f_in;
        wide_items<V, NT>(
            take(d.xt), d.slots, d.counters, wave, n_waves,
            [&](int frow) {                                // the weight rows this wave will update, with their moments
                Pre5<V> pf;
                pf.a = pf.b = pf.pp = pf.mm = pf.vv = zerov<V>();
                if (g < 3 && d.update) {
                    const SmallTensor t = take(d.t[0][ACM_SR_W_LOW + g]);
                    const long i = (long)frow * F + V * m;
                    pf.pp = ldv<V>(t.p + i), pf.mm = ldv<V>(t.m + i), pf.vv = ldv<V>(t.v + i);
                }
                if constexpr (RES) {
                    if (g == 3 && d.update) {              // column frow of W_X: V elements f_in apart
                        const SmallTensor t = take(d.t[0][SR_RES_W]);
#pragma unroll
                        for (int r = 0; r < V; ++r) {
                            const long i = (long)(V * m + r) * f_in + frow;
                            pf.pp[r] = t.p[i], pf.mm[r] = t.m[i], pf.vv[r] = t.v[i];
                        }
                    }
                }
                return pf;
            },
            [&](const AcmItem& item, vt(&acc)[NT]) {
                if (xtv)
                    wide_gather<V, NT, 0>(d.xt.indices, item.begin, item.end, tab, ldc, 0,
                                          [&](int pos) { return xtv[pos] * acm_drop1(dc, sp[pos], 0); }, acc);
                else
                    wide_gather<V, NT, 0>(d.xt.indices, item.begin, item.end, tab, ldc, 0,
                                          [&](int pos) { const int s = sp[pos]; return xv[s] * acm_drop1(dc, s, 0); }, acc);
            },
            [&](int frow, vt(&acc)[NT], const Pre5<V>& pf) {
                if constexpr (RES) {
                    if (g == 3) {
                        const SmallTensor t = take(d.t[0][SR_RES_W]);
                        const float* fc = fact + 2 * SR_RES_W;
#pragma unroll
                        for (int r = 0; r < V; ++r) {
                            const long i = (long)(V * m + r) * f_in + frow;
                            const float gw = acc[NT - 1][r];
                            if (t.g) t.g[i] = gw;
                            if (d.update) {
                                float pp = pf.pp[r], mm = pf.mm[r], vv = pf.vv[r];
                                adam_one(pp, gw, mm, vv, af.decay_eff, af.wd, af.decoupled, af.w1, af.b2, af.w2, fc[0], fc[1], af.eps);
                                t.p[i] = pp, t.m[i] = mm, t.v[i] = vv;
                            }
                        }
                    }
                }
                if (g < 3) {
                    const vt gw = selv(g, acc[0], acc[1], acc[2], acc[2]);
                    const SmallTensor t = take(d.t[0][ACM_SR_W_LOW + g]);
                    const long i = (long)frow * F + V * m;
                    if (t.g) stv<V>(t.g + i, gw);
                    if (d.update) {
                        const float* fc = fact + 2 * (ACM_SR_W_LOW + g);
                        ACM_SMALL_ADAM_LANE(t, i, pf, gw, af, fc)
                    }
                }
            });
    } else if (blk < item_blocks + red_blocks) {
        // RED_EL elements per block: thread (wl, el) adds the producer workgroups wl, wl + 32, ... (independent loads in
        // flight), the 32 partial sums meet in LDS in a fixed order
        const int el = (int)threadIdx.x & (RED_EL - 1), wl = (int)threadIdx.x / RED_EL;
        const int e = (blk - item_blocks) * RED_EL + el;
        const int K = d.k, C = d.C;
        const bool four = e < PART4;
        const int q = e - PART4;
        float s = 0.f;
        if (e < PART4 + PART3) {
            const float* src = four ? d.part4 + e : d.part3 + q;
            const long pitch = four ? PART4 : PART3_PITCH;
            const int nw = four ? d.nwg4 : d.nwg3;
            // sixteen loads in flight per thread, added in the order of the producer workgroups
            // the long rows' own records follow the workgroups' partials as further producers (their finisher varies from
            // run to run, their place in this sum does not)
            const float* lsrc = four ? d.long4 + e : d.long3 + q;
            const long lpitch = four ? LONG4 : PART3_PITCH;
            const int total = nw + d.n_long;
            constexpr int WL = 256 / RED_EL;
            for (int w0 = wl; w0 < total; w0 += 16 * WL) {
                float v[16];
#pragma unroll
                for (int j = 0; j < 16; ++j) {             // unconditional loads (a guarded load is waited for before the next)
                    const int w = min(w0 + WL * j, total - 1);
                    const float* pw = w < nw ? src + (long)w * pitch : lsrc + (long)(w - nw) * lpitch;
                    v[j] = *pw;
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) s += (w0 + WL * j < total) ? v[j] : 0.f;
            }
        }
        red8[wl][el] = s;
        __syncthreads();
        if (wl == 0 && e < PART4 + PART3) {
            s = 0.f;
#pragma unroll
            for (int j = 0; j < 256 / RED_EL; ++j) s += red8[j][el];
            if (four) {
                if (e < 3 * F * C8) {
                    const int ch = e / (F * C8), col = (e / C8) % F, c = e % C8;
                    if (c < C) apply(1, ACM_SR_W_LOW + ch, (long)col * C + c, s);
                } else if (e < 3 * F * C8 + 12 * F) {
                    const int r = e - 3 * F * C8, kind = r / (4 * F), ch = (r / F) % 4, col = r % F;
                    if (ch < K && (kind == 0 || d.layernorm))
                        apply(0, (kind == 0 ? ACM_SR_V_LOW : (kind == 1 ? ACM_SR_LNW_LOW : ACM_SR_LNB_LOW)) + ch, col, s);
                } else if (!RES || e < part4_of(F)) {
                    const int r = e - 3 * F * C8 - 12 * F, a = r / 4, b = r % 4;
                    if (a < K && b < K) apply(0, ACM_SR_MIX, a * K + b, s);
                } else {
                    apply(0, SR_RES_B, e - part4_of(F), s);
                }
            } else if (q < 96) {
                const int kind = q / 32, ch = (q / 8) % 4, c = q % 8;
                if (ch < K && c < C && (kind == 0 || d.layernorm))
                    apply(1, (kind == 0 ? ACM_SR_V_LOW : (kind == 1 ? ACM_SR_LNW_LOW : ACM_SR_LNB_LOW)) + ch, c, s);
            } else if (q < 112) {
                const int a = (q - 96) / 4, b = (q - 96) % 4;
                if (a < K && b < K) apply(1, ACM_SR_MIX, a * K + b, s);
            } else {
                d.loss[0] = s;
            }
        }
    }
    // nothing in this launch reads a step counter (launch 1 left the factors and the dropout counter of the step in the
    // workspace): the first block advances them
    if (blk == 0 && d.update) {
        if ((int)threadIdx.x < 2 * DEV_ROLES) {
            const SmallTensor t = take(d.t[threadIdx.x / DEV_ROLES][threadIdx.x % DEV_ROLES]);
            if (t.p && t.step) {
                // tensors that share one step scalar are advanced once (the first role that names it)
                bool first = true;
                for (int o = 0; o < (int)threadIdx.x; ++o) {
                    const SmallTensor u = take(d.t[o / DEV_ROLES][o % DEV_ROLES]);
                    if (u.p && u.step == t.step) first = false;
                }
                if (first) t.step[0] += 1.0f;
            }
        }
        if (threadIdx.x == 0 && d.also_advance) d.also_advance[0] += 1;
    }
}

// ------------------------------------------------------------------------------------------------ the kernels: single and batched forms
// Single form: the step's SmallDev by value in the kernel arguments (acm_small_step).
// Batched form (acm_small_batch_step, acm_small_batch_step_graphs): grid (an ENVELOPE of the single forms' x, n_slots); grid
// row blockIdx.y takes ITS SmallDev from a device table.  The entry is read through the constant address space -- the table is
// written by copies between launches only, never by a kernel, and the row index is wave-uniform -- so its fields arrive by
// scalar loads exactly as kernel arguments do; the bodies are templates over the block's reference type, so both forms are
// the same source.
// Every body takes n_wg, the producer workgroups of ITS step: the single form hands it gridDim.x, the batched form the width
// the entry was bound with (the slot's own handles' grid).  The launched grid may be wider -- the slots of one table may
// stand on different graphs (synthetic-experiments/train.py:64-164: ten graphs per homophily level, each with its own
// adjacency and features), and the launch is as wide as the widest -- and the workgroups past a slot's own width return before
// they touch LDS or a barrier (blockIdx is workgroup-uniform).  So a body runs with the blockIdx.x / n_wg of the single step,
// on the slot's own part3 / part4 / slots / counters / latch: the same instructions in the same order, the same bits.
struct SmallBatchEntry {
    int32_t active;                  // 0: an empty slot -- every launch returns before it touches anything else
    int32_t key[6];                  // per launch: the slot's OWN grid width * 16 + form (four | variant << 1 | train << 2 |
    int32_t item_blocks;             // (F == 32) << 3) the entry was bound for: a grid row of another form -- or of the other
                                     // hidden width, whose kernels read every table at another pitch -- or a launch narrower
                                     // than the slot's own width does nothing
    SmallDev first;                  // launch 1: reads the live dropout counter and latches it
    SmallDev rest;                   // launches 2-6: draw their masks with the latched copy
};
constexpr int FORM_NARROW = 8;       // the form's width bit: set for F = 32
constexpr int FORM_BITS = 16;        // a key is width * FORM_BITS + form
// V: the width the calling kernel was compiled for (it, not the host's word, decides the form's width bit); 0: a kernel
// that is the same for every width (launch 3), which takes the bit as it is given.  n_wg: the slot's own width (where an
// entry is returned, blockIdx.x < n_wg <= gridDim.x).
template <int LAUNCH, int V>
__device__ __forceinline__ const ACM_CONST_AS SmallBatchEntry* batch_entry(const SmallBatchEntry* table, int form, int& n_wg) {
    const ACM_CONST_AS SmallBatchEntry* e = (const ACM_CONST_AS SmallBatchEntry*)table + blockIdx.y;
    if (V != 0) form = (form & (FORM_NARROW - 1)) | (V == 2 ? FORM_NARROW : 0);
    n_wg = 0;
    if (e->active == 0) return nullptr;
    const int key = e->key[LAUNCH];
    n_wg = key / FORM_BITS;
    if (key % FORM_BITS != form || (int)gridDim.x < n_wg || (int)blockIdx.x >= n_wg) return nullptr;
    return e;
}
__host__ __device__ constexpr int form_of(bool four, bool variant, bool train, int hidden) {
    return (four ? 1 : 0) | (variant ? 2 : 0) | (train ? 4 : 0) | (hidden == 32 ? FORM_NARROW : 0);
}

// (RES: single form only -- the batched forms refuse residual plans at bind, acm_small_batch_host.h)
template <int V, bool RES>
__global__ __launch_bounds__(256) void small_proj1_kernel(SmallDev d) { small_proj1_body<V, RES>(d, (int)gridDim.x); }
template <int V>
__global__ __launch_bounds__(256) void small_proj1_batch_kernel(const SmallBatchEntry* table, int form) {
    int n_wg;
    const ACM_CONST_AS SmallBatchEntry* e = batch_entry<0, V>(table, form, n_wg);
    if (!e) return;
    const ACM_CONST_AS SmallDev& d = e->first;
    small_proj1_body<V, false>(d, n_wg);
}

template <int V, bool FOUR, bool VARIANT, bool RES>
__global__ __launch_bounds__(64 * WAVES) void small_conv1_fwd_kernel(SmallDev d, const float* z1) {
    small_conv1_fwd_body<V, FOUR, VARIANT, RES>(d, z1, (int)gridDim.x);
}
template <int V, bool FOUR, bool VARIANT>
__global__ __launch_bounds__(64 * WAVES) void small_conv1_fwd_batch_kernel(const SmallBatchEntry* table, int form) {
    int n_wg;
    const ACM_CONST_AS SmallBatchEntry* e = batch_entry<1, V>(table, form, n_wg);
    if (!e) return;
    const ACM_CONST_AS SmallDev& d = e->rest;
    small_conv1_fwd_body<V, FOUR, VARIANT, false>(d, d.Z1, n_wg);
}

template <bool FOUR>
__global__ __launch_bounds__(64 * WAVES) void small_conv2_fwd_kernel(SmallDev d) { small_conv2_fwd_body<FOUR>(d, (int)gridDim.x); }
template <bool FOUR>
__global__ __launch_bounds__(64 * WAVES) void small_conv2_fwd_batch_kernel(const SmallBatchEntry* table, int form) {
    int n_wg;
    const ACM_CONST_AS SmallBatchEntry* e = batch_entry<2, 0>(table, form, n_wg);
    if (!e) return;
    const ACM_CONST_AS SmallDev& d = e->rest;
    small_conv2_fwd_body<FOUR>(d, n_wg);
}

template <int V, bool FOUR, bool RES>
__global__ __launch_bounds__(64 * WAVES) void small_conv2_bwd_kernel(SmallDev d, const float* z1) {
    small_conv2_bwd_body<V, FOUR, RES>(d, z1, (int)gridDim.x);
}
template <int V, bool FOUR>
__global__ __launch_bounds__(64 * WAVES) void small_conv2_bwd_batch_kernel(const SmallBatchEntry* table, int form) {
    int n_wg;
    const ACM_CONST_AS SmallBatchEntry* e = batch_entry<3, V>(table, form, n_wg);
    if (!e) return;
    const ACM_CONST_AS SmallDev& d = e->rest;
    small_conv2_bwd_body<V, FOUR, false>(d, d.Z1, n_wg);
}

template <int V, bool FOUR, bool VARIANT>
__global__ __launch_bounds__(64 * WAVES) void small_conv1_bwd_kernel(SmallDev d, const float* z1) {
    small_conv1_bwd_body<V, FOUR, VARIANT>(d, z1, (int)gridDim.x);
}
template <int V, bool FOUR, bool VARIANT>
__global__ __launch_bounds__(64 * WAVES) void small_conv1_bwd_batch_kernel(const SmallBatchEntry* table, int form) {
    int n_wg;
    const ACM_CONST_AS SmallBatchEntry* e = batch_entry<4, V>(table, form, n_wg);
    if (!e) return;
    const ACM_CONST_AS SmallDev& d = e->rest;
    small_conv1_bwd_body<V, FOUR, VARIANT>(d, d.Z1, n_wg);
}

template <int V, bool RES>
__global__ __launch_bounds__(256) void small_finish_kernel(SmallDev d, int item_blocks, int red_blocks) {
    small_finish_body<V, RES>(d, item_blocks, red_blocks);
}
// Three waves per SIMD like the single form.  Left alone the compiler takes 172 registers here (the single form: 168, the
// limit for three waves) and drops to two; held to three it parks loop-invariant addresses in scratch (stored once per
// wave, read back once per work item).  EXPERIMENTS.md has the table.
// The slot's own width here is its own item_blocks + red_blocks (red_blocks depends on the hidden width alone): the reducing
// blocks follow the SLOT's item blocks, wherever the envelope's end.
template <int V>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3))) void small_finish_batch_kernel(const SmallBatchEntry* table, int form, int red_blocks) {
    int n_wg;
    const ACM_CONST_AS SmallBatchEntry* e = batch_entry<5, V>(table, form, n_wg);
    if (!e) return;
    const int item_blocks = e->item_blocks;
    if (item_blocks + red_blocks != n_wg) return;
    const ACM_CONST_AS SmallDev& d = e->rest;
    small_finish_body<V, false>(d, item_blocks, red_blocks);
}

ItemView view_of(const acm_csr* a) {
    ItemView v;
    v.items = a ? a->items : nullptr;
    v.n_items = a ? (int)a->n_items : 0;
    v.long_rows = a ? a->long_rows : nullptr;
    v.long_index = a ? a->long_index : nullptr;
    v.indices = a ? a->indices : nullptr;
    return v;
}

struct Layout {
    size_t Z1, H1, ST1, OUT1, T2, Z2I, G2, DZ2, G1, DZ1, slots, part3, part4, W2T, FACT, latch, long3, long4, counters, total;
    size_t WXT, R, XX, DR;                 // residual plans only
};

// The carve-up is the widest width's at every width (acm_small_step_workspace_bytes takes no shape): a narrower step uses
// the front of each block at its own pitch.  One function for the single and the batched form: they carve identically.
// `residual`: the residual branch's blocks are carved BEHIND the others (a plan without it allocates what it always did):
// the W_X^T table, R / xX / dR, and -- each a size larger than its namesake above, which then lies unused -- slots of four
// sums, partials and long-row records with db_X.
Layout layout_of(const acm_csr* a, const acm_csr* x, const acm_csr* xt, bool residual = false, int64_t f_in = 0) {
    constexpr int F = F_MAX, PART4 = part4_of(F_MAX), LONG4 = PART4;
    static_assert(SLOT_PITCH == 192 && 3 * F == 192 && 4 * F == 256, "the block sizes below are written out for F_MAX = 64");
    const size_t n = (size_t)a->n_rows;
    // the slot buffer and the arrival counters serve one launch at a time: sized for the handle with the most pieces
    size_t n_slots = (size_t)a->n_slots, n_long = (size_t)a->n_long;
    if (x) n_slots = std::max(n_slots, (size_t)x->n_slots), n_long = std::max(n_long, (size_t)x->n_long);
    if (xt) n_slots = std::max(n_slots, (size_t)xt->n_slots), n_long = std::max(n_long, (size_t)xt->n_long);
    Layout L;
    size_t o = 0;
    auto take = [&](size_t floats) {
        const size_t at = o;
        o += (floats + 63) / 64 * 64;          // 256-byte aligned blocks
        return at;
    };
    L.Z1 = take(n * 192), L.H1 = take(n * 256), L.ST1 = take(n * 16), L.OUT1 = take(n * 64);
    L.T2 = take(n * 24), L.Z2I = take(n * 8), L.G2 = take(n * 24), L.DZ2 = take(n * 24);
    L.G1 = take(n * 192), L.DZ1 = take(n * 192);
    L.slots = take((n_slots + 1) * 192);
    const size_t wg = (size_t)std::min<int64_t>(MAX_WG, (a->n_items + WAVES - 1) / WAVES);      // = the gather phases' grid
    L.part3 = take(wg * PART3_PITCH), L.part4 = take(wg * PART4);
    L.W2T = take(3 * F * C8), L.FACT = take(2 * DEV_ROLES * 2), L.latch = take(4);
    L.long3 = take((size_t)a->n_long * PART3_PITCH + 64), L.long4 = take((size_t)a->n_long * LONG4 + 64);
    L.counters = take(n_long + 64);
    L.WXT = L.R = L.XX = L.DR = 0;
    if (residual) {
        constexpr int PART4R = part4_of(F_MAX, true);
        L.WXT = take((size_t)f_in * F), L.R = take(n * 64), L.XX = take(n * 64), L.DR = take(n * 64);
        L.slots = take((n_slots + 1) * SLOT_PITCH_RES);
        L.part4 = take(wg * PART4R), L.long4 = take((size_t)a->n_long * PART4R + 64);
    }
    L.total = o * sizeof(float);
    return L;
}

}  // namespace

extern "C" int acm_small_step_workspace_bytes(const acm_csr_t* a_low, const acm_csr_t* x, const acm_csr_t* x_t, size_t* bytes) {
    ACM_REQUIRE(a_low && bytes, ACM_EINVAL, "acm_small_step_workspace_bytes: NULL argument");
    *bytes = layout_of(a_low, x, x_t).total;
    return ACM_OK;
}

extern "C" int acm_small_step_workspace_bytes_for(const acm_csr_t* a_low, const acm_csr_t* x, const acm_csr_t* x_t, const acm_small_step_t* shape,
                                                  size_t* bytes) {
    ACM_REQUIRE(a_low && shape && bytes, ACM_EINVAL, "acm_small_step_workspace_bytes_for: NULL argument");
    ACM_REQUIRE(shape->residual == 0 || shape->residual == 1, ACM_EINVAL, "acm_small_step_workspace_bytes_for: residual must be 0 or 1 (got %d)",
                (int)shape->residual);
    ACM_REQUIRE(shape->f_in >= 0, ACM_EINVAL, "acm_small_step_workspace_bytes_for: f_in %d", (int)shape->f_in);
    *bytes = layout_of(a_low, x, x_t, shape->residual != 0, shape->f_in).total;
    return ACM_OK;
}

extern "C" int acm_small_step_has_residual(void) { return 1; }

namespace {

// The grids of the six launches: functions of the handles and the hidden width alone -- the same for every slot of a batch on
// one graph; where the slots stand on different graphs, each slot's own (its table entry records them) under a launch of
// their element-wise maximum (acm_small_batch_grids_t).
struct Grids {
    int proj, wide, graph, item_blocks, red_blocks;
};
Grids grids_of(const acm_csr* a, const acm_csr* x, const acm_csr* xt, bool train, int hidden, bool residual = false) {
    const int PART4 = part4_of(hidden, residual);
    Grids g;
    g.proj = std::max((int)std::min<int64_t>(2 * MAX_WG, (x->n_items + 3) / 4), 1);
    g.graph = (int)std::min<int64_t>(MAX_WG, (a->n_items + WAVES - 1) / WAVES);
    g.wide = (int)std::min<int64_t>(MAX_WG_WIDE, (a->n_items + WAVES - 1) / WAVES);
    g.item_blocks = train ? (int)std::min<int64_t>(2 * MAX_WG, (xt->n_items + 3) / 4) : 0;
    g.red_blocks = (PART4 + PART3 + RED_EL - 1) / RED_EL;
    return g;
}

// Validates one run's block against the handles and fills what its kernels read: d1 for launch 1 (the live dropout counter),
// d for launches 2-6 (the latched one).  Shared by acm_small_step and acm_small_batch_bind: one envelope, one set of refusals.
int small_prepare(const acm_csr* a, const acm_csr* x, const acm_csr* xt, const acm_small_step_t* p, SmallDev& d1, SmallDev& d) {
    ACM_REQUIRE(a && p, ACM_EINVAL, "acm_small_step: NULL argument");
    ACM_REQUIRE(acm_small_hidden_ok(p->hidden), ACM_EUNSUPPORTED, "acm_small_step: hidden width %d (32 or 64; 0 means 64)", (int)p->hidden);
    ACM_REQUIRE(p->residual == 0 || p->residual == 1, ACM_EINVAL, "acm_small_step: residual must be 0 or 1 (got %d)", (int)p->residual);
    const bool res = p->residual != 0;
    if (res)
        ACM_REQUIRE(p->res[0].param && p->res[1].param, ACM_EINVAL,
                    "acm_small_step: residual without its parameters (res[0]: the Linear's weight, res[1]: its bias)");
    ACM_REQUIRE(a->vals == nullptr && a->n_rows == a->n_cols, ACM_EUNSUPPORTED,
                "acm_small_step: pattern-only square operators only (acm_csr_create with vals = NULL)");
    ACM_REQUIRE(a->n_rows >= 1 && a->n_rows <= 16384, ACM_EUNSUPPORTED, "acm_small_step: 1 .. 16384 rows (got %lld)", (long long)a->n_rows);
    ACM_REQUIRE(p->n_classes >= 1 && p->n_classes <= C8, ACM_EUNSUPPORTED, "acm_small_step: 1 .. 8 classes (got %d)", p->n_classes);
    ACM_REQUIRE(p->n_channels == 3 || p->n_channels == 4, ACM_EINVAL, "acm_small_step: n_channels must be 3 or 4");
    ACM_REQUIRE(p->row_scale && p->logits && p->att1 && p->att2 && p->workspace, ACM_EINVAL, "acm_small_step: NULL buffer");
    ACM_REQUIRE(x && p->x_vals, ACM_EINVAL, "acm_small_step: the CSR feature handle and its values (x, x_vals)");
    ACM_REQUIRE(x->n_rows == a->n_rows && x->n_cols == p->f_in, ACM_ESHAPE, "acm_small_step: feature handle is %lld x %lld, expected %lld x %d",
                (long long)x->n_rows, (long long)x->n_cols, (long long)a->n_rows, p->f_in);
    const int K = p->n_channels;
    if (p->train) {
        ACM_REQUIRE(p->labels && p->row_weight && p->loss, ACM_EINVAL, "acm_small_step: labels / row_weight / loss");
        ACM_REQUIRE(xt && p->xt_src_pos && xt->n_rows == p->f_in && xt->n_cols == a->n_rows, ACM_EINVAL,
                    "acm_small_step: the transposed feature handle (x_t, xt_src_pos) is needed for dW1");
    }
    const Layout L = layout_of(a, x, p->train ? xt : nullptr, res, p->f_in);
    ACM_REQUIRE(p->workspace_bytes >= L.total, ACM_ESHAPE, "acm_small_step: workspace of %zu bytes, %zu needed", p->workspace_bytes, L.total);
    // required roles
    for (int l = 0; l < 2; ++l) {
        for (int r = ACM_SR_W_LOW; r <= ACM_SR_V_MLP; ++r)
            ACM_REQUIRE(p->t[l][r].param, ACM_EINVAL, "acm_small_step: layer %d role %d has no parameter", l, r);
        ACM_REQUIRE(p->t[l][ACM_SR_MIX].param, ACM_EINVAL, "acm_small_step: layer %d has no mixing matrix", l);
        if (K == 4)
            ACM_REQUIRE(p->t[l][ACM_SR_V_STRUC].param && p->t[l][ACM_SR_STRUC].param, ACM_EINVAL, "acm_small_step: layer %d lacks the structure channel's parameters", l);
        if (p->layernorm)
            for (int c = 0; c < K; ++c)
                ACM_REQUIRE(p->t[l][ACM_SR_LNW_LOW + c].param && p->t[l][ACM_SR_LNB_LOW + c].param, ACM_EINVAL, "acm_small_step: layer %d lacks LayerNorm parameters", l);
    }
    d = SmallDev{};
    d.n = (int)a->n_rows, d.f_in = p->f_in, d.C = p->n_classes, d.k = K;
    d.relu_before = p->relu_before, d.layernorm = p->layernorm, d.train = p->train, d.update = p->update;
    d.scale = p->scale;
    for (int l = 0; l < 2; ++l)
        for (int r = 0; r < ACM_SMALL_ROLES; ++r) {
            const acm_adam_tensor_t& s = p->t[l][r];
            SmallTensor& t = d.t[l][r];
            const bool used = s.param && (r < ACM_SR_LNW_LOW || r == ACM_SR_MIX || r == ACM_SR_STRUC ? true : p->layernorm != 0) &&
                              !((r == ACM_SR_V_STRUC || r == ACM_SR_LNW_STRUC || r == ACM_SR_LNB_STRUC || r == ACM_SR_STRUC) && K == 3);
            if (!used) continue;
            t.p = s.param, t.g = const_cast<float*>(s.grad), t.m = s.exp_avg, t.v = s.exp_avg_sq, t.step = s.step;
            if (p->train && p->update) ACM_REQUIRE(t.m && t.v && t.step, ACM_EINVAL, "acm_small_step: layer %d role %d lacks Adam state", l, r);
            if (p->train && !p->update) ACM_REQUIRE(t.g, ACM_EINVAL, "acm_small_step: layer %d role %d has no gradient buffer (update = 0)", l, r);
        }
    if (res)
        for (int r = 0; r < 2; ++r) {
            const acm_adam_tensor_t& s = p->res[r];
            SmallTensor& t = d.t[0][SR_RES_W + r];
            t.p = s.param, t.g = const_cast<float*>(s.grad), t.m = s.exp_avg, t.v = s.exp_avg_sq, t.step = s.step;
            if (p->train && p->update) ACM_REQUIRE(t.m && t.v && t.step, ACM_EINVAL, "acm_small_step: residual tensor %d lacks Adam state", r);
            if (p->train && !p->update) ACM_REQUIRE(t.g, ACM_EINVAL, "acm_small_step: residual tensor %d has no gradient buffer (update = 0)", r);
        }
    d.graph = view_of(a), d.x = view_of(x), d.xt = view_of(p->train ? xt : nullptr);
    d.x_vals = p->x_vals, d.xt_src_pos = p->xt_src_pos, d.row_scale = p->row_scale;
    d.labels = p->labels, d.row_weight = p->row_weight, d.loss = p->loss, d.logits = p->logits, d.att1 = p->att1, d.att2 = p->att2;
    float* ws = (float*)p->workspace;
    d.Z1 = ws + L.Z1, d.H1 = ws + L.H1, d.ST1 = ws + L.ST1, d.OUT1 = ws + L.OUT1, d.T2 = ws + L.T2, d.Z2I = ws + L.Z2I;
    d.G2 = ws + L.G2, d.DZ2 = ws + L.DZ2, d.G1 = ws + L.G1, d.DZ1 = ws + L.DZ1;
    d.slots = ws + L.slots, d.part3 = ws + L.part3, d.part4 = ws + L.part4, d.W2T = ws + L.W2T, d.FACT = ws + L.FACT;
    d.xt_vals = p->xt_vals;
    d.long3 = ws + L.long3, d.long4 = ws + L.long4, d.n_long = (int)a->n_long;
    d.latch = reinterpret_cast<int64_t*>(ws + L.latch);
    d.counters = (int*)(ws + L.counters);
    d.drop_in = p->drop_in, d.drop_hidden = p->drop_hidden;
    d.residual = res ? 1 : 0;
    if (res) {
        d.WXT = ws + L.WXT, d.R = ws + L.R, d.XX = ws + L.XX, d.DR = ws + L.DR;
        d.drop_res = p->drop_res;
    }
    d.hp = AdamScalars{p->lr, p->beta1, p->beta2, p->eps, p->weight_decay, p->decoupled};
    d.also_advance = p->also_advance, d.arrive = p->arrive;
    d1 = d;                                        // launch 1 reads the live dropout counter and latches it for the others
    if (d.drop_in.p > 0.f) d.drop_in.step = d.latch;
    if (d.drop_hidden.p > 0.f) d.drop_hidden.step = d.latch;
    if (res && d.drop_res.p > 0.f) d.drop_res.step = d.latch;
    d.nwg3 = d.nwg4 = grids_of(a, x, xt, p->train != 0, acm_small_hidden_of(p)).graph;
    return ACM_OK;
}

// the checks acm_small_batch_step can make without the table (device memory): handles and the shared fields of `shape`
int batch_shape_check(const acm_csr* a, const acm_csr* x, const acm_csr* xt, int32_t n_slots, const acm_small_step_t* shape) {
    ACM_REQUIRE(n_slots >= 1, ACM_EINVAL, "acm_small_batch: n_slots must be 1 .. %d (got %d)", ACM_SMALL_BATCH_MAX, (int)n_slots);
    ACM_REQUIRE(n_slots <= ACM_SMALL_BATCH_MAX, ACM_EUNSUPPORTED, "acm_small_batch: n_slots %d > %d slots of one table", (int)n_slots,
                ACM_SMALL_BATCH_MAX);
    ACM_REQUIRE(a && x && shape, ACM_EINVAL, "acm_small_batch: NULL argument");
    ACM_REQUIRE(acm_small_hidden_ok(shape->hidden), ACM_EUNSUPPORTED, "acm_small_batch: hidden width %d (32 or 64; 0 means 64)", (int)shape->hidden);
    ACM_REQUIRE(shape->residual == 0, ACM_EUNSUPPORTED, "acm_small_batch: residual plans run as single steps only (residual = %d)", (int)shape->residual);
    ACM_REQUIRE(shape->n_channels == 3 || shape->n_channels == 4, ACM_EINVAL, "acm_small_batch: n_channels must be 3 or 4");
    ACM_REQUIRE(a->n_rows >= 1 && a->n_rows <= 16384 && a->vals == nullptr && a->n_rows == a->n_cols, ACM_EUNSUPPORTED,
                "acm_small_batch: pattern-only square operators of 1 .. 16384 rows");
    ACM_REQUIRE(x->n_rows == a->n_rows && x->n_cols == shape->f_in, ACM_ESHAPE, "acm_small_batch: feature handle shape");
    if (shape->train)
        ACM_REQUIRE(xt && xt->n_rows == shape->f_in && xt->n_cols == a->n_rows, ACM_EINVAL,
                    "acm_small_batch: the transposed feature handle (x_t) is needed for dW1");
    return ACM_OK;
}

}  // namespace

extern "C" int acm_small_step(const acm_csr_t* a, const acm_csr_t* x, const acm_csr_t* xt, const acm_small_step_t* p,
                              acm_stream_t stream) {
    SmallDev d1, d;
    const int st = small_prepare(a, x, xt, p, d1, d);
    if (st != ACM_OK) return st;
    const float* z1 = d.Z1;
    hipStream_t s = (hipStream_t)stream;
    const int hidden = acm_small_hidden_of(p);
    const Grids gr = grids_of(a, x, xt, p->train != 0, hidden, d.residual != 0);
    const int graph_wg = gr.graph, wide_wg = gr.wide;
    const int picked = acm_pick([&](auto v, auto four, auto variant, auto res) {
        // launch 0 (residual plans): the W_X^T table of this call
        if (res())
            hipLaunchKernelGGL(small_wxt_kernel, dim3((d.f_in + TR - 1) / TR, (hidden + TR - 1) / TR), dim3(256), 0, s,
                               (const float*)d.t[0][SR_RES_W].p, d.WXT, d.f_in, hidden);
        // launch 1
        hipLaunchKernelGGL((small_proj1_kernel<v(), res()>), dim3(gr.proj), dim3(256), 0, s, d1);
        // launch 2
        hipLaunchKernelGGL((small_conv1_fwd_kernel<v(), four(), variant(), res()>), dim3(wide_wg), dim3(64 * WAVES), 0, s, d, z1);
        // launch 3
        hipLaunchKernelGGL(small_conv2_fwd_kernel<four()>, dim3(graph_wg), dim3(64 * WAVES), 0, s, d);
        if (p->train) {
            // launch 4
            hipLaunchKernelGGL((small_conv2_bwd_kernel<v(), four(), res()>), dim3(graph_wg), dim3(64 * WAVES), 0, s, d, z1);
            // launch 5
            hipLaunchKernelGGL((small_conv1_bwd_kernel<v(), four(), variant()>), dim3(wide_wg), dim3(64 * WAVES), 0, s, d, z1);
            // launch 6
            hipLaunchKernelGGL((small_finish_kernel<v(), res()>), dim3(gr.item_blocks + gr.red_blocks), dim3(256), 0, s, d, gr.item_blocks, gr.red_blocks);
        }
        return ACM_OK;
    }, acm_one_of<2, 4>(hidden / 16), acm_flag(p->n_channels == 4), acm_flag(p->relu_before != 0), acm_flag(d.residual != 0));
    ACM_REQUIRE(picked != ACM_NO_INSTANTIATION, ACM_EUNSUPPORTED, "acm_small_step: no kernels for hidden width %d", hidden);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_small_step_has_hidden(int32_t hidden) { return acm_small_hidden_ok(hidden) ? 1 : 0; }

extern "C" int acm_small_batch_table_bytes(int32_t n_slots, size_t* bytes) {
    ACM_REQUIRE(bytes, ACM_EINVAL, "acm_small_batch_table_bytes: NULL argument");
    ACM_REQUIRE(n_slots >= 1, ACM_EINVAL, "acm_small_batch_table_bytes: n_slots must be 1 .. %d (got %d)", ACM_SMALL_BATCH_MAX, (int)n_slots);
    ACM_REQUIRE(n_slots <= ACM_SMALL_BATCH_MAX, ACM_EUNSUPPORTED, "acm_small_batch_table_bytes: n_slots %d > %d", (int)n_slots, ACM_SMALL_BATCH_MAX);
    *bytes = (size_t)n_slots * sizeof(SmallBatchEntry);
    return ACM_OK;
}

namespace {

Grids envelope_of(const acm_small_batch_grids_t& g) { return Grids{g.proj, g.wide, g.graph, g.item_blocks, g.red_blocks}; }
void fold_max(acm_small_batch_grids_t& into, const Grids& g) {
    into.proj = std::max(into.proj, g.proj), into.wide = std::max(into.wide, g.wide), into.graph = std::max(into.graph, g.graph);
    into.item_blocks = std::max(into.item_blocks, g.item_blocks), into.red_blocks = std::max(into.red_blocks, g.red_blocks);
}
// the six launch widths of a set of grids
void widths_of(const Grids& g, int (&w)[6]) {
    w[0] = g.proj, w[1] = g.wide, w[2] = g.graph, w[3] = g.graph, w[4] = g.wide, w[5] = g.item_blocks + g.red_blocks;
}

// Builds and writes the table: slot i's entry from ITS handles (a[i], x[i], xt[i]) -- its workspace carve-up, its nwg3 / nwg4,
// its long rows, its own grid widths -- and, with an envelope, the refusal of a slot whose own grid exceeds it in any launch.
// The caller has run the handle-free checks.  Nothing is copied or launched before every slot has passed.
int batch_bind_impl(const char* who, int32_t n_slots, const acm_csr* const* a, const acm_csr* const* x, const acm_csr* const* xt,
                    const acm_small_step_t* const* slots, const acm_small_batch_grids_t* env, void* table, size_t table_bytes,
                    acm_stream_t stream) {
    ACM_REQUIRE(table, ACM_EINVAL, "%s: NULL table", who);
    ACM_REQUIRE(table_bytes >= (size_t)n_slots * sizeof(SmallBatchEntry), ACM_ESHAPE, "%s: table of %zu bytes, %zu needed", who, table_bytes,
                (size_t)n_slots * sizeof(SmallBatchEntry));
    std::vector<SmallBatchEntry> host((size_t)n_slots);
    for (int i = 0; i < n_slots; ++i) {
        SmallBatchEntry& e = host[(size_t)i];
        e = SmallBatchEntry{};
        const acm_small_step_t* p = slots[i];
        if (!p) continue;
        ACM_REQUIRE(a[i], ACM_EINVAL, "%s: NULL operator handle (slot %d)", who, i);
        const int st = small_prepare(a[i], x[i], xt[i], p, e.first, e.rest);
        if (st != ACM_OK) return st;
        const int hidden = acm_small_hidden_of(p);
        const Grids gr = grids_of(a[i], x[i], xt[i], p->train != 0, hidden);
        const int form = form_of(p->n_channels == 4, p->relu_before != 0, p->train != 0, hidden);
        int gx[6];
        widths_of(gr, gx);
        if (env) {
            int ex[6];
            widths_of(envelope_of(*env), ex);
            for (int l = 0; l < 6; ++l)
                ACM_REQUIRE(gx[l] <= ex[l] && gr.red_blocks == env->red_blocks, ACM_ESHAPE,
                            "%s: slot %d needs %d workgroups in launch %d, the batch's grids have %d (fold every run's handles into the "
                            "grids with acm_small_batch_grids before the first bind)", who, i, gx[l], l + 1, ex[l]);
        }
        for (int l = 0; l < 6; ++l) e.key[l] = gx[l] * FORM_BITS + form;
        e.item_blocks = gr.item_blocks;
        e.active = 1;
    }
    hipStream_t s = (hipStream_t)stream;
    ACM_CHECK_HIP(hipMemcpyAsync(table, host.data(), host.size() * sizeof(SmallBatchEntry), hipMemcpyHostToDevice, s));
    ACM_CHECK_HIP(hipStreamSynchronize(s));         // `host` dies here: complete on return
    return ACM_OK;
}

// The six (train = 0: three) batched launches on grids (gr's x, n_slots).
int batch_launch(const char* who, int32_t n_slots, const acm_small_step_t* shape, const Grids& gr, const void* table, acm_stream_t stream) {
    const SmallBatchEntry* tb = (const SmallBatchEntry*)table;
    hipStream_t s = (hipStream_t)stream;
    const bool train = shape->train != 0, four = shape->n_channels == 4, variant = shape->relu_before != 0;
    const int hidden = acm_small_hidden_of(shape);
    const int form = form_of(four, variant, train, hidden);
    const unsigned B = (unsigned)n_slots;
    const dim3 wide(gr.wide, B), graph(gr.graph, B), blk(64 * WAVES);
    const int picked = acm_pick([&](auto v, auto four_c, auto variant_c) {
        // launch 1
        hipLaunchKernelGGL(small_proj1_batch_kernel<v()>, dim3(gr.proj, B), dim3(256), 0, s, tb, form);
        // launch 2
        hipLaunchKernelGGL((small_conv1_fwd_batch_kernel<v(), four_c(), variant_c()>), wide, blk, 0, s, tb, form);
        // launch 3
        hipLaunchKernelGGL(small_conv2_fwd_batch_kernel<four_c()>, graph, blk, 0, s, tb, form);
        if (train) {
            // launch 4
            hipLaunchKernelGGL((small_conv2_bwd_batch_kernel<v(), four_c()>), graph, blk, 0, s, tb, form);
            // launch 5
            hipLaunchKernelGGL((small_conv1_bwd_batch_kernel<v(), four_c(), variant_c()>), wide, blk, 0, s, tb, form);
            // launch 6
            hipLaunchKernelGGL(small_finish_batch_kernel<v()>, dim3(gr.item_blocks + gr.red_blocks, B), dim3(256), 0, s, tb, form, gr.red_blocks);
        }
        return ACM_OK;
    }, acm_one_of<2, 4>(hidden / 16), acm_flag(four), acm_flag(variant));
    ACM_REQUIRE(picked != ACM_NO_INSTANTIATION, ACM_EUNSUPPORTED, "%s: no kernels for hidden width %d", who, hidden);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

}  // namespace

// The special case "the same handles in every slot, the envelope = their own grids".
extern "C" int acm_small_batch_bind(const acm_csr_t* a, const acm_csr_t* x, const acm_csr_t* xt, int32_t n_slots,
                                    const acm_small_step_t* const* slots, void* table, size_t table_bytes, acm_stream_t stream) {
    // what needs neither a handle nor a device first (acm_small_batch_host.h): count, shared fields, overlaps
    char msg[256];
    const int st0 = acm_small_batch_check_slots(n_slots, slots, a ? a->n_rows : 0, msg, sizeof(msg));
    ACM_REQUIRE(st0 == ACM_OK, st0, "%s", msg);
    const std::vector<const acm_csr*> av((size_t)n_slots, a), xv((size_t)n_slots, x), xtv((size_t)n_slots, xt);
    return batch_bind_impl("acm_small_batch_bind", n_slots, av.data(), xv.data(), xtv.data(), slots, nullptr, table, table_bytes, stream);
}

extern "C" int acm_small_batch_step(const acm_csr_t* a, const acm_csr_t* x, const acm_csr_t* xt, int32_t n_slots,
                                    const acm_small_step_t* shape, const void* table, acm_stream_t stream) {
    const int st = batch_shape_check(a, x, xt, n_slots, shape);
    if (st != ACM_OK) return st;
    ACM_REQUIRE(table, ACM_EINVAL, "acm_small_batch_step: NULL table");
    return batch_launch("acm_small_batch_step", n_slots, shape, grids_of(a, x, xt, shape->train != 0, acm_small_hidden_of(shape)), table, stream);
}

// ---- slots on different graphs (synthetic-experiments/train.py:64-164)
extern "C" int acm_small_batch_grids(const acm_csr_t* a, const acm_csr_t* x, const acm_csr_t* xt, const acm_small_step_t* shape,
                                     acm_small_batch_grids_t* grids) {
    ACM_REQUIRE(grids, ACM_EINVAL, "acm_small_batch_grids: NULL grids");
    const int st = batch_shape_check(a, x, xt, 1, shape);
    if (st != ACM_OK) return st;
    fold_max(*grids, grids_of(a, x, xt, shape->train != 0, acm_small_hidden_of(shape)));
    return ACM_OK;
}

extern "C" int acm_small_batch_bind_graphs(int32_t n_slots, const acm_csr_t* const* a, const acm_csr_t* const* x, const acm_csr_t* const* xt,
                                           const acm_small_step_t* const* slots, const acm_small_batch_grids_t* grids, void* table,
                                           size_t table_bytes, acm_stream_t stream) {
    ACM_REQUIRE(n_slots < 1 || n_slots > ACM_SMALL_BATCH_MAX || (a && x && xt), ACM_EINVAL,
                "acm_small_batch_bind_graphs: NULL handle array (a_low, x and x_t are host arrays of n_slots handles)");
    ACM_REQUIRE(grids, ACM_EINVAL, "acm_small_batch_bind_graphs: NULL grids");
    int64_t rows[ACM_SMALL_BATCH_MAX];
    if (n_slots >= 1 && n_slots <= ACM_SMALL_BATCH_MAX)
        for (int i = 0; i < n_slots; ++i) rows[i] = a[i] ? a[i]->n_rows : 0;
    char msg[256];
    const int st0 = acm_small_batch_check_slots_graphs(n_slots, slots, rows, msg, sizeof(msg));
    ACM_REQUIRE(st0 == ACM_OK, st0, "%s", msg);
    return batch_bind_impl("acm_small_batch_bind_graphs", n_slots, a, x, xt, slots, grids, table, table_bytes, stream);
}

extern "C" int acm_small_batch_step_graphs(int32_t n_slots, const acm_small_step_t* shape, const acm_small_batch_grids_t* grids,
                                           const void* table, acm_stream_t stream) {
    ACM_REQUIRE(n_slots >= 1, ACM_EINVAL, "acm_small_batch: n_slots must be 1 .. %d (got %d)", ACM_SMALL_BATCH_MAX, (int)n_slots);
    ACM_REQUIRE(n_slots <= ACM_SMALL_BATCH_MAX, ACM_EUNSUPPORTED, "acm_small_batch: n_slots %d > %d slots of one table", (int)n_slots,
                ACM_SMALL_BATCH_MAX);
    ACM_REQUIRE(shape && grids && table, ACM_EINVAL, "acm_small_batch_step_graphs: NULL argument");
    ACM_REQUIRE(acm_small_hidden_ok(shape->hidden), ACM_EUNSUPPORTED, "acm_small_batch: hidden width %d (32 or 64; 0 means 64)", (int)shape->hidden);
    ACM_REQUIRE(shape->residual == 0, ACM_EUNSUPPORTED, "acm_small_batch: residual plans run as single steps only (residual = %d)", (int)shape->residual);
    ACM_REQUIRE(shape->n_channels == 3 || shape->n_channels == 4, ACM_EINVAL, "acm_small_batch: n_channels must be 3 or 4");
    const Grids gr = envelope_of(*grids);
    const int PART4 = part4_of(acm_small_hidden_of(shape));
    // what grids_of can produce, and nothing else: a launch never gets a width the caller made up
    ACM_REQUIRE(gr.proj >= 1 && gr.proj <= 2 * MAX_WG && gr.wide >= 1 && gr.wide <= MAX_WG_WIDE && gr.graph >= 1 && gr.graph <= MAX_WG &&
                    gr.item_blocks >= 0 && gr.item_blocks <= 2 * MAX_WG && (shape->train != 0 || gr.item_blocks == 0) &&
                    gr.red_blocks == (PART4 + PART3 + RED_EL - 1) / RED_EL,
                ACM_ESHAPE, "acm_small_batch_step_graphs: grids that acm_small_batch_grids did not form for this shape");
    return batch_launch("acm_small_batch_step_graphs", n_slots, shape, gr, table, stream);
}
