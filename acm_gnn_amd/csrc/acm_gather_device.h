// The gather family: every sparse product of the library goes through launch_gather.  The kernels are templates on the
// epilogue (Epi::Args, Epi::apply, Epi::kFusedHead), so each source that brings epilogues includes this header:
// acm_spmm.hip (EpiPlain), acm_conv.hip (EpiFwd, EpiRaw), acm_conv_bwd.hip (EpiBwd, EpiBwdLow / High / Struc).
//
// Execution shapes (wave = 64 lanes):
//   wide   (F > 8)  one wave per work item, lane l owns columns l, l+64, ... of every channel;
//                   the wave loads 64 (index, value) pairs with one coalesced instruction each,
//                   broadcasts them lane by lane (v_readlane -> SGPR row base) and issues
//                   UNR x NG x NREG independent 256 B row-segment loads before the FMAs.
//   narrow (F <= 8) GS lanes per work item, lanes over *neighbours*, every lane gathers the
//                   whole (NG x F)-float row of its neighbour with vector loads and the group
//                   all-reduces at the end; epilogue runs redundantly in the group.
// Rows longer than `chunk` neighbours are split into several work items whose partial sums
// are combined in slot order by a fix-up kernel (deterministic, no float atomics).
#pragma once
#include <type_traits>

#include "acm_conv_device.h"

// ------------------------------------------------------------------ epilogues
// Layouts A and B give every column exactly one owning lane; layout C replicates the row in
// every lane of the group, so only the group leader stores.
template <class L>
struct Owns {
    static __device__ __forceinline__ bool lane_stores(const L&) { return true; }
};
template <int FP>
struct Owns<LaySerial<FP>> {
    static __device__ __forceinline__ bool lane_stores(const LaySerial<FP>& l) { return l.lead; }
};
template <>
struct Owns<LayPair32> {
    static __device__ __forceinline__ bool lane_stores(const LayPair32& l) { return l.lane < 32; }
};
template <int NB>
struct Owns<LayVec16<NB>> {
    static __device__ __forceinline__ bool lane_stores(const LayVec16<NB>& l) { return l.lane < 16; }
};

// ------------------------------------------------------------------ wide gather
// element load of the gathered operand: fp32, or bf16 widened to fp32 (exact)
template <bool BF16>
__device__ __forceinline__ float load_gathered(const float* rowp_f32_units, long row_elems, int col) {
    if (BF16) {
        const unsigned short* p = reinterpret_cast<const unsigned short*>(rowp_f32_units) + row_elems + col;
        return __uint_as_float(((unsigned)*p) << 16);
    }
    return rowp_f32_units[row_elems + col];
}

template <int NREG, int NG, int UNR, bool BF16>
__device__ __forceinline__ void gather_wide(const GatherSrc& g, int F, const int32_t* __restrict__ indices,
                                            const float* __restrict__ vals, int begin, int end,
                                            int lane, float (&acc)[NG][NREG]) {
    for (int base = begin; base < end; base += 64) {
        const int kk = base + lane;
        int my_j = 0;
        float my_a = 0.f;
        if (kk < end) {
            my_j = indices[kk];
            my_a = vals ? vals[kk] : 1.f;           // pattern-only operator: implicit ones
        }
        const int cnt = min(64, end - base);  // wave-uniform
        int t = 0;
        for (; t + UNR <= cnt; t += UNR) {
            float z[UNR][NG][NREG];
            float a[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int j = __builtin_amdgcn_readlane(my_j, t + u);
                a[u] = acm_lane_f(my_a, t + u);
#pragma unroll
                for (int c = 0; c < NG; ++c) {
                    const long roff = (long)j * g.ld[c];
#pragma unroll
                    for (int r = 0; r < NREG; ++r) {
                        const int col = lane + 64 * r;
                        z[u][c][r] = (col < F) ? load_gathered<BF16>(g.p[c], roff, col) : 0.f;
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u)
#pragma unroll
                for (int c = 0; c < NG; ++c)
#pragma unroll
                    for (int r = 0; r < NREG; ++r) acc[c][r] = fmaf(a[u], z[u][c][r], acc[c][r]);
        }
        for (; t < cnt; ++t) {
            const int j = __builtin_amdgcn_readlane(my_j, t);
            const float a = acm_lane_f(my_a, t);
#pragma unroll
            for (int c = 0; c < NG; ++c) {
                const long roff = (long)j * g.ld[c];
#pragma unroll
                for (int r = 0; r < NREG; ++r) {
                    const int col = lane + 64 * r;
                    const float z = (col < F) ? load_gathered<BF16>(g.p[c], roff, col) : 0.f;
                    acc[c][r] = fmaf(a, z, acc[c][r]);
                }
            }
        }
    }
}

template <int NREG, int NG, class Epi, bool BF16 = false>
__global__ __launch_bounds__(256) void spmm_wide_kernel(CsrView csr, GatherSrc g, int F,
                                                        typename Epi::Args ea, float* __restrict__ partial) {
    // Blocks take work items in dispatch order (block b -> XCD b % 8): every XCD sees a uniform
    // sample of the rows, and on degree-sorted graphs the heavy items start first.  (A contiguous
    // per-XCD range, the usual GEMM swizzle, left 7 XCDs idle behind the hub rows: 133 -> 327 us.)
    const int lane = threadIdx.x & 63;
    const int w = acm_uniform(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (w >= csr.n_items) return;
    const AcmItem it = csr.items[w];
    const int row = acm_uniform(it.row), begin = acm_uniform(it.begin), end = acm_uniform(it.end),
              slot = acm_uniform(it.slot);
    float acc[NG][NREG];
#pragma unroll
    for (int c = 0; c < NG; ++c)
#pragma unroll
        for (int r = 0; r < NREG; ++r) acc[c][r] = 0.f;
    constexpr int UNR = (NG * NREG >= 8) ? 2 : (NG * NREG >= 4 ? 4 : 8);
    gather_wide<NREG, NG, UNR, BF16>(g, F, csr.indices, csr.vals, begin, end, lane, acc);
    if (slot < 0) {
        LayWide<NREG> lay{lane};
        Epi::template apply<LayWide<NREG>, NG>(ea, row, lay, F, acc);
    } else {
        float* ps = partial + (long)slot * (NG * F);
#pragma unroll
        for (int c = 0; c < NG; ++c)
#pragma unroll
            for (int r = 0; r < NREG; ++r) {
                const int col = lane + 64 * r;
                if (col < F) ps[c * F + col] = acc[c][r];
            }
    }
}

// bf16 gathered operand, F <= 64 (even): lane l of each half-wave owns the packed column pair (2l, 2l+1), the two
// half-waves walk alternate neighbours, so one dword load per lane fetches 2 neighbours x 128 B per channel --
// half the bytes AND half the load instructions of the fp32 path (2-byte per-lane loads were slower than fp32:
// 804 -> 1290 us).  The halves are combined with v_permlane32_swap, then the epilogue runs in LayPair32.
template <int NG, class Epi, bool BF16>
__global__ __launch_bounds__(256) void spmm_pair_kernel(CsrView csr, GatherSrc g, int F, typename Epi::Args ea,
                                                        float* __restrict__ partial) {
    const int lane = threadIdx.x & 63, half = lane >> 5, l32 = lane & 31;
    const int w = acm_uniform(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (w >= csr.n_items) return;
    const AcmItem it = csr.items[w];
    const int row = acm_uniform(it.row), begin = acm_uniform(it.begin), end = acm_uniform(it.end),
              slot = acm_uniform(it.slot);
    float acc[NG][2];
#pragma unroll
    for (int c = 0; c < NG; ++c) acc[c][0] = acc[c][1] = 0.f;
    const bool col_ok = 2 * l32 < F;
    constexpr int UNR = 4;
    for (int base = begin; base < end; base += 64) {
        const int kk = base + lane;
        int my_j = 0;
        float my_a = 0.f;
        if (kk < end) {
            my_j = csr.indices[kk];
            my_a = csr.vals ? csr.vals[kk] : 1.f;
        }
        const int cnt = min(64, end - base);
        for (int t = 0; t < cnt; t += 2 * UNR) {
            unsigned zz[UNR][NG];      // bf16: one packed pair
            float2 zf[UNR][NG];        // fp32: the two adjacent columns
            float a[UNR];
            bool ok[UNR];
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                const int t0 = t + 2 * u;                         // wave-uniform
                const bool have0 = t0 < cnt, have1 = t0 + 1 < cnt;
                const int j0 = __builtin_amdgcn_readlane(my_j, have0 ? t0 : 0);
                const int j1 = __builtin_amdgcn_readlane(my_j, have1 ? t0 + 1 : 0);
                const float a0 = acm_lane_f(my_a, have0 ? t0 : 0), a1 = acm_lane_f(my_a, have1 ? t0 + 1 : 0);
                const int j = half ? j1 : j0;
                a[u] = half ? a1 : a0;
                ok[u] = (half ? have1 : have0) && col_ok;
#pragma unroll
                for (int c = 0; c < NG; ++c) {
                    if (BF16) {
                        const unsigned* rowp = reinterpret_cast<const unsigned*>(
                            reinterpret_cast<const unsigned short*>(g.p[c]) + (long)j * g.ld[c]);
                        zz[u][c] = rowp[col_ok ? l32 : 0];
                    } else {
                        const float2* rowp = reinterpret_cast<const float2*>(g.p[c] + (long)j * g.ld[c]);
                        zf[u][c] = rowp[col_ok ? l32 : 0];
                    }
                }
            }
#pragma unroll
            for (int u = 0; u < UNR; ++u)
#pragma unroll
                for (int c = 0; c < NG; ++c) {
                    const float lo = BF16 ? __uint_as_float(zz[u][c] << 16) : zf[u][c].x;
                    const float hi = BF16 ? __uint_as_float(zz[u][c] & 0xFFFF0000u) : zf[u][c].y;
                    acc[c][0] = ok[u] ? fmaf(a[u], lo, acc[c][0]) : acc[c][0];
                    acc[c][1] = ok[u] ? fmaf(a[u], hi, acc[c][1]) : acc[c][1];
                }
        }
    }
    // add the two half-waves (fixed order: lower + upper)
#pragma unroll
    for (int c = 0; c < NG; ++c)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const acm_u32x2 r = __builtin_amdgcn_permlane32_swap(__float_as_uint(acc[c][i]), __float_as_uint(acc[c][i]),
                                                                 false, false);
            acc[c][i] = __uint_as_float(r[0]) + __uint_as_float(r[1]);
        }
    if (slot < 0) {
        LayPair32 lay{lane};
        Epi::template apply<LayPair32, NG>(ea, row, lay, F, acc);
    } else if (lane < 32) {
        float* ps = partial + (long)slot * (NG * F);
#pragma unroll
        for (int c = 0; c < NG; ++c)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int col = 2 * l32 + i;
                if (col < F) ps[c * F + col] = acc[c][i];
            }
    }
}

// ------------------------------------------------------------------ wide gather, vector form
// Four neighbours per load instruction: a 16-lane group (one DPP row) fetches one 64-column block of one neighbour's
// row with a dwordx4 per lane (256 B per group, 1 KB per wave instruction -- the dword-per-lane form above moves 256 B
// per instruction), the four groups of the wave walk four consecutive neighbours.  Column ids are loaded TRANSPOSED
// (lane (q, m) holds neighbour 4 m + q of the 64-id batch) so that step u needs lane u of every group: one
// `v_mov_b32_dpp row_newbcast:u` per step, no readlane / select chain and no LDS crossbar.  UNR steps x NG channels x NB
// blocks of loads are in flight per wave (8 KB at NG = 2), the four groups' partial sums meet at the end through
// v_permlane16/32_swap (fixed order), and the epilogue runs in LayVec16 (lane m owns columns 4 m .. 4 m + 3 of every
// block).  Needs 16-byte aligned rows (F % 4 == 0, ld % 4 == 0); row offsets are 32-bit byte offsets (table < 4 GB).
// B16: the gathered tables hold bf16 (acm_cast_bf16): the lane's four columns are one 8-byte fetch (a 64-column row is ONE
// 128-byte line instead of two), widened exactly to fp32 -- same lane layout, same fp32 sums.
template <int NG, int NB, int UNR, int BLK, bool B16 = false>
__device__ __forceinline__ void gather_vec_block(const GatherSrc& g, const unsigned (&ldb)[3], const unsigned (&blk_off)[NB],
                                                 unsigned ok_mask, int my_j, float my_a, float (&acc)[NG][4 * NB]) {
    float4 z[UNR][NG][NB];
    float a[UNR];
#pragma unroll
    for (int uu = 0; uu < UNR; ++uu) {
        const unsigned j = (unsigned)acm_row_bcast(my_j, BLK * UNR + uu);
        a[uu] = __int_as_float(acm_row_bcast(__float_as_int(my_a), BLK * UNR + uu));
#pragma unroll
        for (int c = 0; c < NG; ++c) {
            const char* rp = reinterpret_cast<const char*>(g.p[c]) + (size_t)(j * ldb[c]);
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                if (B16) {
                    const uint2 w = *reinterpret_cast<const uint2*>(rp + blk_off[b]);
                    z[uu][c][b] = make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xFFFF0000u),
                                              __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xFFFF0000u));
                } else {
                    z[uu][c][b] = *reinterpret_cast<const float4*>(rp + blk_off[b]);
                }
            }
        }
    }
#pragma unroll
    for (int uu = 0; uu < UNR; ++uu) {
        // an idle slot (beyond the row's end) fetched row 0 and a lane whose columns lie beyond F fetched the row's first
        // bytes: select, never multiply by a zero weight (0 * inf = NaN would leak a non-finite row the operator does not
        // reference)
        const float av = a[uu];
#pragma unroll
        for (int c = 0; c < NG; ++c)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                const bool live = ((ok_mask >> b) & 1u) && av != 0.f;
                acc[c][4 * b + 0] = live ? fmaf(av, z[uu][c][b].x, acc[c][4 * b + 0]) : acc[c][4 * b + 0];
                acc[c][4 * b + 1] = live ? fmaf(av, z[uu][c][b].y, acc[c][4 * b + 1]) : acc[c][4 * b + 1];
                acc[c][4 * b + 2] = live ? fmaf(av, z[uu][c][b].z, acc[c][4 * b + 2]) : acc[c][4 * b + 2];
                acc[c][4 * b + 3] = live ? fmaf(av, z[uu][c][b].w, acc[c][4 * b + 3]) : acc[c][4 * b + 3];
            }
    }
}

template <int NG, int NB, class Epi, bool B16 = false>
__global__ __launch_bounds__(256) void spmm_vec_kernel(CsrView csr, GatherSrc g, int F, typename Epi::Args ea,
                                                       float* __restrict__ partial) {
    constexpr int UNR = (NG * NB >= 4) ? 2 : 4;          // 8 (NG * NB <= 2), 12 (NG = 3) or NG * NB * 2 loads in flight
    const int lane = threadIdx.x & 63, m = lane & 15, q = lane >> 4;
    const int w = acm_uniform(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (w >= csr.n_items) return;
    const AcmItem it = csr.items[w];
    const int row = acm_uniform(it.row), begin = acm_uniform(it.begin), end = acm_uniform(it.end),
              slot = acm_uniform(it.slot);
    float acc[NG][4 * NB];
#pragma unroll
    for (int c = 0; c < NG; ++c)
#pragma unroll
        for (int i = 0; i < 4 * NB; ++i) acc[c][i] = 0.f;
    // byte offset of the lane's float4 in column block b; a lane whose columns lie beyond F (F % 4 == 0, F < 64 NB) reads
    // the row's first bytes instead (always inside the row) and contributes nothing
    unsigned blk_off[NB], ok_mask = 0;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const bool ok = 64 * b + 4 * m < F;
        blk_off[b] = ok ? (B16 ? 128u * b + 8u * m : 256u * b + 16u * m) : 0u;
        ok_mask |= ok ? (1u << b) : 0u;
    }
    unsigned ldb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) ldb[c] = c < NG ? (unsigned)g.ld[c] * (B16 ? 2u : 4u) : 0u;
    const int pos = 4 * m + q;                           // transposed id layout (see above)
    for (int base = begin; base < end; base += 64) {
        const int cnt = min(64, end - base);             // wave-uniform
        int my_j = 0;
        float my_a = 0.f;
        if (pos < cnt) {
            my_j = csr.indices[base + pos];
            my_a = csr.vals ? csr.vals[base + pos] : 1.f;
        }
        const int steps = (cnt + 3) >> 2;
        // the step index must be a compile-time constant for the DPP broadcast: 16 / UNR unrolled blocks, uniform exits
#define ACM_VEC_BLK(B)                                                                                          \
        if (B * UNR < steps) gather_vec_block<NG, NB, UNR, B, B16>(g, ldb, blk_off, ok_mask, my_j, my_a, acc)
        ACM_VEC_BLK(0);
        ACM_VEC_BLK(1);
        ACM_VEC_BLK(2);
        ACM_VEC_BLK(3);
        if (UNR == 2) {
            ACM_VEC_BLK(4);
            ACM_VEC_BLK(5);
            ACM_VEC_BLK(6);
            ACM_VEC_BLK(7);
        }
#undef ACM_VEC_BLK
    }
#pragma unroll
    for (int c = 0; c < NG; ++c)
#pragma unroll
        for (int i = 0; i < 4 * NB; ++i) acc[c][i] = acm_cross_row_sum(acc[c][i]);
    if (slot < 0) {
        LayVec16<NB> lay{lane};
        Epi::template apply<LayVec16<NB>, NG>(ea, row, lay, F, acc);
    } else if (q == 0) {
        float* ps = partial + (long)slot * (NG * F);
#pragma unroll
        for (int c = 0; c < NG; ++c)
#pragma unroll
            for (int i = 0; i < 4 * NB; ++i) {
                const int col = 64 * (i >> 2) + 4 * m + (i & 3);
                if (col < F) ps[c * F + col] = acc[c][i];
            }
    }
}

// One wave per long row: add its partial slots in slot order, then the epilogue.
template <int NREG, int NG, class Epi>
__global__ __launch_bounds__(256) void spmm_fixup_kernel(CsrView csr, int F, typename Epi::Args ea,
                                                         const float* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const int w = acm_uniform(blockIdx.x * 4 + (threadIdx.x >> 6));
    if (w >= csr.n_long) return;
    const AcmLongRow lr = csr.long_rows[w];
    const int row = acm_uniform(lr.row), sb = acm_uniform(lr.slot_begin), se = acm_uniform(lr.slot_end);
    float acc[NG][NREG];
#pragma unroll
    for (int c = 0; c < NG; ++c)
#pragma unroll
        for (int r = 0; r < NREG; ++r) acc[c][r] = 0.f;
    // four slots' loads in flight, added in slot order (a dependent load per slot made this the latency of 16 round trips)
    int s = sb;
    for (; s + 4 <= se; s += 4) {
        float v[4][NG][NREG];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float* ps = partial + (long)(s + u) * (NG * F);
#pragma unroll
            for (int c = 0; c < NG; ++c)
#pragma unroll
                for (int r = 0; r < NREG; ++r) {
                    const int col = lane + 64 * r;
                    v[u][c][r] = col < F ? ps[c * F + col] : 0.f;
                }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int c = 0; c < NG; ++c)
#pragma unroll
                for (int r = 0; r < NREG; ++r) acc[c][r] += v[u][c][r];
    }
    for (; s < se; ++s) {
        const float* ps = partial + (long)s * (NG * F);
#pragma unroll
        for (int c = 0; c < NG; ++c)
#pragma unroll
            for (int r = 0; r < NREG; ++r) {
                const int col = lane + 64 * r;
                if (col < F) acc[c][r] += ps[c * F + col];
            }
    }
    LayWide<NREG> lay{lane};
    Epi::template apply<LayWide<NREG>, NG>(ea, row, lay, F, acc);
}

// ------------------------------------------------------------------ narrow gather
template <int FP>
__device__ __forceinline__ void load_row(const float* __restrict__ p, int F, bool vec, float (&z)[FP]) {
    if (vec) {
        if (FP == 2) {
            const float2 v = *reinterpret_cast<const float2*>(p);
            z[0] = v.x;
            z[1] = v.y;
        } else {
#pragma unroll
            for (int q = 0; q < FP / 4; ++q) {
                const float4 v = reinterpret_cast<const float4*>(p)[q];
                z[4 * q + 0] = v.x;
                z[4 * q + 1] = v.y;
                z[4 * q + 2] = v.z;
                z[4 * q + 3] = v.w;
            }
        }
    } else {
#pragma unroll
        for (int f = 0; f < FP; ++f) z[f] = (f < F) ? p[f] : 0.f;
    }
}

// Narrow gather (F <= 8): one neighbour per lane, GS lanes per work item, the whole gathered row in the lane.
// MERGED: channels 0 and 1 are one contiguous 16-byte-aligned block [c0 (FP) | c1 (FP)] in a row of
// g.p[0], fetched with float4 loads -- one L2 request per neighbour instead of two (the narrow
// kernels are bound by L1->L2 request count, profiles/r01_pmc_*.csv).
// Software-pipelined over the work list: most rows of a power-law graph are one step long (79 % of the
// twitch rows have <= 64 neighbours), so the per-item chain
//     item descriptor -> column ids -> gathered rows -> reduce -> epilogue
// is four dependent memory latencies with nothing to overlap them inside the wave.  A group therefore walks
// the work list with a grid stride (grid capped at NARROW_MAX_BLOCKS), and while the rows of the current
// step are in flight it already has the next item's descriptor and the next step's column ids / values
// requested (of the same item, or of the next one when this was its last step).
constexpr int NARROW_MAX_BLOCKS = 8192;
constexpr int NARROW_U = 2;

// U = neighbours per lane and step (rows in flight per lane): a lane takes neighbours gl, gl + GS, gl + 2 GS, ... of its item in
// that order whatever U is, so U changes how many steps an item takes -- the dependent chain of a long item -- and not one bit
// of the result.  Measured (round 4, profiles/r04_narrow_u4.txt): U = 4 changes neither the single-GPU kernels (70.4 / 56.0 us
// against 72 / 54.6) nor a rank's kernels of the 8-rank plan (33.0 us against 32.9): the sixteen pieces of the longest row
// are bound by the texture path of the ONE CU their window runs on, not by the number of dependent steps.
template <int FP, int NG, int GS, bool MERGED, class Epi, int U = NARROW_U>
__global__ __launch_bounds__(256) void spmm_narrow_kernel(CsrView csr, GatherSrc g, int F, int vecmask,
                                                               typename Epi::Args ea, float* __restrict__ partial) {
    constexpr int GPB = 256 / GS;
    // GS == 16: a workgroup round is one window of the work list, so the pieces of a long row meet in LDS and the
    // first piece's group finishes the row -- no partial slots, no fix-up launch (acm_csr.cpp, build_items)
    constexpr bool COOP = GS == ACM_WINDOW && GPB == ACM_WINDOW;
    __shared__ float coop_lds[COOP ? ACM_WINDOW * NG * FP : 1];
    const int gl = threadIdx.x % GS;
    const int G = gridDim.x * GPB;
    int w = blockIdx.x * GPB + threadIdx.x / GS;
    if (w >= csr.n_items) return;
    AcmItem it = csr.items[w];
    int k0 = it.begin;
    const bool unit = csr.vals == nullptr;
    bool v[U];
    int j[U];
    float a[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int k = k0 + gl + u * GS;
        v[u] = k < it.end;
        j[u] = v[u] ? csr.indices[k] : 0;
        a[u] = v[u] ? (unit ? 1.f : csr.vals[k]) : 0.f;
    }
    while (true) {
        const int wn = w + G;
        const bool has_next = wn < csr.n_items;
        AcmItem itn = it;
        if (has_next) itn = csr.items[wn];
        float acc[NG][FP];
#pragma unroll
        for (int c = 0; c < NG; ++c)
#pragma unroll
            for (int f = 0; f < FP; ++f) acc[c][f] = 0.f;
        while (true) {
            float z[U][NG][FP];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                if (MERGED) {
                    float t[2 * FP];
                    load_row<2 * FP>(g.p[0] + (long)j[u] * g.ld[0], 2 * FP, true, t);
#pragma unroll
                    for (int f = 0; f < FP; ++f) {
                        z[u][0][f] = t[f];
                        if (NG > 1) z[u][1 % NG][f] = t[FP + f];
                    }
#pragma unroll
                    for (int c = 2; c < NG; ++c) load_row<FP>(g.p[c] + (long)j[u] * g.ld[c], F, (vecmask >> c) & 1, z[u][c]);
                } else {
#pragma unroll
                    for (int c = 0; c < NG; ++c) load_row<FP>(g.p[c] + (long)j[u] * g.ld[c], F, (vecmask >> c) & 1, z[u][c]);
                }
            }
            // requests of the next step, issued before the rows above are consumed
            const int k1 = k0 + U * GS;
            const bool more = k1 < it.end;
            const int pb = more ? k1 : itn.begin;
            const int pe = more ? it.end : (has_next ? itn.end : pb);
            bool nv[U];
            int nj[U];
            float na[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = pb + gl + u * GS;
                nv[u] = k < pe;
                nj[u] = nv[u] ? csr.indices[k] : 0;
                na[u] = nv[u] ? (unit ? 1.f : csr.vals[k]) : 0.f;
            }
#pragma unroll
            for (int c = 0; c < NG; ++c)
#pragma unroll
                for (int f = 0; f < FP; ++f)
#pragma unroll
                    for (int u = 0; u < U; ++u) acc[c][f] = v[u] ? fmaf(a[u], z[u][c][f], acc[c][f]) : acc[c][f];
#pragma unroll
            for (int u = 0; u < U; ++u) j[u] = nj[u], a[u] = na[u], v[u] = nv[u];
            if (!more) break;
            k0 = k1;
        }
#pragma unroll
        for (int c = 0; c < NG; ++c)
#pragma unroll
            for (int f = 0; f < FP; ++f) acc[c][f] = acm_group_sum<GS>(acc[c][f]);
        if (COOP && w / ACM_WINDOW < csr.n_windows) {          // uniform over the workgroup: every item here is a piece
            const int g = threadIdx.x / GS;
            if (gl == 0) {
#pragma unroll
                for (int c = 0; c < NG; ++c)
#pragma unroll
                    for (int f = 0; f < FP; ++f) coop_lds[(g * NG + c) * FP + f] = acc[c][f];
            }
            __syncthreads();
            const AcmLongRow lr = csr.long_rows[csr.long_index[it.row]];
            // a row of several windows (acm_csr.cpp, build_items) fills this window alone: its sum goes to the slot of the
            // window's first piece and spmm_fixup_windows_kernel adds the windows
            const bool multi = lr.windows > 1;
            if (multi ? g == 0 : it.slot == lr.slot_begin) {    // first piece: add the others in slot order
                const int pieces = multi ? ACM_WINDOW : lr.slot_end - lr.slot_begin;
#pragma unroll
                for (int c = 0; c < NG; ++c)
#pragma unroll
                    for (int f = 0; f < FP; ++f) {
                        float t = 0.f;
                        for (int q = 0; q < pieces; ++q) t += coop_lds[((g + q) * NG + c) * FP + f];
                        acc[c][f] = t;
                    }
                if (!multi) {
                    LaySerial<FP> lay{gl == 0};
                    Epi::template apply<LaySerial<FP>, NG>(ea, it.row, lay, F, acc);
                } else if (gl == 0) {
                    float* ps = partial + (long)it.slot * (NG * F);
#pragma unroll
                    for (int c = 0; c < NG; ++c)
#pragma unroll
                        for (int f = 0; f < FP; ++f)
                            if (f < F) ps[c * F + f] = acc[c][f];
                }
            }
            __syncthreads();
        } else if (it.slot < 0) {
            LaySerial<FP> lay{gl == 0};
            Epi::template apply<LaySerial<FP>, NG>(ea, it.row, lay, F, acc);
        } else if (gl == 0) {
            float* ps = partial + (long)it.slot * (NG * F);
#pragma unroll
            for (int c = 0; c < NG; ++c)
#pragma unroll
                for (int f = 0; f < FP; ++f)
                    if (f < F) ps[c * F + f] = acc[c][f];
        }
        if (!has_next) break;
        it = itn;
        w = wn;
        k0 = it.begin;
    }
}

// Long rows of the narrow path: a 16-lane group per row, lanes over the partial slots (the wide
// fix-up would leave 62 of 64 lanes idle at F = 2 and chain up to deg/chunk dependent loads).
template <int FP, int NG, class Epi>
__global__ __launch_bounds__(256) void spmm_fixup_narrow_kernel(CsrView csr, int F, typename Epi::Args ea,
                                                                const float* __restrict__ partial) {
    const int m = threadIdx.x & 15;
    const int w = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (w >= csr.n_long) return;
    const AcmLongRow lr = csr.long_rows[w];
    float acc[NG][FP];
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
    LaySerial<FP> lay{m == 0};
    Epi::template apply<LaySerial<FP>, NG>(ea, lr.row, lay, F, acc);
}

// Rows of several windows (AcmLongRow.windows > 1) after a narrow gather with sixteen lanes per item: window q of the row
// left its sum in slot slot_begin + 16 q; lane q of a 16-lane group fetches it, one group sum (fixed order), epilogue.
template <int FP, int NG, class Epi>
__global__ __launch_bounds__(256) void spmm_fixup_windows_kernel(CsrView csr, int F, typename Epi::Args ea,
                                                                 const float* __restrict__ partial) {
    const int m = threadIdx.x & 15;
    const int w = blockIdx.x * 16 + (threadIdx.x >> 4);
    if (w >= csr.n_long) return;
    const AcmLongRow lr = csr.long_rows[w];
    if (lr.windows <= 1) return;
    float acc[NG][FP];
    const float* ps = partial + (long)(lr.slot_begin + ACM_WINDOW * m) * (NG * F);
#pragma unroll
    for (int c = 0; c < NG; ++c)
#pragma unroll
        for (int f = 0; f < FP; ++f) acc[c][f] = (m < lr.windows && f < F) ? ps[c * F + f] : 0.f;
#pragma unroll
    for (int c = 0; c < NG; ++c)
#pragma unroll
        for (int f = 0; f < FP; ++f) acc[c][f] = acm_group_sum<16>(acc[c][f]);
    LaySerial<FP> lay{m == 0};
    Epi::template apply<LaySerial<FP>, NG>(ea, lr.row, lay, F, acc);
}

// The four-channel narrow gather (structure_info = 1, F = 2: the output layer of the reference's two-class models) over
// PACKED 32-byte rows [c0 c0 c1 c1 | c2 c2 - -]: with the third gathered channel in a table of its own a neighbour costs two
// fetches to two distinct lines (the [c0 | c1] block and the 8-byte c2 row) -- 115 us on the twitch-shaped graph against
// 51 us for the three-channel layer -- while what bounds these gathers is the number of distinct lines per wave
// instruction, not their width (ta_rate).  Two adjacent lanes fetch the two 16-byte halves of a
// neighbour's row (the form of agg_fused_pair_kernel): one line per neighbour again.
// Lane (e = gl >> 1, h = gl & 1) of the 16-lane group: neighbours k0 + e + 8 u (u = 0..3), half h of the row.
template <class Epi>
__global__ __launch_bounds__(256) void spmm_narrow_pair3_kernel(CsrView csr, const float* __restrict__ table, typename Epi::Args ea,
                                                                float* __restrict__ partial) {
    constexpr int FP = 2, NG = 3, GPB = 16, U = 4, STEP = 8 * U;
    static_assert(GPB == ACM_WINDOW, "one window of work items per workgroup round");
    __shared__ float coop[ACM_WINDOW * 8];
    const int gl = threadIdx.x & 15, e = gl >> 1, h = gl & 1;
    const int G = gridDim.x * GPB;
    int w = blockIdx.x * GPB + (threadIdx.x >> 4);
    if (w >= csr.n_items) return;
    const bool unit = csr.vals == nullptr;
    const float* th = table + 4 * h;
    AcmItem it = csr.items[w];
    int k0 = it.begin;
    int j[U];
    float a[U];
    bool v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
        const int k = k0 + e + 8 * u;
        v[u] = k < it.end;
        j[u] = v[u] ? csr.indices[k] : 0;
        a[u] = v[u] ? (unit ? 1.f : csr.vals[k]) : 0.f;
    }
    while (true) {
        const int wn = w + G;
        const bool has_next = wn < csr.n_items;
        AcmItem itn = it;
        if (has_next) itn = csr.items[wn];
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        while (true) {
            float4 z[U];
#pragma unroll
            for (int u = 0; u < U; ++u) z[u] = *reinterpret_cast<const float4*>(th + (long)j[u] * 8);
            const int k1 = k0 + STEP;
            const bool more = k1 < it.end;
            const int pb = more ? k1 : itn.begin;
            const int pe = more ? it.end : (has_next ? itn.end : pb);
            int nj[U];
            float na[U];
            bool nv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int k = pb + e + 8 * u;
                nv[u] = k < pe;
                nj[u] = nv[u] ? csr.indices[k] : 0;
                na[u] = nv[u] ? (unit ? 1.f : csr.vals[k]) : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                acc[0] = v[u] ? fmaf(a[u], z[u].x, acc[0]) : acc[0];
                acc[1] = v[u] ? fmaf(a[u], z[u].y, acc[1]) : acc[1];
                acc[2] = v[u] ? fmaf(a[u], z[u].z, acc[2]) : acc[2];
                acc[3] = v[u] ? fmaf(a[u], z[u].w, acc[3]) : acc[3];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) j[u] = nj[u], a[u] = na[u], v[u] = nv[u];
            if (!more) break;
            k0 = k1;
        }
        // sum over the eight lanes of the group with the same half (lanes gl, gl^2, gl+-4, gl+-8): fixed order
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            acc[i] += acm_dpp<0x4E>(acc[i]);     // quad_perm [2,3,0,1]
            acc[i] += acm_dpp<0x124>(acc[i]);    // row_ror:4
            acc[i] += acm_dpp<0x128>(acc[i]);    // row_ror:8
        }
        bool finish = it.slot < 0;
        if (w / ACM_WINDOW < csr.n_windows) {                   // a window of pieces: they meet in LDS (see spmm_narrow_kernel)
            const int g = threadIdx.x >> 4;
            if (gl < 2) {
#pragma unroll
                for (int i = 0; i < 4; ++i) coop[g * 8 + 4 * h + i] = acc[i];
            }
            __syncthreads();
            const AcmLongRow lr = csr.long_rows[csr.long_index[it.row]];
            const bool multi = lr.windows > 1;                  // a row of several windows: see spmm_narrow_kernel
            finish = multi ? g == 0 : it.slot == lr.slot_begin;
            if (finish && gl < 2) {
                const int pieces = multi ? ACM_WINDOW : lr.slot_end - lr.slot_begin;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float t = 0.f;
                    for (int q = 0; q < pieces; ++q) t += coop[(g + q) * 8 + 4 * h + i];
                    acc[i] = t;
                }
                if (multi) {                                    // [c0 c0 c1 c1] from half 0, [c2 c2] from half 1: slot layout c * 2 + f
                    float* ps = partial + (long)it.slot * (NG * FP) + 4 * h;
                    ps[0] = acc[0], ps[1] = acc[1];
                    if (h == 0) ps[2] = acc[2], ps[3] = acc[3];
                }
            }
            if (multi) finish = false;
            __syncthreads();
        }
        // lane 0 of the group: [c0 | c1] are its own sums, c2 its neighbour's (the other half of the row)
        const float s0 = acm_dpp<0xB1>(acc[0]), s1 = acm_dpp<0xB1>(acc[1]);      // quad_perm [1,0,3,2]
        if (finish) {
            float out[NG][FP] = {{acc[0], acc[1]}, {acc[2], acc[3]}, {s0, s1}};
            LaySerial<FP> lay{gl == 0};
            Epi::template apply<LaySerial<FP>, NG>(ea, it.row, lay, 2, out);
        }
        if (!has_next) break;
        it = itn;
        w = wn;
        k0 = it.begin;
    }
}

// ------------------------------------------------------------------ host-side dispatch
// A run-time size picks a template argument at several places.  Each rounding is written once, as the choice acm_pick takes
// (acm_dispatch.h): the size rounded to its instantiation, with the list of instantiations.
template <int V>
using acm_int = std::integral_constant<int, V>;
// narrow layers (F <= 8): the row padded to FP = 2, 4 or 8 columns
inline auto acm_fp_of(int F) { return acm_one_of<2, 4, 8>(F <= 2 ? 2 : (F <= 4 ? 4 : 8)); }
inline int acm_fp(int F) { return acm_fp_of(F).v; }
// wide layers (8 < F <= 256), lane l owns columns l + 64 r: NREG = 1, 2 or 4 registers per channel
inline auto acm_nreg_of(int F) { return acm_one_of<1, 2, 4>(F <= 64 ? 1 : (F <= 128 ? 2 : 4)); }
// wide layers, vector form: NB = 1 .. 4 blocks of 64 columns
inline auto acm_nb_of(int F) { return acm_one_of<1, 2, 3, 4>(F <= 64 ? 1 : (F <= 128 ? 2 : (F <= 192 ? 3 : 4))); }
// k = 3 channels of the layer, or 4 with the structure channel (k - 1 of them are gathered)
inline auto acm_k_of(int k) { return acm_one_of<3, 4>(k); }
// lanes per work item of the narrow gather (narrow_lanes)
inline auto acm_lanes_of(int lanes) { return acm_one_of<8, 16, 32>(lanes); }

// lanes per work item of the narrow gather: 8 for very sparse graphs, 16 up to an average degree of 160 (a power-law
// graph with mean 82 has median 30: with 32 lanes x 2 neighbours most lanes of most rows idle), 32 beyond
inline int narrow_lanes(int64_t n_rows, int64_t nnz) {
    const double avg = (double)nnz / (double)(n_rows > 0 ? n_rows : 1);
    return avg <= 12.0 ? 8 : (avg <= 160.0 ? 16 : 32);
}
// with 16 lanes per item a workgroup round is one window: the narrow gather finishes the long rows itself
inline bool narrow_finishes_long_rows(const acm_csr* a) { return narrow_lanes(a->n_rows, a->nnz) == ACM_WINDOW; }

// The chooser's figures (tests/launch_forms.py pins them): gathered tables up to GATHER_L2_BYTES count as resident in the L2;
// the vector form needs a mean row length of VEC_MIN_ROW_ONE with one gathered channel, VEC_MIN_ROW_MANY with several.
constexpr size_t GATHER_L2_BYTES = 8u << 20;
constexpr int VEC_MIN_ROW_ONE = 16;
constexpr int VEC_MIN_ROW_MANY = 4;

// Which kernel of the family a gather takes.  The template arguments that depend on F alone (FP, NB, NREG) follow from the
// roundings above at the launch.
struct GatherForm {
    enum Kind { NARROW, PAIR3, VEC16, VEC, PAIR_BF16, PAIR_F32, WIDE } kind;
    int lanes;      // NARROW: lanes per work item (8, 16 or 32)
    int vecmask;    // NARROW: bit c = the rows of channel c take vector fetches
    bool merged;    // NARROW: channels 0 and 1 are one block [c0 | c1], one fetch for both
};

// The choice, from what it reads: the operator's sizes, the gathered tables, form = acm_tuning_t.wide_form and whether the
// epilogue is a fused head (Epi::kFusedHead).  The caller has checked the shape (bf16: even 8 < F <= 64; F <= 256).
inline GatherForm choose_gather_form(int64_t n_rows, int64_t n_cols, int64_t nnz, int64_t n_long, const int32_t* long_index,
                                     const GatherSrc& g, int NG, int F, bool bf16, int form, bool fused_head) {
    GatherForm f = {GatherForm::WIDE, 0, 0, false};
    if (F <= 8) {
        const int FP = acm_fp(F);
        for (int c = 0; c < NG; ++c) {
            const size_t al = (FP == 2) ? 8 : 16;
            // F < FP: a row pitch of at least FP columns lets the fetch read the whole block (what lies beyond F lands in
            // accumulator columns no epilogue looks at); the operand must cover n_cols x ld floats (acm_hip.h)
            const bool ok = (F == FP || g.ld[c] >= FP) && (((uintptr_t)g.p[c]) % al == 0) &&
                            ((g.ld[c] * sizeof(float)) % al == 0);
            f.vecmask |= ok ? (1 << c) : 0;
        }
        f.lanes = narrow_lanes(n_rows, nnz);
        // three gathered channels of two columns each in packed 32-byte rows [c0 c0 c1 c1 | c2 c2 - -]: the pair-lane kernel
        if (NG == 3 && F == 2 && f.lanes == 16 && !bf16 && g.p[1] == g.p[0] + 2 && g.p[2] == g.p[0] + 4 && g.ld[0] == 8 && g.ld[1] == 8 &&
            g.ld[2] == 8 && ((uintptr_t)g.p[0]) % 32 == 0 && (n_long == 0 || long_index != nullptr)) {
            f.kind = GatherForm::PAIR3;
            return f;
        }
        // [channel 0 | channel 1] contiguous and block-aligned => one vector fetch for both
        // (F < FP: the channels are blocks of FP columns, [c0 pad | c1 pad]; what the fetch reads beyond F lands in
        // accumulator columns no epilogue looks at)
        f.merged = NG >= 2 && g.p[1] == g.p[0] + FP && g.ld[0] == g.ld[1] &&
                   ((uintptr_t)g.p[0]) % (8 * FP) == 0 && (g.ld[0] * sizeof(float)) % (8 * FP) == 0;
        f.kind = GatherForm::NARROW;
        return f;
    }
    // fp32 rows of 34..64 columns whose gathered matrices fit the L2 (Squirrel / Chameleon / Cora sizes): 32 lanes x
    // float2 cover a row, so the two half-waves take two neighbours per instruction -- the wide kernel spends one
    // load + one FMA instruction per neighbour on a half-empty wave and is issue-bound there (81 -> 69 us on
    // Squirrel).  On the 168k-node graph the same gather is bound by the Infinity-Cache fills and the pair form is
    // 5-10 % slower, so it is not used.
    bool pair32 = !bf16 && F > 32 && F <= 64 && F % 2 == 0 && (size_t)n_cols * F * NG * sizeof(float) <= GATHER_L2_BYTES;
    for (int c = 0; c < NG && pair32; ++c) pair32 = ((uintptr_t)g.p[c]) % 8 == 0 && g.ld[c] % 2 == 0;
    // vector form: 16-byte aligned rows, 32-bit byte offsets into the gathered tables
    // Measured on the twitch-shaped graph (scripts/probe_wide.py, profiles/r02_probe_wide.txt): rows served by the L2
    // come at 21 TB/s through the vector form against 12 TB/s, rows from the Infinity Cache at 7.5 TB/s through
    // either -- the fabric, not the load instruction, bounds the large-graph gathers.  With a fused head (EpiFwd) the
    // vector layout runs the head four times redundantly, and with two gathered channels its 58 VGPRs cost
    // occupancy, so it is the default for single-channel products (k-hop chains, spmm_sub, the S gather of the
    // aggregate-first structure channel); acm_tuning_t.wide_form = 2 forces it everywhere, 1 nowhere, 3 keeps the pair form.
    // Rows of a few entries (CSR feature matrices: 5-18 per row) never fill the four-neighbour steps: 24 -> 35 us for
    // the Penn94-shaped feature projection, so the vector form also needs a mean row length of 16.
    // (iii) gathered tables that fit the L2 (Squirrel / Chameleon / Cora sizes) take it for any channel count: there
    // the rows arrive at L2 speed and the instruction count is what bounds the kernel (Squirrel with the structure
    // channel: conv_bwd_spmm 57.8 -> 42.6 us, conv_fwd 64.1 -> 57.7, step 0.283 -> 0.265 ms; it replaces the
    // two-neighbours-per-instruction pair form of round 1 on those graphs).
    const bool l2_resident = (size_t)n_cols * F * NG * sizeof(float) <= GATHER_L2_BYTES;
    bool vec = !bf16 && F % 4 == 0 && form != 1 &&
               ((NG == 1 && nnz >= VEC_MIN_ROW_ONE * n_rows) || (l2_resident && NG > 1 && nnz >= VEC_MIN_ROW_MANY * n_rows) || form == 2);
    for (int c = 0; c < NG && vec; ++c)
        vec = ((uintptr_t)g.p[c]) % 16 == 0 && g.ld[c] % 4 == 0 &&
              (uint64_t)n_cols * (uint64_t)g.ld[c] * 4u < (1ull << 32);
    if (vec && form != 3) pair32 = false;
    // bf16 tables (even 8 < F <= 64): the vector form with 8-byte fetches whenever the fp32 operand would take it (rows of
    // 4 k columns, 8-byte aligned); the two-neighbours-per-instruction pair kernel otherwise.  On the twitch-shaped
    // graph the pair kernel is SLOWER than the fp32 vector form (conv_bwd_spmm 619 -> 707 us: half the bytes, but two
    // neighbours per instruction instead of four)
    // ... except under the fused head once the tables outgrow the 256 MB Infinity Cache: every row then comes from
    // HBM, the kernel lives on loads in flight, and the vector layout (the head four times, fewer waves) loses to the
    // pair kernel -- pokec-shaped forward (1.63 M rows, 418 MB of bf16 tables) 5.39 -> 3.89 ms, while the head-less
    // transposed gather of the backward keeps the vector form (2.32 against 2.88 ms): profiles/r04_bench_scale.jsonl
    const bool head_beyond_cache = fused_head && (size_t)n_cols * F * NG * 2u > ((size_t)256 << 20);
    bool vec16 = bf16 && F % 4 == 0 && form != 1 && form != 3 &&
                 ((NG == 1 && nnz >= VEC_MIN_ROW_ONE * n_rows) || (NG > 1 && nnz >= VEC_MIN_ROW_MANY * n_rows && !head_beyond_cache) ||
                  form == 2);
    for (int c = 0; c < NG && vec16; ++c)
        vec16 = ((uintptr_t)g.p[c]) % 8 == 0 && g.ld[c] % 4 == 0 && (uint64_t)n_cols * (uint64_t)g.ld[c] * 2u < (1ull << 32);
    f.kind = vec16 ? GatherForm::VEC16 : (vec && !pair32) ? GatherForm::VEC : bf16 ? GatherForm::PAIR_BF16 : pair32 ? GatherForm::PAIR_F32 : GatherForm::WIDE;
    return f;
}

// Which launch adds the partial sums of the long rows after the main gather.  Sixteen lanes per item: the narrow gather has
// finished the long rows itself, except the rows of several windows (n_multi of them).  n_long, n_multi: the counts of the
// work list the gather walks; n_rows, nnz: the handle's own.
enum GatherFixup { FIXUP_NONE = 0, FIXUP_NARROW = 1, FIXUP_WINDOWS = 2, FIXUP_WIDE = 3 };
inline GatherFixup choose_gather_fixup(int F, int64_t n_rows, int64_t nnz, int64_t n_long, int64_t n_multi) {
    if (F <= 8 && narrow_lanes(n_rows, nnz) == ACM_WINDOW) return n_multi ? FIXUP_WINDOWS : FIXUP_NONE;
    if (!n_long) return FIXUP_NONE;
    return F <= 8 ? FIXUP_NARROW : FIXUP_WIDE;
}

// The template argument that follows from F alone: FP (NARROW, PAIR3), NB (VEC), NREG (WIDE); 1 for the bf16 vector form, 0 for
// the pair kernels, which have none.
inline int gather_form_f_arg(const GatherForm& f, int F) {
    switch (f.kind) {
    case GatherForm::NARROW:
    case GatherForm::PAIR3: return acm_fp(F);
    case GatherForm::VEC: return acm_nb_of(F).v;
    case GatherForm::WIDE: return acm_nreg_of(F).v;
    case GatherForm::VEC16: return 1;
    default: return 0;
    }
}

// An epilogue that declares `static constexpr bool kWideOnly = true` is never launched with F <= 8: launch_gather then does not
// instantiate the narrow gather and its fix-ups for it (the caller answers narrow shapes another way).  Compile-time only:
// epilogues without the member are what they were.
template <class E, class = void> struct epi_wide_only : std::false_type {};
template <class E> struct epi_wide_only<E, std::void_t<decltype(E::kWideOnly)>> : std::bool_constant<E::kWideOnly> {};

// (spmm_narrow_pair3_kernel exists for three gathered channels only; other NG never reach the call)
template <int NG, class Epi>
void launch_pair3(int grid, hipStream_t st, const CsrView& v, const float* table, const typename Epi::Args& ea, float* partial) {
    if constexpr (NG == 3) hipLaunchKernelGGL((spmm_narrow_pair3_kernel<Epi>), dim3(grid), dim3(256), 0, st, v, table, ea, partial);
}

// after a narrow gather with sixteen lanes per item: the rows of several windows (none on most operators)
template <int NG, class Epi>
int finish_window_rows(const acm_csr* a, const CsrView& v, int F, const typename Epi::Args& ea, const float* partial, hipStream_t st) {
    if (v.n_multi == 0) return ACM_OK;            // (the view's own counts: the handle's, or an override's)
    const int grid = (int)((v.n_long + 15) / 16);
    acm_pick([&](auto fp) {
        hipLaunchKernelGGL((spmm_fixup_windows_kernel<fp(), NG, Epi>), dim3(grid), dim3(256), 0, st, v, F, ea, partial);
        return ACM_OK;
    }, acm_fp_of(F));
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

// `over` (NULL: the handle's own): the work list the gather walks in place of the handle's -- a loss-row attachment's.  The FORM
// is still chosen from the handle's own sizes (narrow_lanes of its n_rows and nnz), so a sub-list runs the very kernel the full
// list runs.
template <int NG, class Epi>
int launch_gather(const acm_csr* a, const GatherSrc& g, int F, const typename Epi::Args& ea,
                  void* workspace, size_t ws_bytes, hipStream_t st, const char* who,
                  const float* vals_override = nullptr, bool bf16 = false, bool defer_fixup = false,
                  const GatherOverride* over = nullptr) {
    const int64_t n_slots = over ? over->n_slots : a->n_slots;
    const size_t need = (size_t)n_slots * (size_t)(NG * F) * sizeof(float);
    ACM_REQUIRE(ws_bytes >= need && (need == 0 || workspace), ACM_ENOMEM,
                "%s: workspace %zu B < required %zu B", who, ws_bytes, need);
    float* partial = (float*)workspace;
    CsrView v = over ? over->view : acm_view(a);
    if (vals_override) v.vals = vals_override;
    const int64_t n_items = v.n_items, n_long = v.n_long;
    if (n_items == 0) return ACM_OK;
    ACM_REQUIRE(!bf16 || (F > 8 && F <= 64 && F % 2 == 0), ACM_EUNSUPPORTED,
                "%s: bf16 gathered operands are implemented for even 8 < F <= 64", who);
    if (bf16) {
        bool aligned = true;
        for (int c = 0; c < NG; ++c) aligned = aligned && ((uintptr_t)g.p[c]) % 4 == 0 && g.ld[c] % 2 == 0;
        ACM_REQUIRE(aligned, ACM_EINVAL, "%s: bf16 operands must be 4-byte aligned with an even leading dimension", who);
    }
    ACM_REQUIRE(F <= 256, ACM_EUNSUPPORTED, "%s: F = %d > 256 columns per channel", who, F);
    const GatherForm form = choose_gather_form(a->n_rows, a->n_cols, a->nnz, a->n_long, a->long_index, g, NG, F, bf16,
                                               acm_tuning().wide_form, Epi::kFusedHead);
    // the forms for F > 8: a wave per work item, the same arguments
    auto wide = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3((int)((n_items + 3) / 4)), dim3(256), 0, st, v, g, F, ea, partial); };
    if constexpr (epi_wide_only<Epi>::value)
        ACM_REQUIRE(F > 8, ACM_EUNSUPPORTED, "%s: this epilogue exists for more than 8 columns (got %d)", who, F);
    int rc = ACM_OK;
    switch (form.kind) {
    case GatherForm::PAIR3: {
      if constexpr (!epi_wide_only<Epi>::value) {
        int grid = (int)((n_items + 15) / 16);
        if (grid > NARROW_MAX_BLOCKS) grid = NARROW_MAX_BLOCKS;
        launch_pair3<NG, Epi>(grid, st, v, g.p[0], ea, partial);
      }
      break;
    }
    case GatherForm::NARROW:
      if constexpr (!epi_wide_only<Epi>::value)
        rc = acm_pick([&](auto fp, auto gs) {
            constexpr int FP = decltype(fp)::value, GS = decltype(gs)::value, gpb = 256 / GS;
            int grid = (int)((n_items + gpb - 1) / gpb);
            if (grid > NARROW_MAX_BLOCKS) grid = NARROW_MAX_BLOCKS;
            if (form.merged)
                hipLaunchKernelGGL((spmm_narrow_kernel<FP, NG, GS, (NG >= 2), Epi>), dim3(grid), dim3(256), 0, st, v, g, F,
                                   form.vecmask, ea, partial);
            else
                hipLaunchKernelGGL((spmm_narrow_kernel<FP, NG, GS, false, Epi>), dim3(grid), dim3(256), 0, st, v, g, F,
                                   form.vecmask, ea, partial);
            return ACM_OK;
        }, acm_fp_of(F), acm_lanes_of(form.lanes));
        break;
    case GatherForm::VEC16: wide(spmm_vec_kernel<NG, 1, Epi, true>); break;
    case GatherForm::VEC: acm_pick([&](auto nb) { wide(spmm_vec_kernel<NG, nb(), Epi>); return ACM_OK; }, acm_nb_of(F)); break;
    case GatherForm::PAIR_BF16: wide(spmm_pair_kernel<NG, Epi, true>); break;
    case GatherForm::PAIR_F32: wide(spmm_pair_kernel<NG, Epi, false>); break;
    case GatherForm::WIDE: acm_pick([&](auto nreg) { wide(spmm_wide_kernel<nreg(), NG, Epi>); return ACM_OK; }, acm_nreg_of(F)); break;
    }
    ACM_REQUIRE(rc == ACM_OK, ACM_EUNSUPPORTED, "%s: no narrow gather for %d lanes per item", who, form.lanes);
    ACM_CHECK_HIP(hipGetLastError());
    const GatherFixup fix = choose_gather_fixup(F, a->n_rows, a->nnz, n_long, v.n_multi);
    if (fix == FIXUP_WINDOWS) {
        if constexpr (!epi_wide_only<Epi>::value) return finish_window_rows<NG, Epi>(a, v, F, ea, partial, st);
        return ACM_OK;
    }
    if (defer_fixup || fix == FIXUP_NONE) return ACM_OK;      // (deferred: the caller's next kernel adds the partial slots of the long rows)
    if (fix == FIXUP_NARROW) {
      if constexpr (!epi_wide_only<Epi>::value)
        acm_pick([&](auto fp) {
            hipLaunchKernelGGL((spmm_fixup_narrow_kernel<fp(), NG, Epi>), dim3((int)((n_long + 15) / 16)), dim3(256), 0, st, v, F, ea,
                               partial);
            return ACM_OK;
        }, acm_fp_of(F));
    } else {
        acm_pick([&](auto nreg) {
            hipLaunchKernelGGL((spmm_fixup_kernel<nreg(), NG, Epi>), dim3((int)((n_long + 3) / 4)), dim3(256), 0, st, v, F, ea, partial);
            return ACM_OK;
        }, acm_nreg_of(F));
    }
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}
