// Model selection and early stopping on the device (gfx950): the bookkeeping train.fit does on the host after every epoch --
// append the history row, compare against the best key, test the early-stopping window -- as one tiny launch at the tail of
// the evaluation pass (acm_select_step), and the snapshot of the selected parameters as a copy predicated on that launch's
// verdict (acm_copy_if).  Both read nothing from host memory at run time, so both can be captured.
//
// acm_select_step is ONE 64-lane block.  Its values must equal the host loop's bit for bit: fp32 inputs are widened to double
// (what float() / tolist() give), comparisons are IEEE comparisons (a NaN never wins and never stops), and the window sum is
// formed in float64 by ONE lane in ascending epoch order, so it does not depend on the launch shape.  The other lanes only
// fetch the window, 64 values at a time, into LDS.  The sum is the plain one, a rounding per addition: Python's sum() of floats
// up to CPython 3.11; the compensated sum() of 3.12 and later can differ from it in the last bit.
#include "acm_common.h"

namespace {

constexpr int CTRL_EPOCH = 0, CTRL_STOPPED = 1, CTRL_BEST_EPOCH = 2, CTRL_IMPROVED = 3;

struct SelectArgs {
    int rule, early_stopping, epochs;
    const float* result;
    const double* result_f64;
    const float* train_loss;
    int32_t* ctrl;
    double* best;
    double* history;
};

__device__ __forceinline__ void select_step_body(const SelectArgs& a) {
    __shared__ double win[64];
    const int lane = threadIdx.x;
    const int epoch = a.ctrl[CTRL_EPOCH];              // block-uniform
    if (a.ctrl[CTRL_STOPPED] != 0 || epoch < 0 || epoch >= a.epochs) {
        if (lane == 0) a.ctrl[CTRL_IMPROVED] = 0;
        return;
    }
    double m_tr, m_va, m_te, val_loss;
    if (a.result_f64) {
        m_tr = a.result_f64[0], m_va = a.result_f64[1], m_te = a.result_f64[2], val_loss = a.result_f64[3];
    } else {
        m_tr = (double)a.result[0], m_va = (double)a.result[1], m_te = (double)a.result[2], val_loss = (double)a.result[3];
    }
    // the window: rows epoch - es .. epoch - 1 (written by earlier launches), summed by lane 0 in epoch order
    const int es = a.early_stopping;
    const bool windowed = a.rule == 1 && es > 0 && epoch > es;
    double sum = 0.0;
    if (windowed) {
        const int first = epoch - es;
        for (int base = 0; base < es; base += 64) {
            const int cnt = es - base < 64 ? es - base : 64;
            if (lane < cnt) win[lane] = a.history[(long)(first + base + lane) * 5 + 4];
            __syncthreads();
            if (lane == 0)
                for (int i = 0; i < cnt; ++i) sum += win[i];
            __syncthreads();
        }
    }
    if (lane != 0) return;
    double* row = a.history + (long)epoch * 5;
    row[0] = (double)a.train_loss[0];
    row[1] = m_tr, row[2] = m_va, row[3] = m_te, row[4] = val_loss;
    const double key = a.rule == 0 ? m_va : -val_loss;
    int improved = 0;
    if (key == key && (a.ctrl[CTRL_BEST_EPOCH] < 0 || key > a.best[0])) {
        a.best[0] = key;
        a.best[1] = m_te;
        a.ctrl[CTRL_BEST_EPOCH] = epoch;
        improved = 1;
    }
    a.ctrl[CTRL_IMPROVED] = improved;
    if (windowed && val_loss > sum / (double)es) a.ctrl[CTRL_STOPPED] = 1;
    a.ctrl[CTRL_EPOCH] = epoch + 1;
}

__global__ __launch_bounds__(64) void select_step_kernel(SelectArgs a) { select_step_body(a); }

// One block per slot on its own argument block of a device table (read through the constant address space: the block index is
// uniform, the fields arrive by scalar loads like kernel arguments).  Both result pointers NULL: an empty slot.
__global__ __launch_bounds__(64) void select_step_batch_kernel(const acm_select_t* table) {
    const __attribute__((address_space(4))) acm_select_t* p = (const __attribute__((address_space(4))) acm_select_t*)table + blockIdx.x;
    if (!p->result && !p->result_f64) return;
    const SelectArgs a{p->rule, p->early_stopping, p->epochs, p->result, p->result_f64, p->train_loss, p->ctrl, p->best, p->history};
    select_step_body(a);
}

// ---------------------------------------------------------------------------------------------- acm_copy_if
constexpr int PACK = 40;          // tensors per launch (acm_adam_step's pack)
constexpr int CHUNK = 2048;       // elements per block and round
constexpr int MAX_BLOCKS = 1024;  // per tensor: a large tensor's blocks take several rounds each

inline int copy_rounds(long n) {
    const long r = (n + (long)CHUNK * MAX_BLOCKS - 1) / ((long)CHUNK * MAX_BLOCKS);
    return r > 1 ? (int)r : 1;
}
inline int copy_blocks(long n) { return (int)((n + (long)CHUNK * copy_rounds(n) - 1) / ((long)CHUNK * copy_rounds(n))); }

struct CopyPack {
    const uint32_t* src[PACK];
    uint32_t* dst[PACK];
    long numel[PACK];
    int rounds[PACK];
    int first_block[PACK + 1];
    int n;
};
static_assert(sizeof(CopyPack) + 16 <= 4096, "kernel arguments: 4 KB");

// Block b copies rounds of CHUNK consecutive 32-bit words of one tensor -- as bits: the element type never enters.
__global__ __launch_bounds__(256) void copy_if_kernel(CopyPack pk, const int32_t* __restrict__ flag) {
    if (flag[0] == 0) return;                                        // block-uniform, before the first load of a tensor
    const int blk = blockIdx.x;
    int t = 0;
    while (t + 1 < pk.n && blk >= pk.first_block[t + 1]) ++t;        // uniform (an empty tensor owns no block: >=)
    const uint32_t* __restrict__ src = pk.src[t];
    uint32_t* __restrict__ dst = pk.dst[t];
    const long n = pk.numel[t];
    const int rounds = pk.rounds[t];
    const bool aligned = ((((uintptr_t)src | (uintptr_t)dst) & 15) == 0);
    for (int rd = 0; rd < rounds; ++rd) {
        const long base = ((long)(blk - pk.first_block[t]) * rounds + rd) * CHUNK;
        if (base >= n) break;
        const long end = base + CHUNK < n ? base + CHUNK : n;
        if (aligned && end - base == CHUNK) {
#pragma unroll
            for (int r = 0; r < CHUNK / 1024; ++r) {
                const long i = base + r * 1024 + threadIdx.x * 4;
                *reinterpret_cast<uint4*>(dst + i) = *reinterpret_cast<const uint4*>(src + i);
            }
        } else {
            for (long i = base + threadIdx.x; i < end; i += 256) dst[i] = src[i];
        }
    }
}

}  // namespace

extern "C" int acm_select_step(const acm_select_t* p, acm_stream_t stream) {
    ACM_REQUIRE(p, ACM_EINVAL, "acm_select_step: NULL parameter block");
    ACM_REQUIRE(p->rule == 0 || p->rule == 1, ACM_EINVAL, "acm_select_step: rule must be 0 (max metric) or 1 (min loss), not %d",
                (int)p->rule);
    ACM_REQUIRE(p->epochs >= 1, ACM_EINVAL, "acm_select_step: epochs must be >= 1");
    ACM_REQUIRE(p->early_stopping >= 0, ACM_EINVAL, "acm_select_step: early_stopping must be >= 0");
    ACM_REQUIRE((p->result != nullptr) != (p->result_f64 != nullptr), ACM_EINVAL,
                "acm_select_step: exactly one of result / result_f64");
    ACM_REQUIRE(p->train_loss && p->ctrl && p->best && p->history, ACM_EINVAL, "acm_select_step: NULL pointer");
    SelectArgs a{p->rule, p->early_stopping, p->epochs, p->result, p->result_f64, p->train_loss, p->ctrl, p->best, p->history};
    hipLaunchKernelGGL(select_step_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, a);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_select_step_batch(int32_t n_slots, const acm_select_t* table, acm_stream_t stream) {
    ACM_REQUIRE(table, ACM_EINVAL, "acm_select_step_batch: NULL table");
    ACM_REQUIRE(n_slots >= 1, ACM_EINVAL, "acm_select_step_batch: n_slots must be 1 .. %d (got %d)", ACM_SMALL_BATCH_MAX, (int)n_slots);
    ACM_REQUIRE(n_slots <= ACM_SMALL_BATCH_MAX, ACM_EUNSUPPORTED, "acm_select_step_batch: n_slots %d > %d", (int)n_slots, ACM_SMALL_BATCH_MAX);
    hipLaunchKernelGGL(select_step_batch_kernel, dim3(n_slots), dim3(64), 0, (hipStream_t)stream, table);
    ACM_CHECK_HIP(hipGetLastError());
    return ACM_OK;
}

extern "C" int acm_copy_if(int32_t n_tensors, const acm_copy_tensor_t* tensors, const int32_t* flag, acm_stream_t stream) {
    ACM_REQUIRE(n_tensors >= 0, ACM_EINVAL, "acm_copy_if: n_tensors < 0");
    ACM_REQUIRE(n_tensors == 0 || tensors, ACM_EINVAL, "acm_copy_if: NULL table");
    ACM_REQUIRE(flag, ACM_EINVAL, "acm_copy_if: NULL flag");
    for (int i = 0; i < n_tensors; ++i) {                      // the whole table before the first launch
        const acm_copy_tensor_t& t = tensors[i];
        ACM_REQUIRE(t.numel >= 0, ACM_EINVAL, "acm_copy_if: tensor %d has numel < 0", i);
        ACM_REQUIRE(t.numel == 0 || (t.src && t.dst), ACM_EINVAL, "acm_copy_if: tensor %d has a NULL pointer", i);
        ACM_REQUIRE((((uintptr_t)t.src | (uintptr_t)t.dst) & 3) == 0, ACM_EINVAL, "acm_copy_if: tensor %d is not 4-byte aligned", i);
        ACM_REQUIRE(t.numel < ((int64_t)1 << 40), ACM_EUNSUPPORTED, "acm_copy_if: tensor %d too large", i);
    }
    for (int first = 0; first < n_tensors; first += PACK) {
        CopyPack pk{};
        int blocks = 0;
        pk.n = n_tensors - first < PACK ? n_tensors - first : PACK;
        for (int i = 0; i < pk.n; ++i) {
            const acm_copy_tensor_t& t = tensors[first + i];
            pk.src[i] = (const uint32_t*)t.src, pk.dst[i] = (uint32_t*)t.dst;
            pk.numel[i] = (long)t.numel;
            pk.rounds[i] = copy_rounds((long)t.numel);
            pk.first_block[i] = blocks;
            blocks += t.numel > 0 ? copy_blocks((long)t.numel) : 0;
        }
        pk.first_block[pk.n] = blocks;
        if (blocks == 0) continue;
        hipLaunchKernelGGL(copy_if_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, pk, flag);
        ACM_CHECK_HIP(hipGetLastError());
    }
    return ACM_OK;
}
