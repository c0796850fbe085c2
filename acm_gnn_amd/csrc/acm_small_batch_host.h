// The part of acm_small_batch_bind's validation that needs neither a device nor an operator handle: the slot count, the
// fields every slot of a batch must share (they choose the kernel templates and the grids, which are per LAUNCH, not per
// slot) and the ranges no two runs may share (each run's workspace, logits and loss are written by its own grid row).
// Plain host C++ over include/acm_hip.h, so a stand-alone program can drive it under the host sanitizers
// (tests/c_abi/small_batch_host.cpp, tests/c_abi/small_graphs_host.cpp); csrc/acm_small.hip calls the same functions.
#ifndef ACM_SMALL_BATCH_HOST_H
#define ACM_SMALL_BATCH_HOST_H
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "acm_hip.h"

// The hidden width a block asks for: acm_small_step_t::hidden, where 0 (a caller from before the field had a meaning) is 64.
inline int acm_small_hidden_of(const acm_small_step_t* p) { return p->hidden == 0 ? 64 : (int)p->hidden; }
// the widths the kernels are instantiated for
inline bool acm_small_hidden_ok(int32_t hidden) { return hidden == 0 || hidden == 32 || hidden == 64; }

// [a, a + alen) and [b, b + blen) share a byte (no sum of an address and a length is formed: a range may end at the top of
// the address space)
inline bool acm_ranges_overlap(uintptr_t a, size_t alen, uintptr_t b, size_t blen) {
    if (alen == 0 || blen == 0) return false;
    return a < b ? (size_t)(b - a) < alen : (size_t)(a - b) < blen;
}

// ACM_OK, or the status of the first objection with its text in msg.  One implementation for the two flavours of a batch:
//   slot_rows == NULL  every slot on ONE graph of n_rows rows (acm_small_batch_bind): the feature values, their transposed
//                      copy and order, and the row scale are shared too;
//   slot_rows != NULL  a graph PER SLOT (acm_small_batch_bind_graphs; synthetic-experiments/train.py:64-164): slot_rows[i] is
//                      the row count of slot i's operator, which must agree across the active slots (the metrics launch
//                      behind the step shares it); the four feature / operator pointers may differ.
// The logits of a slot are rows x n_classes floats; a row count <= 0 counts as one row.
inline int acm_small_batch_check_slots_impl(int n_slots, const acm_small_step_t* const* slots, int64_t n_rows, const int64_t* slot_rows,
                                            char* msg, size_t msg_len) {
    if (n_slots < 1) {
        snprintf(msg, msg_len, "acm_small_batch: n_slots must be 1 .. %d (got %d)", ACM_SMALL_BATCH_MAX, n_slots);
        return ACM_EINVAL;
    }
    if (n_slots > ACM_SMALL_BATCH_MAX) {
        snprintf(msg, msg_len, "acm_small_batch: n_slots %d > %d slots of one table", n_slots, ACM_SMALL_BATCH_MAX);
        return ACM_EUNSUPPORTED;
    }
    if (!slots) {
        snprintf(msg, msg_len, "acm_small_batch: NULL slots array");
        return ACM_EINVAL;
    }
    int first = -1;
    for (int i = 0; i < n_slots; ++i)
        if (slots[i]) {
            first = i;
            break;
        }
    if (first < 0) {
        snprintf(msg, msg_len, "acm_small_batch: every slot is empty");
        return ACM_EINVAL;
    }
    // the batched kernels have no residual form (ACM-GCN++ runs as single steps): refused here, before any launch
    for (int i = first; i < n_slots; ++i)
        if (slots[i] && slots[i]->residual != 0) {
            snprintf(msg, msg_len, "acm_small_batch: slot %d has the residual branch set (residual = %d): residual plans run as single steps only",
                     i, (int)slots[i]->residual);
            return ACM_EUNSUPPORTED;
        }
    const acm_small_step_t* s = slots[first];
    for (int i = first + 1; i < n_slots; ++i) {
        const acm_small_step_t* p = slots[i];
        if (!p) continue;
        const char* what = nullptr;
        if (p->n_classes != s->n_classes) what = "n_classes";
        else if (p->n_channels != s->n_channels) what = "n_channels";
        else if (p->relu_before != s->relu_before) what = "relu_before";
        else if (p->layernorm != s->layernorm) what = "layernorm";
        else if (p->train != s->train) what = "train";
        else if (p->update != s->update) what = "update";
        else if (p->f_in != s->f_in) what = "f_in";
        else if (acm_small_hidden_of(p) != acm_small_hidden_of(s)) what = "hidden";
        else if (slot_rows) {
            if (slot_rows[i] != slot_rows[first]) what = "n_rows";
        } else if (p->x_vals != s->x_vals) what = "x_vals";
        else if (p->xt_vals != s->xt_vals) what = "xt_vals";
        else if (p->xt_src_pos != s->xt_src_pos) what = "xt_src_pos";
        else if (p->row_scale != s->row_scale) what = "row_scale";
        if (what) {
            snprintf(msg, msg_len, "acm_small_batch: slots %d and %d disagree in %s (shared by every slot of a batch)", first, i, what);
            return ACM_EINVAL;
        }
    }
    if (slot_rows) n_rows = slot_rows[first];           // (equal in every active slot by now)
    const size_t rows = n_rows > 0 ? (size_t)n_rows : 1;
    static const char* const kind[3] = {"workspace", "logits", "loss"};
    for (int i = first; i < n_slots; ++i) {
        if (!slots[i]) continue;
        const acm_small_step_t* p = slots[i];
        const uintptr_t pa[3] = {(uintptr_t)p->workspace, (uintptr_t)p->logits, (uintptr_t)p->loss};
        const size_t pl[3] = {p->workspace ? p->workspace_bytes : 0, p->logits ? rows * (size_t)(p->n_classes > 0 ? p->n_classes : 1) * sizeof(float) : 0,
                              p->loss ? sizeof(float) : 0};
        for (int j = i + 1; j < n_slots; ++j) {
            if (!slots[j]) continue;
            const acm_small_step_t* q = slots[j];
            const uintptr_t qa[3] = {(uintptr_t)q->workspace, (uintptr_t)q->logits, (uintptr_t)q->loss};
            const size_t ql[3] = {q->workspace ? q->workspace_bytes : 0, q->logits ? rows * (size_t)(q->n_classes > 0 ? q->n_classes : 1) * sizeof(float) : 0,
                                  q->loss ? sizeof(float) : 0};
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b)
                    if (acm_ranges_overlap(pa[a], pl[a], qa[b], ql[b])) {
                        snprintf(msg, msg_len, "acm_small_batch: the %s of slot %d and the %s of slot %d overlap (every run needs its own)",
                                 kind[a], i, kind[b], j);
                        return ACM_EINVAL;
                    }
        }
    }
    return ACM_OK;
}

// every slot on one graph of n_rows rows
inline int acm_small_batch_check_slots(int n_slots, const acm_small_step_t* const* slots, int64_t n_rows, char* msg, size_t msg_len) {
    return acm_small_batch_check_slots_impl(n_slots, slots, n_rows, nullptr, msg, msg_len);
}

// a graph per slot: slot_rows is a host array of n_slots row counts (entries of empty slots are not read)
inline int acm_small_batch_check_slots_graphs(int n_slots, const acm_small_step_t* const* slots, const int64_t* slot_rows, char* msg,
                                              size_t msg_len) {
    if (!slot_rows) {
        snprintf(msg, msg_len, "acm_small_batch: NULL row-count array");
        return ACM_EINVAL;
    }
    return acm_small_batch_check_slots_impl(n_slots, slots, 0, slot_rows, msg, msg_len);
}

#endif  // ACM_SMALL_BATCH_HOST_H
