// The host-side part of acm_small_batch_bind_graphs's validation (csrc/acm_small_batch_host.h, the graph-per-slot flavour:
// slot count, the fields every slot still shares, one row count, overlapping ranges) driven with crafted slot arrays -- a
// stand-alone program, built with the host sanitizers by tests/test_small_graphs_cpu.py and run on the CPU.  No device, no
// library: the header is plain host C++.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "acm_small_batch_host.h"

static int failures = 0;
#define EXPECT(cond)                                                     \
    do {                                                                 \
        if (!(cond)) {                                                   \
            printf("FAILED line %d: %s [%s]\n", __LINE__, #cond, msg);   \
            ++failures;                                                  \
        }                                                                \
    } while (0)

// slot k of a batch on different graphs: its own feature values, transposed copy, order and row scale
static acm_small_step_t block(int k, uintptr_t base, size_t ws_bytes, int classes) {
    acm_small_step_t p;
    memset(&p, 0, sizeof(p));
    p.n_classes = classes, p.n_channels = 3, p.train = 1, p.update = 1, p.f_in = 7;
    p.x_vals = (const float*)(uintptr_t)(0x100 + 0x1000 * k), p.row_scale = (const float*)(uintptr_t)(0x200 + 0x1000 * k);
    p.xt_vals = (const float*)(uintptr_t)(0x300 + 0x1000 * k), p.xt_src_pos = (const int32_t*)(uintptr_t)(0x400 + 0x1000 * k);
    p.workspace = (void*)base, p.workspace_bytes = ws_bytes;
    p.logits = (float*)(base + ws_bytes), p.loss = (float*)(base + ws_bytes + 4096);
    return p;
}

int main() {
    char msg[256] = "";
    const int B = ACM_SMALL_BATCH_MAX;
    std::vector<acm_small_step_t> blocks;
    std::vector<const acm_small_step_t*> slots;
    std::vector<int64_t> rows((size_t)B, 100);
    for (int i = 0; i < B; ++i) blocks.push_back(block(i, 0x10000000u + (uintptr_t)i * 0x10000, 4096, 3));
    for (auto& b : blocks) slots.push_back(&b);
    // the maximum count, every slot on its own features and row scale: accepted here, refused by the one-graph check
    EXPECT(acm_small_batch_check_slots_graphs(B, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_OK);
    EXPECT(acm_small_batch_check_slots(B, slots.data(), 100, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "x_vals"));
    // each of the four per-graph pointers alone
    {
        acm_small_step_t a = block(0, 0x40000000u, 4096, 3), b = block(0, 0x40010000u, 4096, 3);
        const acm_small_step_t* two[2] = {&a, &b};
        const int64_t r2[2] = {100, 100};
        EXPECT(acm_small_batch_check_slots(2, two, 100, msg, sizeof(msg)) == ACM_OK);
        b.row_scale = (const float*)0x208;
        EXPECT(acm_small_batch_check_slots(2, two, 100, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "row_scale"));
        EXPECT(acm_small_batch_check_slots_graphs(2, two, r2, msg, sizeof(msg)) == ACM_OK);
        b = block(0, 0x40010000u, 4096, 3), b.xt_vals = (const float*)0x308;
        EXPECT(acm_small_batch_check_slots(2, two, 100, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "xt_vals"));
        EXPECT(acm_small_batch_check_slots_graphs(2, two, r2, msg, sizeof(msg)) == ACM_OK);
        b = block(0, 0x40010000u, 4096, 3), b.xt_src_pos = (const int32_t*)0x408;
        EXPECT(acm_small_batch_check_slots(2, two, 100, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "xt_src_pos"));
        EXPECT(acm_small_batch_check_slots_graphs(2, two, r2, msg, sizeof(msg)) == ACM_OK);
    }
    // counts and NULL arrays
    EXPECT(acm_small_batch_check_slots_graphs(0, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "n_slots"));
    EXPECT(acm_small_batch_check_slots_graphs(-3, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_EINVAL);
    EXPECT(acm_small_batch_check_slots_graphs(B + 1, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_EUNSUPPORTED && strstr(msg, "33"));
    EXPECT(acm_small_batch_check_slots_graphs(4, nullptr, rows.data(), msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "NULL"));
    EXPECT(acm_small_batch_check_slots_graphs(4, slots.data(), nullptr, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "NULL"));
    // empty slots: all of them; all but the last (the row counts of empty slots are not compared); every other one
    std::vector<const acm_small_step_t*> holes((size_t)B, nullptr);
    std::vector<int64_t> hole_rows((size_t)B, -7);
    EXPECT(acm_small_batch_check_slots_graphs(B, holes.data(), hole_rows.data(), msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "empty"));
    holes[(size_t)B - 1] = &blocks[5], hole_rows[(size_t)B - 1] = 100;
    EXPECT(acm_small_batch_check_slots_graphs(B, holes.data(), hole_rows.data(), msg, sizeof(msg)) == ACM_OK);
    for (int i = 1; i < B; i += 2) holes[(size_t)i] = &blocks[(size_t)i], hole_rows[(size_t)i] = 100;
    EXPECT(acm_small_batch_check_slots_graphs(B, holes.data(), hole_rows.data(), msg, sizeof(msg)) == ACM_OK);
    EXPECT(acm_small_batch_check_slots_graphs(1, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_OK);
    // the fields every slot still shares
    acm_small_step_t odd = blocks[7];
    slots[7] = &odd;
    odd.n_classes = 4;
    EXPECT(acm_small_batch_check_slots_graphs(B, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "n_classes") && strstr(msg, "7"));
    odd = blocks[7], odd.n_channels = 4;
    EXPECT(acm_small_batch_check_slots_graphs(B, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "n_channels"));
    odd = blocks[7], odd.relu_before = 1;
    EXPECT(acm_small_batch_check_slots_graphs(B, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "relu_before"));
    odd = blocks[7], odd.layernorm = 1;
    EXPECT(acm_small_batch_check_slots_graphs(B, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "layernorm"));
    odd = blocks[7], odd.train = 0;
    EXPECT(acm_small_batch_check_slots_graphs(B, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "train"));
    odd = blocks[7], odd.update = 0;
    EXPECT(acm_small_batch_check_slots_graphs(B, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "update"));
    odd = blocks[7], odd.f_in = 8;
    EXPECT(acm_small_batch_check_slots_graphs(B, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "f_in"));
    odd = blocks[7], odd.hidden = 32;                       // (0 means 64)
    EXPECT(acm_small_batch_check_slots_graphs(B, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "hidden"));
    odd = blocks[7], odd.hidden = 64;
    EXPECT(acm_small_batch_check_slots_graphs(B, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_OK);
    slots[7] = &blocks[7];
    // one row count: the last slot one row short
    rows[(size_t)B - 1] = 99;
    EXPECT(acm_small_batch_check_slots_graphs(B, slots.data(), rows.data(), msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "n_rows") && strstr(msg, "31"));
    rows[(size_t)B - 1] = 100;
    // overlaps are found with the slots' row count: logits of 100 x 3 floats reach into the next slot's workspace, those of
    // 10 rows do not
    acm_small_step_t lo = block(0, 0x20000000u, 4096, 3), hi = block(1, 0x20000000u + 4095, 4096, 3);
    const acm_small_step_t* two[4] = {&lo, nullptr, nullptr, &hi};
    int64_t r4[4] = {100, 0, 0, 100};
    EXPECT(acm_small_batch_check_slots_graphs(4, two, r4, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "overlap") && strstr(msg, "workspace"));
    hi = block(1, 0x20010000u, 4096, 3);
    lo.logits = (float*)(0x20010000u - 400), lo.loss = (float*)0x30100000u;
    EXPECT(acm_small_batch_check_slots_graphs(4, two, r4, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "logits"));
    r4[0] = r4[3] = 10;
    EXPECT(acm_small_batch_check_slots_graphs(4, two, r4, msg, sizeof(msg)) == ACM_OK);
    // ranges at both ends of the address space
    acm_small_step_t top = block(0, 0x50000000u, 4096, 3), bottom = block(1, 0x60000000u, 4096, 3);
    top.workspace = (void*)(UINTPTR_MAX - 4095), top.workspace_bytes = 4096;
    bottom.workspace = (void*)(uintptr_t)1, bottom.workspace_bytes = 64;
    const acm_small_step_t* ends[2] = {&top, &bottom};
    const int64_t r2[2] = {100, 100};
    EXPECT(acm_small_batch_check_slots_graphs(2, ends, r2, msg, sizeof(msg)) == ACM_OK);
    bottom.workspace = (void*)(UINTPTR_MAX - 7), bottom.workspace_bytes = 8;
    EXPECT(acm_small_batch_check_slots_graphs(2, ends, r2, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "overlap"));
    bottom = block(1, 0x60000000u, 4096, 3), bottom.loss = top.loss;
    EXPECT(acm_small_batch_check_slots_graphs(2, ends, r2, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "loss"));
    if (failures) return 1;
    printf("small_graphs_host: ok\n");
    return 0;
}
