// The host-side part of acm_small_batch_bind's validation (csrc/acm_small_batch_host.h: slot count, shared fields, overlapping
// ranges) driven with crafted slot arrays -- a stand-alone program, built with the host sanitizers by
// tests/test_small_batch_cpu.py and run on the CPU.  No device, no library: the header is plain host C++.
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

static acm_small_step_t block(uintptr_t base, size_t ws_bytes, int classes) {
    acm_small_step_t p;
    memset(&p, 0, sizeof(p));
    p.n_classes = classes, p.n_channels = 3, p.train = 1, p.update = 1, p.f_in = 7;
    p.x_vals = (const float*)0x100, p.row_scale = (const float*)0x200;
    p.workspace = (void*)base, p.workspace_bytes = ws_bytes;
    p.logits = (float*)(base + ws_bytes), p.loss = (float*)(base + ws_bytes + 4096);
    return p;
}

int main() {
    char msg[256] = "";
    const int64_t rows = 100;
    // the maximum count, every slot active, ranges back to back: accepted
    std::vector<acm_small_step_t> blocks;
    std::vector<const acm_small_step_t*> slots;
    for (int i = 0; i < ACM_SMALL_BATCH_MAX; ++i) blocks.push_back(block(0x10000000u + (uintptr_t)i * 0x10000, 4096, 3));
    for (auto& b : blocks) slots.push_back(&b);
    EXPECT(acm_small_batch_check_slots(ACM_SMALL_BATCH_MAX, slots.data(), rows, msg, sizeof(msg)) == ACM_OK);
    // counts
    EXPECT(acm_small_batch_check_slots(0, slots.data(), rows, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "n_slots"));
    EXPECT(acm_small_batch_check_slots(-3, slots.data(), rows, msg, sizeof(msg)) == ACM_EINVAL);
    slots.push_back(&blocks[0]);
    EXPECT(acm_small_batch_check_slots(ACM_SMALL_BATCH_MAX + 1, slots.data(), rows, msg, sizeof(msg)) == ACM_EUNSUPPORTED && strstr(msg, "33"));
    slots.pop_back();
    EXPECT(acm_small_batch_check_slots(4, nullptr, rows, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "NULL"));
    // empty slots: all of them; all but the last; the first and every other one
    std::vector<const acm_small_step_t*> holes(ACM_SMALL_BATCH_MAX, nullptr);
    EXPECT(acm_small_batch_check_slots(ACM_SMALL_BATCH_MAX, holes.data(), rows, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "empty"));
    holes[ACM_SMALL_BATCH_MAX - 1] = &blocks[5];
    EXPECT(acm_small_batch_check_slots(ACM_SMALL_BATCH_MAX, holes.data(), rows, msg, sizeof(msg)) == ACM_OK);
    for (int i = 1; i < ACM_SMALL_BATCH_MAX; i += 2) holes[i] = &blocks[i];
    EXPECT(acm_small_batch_check_slots(ACM_SMALL_BATCH_MAX, holes.data(), rows, msg, sizeof(msg)) == ACM_OK);
    EXPECT(acm_small_batch_check_slots(1, slots.data(), rows, msg, sizeof(msg)) == ACM_OK);
    // shared fields
    acm_small_step_t odd = blocks[7];
    odd.n_classes = 4;
    slots[7] = &odd;
    EXPECT(acm_small_batch_check_slots(ACM_SMALL_BATCH_MAX, slots.data(), rows, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "n_classes") && strstr(msg, "7"));
    odd = blocks[7], odd.n_channels = 4;
    EXPECT(acm_small_batch_check_slots(ACM_SMALL_BATCH_MAX, slots.data(), rows, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "n_channels"));
    odd = blocks[7], odd.train = 0;
    EXPECT(acm_small_batch_check_slots(ACM_SMALL_BATCH_MAX, slots.data(), rows, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "train"));
    odd = blocks[7], odd.row_scale = (const float*)0x208;
    EXPECT(acm_small_batch_check_slots(ACM_SMALL_BATCH_MAX, slots.data(), rows, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "row_scale"));
    slots[7] = &blocks[7];
    // overlaps: the last byte of one workspace is the first of the next; a range that ends at the top of the address space;
    // a range that starts at address 1; logits inside another slot's workspace; two runs with one loss scalar
    acm_small_step_t lo = block(0x20000000u, 4096, 3), hi = block(0x20000000u + 4095, 4096, 3);
    const acm_small_step_t* two[4] = {&lo, nullptr, nullptr, &hi};
    EXPECT(acm_small_batch_check_slots(4, two, rows, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "overlap") && strstr(msg, "workspace"));
    hi = block(0x20000000u + 4096, 4096, 3);
    hi.logits = (float*)(0x20000000u + 8192 + 8192), hi.loss = (float*)(0x20000000u + 8192 + 16384);
    lo.logits = (float*)0x30000000u, lo.loss = (float*)0x30100000u;
    EXPECT(acm_small_batch_check_slots(4, two, rows, msg, sizeof(msg)) == ACM_OK);
    acm_small_step_t top = lo, bottom = hi;
    top.workspace = (void*)(UINTPTR_MAX - 4095), top.workspace_bytes = 4096;             // ends at the last address
    bottom.workspace = (void*)(uintptr_t)1, bottom.workspace_bytes = 64;
    const acm_small_step_t* ends[2] = {&top, &bottom};
    EXPECT(acm_small_batch_check_slots(2, ends, rows, msg, sizeof(msg)) == ACM_OK);
    bottom.workspace = (void*)(UINTPTR_MAX - 7), bottom.workspace_bytes = 8;
    EXPECT(acm_small_batch_check_slots(2, ends, rows, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "overlap"));
    bottom.workspace = (void*)(uintptr_t)1, bottom.workspace_bytes = SIZE_MAX;            // covers everything above address 1
    EXPECT(acm_small_batch_check_slots(2, ends, rows, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "overlap"));
    bottom = hi;
    bottom.logits = (float*)((uintptr_t)lo.workspace + 128);
    const acm_small_step_t* mixed[2] = {&lo, &bottom};
    EXPECT(acm_small_batch_check_slots(2, mixed, rows, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "logits") && strstr(msg, "workspace"));
    bottom = hi, bottom.loss = lo.loss;
    EXPECT(acm_small_batch_check_slots(2, mixed, rows, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "loss"));
    // an evaluation batch: no loss, no row count known
    lo.loss = bottom.loss = nullptr, lo.train = bottom.train = 0;
    EXPECT(acm_small_batch_check_slots(2, mixed, 0, msg, sizeof(msg)) == ACM_OK);
    EXPECT(acm_ranges_overlap(10, 0, 10, 5) == false && acm_ranges_overlap(10, 5, 14, 1) && !acm_ranges_overlap(10, 5, 15, 1));
    if (failures) return 1;
    printf("small_batch_host: ok\n");
    return 0;
}
