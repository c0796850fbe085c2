// The slot checks of the batched small-graph forms (csrc/acm_small_batch_host.h) against blocks that set the residual branch
// (acm_small_step_t::residual, ACM-GCN++): the batched launches have no residual kernels, so a residual slot is refused with
// ACM_EUNSUPPORTED before any launch, whichever slot holds it and in both flavours of a batch.  Also where the appended
// fields lie: behind the block's old end, so a block that stops there is complete without the residual.  A stand-alone
// program, built with the host sanitizers by tests/test_small_residual_cpu.py and run on the CPU.  No device, no library.
#include <stddef.h>
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

static acm_small_step_t block(uintptr_t base, size_t ws_bytes) {
    acm_small_step_t p;
    memset(&p, 0, sizeof(p));
    p.n_classes = 3, p.n_channels = 3, p.train = 1, p.update = 1, p.f_in = 7;
    p.x_vals = (const float*)0x100, p.row_scale = (const float*)0x200;
    p.workspace = (void*)base, p.workspace_bytes = ws_bytes;
    p.logits = (float*)(base + ws_bytes), p.loss = (float*)(base + ws_bytes + 4096);
    return p;
}

int main(int argc, char** argv) {
    char msg[256] = "";
    if (argc > 1 && strcmp(argv[1], "--offsets") == 0) {      // for the ctypes mirror (acm_gnn_amd/_lib.py: SmallStep)
        printf("%zu %zu %zu %zu %zu\n", offsetof(acm_small_step_t, residual), offsetof(acm_small_step_t, workspace_bytes),
               offsetof(acm_small_step_t, res), offsetof(acm_small_step_t, drop_res), sizeof(acm_small_step_t));
        return 0;
    }
    const int64_t rows = 100;
    std::vector<acm_small_step_t> blocks;
    std::vector<const acm_small_step_t*> slots;
    for (int i = 0; i < 6; ++i) blocks.push_back(block(0x10000000u + (uintptr_t)i * 0x10000, 4096));
    for (auto& b : blocks) slots.push_back(&b);
    std::vector<int64_t> slot_rows(6, rows);
    EXPECT(acm_small_batch_check_slots(6, slots.data(), rows, msg, sizeof(msg)) == ACM_OK);
    EXPECT(acm_small_batch_check_slots_graphs(6, slots.data(), slot_rows.data(), msg, sizeof(msg)) == ACM_OK);
    // the residual in the first, a middle and the last slot; in every slot; behind empty slots; in a batch of one
    for (int k : {0, 3, 5}) {
        blocks[(size_t)k].residual = 1;
        EXPECT(acm_small_batch_check_slots(6, slots.data(), rows, msg, sizeof(msg)) == ACM_EUNSUPPORTED && strstr(msg, "residual"));
        char want[32];
        snprintf(want, sizeof(want), "slot %d", k);
        EXPECT(strstr(msg, want) != nullptr);
        EXPECT(acm_small_batch_check_slots_graphs(6, slots.data(), slot_rows.data(), msg, sizeof(msg)) == ACM_EUNSUPPORTED && strstr(msg, "residual"));
        blocks[(size_t)k].residual = 0;
    }
    for (auto& b : blocks) b.residual = 1;
    EXPECT(acm_small_batch_check_slots(6, slots.data(), rows, msg, sizeof(msg)) == ACM_EUNSUPPORTED && strstr(msg, "slot 0"));
    EXPECT(acm_small_batch_check_slots(1, slots.data(), rows, msg, sizeof(msg)) == ACM_EUNSUPPORTED && strstr(msg, "residual"));
    const acm_small_step_t* holes[4] = {nullptr, nullptr, &blocks[2], nullptr};
    EXPECT(acm_small_batch_check_slots(4, holes, rows, msg, sizeof(msg)) == ACM_EUNSUPPORTED && strstr(msg, "slot 2"));
    // a value that is neither 0 nor 1 is no residual-free slot either
    for (auto& b : blocks) b.residual = 0;
    blocks[4].residual = 7;
    EXPECT(acm_small_batch_check_slots(6, slots.data(), rows, msg, sizeof(msg)) == ACM_EUNSUPPORTED && strstr(msg, "residual = 7"));
    blocks[4].residual = 0;
    // the refusal comes before the shared-field and overlap objections: one message, the residual's
    blocks[1].residual = 1, blocks[2].n_classes = 4, blocks[3].workspace = blocks[0].workspace;
    EXPECT(acm_small_batch_check_slots(6, slots.data(), rows, msg, sizeof(msg)) == ACM_EUNSUPPORTED && strstr(msg, "residual"));
    blocks[1].residual = 0;
    EXPECT(acm_small_batch_check_slots(6, slots.data(), rows, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "n_classes"));
    // the count checks still come first
    EXPECT(acm_small_batch_check_slots(0, slots.data(), rows, msg, sizeof(msg)) == ACM_EINVAL && strstr(msg, "n_slots"));
    // layout: `residual` where reserved1 was (behind f_in), the new fields behind what was the block's last field
    static_assert(offsetof(acm_small_step_t, residual) == offsetof(acm_small_step_t, f_in) + 4, "residual follows f_in");
    static_assert(offsetof(acm_small_step_t, res) == offsetof(acm_small_step_t, workspace_bytes) + sizeof(size_t), "res follows the old end");
    static_assert(offsetof(acm_small_step_t, drop_res) == offsetof(acm_small_step_t, res) + 2 * sizeof(acm_adam_tensor_t), "drop_res is last");
    static_assert(sizeof(acm_small_step_t) == offsetof(acm_small_step_t, drop_res) + sizeof(acm_dropout_t), "nothing behind drop_res");
    if (failures) return 1;
    printf("small_residual_host: ok\n");
    return 0;
}
