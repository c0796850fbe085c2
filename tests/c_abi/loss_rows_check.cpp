// csrc/acm_items.h on the host: the work list of a subset of the rows (the loss-row attachment, acm_csr_build_loss_rows),
// checked against what the kernels that walk it rely on.  Includes that header alone.
#include <cstdint>
#include <cstdio>
#include <map>
#include <vector>

#include "acm_items.h"

#define CHECK(cond)                                                             \
    do {                                                                        \
        if (!(cond)) {                                                          \
            std::printf("loss_rows_check: line %d: %s\n", __LINE__, #cond);     \
            return 1;                                                           \
        }                                                                       \
    } while (0)

namespace {

uint64_t g_state = 0x2545F4914F6CDD1Dull;
uint32_t rnd() {
    g_state = g_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(g_state >> 33);
}

// one list (full or filtered) against the structure the gathers walk
int check_list(const std::vector<int32_t>& indptr, int chunk, const uint8_t* keep, const std::vector<AcmItem>& items,
               const std::vector<AcmLongRow>& longs, int64_t n_slots, int64_t n_windows, int64_t n_multi,
               const std::vector<AcmItem>* full_items) {
    const int64_t n = (int64_t)indptr.size() - 1;
    // every kept row's edges exactly once, no dropped row
    std::vector<int32_t> covered((size_t)n, 0);
    std::vector<int32_t> next_edge(indptr.begin(), indptr.end() - 1);
    for (const AcmItem& it : items) {
        CHECK(it.row >= 0 && it.row < n);
        CHECK(!keep || keep[it.row]);
        CHECK(it.begin <= it.end && it.begin >= indptr[it.row] && it.end <= indptr[it.row + 1]);
        if (it.begin < it.end) CHECK(it.begin == next_edge[it.row]);          // pieces in order, no gap, no overlap
        if (it.begin < it.end) next_edge[it.row] = it.end;
        covered[it.row] += it.end - it.begin;
    }
    for (int64_t r = 0; r < n; ++r) CHECK(covered[r] == ((keep && !keep[r]) ? 0 : indptr[r + 1] - indptr[r]));
    // pieces first, in whole windows; whole rows behind them
    CHECK(n_windows * ACM_WINDOW <= (int64_t)items.size());
    for (size_t i = 0; i < items.size(); ++i) CHECK((items[i].slot >= 0) == ((int64_t)i < n_windows * ACM_WINDOW));
    // slots: 0, 1, 2, ... in list order; per row consecutive; a row's items never straddle a window unless it fills whole ones
    for (int64_t i = 0; i < n_windows * ACM_WINDOW; ++i) CHECK(items[(size_t)i].slot == (int32_t)i);
    CHECK(n_slots == n_windows * ACM_WINDOW);
    int64_t multi = 0, at = 0;
    for (const AcmLongRow& lr : longs) {
        CHECK(lr.slot_begin == (int32_t)at && lr.slot_end > lr.slot_begin);
        for (int32_t s = lr.slot_begin; s < lr.slot_end; ++s) CHECK(items[(size_t)s].row == lr.row);
        CHECK(indptr[lr.row + 1] - indptr[lr.row] > chunk);
        if (lr.windows > 1) {
            ++multi;
            CHECK(lr.slot_begin % ACM_WINDOW == 0 && lr.slot_end - lr.slot_begin == lr.windows * ACM_WINDOW);
        } else {
            CHECK(lr.slot_begin / ACM_WINDOW == (lr.slot_end - 1) / ACM_WINDOW);      // inside one window
        }
        at = lr.slot_end;
    }
    CHECK(at == n_slots && multi == n_multi);
    // whole rows in row order, each once
    int32_t prev = -1;
    for (size_t i = (size_t)(n_windows * ACM_WINDOW); i < items.size(); ++i) {
        CHECK(items[i].row > prev && items[i].end - items[i].begin <= chunk);
        CHECK(items[i].begin == indptr[items[i].row] && items[i].end == indptr[items[i].row + 1]);
        prev = items[i].row;
    }
    // a kept row's non-empty items are those of the full list, in the same order
    if (full_items) {
        std::map<int32_t, std::vector<std::pair<int32_t, int32_t>>> a, b;
        for (const AcmItem& it : *full_items)
            if (it.begin < it.end && (!keep || keep[it.row])) a[it.row].push_back({it.begin, it.end});
        for (const AcmItem& it : items)
            if (it.begin < it.end) b[it.row].push_back({it.begin, it.end});
        CHECK(a == b);
    }
    return 0;
}

int run_case(const std::vector<int32_t>& deg, int chunk, int mask_kind) {
    const int64_t n = (int64_t)deg.size();
    std::vector<int32_t> indptr((size_t)n + 1, 0);
    for (int64_t r = 0; r < n; ++r) indptr[(size_t)r + 1] = indptr[(size_t)r] + deg[(size_t)r];
    std::vector<uint8_t> keep((size_t)n, 1);
    for (int64_t r = 0; r < n; ++r) {
        if (mask_kind == 1) keep[(size_t)r] = 0;                                 // none
        if (mask_kind == 2) keep[(size_t)r] = (uint8_t)(rnd() & 1);              // random half
        if (mask_kind == 3) keep[(size_t)r] = deg[(size_t)r] > chunk ? 0 : 1;    // only the long rows dropped
        if (mask_kind == 4) keep[(size_t)r] = (uint8_t)((rnd() % 3) ? 7 : 0);    // (any non-zero byte keeps)
    }
    std::vector<AcmItem> full;
    std::vector<AcmLongRow> full_longs;
    int64_t fs = 0, fw = 0, fm = 0;
    int32_t md = 0;
    build_items(indptr, chunk, full, full_longs, fs, md, fw, fm);
    if (check_list(indptr, chunk, nullptr, full, full_longs, fs, fw, fm, nullptr)) return 1;
    AcmLossRowsHost h;
    acm_loss_rows_host(indptr, keep.data(), chunk, h);
    if (check_list(indptr, chunk, keep.data(), h.items, h.longs, h.n_slots, h.n_windows, h.n_multi, &full)) return 1;
    int64_t kept_rows = 0, kept_edges = 0;
    for (int64_t r = 0; r < n; ++r)
        if (keep[(size_t)r]) ++kept_rows, kept_edges += deg[(size_t)r];
    CHECK(h.kept_rows == kept_rows && h.kept_edges == kept_edges);
    CHECK(h.long_index.empty() == h.longs.empty());
    for (size_t i = 0; i < h.longs.size(); ++i) CHECK(h.long_index[(size_t)h.longs[i].row] == (int32_t)i);
    if (mask_kind == 0) {                       // every row kept: the full list itself
        CHECK(h.items.size() == full.size() && h.n_slots == fs && h.n_windows == fw && h.n_multi == fm);
        for (size_t i = 0; i < full.size(); ++i)
            CHECK(h.items[i].row == full[i].row && h.items[i].begin == full[i].begin && h.items[i].end == full[i].end &&
                  h.items[i].slot == full[i].slot);
    }
    if (mask_kind == 1) CHECK(h.items.empty() && h.longs.empty() && h.n_slots == 0);
    return 0;
}

}  // namespace

int main() {
    for (int chunk : {8, 16, 128}) {
        // the row lengths at which the cut changes: empty, 1, chunk, chunk + 1, 16 chunk + 1, beyond 64 chunk (several windows)
        const std::vector<int32_t> edges = {0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk, 5 * chunk + 3, 16 * chunk, 16 * chunk + 1,
                                            33 * chunk, 64 * chunk, 64 * chunk + 1, 100 * chunk + 7};
        for (int mask_kind = 0; mask_kind < 5; ++mask_kind) {
            for (int rep = 0; rep < 6; ++rep) {
                std::vector<int32_t> deg;
                const int n = 40 + (int)(rnd() % 200);
                for (int r = 0; r < n; ++r) {
                    const uint32_t c = rnd() % 10;
                    deg.push_back(c < 4 ? (int32_t)(rnd() % (uint32_t)(chunk + 1)) : edges[rnd() % edges.size()]);
                }
                if (run_case(deg, chunk, mask_kind)) {
                    std::printf("loss_rows_check: chunk %d mask %d rep %d\n", chunk, mask_kind, rep);
                    return 1;
                }
            }
        }
        if (run_case(std::vector<int32_t>(50, 0), chunk, 2)) return 1;                        // no edge at all
        if (run_case(std::vector<int32_t>(3, 70 * chunk), chunk, 2)) return 1;               // long rows alone
    }
    std::printf("loss_rows_check: ok\n");
    return 0;
}
