// The work list of a graph handle as plain host C++ (no device header): the item records, the cut of the rows into work
// items (build_items) and the host-side part of the loss-row attachment (acm_csr_build_loss_rows): the list over a
// subset of the rows.  acm_csr.cpp is the only user inside the library;
// tests/c_abi/loss_rows_check.cpp includes this header alone and checks what the kernels rely on.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#define ACM_WINDOW 16         // work items per window of the piece region (see build_items)

// A work item: neighbours [begin,end) of `row`; slot < 0 => the item is the whole
// row and its owner runs the epilogue, otherwise it is one piece of a long row and
// its partial sums go to partial slot `slot` (combined in order by the fix-up pass, or
// through LDS by a kernel that takes whole windows, see build_items).
struct AcmItem {
    int32_t row, begin, end, slot;
};
// A long row and its partial slots [slot_begin, slot_end).
struct AcmLongRow {
    int32_t row, slot_begin, slot_end, windows;   // windows > 1: the row's pieces fill that many whole windows (build_items)
};

// Split rows into work items of at most `chunk` neighbours -- host side, from a host copy of indptr.
// A long row (more than `chunk` neighbours) becomes P = min(16, ceil(deg / chunk)) near-equal pieces with consecutive
// partial slots.  All pieces come FIRST in the list, packed into windows of ACM_WINDOW = 16 items so that the pieces of
// one row never straddle a window (a window that cannot take the next row is filled up with empty pieces of the row
// before, and so is the last one): a kernel whose workgroup takes one window per round (16 groups of 16 lanes) can
// combine the pieces of a row through LDS and finish the row itself instead of leaving partial sums to a second
// launch; every other kernel writes the pieces to their partial slots as before.  The whole rows follow in row order.
// Returns in n_multi the rows that take several windows.
// `keep` (n bytes, or NULL = every row): the list of the rows with keep[r] != 0 alone.  A kept row gets exactly the items
// it has in the full list -- the cut of a row depends on its own length and `chunk` only --, a dropped row gets none; where
// the padding pieces fall, the slot numbers and the window count are the list's own.
inline void build_items(const std::vector<int32_t>& indptr, int chunk, std::vector<AcmItem>& items,
                        std::vector<AcmLongRow>& longs, int64_t& n_slots, int32_t& max_deg, int64_t& n_windows, int64_t& n_multi,
                        const uint8_t* keep = nullptr) {
    const int64_t n = (int64_t)indptr.size() - 1;
    items.clear();
    longs.clear();
    items.reserve(n + n / 8);
    n_slots = 0;
    max_deg = 0;
    n_multi = 0;
    for (int64_t r = 0; r < n; ++r) {
        const int32_t b = indptr[r], e = indptr[r + 1];
        const int32_t deg = e - b;
        max_deg = std::max(max_deg, deg);
        if (deg <= chunk || (keep && !keep[r])) continue;
        int32_t pieces = (deg + chunk - 1) / chunk;
        // A row that sixteen pieces of up to 4 x chunk neighbours do not cover takes SEVERAL whole windows (at most sixteen)
        // of pieces of about 2 x chunk: sixteen pieces in one window all run on the CU that window's workgroup lands on,
        // and a row of 21 k neighbours then keeps one texture path busy for ~20 us whatever the rest of the chip does (the
        // floor of a rank's gathers in an 8-rank plan: DESIGN.md section 7).  With the chunk sized to the operator
        // (nnz / 32768 < chunk <= nnz / 16384) the bar of 64 x chunk neighbours is 0.5 .. 1 x the mean CU's share of the
        // whole operator: no row of the twitch- or arXiv-year-shaped graphs reaches it on one GPU, the top rows of a rank
        // of an 8-rank plan do.  (A lower bar -- every row above 32 x chunk that is also above nnz / 128 -- left the rows of
        // 8-13 k neighbours in one window each and was slower per rank: 27-29 us against 22-27 us for the output-layer
        // backward gather.)  A window of such a row leaves its sum in its first piece's slot and a small second launch adds
        // the windows (AcmLongRow.windows > 1).
        int32_t windows = 0;
        if (pieces > ACM_WINDOW && (deg + ACM_WINDOW - 1) / ACM_WINDOW > 4 * chunk) {
            windows = (deg + 2 * ACM_WINDOW * chunk - 1) / (2 * ACM_WINDOW * chunk);
            if (windows > ACM_WINDOW) windows = ACM_WINDOW;
            pieces = windows * ACM_WINDOW;
        } else if (pieces > ACM_WINDOW) {
            pieces = ACM_WINDOW;
        }
        const int32_t room = ACM_WINDOW - (int32_t)(items.size() % ACM_WINDOW);
        if ((room < pieces || windows) && room < ACM_WINDOW) {    // does not fit: pad with empty pieces of the row before
            AcmLongRow& prev = longs.back();
            for (int32_t q = 0; q < room; ++q) items.push_back({prev.row, indptr[prev.row + 1], indptr[prev.row + 1], (int32_t)n_slots++});
            prev.slot_end = (int32_t)n_slots;
        }
        const int32_t per = (deg + pieces - 1) / pieces;
        AcmLongRow lr = {(int32_t)r, (int32_t)n_slots, 0, windows};
        for (int32_t q = 0; q < pieces; ++q) {
            const int32_t s = std::min(e, b + q * per);
            items.push_back({(int32_t)r, s, std::min(e, s + per), (int32_t)n_slots++});
        }
        lr.slot_end = (int32_t)n_slots;
        n_multi += windows > 1;
        longs.push_back(lr);
    }
    if (!longs.empty() && items.size() % ACM_WINDOW) {
        AcmLongRow& prev = longs.back();
        while (items.size() % ACM_WINDOW) items.push_back({prev.row, indptr[prev.row + 1], indptr[prev.row + 1], (int32_t)n_slots++});
        prev.slot_end = (int32_t)n_slots;
    }
    n_windows = (int64_t)items.size() / ACM_WINDOW;
    for (int64_t r = 0; r < n; ++r)
        if (indptr[r + 1] - indptr[r] <= chunk && !(keep && !keep[r])) items.push_back({(int32_t)r, indptr[r], indptr[r + 1], -1});
}

// The host-side part of a loss-row attachment, from a host copy of the operator's indptr.
struct AcmLossRowsHost {
    std::vector<AcmItem> items;          // the work list of the kept rows
    std::vector<AcmLongRow> longs;
    std::vector<int32_t> long_index;     // n_rows: index into longs or -1 (empty without long rows)
    int64_t n_slots = 0, n_windows = 0, n_multi = 0;
    int64_t kept_rows = 0, kept_edges = 0;
};

inline void acm_loss_rows_host(const std::vector<int32_t>& indptr, const uint8_t* keep, int chunk, AcmLossRowsHost& out) {
    const int64_t n = (int64_t)indptr.size() - 1;
    out = AcmLossRowsHost();
    for (int64_t r = 0; r < n; ++r)
        if (keep[r]) {
            ++out.kept_rows;
            out.kept_edges += indptr[r + 1] - indptr[r];
        }
    int32_t max_deg = 0;
    build_items(indptr, chunk, out.items, out.longs, out.n_slots, max_deg, out.n_windows, out.n_multi, keep);
    if (!out.longs.empty()) {
        out.long_index.assign((size_t)n, -1);
        for (size_t i = 0; i < out.longs.size(); ++i) out.long_index[(size_t)out.longs[i].row] = (int32_t)i;
    }
}
