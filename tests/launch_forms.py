"""The launch thresholds the large GPU cases rely on, and the sizes those cases use.

The kernels of the synthetic study decide their launch shape from constants sized for real graphs: grid caps behind which a
grid-stride loop takes a second trip, tile limits, rounds per block.  A case that is meant to pass such a threshold imports its
size from here, and tests/test_launch_forms_cpu.py reads every constant back from the source text: a retune that moves a
threshold fails there instead of quietly turning these cases into repeats of the small ones."""

CSRC = "acm_gnn_amd/csrc/"

# name -> (source file, regular expression with one group, the value the cases below were sized for)
THRESHOLDS = {
    "HOM_BALLOT_C": (CSRC + "acm_homophily.hip", r"constexpr int HOM_BALLOT_C = (\d+);", 8),
    "HOM_FIN_BLOCKS": (CSRC + "acm_homophily.hip", r"constexpr int HOM_FIN_BLOCKS = (\d+);", 256),
    "HOM_MEANS_MAX_TILES": (CSRC + "acm_homophily.hip", r"constexpr int HOM_MEANS_MAX_TILES = (\d+);", 2048),
    "HOM_MEANS_MIN_TILE_ROWS": (CSRC + "acm_homophily.hip", r"return \(int\)\(t < (\d+) \? \1 : t\);", 128),
    "HOM_PREP_CAP": (CSRC + "acm_homophily.hip", r"hom_blocks\(n_cols > n_rows \? n_cols : n_rows, 256, (\d+)\)", 4096),
    "HOM_EDGES_ITEMS_PER_BLOCK": (CSRC + "acm_homophily.hip", r"hom_blocks\(a->n_items, (\d+), \d+\)", 64),
    "HOM_EDGES_CAP": (CSRC + "acm_homophily.hip", r"hom_blocks\(a->n_items, \d+, (\d+)\)", 2048),
    "HOM_SCORE_LDS_STEP": (CSRC + "acm_homophily.hip", r"hom_blocks\(n_rows, 64, lds > (\d+) \? \d+ : \d+\)", 16384),
    "HOM_SCORE_CAP_LARGE_LDS": (CSRC + "acm_homophily.hip", r"hom_blocks\(n_rows, 64, lds > \d+ \? (\d+) : \d+\)", 512),
    "HOM_SCORE_CAP": (CSRC + "acm_homophily.hip", r"hom_blocks\(n_rows, 64, lds > \d+ \? \d+ : (\d+)\)", 2048),
    "GCN_BWD_MAX_BLOCKS": (CSRC + "acm_gcn.hip", r"constexpr int GCN_BWD_MAX_BLOCKS = (\d+);", 256),
    "GCN_BWD_MAX_HIDDEN": (CSRC + "acm_gcn.hip", r"constexpr int GCN_BWD_MAX_HIDDEN = (\d+);", 256),
    "GCN_FWD_SHORT_REST": (CSRC + "acm_gcn.hip", r"left - 256 <= (\d+) \? 128 : 256", 8),
    "NARROW_8_LANES_UP_TO": (CSRC + "acm_gather_device.h", r"return avg <= (\d+)\.0 \? 8 :", 12),
    "NARROW_16_LANES_UP_TO": (CSRC + "acm_gather_device.h", r"\? 8 : \(avg <= (\d+)\.0 \? 16 : 32\)", 160),
    "GATHER_L2_MIB": (CSRC + "acm_gather_device.h", r"constexpr size_t GATHER_L2_BYTES = (\d+)u << 20;", 8),
    "VEC_MIN_ROW_ONE": (CSRC + "acm_gather_device.h", r"constexpr int VEC_MIN_ROW_ONE = (\d+);", 16),
    "VEC_MIN_ROW_MANY": (CSRC + "acm_gather_device.h", r"constexpr int VEC_MIN_ROW_MANY = (\d+);", 4),
    "VEC_ROW_ONE_IS_USED": (CSRC + "acm_gather_device.h", r"bool vec = [^;]*\(NG == (\d) && nnz >= VEC_MIN_ROW_ONE \* n_rows\)", 1),
    "VEC_ROW_MANY_IS_USED": (CSRC + "acm_gather_device.h", r"bool vec = [^;]*l2_resident && NG > (\d) && nnz >= VEC_MIN_ROW_MANY \* n_rows\)", 1),
    "K4_SPLIT_MIN_ROW": (CSRC + "acm_conv_bwd.hip", r"constexpr int K4_SPLIT_MIN_ROW = (\d+);", 32),
    "K4_SPLIT_IS_USED": (CSRC + "acm_conv_bwd.hip", r"sizeof\(float\) > GATHER_L2_BYTES && nnz >= K4_SPLIT_MIN_ROW \* n_rows;\n[^\n]*want_split == (\d) \? false", 0),
    "COPY_CHUNK": (CSRC + "acm_select.hip", r"constexpr int CHUNK = (\d+);", 2048),
    "COPY_MAX_BLOCKS": (CSRC + "acm_select.hip", r"constexpr int MAX_BLOCKS = (\d+);", 1024),
    "ADAM_CHUNK": (CSRC + "acm_optim.hip", r"constexpr int CHUNK = (\d+);", 2048),
    "ADAM_MAX_BLOCKS": (CSRC + "acm_optim.hip", r"constexpr int MAX_BLOCKS = (\d+);", 1024),
    "AUC_TILE": (CSRC + "acm_rocauc.hip", r"constexpr int AUC_TILE = (\d+);", 1024),
    "AUC_SCAN_STEP": (CSRC + "acm_rocauc.hip", r"for \(long b0 = 0; b0 < nblk; b0 \+= (\d+)\)", 256),
    "AUC_SCORES_CAP": (CSRC + "acm_rocauc.hip", r"if \(nb > (\d+)\) nb = \1;", 4096),
    "SYN_UNIFORM_CAP": (CSRC + "acm_synth.hip", r"syn_grid\(n_rows \* F4, 256, (\d+)\)", 8192),
    "SYN_DRAW_CAP": (CSRC + "acm_synth.hip", r"syn_grid\(\(n_draws \+ 1\) / 2, 256, (\d+)\)", 4096),
    "SYN_CHUNK": (CSRC + "acm_synth.hip", r"constexpr int SYN_CHUNK = (\d+);", 4096),
    "SYN_SCAN_THREADS": (CSRC + "acm_synth.hip", r"const long per = \(nblk \+ 255\) / (\d+);", 256),
    "ACM_SYNTH_MAX_FEATURES": ("include/acm_hip.h", r"#define ACM_SYNTH_MAX_FEATURES (\d+)", 262144),
}
T = {name: value for name, (_, _, value) in THRESHOLDS.items()}

# ---- acm_class_score ---------------------------------------------------------------------------------------------------------
SCORE_SHAPES = [(2, 1), (15, 3), (16, 4), (17, 15), (32, 16), (33, 17), (48, 60), (49, 64), (64, 65),
                (20, 128), (40, 192), (33, 200), (49, 241), (64, 255), (64, 256)]            # (C, F)
SCORE_SMALL_N = [1, 15, 16, 17, 63, 65, 1000]
SCORE_SECOND_TRIPS = [(3, 4, 2048 * 64 + 83), (64, 80, 512 * 64 + 77)]                      # (C, F, n)

# ---- acm_class_means ---------------------------------------------------------------------------------------------------------
MEANS_CASES = [(262_144, 3, 2, 0), (262_145, 3, 2, 0), (270_001, 3, 2, 0),                  # (n, F, C, padding columns)
               (1000, 64, 5, 3), (1000, 65, 5, 3), (1000, 128, 5, 3), (1000, 129, 5, 3)]

# ---- acm_homophily_census ----------------------------------------------------------------------------------------------------
CENSUS_BALLOT_CLASSES = [8, 9]
CENSUS_SMALL_N = 4099
CENSUS_EDGES_N = 140_001            # work items beyond the edges cap, rows beyond the finish cap
CENSUS_PREP_N = 1_048_577

# ---- acm_gcn_bwd / acm_gcn_fwd -------------------------------------------------------------------------------------------------
GCN_BWD_SHAPES = [(1, 1), (7, 3), (9, 5), (31, 8), (33, 3), (255, 5), (256, 1), (256, 8)]   # (hidden, width)
GCN_BWD_OPERATORS = [(63, None, 8), (300, None, 16), (400, 0.5, 32)]                        # (n, density, lanes at width < 5)
GCN_BWD_MAX_BLOCKS = T["GCN_BWD_MAX_BLOCKS"]
GCN_BWD_HELD_GRIDS = [(9000, 6, 33, 3, 8), (2500, 20, 33, 5, 32)]                           # (n, mean degree, hidden, width, lanes)
GCN_FWD_RIDDEN_WIDTHS = [16, 17, 63, 65, 128, 129, 192, 193, 255, 256]
GCN_FWD_SPLIT_WIDTHS = [264, 265, 520]

# ---- the gather family's chooser (tests/gather_forms.py) ---------------------------------------------------------------------------
GATHER_BIG_COLS = 16_500            # table rows of the large operators: two channels of 64 columns, or one of 128, exceed the L2 bound
GATHER_BIG_ROWS = 300
GATHER_BIG_MEANS = (48, 20)         # mean row lengths aimed at: at least K4's 32 for the automatic split, and below it
GATHER_DENSE_SHAPE = (190, 200)     # density 0.9: more than 160 entries per row and per column (32 lanes, both ways)

# ---- acm_copy_if / acm_adam_step -------------------------------------------------------------------------------------------------
COPY_TABLES = [[2_097_152], [2_097_153, 5, 1025], [3, 4_194_309, 1024, 0, 7]]
ADAM_SIZES = [2_097_153, 4_200_003]

# ---- acm_rocauc ------------------------------------------------------------------------------------------------------------------
AUC_TILE_EDGE_N = [1023, 1024, 1025, 2047, 2048]
AUC_SCAN_N = 300_007
AUC_SCORES_N = 1_048_700

# ---- acm_synth_* -------------------------------------------------------------------------------------------------------------------
SYN_FEATURES = [(2100, 4004), (2100, 4003)]
SYN_DRAWS = 4_200_003
SYN_SELECT = dict(a=300_000, draws=1_100_000, m=250_000)


def coverage():
    """[(what, value that has to exceed, threshold expression)]: every listed size passes the threshold it was chosen for."""
    out = []
    for c, f, n in SCORE_SECOND_TRIPS:
        tiles = (c + 15) // 16
        fp = (f + 15) // 16 * 16
        lds = tiles * 16 * (fp if fp % 64 == 0 else fp + 4) * 4
        cap = T["HOM_SCORE_CAP_LARGE_LDS"] if lds > T["HOM_SCORE_LDS_STEP"] else T["HOM_SCORE_CAP"]
        out.append((f"class_score C={c} F={f} n={n}: a second trip", n, cap * 64))
    out.append(("class_score: the second case sits under the small-LDS cap, so only the large-LDS cap makes it a second trip",
                T["HOM_SCORE_CAP"] * 64, SCORE_SECOND_TRIPS[1][2]))
    big = [n for n, _, _, _ in MEANS_CASES if n > 100_000]
    out.append(("class_means: the smallest large n still has 128-row tiles", T["HOM_MEANS_MAX_TILES"] * T["HOM_MEANS_MIN_TILE_ROWS"] + 1,
                min(big)))
    out.append(("class_means: tiles above the minimum", max(big), T["HOM_MEANS_MAX_TILES"] * T["HOM_MEANS_MIN_TILE_ROWS"]))
    out.append(("census: SMALL boundary", CENSUS_BALLOT_CLASSES[1], T["HOM_BALLOT_C"]))
    out.append(("census: SMALL boundary (below)", T["HOM_BALLOT_C"] + 1, CENSUS_BALLOT_CLASSES[0]))
    out.append(("census: work items beyond the edges grid", CENSUS_EDGES_N, T["HOM_EDGES_CAP"] * T["HOM_EDGES_ITEMS_PER_BLOCK"]))
    out.append(("census: rows beyond the finish grid", CENSUS_EDGES_N, T["HOM_FIN_BLOCKS"] * 256))
    out.append(("census: nodes beyond the prep grid", CENSUS_PREP_N, T["HOM_PREP_CAP"] * 256))
    for n, _, _, _, lanes in GCN_BWD_HELD_GRIDS:
        out.append((f"gcn_bwd n={n}: rows (work items) beyond the held grid", n, T["GCN_BWD_MAX_BLOCKS"] * (256 // lanes)))
    out.append(("gcn_bwd: hidden at the limit", max(h for h, _ in GCN_BWD_SHAPES) + 1, T["GCN_BWD_MAX_HIDDEN"]))
    out.append(("gcn_fwd: 264 columns split 128 + rest", 256 + T["GCN_FWD_SHORT_REST"] + 1, GCN_FWD_SPLIT_WIDTHS[0]))
    out.append(("gcn_fwd: 265 columns split 256 + rest", GCN_FWD_SPLIT_WIDTHS[1], 256 + T["GCN_FWD_SHORT_REST"]))
    l2 = T["GATHER_L2_MIB"] << 20
    out.append(("gather: two channels of 64 columns of the large table exceed the L2 bound", GATHER_BIG_COLS * 64 * 2 * 4, l2))
    out.append(("gather: one channel of 128 columns of the large table exceeds it", GATHER_BIG_COLS * 128 * 4, l2))
    out.append(("gather: one channel of 64 columns of the large table stays resident", l2 + 1, GATHER_BIG_COLS * 64 * 4))
    out.append(("gather: two channels of 32 columns of the large table stay resident", l2 + 1, GATHER_BIG_COLS * 32 * 2 * 4))
    out.append(("gather: the denser large operator takes K4's automatic split", GATHER_BIG_MEANS[0] + 1, T["K4_SPLIT_MIN_ROW"]))
    out.append(("gather: the sparser one does not", T["K4_SPLIT_MIN_ROW"], GATHER_BIG_MEANS[1]))
    out.append(("gather: ... and still takes the vector form with one channel", GATHER_BIG_MEANS[1] + 1, T["VEC_MIN_ROW_ONE"]))
    out.append(("gather: the dense operator's rows exceed the 16-lane bound", int(0.88 * (min(GATHER_DENSE_SHAPE) - 2)),
                T["NARROW_16_LANES_UP_TO"]))
    for table in COPY_TABLES[1:]:
        out.append(("copy_if: rounds > 1", max(table), T["COPY_CHUNK"] * T["COPY_MAX_BLOCKS"]))
    out.append(("copy_if: the last size with one round", T["COPY_CHUNK"] * T["COPY_MAX_BLOCKS"] + 1, COPY_TABLES[0][0]))
    for n in ADAM_SIZES:
        out.append(("adam: rounds > 1", n, T["ADAM_CHUNK"] * T["ADAM_MAX_BLOCKS"]))
    out.append(("rocauc: n + 1 positions beyond the scan's first trip", AUC_SCAN_N + 1, T["AUC_SCAN_STEP"] * T["AUC_TILE"]))
    out.append(("rocauc: rows beyond the scores grid", AUC_SCORES_N, T["AUC_SCORES_CAP"] * 256))
    out.append(("rocauc: tile edges straddle AUC_TILE", max(AUC_TILE_EDGE_N) + 1, 2 * T["AUC_TILE"]))
    for n, f in SYN_FEATURES:
        out.append((f"synth uniform {n} x {f}: quads beyond the grid", n * ((f + 3) // 4), T["SYN_UNIFORM_CAP"] * 256))
        out.append((f"synth uniform: {f} features allowed", T["ACM_SYNTH_MAX_FEATURES"] + 1, f))
    out.append(("synth draw: pairs beyond the grid", (SYN_DRAWS + 1) // 2, T["SYN_DRAW_CAP"] * 256))
    out.append(("synth scan: per > 1", (SYN_SELECT["draws"] + T["SYN_CHUNK"] - 1) // T["SYN_CHUNK"], T["SYN_SCAN_THREADS"]))
    return out
