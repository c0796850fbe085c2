"""Device-resident CSR operators for the ACM filters.

``CsrGraph`` owns an ``acm_csr_t`` handle (CSR arrays + nnz-balanced work list
in HBM).  ``FilterOperators`` bundles what one ACM layer needs: A_low, its
transpose (backward), and -- for the structure channel -- the degree vector
``d = rowsum(I + A)`` that turns A_low into the raw adjacency
(``A = D A_low - I``).

``operators_for(adj_low, adj_high, adj_un)`` is the drop-in entry: it accepts
the tensors the reference hands to ``GraphConvolution.forward`` (sparse COO,
possibly un-coalesced, ACM-Geometric/utils.py:21-28; dense strided ``adj_low``,
ACM-Pytorch/utils.py:619-629), converts once and caches by storage identity.
"""
import ctypes as C
import weakref

import torch

from . import _lib


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _stream():
    """hipStream_t of torch's current stream on the current device (the raw getter is ~10x cheaper than building a
    torch.cuda.Stream object; it is what torch's own extensions use)."""
    if _raw_stream is not None:
        return C.c_void_p(_raw_stream(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _NoSwitch:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NO_SWITCH = _NoSwitch()


def _device_ctx(dev):
    """Make ``dev`` current for the launch; free when it already is (one process per GPU: always)."""
    idx = dev.index if isinstance(dev, torch.device) else torch.device(dev).index
    if idx is None or idx == torch.cuda.current_device():
        return _NO_SWITCH
    return torch.cuda.device(dev)


def _sync(dev):
    torch.cuda.synchronize(dev)


def _copy_from_ptr(ptr, n, dtype, device):
    """New torch tensor holding n elements copied from a raw device pointer owned by a handle."""
    t = torch.empty(n, dtype=dtype, device=device)
    if n:
        C.cdll.LoadLibrary("libamdhip64.so").hipMemcpy(
            C.c_void_p(t.data_ptr()), C.c_void_p(ptr), C.c_size_t(n * t.element_size()), 3)   # device-to-device
    return t


def _require_cuda(t, name):
    if not t.is_cuda:
        raise RuntimeError(
            f"acm_gnn_amd: {name} is on {t.device}; the ACM operators run only on an AMD GPU "
            "(there is no CPU fallback)")


class CsrGraph:
    """A CSR row block in HBM with its work list (``acm_csr_t``)."""

    def __init__(self, handle, device):
        self._h = C.c_void_p(handle)
        self.device = device
        info = _lib.CsrInfo()
        _lib.check(_lib.load().acm_csr_info(self._h, C.byref(info)), "acm_csr_info")
        self.n_rows, self.n_cols, self.nnz = info.n_rows, info.n_cols, info.nnz
        self.n_items, self.n_long_rows = info.n_items, info.n_long_rows
        self.n_partial_slots, self.chunk, self.max_degree = info.n_partial_slots, info.chunk, info.max_degree
        self._ptrs = (info.indptr, info.indices, info.vals)
        self._src_pos_ptr = info.src_pos
        self._src_pos = None
        self._transposed = None
        self.stream_steps, self.stream_waves = info.stream_steps, info.stream_waves
        self.stream_slices, self.stream_long_rows = info.stream_slices, info.stream_long_rows
        self._finalizer = weakref.finalize(self, _lib.load().acm_csr_destroy, C.c_void_p(handle))

    # ---- construction ----------------------------------------------------
    @classmethod
    def from_csr(cls, indptr, indices, vals, n_cols, chunk=0):
        """indptr/indices/vals: device tensors (int32/int32/float32).  ``vals=None`` makes a
        pattern-only operator (every stored entry is 1; no value stream is read by the kernels)."""
        _require_cuda(indptr, "indptr")
        indptr = indptr.to(torch.int32).contiguous()
        indices = indices.to(device=indptr.device, dtype=torch.int32).contiguous()
        n_rows, nnz = indptr.numel() - 1, indices.numel()
        if vals is not None:
            vals = vals.to(device=indptr.device, dtype=torch.float32).contiguous()
            if vals.numel() != nnz:
                raise ValueError(f"vals has {vals.numel()} entries, indices {nnz}")
        out = C.c_void_p()
        with _device_ctx(indptr.device):
            _sync(indptr.device)
            st = _lib.load().acm_csr_create(n_rows, int(n_cols), nnz, indptr.data_ptr(),
                                            indices.data_ptr() if nnz else None,
                                            vals.data_ptr() if (nnz and vals is not None) else None, int(chunk),
                                            C.byref(out))
        _lib.check(st, "acm_csr_create")
        return cls(out.value, indptr.device)

    @classmethod
    def from_torch(cls, adj, chunk=0):
        """Sparse COO (coalesced or not) / sparse CSR / dense strided square-or-not matrix."""
        _require_cuda(adj, "adjacency")
        if adj.layout == torch.sparse_csr:
            return cls.from_csr(adj.crow_indices(), adj.col_indices(), adj.values(), adj.shape[1], chunk)
        if adj.layout == torch.strided:
            adj = adj.to_sparse()
        if adj.layout != torch.sparse_coo:
            raise TypeError(f"unsupported adjacency layout {adj.layout}")
        adj = adj.coalesce()                      # sorts by (row, col), sums duplicates
        idx, vals = adj.indices(), adj.values().to(torch.float32)
        n_rows, n_cols = adj.shape
        counts = torch.bincount(idx[0], minlength=n_rows)
        indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=adj.device)
        indptr[1:] = torch.cumsum(counts, 0)
        return cls.from_csr(indptr.to(torch.int32), idx[1].to(torch.int32), vals, n_cols, chunk)

    @classmethod
    def from_scipy(cls, mat, device, chunk=0):
        m = mat.tocsr()
        m.sort_indices()
        dev = torch.device(device)
        return cls.from_csr(torch.from_numpy(m.indptr.astype("int32")).to(dev),
                            torch.from_numpy(m.indices.astype("int32")).to(dev),
                            torch.from_numpy(m.data.astype("float32")).to(dev), m.shape[1], chunk)

    # ---- per-wave id streams -------------------------------------------
    def build_streams(self, n_waves=0, lmax=0):
        """Sliced-ELL copy of the id stream for the gather waves of the pipelined backward (``acm_csr_build_streams``):
        one-off host-side preprocessing, pattern-only operators only, idempotent.  Returns True when the streams exist."""
        if self.stream_steps:
            return True
        if self._ptrs[2]:                                  # explicit values: the kernels keep the CSR walk
            return False
        with _device_ctx(self.device):
            _sync(self.device)
            st = _lib.load().acm_csr_build_streams(self._h, int(n_waves), int(lmax))
        _lib.check(st, "acm_csr_build_streams")
        info = _lib.CsrInfo()
        _lib.check(_lib.load().acm_csr_info(self._h, C.byref(info)), "acm_csr_info")
        self.stream_steps, self.stream_waves = info.stream_steps, info.stream_waves
        self.stream_slices, self.stream_long_rows = info.stream_slices, info.stream_long_rows
        return True

    def build_item_streams(self, n_waves=0):
        """Per-wave batch streams over the handle's own work items (``acm_csr_build_item_streams``) for the mask form of
        the ACMII first layer: one-off host-side preprocessing, pattern-only operators only, idempotent.  Returns True
        when they exist."""
        if getattr(self, "item_stream_waves", 0):
            return True
        if self._ptrs[2] or self.nnz == 0:
            return False
        with _device_ctx(self.device):
            _sync(self.device)
            st = _lib.load().acm_csr_build_item_streams(self._h, int(n_waves))
        if st == 4:                                        # ACM_EUNSUPPORTED: the caller keeps the other form
            return False
        _lib.check(st, "acm_csr_build_item_streams")
        info = _lib.CsrInfo()
        _lib.check(_lib.load().acm_csr_info(self._h, C.byref(info)), "acm_csr_info")
        self.item_stream_waves = info.item_stream_waves
        return self.item_stream_waves > 0

    def build_loss_rows(self, keep):
        """The loss-row attachment of a square operator (``acm_csr_build_loss_rows``): ``keep`` is a uint8 device tensor of
        n_rows entries, non-zero = the row carries weight in the loss; the handle gets a work list over those rows alone.
        One-off host-side preprocessing: it synchronises the device and must not run while a stream is capturing.  Calling
        it again REPLACES the attachment -- a captured graph that walks the earlier one must not be replayed afterwards.
        Returns the dict of ``acm_csr_loss_rows_info`` (kept_rows, items, slots, kept_edges), or None where the library has
        no such entry point or the operator is not square."""
        lib = _lib.load()
        build, info = getattr(lib, "acm_csr_build_loss_rows", None), getattr(lib, "acm_csr_loss_rows_info", None)
        if build is None or info is None or self.n_rows != self.n_cols:
            return None
        if keep.dtype != torch.uint8 or keep.numel() != self.n_rows or not keep.is_contiguous():
            raise ValueError("build_loss_rows: keep must be a contiguous uint8 tensor of n_rows entries")
        _require_cuda(keep, "keep")
        with _device_ctx(self.device):
            _sync(self.device)
            _lib.check(build(self._h, keep.data_ptr()), "acm_csr_build_loss_rows")
            out = (C.c_int64 * 4)()
            _lib.check(info(self._h, out), "acm_csr_loss_rows_info")
        return dict(zip(("kept_rows", "items", "slots", "kept_edges"), (int(v) for v in out)))

    # ---- derived operators ----------------------------------------------
    def transpose(self):
        if self._transposed is None:
            out = C.c_void_p()
            with _device_ctx(self.device):
                _lib.check(_lib.load().acm_csr_transpose(self._h, 0, C.byref(out)), "acm_csr_transpose")
            self._transposed = CsrGraph(out.value, self.device)
        return self._transposed

    def slice_rows(self, begin, end):
        out = C.c_void_p()
        with _device_ctx(self.device):
            _lib.check(_lib.load().acm_csr_slice_rows(self._h, int(begin), int(end), 0, C.byref(out)),
                       "acm_csr_slice_rows")
        return CsrGraph(out.value, self.device)

    # ---- views (tests, sharding) -----------------------------------------
    def arrays(self):
        """(indptr, indices, vals) copied out to new torch tensors (vals is None for a
        pattern-only operator)."""
        _sync(self.device)
        return (_copy_from_ptr(self._ptrs[0], self.n_rows + 1, torch.int32, self.device),
                _copy_from_ptr(self._ptrs[1], self.nnz, torch.int32, self.device),
                _copy_from_ptr(self._ptrs[2], self.nnz, torch.float32, self.device) if self._ptrs[2] or not self.nnz
                else None)

    @property
    def pattern_only(self):
        return self.nnz > 0 and not self._ptrs[2]

    @property
    def src_pos(self):
        """For a transposed handle: int64 index tensor with vals_T = vals_source[src_pos]."""
        if self._src_pos is None:
            if not self._src_pos_ptr:
                raise RuntimeError("src_pos exists only on handles made by transpose()")
            _sync(self.device)
            self._src_pos = _copy_from_ptr(self._src_pos_ptr, self.nnz, torch.int32, self.device).to(torch.int64)
        return self._src_pos

    def workspace(self, width):
        nbytes = C.c_size_t()
        _lib.check(_lib.load().acm_spmm_workspace_bytes(self._h, int(width), C.byref(nbytes)),
                   "acm_spmm_workspace_bytes")
        n = max(nbytes.value // 4, 1)
        return torch.empty(n, dtype=torch.float32, device=self.device)

    @property
    def handle(self):
        return self._h

    def __repr__(self):
        return (f"CsrGraph({self.n_rows}x{self.n_cols}, nnz={self.nnz}, items={self.n_items}, "
                f"long_rows={self.n_long_rows}, max_degree={self.max_degree})")


class SparseFeatures:
    """Node features X (n x F_in) as CSR for the wide, sparse inputs (bag-of-words, one-hot): the
    structure lives in a CsrGraph handle (and its transpose, for dW = X^T dZ), the values in a separate
    tensor so that input dropout can rescale them every step without touching the handle.
    The projection then costs nnz(X) * 3F FMAs instead of N * F_in * 3F."""

    def __init__(self, csr, values):
        self.csr, self.values = csr, values
        self.shape = (csr.n_rows, csr.n_cols)
        self.device = csr.device

    @classmethod
    def from_scipy(cls, mat, device):
        m = mat.tocsr()
        m.sort_indices()
        csr = CsrGraph.from_scipy(m, device)
        return cls(csr, torch.from_numpy(m.data.astype("float32")).to(torch.device(device)))

    @classmethod
    def from_torch(cls, x):
        """Dense or torch-sparse feature matrix -> SparseFeatures (exact zeros are dropped)."""
        csr = CsrGraph.from_torch(x if x.layout != torch.strided else x.to_sparse())
        return cls(csr, csr.arrays()[2])

    @classmethod
    def auto(cls, x, min_cols=None):
        """A wide, mostly-zero DENSE feature matrix -> its CSR twin, made once per tensor; anything else is returned as is.

        The reference's loaders hand every data set over dense (ACM-Geometric/train.py:66-67: ``dataset.graph["node_feat"]``
        -- Penn94's one-hot block is [41 554, 4 814] with 0.1 % of the entries set; ACM-Pytorch/utils.py densifies Cora's
        bag of words), so a caller of the drop-in never builds SparseFeatures himself.  The projection of such an input
        costs nnz(X) * 3F FMAs from the CSR copy instead of N * F_in * 3F (Penn94-shaped ACM-GCN+ step: 2.33 -> 0.41 ms).
        Taken for: a strided 2-D fp32 CUDA tensor that needs no gradient, of at least ``tuning.HOST.csr_features``
        columns, with at most 1/16 of its entries nonzero (one count per tensor object and version: the answer -- the
        twin or the refusal -- is kept on the tensor itself, so the loop that passes the same ``features`` every epoch pays
        one lookup).  Never inside a stream capture (the count synchronises)."""
        if min_cols is None:
            from . import tuning
            min_cols = tuning.HOST.csr_features
        if (min_cols <= 0 or not isinstance(x, torch.Tensor) or x.layout != torch.strided or x.dim() != 2
                or x.dtype != torch.float32 or x.requires_grad or x.shape[1] < min_cols or x.shape[0] == 0):
            return x
        try:
            _require_cuda(x, "features")
        except RuntimeError:
            return x
        memo = getattr(x, "_acm_csr_twin", None)
        if memo is not None and memo[0] == x._version:
            return x if memo[1] is None else memo[1]
        if x.is_cuda and torch.cuda.is_current_stream_capturing():
            return x
        twin = None
        if int(torch.count_nonzero(x)) * 16 <= x.numel():
            twin = cls.from_torch(x.detach())
        x._acm_csr_twin = (x._version, twin)
        return x if twin is None else twin

    @staticmethod
    def known_twin(x):
        """The twin ``auto`` already made for this very tensor object (and version), or None -- a lookup, no device work."""
        memo = getattr(x, "_acm_csr_twin", None) if isinstance(x, torch.Tensor) else None
        return memo[1] if (memo is not None and memo[0] == x._version) else None

    def twin_of_masked(self, x):
        """``x`` = this matrix with some entries zeroed and the others rescaled (the caller's ``F.dropout`` of the
        features, a NEW dense tensor every step: ACM-Geometric/models.py:54, ACM-Pytorch/models/models.py:70) -> the
        same structure with x's values at the stored positions, or None when x has a nonzero entry outside the structure
        (it is then not a masked copy of this matrix).  The check reads x once and costs one small device-to-host copy."""
        if tuple(x.shape) != tuple(self.shape) or not x.is_contiguous():
            return None
        flat = getattr(self, "_flat_index", None)
        if flat is None:
            ip, ix, _ = self.csr.arrays()
            ip = ip.to(torch.int64)
            rows = torch.repeat_interleave(torch.arange(self.shape[0], device=ip.device), ip[1:] - ip[:-1])
            flat = self._flat_index = rows * self.shape[1] + ix.to(torch.int64)
        vals = x.reshape(-1).index_select(0, flat)
        if flat.numel() < (1 << 24):
            # the L0 "norm" is the nonzero count as an fp32 sum of ones: exact below 2^24 and never below 2^24 for a larger
            # true count (sums of positive terms round monotonically), so it equals the count over the stored positions
            # only if x has no entry elsewhere.  One streaming pass at 0.23 ms for Penn94's 200 M entries, where
            # torch.count_nonzero takes 1.08 ms (scripts/micro/probe_support_check.py)
            same = bool(torch.linalg.vector_norm(x, 0) == torch.linalg.vector_norm(vals, 0))
        else:
            same = int(torch.count_nonzero(x) - torch.count_nonzero(vals)) == 0
        if not same:
            return None
        out = self.with_values(vals)
        out._flat_index = flat
        return out

    def with_values(self, values):
        if values.shape != self.values.shape:
            raise ValueError("values must keep the CSR order and length")
        out = SparseFeatures(self.csr, values)
        out._perm_cache = getattr(self, "_perm_cache", None)       # same structure: the permuted twin can be shared
        return out

    def permute_rows(self, perm):
        """Rows reordered as new row r = old row perm[r] (structure built once per permutation and cached; the values
        follow through an index map, so per-step value changes -- input dropout -- cost one gather)."""
        cache = getattr(self, "_perm_cache", None)
        if cache is None or cache[0] != perm.data_ptr():
            ip, ix, _ = self.csr.arrays()
            ip = ip.to(torch.int64)
            counts = (ip[1:] - ip[:-1]).index_select(0, perm)
            new_ip = torch.zeros(perm.numel() + 1, dtype=torch.int64, device=ip.device)
            new_ip[1:] = torch.cumsum(counts, 0)
            # position of every entry of the permuted matrix in the original value array
            start = ip[:-1].index_select(0, perm)
            pos = torch.repeat_interleave(start - new_ip[:-1], counts) + torch.arange(int(new_ip[-1]), device=ip.device)
            csr = CsrGraph.from_csr(new_ip.to(torch.int32), ix.index_select(0, pos), None, self.csr.n_cols)
            cache = (perm.data_ptr(), csr, pos)
            self._perm_cache = cache
        out = SparseFeatures(cache[1], self.values.index_select(0, cache[2]))
        return out

    @property
    def csr_t(self):
        return self.csr.transpose()


class LossRows:
    """What FilterOperators.loss_rows attached to the forward handle for one row-weight tensor: ``keep`` (uint8, 1 = the row
    carries weight), the counts acm_csr_loss_rows_info reports (``fwd``: kept_rows, items, slots, kept_edges) and the key
    (data_ptr, _version, numel) of the weights."""
    __slots__ = ("key", "keep", "fwd", "__weakref__")

    def __init__(self, key, keep, fwd):
        self.key, self.keep, self.fwd = key, keep, fwd

    def current_for(self, weights):
        return self.key == (weights.data_ptr(), weights._version, weights.numel())

    def __repr__(self):
        return f"LossRows(kept_rows={self.fwd['kept_rows']}, items={self.fwd['items']}, kept_edges={self.fwd['kept_edges']})"


class FilterOperators:
    """What one ACM layer needs from the graph, for the rows this process owns."""

    def __init__(self, low, deg=None, row_offset=0, n_global=None, group=None, row_scale=None):
        self.low = low                                  # A_low rows (local) x columns (global)
        self._low_t = None
        # implicit form A_low = diag(row_scale) P: ``low`` is then the pattern-only operator P (symmetric), which
        # also serves A_low^T G = P (diag(row_scale) G); see implicit_form() / as_implicit()
        self.row_scale = row_scale
        self.self_scale = (1.0 / row_scale) if row_scale is not None else None
        self.deg = deg                                  # d_i for local rows, or None
        self.inv_deg = (1.0 / deg) if deg is not None else None
        self.row_offset = int(row_offset)
        self.n_global = int(n_global if n_global is not None else low.n_cols)
        self.group = group                              # torch.distributed group when row-sharded
        self.plan = None                                # distributed.ShardPlan when row-sharded (halo numbering)
        # in-operator relabelling (relabel_by_degree): the operator lives in a node numbering sorted by decreasing
        # degree; perm[new] = old, inv_perm[old] = new (int64 device tensors).  None: the caller's numbering.
        self.perm = None
        self.inv_perm = None
        self.low_t_override = None                      # local rows of the global A_low^T (sharded)
        # optional, row-sharded runs: the full (replicated, static) input matrix.  With counter-based dropout every
        # rank can then produce the dropped input of ALL nodes itself and the first layer needs no halo all-gather
        self.x_full = None
        self._pregathered = None
        # low-pass hops of the ACM-SGC layer: A_low^hops on the low channel as a chain of 1-hop products (the
        # reference materialises the dense power, ACM-Pytorch/utils.py:631-637); adj_high stays 1-hop
        self.hops = 1
        # general operator pair (adj_high != I - adj_low, or adj_un != D adj_low - I): see operators_for()
        self.general = False
        self.high = None                                # CsrGraph of adj_high
        self.un = None                                  # CsrGraph of adj_low_unnormalized
        self._eye = None
        self._zeros = {}
        self._loss_rows = None                          # weak reference to the live LossRows of these operators (loss_rows())

    @property
    def implicit(self):
        return self.row_scale is not None

    @property
    def low_t(self):
        if self.low_t_override is not None:
            return self.low_t_override
        if self.implicit:
            return self.low                             # P is symmetric: the same column-id stream both ways
        if self._low_t is None:
            self._low_t = self.low.transpose()
        return self._low_t

    def loss_rows(self, weights, replaces=None):
        """The loss-row attachment of these operators for the row weights ``weights`` (rows of weight 0 carry no loss): the
        work list over the weighted rows, on ``low``.  Cached per weights tensor (``data_ptr`` and ``_version``); the caller keeps the returned
        LossRows alive for as long as it launches over it.

        A handle carries ONE attachment, and a captured graph keeps the addresses of the one it was captured over: while a
        LossRows for other weights is alive, a second request is refused (None) unless the caller hands its own object over as
        ``replaces`` (an eager step whose weights changed).  None also for sharded / general operators, non-square operators
        and libraries without the entry points.  Synchronises the device; never call it while a stream is capturing."""
        if self.sharded or self.general or weights.numel() != self.low.n_rows:
            return None
        key = (weights.data_ptr(), weights._version, weights.numel())
        cur = self._loss_rows() if self._loss_rows is not None else None
        if cur is not None and cur.key == key:
            return cur
        if cur is not None and cur is not replaces:
            return None
        keep = (weights.detach().reshape(-1) != 0).to(torch.uint8).contiguous()
        fwd = self.low.build_loss_rows(keep)
        if fwd is None:
            return None
        out = LossRows(key, keep, fwd)
        self._loss_rows = weakref.ref(out)
        return out

    @property
    def n_local(self):
        return self.low.n_rows

    @property
    def eye(self):
        """Identity operator: lets the fused kernels run as pure row-local epilogues in the general path."""
        if self._eye is None:
            n, dev = self.low.n_rows, self.low.device
            ar = torch.arange(n + 1, dtype=torch.int32, device=dev)
            self._eye = CsrGraph.from_csr(ar, ar[:n].clone(), torch.ones(n, device=dev), n)
        return self._eye

    def zeros(self, n, f):
        key = (n, f)
        if key not in self._zeros:
            self._zeros[key] = torch.zeros(n, f, dtype=torch.float32, device=self.low.device)
        return self._zeros[key]

    @property
    def sharded(self):
        return self.group is not None

    @property
    def n_gathered(self):
        """Rows of an all-gathered halo table (= columns of the local operators): world * the longest block."""
        return self.plan.n_gathered if self.plan is not None else self.n_global

    @property
    def uniform(self):
        """All ranks own equally many rows: the halo numbering is the global numbering."""
        return self.plan is None or self.plan.uniform


# --------------------------------------------------------------------------
# implicit (pattern-only) form of the low-pass filter
# --------------------------------------------------------------------------
def implicit_form(indptr, indices, vals, n_rows, n_cols, max_multiplicity=4):
    """A (rows sorted by column) = diag(s) P with P a symmetric 0/1/2.. pattern?  -> (indptr_P, indices_P, s) or None.

    The reference's low-pass filter is D^-1 (I + A) (ACM-Geometric/utils.py:5-18, train.py:75-81): one value
    per row, except that a raw self-loop makes the diagonal of I + A count twice -- P then
    lists that column twice.  With s_i = min of row i, every entry must be an exact small integer multiple of
    s_i (fp32(2/d) == 2 * fp32(1/d) bit for bit) and P must equal its transpose as a multiset, so that
        A G = diag(s) (P G)           A^T G = P (diag(s) G).
    Works on CPU or device tensors (torch primitives only; one-off preprocessing)."""
    if n_rows != n_cols or indices.numel() == 0:
        return None
    dev = indptr.device
    ip = indptr.to(torch.int64)
    counts = ip[1:] - ip[:-1]
    rows = torch.repeat_interleave(torch.arange(n_rows, device=dev), counts)
    v = vals.to(torch.float32)
    if bool((v <= 0).any()):
        return None
    s = torch.full((n_rows,), float("inf"), dtype=torch.float32, device=dev).scatter_reduce(0, rows, v, "amin")
    s = torch.where(torch.isinf(s), torch.ones_like(s), s)
    m = v / s[rows]
    mr = m.round()
    if bool(((mr < 1) | (mr > max_multiplicity) | (m != mr)).any()):
        return None
    mult = mr.to(torch.int64)
    cols = indices.to(torch.int64)
    keys, perm = torch.sort(rows * n_cols + cols)
    keys_t, perm_t = torch.sort(cols * n_cols + rows)
    if not bool(torch.equal(keys, keys_t)) or not bool(torch.equal(mult[perm], mult[perm_t])):
        return None
    if bool((keys[1:] == keys[:-1]).any()):
        return None                                     # un-coalesced input: not handled here
    if bool((mult == 1).all()):
        return indptr.to(torch.int32), indices.to(torch.int32), s
    new_counts = torch.zeros(n_rows, dtype=torch.int64, device=dev).index_add_(0, rows, mult)
    new_ip = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    new_ip[1:] = torch.cumsum(new_counts, 0)
    return new_ip.to(torch.int32), torch.repeat_interleave(cols, mult).to(torch.int32), s


def as_implicit(ops):
    """Replace an explicit single-process FilterOperators by its pattern-only form when A_low allows it
    (otherwise return ``ops`` unchanged).  ``tuning.HOST.implicit = 0`` keeps the explicit value stream."""
    from . import tuning
    if ops.implicit or ops.general or ops.sharded or not tuning.HOST.implicit:
        return ops
    ip, ix, v = ops.low.arrays()
    form = implicit_form(ip, ix, v, ops.low.n_rows, ops.low.n_cols)
    if form is None:
        return ops
    pat = CsrGraph.from_csr(form[0], form[1], None, ops.low.n_cols, ops.low.chunk)
    out = FilterOperators(pat, ops.deg, row_scale=form[2].contiguous())
    out.hops = ops.hops
    return out


# --------------------------------------------------------------------------
# verification of the identities the fused kernel relies on
# --------------------------------------------------------------------------
def _spmm_raw(graph, dense):
    from .functional import spmm
    return spmm(graph, dense)


def verify_high_is_identity_minus_low(low, adj_high, tol=1e-5):
    """adj_high must equal I - adj_low (ACM-Geometric/train.py:78, ACM-Pytorch/utils.py:622)."""
    if adj_high is None:
        return True
    high = CsrGraph.from_torch(adj_high)
    if (high.n_rows, high.n_cols) != (low.n_rows, low.n_cols) or low.n_rows != low.n_cols:
        return False
    gen = torch.Generator(device="cpu").manual_seed(1234)
    r = torch.randn(low.n_cols, 4, generator=gen).to(low.device)
    lhs = _spmm_raw(high, r)
    rhs = r - _spmm_raw(low, r)
    return bool(torch.allclose(lhs, rhs, rtol=tol, atol=tol))


def degree_from_unnormalized(low, adj_un, tol=1e-4):
    """d = 1 + rowsum(A) and a check that A = D A_low - I (train.py:76-77)."""
    un = CsrGraph.from_torch(adj_un)
    ones = torch.ones(un.n_cols, 1, device=low.device)
    deg = (_spmm_raw(un, ones) + 1.0).reshape(-1).contiguous()
    gen = torch.Generator(device="cpu").manual_seed(4321)
    r = torch.randn(low.n_cols, 4, generator=gen).to(low.device)
    lhs = _spmm_raw(un, r)
    rhs = deg[:, None] * _spmm_raw(low, r) - r
    ok = bool(torch.allclose(lhs, rhs, rtol=tol, atol=tol * float(deg.max())))
    return deg, ok


# --------------------------------------------------------------------------
# filter construction on the device, and the on-disk operator cache
# --------------------------------------------------------------------------
def filters_from_edge_index(edge_index, n, undirected=True, chunk=0):
    """edge list -> A_low = D^-1 (I + A) as a device CSR operator (+ d = rowsum(I + A)), entirely on the GPU.

    Restates ACM-Geometric/train.py:66-81 (to_undirected -> scipy A -> normalize_tensor(I + A) in float64 ->
    float32): duplicate edges collapse to one (to_undirected coalesces), a raw self-loop makes the diagonal
    2/d_i (quirk Q5), rows are sorted by column.  The float64-then-cast values of the reference equal the fp32
    quotients computed here bit for bit (double rounding is innocuous for division when 53 >= 2*24 + 2).
    The sort / unique passes are torch's device primitives (one-off preprocessing)."""
    _require_cuda(edge_index, "edge_index")
    dev = edge_index.device
    src, dst = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    if undirected:
        src, dst = torch.cat([src, dst]), torch.cat([dst, src])
    eye = torch.arange(n, device=dev, dtype=torch.int64)
    keys = torch.cat([src * n + dst, eye * n + eye])            # (I + A): the identity joins the edge list
    uniq, counts = torch.unique(keys, return_counts=True)       # sorted by (row, col); self-loop + identity -> 2
    rows, cols = uniq // n, uniq % n
    w = torch.where(rows == cols, counts.clamp(max=2), torch.ones_like(counts)).to(torch.float32)
    deg = torch.zeros(n, dtype=torch.float32, device=dev).index_add_(0, rows, w)
    vals = w / deg[rows]
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    low = CsrGraph.from_csr(indptr.to(torch.int32), cols.to(torch.int32), vals, n, chunk)
    return as_implicit(FilterOperators(low, deg))


def explicit_arrays(ops):
    """(indptr, indices, vals) of A_low itself, whichever form ``ops`` holds (duplicates of the implicit
    pattern are merged back into one entry)."""
    ip, ix, v = ops.low.arrays()
    if not ops.implicit:
        return ip, ix, v
    n = ops.low.n_rows
    counts = (ip[1:] - ip[:-1]).to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(n, device=ip.device), counts)
    keys, mult = torch.unique_consecutive(rows * ops.low.n_cols + ix.to(torch.int64), return_counts=True)
    r, c = keys // ops.low.n_cols, keys % ops.low.n_cols
    new_ip = torch.zeros(n + 1, dtype=torch.int64, device=ip.device)
    new_ip[1:] = torch.cumsum(torch.bincount(r, minlength=n), 0)
    return new_ip.to(torch.int32), c.to(torch.int32), mult.to(torch.float32) * ops.row_scale[r]


def save_operators(path, ops):
    """On-disk cache of a FilterOperators: numpy .npz with int32 indptr / indices, fp32 vals and d."""
    import numpy as np
    ip, ix, v = (t.cpu().numpy() for t in explicit_arrays(ops))
    np.savez_compressed(path, indptr=ip, indices=ix, vals=v, n_cols=np.int64(ops.low.n_cols),
                        deg=ops.deg.cpu().numpy() if ops.deg is not None else np.zeros(0, np.float32))


def load_operators(path, device):
    import numpy as np
    with np.load(path) as f:
        dev = torch.device(device)
        low = CsrGraph.from_csr(torch.from_numpy(f["indptr"]).to(dev), torch.from_numpy(f["indices"]).to(dev),
                                torch.from_numpy(f["vals"]).to(dev), int(f["n_cols"]))
        deg = torch.from_numpy(f["deg"]).to(dev) if f["deg"].size else None
    return as_implicit(FilterOperators(low, deg))


def relabel_by_degree(ops, force=False):
    """The same operators in a node numbering sorted by decreasing degree (ties by id): returns a FilterOperators with
    ``perm`` / ``inv_perm`` set, or ``ops`` itself when the rows already are in that order (or the operator pair is
    general / sharded).  Hubs become the first rows of every gathered table, so the rows most edges point at share
    cache lines and stay L2-resident: 0.44 -> 0.36 ms per training step on the twitch-shaped graph with random ids.
    bench.py applies the relabelling as data preparation; here it is part of the operator, so a caller that hands over
    the reference's tensors unchanged (operators_for, the drop-in route) gets it too -- layers.GraphConvolution /
    models.GCN / train.TrainStep translate rows at the boundary."""
    if ops.perm is not None or ops.general or ops.sharded:
        return ops
    ip, ix, v = explicit_arrays(ops)
    n = ops.low.n_rows
    if n != ops.low.n_cols:
        return ops
    deg = (ip[1:] - ip[:-1]).to(torch.int64)
    if not force and bool((deg[1:] <= deg[:-1]).all()):
        return ops                                      # already sorted by degree
    perm = torch.sort(deg, descending=True, stable=True).indices
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n, device=perm.device)
    counts = deg.index_select(0, perm)
    new_ip = torch.zeros(n + 1, dtype=torch.int64, device=ip.device)
    new_ip[1:] = torch.cumsum(counts, 0)
    start = ip.to(torch.int64)[:-1].index_select(0, perm)
    pos = torch.repeat_interleave(start - new_ip[:-1], counts) + torch.arange(int(new_ip[-1]), device=ip.device)
    rows = torch.repeat_interleave(torch.arange(n, device=ip.device), counts)
    cols = inv.index_select(0, ix.to(torch.int64).index_select(0, pos))
    order = torch.sort(rows * n + cols).indices         # columns ascending inside every row
    low = CsrGraph.from_csr(new_ip.to(torch.int32), cols.index_select(0, order).to(torch.int32),
                            v.index_select(0, pos).index_select(0, order), n, ops.low.chunk)
    out = as_implicit(FilterOperators(low, ops.deg.index_select(0, perm) if ops.deg is not None else None))
    out.hops = ops.hops
    out.perm, out.inv_perm = perm, inv
    return out


def _want_relabel(n):
    from . import tuning
    mode = tuning.HOST.relabel                       # -1: by size, 0: never, 1: always
    return mode == 1 or (mode < 0 and n >= 32768)


_CACHE = {}
_CACHE_LIMIT = 16


def _key(t):
    if t is None:
        return None
    if t.layout == torch.sparse_coo:
        v = t._values()
        return ("coo", v.data_ptr(), t._indices().data_ptr(), t._nnz(), tuple(t.shape), str(t.device))
    if t.layout == torch.sparse_csr:
        return ("csr", t.values().data_ptr(), t.col_indices().data_ptr(), tuple(t.shape), str(t.device))
    return ("dense", t.data_ptr(), tuple(t.shape), tuple(t.stride()), str(t.device))


def _source_state(t):
    """(weak reference, version counter) of a source tensor: the cache entry is valid only while the tensor it was
    built from is alive (its address cannot have been handed to another tensor) and unmodified (in-place edits bump
    the version counter, which views / detach() / the values of a sparse tensor share)."""
    if t is None:
        return None
    payload = t._values() if t.layout == torch.sparse_coo else (t.values() if t.layout == torch.sparse_csr else t)
    return weakref.ref(t), payload._version


def _source_valid(state, t):
    if state is None:
        return t is None
    if t is None:
        return False
    ref, version = state
    src = ref()
    if src is None:
        return False
    payload = t._values() if t.layout == torch.sparse_coo else (t.values() if t.layout == torch.sparse_csr else t)
    # `t` may be another wrapper of the live source's storage (same key => same address, shape, nnz)
    return payload._version == version


def operators_for(adj_low, adj_high=None, adj_low_unnormalized=None, verify=True):
    """Convert the reference's adjacency tensors once; cached by storage identity.  A hit is honoured only if every
    tensor the entry was built from is still alive and has not been written to since (otherwise a freed adjacency's
    address reused by a new one of the same shape / nnz, or an in-place re-normalisation, would silently get the
    stale operators)."""
    if isinstance(adj_low, FilterOperators):
        return adj_low
    sources = (adj_low, adj_high, adj_low_unnormalized)
    key = tuple(_key(t) for t in sources)
    hit = _CACHE.get(key)
    if hit is not None:
        ops, states = hit
        if all(_source_valid(st, t) for st, t in zip(states, sources)):
            return ops
        del _CACHE[key]
    for k in [k for k, (_, states) in _CACHE.items() if any(st is not None and st[0]() is None for st in states)]:
        del _CACHE[k]                                   # entries whose source tensors died
    _require_cuda(adj_low, "adj_low")
    low = CsrGraph.from_torch(adj_low)
    fused_ok = (not verify) or verify_high_is_identity_minus_low(low, adj_high)
    deg = None
    if fused_ok and adj_low_unnormalized is not None:
        deg, ok = degree_from_unnormalized(low, adj_low_unnormalized)
        fused_ok = ok or not verify
    if fused_ok:
        ops = as_implicit(FilterOperators(low, deg))
        if _want_relabel(low.n_rows):
            ops = relabel_by_degree(ops)
    else:
        # General operator pair: the filters are not (A_low, I - A_low[, D A_low - I]) -- e.g. the
        # reference's k-hop ACM-SGC passes A_low^k with an un-powered adj_high
        # (ACM-Pytorch/utils.py:631-637).  Each channel then gets its own plain SpMM and the fused
        # kernels run over the identity operator as row-local epilogues (the ``general`` branches of
        # functional/conv_literal.py: _AcmLiteral.forward, _literal_backward).
        ops = FilterOperators(low, None)
        ops.general = True
        ops.high = CsrGraph.from_torch(adj_high) if adj_high is not None else None
        ops.un = CsrGraph.from_torch(adj_low_unnormalized) if adj_low_unnormalized is not None else None
        if ops.high is None:
            raise ValueError("adj_high is required when it cannot be derived from adj_low")
    if len(_CACHE) >= _CACHE_LIMIT:
        _CACHE.pop(next(iter(_CACHE)))
    _CACHE[key] = (ops, tuple(_source_state(t) for t in sources))
    return ops


def clear_cache():
    _CACHE.clear()
