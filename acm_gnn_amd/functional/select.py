"""Model selection and early stopping kept on the device across epochs (acm_select_step, acm_copy_if): the state of one
training run -- epoch counter, stop flag, best key, selected test metric, the per-epoch history -- and, optionally, a snapshot
of the parameters at the selected epoch."""
import ctypes as C

import torch

from .. import _lib
from ._launch import _F32, _check_device, _vp, launch

RULES = ("max_val_acc", "min_val_loss")          # acm_select_t.rule 0 / 1: train.fit's two selection rules
_CTRL_EPOCH, _CTRL_STOPPED, _CTRL_BEST_EPOCH, _CTRL_IMPROVED = range(4)


def copy_if(pairs, flag, table=None):
    """``dst <- src`` (bitwise) for every ``(src, dst)`` of ``pairs`` if the device int32 ``flag[0]`` is non-zero, nothing
    otherwise -- decided on the device (acm_copy_if; capturable).  Tensors of 32-bit elements, contiguous, same element count
    per pair.  ``table``: the ``_lib.CopyTensor`` array of an earlier :func:`copy_table` for the same pairs."""
    _check_device(flag, "flag")
    if flag.dtype != torch.int32 or flag.numel() < 1:
        raise ValueError("copy_if: flag must be an int32 tensor")
    if table is None:
        table = copy_table(pairs, flag.device)
    launch("acm_copy_if", f"copy_if/{len(table)}", flag.device, len(table), C.cast(table, C.c_void_p) if len(table) else None, _vp(flag))


def copy_table(pairs, device):
    table = (_lib.CopyTensor * len(pairs))()
    for e, (src, dst) in zip(table, pairs):
        for t, name in ((src, "src"), (dst, "dst")):
            _check_device(t, name)
            if t.element_size() != 4 or not t.is_contiguous() or t.device != device:
                raise ValueError(f"copy_if: {name} must be a contiguous tensor of 32-bit elements on {device}")
        if src.numel() != dst.numel():
            raise ValueError(f"copy_if: {src.numel()} source elements, {dst.numel()} destination elements")
        e.src, e.dst, e.numel = src.data_ptr(), dst.data_ptr(), src.numel()
    return table


class SelectionState:
    """The device-resident state of one run of ``train.fit``'s epoch loop.

    ``ctrl`` int32[8] = (epoch, stopped, best_epoch, improved, 0, 0, 0, 0), ``best`` float64[2] = (best_key, selected),
    ``history`` float64[epochs, 5] = (train loss, metric on train / validation / test, validation loss) per epoch.  ``launch``
    folds one epoch in (acm_select_step restates the host loop: same values, bit for bit); once the run has stopped, or the
    budget of ``epochs`` rows is used up, further launches change nothing but ``improved`` = 0.

    ``params`` (keep the best): the tensors to snapshot whenever an epoch is selected (``buffers``: further fp32 tensors kept
    with them, the model's floating-point buffers) -- one flat fp32 allocation with a view per tensor, filled by a copy predicated on ``improved`` (acm_copy_if) right behind the selection launch."""

    def __init__(self, rule, early_stopping, epochs, device, params=None, buffers=None):
        if rule not in RULES:
            raise ValueError(f"rule must be one of {RULES}, not {rule!r}")
        if int(epochs) < 1 or int(early_stopping) < 0:
            raise ValueError("SelectionState: epochs must be >= 1 and early_stopping >= 0")
        self.rule, self.early_stopping, self.epochs = RULES.index(rule), int(early_stopping), int(epochs)
        self.device = torch.device(device)
        self.ctrl = torch.zeros(8, dtype=torch.int32, device=self.device)
        self.best = torch.zeros(2, dtype=torch.float64, device=self.device)
        self.history = torch.zeros(self.epochs, 5, dtype=torch.float64, device=self.device)
        self._ctrl0 = torch.tensor([0, 0, -1, 0, 0, 0, 0, 0], dtype=torch.int32, device=self.device)
        self.params, self.snapshot, self._table = None, None, None
        if params is not None:
            self.params = list(params)
            self._n_owned = len(self.params)                 # restore(model) checks these against model.parameters()
            self.params += list(buffers or ())               # (``buffers``: snapshotted and restored with them, e.g. BatchNorm's
            for p in self.params:                            #  running statistics -- what an evaluation pass reads beside the weights)
                _check_device(p, "parameter")
                if p.dtype != _F32 or not p.is_contiguous() or p.device != self.device:
                    raise ValueError(f"SelectionState: parameters must be contiguous fp32 tensors on {self.device}")
            flat = torch.zeros(sum(p.numel() for p in self.params), dtype=_F32, device=self.device)
            self.snapshot, at = [], 0
            for p in self.params:
                self.snapshot.append(flat[at:at + p.numel()].view(p.shape))
                at += p.numel()
            self._flat = flat
            self._table = copy_table([(p.detach(), s) for p, s in zip(self.params, self.snapshot)], self.device)
        self.reset()

    def reset(self):
        """Back to the start of a run (not capturable: a torch copy)."""
        self.ctrl.copy_(self._ctrl0)
        self.best.zero_()

    def launch(self, loss, res):
        """Enqueue the epoch: ``loss`` the training step's fp32 scalar, ``res`` the evaluation pass's
        [m_tr, m_va, m_te, val_loss] (fp32 or float64).  With snapshots, the predicated copy follows."""
        for t, name in ((loss, "loss"), (res, "res")):
            if not isinstance(t, torch.Tensor):
                raise ValueError(f"SelectionState.launch: {name} must be a tensor")
            _check_device(t, name)
            if t.device != self.device or not t.is_contiguous():
                raise ValueError(f"SelectionState.launch: {name} must be contiguous on {self.device}")
        if loss.dtype != _F32 or loss.numel() != 1:
            raise ValueError("SelectionState.launch: loss must be one fp32 scalar")
        if res.dtype not in (_F32, torch.float64) or res.numel() != 4:
            raise ValueError("SelectionState.launch: res must hold four fp32 or float64 numbers")
        p = _lib.Select()
        p.rule, p.early_stopping, p.epochs = self.rule, self.early_stopping, self.epochs
        if res.dtype == _F32:
            p.result = res.data_ptr()
        else:
            p.result_f64 = res.data_ptr()
        p.train_loss = loss.data_ptr()
        p.ctrl, p.best, p.history = self.ctrl.data_ptr(), self.best.data_ptr(), self.history.data_ptr()
        launch("acm_select_step", "select_step", self.device, C.byref(p))
        if self._table is not None:
            copy_if(None, self.ctrl[_CTRL_IMPROVED:], self._table)

    def poll(self):
        """(epoch, stopped): epochs folded in so far and whether the run has stopped -- ONE small device-to-host copy, which
        waits for everything enqueued on the current stream."""
        epoch, stopped = self.ctrl[:2].tolist()
        return epoch, bool(stopped)

    def result(self):
        """(selected, history rows as tuples of Python floats, best_epoch); best_epoch is -1 and selected 0.0 if no epoch
        had a defined key."""
        ctrl = self.ctrl.tolist()
        selected = self.best.tolist()[1]
        rows = [tuple(r) for r in self.history[:ctrl[_CTRL_EPOCH]].tolist()]
        return selected, rows, ctrl[_CTRL_BEST_EPOCH]

    def restore(self, model=None):
        """Copy the snapshot back into the parameters IN PLACE (captured graphs and the optimizer's pointer tables keep their
        addresses).  Nothing to restore if no epoch was selected.  ``model``: checked to own exactly the snapshot's tensors."""
        if self.snapshot is None:
            raise RuntimeError("SelectionState.restore: the state keeps no snapshot (params=None)")
        if model is not None:
            mine = list(model.parameters())
            if len(mine) != self._n_owned or any(a is not b for a, b in zip(mine, self.params)):
                raise ValueError("SelectionState.restore: not the model whose parameters the snapshot holds")
        if self.ctrl.tolist()[_CTRL_BEST_EPOCH] < 0:
            return False
        with torch.no_grad():
            for p, s in zip(self.params, self.snapshot):
                p.copy_(s)
        return True


def _upload(table, host):
    """Device table <- host ctypes array (a stream-ordered copy; between two replays of a captured epoch, after the
    synchronising look at the runs' state)."""
    table.copy_(torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8))


class BatchMetrics:
    """``acm_eval_metrics`` for the slots of a batch of runs on one graph as ONE launch (acm_eval_metrics_batch): per-slot
    logits and set weights, labels shared or -- runs on different graphs of one row count -- per slot; results ``out[slot] = [m_tr, m_va, m_te, val_loss]`` and workspaces allocated as
    one block.  The per-slot argument blocks live in a device table, so a captured launch survives :meth:`set_slot`."""

    def __init__(self, n_slots, n_rows, n_classes, n_sets, labels, loss_set=1):
        _check_device(labels, "labels")
        if labels.dtype != torch.int64 or labels.dim() != 1 or labels.shape[0] != n_rows or not labels.is_contiguous():
            raise ValueError("BatchMetrics: labels must be a contiguous int64 [n] tensor")
        dev = labels.device
        self.n_slots, self.n, self.c, self.k, self.loss_set = int(n_slots), int(n_rows), int(n_classes), int(n_sets), int(loss_set)
        self.labels, self.device = labels, dev
        from ._launch import _workspace_bytes
        self._ws_bytes = _workspace_bytes("acm_eval_metrics_workspace_bytes", self.n, self.k)
        self.out = torch.zeros(self.n_slots, self.k + 1, dtype=_F32, device=dev)
        self.ws = torch.zeros(self.n_slots, (self._ws_bytes + 15) // 16 * 4, dtype=_F32, device=dev)
        self._host = (_lib.EvalMetricsSlot * self.n_slots)()
        self.table = torch.zeros(C.sizeof(self._host), dtype=torch.uint8, device=dev)
        self._keep = [None] * self.n_slots

    def set_slot(self, i, logits=None, weights=None, labels=None):
        """Slot ``i`` evaluates ``logits`` [n, C] on the sets ``weights`` [k, n] against ``labels`` (None: the shared tensor of
        the constructor); ``logits`` None: an empty slot.  :meth:`flush` uploads."""
        e = self._host[i]
        if logits is None:
            e.logits = e.weights = e.labels = e.out = e.workspace = None
            self._keep[i] = None
            return
        for t, name in ((logits, "logits"), (weights, "weights")):
            _check_device(t, name)
        if logits.dtype != _F32 or tuple(logits.shape) != (self.n, self.c) or not logits.is_contiguous() or logits.device != self.device:
            raise ValueError(f"BatchMetrics: logits must be contiguous fp32 [{self.n}, {self.c}] on {self.device}")
        if weights.dtype != _F32 or tuple(weights.shape) != (self.k, self.n) or not weights.is_contiguous() or weights.device != self.device:
            raise ValueError(f"BatchMetrics: weights must be contiguous fp32 [{self.k}, {self.n}] on {self.device}")
        if labels is None:
            labels = self.labels
        else:
            _check_device(labels, "labels")
            if labels.dtype != torch.int64 or tuple(labels.shape) != (self.n,) or not labels.is_contiguous() or labels.device != self.device:
                raise ValueError(f"BatchMetrics: a slot's labels must be a contiguous int64 [{self.n}] tensor on {self.device}")
        e.logits, e.weights, e.labels = logits.data_ptr(), weights.data_ptr(), labels.data_ptr()
        e.out, e.workspace = self.out[i].data_ptr(), self.ws[i].data_ptr()
        self._keep[i] = (logits, weights, labels)

    def flush(self):
        _upload(self.table, self._host)

    def launch(self):
        launch("acm_eval_metrics_batch", f"eval_metrics_batch/{self.n}x{self.c}k{self.k}b{self.n_slots}", self.device, self.n, self.c,
               self.c, self.n, self.k, self.loss_set, self.n_slots, _vp(self.table), self._ws_bytes)
        return self.out


class BatchSelection:
    """:class:`SelectionState` for the slots of a batch of runs: ``ctrl`` int32[B, 8], ``best`` float64[B, 2], ``history``
    float64[B, epochs, 5] allocated as one block each, folded by ONE launch per epoch (acm_select_step_batch: one block per
    slot, each the single kernel), looked at with ONE device-to-host copy (:meth:`poll`)."""

    def __init__(self, rule, early_stopping, epochs, n_slots, device):
        if rule not in RULES:
            raise ValueError(f"rule must be one of {RULES}, not {rule!r}")
        if int(epochs) < 1 or int(early_stopping) < 0:
            raise ValueError("BatchSelection: epochs must be >= 1 and early_stopping >= 0")
        self.rule, self.early_stopping, self.epochs = RULES.index(rule), int(early_stopping), int(epochs)
        self.n_slots, self.device = int(n_slots), torch.device(device)
        self.ctrl = torch.zeros(self.n_slots, 8, dtype=torch.int32, device=self.device)
        self.best = torch.zeros(self.n_slots, 2, dtype=torch.float64, device=self.device)
        self.history = torch.zeros(self.n_slots, self.epochs, 5, dtype=torch.float64, device=self.device)
        self._ctrl0 = torch.tensor([0, 0, -1, 0, 0, 0, 0, 0], dtype=torch.int32, device=self.device)
        self._host = (_lib.Select * self.n_slots)()
        self.table = torch.zeros(C.sizeof(self._host), dtype=torch.uint8, device=self.device)
        self._keep = [None] * self.n_slots

    def reset(self, i):
        """Slot ``i`` back to the start of a run (torch copies: not capturable)."""
        self.ctrl[i].copy_(self._ctrl0)
        self.best[i].zero_()

    def set_slot(self, i, train_loss=None, result=None):
        """Slot ``i`` folds (``train_loss`` fp32 scalar, ``result`` fp32 [4]) from the start of a run; None: an empty slot."""
        e = self._host[i]
        self.reset(i)
        if train_loss is None:
            e.result = e.result_f64 = e.train_loss = e.ctrl = e.best = e.history = None
            self._keep[i] = None
            return
        for t, name in ((train_loss, "train_loss"), (result, "result")):
            _check_device(t, name)
            if t.device != self.device or not t.is_contiguous() or t.dtype != _F32:
                raise ValueError(f"BatchSelection: {name} must be contiguous fp32 on {self.device}")
        if train_loss.numel() != 1 or result.numel() != 4:
            raise ValueError("BatchSelection: train_loss is one scalar, result holds four numbers")
        e.rule, e.early_stopping, e.epochs = self.rule, self.early_stopping, self.epochs
        e.result, e.result_f64, e.train_loss = result.data_ptr(), None, train_loss.data_ptr()
        e.ctrl, e.best, e.history = self.ctrl[i].data_ptr(), self.best[i].data_ptr(), self.history[i].data_ptr()
        self._keep[i] = (train_loss, result)

    def flush(self):
        _upload(self.table, self._host)

    def launch(self):
        launch("acm_select_step_batch", f"select_step_batch/{self.n_slots}", self.device, self.n_slots, _vp(self.table))

    def poll(self):
        """[(epoch, stopped)] of every slot: ONE device-to-host copy, which waits for what was enqueued on the current stream."""
        return [(c[_CTRL_EPOCH], bool(c[_CTRL_STOPPED])) for c in self.ctrl.tolist()]

    def result(self, i):
        """(selected, history rows, best_epoch) of slot ``i``, as :meth:`SelectionState.result`."""
        ctrl = self.ctrl[i].tolist()
        selected = self.best[i].tolist()[1]
        rows = [tuple(r) for r in self.history[i, :ctrl[_CTRL_EPOCH]].tolist()]
        return selected, rows, ctrl[_CTRL_BEST_EPOCH]
