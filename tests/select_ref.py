"""The loop body of ``train.fit`` (acm_gnn_amd/train.py: the default, host-side epoch loop and ``_selection_key``) restated in
plain Python over a given sequence of per-epoch numbers -- the referee of the device-resident selection state.  Written from
that loop, not from the kernel: ``history.append``; the key (None for NaN); ``key > best_key``; the window mean; ``break`` last.

The window mean.  The host loop writes ``sum(val_hist[epoch - es:epoch]) / es``.  Up to CPython 3.11 ``sum`` of floats is the plain
left-to-right float64 sum; from 3.12 on it is compensated (Neumaier), which can differ from the plain sum in the last bit.  The
contract of the device-resident state is the PLAIN sum in ascending epoch order, so it is spelled out below as a loop and does
not depend on the interpreter: on 3.12+ this restatement (and the kernel) can part from the host loop where a window's plain sum
is inexact and the current loss lies within a rounding error of the mean."""

RULES = ("max_val_acc", "min_val_loss")


def select_ref(rows, rule, early_stopping=0, epochs=None):
    """``rows``: (loss, m_tr, m_va, m_te, val_loss) per epoch, Python floats.  Returns (selected, history, best_epoch,
    stop_epoch): ``best_epoch`` -1 if no epoch was selected, ``stop_epoch`` the epoch whose validation loss tripped the early
    stop (its row is the last of ``history``) or None."""
    assert rule in RULES
    rows = list(rows)
    epochs = len(rows) if epochs is None else min(int(epochs), len(rows))
    best_key, selected, history, best_epoch, stop_epoch = None, 0.0, [], -1, None
    val_hist = []
    for epoch in range(epochs):
        loss, acc_tr, acc_va, acc_te, val_loss = rows[epoch]
        history.append((float(loss), acc_tr, acc_va, acc_te, val_loss))
        key = acc_va if rule == "max_val_acc" else -val_loss
        key = None if key != key else key
        if key is not None and (best_key is None or key > best_key):
            best_key, selected, best_epoch = key, acc_te, epoch
        if rule == "min_val_loss":
            val_hist.append(val_loss)
            if early_stopping > 0 and epoch > early_stopping:
                if val_loss > plain_sum(val_hist[epoch - early_stopping:epoch]) / early_stopping:
                    stop_epoch = epoch
                    break
    return selected, history, best_epoch, stop_epoch


def plain_sum(values):
    """Left-to-right float64 sum, one rounding per addition (``sum`` of floats up to CPython 3.11)."""
    total = 0.0
    for v in values:
        total = total + v
    return total


def same_floats(a, b):
    """Exact equality of two nested sequences of floats where NaN equals NaN and 0.0 differs from -0.0."""
    import struct
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same_floats(u, v) for u, v in zip(a, b))
    a, b = float(a), float(b)
    if a != a or b != b:
        return a != a and b != b
    return struct.pack("<d", a) == struct.pack("<d", b)
