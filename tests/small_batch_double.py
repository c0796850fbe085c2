"""numpy forms of the five batched entry points for the CPU double (tests/fake_lib.py), set on an installed instance: each
loops the double's OWN single-run function over the slots of the table, which is what the batched kernels are to the single
ones.  "Device" tables are host memory here."""
import ctypes as C


def _addr(p):
    return int(p.value if isinstance(p, C.c_void_p) else p)


def install_batch(fake):
    from acm_gnn_amd import _lib
    bound = {}

    def table_bytes(n_slots, out):
        if not 1 <= n_slots <= _lib.SMALL_BATCH_MAX:
            fake._err = b"acm_small_batch_table_bytes: n_slots"
            return 1 if n_slots < 1 else 4
        out._obj.value = 64 * int(n_slots)
        return 0

    def bind(a, x, xt, n_slots, slots, table, table_bytes_, stream):
        if not 1 <= n_slots <= _lib.SMALL_BATCH_MAX:
            fake._err = b"acm_small_batch: n_slots"
            return 1 if n_slots < 1 else 4
        live = [_lib.SmallStep.from_buffer_copy(slots[i].contents) if slots[i] else None for i in range(n_slots)]
        if not any(s is not None for s in live) or not table or table_bytes_ < 64 * n_slots:
            fake._err = b"acm_small_batch_bind: empty / table"
            return 1
        first = next(s for s in live if s is not None)
        for s in live:
            if s is not None and (s.n_classes, s.n_channels, s.train, s.update, s.xt_vals) != \
                    (first.n_classes, first.n_channels, first.train, first.update, first.xt_vals):
                fake._err = b"acm_small_batch: slots disagree"
                return 1
        bound[_addr(table)] = live
        return 0

    def step(a, x, xt, n_slots, shape, table, stream):
        live = bound.get(_addr(table))
        if live is None or len(live) != n_slots:
            fake._err = b"acm_small_batch_step: table not bound"
            return 1
        fake.small_batch_calls = getattr(fake, "small_batch_calls", 0) + 1
        for s in live:
            if s is not None:
                st = fake.acm_small_step(a, x, xt, C.byref(s), stream)
                if st:
                    return st
        return 0

    def metrics(n, c, ldz, ldw, n_sets, loss_set, n_slots, table, wsb, stream):
        for e in (_lib.EvalMetricsSlot * n_slots).from_address(_addr(table)):
            if e.logits:
                st = fake.acm_eval_metrics(n, c, e.logits, ldz, e.labels, e.weights, ldw, n_sets, loss_set, e.out, e.workspace, wsb, stream)
                if st:
                    return st
        return 0

    def select(n_slots, table, stream):
        for e in (_lib.Select * n_slots).from_address(_addr(table)):
            if e.result or e.result_f64:
                st = fake.acm_select_step(C.byref(e), stream)
                if st:
                    return st
        return 0

    fake.acm_small_batch_table_bytes, fake.acm_small_batch_bind, fake.acm_small_batch_step = table_bytes, bind, step
    fake.acm_eval_metrics_batch, fake.acm_select_step_batch = metrics, select
    return fake
