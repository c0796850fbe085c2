"""numpy forms of the three graph-per-slot batch entry points for the CPU double (tests/fake_lib.py), set on an installed
instance beside ``small_batch_double.install_batch``: each loops the double's OWN single-run function over the slots of the
table, every slot with its own handles -- which is what the batched kernels are to the single ones.  "Device" tables are host
memory here; the grids count work as the library's do (here: one unit per stored entry of the handle), so an envelope means
something."""
import ctypes as C

from small_batch_double import _addr


def install_graphs(fake):
    from acm_gnn_amd import _lib
    bound = {}

    def own_grids(a, x, xt, train):
        nnz = lambda h: len(fake._get(h).indices)                 # noqa: E731
        return (nnz(x), nnz(a), nnz(a), nnz(xt) if train and xt else 0, 1)

    def fits(own, g):
        return all(o <= e for o, e in zip(own, (g.proj, g.wide, g.graph, g.item_blocks, g.red_blocks)))

    def grids(a, x, xt, shape, out):
        if not a or not x or (shape._obj.train and not xt):
            fake._err = b"acm_small_batch: NULL argument"
            return 1
        g = out._obj
        for name, v in zip(("proj", "wide", "graph", "item_blocks", "red_blocks"), own_grids(a, x, xt, shape._obj.train)):
            setattr(g, name, max(getattr(g, name), v))
        return 0

    def bind(n_slots, a, x, xt, slots, grids_, table, table_bytes_, stream):
        if not 1 <= n_slots <= _lib.SMALL_BATCH_MAX:
            fake._err = b"acm_small_batch: n_slots"
            return 1 if n_slots < 1 else 4
        if not a or not x or not xt:
            fake._err = b"acm_small_batch_bind_graphs: NULL handle array"
            return 1
        live = [(_lib.SmallStep.from_buffer_copy(slots[i].contents), a[i], x[i], xt[i]) if slots[i] else None for i in range(n_slots)]
        if not any(s is not None for s in live) or not table or table_bytes_ < 64 * n_slots:
            fake._err = b"acm_small_batch_bind_graphs: empty / table"
            return 1
        first = next(s for s in live if s is not None)
        for i, s in enumerate(live):
            if s is None:
                continue
            if (s[0].n_classes, s[0].n_channels, s[0].train, s[0].update, s[0].f_in) != \
                    (first[0].n_classes, first[0].n_channels, first[0].train, first[0].update, first[0].f_in):
                fake._err = b"acm_small_batch: slots disagree"
                return 1
            if fake._get(s[1]).n_rows != fake._get(first[1]).n_rows:
                fake._err = b"acm_small_batch: slots %d and %d disagree in n_rows" % (live.index(first), i)
                return 1
            if not fits(own_grids(s[1], s[2], s[3], s[0].train), grids_._obj):
                fake._err = b"acm_small_batch_bind_graphs: slot %d needs more workgroups than the batch's grids have" % i
                return 2
        bound[_addr(table)] = live                      # (only now: a refused bind leaves the table as it was)
        return 0

    def step(n_slots, shape, grids_, table, stream):
        live = bound.get(_addr(table))
        if live is None or len(live) != n_slots:
            fake._err = b"acm_small_batch_step_graphs: table not bound"
            return 1
        fake.small_graphs_calls = getattr(fake, "small_graphs_calls", 0) + 1
        for s in live:
            if s is not None:
                p, a, x, xt = s
                fake.small_graphs_handles = getattr(fake, "small_graphs_handles", set()) | {a}
                st = fake.acm_small_step(C.c_void_p(a), C.c_void_p(x), C.c_void_p(xt) if xt else None, C.byref(p), stream)
                if st:
                    return st
        return 0

    fake.acm_small_batch_grids, fake.acm_small_batch_bind_graphs, fake.acm_small_batch_step_graphs = grids, bind, step
    return fake
