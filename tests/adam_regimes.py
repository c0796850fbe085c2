"""One Adam / AdamW step pinned per element: the float64 reference, the unit its error is measured in, the element regimes random
training never feeds, and altered updates the comparison must refuse.

``adam_one`` / ``AdamFactors`` / ``acm_adam_step_factors`` (csrc/acm_adam_device.h) are applied by the block update of
acm_adam_step, by the reducing blocks of its flush-in-launch form, by four epilogues of the small-graph step and by the batched
small step.  A single step from a given state is a closed-form function of five numbers per element (p, g, m, v, step), so every
one of those routes can be held to the same per-element statement:

    |got - ref64| <= K * unit        for every element of p', m' and v'; nothing is left out.

With u = 2^-24, floor = 2^-126 (a kernel may flush subnormals), all values the float64 ones:

    s_g      = |g|                    (coupled decay: |g| + wd |p|; g_eff = g + wd p is the value itself and may cancel)
    unit(m') = u (|m| + s_g) + floor
    unit(v') = max(u v', floor) + (1 - beta2) (2 |g_eff| d + d^2),                  d = u s_g
    unit(p') = u (|p_decayed| + |upd|) + (step_size / denom) unit(m')
               + (|upd| / denom) unit(v') / (2 sqrt(v') bc2_sqrt)  [dropped where v' = 0]  + floor

-- first-order propagations of ONE rounding per operand.  K = 8: the update has at most eight fp32 roundings between its inputs
and any one output (two constant conversions, up to six operations), each moves the result by at most one unit, and FMA contraction
only removes roundings.  tests/test_adam_regimes_cpu.py re-establishes the margin on ``restated32`` (the kernel's operation order in
NumPy float32) and shows that every entry of ``MUTANTS`` exceeds it; tests/test_gpu_adam_regimes.py holds the kernels to it."""
import functools
import types

import numpy as np
import scipy.sparse as sp

import head_regimes as H

U = 2.0 ** -24
FLOOR = 2.0 ** -126
TOP = 2.0 ** 127
K = 8
F32, F64 = np.float32, np.float64

# (lr, beta1, beta2, eps, weight_decay, decoupled)
SETTINGS = {
    "adam": (0.01, 0.9, 0.999, 1e-8, 0.0, False),
    "adam-wd5e-4": (0.01, 0.9, 0.999, 1e-8, 5e-4, False),
    "adamw-wd1e-2": (0.01, 0.9, 0.999, 1e-8, 1e-2, True),
    "adam-beta1-0-eps1e-3": (1e-3, 0.0, 0.9, 1e-3, 5e-4, False),
    "adamw-lr0.05": (0.05, 0.9, 0.999, 1e-8, 5e-3, True),
}
STEPS = (0, 1, 9, 700, 100000)
MIN_SHARE = 0.02             # of the elements, for every regime ``coverage`` names
CANCEL_SHARE = 0.12          # coupled runs: elements whose gradient is drawn against wd * p


def _coupled(hp):
    return hp[4] != 0.0 and not hp[5]


def reference(p, g, m, v, step, hp):
    """One step in float64 from fp32 (or any) inputs, torch's documented formula: coupled decay is added to g, decoupled decay
    multiplies p by 1 - lr wd, the bias corrections use k = step + 1, denom = sqrt(v') / sqrt(1 - beta2^k) + eps.  Returns a
    namespace with p, m, v (the results), the intermediates the unit needs and ``all`` (every intermediate, for the range
    statement of ``coverage``)."""
    lr, b1, b2, eps, wd, decoupled = hp
    p, g, m, v = (np.asarray(t, F64) for t in (p, g, m, v))
    decay = wd * p
    if wd != 0.0 and decoupled:
        p_dec, g_eff, s_g = p * (1.0 - lr * wd), g, np.abs(g)
    elif wd != 0.0:
        p_dec, g_eff, s_g = p, g + decay, np.abs(g) + np.abs(decay)
    else:
        p_dec, g_eff, s_g = p, g, np.abs(g)
    k = float(step) + 1.0
    step_size = lr / (1.0 - b1 ** k)
    bc2_sqrt = np.sqrt(1.0 - b2 ** k)
    m1, m2 = b1 * m, (1.0 - b1) * g_eff
    m_new = m1 + m2
    v1, v2 = b2 * v, (1.0 - b2) * g_eff * g_eff
    v_new = v1 + v2
    root = np.sqrt(v_new)
    denom = root / bc2_sqrt + eps
    quot = m_new / denom
    upd = step_size * quot
    p_new = p_dec - upd
    every = [p, g, m, v, decay, p_dec, g_eff, g_eff - m, (1.0 - b1) * (g_eff - m), m1, m2, m_new, v1, (1.0 - b2) * g_eff, v2, v_new, root,
             root / bc2_sqrt, denom, quot, upd, p_new]
    return types.SimpleNamespace(p=p_new, m=m_new, v=v_new, p_in=p, m_in=m, v_in=v, g=g, g_eff=g_eff, s_g=s_g, p_dec=p_dec, upd=upd,
                                 denom=denom, step_size=step_size, bc2_sqrt=bc2_sqrt, eps=eps, beta2=b2, all=every)


def units(ref):
    """{"p", "m", "v"}: the error unit of each result, per element (module docstring)."""
    unit_m = U * (np.abs(ref.m_in) + ref.s_g) + FLOOR
    d = U * ref.s_g
    unit_v = np.maximum(U * ref.v, FLOOR) + (1.0 - ref.beta2) * (2.0 * np.abs(ref.g_eff) * d + d * d)
    live = ref.v > 0
    through_v = np.zeros_like(ref.v)
    through_v[live] = (np.abs(ref.upd[live]) / ref.denom[live]) * unit_v[live] / (2.0 * np.sqrt(ref.v[live]) * ref.bc2_sqrt)
    unit_p = U * (np.abs(ref.p_dec) + np.abs(ref.upd)) + (ref.step_size / ref.denom) * unit_m + through_v + FLOOR
    return {"p": unit_p, "m": unit_m, "v": unit_v}


def ratios(got, ref):
    """{"p", "m", "v"}: max over the elements of |got - ref| / unit (inf where a result is not finite).  ``got``: (p', m', v')."""
    unit = units(ref)
    out = {}
    for name, g, r in zip(("p", "m", "v"), got, (ref.p, ref.m, ref.v)):
        g = np.asarray(g, F64)
        assert g.shape == r.shape, (name, g.shape, r.shape)
        if g.size == 0:
            out[name] = 0.0
            continue
        with np.errstate(invalid="ignore"):
            q = np.abs(g - r) / unit[name]
        q[~np.isfinite(g)] = np.inf
        out[name] = float(q.max())
    return out


def restated32(p, g, m, v, step, hp, neighbour=None, alter=None):
    """adam_one + AdamFactors + acm_adam_step_factors operation by operation in NumPy float32 (the constants are converted from
    double as the kernels convert them).  Used by the CPU test only; the kernels are compared with ``reference``.  ``neighbour``:
    the step counter of the tensor next to this one in the launch's table (default: step - 1, the tables below count 0, 1, 2, ...;
    step + 1 for the first); the update itself never reads it, the "neighbouring counter" entry of MUTANTS reads nothing else.
    ``alter``: which entry of MUTANTS this call is."""
    lr, b1, b2, eps, wd, decoupled = hp
    p, g, m, v = (np.array(t, F32) for t in (p, g, m, v))
    decay_eff = F32(1.0) if wd == 0.0 else F32(1.0 - lr * wd)
    wd32, w1, b2_32, w2, eps32 = F32(wd), F32(1.0 - b1), F32(b2), F32(1.0 - b2), F32(eps)
    as_decoupled = bool(decoupled) or wd == 0.0 or alter == "coupled as decoupled"
    if neighbour is None:                  # tensor i of the tables below starts at step = i: the tensor before it (after the first)
        neighbour = step - 1 if step > 0 else step + 1
    k = float(neighbour if alter == "neighbouring counter" else step) + 1.0
    bc2 = 1.0 - b2 ** k
    with np.errstate(all="ignore"):
        step_size = F32(lr / (1.0 - b1 ** k))
        bc2_sqrt = F32(bc2 if alter == "bc2 without its square root" else np.sqrt(bc2))
        g_raw = g
        if as_decoupled:
            p = p * decay_eff
        else:
            g = g + wd32 * p
        m = m + w1 * (g - m)
        g_sq = g_raw if alter == "v' from g, not g_eff" else g
        v = v * b2_32 + w2 * g_sq * g_sq
        if alter == "eps inside the bias correction":
            denom = (np.sqrt(v) + eps32) / bc2_sqrt
        else:
            denom = np.sqrt(v) / bc2_sqrt + eps32
        p = p - step_size * (m / denom)
    return p, m, v


# Altered updates, same signature as restated32.  "neighbouring counter": the factors of the tensor next door -- pk.step[t] with the
# wrong t, a wrong FACT slot, the covered search of the flush resolving one tensor too far.
MUTANTS = {name: functools.partial(restated32, alter=name) for name in
           ("eps inside the bias correction", "neighbouring counter", "coupled as decoupled", "v' from g, not g_eff",
            "bc2 without its square root")}


def _log_uniform(rng, lo, hi, n):
    return np.exp(rng.uniform(np.log(lo), np.log(hi), n))


def _sign(rng, n):
    return np.where(rng.random(n) < 0.5, -1.0, 1.0)


def draw_p(rng, n):
    """Exactly 0 on 10 % of the elements, otherwise log-uniform 1e-3 .. 30 with a random sign."""
    p = _log_uniform(rng, 1e-3, 30.0, n) * _sign(rng, n)
    p[rng.random(n) < 0.10] = 0.0
    return p.astype(F32)


def draw_g(rng, n, p, hp):
    """Log-uniform 1e-12 .. 1e3 with a random sign, exactly 0 on about 15 %; under coupled decay CANCEL_SHARE of the elements take
    g = -wd p (1 + 3e-3 noise) instead: the decay term cancels the gradient to a few thousandths of either."""
    g = _log_uniform(rng, 1e-12, 1e3, n) * _sign(rng, n)
    if _coupled(hp):
        sel = rng.random(n) < CANCEL_SHARE
        against = -hp[4] * p.astype(F64) * (1.0 + 3e-3 * rng.standard_normal(n))
        g[sel] = against[sel]
    g[rng.random(n) < 0.15] = 0.0
    return g.astype(F32)


def draw_moments(rng, p, g, hp, step):
    """(m, v) by element regime around a given gradient, drawn jointly and independently per element.  m, one of four: 0; ~ g;
    the value at which m' cancels (-g_eff (1 - beta1) / beta1 = -g / 9 at beta1 = 0.9 without coupled decay), off by 1e-4 noise;
    unrelated log-uniform.  v, one of four: 0; ~ g^2; 1e6 g^2; unrelated log-uniform 1e-24 .. 1e6.  step = 0: m = v = 0."""
    n = g.size
    if step == 0:
        return np.zeros(n, F32), np.zeros(n, F32)
    b1 = hp[1]
    g64 = g.astype(F64)
    g_eff = g64 + hp[4] * p.astype(F64) if _coupled(hp) else g64
    back = (1.0 - b1) / b1 if b1 > 0 else 1.0 / 9.0
    m_of = [np.zeros(n), g64 * rng.uniform(0.5, 2.0, n), -g_eff * back * (1.0 + 1e-4 * rng.standard_normal(n)),
            _log_uniform(rng, 1e-12, 1e3, n) * _sign(rng, n)]
    v_of = [np.zeros(n), g64 * g64 * rng.uniform(0.5, 2.0, n), 1e6 * g64 * g64, _log_uniform(rng, 1e-24, 1e6, n)]
    km, kv = rng.integers(0, 4, n), rng.integers(0, 4, n)
    m = np.choose(km, m_of).astype(F32)
    v = np.choose(kv, v_of).astype(F32)
    return m, v


def draw(n, seed, hp, step):
    """(p, g, m, v): n fp32 elements in the regimes above."""
    rng = np.random.default_rng([seed, n, int(step)])
    p = draw_p(rng, n)
    g = draw_g(rng, n, p, hp)
    m, v = draw_moments(rng, p, g, hp, step)
    return p, g, m, v


def coverage(ref, hp, step):
    """({statement: share of the elements}, smallest nonzero magnitude, largest magnitude) on the float64 reference.  step = 0 has
    cold moments: the statements about a warm m do not apply there and are left out of the dict."""
    out = {"eps > 10 % of denom": np.mean(ref.eps > 0.1 * ref.denom), "eps < 1e-4 of denom": np.mean(ref.eps < 1e-4 * ref.denom),
           "v = 0 with g != 0": np.mean((ref.v_in == 0) & (ref.g != 0))}
    if step > 0:
        out["g = 0 with m != 0"] = np.mean((ref.g == 0) & (ref.m_in != 0))
        out["|m'| < 1e-3 (|m| + s_g)"] = np.mean((np.abs(ref.m) < 1e-3 * (np.abs(ref.m_in) + ref.s_g)) & (np.abs(ref.m_in) + ref.s_g > 0))
    if _coupled(hp):
        out["|g_eff| < 1e-2 s_g"] = np.mean((np.abs(ref.g_eff) < 1e-2 * ref.s_g) & (ref.s_g > 0))
    lo, hi = np.inf, 0.0
    for t in ref.all:
        a = np.abs(t[np.isfinite(t)])
        assert a.size == t.size, "a value of the reference is not finite"
        if (a > 0).any():
            lo, hi = min(lo, float(a[a > 0].min())), max(hi, float(a.max()))
    return {k: float(s) for k, s in out.items()}, lo, hi


def assert_coverage(ref, hp, step, what=""):
    shares, lo, hi = coverage(ref, hp, step)
    thin = {k: s for k, s in shares.items() if s < MIN_SHARE}
    assert not thin, (what, thin)
    assert FLOOR <= lo and hi <= TOP, (what, lo, hi)
    return shares


# ---- the tensor tables of tests/test_gpu_adam_regimes.py --------------------------------------------------------------------
# acm_adam_step, plain: 45 tensors (PACK = 40: the last five travel in a second launch).  Even entries get an aligned gradient
# (full chunks of 2048 take the float4 path, the rest of a tensor the scalar one), odd entries a 4-byte-offset view (scalar path).
PLAIN_SIZES = [2048, 1, 4099, 3, 5000, 5, 2049, 33, 2047, 2048, 64, 4099, 7, 2049, 4096, 100, 255, 257, 1023, 1025, 31, 65, 2, 129, 640,
               5000, 9, 17, 320, 63, 448, 2047, 11, 13, 96, 6, 192, 19, 1, 77, 2048, 2049, 4099, 3, 5000]
assert len(PLAIN_SIZES) == 45


def counters(n, far=(7, 700), farther=None):
    """Tensor i starts at step = i -- small, so that k and k +- 1 differ visibly in both factors -- except one at 700 and one at
    100 000 (the last but one by default: in the second pack of a 45-tensor table)."""
    steps = list(range(n))
    steps[far[0] % n] = far[1]
    steps[(n - 2) if farther is None else farther] = 100000
    assert len(set(steps)) == n
    return steps


def table(sizes, steps, seed, hp):
    """[(p, g, m, v)] for the tensors of a launch."""
    return [draw(n, seed + 31 * i, hp, s) for i, (n, s) in enumerate(zip(sizes, steps))]


# ---- the small-graph step -----------------------------------------------------------------------------------------------------
SMALL_F_IN, SMALL_CLASSES, SMALL_HIDDEN = 40, 5, 64
# (model_type, structure_info, attn_layernorm): four channels with LayerNorm -- all 17 roles of both layers, 34 tensors -- and
# three channels without
SMALL_CONFIGS = {"acmgcnp-k4-ln": ("acmgcnp", 1, True), "acmgcn-k3": ("acmgcn", 0, False)}


@functools.lru_cache(maxsize=None)
def small_graph(seed=1):
    """head_regimes.graph (N = 203, three isolated rows, one raw self-loop) thinned to a mean degree near 2 and without its hub:
    with a tenth of the rows in the training set most rows of both [N, .] structure parameters are then out of the loss's
    reach and take a gradient of exactly zero.  A narrow feature matrix with one row of zeros, labels, the training rows."""
    rng = np.random.default_rng(seed)
    a = sp.triu(H.graph(seed), 1).tocoo()
    keep = (rng.random(a.nnz) < 0.1) & (a.row != 0)
    a = sp.csr_matrix((np.ones(int(keep.sum())), (a.row[keep], a.col[keep])), shape=(H.N, H.N))
    a = ((a + a.T) > 0).astype(np.float32).tolil()
    a[3, 3] = 1.0
    adj = sp.csr_matrix(a)
    x = ((rng.random((H.N, SMALL_F_IN)) < 0.2) * rng.uniform(0.5, 1.5, (H.N, SMALL_F_IN))).astype(F32)
    x[5] = 0.0
    y = rng.integers(0, SMALL_CLASSES, H.N)
    train = np.sort(rng.permutation(H.N)[: H.N // 10])
    return types.SimpleNamespace(n=H.N, adj=adj, x=x, y=y, train=train)


def small_counters(n_tensors, slot=0):
    """Distinct counters per role and layer, and per slot of a batch: slot s counts from 40 s; one tensor at 700 + s, one at
    100 000 + s."""
    steps = [40 * slot + i for i in range(n_tensors)]
    steps[3] = 700 + slot
    steps[n_tensors - 2] = 100000 + slot
    return steps
