"""The trainer's optimizer step (tdnnf_net_update) in float64 numpy -- test infrastructure.

A restatement of ApplyL2Regularization, UpdateNnetWithMaxChange, ScaleBatchnormStats, ConstrainOrthonormal and
ConstrainOrthonormalInternal (nnet3/nnet-utils.cc:2223-2245, :2085-2175, :1040-1077, :914-1032) written from their description
and from tests/oracle_net.py::OracleNet.update, for tests/test_gpu_net_update.py (the kernels of csrc/optim_group.hip and
csrc/net_update.hip) and tests/test_update_ref64.py (which pins it against the float32 C oracle).

Arithmetic.  What the reference keeps in a BaseFloat scalar is float32 here too, because comparisons hang on it: the per-component
learning rate and L2 coefficient, `dot` (rounded to float32 BEFORE sqrt and the comparison with max-change), the factors, the
running param_delta_squared (a scalar recurrence of the reference, float32 step by step in component order), the global scale, and
the orthonormal step's scale, ratio, update_speed and coefficient.  Every sum over elements and every matrix product is float64.

One deliberate difference from the reference's text: it tests `param_delta > max_param_change` before it looks for an infinite
change, so a NaN (a clipped component with an infinite dot product gives factor 0 and 0 * 0 * inf = NaN) slips through and the
other components' deltas of the same broken minibatch are applied.  Here, as in optim_group.hip, a param_delta that is not
finite refuses the whole update ("Infinite parameter change, will not apply"), whenever the global max-change is on.
"""
import numpy as np

from tests.oracle_net import decision

F = np.float32
ITEM = 4096  # elements per block of the update kernels (optim_group.hip: kItem)


def ranges(components, num_params):
    """[begin, end) per component: a component owns everything up to the next one's begin, alignment padding included."""
    begins = [c["begin"] for c in components] + [int(num_params)]
    return [(begins[i], begins[i + 1]) for i in range(len(components))]


def owned(c):
    """Number of elements a component really has: rows * cols + num_alpha + bias (the rest of its range is padding)."""
    return c["rows"] * c["cols"] + c["num_alpha"] + (c["rows"] if c["has_bias"] else 0)


def constrained(components):
    return [i for i, c in enumerate(components) if c["orthonormal"] != 0.0]


def schedule(components, step):
    """Indices of the constrained components the 1-in-4 schedule steps at `step` (net_update.hip; RandInt(0, 3) == 0)."""
    return [i for i in constrained(components) if decision(step, 2 * i + 1) % 4 == 0]


def steps_selecting(components, wanted, limit=1 << 20):
    """The smallest step < limit whose schedule steps exactly the set `wanted` of (indices of) constrained components."""
    cons = constrained(components)
    wanted = set(wanted)
    assert wanted <= set(cons), (wanted, cons)
    for step in range(limit):
        if all((decision(step, 2 * i + 1) % 4 == 0) == (i in wanted) for i in cons):
            return step
    raise LookupError("no step below %d selects exactly %s" % (limit, sorted(wanted)))


def ratio64(M):
    """rows * tr(P^2) / tr(P)^2 of P = M M^T in float64 (M wide, or its transpose when tall)."""
    M = np.asarray(M, np.float64)
    if M.shape[0] > M.shape[1]:
        M = M.T
    P = M @ M.T
    return M.shape[0] * float((P * P).sum()) / float(np.trace(P)) ** 2


def matrix_with_ratio(rows, cols, ratio, seed, s0=0.7):
    """U diag(s) V^T (rows <= cols, float64) with random orthonormal U, V: every singular value s0 but one s1 > s0, s1 / s0 found by
    bisection so that rows * sum(s^4) / sum(s^2)^2 is `ratio` (1 <= ratio < rows).  ratio = 1: orthonormal rows times s0."""
    assert 1 <= rows <= cols and 1.0 <= ratio < rows, (rows, cols, ratio)
    rng = np.random.default_rng(seed)
    U = np.linalg.qr(rng.standard_normal((rows, rows)))[0]
    V = np.linalg.qr(rng.standard_normal((cols, rows)))[0]  # cols x rows, orthonormal columns

    def r(t):  # t = (s1 / s0)^2
        return rows * (rows - 1 + t * t) / (rows - 1 + t) ** 2

    lo, hi = 1.0, 2.0
    while r(hi) < ratio:
        hi *= 2.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if r(mid) < ratio else (lo, mid)
    s = np.full(rows, s0)
    s[0] = s0 * np.sqrt(0.5 * (lo + hi))
    return (U * s) @ V.T


def constrain_orthonormal64(M, scale_in=-1.0, exact=False):
    """ConstrainOrthonormalInternal on M (rows <= cols) in float64: returns dict(X, M_new, trP, trPP, scale, ratio, update_speed).
    exact=False: scale, ratio, update_speed and the coefficient are float32 as in the reference; exact=True keeps them in float64
    (the mathematics: tr(M X^T) = 0, fixed points)."""
    M = np.asarray(M, np.float64)
    rows, cols = M.shape
    assert rows <= cols and scale_in != 0.0
    P = M @ M.T
    trP, trPP = float(np.trace(P)), float((P * P).sum())
    T = (lambda v: float(v)) if exact else F
    update_speed, scale, ratio = T(0.125), T(scale_in), T(1.0)
    if scale_in < 0:  # the floating scale, :938-986
        scale = np.sqrt(T(trPP / trP))
        ratio = T(trPP * rows / (trP * trP))
        if ratio > T(1.02):
            update_speed = update_speed * T(0.5)
            if ratio > T(1.1):
                update_speed = update_speed * T(0.5)
    s2 = scale * scale
    coef = T(-4.0) * (update_speed / s2)  # -4 alpha, alpha = update_speed / scale^2 (:1019, :1030)
    X = float(coef) * ((P - float(s2) * np.eye(rows)) @ M)
    return dict(X=X, M_new=M + X, trP=trP, trPP=trPP, scale=float(scale), ratio=float(ratio), update_speed=float(update_speed))


def constrain_component64(W, scale_in=-1.0, exact=False):
    """ConstrainOrthonormal's handling of one parameter matrix: a tall one (rows > cols) is stepped through its transpose (:1068-1075)."""
    W = np.asarray(W, np.float64)
    if W.shape[0] <= W.shape[1]:
        return constrain_orthonormal64(W, scale_in, exact)
    r = constrain_orthonormal64(W.T, scale_in, exact)
    r["X"], r["M_new"] = r["X"].T, r["M_new"].T
    return r


def update_ref64(components, params, grads, lr, l2_scale, max_param_change, step):
    """One optimizer step.  components: ChainNet.components (begin, rows, cols, has_bias, num_alpha, lr_factor, l2, max_change,
    orthonormal); params, grads: the flat float32 vectors.  Returns a dict:
      params   the new parameters, float64
      delta    per component: lr_c g + l2coef_c theta over its range, float64
      dot      per component: <delta, delta> in float64
      factor   per component: its own max-change factor (float32 value)
      scale    the global max-change scale (float32 value)
      total    per component: what its delta is multiplied by = factor * scale in float32 (0 when the update is refused)
      param_delta  the float32 norm the global limit is compared with
      applied  False when the change was not finite and nothing was applied
      stepped  {component index: constrain_component64's dict} for every component the schedule stepped
    """
    params = np.asarray(params)
    grads = np.asarray(grads)
    assert params.dtype == np.float32 and grads.dtype == np.float32 and params.shape == grads.shape
    rng = ranges(components, params.size)
    p = params.astype(np.float64)
    nc = len(components)
    delta, dots, factor = [], np.zeros(nc), np.ones(nc, F)
    pds = F(0.0)
    with np.errstate(all="ignore"):
        for i, (c, (b, e)) in enumerate(zip(components, rng)):
            lrc = F(lr) * F(c["lr_factor"])
            l2c = F(-2.0) * F(l2_scale) * lrc * F(c["l2"])  # ApplyL2Regularization :2240
            d = float(lrc) * grads[b:e].astype(np.float64) + float(l2c) * p[b:e]
            delta.append(d)
            dots[i] = float((d * d).sum())
            dot, mc = F(dots[i]), F(c["max_change"])
            assert mc >= 0
            if mc != 0 and np.sqrt(dot) > mc:
                factor[i] = mc / np.sqrt(dot)
            pds = F(pds + F(F(factor[i] * factor[i]) * dot))
        param_delta = np.sqrt(pds)
        scale, applied = F(1.0), True
        mpc = F(max_param_change)
        if mpc != 0:
            if not np.isfinite(param_delta):
                applied = False
            elif param_delta > mpc:
                scale = mpc / param_delta
        total = (factor * scale).astype(F) if applied else np.zeros(nc, F)
        if applied:
            for i, (b, e) in enumerate(rng):
                if total[i] != 0:
                    p[b:e] += float(total[i]) * delta[i]
    stepped = {}
    for i in schedule(components, step):
        c = components[i]
        n = c["rows"] * c["cols"]
        W = p[c["begin"]:c["begin"] + n].reshape(c["rows"], c["cols"])
        stepped[i] = constrain_component64(W, c["orthonormal"])
        stepped[i]["M"] = W.copy()
        p[c["begin"]:c["begin"] + n] = stepped[i]["M_new"].ravel()
    return dict(params=p, delta=delta, dot=dots, factor=factor, scale=float(scale), total=total, param_delta=float(param_delta),
                applied=applied, stepped=stepped)


def stat_blocks(cfg):
    """([(is_relu, begin, end)], size) of the model-statistics vector (tdnnf_net_get_stats): per BatchNorm [count, sum[D], sumsq[D]],
    per ReLU [count, value_sum[D], deriv_sum[D], oderiv_count, oderiv_sumsq[D]]; order tdnn1, the tdnnf layers, then per head
    BatchNorm, ReLU (hidden width) and BatchNorm (prefinal small width)."""
    Hd, S = cfg.hidden_dim, cfg.prefinal_small_dim
    kinds = [(False, Hd), (True, Hd)] * (1 + cfg.num_layers) + [(False, Hd), (True, Hd), (False, S)] * 2
    out, o = [], 0
    for relu, D in kinds:
        n = 2 + 3 * D if relu else 1 + 2 * D
        out.append((relu, o, o + n))
        o += n
    return out, o


def scale_batchnorm_stats64(stats, cfg):
    """ScaleBatchnormStats after one update: every BatchNorm block times float64(float32(batchnorm_stats_scale)), the ReLU blocks
    untouched; nothing at all at scale 1.0 or in cv-update mode (BatchNormTest components are not scaled)."""
    out = np.array(stats, np.float64)
    s = float(F(cfg.batchnorm_stats_scale))
    if s != 1.0 and not cfg.cv_update:
        for relu, b, e in stat_blocks(cfg)[0]:
            if not relu:
                out[b:e] *= s
    return out


def element_bar(ref, components, num_params):
    """Per element of the flat vector, the bar of an update computed in float32 against `ref` (update_ref64's result):
        2^-24 |p'| + 8 * 2^-24 |f d|.
    The kernels form d = fl(lr g + l2 p) in two or three roundings and p' = fl(p + fl(f d)), f a float32 quotient of a float32
    square root of a sum formed in double: the last rounding is half an ulp of p' (2^-24 |p'|), and the relative errors of d (up to
    3 roundings), of f (quotient, square root, the rounding of dot, the global scale's own quotient and product) and of f d (one)
    add up to less than 8 half-ulps of |f d|."""
    u = 2.0 ** -24
    bar = u * np.abs(ref["params"])
    for i, (b, e) in enumerate(ranges(components, num_params)):
        bar[b:e] += 8 * u * np.abs(float(ref["total"][i]) * ref["delta"][i])
    return bar


def ggemm_slices(K, whole_k=False):
    """The K slices csrc/ggemm.h's GemmList::add cuts a product of depth K into: a list of slice lengths (one entry: no reduction stage)."""
    nsplit = 1 if whole_k else min((K + 127) // 128, 64)
    kchunk = (((K + nsplit - 1) // nsplit) + 15) // 16 * 16
    nsplit = (K + kchunk - 1) // kchunk
    return [min(K, (s + 1) * kchunk) - s * kchunk for s in range(nsplit)]


def row_tiles(rows):
    """Heights of the 64-row tiles of a matrix with `rows` rows."""
    return [min(64, rows - m0) for m0 in range(0, rows, 64)]


def items(components, num_params):
    """Per component the lengths of its 4096-element items (optim_group.hip: upd_group_create)."""
    return [[min(ITEM, e - b0) for b0 in range(b, e, ITEM)] for b, e in ranges(components, num_params)]
