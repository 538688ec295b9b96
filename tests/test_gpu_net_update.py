"""-m gpu: the trainer's optimizer step (tdnnf_net_update: csrc/optim_group.hip, csrc/net_update.hip, the tile tasks of csrc/ggemm.h)
per component against float64 (tests/update_ref64.py).  No forward pass: parameters and gradients are written into net.params /
net.grads, net.update(lr, l2_regularize_scale, step) is the whole call.

Bars (nothing is calibrated against the kernels):
  update elements   |p'_gpu - p'_64| <= 2^-24 |p'| + 8 * 2^-24 |f d|  per element.  The kernels form d = fl(lr g + l2 p) in two or
                    three roundings and p' = fl(p + fl(f d)); f is a float32 quotient of a float32 square root of a sum formed in
                    double (times the global scale, another float32 quotient).  The last rounding is half an ulp of p'; the
                    relative errors of d, f and the product f d add up to fewer than 8 half-ulps of |f d|.
  max-change factor |f_gpu / f_ref - 1| <= 8 * 2^-24 per component, f_gpu = <p' - p, delta> / <delta, delta> in float64.
  M' after an orthonormal step   rel_l2 < 1e-5 (the bar tests/test_gpu_views.py::test_constrain_orthonormal holds the stand-alone
                    entry to).
  the change X = M' - M          rel_l2 <= max(8 e_ref, 64 * 2^-24), e_ref = the rel_l2 between the change the float32 C oracle
                    (oracle_constrain_orthonormal, plain loops) makes on the same matrix and the float64 change, measured per
                    case at run time; 8 is a margin for the other summation order of the tiled split-K float32 products.  A
                    matrix at its fixed point (ratio 1.000) changes by rounding noise on both sides: |X_gpu| <= 1e-5 |M| there.
"""
import functools

import numpy as np
import pytest

from oracle import pyoracle as ora
from tests import update_ref64 as R
from tests.gpu_util import host, rel_l2
from tests.test_gpu_net import CASES as NET_CASES, _D

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
_SMALL = dict(frames_per_chunk=12, num_sequences=2, feat_dim=8, ivector_dim=4, num_pdfs=24)
NETS = {
    # K = 100 and K = 50: one slice, no reduction stage; 50 columns: the scalar-load path; every matrix a partial tile
    "ragged": dict(next(c[1] for c in NET_CASES if c[0] == "ragged-dims")),
    # K = 320: slices 112 + 112 + 96; row tiles 64 + 16 and 64 + 64 + 8; P of 3 x 3 tiles; K = 160: 80 + 80
    "tiles": dict(_SMALL, hidden_dim=160, strides=[1, 0, 3], bottleneck=[80, 24, 136], small_dim=72),
    # K = 236: slices 128 + 108 and their reduction NEXT TO K = 118: one slice, no reduction, in one selection (with hidden_dim 160
    # every K is above 128 and has a reduction stage); 118 columns: scalar loads; 21 x 118 and 35 x 118: the total % 4 tail of M += U
    "mixed": dict(_SMALL, hidden_dim=118, strides=[1, 0, 3], bottleneck=[7, 21, 70], small_dim=35),
    # 72 x 48 and three 64 x 48: the transpose path next to two grouped 16 x 96 ones
    "tall": dict(_SMALL, layer_offsets=[(1, 1), (0, 0), (3, 3)], hidden_dim=48, bottleneck=[16, 72, 16], small_dim=64),
    # 16 x 256 = exactly one 4096-element item
    "items": dict(_SMALL, hidden_dim=128, strides=[1], bottleneck=16, small_dim=16),
    # the production width: K = 3072, 24 slices per tile; 160 rows = 2.5 tiles (strides [3] alone is refused: the first layer must
    # run at the input frame rate, so a stride-1 layer of the same shape stands in front)
    "full-k": dict(_SMALL, hidden_dim=1536, strides=[1, 3], bottleneck=160, small_dim=256, num_pdfs=64),
}
SMALL_NETS = ["ragged", "tiles", "mixed", "tall", "items"]
# the fixed point, one ratio per update_speed regime, and the two sides of each threshold (1.02, 1.1) half a percent away from it
RATIOS = [1.0, 1.01, 1.05, 1.5, 1.015, 1.025, 1.095, 1.105]
LR = 0.05


def grouped(c):
    return c["orthonormal"] != 0.0 and c["rows"] <= c["cols"]


def check_edges(name, comps, num_params):
    """What each net of NETS is there for, asserted from its component table; returns the facts as a dict (for the PARITY lines)."""
    cons = [c for c in comps if c["orthonormal"] != 0.0]
    g = [c for c in cons if grouped(c)]
    tall = [c["name"] for c in cons if not grouped(c)]
    slices = {c["name"]: R.ggemm_slices(c["cols"]) for c in g}
    tiles = {c["name"]: R.row_tiles(c["rows"]) for c in g}
    items = R.items(comps, num_params)
    facts = dict(slices=slices, tiles=tiles, tall=tall, items=[it for it in items if len(it) > 1 or it[0] % 1024])
    assert all(c["begin"] % 4 == 0 for c in comps) and num_params % 4 == 0
    if name == "ragged":
        assert sorted({c["cols"] for c in g}) == [50, 100] and all(len(s) == 1 for s in slices.values()) and not tall
        assert any(c["cols"] % 4 for c in g) and all(t[-1] < 64 for t in tiles.values())
    if name == "tiles":
        assert slices["tdnnf2.linear"] == [112, 112, 96] and slices["tdnnf4.linear"] == [112, 112, 96] and slices["tdnnf3.linear"] == [80, 80]
        assert tiles["tdnnf2.linear"] == [64, 16] and tiles["tdnnf4.linear"] == [64, 64, 8] and tiles["prefinal-l"] == [64, 8] and not tall
    if name == "mixed":
        assert slices["tdnnf2.linear"] == [128, 108] and slices["tdnnf3.linear"] == [118] and slices["prefinal-l"] == [118] and not tall
        assert any(c["cols"] % 4 for c in g) and any(c["cols"] % 4 == 0 for c in g) and sum((c["rows"] * c["cols"]) % 4 != 0 for c in g) >= 2 and tiles["tdnnf4.linear"] == [64, 6]
    if name == "tall":
        shapes = {c["name"]: (c["rows"], c["cols"]) for c in cons}
        assert tall == ["tdnnf3.linear", "prefinal-l", "prefinal-chain.linear", "prefinal-xent.linear"]
        assert shapes["tdnnf3.linear"] == (72, 48) and shapes["prefinal-l"] == (64, 48)
        assert [c["name"] for c in g] == ["tdnnf2.linear", "tdnnf4.linear"] and shapes["tdnnf2.linear"] == (16, 96)
    if name == "items":
        lin = [k for k, c in enumerate(comps) if c["name"] == "tdnnf2.linear"][0]
        assert (comps[lin]["rows"], comps[lin]["cols"]) == (16, 256) and items[lin] == [4096]
        assert any(sum(it) < 4096 for it in items) and any(it[-1] % 1024 for it in items) and any(len(it) > 1 for it in items)
    if name == "full-k":
        assert slices["tdnnf2.linear"] == slices["tdnnf3.linear"] == [128] * 24 and tiles["tdnnf3.linear"] == [64, 64, 32] and not tall
        assert max(len(it) for it in items) >= 96  # 160 x 3072 and 1536 x 320: 120 full items each
    return facts


def make_cfg(pkg, name, **fields):
    cfg = pkg.trainer.make_config(**NETS[name])
    for k, v in fields.items():  # (make_config hard-codes the max-change limits: set on the struct)
        assert hasattr(cfg, k), k
        setattr(cfg, k, v)
    return cfg


def make_net(pkg, name, **fields):
    from tests.oracle_net import component_table
    cfg = make_cfg(pkg, name, **fields)
    net = pkg.trainer.ChainNet(cfg)
    want, num_params = component_table(cfg)
    for a, b in zip(net.components, want):  # the library's table is the one derived without it
        assert all(a[k] == b[k] for k in ("name", "begin", "rows", "cols", "has_bias", "num_alpha", "orthonormal")), (a, b)
        assert all(np.float32(a[k]) == np.float32(b[k]) for k in ("lr_factor", "l2", "max_change")), (a, b)
    assert len(net.components) == len(want) and net.num_params == num_params
    check_edges(name, net.components, net.num_params)
    return net


def owned_mask(comps, num_params):
    m = np.zeros(num_params, bool)
    for c in comps:
        m[c["begin"]:c["begin"] + R.owned(c)] = True
    return m


def random_grads(comps, num_params, seed, norms=None, params=None, lr=LR, l2_scale=0.0):
    """Gradients on the elements each component owns (padding zero).  norms[i] = the norm component i's DELTA lr_c g + l2coef_c theta
    is to have (None: leave the component's gradient at unit scale; 0: zero gradient)."""
    rng = np.random.default_rng(seed)
    g = np.zeros(num_params, np.float64)
    for i, (c, (b, e)) in enumerate(zip(comps, R.ranges(comps, num_params))):
        r = np.zeros(e - b)
        r[:R.owned(c)] = rng.standard_normal(R.owned(c))
        lrc = float(np.float32(lr) * np.float32(c["lr_factor"]))
        if norms is None or norms[i] is None or lrc == 0.0:
            g[b:e] = r
            continue
        l2c = float(np.float32(-2.0) * np.float32(l2_scale) * np.float32(lrc) * np.float32(c["l2"]))
        q = l2c * params[b:e].astype(np.float64)
        A, B, Cq = lrc * lrc * (r @ r), lrc * (r @ q), q @ q - norms[i] ** 2  # |a lrc r + q| = norms[i]
        assert B * B - A * Cq > 0, (c["name"], norms[i])
        g[b:e] = (-B + np.sqrt(B * B - A * Cq)) / A * r
    return g.astype(np.float32)


def run_update(net, params, grads, lr, l2_scale, step):
    import torch
    net.set_params(params)
    net.grads.copy_(torch.from_numpy(grads))
    net.update(lr, l2_regularize_scale=l2_scale, step=step)
    return host(net.params).copy(), host(net.grads).copy()


def check_elements(tag, comps, params, p_gpu, ref, skip=()):
    """Every element of every component not in `skip` against float64 at the element bar; padding still zero."""
    bar = R.element_bar(ref, comps, params.size)
    err = np.abs(p_gpu.astype(np.float64) - ref["params"])
    worst = 0.0
    for i, (c, (b, e)) in enumerate(zip(comps, R.ranges(comps, params.size))):
        if i in skip:
            continue
        k = int(np.argmax(err[b:e] - bar[b:e]))
        worst = max(worst, float((err[b:e] / np.maximum(bar[b:e], 1e-300)).max()) if bar[b:e].any() else 0.0)
        assert (err[b:e] <= bar[b:e]).all(), (tag, c["name"], k, err[b + k], bar[b + k], p_gpu[b + k], ref["params"][b + k])
    assert not p_gpu[~owned_mask(comps, params.size)].any(), tag
    print("PARITY test_gpu_net_update %s elements: worst error / bar %.3f" % (tag, worst))


def check_factors(tag, comps, params, p_gpu, ref):
    worst = 0.0
    for i, (c, (b, e)) in enumerate(zip(comps, R.ranges(comps, params.size))):
        d = ref["delta"][i]
        if i in ref["stepped"] or not d.any():
            continue
        f_gpu = float((p_gpu[b:e].astype(np.float64) - params[b:e].astype(np.float64)) @ d) / float(d @ d)
        dev = abs(f_gpu / float(ref["total"][i]) - 1.0)
        worst = max(worst, dev)
        assert dev <= 8 * U24, (tag, c["name"], f_gpu, float(ref["total"][i]), dev / U24)
    print("PARITY test_gpu_net_update %s factors: worst |f_gpu / f_ref - 1| = %.2f x 2^-24 (bar 8)" % (tag, worst / U24))


def oracle_change32(M32, scale_in):
    """The float32 C oracle's step on a float32 matrix (through the transpose when tall): M' as float32."""
    L = ora.lib()
    M = np.ascontiguousarray(M32, np.float32)
    if M.shape[0] <= M.shape[1]:
        L.oracle_constrain_orthonormal(scale_in, ora.fptr(M), M.shape[0], M.shape[1], M.shape[1])
        return M
    Mt = np.ascontiguousarray(M.T)
    L.oracle_constrain_orthonormal(scale_in, ora.fptr(Mt), Mt.shape[0], Mt.shape[1], Mt.shape[1])
    return np.ascontiguousarray(Mt.T)


def check_stepped(tag, comps, p_gpu, ref, fixed_point=()):
    """Every component the schedule stepped: M' at 1e-5, the change at max(8 e_ref, 64 * 2^-24) -- both changes taken from the
    float64 matrix the step started on; the components in `fixed_point` only |X_gpu| <= 1e-5 |M|.  Returns [(name, e_gpu, e_ref)]."""
    out = []
    for i, s in ref["stepped"].items():
        c = comps[i]
        n = c["rows"] * c["cols"]
        Mg = p_gpu[c["begin"]:c["begin"] + n].astype(np.float64).reshape(c["rows"], c["cols"])
        assert rel_l2(Mg, s["M_new"]) < 1e-5, (tag, c["name"], rel_l2(Mg, s["M_new"]))
        Xg = Mg - s["M"]
        if i in fixed_point:
            assert np.linalg.norm(Xg) <= 1e-5 * np.linalg.norm(s["M"]), (tag, c["name"])
            continue
        assert abs(s["ratio"] / 1.02 - 1) > 1e-3 and abs(s["ratio"] / 1.1 - 1) > 1e-3, (tag, c["name"], s["ratio"], "too close to a threshold: other inputs")
        Xo = oracle_change32(s["M"].astype(np.float32), c["orthonormal"]).astype(np.float64) - s["M"]
        e_gpu, e_ref = rel_l2(Xg, s["X"]), rel_l2(Xo, s["X"])
        bar = max(8 * e_ref, 64 * U24)
        print("PARITY test_gpu_net_update %s %s %dx%d ratio %.4f speed %.5f change e_gpu %.3e e_ref %.3e bar %.3e" %
              (tag, c["name"], c["rows"], c["cols"], s["ratio"], s["update_speed"], e_gpu, e_ref, bar))
        assert e_gpu <= bar, (tag, c["name"], e_gpu, e_ref, bar)
        out.append((c["name"], e_gpu, e_ref))
    return out


@functools.lru_cache(maxsize=None)
def _step_for(name, wanted):
    import __graft_entry__ as ge
    from tests.oracle_net import component_table
    comps, _ = component_table(ge.load_package().trainer.make_config(**NETS[name]))  # (the schedule depends on the table's order alone)
    return R.steps_selecting(comps, set(wanted))


def step_selecting(name, wanted=()):
    return _step_for(name, tuple(sorted(wanted)))


def init_params(net, seed):
    return net.init_params_numpy(seed=seed, output_stddev=0.3)


# ------------------------------------------------------------------------------------------------ 3.1 plain update
@pytest.mark.parametrize("name", list(NETS))
def test_plain_update_by_element(pkg, name):
    """lr = 0.05, l2_scale = num_sequences, gradient norms spread over three decades, nothing clipped, no component stepped: every
    element against float64 at the element bar (module docstring); the gradient buffer is zero afterwards, the padding still zero."""
    net = make_net(pkg, name)
    comps, cfg = net.components, net.cfg
    params = init_params(net, 11)
    rng = np.random.default_rng(12)
    norms = [c["max_change"] * 10.0 ** -rng.uniform(0.5, 3.5) if c["max_change"] else None for c in comps]
    grads = random_grads(comps, net.num_params, 13, norms, params, l2_scale=0.0)  # |lr_c g| = norms; the L2 term comes on top
    step = step_selecting(name)
    ref = R.update_ref64(comps, params, grads, LR, float(cfg.num_sequences), cfg.max_param_change, step)
    dn = np.sqrt(ref["dot"])
    gn = np.array([np.linalg.norm(grads[b:e].astype(np.float64)) for (b, e), c in zip(R.ranges(comps, net.num_params), comps) if c["lr_factor"]])
    assert gn.max() / gn.min() > 100 and not ref["stepped"] and ref["applied"]
    assert (ref["factor"] == 1).all() and ref["scale"] == 1.0 and ref["param_delta"] < 0.99 * cfg.max_param_change
    assert all(dn[i] < 0.99 * c["max_change"] for i, c in enumerate(comps) if c["max_change"])
    p, g = run_update(net, params, grads, LR, float(cfg.num_sequences), step)
    net.close()
    assert not g.any()
    check_elements(name + " plain", comps, params, p, ref)
    assert (p != params).any()


# ------------------------------------------------------------------------------------------------ 3.2 clipping
def _clip_norms(comps, kind):
    """Per-component delta norms, as multiples of max_change, that put the step in the regime `kind` names."""
    upd = [i for i, c in enumerate(comps) if c["lr_factor"] != 0.0]
    hidden = [i for i in upd if not comps[i]["name"].startswith("output")]
    mult = {i: 0.3 for i in upd}
    if kind == "one-component":
        mult[hidden[len(hidden) // 2]] = 2.0
    elif kind in ("every-component", "no-global-limit"):
        mult = {i: 1.5 + 0.25 * (k % 3) for k, i in enumerate(upd)}
    elif kind == "global-only":
        mult = {i: 0.9 for i in upd}
    elif kind == "component-and-global":
        mult = {i: (2.5 if k % 2 else 0.9) for k, i in enumerate(upd)}
    elif kind == "no-output-limit":  # max_change_output = 0: the output layers are never clipped on their own
        mult = {i: 0.5 for i in upd}
    return [None if i not in mult else (mult[i] * comps[i]["max_change"] if comps[i]["max_change"] else 2.1) for i in range(len(comps))]


CLIP_KINDS = ["one-component", "every-component", "global-only", "component-and-global", "no-global-limit", "no-output-limit"]


@pytest.mark.parametrize("kind", CLIP_KINDS)
@pytest.mark.parametrize("name", SMALL_NETS)
def test_max_change_clipping(pkg, name, kind):
    """Per-component and global max-change, each regime entered on purpose: sqrt(dot) of every component at least 1 % from its
    limit and param_delta 1 % from max_param_change, in float64 (conditions on the inputs).  Elements at the element bar, and per
    component |f_gpu / f_ref - 1| <= 8 * 2^-24 with f_gpu = <p' - p, delta> / <delta, delta>."""
    fields = dict(max_param_change=0.0) if kind == "no-global-limit" else dict(max_change_output=0.0) if kind == "no-output-limit" else {}
    net = make_net(pkg, name, **fields)
    comps, cfg = net.components, net.cfg
    params = init_params(net, 21)
    l2s = float(cfg.num_sequences)
    grads = random_grads(comps, net.num_params, 22, _clip_norms(comps, kind), params, l2_scale=l2s)
    step = step_selecting(name)
    ref = R.update_ref64(comps, params, grads, LR, l2s, cfg.max_param_change, step)
    dn = np.sqrt(ref["dot"])
    upd = [i for i, c in enumerate(comps) if c["lr_factor"] != 0.0]
    limited = [i for i in upd if comps[i]["max_change"] != 0.0]
    assert all(abs(dn[i] / comps[i]["max_change"] - 1) >= 0.01 for i in limited)
    over = [i for i in limited if dn[i] > comps[i]["max_change"]]
    clipped_norm = np.sqrt(sum(min(dn[i], comps[i]["max_change"] or np.inf) ** 2 for i in upd))
    assert cfg.max_param_change == 0.0 or abs(clipped_norm / cfg.max_param_change - 1) >= 0.01
    assert [i for i in upd if ref["factor"][i] < 1] == over and ref["applied"] and not ref["stepped"]
    glob = ref["scale"] < 1.0
    if kind == "one-component":
        assert len(over) == 1 and not glob
    elif kind == "every-component":
        assert over == upd
    elif kind == "global-only":
        assert not over and glob
    elif kind == "component-and-global":
        assert over and len(over) < len(upd) and glob
    elif kind == "no-global-limit":
        assert over == upd and not glob and clipped_norm > 2.0  # (the default limit of 2.0 would have been in force)
    elif kind == "no-output-limit":
        free = [i for i in upd if comps[i]["max_change"] == 0.0]
        assert len(free) == 2 and not over and glob and all(dn[i] > 1.5 for i in free)
    p, g = run_update(net, params, grads, LR, l2s, step)
    net.close()
    assert not g.any()
    tag = "%s %s" % (name, kind)
    check_elements(tag, comps, params, p, ref)
    check_factors(tag, comps, params, p, ref)


# ------------------------------------------------------------------------------------------------ 3.3 the orthonormal step alone
def _ratio_params(net, seed, rot):
    """init parameters with every constrained matrix replaced by matrix_with_ratio at RATIOS[(k + rot) % len(RATIOS)] (k-th constrained
    component; a tall one gets the transpose of such a matrix).  Returns (params, {component index: requested ratio})."""
    comps = net.components
    params = init_params(net, seed)
    asked = {}
    for k, i in enumerate(R.constrained(comps)):
        c = comps[i]
        lo, hi = min(c["rows"], c["cols"]), max(c["rows"], c["cols"])
        M = R.matrix_with_ratio(lo, hi, RATIOS[(k + rot) % len(RATIOS)], seed=seed + 7 * i)
        M = (M if c["rows"] <= c["cols"] else M.T).astype(np.float32)
        r = R.ratio64(M)
        assert abs(r / 1.02 - 1) > 1e-3 and abs(r / 1.1 - 1) > 1e-3 and abs(r - RATIOS[(k + rot) % len(RATIOS)]) < 1e-4
        params[c["begin"]:c["begin"] + M.size] = M.ravel()
        asked[i] = RATIOS[(k + rot) % len(RATIOS)]
    return params, asked


def _ortho_cases():
    out = []
    for name in NETS:
        out += [(name, "all"), (name, "first-and-last")]
        if name in ("ragged", "tall", "mixed"):
            out.append((name, "each"))
    return out


@pytest.mark.parametrize("name,which", _ortho_cases(), ids=["%s-%s" % c for c in _ortho_cases()])
def test_orthonormal_step_alone(pkg, name, which):
    """lr = 0: the delta is exactly 0, so every component the schedule leaves alone is unchanged bit for bit and a stepped one shows
    its change alone.  Constrained matrices at ratios 1.000 / 1.01 / 1.05 / 1.5 (one per update_speed regime and the fixed point) and
    1.015 / 1.025 / 1.095 / 1.105 (the two sides of each threshold; none within 1e-3 of one, asserted), every component seeing
    each ratio over the rotations.  Selections: all constrained components at once (one run per rotation), the first and the last
    only (a strict subset), each alone in turn."""
    net = make_net(pkg, name)
    comps, cfg = net.components, net.cfg
    cons = R.constrained(comps)
    if which == "all":
        runs = [(set(cons), rot) for rot in range(len(RATIOS))]
    elif which == "first-and-last":
        runs = [({cons[0], cons[-1]}, rot) for rot in (1, 3, 5, 6)]
    else:
        runs = [({i}, (j - k) % len(RATIOS)) for k, i in enumerate(cons) for j in range(len(RATIOS))]  # component k alone, at RATIOS[j]
    if name == "full-k":  # (there for its 24 K slices, not for the regimes: the float32 oracle's plain loops take 0.1 s per matrix at this width)
        runs = runs[1:4:2]
    assert all(len(w) == (len(cons) if which == "all" else 2 if which == "first-and-last" else 1) for w, _ in runs)
    zeros = np.zeros(net.num_params, np.float32)
    ratios_gpu_ref = []
    speeds = set()
    for wanted, rot in runs:
        params, asked = _ratio_params(net, 31 + rot, rot)
        step = step_selecting(name, wanted)
        ref = R.update_ref64(comps, params, zeros, 0.0, float(cfg.num_sequences), cfg.max_param_change, step)
        assert set(ref["stepped"]) == wanted and not any(d.any() for d in ref["delta"])
        p, g = run_update(net, params, zeros, 0.0, float(cfg.num_sequences), step)
        untouched = np.ones(net.num_params, bool)
        for i in wanted:
            untouched[comps[i]["begin"]:comps[i]["begin"] + comps[i]["rows"] * comps[i]["cols"]] = False
        assert np.array_equal(p[untouched].view(np.uint32), params[untouched].view(np.uint32)) and not g.any()
        tag = "%s ortho %s rot%d" % (name, which, rot)
        res = check_stepped(tag, comps, p, ref, fixed_point={i for i in wanted if asked[i] == 1.0})
        ratios_gpu_ref += [e_gpu / e_ref for _, e_gpu, e_ref in res]
        speeds |= {s["update_speed"] for i, s in ref["stepped"].items() if asked[i] != 1.0}
        for i in wanted:  # a stepped matrix away from its fixed point did move
            if asked[i] != 1.0:
                n = comps[i]["rows"] * comps[i]["cols"]
                assert (p[comps[i]["begin"]:comps[i]["begin"] + n] != params[comps[i]["begin"]:comps[i]["begin"] + n]).any()
    net.close()
    if which != "first-and-last":
        assert speeds == {0.125, 0.0625, 0.03125}, speeds
    print("PARITY test_gpu_net_update %s ortho %s: e_gpu / e_ref min %.2f max %.2f over %d stepped matrices" %
          (name, which, min(ratios_gpu_ref), max(ratios_gpu_ref), len(ratios_gpu_ref)))


# ------------------------------------------------------------------------------------------------ 3.4 whole steps over a schedule
def _schedule_run(pkg, name, check):
    import torch
    net = make_net(pkg, name)
    comps, cfg = net.components, net.cfg
    l2s = float(cfg.num_sequences)
    params = init_params(net, 41)
    net.set_params(params)
    kinds = ["one-component", None, "component-and-global", None, "global-only", None]
    history, stepped_any, clipped_any = [], set(), 0
    for step in range(12):
        kind = kinds[step % len(kinds)]
        rng = np.random.default_rng(400 + step)
        norms = _clip_norms(comps, kind) if kind else [c["max_change"] * 10.0 ** -rng.uniform(0.5, 2.0) if c["max_change"] else None for c in comps]
        grads = random_grads(comps, net.num_params, 500 + step, norms, params, l2_scale=l2s if kind else 0.0)
        net.grads.copy_(torch.from_numpy(grads))
        net.update(LR, l2_regularize_scale=l2s, step=step)  # (parameters carried on the GPU)
        p = host(net.params).copy()
        history.append(p)
        if check:
            ref = R.update_ref64(comps, params, grads, LR, l2s, cfg.max_param_change, step)
            dn = np.sqrt(ref["dot"])
            assert all(abs(dn[i] / c["max_change"] - 1) >= 0.01 for i, c in enumerate(comps) if c["max_change"] and c["lr_factor"])
            assert abs(ref["param_delta"] / cfg.max_param_change - 1) >= 0.01 and ref["applied"]
            clipped_any += int((ref["factor"] < 1).any() or ref["scale"] < 1)
            tag = "%s schedule step %d" % (name, step)
            check_elements(tag, comps, params, p, ref, skip=set(ref["stepped"]))
            if kind:
                check_factors(tag, comps, params, p, ref)
            check_stepped(tag, comps, p, ref)
            stepped_any |= set(ref["stepped"])
            assert not host(net.grads).any()
        params = p  # the reference advances from the GPU's float32 parameters: errors do not compound
    net.close()
    if check:
        assert clipped_any >= 6 and len(stepped_any) >= 3, (clipped_any, stepped_any)
    return history


@pytest.mark.parametrize("name", ["ragged", "tiles", "mixed", "tall"])
def test_whole_step_over_a_schedule(pkg, name):
    """12 consecutive steps, fresh gradients each, clipping on in every other step, the schedule stepping what it steps: components
    it leaves alone at the element bar, stepped ones at the orthonormal bars (their change taken from the float64 matrix after the
    update).  The same 12 steps again give the same bits: every sum of optim_group.hip has a fixed order."""
    first = _schedule_run(pkg, name, check=True)
    second = _schedule_run(pkg, name, check=False)
    for step, (a, b) in enumerate(zip(first, second)):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (name, step)


# ------------------------------------------------------------------------------------------------ 3.6 a refused update
@pytest.mark.parametrize("name", ["ragged", "items"])
def test_infinite_change_is_refused(pkg, name):
    """One gradient element +inf in a middle component: nothing is applied, every parameter keeps its bits, the gradient buffer is
    zeroed all the same, and the next, finite update on the same net is a plain one (the factors are not sticky)."""
    net = make_net(pkg, name)
    comps, cfg = net.components, net.cfg
    l2s = float(cfg.num_sequences)
    params = init_params(net, 51)
    norms = [0.2 * c["max_change"] if c["max_change"] else None for c in comps]
    grads = random_grads(comps, net.num_params, 52, norms, params, l2_scale=l2s)
    mid = comps[len(comps) // 2]
    assert mid["lr_factor"] != 0.0 and mid["max_change"] != 0.0
    bad = grads.copy()
    bad[mid["begin"] + R.owned(mid) // 2] = np.inf
    step = step_selecting(name)
    ref_bad = R.update_ref64(comps, params, bad, LR, l2s, cfg.max_param_change, step)
    assert not ref_bad["applied"] and np.array_equal(ref_bad["params"], params.astype(np.float64))
    p, g = run_update(net, params, bad, LR, l2s, step)
    assert np.array_equal(p.view(np.uint32), params.view(np.uint32))
    assert not g.any()
    import torch
    net.grads.copy_(torch.from_numpy(grads))
    net.update(LR, l2_regularize_scale=l2s, step=step)
    p2, g2 = host(net.params).copy(), host(net.grads).copy()
    net.close()
    ref = R.update_ref64(comps, params, grads, LR, l2s, cfg.max_param_change, step)
    assert ref["applied"] and (ref["factor"] == 1).all() and ref["scale"] == 1.0 and not g2.any()
    check_elements(name + " after-refusal", comps, params, p2, ref)


# ------------------------------------------------------------------------------------------------ 3.7 lr_factor = 0 and L2
def test_frozen_components_and_l2(pkg):
    """set-learning-rate-factor 0 on tdnnf2.*: those components keep their bits at a step that selects none of them, and
    tdnnf2.linear still takes its orthonormal step when the schedule selects it (ConstrainOrthonormal does not look at the
    learning rate).  With zero gradients the step is p (1 - 2 l2_scale lr l2_c) per component, hidden and output l2 differing."""
    name = "ragged"
    net = make_net(pkg, name)
    cfg = net.cfg
    l2s = float(cfg.num_sequences)
    assert net.set_learning_rate_factor(0.0, "tdnnf2.*") == 2
    comps = net.components
    frozen = [i for i, c in enumerate(comps) if c["name"].startswith("tdnnf2.")]
    assert len(frozen) == 2 and all(comps[i]["lr_factor"] == 0.0 for i in frozen)
    lin = [i for i in frozen if comps[i]["name"] == "tdnnf2.linear"][0]
    params = init_params(net, 61)
    norms = [0.2 * c["max_change"] if c["max_change"] else None for c in comps]
    grads = random_grads(comps, net.num_params, 62, norms, params, l2_scale=l2s)
    for i in frozen:  # the frozen components do have gradients
        assert grads[comps[i]["begin"]:comps[i]["begin"] + R.owned(comps[i])].any()
    # (i) nothing selected
    step = step_selecting(name)
    ref = R.update_ref64(comps, params, grads, LR, l2s, cfg.max_param_change, step)
    p, g = run_update(net, params, grads, LR, l2s, step)
    rng = R.ranges(comps, net.num_params)
    for i in frozen:
        b, e = rng[i]
        assert np.array_equal(p[b:e].view(np.uint32), params[b:e].view(np.uint32)), comps[i]["name"]
    check_elements("ragged frozen", comps, params, p, ref)
    assert not g.any()
    # (ii) tdnnf2.linear selected, alone
    step = step_selecting(name, {lin})
    ref = R.update_ref64(comps, params, grads, LR, l2s, cfg.max_param_change, step)
    p, g = run_update(net, params, grads, LR, l2s, step)
    b, e = rng[lin]
    assert (p[b:e] != params[b:e]).any() and set(ref["stepped"]) == {lin} and not ref["delta"][lin].any()
    check_elements("ragged frozen-stepped", comps, params, p, ref, skip={lin})
    assert len(check_stepped("ragged frozen-stepped", comps, p, ref)) == 1
    aff = [i for i in frozen if i != lin][0]
    assert np.array_equal(p[rng[aff][0]:rng[aff][1]].view(np.uint32), params[rng[aff][0]:rng[aff][1]].view(np.uint32))
    # (iii) L2 alone
    assert net.set_learning_rate_factor(1.0, "tdnnf2.*") == 2
    comps = net.components
    zeros = np.zeros(net.num_params, np.float32)
    step = step_selecting(name)
    ref = R.update_ref64(comps, params, zeros, LR, l2s, cfg.max_param_change, step)
    assert (ref["factor"] == 1).all() and ref["scale"] == 1.0
    p, g = run_update(net, params, zeros, LR, l2s, step)
    net.close()
    check_elements("ragged l2-only", comps, params, p, ref)
    seen = set()
    for c, (b, e) in zip(comps, rng):
        if c["lr_factor"] == 0.0:
            continue
        shrink = 1.0 - 2.0 * l2s * LR * float(np.float32(c["lr_factor"])) * float(np.float32(c["l2"]))
        want = params[b:e].astype(np.float64) * shrink
        assert np.abs(p[b:e] - want).max() <= U24 * np.abs(want).max() + 8 * U24 * (1 - shrink) * np.abs(params[b:e]).max(), c["name"]
        seen.add(round(shrink, 6))
    assert len(seen) >= 2, seen  # hidden and output components at their different l2


# ------------------------------------------------------------------------------------------------ 3.8 BatchNorm statistics
@pytest.mark.parametrize("case", ["scaled", "scale-one", "cv-update"])
def test_batchnorm_statistics_scaling(pkg, case):
    """ScaleBatchnormStats: one update multiplies every BatchNorm block by float64(float32(batchnorm_stats_scale)) exactly and leaves
    every ReLU block alone; with scale 1.0, and in cv-update mode (BatchNormTest components), nothing changes."""
    if case == "cv-update":
        cfg = pkg.trainer.make_config(**dict(_D, darts_num_offsets=4, darts_flags=1 | 16, darts_temp_proportion=0.9, cv_update=1))
    else:
        cfg = make_cfg(pkg, "ragged")
        if case == "scale-one":
            cfg.batchnorm_stats_scale = 1.0
    net = pkg.trainer.ChainNet(cfg)
    blocks, total = R.stat_blocks(cfg)
    stats = np.random.default_rng(71).uniform(0.5, 100.0, total)
    assert net.get_stats().size == total
    net.set_stats(stats)
    assert np.array_equal(net.get_stats(), stats)
    net.set_params(init_params(net, 72))
    net.grads.zero_()
    net.update(LR, step=0)
    got = net.get_stats()
    net.close()
    s = float(np.float32(cfg.batchnorm_stats_scale))
    assert (s == 1.0) == (case == "scale-one") and (case != "scaled" or s == float(np.float32(0.8)))
    for relu, b, e in blocks:
        want = stats[b:e] if relu or case != "scaled" else stats[b:e] * s
        assert np.array_equal(got[b:e], want), (case, relu, b)
    assert np.array_equal(got, R.scale_batchnorm_stats64(stats, cfg))
    assert (case == "scaled") == (not np.array_equal(got, stats))
