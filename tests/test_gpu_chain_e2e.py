"""-m gpu: the chain objective with an END-TO-END supervision (tdnnf_supervision_create_e2e: one cyclic graph per sequence, the numerator of
flat-start LF-MMI; csrc/chain_num_e2e.hip, csrc/num_e2e_kernels.h).

1. where both kinds apply (a time-synchronous supervision and the same graphs as an end-to-end one) the two numerators agree: results[3]
   1e-9 relative, [0] 1e-9 (|num| + |den|), [4] [5] [2] [1] bit-equal, deriv and xent_deriv elementwise within 4 * 2^-23 * weight (each
   path rounds weight * gamma to float once and the sum with the denominator's term once; both terms are bounded by weight);
2. cyclic graphs against tests/chain_e2e_ref64.py, one case per launch form of the recursion (threads x where the state vectors and the
   output rows live; the posterior kernel's four forms, threads x LDS or scratch, are among them), on sub-matrix views, with canaries; bars: [3] 1e-9, [4] [6] 1e-6 relative, [0] 1e-6 (|num| + |den|), xent_deriv
   elementwise 2 float32 ulps at xent_regularize * weight, deriv rel_l2 < 1e-4 (tests/test_gpu_chain_hostile.py, tests/test_gpu_posteriors.py);
3. the failure path (a sequence without a path of T arcs), and a good minibatch on the same workspace behind it;
4. tdnnf_chain_objf on the same cases; 5. determinism and tdnnf_chain_numerator_part 1, 4, 2; 6. argument errors;
7. the numerator and AlignGraphs.posteriors run the same device code on the same tables: log-probs and posteriors have the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import chain_e2e_ref64 as E
from tests import chain_ref64 as R
from tests.gpu_util import Hip, dev, host, rel_l2
from tests.view_layouts import laid_out

pytestmark = pytest.mark.gpu
XENT = 0.1
ULP1 = 2.0 ** -23


@pytest.fixture(scope="module")
def hip(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Hip(pkg)


class _Mode:
    def __init__(self, pkg, mode):
        self.pkg, self.mode = pkg, mode

    def __enter__(self):
        self.pkg.hipabi.check(self.pkg.hipabi.load().tdnnf_chain_set_denominator_mode(self.mode))

    def __exit__(self, *exc):
        self.pkg.hipabi.load().tdnnf_chain_set_denominator_mode(0)
        return False


_dens = {}


def _den(pkg, H, P):
    """(dict, device handle) of a small denominator graph, shared"""
    if (H, P) not in _dens:
        g = R.graph(pkg, H, P)
        _dens[(H, P)] = (g, pkg.hipabi.DenGraph(g))
    return _dens[(H, P)]


def _full(hip, dg, ds, y, xo, leaky, l2, d, xd, ws=None):
    """results[8] of tdnnf_chain_objf_and_deriv on a NaN-filled workspace (or the caller's); d / xd are written in place"""
    nb = hip.chain_workspace_bytes(dg.h, ds.B, ds.T)
    if ws is None:
        ws = hip.ws(nb)
        ws.fill_(float("nan"))
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    hip.chain_objf_and_deriv(dg.h, ds.h, y, xo, leaky, l2, XENT, hip.vec(res), d, xd, hip.vec(ws), nb, hip.stream())
    return host(res).copy()


def _objf(hip, dg, ds, y, xo, leaky, l2):
    nb = hip.chain_objf_workspace_bytes(dg.h, ds.B, ds.T)
    ws = hip.ws(nb)
    ws.fill_(float("nan"))
    res = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    hip.chain_objf(dg.h, ds.h, y, xo, leaky, l2, hip.vec(res), hip.vec(ws), nb, hip.stream())
    return host(res).copy()


# ------------------------------------------------------------------------------------------------ 1. same answer where both kinds apply
# the persistent-form shapes of tests/test_gpu_chain_hostile.py: (denominator mode, states, pdfs, sequences, frames)
SAME_SHAPES = {"split-fast": (3, 300, 150, 3, 40), "serial-fast": (4, 300, 150, 3, 40), "split-plain-loop": (3, 4200, 64, 2, 12)}
SAME = [(f, d, lk) for f in SAME_SHAPES for d in ("peaky", "beyond") for lk in (0.1, 1e-5)] + [("split-fast", "long-peaky", lk) for lk in (0.1, 1e-5)]


_same = {}


def _same_runs(hip, ora, pkg, family, data, leaky):
    """(results, deriv, xent_deriv) of one call with the time-synchronous supervision, one with its end-to-end form and a second with the
    time-synchronous one, computed once"""
    key = (family, data, leaky)
    if key in _same:
        return _same[key]
    mode, H, P, B, T = SAME_SHAPES[family]
    if data == "long-peaky":
        B, T = 2, 150
    c = R.make_case(pkg, ora, data, H, P, B, T, leaky)
    _, dg = _den(pkg, H, P)
    sync = pkg.hipabi.Supervision(c.sup)
    e2e = pkg.hipabi.Supervision(pkg.synth.e2e_supervision_from_supervision(c.sup, P))
    assert (sync.kind, e2e.kind) == (0, 1)
    print("E2E same-answer %s %s: form %r" % (family, data, e2e.e2e_form()))
    rng = np.random.default_rng(3)
    yd, xod = dev(c.y.copy()), dev((-np.abs(rng.standard_normal(c.y.shape)) - 0.1).astype(np.float32))
    out = []
    with _Mode(pkg, mode):
        for ds in (sync, e2e, sync):
            d, xd = torch.full(yd.shape, 5.0, device="cuda"), torch.full(yd.shape, 5.0, device="cuda")
            r = _full(hip, dg, ds, yd, xod, leaky, 5e-5, d, xd)
            out.append((r, host(d).copy(), host(xd).copy()))
    _same[key] = (float(c.sup["weight"]), out)
    return _same[key]


@pytest.mark.parametrize("family,data,leaky", SAME, ids=["%s-%s-leaky%g" % c for c in SAME])
def test_same_answer_as_the_time_synchronous_numerator(hip, ora, pkg, family, data, leaky):
    w, ((ra, da, xa), (rb, db, xb), _) = _same_runs(hip, ora, pkg, family, data, leaky)
    e = dict(num=abs(rb[3] - ra[3]) / abs(ra[3]), objf=abs(rb[0] - ra[0]) / (abs(ra[3]) + abs(ra[4])), deriv=float(np.abs(db - da).max()),
             xent=float(np.abs(xb - xa).max()))
    print("E2E same-answer %s %s leaky %g: num %.2e objf %.2e (bars 1e-9) deriv max abs %.2e (bar %.2e) xent_deriv %.2e (bar %.2e) xent objf %r / %r"
          % (family, data, leaky, e["num"], e["objf"], e["deriv"], 4 * ULP1 * w, e["xent"], 4 * ULP1 * w * XENT, ra[6], rb[6]))
    assert ra[5] == 1.0
    assert e["num"] <= 1e-9 and e["objf"] <= 1e-9
    for k in (4, 5, 2, 1):
        assert ra[k] == rb[k], (k, ra[k], rb[k])
    assert e["deriv"] <= 4 * ULP1 * w and e["xent"] <= 4 * ULP1 * w * XENT


def test_same_answer_l2_term_has_the_same_bits(hip, ora, pkg):
    """results[1] of every case above: the same bits from the time-synchronous call, the end-to-end call and a second time-synchronous
    call.  (chain_finish once added per-block sums of squares with atomicAdd on a double, in the order the blocks arrived: the term then
    differed by 1 - 4 ulps of a double between ANY two calls, measured here on an MI355X in 9 of 14 cases between two calls with the same
    supervision.  It now sums per-block partial sums in ascending order, as tdnnf_chain_objf always did.)"""
    for family, data, leaky in SAME:
        w, ((ra, _, _), (rb, _, _), (rc, _, _)) = _same_runs(hip, ora, pkg, family, data, leaky)
        print("E2E same-answer l2 term %s %s leaky %g: time-synchronous %r / end-to-end %r / time-synchronous again %r"
              % (family, data, leaky, ra[1], rb[1], rc[1]))
        assert ra[1] != 0.0 and ra[1] == rb[1] == rc[1], (family, data, leaky, ra[1], rb[1], rc[1])


# ------------------------------------------------------------------------------------------------ 2. cyclic graphs against float64
def _small(pkg, T, P, seed):
    return pkg.synth.make_e2e_supervision(1, T, P, units=(2, 6), seed=seed)["graphs"][0]


def _medium(pkg, T, P, seed):
    """65-300 states: a one-unit transcript beside a 100-unit alternative; with its self-loops the main unit accepts any T >= 1"""
    rng = np.random.default_rng(seed)
    return pkg.synth.make_alignment_graph(rng.integers(0, P, size=1), alternatives={0: rng.integers(0, P, size=100)}, seed=seed, num_pdfs=P)


def _heavy(pkg, T, P, seed):
    """81 states, every main unit but the last optional: the last unit has 80 incoming arcs (a heavy row), which all carry its pdf (a heavy pdf)"""
    rng = np.random.default_rng(seed)
    g = pkg.synth.make_alignment_graph(rng.integers(0, P, size=80), optional=range(79), seed=seed, num_pdfs=P)
    assert np.bincount(g["dst"]).max() > 64 and np.bincount(g["pdf"]).max() > 64
    return g


def _big(pkg, T, P, seed):
    """more than 1024 states: the free path through an 1100-state denominator graph, every state final"""
    return pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(1100, P, mean_out_degree=4.0, seed=seed))


_KINDS = {"s": _small, "m": _medium, "h": _heavy, "b": _big}
# name: (graphs of the minibatch, T, P, weight, align_form at creation, xent head, l2_regularize, view layout or None, (threads, vectors in LDS, rows in LDS))
CYCLIC = {
    "64-rows-lds": ("s", 1, 41, 1.0, 0, True, 0.0, None, (64, 1, 1)),
    "64-rows-lds-noxent": ("sss", 2, 41, 0.75, 0, False, 5e-5, "pitched", (64, 1, 1)),
    "256-rows-lds": ("shs", 7, 41, 1.0, 0, True, 5e-5, "off1-odd", (256, 1, 1)),
    "256-rows-lds-T33": ("smshs", 33, 41, 0.75, 0, True, 0.0, "off1", (256, 1, 1)),
    "1024-rows-lds": ("bs", 7, 41, 1.0, 0, True, 5e-5, "pitched", (1024, 1, 1)),
    "64-global": ("sss", 7, 41, 0.75, 2, True, 0.0, "off1", (64, 0, 0)),
    "256-global": ("hms", 33, 41, 1.0, 2, False, 0.0, None, (256, 0, 0)),
    "1024-global": ("bs", 2, 41, 1.0, 2, True, 5e-5, "odd-stride", (1024, 0, 0)),
    # (more pdfs than 8 x threads: the rows are not staged; cases of this test's own beside the P = 41 ones)
    "64-lds-P600": ("sss", 7, 600, 1.0, 0, True, 0.0, "pitched", (64, 1, 0)),
    "256-lds-P2100": ("h", 2, 2100, 0.75, 0, True, 5e-5, None, (256, 1, 0)),
    "1024-lds-P8200": ("b", 1, 8200, 1.0, 0, True, 0.0, None, (1024, 1, 0)),
}
_cyclic = {}


def _cyclic_case(pkg, name):
    """the minibatch, its inputs and its float64 reference, computed once"""
    if name in _cyclic:
        return _cyclic[name]
    kinds, T, P, w, form, xent, l2, layout, want = CYCLIC[name]
    B = len(kinds)
    seed = sorted(CYCLIC).index(name)
    graphs = [_KINDS[k](pkg, T, P, 100 * seed + i) for i, k in enumerate(kinds)]
    c = dict(e2e={"B": B, "T": T, "P": P, "weight": w, "graphs": graphs}, B=B, T=T, P=P, w=w)
    rng = np.random.default_rng(seed)
    c["y"] = (1.5 * rng.standard_normal((T * B, P))).astype(np.float32)
    xo = rng.standard_normal((T * B, P))
    c["xo"] = (xo - np.log(np.exp(xo).sum(1, keepdims=True))).astype(np.float32) if xent else None
    c["den"], _ = _den(pkg, 30, P)
    c["ref"] = E.objective(c["den"], c["e2e"], c["y"], 0.1, float(np.float32(l2)), float(np.float32(XENT)), c["xo"])  # (the C ABI takes floats)
    assert c["ref"].ok
    c["sync"] = pkg.synth.make_supervision(B, T, P, max_alt=1, seed=seed, weight=w)  # names one pdf per frame: for the denominator-only canary
    _cyclic[name] = c
    return c


def _views(c, layout):
    """y, xent_output (read: NaN guards), deriv, xent_deriv (written: pattern guards) in the case's layout"""
    if layout is None:
        fresh = lambda: torch.full((c["T"] * c["B"], c["P"]), 5.0, device="cuda")
        return dev(c["y"]), dev(c["xo"]) if c["xo"] is not None else None, fresh(), fresh(), []
    five = np.full(c["y"].shape, 5.0, dtype=np.float32)
    yv, _, cy = laid_out(c["y"], layout)
    xov, cx = None, lambda: None
    if c["xo"] is not None:
        xov, _, cx = laid_out(c["xo"], layout)
    dv, _, cd = laid_out(five, layout, writes=True)
    xdv, _, cxd = laid_out(five, layout, writes=True)
    return yv, xov, dv, xdv, [cy, cx, cd, cxd]


def _check_cyclic(c, name, r, d, xd, l2):
    ref, w = c["ref"], c["w"]
    e = dict(num=abs(r[3] - ref.num) / abs(ref.num), den=abs(r[4] - ref.den) / abs(ref.den), objf=abs(r[0] - ref.objf) / (abs(ref.num) + abs(ref.den)),
             xobjf=abs(r[6] - ref.xent_objf) / abs(ref.xent_objf) if c["xo"] is not None else abs(r[6]), deriv=rel_l2(d, ref.deriv),
             xent=float(np.abs(xd.astype(np.float64) - ref.xent_deriv).max()))
    xbar = 2 * float(np.spacing(np.float32(XENT * w)))
    print("E2E cyclic %s: num %.2e (bar 1e-9) den %.2e objf %.2e xent objf %.2e (bars 1e-6) deriv rel_l2 %.2e (bar 1e-4) xent_deriv max abs %.2e (bar %.2e)"
          % (name, e["num"], e["den"], e["objf"], e["xobjf"], e["deriv"], e["xent"], xbar))
    assert r[5] == 1.0 and r[2] == ref.weight
    assert e["num"] <= 1e-9 and e["den"] <= 1e-6 and e["objf"] <= 1e-6 and e["xobjf"] <= 1e-6
    assert abs(r[1] - ref.l2_term) <= 1e-9 * abs(ref.l2_term) if l2 else r[1] == 0.0
    assert e["xent"] <= xbar and e["deriv"] < 1e-4


def _named(graphs_or_sync, B, T, P):
    """[T * B, P] bool: the pdf is named by an arc of the row's sequence (end-to-end graphs: at every frame alike)"""
    m = np.zeros((T * B, P), dtype=bool)
    if isinstance(graphs_or_sync, dict):
        sup = graphs_or_sync
        for s in range(B):
            for t in range(T):
                m[t * B + s, R.supervision_pdfs(sup, s, t)] = True
    else:
        for s, g in enumerate(graphs_or_sync):
            m[s::B, np.unique(g["pdf"])] = True
    return m


@pytest.mark.parametrize("name", list(CYCLIC))
def test_cyclic_graphs_against_float64(hip, pkg, name):
    kinds, T, P, w, form, xent, l2, layout, want = CYCLIC[name]
    c = _cyclic_case(pkg, name)
    _, dg = _den(pkg, 30, P)
    with pkg.hipabi.option("align_form", form):
        ds = pkg.hipabi.Supervision(c["e2e"])
    f = ds.e2e_form()
    states = [int(g["S"]) for g in c["e2e"]["graphs"]]
    # (the posterior kernel has four forms, which follow from the same facts: 1024 threads above 1024 states, alpha / beta staged in LDS
    # where the recursion's vectors live there -- 256 and 1024 threads x LDS and scratch are all among the cases)
    print("E2E cyclic %s: recursion form %r, posterior kernel %d threads, vectors %s; states %r"
          % (name, f, 1024 if max(states) > 1024 else 256, "staged in LDS" if f["vectors_in_lds"] else "gathered from the scratch", states))
    assert (f["threads"], f["vectors_in_lds"], f["rows_in_lds"]) == want  # the case selects the form its name says
    info = ds.info()
    assert info == dict(num_states=sum(int(g["S"]) for g in c["e2e"]["graphs"]), num_arcs=sum(len(g["src"]) for g in c["e2e"]["graphs"]),
                        max_states_per_frame=max(int(g["S"]) for g in c["e2e"]["graphs"]), wide=0)
    yv, xov, dv, xdv, checks = _views(c, layout)
    r = _full(hip, dg, ds, yv, xov, 0.1, l2, dv, xdv)
    d, xd = host(dv).copy(), host(xdv).copy()
    for chk in checks:
        chk()  # columns and rows outside the views are unchanged
    assert np.array_equal(host(yv), c["y"])
    _check_cyclic(c, name, r, d, xd, l2)
    # canary: where neither supervision names the pdf, deriv is the denominator's (and the l2 term's) value of an ordinary call, bit for bit
    yv2, xov2, dv2, xdv2, _ = _views(c, layout)
    r2 = _full(hip, dg, pkg.hipabi.Supervision(c["sync"]), yv2, xov2, 0.1, l2, dv2, xdv2)
    assert r2[5] == 1.0 and r2[4] == r[4]
    free = ~(_named(c["e2e"]["graphs"], c["B"], T, P) | _named(c["sync"], c["B"], T, P))
    assert free.any()
    assert np.array_equal(d[free], host(dv2)[free])
    assert not xd[~_named(c["e2e"]["graphs"], c["B"], T, P)].any()  # xent_deriv: zero-filled, then the named pdfs only


# ------------------------------------------------------------------------------------------------ 3. failure path
def test_failure_path_then_a_good_minibatch_on_the_same_workspace(hip, pkg):
    name = "256-rows-lds"
    c = _cyclic_case(pkg, name)
    B, T, P, w = c["B"], c["T"], c["P"], 0.75
    bad = dict(c["e2e"], weight=w, graphs=list(c["e2e"]["graphs"]))
    bad["graphs"][1] = pkg.synth.make_alignment_graph(np.arange(T + 3) % P, seed=1, num_pdfs=P)  # shortest accepting path: T + 3 arcs
    ref = E.objective(c["den"], bad, c["y"], 0.1, float(np.float32(5e-5)), float(np.float32(XENT)), c["xo"])
    assert not ref.ok and ref.objf == -10.0 * w * B * T and not ref.deriv.any()
    _, dg = _den(pkg, 30, P)
    ds_bad, ds_good = pkg.hipabi.Supervision(bad), pkg.hipabi.Supervision(c["e2e"])
    nb = hip.chain_workspace_bytes(dg.h, B, T)
    ws = hip.ws(nb)
    ws.fill_(float("nan"))
    yd, xod = dev(c["y"]), dev(c["xo"])
    d, xd = torch.full(yd.shape, 5.0, device="cuda"), torch.full(yd.shape, 5.0, device="cuda")
    r = _full(hip, dg, ds_bad, yd, xod, 0.1, 5e-5, d, xd, ws=ws)
    assert r[5] == 0.0 and r[0] == -10.0 * w * B * T and r[6] == 0.0 and r[2] == w * B * T
    assert not host(d).any() and not host(xd).any()
    ro = _objf(hip, dg, ds_bad, yd, xod, 0.1, 5e-5)
    assert ro[5] == 0.0 and ro[0] == r[0] and ro[6] == 0.0
    d.fill_(5.0)
    xd.fill_(5.0)
    r = _full(hip, dg, ds_good, yd, xod, 0.1, CYCLIC[name][6], d, xd, ws=ws)
    _check_cyclic(c, name + " (behind a failed minibatch)", r, host(d).copy(), host(xd).copy(), CYCLIC[name][6])


# ------------------------------------------------------------------------------------------------ 4. tdnnf_chain_objf
def _objf_runs(hip, pkg, name):
    kinds, T, P, w, form, xent, l2, layout, want = CYCLIC[name]
    c = _cyclic_case(pkg, name)
    _, dg = _den(pkg, 30, P)
    with pkg.hipabi.option("align_form", form):
        ds, fresh = pkg.hipabi.Supervision(c["e2e"]), pkg.hipabi.Supervision(c["e2e"])
    yv, xov, dv, xdv, checks = _views(c, layout)
    full_fresh = _full(hip, dg, fresh, yv, xov, 0.1, l2, dv, xdv)
    d_fresh, xd_fresh = host(dv).copy(), host(xdv).copy()
    o1, o2 = _objf(hip, dg, ds, yv, xov, 0.1, l2), _objf(hip, dg, ds, yv, xov, 0.1, l2)
    n1, n2 = _objf(hip, dg, ds, yv, None, 0.1, l2), _objf(hip, dg, ds, yv, None, 0.1, l2)  # forward-only recursion: nothing kept per frame
    dv.fill_(5.0)
    xdv.fill_(5.0)
    full = _full(hip, dg, ds, yv, xov, 0.1, l2, dv, xdv)
    for chk in checks:
        chk()
    return c, full, full_fresh, (host(dv).copy(), host(xdv).copy()), (d_fresh, xd_fresh), (o1, o2), (n1, n2)


@pytest.mark.parametrize("name", list(CYCLIC))
def test_chain_objf_numerator_entries(hip, pkg, name):
    """The entries the numerator forms: [3] has the recursion's bits (with an xent_output the same kernel runs; without one its forward-only
    form, the same arithmetic in the same order), [6] comes from the same posterior kernel in its objective-only mode; [2] and [5]; two calls
    give the same bits; a full call behind the objective-only ones has the bits of a fresh supervision's."""
    c, full, full_fresh, (d, xd), (d_fresh, xd_fresh), (o1, o2), (n1, n2) = _objf_runs(hip, pkg, name)
    assert np.array_equal(o1, o2) and np.array_equal(n1, n2)
    assert o1[3] == full[3] and n1[3] == full[3]
    assert o1[2] == full[2] and o1[5] == full[5] == 1.0 and n1[5] == 1.0
    assert abs(o1[6] - full[6]) <= 1e-12 * abs(full[6]) and n1[6] == 0.0
    assert np.array_equal(full, full_fresh) and np.array_equal(d, d_fresh) and np.array_equal(xd, xd_fresh)


@pytest.mark.parametrize("name", list(CYCLIC))
def test_chain_objf_every_entry(hip, pkg, name):
    """Every entry of tdnnf_chain_objf's results within 1e-12 relative of tdnnf_chain_objf_and_deriv's."""
    c, full, _, _, _, (o1, _), _ = _objf_runs(hip, pkg, name)
    rel = [abs(o1[k] - full[k]) / max(abs(full[k]), 1e-300) for k in range(7)]
    print("E2E chain_objf %s: relative differences of results[0..6] from the full call %s" % (name, " ".join("%.2e" % v for v in rel)))
    assert max(rel) <= 1e-12, rel


# ------------------------------------------------------------------------------------------------ 5. determinism and parts
@pytest.mark.parametrize("name", list(CYCLIC))
def test_two_calls_give_the_same_bits(hip, pkg, name):
    kinds, T, P, w, form, xent, l2, layout, want = CYCLIC[name]
    c = _cyclic_case(pkg, name)
    _, dg = _den(pkg, 30, P)
    with pkg.hipabi.option("align_form", form):
        ds = pkg.hipabi.Supervision(c["e2e"])
    yd, xod = dev(c["y"]), dev(c["xo"]) if c["xo"] is not None else None
    runs = []
    for _ in range(2):
        d, xd = torch.full(yd.shape, 5.0, device="cuda"), torch.full(yd.shape, 5.0, device="cuda")
        runs.append((_full(hip, dg, ds, yd, xod, 0.1, l2, d, xd), host(d).copy(), host(xd).copy()))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# (cases whose graphs leave pdfs unnamed: the auxiliary supervision below lives on those)
@pytest.mark.parametrize("name", ["64-global", "64-lds-P600", "256-lds-P2100", "1024-lds-P8200"])
def test_the_three_parts_give_the_bits_of_the_whole_call(hip, pkg, name):
    """tdnnf_chain_numerator_part 1, 4, 2 behind the denominator.  The library has no entry that leaves the denominator's term alone, so the
    term comes from a whole call (mode 4: every launch on the caller's stream) with an AUXILIARY time-synchronous supervision that names only
    pdfs no graph of the case names: everywhere else its derivative is the denominator's.  Parts 1, 4, 2 of the end-to-end supervision on
    top of that matrix then give the whole end-to-end call's bits wherever the auxiliary supervision named nothing; xent_deriv, which
    part 4 adds onto zeros as the whole call does, everywhere."""
    kinds, T, P, w, form, xent, l2, layout, want = CYCLIC[name]
    c = _cyclic_case(pkg, name)
    B = c["B"]
    _, dg = _den(pkg, 30, P)
    with pkg.hipabi.option("align_form", form):
        ds = pkg.hipabi.Supervision(c["e2e"])
    unnamed = np.setdiff1d(np.arange(P), np.concatenate([g["pdf"] for g in c["e2e"]["graphs"]]))
    assert len(unnamed) >= 2
    aux = pkg.synth.make_supervision(B, T, len(unnamed), max_alt=1, seed=1, weight=w)
    aux["arc_pdf"] = unnamed[aux["arc_pdf"]].astype(np.int32)
    aux_named = _named(aux, B, T, P)
    yd = dev(c["y"])
    with _Mode(pkg, 4):
        nb = hip.chain_workspace_bytes(dg.h, B, T)
        ws = hip.ws(nb)
        ws.fill_(float("nan"))
        d, xd = torch.full(yd.shape, 5.0, device="cuda"), torch.full(yd.shape, 5.0, device="cuda")
        whole = _full(hip, dg, ds, yd, None, 0.1, 0.0, d, xd, ws=ws)
        d_whole, xd_whole = host(d).copy(), host(xd).copy()
        _full(hip, dg, pkg.hipabi.Supervision(aux), yd, None, 0.1, 0.0, d, xd, ws=ws)  # d: the denominator's term off aux_named
        xd.fill_(0.0)
        res = torch.zeros(8, dtype=torch.float64, device="cuda")
        hip.chain_numerator_part(dg.h, ds.h, yd, 1, hip.vec(res), None, None, hip.vec(ws), nb, hip.stream())
        hip.chain_numerator_part(dg.h, ds.h, yd, 4, hip.vec(res), None, xd, hip.vec(ws), nb, hip.stream())
        hip.chain_numerator_part(dg.h, ds.h, yd, 2, hip.vec(res), d, None, hip.vec(ws), nb, hip.stream())
        rp, d_parts, xd_parts = host(res).copy(), host(d).copy(), host(xd).copy()
    assert whole[5] == 1.0 and np.array_equal(rp[[0, 2, 3, 4, 5]], whole[[0, 2, 3, 4, 5]])
    assert np.array_equal(xd_parts, xd_whole)
    assert np.array_equal(d_parts[~aux_named], d_whole[~aux_named])
    assert _named(c["e2e"]["graphs"], B, T, P).sum() > 0 and not (aux_named & _named(c["e2e"]["graphs"], B, T, P)).any()


# ------------------------------------------------------------------------------------------------ 6. argument errors
def test_argument_errors(hip, pkg):
    abi, lib = pkg.hipabi, pkg.hipabi.load()
    P, T = 41, 7
    good = [_small(pkg, T, P, 1), _small(pkg, T, P, 2)]
    assert abi.Supervision.from_graphs(good, T, weight=0.5).kind == 1

    def broken(change, match):
        g = {k: np.array(v, copy=True) if isinstance(v, np.ndarray) else v for k, v in good[1].items()}
        change(g)
        with pytest.raises(abi.HipAbiError, match=match):
            abi.Supervision.from_graphs([good[0], g], T, num_pdfs=P)

    broken(lambda g: g["pdf"].__setitem__(0, P), "pdf")
    broken(lambda g: g["pdf"].__setitem__(0, -1), "pdf")
    broken(lambda g: g["dst"].__setitem__(0, int(g["S"])), "state")
    broken(lambda g: g["src"].__setitem__(0, -1 - int(good[0]["S"])), "state")
    broken(lambda g: g["init"].fill(-np.inf), "initial")
    broken(lambda g: g["final"].fill(-np.inf), "final")
    with pytest.raises(abi.HipAbiError, match="supervision_create_e2e"):
        abi.Supervision.from_graphs(good, 0)
    # num_pdfs above the denominator graph's
    _, dg = _den(pkg, 30, P)
    ds = abi.Supervision.from_graphs(good, T, num_pdfs=P + 1)
    B = 2
    y = torch.zeros(B * T, P, device="cuda")
    d = torch.zeros_like(y)
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    nb = lib.tdnnf_chain_workspace_bytes(dg.h, B, T)
    ws = abi.workspace(nb)
    args = lambda ds, y, d: (dg.h, ds.h, abi.pmat(y), None, 0.1, 0.0, XENT, abi.ptr(res), abi.pmat(d), None, abi.ptr(ws), nb, abi.stream())
    assert lib.tdnnf_chain_objf_and_deriv(*args(ds, y, d)) == 1 and b"num_pdfs" in lib.tdnnf_last_error()
    assert lib.tdnnf_chain_objf(dg.h, ds.h, abi.pmat(y), None, 0.1, 0.0, abi.ptr(res), abi.ptr(ws), nb, abi.stream()) == 1
    assert b"num_pdfs" in lib.tdnnf_last_error()
    assert lib.tdnnf_chain_numerator_part(dg.h, ds.h, abi.pmat(y), 1, abi.ptr(res), None, None, abi.ptr(ws), nb, abi.stream()) == 1
    assert b"num_pdfs" in lib.tdnnf_last_error()
    # mismatched B * T rows
    ds = abi.Supervision.from_graphs(good, T, num_pdfs=P)
    short = torch.zeros(B * T - 1, P, device="cuda")
    assert lib.tdnnf_chain_objf_and_deriv(*args(ds, short, torch.zeros_like(short))) == 1 and b"nnet_output" in lib.tdnnf_last_error()
    assert lib.tdnnf_supervision_kind(None) == -1


# ------------------------------------------------------------------------------------------------ 7. the bits of AlignGraphs.posteriors
def _dense(S, P, seed, heavy_state=None, heavy_pdf=None):
    """S states, all initial and final (every path of T arcs accepts), three arcs out of each (loop, next, seventh on) with pdfs below
    P - 4, so the last four are free: heavy_state gets arcs from further states until 65 enter it, heavy_pdf is put on 65 arcs."""
    rng = np.random.default_rng(seed)
    st = np.arange(S)
    src, dst = np.repeat(st, 3), np.stack([st, (st + 1) % S, (st + 7) % S], 1).reshape(-1)
    if heavy_state is not None:
        more = np.setdiff1d(st, src[dst == heavy_state])[:65 - int((dst == heavy_state).sum())]
        src, dst = np.concatenate([src, more]), np.concatenate([dst, np.full(len(more), heavy_state)])
    pdf = rng.integers(0, P - 4, size=len(src))
    if heavy_pdf is not None:
        pdf[rng.permutation(len(src))[:65]] = heavy_pdf
    f32 = lambda a: a.astype(np.float32)
    return {"S": S, "P": P, "src": src.astype(np.int32), "dst": dst.astype(np.int32), "pdf": pdf.astype(np.int32),
            "logprob": f32(-rng.random(len(src))), "init": f32(-rng.random(S)), "final": f32(-rng.random(S))}


@pytest.mark.parametrize("form", [1, 2], ids=["lds", "global"])
def test_numerator_has_the_bits_of_align_posteriors(hip, pkg, form):
    """Three graphs of 70 to 80 states (256 threads), T = 12, 40 pdfs, a state that 65 arcs enter and a pdf on 65 arcs (a heavy row by
    destination and one by pdf, beside light ones), vectors in LDS and in the scratch.  The supervision's recursion and
    AlignGraphs.posteriors(row_stride=B, acoustic_scale=1) walk the same tables with the same step in the same order, so
      * results[3] = weight * (num_lp[0] + num_lp[1] + num_lp[2]) (chain_finalize_kernel: from 0, ascending, weight 1) is that sum of the
        three logprobs, bit for bit;
      * parts 1 and 2 on a zeroed matrix (weight 1, no l2 term) leave (float)gamma: the bits of post on every pdf the sequence names, zero elsewhere."""
    B, T, P = 3, 12, 40
    graphs = [_dense(70, P, 1), _dense(77, P, 2, heavy_state=5), _dense(80, P, 3, heavy_pdf=P - 1)]
    assert np.bincount(graphs[1]["dst"]).max() == 65 and np.bincount(graphs[2]["pdf"]).max() == 65
    assert max(np.bincount(g["dst"]).max() for g in (graphs[0], graphs[2])) <= 64 and max(np.bincount(g["pdf"]).max() for g in graphs[:2]) <= 64
    named = _named(graphs, B, T, P)
    assert named.any() and not named.all()
    y = dev((1.5 * np.random.default_rng(7).standard_normal((T * B, P))).astype(np.float32))
    _, dg = _den(pkg, 30, P)
    with pkg.hipabi.option("align_form", form), _Mode(pkg, 4):
        ds = pkg.hipabi.Supervision({"B": B, "T": T, "P": P, "weight": 1.0, "graphs": graphs})
        f = ds.e2e_form()
        assert (f["threads"], f["vectors_in_lds"]) == (256, 1 if form == 1 else 0)
        post, res = pkg.hipabi.AlignGraphs(graphs, num_pdfs=P).posteriors(y, [T] * B, list(range(B)), row_stride=B, acoustic_scale=1.0)
        post, res = host(post).copy(), host(res).copy()
        nb = hip.chain_workspace_bytes(dg.h, B, T)
        ws = hip.ws(nb)
        ws.fill_(float("nan"))
        d, xd = torch.full(y.shape, 5.0, device="cuda"), torch.full(y.shape, 5.0, device="cuda")
        whole = _full(hip, dg, ds, y, None, 0.1, 0.0, d, xd, ws=ws)  # (leaves the denominator's log-probs, which part 2 reads, in ws)
        d.zero_()
        r = torch.zeros(8, dtype=torch.float64, device="cuda")
        hip.chain_numerator_part(dg.h, ds.h, y, 1, hip.vec(r), None, None, hip.vec(ws), nb, hip.stream())
        hip.chain_numerator_part(dg.h, ds.h, y, 2, hip.vec(r), d, None, hip.vec(ws), nb, hip.stream())
        parts, gamma = host(r).copy(), host(d).copy()
    lp = res[:, 0]
    want = ((np.float64(0.0) + lp[0]) + lp[1]) + lp[2]
    print("E2E bits of align_posteriors, align_form %d: form %r logprob %r sum %r results[3] %r / parts %r; posteriors differ in %d of %d named elements"
          % (form, f, lp.tolist(), want, whole[3], parts[3], int((gamma[named].view(np.uint32) != post[named].view(np.uint32)).sum()), int(named.sum())))
    assert np.all(res[:, 1] == 1.0) and whole[5] == 1.0 and parts[5] == 1.0
    assert whole[3] == want and parts[3] == want
    assert np.array_equal(gamma[named].view(np.uint32), post[named].view(np.uint32))
    assert post[named].any() and not gamma[~named].any() and not post[~named].any()
