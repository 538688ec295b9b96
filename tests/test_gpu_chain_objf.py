"""-m gpu: tdnnf_chain_objf (the chain objective without derivatives) against tdnnf_chain_objf_and_deriv on the same inputs, one case per
kernel variant of the objective-only denominator: persistent with the state vectors in LDS (FAST loop, plain loop, more pdfs than the
register-held part of the output row), persistent with the vectors in global memory, and the wide form on two alpha frames.

Bars: weight and ok flag equal; numerator, denominator and xent objective within 1e-6 relative and |d objf| <= 1e-6 (|num| + |den|) -- the
bar the project holds between two forms of the denominator (test_bench_shape_denominator_forms_agree); the l2 term within 1e-9 relative (a
double sum in another order)."""
import numpy as np
import pytest
import torch

from tests.gpu_util import Hip, dev, host, padded

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def hip(pkg):
    return Hip(pkg)


class _Mode:
    """tdnnf_chain_set_denominator_mode for a block; mode 0 again afterwards."""

    def __init__(self, pkg, mode):
        self.pkg, self.mode = pkg, mode

    def __enter__(self):
        self.pkg.hipabi.check(self.pkg.hipabi.load().tdnnf_chain_set_denominator_mode(self.mode))

    def __exit__(self, *exc):
        self.pkg.hipabi.load().tdnnf_chain_set_denominator_mode(0)
        return False


def _inputs(pkg, H, P, B, T, seed=0):
    g = pkg.synth.make_den_graph(H, P, mean_out_degree=4.0, seed=H + seed)
    sup = pkg.synth.make_supervision_from_den(g, B, T, num_paths=2, seed=T + seed)
    rng = np.random.default_rng(H + T + seed)
    return g, sup, rng.standard_normal((T * B, P)).astype(F), rng.standard_normal((T * B, P)).astype(F)


def _objf(hip, dg, ds, y, xo, leaky, l2, ws_bytes=None):
    """results of tdnnf_chain_objf on a NaN-filled workspace of its own size (or ws_bytes)"""
    nb = hip.chain_objf_workspace_bytes(dg.h, ds.B, ds.T) if ws_bytes is None else ws_bytes
    ws = hip.ws(nb)
    ws.fill_(float("nan"))
    res = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    hip.chain_objf(dg.h, ds.h, y, xo, leaky, l2, hip.vec(res), hip.vec(ws), nb, hip.stream())
    return host(res).copy()


def _reference(hip, dg, ds, y, xo, leaky, l2):
    nb = hip.chain_workspace_bytes(dg.h, ds.B, ds.T)
    ws = hip.ws(nb)
    ws.fill_(float("nan"))
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    d = torch.zeros(y.shape, device="cuda")
    hip.chain_objf_and_deriv(dg.h, ds.h, y, xo, leaky, l2, 0.1, hip.vec(res), d, None, hip.vec(ws), nb, hip.stream())
    return host(res).copy()


def _check(r, ref):
    print("CHAIN_OBJF objf %.17g / %.17g  num %.17g / %.17g  den %.17g / %.17g  xent %.17g / %.17g  l2 %.17g / %.17g"
          % (r[0], ref[0], r[3], ref[3], r[4], ref[4], r[6], ref[6], r[1], ref[1]))
    assert r[2] == ref[2] and r[5] == ref[5] == 1.0
    for k in (3, 4, 6):
        assert abs(r[k] - ref[k]) <= 1e-6 * abs(ref[k]), (k, r[k], ref[k])
    assert abs(r[0] - ref[0]) <= 1e-6 * (abs(ref[3]) + abs(ref[4])), (r[0], ref[0])
    assert abs(r[1] - ref[1]) <= 1e-9 * abs(ref[1]), (r[1], ref[1])


# (variant, denominator mode, states, pdfs, sequences, frames)
CASES = [
    ("persistent-fast", 3, 300, 150, 3, 7),
    ("persistent-fast-one-frame", 3, 300, 150, 3, 1),
    ("persistent-plain-loop", 3, 4200, 64, 2, 5),        # more than 4 096 states: not FAST
    ("persistent-row-beyond-registers", 3, 100, 8200, 2, 3),  # more than 8 192 pdfs
    ("persistent-global-vectors", 1, 13000, 40, 2, 4),   # P + 3 x states floats over the LDS budget
    ("wide-ragged-group-of-16", 2, 200, 150, 5, 6),
    ("wide-full-32-and-ragged", 2, 200, 150, 40, 6),
]


@pytest.mark.parametrize("name,mode,H,P,B,T", CASES, ids=[c[0] for c in CASES])
def test_chain_objf_matches_objf_and_deriv(hip, pkg, name, mode, H, P, B, T):
    g, sup, y, xo = _inputs(pkg, H, P, B, T)
    dg, ds = pkg.hipabi.DenGraph(g), pkg.hipabi.Supervision(sup)
    yd, xod = dev(y), dev(xo)
    with _Mode(pkg, mode):
        nb, nb_full = hip.chain_objf_workspace_bytes(dg.h, B, T), hip.chain_workspace_bytes(dg.h, B, T)
        assert 0 < nb <= nb_full
        r = _objf(hip, dg, ds, yd, xod, 0.1, 0.01)
        _check(r, _reference(hip, dg, ds, yd, xod, 0.1, 0.01))
        # two calls: the same bits; and a workspace of the full entry's size is accepted
        assert np.array_equal(_objf(hip, dg, ds, yd, xod, 0.1, 0.01), r)
        assert np.array_equal(_objf(hip, dg, ds, yd, xod, 0.1, 0.01, ws_bytes=nb_full), r)


@pytest.mark.parametrize("mode", [3, 2], ids=["persistent", "wide"])
def test_chain_objf_without_leaky_hmm_and_without_xent_output(hip, pkg, mode):
    g, sup, y, xo = _inputs(pkg, 300, 150, 3, 7, seed=1)
    dg, ds = pkg.hipabi.DenGraph(g), pkg.hipabi.Supervision(sup)
    yd, xod = dev(y), dev(xo)
    with _Mode(pkg, mode):
        _check(_objf(hip, dg, ds, yd, xod, 0.0, 0.01), _reference(hip, dg, ds, yd, xod, 0.0, 0.01))
        r = _objf(hip, dg, ds, yd, None, 0.1, 0.01)
        _check(r, _reference(hip, dg, ds, yd, None, 0.1, 0.01))
        assert r[6] == 0.0


@pytest.mark.parametrize("mode", [3, 2], ids=["persistent", "wide"])
def test_chain_objf_on_column_views(hip, pkg, mode):
    g, sup, y, xo = _inputs(pkg, 300, 150, 3, 7, seed=2)
    dg, ds = pkg.hipabi.DenGraph(g), pkg.hipabi.Supervision(sup)
    (yv, ybuf), (xv, xbuf) = padded(y), padded(xo)
    assert yv.stride(0) > yv.shape[1]
    with _Mode(pkg, mode):
        r = _objf(hip, dg, ds, yv, xv, 0.1, 0.01)
        assert np.array_equal(r, _objf(hip, dg, ds, dev(y), dev(xo), 0.1, 0.01))  # the view changes nothing
        _check(r, _reference(hip, dg, ds, yv, xv, 0.1, 0.01))
    assert (host(ybuf)[:, y.shape[1]:] == 7.0).all() and (host(xbuf)[:, y.shape[1]:] == 7.0).all()
    assert np.array_equal(host(yv), y) and np.array_equal(host(xv), xo)  # inputs are read only


def test_chain_objf_with_the_wide_numerator(hip, pkg):
    g, sup, y, xo = _inputs(pkg, 300, 150, 3, 7, seed=3)
    dg = pkg.hipabi.DenGraph(g)
    yd, xod = dev(y), dev(xo)
    with _Mode(pkg, 3), pkg.hipabi.option("num_form", 2):
        ds = pkg.hipabi.Supervision(sup)  # created under the option: it carries the wide form's arc lists
        _check(_objf(hip, dg, ds, yd, xod, 0.1, 0.01), _reference(hip, dg, ds, yd, xod, 0.1, 0.01))


@pytest.mark.parametrize("mode", [3, 2], ids=["persistent", "wide"])
def test_chain_objf_failure_path(hip, pkg, mode):
    g, sup, y, xo = _inputs(pkg, 300, 150, 3, 7, seed=4)
    y[5, 3] = np.nan
    dg, ds = pkg.hipabi.DenGraph(g), pkg.hipabi.Supervision(sup)
    with _Mode(pkg, mode):
        r = _objf(hip, dg, ds, dev(y), dev(xo), 0.1, 0.0)
    assert r[5] == 0.0 and r[2] == 3 * 7 and r[0] == -10.0 * r[2] and r[6] == 0.0


def test_chain_objf_workspace_has_no_alpha_array(hip, pkg):
    """4 000 states, 128 sequences of 500 frames (the persistent form): the full entry keeps (T + 1) x states floats of alpha per sequence, 1 GB;
    the objective-only entry keeps the per-sequence sums and the numerator's scratch."""
    dg = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(4000, 100, mean_out_degree=4.0, seed=1))
    small, full = hip.chain_objf_workspace_bytes(dg.h, 128, 500), hip.chain_workspace_bytes(dg.h, 128, 500)
    print("CHAIN_OBJF workspace %d bytes against %d" % (small, full))
    assert full > 1 << 30 and 0 < small < full / 10
    # never larger than the full entry's, down to the smallest shapes (a full-size workspace is always accepted)
    tiny = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(4, 3, mean_out_degree=2.0, seed=1))
    for mode in (0, 1, 2, 3, 4):
        with _Mode(pkg, mode):
            for B, T in ((1, 1), (2, 3), (17, 1), (40, 2)):
                assert 0 < hip.chain_objf_workspace_bytes(tiny.h, B, T) <= hip.chain_workspace_bytes(tiny.h, B, T), (mode, B, T)
