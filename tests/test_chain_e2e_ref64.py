"""Pins tests/chain_e2e_ref64.py (the float64 reference of the chain objective with an end-to-end numerator) three ways, without a GPU:
(i) on a time-synchronous supervision turned into graphs its numerator is tests/chain_ref64.num_forward_backward's; (ii) its derivative is
the derivative of its objective (central differences); (iii) the failure path, and that synth.make_e2e_supervision never makes a graph
that takes it."""
import numpy as np
import pytest

from tests import chain_e2e_ref64 as E
from tests import chain_ref64 as R


def test_numerator_equals_the_time_synchronous_reference(pkg):
    B, T, P = 3, 9, 17
    sup = pkg.synth.make_supervision(B, T, P, max_alt=3, seed=5)
    y = (2.0 * np.random.default_rng(1).standard_normal((T * B, P))).astype(np.float32)
    lp_ref, post_ref = R.num_forward_backward(sup, y)
    lp, post = E.num_forward_backward(pkg.synth.alignment_graphs_from_supervision(sup), y, B)
    assert np.abs(lp - lp_ref).max() <= 1e-12 * np.abs(lp_ref).max()
    assert np.abs(post - post_ref).max() <= 1e-12 * np.abs(post_ref).max()
    e2e = pkg.synth.e2e_supervision_from_supervision(sup, P)
    assert (e2e["B"], e2e["T"], e2e["P"], e2e["weight"], len(e2e["graphs"])) == (B, T, P, 1.0, B)


def test_derivative_matches_central_differences(pkg):
    """8 random directions, cyclic graphs, B = 2, T = 5, P = 7; 1e-6 relative.  The reference reads float32 y, so y, the directions and the step
    are dyadic (y on a 2^-12 grid, directions on 2^-3, h = 2^-7): every y + k h dir is a float32 exactly and the differences are float64
    differences of the objective at exact points.  Five-point central differences: their truncation error is O(h^4) ~ 4e-9 of the third-order
    scale, where the three-point form's O(h^2) ~ 6e-5 would sit above the bar."""
    B, T, P, w, l2, leaky = 2, 5, 7, 0.75, 5e-3, 0.1
    den = pkg.synth.make_den_graph(6, P, mean_out_degree=3.0, seed=2)
    e2e = pkg.synth.make_e2e_supervision(B, T, P, units=(2, 4), seed=3, weight=w, optional=[1])
    assert all((g["src"] == g["dst"]).any() for g in e2e["graphs"])  # cyclic
    rng = np.random.default_rng(4)
    y = (np.round(rng.standard_normal((T * B, P)) * 4096) / 4096).astype(np.float32)
    f = lambda yy: (lambda r: r.objf + r.l2_term)(E.objective(den, e2e, yy.astype(np.float32), leaky, l2))
    r = E.objective(den, e2e, y, leaky, l2)
    assert r.ok
    h = 2.0 ** -7
    for k in range(8):
        d = rng.integers(-8, 9, size=y.shape) / 8.0
        y64 = y.astype(np.float64)
        pts = [y64 + c * h * d for c in (-2, -1, 1, 2)]
        assert all(np.array_equal(p.astype(np.float32).astype(np.float64), p) for p in pts)
        fm2, fm1, fp1, fp2 = (f(p) for p in pts)
        numeric = (fm2 - 8 * fm1 + 8 * fp1 - fp2) / (12 * h)
        analytic = float((r.deriv * d).sum())
        assert abs(numeric - analytic) <= 1e-6 * abs(analytic), (k, numeric, analytic)


def test_failure_path(pkg):
    B, T, P, w = 3, 4, 9, 0.5
    den = pkg.synth.make_den_graph(6, P, mean_out_degree=3.0, seed=2)
    e2e = pkg.synth.make_e2e_supervision(B, T, P, seed=1, weight=w)
    y = np.random.default_rng(0).standard_normal((T * B, P)).astype(np.float32)
    assert E.objective(den, e2e, y, 0.1, 0.0, 0.1, y).ok
    e2e["graphs"][1] = pkg.synth.make_alignment_graph(np.arange(T + 1) % P, seed=1, num_pdfs=P)  # shortest accepting path: T + 1 arcs
    r = E.objective(den, e2e, y, 0.1, 5e-5, 0.1, y)
    assert not r.ok and r.objf == -10.0 * w * B * T and r.num_lp[1] == -np.inf and np.isfinite(r.num_lp[[0, 2]]).all()
    assert not r.deriv.any() and not r.xent_deriv.any() and r.xent_objf == 0.0


@pytest.mark.parametrize("T", [1, 2, 7, 33])
def test_make_e2e_supervision_always_accepts_its_frame_count(pkg, T):
    """50 seeds at the shapes of tests/test_gpu_chain_e2e.py (and the units / optional variants the tests use): every graph has a path of exactly T arcs."""
    P = 41
    for seed in range(50):
        for B, kw in ((1, {}), (3, {}), (5, dict(units=(2, 4), optional=[1]))):
            e2e = pkg.synth.make_e2e_supervision(B, T, P, seed=seed, **kw)
            assert (e2e["B"], e2e["T"], e2e["P"], len(e2e["graphs"])) == (B, T, P, B)
            lp, _ = E.num_forward_backward(e2e["graphs"], np.zeros((T * B, P), dtype=np.float32), B)
            assert np.isfinite(lp).all(), (seed, B, T)
            for g in e2e["graphs"]:
                assert int(g["P"]) == P and (g["src"] == g["dst"]).sum() == int(g["S"]) - 1  # a self-loop on every unit
