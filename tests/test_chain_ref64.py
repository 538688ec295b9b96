"""Pins tests/chain_ref64.py (the float64 forward-backward the hostile-data GPU tests compare with), and the oracle against it:
 - the reference against torch float64 autograd of the dense recursion and against brute-force path enumeration, on tiny cases inside +-30
   (where the clamp does nothing, so autograd and the occupancies agree);
 - the clamp: outside +-30 the reference computes on clip(y) and still returns an occupancy for every element;
 - the oracle (f32 alpha, double accumulation) against the reference on the hostile families, at the margins measured when the families
   were chosen (occupancies 3.3e-7 relative L2, log-prob 7e-9 relative, frame sums 9.1e-7) with some slack."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import chain_ref64 as R
from tests.test_oracle_chain_optim import _den_brute_force_logprobs, _den_logprob_torch, _num_brute_force_logprobs

F = np.float32


@pytest.mark.parametrize("leaky", [0.0, 0.1, 1e-5])
def test_denominator_reference_vs_autograd(pkg, leaky):
    H, P, B, T = 17, 9, 3, 12
    g = pkg.synth.make_den_graph(H, P, mean_out_degree=3.0, seed=5)
    y = (np.random.default_rng(1).standard_normal((T * B, P)) * 4.0).astype(F)  # (inside +-30: max |y| about 16)
    assert np.abs(y).max() < 30
    yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    lp = _den_logprob_torch(g, yt, B, leaky)
    lp.sum().backward()
    lp_ref, gamma = R.den_forward_backward(g, y, B, leaky)
    np.testing.assert_allclose(lp_ref, lp.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(gamma, yt.grad.numpy(), rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(gamma.sum(1), 1.0, rtol=1e-12)


def test_denominator_reference_vs_brute_force_paths(pkg):
    g = pkg.synth.make_den_graph(3, 4, mean_out_degree=2.0, seed=11)
    B, T, P = 2, 3, 4
    y = np.random.default_rng(0).standard_normal((T * B, P)).astype(F)
    lp, _ = R.den_forward_backward(g, y, B, 0.0)
    np.testing.assert_allclose(lp, _den_brute_force_logprobs(g, y, B), rtol=1e-12)


def test_denominator_reference_clamps_and_keeps_every_occupancy(pkg):
    """y beyond +-30 acts as +-30, and the occupancy of a clamped element is still its gamma (not autograd's 0)."""
    H, P, B, T = 17, 9, 2, 6
    g = pkg.synth.make_den_graph(H, P, mean_out_degree=3.0, seed=5)
    y = (np.random.default_rng(2).standard_normal((T * B, P)) * 25.0).astype(F)
    assert (np.abs(y) > 30).mean() > 0.15
    lp, gamma = R.den_forward_backward(g, y, B, 0.1)
    lp_c, gamma_c = R.den_forward_backward(g, np.clip(y, -30, 30), B, 0.1)
    assert np.array_equal(lp, lp_c) and np.array_equal(gamma, gamma_c)
    assert gamma[y > 30].max() > 1e-3  # clamped from above, occupied all the same
    np.testing.assert_allclose(gamma.sum(1), 1.0, rtol=1e-12)
    yt = torch.tensor(np.clip(y, -30, 30), dtype=torch.float64, requires_grad=True)
    tot = _den_logprob_torch(g, yt, B, 0.1)
    tot.sum().backward()
    np.testing.assert_allclose(lp, tot.detach().numpy(), rtol=1e-12)
    np.testing.assert_allclose(gamma, yt.grad.numpy(), rtol=1e-9, atol=1e-14)


def test_numerator_reference_vs_brute_force_and_autograd(pkg):
    B, T, P = 2, 4, 6
    sup = pkg.synth.make_supervision(B, T, P, max_alt=2, seed=3, weight=1.0)
    y = (np.random.default_rng(2).standard_normal((T * B, P)) * 40.0).astype(F)  # the numerator takes y as it is: no clamp
    assert np.abs(y).max() > 60
    yt = torch.tensor(y, dtype=torch.float64, requires_grad=True)
    per_seq = _num_brute_force_logprobs(sup, yt)
    sum(per_seq).backward()
    lp, post = R.num_forward_backward(sup, y)
    np.testing.assert_allclose(lp, [float(v.detach()) for v in per_seq], rtol=1e-12)
    np.testing.assert_allclose(post, yt.grad.numpy(), rtol=1e-9, atol=1e-14)
    np.testing.assert_allclose(post.sum(1), 1.0, rtol=1e-12)


def test_hostile_families_are_what_they_say(pkg):
    g = R.graph(pkg, 300, 150)
    sup = pkg.synth.make_supervision_from_den(g, 3, 40, num_paths=2, seed=40)
    y = R.make_logits("peaky", sup, 150)
    assert np.array_equal(y, R.make_logits("peaky", sup, 150))  # seeded
    top = y.argmax(1)
    assert (np.sort(y, 1)[:, -1] - np.sort(y, 1)[:, -2] > 10).all() and np.abs(y).max() < 30
    on_path = np.mean([top[t * 3 + s] in R.supervision_pdfs(sup, s, t) for t in range(40) for s in range(3)])
    assert 0.35 < on_path < 0.65, on_path
    y = R.make_logits("beyond", sup, 150)
    assert 0.20 < (np.abs(y) > 30).mean() < 0.26


# the shapes the margins were measured at: 300 states, 150 pdfs, out-degree 4; 3 x 40 frames, long-peaky 2 x 150
@pytest.mark.parametrize("leaky", [0.1, 1e-5, 0.0])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_oracle_stays_close_to_float64_on_hostile_data(pkg, ora, family, leaky):
    B, T = (2, 150) if family == "long-peaky" else (3, 40)
    c = R.make_case(pkg, ora, family, 300, 150, B, T, leaky)  # (asserts the oracle's ok == 1)
    print("CHAIN_REF64 %s leaky %g: oracle occupancies %.2e (bar 2e-6), max abs %.2e, log-prob %.2e (bar 1e-7), frame sums %.2e (bar 5e-6); "
          "numerator log-prob %.2e, posteriors max abs %.2e" % (family, leaky, c.ora_gamma_rel, c.ora_gamma_maxabs, c.ora_lp_rel, c.ora_frame_sum,
                                                                abs(c.num_ora - c.num_lp.sum()) / abs(c.num_lp.sum()), c.ora_post_maxabs))
    assert c.ora_gamma_rel < 2e-6
    assert c.ora_lp_rel < 1e-7
    assert c.ora_frame_sum < 5e-6
    # the reference itself: both posteriors sum to 1 per frame to the last bits of a double
    np.testing.assert_allclose(c.den_gamma.sum(1), 1.0, rtol=1e-11)
    np.testing.assert_allclose(c.num_post.sum(1), 1.0, rtol=1e-11)
    # the oracle's numerator is log-domain in double on the raw y as well: only the float posteriors differ
    assert abs(c.num_ora - c.num_lp.sum()) <= 1e-12 * abs(c.num_lp.sum())
    assert c.ora_post_maxabs < 1e-7
    assert abs(c.objf_ora - (c.num_ora - c.den_ora)) < 1e-9 * (abs(c.num_ora) + abs(c.den_ora))
