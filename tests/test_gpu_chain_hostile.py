"""-m gpu: every kernel family of the chain denominator, and the numerator, on the inputs a trained chain net and a diverging one produce
(tests/chain_ref64.py: `peaky`, one pdf per frame 25 nats above the rest, 10-25 decades of dynamic range per frame in the recursions;
`beyond`, N(0, 25^2), 23 % of the elements outside the +-30 of ApplyExpLimited; `long-peaky`, 150 frames of the first) against a float64
forward-backward and the CPU oracle.  Every other chain test feeds N(0, 1) or N(0, 1.5^2): a kernel that forgot the clamp, a numerator that
applied one, or a renormalisation that loses the small states would pass them all.

One case per (family, data, leaky-HMM coefficient); each family at the smallest shape that still selects it.  Bars (the project's own):
denominator and numerator log-prob within 1e-6 relative of float64, |d objf| <= 1e-6 (|num| + |den|), derivative and xent derivative
rel_l2 < 1e-4 against the oracle (BASELINE), posteriors of every frame sum to 1 within 2e-5, ok flag, reruns bit-identical.  The largest
single occupancy error has no bar in the project: it is held to ten times what the oracle (f32 alpha, double accumulation) shows against
float64 on the same input, at most 1e-4.  Measured values: docs/experiments.md, "Chain kernels on hostile data"."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import chain_ref64 as R
from tests.gpu_util import Hip, dev, host, rel_l2

pytestmark = pytest.mark.gpu
XENT = 0.1

# family -> (denominator mode, states, pdfs, sequences, frames, the split form's occupancy pass runs)
FAMILIES = {
    "mw-four-workgroups": (1, 300, 150, 3, 40, True),      # den_mw_kernel<0> / <1>, den_gamma2_kernel
    "split-fast": (3, 300, 150, 3, 40, True),              # den_forward_kernel<true, true> beside den_beta_kernel<true>
    "split-plain-loop": (3, 4200, 64, 2, 12, True),        # more than 4 096 states: not FAST
    "serial-fast": (4, 300, 150, 3, 40, False),            # den_forward_kernel<true, true>, then den_backward_kernel<true>
    "serial-plain-loop": (4, 4200, 64, 2, 12, False),      # den_forward_kernel<true, false>, then den_backward_kernel<true>
    "serial-global-vectors": (1, 13000, 40, 2, 8, False),  # P + 3 x states floats over the LDS budget: den_backward_kernel<false>
    "wide-ragged-16": (2, 200, 150, 5, 12, False),         # one ragged group of 16
    "wide-32-and-ragged": (2, 200, 150, 40, 12, False),    # a full group of 32 and a ragged one
}
LONG = ("mw-four-workgroups", "split-fast", "serial-fast")  # long-peaky: 2 sequences of 150 frames
CASES = [(f, d, lk) for f in FAMILIES for d in ("peaky", "beyond") for lk in (0.1, 1e-5)] + [(f, "long-peaky", lk) for f in LONG for lk in (0.1, 1e-5)]


@pytest.fixture(scope="module")
def hip(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
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


_handles = {}


def _device_graph(pkg, H, P):
    if (H, P) not in _handles:
        _handles[(H, P)] = pkg.hipabi.DenGraph(R.graph(pkg, H, P))
    return _handles[(H, P)]


def _run(hip, dg, ds, yd, leaky):
    """(results[8], derivative, xent derivative) of tdnnf_chain_objf_and_deriv on a NaN-filled workspace and 5-filled outputs"""
    nb = hip.chain_workspace_bytes(dg.h, ds.B, ds.T)
    ws = hip.ws(nb)
    ws.fill_(float("nan"))
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    d, xd = torch.full(yd.shape, 5.0, device="cuda"), torch.full(yd.shape, 5.0, device="cuda")
    hip.chain_objf_and_deriv(dg.h, ds.h, yd, None, leaky, 0.0, XENT, hip.vec(res), d, xd, hip.vec(ws), nb, hip.stream())
    return host(res).copy(), host(d).copy(), host(xd).copy()


@pytest.mark.parametrize("family,data,leaky", CASES, ids=["%s-%s-leaky%g" % c for c in CASES])
def test_chain_objf_and_deriv_on_hostile_data(hip, ora, pkg, family, data, leaky):
    mode, H, P, B, T, split = FAMILIES[family]
    if data == "long-peaky":
        B, T = 2, 150
    c = R.make_case(pkg, ora, data, H, P, B, T, leaky)  # (asserts that the oracle copes: ok == 1)
    dg, ds = _device_graph(pkg, H, P), pkg.hipabi.Supervision(c.sup)
    yd = dev(c.y.copy())
    lib = pkg.hipabi.load()
    fb, off = C.c_int(), C.c_int()
    with _Mode(pkg, mode):
        if family.startswith("mw"):
            pkg.hipabi.check(lib.tdnnf_chain_den_mw_status(C.byref(fb), C.byref(off), 1))
        r, d, xd = _run(hip, dg, ds, yd, leaky)
        if family.startswith("mw"):  # the multi-workgroup recursions did run, and to their end: otherwise this row tested the one-workgroup kernels
            pkg.hipabi.check(lib.tdnnf_chain_den_mw_status(C.byref(fb), C.byref(off), 0))
            assert fb.value == 0 and off.value == 0
        r2, d2, xd2 = _run(hip, dg, ds, yd, leaky)
        if split:  # den_gamma2_kernel promises den_gamma_kernel's bits
            with pkg.hipabi.option("den_gamma_pairs", 1):
                r1, d1, _ = _run(hip, dg, ds, yd, leaky)
        if family.startswith("mw"):
            with _Mode(pkg, 3):
                _, d_one, _ = _run(hip, dg, ds, yd, leaky)
            pkg.hipabi.check(lib.tdnnf_chain_set_denominator_mode(mode))
    num, den = float(c.num_lp.sum()), float(c.den_lp.sum())
    post = xd.astype(np.float64) / float(np.float32(XENT))  # (the kernel's factor is the float)
    gamma = post - d  # the derivative is numerator posteriors - denominator occupancies (weight 1, no l2 term)
    e = dict(den=abs(r[4] - den) / abs(den), num=abs(r[3] - num) / abs(num), objf=abs(r[0] - (num - den)) / (abs(num) + abs(den)),
             deriv=rel_l2(d, c.d_ora), xent=rel_l2(xd, XENT * c.xd_ora), num_sum=float(np.abs(post.sum(1) - 1).max()),
             den_sum=float(np.abs(gamma.sum(1) - 1).max()), occ=float(np.abs(gamma - c.den_gamma).max()),
             occ_l2=rel_l2(gamma, c.den_gamma))
    occ_bar = min(10 * c.ora_gamma_maxabs, 1e-4)
    print("PARITY test_gpu_chain_hostile %s %s leaky %g: den %.2e num %.2e objf %.2e (bars 1e-6) deriv %.2e xent %.2e (bars 1e-4) frame sums num %.2e "
          "den %.2e (bars 2e-5) occupancy max abs %.2e (oracle %.2e, bar %.2e) rel_l2 %.2e (oracle %.2e)"
          % (family, data, leaky, e["den"], e["num"], e["objf"], e["deriv"], e["xent"], e["num_sum"], e["den_sum"], e["occ"], c.ora_gamma_maxabs,
             occ_bar, e["occ_l2"], c.ora_gamma_rel))
    assert r[5] == 1.0 and r[2] == c.weight
    assert np.isfinite(d).all() and np.isfinite(xd).all()
    assert e["den"] <= 1e-6 and e["num"] <= 1e-6, (r[4], den, r[3], num)
    assert e["objf"] <= 1e-6, (r[0], num - den)
    assert e["deriv"] < 1e-4 and e["xent"] < 1e-4
    assert e["num_sum"] <= 2e-5 and e["den_sum"] <= 2e-5
    assert e["occ"] <= occ_bar
    assert np.array_equal(r2, r) and np.array_equal(d2, d) and np.array_equal(xd2, xd)  # reruns: the same bits
    if split:
        assert np.array_equal(d1, d) and np.array_equal(r1, r)
    if family.startswith("mw"):
        assert not np.array_equal(d_one, d)  # the switch did switch: other summation orders


# the objective-only entry: its four denominator forms (chain_den.hip chain_objf_den)
OBJF_FORMS = {
    "logprob-lds-fast": (3, 300, 150, 3, 40),            # den_logprob_kernel<true, true>
    "logprob-lds-plain-loop": (3, 4200, 64, 2, 12),      # den_logprob_kernel<true, false>
    "logprob-global-vectors": (1, 13000, 40, 2, 8),      # den_logprob_kernel<false, false>
    "logprob-wide": (2, 200, 150, 5, 12),                # den_wide_logprob
}


@pytest.mark.parametrize("data", ["peaky", "beyond"])
@pytest.mark.parametrize("form", list(OBJF_FORMS))
def test_chain_objf_on_hostile_data(hip, ora, pkg, form, data):
    mode, H, P, B, T = OBJF_FORMS[form]
    c = R.make_case(pkg, ora, data, H, P, B, T, 0.1)
    dg, ds = _device_graph(pkg, H, P), pkg.hipabi.Supervision(c.sup)
    yd = dev(c.y.copy())
    with _Mode(pkg, mode):
        nb = hip.chain_objf_workspace_bytes(dg.h, B, T)
        out = []
        for _ in range(2):
            ws = hip.ws(nb)
            ws.fill_(float("nan"))
            res = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
            hip.chain_objf(dg.h, ds.h, yd, None, 0.1, 0.0, hip.vec(res), hip.vec(ws), nb, hip.stream())
            out.append(host(res).copy())
    r = out[0]
    num, den = float(c.num_lp.sum()), float(c.den_lp.sum())
    print("PARITY test_gpu_chain_hostile %s %s: den %.2e num %.2e objf %.2e (bars 1e-6)"
          % (form, data, abs(r[4] - den) / abs(den), abs(r[3] - num) / abs(num), abs(r[0] - (num - den)) / (abs(num) + abs(den))))
    assert r[5] == 1.0 and r[2] == c.weight
    assert abs(r[4] - den) <= 1e-6 * abs(den) and abs(r[3] - num) <= 1e-6 * abs(num), (r[4], den, r[3], num)
    assert abs(r[0] - (num - den)) <= 1e-6 * (abs(num) + abs(den))
    assert np.array_equal(out[1], r)


def test_one_kernel_backward_pass_leaves_the_split_region_alone(hip, ora, pkg):
    """Mode 4 (the trainer's den_split 0): the last tdnnf_chain_split_region_bytes bytes of the workspace keep their fill pattern, which is what
    entitles a trainer that never runs the side-by-side form to allocate that much less; modes 1 and 3 do write there."""
    mode, H, P, B, T, _ = FAMILIES["serial-fast"]
    c = R.make_case(pkg, ora, "peaky", H, P, B, T, 0.1)
    dg, ds = _device_graph(pkg, H, P), pkg.hipabi.Supervision(c.sup)
    yd = dev(c.y.copy())

    def tail_after(mode):
        with _Mode(pkg, mode):
            nb, region = hip.chain_workspace_bytes(dg.h, B, T), pkg.hipabi.chain_split_region_bytes(dg, B, T)
            assert 0 < region < nb and region % 4 == 0 and nb % 4 == 0
            ws = torch.full((nb // 4,), float("nan"), device="cuda")  # exactly the workspace: its last bytes are the tensor's
            res = torch.zeros(8, dtype=torch.float64, device="cuda")
            d = torch.zeros(yd.shape, device="cuda")
            hip.chain_objf_and_deriv(dg.h, ds.h, yd, None, 0.1, 0.0, XENT, hip.vec(res), d, None, hip.vec(ws), nb, hip.stream())
            assert host(res)[5] == 1.0
            return host(ws)[-(region // 4):], nb, region

    tail4, nb4, region4 = tail_after(4)
    tail3, nb3, region3 = tail_after(3)
    assert (nb4, region4) == (nb3, region3)  # plan and workspace follow mode 1 / 3
    assert np.isnan(tail4).all()
    assert not np.isnan(tail3).all()  # (the side-by-side form keeps beta of every frame there)
    with _Mode(pkg, 2):  # no such region in the wide form, nor where the state vectors live in global memory
        assert hip.chain_split_region_bytes(dg.h, B, T) == 0
    big = _device_graph(pkg, 13000, 40)
    with _Mode(pkg, 4):
        assert hip.chain_split_region_bytes(big.h, 2, 8) == 0


def test_denominator_mode_range(pkg):
    lib = pkg.hipabi.load()
    try:
        pkg.hipabi.check(lib.tdnnf_chain_set_denominator_mode(4))
        with pytest.raises(pkg.hipabi.HipAbiError, match="4 persistent, forward then one-kernel backward"):
            pkg.hipabi.check(lib.tdnnf_chain_set_denominator_mode(5))
    finally:
        lib.tdnnf_chain_set_denominator_mode(0)
