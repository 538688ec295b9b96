"""-m gpu: the chain numerator on supervisions of any width (synth.make_supervision_lattice) -- the kernel entry and the trainer, both
forms of the numerator (option num_form), against the CPU oracle with the bars of test_gpu_parity._chain_case (BASELINE's): objective 1e-4
relative, derivative and xent derivative rel-L2 1e-4, posteriors summing to 1 per frame at rtol 1e-4, a NaN-filled workspace, a second call
equal bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import F, VIEW_LAYOUTS, Hip, dev, host, padded, placed, rel_l2
from tests.oracle_net import OracleNet

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Hip(pkg)


def _concat(sups):
    """Minibatch of all the sequences of several supervisions with the same T."""
    out = {"B": sum(s["B"] for s in sups), "T": sups[0]["T"], "weight": sups[0]["weight"]}
    ns = na = 0
    ssb, sab, rest = [np.zeros(1, np.int32)], [np.zeros(1, np.int32)], {k: [] for k in ("state_time", "final_logprob", "arc_src", "arc_dst", "arc_pdf", "arc_logprob")}
    for s in sups:
        assert s["T"] == out["T"]
        ssb.append(s["seq_state_begin"][1:] + ns)
        sab.append(s["seq_arc_begin"][1:] + na)
        for k in rest:
            rest[k].append(s[k] + ns if k in ("arc_src", "arc_dst") else s[k])
        ns += len(s["state_time"])
        na += len(s["arc_src"])
    out["seq_state_begin"] = np.concatenate(ssb).astype(np.int32)
    out["seq_arc_begin"] = np.concatenate(sab).astype(np.int32)
    for k in rest:
        out[k] = np.concatenate(rest[k]).astype(rest[k][0].dtype)
    return out


def _max_per_frame(sup):
    m = 0
    for b in range(sup["B"]):
        m = max(m, int(np.bincount(sup["state_time"][sup["seq_state_begin"][b]:sup["seq_state_begin"][b + 1]]).max()))
    return m


def _case(hip, ora, pkg, H, P, B, T, sup, leaky=0.1, l2=0.0, expect_wide=True, seed=0, layout=None):
    """_chain_case of test_gpu_parity.py on a given supervision; returns (derivative, results) of the first call."""
    L = ora.lib()
    g = pkg.synth.make_den_graph(H, P, mean_out_degree=6.0, seed=H)
    rng = np.random.default_rng(H + T + seed)
    y = (rng.standard_normal((T * B, P)) * 1.5).astype(F)
    xo = rng.standard_normal((T * B, P)).astype(F)
    gs, ss = ora.den_graph_struct(g), ora.supervision_struct(sup)
    objf, l2t, w = C.c_double(), C.c_double(), C.c_double()
    d_ref, xd_ref = np.zeros_like(y), np.zeros_like(y)
    ok = L.oracle_chain_objf_and_deriv(C.byref(gs), C.byref(ss), ora.omat(y), leaky, l2, 0.1, C.byref(objf), C.byref(l2t), C.byref(w), ora.omat(d_ref),
                                       ora.omat(xd_ref))
    assert ok == 1
    dg, ds = pkg.hipabi.DenGraph(g), pkg.hipabi.Supervision(sup)
    info = ds.info()
    assert info["num_states"] == len(sup["state_time"]) and info["num_arcs"] == len(sup["arc_src"]) and info["max_states_per_frame"] == _max_per_frame(sup)
    assert bool(info["wide"]) == expect_wide, info
    nb = hip.chain_workspace_bytes(dg.h, B, T)
    ws = hip.ws(nb)
    ws.fill_(float("nan"))  # nothing may depend on what the workspace held
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    if layout is None:
        yd, _ = padded(y)
        dd, dbuf = padded(np.full_like(y, 5.0))
        xod, xdd = dev(xo), torch.full((T * B, P), 5.0, device="cuda")
        checks = []
    else:  # all four matrices as guarded sub-matrix views (any base pointer, any stride)
        (yd, c0), (dd, c1), (xod, c2), (xdd, c3) = (placed(y, layout), placed(np.full_like(y, 5.0), layout, writes=True), placed(xo, layout),
                                                    placed(np.full_like(y, 5.0), layout, writes=True))
        dbuf, checks = None, [c0, c1, c2, c3]
    hip.chain_objf_and_deriv(dg.h, ds.h, yd, xod, leaky, l2, 0.1, hip.vec(res), dd, xdd, hip.vec(ws), nb, hip.stream())
    for check in checks:
        check()
    r = host(res)
    print("PARITY test_gpu_num_lattice H%d P%d B%d T%d states/frame %.1f widest %d: objf %.2e deriv %.2e xent_deriv %.2e" % (
        H, P, B, T, info["num_states"] / (B * T), info["max_states_per_frame"], abs(r[0] - objf.value) / abs(objf.value), rel_l2(host(dd), d_ref),
        rel_l2(host(xdd), 0.1 * xd_ref)))
    assert r[5] == 1.0 and r[2] == w.value
    assert abs(r[0] - objf.value) < 1e-4 * abs(objf.value), (r[0], objf.value)
    assert abs(r[1] - l2t.value) <= 1e-5 * abs(l2t.value) + 1e-12
    assert rel_l2(host(dd), d_ref) < 1e-4
    assert rel_l2(host(xdd), 0.1 * xd_ref) < 1e-4
    assert abs(r[6] - float((xo.astype(np.float64) * xd_ref).sum())) < 1e-4 * max(1.0, abs(r[6]))
    np.testing.assert_allclose(host(xdd).sum(1) / 0.1, 1.0, rtol=1e-4)
    assert dbuf is None or (host(dbuf)[:, P:] == 7.0).all(), "wrote outside the view"
    assert torch.isnan(ws[(nb + 3) // 4:]).all(), "wrote behind the workspace"  # (the slack hipabi.workspace adds behind the nb bytes)
    dd2 = torch.zeros_like(dd)  # bitwise reproducible
    hip.chain_objf_and_deriv(dg.h, ds.h, yd, None, leaky, l2, 0.1, hip.vec(res), dd2, None, hip.vec(ws), nb, hip.stream())
    assert torch.equal(dd2, dd) and host(res)[0] == r[0]
    return host(dd).copy(), r.copy()


@pytest.mark.parametrize("H,P,B,T,alts", [(50, 40, 3, 8, 3), (300, 200, 6, 30, 2), (120, 90, 130, 4, 6)])
def test_kernel_entry_small(hip, ora, pkg, H, P, B, T, alts):
    _case(hip, ora, pkg, H, P, B, T, pkg.synth.make_supervision_lattice(B, T, P, alternatives=alts, seed=T), l2=5e-5 if T == 30 else 0.0)


@pytest.mark.parametrize("layout", VIEW_LAYOUTS)
def test_kernel_entry_small_on_views(hip, ora, pkg, layout):
    _case(hip, ora, pkg, 50, 40, 3, 8, pkg.synth.make_supervision_lattice(3, 8, 40, alternatives=3, seed=8), layout=layout)


@pytest.mark.parametrize("alts,over", [(24, 64), (100, 256)], ids=["over64", "over256"])
def test_kernel_entry_wide_frames(hip, ora, pkg, alts, over):
    sup = pkg.synth.make_supervision_lattice(2, 20, 200, alternatives=alts, seed=1)
    assert _max_per_frame(sup) > over
    _case(hip, ora, pkg, 300, 200, 2, 20, sup)


def test_kernel_entry_long_chunk(hip, ora, pkg):
    """500 frames at the default width: what the double-precision log domain is for."""
    _case(hip, ora, pkg, 2000, 600, 4, 500, pkg.synth.make_supervision_lattice(4, 500, 600))


@pytest.mark.parametrize("mode", [1, 2], ids=["persistent", "wide"])
def test_both_denominator_modes(hip, ora, pkg, mode):
    pkg.hipabi.check(pkg.hipabi.load().tdnnf_chain_set_denominator_mode(mode))
    try:
        _case(hip, ora, pkg, 300, 200, 6, 30, pkg.synth.make_supervision_lattice(6, 30, 200, alternatives=4, seed=2))
    finally:
        pkg.hipabi.load().tdnnf_chain_set_denominator_mode(0)


def test_frontier_in_global_memory(hip, ora, pkg):
    """The form a frame too wide for the LDS takes (forced by the test hook)."""
    sup = pkg.synth.make_supervision_lattice(3, 25, 200, alternatives=30, seed=3)
    with pkg.hipabi.option("num_frontier_cap", 8):
        d_glob, r_glob = _case(hip, ora, pkg, 300, 200, 3, 25, sup)
    d_lds, r_lds = _case(hip, ora, pkg, 300, 200, 3, 25, sup)
    assert np.array_equal(d_glob, d_lds) and np.array_equal(r_glob, r_lds)  # (the same sums in the same order)


def test_mixed_minibatch(hip, ora, pkg):
    B, T, P = 8, 30, 200
    sup = _concat([pkg.synth.make_supervision(B // 2, T, P, seed=3), pkg.synth.make_supervision_lattice(B // 2, T, P, alternatives=8, seed=4)])
    _case(hip, ora, pkg, 300, P, B, T, sup)


def test_num_form_narrow_input_is_bitwise_the_default(hip, ora, pkg):
    B, T, P = 6, 30, 200
    sup = pkg.synth.make_supervision(B, T, P, seed=T)
    d0, r0 = _case(hip, ora, pkg, 300, P, B, T, sup, expect_wide=False)
    with pkg.hipabi.option("num_form", 1):
        d1, r1 = _case(hip, ora, pkg, 300, P, B, T, sup, expect_wide=False)
    assert np.array_equal(d0, d1) and np.array_equal(r0, r1)
    # a narrow supervision created under num_form = 2 can take the wide form too; one created without it cannot
    with pkg.hipabi.option("num_form", 2):
        d2, r2 = _case(hip, ora, pkg, 300, P, B, T, sup, expect_wide=False)
    np.testing.assert_allclose(d2.sum(1, dtype=np.float64), d0.sum(1, dtype=np.float64), rtol=1e-5, atol=1e-5)  # (see test_num_form_wide_input)
    ds = pkg.hipabi.Supervision(sup)
    with pkg.hipabi.option("num_form", 2):
        g = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(300, P, mean_out_degree=6.0, seed=300))
        nb = hip.chain_workspace_bytes(g.h, B, T)
        ws = hip.ws(nb)
        y, d, res = torch.zeros(T * B, P, device="cuda"), torch.zeros(T * B, P, device="cuda"), torch.zeros(8, dtype=torch.float64, device="cuda")
        rc = hip.lib.tdnnf_chain_objf_and_deriv(g.h, ds.h, pkg.hipabi.pmat(y), None, 0.1, 0.0, 0.1, pkg.hipabi.ptr(res), pkg.hipabi.pmat(d), None,
                                                pkg.hipabi.ptr(ws), nb, None)
        assert rc == 1 and b"num_form" in hip.lib.tdnnf_last_error()
        torch.cuda.synchronize()


def test_num_form_wide_input(hip, ora, pkg):
    B, T, P = 6, 30, 200
    sup = pkg.synth.make_supervision_lattice(B, T, P, alternatives=6, seed=5)
    with pkg.hipabi.option("num_form", 1):
        d1, r1 = _case(hip, ora, pkg, 300, P, B, T, sup)
    with pkg.hipabi.option("num_form", 2):
        d2, r2 = _case(hip, ora, pkg, 300, P, B, T, sup)
    d0, r0 = _case(hip, ora, pkg, 300, P, B, T, sup)
    assert np.array_equal(d0, d2) and np.array_equal(r0, r2)  # automatic: the wide form
    # a row of the derivative sums to (numerator mass 1) - (denominator mass 1): the two forms' sums agree to 1e-5 of that unit mass (a
    # relative bound alone says nothing about a difference that is zero up to rounding)
    np.testing.assert_allclose(d1.sum(1, dtype=np.float64), d2.sum(1, dtype=np.float64), rtol=1e-5, atol=1e-5)
    assert r1[3] == r2[3]  # the recursions give the same total bit for bit


def test_failure_path_on_a_wide_supervision(hip, ora, pkg):
    """_chain_failure of test_gpu_parity.py with a lattice."""
    g = pkg.synth.make_den_graph(30, 20, seed=1)
    sup = pkg.synth.make_supervision_lattice(2, 5, 20, alternatives=6, seed=1)
    y = np.zeros((10, 20), F)
    y[3, 4] = np.nan
    dg, ds = pkg.hipabi.DenGraph(g), pkg.hipabi.Supervision(sup)
    assert ds.info()["wide"] == 1
    nb = hip.chain_workspace_bytes(dg.h, 2, 5)
    ws = hip.ws(nb)
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    d, xd = torch.ones(10, 20, device="cuda"), torch.ones(10, 20, device="cuda")
    hip.chain_objf_and_deriv(dg.h, ds.h, dev(y), None, 0.1, 0.0, 0.1, hip.vec(res), d, xd, hip.vec(ws), nb, hip.stream())
    r = host(res)
    assert r[5] == 0.0 and r[0] == -10.0 * 10 and not host(d).any() and not host(xd).any()


# ------------------------------------------------------------------------------------------------ trainer
_NET = dict(frames_per_chunk=30, num_sequences=4, strides=[1, 1, 0, 3], bottleneck=24, feat_dim=40, ivector_dim=100, num_pdfs=150, hidden_dim=96, small_dim=48)


def _step_matches_oracle(pkg, net, ref, params, feats, iv, den, dg, sup, step, expect_wide):
    cfg = net.cfg
    ds = pkg.hipabi.Supervision(sup)
    assert bool(ds.info()["wide"]) == expect_wide
    draws = np.random.default_rng(100 + step).uniform(1e-3, 1 - 1e-3, max(net.num_draws, 1)).astype(np.float32)
    net.set_random_draws(draws)
    res_ref, g_ref, acts = ref.forward_backward(params, feats, iv, den, sup, step=step, draws=draws)
    net.grads.zero_()
    r = host(net.forward_backward(dev(feats), dev(iv), dg, ds, step=step)).copy()
    e = rel_l2(host(net.activation("output.deriv")), acts["output.deriv"])
    print("PARITY test_gpu_num_lattice trainer step %d wide %d: objf %.2e output.deriv %.2e gradient %.2e" % (
        step, expect_wide, abs(r[0] - res_ref["objf"]) / abs(res_ref["objf"]), e, rel_l2(host(net.grads), g_ref)))
    assert r[5] == 1.0 and r[2] == res_ref["weight"]
    assert abs(r[0] - res_ref["objf"]) < 1e-4 * abs(res_ref["objf"]), (r[0], res_ref["objf"])
    assert abs(r[6] - res_ref["xent_objf"]) < 1e-4 * abs(res_ref["xent_objf"])
    assert e < 1e-4
    assert rel_l2(host(net.grads), g_ref) < 1e-3  # BASELINE's bar, as tests/test_gpu_net.py
    return r, host(net.grads).copy(), g_ref


@pytest.mark.parametrize("ng", [0, 1], ids=["raw-gradient", "natural-gradient"])
def test_trainer_step_on_lattice_supervision(pkg, ng):
    kw = dict(_NET, frames_per_chunk=48, num_sequences=8, use_natural_gradient=1) if ng else _NET
    cfg = pkg.trainer.make_config(**kw)
    net = pkg.trainer.ChainNet(cfg)
    params = net.init_params_numpy(seed=3, output_stddev=0.3)
    net.set_params(params)
    ref = OracleNet(pkg, cfg, net.components)
    feats, iv = pkg.trainer.synthetic_egs(net, seed=4)
    den = pkg.synth.make_den_graph(60, cfg.num_pdfs, mean_out_degree=4.0, seed=5)
    dg = pkg.hipabi.DenGraph(den)
    sup = pkg.synth.make_supervision_lattice(cfg.num_sequences, cfg.frames_per_chunk // 3, cfg.num_pdfs, alternatives=5, seed=6)
    for step in (0, 1):
        _, _, g_ref = _step_matches_oracle(pkg, net, ref, params, feats, iv, den, dg, sup, step, True)
        p_ref = ref.update(params, g_ref, 1e-3, float(cfg.num_sequences), step)
        net.update(1e-3, step=step)
        assert rel_l2(host(net.params) - params, p_ref - params) < 2e-3
        params = p_ref
        net.set_params(params)
    net.close()


def test_trainer_three_steps_wide_narrow_wider(pkg):
    """One net, three supervisions of different widths one after the other: nothing of the net is sized by the supervision."""
    cfg = pkg.trainer.make_config(**_NET)
    net = pkg.trainer.ChainNet(cfg)
    params = net.init_params_numpy(seed=3, output_stddev=0.3)
    net.set_params(params)
    ref = OracleNet(pkg, cfg, net.components)
    feats, iv = pkg.trainer.synthetic_egs(net, seed=4)
    den = pkg.synth.make_den_graph(60, cfg.num_pdfs, mean_out_degree=4.0, seed=5)
    dg = pkg.hipabi.DenGraph(den)
    B, T, P = cfg.num_sequences, cfg.frames_per_chunk // 3, cfg.num_pdfs
    sups = [(pkg.synth.make_supervision_lattice(B, T, P, alternatives=4, seed=7), True), (pkg.synth.make_supervision(B, T, P, seed=8), False),
            (pkg.synth.make_supervision_lattice(B, T, P, alternatives=40, seed=9), True)]
    for step, (sup, wide) in enumerate(sups):
        _, _, g_ref = _step_matches_oracle(pkg, net, ref, params, feats, iv, den, dg, sup, step, wide)
        params = ref.update(params, g_ref, 1e-3, float(B), step)
        net.set_params(params)
    net.close()


def test_trainer_step_from_an_archive_of_lattices(pkg, tmp_path):
    E = pkg.egs
    cfg = pkg.trainer.make_config(frames_per_chunk=24, num_sequences=4, strides=[1, 0, 3], bottleneck=16, feat_dim=40, ivector_dim=100, num_pdfs=60,
                                  hidden_dim=64, small_dim=32)
    net = pkg.trainer.ChainNet(cfg)
    net.set_params(net.init_params_numpy(seed=1, output_stddev=0.3))
    B = cfg.num_sequences
    den = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(30, cfg.num_pdfs, mean_out_degree=4.0, seed=5))
    feats, iv = pkg.trainer.synthetic_egs(net, seed=10)
    sup = pkg.synth.make_supervision_lattice(B, cfg.frames_per_chunk // 3, cfg.num_pdfs, alternatives=6, seed=20)
    path = tmp_path / "cegs.lattice.ark"
    with E.Writer(path) as w:
        for b in range(B):
            w.write("u%d" % b, feats[b::B], net.first_t, E.sequence_of(sup, b), cfg.num_pdfs, ivector=iv[b], compress=False)
    (f_dev, iv_dev, sup_dev), = list(E.minibatches(path, net))
    assert sup_dev.info()["wide"] == 1
    net.grads.zero_()
    r1 = host(net.forward_backward(f_dev, iv_dev, den, sup_dev, step=3)).copy()
    g1 = host(net.grads).copy()
    net.grads.zero_()
    r2 = host(net.forward_backward(dev(feats), dev(iv), den, pkg.hipabi.Supervision(sup), step=3))
    assert r1[5] == 1.0 and np.array_equal(r1, r2) and np.array_equal(g1, host(net.grads))
    net.close()
