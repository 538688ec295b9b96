"""-m gpu: tdnnf_net_objective / ChainNet.objective -- the forward pass and the chain objective without derivatives -- against the CPU
reference of the whole step run forward only (tests/oracle_net.py; BASELINE's bar 1e-4 relative on the objectives), against
forward_backward on a twin net (the bars of tests/test_gpu_chain_objf.py: the objective-only denominator may take another form of the same
recursion), and for what the call must NOT do: leave a trace in the net, run anything of the backward pass, touch the ReLU statistics."""
import numpy as np
import pytest
import torch

from tests.gpu_util import dev, host
from tests.oracle_net import OracleNet

pytestmark = pytest.mark.gpu

# configurations of tests/test_gpu_net.py's CASES, by value: (name, make_config keywords, states of the denominator graph)
_7Q = dict(frames_per_chunk=30, num_sequences=4, strides=[1, 1, 1, 0, 3, 3, 3], bottleneck=40, feat_dim=40, ivector_dim=100, num_pdfs=300, hidden_dim=192,
           small_dim=64)
_D = dict(frames_per_chunk=18, num_sequences=3, strides=[1, 1, 1, 1], bottleneck=16, feat_dim=40, ivector_dim=100, num_pdfs=120, hidden_dim=64, small_dim=32)
_B = dict(frames_per_chunk=24, num_sequences=3, strides=[1, 1, 0, 3], feat_dim=40, ivector_dim=100, num_pdfs=120, hidden_dim=128, small_dim=32)
_C = dict(frames_per_chunk=24, num_sequences=3, feat_dim=40, ivector_dim=100, num_pdfs=120, hidden_dim=128, small_dim=32)
_NG = dict(frames_per_chunk=48, num_sequences=8, strides=[1, 1, 1, 0, 3, 3, 3], bottleneck=24, feat_dim=40, ivector_dim=100, num_pdfs=150, hidden_dim=96,
           small_dim=48, use_natural_gradient=1)
CASES = [
    ("tiny", dict(frames_per_chunk=12, num_sequences=2, strides=[1, 1, 0, 3, 3], bottleneck=8, feat_dim=8, ivector_dim=4, num_pdfs=24, hidden_dim=32,
                  small_dim=16), 12),
    ("7q-shape-small", _7Q, 60),
    ("child-offsets", dict(_C, layer_offsets=[(1, 2), (0, 1), (2, 0), (3, 0), (2, 1)], bottleneck=32), 40),  # the last layer: rho = 3 row order
    ("darts-k4-gumbel-entropy-updatealpha", dict(_D, darts_num_offsets=4, darts_flags=1 | 8 | 16, darts_temp_proportion=0.7), 40),
    ("bn-supernet-softmax-flops", dict(_B, bn_choice_dims=[8, 8, 16, 32], bn_mode=1, bn_flops_scale=2.0), 40),
    ("7q-shape-small-dropout", dict(_7Q, use_dropout=1, dropout_proportion=0.3), 60),
    ("7q-shape-small-f16x3-planes", dict(_7Q, gemm_precision=3, planes=1), 60),
]
NG_CASES = [("7q-shape-small-NG", _NG, 60), ("7q-shape-small-NG-f16x3-planes", dict(_NG, gemm_precision=3, planes=1), 60)]


def _make_net(pkg, kw, **more):
    kw = dict(kw, **more)
    dropout_p = kw.pop("dropout_proportion", 0.0)
    planes = kw.pop("planes", 0)
    cfg = pkg.trainer.make_config(**kw)
    with pkg.hipabi.option("wgrad_stream", 0 if planes else -1):  # (plane operands need the one-stream schedule; read by tdnnf_net_create)
        net = pkg.trainer.ChainNet(cfg)
    if dropout_p:
        net.set_dropout_proportion(dropout_p)
    return net, cfg, dropout_p


def _params(net, cfg):
    params = net.init_params_numpy(seed=3, output_stddev=0.3)
    if cfg.darts_num_offsets:  # non-trivial architecture logits
        rng = np.random.default_rng(17)
        for c in net.components:
            n = c["rows"] * c["cols"]
            params[c["begin"] + n:c["begin"] + n + c["num_alpha"]] = rng.standard_normal(c["num_alpha"]).astype(np.float32) * 0.5
    if cfg.bn_num_choices:
        rng = np.random.default_rng(19)
        for c in net.components:
            if c["name"].endswith((".alpha", ".softmax")):
                params[c["begin"]:c["begin"] + c["rows"]] = rng.standard_normal(c["rows"]).astype(np.float32) * 0.7
    return params


def _egs(pkg, net, cfg, H, seed=4):
    feats, iv = pkg.trainer.synthetic_egs(net, seed=seed)
    den = pkg.synth.make_den_graph(H, cfg.num_pdfs, mean_out_degree=4.0, seed=5)
    sup = pkg.synth.make_supervision(cfg.num_sequences, cfg.frames_per_chunk // 3, cfg.num_pdfs, seed=seed + 2)
    return feats, iv, den, sup


def _draws(net, seed):
    return np.random.default_rng(seed).uniform(1e-3, 1 - 1e-3, max(net.num_draws, 1)).astype(np.float32)


def _chain_bars(r, ref):
    """tests/test_gpu_chain_objf.py's bars between tdnnf_chain_objf and tdnnf_chain_objf_and_deriv"""
    assert r[2] == ref[2] and r[5] == ref[5] == 1.0
    for k in (3, 4, 6):
        assert abs(r[k] - ref[k]) <= 1e-6 * abs(ref[k]), (k, r[k], ref[k])
    assert abs(r[0] - ref[0]) <= 1e-6 * (abs(ref[3]) + abs(ref[4])), (r[0], ref[0])
    assert abs(r[1] - ref[1]) <= 1e-9 * abs(ref[1]), (r[1], ref[1])


def _bn_mask(cfg):
    """True where an entry of get_stats() belongs to a BatchNorm block (net order: tdnn1 and every layer (batchnorm, relu), both heads
    (batchnorm1, relu, batchnorm2); BatchNorm [count, sum[D], sumsq[D]], ReLU 2 + 3 D doubles)"""
    Hd, S = cfg.hidden_dim, cfg.prefinal_small_dim
    m = []
    for _ in range(cfg.num_layers + 1):
        m += [True] * (1 + 2 * Hd) + [False] * (2 + 3 * Hd)
    for _ in range(2):
        m += [True] * (1 + 2 * Hd) + [False] * (2 + 3 * Hd) + [True] * (1 + 2 * S)
    return np.array(m)


# every configuration in training mode and in cv-update mode (BatchNormTest); the library builds no cv-update net with dropout
_BOTH_MODES = [(n, kw, H, cv) for n, kw, H in CASES for cv in (0, 1) if not (cv and kw.get("use_dropout"))]


@pytest.mark.parametrize("name,kw,H,cv", _BOTH_MODES, ids=["%s-%s" % (c[0], "cv-update" if c[3] else "train-mode") for c in _BOTH_MODES])
def test_objective_matches_oracle_and_forward_backward(pkg, name, kw, H, cv):
    net, cfg, dropout_p = _make_net(pkg, kw, cv_update=cv, chain_l2=1e-3)
    twin, _, _ = _make_net(pkg, kw, cv_update=cv, chain_l2=1e-3)
    params = _params(net, cfg)
    feats, iv, den, sup = _egs(pkg, net, cfg, H)
    dg, ds = pkg.hipabi.DenGraph(den), pkg.hipabi.Supervision(sup)
    fd, ivd = dev(feats), dev(iv)
    ref = OracleNet(pkg, cfg, net.components)
    if dropout_p:
        ref.set_dropout_proportion(dropout_p)
    if cv:  # BatchNormTest needs statistics: those of one training step of the same model
        pre, _, _ = _make_net(pkg, kw, cv_update=0)
        pre.set_params(params)
        pre.set_random_draws(_draws(pre, 99))
        pre.forward_backward(fd, ivd, dg, ds, step=0)
        stats = pre.get_stats()
        pre.close()
        for n in (net, twin, ref):
            n.set_stats(stats)
    draws = _draws(net, 100)
    for n in (net, twin):
        n.set_params(params)
        n.set_random_draws(draws)
    assert np.array_equal(net.get_stats(), twin.get_stats())
    res_ref, g_ref, _ = ref.forward_backward(params, feats, iv, den, sup, step=0, draws=draws, forward_only=True)
    assert g_ref is None
    r = host(net.objective(fd, ivd, dg, ds)).copy()
    rt = host(twin.forward_backward(fd, ivd, dg, ds, step=0)).copy()
    print("NET_OBJECTIVE %s cv %d: objf %.10g oracle %.10g forward_backward %.10g; xent %.10g / %.10g / %.10g; l2 %.10g / %.10g"
          % (name, cv, r[0], res_ref["objf"], rt[0], r[6], res_ref["xent_objf"], rt[6], r[1], rt[1]))
    assert r[5] == 1.0 and r[2] == res_ref["weight"]
    assert abs(r[0] - res_ref["objf"]) < 1e-4 * abs(res_ref["objf"]), (r[0], res_ref["objf"])
    assert abs(r[6] - res_ref["xent_objf"]) < 1e-4 * abs(res_ref["xent_objf"]), (r[6], res_ref["xent_objf"])
    _chain_bars(r, rt)
    assert np.array_equal(host(net.objective(fd, ivd, dg, ds)), r)  # repeatable, bit for bit
    net.close()
    twin.close()


@pytest.mark.parametrize("name,kw,H", NG_CASES, ids=[c[0] for c in NG_CASES])
def test_objective_calls_leave_no_trace_in_a_training_run(pkg, name, kw, H):
    """Three steps of forward_backward + update with natural gradient on, on two nets from the same state; one of them evaluates the
    objective before every step and after the last.  Parameters, statistics and every step's results: the same bits."""
    nets = [_make_net(pkg, kw)[0] for _ in range(2)]
    cfg = nets[0].cfg
    params = _params(nets[0], cfg)
    egs = [_egs(pkg, nets[0], cfg, H, seed=10 * i + 4) for i in range(3)]
    dg = pkg.hipabi.DenGraph(egs[0][2])
    out = []
    for k, net in enumerate(nets):
        net.set_params(params)
        steps = []
        for i, (feats, iv, _, sup) in enumerate(egs):
            fd, ivd, ds = dev(feats), dev(iv), pkg.hipabi.Supervision(sup)
            if k == 1:
                before = net.grads.clone()
                o = host(net.objective(fd, ivd, dg, ds)).copy()
                assert o[5] == 1.0 and torch.equal(net.grads, before)
            steps.append(host(net.forward_backward(fd, ivd, dg, ds, step=i)).copy())
            if k == 1 and i == 1:  # on a non-zero gradient buffer (between forward_backward and update)
                before = net.grads.clone()
                assert before.abs().sum().item() > 0
                net.objective(fd, ivd, dg, ds)
                assert torch.equal(net.grads, before)
            net.update(1e-3, step=i)
        if k == 1:
            net.objective(fd, ivd, dg, ds)
        out.append((host(net.params).copy(), net.get_stats().copy(), steps))
        net.close()
    (pa, sa, ra), (pb, sb, rb) = out
    assert np.array_equal(pa, pb) and np.array_equal(sa, sb)
    for a, b in zip(ra, rb):
        assert np.array_equal(a, b), (a, b)


@pytest.mark.parametrize("name,kw,H", [CASES[0], CASES[6]], ids=["tiny", "7q-shape-small-f16x3-planes"])
def test_objective_runs_the_forward_gemms_and_nothing_of_the_backward_pass(pkg, name, kw, H):
    net, cfg, _ = _make_net(pkg, kw)
    net.set_params(_params(net, cfg))
    feats, iv, den, sup = _egs(pkg, net, cfg, H)
    dg, ds = pkg.hipabi.DenGraph(den), pkg.hipabi.Supervision(sup)
    fd, ivd = dev(feats), dev(iv)
    net.objective(fd, ivd, dg, ds)  # (the first call of a net allocates; counted from the second)
    torch.cuda.synchronize()
    pkg.hipabi.launch_forms(reset=True)
    net.objective(fd, ivd, dg, ds)
    torch.cuda.synchronize()
    forms = pkg.hipabi.launch_forms()
    print("NET_OBJECTIVE launch forms of one call (%s): %r" % (name, forms))
    assert not any(k.startswith("wgrad.") and k != "wgrad.last_slabs" for k in forms), forms
    # one GEMM per weight component: lda, tdnn1, .linear and .affine of every layer, prefinal-l, three per head -- each counted once, as a rows
    # GEMM in one launch form or as a plane GEMM (a launch of whole rounds with a tail would count twice: these shapes have none)
    assert not any(k.endswith(("main_split_tail", "main_plain_tail")) for k in forms), forms
    one_launch = ("plain", "ring", "splitk") + tuple("partial_s%d" % s for s in range(2, 9))
    gemms = sum(v for k, v in forms.items() if (k.startswith("rows.") and k.split(".")[-1] in one_launch) or k == "planes.plain")
    assert gemms == 2 + 2 * cfg.num_layers + 1 + 6, forms
    net.close()


def test_objective_batchnorm_statistics_flag(pkg):
    name, kw, H = CASES[1]
    nets = [_make_net(pkg, kw)[0] for _ in range(2)]
    cfg = nets[0].cfg
    params = _params(nets[0], cfg)
    feats, iv, den, sup = _egs(pkg, nets[0], cfg, H)
    dg, ds = pkg.hipabi.DenGraph(den), pkg.hipabi.Supervision(sup)
    fd, ivd = dev(feats), dev(iv)
    for net in nets:  # a state with statistics in it: one training step
        net.set_params(params)
        net.forward_backward(fd, ivd, dg, ds, step=0)
        net.grads.zero_()
    a, b = nets
    s0 = a.get_stats().copy()
    assert np.array_equal(s0, b.get_stats()) and s0[0] > 0
    bn = _bn_mask(cfg)
    assert bn.size == s0.size
    # without the flag: nothing moves
    a.objective(fd, ivd, dg, ds)
    assert np.array_equal(a.get_stats(), s0)
    # with it: the BatchNorm blocks as after forward_backward from the same state, the ReLU blocks as before
    a.objective(fd, ivd, dg, ds, store_stats=True)
    b.forward_backward(fd, ivd, dg, ds, step=0)  # (step 0: every ReLU stores)
    sa, sb = a.get_stats(), b.get_stats()
    assert np.array_equal(sa[bn], sb[bn]) and not np.array_equal(sa[bn], s0[bn])
    assert np.array_equal(sa[~bn], s0[~bn]) and not np.array_equal(sb[~bn], s0[~bn])
    for net in nets:
        net.close()
    # cv-update mode: the flag is ignored
    cv, _, _ = _make_net(pkg, kw, cv_update=1)
    cv.set_params(params)
    cv.set_stats(s0)
    r = host(cv.objective(fd, ivd, dg, ds, store_stats=True)).copy()
    assert r[5] == 1.0 and np.array_equal(cv.get_stats(), s0)
    cv.close()


def test_objective_refuses_mismatched_dimensions(pkg):
    name, kw, H = CASES[0]
    net, cfg, _ = _make_net(pkg, kw)
    net.set_params(_params(net, cfg))
    feats, iv, den, sup = _egs(pkg, net, cfg, H)
    dg, ds = pkg.hipabi.DenGraph(den), pkg.hipabi.Supervision(sup)
    lib, abi = pkg.hipabi.load(), pkg.hipabi
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    short = dev(feats[:-1])
    assert lib.tdnnf_net_objective(net.h, abi.pmat(short), abi.pmat(dev(iv)), dg.h, ds.h, abi.ptr(res), 0, abi.stream()) == 1
    assert b"net_objective" in lib.tdnnf_last_error()
    assert lib.tdnnf_net_objective(net.h, abi.pmat(dev(feats)), abi.pmat(dev(iv)), dg.h, ds.h, abi.ptr(res), 2, abi.stream()) == 1  # unknown flag
    y = torch.zeros(ds.B * ds.T, cfg.num_pdfs + 1, device="cuda")
    nb = lib.tdnnf_chain_objf_workspace_bytes(dg.h, ds.B, ds.T)
    ws = abi.workspace(nb)
    assert lib.tdnnf_chain_objf(dg.h, ds.h, abi.pmat(y), None, 0.1, 0.0, abi.ptr(res), abi.ptr(ws), nb, abi.stream()) == 1  # one column too many
    y = torch.zeros(ds.B * ds.T, cfg.num_pdfs, device="cuda")
    assert lib.tdnnf_chain_objf(dg.h, ds.h, abi.pmat(y), None, 0.1, 0.0, abi.ptr(res), abi.ptr(ws), nb - 1, abi.stream()) == 1  # workspace too small
    assert lib.tdnnf_chain_objf(dg.h, ds.h, abi.pmat(y), abi.pmat(y[:-1]), 0.1, 0.0, abi.ptr(res), abi.ptr(ws), nb, abi.stream()) == 1
    net.close()


# ---- the outer loop: the small setup of tests/test_gpu_outer_loop.py::_setup, restated
KW = dict(frames_per_chunk=24, num_sequences=4, strides=[1, 0, 3], bottleneck=16, feat_dim=40, ivector_dim=100, num_pdfs=40, hidden_dim=64, small_dim=32,
          use_natural_gradient=1)


def _outer_setup(pkg):
    cfg = pkg.trainer.make_config(**KW)
    net = pkg.trainer.ChainNet(cfg)
    net.set_params(net.init_params_numpy(seed=1, output_stddev=0.1))
    den = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(30, cfg.num_pdfs, mean_out_degree=4.0, seed=5))
    egs = []
    for m in range(3):
        feats, iv = pkg.trainer.synthetic_egs(net, seed=100 + m)
        sup = pkg.synth.make_supervision(cfg.num_sequences, cfg.frames_per_chunk // 3, cfg.num_pdfs, seed=200 + m)
        egs.append((dev(feats), dev(iv), den, pkg.hipabi.Supervision(sup)))
    return cfg, net, egs


def test_compute_prob_is_repeatable_and_leaves_the_net_alone(pkg):
    cfg, net, egs = _outer_setup(pkg)
    for i, (f, v, d, s) in enumerate(egs):  # a model with statistics
        net.forward_backward(f, v, d, s, step=i)
        net.update(1e-3, step=i)
    o = pkg.outer_loop
    prob = pkg.trainer.ChainNet(o.evaluation_config(cfg, True))
    prob.params.copy_(net.params)
    prob.set_stats(net.get_stats())
    p0, s0 = host(prob.params).copy(), prob.get_stats().copy()
    a = o.compute_prob(prob, egs[:2])
    b = o.compute_prob(prob, egs[:2])
    assert a == b and np.isfinite(a["output"]) and np.isfinite(a["output_xent"]) and a["weight"] == 2 * cfg.num_sequences * (cfg.frames_per_chunk // 3)
    assert np.array_equal(host(prob.params), p0) and np.array_equal(prob.get_stats(), s0)
    # the same numbers as an evaluation through forward_backward, to rounding
    t = o._objective(prob, egs[:2])
    assert abs(a["output"] - (t[0] + t[1]) / t[2]) <= 1e-6 * (abs(t[3]) + abs(t[4])) / t[2]
    assert abs(a["output_xent"] - t[6] / t[2]) <= 1e-6 * abs(t[6] / t[2])
    prob.close()
    net.close()


def test_combine_models_forward_only_picks_the_same_models(pkg):
    cfg, net, egs = _outer_setup(pkg)
    models = []
    for i, (f, v, d, s) in enumerate(egs):
        net.forward_backward(f, v, d, s, step=i)
        net.update(2e-3, step=i)
        models.append((host(net.params).copy(), net.get_stats().copy()))
    net.close()
    models.reverse()  # latest first
    o = pkg.outer_loop
    got = []
    for forward_only in (False, True):
        comb = pkg.trainer.ChainNet(o.evaluation_config(cfg, False))
        count, first, objf = o.combine_models(comb, iter(models), len(models), egs[:2], forward_only=forward_only)
        got.append((count, first, objf, host(comb.params).copy(), comb.get_stats().copy()))
        comb.close()
    (ca, fa, oa, pa, sa), (cb, fb, ob, pb, sb) = got
    print("NET_OBJECTIVE combine: count %d / %d, objf %.10g / %.10g" % (ca, cb, oa, ob))
    assert ca == cb
    np.testing.assert_allclose(pb, pa, rtol=0, atol=1e-7)
    assert abs(ob - oa) <= 1e-6 * abs(oa) and abs(fb - fa) <= 1e-6 * abs(fa)
    np.testing.assert_allclose(sb, sa, rtol=1e-6)  # (the statistics are recomputed by the same forward_backward pass either way)
