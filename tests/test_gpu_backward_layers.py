"""-m gpu: the trainer's backward pass LAYER BY LAYER, between output.deriv and the weight gradients -- the span the whole-step
tests (tests/test_gpu_net.py: gradient relative L2 1e-3, a handful of forward activations) only see contracted over all rows.

(a) Teacher-forced, per element, against float64.  One forward_backward call with tdnnf_net_set_capture on; for every BatchNorm /
    ReLU sweep of the net (fused.hip bn_relu_bwd: tdnn1, every tdnnf layer, both heads) the GPU's OWN inputs are read back -- the ReLU
    output, the derivative going in, the dropout mask rows, the statistics block in test mode -- and tests/backward_ref64.py restates
    the sweep in float64.  Compared: X.affine.deriv element by element, the affine's bias gradient (raw-gradient nets), the ReLU
    statistics increments; and forward X.noop / tdnn1.batchnorm against bn_apply_bypass64.  No ReLU tie can occur: the mask comes from
    the GPU's own x.  Bars: scaled error |got - ref64| / (2^-24 mag) <= K, K from the float32 C oracle's own error on these shapes
    (tests/backward_ref64.py, measured by tests/test_backward_ref64.py), never from the kernels.
    Every case asserts, through the sweeps' form counters (tdnnf_fused_launch_forms), that the kernel form it names ran.
    What the library does not expose and this file therefore cannot read: the memo rows 3 / 4 (vdm, temp) -- test mode is held through
    d_aff = relu'(x) dz scale instead, which is what their being zero means; the natural-gradient statistic H = d_aff W^T of the ng
    form -- the fused and the separate-pass gradients are held together as tests/test_gpu_net.py does, besides d_aff per element.
(b) reverse_passes = 3 against 0: every activation, every captured derivative and the gradient bit for bit.
(c) Chained, against the CPU oracle of the whole step, every layer's derivative by relative L2 at the activation bar of
    tests/test_gpu_net.py::test_net_step_matches_oracle (1e-4; 1e-3 for gemm_precision 1), ReLU ties handed over and capped.
"""
import contextlib

import numpy as np
import pytest

from tests import backward_ref64 as R
from tests.gpu_util import dev, host, rel_l2
from tests.oracle_net import OracleNet, decision
from tests.test_gpu_net import CASES as NET_CASES, CV_CASES

pytestmark = pytest.mark.gpu


def net_case(name):
    c = next(c for c in NET_CASES if c[0] == name)
    return dict(c[1]), c[2]


# the kwargs of tests/test_gpu_net.py::test_fused_output_statistics_match_the_separate_pass; hidden_dim by the output rank's class
_NG = dict(frames_per_chunk=30, num_sequences=8, strides=[1, 1, 0, 3, 3], bottleneck=16, feat_dim=8, ivector_dim=4, small_dim=32, num_pdfs=50,
           use_natural_gradient=1, use_dropout=1)
_PLANES = dict(frames_per_chunk=24, num_sequences=4, strides=[1, 3], bottleneck=32, feat_dim=40, ivector_dim=100, num_pdfs=90, hidden_dim=1024,
               small_dim=64, gemm_precision=3)

# name -> (net kwargs, den-graph states, dropout proportion, options for the whole run, steps, forms that must show non-zero)
TEACHER_CASES = {
    "vec4": (net_case("7q-shape-small")[0], 60, 0.0, {}, (0, 1),
             ["bwd.reduce.vec4.stats", "bwd.reduce.vec4.nostats", "bwd.apply.vec4", "bwd.apply.rows_unrolled", "bwd.apply.rows_tail",
              "apply_bypass.vec4", "bwd.finalize.train"]),
    "scalar": (net_case("ragged-dims")[0], 30, 0.0, {}, (0, 1),
               ["bwd.reduce.scalar.stats", "bwd.apply.scalar", "apply_bypass.scalar", "bwd.apply.short_last_chunk"]),  # (35 rows: chunks of 18 and 17)
    "mask-superrow": (net_case("7q-shape-small-dropout")[0], 60, 0.3, {}, (0, 1),
                      ["bwd.apply.vec4.mask", "apply_bypass.vec4.mask", "apply_bypass.vec4.super.mask"]),
    "ng-nt1-dropout": (dict(_NG, hidden_dim=64), 30, 0.2, {"ng_fuse": 2}, (0, 1, 2), ["bwd.apply_ng.nt1.mask", "bwd.apply_ng.nt1", "bwd.apply_ng.partial_block"]),
    "ng-nt2-dropout": (dict(_NG, hidden_dim=96), 30, 0.2, {"ng_fuse": 2}, (0, 1, 2), ["bwd.apply_ng.nt2.mask", "bwd.apply_ng.partial_block"]),
    "ng-nt3-dropout": (dict(_NG, hidden_dim=160), 30, 0.2, {"ng_fuse": 2}, (0, 1, 2), ["bwd.apply_ng.nt3.mask", "bwd.apply_ng.partial_block"]),
    "ng-nt1": (dict(_NG, hidden_dim=64, use_dropout=0), 30, 0.0, {"ng_fuse": 2}, (0, 1, 2), ["bwd.apply_ng.nt1", "bwd.apply_ng.partial_block"]),
    "ng-nt2": (dict(_NG, hidden_dim=96, use_dropout=0), 30, 0.0, {"ng_fuse": 2}, (0, 1, 2), ["bwd.apply_ng.nt2", "bwd.apply_ng.partial_block"]),
    "ng-nt3": (dict(_NG, hidden_dim=160, use_dropout=0), 30, 0.0, {"ng_fuse": 2}, (0, 1, 2), ["bwd.apply_ng.nt3", "bwd.apply_ng.partial_block"]),
    # 48 frames x 8 sequences: the heads' sweeps have 16 x 8 = 128 rows, one whole block
    "ng-full-blocks": (dict(_NG, hidden_dim=96, frames_per_chunk=48), 30, 0.2, {"ng_fuse": 2}, (0, 1), ["bwd.apply_ng.nt2", "bwd.apply_ng.full_blocks"]),
    # the sweeps that write their result as f16 planes too (bwd_planes needs 1024 columns and the one-stream schedule); only the float32
    # matrices of those kernels are compared
    "planes": (_PLANES, 40, 0.0, {"wgrad_stream": 0}, (0, 1), ["apply_bypass.planes", "bwd.apply.planes"]),
}


def _has(forms, form):
    """whether a counter named `form`, or `form` with further flags behind it (.mask, .planes, .rev), is non-zero"""
    return any(name == form or name.startswith(form + ".") for name in forms)


class Run:
    """One net on the GPU with capture on, the OracleNet of the same configuration (for its grids, masks and, in (c), its step), and
    one minibatch of seeded egs."""

    def __init__(self, pkg, kw, H, dropout=0.0, param_seed=3, stddev=0.3, egs_seed=4):
        kw = dict(kw)
        dropout = kw.pop("dropout_proportion", dropout)
        kw.pop("planes", None)
        self.pkg, self.cfg = pkg, pkg.trainer.make_config(**kw)
        cfg = self.cfg
        self.net = net = pkg.trainer.ChainNet(cfg)
        params = net.init_params_numpy(seed=param_seed, output_stddev=stddev)
        if cfg.darts_num_offsets:  # non-trivial architecture logits (as tests/test_gpu_net.py)
            rng = np.random.default_rng(17)
            for c in net.components:
                n = c["rows"] * c["cols"]
                params[c["begin"] + n:c["begin"] + n + c["num_alpha"]] = rng.standard_normal(c["num_alpha"]).astype(np.float32) * 0.5
        if cfg.bn_num_choices:
            rng = np.random.default_rng(19)
            for c in net.components:
                if c["name"].endswith((".alpha", ".softmax")):
                    params[c["begin"]:c["begin"] + c["rows"]] = rng.standard_normal(c["rows"]).astype(np.float32) * 0.7
        self.params = params
        net.set_params(params)
        net.set_capture(True)
        self.ref = OracleNet(pkg, cfg, net.components)
        if dropout:
            net.set_dropout_proportion(dropout)
            self.ref.set_dropout_proportion(dropout)
        self.feats, self.iv = pkg.trainer.synthetic_egs(net, seed=egs_seed)
        self.den = pkg.synth.make_den_graph(H, cfg.num_pdfs, mean_out_degree=4.0, seed=5)
        self.sup = pkg.synth.make_supervision(cfg.num_sequences, cfg.frames_per_chunk // 3, cfg.num_pdfs, seed=6)
        self.dg, self.ds = pkg.hipabi.DenGraph(self.den), pkg.hipabi.Supervision(self.sup)
        self.fd, self.ivd = dev(self.feats), dev(self.iv)

    def draws(self, step):
        return np.random.default_rng(100 + step).uniform(1e-3, 1 - 1e-3, max(self.net.num_draws, 1)).astype(np.float32)

    def step(self, step):
        """-> (draws, stats before, stats after, results) of one forward_backward from zeroed gradients"""
        net = self.net
        d = self.draws(step)
        net.set_random_draws(d)
        net.grads.zero_()
        st0 = net.get_stats()
        r = host(net.forward_backward(self.fd, self.ivd, self.dg, self.ds, step=step)).copy()
        assert r[5] == 1.0
        return d, st0, net.get_stats(), r

    def act(self, name):
        return host(self.net.activation(name))

    def close(self):
        self.net.close()


def sweep_specs(cfg):
    """The BatchNorm / ReLU backward sweeps of one step in the order the trainer runs them (xent head, chain head, the tdnnf layers from
    the top, tdnn1): that order numbers the store / repair coins and the StoreBackpropStats draws."""
    sp = []
    for hn in ("xent", "chain"):
        p = "prefinal-" + hn
        sp.append(dict(tag=p, x=p + ".relu", dz=p + ".batchnorm1.deriv", d=p + ".affine.deriv", mask=None, bn=hn + "1", relu="head" + hn, comp=p + ".affine"))
    for i in reversed(range(cfg.num_layers)):
        p = "tdnnf%d" % (i + 2)
        sp.append(dict(tag=p, x=p + ".relu", dz=p + ".noop.deriv", d=p + ".affine.deriv", mask=i + 1, bn=p, relu=p, comp=p + ".affine"))
    sp.append(dict(tag="tdnn1", x="tdnn1.relu", dz="tdnn1.batchnorm.deriv", d="tdnn1.affine.deriv", mask=0, bn="tdnn1", relu="tdnn1", comp="tdnn1.affine"))
    return sp


def stat_offsets(ref):
    out, o = {}, 0
    for kind, key in ref._stat_keys():
        D = ref._stat_dim(kind, key)
        out[(kind, key)] = (o, D)
        o += 1 + 2 * D if kind == "bn" else 2 + 3 * D
    return out


def _upd(worst, key, value):
    worst[key] = max(worst.get(key, 0.0), float(value))


def check_sweeps(run, step, draws, st0, st1, worst, repairs=None):
    """(a) for one step: every sweep's d_aff, bias gradient and ReLU statistics, every layer's forward output.  worst: {quantity: largest
    scaled error so far}, updated BEFORE each assertion.  repairs (optional list): receives every sweep's repair vector that was on."""
    cfg, ref, net = run.cfg, run.ref, run.net
    cv = bool(cfg.cv_update)
    masks = ref._dropout_masks(draws)
    offs = stat_offsets(ref)
    g = host(net.grads)
    coin_k = 0

    def coin():
        nonlocal coin_k
        v = decision(step, 2 * coin_k) & 1
        coin_k += 1
        return v

    def columns(sp, x):
        """-> mean, scale and the scale's conditioning (backward_ref64.scale_cond64) per column"""
        if cv:
            o, D = offs[("bn", sp["bn"])]
            mean, var, scale = R.bn_columns_test64(st0[o:o + 1 + 2 * D])
        else:
            mean, var, scale = R.bn_columns64(x)
        return mean, scale, R.scale_cond64(mean, var)

    for k, sp in enumerate(sweep_specs(cfg)):
        x, dz, got = run.act(sp["x"]), run.act(sp["dz"]), run.act(sp["d"])
        N, D = x.shape
        c = coin()
        store = bool(c) or step == 0
        repair_on = cfg.relu_self_repair_scale > 0 and bool(coin())
        mrows = ref._mask_rows(masks[sp["mask"]], N) if masks is not None and sp["mask"] is not None else None
        mean, scale, cond = columns(sp, x)
        o, _ = offs[("relu", sp["relu"])]
        b0, b1 = st0[o:o + 2 + 3 * D], st1[o:o + 2 + 3 * D]
        # (RepairGradients sees the statistics including this minibatch's, when it was stored: the block AFTER the step)
        rep = R.relu_repair64(b1[1 + D:1 + 2 * D], b1[0], cfg.relu_self_repair_scale) if repair_on else None
        if rep is not None and repairs is not None:
            repairs.append(rep)
        want = R.bn_relu_bwd64(x, dz, mean, scale, 1.0, mrows, cv, rep, cond)
        e = R.scaled_error(got, want["d_aff"], want["d_aff_mag"])
        _upd(worst, "d_aff", e.max())
        assert e.max() <= R.K["d_aff"], (sp["tag"], step, e.max(), np.unravel_index(e.argmax(), e.shape))
        off = ~want["on"]  # a unit that is off passes nothing but the repair term, exactly
        assert np.array_equal(got[off], np.broadcast_to(want["repair"].astype(np.float32), got.shape)[off]), (sp["tag"], step)
        comp = ref.comp[sp["comp"]]
        if not cfg.use_natural_gradient:  # (with it the bias is a column of the preconditioned matrix)
            b = comp["begin"] + comp["rows"] * comp["cols"] + comp["num_alpha"]
            if comp["lr_factor"] == 0.0:
                assert not g[b:b + D].any(), sp["tag"]
            else:
                g64 = got.astype(np.float64)
                e = R.scaled_error(g[b:b + D], g64.sum(0), np.abs(g64).sum(0))
                _upd(worst, "colsum", e.max())
                assert e.max() <= R.K["colsum"], (sp["tag"], step, e.max())
        if store:
            assert b1[0] - b0[0] == N and np.array_equal(b1[1 + D:1 + 2 * D] - b0[1 + D:1 + 2 * D], want["deriv_count"]), (sp["tag"], step)
            e = R.scaled_error(b1[1:1 + D] - b0[1:1 + D], want["value_sum"], want["value_sum_mag"])
            _upd(worst, "value_sum", e.max())
            assert e.max() <= R.K["value_sum"], (sp["tag"], step, e.max())
        else:
            assert np.array_equal(b1[:1 + 2 * D], b0[:1 + 2 * D]), (sp["tag"], step)
        skip = b0[1 + 2 * D] != 0 and decision(step, 2 * (4096 + k)) % 4 == 0  # StoreBackpropStats: three minibatches in four
        if skip:
            assert np.array_equal(b1[1 + 2 * D:], b0[1 + 2 * D:]), (sp["tag"], step)
        else:
            assert b1[1 + 2 * D] - b0[1 + 2 * D] == N, (sp["tag"], step)
            e = R.scaled_error(b1[2 + 2 * D:] - b0[2 + 2 * D:], want["oderiv_sumsq"], want["oderiv_mag"])
            _upd(worst, "oderiv_sumsq", e.max())
            assert e.max() <= R.K["oderiv_sumsq"], (sp["tag"], step, e.max())

    # forward: tdnn1.batchnorm = BN(tdnn1.relu) mask; X.noop = BN(X.relu) mask + bypass_scale * (the layer's input on the output-grid rows)
    x = run.act("tdnn1.relu")
    mean, scale, cond = columns(dict(bn="tdnn1"), x)
    m0 = ref._mask_rows(masks[0], x.shape[0]) if masks is not None else None
    prev = run.act("tdnn1.batchnorm")
    e = R.scaled_error(prev, R.bn_apply_bypass64(x, mean, scale, m0), R.bn_apply_bypass_mag64(x, mean, scale, m0, cond=cond))
    _upd(worst, "forward", e.max())
    assert e.max() <= R.K["forward"], ("tdnn1.batchnorm", step, e.max())
    for i, Ly in enumerate(ref.layers):
        nm = "tdnnf%d" % (i + 2)
        x, out = run.act(nm + ".relu"), run.act(nm + ".noop")
        mean, scale, cond = columns(dict(bn=nm), x)
        mrows = ref._mask_rows(masks[i + 1], x.shape[0]) if masks is not None else None
        rows = ref._rows_on(Ly["inn"], Ly["out"])
        args = (x, mean, scale, mrows, cfg.bypass_scale, prev[rows])
        e = R.scaled_error(out, R.bn_apply_bypass64(*args), R.bn_apply_bypass_mag64(*args, cond=cond))
        _upd(worst, "forward", e.max())
        assert e.max() <= R.K["forward"], (nm + ".noop", step, e.max(), np.unravel_index(e.argmax(), e.shape))
        prev = out


def _report(case, worst):
    print("PARITY test_gpu_backward_layers %s scaled error (x 2^-24 mag) " % case +
          " ".join("%s %.2f (bar %.0f)" % (q, v, R.K[q]) for q, v in sorted(worst.items())))


def _assert_forms(forms, wanted):
    for form in wanted:
        assert _has(forms, form), (form, forms)


@pytest.mark.parametrize("case", list(TEACHER_CASES))
def test_sweeps_match_float64_per_element(pkg, case):
    kw, H, dropout, options, steps, wanted = TEACHER_CASES[case]
    worst = {}
    with contextlib.ExitStack() as stack:
        for name, value in options.items():
            stack.enter_context(pkg.hipabi.option(name, value))
        run = Run(pkg, kw, H, dropout, stddev=0.1 if kw.get("use_natural_gradient") else 0.3)
        pkg.hipabi.fused_forms(reset=True)
        grads = []
        for step in steps:
            draws, st0, st1, _ = run.step(step)
            check_sweeps(run, step, draws, st0, st1, worst)
            grads.append(host(run.net.grads).copy())
            run.net.update(1e-3, step=step)
        forms = pkg.hipabi.fused_forms(reset=True)
        run.close()
        _report(case, worst)
        _assert_forms(forms, wanted)
        if case == "ng-nt2-dropout":  # hidden 96: output rank 48, the two-tile class
            assert not _has(forms, "bwd.apply_ng.nt1") and not _has(forms, "bwd.apply_ng.nt3"), forms
        if kw.get("use_natural_gradient"):
            # H = d_aff W^T rides on the sweep and is not exposed: the gradients it preconditions against those of the separate pass
            # (option ng_fuse 0), as tests/test_gpu_net.py::test_fused_output_statistics_match_the_separate_pass holds them
            with pkg.hipabi.option("ng_fuse", 0):
                sep = Run(pkg, kw, H, dropout, stddev=0.1)
                for step, gf in zip(steps, grads):
                    sep.step(step)
                    gs = host(sep.net.grads)
                    assert rel_l2(gf, gs) < 1e-4, (step, rel_l2(gf, gs))
                    sep.net.update(1e-3, step=step)
                assert not _has(pkg.hipabi.fused_forms(reset=True), "bwd.apply_ng")
                sep.close()


def test_self_repair_term_in_both_directions(pkg):
    """Step 1 of the vec4 net with the ReLU statistics of step 0 rewritten (set_stats) so that a third of the columns of every ReLU sit
    under the 5 % threshold, a third over the 95 % one: the repair term is +, - and 0 within one sweep."""
    kw, H = net_case("7q-shape-small")
    run = Run(pkg, kw, H)
    run.step(0)
    run.net.update(1e-3, step=0)
    st, ref = run.net.get_stats(), run.ref
    for (kind, key), (o, D) in stat_offsets(ref).items():
        if kind != "relu":
            continue
        st[o] *= 100.0  # (a count this minibatch's own frames cannot move across a threshold)
        ds = np.full(D, 0.5 * st[o])
        ds[0::3], ds[1::3] = 0.0, st[o]
        st[o + 1 + D:o + 1 + 2 * D] = ds
    run.net.set_stats(st)
    pkg.hipabi.fused_forms(reset=True)
    worst, repairs = {}, []
    draws, st0, st1, _ = run.step(1)
    assert np.array_equal(st0, st)
    check_sweeps(run, 1, draws, st0, st1, worst, repairs)
    forms = pkg.hipabi.fused_forms(reset=True)
    run.close()
    _report("self-repair", worst)
    assert forms.get("bwd.repair", 0) == len(repairs) >= 1, (forms, len(repairs))
    assert any((r > 0).any() and (r < 0).any() and (r == 0).any() for r in repairs)


def test_test_mode_sweeps(pkg):
    """cv-update: BatchNormTestComponent from stored statistics (here: those two training steps of the pretrain net left) -- the
    finalize launch's test mode, d_aff = relu'(x) dz scale with mean and scale from the statistics block."""
    _, pre_kw, cv_kw = CV_CASES[0]
    pre = Run(pkg, pre_kw, 40)
    for step in (0, 1):
        pre.step(step)
        pre.net.update(1e-3, step=step)
    st = pre.net.get_stats()
    pre.close()
    run = Run(pkg, cv_kw, 40)
    run.net.set_stats(st)
    pkg.hipabi.fused_forms(reset=True)
    worst = {}
    for step in (0, 1):
        draws, st0, st1, _ = run.step(step)
        check_sweeps(run, step, draws, st0, st1, worst)
    forms = pkg.hipabi.fused_forms(reset=True)
    run.close()
    _report("test-mode", worst)
    assert forms.get("bwd.finalize.test", 0) >= 1 and not forms.get("bwd.finalize.train"), forms


_NAMES = ["lda", "tdnn1.relu", "tdnn1.batchnorm", "tdnn1.batchnorm.deriv", "tdnn1.affine.deriv", "prefinal-l", "prefinal-l.deriv", "output", "output-xent",
          "output.deriv", "output-xent.deriv"]


def all_names(cfg):
    names = list(_NAMES)
    for i in range(cfg.num_layers):
        names += ["tdnnf%d%s" % (i + 2, s) for s in (".linear", ".relu", ".noop", ".noop.deriv", ".affine.deriv", ".linear.deriv")]
    for hn in ("chain", "xent"):
        names += ["prefinal-%s%s" % (hn, s) for s in (".relu", ".batchnorm2.deriv", ".linear.deriv", ".batchnorm1.deriv", ".affine.deriv")]
    return names


@pytest.mark.parametrize("case", ["vec4", "mask-superrow", "ng-nt2-dropout"])
def test_reversed_walk_changes_no_bit(pkg, case):
    """Option reverse_passes (bit 0: bn_apply_bypass, bit 1: bn_relu_bwd's apply launch) only changes which rows a block takes first, not
    the order of any sum: every activation, every captured derivative and the gradient are the same bits."""
    kw, H, dropout, options, steps, _ = TEACHER_CASES[case]

    def collect(rev):
        out = []
        with contextlib.ExitStack() as stack:  # (restores every option on the way out, whatever happens)
            for name, value in dict(options, reverse_passes=rev).items():
                stack.enter_context(pkg.hipabi.option(name, value))
            run = Run(pkg, kw, H, dropout, stddev=0.1 if kw.get("use_natural_gradient") else 0.3)
            pkg.hipabi.fused_forms(reset=True)
            for step in steps:
                run.step(step)
                out.append(dict({n: run.act(n) for n in all_names(run.cfg)}, grads=host(run.net.grads).copy()))
                run.net.update(1e-3, step=step)
            forms = pkg.hipabi.fused_forms(reset=True)
            run.close()
        return out, forms

    plain, forms0 = collect(0)
    rev, forms3 = collect(3)
    assert not any(".rev" in f for f in forms0), forms0
    assert any(f.startswith("apply_bypass.vec4") and f.endswith(".rev") for f in forms3), forms3
    assert any(f.startswith("bwd.apply_ng" if "ng" in case else "bwd.apply.vec4") and f.endswith(".rev") for f in forms3), forms3
    assert {f.replace(".rev", ""): v for f, v in forms3.items()} == forms0  # the same launches otherwise
    for step, (a, b) in enumerate(zip(plain, rev)):
        for name in a:
            assert np.array_equal(a[name], b[name]), (step, name)


# one case per family of tests/test_gpu_net.py's CASES (+ the cv-update hand-over of CV_CASES)
CHAIN_CASES = ["7q-shape-small", "manual-offset6", "ragged-dims", "darts-k7-softmax", "bn-supernet-softmax-flops", "child-offsets", "7q-shape-small-dropout",
               "7q-shape-small-NG", "cv-update"]
TIE_CAP = 2000  # ties handed over by relu_like: at most 1 in 2 000 elements of each ReLU
# the seed of a case's features where it is not 4: chosen so that the oracle's own pre-activations keep the cap (tests/test_backward_ref64.py)
CHAIN_EGS_SEED = {"manual-offset6": 7}


def chain_setup(pkg, case):
    """-> (kwargs, den-graph states, pretrain kwargs or None) of one chained case"""
    if case == "cv-update":
        return dict(CV_CASES[0][2]), 40, dict(CV_CASES[0][1])
    kw, H = net_case(case)
    return kw, H, None


def relu_names(cfg):
    return ["tdnn1.relu"] + ["tdnnf%d.relu" % (l + 2) for l in range(cfg.num_layers)] + ["prefinal-chain.relu", "prefinal-xent.relu"]


@pytest.mark.parametrize("case", CHAIN_CASES)
def test_every_derivative_matches_the_oracle(pkg, case):
    kw, H, pre_kw = chain_setup(pkg, case)
    run = Run(pkg, kw, H, egs_seed=CHAIN_EGS_SEED.get(case, 4))
    cfg, net, ref = run.cfg, run.net, run.ref
    if pre_kw is not None:  # the statistics two training steps of the pretrain net left, for both sides
        pre = Run(pkg, pre_kw, H, egs_seed=CHAIN_EGS_SEED.get(case, 4))
        for step in (0, 1):
            pre.step(step)
            pre.net.update(1e-3, step=step)
        st = pre.net.get_stats()
        pre.close()
        net.set_stats(st)
        ref.set_stats(st)
    bar = 1e-3 if cfg.gemm_precision == 1 else 1e-4  # the activation bar of test_net_step_matches_oracle
    params = run.params
    compared = set()
    for step in (0, 1):
        draws, _, _, r = run.step(step)
        like = {k: run.act(k) for k in relu_names(cfg)}
        res_ref, g_ref, acts = ref.forward_backward(params, run.feats, run.iv, run.den, run.sup, step=step, draws=draws, relu_like=like)
        for name, n in ref.relu_ties.items():
            assert n * TIE_CAP <= like[name].size, (name, n, like[name].size)
        for name in sorted(k for k in acts if k.endswith(".deriv")):
            try:
                got = run.act(name)
            except pkg.hipabi.HipAbiError:
                continue  # (a name only the oracle holds)
            e = rel_l2(got, acts[name])
            print("PARITY test_gpu_backward_layers chained %s step %d %s %.3e (bar %.0e)" % (case, step, name, e, bar))
            assert e < bar, (name, step, e)
            compared.add(name)
        params = ref.update(params, g_ref, 1e-3, float(cfg.num_sequences), step)
        net.set_params(params)
    run.close()
    want = {"tdnn1.batchnorm.deriv", "tdnn1.affine.deriv", "prefinal-l.deriv", "output-xent.deriv"}
    want |= {"tdnnf%d%s" % (i + 2, s) for i in range(cfg.num_layers) for s in (".noop.deriv", ".affine.deriv", ".linear.deriv")}
    want |= {"prefinal-%s%s" % (hn, s) for hn in ("chain", "xent") for s in (".batchnorm2.deriv", ".linear.deriv", ".batchnorm1.deriv", ".affine.deriv")}
    assert want <= compared, sorted(want - compared)
