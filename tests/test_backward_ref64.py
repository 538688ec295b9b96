"""Pins tests/backward_ref64.py (the float64 restatement of the fused BatchNorm / ReLU sweeps) without a GPU:
  * against float64 torch autograd: d_aff is the gradient w.r.t. a of sum(dz * mask * BN(relu(a))), train and test mode, with and
    without a mask, to 1e-12;
  * against the float32 C oracle chained over the same inputs (oracle_batchnorm_propagate / _backprop, the ReLU mask,
    oracle_relu_repair) on every sweep shape tests/test_gpu_backward_layers.py runs: the oracle's largest scaled error per quantity is
    PRINTED and four times it must stay within the bar K that file holds the kernels to (backward_ref64.K; at least 8);
  * the ReLU ties the chained GPU test may hand over are capped by the oracle alone, for the seeds that test uses.
"""
import types

import numpy as np
import pytest
import torch

from tests import backward_ref64 as R
from tests.oracle_net import OracleNet, component_table
from tests.test_gpu_backward_layers import CHAIN_CASES, CHAIN_EGS_SEED, TEACHER_CASES, TIE_CAP, chain_setup
from tests.test_gpu_net import CV_CASES

F = np.float32


def _inputs(rows, D, seed, B=None):
    """A ReLU output with a spread of column means and on-rates (pre-activations kept 0.05 away from zero), a derivative, and mask rows
    in the dropout component's range for p = 0.3 (one row per sequence, row r -> sequence r % B)."""
    rng = np.random.default_rng(seed)
    a = rng.standard_normal((rows, D)) * rng.uniform(0.5, 2.0, D) + rng.uniform(-1.0, 1.0, D)
    a = np.where(np.abs(a) < 0.05, np.where(a < 0, -0.05, 0.05), a)
    dz = rng.standard_normal((rows, D)) * 10.0 ** rng.uniform(-3, 0, D)
    mask = None
    if B:
        mask = np.tile(rng.uniform(0.4, 1.6, (B, D)), (-(-rows // B), 1))[:rows]
    return a.astype(F), dz.astype(F), None if mask is None else mask.astype(F)


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("test_mode", [False, True], ids=["train", "test"])
def test_d_aff_is_the_autograd_gradient(test_mode, masked):
    a32, dz32, m32 = _inputs(37, 21, 1, B=5 if masked else None)
    a = torch.tensor(a32.astype(np.float64), requires_grad=True)
    dz = torch.tensor(dz32.astype(np.float64))
    m = torch.tensor(m32.astype(np.float64)) if masked else torch.ones_like(dz)
    x = torch.relu(a)
    if test_mode:  # stored statistics of some other data: constants of the graph
        st = np.concatenate([[50.0], np.random.default_rng(2).uniform(10, 40, 21), np.random.default_rng(3).uniform(60, 90, 21)])
        mean, _, scale = R.bn_columns_test64(st)
        z = (x - torch.tensor(mean)) * torch.tensor(scale)
    else:
        mean_t = x.mean(0)
        var_t = (x * x).mean(0) - mean_t * mean_t
        z = (x - mean_t) / torch.sqrt(var_t + 1e-3)
        mean, _, scale = R.bn_columns64(x.detach().numpy())
    (dz * m * z).sum().backward()
    got = R.bn_relu_bwd64(x.detach().numpy(), dz32, mean, scale, 1.0, m32, test_mode, None)
    want = a.grad.numpy()
    err = np.linalg.norm(got["d_aff"] - want) / np.linalg.norm(want)
    assert err < 1e-12, err
    assert np.abs(got["d_aff"] - want).max() <= 1e-12 * got["d_aff_mag"].max()
    assert np.array_equal(got["colsum"], got["d_aff"].sum(0)) and (got["d_aff_mag"] >= np.abs(got["d_aff"]) * (1 - 1e-12)).all()


def test_repair_term_thresholds():
    ds = np.array([0.0, 4.0, 5.0, 6.0, 50.0, 94.0, 95.0, 96.0, 100.0])
    r = R.relu_repair64(ds, 100.0, 1e-5)
    assert np.array_equal(np.sign(r), [1, 1, 1, 0, 0, 0, 0, -1, -1]) and set(np.abs(r[r != 0])) == {1e-5 / 0.5}
    assert not R.relu_repair64(ds, 0.0, 1e-5).any() and not R.relu_repair64(ds, 100.0, 0.0).any()


def sweep_shapes(pkg):
    """{(rows, columns, sequences or 0 = no mask, test mode)} over every sweep of every net of the GPU test's teacher-forced cases"""
    shapes = set()
    nets = [(kw, dropout, False) for kw, _, dropout, _, _, _ in TEACHER_CASES.values()] + [(CV_CASES[0][2], 0.0, True)]
    for kw, dropout, cv in nets:
        kw = dict(kw)
        kw.pop("dropout_proportion", None)
        kw.pop("planes", None)
        cfg = pkg.trainer.make_config(**kw)
        ref = OracleNet(pkg, cfg, component_table(cfg)[0])
        B, D = cfg.num_sequences, cfg.hidden_dim
        mb = B if dropout else 0
        shapes.add((ref.Tout * B, D, 0, cv))  # the heads: never masked
        shapes.add((ref.g_lda[2] * B, D, mb, cv))
        for Ly in ref.layers:
            shapes.add((Ly["out"][2] * B, D, mb, cv))
    return sorted(shapes)


def test_oracle_chain_scaled_errors_give_the_gpu_bars(pkg, ora):
    """The float32 C oracle, chained as OracleNet chains it, against backward_ref64 on the GPU test's sweep shapes.  Prints the oracle's
    largest scaled error max |oracle - ref64| / (2^-24 mag) per quantity and shape; K (backward_ref64.K) must be at least four times the
    largest of them, and is never below 8."""
    L = ora.lib()
    worst = {q: 0.0 for q in R.K}
    for rows, D, B, cv in sweep_shapes(pkg):
        x, dz, mask = _inputs(rows, D, 7 + rows + D, B or None)
        x = np.maximum(x, 0)
        prev = np.random.default_rng(rows).standard_normal((rows, D)).astype(F)
        z, memo = np.zeros_like(x), np.zeros((5, D), F)
        if cv:
            rng = np.random.default_rng(5)
            cnt = 3.0 * rows
            st = np.concatenate([[cnt], cnt * (x.mean(0) + rng.uniform(-0.1, 0.1, D)), cnt * ((x.astype(np.float64) ** 2).mean(0) * rng.uniform(1.0, 1.3, D))])
            scale, offset = np.zeros(D, F), np.zeros(D, F)
            L.oracle_batchnorm_compute_derived(cnt, ora.dptr(np.ascontiguousarray(st[1:1 + D])), ora.dptr(np.ascontiguousarray(st[1 + D:])), D, 1e-3, 1.0,
                                               ora.fptr(scale), ora.fptr(offset))
            L.oracle_batchnorm_test_propagate(ora.omat(x), ora.fptr(scale), ora.fptr(offset), ora.omat(z))
            mean64, var64, scale64 = R.bn_columns_test64(st)
        else:
            L.oracle_batchnorm_propagate(ora.omat(x), 1e-3, 1.0, ora.omat(z), ora.fptr(memo))
            mean64, var64, scale64 = R.bn_columns64(x)
        cond = R.scale_cond64(mean64, var64)
        # forward, as OracleNet: (z * mask), bypass_scale * prev + that
        zm = z if mask is None else (z * mask).astype(F)
        out = (F(0.66) * prev + zm).astype(F)
        args = (x, mean64, scale64, mask, float(F(0.66)), prev)
        e_fwd = R.scaled_error(out, R.bn_apply_bypass64(*args), R.bn_apply_bypass_mag64(*args, cond=cond)).max()
        # backward: derivative through the mask, BatchNorm, ReLU mask, repair
        dzm = dz if mask is None else (dz * mask).astype(F)
        dx = np.zeros_like(x)
        if cv:
            L.oracle_batchnorm_test_backprop(ora.omat(dzm), ora.fptr(scale), ora.omat(dx))
        else:
            L.oracle_batchnorm_backprop(ora.omat(z), ora.omat(dzm), 1.0, ora.fptr(memo), ora.omat(dx))
        dd = ((x > 0) * dx).astype(F)
        cnt_relu = 10.0 * rows
        ds = np.ascontiguousarray(np.random.default_rng(9).choice([0.0, 0.5, 1.0], D) * cnt_relu)
        L.oracle_relu_repair(ora.dptr(ds), cnt_relu, D, 1e-5, 0.05, 0.95, ora.omat(dd))
        rep = R.relu_repair64(ds, cnt_relu, 1e-5)
        assert (rep > 0).any() and (rep < 0).any()
        want = R.bn_relu_bwd64(x, dz, mean64, scale64, 1.0, mask, cv, rep, cond)
        e = dict(forward=e_fwd, d_aff=R.scaled_error(dd, want["d_aff"], want["d_aff_mag"]).max(),
                 # float32 column sums of the oracle's d_aff as its update forms them (double accumulation, one rounding)
                 colsum=R.scaled_error(dd.astype(np.float64).sum(0).astype(F), dd.astype(np.float64).sum(0), np.abs(dd.astype(np.float64)).sum(0)).max(),
                 value_sum=R.scaled_error(x.astype(np.float64).sum(0), want["value_sum"], want["value_sum_mag"]).max(),
                 oderiv_sumsq=R.scaled_error((dx.astype(np.float64) ** 2).sum(0), want["oderiv_sumsq"], want["oderiv_mag"]).max())
        print("PARITY test_backward_ref64 oracle %4d x %4d %s %s  " % (rows, D, "mask" if B else "    ", "test " if cv else "train") +
              " ".join("%s %.2f" % kv for kv in sorted(e.items())))
        for q, v in e.items():
            worst[q] = max(worst[q], float(v))
    print("PARITY test_backward_ref64 oracle maxima " + " ".join("%s %.2f -> K %.0f" % (q, v, R.K[q]) for q, v in sorted(worst.items())))
    for q, v in worst.items():
        assert R.K[q] >= 8.0 and 4.0 * v <= R.K[q], (q, v, R.K[q])
        assert R.K[q] <= max(8.0, 4.0 * v + 1.0), (q, v, R.K[q])  # (not wider than the rule gives either: 4 x, rounded up to a whole number)


def _host_net(pkg, cfg, comps, num_params, ref):
    """what trainer.synthetic_egs and ChainNet.init_params_numpy read of a net, without a GPU"""
    return types.SimpleNamespace(cfg=cfg, components=comps, num_params=num_params, num_t_in=ref.num_t_in)


def _params(pkg, cfg, hn):
    params = pkg.trainer.ChainNet.init_params_numpy(hn, seed=3, output_stddev=0.3)
    if cfg.darts_num_offsets:
        rng = np.random.default_rng(17)
        for c in hn.components:
            n = c["rows"] * c["cols"]
            params[c["begin"] + n:c["begin"] + n + c["num_alpha"]] = rng.standard_normal(c["num_alpha"]).astype(F) * 0.5
    if cfg.bn_num_choices:
        rng = np.random.default_rng(19)
        for c in hn.components:
            if c["name"].endswith((".alpha", ".softmax")):
                params[c["begin"]:c["begin"] + c["rows"]] = rng.standard_normal(c["rows"]).astype(F) * 0.7
    return params


def _oracle_steps(pkg, kw, H, dropout, stats=None, egs_seed=4):
    """The two steps of tests/test_gpu_backward_layers.py::Run on the oracle alone -> (ref, [relu_near_zero of each step])"""
    kw = dict(kw)
    dropout = kw.pop("dropout_proportion", dropout)
    kw.pop("planes", None)
    cfg = pkg.trainer.make_config(**kw)
    comps, num_params = component_table(cfg)
    ref = OracleNet(pkg, cfg, comps)
    if stats is not None:
        ref.set_stats(stats)
    if dropout:
        ref.set_dropout_proportion(dropout)
    hn = _host_net(pkg, cfg, comps, num_params, ref)
    params = _params(pkg, cfg, hn)
    feats, iv = pkg.trainer.synthetic_egs(hn, seed=egs_seed)
    den = pkg.synth.make_den_graph(H, cfg.num_pdfs, mean_out_degree=4.0, seed=5)
    sup = pkg.synth.make_supervision(cfg.num_sequences, cfg.frames_per_chunk // 3, cfg.num_pdfs, seed=6)
    # (the trainer's draw count is the library's to say; numpy's generator fills an array front to back, so a longer one starts the same)
    L, K = cfg.num_layers, int(cfg.darts_num_offsets)
    n_draws = 2 * (K + 1) * L + int(cfg.bn_num_choices) * L + (L + 1) * cfg.num_sequences * cfg.hidden_dim + 16
    near = []
    for step in (0, 1):
        draws = np.random.default_rng(100 + step).uniform(1e-3, 1 - 1e-3, n_draws).astype(F)
        _, g_ref, _ = ref.forward_backward(params, feats, iv, den, sup, step=step, draws=draws)
        near.append(dict(ref.relu_near_zero))
        params = ref.update(params, g_ref, 1e-3, float(cfg.num_sequences), step)
    return ref, near


@pytest.mark.parametrize("case", CHAIN_CASES)
def test_relu_ties_of_the_chained_cases_stay_under_the_cap(pkg, case):
    """Only a pre-activation within relu_tie_tol x rms of zero ON THE ORACLE'S SIDE can be handed over as a tie (tests/oracle_net.py,
    relu_of).  For the seeds of the chained GPU test the oracle's own count of those stays within 1 in 2 000 elements of every ReLU,
    so the cap that test asserts can only be exceeded by a genuine difference."""
    kw, H, pre_kw = chain_setup(pkg, case)
    stats = None
    if pre_kw is not None:
        stats = _oracle_steps(pkg, pre_kw, H, 0.0, egs_seed=CHAIN_EGS_SEED.get(case, 4))[0].get_stats()
    _, near = _oracle_steps(pkg, kw, H, 0.0, stats, egs_seed=CHAIN_EGS_SEED.get(case, 4))
    for step, d in enumerate(near):
        assert len(d) == pkg.trainer.make_config(**{k: v for k, v in kw.items() if k not in ("dropout_proportion", "planes")}).num_layers + 3
        for name, (n, size) in d.items():
            assert n * TIE_CAP <= size, (case, step, name, n, size)
