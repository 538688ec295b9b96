"""-m gpu: every C-ABI entry on sub-matrix views.  include/tdnnf_hip.h promises that a tdnnf_mat is Kaldi's CuMatrixBase<float>
view -- any device pointer, any stride >= cols -- and almost every pass in csrc/ picks one of two or three bodies on the host from
exactly those properties (vec4_ok, operands_vec4 / c_vec of the rows GEMM, the vec flag of the weight gradient and of the tap dots,
the alignment test in front of the one-pass log-softmax).  Each entry runs here

  - with all its matrix operands in each layout of tests/view_layouts.py (dense, pitched, odd stride, base 4 / 8 bytes off, both),
    at a width that is a multiple of 4, one that is 2 mod 4 and an odd one,
  - then once per operand with only that operand misaligned (matrices: off1-odd; vectors: one float off, the bias three floats off
    as behind the three architecture logits of a DARTS component) and the rest dense: a term missing from a dispatch AND,
  - and, where the component advertises it (include/tdnnf_nnet3_components.h), in place,

and is held to a float64 restatement of the operation at the tolerance tests/test_gpu_parity.py has for the entry (exact copies and
selections: equality), to the guard cells around every operand (NaN around what is read, a fixed pattern around what is written),
and -- per-element maps -- to bit-identity with the dense run.  Reductions and GEMMs print whether they came out bit-identical
("LAYOUT-BITS ...", shown with -s).  Shapes: 261 rows (three 128-row tiles with a ragged one, nine chunks of the column reduction),
260 / 262 / 261 columns (more than one 256-, 128- and 64-column block of the column reduction)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.gpu_util import F, Hip, host, rel_l2
from tests.view_layouts import LAYOUTS, laid_out, laid_out_vec

pytestmark = pytest.mark.gpu
TOL = 2e-5          # tests/test_gpu_parity.py: the GEMMs and BatchNorm, relative L2
N = 261
WIDTHS = (260, 262, 261)
WIDS = ["w4", "w2", "odd"]
D64 = np.float64


@pytest.fixture(scope="module")
def hip(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Hip(pkg)


def _rand(rng, *shape):
    return rng.standard_normal(shape).astype(F)


class Lay:
    """Hands a run its operands: every matrix in `default`, except the operand named `special` (matrix: off1-odd, vector: shifted)."""

    def __init__(self, default="dense", special=None):
        self.default, self.special, self.checks, self.names = default, special, [], []

    def _keep(self, name, made):
        view, _, check = made
        if name not in self.names:
            self.names.append(name)
        self.checks.append((name, check))
        return view

    def m(self, name, a, writes=False):
        return self._keep(name, laid_out(a, "off1-odd" if name == self.special else self.default, writes=writes))

    def v(self, name, a, writes=False, shift=1):
        return self._keep(name, laid_out_vec(a, shift if name == self.special else 0, writes=writes))

    def check(self, what):
        for name, check in self.checks:
            try:
                check()
            except AssertionError as e:
                raise AssertionError("%s: operand %s: %s" % (what, name, e)) from None


def _compare(got, ref, what):
    for key, (want, kind, *tol) in ref.items():
        g = got[key]
        assert g.shape == np.shape(want), (what, key)
        if kind == "exact":
            assert np.array_equal(g, np.asarray(want, dtype=g.dtype)), "%s: %s differs" % (what, key)
        elif kind == "close":
            np.testing.assert_allclose(g, want, rtol=tol[0], atol=tol[1], err_msg="%s: %s" % (what, key))
        else:
            assert np.isfinite(g).all() and rel_l2(g, want) < tol[0], "%s: %s rel-L2 %.3g" % (what, key, rel_l2(g, want))


def sweep(hip, name, run, d, ref, bitwise, layouts=LAYOUTS):
    """run(hip, L, d) -> {output: host array}.  All operands per layout, then one operand misaligned at a time."""
    L = Lay("dense")
    base = run(hip, L, d)
    L.check(name + " dense")
    _compare(base, ref, name + " dense")
    operands = list(L.names)
    plans = [(lay, Lay(lay)) for lay in layouts if lay != "dense"]
    if len(operands) >= 2:
        plans += [("only-" + op, Lay("dense", special=op)) for op in operands]
    same = []
    for tag, L in plans:
        what = "%s %s" % (name, tag)
        got = run(hip, L, d)
        L.check(what)
        _compare(got, ref, what)
        eq = all(np.array_equal(got[k], base[k]) for k in base)
        if bitwise:
            assert eq, "%s: not bit-identical to the dense run" % what
        same.append((tag, eq))
    if not bitwise:
        print("LAYOUT-BITS %s: %s" % (name, " ".join("%s=%s" % (t, "same" if e else "DIFFERS") for t, e in same)))


# ------------------------------------------------------------------------------------------------------ GEMM entries
GEMM_DIMS = [(36, 132), (38, 134), (37, 133)]
TAPS = [("taps-1-0", [-1, 0], 1), ("stride3", [0, 3], 3)]


def _gemm_data(pkg, wi, offs, step):
    Di, Do = GEMM_DIMS[wi]
    rho, ro, rows_in, n = pkg.synth.tdnn_indexes(offs, 29, 9, t_step_out=step)   # 29 x 9 = 261 output rows
    K = len(offs)
    rng = np.random.default_rng(100 + wi + 10 * step)
    d = dict(Di=Di, Do=Do, K=K, rho=rho, ro=ro, rows_in=rows_in, n=n, ix=pkg.hipabi.indexes(rho, ro))
    d["x"], d["dy"] = _rand(rng, rows_in, Di), _rand(rng, n, Do)
    d["W"] = (_rand(rng, Do, K * Di) / np.sqrt(K * Di)).astype(F)
    d["b"], d["y0"], d["dx0"] = _rand(rng, Do), _rand(rng, n, Do), _rand(rng, rows_in, Di)
    d["W0"], d["b0"] = _rand(rng, Do, K * Di), _rand(rng, Do)
    return d


def _taps64(d, c):
    """sum_k c_k X_k W_k^T in float64 (TdnnComponent::Propagate); X_k = the rows ro[k] + rho m of x"""
    rows = np.arange(d["n"]) * d["rho"]
    y = np.zeros((d["n"], d["Do"]))
    for k in range(d["K"]):
        y += c[k] * d["x"].astype(D64)[d["ro"][k] + rows] @ d["W"].astype(D64)[:, k * d["Di"]:(k + 1) * d["Di"]].T
    return y


C_BIAS, C_ZERO = np.asarray([0.6, 1.3], F), np.asarray([0.0, 0.8], F)   # (a zero coefficient skips its tap)


def _run_tdnn_propagate(hip, L, d):
    xd, Wd = L.m("in", d["x"]), L.m("W", d["W"])
    out = {}
    for mode, bias, c in ((1, d["b"], C_BIAS), (0, None, C_ZERO), (2, None, None)):
        yd = L.m("out", d["y0"], writes=True)
        bd = L.v("bias", bias, shift=3) if bias is not None else None
        cd = L.v("coef", c) if c is not None else None
        hip.tdnn_propagate(C.byref(d["ix"]), xd, hip.vec(Wd), Wd.stride(0), d["Do"], d["Di"], bd, cd, mode, yd, hip.stream())
        out["mode%d" % mode] = host(yd)
    return out


@pytest.mark.parametrize("taps", TAPS, ids=[t[0] for t in TAPS])
@pytest.mark.parametrize("wi", range(3), ids=WIDS)
def test_tdnn_propagate(hip, pkg, wi, taps):
    d = _gemm_data(pkg, wi, taps[1], taps[2])
    ref = {"mode1": (d["b"].astype(D64) + _taps64(d, C_BIAS.astype(D64)), "rel", TOL),
           "mode0": (d["y0"].astype(D64) + _taps64(d, C_ZERO.astype(D64)), "rel", TOL),
           "mode2": (_taps64(d, np.ones(2)), "rel", TOL)}
    sweep(hip, "tdnn_propagate", _run_tdnn_propagate, d, ref, bitwise=False)


def _run_tdnn_backprop_data(hip, L, d):
    dyd, Wd, cd = L.m("out_deriv", d["dy"]), L.m("W", d["W"]), L.v("coef", C_BIAS)
    dxd = L.m("in_deriv", d["dx0"], writes=True)
    hip.tdnn_backprop_data(C.byref(d["ix"]), dyd, hip.vec(Wd), Wd.stride(0), d["Do"], d["Di"], cd, dxd, hip.stream())
    return {"added": host(dxd) - d["dx0"]}


@pytest.mark.parametrize("taps", TAPS, ids=[t[0] for t in TAPS])
@pytest.mark.parametrize("wi", range(3), ids=WIDS)
def test_tdnn_backprop_data(hip, pkg, wi, taps):
    d = _gemm_data(pkg, wi, taps[1], taps[2])
    rows = np.arange(d["n"]) * d["rho"]
    want = np.zeros((d["rows_in"], d["Di"]))
    for k in range(d["K"]):   # in_deriv views += c_k dY W_k (kBackpropAdds)
        want[d["ro"][k] + rows] += float(C_BIAS[k]) * d["dy"].astype(D64) @ d["W"].astype(D64)[:, k * d["Di"]:(k + 1) * d["Di"]]
    sweep(hip, "tdnn_backprop_data", _run_tdnn_backprop_data, d, {"added": (want, "rel", TOL)}, bitwise=False)


def _run_tdnn_update_simple(hip, L, d):
    xd, dyd, cd = L.m("in_value", d["x"]), L.m("out_deriv", d["dy"]), L.v("coef", C_BIAS)
    Wacc, bacc = L.m("W_acc", d["W0"], writes=True), L.v("bias_acc", d["b0"], writes=True, shift=3)
    nb = hip.tdnn_update_workspace_bytes(d["Do"], d["Di"], d["K"], d["n"])
    ws = hip.ws(nb)
    hip.tdnn_update_simple(C.byref(d["ix"]), xd, dyd, d["Do"], d["Di"], cd, 0.5, hip.vec(Wacc), Wacc.stride(0), bacc, hip.vec(ws), nb,
                           hip.stream())
    return {"W": host(Wacc) - d["W0"], "bias": host(bacc) - d["b0"]}


@pytest.mark.parametrize("taps", TAPS, ids=[t[0] for t in TAPS])
@pytest.mark.parametrize("wi", range(3), ids=WIDS)
def test_tdnn_update_simple(hip, pkg, wi, taps):
    d = _gemm_data(pkg, wi, taps[1], taps[2])
    rows = np.arange(d["n"]) * d["rho"]
    dy = d["dy"].astype(D64)
    want = np.concatenate([0.5 * float(C_BIAS[k]) * dy.T @ d["x"].astype(D64)[d["ro"][k] + rows] for k in range(d["K"])], axis=1)
    ref = {"W": (want, "rel", TOL), "bias": (0.5 * dy.sum(0), "rel", TOL)}
    sweep(hip, "tdnn_update_simple", _run_tdnn_update_simple, d, ref, bitwise=False)


def _affine_data(wi):
    Di, Do = GEMM_DIMS[wi]
    rng = np.random.default_rng(200 + wi)
    d = dict(Di=Di, Do=Do, x=_rand(rng, N, Di), dy=_rand(rng, N, Do), W=(_rand(rng, Do, Di) / 6).astype(F), b=_rand(rng, Do),
             W0=_rand(rng, Do, Di), b0=_rand(rng, Do))
    return d


def _run_affine_propagate(hip, L, d):
    xd, Wd, bd = L.m("in", d["x"]), L.m("W", d["W"]), L.v("bias", d["b"], shift=3)
    yd = L.m("out", np.full((N, d["Do"]), 3.0, F), writes=True)
    hip.affine_propagate(xd, hip.vec(Wd), Wd.stride(0), bd, d["Do"], yd, hip.stream())
    return {"out": host(yd)}


def _run_affine_backprop(hip, L, d):
    dyd, Wd = L.m("out_deriv", d["dy"]), L.m("W", d["W"])
    dxd = L.m("in_deriv", np.full((N, d["Di"]), 3.0, F), writes=True)   # must be overwritten
    hip.affine_backprop(dyd, hip.vec(Wd), Wd.stride(0), d["Di"], dxd, hip.stream())
    return {"in_deriv": host(dxd)}


def _run_affine_update_simple(hip, L, d):
    xd, dyd = L.m("in_value", d["x"]), L.m("out_deriv", d["dy"])
    Wacc, bacc = L.m("W_acc", d["W0"], writes=True), L.v("bias_acc", d["b0"], writes=True, shift=3)
    nb = hip.tdnn_update_workspace_bytes(d["Do"], d["Di"], 1, N)
    ws = hip.ws(nb)
    hip.affine_update_simple(xd, dyd, 1.0, hip.vec(Wacc), Wacc.stride(0), bacc, hip.vec(ws), nb, hip.stream())
    return {"W": host(Wacc) - d["W0"], "bias": host(bacc) - d["b0"]}


@pytest.mark.parametrize("wi", range(3), ids=WIDS)
def test_affine(hip, wi):
    d = _affine_data(wi)
    x, dy, W = d["x"].astype(D64), d["dy"].astype(D64), d["W"].astype(D64)
    sweep(hip, "affine_propagate", _run_affine_propagate, d, {"out": (x @ W.T + d["b"], "rel", TOL)}, bitwise=False)
    sweep(hip, "affine_backprop", _run_affine_backprop, d, {"in_deriv": (dy @ W, "rel", TOL)}, bitwise=False)
    sweep(hip, "affine_update_simple", _run_affine_update_simple, d, {"W": (dy.T @ x, "rel", TOL), "bias": (dy.sum(0), "rel", TOL)},
          bitwise=False)


# ------------------------------------------------------------------------------------------------------ BatchNorm
EPS, TRMS = 1e-3, 1.0


def _bn_data(w):
    rng = np.random.default_rng(300 + w)
    x = (_rand(rng, N, w) * 1.7 + 0.3).astype(F)
    x64 = x.astype(D64)
    mean, uvar = x64.mean(0), (x64 * x64).mean(0)
    vs = 1.0 / (TRMS * TRMS)
    scale = 1.0 / np.sqrt(np.maximum(vs * (uvar - mean * mean), 0.0) + vs * EPS)   # nnet-normalize-component.cc:433-445
    z = (x64 - mean) * scale
    dz = _rand(rng, N, w)
    memo = np.zeros((5, w), F)
    memo[0], memo[1], memo[2] = mean, uvar, scale
    zf = z.astype(F)
    # Backprop :505-542 from the float memo and output the caller holds
    sc = memo[2].astype(D64)
    vdm = -1.0 / (TRMS * TRMS * N) * (zf.astype(D64) * dz).sum(0) * sc
    temp = -dz.astype(D64).sum(0) / N
    dx = (dz + temp) * sc + zf.astype(D64) * vdm
    tsc, tof = (rng.random(w) + 0.5).astype(F), _rand(rng, w)
    return dict(w=w, x=x, dz=dz, z=zf, memo=memo, z64=z, dx64=dx, stats64=np.stack([mean, uvar, scale]), tsc=tsc, tof=tof)


def _run_bn_propagate(hip, L, d):
    xd, zd = L.m("in", d["x"]), L.m("out", np.zeros_like(d["x"]), writes=True)
    memo = L.v("memo", np.zeros((5, d["w"]), F), writes=True)
    nb = hip.colreduce_workspace_bytes(N, d["w"])
    ws = hip.ws(nb)
    hip.batchnorm_propagate(xd, EPS, TRMS, zd, memo, hip.vec(ws), nb, hip.stream())
    return {"out": host(zd), "memo": host(memo).reshape(5, -1)[:3]}


def _run_bn_backprop(hip, L, d, inplace=False):
    zd, dzd = L.m("out_value", d["z"]), L.m("out_deriv", d["dz"], writes=inplace)
    dxd = dzd if inplace else L.m("in_deriv", np.zeros_like(d["x"]), writes=True)
    memo = L.v("memo", d["memo"], writes=True)
    nb = hip.colreduce_workspace_bytes(N, d["w"])
    ws = hip.ws(nb)
    hip.batchnorm_backprop(zd, dzd, TRMS, memo, dxd, hip.vec(ws), nb, hip.stream())
    return {"in_deriv": host(dxd)}


def _run_bn_test_propagate(hip, L, d, inplace=False):
    xd = L.m("in", d["x"], writes=inplace)
    sc, of = L.v("scale", d["tsc"]), L.v("offset", d["tof"])
    od = xd if inplace else L.m("out", np.zeros_like(d["x"]), writes=True)
    hip.batchnorm_test_propagate(xd, sc, of, od, hip.stream())
    return {"out": host(od)}


def _run_bn_test_backprop(hip, L, d, inplace=False):
    dzd, sc = L.m("out_deriv", d["dz"], writes=inplace), L.v("scale", d["tsc"])
    dxd = dzd if inplace else L.m("in_deriv", np.zeros_like(d["x"]), writes=True)
    hip.batchnorm_test_backprop(dzd, sc, dxd, hip.stream())
    return {"in_deriv": host(dxd)}


@pytest.mark.parametrize("w", WIDTHS, ids=WIDS)
def test_batchnorm(hip, w):
    d = _bn_data(w)
    sweep(hip, "batchnorm_propagate", _run_bn_propagate, d, {"memo": (d["stats64"], "close", 2e-5, 1e-6), "out": (d["z64"], "rel", TOL)},
          bitwise=False)
    sweep(hip, "batchnorm_backprop", _run_bn_backprop, d, {"in_deriv": (d["dx64"], "rel", 5e-5)}, bitwise=False)
    x, dz = d["x"].astype(D64), d["dz"].astype(D64)
    sweep(hip, "batchnorm_test_propagate", _run_bn_test_propagate, d, {"out": (x * d["tsc"] + d["tof"], "rel", 1e-4)}, bitwise=True)
    sweep(hip, "batchnorm_test_backprop", _run_bn_test_backprop, d, {"in_deriv": (dz * d["tsc"], "rel", 1e-4)}, bitwise=True)


# ------------------------------------------------------------------------------------------------------ ReLU, scaled sums, dropout
def _ew_data(w):
    rng = np.random.default_rng(400 + w)
    d = dict(w=w, x=_rand(rng, N, w), dy=_rand(rng, N, w), a=_rand(rng, N, w), b=_rand(rng, N, w))
    d["x"][::7, ::5] = 0.0   # exact zeros: the boundary of both ReLU passes
    d["mask"] = (1 + 0.2 * _rand(rng, 9, w)).astype(F)
    d["repair_stats"] = np.concatenate([[100.0], np.zeros(w), rng.choice([0.0, 50.0, 100.0], w)])   # trips both thresholds
    return d


def _run_relu_propagate(hip, L, d, inplace=False):
    xd = L.m("in", d["x"], writes=inplace)
    od = xd if inplace else L.m("out", np.full_like(d["x"], 3.0), writes=True)
    hip.relu_propagate(xd, od, hip.stream())
    return {"out": host(od)}


def _run_relu_backprop(hip, L, d, inplace=False):
    vd, dyd = L.m("out_value", np.maximum(d["x"], 0)), L.m("out_deriv", d["dy"], writes=inplace)
    dxd = dyd if inplace else L.m("in_deriv", np.full_like(d["x"], 3.0), writes=True)
    hip.relu_backprop(vd, dyd, dxd, hip.stream())
    return {"in_deriv": host(dxd)}


def _run_relu_store_stats(hip, L, d):
    vd = L.m("out_value", np.maximum(d["x"], 0))
    stats = torch.zeros(1 + 2 * d["w"], dtype=torch.float64, device="cuda")
    nb = hip.colreduce_workspace_bytes(N, d["w"])
    ws = hip.ws(nb)
    hip.relu_store_stats(vd, hip.vec(stats), hip.vec(ws), nb, hip.stream())
    st = host(stats)
    return {"count": st[:1], "value_sum": st[1:1 + d["w"]], "deriv_sum": st[1 + d["w"]:]}


def _run_relu_repair(hip, L, d):
    dd = L.m("in_deriv", d["dy"], writes=True)
    stats = torch.from_numpy(d["repair_stats"]).cuda()
    hip.relu_repair(hip.vec(stats), d["w"], 1e-5, 0.05, 0.95, dd, hip.stream())
    return {"in_deriv": host(dd)}


def _run_sum_scaled(hip, L, d):
    ad, bd = L.m("a", d["a"]), L.m("b", d["b"])
    od = L.m("out", np.full_like(d["a"], 3.0), writes=True)
    hip.sum_scaled(ad, 0.66, bd, 1.0, od, hip.stream())
    o2 = L.m("out", np.full_like(d["a"], 3.0), writes=True)
    hip.sum_scaled(ad, 0.66, None, 0.0, o2, hip.stream())
    return {"sum": host(od), "scaled": host(o2)}


def _run_add_scaled(hip, L, d):
    ad, od = L.m("a", d["a"]), L.m("out", d["b"], writes=True)
    hip.add_scaled(ad, 2.0, od, hip.stream())
    return {"out": host(od)}


def _run_dropout(hip, L, d, inplace=False):
    xd, md = L.m("in", d["x"], writes=inplace), L.v("mask", d["mask"])
    od = xd if inplace else L.m("out", np.full_like(d["x"], 3.0), writes=True)
    hip.general_dropout(xd, md, 9, od, hip.stream())
    return {"out": host(od)}


@pytest.mark.parametrize("w", WIDTHS, ids=WIDS)
def test_relu(hip, w):
    d = _ew_data(w)
    x, dy = d["x"], d["dy"]
    sweep(hip, "relu_propagate", _run_relu_propagate, d, {"out": (np.maximum(x, 0), "exact")}, bitwise=True)
    sweep(hip, "relu_backprop", _run_relu_backprop, d, {"in_deriv": ((x > 0) * dy, "exact")}, bitwise=True)
    ref = {"count": ([float(N)], "exact"), "deriv_sum": ((x > 0).sum(0).astype(D64), "exact"),
           "value_sum": (np.maximum(x, 0).astype(D64).sum(0), "close", 1e-5, 0.0)}
    sweep(hip, "relu_store_stats", _run_relu_store_stats, d, ref, bitwise=False)
    # RepairGradients (nnet-simple-component.cc:1028-1073): +-scale / 0.5 on the columns outside the thresholds
    st = d["repair_stats"][1 + w:]
    v = ((st > 0.05 * 100.0).astype(D64) + (st > 0.95 * 100.0).astype(D64) - 1.0) * (-1e-5 / 0.5)
    sweep(hip, "relu_repair", _run_relu_repair, d, {"in_deriv": (dy.astype(D64) + v, "close", 1e-6, 1e-9)}, bitwise=True)


@pytest.mark.parametrize("w", WIDTHS, ids=WIDS)
def test_scaled_sums_and_dropout(hip, w):
    d = _ew_data(w)
    a, b, x = d["a"].astype(D64), d["b"].astype(D64), d["x"].astype(D64)
    s = float(F(0.66))
    sweep(hip, "sum_scaled", _run_sum_scaled, d, {"sum": (s * a + b, "close", 1e-6, 1e-6), "scaled": (s * a, "close", 1e-6, 1e-6)},
          bitwise=True)
    sweep(hip, "add_scaled", _run_add_scaled, d, {"out": (b + 2.0 * a, "close", 1e-5, 1e-6)}, bitwise=True)
    want = x * np.tile(d["mask"].astype(D64), (N // 9, 1))   # row r uses mask row r % num_seq
    sweep(hip, "general_dropout", _run_dropout, d, {"out": (want, "close", 1e-6, 0.0)}, bitwise=True)


def test_sum_scaled_rounds_alike_on_the_vector_and_the_scalar_path(hip):
    """Regression: sa * a + sb * b was left to the compiler, which contracted it to fma(sa, a, sb * b) in the 16-byte body and not at
    all in the scalar one, so a Sum(Scale(..), ..) on an odd-stride view differed in the last bit from the same sum on a dense matrix."""
    d = _ew_data(260)
    a, b = d["a"].astype(D64), d["b"].astype(D64)
    ref = {"sum": (float(F(0.66)) * a + b, "close", 1e-6, 1e-6), "scaled": (float(F(0.66)) * a, "close", 1e-6, 1e-6)}
    sweep(hip, "sum_scaled", _run_sum_scaled, d, ref, bitwise=True, layouts=("dense", "odd-stride"))


# ------------------------------------------------------------------------------------------------------ log-softmax
# (rows, cols): at most 2048 columns -> the one-pass kernel with 2 float4 per thread; 6034 -> 8 per thread; above 8192 -> one block
# per row in three passes, which every misaligned view takes as well
# The last three sit ON the boundaries of that choice: 2048 is the last width 2 float4 per thread hold (every lane full), 2052 the first that
# needs 8 (sent to 2, its last float4 would be dropped), 8192 the last that 8 hold (8196 above is the first of the three-pass kernel).
LSM_SHAPES = [(5, 8196), (17, 6034), (N, 261), (3, 2048), (3, 2052), (2, 8192)]


def _run_log_softmax(hip, L, d):
    zd, od = L.m("in", d["z"]), L.m("out", np.full_like(d["z"], 3.0), writes=True)
    hip.log_softmax_propagate(zd, od, hip.stream())
    return {"out": host(od)}


def _run_log_softmax_backprop(hip, L, d):
    yd, ed = L.m("out_value", d["y"]), L.m("out_deriv", d["e"])
    dd = L.m("in_deriv", np.full_like(d["z"], 3.0), writes=True)
    hip.log_softmax_backprop(yd, ed, dd, hip.stream())
    return {"in_deriv": host(dd)}


@pytest.mark.parametrize("shape", LSM_SHAPES, ids=WIDS + ["nv2-last", "nv8-first", "nv8-last"])
def test_log_softmax(hip, shape):
    rng = np.random.default_rng(shape[1])
    z = (_rand(rng, *shape) * 3).astype(F)
    z64 = z.astype(D64)
    mx = z64.max(1, keepdims=True)
    y64 = z64 - (mx + np.log(np.exp(z64 - mx).sum(1, keepdims=True)))
    y, e = y64.astype(F), _rand(rng, *shape)
    d = dict(z=z, y=y, e=e)
    sweep(hip, "log_softmax_propagate", _run_log_softmax, d, {"out": (y64, "close", 1e-5, 1e-5)}, bitwise=False)
    want = e.astype(D64) - np.exp(y.astype(D64)) * e.astype(D64).sum(1, keepdims=True)
    sweep(hip, "log_softmax_backprop", _run_log_softmax_backprop, d, {"in_deriv": (want, "close", 1e-4, 1e-5)}, bitwise=False)


# ------------------------------------------------------------------------------------------------------ DARTS mixing ops
def _run_copyn_propagate(hip, L, d):
    ad, od = L.m("in", d["a"]), L.m("out", d["o0"], writes=True)
    hip.copyn_propagate(ad, 1.5, od, hip.stream())
    return {"out": host(od)}


def _run_copyn_backprop(hip, L, d):
    dod, dad = L.m("out_deriv", d["do"]), L.m("in_deriv", d["a"], writes=True)
    hip.copyn_backprop(dod, 1.5, dad, hip.stream())
    return {"in_deriv": host(dad)}


def _copyn_refs(d):
    nb = d["o0"].shape[1] // d["a"].shape[1]
    fwd = d["o0"].astype(D64) + 1.5 * np.tile(d["a"].astype(D64), (1, nb))   # AddMatBlocks: both directions add
    bwd = d["a"].astype(D64) + 1.5 * d["do"].astype(D64).reshape(N, nb, -1).sum(1)
    return {"out": (fwd, "close", 1e-6, 1e-6)}, {"in_deriv": (bwd, "close", 1e-5, 1e-6)}


# (at most 40 blocks per row, the 1 -> 40 of tests/test_gpu_parity.py whose bounds these are: the backward pass adds a row's blocks in float)
@pytest.mark.parametrize("din,dout", [(13, 260), (131, 262), (9, 261), (1, 37)], ids=["w4", "w2", "odd", "1-to-37"])
def test_copyn(hip, din, dout):
    rng = np.random.default_rng(din + dout)
    d = dict(a=_rand(rng, N, din), o0=_rand(rng, N, dout), do=_rand(rng, N, dout))
    fwd, bwd = _copyn_refs(d)
    sweep(hip, "copyn_propagate", _run_copyn_propagate, d, fwd, bitwise=True)
    sweep(hip, "copyn_backprop", _run_copyn_backprop, d, bwd, bitwise=True)


def _ranged(hip, name, run, d, ref, placing):
    """One run with the named operands as column ranges of wider parents ({operand: ("range", parent_cols, first_col)}), bit-identical
    to the dense run for these per-element maps."""
    dense = Lay("dense")
    base = run(hip, dense, d)

    class Ranges(Lay):
        def m(self, op, a, writes=False):
            return self._keep(op, laid_out(a, placing.get(op, "dense"), writes=writes))

    L = Ranges()
    got = run(hip, L, d)
    L.check(name)
    _compare(got, ref, name)
    assert all(np.array_equal(got[k], base[k]) for k in base), name + ": not bit-identical to the dense run"


# the reference's own views (local/chain_NAS/scripts/generate_bottleneckCB8share_onehottrain_config.py:13-20, :52-59): X.softmax cut into
# eight 1-column dim-range-nodes of its 8 columns, X.linear cut into ranges of widths 25, 25, 30, ... at column offsets 0, 25, 50, ...
@pytest.mark.parametrize("k,first,width", [(k, 25, 25) for k in range(8)] + [(3, 50, 30)])
def test_copyn_on_the_recipes_dim_ranges(hip, k, first, width):
    rng = np.random.default_rng(k)
    d = dict(a=_rand(rng, N, 1), o0=_rand(rng, N, width), do=_rand(rng, N, width))
    fwd, bwd = _copyn_refs(d)
    placing = {"in": ("range", 8, k), "in_deriv": ("range", 8, k), "out": ("range", 240, first), "out_deriv": ("range", 240, first)}
    _ranged(hip, "copyn_propagate softmax[%d] -> linear[%d:%d]" % (k, first, first + width), _run_copyn_propagate, d, fwd, placing)
    _ranged(hip, "copyn_backprop softmax[%d] <- linear[%d:%d]" % (k, first, first + width), _run_copyn_backprop, d, bwd, placing)


def _run_ewprod_propagate(hip, L, d):
    xd, yd = L.m("in", d["x"]), L.m("out", np.full((N, d["od"]), 3.0, F), writes=True)
    hip.elementwise_product_propagate(xd, d["od"], yd, hip.stream())
    return {"out": host(yd)}


def _run_ewprod_backprop(hip, L, d):
    xd, dyd = L.m("in_value", d["x"]), L.m("out_deriv", d["dy"])
    dxd = L.m("in_deriv", np.full_like(d["x"], 3.0), writes=True)
    hip.elementwise_product_backprop(xd, dyd, d["od"], dxd, hip.stream())
    return {"in_deriv": host(dxd)}


def _ewprod(od):
    rng = np.random.default_rng(500 + od)
    d = dict(od=od, x=_rand(rng, N, 2 * od), dy=_rand(rng, N, od))
    x, dy = d["x"].astype(D64), d["dy"].astype(D64)
    fwd = {"out": (x[:, :od] * x[:, od:], "close", 1e-6, 0.0)}
    bwd = {"in_deriv": (np.concatenate([dy * x[:, od:], dy * x[:, :od]], axis=1), "close", 1e-6, 0.0)}
    return d, fwd, bwd


@pytest.mark.parametrize("od", [132, 130, 131], ids=WIDS)   # (the input is twice as wide: 264 / 260 / 262)
def test_elementwise_product(hip, od):
    d, fwd, bwd = _ewprod(od)
    sweep(hip, "elementwise_product_propagate", _run_ewprod_propagate, d, fwd, bitwise=True)
    sweep(hip, "elementwise_product_backprop", _run_ewprod_backprop, d, bwd, bitwise=True)


@pytest.mark.parametrize("first,width", [(25, 25), (50, 30)])
def test_elementwise_product_on_the_recipes_dim_ranges(hip, first, width):
    d, fwd, bwd = _ewprod(width)
    placing = {"out": ("range", 240, first), "out_deriv": ("range", 240, first)}
    _ranged(hip, "elementwise_product_propagate -> [%d:%d]" % (first, first + width), _run_ewprod_propagate, d, fwd, placing)
    _ranged(hip, "elementwise_product_backprop <- [%d:%d]" % (first, first + width), _run_ewprod_backprop, d, bwd, placing)


FLOPS8 = -np.asarray([25, 50, 80, 100, 120, 160, 200, 240], F)


def _run_softmax_flops_propagate(hip, L, d):
    xd, pd = L.m("in", d["x"]), L.m("out", np.full_like(d["x"], 3.0), writes=True)
    ud = L.v("gumbel_u", d["u"]) if d["u"] is not None else None
    hip.softmax_flops_propagate(xd, ud, d["tau"], pd, hip.stream())
    return {"out": host(pd)}


def _run_softmax_flops_backprop(hip, L, d, inplace=False):
    pd, dpd = L.m("out_value", d["p"]), L.m("out_deriv", d["dp"], writes=True)
    dxd = dpd if inplace else L.m("in_deriv", np.full_like(d["x"], 3.0), writes=True)
    fd = L.v("flops", d["flops"]) if d["flops"] is not None else None
    hip.softmax_flops_backprop(pd, dpd, 0.3, fd, d["dim"], d["tau"], dxd, hip.stream())
    return {"in_deriv": host(dxd)} if inplace else {"in_deriv": host(dxd), "out_deriv": host(dpd)}


def _softmax_flops_data(cols, gumbel, flops):
    rng = np.random.default_rng(600 + cols + gumbel)
    tau = 0.6 if gumbel else 1.0
    x = _rand(rng, N, cols)
    u = rng.uniform(0.05, 0.95, cols).astype(F) if gumbel else None
    v = x.astype(D64) if not gumbel else (x.astype(D64) - np.log(-np.log(u.astype(D64)))) / tau
    p64 = np.exp(v - v.max(1, keepdims=True))
    p64 = np.maximum(p64 / p64.sum(1, keepdims=True), 1e-20)
    p, dp = p64.astype(F), _rand(rng, N, cols)
    dim = cols if flops else 0
    e = dp.astype(D64)
    if flops:   # out_deriv[:, :dim] += scale / (rows * cols) * flops, in place as the reference does
        e = e + 0.3 / N / cols * FLOPS8[:cols].astype(D64)
    pd = p.astype(D64)
    dx = pd * (e - (pd * e).sum(1, keepdims=True)) / tau
    return dict(x=x, u=u, tau=tau, p=p, dp=dp, dim=dim, flops=FLOPS8[:cols].copy() if flops else None), p64, e, dx


@pytest.mark.parametrize("gumbel", [False, True], ids=["softmax", "gumbel"])
@pytest.mark.parametrize("cols", [8, 6, 5], ids=WIDS)
def test_softmax_flops(hip, cols, gumbel):
    d, p64, e, dx = _softmax_flops_data(cols, gumbel, True)
    sweep(hip, "softmax_flops_propagate", _run_softmax_flops_propagate, d, {"out": (p64, "close", 2e-5, 1e-20)}, bitwise=False)
    # (e_c - <p, e> cancels for some elements: the bound is absolute there, as in test_plain_gumbel_softmax_without_flops_vector)
    # out_deriv + a flops cancels for a few elements: the 1e-6 of test_softmax_flops (there against the same float sum) is taken of the
    # larger addend where it is the penalty, since a float sum is only that accurate against the exact one
    pen = 1e-6 * float(np.abs(0.3 / N / cols * FLOPS8[:cols].astype(D64)).max())
    ref = {"out_deriv": (e, "close", 1e-6, pen), "in_deriv": (dx, "close", 2e-4, 2e-6)}
    sweep(hip, "softmax_flops_backprop", _run_softmax_flops_backprop, d, ref, bitwise=False)
    d, p64, e, dx = _softmax_flops_data(cols, gumbel, False)   # no flops vector: out_deriv is left alone
    ref = {"out_deriv": (d["dp"], "exact"), "in_deriv": (dx, "close", 2e-4, 2e-6)}
    sweep(hip, "softmax_flops_backprop (no flops)", _run_softmax_flops_backprop, d, ref, bitwise=False)


def _run_onehot_propagate(hip, L, d):
    ud, od = L.v("sample_u", np.asarray([d["u"]], F)), L.m("out", np.full((N, d["cols"]), 3.0, F), writes=True)
    hip.onehot_propagate(ud, od, hip.stream())
    return {"out": host(od)}


def _run_colsum(entry, lr):
    def run(hip, L, d):
        dd, acc = L.m("out_deriv", d["dy"]), L.v("output_acc", d["acc0"], writes=True)
        nb = hip.colreduce_workspace_bytes(N, d["dy"].shape[1])
        ws = hip.ws(nb)
        getattr(hip, entry)(dd, lr, acc, hip.vec(ws), nb, hip.stream())
        return {"acc": host(acc)}
    return run


def _run_constant_propagate(hip, L, d):
    ad, od = L.v("output", d["acc0"]), L.m("out", np.full_like(d["dy"], 3.0), writes=True)
    hip.constant_function_propagate(ad, od, hip.stream())
    return {"out": host(od)}


def _run_flops_constraint(hip, L, d):
    fd, od = L.v("flops", d["acc0"]), L.m("in_deriv", np.full_like(d["dy"], 3.0), writes=True)
    hip.flops_constraint_backprop(fd, 0.2, N, d["dy"].shape[1], od, hip.stream())
    return {"in_deriv": host(od)}


@pytest.mark.parametrize("cols", [8, 6, 5] + list(WIDTHS), ids=["c8", "c6", "c5"] + WIDS)
def test_onehot_constant_flops_constraint(hip, cols):
    rng = np.random.default_rng(700 + cols)
    d = dict(cols=cols, dy=_rand(rng, N, cols), acc0=_rand(rng, cols))
    for u in (0.0, 0.124, 0.125, 0.5, 0.999):   # OnehotFunctionComponent::Propagate :9504-9519: column c is 1 where c / C <= u < (c + 1) / C
        d["u"] = u
        c = np.arange(cols)
        lo, hi = c.astype(F) / F(cols), (c + 1).astype(F) / F(cols)   # float divisions, as the component does them
        want = np.tile(((F(u) >= lo) & (F(u) < hi)).astype(F), (N, 1))
        sweep(hip, "onehot_propagate u=%g" % u, _run_onehot_propagate, d, {"out": (want, "exact")}, bitwise=True, layouts=LAYOUTS if u == 0.5 else LAYOUTS[:1])
    s = d["dy"].astype(D64).sum(0)
    sweep(hip, "onehot_backprop", _run_colsum("onehot_backprop", 0.25), d, {"acc": (d["acc0"] + 0.25 * s, "rel", 2e-6)}, bitwise=False)
    sweep(hip, "constant_function_backprop", _run_colsum("constant_function_backprop", 0.1), d,
          {"acc": (d["acc0"] + 5 * 0.1 * s, "close", 1e-4, 1e-5)}, bitwise=False)   # :2636: output += 5 lr colsum
    sweep(hip, "constant_function_propagate", _run_constant_propagate, d, {"out": (np.tile(d["acc0"], (N, 1)), "exact")}, bitwise=True)
    want = np.tile(0.2 / N / cols * d["acc0"].astype(D64), (N, 1))
    sweep(hip, "flops_constraint_backprop", _run_flops_constraint, d, {"in_deriv": (want, "close", 1e-6, 0.0)}, bitwise=True)


# ------------------------------------------------------------------------------------------------------ row plumbing
def _run_splice(hip, L, d):
    fd, iv = L.m("feats", d["feats"]), L.m("ivectors", d["iv"])
    od = L.m("out", np.full((d["T"] * 9, 3 * d["fd"] + d["ivd"]), 3.0, F), writes=True)
    hip.splice_input(fd, iv, 9, 3, od, hip.stream())
    return {"out": host(od)}


@pytest.mark.parametrize("fd,ivd", [(40, 100), (42, 12), (43, 6)], ids=WIDS)   # out: 220 / 138 / 135 columns from blocks of 40 / 42 / 43
def test_splice_input(hip, fd, ivd):
    rng = np.random.default_rng(fd)
    T = 29
    d = dict(T=T, fd=fd, ivd=ivd, feats=_rand(rng, (T + 2) * 9, fd), iv=_rand(rng, 9, ivd))
    f3 = d["feats"].reshape(T + 2, 9, fd)
    want = np.concatenate([f3[0:T], f3[1:T + 1], f3[2:T + 2], np.broadcast_to(d["iv"], (T, 9, ivd))], axis=2).reshape(T * 9, -1)
    sweep(hip, "splice_input", _run_splice, d, {"out": (want, "exact")}, bitwise=True)


def _run_reorder(to_rho):
    def run(hip, L, d):
        xd, od = L.m("in", d["x"]), L.m("out", np.full_like(d["x"], 3.0), writes=True)
        hip.reorder_rows(xd, 9, 3, to_rho, od, hip.stream())
        return {"out": host(od)}
    return run


@pytest.mark.parametrize("w", WIDTHS, ids=WIDS)
def test_reorder_rows(hip, w):
    rows = 270   # a multiple of num_seq * rho = 27
    x = _rand(np.random.default_rng(w), rows, w)
    tau, b = np.divmod(np.arange(rows), 9)
    perm = (tau // 3) * 27 + b * 3 + tau % 3   # nnet-tdnn-component.cc:897-902: where t-major row tau * B + b goes
    fwd = np.zeros_like(x)
    fwd[perm] = x
    sweep(hip, "reorder_rows to rho order", _run_reorder(1), dict(x=x), {"out": (fwd, "exact")}, bitwise=True)
    sweep(hip, "reorder_rows from rho order", _run_reorder(0), dict(x=x), {"out": (x[perm], "exact")}, bitwise=True)


# ------------------------------------------------------------------------------------------------------ alpha update, orthonormal constraint
def _run_alpha_update(hip, L, d):
    Gd, Wd, cd = L.m("tap_grad", d["G"]), L.m("W", d["W"]), L.v("coef_memo", d["coef"])
    acc = L.v("alpha_acc", d["acc0"], writes=True)
    dots = torch.zeros(3 * 65, dtype=torch.float64, device="cuda")   # TDNNF_TAP_DOTS_DOUBLES(K)
    hip.tdnn_darts_alpha_update(hip.vec(Gd), Gd.stride(0), hip.vec(Wd), Wd.stride(0), 20, d["Di"], 3, cd, 0, 2, 0.7, 0.01, acc, hip.vec(dots),
                                hip.stream())
    return {"dots": host(dots)[:3], "acc": host(acc)}


@pytest.mark.parametrize("Di", [24, 26, 25], ids=WIDS)
def test_tdnn_darts_alpha_update(hip, Di):
    rng = np.random.default_rng(Di)
    K, Do, share, lr = 3, 20, 2, 0.01
    d = dict(Di=Di, G=_rand(rng, Do, K * Di), W=_rand(rng, Do, K * Di), coef=np.asarray([0.2, 0.5, 0.3], F), acc0=_rand(rng, K))
    s = (d["G"].astype(D64) * d["W"].astype(D64)).reshape(Do, K, Di).sum((0, 2))   # s_i = <dW_i, W_i>
    coef, acc = d["coef"].astype(D64), d["acc0"].astype(D64).copy()
    for i in range(K):   # the softmax branch of UpdateNaturalGradient, nnet-tdnn-component.cc:540-560, then the scaling by 5 lr (:565-590)
        if i != share:
            acc += -s[i] * coef[i] * coef
            acc[i] += s[i] * coef[i]
    acc *= 5.0 * lr
    sweep(hip, "tdnn_darts_alpha_update", _run_alpha_update, d, {"dots": (s, "close", 1e-4, 0.0), "acc": (acc, "close", 2e-4, 1e-6)}, bitwise=False)


def _run_orthonormal(hip, L, d):
    Md = L.m("M", d["M"], writes=True)
    rows, cols = d["M"].shape
    nb = hip.constrain_orthonormal_workspace_bytes(rows, cols)
    ws = hip.ws(nb)
    for _ in range(3):
        hip.constrain_orthonormal(d["scale"], hip.vec(Md), rows, cols, Md.stride(0), hip.vec(ws), nb, hip.stream())
    return {"M": host(Md)}


def _orthonormal64(M, scale):
    """ConstrainOrthonormalInternal (nnet-utils.cc:914-1032) in float64"""
    rows = M.shape[0]
    P = M @ M.T
    speed = 0.125
    if scale < 0:
        tp, tpp = np.trace(P), (P * P).sum()
        scale = np.sqrt(tpp / tp)
        ratio = tpp * rows / (tp * tp)
        if ratio > 1.02:
            speed *= 0.5
            if ratio > 1.1:
                speed *= 0.5
    P = P - scale * scale * np.eye(rows)
    return M - 4.0 * (speed / (scale * scale)) * P @ M


@pytest.mark.parametrize("scale", [-1.0, 1.0], ids=["floating-scale", "scale-1"])
@pytest.mark.parametrize("cols", [52, 54, 53], ids=WIDS)
def test_constrain_orthonormal(hip, cols, scale):
    rng = np.random.default_rng(cols)
    M = (_rand(rng, 24, cols) / np.sqrt(cols)).astype(F)
    want = M.astype(D64)
    for _ in range(3):
        want = _orthonormal64(want, scale)
    sweep(hip, "constrain_orthonormal", _run_orthonormal, dict(M=M, scale=scale), {"M": (want, "rel", 1e-5)}, bitwise=False)


# ------------------------------------------------------------------------------------------------------ in place
# The classes that advertise kPropagateInPlace / kBackpropInPlace in include/tdnnf_nnet3_components.h, on views: the same kernel on the
# same inputs, so the result equals the out-of-place result of the same call bit for bit.
def _softmax_flops_inplace_data(flops):
    return _softmax_flops_data(8, True, flops)[0]


INPLACE = [
    ("batchnorm_backprop", _run_bn_backprop, lambda: _bn_data(261), "in_deriv"),
    ("batchnorm_test_propagate", _run_bn_test_propagate, lambda: _bn_data(262), "out"),
    ("batchnorm_test_backprop", _run_bn_test_backprop, lambda: _bn_data(260), "in_deriv"),
    ("relu_propagate", _run_relu_propagate, lambda: _ew_data(260), "out"),
    ("relu_backprop", _run_relu_backprop, lambda: _ew_data(262), "in_deriv"),
    ("general_dropout", _run_dropout, lambda: _ew_data(261), "out"),
    ("softmax_flops_backprop-flops", _run_softmax_flops_backprop, lambda: _softmax_flops_inplace_data(True), "in_deriv"),
    ("softmax_flops_backprop-noflops", _run_softmax_flops_backprop, lambda: _softmax_flops_inplace_data(False), "in_deriv"),
]


@pytest.mark.parametrize("layout", ["pitched", "off1-odd"])
@pytest.mark.parametrize("entry", INPLACE, ids=[e[0] for e in INPLACE])
def test_in_place(hip, entry, layout):
    name, run, make, key = entry
    d = make()
    L = Lay(layout)
    want = run(hip, L, d)[key]
    L.check(name)
    L = Lay(layout)
    got = run(hip, L, d, inplace=True)[key]
    L.check(name + " in place")
    assert np.isfinite(want).all() and np.array_equal(got, want), "%s in place on %s views differs from the out-of-place call" % (name, layout)
