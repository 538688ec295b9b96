"""Pins the float64 restatement of the optimizer step (tests/update_ref64.py) without a GPU: against OracleNet.update (the float32
C oracle: oracle_max_change_scales, oracle_constrain_orthonormal) over schedules with and without clipping, and by facts that need
no oracle.  tests/test_gpu_net_update.py holds the kernels to this restatement."""
import numpy as np
import pytest

from tests import update_ref64 as R
from tests.oracle_net import OracleNet, component_table, decision
from tests.test_gpu_net import CASES as NET_CASES
from tests.test_gpu_net_update import NETS, U24, _clip_norms, check_edges, random_grads

LR = 0.05


def _table(pkg, kw):
    cfg = pkg.trainer.make_config(**kw)
    comps, num_params = component_table(cfg)
    return cfg, comps, num_params


def _init(comps, num_params, seed):
    rng = np.random.default_rng(seed)
    p = np.zeros(num_params, np.float32)
    for c in comps:
        n = c["rows"] * c["cols"]
        p[c["begin"]:c["begin"] + n] = (rng.standard_normal(n) / np.sqrt(c["cols"])).astype(np.float32)
        if c["has_bias"]:
            p[c["begin"] + n + c["num_alpha"]:c["begin"] + R.owned(c)] = rng.standard_normal(c["rows"]).astype(np.float32) * 0.3
    return p


@pytest.mark.parametrize("regime", ["unclipped", "one-component", "component-and-global", "global-only"])
@pytest.mark.parametrize("case", ["tiny", "ragged-dims"])
def test_restatement_against_the_float32_oracle(pkg, case, regime):
    """8 steps of OracleNet.update (float32 numpy + the C oracle) and of update_ref64 from the same float32 parameters: the oracle
    is one float32 evaluation of the formula, so it is held to the bar test_gpu_net_update.py derives for such an evaluation
    (2^-24 |p'| + 8 * 2^-24 |f d| per element); a stepped matrix to rel_l2 1e-5 and its change to 64 * 2^-24 x max(1, |P| / |Q|),
    Q = P - s^2 I: the oracle rounds P and s to float32, an error of 2^-24 |P| in Q that the product with M carries into X."""
    cfg, comps, num_params = _table(pkg, next(c[1] for c in NET_CASES if c[0] == case))
    net = OracleNet(pkg, cfg, comps)
    l2s = float(cfg.num_sequences)
    params = _init(comps, num_params, 1)  # (a seed with no stepped matrix within 1e-3 of a ratio threshold: asserted below)
    rngs = R.ranges(comps, num_params)
    stepped_total = clipped = 0
    for step in range(8):
        rng = np.random.default_rng(100 + step)
        if regime == "unclipped":
            norms = [c["max_change"] * 10.0 ** -rng.uniform(0.5, 2.5) if c["max_change"] else None for c in comps]
            grads = random_grads(comps, num_params, 200 + step, norms, params, lr=LR, l2_scale=0.0)
        else:
            grads = random_grads(comps, num_params, 200 + step, _clip_norms(comps, regime), params, lr=LR, l2_scale=l2s)
        ref = R.update_ref64(comps, params, grads, LR, l2s, cfg.max_param_change, step)
        dn = np.sqrt(ref["dot"])
        assert all(abs(dn[i] / c["max_change"] - 1) >= 0.01 for i, c in enumerate(comps) if c["max_change"] and c["lr_factor"])
        assert abs(ref["param_delta"] / cfg.max_param_change - 1) >= 0.01
        over, glob = bool((ref["factor"] < 1).any()), ref["scale"] < 1
        assert (over, glob) == {"unclipped": (False, False), "one-component": (True, False), "component-and-global": (True, True),
                                "global-only": (False, True)}[regime]
        clipped += int(over or glob)
        assert set(ref["stepped"]) == {i for i, c in enumerate(comps) if c["orthonormal"] != 0.0 and decision(step, 2 * i + 1) % 4 == 0}
        p_o = net.update(params, grads, LR, l2s, step)
        bar = R.element_bar(ref, comps, num_params)
        err = np.abs(p_o.astype(np.float64) - ref["params"])
        for i, (c, (b, e)) in enumerate(zip(comps, rngs)):
            if i not in ref["stepped"]:
                assert (err[b:e] <= bar[b:e]).all(), (c["name"], step, float((err[b:e] / np.maximum(bar[b:e], 1e-300)).max()))
                continue
            s = ref["stepped"][i]
            n = c["rows"] * c["cols"]
            Mo = p_o[b:b + n].astype(np.float64).reshape(c["rows"], c["cols"])
            assert np.linalg.norm(Mo - s["M_new"]) < 1e-5 * np.linalg.norm(s["M_new"])
            assert abs(s["ratio"] / 1.02 - 1) > 1e-3 and abs(s["ratio"] / 1.1 - 1) > 1e-3, (c["name"], step, s["ratio"])
            W = s["M"] if c["rows"] <= c["cols"] else s["M"].T
            P = W @ W.T
            Q = P - s["scale"] ** 2 * np.eye(P.shape[0])
            xbar = 64 * U24 * max(1.0, np.linalg.norm(P) / np.linalg.norm(Q))
            e_x = np.linalg.norm((Mo - s["M"]) - s["X"]) / np.linalg.norm(s["X"])
            assert e_x <= xbar, (c["name"], step, e_x, xbar)
            assert (err[b + n:e] <= bar[b + n:e]).all()
            stepped_total += 1
        params = p_o
    assert stepped_total >= 6 and (clipped == 8) == (regime != "unclipped")


@pytest.mark.parametrize("rows,cols", [(6, 100), (10, 100), (16, 96), (48, 72), (64, 160), (136, 320)])
def test_matrix_with_ratio_delivers_its_ratio(rows, cols):
    for k, ratio in enumerate([1.0, 1.01, 1.05, 1.5]):
        M = R.matrix_with_ratio(rows, cols, ratio, seed=10 * rows + k)
        assert M.shape == (rows, cols) and abs(R.ratio64(M) - ratio) <= 1e-9, (ratio, R.ratio64(M))
        s = R.constrain_orthonormal64(M.astype(np.float32))
        assert s["update_speed"] == {1.0: 0.125, 1.01: 0.125, 1.05: 0.0625, 1.5: 0.03125}[ratio]
    assert abs(R.ratio64(R.matrix_with_ratio(rows, cols, 1.5, seed=1).T) - 1.5) <= 1e-9  # (a tall matrix: the ratio of its transpose)


@pytest.mark.parametrize("s0", [0.7, 1.0, 3.5])
def test_orthonormal_rows_times_any_scale_are_a_fixed_point(s0):
    M = R.matrix_with_ratio(14, 50, 1.0, seed=2, s0=s0)
    assert np.abs(M @ M.T - s0 * s0 * np.eye(14)).max() < 1e-13 * s0 * s0
    r = R.constrain_orthonormal64(M, exact=True)
    assert np.linalg.norm(r["X"]) <= 1e-12 * np.linalg.norm(M) and abs(r["scale"] - s0) < 1e-12 * s0
    # with the reference's float32 scale the step is the rounding of s^2, nothing more
    assert np.linalg.norm(R.constrain_orthonormal64(M)["X"]) <= 4 * U24 * np.linalg.norm(M)


@pytest.mark.parametrize("ratio", [1.01, 1.05, 1.5, None])
def test_floating_scale_makes_the_change_orthogonal_to_the_matrix(ratio):
    M = R.matrix_with_ratio(10, 100, ratio, seed=3) if ratio else np.random.default_rng(4).standard_normal((10, 100)) / 10.0
    r = R.constrain_orthonormal64(M, exact=True)
    assert np.linalg.norm(r["X"]) > 1e-3 * np.linalg.norm(M)
    assert abs(np.trace(M @ r["X"].T)) <= 1e-12 * np.linalg.norm(M) * np.linalg.norm(r["X"])
    assert abs(r["scale"] ** 2 - r["trPP"] / r["trP"]) <= 1e-15 * r["scale"] ** 2


def test_tall_matrix_is_stepped_through_its_transpose(pkg):
    cfg, comps, num_params = _table(pkg, NETS["tall"])
    i = [k for k, c in enumerate(comps) if c["name"] == "tdnnf3.linear"][0]
    c = comps[i]
    assert c["rows"] > c["cols"]
    params = _init(comps, num_params, 5)
    step = R.steps_selecting(comps, {i})
    ref = R.update_ref64(comps, params, np.zeros_like(params), 0.0, 2.0, 2.0, step)
    W = params[c["begin"]:c["begin"] + c["rows"] * c["cols"]].astype(np.float64).reshape(c["rows"], c["cols"])
    t = R.constrain_orthonormal64(W.T, c["orthonormal"])
    assert set(ref["stepped"]) == {i} and np.array_equal(ref["stepped"][i]["M_new"], t["M_new"].T) and np.array_equal(ref["stepped"][i]["X"], t["X"].T)
    n = c["rows"] * c["cols"]
    assert np.array_equal(ref["params"][c["begin"]:c["begin"] + n].reshape(c["rows"], c["cols"]), t["M_new"].T) and t["X"].any()
    other = np.ones(num_params, bool)
    other[c["begin"]:c["begin"] + n] = False
    assert np.array_equal(ref["params"][other], params[other].astype(np.float64))


def test_one_infinite_gradient_element_refuses_the_update(pkg):
    cfg, comps, num_params = _table(pkg, NETS["ragged"])
    params = _init(comps, num_params, 6)
    grads = random_grads(comps, num_params, 7, [0.2 * c["max_change"] if c["max_change"] else None for c in comps], params, l2_scale=5.0)
    step = R.steps_selecting(comps, set())
    assert R.update_ref64(comps, params, grads, LR, 5.0, 2.0, step)["applied"]
    for sign in (np.inf, -np.inf):
        bad = grads.copy()
        mid = comps[len(comps) // 2]
        bad[mid["begin"] + 3] = sign
        ref = R.update_ref64(comps, params, bad, LR, 5.0, 2.0, step)
        assert not ref["applied"] and not ref["total"].any() and np.array_equal(ref["params"], params.astype(np.float64))


def test_steps_selecting_returns_the_first_step_with_exactly_that_schedule(pkg):
    cfg, comps, num_params = _table(pkg, NETS["ragged"])
    cons = R.constrained(comps)
    assert len(cons) == 6 and all(comps[i]["orthonormal"] == -1.0 for i in cons)
    for wanted in [set(), {cons[0]}, {cons[-1]}, {cons[0], cons[-1]}, set(cons[1:4]), set(cons)]:
        step = R.steps_selecting(comps, wanted)
        assert set(R.schedule(comps, step)) == wanted
        assert all(set(R.schedule(comps, s)) != wanted for s in range(step))
    with pytest.raises(LookupError):
        R.steps_selecting(comps, set(cons), limit=R.steps_selecting(comps, set(cons)))


def test_batchnorm_statistics_layout_and_scaling_match_the_oracle(pkg):
    cfg, comps, num_params = _table(pkg, NETS["ragged"])
    net = OracleNet(pkg, cfg, comps)
    blocks, total = R.stat_blocks(cfg)
    assert net.get_stats().size == total and sum(r for r, _, _ in blocks) == cfg.num_layers + 3 and len(blocks) == 2 * cfg.num_layers + 8
    stats = np.random.default_rng(9).uniform(0.5, 100.0, total)
    net.set_stats(stats)
    assert np.array_equal(net.get_stats(), stats)
    params = _init(comps, num_params, 2)
    net.update(params, np.zeros_like(params), LR, 5.0, step=0)
    want = R.scale_batchnorm_stats64(stats, cfg)
    assert np.array_equal(net.get_stats(), want) and not np.array_equal(want, stats)
    for relu, b, e in blocks:
        assert np.array_equal(want[b:e], stats[b:e] if relu else stats[b:e] * float(np.float32(0.8)))
    cfg.batchnorm_stats_scale = 1.0
    assert np.array_equal(R.scale_batchnorm_stats64(stats, cfg), stats)


@pytest.mark.parametrize("name", list(NETS))
def test_the_gpu_tests_nets_reach_their_edges(pkg, name):
    """The component tables of tests/test_gpu_net_update.py's nets, derived without the library: slice counts, tile heights, item
    lengths and which matrices are tall are what that file says they are (the GPU tests assert the same on the library's table)."""
    cfg, comps, num_params = _table(pkg, NETS[name])
    facts = check_edges(name, comps, num_params)
    assert len(R.constrained(comps)) <= 7
    print(name, facts)


def test_slices_and_items_helpers():
    assert R.ggemm_slices(100) == [100] and R.ggemm_slices(128) == [128] and R.ggemm_slices(129) == [80, 49]
    assert R.ggemm_slices(320) == [112, 112, 96] and R.ggemm_slices(3072) == [128] * 24 and R.ggemm_slices(136, whole_k=True) == [136]
    assert sum(R.ggemm_slices(12345)) == 12345 and len(R.ggemm_slices(12345)) <= 64
    assert R.row_tiles(136) == [64, 64, 8] and R.row_tiles(64) == [64]
    comps = [dict(begin=0), dict(begin=4096), dict(begin=4096 + 5000)]
    assert R.items(comps, 4096 + 5000 + 12) == [[4096], [4096, 904], [12]]
