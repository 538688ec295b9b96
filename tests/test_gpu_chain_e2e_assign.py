"""-m gpu: the reusable end-to-end supervision (tdnnf_supervision_reserve_e2e / _assign_e2e; include/tdnnf_hip.h).  ONE reserved supervision
is assigned two consecutive minibatches that differ in the number of sequences, the frames and the graphs; for each,
tdnnf_chain_objf_and_deriv and tdnnf_chain_objf give the BITS of a supervision created from the same arrays -- results, nnet_output_deriv
and xent_deriv.  The assigned graph set's tables are the created one's bytes (tests/test_gpu_align_assign.py) and the kernels are the same,
so the bar is equality.  One case per launch form of the recursion (64 / 256 / 1024 threads by the minibatch's largest graph; the two
state vectors in the scratch under option align_form 2); in three of them the form CHANGES between the two minibatches."""
import numpy as np
import pytest
import torch

from tests.gpu_util import Hip, dev, host
from tests.test_gpu_chain_e2e import _KINDS

pytestmark = pytest.mark.gpu
XENT, LEAKY, L2 = 0.1, 0.1, 5e-5
P = 41


@pytest.fixture(scope="module")
def hip(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Hip(pkg)


@pytest.fixture(scope="module")
def den(pkg):
    return pkg.hipabi.DenGraph(pkg.synth.make_den_graph(30, P, mean_out_degree=4.0, seed=5))


# name: (align_form, (kinds of tests/test_gpu_chain_e2e.py, T, weight, the recursion's threads) of the first and of the second minibatch)
CASES = {
    "64": (0, ("sss", 7, 1.0, 64), ("ss", 5, 0.75, 64)),
    "256": (0, ("ssss", 5, 1.0, 64), ("shs", 7, 0.75, 256)),
    "1024": (0, ("shs", 7, 1.0, 256), ("bs", 4, 0.5, 1024)),
    "global": (2, ("hss", 7, 1.0, 256), ("ss", 3, 0.75, 64)),
}


def minibatch(pkg, name, i):
    kinds, T, w, threads = CASES[name][1 + i]
    seed = 1000 * sorted(CASES).index(name) + 100 * i
    graphs = [_KINDS[k](pkg, T, P, seed + j) for j, k in enumerate(kinds)]
    rng = np.random.default_rng(seed)
    y = (1.5 * rng.standard_normal((T * len(kinds), P))).astype(np.float32)
    xo = rng.standard_normal((T * len(kinds), P))
    return graphs, T, w, threads, dev(y), dev((xo - np.log(np.exp(xo).sum(1, keepdims=True))).astype(np.float32))


def capacity(batches):
    return (max(len(g) for g, *_ in batches), max(b[1] for b in batches), max(sum(x["S"] for x in g) for g, *_ in batches),
            max(sum(len(x["src"]) for x in g) for g, *_ in batches))


def run(hip, dg, ds, y, xo):
    """(results of tdnnf_chain_objf_and_deriv, deriv, xent_deriv, results of tdnnf_chain_objf), downloaded"""
    nb = hip.chain_workspace_bytes(dg.h, ds.B, ds.T)
    ws = hip.ws(nb)
    ws.fill_(float("nan"))
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    d, xd = torch.full_like(y, 5.0), torch.full_like(y, 5.0)
    hip.chain_objf_and_deriv(dg.h, ds.h, y, xo, LEAKY, L2, XENT, hip.vec(res), d, xd, hip.vec(ws), nb, hip.stream())
    nb2 = hip.chain_objf_workspace_bytes(dg.h, ds.B, ds.T)
    ws2 = hip.ws(nb2)
    ws2.fill_(float("nan"))
    res2 = torch.full((8,), -7.0, dtype=torch.float64, device="cuda")
    hip.chain_objf(dg.h, ds.h, y, xo, LEAKY, L2, hip.vec(res2), hip.vec(ws2), nb2, hip.stream())
    return [host(t).copy() for t in (res, d, xd, res2)]


def same_bits(a, b):
    for i, (x, z) in enumerate(zip(a, b)):
        assert x.shape == z.shape and np.array_equal(x.view(np.int64 if x.dtype == np.float64 else np.int32), z.view(np.int64 if z.dtype == np.float64 else np.int32)), i


@pytest.mark.parametrize("name", list(CASES))
def test_two_minibatches_on_one_reserved_supervision(hip, pkg, den, name):
    abi = pkg.hipabi
    batches = [minibatch(pkg, name, i) for i in range(2)]
    assert len(batches[0][0]) != len(batches[1][0]) and batches[0][1] != batches[1][1]
    with abi.option("align_form", CASES[name][0]):
        ds = abi.Supervision.reserve_e2e(*capacity(batches)[:2], P, *capacity(batches)[2:])
        assert ds.kind == 1
        for graphs, T, w, threads, y, xo in batches + batches[:1]:
            ds.assign(graphs, T, weight=w)
            made = abi.Supervision.from_graphs(graphs, T, weight=w, num_pdfs=P)
            assert ds.e2e_form() == made.e2e_form() and ds.e2e_form()["threads"] == threads
            assert ds.e2e_form()["vectors_in_lds"] == (0 if CASES[name][0] == 2 else 1)
            assert ds.info() == made.info() and (ds.B, ds.T) == (made.B, made.T)
            want, got = run(hip, den, made, y, xo), run(hip, den, ds, y, xo)
            assert want[0][5] == 1.0 and np.isfinite(want[0][:7]).all() and np.abs(want[1]).sum() > 0
            same_bits(want, got)


def test_refusals(hip, pkg, den):
    abi, lib = pkg.hipabi, pkg.hipabi.load()
    graphs, T, w, _, y, xo = minibatch(pkg, "64", 0)
    B, S, A = len(graphs), sum(g["S"] for g in graphs), sum(len(g["src"]) for g in graphs)
    ds = abi.Supervision.reserve_e2e(B, T, P, S, A)
    # before the first assign: refused, and says so
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    ws = hip.ws(hip.chain_workspace_bytes(den.h, B, T))
    empty = y[:0]  # B * T = 0 rows: the shape the entries would ask of a supervision without a minibatch
    for call in (lambda: hip.chain_objf_and_deriv(den.h, ds.h, empty, None, LEAKY, L2, XENT, hip.vec(res), empty, None, hip.vec(ws), 1 << 20, hip.stream()),
                 lambda: hip.chain_objf(den.h, ds.h, empty, None, LEAKY, L2, hip.vec(res), hip.vec(ws), 1 << 20, hip.stream())):
        with pytest.raises(abi.HipAbiError, match="holds no minibatch yet"):
            call()
    ds.assign(graphs, T, weight=w)
    made = abi.Supervision.from_graphs(graphs, T, weight=w, num_pdfs=P)
    want = run(hip, den, made, y, xo)

    def refused(call, *words):
        with pytest.raises(abi.HipAbiError) as e:
            call()
        assert "tdnnf error 1:" in str(e.value)  # TDNNF_EINVAL
        for word in words:
            assert word in str(e.value), (word, str(e.value))
        assert (ds.B, ds.T) == (B, T) and ds.info() == made.info()
        same_bits(want, run(hip, den, ds, y, xo))  # the previous minibatch, with the previous bits

    small = _KINDS["s"](pkg, T, P, 5)
    refused(lambda: ds.assign(graphs + [small], T), "supervision_assign_e2e", "max_sequences", "by 1")
    refused(lambda: ds.assign(graphs, T + 1), "supervision_assign_e2e", "max_frames", "by 1")
    more_states = dict(graphs[0], S=graphs[0]["S"] + 1, init=np.append(graphs[0]["init"], -np.inf), final=np.append(graphs[0]["final"], -np.inf))
    refused(lambda: ds.assign([more_states] + graphs[1:], T), "max_states", "by 1")
    g = graphs[0]
    more_arcs = dict(g, **{k: np.append(g[k], g[k][-1]) for k in ("src", "dst", "pdf", "logprob")})
    refused(lambda: ds.assign([more_arcs] + graphs[1:], T), "max_arcs", "by 1")
    bad_pdf = dict(g, pdf=np.where(np.arange(len(g["pdf"])) == 0, P, g["pdf"]))
    refused(lambda: ds.assign([bad_pdf] + graphs[1:], T), "epsilon arcs are not supported")
    # the assign entry takes a reserved supervision only
    k = abi.Supervision._stack_e2e(graphs)[1]
    assert lib.tdnnf_supervision_assign_e2e(made.h, B, T, *[x[1] for x in k], 1.0, None) == 1
    assert b"tdnnf_supervision_reserve_e2e" in lib.tdnnf_last_error()


def test_the_trainer_accepts_an_assigned_supervision(pkg):
    """two nets with the same parameters (a net's gradients add up from call to call): one steps on a created supervision, the other on the
    reserved one that held another minibatch before -- the same results and gradients, bit for bit; then the other minibatch trains too"""
    from tests.test_gpu_net_e2e import _inputs, _net
    (cfg, net_made), (_, net) = _net(pkg), _net(pkg)
    T = cfg.frames_per_chunk // 3
    dg = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(30, cfg.num_pdfs, mean_out_degree=4.0, seed=5))
    e2e = pkg.synth.make_e2e_supervision(cfg.num_sequences, T, cfg.num_pdfs, units=(2, 6), seed=7, optional=[1])
    other = pkg.synth.make_e2e_supervision(cfg.num_sequences, T, cfg.num_pdfs, units=(3, 5), seed=8)
    f, v = _inputs(pkg, net, cfg, 100)
    want = host(net_made.forward_backward(f, v, dg, pkg.hipabi.Supervision(e2e), step=0)).copy()
    want_grads = host(net_made.grads).copy()
    net_made.close()
    ds = pkg.hipabi.Supervision.reserve_e2e(cfg.num_sequences, T, cfg.num_pdfs, 2 * sum(g["S"] for g in e2e["graphs"] + other["graphs"]),
                                            2 * sum(len(g["src"]) for g in e2e["graphs"] + other["graphs"]))
    ds.assign(other["graphs"], T)
    ds.assign(e2e["graphs"], T, weight=e2e.get("weight", 1.0))
    got = host(net.forward_backward(f, v, dg, ds, step=0)).copy()
    assert want[5] == 1.0 and np.array_equal(want.view(np.int64), got.view(np.int64))
    assert np.abs(want_grads).sum() > 0 and np.array_equal(want_grads.view(np.int32), host(net.grads).view(np.int32))
    ds.assign(other["graphs"], T)
    r = host(net.forward_backward(f, v, dg, ds, step=1)).copy()
    assert r[5] == 1.0 and np.isfinite(r[:7]).all() and r[0] != want[0]
    net.close()
