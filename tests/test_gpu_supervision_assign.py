"""-m gpu: the reusable time-synchronous supervision (tdnnf_supervision_reserve / _assign; include/tdnnf_hip.h).  ONE reserved supervision is
assigned minibatch after minibatch; after each, its device tables are the bytes of a supervision created from the same arrays (the pf_*
tables against tests/supervision_tables_ref.py where the created one has none), and tdnnf_chain_objf_and_deriv and tdnnf_chain_objf give the
created one's BITS -- both ways run the same kernels on equal tables and chain_finish sums without atomics, so the bar is equality.  Then
stream order, the refusals (each by words of its message, the previous minibatch keeping its bits), the trainer and egs.minibatches(reuse=True).
The capacity excess is checked here on the entry itself (TDNNF_EINVAL, the handle untouched) and, without a device, on the host-only header
in tests/test_supervision_tables_ref.py."""
import numpy as np
import pytest
import torch

from tests import supervision_tables_ref as ref
from tests.gpu_util import Hip, dev, host

pytestmark = pytest.mark.gpu
XENT, LEAKY, L2 = 0.1, 0.1, 5e-5
P = 200  # the denominator graph's pdfs; every minibatch below names pdfs below it


@pytest.fixture(scope="module")
def hip(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return Hip(pkg)


@pytest.fixture(scope="module")
def den(pkg):
    return pkg.hipabi.DenGraph(pkg.synth.make_den_graph(30, P, mean_out_degree=4.0, seed=5))


@pytest.fixture(scope="module")
def batches(pkg):
    """name -> supervision dict; the sizes are asserted in test_the_set_is_the_one_the_kernels_need"""
    S = pkg.synth
    lat_wide = S.make_supervision_lattice(2, 23, 40, tolerance=4, alternatives=2, seed=2)
    return {"one": S.make_supervision(1, 1, 5, max_alt=1, seed=1),
            "narrow": S.make_supervision(3, 7, 30, max_alt=3, seed=1),
            "lat-narrow": S.make_supervision_lattice(2, 23, 40, tolerance=2, alternatives=1, seed=2),
            "lat-wide": lat_wide,
            "lat-128": S.make_supervision_lattice(1, 40, 200, tolerance=8, alternatives=8, seed=2),
            "lat-430": S.make_supervision_lattice(1, 40, 200, tolerance=10, alternatives=12, seed=2),
            "lat-wide-permuted": ref.permuted_within_sequences(lat_wide, seed=3),
            "P3": S.make_supervision_lattice(2, 17, 3, tolerance=3, alternatives=2, seed=4),
            "dead": ref.dead_states()}


# large -> `one` -> large, so that a stale tail of a larger minibatch would show
ORDER = ["lat-430", "one", "lat-128", "narrow", "lat-wide", "lat-narrow", "lat-wide-permuted", "P3", "dead", "one", "lat-430"]


def capacity(sups):
    return (max(int(s["B"]) for s in sups), max(int(s["T"]) for s in sups), max(len(s["state_time"]) for s in sups), max(len(s["arc_src"]) for s in sups))


def inputs(s, seed):
    rng = np.random.default_rng(seed)
    rows = int(s["B"]) * int(s["T"])
    y = (1.5 * rng.standard_normal((rows, P))).astype(np.float32)
    xo = rng.standard_normal((rows, P))
    return dev(y), dev((xo - np.log(np.exp(xo).sum(1, keepdims=True))).astype(np.float32))


def enqueue(hip, dg, ds, y, xo):
    """tdnnf_chain_objf_and_deriv with an xent output and tdnnf_chain_objf, enqueued on the current stream: (results, deriv, xent_deriv,
    results of the objective alone) as device tensors, with the workspaces that must outlive the kernels"""
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
    return (res, d, xd, res2), (ws, ws2)


def run(hip, dg, ds, y, xo):
    out, _keep = enqueue(hip, dg, ds, y, xo)
    return [host(t).copy() for t in out]


def same_bits(a, b):
    for i, (x, z) in enumerate(zip(a, b)):
        assert x.shape == z.shape and np.array_equal(x.view(np.int64 if x.dtype == np.float64 else np.int32), z.view(np.int64 if z.dtype == np.float64 else np.int32)), i


def same_tables(got, made, s):
    """the assigned handle's tables are the created one's bytes; the pf_* tables the statement's where the created one carries none"""
    want = ref.tables(s)
    for name in ref.NAMES:
        a, b = got[name], made[name] if len(made[name]) or not name.startswith("pf_") else want[name]
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32)), name
        assert np.array_equal(a.view(np.int32), want[name].view(np.int32)), name


def test_the_set_is_the_one_the_kernels_need(batches):
    w = {k: ref.widths(s) for k, s in batches.items()}
    sizes = lambda k: (w[k]["num_states"], w[k]["num_arcs"], w[k]["wide"], w[k]["max_states_per_frame"], w[k]["max_arcs_per_frame"])
    assert sizes("one") == (2, 1, 0, 1, 1) and sizes("narrow") == (48, 92, 0, 3, 9) and sizes("lat-narrow") == (174, 277, 0, 7, 13)
    assert sizes("lat-wide") == (502, 855, 1, 18, 31) and sizes("lat-128") == (3771, 7002, 1, 126, 241) and sizes("lat-430") == (6261, 11697, 1, 223, 430)
    assert all(int(np.max(s["arc_pdf"])) < P for s in batches.values())


def test_tables_and_info_are_the_created_supervisions(pkg, batches):
    abi = pkg.hipabi
    ds = abi.Supervision.reserve(*capacity(list(batches.values())))
    assert ds.kind == 0 and ds.capacity()["assigns"] == 0 and ds.capacity()["allocations"] == 0
    for n, name in enumerate(ORDER):
        s = batches[name]
        ds.assign(s)
        made = abi.Supervision(s)
        assert ds.kind == 0 and ds.info() == made.info() and (ds.B, ds.T) == (made.B, made.T), name
        w = ref.widths(s)
        assert ds.info() == {k: w[k] for k in ("num_states", "num_arcs", "max_states_per_frame", "wide")}, name
        t = made.tables()
        assert (len(t["pf_src"]) > 0) == bool(w["wide"]) and len(t["in_begin"]) == w["num_states"] + 1
        same_tables(ds.tables(), t, s)
        c = ds.capacity()
        assert c["allocations"] == 0 and c["assigns"] == n + 1 and (c["max_states"], c["max_arcs"]) == (6261, 11697), name


@pytest.mark.parametrize("num_form", [0, 2])
def test_results_are_the_created_supervisions_bits(hip, pkg, den, batches, num_form):
    abi = pkg.hipabi
    names = ORDER[:9] if num_form == 0 else ["lat-wide", "narrow", "lat-narrow"]  # under num_form 2 narrow minibatches take the wide form
    ds = abi.Supervision.reserve(*capacity([batches[k] for k in names]))
    with abi.option("num_form", num_form):
        for i, name in enumerate(names):
            s = batches[name]
            ds.assign(s)
            made = abi.Supervision(s)  # (under the option: num_call needs a narrow created supervision to carry the pf_* tables)
            y, xo = inputs(s, 100 + i)
            want, got = run(hip, den, made, y, xo), run(hip, den, ds, y, xo)
            assert want[0][5] == 1.0 and np.isfinite(want[0][:7]).all() and np.abs(want[1]).sum() > 0 and np.abs(want[2]).sum() > 0, name
            same_bits(want, got)
            if num_form == 2:
                assert len(made.tables()["pf_src"]) == len(s["arc_src"])
                same_tables(ds.tables(), made.tables(), s)


def test_stream_order(hip, pkg, den, batches):
    """objective on A, assign B, objective on B, and only then a look at either; three times over, so that both staging buffers come round"""
    abi = pkg.hipabi
    a, b = batches["lat-wide"], batches["lat-narrow"]
    ya, xa = inputs(a, 1)
    yb, xb = inputs(b, 2)
    want_a, want_b = run(hip, den, abi.Supervision(a), ya, xa), run(hip, den, abi.Supervision(b), yb, xb)
    ds = abi.Supervision.reserve(*capacity([a, b]))
    ds.assign(a)
    for _ in range(3):
        out_a, keep_a = enqueue(hip, den, ds, ya, xa)
        ds.assign(b)
        out_b, keep_b = enqueue(hip, den, ds, yb, xb)
        ds.assign(a)
        same_bits(want_a, [host(t).copy() for t in out_a])
        same_bits(want_b, [host(t).copy() for t in out_b])
    assert ds.capacity()["assigns"] == 7 and ds.capacity()["allocations"] == 0


def test_refusals(hip, pkg, den, batches):
    abi, lib = pkg.hipabi, pkg.hipabi.load()
    s = batches["narrow"]
    B, T, NS, NA = capacity([s])
    ds = abi.Supervision.reserve(B, T, NS, NA)
    y, xo = inputs(s, 7)
    # before the first assign: every entry refuses the handle, and names the call that helps
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    ws = hip.ws(hip.chain_workspace_bytes(den.h, B, T))
    empty = y[:0]
    from tests.test_gpu_net_e2e import _inputs, _net
    cfg, net = _net(pkg, use_natural_gradient=0)
    dn = abi.DenGraph(pkg.synth.make_den_graph(30, cfg.num_pdfs, mean_out_degree=4.0, seed=5))
    f, v = _inputs(pkg, net, cfg, 100)
    for call in (lambda: hip.chain_objf_and_deriv(den.h, ds.h, empty, None, LEAKY, L2, XENT, hip.vec(res), empty, None, hip.vec(ws), 1 << 20, hip.stream()),
                 lambda: hip.chain_objf(den.h, ds.h, empty, None, LEAKY, L2, hip.vec(res), hip.vec(ws), 1 << 20, hip.stream()),
                 lambda: hip.chain_numerator_part(den.h, ds.h, empty, 1, hip.vec(res), None, None, hip.vec(ws), 1 << 20, hip.stream()),
                 lambda: net.forward_backward(f, v, dn, ds, step=0),
                 lambda: net.objective(f, v, dn, ds)):
        with pytest.raises(abi.HipAbiError, match=r"holds no minibatch yet \(tdnnf_supervision_assign gives it one\)"):
            call()
    net.close()
    with pytest.raises(abi.HipAbiError, match="tdnnf_supervision_assign gives it one"):
        ds.tables()
    ds.assign(s)
    made = abi.Supervision(s)
    want = run(hip, den, made, y, xo)

    def refused(call, *words):
        with pytest.raises(abi.HipAbiError) as e:
            call()
        assert "tdnnf error 1:" in str(e.value)  # TDNNF_EINVAL
        for word in words:
            assert word in str(e.value), (word, str(e.value))
        assert (ds.B, ds.T) == (B, T) and ds.info() == made.info() and ds.capacity()["assigns"] == 1
        same_bits(want, run(hip, den, ds, y, xo))  # the previous minibatch, with the previous bits

    # each capacity one over
    S = pkg.synth
    refused(lambda: ds.assign(S.make_supervision(B + 1, T, 30, max_alt=1, seed=1)), "supervision_assign: ", "max_sequences = 3 by 1")
    refused(lambda: ds.assign(S.make_supervision(B, T + 1, 30, max_alt=1, seed=1)), "supervision_assign: ", "max_frames = 7 by 1")
    one_more_state = dict(s, seq_state_begin=np.append(s["seq_state_begin"][:-1], NS + 1), state_time=np.append(s["state_time"], T),
                          final_logprob=np.append(s["final_logprob"], 0.0))
    refused(lambda: ds.assign(one_more_state), "supervision_assign: ", "49 states exceed the capacity max_states = 48 by 1")
    one_more_arc = dict(s, seq_arc_begin=np.append(s["seq_arc_begin"][:-1], NA + 1), **{k: np.append(s[k], s[k][-1]) for k in ("arc_src", "arc_dst", "arc_pdf", "arc_logprob")})
    refused(lambda: ds.assign(one_more_arc), "supervision_assign: ", "93 arcs exceed the capacity max_arcs = 92 by 1")
    # each validation failure of tdnnf_supervision_create, in its words
    from tests.test_supervision_tables_ref import bad_inputs
    for changed, words in bad_inputs(s):
        refused(lambda: ds.assign(dict(s, **changed)), "supervision_assign: " + words)
        with pytest.raises(abi.HipAbiError) as e:
            abi.Supervision(dict(s, **changed))
        assert "supervision_create: " + words in str(e.value)
    # a created handle, an end-to-end handle; and this handle at the end-to-end assign
    k = [abi.iarr(s["seq_state_begin"]), abi.iarr(s["seq_arc_begin"]), abi.iarr(s["state_time"]), abi.farr(s["final_logprob"]), abi.iarr(s["arc_src"]),
         abi.iarr(s["arc_dst"]), abi.iarr(s["arc_pdf"]), abi.farr(s["arc_logprob"])]
    assert lib.tdnnf_supervision_assign(made.h, B, T, *[x[1] for x in k], 1.0, None) == 1
    assert b"tdnnf_supervision_create" in lib.tdnnf_last_error() and b"tdnnf_supervision_reserve" in lib.tdnnf_last_error()
    e2e = abi.Supervision.reserve_e2e(B, T, P, 64, 256)
    assert lib.tdnnf_supervision_assign(e2e.h, B, T, *[x[1] for x in k], 1.0, None) == 1
    assert b"end-to-end" in lib.tdnnf_last_error() and b"tdnnf_supervision_assign_e2e" in lib.tdnnf_last_error()
    with pytest.raises(abi.HipAbiError, match="end-to-end"):
        e2e.assign(s)
    graphs = pkg.synth.make_e2e_supervision(B, T, P, seed=3)["graphs"]
    with pytest.raises(abi.HipAbiError, match="time-synchronous"):
        ds.assign(graphs, T)
    g = abi.Supervision._stack_e2e(graphs)[1]
    assert lib.tdnnf_supervision_assign_e2e(ds.h, B, T, *[x[1] for x in g], 1.0, None) == 1
    assert b"tdnnf_supervision_reserve_e2e" in lib.tdnnf_last_error()
    with pytest.raises(abi.HipAbiError, match="tdnnf_supervision_reserve did not make"):
        made.capacity()
    same_bits(want, run(hip, den, ds, y, xo))


def test_the_trainer_takes_an_assigned_supervision(pkg):
    """two nets from the same parameters, two steps with updates each: one on created supervisions, one on ONE reserved supervision assigned
    the two minibatches -- the same results bits and the same parameters"""
    from tests.test_gpu_net_e2e import _inputs, _net
    (cfg, net_made), (_, net) = _net(pkg), _net(pkg)
    T = cfg.frames_per_chunk // 3
    dg = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(30, cfg.num_pdfs, mean_out_degree=4.0, seed=5))
    sups = [pkg.synth.make_supervision(cfg.num_sequences, T, cfg.num_pdfs, max_alt=2, seed=11),
            pkg.synth.make_supervision_lattice(cfg.num_sequences, T, cfg.num_pdfs, tolerance=3, alternatives=2, seed=12)]
    assert [ref.widths(s)["wide"] for s in sups] == [0, 1]
    ds = pkg.hipabi.Supervision.reserve(*capacity(sups))
    ds.assign(sups[1])  # (it held another minibatch before)
    for i, s in enumerate(sups):
        f, v = _inputs(pkg, net, cfg, 100 + i)
        want = host(net_made.forward_backward(f, v, dg, pkg.hipabi.Supervision(s), step=i)).copy()
        net_made.update(1e-3, step=i)
        ds.assign(s)
        got = host(net.forward_backward(f, v, dg, ds, step=i)).copy()
        net.update(1e-3, step=i)
        assert want[5] == 1.0 and np.array_equal(want.view(np.int64), got.view(np.int64)), i
    pa, pb = host(net_made.params).copy(), host(net.params).copy()
    assert np.array_equal(pa.view(np.int32), pb.view(np.int32)) and float(np.abs(pa.astype(np.float64)).sum()) == float(np.abs(pb.astype(np.float64)).sum())
    assert ds.capacity()["allocations"] == 0
    net_made.close()
    net.close()


def test_egs_minibatches_reuse(pkg, tmp_path):
    E = pkg.egs
    cfg = pkg.trainer.make_config(frames_per_chunk=24, num_sequences=4, strides=[1, 0, 3], bottleneck=16, feat_dim=40, ivector_dim=100, num_pdfs=60,
                                  hidden_dim=64, small_dim=32)
    net = pkg.trainer.ChainNet(cfg)
    B, T = cfg.num_sequences, cfg.frames_per_chunk // 3

    def archive(path, sups):
        with E.Writer(path) as w:
            for m, sup in enumerate(sups):
                feats, iv = pkg.trainer.synthetic_egs(net, seed=10 + m)
                for b in range(B):
                    w.write("u%d-%d" % (m, b), feats[b::B], net.first_t, E.sequence_of(sup, b), cfg.num_pdfs, ivector=iv[b], compress=False)
        return path

    # minibatches of about one size: one reserve, sized from the first with headroom
    alike = sorted((pkg.synth.make_supervision(B, T, cfg.num_pdfs, max_alt=2, seed=20 + m) for m in range(3)), key=lambda s: -len(s["arc_src"]))
    assert all(len(s[k]) <= len(alike[0][k]) * 1.25 for s in alike for k in ("state_time", "arc_src"))  # (the largest first: the rest fit its headroom)
    path = archive(tmp_path / "alike.ark", alike)
    plain = [sup.tables() for _, _, sup in E.minibatches(path, net)]
    handles, n = set(), 0
    for (f, iv, sup), want in zip(E.minibatches(path, net, reuse=True), plain):
        got = sup.tables()  # (valid until the next item is requested)
        assert all(np.array_equal(got[k].view(np.int32), want[k].view(np.int32)) for k in ref.NAMES if len(want[k]) or not k.startswith("pf_"))
        assert sup.reserves == 1 and sup.capacity()["allocations"] == 0
        handles.add(id(sup))
        n += 1
    assert n == 3 and len(handles) == 1
    # a later minibatch larger than the first with its headroom: reserved again, once
    grows = [alike[0], pkg.synth.make_supervision_lattice(B, T, cfg.num_pdfs, tolerance=3, alternatives=3, seed=5), alike[1]]
    assert len(grows[1]["state_time"]) > 1.25 * len(grows[0]["state_time"]) + 1
    path = archive(tmp_path / "grows.ark", grows)
    plain = [sup.tables() for _, _, sup in E.minibatches(path, net)]
    reserves = []
    for (f, iv, sup), want in zip(E.minibatches(path, net, reuse=True, prefetch=1), plain):
        got = sup.tables()
        assert all(np.array_equal(got[k].view(np.int32), want[k].view(np.int32)) for k in ref.NAMES if len(want[k]) or not k.startswith("pf_"))
        reserves.append(sup.reserves)
    assert reserves == [1, 2, 2]
    net.close()
