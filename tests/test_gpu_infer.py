"""-m gpu: forward-only inference over whole utterances (csrc/infer.hip on the schedule of csrc/infer_forward.hip, include/tdnnf_hip.h "inference").

The expectation is built in numpy from the contract: each chunk's clamped input window and i-vector, the CPU oracle's
forward pass in test mode (OracleNet, cv_update) over those chunks, and the valid rows scattered into the stacked output."""
import ctypes as C

import numpy as np
import pytest

from tests.gpu_util import dev, host, rel_l2
from tests.oracle_net import OracleNet
from tests.test_infer_plan import plan_ref

pytestmark = pytest.mark.gpu

FSF = 3
SMALL = dict(frames_per_chunk=24, num_sequences=3, strides=[1, 1, 0, 3, 3], bottleneck=16, feat_dim=40, ivector_dim=100, num_pdfs=50,
             hidden_dim=64, small_dim=32)
# a derived child: per-layer X.linear {-a, 0} / X.affine {0, b} (row-stride > 1 layers: the rho row order) and bottleneck dims
CHILD = dict(SMALL, strides=None, layer_offsets=[(2, 1), (0, 3), (5, 0), (1, 2)], bottleneck=[16, 8, 24, 16])


def model_stats(cfg, seed):
    """Plausible BatchNorm / ReLU statistics in tdnnf_net_get_stats order (tdnn1, the tdnnf layers, both heads)."""
    rng = np.random.default_rng(seed)
    Hd, S = cfg.hidden_dim, cfg.prefinal_small_dim
    out = []

    def bn(D):
        cnt, mean, var = 64.0, rng.normal(0.3, 0.3, D), rng.uniform(0.3, 2.0, D)
        out.append(np.concatenate([[cnt], cnt * mean, cnt * (var + mean * mean)]))

    def relu(D):
        out.append(np.concatenate([[64.0], rng.uniform(0, 30, D), rng.uniform(0, 30, D), [0.0], np.zeros(D)]))

    bn(Hd), relu(Hd)
    for _ in range(cfg.num_layers):
        bn(Hd), relu(Hd)
    for _ in range(2):
        bn(Hd), relu(Hd), bn(S)
    return np.concatenate(out)


def make_model(pkg, kw, seed=3, cv=1):
    cfg = pkg.trainer.make_config(**dict(kw, cv_update=cv))
    net = pkg.trainer.ChainNet(cfg)
    net.set_params(net.init_params_numpy(seed=seed, output_stddev=0.3))
    if cv:
        net.set_stats(model_stats(cfg, seed + 1))
    return cfg, net


def utterances(rng, lengths, feat_dim=40, ivector_dim=100, period=10, constant_iv=False):
    utts = []
    for T in lengths:
        f = rng.standard_normal((T, feat_dim)).astype(np.float32)
        R = max(1, -(-T // period))
        iv = rng.standard_normal((1 if constant_iv else R, ivector_dim)).astype(np.float32)
        if constant_iv:
            iv = np.repeat(iv, R, axis=0)
        utts.append((f, iv))
    return utts


def gathered(utts, plan, num_t_in, first_t, F, period):
    """t-major input windows (row i B + b) and i-vectors of the chunks of `plan`, frames clamped to their utterance."""
    B = len(plan)
    fd = utts[0][0].shape[1]
    feats = np.zeros((num_t_in * B, fd), np.float32)
    ivs = np.zeros((B, utts[0][1].shape[1]), np.float32)
    for b, (u, t0, row, n) in enumerate(plan):
        f, iv = utts[u]
        t = np.clip(t0 + first_t + np.arange(num_t_in), 0, f.shape[0] - 1)
        feats[np.arange(num_t_in) * B + b] = f[t]
        ivs[b] = iv[row if period > 0 else 0]
    return feats, ivs


def expected(pkg, cfg_kw, net, stats, utts, F, period, which="output", max_chunks=None):
    """numpy expectation: oracle forward (test-mode BatchNorm) per batch of chunks, valid rows scattered"""
    frames = [u[0].shape[0] for u in utts]
    rows = [u[1].shape[0] for u in utts]
    plan = plan_ref(F, FSF, frames, rows, period)
    Tout = F // FSF
    out0 = np.concatenate([[0], np.cumsum([-(-t // FSF) for t in frames])])
    out = np.zeros((out0[-1], cfg_kw["num_pdfs"]), np.float32)
    params = host(net.params)
    step = max_chunks or len(plan)
    for k0 in range(0, len(plan), step):
        part = plan[k0:k0 + step]
        B = len(part)
        cfg = pkg.trainer.make_config(**dict(cfg_kw, frames_per_chunk=F, num_sequences=B, cv_update=1))
        ref = OracleNet(pkg, cfg, net.components)
        ref.set_stats(stats)
        feats, ivs = gathered(utts, part, ref.num_t_in, ref.g_lda[0] - 1, F, period)
        den = pkg.synth.make_den_graph(8, cfg.num_pdfs, mean_out_degree=3.0, seed=5)
        sup = pkg.synth.make_supervision(B, Tout, cfg.num_pdfs, seed=6)
        _, _, acts = ref.forward_backward(params, feats, ivs, den, sup, forward_only=True)
        y = acts[which]
        for b, (u, t0, _, n) in enumerate(part):
            j = np.arange(n)
            out[out0[u] + t0 // FSF + j] = y[j * B + b]
    return out


def stacked(outs):
    return np.concatenate([host(o) for o in outs]) if outs else np.zeros((0, 0), np.float32)


LENGTHS = lambda F: [1, FSF - 1, F - 1, F, F + 1, int(3.5 * F)]


@pytest.mark.parametrize("which", ["output", "output-xent"])
@pytest.mark.parametrize("name,kw", [("7q-small", SMALL), ("child", CHILD)])
def test_parity_with_the_oracle(pkg, name, kw, which):
    cfg, net = make_model(pkg, kw)
    stats = net.get_stats()
    F = 30
    rng = np.random.default_rng(11)
    utts = utterances(rng, LENGTHS(F) + [17, 44])
    am = pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=5, output=which)
    got = stacked(am.compute(utts, ivector_period=10))
    ref = expected(pkg, kw, net, stats, utts, F, 10, which=which)
    e = rel_l2(got, ref)
    print("PARITY test_gpu_infer %s %s rel_l2 %.3e" % (name, which, e))
    assert got.shape == ref.shape and e < 1e-4, e
    # one i-vector per utterance (ivector_period <= 0)
    got0 = stacked(am.compute(utts, ivector_period=0))
    ref0 = expected(pkg, kw, net, stats, [(f, iv[:1]) for f, iv in utts], F, 0, which=which)
    assert rel_l2(got0, ref0) < 1e-4


@pytest.mark.parametrize("name,kw", [("7q-small", SMALL), ("child", CHILD)])
def test_chunk_width_does_not_change_the_output(pkg, name, kw):
    cfg, net = make_model(pkg, kw, seed=7)
    rng = np.random.default_rng(12)
    utts = utterances(rng, [1, 2, 50, 51, 52, 178, 301, 640], constant_iv=True)
    base = None
    for F in (51, 150, 300):
        for mc in (1, 256):
            got = stacked(pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=mc).compute(utts, ivector_period=10))
            if base is None:
                base = got
            e = rel_l2(got, base)
            assert e < 1e-5, (F, mc, e)


def test_agrees_with_the_training_forward(pkg):
    kw = SMALL
    cfg, net = make_model(pkg, kw, seed=9)
    F, B = 24, 4
    rng = np.random.default_rng(13)
    utts = utterances(rng, [24, 24, 24, 24])
    tcfg = pkg.trainer.make_config(**dict(kw, frames_per_chunk=F, num_sequences=B, cv_update=1))
    tnet = pkg.trainer.ChainNet(tcfg, share=net)
    tnet.set_capture(True)
    plan = plan_ref(F, FSF, [24] * 4, [3] * 4, 10)
    feats, ivs = gathered(utts, plan, tnet.num_t_in, tnet.first_t, F, 10)
    den = pkg.synth.make_den_graph(8, cfg.num_pdfs, mean_out_degree=3.0, seed=5)
    sup = pkg.synth.make_supervision(B, F // FSF, cfg.num_pdfs, seed=6)
    tnet.forward_backward(dev(feats), dev(ivs), pkg.hipabi.DenGraph(den), pkg.hipabi.Supervision(sup))
    y = host(tnet.activation("output"))
    want = np.concatenate([y[np.arange(F // FSF) * B + b] for b in range(B)])
    got = stacked(pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=B).compute(utts, ivector_period=10))
    e = rel_l2(got, want)
    assert e <= 1e-5, e
    tnet.close()


def test_model_file_and_updates(pkg, tmp_path):
    kw = SMALL
    cfg, net = make_model(pkg, kw, seed=21, cv=0)
    feats, iv = pkg.trainer.synthetic_egs(net, seed=4)
    den = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(8, cfg.num_pdfs, mean_out_degree=3.0, seed=5))
    sup = pkg.hipabi.Supervision(pkg.synth.make_supervision(cfg.num_sequences, cfg.frames_per_chunk // 3, cfg.num_pdfs, seed=6))
    fd, ivd = dev(feats), dev(iv)
    for step in range(3):
        net.grads.zero_()
        net.forward_backward(fd, ivd, den, sup, step=step)
        net.update(1e-3, step=step)
    rng = np.random.default_rng(14)
    utts = utterances(rng, [40, 100, 7])
    path = tmp_path / "final.mdl"
    net.write_model(path)
    am = pkg.infer.AcousticModel(net, frames_per_chunk=30, max_chunks=8)
    a = stacked(am.compute(utts))
    b = stacked(pkg.infer.AcousticModel.from_model_file(path, frames_per_chunk=30, max_chunks=8).compute(utts))
    assert rel_l2(a, b) < 1e-6
    net.grads.zero_()
    net.forward_backward(fd, ivd, den, sup, step=3)
    net.update(1e-3, step=3)
    c = stacked(am.compute(utts))  # the same AcousticModel: sees the new parameters and statistics
    path2 = tmp_path / "final2.mdl"
    net.write_model(path2)
    d = stacked(pkg.infer.AcousticModel.from_model_file(path2, frames_per_chunk=30, max_chunks=8).compute(utts))
    assert rel_l2(c, a) > 1e-6 and rel_l2(c, d) < 1e-6


@pytest.mark.parametrize("name,kw", [("7q-small", SMALL), ("child", CHILD)])
def test_fusion_is_real(pkg, name, kw):
    cfg, net = make_model(pkg, kw, seed=5)
    am = pkg.infer.AcousticModel(net, frames_per_chunk=30, max_chunks=4)
    pkg.hipabi.launch_forms(reset=True)
    am.compute(utterances(np.random.default_rng(2), [90, 31]))
    counted = pkg.hipabi.launch_forms(reset=True)
    ref = OracleNet(pkg, pkg.trainer.make_config(**dict(kw, frames_per_chunk=30, num_sequences=4, cv_update=1)), net.components)
    strided = sum(1 for L in ref.layers if L["out"][1] != L["inn"][1])
    assert strided >= 1
    fused, fallback = am.counts()
    assert (fused, fallback) == (cfg.num_layers + 3 - strided, strided)
    # every fused layer is (at least) one GEMM with the inference epilogue: the launch-form counters saw them
    assert sum(v for k, v in counted.items() if k.endswith(".post")) >= fused, counted


@pytest.mark.parametrize("name,extra", [("offset-supernet", dict(darts_num_offsets=3, darts_flags=1 | 16, darts_temp_proportion=0.8)),
                                        ("bottleneck-supernet", dict(bn_choice_dims=[4, 4, 8], bn_mode=0)),
                                        ("f16x3", dict(gemm_precision=3))])
def test_rejections(pkg, name, extra):
    lib = pkg.hipabi.load()
    kw = dict(SMALL, **extra)
    cfg = pkg.trainer.make_config(**kw)
    net = pkg.trainer.ChainNet(cfg)
    net.set_params(net.init_params_numpy(seed=1, output_stddev=0.3))
    feats, iv = pkg.trainer.synthetic_egs(net, seed=4)
    den = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(8, cfg.num_pdfs, mean_out_degree=3.0, seed=5))
    sup = pkg.hipabi.Supervision(pkg.synth.make_supervision(cfg.num_sequences, cfg.frames_per_chunk // 3, cfg.num_pdfs, seed=6))
    draws = np.random.default_rng(3).uniform(0.01, 0.99, max(net.num_draws, 1)).astype(np.float32)
    fd, ivd = dev(feats), dev(iv)

    def step():
        net.set_random_draws(draws)
        net.grads.zero_()
        r = host(net.forward_backward(fd, ivd, den, sup, step=0)).copy()
        return r, host(net.grads).copy()

    r0, g0 = step()
    h = C.c_void_p()
    assert lib.tdnnf_infer_create(net.h, 30, 4, 0, C.byref(h)) == 1
    msg = lib.tdnnf_last_error().decode()
    assert ("supernet" in msg) if name != "f16x3" else ("gemm_precision" in msg), msg
    r1, g1 = step()
    assert np.array_equal(r0, r1) and np.array_equal(g0, g1)
    # and a chunk width that is not a multiple of the subsampling
    cfg2, net2 = make_model(pkg, SMALL)
    assert lib.tdnnf_infer_create(net2.h, 31, 4, 0, C.byref(h)) == 1
    assert b"frame_subsampling" in lib.tdnnf_last_error()


def test_full_width(pkg):
    kw = dict(frames_per_chunk=150, num_sequences=1, feat_dim=40, ivector_dim=100, num_pdfs=6034, hidden_dim=1536, small_dim=256, bottleneck=160)
    cfg, net = make_model(pkg, kw, seed=31)
    stats = net.get_stats()
    rng = np.random.default_rng(15)
    lengths = rng.integers(300, 901, size=8).tolist()
    utts = utterances(rng, lengths)
    F = 51
    am = pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=256)
    got = stacked(am.compute(utts))
    # the oracle on a bounded sample: the first utterance's first and last chunks and another's middle one
    frames = [u[0].shape[0] for u in utts]
    plan = plan_ref(F, FSF, frames, [u[1].shape[0] for u in utts], 10)
    pick = [0, int(np.nonzero(plan[:, 0] == 0)[0][-1]), int(np.nonzero(plan[:, 0] == 5)[0][3])]
    out0 = np.concatenate([[0], np.cumsum([-(-t // FSF) for t in frames])])
    part = plan[pick]
    ocfg = pkg.trainer.make_config(**dict(kw, frames_per_chunk=F, num_sequences=len(part), cv_update=1))
    ref = OracleNet(pkg, ocfg, net.components)
    ref.set_stats(stats)
    feats, ivs = gathered(utts, part, ref.num_t_in, ref.g_lda[0] - 1, F, 10)
    den = pkg.synth.make_den_graph(8, cfg.num_pdfs, mean_out_degree=3.0, seed=5)
    sup = pkg.synth.make_supervision(len(part), F // FSF, cfg.num_pdfs, seed=6)
    _, _, acts = ref.forward_backward(host(net.params), feats, ivs, den, sup, forward_only=True)
    B = len(part)
    for b, (u, t0, _, n) in enumerate(part):
        j = np.arange(n)
        e = rel_l2(got[out0[u] + t0 // FSF + j], acts["output"][j * B + b])
        print("PARITY test_gpu_infer full width chunk (%d, %d) rel_l2 %.3e" % (u, t0, e))
        assert e < 1e-4, (u, t0, e)
    fused, fallback = am.counts()
    assert fused + fallback == cfg.num_layers + 3 and fallback >= 1
