"""-m gpu: whole-utterance inference in f16x3 (csrc/infer_planes.hip on the schedule of csrc/infer_forward.hip, tdnnf_infer_create_arith with gemm_precision 3): every GEMM of
the forward pass from f16 planes, held to the same expectation and the same bars as the f32 path (tests/test_gpu_infer.py).

Shapes: the smallest at which a tile's overhang (fewer rows than one 256-row tile, a batch of one after a full batch), the taps'
shifted rows and the strided rows of a rho-ordered layer can go wrong; one case at the workload's own widths."""
import ctypes as C

import numpy as np
import pytest

from tests.gpu_util import dev, host, rel_l2
from tests.test_gpu_infer import CHILD, LENGTHS, SMALL, expected, make_model, stacked, utterances

pytestmark = pytest.mark.gpu


def gemms_per_batch(cfg):
    """lda, tdnn1, every layer's .linear and .affine, prefinal-l, the head's affine and linear, the output"""
    return 2 * cfg.num_layers + 6


def batches(am, utts, period=10):
    frames = [u[0].shape[0] for u in utts]
    rows = [u[1].shape[0] if period > 0 else 1 for u in utts]
    n = len(am.plan(frames, rows, period))
    return -(-n // am.max_chunks)


@pytest.mark.parametrize("which", ["output", "output-xent"])
@pytest.mark.parametrize("name,kw", [("7q-small", SMALL), ("child", CHILD)])
def test_parity_with_the_oracle(pkg, name, kw, which):
    cfg, net = make_model(pkg, kw)
    stats = net.get_stats()
    F = 30
    rng = np.random.default_rng(11)
    utts = utterances(rng, LENGTHS(F) + [17, 44])
    am = pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=5, output=which, arithmetic="f16x3")
    got = stacked(am.compute(utts, ivector_period=10))
    ref = expected(pkg, kw, net, stats, utts, F, 10, which=which)
    e = rel_l2(got, ref)
    print("PARITY test_gpu_infer_f16x3 %s %s rel_l2 %.3e" % (name, which, e))
    f32 = stacked(pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=5, output=which).compute(utts, ivector_period=10))
    print("PARITY test_gpu_infer_f16x3 %s %s against the f32 AcousticModel rel_l2 %.3e" % (name, which, rel_l2(got, f32)))
    assert got.shape == ref.shape and e < 1e-4, e
    # one i-vector per utterance (ivector_period <= 0)
    got0 = stacked(am.compute(utts, ivector_period=0))
    ref0 = expected(pkg, kw, net, stats, [(f, iv[:1]) for f, iv in utts], F, 0, which=which)
    e0 = rel_l2(got0, ref0)
    print("PARITY test_gpu_infer_f16x3 %s %s one i-vector rel_l2 %.3e" % (name, which, e0))
    assert e0 < 1e-4, e0


def test_the_planes_really_ran(pkg):
    utts = utterances(np.random.default_rng(2), [90, 31, 200])
    cfg, net = make_model(pkg, SMALL, seed=5)
    am = pkg.infer.AcousticModel(net, frames_per_chunk=30, max_chunks=4, arithmetic="f16x3")
    am.compute(utts)
    nb = batches(am, utts)
    assert nb >= 2
    planes, f32 = am.gemm_counts()
    print("COUNTS 7q-small plane_gemms %d f32_gemms %d batches %d" % (planes, f32, nb))
    assert f32 == 0 and planes >= nb * gemms_per_batch(cfg), (planes, f32)
    ccfg, cnet = make_model(pkg, CHILD, seed=5)
    cam = pkg.infer.AcousticModel(cnet, frames_per_chunk=30, max_chunks=4, arithmetic="f16x3")
    cam.compute(utts)
    planes, f32 = cam.gemm_counts()
    print("COUNTS child plane_gemms %d f32_gemms %d" % (planes, f32))
    assert planes > 0 and planes + f32 == batches(cam, utts) * gemms_per_batch(ccfg), (planes, f32)
    fam = pkg.infer.AcousticModel(net, frames_per_chunk=30, max_chunks=4, arithmetic="f32")
    fam.compute(utts)
    assert fam.gemm_counts()[0] == 0
    assert am.counts() == fam.counts()  # the BatchNorm stages are fused (or not) as in f32


def test_batch_tails_and_tile_edges(pkg):
    kw = SMALL
    cfg, net = make_model(pkg, kw, seed=17)
    stats = net.get_stats()
    F, mc = 30, 4
    rng = np.random.default_rng(19)
    inputs = [utterances(rng, [4 * F]),        # a batch that fills 4 chunks
              utterances(rng, [1]),            # fewer rows than one tile
              utterances(rng, [3 * F + 5, 7])]  # 4 + 1 chunks: a full batch, then a batch of one
    am = pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=mc, arithmetic="f16x3")
    assert [len(am.plan([u[0].shape[0] for u in x], [u[1].shape[0] for u in x])) for x in inputs] == [4, 1, 5]
    for i, utts in enumerate(inputs):
        got = stacked(am.compute(utts))
        e = rel_l2(got, expected(pkg, kw, net, stats, utts, F, 10, max_chunks=mc))
        print("PARITY test_gpu_infer_f16x3 tails compute %d rel_l2 %.3e" % (i, e))
        assert e < 1e-4, (i, e)
        if i > 0:  # an object that saw only this input: rows of the earlier, larger batch must not be read
            fresh = stacked(pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=mc, arithmetic="f16x3").compute(utts))
            d = rel_l2(got, fresh)
            assert d <= 1e-6, (i, d)


def test_odd_widths(pkg):
    kw = dict(SMALL, hidden_dim=96, small_dim=48, bottleneck=16, num_pdfs=50)
    cfg, net = make_model(pkg, kw, seed=23)
    F = 30
    utts = utterances(np.random.default_rng(24), LENGTHS(F))
    am = pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=5, arithmetic="f16x3")
    e = rel_l2(stacked(am.compute(utts)), expected(pkg, kw, net, net.get_stats(), utts, F, 10, max_chunks=5))
    print("PARITY test_gpu_infer_f16x3 odd widths rel_l2 %.3e" % e)
    assert e < 1e-4, e
    assert am.gemm_counts()[1] == 0


@pytest.mark.parametrize("name,kw", [("7q-small", SMALL), ("child", CHILD)])
def test_chunk_width_does_not_change_the_output(pkg, name, kw):
    cfg, net = make_model(pkg, kw, seed=7)
    utts = utterances(np.random.default_rng(12), [1, 2, 50, 51, 178], constant_iv=True)
    a = stacked(pkg.infer.AcousticModel(net, frames_per_chunk=24, max_chunks=4, arithmetic="f16x3").compute(utts))
    b = stacked(pkg.infer.AcousticModel(net, frames_per_chunk=60, max_chunks=4, arithmetic="f16x3").compute(utts))
    e = rel_l2(a, b)
    print("PARITY test_gpu_infer_f16x3 %s F 24 against F 60 rel_l2 %.3e" % (name, e))
    assert e < 1e-5, e


@pytest.mark.parametrize("log2_scale", [10, -10])
def test_feature_scale(pkg, log2_scale):
    kw = SMALL
    cfg, net = make_model(pkg, kw, seed=27)
    F = 30
    utts = [(f * np.float32(2.0 ** log2_scale), iv) for f, iv in utterances(np.random.default_rng(28), [F + 1, 44, 3])]
    am = pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=5, arithmetic="f16x3")
    e = rel_l2(stacked(am.compute(utts)), expected(pkg, kw, net, net.get_stats(), utts, F, 10, max_chunks=5))
    print("PARITY test_gpu_infer_f16x3 features x 2^%d rel_l2 %.3e" % (log2_scale, e))
    assert e < 1e-4, e


def test_parameters_are_read_at_every_compute(pkg):
    kw = SMALL
    cfg, net = make_model(pkg, kw, seed=33)
    F = 30
    utts = utterances(np.random.default_rng(34), [40, 100, 7])
    am = pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=4, arithmetic="f16x3")
    a = stacked(am.compute(utts))
    net.set_params(net.init_params_numpy(seed=35, output_stddev=0.3))
    b = stacked(am.compute(utts))
    e = rel_l2(b, expected(pkg, kw, net, net.get_stats(), utts, F, 10, max_chunks=4))
    assert e < 1e-4, e
    assert rel_l2(b, a) > 1e-2  # (the new parameters, not the planes of the old ones)


def raw_create(pkg, net, F, mc, which, precision):
    lib = pkg.hipabi.load()
    h = C.c_void_p()
    rc = lib.tdnnf_infer_create_arith(net.h, F, mc, which, precision, C.byref(h))
    return rc, h, lib.tdnnf_last_error().decode()


def test_entry_rules(pkg):
    lib = pkg.hipabi.load()
    cfg, net = make_model(pkg, SMALL)
    F = 30
    utts = utterances(np.random.default_rng(11), LENGTHS(F) + [17, 44])
    for precision in (1, 2):
        rc, h, msg = raw_create(pkg, net, F, 4, 0, precision)
        assert rc == 1 and "gemm_precision" in msg, (rc, msg)
    # precision 0: the object tdnnf_infer_create builds, bit for bit
    ref_am = pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=5)
    rc, h, msg = raw_create(pkg, net, F, 5, 0, 0)
    assert rc == 0, msg
    am0 = pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=5)
    lib.tdnnf_infer_destroy(am0.h)
    am0.h = h
    assert np.array_equal(stacked(am0.compute(utts)), stacked(ref_am.compute(utts)))
    assert am0.gemm_counts()[0] == 0
    # a model trained in f16x3: the old entry refuses it (test_gpu_infer.py::test_rejections), the new one reads its f32 parameters
    kw3 = dict(SMALL, gemm_precision=3)
    cfg3, net3 = make_model(pkg, kw3)
    am3 = pkg.infer.AcousticModel(net3, frames_per_chunk=F, max_chunks=5, arithmetic="f16x3")
    e = rel_l2(stacked(am3.compute(utts)), expected(pkg, kw3, net3, net3.get_stats(), utts, F, 10, max_chunks=5))
    print("PARITY test_gpu_infer_f16x3 model with gemm_precision 3 rel_l2 %.3e" % e)
    assert e < 1e-4, e
    rc, h, msg = raw_create(pkg, net, 31, 4, 0, 3)
    assert rc == 1 and "frame_subsampling" in msg, msg


@pytest.mark.parametrize("name,extra", [("offset-supernet", dict(darts_num_offsets=3, darts_flags=1 | 16, darts_temp_proportion=0.8)),
                                        ("bottleneck-supernet", dict(bn_choice_dims=[4, 4, 8], bn_mode=0))])
def test_supernets_are_refused(pkg, name, extra):
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
    for precision in (0, 3):
        rc, h, msg = raw_create(pkg, net, 30, 4, 0, precision)
        assert rc == 1 and "supernet" in msg, (precision, msg)
    r1, g1 = step()
    assert np.array_equal(r0, r1) and np.array_equal(g0, g1)


def test_full_width(pkg):
    """The only case at the workload's own widths."""
    kw = dict(frames_per_chunk=150, num_sequences=1, feat_dim=40, ivector_dim=100, num_pdfs=6034, hidden_dim=1536, small_dim=256, bottleneck=160)
    cfg, net = make_model(pkg, kw, seed=31)
    F, mc = 150, 4
    utts = utterances(np.random.default_rng(15), [200, 251, 301])
    am = pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=mc, arithmetic="f16x3")
    got = stacked(am.compute(utts))
    e = rel_l2(got, expected(pkg, kw, net, net.get_stats(), utts, F, 10, max_chunks=mc))
    print("PARITY test_gpu_infer_f16x3 full width rel_l2 %.3e" % e)
    assert e < 1e-4, e
    planes, f32 = am.gemm_counts()
    assert f32 == 0 and planes == batches(am, utts) * gemms_per_batch(cfg), (planes, f32)
