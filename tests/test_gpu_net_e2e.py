"""-m gpu: the trainer with an END-TO-END supervision (tdnnf_supervision_create_e2e) -- ChainNet.forward_backward, objective and update need
no change for it.  A small net: the KW shape of tests/test_gpu_net_objective.py with 36 frames per chunk (T = 12 output frames), B = 4.

 * the end-to-end form of a time-synchronous supervision trains as the supervision itself does: results[0] within 1e-9 (|num| + |den|), the
   flat gradient and the parameters after one update rel_l2 < 1e-4;
 * a cyclic minibatch (synth.make_e2e_supervision): ok = 1, a finite objective, objective() within 1e-6 relative of it and without a trace
   in parameters, gradients and statistics;
 * natural gradient on, three steps with updates, twice from the same seed: the same bits."""
import numpy as np
import pytest
import torch

from tests.gpu_util import dev, host, rel_l2

pytestmark = pytest.mark.gpu

KW = dict(frames_per_chunk=36, num_sequences=4, strides=[1, 0, 3], bottleneck=16, feat_dim=40, ivector_dim=100, num_pdfs=40, hidden_dim=64, small_dim=32,
          use_natural_gradient=1)


def _net(pkg, **more):
    cfg = pkg.trainer.make_config(**dict(KW, **more))
    net = pkg.trainer.ChainNet(cfg)
    net.set_params(net.init_params_numpy(seed=1, output_stddev=0.1))
    return cfg, net


def _inputs(pkg, net, cfg, seed):
    feats, iv = pkg.trainer.synthetic_egs(net, seed=seed)
    return dev(feats), dev(iv)


def test_end_to_end_form_of_a_time_synchronous_supervision_trains_alike(pkg):
    out = []
    for kind in (0, 1):
        cfg, net = _net(pkg, use_natural_gradient=0)
        T = cfg.frames_per_chunk // 3
        assert cfg.num_sequences == 4 and 10 <= T <= 16
        den = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(30, cfg.num_pdfs, mean_out_degree=4.0, seed=5))
        sup = pkg.synth.make_supervision(cfg.num_sequences, T, cfg.num_pdfs, seed=202)
        ds = pkg.hipabi.Supervision(pkg.synth.e2e_supervision_from_supervision(sup, cfg.num_pdfs) if kind else sup)
        assert ds.kind == kind
        f, v = _inputs(pkg, net, cfg, 100)
        r = host(net.forward_backward(f, v, den, ds, step=0)).copy()
        g = host(net.grads).copy()
        net.update(1e-3, step=0)
        out.append((r, g, host(net.params).copy()))
        net.close()
    (ra, ga, pa), (rb, gb, pb) = out
    print("NET_E2E same supervision, two kinds: objf %.12g / %.12g, gradient rel_l2 %.2e, parameters rel_l2 %.2e" % (ra[0], rb[0], rel_l2(gb, ga), rel_l2(pb, pa)))
    assert ra[5] == rb[5] == 1.0
    assert abs(rb[0] - ra[0]) <= 1e-9 * (abs(ra[3]) + abs(ra[4]))
    assert rel_l2(gb, ga) < 1e-4 and rel_l2(pb, pa) < 1e-4


def test_cyclic_minibatch_forward_backward_and_objective(pkg):
    cfg, net = _net(pkg)
    T = cfg.frames_per_chunk // 3
    den = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(30, cfg.num_pdfs, mean_out_degree=4.0, seed=5))
    ds = pkg.hipabi.Supervision(pkg.synth.make_e2e_supervision(cfg.num_sequences, T, cfg.num_pdfs, units=(2, 6), seed=7, optional=[1]))
    f, v = _inputs(pkg, net, cfg, 100)
    r = host(net.forward_backward(f, v, den, ds, step=0)).copy()
    assert r[5] == 1.0 and np.isfinite(r[:7]).all() and r[2] == cfg.num_sequences * T
    assert host(net.grads.abs().sum()).item() > 0
    before = (host(net.params).copy(), host(net.grads).copy(), net.get_stats().copy())
    o = host(net.objective(f, v, den, ds)).copy()
    print("NET_E2E cyclic: forward_backward objf %.12g num %.12g den %.12g xent %.12g; objective() %.12g %.12g %.12g %.12g" % (r[0], r[3], r[4], r[6], o[0], o[3], o[4], o[6]))
    assert o[5] == 1.0 and abs(o[0] - r[0]) <= 1e-6 * abs(r[0])
    after = (host(net.params).copy(), host(net.grads).copy(), net.get_stats().copy())
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    assert np.array_equal(host(net.objective(f, v, den, ds)), o)
    net.close()


def test_three_natural_gradient_steps_twice_give_the_same_bits(pkg):
    out = []
    for _ in range(2):
        cfg, net = _net(pkg)
        T = cfg.frames_per_chunk // 3
        den = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(30, cfg.num_pdfs, mean_out_degree=4.0, seed=5))
        steps = []
        for i in range(3):
            ds = pkg.hipabi.Supervision(pkg.synth.make_e2e_supervision(cfg.num_sequences, T, cfg.num_pdfs, seed=300 + i))
            f, v = _inputs(pkg, net, cfg, 100 + i)
            steps.append(host(net.forward_backward(f, v, den, ds, step=i)).copy())
            net.update(1e-3, step=i)
        out.append((host(net.params).copy(), steps))
        net.close()
    (pa, sa), (pb, sb) = out
    assert all(s[5] == 1.0 for s in sa)
    assert np.array_equal(pa, pb)
    for a, b in zip(sa, sb):
        assert np.array_equal(a, b)
