"""-m gpu: the split form's occupancy pass, one (frame, sequence) per workgroup (option den_gamma_pairs = 1, den_gamma_kernel) against
two frames per workgroup (den_gamma_pairs = 0, den_gamma2_kernel where both frames' vectors fit the LDS).  The two must agree bit for bit:
the derivative, the results vector and, through a whole training step, the gradient buffer."""
import numpy as np
import pytest
import torch

from tests.gpu_util import Hip, dev, host, padded

pytestmark = pytest.mark.gpu


def _objf_and_deriv(pkg, hip, g, sup, y, B, T, pairs):
    dg, ds = pkg.hipabi.DenGraph(g), pkg.hipabi.Supervision(sup)
    nb = hip.chain_workspace_bytes(dg.h, B, T)
    ws = hip.ws(nb)
    ws.fill_(float("nan"))
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    dd = torch.full_like(y, 5.0)
    with pkg.hipabi.option("den_gamma_pairs", pairs):
        hip.chain_objf_and_deriv(dg.h, ds.h, y, None, 0.1, 0.0, 0.1, hip.vec(res), dd, None, hip.vec(ws), nb, hip.stream())
    torch.cuda.synchronize()
    return res, dd


# (states, pdfs, sequences, frames): the bench's shape; an odd number of frames and sequences (the last workgroup has one frame); pdfs = 1 mod 4;
# 10 000 states (two frames' vectors do not fit the LDS: den_gamma_kernel either way)
@pytest.mark.parametrize("H,P,B,T", [(4000, 6034, 128, 500), (500, 300, 3, 37), (1200, 1001, 5, 21), (10000, 6034, 8, 20)],
                         ids=["bench-4000x6034-128x500", "odd-3x37", "pdfs-1-mod-4", "swbd-10000"])
def test_occupancy_pass_two_frames_per_workgroup_is_bit_identical(pkg, H, P, B, T):
    hip = Hip(pkg)
    g = pkg.synth.make_den_graph(H, P, mean_out_degree=12.0 if P == 6034 else 6.0, seed=H)
    sup = pkg.synth.make_supervision_from_den(g, B, T, num_paths=2, seed=3)
    gen = torch.Generator(device="cuda").manual_seed(H + T)
    y = torch.randn(T * B, P, device="cuda", generator=gen) * 1.5
    if B * T < 1000:  # (a row stride beyond the pdfs, as a sub-matrix has)
        y, _ = padded(host(y))
    r1, d1 = _objf_and_deriv(pkg, hip, g, sup, y, B, T, 1)
    r0, d0 = _objf_and_deriv(pkg, hip, g, sup, y, B, T, 0)
    assert host(r1)[5] == 1.0 and torch.isfinite(d1).all()
    assert torch.equal(r0, r1), (host(r0), host(r1))
    diff = d0.view(torch.int32) != d1.view(torch.int32)
    assert not diff.any(), "%d of %d elements differ, in %d rows" % (int(diff.sum()), diff.numel(), int(diff.any(1).sum()))


def test_training_step_gradients_are_bit_identical(pkg):
    T = pkg.trainer
    kw = dict(frames_per_chunk=30, num_sequences=8, strides=[1, 1, 0, 3, 3], bottleneck=16, feat_dim=8, ivector_dim=4, hidden_dim=64, small_dim=32,
              num_pdfs=301, use_natural_gradient=1, use_dropout=0)

    def run(pairs):
        with pkg.hipabi.option("den_gamma_pairs", pairs):
            cfg = T.make_config(**kw)
            net = T.ChainNet(cfg)
            net.set_params(net.init_params_numpy(seed=1, output_stddev=0.1))
            den = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(400, cfg.num_pdfs, mean_out_degree=6.0, seed=5))
            out = []
            for i in range(3):
                feats, iv = T.synthetic_egs(net, seed=100 + i)
                sup = pkg.hipabi.Supervision(pkg.synth.make_supervision(cfg.num_sequences, cfg.frames_per_chunk // 3, cfg.num_pdfs, seed=200 + i))
                r = host(net.forward_backward(dev(feats), dev(iv), den, sup, step=i))
                out.append((host(net.grads).copy(), r.copy()))
                net.update(1e-3, step=i)
            net.close()
            return out

    one, two = run(1), run(0)
    for (ga, ra), (gb, rb) in zip(one, two):
        assert ra[5] == 1.0 and np.array_equal(ra, rb), (ra, rb)
        assert np.array_equal(ga.view(np.int32), gb.view(np.int32)), "%d elements differ" % int((ga != gb).sum())
