#!/usr/bin/env python3
"""Objective-only evaluation against the training step's evaluation path: ms per call of ChainNet.objective and of
ChainNet.forward_backward on the same nets -- built with outer_loop.evaluation_config(cfg, True) (nnet3-chain-compute-prob: BatchNorm in
test mode) and evaluation_config(cfg, False) (nnet3-chain-combine: training mode) -- for the full-width 7q model (1536 hidden, 6034
pdfs, 4 000-state denominator graph) at 150 x 64 and 1500 x 128.  The two calls are timed in interleaved repeats; one process per
arithmetic.  Prints one JSON line with the ms pairs and tdnnf_chain_objf_workspace_bytes against tdnnf_chain_workspace_bytes at both shapes.
usage (GPU box): python tools/eval_bench.py [--gemm f32|f16x3] [--repeats R] [--calls K] [--shapes 150x64,1500x128]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402


def model_stats(cfg):
    """BatchNorm statistics of mean 0.3, variance 1 (and ReLU statistics) in tdnnf_net_get_stats order."""
    Hd, S, out = cfg.hidden_dim, cfg.prefinal_small_dim, []
    bn = lambda D: out.append(np.concatenate([[64.0], np.full(D, 64 * 0.3), np.full(D, 64 * 1.09)]))  # noqa: E731
    relu = lambda D: out.append(np.concatenate([[64.0], np.full(D, 10.0), np.full(D, 32.0), [0.0], np.zeros(D)]))  # noqa: E731
    for _ in range(cfg.num_layers + 1):
        bn(Hd), relu(Hd)
    for _ in range(2):
        bn(Hd), relu(Hd), bn(S)
    return np.concatenate(out)


def timed(fn, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gemm", default="f32", choices=["f32", "f16x3"])
    ap.add_argument("--repeats", type=int, default=3, help="interleaved repeats of (objective, forward_backward)")
    ap.add_argument("--calls", type=int, default=5, help="calls per timed repeat")
    ap.add_argument("--shapes", default="150x64,1500x128")
    ap.add_argument("--den-states", type=int, default=4000)
    ap.add_argument("--den-degree", type=float, default=12.0)
    args = ap.parse_args()
    pkg = ge.load_package()
    lib, T, o = pkg.hipabi.load(), pkg.trainer, pkg.outer_loop
    res = dict(metric="eval_7q_full_width", gemm=args.gemm, den_states=args.den_states, repeats=args.repeats, calls=args.calls)
    for shape in args.shapes.split(","):
        chunk, seqs = (int(v) for v in shape.split("x"))
        cfg = T.make_config(frames_per_chunk=chunk, num_sequences=seqs, gemm_precision=3 if args.gemm == "f16x3" else 0)
        den = pkg.synth.make_den_graph(args.den_states, cfg.num_pdfs, mean_out_degree=args.den_degree, seed=1)
        sup = pkg.hipabi.Supervision(pkg.synth.make_supervision_from_den(den, seqs, chunk // 3, num_paths=2, seed=2))
        dg = pkg.hipabi.DenGraph(den)
        item = dict(objf_workspace_bytes=int(lib.tdnnf_chain_objf_workspace_bytes(dg.h, seqs, chunk // 3)),
                    full_workspace_bytes=int(lib.tdnnf_chain_workspace_bytes(dg.h, seqs, chunk // 3)))
        for mode, test_mode in (("compute_prob", True), ("combine", False)):
            net = T.ChainNet(o.evaluation_config(cfg, test_mode))
            net.set_params(net.init_params_numpy(seed=0, output_stddev=0.05))
            net.set_stats(model_stats(cfg))
            feats, iv = T.synthetic_egs(net, seed=3)
            fd, ivd = torch.from_numpy(feats).cuda(), torch.from_numpy(iv).cuda()
            calls = {"objective": lambda: net.objective(fd, ivd, dg, sup), "forward_backward": lambda: net.forward_backward(fd, ivd, dg, sup, step=1)}
            for fn in calls.values():  # warm-up: allocations, first launches
                fn(), fn()
            torch.cuda.synchronize()
            ms = {k: [] for k in calls}
            for _ in range(args.repeats):
                for k, fn in calls.items():
                    ms[k].append(timed(fn, args.calls))
            r = net.objective(fd, ivd, dg, sup).cpu().numpy()
            item[mode] = dict(objective_ms=round(float(np.median(ms["objective"])), 3), forward_backward_ms=round(float(np.median(ms["forward_backward"])), 3),
                              objective_ms_all=[round(v, 3) for v in ms["objective"]], forward_backward_ms_all=[round(v, 3) for v in ms["forward_backward"]],
                              ok=float(r[5]))
            net.close()
        res[shape] = item
    print(json.dumps(res))


if __name__ == "__main__":
    main()
