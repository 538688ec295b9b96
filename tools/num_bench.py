#!/usr/bin/env python3
"""Stand-alone timing of the chain numerator on lattice supervisions (synth.make_supervision_lattice): the recursion and the two posterior
passes, the numerator's wide form (option num_form = 2) against the one-wave kernel (num_form = 1) in interleaved pairs; with --step, a whole
trainer step on the lattice against the same step on synth.make_supervision.
usage (GPU box): python tools/num_bench.py [--B 128] [--T 500] [--P 6034] [--tolerance 2] [--alternatives 1 4 16] [--pairs 5] [--step]"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=128)
ap.add_argument("--T", type=int, default=500)
ap.add_argument("--P", type=int, default=6034)
ap.add_argument("--tolerance", type=int, default=2)
ap.add_argument("--alternatives", type=int, nargs="+", default=[1, 4, 16])
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
ap.add_argument("--step", action="store_true", help="a whole trainer step (1500 frames per chunk x B) instead of the numerator alone")
args = ap.parse_args()

pkg = ge.load_package()
abi = pkg.hipabi
lib = abi.load()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def numerator(alts):
    B, T, P = args.B, args.T, args.P
    sup = pkg.synth.make_supervision_lattice(B, T, P, tolerance=args.tolerance, alternatives=alts, seed=2)
    den = pkg.synth.make_den_graph(64, P, mean_out_degree=4.0, seed=1)  # (the numerator takes the workspace layout from it, nothing else)
    with abi.option("num_form", 2):  # (so that a narrow supervision gets the wide form's tables too)
        dg, ds = abi.DenGraph(den), abi.Supervision(sup)
    info = ds.info()
    y = torch.randn(B * T, P, device="cuda")
    d, xd = torch.zeros_like(y), torch.zeros_like(y)
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    nb = lib.tdnnf_chain_workspace_bytes(dg.h, B, T)
    ws = abi.workspace(nb)
    ws.zero_()
    s = abi.stream()

    def part(k):
        return lambda: abi.check(lib.tdnnf_chain_numerator_part(dg.h, ds.h, abi.pmat(y), k, abi.ptr(res), abi.pmat(d), abi.pmat(xd), abi.ptr(ws), nb, s))

    print("B %d T %d P %d tolerance %d alternatives %d: %.1f states and %.1f arcs per frame, widest frame %d" % (
        B, T, P, args.tolerance, alts, info["num_states"] / (B * T), info["num_arcs"] / (B * T), info["max_states_per_frame"]))
    for name, k in (("recursion", 1), ("xent posteriors", 4), ("deriv posteriors + finish", 2)):
        ms = {1: [], 2: []}
        for _ in range(args.pairs):
            for form in (1, 2):
                with abi.option("num_form", form):
                    ms[form].append(timed(part(k), args.reps))
        ratio = [a / b for a, b in zip(ms[1], ms[2])]
        print("  %-26s num_form 1: %8.3f ms (%.3f .. %.3f)   num_form 2: %8.3f ms (%.3f .. %.3f)   old / new per pair %.2f .. %.2f" % (
            name, float(np.median(ms[1])), min(ms[1]), max(ms[1]), float(np.median(ms[2])), min(ms[2]), max(ms[2]), min(ratio), max(ratio)))


def step(alts):
    cfg = pkg.trainer.make_config(frames_per_chunk=3 * args.T, num_sequences=args.B, num_pdfs=args.P)
    net = pkg.trainer.ChainNet(cfg)
    net.set_params(net.init_params_numpy(seed=1, output_stddev=0.3))
    feats, iv = pkg.trainer.synthetic_egs(net, seed=2)
    fd, ivd = torch.from_numpy(feats).cuda(), torch.from_numpy(iv).cuda()
    dg = abi.DenGraph(pkg.synth.make_den_graph(4000, args.P, mean_out_degree=12.0, seed=1))
    sups = {"make_supervision": abi.Supervision(pkg.synth.make_supervision(args.B, args.T, args.P, seed=3))}
    for a in alts:
        sups["lattice x%d" % a] = abi.Supervision(pkg.synth.make_supervision_lattice(args.B, args.T, args.P, tolerance=args.tolerance, alternatives=a, seed=2))
    ms = {k: [] for k in sups}
    for _ in range(args.pairs):
        for k, ds in sups.items():
            def one():
                net.grads.zero_()
                net.forward_backward(fd, ivd, dg, ds, step=1)
            ms[k].append(timed(one, args.reps))
    for k, v in ms.items():
        print("step %d x %d, %-18s %.2f ms (%.2f .. %.2f), %.1f states per frame" % (3 * args.T, args.B, k + ":", float(np.median(v)), min(v), max(v),
                                                                                   sups[k].info()["num_states"] / (args.B * args.T)))
    net.close()


if args.step:
    step(args.alternatives)
else:
    for a in args.alternatives:
        numerator(a)
