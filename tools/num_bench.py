#!/usr/bin/env python3
"""Stand-alone timing of the chain numerator on lattice supervisions (synth.make_supervision_lattice): the recursion and the two posterior
passes, the numerator's wide form (option num_form = 2) against the one-wave kernel (num_form = 1) in interleaved pairs; with --step, a whole
trainer step on the lattice against the same step on synth.make_supervision.  With --e2e: parts 1, 4 and 2 of the numerator on an end-to-end
supervision (synth.make_e2e_supervision, 128 sequences x 150 output frames by default; --states N: graphs of N states -- transcripts of
N - 1 units, or the free path through an N-state denominator graph where N - 1 units would not fit the frames), beside the same parts on an
alignment supervision of the same B and T and tdnnf_align_posteriors on the same graphs with row_stride = B (what a caller could run
before the end-to-end supervision existed), interleaved.
usage (GPU box): python tools/num_bench.py [--B 128] [--T 500] [--P 6034] [--tolerance 2] [--alternatives 1 4 16] [--pairs 5] [--step]
                 python tools/num_bench.py --e2e [--states N] [--B 128] [--T 150] [--P 6034] [--pairs 5]"""
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
ap.add_argument("--T", type=int, default=None, help="output frames per sequence (default 500; 150 with --e2e)")
ap.add_argument("--P", type=int, default=6034)
ap.add_argument("--tolerance", type=int, default=2)
ap.add_argument("--alternatives", type=int, nargs="+", default=[1, 4, 16])
ap.add_argument("--pairs", type=int, default=5)
ap.add_argument("--reps", type=int, default=5, help="calls per timed window")
ap.add_argument("--step", action="store_true", help="a whole trainer step (1500 frames per chunk x B) instead of the numerator alone")
ap.add_argument("--e2e", action="store_true", help="the end-to-end numerator's three parts beside an alignment supervision's and tdnnf_align_posteriors")
ap.add_argument("--states", type=int, default=0, help="--e2e: states per graph (default: transcripts of 40 .. 100 units)")
args = ap.parse_args()
if args.T is None:
    args.T = 150 if args.e2e else 500

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


def e2e():
    B, T, P = args.B, args.T, args.P
    if args.states and args.states - 1 > T:
        g = pkg.synth.alignment_graph_from_den(pkg.synth.make_den_graph(args.states, P, mean_out_degree=12.0, seed=1))
        sup = {"B": B, "T": T, "P": P, "weight": 1.0, "graphs": [g] * B}
    else:
        units = (args.states - 1, args.states - 1) if args.states else (40, 100)
        sup = pkg.synth.make_e2e_supervision(B, T, P, units=units, seed=2)
    den = pkg.synth.make_den_graph(64, P, mean_out_degree=4.0, seed=1)  # (the numerator takes the workspace layout from it, nothing else)
    dg, de, da = abi.DenGraph(den), abi.Supervision(sup), abi.Supervision(pkg.synth.make_supervision(B, T, P, seed=3))
    graphs = abi.AlignGraphs(sup["graphs"], num_pdfs=P)
    info, form = de.info(), de.e2e_form()
    y = torch.randn(B * T, P, device="cuda")
    d, xd, post = torch.zeros_like(y), torch.zeros_like(y), torch.zeros_like(y)
    res = torch.zeros(8, dtype=torch.float64, device="cuda")
    nb = lib.tdnnf_chain_workspace_bytes(dg.h, B, T)
    ws = abi.workspace(nb)
    ws.zero_()
    s = abi.stream()
    frames, (rows, rows_p) = abi.iarr([T] * B), abi.iarr(np.arange(B))
    nbp = graphs.posteriors_workspace_bytes(None, frames[0])
    wsp, resp = abi.workspace(nbp), torch.zeros((B, 2), dtype=torch.float64, device="cuda")

    def part(ds, k):
        return lambda: abi.check(lib.tdnnf_chain_numerator_part(dg.h, ds.h, abi.pmat(y), k, abi.ptr(res), abi.pmat(d), abi.pmat(xd), abi.ptr(ws), nb, s))

    def align_posteriors():
        abi.check(lib.tdnnf_align_posteriors(graphs.h, B, None, frames[1], rows_p, B, abi.pmat(y), 1.0, 1.0, abi.pmat(post), abi.ptr(resp), abi.ptr(wsp), nbp, s))

    print("e2e B %d T %d P %d: %.1f states and %.1f arcs per graph, largest graph %d states; recursion form %r; scratch %.1f MB" % (
        B, T, P, info["num_states"] / B, info["num_arcs"] / B, info["max_states_per_frame"], form, 16e-6 * (T + 1) * info["num_states"]))
    runs = [("e2e part %d" % k, part(de, k)) for k in (1, 4, 2)] + [("alignment part %d" % k, part(da, k)) for k in (1, 4, 2)]
    runs.append(("tdnnf_align_posteriors", align_posteriors))
    ms = {name: [] for name, _ in runs}
    for _ in range(args.pairs):  # interleaved: every round times every entry once
        for name, fn in runs:
            ms[name].append(timed(fn, args.reps))
    for name, _ in runs:
        v = ms[name]
        print("  %-24s %8.3f ms (%.3f .. %.3f)" % (name, float(np.median(v)), min(v), max(v)))
    tot = lambda who: sum(float(np.median(ms["%s part %d" % (who, k)])) for k in (1, 4, 2))
    print("  parts 1 + 4 + 2: e2e %.3f ms, alignment %.3f ms; tdnnf_align_posteriors %.3f ms" % (tot("e2e"), tot("alignment"), float(np.median(ms["tdnnf_align_posteriors"]))))


if args.e2e:
    e2e()
elif args.step:
    step(args.alternatives)
else:
    for a in args.alternatives:
        numerator(a)
