#!/usr/bin/env python3
"""Timing of best-path alignment (tdnnf_align_best_path) in its two uses:
  forced  64 utterances x 500 frames, each on its own transcript graph of a few hundred states (synth.make_alignment_graph);
  free    128 utterances x 500 frames sharing the bench's 4 000-state / 48 k-arc denominator graph.
Prints ms per call and us per frame (ms / frames of one utterance: the utterances run side by side, one workgroup each) for both, and
for the free decode the yardstick: tdnnf_chain_objf on the same graph and shape -- the denominator's forward recursion (the same
per-frame gather with a sum in float, no back-pointer) with the numerator's recursion beside it -- and the ratio.  One JSON line.
--posteriors: instead of the yardstick, forward-backward (tdnnf_align_posteriors) on the same two workloads and the same data, with the
posterior matrix ("posteriors") and without ("logprob": the forward recursion alone), timed INTERLEAVED with the best path (one
repeat of each after the other), and the two ratios to the best path.
--posteriors --compact: the compact call (tdnnf_align_posteriors_compact) joins that interleaved round, and for both output forms the time
from the finished device result to host-side per-frame (pdf-ids, posteriors) lists -- the copy and the sparsification ("to_lists_ms": the
dense form copies frames x num_pdfs floats and searches every row, the compact form frames x D and maps columns to pdfs); the lists of the
two forms are compared, ids and bits.
--posteriors --sparse [--min-post X --max-per-frame K]: the compact and the sparse call (tdnnf_align_posteriors_sparse: the compact pass
into the workspace, then the selection of at most K pairs above X a frame) join the interleaved round, and for both the time from the
finished device result to host-side per-frame (pdf-ids, posteriors) lists of the entries above X: the compact form copies frames x D
floats and searches every row, the sparse form copies frames x K pairs and their counts and slices.  Where no frame was truncated the lists
are compared, ids and bits.
--labels unit|arc: the graphs carry labels (synth.make_alignment_graph's: the unit an arc enters, or the arc's index; on the denominator
graph the state an arc enters, or the arc's index) and the labelled call joins the interleaved round beside its pdf counterpart, with the
ratio to it: tdnnf_align_best_path_labels beside the best path (without --posteriors), tdnnf_align_label_posteriors_compact beside the
compact call (--posteriors --compact), tdnnf_align_label_posteriors_sparse beside the sparse call (--posteriors --sparse).  With
--labels arc the free workload has 64 utterances, not 128: the label block of 128 would pass the compact call's 8 GiB limit.
--checkpoint C (with --posteriors --compact or --posteriors --sparse): the compact (sparse) call under option align_checkpoint = C -- alpha of
every C-th frame only, -1 for ceil(sqrt(frames)) -- joins the interleaved round beside the full call, in the workspace the option asks for;
the JSON gains both workspace sizes, the time ratio and whether the bits agree.  A third workload, "long": 4 utterances of 20 000 frames,
each on its own transcript graph of some 3 000 states, through the compact call.  Without --checkpoint (or with 0) it reports the bytes it
would need and is skipped; with it, it runs in the checkpointed workspace.
--path-checkpoint C (the best path alone: without --posteriors and --labels): both workloads also run under option
align_path_checkpoint = C -- back-pointers of C frames at a time, -1 for ceil(sqrt(frames)) -- INTERLEAVED with the option-0 call in one
process (one repeat of each after the other, medians of --repeats), in the workspace the option asks for; the JSON gains both workspace
sizes, the time ratio and whether pdf_out and the results are equal.  A third workload, "long": the 4 utterances of 20 000 frames of
--checkpoint's long case through the best path.  Without --path-checkpoint (or with 0) it reports the bytes it would need and is skipped;
with it, it runs in the checkpointed workspace and reports ms and us per frame.
usage (GPU box): python tools/align_bench.py [--repeats R] [--calls K] [--pdfs P] [--form 0|1|2] [--posteriors [--compact | --sparse]]
                                             [--labels unit|arc] [--checkpoint C] [--path-checkpoint C]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402


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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--pdfs", type=int, default=6034)
    ap.add_argument("--form", type=int, default=0, help="option align_form")
    ap.add_argument("--posteriors", action="store_true", help="time tdnnf_align_posteriors beside the best path")
    ap.add_argument("--compact", action="store_true", help="with --posteriors: time tdnnf_align_posteriors_compact and the way to host-side lists as well")
    ap.add_argument("--sparse", action="store_true", help="with --posteriors: time the compact and the sparse call and their ways to host-side lists")
    ap.add_argument("--min-post", type=float, default=0.01, help="--sparse: the floor")
    ap.add_argument("--max-per-frame", type=int, default=16, help="--sparse: pairs a frame")
    ap.add_argument("--labels", choices=["unit", "arc"], help="labelled graphs: time the labelled call beside its pdf counterpart")
    ap.add_argument("--checkpoint", type=int, help="with --posteriors --compact | --sparse: option align_checkpoint for a second compact (sparse) call")
    ap.add_argument("--path-checkpoint", type=int, help="the best path alone: option align_path_checkpoint for a second best-path call, and the long workload")
    args = ap.parse_args()
    if args.path_checkpoint is not None and (args.posteriors or args.labels):
        ap.error("--path-checkpoint goes with the best path alone")
    if args.checkpoint is not None and not (args.compact or args.sparse):
        ap.error("--checkpoint goes with --posteriors --compact or --posteriors --sparse")
    if args.labels and args.posteriors and not (args.compact or args.sparse):
        ap.error("--labels goes with the best path, with --posteriors --compact or with --posteriors --sparse")
    if (args.compact or args.sparse) and not args.posteriors:
        ap.error("--compact and --sparse go with --posteriors")
    if args.compact and args.sparse:
        ap.error("--compact or --sparse")
    pkg = ge.load_package()
    abi = pkg.hipabi
    lib = abi.load()
    abi.check(lib.tdnnf_set_option(b"align_form", args.form))
    P, T = args.pdfs, 500
    rng = np.random.default_rng(0)
    res = dict(metric="align_best_path", pdfs=P, frames=T, form=args.form, repeats=args.repeats, calls=args.calls)

    def case(ag, B, utt_graph):
        y = torch.randn(B * T, P, device="cuda")
        frames, rows = abi.iarr([T] * B), abi.iarr(np.arange(B) * T)
        ug = abi.iarr(utt_graph)
        nb = int(lib.tdnnf_align_workspace_bytes(ag.h, B, ug[1], frames[1]))
        ws = abi.workspace(nb)
        pdfs = torch.zeros(B * T, dtype=torch.int32, device="cuda")
        out = torch.zeros(B, 2, dtype=torch.float64, device="cuda")
        s = abi.stream()

        def run():
            abi.check(lib.tdnnf_align_best_path(ag.h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, abi.ptr(pdfs), None, abi.ptr(out), abi.ptr(ws), nb, s))

        run(), run()
        torch.cuda.synchronize()
        if args.posteriors:
            return y, posteriors_case(ag, B, y, frames, rows, ug, run, out)
        if args.path_checkpoint is not None:
            with abi.option("align_path_checkpoint", args.path_checkpoint):
                nb_k = int(lib.tdnnf_align_workspace_bytes(ag.h, B, ug[1], frames[1]))
            ws_k = abi.workspace(nb_k)
            pdfs_k = torch.zeros(B * T, dtype=torch.int32, device="cuda")
            out_k = torch.zeros(B, 2, dtype=torch.float64, device="cuda")

            def run_checkpoint():
                with abi.option("align_path_checkpoint", args.path_checkpoint):
                    abi.check(lib.tdnnf_align_best_path(ag.h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, abi.ptr(pdfs_k), None, abi.ptr(out_k),
                                                        abi.ptr(ws_k), nb_k, s))

            run_checkpoint(), run_checkpoint()
            torch.cuda.synchronize()
            ms, ms_k = [], []
            for _ in range(args.repeats):
                ms.append(timed(run, args.calls))
                ms_k.append(timed(run_checkpoint, args.calls))
            r = out.cpu().numpy()
            d = dict(utterances=B, workspace_bytes=nb, ms=round(float(np.median(ms)), 3), ms_all=[round(v, 3) for v in ms],
                     us_per_frame=round(1e3 * float(np.median(ms)) / T, 3), ok=int(r[:, 1].sum()), path_checkpoint=args.path_checkpoint,
                     workspace_bytes_checkpoint=nb_k,
                     best_path_checkpoint=dict(ms=round(float(np.median(ms_k)), 3), ms_all=[round(v, 3) for v in ms_k],
                                               us_per_frame=round(1e3 * float(np.median(ms_k)) / T, 3)))
            d["checkpoint_over_best_path"] = round(d["best_path_checkpoint"]["ms"] / d["ms"], 3)
            d["checkpoint_equal"] = bool(torch.equal(pdfs_k, pdfs) and torch.equal(out_k.view(torch.int64), out.view(torch.int64)))
            return y, d
        if args.labels:
            labels = torch.zeros(B * T, dtype=torch.int32, device="cuda")
            arcs = torch.zeros(B * T, dtype=torch.int32, device="cuda")

            def run_labels():
                abi.check(lib.tdnnf_align_best_path_labels(ag.h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, abi.ptr(pdfs), None, abi.ptr(labels),
                                                           abi.ptr(arcs), abi.ptr(out), abi.ptr(ws), nb, s))

            run_labels(), run_labels()
            torch.cuda.synchronize()
            ms, ms_l = [], []
            for _ in range(args.repeats):
                ms.append(timed(run, args.calls))
                ms_l.append(timed(run_labels, args.calls))
        else:
            ms = [timed(run, args.calls) for _ in range(args.repeats)]
        r = out.cpu().numpy()
        d = dict(utterances=B, workspace_bytes=nb, ms=round(float(np.median(ms)), 3), ms_all=[round(v, 3) for v in ms],
                 us_per_frame=round(1e3 * float(np.median(ms)) / T, 3), ok=int(r[:, 1].sum()))
        if args.labels:
            d["best_path_labels"] = dict(ms=round(float(np.median(ms_l)), 3), ms_all=[round(v, 3) for v in ms_l])
            d["labels_over_best_path"] = round(d["best_path_labels"]["ms"] / d["ms"], 3)
        return y, d

    def posteriors_case(ag, B, y, frames, rows, ug, best_path, bp_out):
        nb = [int(lib.tdnnf_align_posteriors_workspace_bytes(ag.h, B, ug[1], frames[1], want)) for want in (0, 1)]
        ws = abi.workspace(nb[1])
        post = torch.zeros(B * T, P, device="cuda")
        out = torch.zeros(B, 2, dtype=torch.float64, device="cuda")
        s = abi.stream()

        def full():
            abi.check(lib.tdnnf_align_posteriors(ag.h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, 1.0, abi.pmat(post), abi.ptr(out), abi.ptr(ws), nb[1], s))

        def forward():
            abi.check(lib.tdnnf_align_posteriors(ag.h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, 1.0, None, abi.ptr(out), abi.ptr(ws), nb[0], s))

        fns = dict(best_path=best_path, posteriors=full, logprob=forward)
        if args.sparse:
            return sparse_case(ag, B, y, frames, rows, ug, ws, nb[1], fns)
        if args.compact:
            begin = ag.posteriors_compact_layout(frames[0], ug[0])
            elems = int(begin[-1])
            values = torch.zeros(elems, device="cuda")
            out_c = torch.zeros(B, 2, dtype=torch.float64, device="cuda")

            def compact():
                abi.check(lib.tdnnf_align_posteriors_compact(ag.h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, 1.0, abi.ptr(values), elems, abi.ptr(out_c),
                                                             abi.ptr(ws), nb[1], s))

            fns["posteriors_compact"] = compact
            if args.checkpoint is not None:
                with abi.option("align_checkpoint", args.checkpoint):
                    nb_k = int(lib.tdnnf_align_posteriors_workspace_bytes(ag.h, B, ug[1], frames[1], 1))
                values_k = torch.zeros(elems, device="cuda")
                out_k = torch.zeros(B, 2, dtype=torch.float64, device="cuda")

                def compact_checkpoint():
                    with abi.option("align_checkpoint", args.checkpoint):
                        abi.check(lib.tdnnf_align_posteriors_compact(ag.h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, 1.0, abi.ptr(values_k), elems,
                                                                     abi.ptr(out_k), abi.ptr(ws), nb_k, s))

                fns["posteriors_compact_checkpoint"] = compact_checkpoint
            if args.labels:
                lbegin = ag.label_posteriors_compact_layout(frames[0], ug[0])
                lelems = int(lbegin[-1])
                lvalues = torch.zeros(lelems, device="cuda")
                out_l = torch.zeros(B, 2, dtype=torch.float64, device="cuda")

                def label_compact():
                    abi.check(lib.tdnnf_align_label_posteriors_compact(ag.h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, 1.0, abi.ptr(lvalues), lelems,
                                                                       abi.ptr(out_l), abi.ptr(ws), nb[1], s))

                fns["label_posteriors_compact"] = label_compact
        for fn in fns.values():
            fn(), fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                ms[k].append(timed(fn, args.calls))
        full()
        r, rb = out.cpu().numpy(), bp_out.cpu().numpy()
        d = dict(utterances=B, workspace_bytes=nb[1], workspace_bytes_logprob=nb[0], ok=int(r[:, 1].sum()),
                 logprob_minus_best_path_min=round(float((r[:, 0] - rb[:, 0]).min()), 3),
                 row_sum_err=float((post.sum(1, dtype=torch.float64) - 1.0).abs().max()))
        for k, v in ms.items():
            d[k] = dict(ms=round(float(np.median(v)), 3), ms_all=[round(x, 3) for x in v], us_per_frame=round(1e3 * float(np.median(v)) / T, 3))
        d["posteriors_over_best_path"] = round(d["posteriors"]["ms"] / d["best_path"]["ms"], 3)
        d["logprob_over_best_path"] = round(d["logprob"]["ms"] / d["best_path"]["ms"], 3)
        if args.compact:
            d["compact_over_posteriors"] = round(d["posteriors_compact"]["ms"] / d["posteriors"]["ms"], 3)
            d["output_bytes"] = dict(posteriors=4 * post.numel(), posteriors_compact=4 * elems)
            if args.checkpoint is not None:
                d["checkpoint"] = args.checkpoint
                d["workspace_bytes_checkpoint"] = nb_k
                d["checkpoint_over_compact"] = round(d["posteriors_compact_checkpoint"]["ms"] / d["posteriors_compact"]["ms"], 3)
                d["checkpoint_same_bits"] = bool(torch.equal(values_k.view(torch.int32), values.view(torch.int32))
                                                 and torch.equal(out_k.view(torch.int64), out_c.view(torch.int64)))
            if args.labels:
                d["label_over_compact"] = round(d["label_posteriors_compact"]["ms"] / d["posteriors_compact"]["ms"], 3)
                d["output_bytes"]["label_posteriors_compact"] = 4 * lelems
                d["label_row_sum_err"] = float(max((lvalues[int(lbegin[u]):int(lbegin[u + 1])].view(T, -1).sum(1, dtype=torch.float64) - 1.0).abs().max()
                                                   for u in range(B)))
                assert np.array_equal(out_l.cpu().numpy().view(np.int64), out_c.cpu().numpy().view(np.int64)), "logprob / ok differ between pdfs and labels"
            lists_of = [ag.pdfs(int(gi)) for gi in ug[0]]

            def dense_lists():
                m = post.cpu().numpy()
                return [(ids, row[ids]) for row in m for ids in (np.nonzero(row > 0)[0],)]

            def compact_lists():
                v, res = values.cpu().numpy(), []
                for u in range(B):
                    m = v[begin[u]:begin[u + 1]].reshape(T, -1)
                    res += [(lists_of[u][ids], row[ids]) for row in m for ids in (np.nonzero(row > 0)[0],)]
                return res

            compact()
            torch.cuda.synchronize()
            to_lists = dict(posteriors=[], posteriors_compact=[])
            for _ in range(args.repeats):
                for k, fn in (("posteriors", dense_lists), ("posteriors_compact", compact_lists)):
                    t0 = time.perf_counter()
                    got = fn()
                    to_lists[k].append(1e3 * (time.perf_counter() - t0))
                    if k == "posteriors":
                        want = got
                    else:
                        assert len(got) == len(want) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
                                                             for a, b in zip(got, want)), "the two forms give different lists"
            for k, v in to_lists.items():
                d[k]["to_lists_ms"] = round(float(np.median(v)), 1)
                d[k]["to_lists_ms_all"] = [round(x, 1) for x in v]
            assert np.array_equal(out_c.cpu().numpy().view(np.int64), r.view(np.int64)), "logprob / ok differ between the forms"
            d["pairs"] = int(sum(len(a[0]) for a in want))
        return d

    def sparse_case(ag, B, y, frames, rows, ug, ws, nb, fns):
        K, floor = args.max_per_frame, np.float32(args.min_post)
        begin = ag.posteriors_compact_layout(frames[0], ug[0])
        elems = int(begin[-1])
        values = torch.zeros(elems, device="cuda")
        out_c = torch.zeros(B, 2, dtype=torch.float64, device="cuda")
        nbs = int(lib.tdnnf_align_posteriors_sparse_workspace_bytes(ag.h, B, ug[1], frames[1], K))
        wss = abi.workspace(nbs)
        pdf = torch.zeros(B * T, K, dtype=torch.int32, device="cuda")
        post = torch.zeros(B * T, K, device="cuda")
        count = torch.zeros(B * T, dtype=torch.int32, device="cuda")
        out_s = torch.zeros(B, 4, dtype=torch.float64, device="cuda")
        s = abi.stream()

        def compact():
            abi.check(lib.tdnnf_align_posteriors_compact(ag.h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, 1.0, abi.ptr(values), elems, abi.ptr(out_c),
                                                         abi.ptr(ws), nb, s))

        def sparse():
            abi.check(lib.tdnnf_align_posteriors_sparse(ag.h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, 1.0, float(floor), K, abi.ptr(pdf), abi.ptr(post),
                                                        abi.ptr(count), abi.ptr(out_s), abi.ptr(wss), nbs, s))

        fns = dict(best_path=fns["best_path"], posteriors_compact=compact, posteriors_sparse=sparse)
        if args.checkpoint is not None:
            with abi.option("align_checkpoint", args.checkpoint):
                nbs_k = int(lib.tdnnf_align_posteriors_sparse_workspace_bytes(ag.h, B, ug[1], frames[1], K))
            pdf_k, post_k = torch.zeros(B * T, K, dtype=torch.int32, device="cuda"), torch.zeros(B * T, K, device="cuda")
            count_k, out_k = torch.zeros(B * T, dtype=torch.int32, device="cuda"), torch.zeros(B, 4, dtype=torch.float64, device="cuda")

            def sparse_checkpoint():
                with abi.option("align_checkpoint", args.checkpoint):
                    abi.check(lib.tdnnf_align_posteriors_sparse(ag.h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, 1.0, float(floor), K, abi.ptr(pdf_k),
                                                                abi.ptr(post_k), abi.ptr(count_k), abi.ptr(out_k), abi.ptr(wss), nbs_k, s))

            fns["posteriors_sparse_checkpoint"] = sparse_checkpoint
        if args.labels:
            nbl = int(lib.tdnnf_align_label_posteriors_sparse_workspace_bytes(ag.h, B, ug[1], frames[1], K))
            wsl = abi.workspace(nbl)
            lab, lpost = torch.zeros(B * T, K, dtype=torch.int32, device="cuda"), torch.zeros(B * T, K, device="cuda")
            lcount, out_l = torch.zeros(B * T, dtype=torch.int32, device="cuda"), torch.zeros(B, 4, dtype=torch.float64, device="cuda")

            def label_sparse():
                abi.check(lib.tdnnf_align_label_posteriors_sparse(ag.h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, 1.0, float(floor), K, abi.ptr(lab),
                                                                  abi.ptr(lpost), abi.ptr(lcount), abi.ptr(out_l), abi.ptr(wsl), nbl, s))

            fns["label_posteriors_sparse"] = label_sparse
        for fn in fns.values():
            fn(), fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in fns}
        for _ in range(args.repeats):
            for k, fn in fns.items():
                ms[k].append(timed(fn, args.calls))
        rs = out_s.cpu().numpy()
        d = dict(utterances=B, min_post=float(floor), max_per_frame=K, workspace_bytes=dict(posteriors_compact=nb, posteriors_sparse=nbs), ok=int(rs[:, 1].sum()),
                 truncated_frames=int(rs[:, 2].sum()), most_candidates=int(rs[:, 3].max()))
        for k, v in ms.items():
            d[k] = dict(ms=round(float(np.median(v)), 3), ms_all=[round(x, 3) for x in v], us_per_frame=round(1e3 * float(np.median(v)) / T, 3))
        if args.checkpoint is not None:
            d["checkpoint"] = args.checkpoint
            d["workspace_bytes"]["posteriors_sparse_checkpoint"] = nbs_k
            d["checkpoint_over_sparse"] = round(d["posteriors_sparse_checkpoint"]["ms"] / d["posteriors_sparse"]["ms"], 3)
            d["checkpoint_same_bits"] = bool(torch.equal(pdf_k, pdf) and torch.equal(post_k.view(torch.int32), post.view(torch.int32))
                                             and torch.equal(count_k, count) and torch.equal(out_k.view(torch.int64), out_s.view(torch.int64)))
        d["selection_ms"] = round(d["posteriors_sparse"]["ms"] - d["posteriors_compact"]["ms"], 3)
        d["sparse_over_compact"] = round(d["posteriors_sparse"]["ms"] / d["posteriors_compact"]["ms"], 3)
        if args.labels:
            rl = out_l.cpu().numpy()
            d["label_sparse_over_sparse"] = round(d["label_posteriors_sparse"]["ms"] / d["posteriors_sparse"]["ms"], 3)
            d["label_sparse"] = dict(workspace_bytes=nbl, truncated_frames=int(rl[:, 2].sum()), most_candidates=int(rl[:, 3].max()), pairs=int(lcount.sum().item()))
        d["output_bytes"] = dict(posteriors_compact=4 * elems, posteriors_sparse=B * T * (8 * K + 4))
        lists_of = [ag.pdfs(int(gi)) for gi in ug[0]]

        def compact_lists():
            v, res = values.cpu().numpy(), []
            for u in range(B):
                m = v[begin[u]:begin[u + 1]].reshape(T, -1)
                res += [(lists_of[u][ids], row[ids]) for row in m for ids in (np.nonzero(row > floor)[0],)]
            return res

        def sparse_lists():
            p, v, c = pdf.cpu().numpy(), post.cpu().numpy(), count.cpu().numpy()
            return [(p[f, :n], v[f, :n]) for f, n in enumerate(c.tolist())]

        to_lists = dict(posteriors_compact=[], posteriors_sparse=[])
        for _ in range(args.repeats):
            for k, fn in (("posteriors_compact", compact_lists), ("posteriors_sparse", sparse_lists)):
                t0 = time.perf_counter()
                got = fn()
                to_lists[k].append(1e3 * (time.perf_counter() - t0))
                if k == "posteriors_compact":
                    want = got
                elif d["truncated_frames"] == 0:
                    assert len(got) == len(want) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
                                                         for a, b in zip(got, want)), "the two forms give different lists"
        for k, v in to_lists.items():
            d[k]["to_lists_ms"] = round(float(np.median(v)), 1)
            d[k]["to_lists_ms_all"] = [round(x, 1) for x in v]
        assert np.array_equal(out_c.cpu().numpy().view(np.int64), np.ascontiguousarray(rs[:, :2]).view(np.int64)), "logprob / ok differ between the forms"
        d["pairs"] = dict(posteriors_compact=int(sum(len(a[0]) for a in want)), posteriors_sparse=int(count.sum().item()))
        return d

    def long_graphs(B):
        """B transcript graphs of 1 200 units with optional units and alternative branches: some 3 000 states each"""
        lrng = np.random.default_rng(1)
        lgraphs = [pkg.synth.make_alignment_graph(lrng.integers(0, P, size=1200).tolist(), optional=list(range(5, 1200, 10)),
                                                  alternatives={k: lrng.integers(0, P, size=12).tolist() for k in range(3, 1200, 8)}, num_pdfs=P, seed=u)
                   for u in range(B)]
        return abi.AlignGraphs(lgraphs, num_pdfs=P)

    def long_path_case():
        """4 utterances of 20 000 frames, each on its own graph of long_graphs, through the best path: what a back-pointer per (frame,
        state) would need, and -- under --path-checkpoint -- the call in the checkpointed workspace"""
        B, TL = 4, 20000
        lag = long_graphs(B)
        frames, rows, ug = abi.iarr([TL] * B), abi.iarr(np.arange(B) * TL), abi.iarr(np.arange(B))
        nb0 = int(lib.tdnnf_align_workspace_bytes(lag.h, B, ug[1], frames[1]))
        d = dict(utterances=B, frames=TL, states_per_graph=int(np.mean(lag.num_states)), workspace_bytes=nb0)
        if not args.path_checkpoint:
            d["skipped"] = "a back-pointer per (frame, state): %d bytes of workspace; run with --path-checkpoint" % nb0
            return d
        with abi.option("align_path_checkpoint", args.path_checkpoint):
            nb_k = int(lib.tdnnf_align_workspace_bytes(lag.h, B, ug[1], frames[1]))
        y = torch.randn(B * TL, P, device="cuda")
        ws = abi.workspace(nb_k)
        pdfs = torch.zeros(B * TL, dtype=torch.int32, device="cuda")
        out = torch.zeros(B, 2, dtype=torch.float64, device="cuda")
        s = abi.stream()

        def run_checkpoint():
            with abi.option("align_path_checkpoint", args.path_checkpoint):
                abi.check(lib.tdnnf_align_best_path(lag.h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, abi.ptr(pdfs), None, abi.ptr(out), abi.ptr(ws),
                                                    nb_k, s))

        run_checkpoint()
        torch.cuda.synchronize()
        ms = [timed(run_checkpoint, args.calls) for _ in range(args.repeats)]
        r = out.cpu().numpy()
        d.update(path_checkpoint=args.path_checkpoint, workspace_bytes_checkpoint=nb_k, ok=int(r[:, 1].sum()),
                 best_path_checkpoint=dict(ms=round(float(np.median(ms)), 3), ms_all=[round(v, 3) for v in ms],
                                           us_per_frame=round(1e3 * float(np.median(ms)) / TL, 3)))
        return d

    def long_case():
        """4 utterances of 20 000 frames, each on its own graph of long_graphs, through the compact call: what alpha of every frame
        would need, and -- under --checkpoint -- the call in the checkpointed workspace"""
        B, TL = 4, 20000
        lag = long_graphs(B)
        frames, rows, ug = abi.iarr([TL] * B), abi.iarr(np.arange(B) * TL), abi.iarr(np.arange(B))
        nb0 = int(lib.tdnnf_align_posteriors_workspace_bytes(lag.h, B, ug[1], frames[1], 1))
        d = dict(utterances=B, frames=TL, states_per_graph=int(np.mean(lag.num_states)), workspace_bytes=nb0)
        if not args.checkpoint:
            d["skipped"] = "alpha of every frame: %d bytes of workspace; run with --checkpoint" % nb0
            return d
        with abi.option("align_checkpoint", args.checkpoint):
            nb_k = int(lib.tdnnf_align_posteriors_workspace_bytes(lag.h, B, ug[1], frames[1], 1))
        y = torch.randn(B * TL, P, device="cuda")
        ws = abi.workspace(nb_k)
        elems = int(lag.posteriors_compact_layout(frames[0], ug[0])[-1])
        values = torch.zeros(elems, device="cuda")
        out = torch.zeros(B, 2, dtype=torch.float64, device="cuda")
        s = abi.stream()

        def compact_checkpoint():
            with abi.option("align_checkpoint", args.checkpoint):
                abi.check(lib.tdnnf_align_posteriors_compact(lag.h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, 1.0, abi.ptr(values), elems, abi.ptr(out),
                                                             abi.ptr(ws), nb_k, s))

        compact_checkpoint()
        torch.cuda.synchronize()
        ms = [timed(compact_checkpoint, args.calls) for _ in range(args.repeats)]
        r = out.cpu().numpy()
        d.update(checkpoint=args.checkpoint, workspace_bytes_checkpoint=nb_k, ok=int(r[:, 1].sum()), output_bytes=4 * elems,
                 posteriors_compact_checkpoint=dict(ms=round(float(np.median(ms)), 3), ms_all=[round(v, 3) for v in ms],
                                                    us_per_frame=round(1e3 * float(np.median(ms)) / TL, 3)),
                 mass_per_frame=round(float(values.sum(dtype=torch.float64).item()) / (B * TL), 9))
        return d

    # forced alignment: transcripts of 120 units with optional units and alternative branches -- a few hundred states each
    graphs = [pkg.synth.make_alignment_graph(rng.integers(0, P, size=120).tolist(), optional=list(range(5, 120, 10)),
                                             alternatives={k: rng.integers(0, P, size=12).tolist() for k in range(3, 120, 8)}, num_pdfs=P, seed=u,
                                             labels=args.labels)
              for u in range(64)]
    ag = abi.AlignGraphs(graphs, num_pdfs=P, num_labels=max(g["L"] for g in graphs) if args.labels else None)
    if args.labels:
        res["labels"] = args.labels
    _, res["forced"] = case(ag, 64, np.arange(64))
    res["forced"]["states_per_graph"] = int(np.mean(ag.num_states))
    del ag
    # free decode on the bench's denominator graph
    den = pkg.synth.make_den_graph(4000, P, mean_out_degree=12.0, seed=1)
    if args.labels:
        g = pkg.synth.alignment_graph_from_den(den)
        g["label"] = g["dst"] if args.labels == "unit" else np.arange(len(g["src"]), dtype=np.int32)
        ag = abi.AlignGraphs(g, num_labels=int(g["label"].max()) + 1)
    else:
        ag = abi.AlignGraphs.from_den_graph(den)
    # (one column per arc: 48 k floats a frame, and an utterance's block must start below float 2^31 of the output -- 64 utterances do)
    B = 64 if args.labels == "arc" else 128
    y, res["free"] = case(ag, B, np.zeros(B, np.int32))
    res["free"].update(ag.info())
    if args.posteriors:
        res["metric"] = "align_posteriors"
        if args.compact:
            del y, ag
            torch.cuda.empty_cache()
            res["long"] = long_case()
        print(json.dumps(res))
        return
    # the yardstick: the objective-only chain computation (forward recursions only) on the same graph and shape, rows read as a t-major minibatch
    dg = abi.DenGraph(den)
    ds = abi.Supervision(pkg.synth.make_supervision_from_den(den, B, T, num_paths=2, seed=2))
    nb = int(lib.tdnnf_chain_objf_workspace_bytes(dg.h, B, T))
    ws = abi.workspace(nb)
    out = torch.zeros(8, dtype=torch.float64, device="cuda")
    s = abi.stream()

    def objf():
        abi.check(lib.tdnnf_chain_objf(dg.h, ds.h, abi.pmat(y), None, 0.1, 0.0, abi.ptr(out), abi.ptr(ws), nb, s))

    objf(), objf()
    torch.cuda.synchronize()
    ms = [timed(objf, args.calls) for _ in range(args.repeats)]
    res["chain_objf"] = dict(ms=round(float(np.median(ms)), 3), ms_all=[round(v, 3) for v in ms], us_per_frame=round(1e3 * float(np.median(ms)) / T, 3))
    res["free_over_chain_objf"] = round(res["free"]["ms"] / res["chain_objf"]["ms"], 3)
    del y, ag, dg, ds, ws
    torch.cuda.empty_cache()
    res["long"] = long_path_case()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
