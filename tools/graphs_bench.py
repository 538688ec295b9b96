#!/usr/bin/env python3
"""What a NEW batch of graphs costs per call: (a) tdnnf_align_graphs_create + the call + tdnnf_align_graphs_destroy against (b)
tdnnf_align_graphs_assign on one reserved handle + the call -- and the same for the end-to-end supervision (tdnnf_supervision_create_e2e /
_destroy against tdnnf_supervision_assign_e2e) through tdnnf_chain_objf_and_deriv.  Every iteration has different graphs, from a cycle of
--cycle (at least 8) batches generated and stacked beforehand, so the time is the C path's: host validation and table build or staging,
allocations and copies or the device build, the call, the frees.
  forced     64 transcript graphs of some 300 states x 500 frames: tdnnf_align_best_path, and tdnnf_align_posteriors_compact
  free       the 4 000-state denominator-like graph (one graph a batch, its arcs reordered per batch), 16 utterances x 100 frames: best path
  numerator  128 graphs of 70 states x 150 frames through tdnnf_chain_objf_and_deriv
The clock is the host's around a loop over the cycle that ends in ONE synchronise; (a) and (b) alternate in one process, medians of
--repeats.  After the timing every batch of the cycle runs once either way and the outputs are compared for equality.  One JSON line.
--transcripts: instead, the cost of a new batch for a caller who starts from transcripts (see transcripts() below): arc arrays built on the
host + assign, assign alone, and tdnnf_align_graphs_assign_transcripts / tdnnf_supervision_assign_e2e_transcripts, alternating.
--pronunciations: instead, the same for transcripts with pronunciation alternatives (see pronunciations() below): statement-style arc arrays
built on the host + assign, assign alone, and tdnnf_align_graphs_assign_pronunciations, alternating.
--supervision [--tolerance N --alternatives N]: instead, the time-synchronous supervision of regular LF-MMI (see supervision() below):
tdnnf_supervision_create + tdnnf_chain_objf_and_deriv + tdnnf_supervision_destroy against tdnnf_supervision_assign + the same call.
--supervision --alignment [--tolerance N]: instead, the same supervision for a caller who starts from alignments (see alignment() below):
the lattice built on the host + tdnnf_supervision_assign, assign alone, and tdnnf_supervision_assign_alignments, alternating.
--supervision --alignment --chunks [--utt-frames N]: the same three routes for chunks of --frames frames cut at random begins out of
utterances of --utt-frames (default 1000): the utterance's lattice built and cut on the host + assign, assign alone, and
tdnnf_supervision_assign_alignment_chunks.
--features [--sequences B --frames T --utt-frames N]: instead, the INPUT of a minibatch of chunks (see features() below): the t-major
features and the i-vectors sliced out of host copies with numpy and uploaded, against tdnnf_chunk_input_gather from the device copies.
--features --stored 1|2|3: the utterances' features held as Kaldi's compressed codes in a feature store of that format (see stored_features()
below): the float gather against tdnnf_chunk_input_gather_stored, a device copy of a batch of utterances against tdnnf_feature_store_expand.
usage (GPU box): python tools/graphs_bench.py [--repeats R] [--cycle N] [--pdfs P] [--only forced|free|numerator] [--transcripts] [--pronunciations]
                                              [--features [--stored 1|2|3] [--sequences B --frames T --utt-frames N]]
                                              [--supervision [--tolerance N --alternatives N] [--sequences B --frames T]]
                                              [--supervision --alignment [--chunks [--utt-frames N]] [--tolerance N] [--sequences B --frames T]]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402


def transcripts(args, pkg):
    """--transcripts: what a new batch costs when the caller starts from TRANSCRIPTS, three ways, alternating in one process, a different
    batch every iteration, medians of --repeats:
      host_graphs_assign  (a) the arc arrays made on the host (tests/transcript_graphs_ref.py transcript_graph_vectorised, then stacked), assign,
                          the call -- what a caller had to do before tdnnf_align_graphs_assign_transcripts;
      assign              (b) assign from arrays made outside the timed region, the call: the assign's own cost, the control;
      assign_transcripts  (c) assign_transcripts, the call.
    forced: 64 transcripts of some 300 states x 500 frames, tdnnf_align_best_path.  numerator: 128 of some 70 states x 150 frames through
    tdnnf_chain_objf_and_deriv on a reserved supervision.  The outputs of the three are compared for equality in the same run."""
    from tests import transcript_graphs_ref as ref
    abi, synth = pkg.hipabi, pkg.synth
    lib = abi.load()
    P = args.pdfs
    us = synth.make_unit_set(42, context=1, seed=1, distinct=False, P=P)
    units = abi.UnitSet(us["entry_pdf"], us["loop_pdf"], us["loop_logprob"], us["leave_logprob"], P, us["take_logprob"], us["skip_logprob"])
    res = dict(metric="transcripts_per_batch", pdfs=P, cycle=args.cycle, repeats=args.repeats, units=42, context=1)
    s = abi.stream()

    def host_graphs(batch):
        return abi.Supervision._stack_e2e([ref.transcript_graph_vectorised(us, u, o) for u, o in batch])[1]

    def case(name, B, T, slots, assign, assign_transcripts, call, outputs):
        batches = [synth.make_transcripts(B, 42, slots=slots, optional_rate=0.15, seed=100 + c) for c in range(args.cycle)]
        slot_arrays = [abi._slots(b) for b in batches]
        stacked = [host_graphs(b) for b in batches]
        fns = dict(host_graphs_assign=lambda i: (assign(host_graphs(batches[i])), call()),
                   assign=lambda i: (assign(stacked[i]), call()),
                   assign_transcripts=lambda i: (assign_transcripts(slot_arrays[i]), call()))

        def loop(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.cycle):
                fn(i)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / args.cycle

        ms = {k: [] for k in fns}
        for r in range(args.repeats + 1):  # the first round warms up: kernels loaded, the allocator's pools filled
            for k, fn in fns.items():
                t = loop(fn)
                if r:
                    ms[k].append(t)
        equal = True
        for i in range(args.cycle):
            got = []
            for fn in fns.values():
                for t in outputs:
                    t.zero_()
                fn(i)
                torch.cuda.synchronize()
                got.append([t.clone() for t in outputs])
            equal = equal and all(torch.equal(x.view(torch.uint8), z.view(torch.uint8)) for other in got[1:] for x, z in zip(got[0], other))
        d = dict(sequences=B, frames=T, states=int(max(k[0][0][-1] for k in stacked)), arcs=int(max(k[1][0][-1] for k in stacked)), outputs_equal=bool(equal))
        for k, v in ms.items():
            d[k] = dict(ms=round(float(np.median(v)), 3), ms_all=[round(x, 3) for x in v])
        d["transcripts_over_host_graphs"] = round(d["assign_transcripts"]["ms"] / d["host_graphs_assign"]["ms"], 3)
        d["transcripts_over_assign"] = round(d["assign_transcripts"]["ms"] / d["assign"]["ms"], 3)
        res[name] = d

    # forced alignment
    B, T = 64, 500
    graphs = C.c_void_p()
    abi.check(lib.tdnnf_align_graphs_reserve(B, P, 0, B * 340, B * 1000, C.byref(graphs)))
    y = torch.randn(B * T, P, device="cuda")
    frames, rows = abi.iarr([T] * B), abi.iarr(np.arange(B) * T)
    nb = 16 + 32 * B + 256 + 4 * T * B * 340 + 16 * B * 340  # the header's formula at the capacity
    ws = abi.workspace(nb)
    pdfs, results = torch.zeros(B * T, dtype=torch.int32, device="cuda"), torch.zeros(B, 2, dtype=torch.float64, device="cuda")
    case("forced", B, T, (255, 265),
         lambda k: abi.check(lib.tdnnf_align_graphs_assign(graphs, B, *[x[1] for x in k], None, s)),
         lambda a: abi.check(lib.tdnnf_align_graphs_assign_transcripts(graphs, units.h, B, a[0][1], a[1][1], a[2][1], s)),
         lambda: abi.check(lib.tdnnf_align_best_path(graphs, B, None, frames[1], rows[1], 1, abi.pmat(y), 1.0, abi.ptr(pdfs), None, abi.ptr(results), abi.ptr(ws), nb, s)),
         [pdfs, results])
    lib.tdnnf_align_graphs_destroy(graphs)
    # the flat-start numerator
    B, T = 128, 150
    sup = C.c_void_p()
    abi.check(lib.tdnnf_supervision_reserve_e2e(B, T, P, B * 90, B * 270, C.byref(sup)))
    dg = abi.DenGraph(synth.make_den_graph(64, P, mean_out_degree=4.0, seed=1))  # (the numerator takes the workspace layout from it, nothing else)
    y = torch.randn(B * T, P, device="cuda")
    xo = torch.log_softmax(torch.randn(B * T, P, device="cuda"), dim=1)
    nb = int(lib.tdnnf_chain_workspace_bytes(dg.h, B, T))
    ws = abi.workspace(nb)
    ws.zero_()
    out = (torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros_like(y), torch.zeros_like(y))
    case("numerator", B, T, (60, 62),
         lambda k: abi.check(lib.tdnnf_supervision_assign_e2e(sup, B, T, *[x[1] for x in k], 1.0, s)),
         lambda a: abi.check(lib.tdnnf_supervision_assign_e2e_transcripts(sup, units.h, B, T, a[0][1], a[1][1], a[2][1], 1.0, s)),
         lambda: abi.check(lib.tdnnf_chain_objf_and_deriv(dg.h, sup, abi.pmat(y), abi.pmat(xo), 0.1, 5e-5, 0.1, abi.ptr(out[0]), abi.pmat(out[1]), abi.pmat(out[2]),
                                                         abi.ptr(ws), nb, s)),
         list(out))
    lib.tdnnf_supervision_destroy(sup)
    print(json.dumps(res))


def pronunciations(args, pkg):
    """--pronunciations: what a new batch of graph tables costs when the caller starts from transcripts with PRONUNCIATION ALTERNATIVES,
    three ways, alternating in one process, a different batch every iteration, medians of --repeats; the clock stops behind one synchronise
    after the cycle's assigns (no alignment call: the tables are the product):
      host_graphs_assign     (a) the arc arrays made on the host as the numpy statement makes them (tests/pronunciation_graphs_ref.py
                             pronunciation_graph: a Python walk over states and arcs, then stacked), tdnnf_align_graphs_assign -- the
                             only route before tdnnf_align_graphs_assign_pronunciations;
      assign                 (b) assign from arrays made outside the timed region: the assign's own cost, the control;
      assign_pronunciations  (c) tdnnf_align_graphs_assign_pronunciations from the six flat arrays.
    Two shapes, context 1, 42 units, alternatives of 3 units, 1 or 2 a position (mean 1.5): 128 transcripts of 11 to 13 positions, and
    64 of 39 to 41.  Also the bytes each route stages on the host, and the host time of the assign_pronunciations call alone.  After the
    timing the device tables of (b) and (c) are compared for equality on every batch of the cycle.  One JSON line."""
    from tests import pronunciation_graphs_ref as ref
    abi, synth = pkg.hipabi, pkg.synth
    lib = abi.load()
    P, U = args.pdfs, 42
    us = synth.make_unit_set(U, context=1, seed=1, distinct=False, P=P)
    units = abi.UnitSet(us["entry_pdf"], us["loop_pdf"], us["loop_logprob"], us["leave_logprob"], P, us["take_logprob"], us["skip_logprob"])
    res = dict(metric="pronunciations_per_batch", pdfs=P, cycle=args.cycle, repeats=args.repeats, units=U, context=1)
    s = abi.stream()
    keys = ("S", "P", "src", "dst", "pdf", "logprob", "init", "final")

    def host_graphs(batch):
        return abi.Supervision._stack_e2e([{k: g[k] for k in keys} for g in (ref.pronunciation_graph(us, t) for t in batch)])[1]

    def case(name, B, positions):
        batches = [synth.make_pronunciation_transcripts(B, U, positions=positions, alternatives=(1, 2), units=(3, 3), optional_rate=0.15, seed=100 + c)
                   for c in range(args.cycle)]
        flat = [abi._pronunciations(b) for b in batches]
        stacked = [host_graphs(b) for b in batches]
        NS, NA = int(max(k[0][0][-1] for k in stacked)), int(max(k[1][0][-1] for k in stacked))
        graphs = abi.AlignGraphs.reserve(B, P, NS, NA)

        def assign(k):
            abi.check(lib.tdnnf_align_graphs_assign(graphs.h, B, *[x[1] for x in k], None, s))

        def assign_pronunciations(i):
            abi.check(lib.tdnnf_align_graphs_assign_pronunciations(graphs.h, units.h, B, *[x[1] for x in flat[i]], s))

        fns = dict(host_graphs_assign=lambda i: assign(host_graphs(batches[i])), assign=lambda i: assign(stacked[i]), assign_pronunciations=assign_pronunciations)

        def loop(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.cycle):
                fn(i)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / args.cycle

        ms = {k: [] for k in fns}
        for r in range(args.repeats + 1):  # the first round warms up
            for k, fn in fns.items():
                t = loop(fn)
                if r:
                    ms[k].append(t)
        host_ms = []
        for i in range(args.cycle):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            assign_pronunciations(i)
            host_ms.append(1e3 * (time.perf_counter() - t0))
        equal = True
        for i in range(args.cycle):
            tables = []
            for k in ("assign", "assign_pronunciations"):
                fns[k](i)
                graphs.G = B
                tables.append(graphs.tables())
            flatten = lambda t: [v for x in t.values() for v in (x.values() if isinstance(x, dict) else [x])]
            equal = equal and all(np.array_equal(x, z) for x, z in zip(flatten(tables[0]), flatten(tables[1])))
        # what the two routes stage on the host per batch (the largest of the cycle): assign 28 bytes an arc, 8 a state and the begins;
        # assign_pronunciations the six flat arrays, two ints a position and one an alternative more, and the begins
        entries = max(len(f[5][0]) for f in flat)
        staged = max(4 * (5 * (B + 1) + 2 * len(f[1][0]) + 1 + 3 * len(f[3][0]) + 1 + len(f[5][0])) for f in flat)
        d = dict(transcripts=B, positions=list(positions), entries=entries, states=NS, arcs=NA, tables_equal=bool(equal),
                 staged_bytes_assign=4 * (4 * (B + 1) + 4 * NA + 2 * NS), staged_bytes_assign_pronunciations=staged,
                 assign_pronunciations_host=round(float(np.median(host_ms)), 3))
        for k, v in ms.items():
            d[k] = dict(ms=round(float(np.median(v)), 3), ms_all=[round(x, 3) for x in v])
        d["pronunciations_over_host_graphs"] = round(d["assign_pronunciations"]["ms"] / d["host_graphs_assign"]["ms"], 4)
        d["pronunciations_over_assign"] = round(d["assign_pronunciations"]["ms"] / d["assign"]["ms"], 3)
        res[name] = d

    case("128x12", 128, (11, 13))
    case("64x40", 64, (39, 41))
    print(json.dumps(res))


def supervision(args, pkg):
    """--supervision: what a NEW time-synchronous minibatch costs per step, two ways alternating in one process, a different synthetic
    minibatch every iteration (a cycle generated beforehand), medians of --repeats:
      create_call_destroy  tdnnf_supervision_create, tdnnf_chain_objf_and_deriv, tdnnf_supervision_destroy;
      assign_call          tdnnf_supervision_assign on ONE reserved supervision, the same call.
    --tolerance 0 (default): synth.make_supervision (alignment-like, narrow); --tolerance N --alternatives M: synth.make_supervision_lattice
    (tolerance lattices, the wide case).  Also reported: the host time of the assign call alone (a clock around the call, no synchronise)
    and the device time of what an assign enqueues -- its copies and the two build kernels -- between two events on an otherwise idle
    stream.  After the timing every minibatch of the cycle runs once either way and results, nnet_output_deriv and xent_deriv are compared
    for equality.  One JSON line."""
    abi, synth = pkg.hipabi, pkg.synth
    lib = abi.load()
    P, B, T = args.pdfs, args.sequences, args.frames
    if args.tolerance > 0:
        sups = [synth.make_supervision_lattice(B, T, P, tolerance=args.tolerance, alternatives=args.alternatives, seed=10 + c) for c in range(args.cycle)]
    else:
        sups = [synth.make_supervision(B, T, P, max_alt=2, seed=10 + c) for c in range(args.cycle)]
    batches = []
    for sup in sups:
        keep = [abi.iarr(sup["seq_state_begin"]), abi.iarr(sup["seq_arc_begin"]), abi.iarr(sup["state_time"]), abi.farr(sup["final_logprob"]),
                abi.iarr(sup["arc_src"]), abi.iarr(sup["arc_dst"]), abi.iarr(sup["arc_pdf"]), abi.farr(sup["arc_logprob"])]
        batches.append(dict(S=len(keep[2][0]), A=len(keep[4][0]), keep=keep, ptrs=[k[1] for k in keep]))
    dg = abi.DenGraph(synth.make_den_graph(64, P, mean_out_degree=4.0, seed=1))
    reserved = C.c_void_p()
    abi.check(lib.tdnnf_supervision_reserve(B, T, max(b["S"] for b in batches), max(b["A"] for b in batches), C.byref(reserved)))
    y = torch.randn(B * T, P, device="cuda")
    xo = torch.log_softmax(torch.randn(B * T, P, device="cuda"), dim=1)
    nb = int(lib.tdnnf_chain_workspace_bytes(dg.h, B, T))
    ws = abi.workspace(nb)
    ws.zero_()
    s = abi.stream()
    out = {k: (torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros_like(y), torch.zeros_like(y)) for k in "ab"}

    def call(h, o):
        abi.check(lib.tdnnf_chain_objf_and_deriv(dg.h, h, abi.pmat(y), abi.pmat(xo), 0.1, 5e-5, 0.1, abi.ptr(o[0]), abi.pmat(o[1]), abi.pmat(o[2]), abi.ptr(ws), nb, s))

    def created(b, o=out["a"]):
        h = C.c_void_p()
        abi.check(lib.tdnnf_supervision_create(B, T, *b["ptrs"], 1.0, C.byref(h)))
        call(h, o)
        lib.tdnnf_supervision_destroy(h)

    def assign(b):
        abi.check(lib.tdnnf_supervision_assign(reserved, B, T, *b["ptrs"], 1.0, s))

    def assigned(b, o=out["b"]):
        assign(b)
        call(reserved, o)

    def loop(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for b in batches:
            fn(b)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / len(batches)

    def assign_alone():
        """(host ms per assign call, device ms per assign between two events), the stream idle before each"""
        host_ms, dev_ms = [], []
        for b in batches:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            assign(b)
            host_ms.append(1e3 * (time.perf_counter() - t0))
            e1.record()
            torch.cuda.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
        return float(np.median(host_ms)), float(np.median(dev_ms))

    loop(created), loop(assigned), loop(lambda b: call(reserved, out["b"]))  # warm-up: kernels loaded, the allocator's pools filled
    ms = dict(create_call_destroy=[], assign_call=[], call_alone=[], assign_host=[], assign_device=[])
    for _ in range(args.repeats):
        ms["create_call_destroy"].append(loop(created))
        ms["assign_call"].append(loop(assigned))
        ms["call_alone"].append(loop(lambda b: call(reserved, out["b"])))
        h, d = assign_alone()
        ms["assign_host"].append(h)
        ms["assign_device"].append(d)
    equal = True
    for b in batches:
        for o in out.values():
            for t in o:
                t.zero_()
        created(b), assigned(b)
        torch.cuda.synchronize()
        equal = equal and torch.equal(out["a"][0].view(torch.int64), out["b"][0].view(torch.int64)) and all(
            torch.equal(x.view(torch.int32), z.view(torch.int32)) for x, z in zip(out["a"][1:], out["b"][1:]))
    info = [C.c_int() for _ in range(4)]
    abi.check(lib.tdnnf_supervision_info(reserved, *[C.byref(x) for x in info]))
    cap = [C.c_int() for _ in range(6)] + [C.c_longlong()]
    abi.check(lib.tdnnf_supervision_capacity(reserved, *[C.byref(x) for x in cap]))
    res = dict(metric="supervision_per_minibatch", pdfs=P, cycle=args.cycle, repeats=args.repeats, sequences=B, frames=T, tolerance=args.tolerance,
               alternatives=args.alternatives, states=max(b["S"] for b in batches), arcs=max(b["A"] for b in batches), wide=int(info[3].value),
               max_states_per_frame=int(info[2].value), device_bytes=int(cap[6].value), allocations_since_reserve=int(cap[5].value), outputs_equal=bool(equal))
    for k, v in ms.items():
        res[k] = dict(ms=round(float(np.median(v)), 3), ms_all=[round(x, 3) for x in v])
    res["assign_over_create"] = round(res["assign_call"]["ms"] / res["create_call_destroy"]["ms"], 3)
    lib.tdnnf_supervision_destroy(reserved)
    print(json.dumps(res))


def alignment(args, pkg):
    """--supervision --alignment [--tolerance N, default 5]: what a new minibatch costs per step for a caller who starts from ALIGNMENTS,
    three ways alternating in one process, a different minibatch every iteration (a cycle of random segmentations generated beforehand),
    medians of --repeats:
      host_lattice_assign  (a) the lattice's arrays made on the host (synth.supervision_lattice_from_alignments, numpy array operations),
                           tdnnf_supervision_assign, tdnnf_chain_objf_and_deriv -- what a caller had to do before
                           tdnnf_supervision_assign_alignments;
      assign               (b) assign from arrays made outside the timed region, the call: the assign's own cost, the control;
      assign_alignments    (c) tdnnf_supervision_assign_alignments, the call.
    Two shapes: --sequences x --frames (default 128 x 150) at the tolerance with mean duration 6 frames, and one wide shape, 64 x 150 at
    tolerance 40 with mean duration 3.  Also the host time of the assign_alignments call alone and the device time of what it enqueues.
    The outputs of the three are compared for equality in the same run.  One JSON line.
    --chunks: every sequence is a chunk of --frames frames at a random begin of an utterance of --utt-frames frames with an alignment of
    its own; (a) builds the utterance's lattice and cuts it (synth.supervision_lattice_from_alignment_chunks), (c) is
    tdnnf_supervision_assign_alignment_chunks; the keys of the JSON line keep their names."""
    abi, synth = pkg.hipabi, pkg.synth
    lib = abi.load()
    P, U = args.pdfs, 42
    us = synth.make_unit_set(U, context=1, seed=1, distinct=False, P=P)
    units = abi.UnitSet(us["entry_pdf"], us["loop_pdf"], us["loop_logprob"], us["leave_logprob"], P, us["take_logprob"], us["skip_logprob"])
    dg = abi.DenGraph(synth.make_den_graph(64, P, mean_out_degree=4.0, seed=1))
    s = abi.stream()
    res = dict(metric="alignment_chunk_supervision_per_minibatch" if args.chunks else "alignment_supervision_per_minibatch", pdfs=P, cycle=args.cycle,
               repeats=args.repeats, units=U, context=1)
    if args.chunks:
        res["utt_frames"] = args.utt_frames

    def random_alignment(rng, T, mean_dur):
        d = 1 + np.floor(rng.exponential(mean_dur - 1.0, size=T)).astype(np.int64)
        b = np.concatenate([[0], np.cumsum(d)])
        b = b[:int(np.searchsorted(b, T))]
        return rng.integers(0, U, size=len(b)).astype(np.int32), b.astype(np.int32)

    def pointers(sup):
        keep = [abi.iarr(sup["seq_state_begin"]), abi.iarr(sup["seq_arc_begin"]), abi.iarr(sup["state_time"]), abi.farr(sup["final_logprob"]),
                abi.iarr(sup["arc_src"]), abi.iarr(sup["arc_dst"]), abi.iarr(sup["arc_pdf"]), abi.farr(sup["arc_logprob"])]
        return keep, [k[1] for k in keep]

    def case(name, B, T, tol, mean_dur):
        rng = np.random.default_rng(1)
        Tu = args.utt_frames if args.chunks else T  # (without --chunks a sequence is its utterance)
        assert Tu >= T, "--utt-frames below --frames"
        batches = [[random_alignment(rng, Tu, mean_dur) for _ in range(B)] for _ in range(args.cycle)]
        begins = [abi._chunks(B, [Tu] * B, rng.integers(0, Tu - T + 1, size=B)) for _ in range(args.cycle)]

        def host_lattice(i):
            if args.chunks:
                return synth.supervision_lattice_from_alignment_chunks(us, batches[i], begins[i][0][0], begins[i][1][0], T, tol)
            return synth.supervision_lattice_from_alignments(us, batches[i], T, tol)

        made = [pointers(host_lattice(i)) for i in range(args.cycle)]
        flat = [abi._alignments(b) for b in batches]
        NS, NA = max(len(m[0][2][0]) for m in made), max(len(m[0][4][0]) for m in made)
        reserved = C.c_void_p()
        abi.check(lib.tdnnf_supervision_reserve(B, T, NS, NA, C.byref(reserved)))
        y = torch.randn(B * T, P, device="cuda")
        xo = torch.log_softmax(torch.randn(B * T, P, device="cuda"), dim=1)
        nb = int(lib.tdnnf_chain_workspace_bytes(dg.h, B, T))
        ws = abi.workspace(nb)
        ws.zero_()
        out = (torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros_like(y), torch.zeros_like(y))

        def call():
            abi.check(lib.tdnnf_chain_objf_and_deriv(dg.h, reserved, abi.pmat(y), abi.pmat(xo), 0.1, 5e-5, 0.1, abi.ptr(out[0]), abi.pmat(out[1]), abi.pmat(out[2]),
                                                     abi.ptr(ws), nb, s))

        def assign(ptrs):
            abi.check(lib.tdnnf_supervision_assign(reserved, B, T, *ptrs, 1.0, s))

        def assign_alignments(i):
            a = flat[i]
            if args.chunks:
                abi.check(lib.tdnnf_supervision_assign_alignment_chunks(reserved, units.h, B, T, a[0][1], a[1][1], a[2][1], begins[i][0][1], begins[i][1][1], tol,
                                                                        1.0, s))
            else:
                abi.check(lib.tdnnf_supervision_assign_alignments(reserved, units.h, B, T, a[0][1], a[1][1], a[2][1], tol, 1.0, s))

        fns = dict(host_lattice_assign=lambda i: (assign(pointers(host_lattice(i))[1]), call()),
                   assign=lambda i: (assign(made[i][1]), call()),
                   assign_alignments=lambda i: (assign_alignments(i), call()))

        def loop(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.cycle):
                fn(i)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / args.cycle

        ms = {k: [] for k in fns}
        for r in range(args.repeats + 1):  # the first round warms up
            for k, fn in fns.items():
                t = loop(fn)
                if r:
                    ms[k].append(t)
        host_ms, dev_ms = [], []
        for i in range(args.cycle):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            assign_alignments(i)
            host_ms.append(1e3 * (time.perf_counter() - t0))
            e1.record()
            torch.cuda.synchronize()
            dev_ms.append(e0.elapsed_time(e1))
        equal = True
        for i in range(args.cycle):
            got = []
            for fn in fns.values():
                for t in out:
                    t.zero_()
                fn(i)
                torch.cuda.synchronize()
                got.append([t.clone() for t in out])
            equal = equal and all(torch.equal(x.view(torch.uint8), z.view(torch.uint8)) for other in got[1:] for x, z in zip(got[0], other))
        info = [C.c_int() for _ in range(4)]
        abi.check(lib.tdnnf_supervision_info(reserved, *[C.byref(x) for x in info]))
        cap = [C.c_int() for _ in range(6)] + [C.c_longlong()]
        abi.check(lib.tdnnf_supervision_capacity(reserved, *[C.byref(x) for x in cap]))
        d = dict(sequences=B, frames=T, tolerance=tol, mean_duration=mean_dur, units=int(max(len(a[1][0]) for a in flat)), states=NS, arcs=NA,
                 wide=int(info[3].value), max_states_per_frame=int(info[2].value), allocations_since_reserve=int(cap[5].value), outputs_equal=bool(equal),
                 assign_alignments_host=round(float(np.median(host_ms)), 3), assign_alignments_device=round(float(np.median(dev_ms)), 3))
        for k, v in ms.items():
            d[k] = dict(ms=round(float(np.median(v)), 3), ms_all=[round(x, 3) for x in v])
        d["alignments_over_host_lattice"] = round(d["assign_alignments"]["ms"] / d["host_lattice_assign"]["ms"], 3)
        d["alignments_over_assign"] = round(d["assign_alignments"]["ms"] / d["assign"]["ms"], 3)
        lib.tdnnf_supervision_destroy(reserved)
        res[name] = d

    tol = args.tolerance if args.tolerance > 0 else 5
    case("regular", args.sequences, args.frames, tol, 6.0)
    case("wide", 64, 150, 40, 3.0)
    print(json.dumps(res))


def features(args, pkg):
    """--features: what the INPUT of a minibatch of chunks costs when the utterances' features are already on the device (as
    AcousticModel.compute took them for the alignment pass), two ways, alternating in one process, other chunks every iteration, medians
    of --repeats:
      host_slice_upload  the t-major matrix sliced out of host copies with numpy (one fancy index through the clamped row numbers) and
                         uploaded, the i-vector rows alike -- what a caller had to do before tdnnf_chunk_input_gather;
      gather             hipabi.ChunkInput.gather into the same output buffers.
    --sequences x --frames output frames and 64 x --frames, feat_dim 40, ivector_dim 100, the input window of the default model graph at
    that chunk width (a net of small dimensions is made for tdnnf_net_input_frames alone); --utt-frames output frames an utterance.  The
    outputs of the two are compared for equality in the same run.  bytes: what the host route uploads per minibatch (the gather reads and
    writes as many on the device) and what the gather stages."""
    abi, fsf, D, Di, period = pkg.hipabi, 3, 40, 100, 10
    net = pkg.trainer.ChainNet(pkg.trainer.make_config(frames_per_chunk=args.frames * fsf, num_sequences=1, bottleneck=16, feat_dim=D, ivector_dim=Di, num_pdfs=64,
                                                       hidden_dim=64, small_dim=32))
    shape = (net.first_t, net.num_t_in, fsf)
    net.close()
    rng = np.random.default_rng(0)
    U, T = 64, args.frames
    frames = rng.integers(args.utt_frames * fsf - 2 * fsf, args.utt_frames * fsf + 1, size=U)
    rows = (frames + period - 1) // period
    F, IV = rng.standard_normal((int(frames.sum()), D)).astype(np.float32), rng.standard_normal((int(rows.sum()), Di)).astype(np.float32)
    feat0, iv0 = np.concatenate([[0], np.cumsum(frames)[:-1]]), np.concatenate([[0], np.cumsum(rows)[:-1]])
    F_dev, IV_dev = torch.from_numpy(F).cuda(), torch.from_numpy(IV).cuda()
    res = dict(metric="chunk_features_per_minibatch", cycle=args.cycle, repeats=args.repeats, feat_dim=D, ivector_dim=Di, first_t=shape[0], num_t=shape[1],
               frame_subsampling=fsf, utterances=U, utt_frames=args.utt_frames)

    def case(name, B):
        batches = []
        for c in range(args.cycle):
            utt = rng.integers(0, U, size=B)
            batches.append((utt, rng.integers(0, (frames[utt] + fsf - 1) // fsf - T + 1), int(rng.integers(-(fsf - 1), fsf))))
        h = abi.ChunkInput(B)
        out = {k: (torch.zeros(shape[1] * B, D, device="cuda"), torch.zeros(B, Di, device="cuda")) for k in ("host_slice_upload", "gather")}
        times = np.arange(shape[0], shape[0] + shape[1])

        def host_route(i, o=out["host_slice_upload"]):
            utt, begins, shift = batches[i]
            t = np.clip(begins[None, :] * fsf + times[:, None] - shift, 0, frames[utt][None, :] - 1) + feat0[utt][None, :]
            o[0].copy_(torch.from_numpy(F[t.reshape(-1)]), non_blocking=False)
            o[1].copy_(torch.from_numpy(IV[iv0[utt] + np.minimum(((begins + T // 2) * fsf) // period, rows[utt] - 1)]), non_blocking=False)

        def gather(i, o=out["gather"]):
            utt, begins, shift = batches[i]
            h.gather(shape, T, utt, begins, frames, F_dev, rows, IV_dev, period, frame_shift=shift, out=o)

        fns = dict(host_slice_upload=host_route, gather=gather)

        def loop(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.cycle):
                fn(i)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / args.cycle

        ms = {k: [] for k in fns}
        for r in range(args.repeats + 1):  # the first round warms up
            for k, fn in fns.items():
                t = loop(fn)
                if r:
                    ms[k].append(t)
        equal = True
        for i in range(args.cycle):
            host_route(i), gather(i)
            torch.cuda.synchronize()
            equal = equal and all(torch.equal(x.view(torch.int32), z.view(torch.int32)) for x, z in zip(out["host_slice_upload"], out["gather"]))
        info = h.info()
        d = dict(sequences=B, frames=T, outputs_equal=bool(equal), last_form=info["last_form"], allocations=info["allocations"],
                 bytes_uploaded_host_route=4 * (shape[1] * B * D + B * Di), bytes_staged_gather=16 * B)
        for k, v in ms.items():
            d[k] = dict(ms=round(float(np.median(v)), 3), ms_all=[round(x, 3) for x in v])
        d["gather_over_host"] = round(d["gather"]["ms"] / d["host_slice_upload"]["ms"], 3)
        res[name] = d

    case("regular", args.sequences)
    case("half", 64)
    print(json.dumps(res))


def stored_features(args, pkg):
    """--features --stored FORMAT: the same minibatches with the utterances' features held in a hipabi.FeatureStore of format 1 (CM), 2
    (CM2) or 3 (CM3) (include/tdnnf_hip.h, "FEATURE STORES") instead of a float matrix, alternating in one process, medians of --repeats:
      gather / gather_stored   ChunkInput.gather from the float copy against ChunkInput.gather_stored from the store, into the same kind of
                               output buffers; the float copy IS the store's expand, so the outputs are compared for equality;
      copy / expand            a batch of --expand-utts utterances: torch.index_select of their rows out of the float copy (one device
                               kernel through a row list made beforehand) against FeatureStore.expand.
    Wall-clock per call including the enqueue, not the kernels alone.  device_bytes: what the utterances take each way."""
    abi, fsf, D, Di, period, fmt = pkg.hipabi, 3, 40, 100, 10, args.stored
    net = pkg.trainer.ChainNet(pkg.trainer.make_config(frames_per_chunk=args.frames * fsf, num_sequences=1, bottleneck=16, feat_dim=D, ivector_dim=Di, num_pdfs=64,
                                                       hidden_dim=64, small_dim=32))
    shape = (net.first_t, net.num_t_in, fsf)
    net.close()
    rng = np.random.default_rng(0)
    U, T = 64, args.frames
    frames = rng.integers(args.utt_frames * fsf - 2 * fsf, args.utt_frames * fsf + 1, size=U)
    rows = (frames + period - 1) // period
    store = abi.FeatureStore(fmt, D, U, int(frames.sum()))
    for f in frames:  # codes and headers drawn directly: any codes cost the same
        f = int(f)
        item = dict(format=fmt, min=np.float32(-3.0), range=np.float32(9.0), rows=f, cols=D)
        if fmt == 1:
            item["percentiles"] = np.sort(rng.integers(0, 65536, size=(D, 4)), axis=1).astype(np.uint16)
            item["codes"] = rng.integers(0, 256, size=(D, f)).astype(np.uint8)
        else:
            item["codes"] = rng.integers(0, 65536 if fmt == 2 else 256, size=(f, D)).astype(np.uint16 if fmt == 2 else np.uint8)
        store.append([item])
    F_dev = store.expand(np.arange(U))
    IV_dev = torch.from_numpy(rng.standard_normal((int(rows.sum()), Di)).astype(np.float32)).cuda()
    feat0 = np.concatenate([[0], np.cumsum(frames)[:-1]])
    res = dict(metric="stored_chunk_features_per_minibatch", format=fmt, cycle=args.cycle, repeats=args.repeats, feat_dim=D, ivector_dim=Di, first_t=shape[0],
               num_t=shape[1], frame_subsampling=fsf, utterances=U, utt_frames=args.utt_frames, device_bytes_float=4 * int(frames.sum()) * D,
               device_bytes_stored=store.info()["device_bytes"], reserved_bytes_stored=store.info()["reserved_bytes"])

    def timed(fns):
        def loop(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.cycle):
                fn(i)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / args.cycle
        ms = {k: [] for k in fns}
        for r in range(args.repeats + 1):  # the first round warms up
            for k, fn in fns.items():
                t = loop(fn)
                if r:
                    ms[k].append(t)
        return {k: dict(ms=round(float(np.median(v)), 3), ms_all=[round(x, 3) for x in v]) for k, v in ms.items()}

    def case(name, B):
        batches = []
        for c in range(args.cycle):
            utt = rng.integers(0, U, size=B)
            batches.append((utt, rng.integers(0, (frames[utt] + fsf - 1) // fsf - T + 1), int(rng.integers(-(fsf - 1), fsf))))
        h = abi.ChunkInput(B)
        out = {k: (torch.zeros(shape[1] * B, D, device="cuda"), torch.zeros(B, Di, device="cuda")) for k in ("gather", "gather_stored")}

        def gather(i, o=out["gather"]):
            utt, begins, shift = batches[i]
            h.gather(shape, T, utt, begins, frames, F_dev, rows, IV_dev, period, frame_shift=shift, out=o)

        def gather_stored(i, o=out["gather_stored"]):
            utt, begins, shift = batches[i]
            h.gather_stored(shape, T, utt, begins, store, rows, IV_dev, period, frame_shift=shift, out=o)

        d = dict(sequences=B, frames=T, **timed(dict(gather=gather, gather_stored=gather_stored)))
        equal = True
        for i in range(args.cycle):
            gather(i), gather_stored(i)
            torch.cuda.synchronize()
            equal = equal and all(torch.equal(x.view(torch.int32), z.view(torch.int32)) for x, z in zip(out["gather"], out["gather_stored"]))
        d.update(outputs_equal=bool(equal), last_form=store.info()["last_form"], stored_over_float=round(d["gather_stored"]["ms"] / d["gather"]["ms"], 3))
        res[name] = d

    case("regular", args.sequences)
    case("half", 64)
    # the expand of a batch of utterances against a device copy of the same float rows
    n = min(args.expand_utts, U)
    lists = [rng.permutation(U)[:n] for _ in range(args.cycle)]
    row_lists = [torch.from_numpy(np.concatenate([np.arange(feat0[u], feat0[u] + frames[u]) for u in l])).cuda() for l in lists]
    most = max(len(r) for r in row_lists)
    bufs = {k: torch.zeros(most, D, device="cuda") for k in ("copy", "expand")}

    def copy(i):
        torch.index_select(F_dev, 0, row_lists[i], out=bufs["copy"][:len(row_lists[i])])

    def expand(i):
        store.expand(lists[i], out=bufs["expand"][:len(row_lists[i])])

    d = dict(utterances=n, rows=int(np.mean([len(r) for r in row_lists])), **timed(dict(copy=copy, expand=expand)))
    equal = True
    for i in range(args.cycle):
        copy(i), expand(i)
        torch.cuda.synchronize()
        k = len(row_lists[i])
        equal = equal and torch.equal(bufs["copy"][:k].view(torch.int32), bufs["expand"][:k].view(torch.int32))
    d.update(outputs_equal=bool(equal), last_form=store.info()["last_form"], expand_over_copy=round(d["expand"]["ms"] / d["copy"]["ms"], 3))
    res["expand"] = d
    res["allocations"] = store.info()["allocations"]
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--cycle", type=int, default=8)
    ap.add_argument("--pdfs", type=int, default=6034)
    ap.add_argument("--only", choices=["forced", "free", "numerator"])
    ap.add_argument("--transcripts", action="store_true", help="graphs from transcripts: host-built arrays + assign against assign_transcripts")
    ap.add_argument("--pronunciations", action="store_true",
                    help="graphs from transcripts with pronunciation alternatives: host-built arrays + assign against assign_pronunciations")
    ap.add_argument("--supervision", action="store_true", help="time-synchronous supervisions: create + call + destroy against assign + call")
    ap.add_argument("--tolerance", type=int, default=0, help="--supervision: > 0 tolerance lattices (synth.make_supervision_lattice)")
    ap.add_argument("--alignment", action="store_true",
                    help="--supervision: from alignments -- host-built lattice + assign against assign_alignments (--tolerance, default 5)")
    ap.add_argument("--chunks", action="store_true",
                    help="--supervision --alignment: chunks of --frames frames out of utterances of --utt-frames, assign_alignment_chunks")
    ap.add_argument("--utt-frames", type=int, default=1000)
    ap.add_argument("--features", action="store_true",
                    help="the input of a minibatch of chunks: numpy slicing of host copies + upload against tdnnf_chunk_input_gather (--sequences, --frames, --utt-frames)")
    ap.add_argument("--stored", type=int, default=0, choices=[0, 1, 2, 3],
                    help="--features: the features held in a FeatureStore of this format (1 CM, 2 CM2, 3 CM3): float gather against gather_stored, copy against expand")
    ap.add_argument("--expand-utts", type=int, default=16, help="--features --stored: utterances in an expand")
    ap.add_argument("--alternatives", type=int, default=1)
    ap.add_argument("--sequences", type=int, default=128)
    ap.add_argument("--frames", type=int, default=150)
    args = ap.parse_args()
    assert args.cycle >= 8, "different graphs every iteration: a cycle of at least 8 batches"
    pkg = ge.load_package()
    if args.features:
        return stored_features(args, pkg) if args.stored else features(args, pkg)
    if args.supervision:
        return alignment(args, pkg) if args.alignment else supervision(args, pkg)
    if args.transcripts:
        return transcripts(args, pkg)
    if args.pronunciations:
        return pronunciations(args, pkg)
    abi, synth = pkg.hipabi, pkg.synth
    lib = abi.load()
    P = args.pdfs
    res = dict(metric="graphs_per_batch", pdfs=P, cycle=args.cycle, repeats=args.repeats)

    def stacked(graphs):
        """the eight host arrays of one batch as ctypes pointers (kept alive beside them)"""
        keep = abi.Supervision._stack_e2e(graphs)[1]
        return dict(G=len(graphs), S=int(keep[0][0][-1]), A=int(keep[1][0][-1]), keep=keep, ptrs=[k[1] for k in keep])

    def median_ms(fn_a, fn_b, batches):
        """fn(batch) enqueues one batch's work; ms per batch of each, alternating, medians of --repeats"""
        def loop(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for b in batches:
                fn(b)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0) / len(batches)
        loop(fn_a), loop(fn_b)  # warm-up: kernels loaded, the allocator's pools filled
        ms = ([], [])
        for _ in range(args.repeats):
            ms[0].append(loop(fn_a))
            ms[1].append(loop(fn_b))
        return [dict(ms=round(float(np.median(v)), 3), ms_all=[round(x, 3) for x in v]) for v in ms]

    def align_case(name, batches, B, T, utt_graph, entries):
        """batches: stacked batches of graphs; B utterances x T frames, utterance u on graph utt_graph[u]"""
        cap = [max(b[k] for b in batches) for k in ("G", "S", "A")]
        reserved = C.c_void_p()
        abi.check(lib.tdnnf_align_graphs_reserve(cap[0], P, 0, cap[1], cap[2], C.byref(reserved)))
        y = torch.randn(B * T, P, device="cuda")
        frames, rows, ug = abi.iarr([T] * B), abi.iarr(np.arange(B) * T), abi.iarr(utt_graph)
        s = abi.stream()
        # per batch the workspace and the compact layout (host questions, asked once on a created handle), one buffer at the largest
        for b in batches:
            h = C.c_void_p()
            abi.check(lib.tdnnf_align_graphs_create(b["G"], P, *b["ptrs"], C.byref(h)))
            b["nb_path"] = int(lib.tdnnf_align_workspace_bytes(h, B, ug[1], frames[1]))
            b["nb_post"] = int(lib.tdnnf_align_posteriors_workspace_bytes(h, B, ug[1], frames[1], 1))
            elems = C.c_longlong()
            abi.check(lib.tdnnf_align_posteriors_compact_layout(h, B, ug[1], frames[1], C.byref(elems), None))
            b["elems"] = int(elems.value)
            lib.tdnnf_align_graphs_destroy(h)
        nb = max(max(b["nb_path"], b["nb_post"]) for b in batches)
        ws = abi.workspace(nb)
        out = {k: (torch.zeros(B * T, dtype=torch.int32, device="cuda"), torch.zeros(max(b["elems"] for b in batches), device="cuda"),
                   torch.zeros(B, 2, dtype=torch.float64, device="cuda")) for k in "ab"}

        def call(entry, h, b, o):
            pdfs, values, results = o
            if entry == "best_path":
                abi.check(lib.tdnnf_align_best_path(h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, abi.ptr(pdfs), None, abi.ptr(results), abi.ptr(ws), nb, s))
            else:
                abi.check(lib.tdnnf_align_posteriors_compact(h, B, ug[1], frames[1], rows[1], 1, abi.pmat(y), 1.0, 1.0, abi.ptr(values), b["elems"], abi.ptr(results),
                                                             abi.ptr(ws), nb, s))

        d = dict(graphs=cap[0], states=cap[1], arcs=cap[2], utterances=B, frames=T)
        for entry in entries:
            def created(b, o=out["a"]):
                h = C.c_void_p()
                abi.check(lib.tdnnf_align_graphs_create(b["G"], P, *b["ptrs"], C.byref(h)))
                call(entry, h, b, o)
                lib.tdnnf_align_graphs_destroy(h)

            def assigned(b, o=out["b"]):
                abi.check(lib.tdnnf_align_graphs_assign(reserved, b["G"], *b["ptrs"], None, s))
                call(entry, reserved, b, o)

            a, bb = median_ms(created, assigned, batches)
            equal = True
            for b in batches:
                for o in out.values():
                    for t in o:
                        t.zero_()
                created(b), assigned(b)
                torch.cuda.synchronize()
                equal = equal and all(torch.equal(x.view(torch.int64) if x.dtype == torch.float64 else x.view(torch.int32),
                                                  z.view(torch.int64) if z.dtype == torch.float64 else z.view(torch.int32)) for x, z in zip(out["a"], out["b"]))
            d[entry] = dict(create_call_destroy=a, assign_call=bb, assign_over_create=round(bb["ms"] / a["ms"], 3), outputs_equal=bool(equal))
        lib.tdnnf_align_graphs_destroy(reserved)
        res[name] = d

    rng = np.random.default_rng(0)
    if args.only in (None, "forced"):
        batches = []
        for c in range(args.cycle):
            batches.append(stacked([synth.make_alignment_graph(rng.integers(0, P, size=120).tolist(), optional=list(range(5, 120, 10)),
                                                               alternatives={k: rng.integers(0, P, size=12).tolist() for k in range(3, 120, 8)}, num_pdfs=P,
                                                               seed=64 * c + u) for u in range(64)]))
        align_case("forced", batches, 64, 500, np.arange(64), ("best_path", "posteriors_compact"))
    if args.only in (None, "free"):
        g = synth.alignment_graph_from_den(synth.make_den_graph(4000, P, mean_out_degree=12.0, seed=1))
        batches = []
        for c in range(args.cycle):  # the same graph with its arcs in another order: other arrays, other tables
            order = np.random.default_rng(c).permutation(len(g["src"]))
            batches.append(stacked([dict(g, **{k: g[k][order] for k in ("src", "dst", "pdf", "logprob")})]))
        align_case("free", batches, 16, 100, np.zeros(16, np.int64), ("best_path",))
    if args.only in (None, "numerator"):
        B, T = 128, 150
        batches = [stacked(synth.make_e2e_supervision(B, T, P, units=(69, 69), seed=10 + c)["graphs"]) for c in range(args.cycle)]
        dg = abi.DenGraph(synth.make_den_graph(64, P, mean_out_degree=4.0, seed=1))  # (the numerator takes the workspace layout from it, nothing else)
        reserved = C.c_void_p()
        abi.check(lib.tdnnf_supervision_reserve_e2e(B, T, P, max(b["S"] for b in batches), max(b["A"] for b in batches), C.byref(reserved)))
        y = torch.randn(B * T, P, device="cuda")
        xo = torch.log_softmax(torch.randn(B * T, P, device="cuda"), dim=1)
        nb = int(lib.tdnnf_chain_workspace_bytes(dg.h, B, T))
        ws = abi.workspace(nb)
        ws.zero_()
        s = abi.stream()
        out = {k: (torch.zeros(8, dtype=torch.float64, device="cuda"), torch.zeros_like(y), torch.zeros_like(y)) for k in "ab"}

        def call(h, o):
            abi.check(lib.tdnnf_chain_objf_and_deriv(dg.h, h, abi.pmat(y), abi.pmat(xo), 0.1, 5e-5, 0.1, abi.ptr(o[0]), abi.pmat(o[1]), abi.pmat(o[2]), abi.ptr(ws), nb, s))

        def created(b, o=out["a"]):
            h = C.c_void_p()
            abi.check(lib.tdnnf_supervision_create_e2e(B, T, P, *b["ptrs"], 1.0, C.byref(h)))
            call(h, o)
            lib.tdnnf_supervision_destroy(h)

        def assigned(b, o=out["b"]):
            abi.check(lib.tdnnf_supervision_assign_e2e(reserved, B, T, *b["ptrs"], 1.0, s))
            call(reserved, o)

        a, bb = median_ms(created, assigned, batches)
        equal = True
        for b in batches:
            created(b), assigned(b)
            torch.cuda.synchronize()
            equal = equal and torch.equal(out["a"][0].view(torch.int64), out["b"][0].view(torch.int64)) and all(
                torch.equal(x.view(torch.int32), z.view(torch.int32)) for x, z in zip(out["a"][1:], out["b"][1:]))
        res["numerator"] = dict(sequences=B, frames=T, states=max(b["S"] for b in batches), arcs=max(b["A"] for b in batches), create_call_destroy=a,
                                assign_call=bb, assign_over_create=round(bb["ms"] / a["ms"], 3), outputs_equal=bool(equal))
        lib.tdnnf_supervision_destroy(reserved)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
