"""Seeded synthetic inputs of the shapes SURVEY.md 8(d) prescribes: denominator
graphs, numerator (supervision) graphs, fbank/ivector egs and tdnn index sets.
numpy only; shared by tests/, bench.py and __graft_entry__.smoke().

Shapes follow the reference recipes: 40-dim fbank + 100-dim ivector inputs
(local/chain_NAS/run_tdnn_fbk_40_iv_sp_7q.sh:160-161), t-major row order
row = t_index * num_sequences + n (src/nnet3/nnet-tdnn-component.cc:642-646,897-902).
"""
import numpy as np


def make_den_graph(H, P, mean_out_degree=12.0, seed=0):
    """Strongly connected HMM: ring arcs h->h+1 plus Poisson extra arcs, pdf ids
    uniform, transition probs row-normalised Dirichlet(1).  init = average
    occupancy over 100 steps from state 0 (DenominatorGraph::SetInitialProbs, UPSTREAM)."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for h in range(H):
        k = max(1, int(rng.poisson(mean_out_degree)))
        d = rng.integers(0, H, size=k)
        d[0] = (h + 1) % H
        src.append(np.full(k, h))
        dst.append(d)
    src = np.concatenate(src).astype(np.int32)
    dst = np.concatenate(dst).astype(np.int32)
    A = len(src)
    pdf = rng.integers(0, P, size=A).astype(np.int32)
    raw = rng.gamma(1.0, 1.0, size=A)
    tot = np.zeros(H)
    np.add.at(tot, src, raw)
    prob = (raw / tot[src]).astype(np.float32)
    # initial probs
    cur = np.zeros(H)
    cur[0] = 1.0
    avg = np.zeros(H)
    for _ in range(100):
        avg += cur / 100
        nxt = np.zeros(H)
        np.add.at(nxt, dst, cur[src] * prob)
        cur = nxt
    return {"H": H, "P": P, "src": src, "dst": dst, "pdf": pdf, "prob": prob,
            "init": avg.astype(np.float32)}


def make_supervision(B, T, P, max_alt=2, seed=0, weight=1.0):
    """Per-sequence time-synchronous numerator graphs: at every frame 1..max_alt
    alternative states, fully connected to the next frame's states, one random
    pdf and a small random log-weight per arc; every state at time T is final."""
    rng = np.random.default_rng(seed)
    state_time, final, a_src, a_dst, a_pdf, a_lp = [], [], [], [], [], []
    seq_state_begin, seq_arc_begin = [0], [0]
    ns = 0
    for _ in range(B):
        counts = [1] + [int(rng.integers(1, max_alt + 1)) for _ in range(T)]
        first = ns + np.concatenate([[0], np.cumsum(counts)[:-1]])
        for t, c in enumerate(counts):
            state_time += [t] * c
            final += [0.0 if t == T else -np.inf] * c
        for t in range(T):
            for i in range(counts[t]):
                for j in range(counts[t + 1]):
                    a_src.append(first[t] + i)
                    a_dst.append(first[t + 1] + j)
                    a_pdf.append(int(rng.integers(0, P)))
                    a_lp.append(float(-rng.random() * 0.5))
        ns += sum(counts)
        seq_state_begin.append(ns)
        seq_arc_begin.append(len(a_src))
    i32 = lambda x: np.asarray(x, dtype=np.int32)
    return {"B": B, "T": T, "seq_state_begin": i32(seq_state_begin),
            "seq_arc_begin": i32(seq_arc_begin), "state_time": i32(state_time),
            "final_logprob": np.asarray(final, dtype=np.float32), "arc_src": i32(a_src),
            "arc_dst": i32(a_dst), "arc_pdf": i32(a_pdf),
            "arc_logprob": np.asarray(a_lp, dtype=np.float32), "weight": float(weight)}


def make_supervision_from_den(den, B, T, num_paths=2, seed=0, weight=1.0):
    """Numerator graphs whose paths are paths of the denominator graph (as real chain supervisions are, after
    composition with the normalization FST): per sequence `num_paths` independent random walks on the den graph
    from one start state drawn from the initial distribution; arc log-weights are the den transition
    log-probs, and a path's first arc also carries the log of the denominator's initial probability of its start state -- the
    weight the denominator's own recursion gives that start (alpha(0, i) = init(i)).  Every numerator path is then a
    denominator path with the same weight, so log p_num <= log p_den and the LF-MMI objective stays <= 0 however long a net is
    trained on it (without the start weight the objective of a long run settled at +log(1 / init) / T per frame)."""
    rng = np.random.default_rng(seed)
    H = den["H"]
    order = np.argsort(den["src"], kind="stable")
    src_sorted = den["src"][order]
    begin = np.searchsorted(src_sorted, np.arange(H + 1))
    init = den["init"].astype(np.float64)
    init = init / init.sum()
    state_time, final, a_src, a_dst, a_pdf, a_lp = [], [], [], [], [], []
    seq_state_begin, seq_arc_begin = [0], [0]
    ns = 0
    for _ in range(B):
        h0 = int(rng.choice(H, p=init))
        # state ids: start, then per frame t = 1..T one state per path
        state_time.append(0)
        final.append(-np.inf)
        for t in range(1, T + 1):
            for _p in range(num_paths):
                state_time.append(t)
                final.append(0.0 if t == T else -np.inf)
        cur = [h0] * num_paths
        for t in range(T):
            for pth in range(num_paths):
                lo, hi = begin[cur[pth]], begin[cur[pth] + 1]
                a = order[int(rng.integers(lo, hi))]
                s_from = ns if t == 0 else ns + 1 + (t - 1) * num_paths + pth
                s_to = ns + 1 + t * num_paths + pth
                a_src.append(s_from)
                a_dst.append(s_to)
                a_pdf.append(int(den["pdf"][a]))
                lp = float(np.log(max(float(den["prob"][a]), 1e-30)))
                if t == 0:
                    lp += float(np.log(max(float(den["init"][h0]), 1e-30)))
                a_lp.append(lp)
                cur[pth] = int(den["dst"][a])
        ns += 1 + T * num_paths
        seq_state_begin.append(ns)
        seq_arc_begin.append(len(a_src))
    i32 = lambda x: np.asarray(x, dtype=np.int32)
    return {"B": B, "T": T, "seq_state_begin": i32(seq_state_begin), "seq_arc_begin": i32(seq_arc_begin),
            "state_time": i32(state_time), "final_logprob": np.asarray(final, dtype=np.float32), "arc_src": i32(a_src),
            "arc_dst": i32(a_dst), "arc_pdf": i32(a_pdf), "arc_logprob": np.asarray(a_lp, dtype=np.float32),
            "weight": float(weight)}


def tdnn_indexes(time_offsets, num_t_out, B, start_t_in=None, t_step_in=1, t_step_out=1,
                 start_t_out=0):
    """Restates TdnnDARTSV3Component::PrecomputeIndexes for a regular grid
    (src/nnet3/nnet-tdnn-component.cc:846-905).  Returns (row_stride, row_offsets,
    num_rows_in, num_rows_out)."""
    offs = list(time_offsets)
    if start_t_in is None:
        start_t_in = start_t_out + min(offs)
    rho = t_step_out // t_step_in
    assert t_step_out % t_step_in == 0
    last_t_in = start_t_out + (num_t_out - 1) * t_step_out + max(offs)
    num_t_in = (last_t_in - start_t_in) // t_step_in + 1
    num_t_in = rho * ((num_t_in + rho - 1) // rho)  # :841-843
    row_offsets = []
    for o in offs:
        req = start_t_out + o
        input_t = (req - start_t_in) // t_step_in
        assert req == start_t_in + t_step_in * input_t
        mult, rem = rho * (input_t // rho), input_t % rho
        row_offsets.append(mult * B + rem)  # :897-902
    return rho, np.asarray(row_offsets, dtype=np.int32), num_t_in * B, num_t_out * B


def _ranges(starts, counts):
    """Concatenated aranges starts[i] .. starts[i] + counts[i] - 1 and, per element, the index i."""
    counts = np.maximum(counts, 0)
    owner = np.repeat(np.arange(len(counts)), counts)
    first = np.cumsum(counts) - counts
    return starts[owner] + (np.arange(int(counts.sum())) - first[owner]), owner


def make_supervision_lattice(B, T, P, tolerance=2, alternatives=1, mean_dur=3.0, seed=0, weight=1.0):
    """Per-sequence tolerance lattices, the shape of unconstrained chain egs: `alternatives` unit sequences that share the start
    state, every unit boundary free to move by +-`tolerance` frames.  Same dict as make_supervision.

    A unit has two pdfs as in the chain topology, one on its entry frame and one on every later frame.  Its nominal duration is
    1 + floor(Exp(mean_dur - 1)) frames -- the geometric tail a self-loop gives -- and the last unit is cut at T.  The unit that
    nominally starts at frame b may start at any frame of [b - tolerance, b + tolerance] that leaves every other unit at least one
    frame; the first starts at 0, the last ends at T.  States: the start, then one per (frame, alternative, unit, entered | looping)
    on a path from the start to a final state at frame T (the windows are tightened from both ends, which is the pruning of the
    states that cannot reach a final one), sorted by time.  About 1 + 4 tolerance / E[duration] states per frame and alternative.
    Arcs carry small random log-weights."""
    rng = np.random.default_rng(seed)
    state_time, final, a_src, a_dst, a_pdf = [], [], [], [], []
    seq_state_begin, seq_arc_begin = [0], [0]
    ns = na = 0
    for _ in range(B):
        times, fin, srcs, dsts, pdfs = [np.zeros(1, np.int64)], [np.zeros(1, bool)], [], [], []
        n_loc = 1
        for _alt in range(alternatives):
            d = 1 + np.floor(rng.exponential(max(mean_dur - 1.0, 1e-9), size=T)).astype(np.int64)
            b = np.concatenate([[0], np.cumsum(d)])
            U = int(np.searchsorted(b, T))  # units 0 .. U-1 start before T
            b = b[:U].copy()
            e_pdf, l_pdf = rng.integers(0, P, size=U), rng.integers(0, P, size=U)
            # entry windows [lo, hi] of every unit and of the virtual unit U that "enters" at T
            lo = np.maximum(b - tolerance, 0)
            hi = np.minimum(b + tolerance, T - 1)
            lo[0] = hi[0] = 0
            lo = np.maximum.accumulate(lo - np.arange(U)) + np.arange(U)              # lo[u] >= lo[u-1] + 1
            hi = np.append(hi, T)
            hi = np.minimum.accumulate((hi - np.arange(U + 1))[::-1])[::-1] + np.arange(U + 1)  # hi[u] <= hi[u+1] - 1
            lo = np.append(lo, T)
            # entered(t, u): unit u's entry frame was t - 1;  looping(t, u): t - 1 was a later frame of unit u
            cE = hi[:U] - lo[:U] + 1
            cL = hi[1:] - lo[:U] - 1
            tE, uE = _ranges(lo[:U] + 1, cE)
            tL, uL = _ranges(lo[:U] + 2, cL)
            offE = n_loc + np.cumsum(cE) - cE
            offL = n_loc + int(cE.sum()) + np.cumsum(np.maximum(cL, 0)) - np.maximum(cL, 0)
            idE = offE[uE] + (tE - lo[uE] - 1)
            idL = offL[uL] + (tL - lo[uL] - 2)
            t_all, u_all, id_all = np.concatenate([tE, tL]), np.concatenate([uE, uL]), np.concatenate([idE, idL])
            # stay in the unit (loop pdf)
            m = t_all + 1 <= hi[u_all + 1]
            srcs.append(id_all[m]); dsts.append(offL[u_all[m]] + (t_all[m] + 1 - lo[u_all[m]] - 2)); pdfs.append(l_pdf[u_all[m]])
            # enter the next unit at frame t (its entry pdf)
            m = (u_all + 1 < U) & (t_all >= lo[u_all + 1]) & (t_all <= hi[u_all + 1])
            un = u_all[m] + 1
            srcs.append(id_all[m]); dsts.append(offE[un] + (t_all[m] - lo[un])); pdfs.append(e_pdf[un])
            # the start state enters unit 0
            srcs.append(np.zeros(1, np.int64)); dsts.append(offE[:1].copy()); pdfs.append(e_pdf[:1])
            times += [tE, tL]
            fin += [(tE == T) & (uE == U - 1), (tL == T) & (uL == U - 1)]
            n_loc += int(cE.sum() + np.maximum(cL, 0).sum())
        t_loc, f_loc = np.concatenate(times), np.concatenate(fin)
        s_loc, d_loc, p_loc = np.concatenate(srcs), np.concatenate(dsts), np.concatenate(pdfs)
        order = np.argsort(t_loc, kind="stable")  # by time; the start (the only state of time 0) stays first
        new_id = np.empty(n_loc, np.int64)
        new_id[order] = np.arange(n_loc)
        s_loc, d_loc = new_id[s_loc], new_id[d_loc]
        ao = np.lexsort((d_loc, s_loc))
        state_time.append(t_loc[order]); final.append(np.where(f_loc[order], 0.0, -np.inf))
        a_src.append(ns + s_loc[ao]); a_dst.append(ns + d_loc[ao]); a_pdf.append(p_loc[ao])
        ns += n_loc
        na += len(ao)
        seq_state_begin.append(ns)
        seq_arc_begin.append(na)
    i32 = lambda x: np.asarray(x, dtype=np.int32)
    a_lp = (-rng.random(na) * 0.5).astype(np.float32)
    return {"B": B, "T": T, "seq_state_begin": i32(seq_state_begin), "seq_arc_begin": i32(seq_arc_begin),
            "state_time": i32(np.concatenate(state_time)), "final_logprob": np.concatenate(final).astype(np.float32),
            "arc_src": i32(np.concatenate(a_src)), "arc_dst": i32(np.concatenate(a_dst)), "arc_pdf": i32(np.concatenate(a_pdf)),
            "arc_logprob": a_lp, "weight": float(weight)}


def supervision_lattice_from_alignments(unit_set, alignments, T, tolerance, weight=1.0):
    """The tolerance lattices of GIVEN alignments, on the host: what hipabi.Supervision.assign_alignments compiles on the device
    (include/tdnnf_hip.h, "ALIGNMENT SUPERVISIONS"), as the dict of make_supervision that Supervision.assign takes.  unit_set: the dict of
    make_unit_set; alignments: one (units, starts) pair per sequence, starts in output frames, the first 0, strictly increasing, below T.
    make_supervision_lattice's construction with one alternative and its state and arc order, the pdfs from the unit set -- the entry pdf
    at (unit before or -1, unit) on the frame a unit is entered, its loop pdf on every later one -- and every arc log-prob 0."""
    ctx, entry, loop = int(unit_set["context"]), np.asarray(unit_set["entry_pdf"]), np.asarray(unit_set["loop_pdf"])
    state_time, final, a_src, a_dst, a_pdf = [], [], [], [], []
    seq_state_begin, seq_arc_begin = [0], [0]
    ns = na = 0
    for units, starts in alignments:
        u, b = np.asarray(units, np.int64).reshape(-1), np.asarray(starts, np.int64).reshape(-1)
        U = len(u)
        assert U >= 1 and len(b) == U and b[0] == 0 and np.all(np.diff(b) > 0) and b[-1] < T and tolerance >= 0
        left = np.concatenate([[-1], u[:-1]])
        e_pdf, l_pdf = (entry[left + 1, u], loop[left + 1, u]) if ctx else (entry[u], loop[u])
        lo = np.maximum(b - tolerance, 0)
        hi = np.minimum(b + tolerance, T - 1)
        lo[0] = hi[0] = 0
        lo = np.maximum.accumulate(lo - np.arange(U)) + np.arange(U)
        hi = np.append(hi, T)
        hi = np.minimum.accumulate((hi - np.arange(U + 1))[::-1])[::-1] + np.arange(U + 1)
        lo = np.append(lo, T)
        cE = hi[:U] - lo[:U] + 1
        cL = hi[1:] - lo[:U] - 1
        tE, uE = _ranges(lo[:U] + 1, cE)
        tL, uL = _ranges(lo[:U] + 2, cL)
        offE = 1 + np.cumsum(cE) - cE
        offL = 1 + int(cE.sum()) + np.cumsum(cL) - cL
        idE = offE[uE] + (tE - lo[uE] - 1)
        idL = offL[uL] + (tL - lo[uL] - 2)
        t_all, u_all, id_all = np.concatenate([tE, tL]), np.concatenate([uE, uL]), np.concatenate([idE, idL])
        stay = t_all + 1 <= hi[u_all + 1]
        enter = (u_all + 1 < U) & (t_all >= lo[np.minimum(u_all + 1, U)]) & (t_all <= hi[u_all + 1])
        un = u_all[enter] + 1
        s_loc = np.concatenate([np.zeros(1, np.int64), id_all[stay], id_all[enter]])
        d_loc = np.concatenate([offE[:1], offL[u_all[stay]] + (t_all[stay] + 1 - lo[u_all[stay]] - 2), offE[un] + (t_all[enter] - lo[un])])
        p_loc = np.concatenate([e_pdf[:1], l_pdf[u_all[stay]], e_pdf[un]])
        t_loc = np.concatenate([np.zeros(1, np.int64), tE, tL])
        f_loc = np.concatenate([np.zeros(1, bool), (tE == T) & (uE == U - 1), (tL == T) & (uL == U - 1)])
        n_loc = len(t_loc)
        order = np.argsort(t_loc, kind="stable")  # by time; within a time the entered states by unit, then the looping ones
        new_id = np.empty(n_loc, np.int64)
        new_id[order] = np.arange(n_loc)
        s_loc, d_loc = new_id[s_loc], new_id[d_loc]
        ao = np.lexsort((d_loc, s_loc))
        state_time.append(t_loc[order]); final.append(np.where(f_loc[order], 0.0, -np.inf))
        a_src.append(ns + s_loc[ao]); a_dst.append(ns + d_loc[ao]); a_pdf.append(p_loc[ao])
        ns += n_loc
        na += len(ao)
        seq_state_begin.append(ns)
        seq_arc_begin.append(na)
    i32 = lambda x: np.asarray(x, dtype=np.int32)
    return {"B": len(alignments), "T": int(T), "seq_state_begin": i32(seq_state_begin), "seq_arc_begin": i32(seq_arc_begin),
            "state_time": i32(np.concatenate(state_time)), "final_logprob": np.concatenate(final).astype(np.float32),
            "arc_src": i32(np.concatenate(a_src)), "arc_dst": i32(np.concatenate(a_dst)), "arc_pdf": i32(np.concatenate(a_pdf)),
            "arc_logprob": np.zeros(na, np.float32), "weight": float(weight)}


def supervision_lattice_from_alignment_chunks(unit_set, alignments, utt_frames, chunk_begins, T, tolerance, weight=1.0):
    """The tolerance lattices of chunks of GIVEN whole-utterance alignments, on the host: what hipabi.Supervision.assign_alignment_chunks
    compiles on the device (include/tdnnf_hip.h, "ALIGNMENT CHUNKS"), as the dict of make_supervision that Supervision.assign takes.
    Sequence s is the frames [chunk_begins[s], chunk_begins[s] + T) of an utterance of utt_frames[s] frames with the alignment
    alignments[s].  The route a caller without the device compile takes: the utterance's lattice from
    supervision_lattice_from_alignments, cut to the states of the chunk's times behind a new start, which enters every state of the
    first time with the pdf of the arcs into it; every state of the last time is final."""
    state_time, final, a_src, a_dst, a_pdf = [], [], [], [], []
    seq_state_begin, seq_arc_begin = [0], [0]
    ns = na = 0
    for al, Tu, o in zip(alignments, utt_frames, chunk_begins):
        Tu, o = int(Tu), int(o)
        assert 0 <= o and o + T <= Tu and T >= 1
        utt = supervision_lattice_from_alignments(unit_set, [al], Tu, tolerance)
        t, src, dst, pdf = (utt[k].astype(np.int64) for k in ("state_time", "arc_src", "arc_dst", "arc_pdf"))
        keep = (t > o) & (t <= o + T)
        new_id = np.cumsum(keep)  # (the new start is 0)
        pdf_in = np.zeros(len(t), np.int64)
        pdf_in[dst] = pdf  # (all arcs into a state carry one pdf)
        first = np.flatnonzero(t == o + 1)
        inner = keep[src] & keep[dst]
        state_time.append(np.concatenate([[0], t[keep] - o]))
        final.append(np.where(state_time[-1] == T, 0.0, -np.inf))
        a_src.append(ns + np.concatenate([np.zeros(len(first), np.int64), new_id[src[inner]]]))
        a_dst.append(ns + np.concatenate([new_id[first], new_id[dst[inner]]]))
        a_pdf.append(np.concatenate([pdf_in[first], pdf[inner]]))
        ns += len(state_time[-1])
        na += len(first) + int(inner.sum())
        seq_state_begin.append(ns)
        seq_arc_begin.append(na)
    i32 = lambda x: np.asarray(x, dtype=np.int32)
    return {"B": len(alignments), "T": int(T), "seq_state_begin": i32(seq_state_begin), "seq_arc_begin": i32(seq_arc_begin),
            "state_time": i32(np.concatenate(state_time)), "final_logprob": np.concatenate(final).astype(np.float32),
            "arc_src": i32(np.concatenate(a_src)), "arc_dst": i32(np.concatenate(a_dst)), "arc_pdf": i32(np.concatenate(a_pdf)),
            "arc_logprob": np.zeros(na, np.float32), "weight": float(weight)}


def make_alignment_graph(pdf_sequence, self_loops=True, optional=(), alternatives=None, seed=0, num_pdfs=None, labels=None):
    """Left-to-right transcript graph for best-path alignment: the shape of a compile-train-graphs output reduced to pdf labels.
    Epsilon-free, so a state is "inside a unit": state 0 is the start, unit k is one state, every arc INTO it carries its pdf --
    the entering arc and, with self_loops, its loop.  The main chain is one unit per entry of pdf_sequence.
      alternatives  {k: [pdfs]}: a parallel branch of units with these pdfs beside main unit k (entered from k's predecessors,
                    left to k's successors);
      optional      main units that may be skipped: their predecessors also enter their successors (one unit per skip; with
                    the last unit optional its predecessors are final, with the first the start enters unit 1).
    Arcs are ordered by (source, destination) and carry small random log-weights (seed).  Returns {S, P, src, dst, pdf, logprob,
    init, final} with states numbered from 0: init is 0 at the start state, final 0 at the last units, -inf elsewhere.
      labels        None: no labels.  "unit": the dict also has "label", per arc the index of the unit it enters (main units first, then
                    the alternatives' in ascending k) -- phone-like, shared by the entering arcs and the self-loop -- and "L", the number
                    of units; "arc": "label" is the arc's index and "L" the number of arcs -- transition-id-like.  For
                    hipabi.AlignGraphs(..., num_labels=...)."""
    assert labels in (None, "unit", "arc")
    rng = np.random.default_rng(seed)
    pdfs = [int(p) for p in pdf_sequence]
    n = len(pdfs)
    assert n >= 1
    edges = {(k - 1, k) for k in range(n)}  # unit -1 is the start
    finals = {n - 1}
    for k, branch in sorted((alternatives or {}).items()):
        assert 0 <= k < n and len(branch) >= 1
        first = len(pdfs)
        pdfs += [int(p) for p in branch]
        last = len(pdfs) - 1
        edges |= {(b, b + 1) for b in range(first, last)}
        edges.add((k - 1, first))
        if k + 1 < n:
            edges.add((last, k + 1))
        else:
            finals.add(last)
    for k in sorted(set(optional)):
        assert 0 <= k < n
        pred = [u for (u, v) in edges if v == k]
        succ = [v for (u, v) in edges if u == k and v != k]
        edges |= {(u, v) for u in pred for v in succ}
        if k in finals:
            finals |= set(pred)
    if self_loops:
        edges |= {(u, u) for u in range(len(pdfs))}
    arcs = sorted((u + 1, v + 1) for (u, v) in edges)
    S = len(pdfs) + 1
    src = np.asarray([a[0] for a in arcs], dtype=np.int32)
    dst = np.asarray([a[1] for a in arcs], dtype=np.int32)
    init = np.full(S, -np.inf, dtype=np.float32)
    init[0] = 0.0
    final = np.full(S, -np.inf, dtype=np.float32)
    final[[f + 1 for f in finals]] = 0.0
    P = int(num_pdfs if num_pdfs is not None else max(pdfs) + 1)
    g = {"S": S, "P": P, "src": src, "dst": dst, "pdf": np.asarray(pdfs, dtype=np.int32)[dst - 1],
         "logprob": (-rng.random(len(arcs)) * 0.5).astype(np.float32), "init": init, "final": final}
    if labels == "unit":
        g["label"], g["L"] = (dst - 1).astype(np.int32), len(pdfs)
    elif labels == "arc":
        g["label"], g["L"] = np.arange(len(arcs), dtype=np.int32), len(arcs)
    return g


def alignment_graph_from_den(den):
    """The graph of the free best path through a denominator graph (make_den_graph's dict), in make_alignment_graph's form: arcs
    log(prob), initial log(init) with -inf where init is 0, every state final at 0."""
    with np.errstate(divide="ignore"):
        logprob = np.log(np.asarray(den["prob"], dtype=np.float64)).astype(np.float32)
        init = np.log(np.asarray(den["init"], dtype=np.float64)).astype(np.float32)
    return {"S": int(den["H"]), "P": int(den["P"]), "src": np.asarray(den["src"], dtype=np.int32), "dst": np.asarray(den["dst"], dtype=np.int32),
            "pdf": np.asarray(den["pdf"], dtype=np.int32), "logprob": logprob, "init": init, "final": np.zeros(int(den["H"]), dtype=np.float32)}


def alignment_graphs_from_supervision(sup):
    """One graph per sequence of a supervision dict (make_supervision ...), in make_alignment_graph's form: the sequence's states and
    arcs as they are, its time-0 state initial at 0, final_logprob as given."""
    out = []
    for s in range(int(sup["B"])):
        s0, s1 = int(sup["seq_state_begin"][s]), int(sup["seq_state_begin"][s + 1])
        a0, a1 = int(sup["seq_arc_begin"][s]), int(sup["seq_arc_begin"][s + 1])
        init = np.full(s1 - s0, -np.inf, dtype=np.float32)
        init[0] = 0.0
        pdf = np.asarray(sup["arc_pdf"][a0:a1], dtype=np.int32)
        out.append({"S": s1 - s0, "P": int(pdf.max()) + 1 if len(pdf) else 1, "src": np.asarray(sup["arc_src"][a0:a1], dtype=np.int32) - s0,
                    "dst": np.asarray(sup["arc_dst"][a0:a1], dtype=np.int32) - s0, "pdf": pdf,
                    "logprob": np.asarray(sup["arc_logprob"][a0:a1], dtype=np.float32), "init": init,
                    "final": np.asarray(sup["final_logprob"][s0:s1], dtype=np.float32)})
    return out


def _shortest_accepting_path(g):
    """Fewest arcs on a path from an initial to a final state of a make_alignment_graph dict (inf: none)."""
    dist = np.where(np.asarray(g["init"]) > -np.inf, 0.0, np.inf)
    for _ in range(int(g["S"])):
        nxt = dist.copy()
        np.minimum.at(nxt, g["dst"], dist[g["src"]] + 1)
        if np.array_equal(nxt, dist):
            break
        dist = nxt
    return float(dist[np.asarray(g["final"]) > -np.inf].min())


def make_e2e_supervision(B, T, P, units=(2, 6), seed=0, weight=1.0, **graph_kw):
    """End-to-end (flat-start) supervision: per sequence one make_alignment_graph transcript -- lo..hi units (at most T) with random pdfs,
    self-loops on, graph_kw (optional=..., alternatives=...) passed through -- whose shortest accepting path is at most T arcs, so that
    with its self-loops it accepts exactly T frames.  Returns {B, T, P, weight, graphs: [...]}: what hipabi.Supervision takes."""
    rng = np.random.default_rng(seed)
    lo, hi = units
    graphs = []
    for s in range(B):
        n = int(rng.integers(min(lo, T), min(hi, T) + 1))
        n = max(n, 1)
        kw = dict(graph_kw)
        if "optional" in kw:
            kw["optional"] = [k for k in kw["optional"] if k < n]
        if "alternatives" in kw:
            kw["alternatives"] = {k: v for k, v in kw["alternatives"].items() if k < n}
        g = make_alignment_graph(rng.integers(0, P, size=n), self_loops=True, seed=int(rng.integers(1 << 30)), num_pdfs=P, **kw)
        assert _shortest_accepting_path(g) <= T
        graphs.append(g)
    return {"B": int(B), "T": int(T), "P": int(P), "weight": float(weight), "graphs": graphs}


def e2e_supervision_from_supervision(sup, P):
    """The end-to-end form of a time-synchronous supervision dict: its sequences as graphs (alignment_graphs_from_supervision), same
    weight.  Both forms have the same paths, so the chain objective and its derivatives agree."""
    return {"B": int(sup["B"]), "T": int(sup["T"]), "P": int(P), "weight": float(sup.get("weight", 1.0)),
            "graphs": alignment_graphs_from_supervision(sup)}


def make_unit_set(U, context=0, seed=0, distinct=True, P=None):
    """A unit set for transcript graphs (hipabi.UnitSet): {U, P, context, entry_pdf, loop_pdf, loop_logprob, leave_logprob, take_logprob,
    skip_logprob}.  context 0: entry_pdf / loop_pdf of shape (U,); context 1 (left-biphone): (U + 1, U), row left + 1.  distinct: every
    entry and loop pdf is a pdf of its own (P = twice their number), so that a pdf sequence names its states; otherwise they are drawn
    from P (default U + 2) pdfs and collide.  The weights are multiples of 1/8 in [-2, 0]: sums of a few of them are exact in float32."""
    rng = np.random.default_rng(seed)
    shape = (U + 1, U) if context else (U,)
    n = int(np.prod(shape))
    if distinct:
        P = 2 * n if P is None else int(P)
        assert P >= 2 * n
        perm = rng.permutation(P)[:2 * n]
        entry, loop = perm[:n].reshape(shape), perm[n:].reshape(shape)
    else:
        P = U + 2 if P is None else int(P)
        entry, loop = rng.integers(0, P, size=shape), rng.integers(0, P, size=shape)
    eighths = lambda size=None: (-rng.integers(0, 17, size=size) / 8.0)
    return {"U": int(U), "P": int(P), "context": int(context), "entry_pdf": entry.astype(np.int32), "loop_pdf": loop.astype(np.int32),
            "loop_logprob": eighths(U).astype(np.float32), "leave_logprob": eighths(U).astype(np.float32),
            "take_logprob": float(eighths()), "skip_logprob": float(eighths())}


def make_transcripts(B, U, slots=(1, 8), optional_rate=0.3, seed=0):
    """B transcripts for hipabi.UnitSet: each a (units, optional) pair of int32 arrays of lo .. hi slots, units at random from U, a slot
    optional with probability optional_rate where the slot before it is not -- never two adjacent -- and at least one slot mandatory."""
    rng = np.random.default_rng(seed)
    lo, hi = slots
    out = []
    for _ in range(B):
        n = int(rng.integers(lo, hi + 1))
        units = rng.integers(0, U, size=n).astype(np.int32)
        opt = np.zeros(n, np.int32)
        for k in range(n):
            opt[k] = int(rng.random() < optional_rate and not (k and opt[k - 1]))
        if opt.all():  # (n = 1)
            opt[0] = 0
        out.append((units, opt))
    return out


def make_pronunciation_transcripts(B, U, positions=(1, 6), alternatives=(1, 3), units=(1, 3), optional_rate=0.3, seed=0):
    """B transcripts with pronunciation alternatives for hipabi.UnitSet: each (positions, optional, alt_logprob) -- lo .. hi positions,
    positions[p] a list of lo .. hi alternatives, each an int32 array of lo .. hi units at random from U; optional[p] as make_transcripts
    draws it (never two adjacent, one position mandatory at least); alt_logprob[p] one multiple of 1/8 in [-2, 0] per alternative, so that
    sums of a few weights are exact in float32."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(B):
        n = int(rng.integers(positions[0], positions[1] + 1))
        pos, logprob = [], []
        for _ in range(n):
            A = int(rng.integers(alternatives[0], alternatives[1] + 1))
            pos.append([rng.integers(0, U, size=int(rng.integers(units[0], units[1] + 1))).astype(np.int32) for _ in range(A)])
            logprob.append((-rng.integers(0, 17, size=A) / 8.0).astype(np.float32))
        opt = np.zeros(n, np.int32)
        for k in range(n):
            opt[k] = int(rng.random() < optional_rate and not (k and opt[k - 1]))
        if opt.all():  # (n = 1)
            opt[0] = 0
        out.append((pos, opt, logprob))
    return out
