"""The graph of a transcript as include/tdnnf_hip.h ("transcript graphs") defines it, in numpy with float32 weights: what
tdnnf_align_graphs_assign_transcripts compiles on the device.  transcript_graph walks the definition state by state;
transcript_graph_vectorised gives the same arrays without a Python loop over the slots (tools/graphs_bench.py times it as the host's way
to the arc arrays).  Both return synth.make_alignment_graph's dict {S, P, src, dst, pdf, logprob, init, final} plus "label" and "L"."""
import numpy as np

F32 = np.float32


def check_transcript(U, units, optional):
    """The three refusals of the definition, as assertions."""
    units, optional = np.asarray(units), np.asarray(optional) != 0
    assert len(units) == len(optional) >= 1
    assert ((units >= 0) & (units < U)).all(), "a unit outside [0, U)"
    assert not (optional[1:] & optional[:-1]).any(), "adjacent optional slots"
    assert not optional.all(), "no mandatory slot"


def transcript_graph(us, units, optional, num_labels=None):
    """us: a unit set dict (synth.make_unit_set).  units, optional: the transcript's slots."""
    units, opt = [int(u) for u in units], [bool(o) for o in optional]
    n, U, ctx = len(units), int(us["U"]), int(us["context"])
    check_transcript(U, units, opt)
    entry, loop = np.asarray(us["entry_pdf"]), np.asarray(us["loop_pdf"])
    leave, loop_lp = np.asarray(us["leave_logprob"], F32), np.asarray(us["loop_logprob"], F32)
    take, skip = F32(us["take_logprob"]), F32(us["skip_logprob"])
    pdf_of = lambda table, left, u: int(table[left + 1, u] if ctx else table[u])

    # the states: (slot, left neighbour's slot or -1); state 0 is the start
    states, of_slot = [None], [[] for _ in range(n)]
    for k in range(n):
        of_slot[k].append(len(states))
        states.append((k, k - 1))                  # A_k
        if ctx and k >= 1 and opt[k - 1]:
            of_slot[k].append(len(states))
            states.append((k, k - 2))              # B_k: slot k-1 was skipped
    S = len(states)
    left_unit = lambda s: units[states[s][1]] if states[s][1] >= 0 else -1
    entry_pdf = lambda s: pdf_of(entry, left_unit(s), units[states[s][0]])
    loop_pdf = lambda s: pdf_of(loop, left_unit(s), units[states[s][0]])

    arcs = {}  # (src, dst) -> (pdf, weight, label)

    def add(src, dst, pdf, w):
        assert (src, dst) not in arcs
        arcs[(src, dst)] = (pdf, F32(w), states[dst][0])

    for k in range(n):
        for s in of_slot[k]:
            add(s, s, loop_pdf(s), loop_lp[units[k]])
        a = of_slot[k][0]
        # the entering arcs
        if k == 0:
            add(0, a, entry_pdf(a), F32(0) + take if opt[0] else F32(0))
        else:
            for s in of_slot[k - 1]:
                add(s, a, entry_pdf(a), leave[units[k - 1]] + take if opt[k] else leave[units[k - 1]])
        # the skip arcs over an optional slot k-1
        if k >= 1 and opt[k - 1]:
            d = of_slot[k][1] if ctx else a
            if k == 1:
                add(0, d, entry_pdf(d), skip)
            else:
                for s in of_slot[k - 2]:
                    add(s, d, entry_pdf(d), leave[units[k - 2]] + skip)
    init = np.full(S, -np.inf, F32)
    init[0] = 0
    final = np.full(S, -np.inf, F32)
    final[of_slot[n - 1]] = leave[units[n - 1]]
    if opt[n - 1]:
        final[of_slot[n - 2]] = leave[units[n - 2]] + skip
    order = sorted(arcs)
    col = lambda i, dtype: np.asarray([arcs[a][i] for a in order], dtype=dtype)
    return {"S": S, "P": int(us["P"]), "src": np.asarray([a[0] for a in order], np.int32), "dst": np.asarray([a[1] for a in order], np.int32),
            "pdf": col(0, np.int32), "logprob": col(1, F32), "init": init, "final": final, "label": col(2, np.int32),
            "L": int(num_labels if num_labels is not None else n)}


def transcript_sizes(context, optional):
    """(states, arcs) from the closed forms: S = 1 + n + #B; every state of slot k has 1 + [k+1 < n] + [k+2 < n and opt_k+1] arcs, the start
    1 + [n >= 2 and opt_0]."""
    opt = np.asarray(optional) != 0
    n = len(opt)
    count = np.ones(n, np.int64)
    if context:
        count[1:] += opt[:-1]
    fan = np.ones(n, np.int64)
    fan[:-1] += 1
    fan[:-2] += opt[1:-1]
    return int(1 + count.sum()), int(1 + (n >= 2 and opt[0]) + (count * fan).sum())


def transcript_graph_vectorised(us, units, optional, num_labels=None):
    """transcript_graph's arrays by array arithmetic: per state its three possible arcs, the absent ones masked out."""
    units, opt = np.asarray(units, np.int64), np.asarray(optional) != 0
    n, U, ctx = len(units), int(us["U"]), int(us["context"])
    check_transcript(U, units, opt)
    entry, loop = np.asarray(us["entry_pdf"]).reshape(-1), np.asarray(us["loop_pdf"]).reshape(-1)
    leave, loop_lp = np.asarray(us["leave_logprob"], F32), np.asarray(us["loop_logprob"], F32)
    take, skip = F32(us["take_logprob"]), F32(us["skip_logprob"])
    index = (lambda left, u: (left + 1) * U + u) if ctx else (lambda left, u: u)
    before = np.concatenate([[False], opt[:-1]])            # opt_k-1
    count = 1 + (before if ctx else np.zeros(n, bool))      # states of slot k
    A = 1 + np.cumsum(count) - count                        # A_k
    # the unit states in order: their slot, and the slot of their left neighbour
    slot = np.repeat(np.arange(n), count)
    is_b = np.concatenate([[False], slot[1:] == slot[:-1]])
    left_slot = slot - 1 - is_b
    u_of = units[slot]
    left_unit = np.where(left_slot >= 0, units[np.maximum(left_slot, 0)], -1)
    s = 1 + np.arange(len(slot))
    S = 1 + len(slot)
    pad = lambda a, fill: np.concatenate([a, [fill, fill]])
    units_p, opt_p, A_p, count_p = pad(units, 0), pad(opt, False), pad(A, 0), pad(count, 1)
    has_next, has_skip = slot + 1 < n, (slot + 2 < n) & opt_p[slot + 1]
    w_leave = leave[u_of]
    # per state: loop, enter the next slot, skip over it
    src = np.stack([s, s, s], 1)
    dst = np.stack([s, A_p[slot + 1], A_p[slot + 2] + (1 if ctx else 0)], 1)
    pdf = np.stack([loop[index(left_unit, u_of)], entry[index(u_of, units_p[slot + 1])], entry[index(u_of, units_p[slot + 2])]], 1)
    lp = np.stack([loop_lp[u_of], np.where(opt_p[slot + 1], w_leave + take, w_leave), w_leave + skip], 1).astype(F32)
    label = np.stack([slot, slot + 1, slot + 2], 1)
    keep = np.stack([np.ones(len(slot), bool), has_next, has_skip], 1).reshape(-1)
    # the start's arcs in front
    first = [[0, 1, entry[index(-1, units[0])], F32(0) + take if opt[0] else F32(0), 0]]
    if n >= 2 and opt[0]:
        first.append([0, 3 if ctx else 2, entry[index(-1, units[1])], skip, 1])
    head = lambda i, dtype: np.asarray([f[i] for f in first], dtype)
    flat = lambda a, i, dtype: np.concatenate([head(i, dtype), a.reshape(-1)[keep].astype(dtype)])
    init = np.full(S, -np.inf, F32)
    init[0] = 0
    final = np.full(S, -np.inf, F32)
    final[1:][slot == n - 1] = leave[units[n - 1]]
    if opt[n - 1]:
        final[1:][slot == n - 2] = leave[units[n - 2]] + skip
    return {"S": S, "P": int(us["P"]), "src": flat(src, 0, np.int32), "dst": flat(dst, 1, np.int32), "pdf": flat(pdf, 2, np.int32),
            "logprob": flat(lp, 3, F32), "init": init, "final": final, "label": flat(label, 4, np.int32),
            "L": int(num_labels if num_labels is not None else n)}
