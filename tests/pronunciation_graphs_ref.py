"""The graph of a transcript with pronunciation alternatives as include/tdnnf_hip.h ("PRONUNCIATION GRAPHS") defines it, in numpy with
float32 weights: what tdnnf_align_graphs_assign_pronunciations compiles on the device.  A transcript is (positions, optional[, alt_logprob]):
positions[p] a list of unit sequences (the alternatives of position p), optional[p] its flag, alt_logprob[p] one float per alternative
(default 0).  pronunciation_graph walks the definition state by state and returns synth.make_alignment_graph's dict {S, P, src, dst, pdf,
logprob, init, final} plus "label", "L" and, for the tests, "states": per state (entry, predecessor) -- the predecessor of a first entry's
state is (position, alternative), (-1, 0) for the start; None for an inner entry.  An entry is one unit of one alternative, numbered from 0
in flat order (position, alternative, unit)."""
import numpy as np

F32 = np.float32


def normalise(transcript):
    """(positions as lists of lists of ints, optional as bools, alt_logprob as lists of float32) of a transcript given with or without its
    third member."""
    positions = [[[int(u) for u in alt] for alt in pos] for pos in transcript[0]]
    opt = [bool(o) for o in transcript[1]]
    if len(transcript) > 2 and transcript[2] is not None:
        logp = [[F32(x) for x in row] for row in transcript[2]]
    else:
        logp = [[F32(0)] * len(pos) for pos in positions]
    return positions, opt, logp


def check_transcript(U, positions, opt, logp):
    """The refusals of the definition, as assertions."""
    assert len(positions) == len(opt) == len(logp) >= 1
    for pos, row in zip(positions, logp):
        assert len(pos) >= 1, "a position without an alternative"
        assert len(row) == len(pos)
        assert all(np.isfinite(x) for x in row), "an alt_logprob that is NaN or infinite"
        for alt in pos:
            assert len(alt) >= 1, "an empty alternative"
            assert all(0 <= u < U for u in alt), "a unit outside [0, U)"
    assert not any(a and b for a, b in zip(opt[1:], opt[:-1])), "adjacent optional positions"
    assert not all(opt), "no mandatory position"


def entry_numbers(positions):
    """{(p, a, j): entry number}, in flat order."""
    numbers = {}
    for p, pos in enumerate(positions):
        for a, alt in enumerate(pos):
            for j in range(len(alt)):
                numbers[(p, a, j)] = len(numbers)
    return numbers


def pronunciation_graph(us, transcript, num_labels=None):
    """us: a unit set dict (synth.make_unit_set)."""
    positions, opt, logp = normalise(transcript)
    n, U, ctx = len(positions), int(us["U"]), int(us["context"])
    check_transcript(U, positions, opt, logp)
    entry, loop = np.asarray(us["entry_pdf"]), np.asarray(us["loop_pdf"])
    leave, loop_lp = np.asarray(us["leave_logprob"], F32), np.asarray(us["loop_logprob"], F32)
    take, skip = F32(us["take_logprob"]), F32(us["skip_logprob"])
    pdf_of = lambda table, left, u: int(table[left + 1, u] if ctx else table[u])
    START = (-1, 0)
    number = entry_numbers(positions)

    def alternatives(p):  # of position p; the start stands in for a position -1
        return [START] if p < 0 else [(p, a) for a in range(len(positions[p]))]

    def predecessors(p):  # the near ones, then the far ones
        return alternatives(p - 1) + (alternatives(p - 2) if p >= 1 and opt[p - 1] else [])

    last_unit = lambda q: -1 if q == START else positions[q[0]][q[1]][-1]

    # the states: state 0 is the start, the entries follow in flat order
    states = [None]            # per state ((p, a, j), predecessor or None)
    left = [None]              # per state its left unit
    of_entry = {}              # (p, a, j) -> its states; a first entry's in the order of predecessors(p)
    for p, pos in enumerate(positions):
        for a, alt in enumerate(pos):
            for j in range(len(alt)):
                if j > 0:
                    mine = [(None, alt[j - 1])]
                elif ctx:
                    mine = [(q, last_unit(q)) for q in predecessors(p)]
                else:
                    mine = [(None, -1)]
                of_entry[(p, a, j)] = list(range(len(states), len(states) + len(mine)))
                for q, l in mine:
                    states.append(((p, a, j), q))
                    left.append(l)
    S = len(states)
    unit_of = lambda s: positions[states[s][0][0]][states[s][0][1]][states[s][0][2]]
    entry_pdf = lambda s: pdf_of(entry, left[s], unit_of(s))
    loop_pdf = lambda s: pdf_of(loop, left[s], unit_of(s))

    def state_for(p, a, q):  # the state of first entry (p, a, 0) that belongs to predecessor q
        return of_entry[(p, a, 0)][predecessors(p).index(q) if ctx else 0]

    arcs = {}  # (src, dst) -> (pdf, weight, label)

    def add(src, dst, pdf, w):
        assert (src, dst) not in arcs
        arcs[(src, dst)] = (pdf, F32(w), number[states[dst][0]])

    def leave_arcs(sources, q, base):
        """The arcs out of the last entry of alternative q = (p, a) -- sources: its states; base: leave_logprob of its unit, None for the
        start -- into position p + 1 and, over an optional position p + 1, into position p + 2."""
        p = q[0]
        if p + 1 < n:
            for a2 in range(len(positions[p + 1])):
                w = (F32(0) + take if opt[p + 1] else F32(0)) if base is None else (base + take if opt[p + 1] else base)
                if len(positions[p + 1]) >= 2:
                    w = w + logp[p + 1][a2]
                d = state_for(p + 1, a2, q)
                for s in sources:
                    add(s, d, entry_pdf(d), w)
        if p + 2 < n and opt[p + 1]:
            for a2 in range(len(positions[p + 2])):
                w = skip if base is None else base + skip
                if len(positions[p + 2]) >= 2:
                    w = w + logp[p + 2][a2]
                d = state_for(p + 2, a2, q)
                for s in sources:
                    add(s, d, entry_pdf(d), w)

    leave_arcs([0], START, None)
    for p, pos in enumerate(positions):
        for a, alt in enumerate(pos):
            for j, u in enumerate(alt):
                mine = of_entry[(p, a, j)]
                for s in mine:
                    add(s, s, loop_pdf(s), loop_lp[u])
                if j + 1 < len(alt):
                    d, = of_entry[(p, a, j + 1)]
                    for s in mine:
                        add(s, d, entry_pdf(d), leave[u])
                else:
                    leave_arcs(mine, (p, a), leave[u])
    init = np.full(S, -np.inf, F32)
    init[0] = 0
    final = np.full(S, -np.inf, F32)
    for a, alt in enumerate(positions[n - 1]):
        final[of_entry[(n - 1, a, len(alt) - 1)]] = leave[alt[-1]]
    if opt[n - 1] and n >= 2:
        for a, alt in enumerate(positions[n - 2]):
            final[of_entry[(n - 2, a, len(alt) - 1)]] = leave[alt[-1]] + skip
    order = sorted(arcs)
    col = lambda i, dtype: np.asarray([arcs[a][i] for a in order], dtype=dtype)
    return {"S": S, "P": int(us["P"]), "src": np.asarray([a[0] for a in order], np.int32), "dst": np.asarray([a[1] for a in order], np.int32),
            "pdf": col(0, np.int32), "logprob": col(1, F32), "init": init, "final": final, "label": col(2, np.int32),
            "L": int(num_labels if num_labels is not None else len(number)), "states": states, "left": left}


def as_slots(units, optional):
    """The slot transcript (units, optional) of tests/transcript_graphs_ref.py as a pronunciation transcript: every position one alternative of
    one unit."""
    return [[[int(u)]] for u in units], [bool(o) for o in optional]


def flat_arrays(transcripts):
    """The six flat arrays of the C entries for a batch: pos_begin, pos_optional, pos_alt_begin, alt_logprob, alt_unit_begin, alt_units."""
    pos_begin, pos_optional, pos_alt_begin, alt_logprob, alt_unit_begin, alt_units = [0], [], [0], [], [0], []
    for t in transcripts:
        positions, opt, logp = normalise(t)
        for pos, o, row in zip(positions, opt, logp):
            pos_optional.append(int(o))
            for alt, lp in zip(pos, row):
                alt_logprob.append(lp)
                alt_units += alt
                alt_unit_begin.append(len(alt_units))
            pos_alt_begin.append(len(alt_logprob))
        pos_begin.append(len(pos_optional))
    i32 = lambda a: np.asarray(a, np.int32)
    return i32(pos_begin), i32(pos_optional), i32(pos_alt_begin), np.asarray(alt_logprob, F32), i32(alt_unit_begin), i32(alt_units)


# ---- the batches the CPU driver and the GPU tests share: the smallest shapes at which the compile can go wrong

U = 6


def unit_set(synth, context, distinct=True):
    return synth.make_unit_set(U, context=context, seed=11 + context, distinct=distinct)


def edge_batch():
    """7 transcripts of 1 to 6 positions, 1 to 3 alternatives of 1 to 3 units: an optional position first, last, and between two
    multi-alternative positions; one-unit alternatives on both sides of an optional position (the largest first-entry state counts); equal
    last units among a position's alternatives (states that are not merged)."""
    eighths = lambda *x: [F32(-v / 8.0) for v in x]
    return [
        ([[[3]]], [0]),
        ([[[1, 2], [4]], [[0], [5, 5, 1], [2]]], [0, 0], [eighths(1, 3), eighths(0, 2, 16)]),
        ([[[2]], [[0, 1], [3]], [[4], [4, 2]]], [1, 0, 0], [eighths(0), eighths(5, 1), eighths(2, 2)]),                 # optional first
        ([[[1], [2, 3]], [[5]], [[0], [1], [3, 3, 3]], [[2]]], [0, 0, 0, 1], [eighths(1, 1), eighths(7), eighths(3, 0, 9), eighths(4)]),  # last
        ([[[0, 1], [2], [3, 4, 5]], [[1], [0, 0]], [[5], [4, 1], [2]], [[3]], [[1, 1]]], [0, 1, 0, 0, 0],
         [eighths(1, 2, 3), eighths(6, 0), eighths(2, 8, 1), eighths(0), eighths(5)]),                                    # between two
        ([[[4], [1], [0]], [[2], [3]], [[5], [5], [1]], [[0]], [[2], [4]], [[3], [1, 2]]], [0, 1, 0, 1, 0, 0],
         [eighths(1, 0, 2), eighths(3, 4), eighths(0, 5, 1), eighths(2), eighths(6, 1), eighths(0, 7)]),                  # one-unit alternatives round optional positions
        ([[[5, 0, 1]], [[2, 2]]], [0, 1]),
    ]


def long_transcript(seed=5):
    """One transcript of more than 256 entries (the kernel's chunk carries): 90 positions, every third optional."""
    rng = np.random.default_rng(seed)
    positions, opt, logp = [], [], []
    for p in range(90):
        A = int(rng.integers(1, 4))
        positions.append([[int(u) for u in rng.integers(0, U, size=int(rng.integers(1, 4)))] for _ in range(A)])
        logp.append([F32(-int(x) / 8.0) for x in rng.integers(0, 17, size=A)])
        opt.append(int(p % 3 == 1))
    assert sum(len(alt) for pos in positions for alt in pos) > 256
    return positions, opt, logp


def heavy_transcript():
    """Two positions of 65 one-unit alternatives, one behind the other, between two plain ones: the first entries of the second have 65
    states each, so 66 arcs enter every state of the position behind it (context 1) or of itself (context 0): a row beyond kAlignHeavy."""
    many = lambda shift: [[(a + shift) % U] for a in range(65)]
    logp = lambda shift: [F32(-((a + shift) % 17) / 8.0) for a in range(65)]
    return [[[1, 2]], many(0), many(1), [[3], [0, 4]]], [0, 0, 0, 0], [[F32(0)], logp(0), logp(3), [F32(-0.5), F32(-0.25)]]
