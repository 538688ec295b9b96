"""The supervision lattice of an alignment and a frame tolerance (include/tdnnf_hip.h, "ALIGNMENT SUPERVISIONS") stated in numpy from its
definition -- the windows, the states as (time, kind, unit) triples sorted, the arcs looked up in a dict -- with none of the closed forms of
tdnn-f_nas_amd/csrc/chain_sup_alignment.h.  lattice() returns the supervision dict of synth.make_supervision, which Supervision.assign
takes.  Also the minibatches the tests of the feature share (tests/test_alignment_supervision_ref.py, tests/test_alignment_plan_cpu.py,
tests/test_gpu_assign_alignments.py)."""
import numpy as np

P, U = 12, 5
FRAMES = (1, 2, 7, 40)


def tolerances(T):
    return (0, 1, 2, 5, T + 3)


def windows(starts, T, tol):
    """(lo, hi), n + 1 entries each: the entry windows of the units, tightened, and the virtual unit n that "enters" at T"""
    n = len(starts)
    lo = [max(int(b) - tol, 0) for b in starts]
    hi = [min(int(b) + tol, T - 1) for b in starts]
    lo[0] = hi[0] = 0
    for k in range(1, n):
        lo[k] = max(lo[k], lo[k - 1] + 1)
    lo.append(T)
    hi.append(T)
    for k in range(n - 1, -1, -1):
        hi[k] = min(hi[k], hi[k + 1] - 1)
    return lo, hi


def entry_pdf(us, left, unit):
    return int(us["entry_pdf"][left + 1, unit] if us["context"] else us["entry_pdf"][unit])


def loop_pdf(us, left, unit):
    return int(us["loop_pdf"][left + 1, unit] if us["context"] else us["loop_pdf"][unit])


def sequence(us, units, starts, T, tol):
    """(state_time, final, [(src, dst, pdf)]) of one sequence, states numbered from 0"""
    n = len(units)
    lo, hi = windows(starts, T, tol)
    E, L = 0, 1
    states = [(0, -1, 0)]
    states += [(t, E, k) for k in range(n) for t in range(lo[k] + 1, hi[k] + 2)]
    states += [(t, L, k) for k in range(n) for t in range(lo[k] + 2, hi[k + 1] + 1)]
    states.sort()
    index = {s: i for i, s in enumerate(states)}
    assert len(index) == len(states)
    arcs = [(0, index[(1, E, 0)], entry_pdf(us, -1, units[0]))]
    for i, (t, kind, k) in enumerate(states[1:], start=1):
        if t + 1 <= hi[k + 1]:
            arcs.append((i, index[(t + 1, L, k)], loop_pdf(us, units[k - 1] if k else -1, units[k])))
        if k + 1 < n and lo[k + 1] <= t <= hi[k + 1]:
            arcs.append((i, index[(t + 1, E, k + 1)], entry_pdf(us, units[k], units[k + 1])))
    arcs.sort(key=lambda a: (a[0], a[1]))
    time = [s[0] for s in states]
    final = [0.0 if (t == T and k == n - 1 and kind >= 0) else -np.inf for t, kind, k in states]
    return time, final, arcs


def lattice(us, alignments, T, tol, weight=1.0):
    """The supervision dict of a minibatch: alignments a list of (units, starts) pairs, us a unit set dict (synth.make_unit_set)"""
    time, final, src, dst, pdf = [], [], [], [], []
    ssb, sab = [0], [0]
    for units, starts in alignments:
        t, f, arcs = sequence(us, [int(u) for u in units], [int(b) for b in starts], T, tol)
        base = ssb[-1]
        time += t
        final += f
        src += [base + a[0] for a in arcs]
        dst += [base + a[1] for a in arcs]
        pdf += [a[2] for a in arcs]
        ssb.append(base + len(t))
        sab.append(len(src))
    i32 = lambda x: np.asarray(x, dtype=np.int32)
    return {"B": len(alignments), "T": int(T), "seq_state_begin": i32(ssb), "seq_arc_begin": i32(sab), "state_time": i32(time),
            "final_logprob": np.asarray(final, dtype=np.float32), "arc_src": i32(src), "arc_dst": i32(dst), "arc_pdf": i32(pdf),
            "arc_logprob": np.zeros(len(src), np.float32), "weight": float(weight)}


def random_alignment(rng, T, mean_dur=3.0, num_units=U):
    """(units, starts): durations 1 + floor(Exp(mean_dur - 1)) as synth.make_supervision_lattice draws them, cut at T"""
    d = 1 + np.floor(rng.exponential(max(mean_dur - 1.0, 1e-9), size=T)).astype(np.int64)
    b = np.concatenate([[0], np.cumsum(d)])
    b = b[:int(np.searchsorted(b, T))]
    return rng.integers(0, num_units, size=len(b)).astype(np.int32), b.astype(np.int32)


def unit_set(synth, context):
    return synth.make_unit_set(U, context=context, seed=3 + context, distinct=False, P=P)


def small_batch(T, seed=0):
    """B = 3: one unit; T units of one frame each (a single path for any tolerance); a random segmentation"""
    rng = np.random.default_rng(100 * T + seed)
    return [(rng.integers(0, U, size=1).astype(np.int32), np.zeros(1, np.int32)),
            (rng.integers(0, U, size=T).astype(np.int32), np.arange(T, dtype=np.int32)),
            random_alignment(rng, T, mean_dur=2.5)]


def narrow_batch():
    """B = 4, T = 150, tolerance 5: narrow (`wide` false)"""
    rng = np.random.default_rng(7)
    return [random_alignment(rng, 150, mean_dur=8.0) for _ in range(4)], 150, 5


def wide_batch():
    """B = 2, T = 60, mean duration 1.5, tolerance 40: `wide` true"""
    rng = np.random.default_rng(8)
    return [random_alignment(rng, 60, mean_dur=1.5) for _ in range(2)], 60, 40


def is_wide(sup):
    return len(sup["state_time"]) > int(sup["B"]) * 4 * (int(sup["T"]) + 1)


def flat(alignments):
    """(unit_begin, units, starts) int32 arrays as the C entries take them"""
    begin = np.concatenate([[0], np.cumsum([len(u) for u, _ in alignments])]).astype(np.int32)
    return begin, np.concatenate([np.asarray(u, np.int32) for u, _ in alignments]), np.concatenate([np.asarray(b, np.int32) for _, b in alignments])
