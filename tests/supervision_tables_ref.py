"""The device tables of a time-synchronous supervision (tdnn-f_nas_amd/csrc/chain_types.h), stated in numpy: what the host loops of
tdnnf_supervision_create upload and what the device build of tdnnf_supervision_assign (chain_sup_build_kernels.h) must give, byte for byte.
`s` is the dict of synth.make_supervision.  tests/test_supervision_tables_ref.py pins this statement by brute force; the GPU tests and the
stand-alone driver of chain_sup_tables.h compare against it."""
import numpy as np

NAMES = ("seq_state_begin", "state_time", "final_logprob", "frame_state_begin", "in_begin", "in_src", "in_pdf", "in_lp", "out_begin", "out_dst",
         "out_pdf", "out_lp", "pf_src", "pf_dst", "pf_pdf", "pf_t", "pf_lp")


def arrays(s):
    """(B, T, seq_state_begin, seq_arc_begin, state_time, final_logprob, arc_src, arc_dst, arc_pdf, arc_logprob) with the C types"""
    i, f = (lambda k: np.ascontiguousarray(s[k], dtype=np.int32)), (lambda k: np.ascontiguousarray(s[k], dtype=np.float32))
    return (int(s["B"]), int(s["T"]), i("seq_state_begin"), i("seq_arc_begin"), i("state_time"), f("final_logprob"), i("arc_src"), i("arc_dst"),
            i("arc_pdf"), f("arc_logprob"))


def tables(s):
    """{name: array} for every name of NAMES: int32, the log-probs float32.
    frame_state_begin[q * (T + 2) + t]: the first state of sequence q with time >= t, t = 0 .. T + 1.
    in_*: the arcs grouped by destination state, in original arc order within a state; in_begin the first of every state's, NS + 1 entries.
    out_*: the same by source state.
    pf_*: the by-source lists, and within every (sequence, frame) -- the by-source range of the states of that time -- ordered by pdf, stably;
    source state, destination state, pdf, frame, log-prob."""
    B, T, ssb, sab, time, fin, src, dst, pdf, lp = arrays(s)
    NS = int(ssb[B])
    fsb = np.concatenate([ssb[q] + np.searchsorted(time[ssb[q]:ssb[q + 1]], np.arange(T + 2), side="left") for q in range(B)]).astype(np.int32)
    t = {"seq_state_begin": ssb, "state_time": time, "final_logprob": fin, "frame_state_begin": fsb}
    by_dst, by_src = np.argsort(dst, kind="stable"), np.argsort(src, kind="stable")
    t["in_begin"] = np.concatenate([[0], np.cumsum(np.bincount(dst, minlength=NS))]).astype(np.int32)
    t["in_src"], t["in_pdf"], t["in_lp"] = src[by_dst], pdf[by_dst], lp[by_dst]
    t["out_begin"] = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=NS))]).astype(np.int32)
    t["out_dst"], t["out_pdf"], t["out_lp"] = dst[by_src], pdf[by_src], lp[by_src]
    # the states are numbered sequence after sequence and by time within one: the frame of a by-source position never decreases
    out_src = src[by_src]
    seq_of_state = np.repeat(np.arange(B), np.diff(ssb))
    frame = seq_of_state[out_src].astype(np.int64) * (T + 1) + time[out_src]
    assert np.all(np.diff(frame) >= 0)
    by_pdf = np.lexsort((t["out_pdf"], frame))  # (stable; the last key is the primary one)
    t["pf_src"], t["pf_dst"], t["pf_pdf"], t["pf_lp"] = out_src[by_pdf], t["out_dst"][by_pdf], t["out_pdf"][by_pdf], t["out_lp"][by_pdf]
    t["pf_t"] = time[t["pf_src"]]
    return {k: np.ascontiguousarray(v, dtype=np.float32 if k.endswith("_lp") or k == "final_logprob" else np.int32) for k, v in t.items()}


def widths(s):
    """{num_states, num_arcs, max_states_per_seq, max_states_per_frame, max_arcs_per_frame, wide} as tdnnf_supervision_create finds them"""
    B, T, ssb, sab, time, fin, src, dst, pdf, lp = arrays(s)
    t = tables(s)
    fsb = t["frame_state_begin"].reshape(B, T + 2)
    return {"num_states": int(ssb[B]), "num_arcs": int(sab[B]), "max_states_per_seq": int(np.diff(ssb).max()),
            "max_states_per_frame": int(np.diff(fsb[:, :T + 2], axis=1).max()),
            "max_arcs_per_frame": int(np.diff(t["out_begin"][fsb], axis=1).max()), "wide": int(int(ssb[B]) > B * 4 * (T + 1))}


def permuted_within_sequences(s, seed=0):
    """`s` with the arcs of every sequence in a random order: the same graphs, and the case that catches an unstable placement"""
    rng = np.random.default_rng(seed)
    sab = np.asarray(s["seq_arc_begin"])
    perm = np.concatenate([sab[q] + rng.permutation(int(sab[q + 1] - sab[q])) for q in range(int(s["B"]))]).astype(np.int64)
    out = dict(s)
    for k in ("arc_src", "arc_dst", "arc_pdf", "arc_logprob"):
        out[k] = np.asarray(s[k])[perm]
    return out


def dead_states():
    """A hand-made supervision of two sequences, T = 3: sequence 0 has a state with no arc in (state 2, time 1: unreachable) and one with no
    arc out (state 3, time 1: a dead end); sequence 1 is a plain chain with two parallel arcs of one pdf."""
    time = [0, 1, 1, 1, 2, 3, 0, 1, 2, 3]
    arcs = [(0, 1, 4, -0.5), (0, 3, 2, -1.0), (1, 4, 1, -0.25), (2, 4, 1, -0.75), (4, 5, 0, 0.0), (1, 4, 0, -2.0),
            (6, 7, 3, -0.5), (6, 7, 3, -1.5), (7, 8, 2, 0.0), (8, 9, 2, -0.125)]
    return {"B": 2, "T": 3, "P": 5, "weight": 1.0, "seq_state_begin": np.asarray([0, 6, 10], np.int32), "seq_arc_begin": np.asarray([0, 6, 10], np.int32),
            "state_time": np.asarray(time, np.int32), "final_logprob": np.asarray([0.0 if x == 3 else -np.inf for x in time], np.float32),
            "arc_src": np.asarray([a[0] for a in arcs], np.int32), "arc_dst": np.asarray([a[1] for a in arcs], np.int32),
            "arc_pdf": np.asarray([a[2] for a in arcs], np.int32), "arc_logprob": np.asarray([a[3] for a in arcs], np.float32)}
