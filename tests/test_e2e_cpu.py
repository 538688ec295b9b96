"""CPU-side checks of the end-to-end supervision's plumbing: the two new C-ABI names are declared and exported, and
trainer.shard_supervision slices an end-to-end dict by sequence while leaving the time-synchronous dict's result as it was."""
import subprocess

import numpy as np


def test_new_symbols_are_declared_and_exported(pkg):
    names = pkg.hipabi.declared_symbols()
    new = {"tdnnf_supervision_create_e2e", "tdnnf_supervision_kind"}
    assert new <= set(names)
    pkg.hipabi.load()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.hipabi.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert new <= exported
    res, args = pkg.hipabi._prototypes()["tdnnf_supervision_create_e2e"]
    assert len(args) == 13 and pkg.hipabi.load().tdnnf_abi_version() == 1


def test_shard_supervision_on_an_end_to_end_dict(pkg):
    e2e = pkg.synth.make_e2e_supervision(5, 7, 41, seed=2, weight=0.5)
    a, b = pkg.trainer.shard_supervision(e2e, 0, 2), pkg.trainer.shard_supervision(e2e, 2, 5)
    assert (a["B"], b["B"]) == (2, 3) and len(e2e["graphs"]) == e2e["B"] == 5
    for sh, lo in ((a, 0), (b, 2)):
        assert (sh["T"], sh["P"], sh["weight"]) == (7, 41, 0.5)
        assert len(sh["graphs"]) == sh["B"]
        for i, g in enumerate(sh["graphs"]):
            assert g is e2e["graphs"][lo + i]


def test_shard_supervision_is_unchanged_on_the_time_synchronous_dict(pkg):
    sup = pkg.synth.make_supervision(5, 6, 11, max_alt=2, seed=3, weight=0.5)
    sh = pkg.trainer.shard_supervision(sup, 2, 5)
    # the expected shard, cut out here: states and arcs of sequences 2 .. 4, renumbered from 0
    sb, ab = sup["seq_state_begin"], sup["seq_arc_begin"]
    s0, s1, a0, a1 = int(sb[2]), int(sb[5]), int(ab[2]), int(ab[5])
    want = dict(B=3, T=6, weight=0.5, seq_state_begin=sb[2:] - s0, seq_arc_begin=ab[2:] - a0, state_time=sup["state_time"][s0:s1],
                final_logprob=sup["final_logprob"][s0:s1], arc_src=sup["arc_src"][a0:a1] - s0, arc_dst=sup["arc_dst"][a0:a1] - s0,
                arc_pdf=sup["arc_pdf"][a0:a1], arc_logprob=sup["arc_logprob"][a0:a1])
    assert set(sh) == set(want) and "graphs" not in sh
    for k, v in want.items():
        assert np.array_equal(np.asarray(sh[k]), np.asarray(v)), k
    assert sh["seq_state_begin"].dtype == np.int32 and sh["arc_src"].dtype == np.int32
