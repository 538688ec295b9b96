"""CPU: the host side of tdnnf_supervision_assign_alignments (tdnn-f_nas_amd/csrc/chain_sup_alignment.h) as a stand-alone program under the
address and undefined-behaviour sanitizers (tests/alignment_driver.cc).  For every minibatch the GPU test assigns, the plan made from the
alignments alone -- counts, the four maxima, `wide`, frame_state_begin, seq_state_begin, seq_arc_begin, the sizes entry's answers -- is what
sup_validate and sup_widths (chain_sup_tables.h) find on the arrays of the numpy statement (tests/alignment_supervision_ref.py); every
refusal is checked by its message, each capacity one short by name."""
import os
import subprocess

import numpy as np

from tests import alignment_supervision_ref as ali

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def minibatches():
    out = [(ali.small_batch(T), T, tol) for T in ali.FRAMES for tol in ali.tolerances(T)]
    return out + [ali.narrow_batch(), ali.wide_batch()]


def test_host_driver_runs_clean_under_the_sanitizers(tmp_path, pkg):
    exe = tmp_path / "alignment_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"), os.path.join(ROOT, "tests", "alignment_driver.cc"), "-o", str(exe)])
    want = []
    with open(tmp_path / "minibatches.txt", "w") as f:
        for context in (0, 1):
            us = ali.unit_set(pkg.synth, context)
            for al, T, tol in minibatches():
                s = ali.lattice(us, al, T, tol)
                begin, units, starts = ali.flat(al)
                f.write("%d %d %d %d %d %d %d\n" % (ali.U, len(al), T, tol, len(units), len(s["state_time"]), len(s["arc_src"])))
                for a in (begin, units, starts, s["seq_state_begin"], s["seq_arc_begin"], s["state_time"], s["final_logprob"], s["arc_src"], s["arc_dst"],
                          s["arc_pdf"], s["arc_logprob"]):
                    f.write(" ".join(("%d" % x) if a.dtype == np.int32 else ("%.9g" % x if np.isfinite(x) else "-1e30") for x in a) + "\n")
                want.append((len(s["state_time"]), len(s["arc_src"]), int(ali.is_wide(s))))
    out = subprocess.run([str(exe), str(tmp_path / "minibatches.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out
    lines = out.stdout.splitlines()
    assert lines[-1] == "0 failures" and lines[-2] == "plans: %d minibatches" % len(want) and len(want) == 44, out.stdout
    assert sum(line.startswith("refusal: ") for line in lines) == 11 and sum(line.startswith("capacity: ") for line in lines) == 4, out.stdout
    got = [tuple(int(x) for x in line.split()[1:]) for line in lines if line.startswith("minibatch: ")]
    assert [(g[0], g[1], g[6]) for g in got] == want
    assert {w[2] for w in want} == {0, 1}
