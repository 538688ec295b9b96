"""CPU: the host side of tdnnf_supervision_assign_alignment_chunks (tdnn-f_nas_amd/csrc/chain_sup_alignment.h) as a stand-alone program
under the address and undefined-behaviour sanitizers (tests/alignment_chunk_driver.cc).  For every minibatch the GPU test assigns, the plan
made from the alignments and the chunks alone -- counts, the four maxima, `wide`, frame_state_begin, seq_state_begin, seq_arc_begin, the
sizes entry's answers -- is what sup_validate and sup_widths (chain_sup_tables.h) find on the arrays of the statement
(tests/alignment_chunk_ref.py); the staged slice holds every unit the cut lattice names; the compile kernel's per-state function, run on
the host over slices in allocations of exactly their size, writes the statement's states and arcs; every refusal is checked by its
message, each capacity one short by name, and the staging refusal on a reserve too small for a minibatch of one-frame chunks."""
import os
import subprocess

import numpy as np

from tests import alignment_chunk_ref as chk
from tests import alignment_supervision_ref as ali

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_driver_runs_clean_under_the_sanitizers(tmp_path, pkg):
    exe = tmp_path / "alignment_chunk_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"), os.path.join(ROOT, "tests", "alignment_chunk_driver.cc"), "-o", str(exe)])
    want = []
    with open(tmp_path / "minibatches.txt", "w") as f:
        for context in (0, 1):
            us = ali.unit_set(pkg.synth, context)
            for chunks, T, tol in chk.minibatches():
                s = chk.lattice(us, chunks, T, tol)
                begin, units, starts, utt_frames, chunk_begin = chk.flat(chunks)
                named = [chk.named_units([int(u) for u in al[0]], [int(b) for b in al[1]], Tu, o, T, tol) for al, Tu, o in chunks]
                named = np.asarray([[min(k), max(k)] for k in named], np.int32).reshape(-1)
                f.write("%d %d %d %d %d %d %d %d\n" % (ali.U, context, len(chunks), T, tol, len(units), len(s["state_time"]), len(s["arc_src"])))
                tables = [np.asarray(us[k], np.int32).reshape(-1) for k in ("entry_pdf", "loop_pdf")]
                for a in tables + [begin, units, starts, utt_frames, chunk_begin, named, s["seq_state_begin"], s["seq_arc_begin"], s["state_time"],
                                   s["final_logprob"], s["arc_src"], s["arc_dst"], s["arc_pdf"], s["arc_logprob"]]:
                    f.write(" ".join(("%d" % x) if a.dtype == np.int32 else ("%.9g" % x if np.isfinite(x) else "-1e30") for x in a) + "\n")
                want.append((len(s["state_time"]), len(s["arc_src"]), int(ali.is_wide(s))))
    out = subprocess.run([str(exe), str(tmp_path / "minibatches.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out
    lines = out.stdout.splitlines()
    assert lines[-1] == "0 failures" and lines[-2] == "plans: %d minibatches" % len(want) and len(want) == 84, out.stdout
    assert sum(line.startswith("refusal: ") for line in lines) == 16 and sum(line.startswith("capacity: ") for line in lines) == 4, out.stdout
    assert sum(line.startswith("staging: ") and "short by" in line for line in lines) == 1, out.stdout
    got = [tuple(int(x) for x in line.split()[1:]) for line in lines if line.startswith("minibatch: ")]
    assert [(g[0], g[1], g[6]) for g in got] == want
    assert {w[2] for w in want} == {0, 1}
    # the slices are slices: the 400-frame utterances of the narrow minibatch stage a fraction of their units
    narrow = chk.narrow_batch()[0]
    assert got[-2][7] < sum(len(al[0]) for al, _, _ in narrow) // 2
