"""CPU: the host side that the three assign paths share (tdnn-f_nas_amd/csrc/assign_stage.h: tdnnf_align_graphs_assign,
tdnnf_align_graphs_assign_transcripts, tdnnf_supervision_assign) as a stand-alone program under the address and undefined-behaviour
sanitizers (tests/assign_stage_driver.cc): a batch's arrays go into the staging buffer one behind the other, the raw prefix in front of the
arrays that are copied to the handle's own, an empty array takes no bytes and no copy entry, an append beyond the buffer or beyond the copy
list is refused and writes nothing.  And the staging layout of a small labelled batch, written down here: the offsets are device addresses
(the build kernels read the device staging at them), so they are what they were before the packer existed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (offset, length) in bytes of a labelled batch of 2 graphs, 5 states, 7 arcs, 5 pdf columns and 4 label columns in the staging buffer of
# tdnnf_align_graphs_assign: the raw prefix -- state_begin, arc_begin, col_begin, lcol_begin [G + 1], arc_src, arc_dst, arc_pdf,
# arc_logprob [arcs] -- and behind it initial_logprob, final_logprob [states], num_cols [G], col_pdfs, arc_label [arcs], num_lcols [G], col_labels
RAW = [(0, 12), (12, 12), (24, 12), (36, 12), (48, 28), (76, 28), (104, 28), (132, 28)]
DIRECT = [(160, 20), (180, 20), (200, 8), (208, 20), (228, 28), (256, 8), (264, 16)]


def test_the_packer_runs_clean_under_the_sanitizers_and_keeps_the_layout(tmp_path):
    exe = tmp_path / "assign_stage_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"), os.path.join(ROOT, "tests", "assign_stage_driver.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out
    lines = out.stdout.splitlines()
    assert lines[0] == "offsets: 28 raw bytes, 40 in all, 2 copies" and lines[-1] == "0 failures", out.stdout
    assert lines[1:3] == ["refusal: needs 28 bytes of 20", "refusal: copy list full at 8"], out.stdout
    assert lines[4] == "capacity: driver: 9 arcs exceed the capacity max_arcs = 7 by 2", out.stdout
    words = lines[3].split()
    assert words[0] == "layout:" and words[17] == "raw" and words[33] == "copies", lines[3]
    pairs = lambda w: [(int(a), int(b)) for a, b in zip(w[0::2], w[1::2])]
    assert pairs(words[1:17]) == RAW and int(words[18]) == 160 and pairs(words[19:33]) == DIRECT, lines[3]
    assert words[34:] == ["7", "of", "300"] and DIRECT[-1][0] + DIRECT[-1][1] <= 300

