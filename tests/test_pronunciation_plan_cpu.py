"""CPU: the host side of tdnnf_align_graphs_assign_pronunciations (tdnn-f_nas_amd/csrc/align_pronunciations.h) as a stand-alone program
under the address and undefined-behaviour sanitizers (tests/pronunciation_driver.cc).  For every batch the GPU test assigns, in both
contexts, the plan made from the flat arrays alone -- begins, arcs and largest in-degree per graph, the column lists, the first state of
every position, the sizes entry's answers -- is what the numpy statement (tests/pronunciation_graphs_ref.py) has on its arc arrays; every
refusal is checked by its message, each capacity one short by name.  And the three adapter methods compile, link and report a refusal
(tests/pronunciation_adapter_driver.cc)."""
import os
import subprocess

import numpy as np

from tests import pronunciation_graphs_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def batches(synth):
    random = synth.make_pronunciation_transcripts(40, ref.U, seed=2)
    return [ref.edge_batch(), [ref.edge_batch()[4]], [ref.long_transcript()], [ref.heavy_transcript()], random]


def first_states(g, positions):
    """The first state of every position on the statement's state list."""
    first = {}
    for s, st in enumerate(g["states"]):
        if st is not None:
            first.setdefault(st[0][0], s)
    return [first[p] for p in range(len(positions))]


def test_host_driver_runs_clean_under_the_sanitizers(tmp_path, pkg):
    exe = tmp_path / "pronunciation_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"), os.path.join(ROOT, "tests", "pronunciation_driver.cc"), "-o", str(exe)])
    want = []
    with open(tmp_path / "batches.txt", "w") as f:
        for context in (0, 1):
            for distinct in (True, False):
                us = ref.unit_set(pkg.synth, context, distinct)
                for batch in batches(pkg.synth):
                    graphs = [ref.pronunciation_graph(us, t) for t in batch]
                    flat = ref.flat_arrays(batch)
                    cols = [np.unique(g["pdf"]) for g in graphs]
                    degree = [int(np.bincount(g["dst"], minlength=g["S"]).max()) for g in graphs]
                    begin = lambda counts: np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
                    f.write("%d %d %d %d %d %d %d\n" % (ref.U, context, us["P"], len(batch), len(flat[1]), len(flat[3]), len(flat[5])))
                    arrays = [np.asarray(us["entry_pdf"], np.int32).reshape(-1), np.asarray(us["loop_pdf"], np.int32).reshape(-1), *flat,
                              begin([g["S"] for g in graphs]), begin([len(g["src"]) for g in graphs]), np.asarray(degree, np.int32),
                              begin([len(c) for c in cols]), np.concatenate(cols).astype(np.int32),
                              np.asarray([s for g, t in zip(graphs, batch) for s in first_states(g, t[0])], np.int32)]
                    for a in arrays:
                        f.write(" ".join(("%d" % x) if a.dtype == np.int32 else ("%.9g" % x) for x in a) + "\n")
                    for g in graphs:  # the statement's own shape: the labels are the entries, every one of them
                        assert np.array_equal(np.unique(g["label"]), np.arange(g["L"]))
                    want.append((len(batch), sum(g["S"] for g in graphs), sum(len(g["src"]) for g in graphs), max(degree)))
    out = subprocess.run([str(exe), str(tmp_path / "batches.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out
    lines = out.stdout.splitlines()
    assert lines[-1] == "0 failures" and "plans: %d batches" % len(want) in lines and len(want) == 20, out.stdout
    assert sum(line.startswith("refusal: ") for line in lines) == 12 and sum(line.startswith("capacity: ") for line in lines) == 3, out.stdout
    got = [tuple(int(x) for x in line.split()[1:]) for line in lines if line.startswith("batch: ")]
    assert got == want
    assert max(w[3] for w in want) > 64  # a row beyond kAlignHeavy is among them


def test_adapter_driver_compiles_links_and_reports_refusals(tmp_path, pkg):
    exe = tmp_path / "pronunciation_adapter_driver"
    lib_dir = os.path.dirname(pkg.hipabi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "pronunciation_adapter_driver.cc"), "-o", str(exe), "-L", lib_dir, "-ltdnnf_hip", f"-Wl,-rpath,{lib_dir}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out
    assert [line.split(":")[0] for line in out.stdout.splitlines()] == ["sizes", "graphs", "supervision", "components sizes", "components graphs",
                                                                   "components supervision"], out.stdout


def test_the_library_declares_and_exports_the_pronunciation_entries(pkg):
    lib = pkg.hipabi.load()
    for name in ("tdnnf_pronunciation_graph_sizes", "tdnnf_align_graphs_assign_pronunciations", "tdnnf_supervision_assign_e2e_pronunciations"):
        assert name in pkg.hipabi.declared_symbols() and getattr(lib, name)
    assert hasattr(pkg.hipabi.UnitSet, "pronunciation_sizes") and hasattr(pkg.hipabi.AlignGraphs, "assign_pronunciations")
    assert hasattr(pkg.hipabi.Supervision, "assign_pronunciations") and hasattr(pkg.synth, "make_pronunciation_transcripts")
    assert hasattr(pkg.infer, "alignment_from_pronunciation_path")
