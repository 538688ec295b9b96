"""The labelled entries of the Kaldi-side headers (include/tdnnf_nnet3_adapter.h, include/tdnnf_nnet3_components.h: AlignBestPathLabels,
AlignLabelPosteriorsCompact, AlignLabelPosteriorsSparse) compile with -Wall -Werror and link against the library (tests/label_driver.cc
instantiates all six), and a refusal of the C entry surfaces as an exception that names the call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_label_driver_compiles_links_and_reports_refusals(tmp_path, pkg):
    exe = tmp_path / "label_driver"
    lib_dir = os.path.dirname(pkg.hipabi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "label_driver.cc"),
                           "-o", str(exe), "-L", lib_dir, "-ltdnnf_hip", f"-Wl,-rpath,{lib_dir}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out
    lines = out.stdout.splitlines()
    assert len(lines) == 6, out.stdout
    for line, (who, call) in zip(lines, [(w, c) for c in ("align_best_path_labels", "align_label_posteriors_compact", "align_label_posteriors_sparse")
                                         for w in ("adapter", "components")]):
        assert line.startswith(who) and call + ": " in line, out.stdout
