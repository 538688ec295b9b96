"""The reusable-supervision calls of the Kaldi-side headers (include/tdnnf_nnet3_adapter.h, include/tdnnf_nnet3_components.h) compile and
link against the library, and a refusal of each C entry surfaces as an exception that names it (tests/supervision_adapter_driver.cc).  And
the host side of tdnnf_supervision_assign (tdnn-f_nas_amd/csrc/chain_sup_tables.h) as a stand-alone program under the address and
undefined-behaviour sanitizers (tests/supervision_driver.cc): validation against loops from the definition, every refusal of
tdnnf_supervision_create, each capacity one short, and the widths and frame_state_begin of synth.py's minibatches against the numpy
statement (tests/supervision_tables_ref.py)."""
import os
import subprocess

import numpy as np

from tests import supervision_tables_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adapter_driver_compiles_links_and_reports_refusals(tmp_path, pkg):
    exe = tmp_path / "supervision_adapter_driver"
    lib_dir = os.path.dirname(pkg.hipabi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "supervision_adapter_driver.cc"), "-o", str(exe), "-L", lib_dir, "-ltdnnf_hip", f"-Wl,-rpath,{lib_dir}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out
    assert [line.split(":")[0] for line in out.stdout.splitlines()] == ["reserve", "reserve states", "assign", "components reserve", "components assign"], out.stdout


def test_host_driver_runs_clean_under_the_sanitizers(tmp_path, pkg):
    exe = tmp_path / "supervision_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"), os.path.join(ROOT, "tests", "supervision_driver.cc"), "-o", str(exe)])
    from tests.test_supervision_tables_ref import minibatches
    sups = list(minibatches(pkg.synth).values()) + [pkg.synth.make_supervision_lattice(1, 40, 200, tolerance=10, alternatives=12, seed=2)]
    with open(tmp_path / "minibatches.txt", "w") as f:
        for s in sups:
            B, T, *arr = ref.arrays(s)
            f.write("%d %d %d %d\n" % (B, T, len(arr[2]), len(arr[4])))
            for a in arr:
                f.write(" ".join(("%d" % x) if a.dtype == np.int32 else ("%.9g" % x if np.isfinite(x) else "-1e30") for x in a) + "\n")
    out = subprocess.run([str(exe), str(tmp_path / "minibatches.txt")], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out
    lines = out.stdout.splitlines()
    assert lines[0] == "plans: 60 minibatches" and lines[-1] == "0 failures", out.stdout
    assert sum(line.startswith("refusal: ") for line in lines) == 13 and sum(line.startswith("capacity: ") for line in lines) == 4, out.stdout
    got = [line for line in lines if line.startswith(("minibatch: ", "frames:"))]
    assert len(got) == 2 * len(sups)
    for i, s in enumerate(sups):
        w = ref.widths(s)
        assert [int(x) for x in got[2 * i].split()[1:]] == [w[k] for k in ("num_states", "num_arcs", "max_states_per_seq", "max_states_per_frame",
                                                                             "max_arcs_per_frame", "wide")], i
        assert np.array_equal(np.asarray(got[2 * i + 1].split()[1:], dtype=np.int32), ref.tables(s)["frame_state_begin"]), i
