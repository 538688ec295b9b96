"""The alignment-supervision calls of the Kaldi-side header (include/tdnnf_nnet3_adapter.h: AlignmentSupervisionSizes,
SupervisionAssignAlignments) compile and link against the library, and a refusal of each C entry surfaces as an exception that names it
(tests/alignment_adapter_driver.cc).  And the library declares and exports the two entries, with their Python forms."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adapter_driver_compiles_links_and_reports_refusals(tmp_path, pkg):
    exe = tmp_path / "alignment_adapter_driver"
    lib_dir = os.path.dirname(pkg.hipabi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "alignment_adapter_driver.cc"), "-o", str(exe), "-L", lib_dir, "-ltdnnf_hip", f"-Wl,-rpath,{lib_dir}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out
    assert [line.split(":")[0] for line in out.stdout.splitlines()] == ["sizes", "supervision", "components sizes", "components supervision"], out.stdout


def test_the_library_declares_and_exports_the_entries(pkg):
    lib = pkg.hipabi.load()
    for name in ("tdnnf_supervision_assign_alignments", "tdnnf_alignment_supervision_sizes"):
        assert name in pkg.hipabi.declared_symbols() and getattr(lib, name)
    assert hasattr(pkg.hipabi.Supervision, "assign_alignments") and hasattr(pkg.hipabi.UnitSet, "alignment_sizes")
    assert hasattr(pkg.infer, "alignment_from_path")


def test_alignment_from_path_drops_skipped_slots(pkg):
    import numpy as np
    import pytest
    transcript = (np.asarray([4, 0, 2, 3]), np.asarray([0, 1, 0, 0]))
    units, starts = pkg.infer.alignment_from_path([0, 0, 2, 2, 2, 3], transcript)  # (slot 1, optional, was skipped)
    assert units.tolist() == [4, 2, 3] and starts.tolist() == [0, 2, 5] and units.dtype == np.int32 == starts.dtype
    units, starts = pkg.infer.alignment_from_path([0, 1, 2, 3], transcript)
    assert units.tolist() == [4, 0, 2, 3] and starts.tolist() == [0, 1, 2, 3]
    for bad in ([], [-1, -1], [0, 2, 1], [0, 4]):
        with pytest.raises(ValueError, match="alignment_from_path"):
            pkg.infer.alignment_from_path(bad, transcript)
