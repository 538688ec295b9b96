"""The alignment-chunk calls of the Kaldi-side header (include/tdnnf_nnet3_adapter.h: AlignmentChunkSupervisionSizes,
SupervisionAssignAlignmentChunks) compile and link against the library, and a refusal of each C entry surfaces as an exception that names
it (tests/alignment_chunk_adapter_driver.cc).  And the library declares and exports the two entries, with their Python forms."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adapter_driver_compiles_links_and_reports_refusals(tmp_path, pkg):
    exe = tmp_path / "alignment_chunk_adapter_driver"
    lib_dir = os.path.dirname(pkg.hipabi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "alignment_chunk_adapter_driver.cc"), "-o", str(exe), "-L", lib_dir, "-ltdnnf_hip",
                           f"-Wl,-rpath,{lib_dir}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out
    assert [line.split(":")[0] for line in out.stdout.splitlines()] == ["sizes", "supervision", "components sizes", "components supervision", "components lengths"], out.stdout


def test_the_library_declares_and_exports_the_entries(pkg):
    lib = pkg.hipabi.load()
    for name in ("tdnnf_supervision_assign_alignment_chunks", "tdnnf_alignment_chunk_supervision_sizes"):
        assert name in pkg.hipabi.declared_symbols() and getattr(lib, name)
    assert hasattr(pkg.hipabi.Supervision, "assign_alignment_chunks") and hasattr(pkg.hipabi.UnitSet, "alignment_chunk_sizes")
    assert hasattr(pkg.infer, "chunk_begins") and hasattr(pkg.synth, "supervision_lattice_from_alignment_chunks")


def test_python_refuses_arrays_of_the_wrong_length(pkg):
    with pytest.raises(pkg.hipabi.HipAbiError, match="2 alignments, 1 utt_frames and 2 chunk_begins"):
        pkg.hipabi._chunks(2, [5], [0, 0])
