"""The chunk-input calls of the Kaldi-side header (include/tdnnf_nnet3_adapter.h: ChunkInputCreate, ChunkInputGather) compile and link
against the library, and a refusal of each C entry surfaces as an exception that names it (tests/chunk_input_adapter_driver.cc).  And the
library declares and exports the entries, with their Python forms."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adapter_driver_compiles_links_and_reports_refusals(tmp_path, pkg):
    exe = tmp_path / "chunk_input_adapter_driver"
    lib_dir = os.path.dirname(pkg.hipabi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "chunk_input_adapter_driver.cc"), "-o", str(exe), "-L", lib_dir, "-ltdnnf_hip",
                           f"-Wl,-rpath,{lib_dir}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out
    assert [line.split(":")[0] for line in out.stdout.splitlines()] == ["create", "gather", "gather without i-vectors", "gather without an output", "components create",
                                                                       "components gather", "components lengths", "plan"], out.stdout


def test_the_library_declares_and_exports_the_entries(pkg):
    lib = pkg.hipabi.load()
    for name in ("tdnnf_chunk_input_create", "tdnnf_chunk_input_destroy", "tdnnf_chunk_input_plan", "tdnnf_chunk_input_gather", "tdnnf_chunk_input_info"):
        assert name in pkg.hipabi.declared_symbols() and getattr(lib, name)
    for name in ("plan", "gather", "info"):
        assert hasattr(pkg.hipabi.ChunkInput, name)
    for name in ("minibatches_from_utterances", "write_chunk_egs", "utterance_chunks", "chunk_minibatches"):
        assert hasattr(pkg.egs, name)
    assert lib.tdnnf_abi_version() == 1


def test_python_refuses_arrays_of_the_wrong_length(pkg):
    with pytest.raises(pkg.hipabi.HipAbiError, match="2 seq_utt and 1 chunk_begins"):
        pkg.hipabi._sequence_chunks([0, 1], [0])
