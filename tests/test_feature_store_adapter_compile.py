"""The feature-store calls of the Kaldi-side header (include/tdnnf_nnet3_adapter.h: FeatureStoreCreate, FeatureStoreAppend,
FeatureStoreExpand, ChunkInputGatherStored) compile and link against the library, and a refusal of each C entry surfaces as an exception that
names it (tests/feature_store_adapter_driver.cc).  And the library declares and exports the entries, with their Python forms."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adapter_driver_compiles_links_and_reports_refusals(tmp_path, pkg):
    exe = tmp_path / "feature_store_adapter_driver"
    lib_dir = os.path.dirname(pkg.hipabi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "feature_store_adapter_driver.cc"), "-o", str(exe), "-L", lib_dir, "-ltdnnf_hip",
                           f"-Wl,-rpath,{lib_dir}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out
    assert [line.split(":")[0] for line in out.stdout.splitlines()] == ["create", "create capacities", "append", "expand", "expand without an output", "gather",
                                                                       "gather without an output", "components create", "components append", "components expand",
                                                                       "components gather", "components lengths", "layout and pack", "compress", "pack"], out.stdout


def test_the_library_declares_and_exports_the_entries(pkg):
    lib = pkg.hipabi.load()
    for name in ("create", "destroy", "layout", "pack", "compress", "append", "append_float", "expand", "info", "frames"):
        assert "tdnnf_feature_store_" + name in pkg.hipabi.declared_symbols() and getattr(lib, "tdnnf_feature_store_" + name)
    assert "tdnnf_chunk_input_gather_stored" in pkg.hipabi.declared_symbols() and lib.tdnnf_chunk_input_gather_stored
    for name in ("append", "append_float", "expand", "utterances", "info", "layout", "pack"):
        assert hasattr(pkg.hipabi.FeatureStore, name)
    assert hasattr(pkg.hipabi.ChunkInput, "gather_stored")
    for name in ("minibatches_from_store", "read_feature_archive", "write_feature_archive"):
        assert hasattr(pkg.egs, name)
    assert lib.tdnnf_abi_version() == 1
