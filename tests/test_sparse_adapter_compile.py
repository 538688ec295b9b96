"""The AlignPosteriorsSparse of the Kaldi-side headers (include/tdnnf_nnet3_adapter.h, include/tdnnf_nnet3_components.h) compile and link
against the library (tests/sparse_driver.cc instantiates both; tests/adapter_driver.cc does not reach them), and a refusal of
tdnnf_align_posteriors_sparse surfaces as an exception that names the call."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sparse_driver_compiles_links_and_reports_refusals(tmp_path, pkg):
    exe = tmp_path / "sparse_driver"
    lib_dir = os.path.dirname(pkg.hipabi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "sparse_driver.cc"),
                           "-o", str(exe), "-L", lib_dir, "-ltdnnf_hip", f"-Wl,-rpath,{lib_dir}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out
    lines = out.stdout.splitlines()
    assert len(lines) == 2 and lines[0].startswith("adapter: ") and lines[1].startswith("components: "), out.stdout
    assert all("align_posteriors_sparse: " in line for line in lines)
