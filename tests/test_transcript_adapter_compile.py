"""The transcript calls of the Kaldi-side header (include/tdnnf_nnet3_adapter.h) compile and link against the library, and a refusal of each
C entry surfaces as an exception that names it (tests/transcript_adapter_driver.cc).  And the host side of the transcript compile
(tdnn-f_nas_amd/csrc/align_transcripts.h) as a stand-alone program under the address and undefined-behaviour sanitizers
(tests/transcript_driver.cc): every pattern of optional slots up to 11 slots against a graph built arc by arc, and the refusals."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_adapter_driver_compiles_links_and_reports_refusals(tmp_path, pkg):
    exe = tmp_path / "transcript_adapter_driver"
    lib_dir = os.path.dirname(pkg.hipabi.LIB_PATH)
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "transcript_adapter_driver.cc"), "-o", str(exe), "-L", lib_dir, "-ltdnnf_hip", f"-Wl,-rpath,{lib_dir}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out
    lines = out.stdout.splitlines()
    assert [line.split(":")[0] for line in lines] == ["unit set", "graphs", "supervision", "components unit set", "components sizes", "components graphs",
                                                      "components supervision"], out.stdout


def test_host_driver_runs_clean_under_the_sanitizers(tmp_path):
    exe = tmp_path / "transcript_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                           os.path.join(ROOT, "tdnn-f_nas_amd", "csrc"), os.path.join(ROOT, "tests", "transcript_driver.cc"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and out.stderr == "", out
    lines = out.stdout.splitlines()
    assert lines[0].startswith("sizes and plans: ") and lines[-1] == "0 failures" and sum(line.startswith("refusal: ") for line in lines) == 7, out.stdout
