"""CPU-side checks of the boundary: the library loads without a GPU and exports every symbol
include/tdnnf_hip.h declares; argument validation rejects bad calls before anything is launched."""
import ctypes as C
import os
import subprocess

import pytest


def test_library_exports_every_declared_symbol(pkg):
    lib = pkg.hipabi.load()
    names = pkg.hipabi.declared_symbols()
    assert len(names) >= 50
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.hipabi.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    assert set(names) <= exported, sorted(set(names) - exported)
    assert {"tdnnf_gemm_launch_forms", "tdnnf_gemm_launch_form_name", "tdnnf_fused_launch_forms", "tdnnf_fused_launch_form_name"} <= set(names)
    assert lib.tdnnf_abi_version() == 1


def test_fused_form_counters_are_named_and_start_at_zero(pkg):
    """tdnnf_fused_launch_forms needs no GPU: every counter has a name of its own, none outside the range, and nothing has counted."""
    lib = pkg.hipabi.load()
    n = lib.tdnnf_fused_launch_forms(None, 0, 1)
    names = [lib.tdnnf_fused_launch_form_name(i).decode() for i in range(n)]
    assert n > 0 and len(set(names)) == n and lib.tdnnf_fused_launch_form_name(n) is None and lib.tdnnf_fused_launch_form_name(-1) is None
    for want in ("apply_bypass.vec4.super.mask.rev", "apply_bypass.planes", "bwd.reduce.scalar.nostats", "bwd.finalize.test", "bwd.apply.planes.mask.rev",
                 "bwd.apply.rows_tail", "bwd.apply_ng.nt3.mask.planes.rev", "bwd.apply_ng.partial_block", "bwd.repair"):
        assert want in names, want
    assert pkg.hipabi.fused_forms() == {}


def test_one_hip_runtime_per_process():
    """build() then smoke() in ONE fresh process (what a driver may do): the library must come up on the HIP runtime torch
    brought, whichever is asked for first -- a second runtime in the process sees no device (hipErrorNoDevice at the first
    launch).  Checked without a GPU through the mapped files: exactly one libamdhip64 after load()."""
    import subprocess
    import sys
    code = ("import __graft_entry__ as g; p = g.load_package(); p.hipabi.load(); import torch; "
            "m = sorted({l.split()[-1] for l in open('/proc/self/maps') if 'libamdhip64' in l}); print(len(m), m)")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.split()[0] == "1", out.stdout


def test_code_object_is_gfx950_only(pkg, tmp_path):
    # (llvm-objdump --offloading EXTRACTS every bundle as a file beside its input -- libtdnnf_hip.so.N.hipv4-... / .host-...: 17.8 MB of
    # leftovers in the package directory per run until round 5; it works on a copy in a scratch directory now)
    import shutil
    copy = tmp_path / "libtdnnf_hip.so"
    shutil.copy(pkg.hipabi.LIB_PATH, copy)
    out = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-objdump", "--offloading", str(copy)], capture_output=True, text=True, cwd=str(tmp_path))
    text = out.stdout + out.stderr
    if "gfx" in text:
        assert "gfx950" in text and "gfx90a" not in text and "gfx942" not in text


def test_argument_validation_without_gpu(pkg):
    lib = pkg.hipabi.load()
    M = pkg.hipabi.Mat
    a = M(None, 4, 8, 8)      # rows*cols != 0 with a null pointer
    rc = lib.tdnnf_relu_propagate(C.byref(a), C.byref(a), None)
    assert rc == 1 and b"relu_propagate" in lib.tdnnf_last_error()
    rc = lib.tdnnf_constrain_orthonormal(0.0, None, 4, 8, 8, None, 0, None)
    assert rc == 1
    assert lib.tdnnf_tdnn_update_workspace_bytes(160, 1536, 2, 19200) > 0
    assert lib.tdnnf_colreduce_workspace_bytes(19200, 1536) > 0


def test_product_never_touches_the_oracle():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for dirpath, _, files in os.walk(os.path.join(root, "tdnn-f_nas_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp", "Makefile")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "oracle" not in text.lower(), os.path.join(dirpath, f)


def test_training_schedule_restates_train_py(pkg):
    """steps/nnet3/chain/train.py:473-531 + common.py:606-618 + temperature_schedule.py:51 for a 2 -> 4 job ramp."""
    tr = pkg.trainer
    sched = list(tr.training_schedule(num_iters=6, num_archives_to_process=18, num_jobs_initial=2, num_jobs_final=4, use_temperature_schedule=True))
    assert [s["num_jobs"] for s in sched] == [2, 2, 3, 3, 3, 4]
    processed = [0, 2, 4, 7, 10, 13]
    for s, p in zip(sched, processed):
        assert abs(s["data_fraction"] - p / 18.0) < 1e-12
        assert abs(s["temperature_proportion"] - ((1 - p / 18.0) * 0.97 + 0.03)) < 1e-12
    import math
    assert abs(sched[2]["learning_rate"] - 3 * 2.5e-4 * math.exp(4 * math.log(0.1) / 18)) < 1e-12
    assert abs(sched[-1]["learning_rate"] - 4 * 2.5e-5) < 1e-15  # the last iteration runs at the final rate
    assert abs(tr.temperature(1.0, 0.1, 0.5) - 10 ** -0.5) < 1e-12 and tr.temperature_proportion(1.0) == pytest.approx(0.03)


def test_temperature_schedule_against_the_reference_module(pkg):
    # tests/golden/r01_schedule_golden.json: return values of the reference's temperature_schedule.py, imported in the
    # build container (tests/golden/make_schedule_golden.py)
    import json
    G = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "r01_schedule_golden.json")))
    t = pkg.trainer
    for c in G["proportion"]:
        assert t.temperature_edit_string(c["data_fraction"]) == c["edit"]
        assert "proportion=%s'" % t.temperature_proportion(c["data_fraction"]) in c["edit"]
    for c in G["adapt"]:
        assert t.temperature_adapt_edit_string(c["init"], c["final"], c["data_fraction"]) == c["edit"]
    assert G["adapt_none"] is None and t.temperature_adapt_edit_string(None, 0.5, 0.3) is None


def test_outer_loop_plan(pkg):
    """train.py:405-531 bookkeeping (host only): iteration count, job ramp, learning rates, archives, combination set."""
    o = pkg.outer_loop
    to_process, iters = o.num_iterations(num_epochs=4, num_archives=10, frame_subsampling_factor=3, num_jobs_initial=2, num_jobs_final=6)
    assert (to_process, iters) == (120, 30)  # 4 * 10 * 3 archives at an average of 4 jobs
    plan = o.iteration_plan(4, 10, 3, 2, 6, 2.5e-4, 2.5e-5, temperature_schedule=True, dropout_schedule='0,0@0.20,0.5@0.50,0')
    dp = [p["dropout_proportion"] for p in plan]
    assert dp[0] == 0.0 and max(dp) > 0.45 and dp[-1] < 0.1 and all(v == 0.0 for p, v in zip(plan, dp) if p["data_fraction"] <= 0.2)
    t = pkg.trainer  # the option's own examples (common.py:883-905)
    assert t.dropout_proportion('0,0.2,0', 0.5) == pytest.approx(0.2) and t.dropout_proportion('0,0.2,0', 0.25) == pytest.approx(0.1)
    assert t.dropout_proportion('0,0.2@0.25,0', 0.25) == pytest.approx(0.2) and t.dropout_proportion('0,0.2@0.25,0', 0.625) == pytest.approx(0.1)
    assert t.dropout_proportion('0,0@0.20,0.5@0.50,0', 0.35) == pytest.approx(0.25) and t.dropout_proportion(None, 0.3) == 0.0
    # the upstream parser the reference keeps (temperature_schedule.py:122-182): an unspecified middle x is 0.5, not "evenly spread"
    assert t.parse_dropout_schedule('0,0.1,0.3,0') == [(0.0, 0.0), (0.5, 0.1), (0.5, 0.3), (1.0, 0.0)]
    assert t.dropout_proportion('0,0.1,0.3,0', 0.25) == pytest.approx(0.05) and t.dropout_proportion('0,0.1,0.3,0', 0.5) == pytest.approx(0.3)
    assert t.dropout_proportion('0,0.1,0.3,0', 0.75) == pytest.approx(0.15) and t.dropout_proportion('0.2,0.5', 1.0) == pytest.approx(0.5)
    for bad in ('0.3', '0,0.2@0.6,0.1@0.4,0', '0,0.2@1.5,0', '0,1.2,0'):
        with pytest.raises(ValueError):
            t.parse_dropout_schedule(bad)
    assert len(plan) == 30 and plan[0]["num_jobs"] == 2 and plan[-1]["num_jobs"] == 6
    assert [p["num_jobs"] for p in plan] == sorted(p["num_jobs"] for p in plan)
    assert abs(sum(p["num_jobs"] for p in plan) - to_process) <= 6
    assert plan[0]["learning_rate"] == pytest.approx(2 * 2.5e-4) and plan[-1]["learning_rate"] == pytest.approx(6 * 2.5e-5)
    eff = [p["learning_rate"] / p["num_jobs"] for p in plan]
    assert all(a > b for a, b in zip(eff, eff[1:]))  # the effective rate decays monotonically
    assert plan[0]["temperature_proportion"] == 1.0 and 0.03 < plan[-1]["temperature_proportion"] < 0.1
    assert plan[0]["archives"] == [0, 1] and plan[1]["archives"] == [2, 3] and all(0 <= a < 30 for p in plan for a in p["archives"])
    seen = {o.archive_and_frame_shift(k, 10, 3) for k in range(30)}
    assert seen == {(a, sh) for a in range(1, 11) for sh in range(3)}  # one epoch of expanded archives = every archive at every shift
    assert o.archive_and_frame_shift(0, 10) == (1, 1) and o.archive_and_frame_shift(10, 10) == (1, 2)
    with pytest.raises(ValueError):
        o.num_iterations(1, 2, 3, 1, 7)
    with pytest.raises(ValueError):
        o.shrinkage_value(1e-3, proportional_shrink=600.0)
    assert o.shrinkage_value(1e-3, 150.0) == pytest.approx(0.85)
    # common.py:562-603 worked by hand: half an epoch at the final rate is 3 iterations (<= max 20) -> the last
    # min(20, iters // 2) models; 51 iterations (> 20) -> every 2nd of the last 51, plus the last
    assert o.model_combine_iters(30, 4, 30, 20, 6) == set(range(16, 31))
    assert o.model_combine_iters(400, 4, 600, 20, 6) == set(range(350, 401, 2))
    assert o.model_combine_iters(10, 1, 4, 20, 1) == {6, 7, 8, 9, 10}


def test_lda_matrix_files(pkg, tmp_path):
    import struct
    import numpy as np
    t = pkg.trainer
    m = np.random.default_rng(0).standard_normal((5, 6)).astype(np.float32)
    (tmp_path / "b.mat").write_bytes(b"\0BFM " + b"\x04" + struct.pack("<i", 5) + b"\x04" + struct.pack("<i", 6) + m.tobytes())
    (tmp_path / "d.mat").write_bytes(b"\0BDM " + b"\x04" + struct.pack("<i", 5) + b"\x04" + struct.pack("<i", 6) + m.astype(np.float64).tobytes())
    (tmp_path / "t.mat").write_text(" [\n  " + "\n  ".join(" ".join("%.9g" % v for v in r) for r in m) + " ]\n")
    for name in ("b.mat", "d.mat", "t.mat"):
        assert np.array_equal(t.read_kaldi_matrix(tmp_path / name), m), name
    comps = [dict(name="lda", begin=8, rows=5, cols=5, has_bias=1)]
    p = t.set_lda(np.zeros(64, np.float32), comps, m)
    assert np.array_equal(p[8:33].reshape(5, 5), m[:, :5]) and np.array_equal(p[33:38], m[:, 5]) and not p[38:].any() and not p[:8].any()
    with pytest.raises(ValueError):
        t.set_lda(np.zeros(64, np.float32), comps, m[:, :5])
    (tmp_path / "x.mat").write_bytes(b"\0BFM " + b"\x04" + struct.pack("<i", 5) + b"\x04" + struct.pack("<i", 6) + m.tobytes()[:40])
    with pytest.raises(ValueError):
        t.read_kaldi_matrix(tmp_path / "x.mat")
