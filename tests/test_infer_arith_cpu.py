"""No GPU: the boundary of the inference arithmetic (tdnnf_infer_create_arith / tdnnf_infer_gemm_counts, infer.py's `arithmetic`)."""
import ctypes as C
import subprocess

import pytest

NEW = ("tdnnf_infer_create_arith", "tdnnf_infer_gemm_counts")


def test_header_declares_and_library_exports_the_entries(pkg):
    lib = pkg.hipabi.load()
    names = pkg.hipabi.declared_symbols()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.hipabi.LIB_PATH], capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if l.strip()}
    for name in NEW:
        assert name in names and name in exported, name
    create = lib.tdnnf_infer_create_arith
    assert create.restype is C.c_int and len(create.argtypes) == 6 and create.argtypes[1:5] == [C.c_int] * 4
    counts = lib.tdnnf_infer_gemm_counts
    assert counts.restype is C.c_int and counts.argtypes == [C.c_void_p] * 3


def test_bad_arguments_fail_before_any_device_call(pkg):
    lib = pkg.hipabi.load()
    h = C.c_void_p()
    # null model / null result
    assert lib.tdnnf_infer_create_arith(None, 30, 4, 0, 3, C.byref(h)) == 1
    assert b"infer_create_arith" in lib.tdnnf_last_error() and b"null" in lib.tdnnf_last_error()
    assert lib.tdnnf_infer_create_arith(None, 30, 4, 0, 0, None) == 1
    # the arithmetic: 0 and 3 only, and the message names the argument
    for precision in (1, 2, -1, 4, 6):
        assert lib.tdnnf_infer_create_arith(None, 30, 4, 0, precision, C.byref(h)) == 1
        msg = lib.tdnnf_last_error().decode()
        assert "gemm_precision" in msg and str(precision) in msg, msg
    for max_chunks, which in ((0, 0), (-3, 1), (4, 2), (4, -1)):
        assert lib.tdnnf_infer_create_arith(None, 30, max_chunks, which, 3, C.byref(h)) == 1
        msg = lib.tdnnf_last_error().decode()
        assert "max_chunks" in msg and "which_output" in msg, msg
    assert not h.value
    assert lib.tdnnf_infer_gemm_counts(None, None, None) == 1
    assert b"infer_gemm_counts" in lib.tdnnf_last_error()


def test_arithmetic_names(pkg):
    infer = pkg.infer
    assert infer.arithmetic_precision("f32") == 0 and infer.arithmetic_precision("f16x3") == 3
    for bad in ("bf16x6", "f16", "F32", "", None, 3):
        with pytest.raises(ValueError, match="arithmetic"):
            infer.arithmetic_precision(bad)

    class Untouchable:  # stands for the net: the name is checked before the net or the library is looked at
        def __getattr__(self, name):
            raise AssertionError("touched " + name)

    with pytest.raises(ValueError, match="arithmetic"):
        infer.AcousticModel(Untouchable(), arithmetic="bf16x6")
    with pytest.raises(ValueError, match="arithmetic"):
        infer.AcousticModel.from_model_file("/nonexistent/final.mdl", arithmetic="f16")
