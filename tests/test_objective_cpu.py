"""No GPU: the objective-only entries (tdnnf_chain_objf, tdnnf_net_objective) are declared, exported and refuse bad arguments before any
device call.  (Mismatched dimensions need a graph or a net, which live on the device: tests/test_gpu_chain_objf.py and
tests/test_gpu_net_objective.py check those.)"""
import ctypes as C

NEW = ["tdnnf_chain_objf_workspace_bytes", "tdnnf_chain_objf", "tdnnf_net_objective"]


def test_header_declares_and_library_exports_the_objective_entries(pkg):
    declared = pkg.hipabi.declared_symbols()
    lib = pkg.hipabi.load()
    for name in NEW:
        assert name in declared, name
        assert getattr(lib, name) is not None
    header = open(pkg.hipabi.HEADER).read()
    assert "#define TDNNF_OBJECTIVE_STORE_BATCHNORM_STATS 1" in header and pkg.hipabi.OBJECTIVE_STORE_BATCHNORM_STATS == 1
    adapter = open(pkg.hipabi.HEADER.replace("tdnnf_hip.h", "tdnnf_nnet3_adapter.h")).read()
    assert "inline void ChainObjf(" in adapter and "tdnnf_chain_objf(" in adapter
    assert lib.tdnnf_chain_objf_workspace_bytes.restype is C.c_size_t and lib.tdnnf_chain_objf.restype is C.c_int
    assert lib.tdnnf_abi_version() == 1
    assert hasattr(pkg.trainer.ChainNet, "objective")


def test_objective_entries_validate_arguments_without_gpu(pkg):
    lib = pkg.hipabi.load()
    M = pkg.hipabi.Mat
    res = (C.c_double * 8)()
    ok = M(None, 0, 0, 0)
    bad = M(None, 4, 8, 8)  # rows * cols != 0 with a null pointer
    assert lib.tdnnf_chain_objf_workspace_bytes(None, 4, 10) == 0
    # null graph / supervision / matrix / results
    assert lib.tdnnf_chain_objf(None, None, C.byref(ok), None, 0.1, 0.0, res, None, 0, None) == 1
    assert b"chain_objf" in lib.tdnnf_last_error()
    assert lib.tdnnf_chain_objf(None, None, None, None, 0.1, 0.0, None, None, 0, None) == 1
    assert lib.tdnnf_net_objective(None, C.byref(ok), C.byref(ok), None, None, res, 0, None) == 1
    assert b"net_objective" in lib.tdnnf_last_error()
    assert lib.tdnnf_net_objective(None, C.byref(bad), C.byref(bad), None, None, None, 0, None) == 1
