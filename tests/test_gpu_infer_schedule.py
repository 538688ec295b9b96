"""-m gpu: the launches of the one forward-only schedule (csrc/infer_forward.hip) for its three readers -- the whole-utterance inference
in f32 (csrc/infer.hip) and f16x3 (csrc/infer_planes.hip) and a streaming step (csrc/online.hip).

The GEMM launch-form histogram and the counters of one call each are compared with what commit 7866cd3 (the last one in which every reader
wrote the schedule out by hand) gave for this same test body; what can be derived without a measurement is asserted beside it."""
import numpy as np
import pytest

from tests.test_gpu_infer import CHILD, SMALL, make_model, utterances

pytestmark = pytest.mark.gpu

# measured at commit 7866cd3 with this test body: (launch forms, counts(), gemm_counts()) of the two computes, (launch forms,
# tdnnf_online_counts) of the step
PARENT = {
    "7q-small": dict(f32=({"rows.64x128k16.f32.plain": 16, "rows.64x128k16.f32.post": 16, "rows.launches_vec4": 32}, (7, 1), (0, 32)),
                     f16x3=({}, (7, 1), (32, 0)),  # (the plane GEMM with the inference epilogue has no launch-form counter)
                     online=({"rows.64x128k16.f32.plain": 8, "rows.64x128k16.f32.post": 8, "rows.launches_vec4": 16}, (780, 36, 7, 1))),
    "child": dict(f32=({"rows.64x128k16.f32.plain": 14, "rows.64x128k16.f32.post": 14, "rows.launches_vec4": 28}, (6, 1), (0, 28)),
                  f16x3=({}, (6, 1), (28, 0)),
                  online=({"rows.64x128k16.f32.plain": 7, "rows.64x128k16.f32.post": 7, "rows.launches_vec4": 14}, (960, 69, 6, 1))),
}


def plain_and_post(forms):
    """launches of the f32 rows GEMM (rows.<tile>.f32.plain and .post: without and with the inference epilogue) and those with it"""
    post = sum(v for k, v in forms.items() if k.startswith("rows.") and k.endswith(".post"))
    return post + sum(v for k, v in forms.items() if k.startswith("rows.") and k.endswith(".plain")), post


@pytest.mark.parametrize("name,kw", [("7q-small", SMALL), ("child", CHILD)])
def test_launches_are_those_of_the_parent(pkg, name, kw):
    cfg, net = make_model(pkg, kw, seed=5)
    utts = utterances(np.random.default_rng(2), [90, 31])
    per_pass = 2 * cfg.num_layers + 6  # lda, tdnn1, every layer's .linear and .affine, prefinal-l, the head's affine / linear / output
    got = {}
    for arith in ("f32", "f16x3"):
        am = pkg.infer.AcousticModel(net, frames_per_chunk=30, max_chunks=4, arithmetic=arith)
        pkg.hipabi.launch_forms(reset=True)
        am.compute(utts)
        got[arith] = (pkg.hipabi.launch_forms(reset=True), tuple(am.counts()), tuple(am.gemm_counts()))
        nbatches = -(-len(am.plan([90, 31], [9, 4], 10)) // 4)
        am.close()
    F, B = 30, 3
    om = pkg.infer.OnlineAcousticModel(net, frames_per_step=F, num_slots=B)
    for f, iv in utterances(np.random.default_rng(2), [200] * B, constant_iv=True):
        om.push(om.open(), f, iv[0], final=True)
    for k in range(3):  # warm-up (left context <= F), then two full windows: the last one is steady state
        if k == 2:
            pkg.hipabi.launch_forms(reset=True)
        assert len(om.step()) == B
    got["online"] = (pkg.hipabi.launch_forms(reset=True), tuple(om.counts()))
    om.close()
    for key in ("f32", "f16x3", "online"):
        print("SCHEDULE %s %s %r" % (name, key, got[key]))
    # derived: every GEMM of an f32 pass is one launch of the rows GEMM, and every fused stage one with the inference epilogue
    assert nbatches >= 2
    forms, (fused, fallback), (planes, f32) = got["f32"]
    assert plain_and_post(forms)[0] == nbatches * per_pass == f32 and planes == 0
    assert plain_and_post(forms)[1] >= fused and fused + fallback == cfg.num_layers + 3
    forms, (gemm_rows, carried_rows, fused, fallback) = got["online"]
    assert plain_and_post(forms)[0] == per_pass and plain_and_post(forms)[1] >= fused and fused + fallback == cfg.num_layers + 3
    planes, f32 = got["f16x3"][2]
    assert planes + f32 == nbatches * per_pass
    for key in ("f32", "f16x3", "online"):
        assert got[key] == PARENT[name][key], key
