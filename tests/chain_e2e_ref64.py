"""Float64 reference of the whole chain objective with an END-TO-END numerator (include/tdnnf_hip.h, tdnnf_supervision_create_e2e): a
helper module like tests/chain_ref64.py, no library code; pinned by tests/test_chain_e2e_ref64.py, used by tests/test_gpu_chain_e2e.py.

Numerator: tests/posteriors_ref64.forward_backward per sequence, on the rows y[s::B] of the t-major nnet_output (row = t * B + s), with
acoustic_scale 1.  Denominator: tests/chain_ref64.den_forward_backward.  A minibatch with a sequence whose numerator log-prob is not finite
takes the objective's failure path: ok False, objf = -10 * weight * B * T, every derivative zero, xent objective zero."""
import types

import numpy as np

from tests import chain_ref64, posteriors_ref64


def num_forward_backward(graphs, y, B):
    """(log p_num per sequence [B], UNWEIGHTED posteriors [T * B, P of y]); a sequence without a path of T arcs: -inf and zero rows."""
    y = np.asarray(y, dtype=np.float32)
    T = y.shape[0] // B
    assert len(graphs) == B and y.shape[0] == T * B
    lp, post = np.zeros(B), np.zeros(y.shape, dtype=np.float64)
    for s, g in enumerate(graphs):
        assert int(g["P"]) <= y.shape[1]
        r = posteriors_ref64.forward_backward(g, y[s::B], 1.0)
        lp[s] = r["logprob"]
        post[s::B, :int(g["P"])] = r["post"]
    return lp, post


def objective(den, e2e, y, leaky, l2_regularize=0.0, xent_regularize=0.0, xent_output=None):
    """e2e: {B, T, P, weight, graphs} (synth.make_e2e_supervision).  Returns a namespace: num_lp[B], den_lp[B], objf, ok, l2_term, weight (= w B T),
    deriv = w (post_num - gamma_den) - w l2 y, xent_deriv = xent_regularize w post_num, xent_objf = sum w post_num xent_output, post_num."""
    B, T, w = int(e2e["B"]), int(e2e["T"]), float(e2e["weight"])
    y = np.asarray(y, dtype=np.float32)
    assert y.shape == (T * B, int(den["P"]))
    r = types.SimpleNamespace()
    r.num_lp, r.post_num = num_forward_backward(e2e["graphs"], y, B)
    r.den_lp, r.gamma_den = chain_ref64.den_forward_backward(den, y, B, leaky)
    r.weight = w * B * T
    r.num, r.den = w * float(r.num_lp.sum()), w * float(r.den_lp.sum())
    objf = r.num - r.den
    r.ok = bool(np.isfinite(objf))
    y64 = y.astype(np.float64)
    r.l2_term = -0.5 * w * l2_regularize * float((y64 * y64).sum())
    if r.ok:
        r.objf = objf
        r.deriv = w * (r.post_num - r.gamma_den) - w * l2_regularize * y64
        r.xent_deriv = xent_regularize * w * r.post_num
        r.xent_objf = float((w * r.post_num * np.asarray(xent_output, dtype=np.float64)).sum()) if xent_output is not None else 0.0
    else:
        r.objf = -10.0 * r.weight
        r.deriv, r.xent_deriv, r.xent_objf = np.zeros(y.shape), np.zeros(y.shape), 0.0
    return r
