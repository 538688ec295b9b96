"""-m gpu: training and inference straight from a feature store (egs.minibatches_from_store, hipabi.FeatureStore.utterances; include/
tdnnf_hip.h "FEATURE STORES") give the BITS of the float route on the same values.  With the tiny net and the aligned utterances of
tests/test_gpu_chunk_training.py (tiny_net and aligned_utterances, which that file and this one import from tests/test_gpu_chunk_input.py,
where they are defined), their features replaced by compressed ones (codes and headers drawn directly, format 1 and format 2):
one epoch of minibatches_from_store is, minibatch for minibatch, minibatches_from_utterances on the store's expanded features; one
forward_backward step from it has the same `results` and the same gradient buffer; AcousticModel.compute on the store's views equals
compute on the features the numpy statement decodes on the host."""
import numpy as np
import pytest
import torch

from tests import alignment_supervision_ref as ali
from tests import feature_store_ref as ref
from tests.gpu_util import host
from tests.test_gpu_chunk_input import aligned_utterances, tiny_net

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(pkg):
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    net = tiny_net(pkg)
    net.set_params(net.init_params_numpy(seed=1, output_stddev=0.3))
    us = ali.unit_set(pkg.synth, 1)
    units = pkg.hipabi.UnitSet(us["entry_pdf"], us["loop_pdf"], us["loop_logprob"], us["leave_logprob"], us["P"], us["take_logprob"], us["skip_logprob"])
    utts, als = aligned_utterances()
    yield net, units, [iv for _, iv in utts], [len(f) for f, _ in utts], als
    net.close()


def stored(pkg, fmt, frames):
    """(store, the statement's decoded features): values of a few units, as features have"""
    items = ref.random_items(20 + fmt, fmt, 40, frames)
    for it in items:
        it["min"], it["range"] = np.float32(-2.5), np.float32(6.0)
    store = pkg.hipabi.FeatureStore(fmt, 40, len(frames), sum(frames))
    store.append(items[:3])
    store.append(items[3:])
    return store, [ref.decode(it) for it in items]


def same_bits(a, b):
    a, b = (np.ascontiguousarray(x if isinstance(x, np.ndarray) else host(x)) for x in (a, b))
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("fmt", [1, 2])
def test_an_epoch_is_the_epoch_of_the_expanded_features(pkg, setup, fmt):
    net, units, ivs, frames, als = setup
    store, decoded = stored(pkg, fmt, frames)
    expanded = store.utterances(range(len(frames)), ivs)
    for u, (f, _) in enumerate(expanded):
        assert same_bits(f, decoded[u]), u
    E = pkg.egs
    for shift in (0, 1):
        from_store = E.minibatches_from_store(store, ivs, als, net, units, 2, frame_shift=shift, seed=4, weight=0.5, discard_partial=False)
        from_floats = E.minibatches_from_utterances(expanded, als, net, units, 2, frame_shift=shift, seed=4, weight=0.5, discard_partial=False)
        count = 0
        for (f1, iv1, sup1), (f2, iv2, sup2) in zip(from_store, from_floats):
            assert f1.shape == (net.num_t_in * 4, 40) and same_bits(f1, f2) and same_bits(iv1, iv2), (shift, count)
            assert sup1.chunks == sup2.chunks and (sup1.B, sup1.T) == (sup2.B, sup2.T) == (4, 8) and sup1.capacity()["allocations"] == 0
            count += 1
        assert count == 2 and next(from_store, None) is None and next(from_floats, None) is None
    info = store.info()
    assert (info["gathers"], info["expands"], info["allocations"], info["last_form"]) == (4, 1, 0, 4)
    with pytest.raises(ValueError, match="4 utterances and 3 alignments"):
        next(E.minibatches_from_store(store, ivs, als[:3], net, units, 2))


@pytest.mark.parametrize("fmt", [1, 2])
def test_one_step_has_the_bits_of_the_float_route(pkg, setup, fmt):
    net, units, ivs, frames, als = setup
    store, _ = stored(pkg, fmt, frames)
    den = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(30, net.cfg.num_pdfs, mean_out_degree=4.0, seed=5))
    results, grads, chunks = [], [], []
    for batches in (pkg.egs.minibatches_from_store(store, ivs, als, net, units, 2, frame_shift=-1, seed=4, weight=0.5),
                    pkg.egs.minibatches_from_utterances(store.utterances(range(len(frames)), ivs), als, net, units, 2, frame_shift=-1, seed=4, weight=0.5)):
        f, iv, sup = next(batches)
        net.grads.zero_()
        results.append(host(net.forward_backward(f, iv, den, sup, step=3)).copy())
        grads.append(host(net.grads).copy())
        chunks.append(list(sup.chunks))
        batches.close()
    assert chunks[0] == chunks[1] and len(chunks[0]) == 4
    assert results[0][5] == 1.0 and np.isfinite(results[0][:7]).all() and np.abs(grads[0]).sum() > 0
    assert np.array_equal(results[0].view(np.int64), results[1].view(np.int64)) and np.array_equal(grads[0].view(np.int32), grads[1].view(np.int32))


@pytest.mark.parametrize("fmt", [1, 3])
def test_compute_from_a_store_is_compute_on_the_host_decoded_features(pkg, setup, fmt):
    net, units, ivs, frames, als = setup
    store, decoded = stored(pkg, fmt, frames)
    model = pkg.infer.AcousticModel(net, frames_per_chunk=24)
    order = [2, 0, 3]
    got = model.compute(store.utterances(order, [ivs[u] for u in order]))
    want = model.compute([(decoded[u], ivs[u]) for u in order])
    assert len(got) == 3 and store.info()["expands"] == 1
    for g, w, u in zip(got, want, order):
        assert g.shape == ((frames[u] + 2) // 3, net.cfg.num_pdfs) and same_bits(g, w), u
        assert np.isfinite(host(g)).all() and np.abs(host(g)).sum() > 0
