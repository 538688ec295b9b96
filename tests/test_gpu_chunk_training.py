"""-m gpu: a training step straight from aligned utterances (egs.minibatches_from_utterances: the features gathered by hipabi.ChunkInput, the
supervision compiled by assign_alignment_chunks; include/tdnnf_hip.h "CHUNK INPUTS", "ALIGNMENT CHUNKS") gives the BITS of the host route
-- the numpy statement's features uploaded, the host lattice of the same chunks assigned: `results` and the whole gradient buffer.  And the
epochs: the same seed the same chunk order, another seed another, every chunk exactly once."""
import numpy as np
import pytest
import torch

from tests import alignment_supervision_ref as ali
from tests import chunk_input_ref as ref
from tests.gpu_util import dev, host
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
    yield net, us, units, utts, als
    net.close()


@pytest.mark.parametrize("shift", [0, -1])
def test_one_step_has_the_bits_of_the_host_route(pkg, setup, shift):
    net, us, units, utts, als = setup
    den = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(30, net.cfg.num_pdfs, mean_out_degree=4.0, seed=5))
    out_frames = [(len(f) + 2) // 3 for f, _ in utts]
    batches = pkg.egs.minibatches_from_utterances(utts, als, net, units, 2, frame_shift=shift, seed=4, weight=0.5)
    f_dev, iv_dev, sup = next(batches)
    chunks = sup.chunks
    assert len(chunks) == 4 and sup.reserves == 1 and (sup.B, sup.T) == (4, 8)
    net.grads.zero_()
    r1 = host(net.forward_backward(f_dev, iv_dev, den, sup, step=3)).copy()
    g1 = host(net.grads).copy()
    # the host route on the same chunks
    utt, begins = [u for u, _ in chunks], [o for _, o in chunks]
    want_f, want_iv = ref.gather(net.first_t, net.num_t_in, 3, 8, utt, begins, utts, 10, shift)
    assert np.array_equal(host(f_dev), want_f) and np.array_equal(host(iv_dev), want_iv)
    lattice = pkg.synth.supervision_lattice_from_alignment_chunks(us, [als[u] for u in utt], [out_frames[u] for u in utt], begins, 8, 2, weight=0.5)
    assigned = pkg.hipabi.Supervision.reserve(4, 8, len(lattice["state_time"]), len(lattice["arc_src"]))
    assigned.assign(lattice)
    net.grads.zero_()
    r2 = host(net.forward_backward(dev(want_f), dev(want_iv), den, assigned, step=3))
    assert r1[5] == 1.0 and np.isfinite(r1[:7]).all() and np.abs(g1).sum() > 0
    assert np.array_equal(r1.view(np.int64), r2.view(np.int64)) and np.array_equal(g1.view(np.int32), host(net.grads).view(np.int32))
    batches.close()


def test_epochs(pkg, setup):
    net, us, units, utts, als = setup
    E = pkg.egs
    out_frames = [(len(f) + 2) // 3 for f, _ in utts]
    every = E.utterance_chunks(out_frames, 8)
    assert len(every) == 8  # two minibatches of 4: discard_partial=False divides evenly

    def epoch(seed):
        order = []
        for f, iv, sup in E.minibatches_from_utterances(utts, als, net, units, 2, seed=seed, discard_partial=False):
            assert f.shape == (net.num_t_in * 4, 40) and iv.shape == (4, 100) and sup.capacity()["allocations"] == 0
            order.append(list(sup.chunks))
        return order

    a, b, c = epoch(0), epoch(0), epoch(1)
    assert a == b and a != c and [len(m) for m in a] == [4, 4]
    assert sorted(ch for m in a for ch in m) == sorted(every) == sorted(ch for m in c for ch in m)
    assert a == E.chunk_minibatches(every, 4, 0)
    # utterances shorter than a chunk contribute none; alignments and utterances go together
    short = utts + [(utts[0][0][:20], utts[0][1][:2])]
    got = [sup.chunks for _, _, sup in E.minibatches_from_utterances(short, als + [ali.random_alignment(np.random.default_rng(9), 7)], net, units, 2, seed=0)]
    assert got == a
    with pytest.raises(ValueError, match="5 utterances and 4 alignments"):
        next(E.minibatches_from_utterances(short, als, net, units, 2))
