"""-m gpu: streaming inference with per-stream state carried between calls (csrc/online.hip on the schedule of csrc/infer_forward.hip, include/tdnnf_hip.h "inference (forward
only, streaming)").

The expectation is always the CPU oracle over whole utterances (tests/test_gpu_infer.py `expected`): streaming a constant i-vector
must give the whole-utterance output, whatever the step width, the slot, the order of the active list or what the slot held before."""
import ctypes as C

import numpy as np
import pytest

from tests.gpu_util import dev, host, rel_l2
from tests.oracle_net import OracleNet
from tests.test_gpu_infer import CHILD, FSF, SMALL, expected, make_model, utterances

pytestmark = pytest.mark.gpu


def whole(utts):
    """the utterances with one i-vector each (their first row)"""
    return [(f, iv[:1]) for f, iv in utts]


def stream(om, utts, pieces=None):
    """Streams the utterances through om's slots -- more utterances than slots: a slot is released when its utterance is finished and
    the next one opened in it.  pieces: frames pushed per step (default: the whole utterance at once).  Returns one array each."""
    pending, active, fed = list(range(len(utts))), {}, {}
    outs = [[] for _ in utts]
    idle = 0
    while pending or active:
        while pending and om.free:
            u = pending.pop(0)
            active[om.open()] = u
            fed[u] = 0
        for slot, u in active.items():
            f, iv = utts[u]
            if fed[u] < len(f):
                n = len(f) - fed[u] if pieces is None else min(pieces, len(f) - fed[u])
                om.push(slot, f[fed[u]:fed[u] + n], iv[0], final=fed[u] + n == len(f))
                fed[u] += n
        res = om.step()
        idle = 0 if res else idle + 1
        assert idle < 3, "no stream made progress"
        for slot, rows in res.items():
            outs[active[slot]].append(host(rows).copy())
        for slot in [s for s in active if om.finished(s)]:
            om.release(slot)
            del active[slot]
    return [np.concatenate(o) for o in outs]


def alone(pkg, net, F, utt, which="output"):
    om = pkg.infer.OnlineAcousticModel(net, frames_per_step=F, num_slots=1, output=which)
    out = stream(om, [utt])[0]
    om.close()
    return out


@pytest.mark.parametrize("F", [3, 30])
@pytest.mark.parametrize("which", ["output", "output-xent"])
@pytest.mark.parametrize("name,kw", [("7q-small", SMALL), ("child", CHILD)])
def test_parity_with_the_oracle(pkg, name, kw, which, F):
    cfg, net = make_model(pkg, kw)
    stats = net.get_stats()
    rng = np.random.default_rng(11)
    utts = whole(utterances(rng, [1, 2, F - 1, F, F + 1, int(3.5 * F), 17, 44], constant_iv=True))
    om = pkg.infer.OnlineAcousticModel(net, frames_per_step=F, num_slots=3, output=which)
    got = stream(om, utts)
    ref = expected(pkg, kw, net, stats, utts, 30, 0, which=which)
    e = rel_l2(np.concatenate(got), ref)
    print("PARITY test_gpu_online %s %s F %d rel_l2 %.3e" % (name, which, F, e))
    assert np.concatenate(got).shape == ref.shape and e < 1e-4, e
    sizes = np.cumsum([-(-len(f) // FSF) for f, _ in utts])[:-1]
    chunked = [host(o) for o in pkg.infer.AcousticModel(net, frames_per_chunk=30, max_chunks=8, output=which).compute(utts, ivector_period=0)]
    for u, (g, r, a) in enumerate(zip(got, np.split(ref, sizes), chunked)):
        eu, ea = rel_l2(g, r), rel_l2(g, a)
        print("PARITY test_gpu_online %s %s F %d utterance %d (%d frames) rel_l2 %.3e, against AcousticModel.compute %.3e" % (name, which, F, u, len(utts[u][0]), eu, ea))
        assert g.shape == r.shape and eu < 1e-4, (u, eu)
        assert ea < 1e-5, (u, ea)  # the project's bar for "chunk width does not change the output"


def test_staggered_and_partial_activity(pkg):
    kw = CHILD
    cfg, net = make_model(pkg, kw, seed=7)
    F = 6
    rng = np.random.default_rng(12)
    utts = whole(utterances(rng, [50, 23, 71], constant_iv=True))
    want = [alone(pkg, net, F, u) for u in utts]
    om = pkg.infer.OnlineAcousticModel(net, frames_per_step=F, num_slots=3)
    open_at = {0: 0, 1: 2, 2: 5}  # utterance -> step at which its slot is opened
    slot_of, fed, outs = {}, {}, [[] for _ in utts]
    subsets = 0
    for k in range(200):
        for u, at in open_at.items():
            if at == k:
                slot_of[u] = om.open()
                fed[u] = 0
        live = [u for u in slot_of if not om.finished(slot_of[u])]
        if not live and len(slot_of) == len(utts):
            break
        for u in live:  # frames arrive 7 at a time: windows fill at another rhythm than the steps
            f, iv = utts[u]
            if fed[u] < len(f):
                n = min(7, len(f) - fed[u])
                om.push(slot_of[u], f[fed[u]:fed[u] + n], iv[0], final=fed[u] + n == len(f))
                fed[u] += n
        order = [slot_of[u] for u in live]
        order = order[k % len(order):] + order[:k % len(order)] if order else order  # permuted
        if k % 3 == 1 and len(order) > 1:  # a strict subset: the slot left out keeps its state and clock
            order = order[1:][::-1]
            subsets += 1
        for slot, rows in om.step(order).items():
            u = [u for u in slot_of if slot_of[u] == slot][0]
            outs[u].append(host(rows).copy())
    assert subsets >= 3
    for u in range(len(utts)):
        e = rel_l2(np.concatenate(outs[u]), want[u])
        assert np.concatenate(outs[u]).shape == want[u].shape and e < 1e-5, (u, e)


def test_reset_isolates_utterances(pkg):
    kw = CHILD
    cfg, net = make_model(pkg, kw, seed=8)
    F = 30
    rng = np.random.default_rng(13)
    (loud, iv0), normal = whole(utterances(rng, [70, 40], constant_iv=True))
    om = pkg.infer.OnlineAcousticModel(net, frames_per_step=F, num_slots=1)
    stream(om, [(1.0e3 * loud, iv0)])
    got = stream(om, [normal])[0]  # open() takes the same slot again
    want = alone(pkg, net, F, normal)
    e = rel_l2(got, want)
    assert got.shape == want.shape and e < 1e-5, e


def test_changing_ivector(pkg):
    # SMALL: right context 9 = its latency, so "first computed in a step" and "receptive field" draw the same line
    kw = SMALL
    cfg, net = make_model(pkg, kw, seed=9)
    stats = net.get_stats()
    F, T, switch = 30, 240, 120
    rng = np.random.default_rng(14)
    f = rng.standard_normal((T, 40)).astype(np.float32)
    iv1, iv2 = rng.standard_normal((2, 1, 100)).astype(np.float32)
    om = pkg.infer.OnlineAcousticModel(net, frames_per_step=F, num_slots=2)
    left, right, latency = om.context()
    assert latency == right
    slot = om.open()
    out, steps = [], 0
    om.push(slot, f[:switch], iv1[0])
    while True:
        res = om.step()
        if not res:
            break
        out.append(host(res[slot]).copy())
        steps += 1
    om.push(slot, f[switch:], iv2[0], final=True)
    while not om.finished(slot):
        out.append(host(om.step()[slot]).copy())
        steps += 1
    assert steps >= 8
    got = np.concatenate(out)
    ref1 = expected(pkg, kw, net, stats, [(f, iv1)], F, 0)
    ref2 = expected(pkg, kw, net, stats, [(f, iv2)], F, 0)
    t = np.arange(got.shape[0]) * FSF
    before, after = t + right < switch, t - left >= switch
    e1, e2 = rel_l2(got[before], ref1[before]), rel_l2(got[after], ref2[after])
    between = int((~before & ~after).sum())
    print("PARITY test_gpu_online changing i-vector: before %.3e (%d rows), after %.3e (%d rows), %d rows in between" % (e1, before.sum(), e2, after.sum(), between))
    assert got.shape == ref1.shape and e1 < 1e-4 and e2 < 1e-4, (e1, e2)
    assert between <= -(-(left + right + 1) // FSF) + 1 and before.sum() + after.sum() >= got.shape[0] / 2
    assert rel_l2(ref1[after], ref2[after]) > 1e-3  # (the i-vector matters)


@pytest.mark.parametrize("name,kw", [("7q-small", SMALL), ("child", CHILD)])
def test_state_is_carried_not_recomputed(pkg, name, kw):
    cfg, net = make_model(pkg, kw, seed=5)
    F, B = 30, 3
    om = pkg.infer.OnlineAcousticModel(net, frames_per_step=F, num_slots=B)
    rng = np.random.default_rng(2)
    utts = whole(utterances(rng, [200] * B, constant_iv=True))
    for f, iv in utts:
        om.push(om.open(), f, iv[0], final=True)
    for _ in range(3):  # warm-up (left context <= F), then two full windows: the last one is steady state
        assert len(om.step()) == B
    assert all(om.slot_state(s) == (2 * F, -1) for s in range(B))
    gemm_rows, carried_rows, fused, fallback = om.counts()
    ref = OracleNet(pkg, pkg.trainer.make_config(**dict(kw, frames_per_chunk=F, num_sequences=B, cv_update=1)), net.components)
    # GEMM stages: lda, tdnn1, every layer's .linear and .affine, prefinal-l and the head's affine / linear / output
    step_rows = 2 * B * F + sum(B * F // L["lin"][1] + B * F // L["out"][1] for L in ref.layers) + 4 * B * F // FSF
    chunk_rows = 2 * B * ref.g_lda[2] + sum(B * L["lin"][2] + B * L["out"][2] for L in ref.layers) + 4 * B * F // FSF
    print("ROWS test_gpu_online %s: %d GEMM rows a step, %d a chunk of the same width (ratio %.2f), %d carried" % (name, gemm_rows, chunk_rows, chunk_rows / gemm_rows, carried_rows))
    assert gemm_rows == step_rows and step_rows < chunk_rows
    assert carried_rows > 0
    assert fused + fallback == cfg.num_layers + 3


@pytest.mark.parametrize("name,extra", [("offset-supernet", dict(darts_num_offsets=3, darts_flags=1 | 16, darts_temp_proportion=0.8)),
                                        ("bottleneck-supernet", dict(bn_choice_dims=[4, 4, 8], bn_mode=0)),
                                        ("f16x3", dict(gemm_precision=3))])
def test_rejected_models(pkg, name, extra):
    lib = pkg.hipabi.load()
    cfg = pkg.trainer.make_config(**dict(SMALL, **extra))
    net = pkg.trainer.ChainNet(cfg)
    net.set_params(net.init_params_numpy(seed=1, output_stddev=0.3))
    h = C.c_void_p()
    assert lib.tdnnf_online_create(net.h, 30, 4, 0, C.byref(h)) == 1
    msg = lib.tdnnf_last_error().decode()
    assert ("supernet" in msg) if name != "f16x3" else ("gemm_precision" in msg), msg


def test_rejected_steps_change_nothing(pkg):
    lib = pkg.hipabi.load()
    cfg, net = make_model(pkg, SMALL)
    h = C.c_void_p()
    assert lib.tdnnf_online_create(net.h, 31, 4, 0, C.byref(h)) == 1  # F not a multiple of fsf
    assert b"frame_subsampling" in lib.tdnnf_last_error()
    F = 30
    rng = np.random.default_rng(16)
    utt = whole(utterances(rng, [100], constant_iv=True))[0]
    want = alone(pkg, net, F, utt)
    om = pkg.infer.OnlineAcousticModel(net, frames_per_step=F, num_slots=2)
    slot = om.open()
    om.push(slot, utt[0], utt[1][0], final=True)
    other = om.open()
    out = []
    for k in range(100):
        if om.finished(slot):
            break
        if k == 2:  # slot is at clock F: a full window that is not final comes next
            state = om.slot_state(slot)
            assert state == (F, -1)
            fd, ivd = dev(utt[0]), dev(np.repeat(utt[1], 2, axis=0))
            bad = [("exactly %d rows" % F, [slot], [F - 1], [0], fd[F:2 * F - 1], ivd[:1]),     # a non-final window with fewer than F rows
                   ("listed twice", [slot, slot], [F, F], [0, 0], dev(np.concatenate([utt[0][F:2 * F]] * 2)), ivd),
                   ("out of range", [slot, 2], [F, 1], [0, 0], fd[F:2 * F + 1], ivd),
                   ("out of range", [-1], [1], [0], fd[:1], ivd[:1]),
                   ("warming up", [other], [F], [0], fd[:F], ivd[:1]),                   # a warm-up window passes frame 0 alone
                   ("feats must be", [slot], [F], [0], fd[F:2 * F - 1], ivd[:1])]
            for what, slots, rows, finals, feats, ivs in bad:
                with pytest.raises(pkg.hipabi.HipAbiError, match="tdnnf error 1.*" + what):
                    om.step_raw(slots, rows, finals, feats, ivs)
                assert om.slot_state(slot) == state and om.slot_state(other) == (-F, -1)
        out.append(host(om.step()[slot]).copy())
    e = rel_l2(np.concatenate(out), want)
    assert np.concatenate(out).shape == want.shape and e < 1e-5, e


def test_model_updates_are_seen(pkg, tmp_path):
    kw = SMALL
    cfg, net = make_model(pkg, kw, seed=21, cv=0)
    feats, iv = pkg.trainer.synthetic_egs(net, seed=4)
    den = pkg.hipabi.DenGraph(pkg.synth.make_den_graph(8, cfg.num_pdfs, mean_out_degree=3.0, seed=5))
    sup = pkg.hipabi.Supervision(pkg.synth.make_supervision(cfg.num_sequences, cfg.frames_per_chunk // 3, cfg.num_pdfs, seed=6))
    fd, ivd = dev(feats), dev(iv)
    for step in range(3):
        net.grads.zero_()
        net.forward_backward(fd, ivd, den, sup, step=step)
        net.update(1e-3, step=step)
    rng = np.random.default_rng(14)
    utts = whole(utterances(rng, [40, 100, 7], constant_iv=True))
    path = tmp_path / "final.mdl"
    net.write_model(path)
    om = pkg.infer.OnlineAcousticModel(net, frames_per_step=30, num_slots=2)
    a = np.concatenate(stream(om, utts))
    b = np.concatenate(stream(pkg.infer.OnlineAcousticModel.from_model_file(path, frames_per_step=30, num_slots=2), utts))
    assert rel_l2(a, b) < 1e-6
    net.grads.zero_()
    net.forward_backward(fd, ivd, den, sup, step=3)
    net.update(1e-3, step=3)
    c = np.concatenate(stream(om, utts))  # the same object: the next utterances see the new parameters and statistics
    path2 = tmp_path / "final2.mdl"
    net.write_model(path2)
    d = np.concatenate(stream(pkg.infer.OnlineAcousticModel.from_model_file(path2, frames_per_step=30, num_slots=2), utts))
    assert rel_l2(c, a) > 1e-6 and rel_l2(c, d) < 1e-6
