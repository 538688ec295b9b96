#!/usr/bin/env python3
"""Forward-only inference over whole utterances (tdnnf_infer_compute) of the 7q model at full width: 1536 hidden, 6034 pdfs,
200 synthetic utterances of 300-1500 frames, frames_per_chunk 51 (decode.sh's 50 rounded to frame_subsampling) and 150.
Prints one JSON line: input frames/s and ms per call, the GEMM rate against the 157.3 TFLOP/s exact-f32 MFMA peak (GEMM FLOPs
from the library's own launch accounting, tdnnf_profile_*, in a separate call), the chunk-context overhead (F + context) / F
and the fused / fallback counts.
--gemm f16x3 runs the same calls in f16x3 (AcousticModel(arithmetic="f16x3")) and adds the plane / f32 GEMM launch counts and, from the
profiled call's HIP events, the time of the GEMMs and of the splits into planes (split_share = splits / (GEMMs + splits)).
--online adds streaming inference (tdnnf_online_step) of the same model: steady-state steps of F in {30, 150} input frames for 1, 16
and 64 concurrent streams -- input frames/s and ms per step -- and the algorithmic row ratio: the GEMM rows of a chunk of width F
(from the chunk grids) over those of a step (tdnnf_online_counts).
usage (GPU box): python tools/infer_bench.py [--calls K] [--utts N] [--max-chunks M] [--gemm f32|f16x3] [--online [--steps K]]"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

PEAK_TFLOPS = 157.3


def model_stats(cfg):
    """BatchNorm statistics of mean 0.3, variance 1 (and ReLU statistics) in tdnnf_net_get_stats order."""
    Hd, S, out = cfg.hidden_dim, cfg.prefinal_small_dim, []
    bn = lambda D: out.append(np.concatenate([[64.0], np.full(D, 64 * 0.3), np.full(D, 64 * 1.09)]))
    relu = lambda D: out.append(np.concatenate([[64.0], np.full(D, 10.0), np.full(D, 32.0), [0.0], np.zeros(D)]))
    for _ in range(cfg.num_layers + 1):
        bn(Hd), relu(Hd)
    for _ in range(2):
        bn(Hd), relu(Hd), bn(S)
    return np.concatenate(out)


def chunk_gemm_rows(cfg, F):
    """GEMM output rows of one chunk of width F per sequence, from the chunk grids (net_layer_grids restated: a layer's .linear runs
    on the grid of step gcd(output step, left, right), padded to whole blocks where that is finer than the output grid)."""
    from math import gcd
    fsf = cfg.frame_subsampling
    step, n = fsf, F // fsf
    rows = 4 * n  # prefinal-l and the head's affine, linear, output
    for l in reversed(range(cfg.num_layers)):
        a = cfg.offset_left[l] if cfg.use_layer_offsets else cfg.time_stride[l]
        b = cfg.offset_right[l] if cfg.use_layer_offsets else cfg.time_stride[l]
        rows += n  # .affine
        if a or b:
            ls = gcd(gcd(step, a), b)
            if ls == step:
                n_lin = n + b // step
            else:
                rho = step // ls
                n_lin = -(-(((n - 1) * step + b) // ls + 1) // rho) * rho
            step, n = ls, n_lin + a // ls
        else:
            n_lin = n
        rows += n_lin  # .linear
    return rows + 2 * n  # lda, tdnn1


def online(pkg, net, steps):
    """Steady-state streaming steps: every slot warmed up, then `steps` full windows for all slots at once."""
    res = {}
    for F in (30, 150):
        for slots in (1, 16, 64):
            om = pkg.infer.OnlineAcousticModel(net, frames_per_step=F, num_slots=slots)
            rng = np.random.default_rng(2)
            feats = torch.from_numpy(rng.standard_normal((slots * F, 40)).astype(np.float32)).cuda()
            ivs = torch.from_numpy(rng.standard_normal((slots, 100)).astype(np.float32)).cuda()
            ids = list(range(slots))
            for sl in ids:
                om.open()
            while om.slot_state(0)[0] < 0:  # warm-up windows: frame 0 alone
                om.step_raw(ids, [1] * slots, [0] * slots, feats[:slots], ivs)
            for _ in range(3):
                om.step_raw(ids, [F] * slots, [0] * slots, feats, ivs)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                om.step_raw(ids, [F] * slots, [0] * slots, feats, ivs)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / steps
            gemm_rows, carried_rows, fused, fallback = om.counts()
            res[f"F{F}_slots{slots}"] = dict(frames_per_s=round(slots * F / (ms / 1e3)), ms_per_step=round(ms, 3), gemm_rows=gemm_rows,
                                             carried_rows=carried_rows, row_ratio=round(slots * chunk_gemm_rows(net.cfg, F) / gemm_rows, 3),
                                             fused_layers=fused, fallback_passes=fallback)
            om.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--utts", type=int, default=200)
    ap.add_argument("--max-chunks", type=int, default=256)
    ap.add_argument("--widths", default="51,150")
    ap.add_argument("--gemm", default="f32", choices=["f32", "f16x3"], help="arithmetic of the whole-utterance GEMMs")
    ap.add_argument("--online", action="store_true", help="also time streaming steps (F 30 / 150, 1 / 16 / 64 streams)")
    ap.add_argument("--steps", type=int, default=50, help="--online: timed steps per configuration")
    args = ap.parse_args()
    if args.online and args.gemm != "f32":
        ap.error("--gemm %s: streaming inference runs exact f32 only; --online takes --gemm f32" % args.gemm)
    pkg = ge.load_package()
    lib = pkg.hipabi.load()
    cfg = pkg.trainer.make_config(frames_per_chunk=150, num_sequences=1, cv_update=1)  # 7q graph, 1536 / 6034
    net = pkg.trainer.ChainNet(cfg)
    net.set_params(net.init_params_numpy(seed=0, output_stddev=0.05))
    net.set_stats(model_stats(cfg))
    rng = np.random.default_rng(1)
    lengths = rng.integers(300, 1501, size=args.utts)
    utts = [(rng.standard_normal((int(T), 40)).astype(np.float32), rng.standard_normal((-(-int(T) // 10), 100)).astype(np.float32)) for T in lengths]
    frames = int(lengths.sum())
    res = dict(metric="infer_7q_full_width", gemm=args.gemm, utterances=args.utts, input_frames=frames, max_chunks=args.max_chunks, peak_tflops=PEAK_TFLOPS)
    for F in [int(w) for w in args.widths.split(",")]:
        am = pkg.infer.AcousticModel(net, frames_per_chunk=F, max_chunks=args.max_chunks, arithmetic=args.gemm)
        probe = pkg.trainer.ChainNet(pkg.trainer.make_config(frames_per_chunk=F, num_sequences=1, cv_update=1), share=net)
        context = probe.num_t_in - F
        probe.close()
        am.compute(utts)  # warm-up (uploads, first launches)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.calls):
            am.compute(utts)
        e1.record()
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / args.calls
        pkg.hipabi.check(lib.tdnnf_profile_enable(1))
        am.compute(utts)
        torch.cuda.synchronize()
        flops, gemm_ms, split_ms = 0.0, 0.0, 0.0
        for k in (0, 1, 2, 3, 7):  # the GEMM classes; 7: the splits into planes
            n, t, fl = C.c_double(), C.c_double(), C.c_double()
            pkg.hipabi.check(lib.tdnnf_profile_read(k, C.byref(n), C.byref(t), C.byref(fl)))
            if k == 7:
                split_ms = t.value
            else:
                flops += fl.value
                gemm_ms += t.value
        pkg.hipabi.check(lib.tdnnf_profile_enable(0))
        fused, fallback = am.counts()
        res[f"F{F}"] = dict(frames_per_s=round(frames / (ms / 1e3)), ms_per_call=round(ms, 2), gemm_tflop=round(flops / 1e12, 3),
                           gemm_tflops_per_s=round(flops / (ms / 1e3) / 1e12, 1), of_peak=round(flops / (ms / 1e3) / 1e12 / PEAK_TFLOPS, 3),
                           context_overhead=round((F + context) / F, 3), fused_layers=fused, fallback_passes=fallback)
        if args.gemm != "f32":
            planes, f32 = am.gemm_counts()
            res[f"F{F}"].update(plane_gemms=planes, f32_gemms=f32, gemm_ms=round(gemm_ms, 2), split_ms=round(split_ms, 2),
                                split_share=round(split_ms / max(gemm_ms + split_ms, 1e-9), 3))
        am.close()
    if args.online:
        res["online"] = online(pkg, net, args.steps)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
