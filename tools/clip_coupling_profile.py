"""Measurements behind profiles/clip_coupling.md: what per-clip cross-view pairing (ops.set_clip_coupling("clip"),
VideoPredictor(coupling="clip"), include/mumpy_hip_ext8.h) costs and what it buys.

    python tools/clip_coupling_profile.py rate [--frames 96] [--rounds 5] [--T 3]        (one process per T, see below)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/clip_coupling_profile.py kernels [--reps 20]
    python tools/clip_coupling_profile.py kernels-report <dir>

rate      frames/s of the graphed VideoPredictor on a synthetic 432 x 240 video (seeded frames and weights, as
          tools/video_predict_profile.py): batch 1 (the only route to batch-size-1 results without the option), batch 8 with
          coupling="clip", batch 8 with coupling="batch".  A sample is one whole video, host clock from the first host instruction to
          a device synchronise after the metric vector is complete; the three alternate in one process, order reversed every round,
          one warm-up round; median and [min .. max].  Before the timing: how far each variant's logits are from the batch-1 ones.
          Three graphed predictors hold most of torch's pool of 32 side streams (each capture owns its fork/join streams), so a
          process measures one T.
kernels   launches the five grouped entries (groups = B) and their frozen siblings at the B = 8 stage shapes, r = 1, 3 and 5, `reps`
          times each, in a fixed order that it writes to <out>/clip_kernels_manifest.json.  Meant to run under a kernel trace.
kernels-report  splits the trace's dispatches of the five kernels by that order and prints the median time per entry and shape."""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multilateral-temporal-view-pyramid-transformer-for-video-inpainting-detection_amd"),
          os.path.join(ROOT, "tests", "golden")):
    sys.path.insert(0, p)
HS, WS, SIDE = 240, 432, 224
OUT = os.environ.get("MUMPY_PROFILE_OUT", os.path.join(ROOT, "profile_out"))
STAGES = [(56, 96), (28, 192), (14, 384), (7, 768)]
KERNELS = ("deform_sample_lds_kernel", "deform_sample_kv_kernel", "win_attn_cross_kernel", "win_attn_cross_mm16_kernel")


def rate(args):
    import torch
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from mumpy_hip.video import VideoPredictor
    from weight_fill import fill_module_
    dev = torch.device("cuda:0")
    g = np.random.default_rng(432)
    n = args.frames
    frames_t = torch.from_numpy(g.integers(0, 256, (n, HS, WS, 3), dtype=np.uint8))
    gt_t = torch.from_numpy((g.integers(0, 3, (n, SIDE, SIDE)) > 1).astype(np.uint8) * 255)
    report = dict(device=torch.cuda.get_device_name(0), frames=n, source=[HS, WS], rounds=args.rounds, T={})
    for T in (args.T,):
        enc = fill_module_(Encoder(num_frames=T).eval()).to(dev)
        dec = fill_module_(Decoder(input_token_temporal_dims=[1, 1, T]).eval()).to(dev)
        vps = {"batch1": VideoPredictor(enc, dec, T=T, src_hw=(HS, WS), batch=1, max_frames=n),
               "batch8_clip": VideoPredictor(enc, dec, T=T, src_hw=(HS, WS), batch=8, max_frames=n, coupling="clip"),
               "batch8_batch": VideoPredictor(enc, dec, T=T, src_hw=(HS, WS), batch=8, max_frames=n)}

        def run(vp, keep=None):
            vp.reset_metrics()
            cb = None if keep is None else (lambda b, logits, mask: keep.append(logits.clone()))
            masks = vp.predict(frames_t, gt_t, on_batch=cb)
            return masks, vp.metric_vector()
        logits, masks = {}, {}
        for name, vp in vps.items():                                 # warm-up of every shape, and what the variants compute
            keep = []
            masks[name] = run(vp, keep)[0].clone()
            torch.cuda.synchronize()
            logits[name] = torch.cat(keep)[:n].double()
        ref = logits["batch1"]
        diff = {name: dict(logits_rel=float((logits[name] - ref).abs().max() / ref.abs().max()),
                           logits_rms=float((logits[name] - ref).pow(2).mean().sqrt() / ref.pow(2).mean().sqrt()),
                           mask_bits_differ=float((masks[name] != masks["batch1"]).double().mean()))
                for name in ("batch8_clip", "batch8_batch")}
        times, names = {v: [] for v in vps}, list(vps)
        for r in range(1 + args.rounds):
            for name in (names if r % 2 == 0 else names[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(vps[name])
                torch.cuda.synchronize()
                if r >= 1:
                    times[name].append(time.perf_counter() - t0)
        row = {name: dict(fps_median=round(n / statistics.median(v), 1), fps_min=round(n / max(v), 1), fps_max=round(n / min(v), 1),
                          ms_per_video_median=round(1e3 * statistics.median(v), 1)) for name, v in times.items()}
        row["ratio_clip8_over_batch1"] = round(statistics.median(times["batch1"]) / statistics.median(times["batch8_clip"]), 2)
        row["ratio_clip8_over_batch8"] = round(statistics.median(times["batch8_batch"]) / statistics.median(times["batch8_clip"]), 3)
        row["against_batch1"] = diff
        report["T"][T] = row
        print(f"T={T}", json.dumps(row), flush=True)
        del vps
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, f"clip_coupling_rate_T{args.T}.json"), "w") as f:
        json.dump(report, f, indent=1)


def kernels(args):
    import torch
    from mumpy_hip import ops
    from weight_fill import seeded_randn
    dev = torch.device("cuda:0")
    b, manifest = 8, []
    pad = ops.pad_mask(dev)
    for side, c in STAGES:
        for r in (1, 3, 5):
            nq = b * (side // 7) ** 2
            x2 = seeded_randn(side + r, b, r * side * side, c).to(dev)
            q = seeded_randn(side + r + 1, b, side * side, c).to(dev)
            pos = (torch.rand(nq, 3, 49, 2, generator=torch.Generator().manual_seed(side + r)) * 2.2 - 1.1).to(dev)
            wkv, bkv = (seeded_randn(c, 2 * c, c) / c ** 0.5).to(dev), seeded_randn(c + 1, 2 * c).to(dev)
            kv = ops.deform_sample_kv(x2, pos, wkv, bkv, b, r * side, side, c, nq)
            calls = {
                "sample": lambda g: ops.deform_sample(x2, pos, b, r * side, side, c, nq, groups=g),
                "sample_kv": lambda g: ops.deform_sample_kv(x2, pos, wkv, bkv, b, r * side, side, c, nq, groups=g),
                "sample_kv_mm16": lambda g: ops.deform_sample_kv(x2, pos, wkv, bkv, b, r * side, side, c, nq, math="bf16", groups=g),
                "attention": lambda g: ops.deform_attention(q, kv, pad, b, side, side, c, r, 32 ** -0.5, groups=g),
                "attention_mm16": lambda g: ops.deform_attention(q, kv, pad, b, side, side, c, r, 32 ** -0.5, math="bf16", groups=g),
            }
            torch.cuda.synchronize()
            manifest.append(dict(label="setup", launches=1))          # the deform_sample_kv above
            for name, fn in calls.items():
                for rep in range(args.reps):                          # frozen and grouped alternate, launch by launch
                    fn(1)
                    fn(b)
                torch.cuda.synchronize()
                manifest.append(dict(label=f"{name} {side}x{side} C={c} r={r}", launches=2 * args.reps))
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "clip_kernels_manifest.json"), "w") as f:
        json.dump(manifest, f)
    print(f"{len(manifest)} groups of launches issued")


def kernels_report(args):
    manifest = json.load(open(os.path.join(args.dir, "clip_kernels_manifest.json")))
    trace = glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(trace)))
    rows = [r for r in rows if any(k in r[2] for k in KERNELS)]
    assert len(rows) == sum(m["launches"] for m in manifest), (len(rows), sum(m["launches"] for m in manifest))
    i, out = 0, []
    for m in manifest:
        part, i = rows[i:i + m["launches"]], i + m["launches"]
        if m["label"] == "setup":
            continue
        frozen, grouped = [(e - s) / 1e3 for s, e, _ in part[0::2]], [(e - s) / 1e3 for s, e, _ in part[1::2]]
        f, g = statistics.median(frozen), statistics.median(grouped)
        out.append(dict(case=m["label"], frozen_us=round(f, 2), grouped_us=round(g, 2), ratio=round(g / f, 3),
                        frozen_range=[round(min(frozen), 2), round(max(frozen), 2)], grouped_range=[round(min(grouped), 2), round(max(grouped), 2)]))
        print(f"{m['label']:42s} frozen {f:8.2f} us   grouped {g:8.2f} us   x{g / f:.3f}")
    with open(os.path.join(args.dir, "clip_kernels.json"), "w") as fjson:
        json.dump(out, fjson, indent=1)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    a = sub.add_parser("rate")
    a.add_argument("--frames", type=int, default=96)
    a.add_argument("--rounds", type=int, default=5)
    a.add_argument("--T", type=int, default=3)
    a = sub.add_parser("kernels")
    a.add_argument("--reps", type=int, default=20)
    a = sub.add_parser("kernels-report")
    a.add_argument("dir")
    args = ap.parse_args()
    if args.mode == "kernels-report":
        return kernels_report(args)
    import torch
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 8)))
    with torch.no_grad():
        (rate if args.mode == "rate" else kernels)(args)


if __name__ == "__main__":
    main()
