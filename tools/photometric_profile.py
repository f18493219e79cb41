"""Measurements behind profiles/photometric.md: ops.photometric_u8 (the nine photometric operations of include/mumpy_photometric.h)
against the per-frame Pillow loops it replaces, and VideoPredictor with ("contrast", 1.4) on and off.

    python tools/photometric_profile.py [--rounds 5] [--reps 20] [--kinds contrast,invert] [--jobs batch,hd] [--pillow-frames 8]
                                        [--video-frames 100] [--no-pillow] [--no-predictor]

Two jobs: `batch`, 40 frames of 224 x 224 (a B = 8, T = 5 training batch on its canvas), and `hd`, 64 frames of 1080 x 1920.  The
frames are a seeded ramp with noise.  Before anything is timed each kind's output is compared with Pillow's byte for byte (on the
first --pillow-frames frames of the hd job); the outcome is part of the report.
  <kind>          device events around `--reps` back-to-back calls of the entry (its three launches together), src -> dst on frames
                  that are already on the device, with the caller's workspace and a params tensor, per call; median and range over
                  `--rounds` rounds after one warm-up round.  algorithmic_gbps is 6 H W bytes per image (one read, one write) over
                  that time: the whole call's rate, not the apply kernel's (kinds without statistics launch two near-empty kernels
                  first); hbm_share is that rate over the 6.3 TB/s a copy achieves on this chip.
  pillow_<kind>   host clock around the per-frame Pillow loop on one thread of the same machine in the same process, per frame times
                  the job's frame count (the hd job times --pillow-frames frames).
  predictor       host clock to a device synchronise around VideoPredictor.predict of 100 frames of 240 x 432 (T = 3, batch 8,
                  graphed, seeded weights, annotations given): perturb=None and ("contrast", 1.4); frames/s."""
import argparse
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
SIDE = 224
HBM_ACHIEVABLE = 6.3e12          # bytes/s of a float4 copy on this chip
SETTINGS = dict(autocontrast=None, invert=None, equalize=None, solarize=77.5, posterize=4, contrast=1.4, color=0.6, brightness=1.4,
                sharpness=1.9)
JOBS = dict(batch=(40, SIDE, SIDE), hd=(64, 1080, 1920))


def frames_of(n, h, w, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([yy // 5 + xx // 9, 235 - xx // 9, (yy * 2 + xx) % 200 + 20], -1)
    return np.stack([np.clip(base + g.integers(-20, 21, (h, w, 3)), 0, 255).astype(np.uint8) for _ in range(n)])


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    import torch
    from gen_photometric_goldens import pil_photometric
    from mumpy_hip import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kinds", default=",".join(SETTINGS))
    ap.add_argument("--jobs", default=",".join(JOBS))
    ap.add_argument("--pillow-frames", type=int, default=8)
    ap.add_argument("--video-frames", type=int, default=100)
    ap.add_argument("--no-pillow", action="store_true")
    ap.add_argument("--no-predictor", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)
    kinds = [k for k in args.kinds.split(",") if k]
    report = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, settings={k: SETTINGS[k] for k in kinds}, jobs={})

    def device_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def host_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def measure(variants):
        times, names = {v: [] for v in variants}, list(variants)
        for r in range(1 + args.rounds):
            for name in (names if r % 2 == 0 else names[::-1]):
                t = variants[name]()
                if r >= 1:
                    times[name].append(t)
        return {name: spread(t) for name, t in times.items()}                                     # milliseconds

    for job in [j for j in args.jobs.split(",") if j]:
        n, h, w = JOBS[job]
        host = frames_of(n, h, w, seed=h)
        src = torch.from_numpy(host).to(dev)
        work = torch.empty_like(src)
        ws = torch.empty(int(ops._lib().mumpy_photometric_workspace_bytes(n, h, w)), dtype=torch.uint8, device=dev)
        m = n if job == "batch" else min(n, args.pillow_frames)
        rows = {k: ops.photometric_params((k, SETTINGS[k]), n, dev) for k in kinds}
        differing, variants = {}, {}
        for k in kinds:
            ops.photometric_u8(src, rows[k], out=work, workspace=ws)
            if not args.no_pillow:
                differing[k] = int((work[:m].cpu().numpy() != np.stack([pil_photometric(a, k, SETTINGS[k]) for a in host[:m]])).sum())
                variants["pillow_" + k] = lambda k=k: host_ms(lambda: [pil_photometric(a, k, SETTINGS[k]) for a in host[:m]]) * n / m
            variants[k] = lambda k=k: device_ms(lambda: ops.photometric_u8(src, rows[k], out=work, workspace=ws))
        row = measure(variants)
        row["frames"], row["size"], row["algorithmic_bytes"], row["workspace_bytes"] = n, [h, w], 6 * n * h * w, ws.numel()
        row["bytes_differing_from_pillow"], row["pillow_frames_timed"] = differing, m
        for k in kinds:
            rate = row["algorithmic_bytes"] / (1e-3 * row[k]["median"])
            row[k]["algorithmic_gbps"], row[k]["hbm_share"] = round(rate / 1e9, 1), round(rate / HBM_ACHIEVABLE, 3)
            if not args.no_pillow:
                row[k]["pillow_over_kernel"] = round(row["pillow_" + k]["median"] / row[k]["median"], 1)
        report["jobs"][job] = row
        print(job, json.dumps(row), flush=True)
        del src, work, ws

    if not args.no_predictor:
        from models.decoder.decoder import Decoder
        from models.encoder.encoder import Encoder
        from mumpy_hip.video import VideoPredictor
        from weight_fill import fill_module_
        torch.set_num_threads(max(1, min(16, os.cpu_count() or 8)))
        n = args.video_frames
        enc, dec = fill_module_(Encoder().eval()).to(dev), fill_module_(Decoder().eval()).to(dev)
        frames_t = torch.from_numpy(frames_of(n, 240, 432, seed=240))
        gt_t = torch.from_numpy(((np.random.default_rng(3).random((n, SIDE, SIDE)) < 0.3) * 255).astype(np.uint8))
        specs = {"off": None, "contrast": ("contrast", 1.4)}
        vps = {name: VideoPredictor(enc, dec, T=3, src_hw=(240, 432), batch=8, max_frames=n, perturb=s) for name, s in specs.items()}

        def run(vp):
            def go():
                vp.reset_metrics()
                vp.predict(frames_t, gt_t)
            return lambda: host_ms(go)
        row = measure({name: run(vp) for name, vp in vps.items()})
        for name in row:
            row[name]["fps_median"] = round(n / (1e-3 * row[name]["median"]), 1)
        report["predictor"] = dict(frames=n, T=3, batch=8, **row)
        print("predictor", json.dumps(report["predictor"]), flush=True)
    out_dir = os.environ.get("MUMPY_PROFILE_OUT", os.path.join(ROOT, "profile_out"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "photometric.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
