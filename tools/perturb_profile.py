"""Measurements behind profiles/perturb.md: ops.jpeg_roundtrip_u8 / ops.gaussian_blur_u8 / ops.resize_nearest_u8 (the ordinary
perturbations of include/mumpy_perturb.h) against the per-frame Pillow loops they replace, and VideoPredictor with perturb on and off.

    python tools/perturb_profile.py [--rounds 7] [--reps 50] [--quality 75] [--radius 2.0] [--video-frames 100] [--no-predictor]

Two jobs: `batch`, 40 frames of 224 x 224 (a B = 8, T = 5 training batch on its canvas), and `video`, 100 frames of 240 x 432 (one
uploaded video).  The frames are a seeded ramp with noise.  Before anything is timed each entry's output is compared with Pillow's
byte for byte; the outcome is part of the report.
  jpeg / blur     device events around `--reps` back-to-back calls of the entry (its two launches together: block coding + merge,
                  row passes + column passes), in place on frames that are already on the device, with the caller's workspace, per call;
                  median and range over `--rounds` rounds after one warm-up round.  The buffers (7 - 31 MB) stay in the Infinity Cache.
  resize          the NEAREST gather 240 x 432 -> 224 x 224 of the batch job's 40 frames, the same way.
  pillow_*        host clock around the per-frame loop on one thread of the same machine in the same process:
                  save(format="JPEG", quality=q) + Image.open + load, and filter(ImageFilter.GaussianBlur(radius)).
  predictor       host clock to a device synchronise around VideoPredictor.predict of the video job (T = 3, batch 8, graphed, seeded
                  weights, annotations given): perturb=None, ("jpeg", q), ("blur", r) and both; frames/s."""
import argparse
import io
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


def frames_of(n, h, w, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([yy + xx // 2, 255 - xx // 2, (yy * 2 + xx) % 256], -1)
    return np.clip(base[None] + g.integers(-20, 21, (n, h, w, 3)), 0, 255).astype(np.uint8)


def spread(v):
    return dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))


def main():
    import torch
    from PIL import Image, ImageFilter
    from mumpy_hip import ops
    from mumpy_hip.perturb import jpeg_tables
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--quality", type=int, default=75)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--video-frames", type=int, default=100)
    ap.add_argument("--no-predictor", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)
    q, rad = args.quality, args.radius
    report = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, quality=q, radius=rad, jobs={})

    def pil_jpeg(a):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, format="JPEG", quality=q)
        buf.seek(0)
        return np.asarray(Image.open(buf))

    def pil_blur(a):
        return np.asarray(Image.fromarray(a).filter(ImageFilter.GaussianBlur(radius=rad)))

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

    for job, (n, h, w) in dict(batch=(40, SIDE, SIDE), video=(args.video_frames, 240, 432)).items():
        host = frames_of(n, h, w, seed=h)
        src = torch.from_numpy(host).to(dev)
        work = torch.empty_like(src)
        lib = ops._lib()
        ws = torch.empty(max(int(lib.mumpy_jpeg_roundtrip_workspace_bytes(n, h, w)), int(lib.mumpy_gaussian_blur_workspace_bytes(n, h, w))),
                         dtype=torch.uint8, device=dev)
        tabs = ops.jpeg_tables_u16(jpeg_tables(q)[None], dev)
        sel = torch.zeros(n, dtype=torch.int32, device=dev)
        params = ops.blur_params(rad, n, dev)
        differing = dict(jpeg=int((ops.jpeg_roundtrip_u8(src, tabs, sel=sel).cpu().numpy() != np.stack([pil_jpeg(a) for a in host])).sum()),
                         blur=int((ops.gaussian_blur_u8(src, params).cpu().numpy() != np.stack([pil_blur(a) for a in host])).sum()))
        work.copy_(src)
        variants = {"jpeg": lambda: device_ms(lambda: ops.jpeg_roundtrip_u8(work, tabs, sel=sel, out=work, workspace=ws)),
                    "blur": lambda: device_ms(lambda: ops.gaussian_blur_u8(work, params, out=work, workspace=ws)),
                    "pillow_jpeg": lambda: host_ms(lambda: [pil_jpeg(a) for a in host]),
                    "pillow_blur": lambda: host_ms(lambda: [pil_blur(a) for a in host])}
        if job == "batch":
            big = torch.from_numpy(frames_of(n, 240, 432, seed=1)).to(dev)
            ops.resize_nearest_u8(big, (SIDE, SIDE), out=work)                                     # uploads the tables
            variants["resize"] = lambda: device_ms(lambda: ops.resize_nearest_u8(big, (SIDE, SIDE), out=work))
        row = measure(variants)
        row["frames"], row["size"], row["bytes_per_pass"] = n, [h, w], 2 * n * h * w * 3
        row["bytes_differing_from_pillow"] = differing
        row["pillow_over_kernel"] = dict(jpeg=round(row["pillow_jpeg"]["median"] / row["jpeg"]["median"], 1),
                                         blur=round(row["pillow_blur"]["median"] / row["blur"]["median"], 1))
        report["jobs"][job] = row
        print(job, json.dumps(row), flush=True)

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
        specs = {"off": None, "jpeg": ("jpeg", q), "blur": ("blur", rad), "blur+jpeg": [("blur", rad), ("jpeg", q)]}
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
    with open(os.path.join(out_dir, "perturb.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
