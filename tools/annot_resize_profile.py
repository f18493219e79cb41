"""Measurements behind profiles/annot_resize.md: ops.resize_bilinear_u8 (the annotation resize of measure.py:21-40 on the device)
against the per-frame Pillow loop it replaces.

    python tools/annot_resize_profile.py [--frames 64] [--rounds 7] [--reps 50] [--sizes 480x854,1080x1920]

Per source size, N synthetic annotations (blobs of 255 on zeros, seeded) are resized to 224 x 224.  Before anything is timed the
kernel's output is compared with Pillow's byte for byte; the outcome is part of the report.
  kernel     device events around `--reps` back-to-back launches on annotations that are already on the device, per launch; median and
             range over `--rounds` rounds after one warm-up round.  `rotating`: the launches walk through enough distinct source
             buffers (> 300 MB together) that none is still in the 256 MiB Infinity Cache when its turn comes again -- the figure for
             annotations that arrive from memory; `resident`: the same buffer every time.  bytes/s = (N * Hs * Ws read + N * 224 * 224
             written) / time, the bytes the algorithm needs (the re-read of the rows two bands share is not counted).
  upload+kernel   host clock from the first host instruction to a device synchronise: the N native annotations copied from pageable host
             memory and resized (what VideoPredictor(gt_hw=...) does with a host tensor, in one chunk).
  pillow     host clock around `[Image.fromarray(a).resize((224, 224), Image.BILINEAR) for a in annotations]` on one thread of the
             same machine in the same process (Pillow's resize is single-threaded), and the same loop followed by the upload of
             its N x 224 x 224 result, which is what the caller of a gt_hw=None predictor pays."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilateral-temporal-view-pyramid-transformer-for-video-inpainting-detection_amd"))
SIDE = 224


def annotations(n, hs, ws, seed):
    """(n, hs, ws) uint8: a few rectangles of 255 per frame on zeros, about a tenth of the pixels."""
    g = np.random.default_rng(seed)
    a = np.zeros((n, hs, ws), np.uint8)
    for f in range(n):
        for _ in range(4):
            h, w = int(g.integers(hs // 16, hs // 4)), int(g.integers(ws // 16, ws // 4))
            y, x = int(g.integers(0, hs - h)), int(g.integers(0, ws - w))
            a[f, y:y + h, x:x + w] = 255
    return a


def spread(v):
    return dict(median=statistics.median(v), min=min(v), max=max(v))


def main():
    import torch
    from PIL import Image
    from mumpy_hip import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--sizes", default="480x854,1080x1920")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)
    n = args.frames
    report = dict(device=torch.cuda.get_device_name(0), frames=n, rounds=args.rounds, reps=args.reps, sizes={})
    for size in args.sizes.split(","):
        hs, ws = (int(v) for v in size.split("x"))
        host = annotations(n, hs, ws, seed=hs)
        host_t = torch.from_numpy(host)
        nbytes = n * hs * ws + n * SIDE * SIDE
        nbuf = max(2, -(-300_000_000 // (n * hs * ws)) + 1)
        bufs = [host_t.to(dev)]
        bufs += [bufs[0] + i for i in range(1, nbuf)]               # distinct memory; the values do not matter to the time
        out = torch.empty(n, SIDE, SIDE, device=dev, dtype=torch.uint8)

        def pillow():
            return np.stack([np.asarray(Image.fromarray(a).resize((SIDE, SIDE), Image.BILINEAR)) for a in host])

        want = pillow()
        ops.resize_bilinear_u8(bufs[0], (SIDE, SIDE), out=out)
        torch.cuda.synchronize()
        differing = int((out.cpu().numpy() != want).sum())

        def kernel_ms(rotate):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for r in range(args.reps):
                ops.resize_bilinear_u8(bufs[r % nbuf if rotate else 0], (SIDE, SIDE), out=out)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / args.reps

        def host_ms(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0)

        def upload_kernel():
            ops.resize_bilinear_u8(host_t.to(dev, non_blocking=True), (SIDE, SIDE), out=out)

        def pillow_upload():
            out.copy_(torch.from_numpy(pillow()), non_blocking=True)

        variants = {"kernel_rotating": lambda: kernel_ms(True), "kernel_resident": lambda: kernel_ms(False),
                    "upload_kernel": lambda: host_ms(upload_kernel), "pillow": lambda: host_ms(pillow),
                    "pillow_upload": lambda: host_ms(pillow_upload)}
        times, names = {v: [] for v in variants}, list(variants)
        for r in range(1 + args.rounds):
            for name in (names if r % 2 == 0 else names[::-1]):
                t = variants[name]()
                if r >= 1:
                    times[name].append(t)
        row = {name: {k: round(v, 4) for k, v in spread(t).items()} for name, t in times.items()}      # milliseconds
        for name in ("kernel_rotating", "kernel_resident"):
            row[name]["GBps_median"] = round(nbytes / (1e-3 * row[name]["median"]) / 1e9, 1)
        row["bytes"] = nbytes
        row["source_buffers"] = nbuf
        row["bytes_differing_from_pillow"] = differing
        row["pillow_over_kernel_rotating"] = round(row["pillow"]["median"] / row["kernel_rotating"]["median"], 1)
        row["pillow_upload_over_upload_kernel"] = round(row["pillow_upload"]["median"] / row["upload_kernel"]["median"], 2)
        report["sizes"][size] = row
        print(size, json.dumps(row), flush=True)
        del bufs, out
        torch.cuda.empty_cache()
    out_dir = os.environ.get("MUMPY_PROFILE_OUT", os.path.join(ROOT, "profile_out"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "annot_resize.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
