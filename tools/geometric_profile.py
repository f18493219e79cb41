"""Measurements behind profiles/geometric.md: ops.geometric_u8 (the affine operations and Cutout of include/mumpy_geometric.h) per kind
against the per-frame Pillow loop it replaces and next to the photometric streaming launch, in one job.

    python tools/geometric_profile.py [--rounds 5] [--reps 50] [--kinds shear_x,rotate] [--jobs batch,many] [--pillow-frames 40]
                                      [--no-pillow]

Two jobs: `batch`, 40 frames of 224 x 224 x 3 (a B = 8, T = 5 training batch on its canvas: 6 MB in, 6 MB out, a launch of a few
microseconds of traffic, so its time is mostly the launch), and `many`, 1280 such frames (193 MB in, 193 MB out: more than the last
cache level holds, so its rate is a memory rate).  The frames are a seeded ramp with noise.  Before anything is timed each kind's
output is compared with Pillow's byte for byte (on the first --pillow-frames frames); the outcome is part of the report.
  <kind>          device events around `--reps` back-to-back calls of the entry (one launch each), src -> dst on frames that are
                  already on the device, with a params tensor, per call; median and range over `--rounds` rounds after one warm-up
                  round, the variants alternating in order.  algorithmic_gbps is 6 H W bytes per image (one read, one write) over
                  that time; hbm_share is that rate over the 6.3 TB/s a copy achieves on this chip.  A shift or rotation that moves
                  pixels out reads less than that; the figure is the nominal one for every kind.
  none            the same entry with mode 0 rows: the dword-copy path.
  photo_invert    ops.photometric_u8 with ("invert", None) on the same frames, out of place: the streaming launch of the sibling
                  surface (its call is three launches, two of them near-empty for this kind), by the same accounting.
  pillow_<kind>   host clock around the per-frame Pillow loop (gen_geometric_goldens.pil_geometric / pil_cutout, the reference's
                  calls) on one thread of the same machine in the same process, per frame times the job's frame count."""
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
SETTINGS = dict(shear_x=0.2, shear_y=-0.2, translate_x=0.25, translate_y=-0.25, translate_x_abs=7.5, translate_y_abs=-7.5, rotate=-30.0,
                rotate90=90.0, cutout=(60, 40, 127.7, 107.2))
JOBS = dict(batch=40, many=1280)


def frames_of(n, h, w, seed):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([yy // 5 + xx // 9, 235 - xx // 9, (yy * 2 + xx) % 200 + 20], -1)
    noise = g.integers(-20, 21, (min(n, 40), h, w, 3))
    return np.stack([np.clip(base + noise[k % len(noise)] + k % 7, 1, 255).astype(np.uint8) for k in range(n)])


def spread(v):
    return dict(median=round(statistics.median(v), 5), min=round(min(v), 5), max=round(max(v), 5))


def main():
    import torch
    from gen_geometric_goldens import pil_cutout, pil_geometric
    from mumpy_hip import geometric as G
    from mumpy_hip import ops
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--kinds", default=",".join(SETTINGS))
    ap.add_argument("--jobs", default=",".join(JOBS))
    ap.add_argument("--pillow-frames", type=int, default=40)
    ap.add_argument("--no-pillow", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)
    kinds = [k for k in args.kinds.split(",") if k]
    hw = (SIDE, SIDE)
    report = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, settings={k: SETTINGS[k] for k in kinds}, jobs={})

    def name_of(k):
        return "rotate" if k.startswith("rotate") else k

    def pil(a, k):
        return pil_cutout(a, SETTINGS[k]) if k == "cutout" else pil_geometric(a, name_of(k), SETTINGS[k])

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
        t0 = time.perf_counter()
        fn()
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
        n = JOBS[job]
        host = frames_of(n, SIDE, SIDE, seed=SIDE)
        src = torch.from_numpy(host).to(dev)
        work = torch.empty_like(src)
        m = min(n, args.pillow_frames)
        rows = {k: torch.from_numpy(np.stack([G.params_row(name_of(k), SETTINGS[k], hw)] * n)).to(dev) for k in kinds}
        rows["none"] = torch.zeros(n, 8, dtype=torch.int32, device=dev)
        photo = ops.photometric_params(("invert", None), n, dev)
        ws = torch.empty(int(ops._lib().mumpy_photometric_workspace_bytes(n, SIDE, SIDE)), dtype=torch.uint8, device=dev)
        differing, variants = {}, {}
        for k in kinds:
            ops.geometric_u8(src, rows[k], out=work)
            if not args.no_pillow:
                differing[k] = int((work[:m].cpu().numpy() != np.stack([pil(a, k) for a in host[:m]])).sum())
                variants["pillow_" + k] = lambda k=k: host_ms(lambda: [pil(a, k) for a in host[:m]]) * n / m
            variants[k] = lambda k=k: device_ms(lambda: ops.geometric_u8(src, rows[k], out=work))
        variants["none"] = lambda: device_ms(lambda: ops.geometric_u8(src, rows["none"], out=work))
        variants["photo_invert"] = lambda: device_ms(lambda: ops.photometric_u8(src, photo, out=work, workspace=ws))
        row = measure(variants)
        row["frames"], row["size"], row["algorithmic_bytes"] = n, [SIDE, SIDE, 3], 6 * n * SIDE * SIDE
        row["bytes_differing_from_pillow"], row["pillow_frames_timed"] = differing, m
        for k in kinds + ["none", "photo_invert"]:
            rate = row["algorithmic_bytes"] / (1e-3 * row[k]["median"])
            row[k]["algorithmic_gbps"], row[k]["hbm_share"] = round(rate / 1e9, 1), round(rate / HBM_ACHIEVABLE, 3)
            if not args.no_pillow and "pillow_" + k in row:
                row[k]["pillow_over_kernel"] = round(row["pillow_" + k]["median"] / row[k]["median"], 1)
        report["jobs"][job] = row
        print(job, json.dumps(row), flush=True)
        del src, work, ws
    out_dir = os.environ.get("MUMPY_PROFILE_OUT", os.path.join(ROOT, "profile_out"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "geometric.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
