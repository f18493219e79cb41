"""Measurements behind profiles/mask_clean.md: ops.mask_clean_u8 (include/mumpy_postprocess.h) on 224 x 224 masks against the host
round trip it replaces, and VideoPredictor.predict with clean= on and off, in one job.

    python tools/mask_clean_profile.py [--rounds 5] [--reps 20] [--nimg 8,64,1024] [--host-frames 32] [--predict-frames 64] [--no-predict]

Three kinds of mask, seeded: `sparse` (noise at density 0.02 plus a few filled discs: a clean prediction with specks), `percolating`
(noise at density 0.59, the site-percolation threshold of the square lattice: components of every size, the most unions per pixel) and
`spiral` (one component of 25,312 pixels, the longest chain of links).  Every row is {min_area 20, max_hole 50, connectivity 8}.
Before anything is timed the device result of the first --host-frames masks is compared with the numpy statement byte for byte; the
outcome is part of the report.
  device        device events around `--reps` back-to-back launches on masks that are already on the device, with gt and counts, per
                launch; median and range over `--rounds` rounds after one warm-up round, the kinds alternating in order.
                per_frame_us = that time over nimg; read_write_gbps = 3 nimg H W bytes (mask and gt read, out written) over it.
  host          a host clock around what a caller does today: the bank .cpu() (ends in a synchronise), a per-frame loop on one
                thread, rescoring of the cleaned masks with numpy; timed on --host-frames frames and scaled to nimg.  The loop is
                scipy.ndimage (label + bincount, twice) when scipy imports, mumpy_hip.postprocess.clean otherwise; which is reported.
  predict       host clock around VideoPredictor.predict + synchronise on --predict-frames random frames with annotations (seeded
                weights, graph=True, batch 8), clean=None against clean=dict(min_area=20, max_hole=50), alternating, after a warm-up
                predict of each; frames/s.  The masks of random weights are noise-like, which is the heavy case for the kernel."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "multilateral-temporal-view-pyramid-transformer-for-video-inpainting-detection_amd"),
          os.path.join(ROOT, "tests", "golden"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
SIDE = 224
SETTING = dict(min_area=20, max_hole=50, connectivity=8)


def masks_of(kind, n, seed):
    from gen_mask_clean_goldens import spiral
    g = np.random.default_rng(seed)
    if kind == "spiral":
        return np.stack([np.where(spiral(SIDE, SIDE), 255, 0).astype(np.uint8)] * n)
    if kind == "percolating":
        base = [(g.random((SIDE, SIDE)) < 0.59) for _ in range(min(n, 16))]
    else:
        yy, xx = np.mgrid[0:SIDE, 0:SIDE]
        base = []
        for _ in range(min(n, 16)):
            m = g.random((SIDE, SIDE)) < 0.02
            for _ in range(3):
                cy, cx, r = g.integers(30, SIDE - 30), g.integers(30, SIDE - 30), g.integers(8, 28)
                m |= ((yy - cy) ** 2 + (xx - cx) ** 2 <= r * r) & (g.random((SIDE, SIDE)) < 0.97)
            base.append(m)
    return np.stack([np.where(base[k % len(base)], 255, 0).astype(np.uint8) for k in range(n)])


def spread(v):
    return dict(median=round(statistics.median(v), 5), min=round(min(v), 5), max=round(max(v), 5))


def host_clean(have_scipy):
    from mumpy_hip import postprocess as P
    if not have_scipy:
        return lambda m: P.clean(m, SETTING["min_area"], SETTING["max_hole"], 8)[0]
    from gen_mask_clean_goldens import scipy_clean
    return lambda m: scipy_clean(m, SETTING["min_area"], SETTING["max_hole"], 8)[0]


def main():
    import torch
    from mumpy_hip import ops
    from mumpy_hip import postprocess as P
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nimg", default="8,64,1024")
    ap.add_argument("--host-frames", type=int, default=32)
    ap.add_argument("--predict-frames", type=int, default=64)
    ap.add_argument("--no-predict", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(1)
    try:
        import scipy
        have_scipy = scipy.__version__
    except ImportError:
        have_scipy = None
    clean_one = host_clean(have_scipy)
    report = dict(device=torch.cuda.get_device_name(0), rounds=args.rounds, reps=args.reps, setting=SETTING,
                  host_loop="scipy.ndimage " + have_scipy if have_scipy else "mumpy_hip.postprocess.clean (numpy)", launches={})

    def device_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / args.reps

    def measure(variants):
        times, names = {v: [] for v in variants}, list(variants)
        for r in range(1 + args.rounds):
            for name in (names if r % 2 == 0 else names[::-1]):
                t = variants[name]()
                if r >= 1:
                    times[name].append(t)
        return {name: spread(t) for name, t in times.items()}                                     # milliseconds

    g = np.random.default_rng(1)
    for n in [int(v) for v in args.nimg.split(",") if v]:
        gt = torch.from_numpy((g.random((min(n, 16), SIDE, SIDE)) < 0.3).astype(np.uint8) * 255).to(dev).repeat(-(-n // 16), 1, 1)[:n].contiguous()
        rows = ops.mask_clean_params(SETTING, n, dev)
        ws = ops.mask_clean_workspace(n, SIDE, SIDE, dev)
        counts, stats = torch.empty(n, 4, dtype=torch.int32, device=dev), torch.empty(n, 8, dtype=torch.int32, device=dev)
        m = min(n, args.host_frames)
        bufs, variants, row = {}, {}, dict(frames=n, host_frames_timed=m, bytes_differing_from_numpy={}, status_nonzero={}, stats_first={})
        for kind in ("sparse", "percolating", "spiral"):
            host = masks_of(kind, n, seed=n)
            src = torch.from_numpy(host).to(dev)
            out = torch.empty_like(src)
            bufs[kind] = (host, src, out)
            ops.mask_clean_u8(src, rows, out=out, gt=gt, counts=counts, stats=stats, workspace=ws)
            want = np.stack([P.clean(a, SETTING["min_area"], SETTING["max_hole"], 8)[0] for a in host[:m]])
            row["bytes_differing_from_numpy"][kind] = int((out[:m].cpu().numpy() != want).sum())
            row["status_nonzero"][kind] = int((stats[:, 7] != 0).sum())
            row["stats_first"][kind] = stats[0].cpu().tolist()
            variants[kind] = lambda k=kind: device_ms(lambda: ops.mask_clean_u8(bufs[k][1], rows, out=bufs[k][2], gt=gt, counts=counts,
                                                                                stats=stats, workspace=ws))

            def host_path(k=kind):
                t0 = time.perf_counter()
                bank = bufs[k][1][:m].cpu().numpy()                                               # ends in a synchronise
                t1 = time.perf_counter()
                cleaned = [clean_one(a) for a in bank]
                t2 = time.perf_counter()
                gth = gt[:m].cpu().numpy() > 0
                for c, t in zip(cleaned, gth):
                    p = c != 0
                    (p & t).sum(), p.sum(), t.sum(), (p | t).sum()
                t3 = time.perf_counter()
                row.setdefault("host_parts_ms_per_frame", {})[k] = dict(copy=round(1e3 * (t1 - t0) / m, 4), loop=round(1e3 * (t2 - t1) / m, 4),
                                                                        rescore=round(1e3 * (t3 - t2) / m, 4))
                return 1e3 * (t3 - t0) * n / m
            variants["host_" + kind] = host_path
        row.update(measure(variants))
        for kind in ("sparse", "percolating", "spiral"):
            ms = row[kind]["median"]
            row[kind]["per_frame_us"] = round(1e3 * ms / n, 2)
            row[kind]["read_write_gbps"] = round(3 * n * SIDE * SIDE / (1e-3 * ms) / 1e9, 1)
            row[kind]["host_over_device"] = round(row["host_" + kind]["median"] / ms, 1)
        report["launches"][str(n)] = row
        print(n, json.dumps(row), flush=True)
        del bufs, gt, ws

    if not args.no_predict:
        from models.decoder.decoder import Decoder
        from models.encoder.encoder import Encoder
        from mumpy_hip.video import VideoPredictor
        from weight_fill import fill_module_
        enc, dec = fill_module_(Encoder()).eval().to(dev), fill_module_(Decoder()).eval().to(dev)
        n, hs, ws_ = args.predict_frames, 240, 432
        frames = torch.from_numpy(g.integers(0, 256, (n, hs, ws_, 3), dtype=np.uint8)).to(dev)
        gt = torch.from_numpy((g.random((n, SIDE, SIDE)) < 0.3).astype(np.uint8) * 255).to(dev)
        kw = dict(T=3, src_hw=(hs, ws_), batch=8, max_frames=n, graph=True)
        vps = dict(off=VideoPredictor(enc, dec, **kw), on=VideoPredictor(enc, dec, clean=SETTING, **kw))
        for vp in vps.values():
            vp.predict(frames, gt)
        torch.cuda.synchronize()

        def predict_ms(vp):
            t0 = time.perf_counter()
            vp.predict(frames, gt)
            torch.cuda.synchronize()
            return 1e3 * (time.perf_counter() - t0)
        row = measure({k: (lambda vp=vp: predict_ms(vp)) for k, vp in vps.items()})
        for k in vps:
            row[k]["frames_per_s"] = round(n / (1e-3 * row[k]["median"]), 1)
        row["clean_cost_ms"] = round(row["on"]["median"] - row["off"]["median"], 3)
        bank = vps["on"].bank[:n]
        t0 = time.perf_counter()
        host = bank.cpu().numpy().reshape(n, SIDE, SIDE)
        cleaned = [clean_one(a) for a in host[:min(n, args.host_frames)]]
        row["host_round_trip_ms"] = round(1e3 * (time.perf_counter() - t0) * n / len(cleaned), 1)
        row["frames"], row["stats_mean"] = n, vps["on"].clean_statistics().double().mean(0).cpu().tolist()
        row["bytes_differing_from_host_loop"] = int(sum((c != o).sum() for c, o in zip(cleaned, vps["on"].clean_bank[:len(cleaned)].view(-1, SIDE, SIDE).cpu().numpy())))
        report["predict"] = row
        print("predict", json.dumps(row), flush=True)
    out_dir = os.environ.get("MUMPY_PROFILE_OUT", os.path.join(ROOT, "profile_out"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "mask_clean.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
