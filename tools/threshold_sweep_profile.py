"""Measurements behind profiles/threshold_sweep.md: what scoring a video at every threshold of a table costs beside scoring it at one.

    python tools/threshold_sweep_profile.py [--frames 96] [--rounds 5] [--launches 200]

The method is that of tools/video_predict_profile.py: one process, the variants alternate (order reversed every round), one warm-up
round, `--rounds` timed ones, median and [min .. max].
  1. launches: ops.score_exceed at (8 clips, 224 x 224, K = 255) and ops.sweep_metrics at `--frames` frames, beside ops.mask_score_u8
     and ops.frame_metrics at the same shapes in the same run.  A sample is `--launches` back-to-back launches between two events,
     divided by their number.  Twice: with about 3 % of the pixels set and with 50 % -- a set pixel's probability is uniform over
     (0, 1), so it lands in an interior bin of the table and costs an LDS atomic (the contention case); the others sit at a logit
     of -12, below every threshold.  The annotation has the same density.
  2. predictor: frames/s of the graphed VideoPredictor (T = 5, batch 8) on the 96-frame job of profiles/video_predict.md with
     sweep=None and with the default table.  A sample is one whole video, host clock from the first host instruction to a device
     synchronise after the accumulators are complete.
  3. what it replaces: the same video scored at 255 thresholds by 255 passes of the sweep=None predictor -- EXTRAPOLATED from the
     passes timed in (2), 255 times their median."""
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
HS, WS, SIDE = 240, 432, 224
T, BATCH, K = 5, 8, 255


def _spread(v, scale=1.0, digits=2):
    return dict(median=round(scale * statistics.median(v), digits), min=round(scale * min(v), digits), max=round(scale * max(v), digits))


def _alternate(variants, rounds):
    """{name: [sample, ...]}: every variant once per round, order reversed every round, the first round dropped."""
    times, names = {v: [] for v in variants}, list(variants)
    for r in range(1 + rounds):
        for name in (names if r % 2 == 0 else names[::-1]):
            s = variants[name]()
            if r >= 1:
                times[name].append(s)
    return times


def launches(torch, ops, video, dev, density, nframes, rounds, reps):
    g = np.random.default_rng(int(1000 * density))
    npix = SIDE * SIDE
    on = g.random((BATCH, npix)) < density
    u = np.clip(g.random((BATCH, npix)), 1e-4, 1 - 1e-4)
    logits = torch.from_numpy(np.where(on, np.log(u / (1 - u)), -12.0).astype(np.float32)).to(dev)
    mask = torch.from_numpy((on & (u > 0.5)).astype(np.uint8)).to(dev)
    gt = torch.from_numpy(((g.random((nframes, npix)) < density) * 255).astype(np.uint8)).to(dev)
    dest = torch.arange(BATCH, dtype=torch.int32, device=dev)
    table = torch.from_numpy(video.sweep_table()).to(dev)
    bank = torch.zeros(nframes, npix, dtype=torch.uint8, device=dev)
    counts = torch.zeros(nframes, 4, dtype=torch.int32, device=dev)
    exceed = torch.zeros(nframes, 2, K + 1, dtype=torch.int32, device=dev)
    acc3, acc = torch.zeros(3, dtype=torch.float64, device=dev), torch.zeros(K, 3, dtype=torch.float64, device=dev)
    pooled = torch.zeros(2, K + 1, dtype=torch.int64, device=dev)
    ops.score_exceed(logits, gt, dest, table, exceed)
    interior = float((exceed[:BATCH, :, 0] - exceed[:BATCH, :, K - 1]).sum()) / (BATCH * npix)
    for b in range(BATCH, nframes, BATCH):                           # every frame gets plausible counts for the metrics launches
        exceed[b:b + BATCH] = exceed[:BATCH][:nframes - b]
    ops.mask_score_u8(mask, dest, bank, gt=gt, counts=counts)
    for b in range(BATCH, nframes, BATCH):
        counts[b:b + BATCH] = counts[:BATCH][:nframes - b]

    def timed(fn):
        def run():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return 1e3 * e0.elapsed_time(e1) / reps                  # microseconds per launch
        return run
    variants = {
        "mask_score_u8": timed(lambda: ops.mask_score_u8(mask, dest, bank, gt=gt, counts=counts)),
        "score_exceed": timed(lambda: ops.score_exceed(logits, gt, dest, table, exceed)),
        "frame_metrics": timed(lambda: ops.frame_metrics(counts, nframes, npix, acc=acc3)),
        "sweep_metrics": timed(lambda: ops.sweep_metrics(exceed, nframes, npix, acc=acc, pooled=pooled)),
    }
    row = {name: _spread(v) for name, v in _alternate(variants, rounds).items()}
    row["interior_bin_fraction"] = round(interior, 4)
    return row


def main():
    import torch
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from mumpy_hip import ops, video
    from mumpy_hip.evaluate import finalize_sweep
    from weight_fill import fill_module_
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 8)))
    n = args.frames
    report = dict(device=torch.cuda.get_device_name(0), frames=n, rounds=args.rounds, launches_per_sample=args.launches, T=T, batch=BATCH, K=K)
    report["launch_us"] = {f"{int(100 * d)}%": launches(torch, ops, video, dev, d, n, args.rounds, args.launches) for d in (0.03, 0.5)}
    print("launch_us", json.dumps(report["launch_us"]), flush=True)

    g = np.random.default_rng(432)
    frames = torch.from_numpy(g.integers(0, 256, (n, HS, WS, 3), dtype=np.uint8))
    gt = torch.from_numpy((g.integers(0, 3, (n, SIDE, SIDE)) > 1).astype(np.uint8) * 255)
    enc = fill_module_(Encoder(num_frames=T).eval()).to(dev)
    dec = fill_module_(Decoder(input_token_temporal_dims=[1, 1, T]).eval()).to(dev)
    vps = {name: video.VideoPredictor(enc, dec, T=T, src_hw=(HS, WS), batch=BATCH, max_frames=n, graph=True, sweep=sweep)
           for name, sweep in (("sweep_off", None), ("sweep_on", True))}

    def whole_video(vp):
        def run():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vp.reset_metrics()
            vp.predict(frames, gt)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        return run
    masks = {}
    for name, vp in vps.items():                                     # the same masks and metric vector, before anything is timed
        vp.reset_metrics()
        masks[name] = (vp.predict(frames, gt).clone(), vp.metric_vector().clone())
    torch.cuda.synchronize()
    same = bool(torch.equal(masks["sweep_on"][0], masks["sweep_off"][0]) and torch.equal(masks["sweep_on"][1], masks["sweep_off"][1]))
    on = vps["sweep_on"]
    agree = bool(torch.equal(video.exceed_counts(on.exceed[:n], 127), on.counts[:n]))        # table[127] is 0.5, the predictor's thr
    result = finalize_sweep(*on.sweep_vector())
    times = _alternate({name: whole_video(vp) for name, vp in vps.items()}, args.rounds)
    med = {name: statistics.median(v) for name, v in times.items()}
    report["predictor"] = {name: dict(fps=_spread([n / s for s in v], digits=1), ms_per_video=_spread(v, 1e3, 1)) for name, v in times.items()}
    report["predictor"]["ratio_on_over_off"] = round(med["sweep_off"] / med["sweep_on"], 4)
    report["predictor"]["masks_and_metric_equal"] = same
    report["predictor"]["counts_at_0.5_equal"] = agree
    report["predictor"]["best"], report["predictor"]["auc"] = [round(v, 6) for v in result["best"]], round(result["auc"], 6)
    report["replaces"] = dict(passes=K, seconds_extrapolated=round(K * med["sweep_off"], 1), seconds_one_sweep_pass=round(med["sweep_on"], 3),
                              note=f"extrapolated: {K} x the median of the {args.rounds} timed sweep_off passes")
    print("predictor", json.dumps(report["predictor"]), flush=True)
    print("replaces", json.dumps(report["replaces"]), flush=True)
    out_dir = os.environ.get("MUMPY_PROFILE_OUT", os.path.join(ROOT, "profile_out"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "threshold_sweep.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
