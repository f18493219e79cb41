"""Measurements behind profiles/video_predict.md: frames/s of mumpy_hip.video.VideoPredictor on a whole video against the loop a user
writes without it, and the B = 1, T = 3 eager latency.

    python tools/video_predict_profile.py [--frames 96] [--rounds 5] [--configs 3x8,3x1,5x8,5x1]

Synthetic 432 x 240 footage (frames (N, 240, 432, 3) uint8 and annotations (N, 224, 224) uint8 on the host, seeded), seeded weights.
Per configuration T x batch, three variants process the same video and produce its N masks and its metric vector:
  loop       host-assembled clip batches -> evaluate.eval_step -> distributed.eval_metric_vector: the index lists built by hand, every
             batch's (batch, T, 240, 432, 3) uint8 clips gathered on the host and uploaded (each frame T times), eval_step's staging
             kernel, the eager forward, the metric vector added up on the device;
  eager      VideoPredictor(graph=False): frames uploaded once, the same launches issued from Python;
  graphed    VideoPredictor(graph=True): frames uploaded once, two table uploads and one graph replay per batch.
A sample is one whole video, host clock from the first host instruction to a device synchronise after the metric vector is complete
(uploads included); the variants alternate in one process (order reversed every round), one warm-up round, `--rounds` timed ones;
median and range.  Before anything is timed the masks of the three variants are compared bit for bit and the metric vectors to 1e-12;
the outcome is part of the report.
latency: evaluate.eval_step on one assembled B = 1, T = 3 uint8 clip, synchronised after every call (the eager latency), and one
replay of the B = 1 predictor's graph, median of 50 each."""
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


def main():
    import torch
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from mumpy_hip.distributed import eval_metric_vector
    from mumpy_hip.evaluate import eval_step
    from mumpy_hip.video import VideoPredictor
    from weight_fill import fill_module_
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=96)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--configs", default="3x8,3x1,5x8,5x1")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 8)))
    g = np.random.default_rng(432)
    n = args.frames
    frames = g.integers(0, 256, (n, HS, WS, 3), dtype=np.uint8)
    gt = (g.integers(0, 3, (n, SIDE, SIDE)) > 1).astype(np.uint8) * 255
    frames_t, gt_t = torch.from_numpy(frames), torch.from_numpy(gt)
    report = dict(device=torch.cuda.get_device_name(0), frames=n, source=[HS, WS], rounds=args.rounds, configs={})
    models = {}
    for cfg in args.configs.split(","):
        T, batch = (int(v) for v in cfg.split("x"))
        if T not in models:
            models[T] = (fill_module_(Encoder(num_frames=T).eval()).to(dev),
                         fill_module_(Decoder(input_token_temporal_dims=[1, 1, T]).eval()).to(dev))
        enc, dec = models[T]
        k = T // 2

        def loop():
            rows = [[min(max(j, 0), n - 1) for j in range(i - k, i + k + 1)] for i in range(n)]       # universaldataloader.py:46
            total, masks = torch.zeros(3, dtype=torch.float64, device=dev), []
            for b0 in range(0, n, batch):
                clips = torch.from_numpy(frames[np.asarray(rows[b0:b0 + batch])]).to(dev)              # (b, T, 240, 432, 3) uint8
                mask, _, _ = eval_step(enc, dec, clips)
                total += eval_metric_vector(mask, gt_t[b0:b0 + batch].to(dev))
                masks.append(mask)
            return torch.cat(masks).reshape(n, SIDE, SIDE) * 255, total

        def predictor(vp):
            def run():
                vp.reset_metrics()
                return vp.predict(frames_t, gt_t), vp.metric_vector()
            return run

        vps = {name: VideoPredictor(enc, dec, T=T, src_hw=(HS, WS), batch=batch, max_frames=n, graph=graph)
               for name, graph in (("eager", False), ("graphed", True))}
        variants = {"loop": loop, "eager": predictor(vps["eager"]), "graphed": predictor(vps["graphed"])}
        # the same masks and the same metric vector, before anything is timed (also the warm-up of every shape)
        outs = {}
        for name, fn in variants.items():
            masks, metric = fn()
            torch.cuda.synchronize()
            outs[name] = (masks.clone(), metric.clone())
        same = {name: bool(torch.equal(outs[name][0], outs["loop"][0])) for name in ("eager", "graphed")}
        mdiff = {name: float(((outs[name][1] - outs["loop"][1]).abs() / outs["loop"][1].abs().clamp_min(1e-30)).max())
                 for name in ("eager", "graphed")}
        if not (all(same.values()) and max(mdiff.values()) <= 1e-12):       # (expected only with a ragged tail: the loop's last batch is smaller)
            print(f"{cfg}: the variants DISAGREE: masks equal {same}, metric relative difference {mdiff}", flush=True)
        times, names = {v: [] for v in variants}, list(variants)
        for r in range(1 + args.rounds):
            for name in (names if r % 2 == 0 else names[::-1]):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                variants[name]()
                torch.cuda.synchronize()
                if r >= 1:
                    times[name].append(time.perf_counter() - t0)
        row = {name: dict(fps_median=round(n / statistics.median(v), 1), fps_min=round(n / max(v), 1), fps_max=round(n / min(v), 1),
                          ms_per_video_median=round(1e3 * statistics.median(v), 1)) for name, v in times.items()}
        row["ratio_graphed_over_loop"] = round(statistics.median(times["loop"]) / statistics.median(times["graphed"]), 2)
        row["ratio_eager_over_loop"] = round(statistics.median(times["loop"]) / statistics.median(times["eager"]), 2)
        row["masks_equal_loop"], row["metric_rel_diff"] = same, mdiff
        row["mask_fraction"] = round(float((outs["graphed"][0] != 0).double().mean()), 4)
        if (T, batch) == (3, 1):
            clip = torch.from_numpy(frames[[0, 0, 1]][None]).to(dev)
            vp = vps["graphed"]

            def timed(fn, reps=50):
                v = []
                for _ in range(reps):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    torch.cuda.synchronize()
                    v.append(1e3 * (time.perf_counter() - t0))
                return dict(median_ms=round(statistics.median(v), 3), min_ms=round(min(v), 3), max_ms=round(max(v), 3))
            row["latency_b1_t3"] = dict(eval_step_eager=timed(lambda: eval_step(enc, dec, clip)), graph_replay=timed(vp.graph.replay))
        report["configs"][cfg] = row
        print(cfg, json.dumps(row), flush=True)
        del vps, variants
    out_dir = os.environ.get("MUMPY_PROFILE_OUT", os.path.join(ROOT, "profile_out"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "video_predict.json"), "w") as f:
        json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
