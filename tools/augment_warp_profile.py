"""Measurements behind profiles/augment_warp.md.

    python tools/augment_warp_profile.py launch     # GPU: time per launch of mumpy_augment_warp_u8_fwd by mode, beside the gather stage
    python tools/augment_warp_profile.py host       # CPU: per-sample host time of sample_double_full + clip_warp_params

launch: the DAVIS recipe's shape, 18 clips (6 samples x 3 sequences) x T = 3, L = 224 from 240 x 432 sources, 6 masks.  Every variant
is captured as a graph of 100 back-to-back launches; a sample is 10 replays between two events; the variants alternate (order
reversed every round) in one process, 4 warm-up rounds, 25 timed ones; median and range over the rounds, in microseconds per launch.
The baseline, mumpy_augment_stage_u8_fwd with the same tables, is timed in the same rounds.
host: one training sample of the Double strategy at the same shape, the mask a 70 x 200 rectangle."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilateral-temporal-view-pyramid-transformer-for-video-inpainting-detection_amd"))
SAMPLES, T, L, SRC = 6, 3, 224, (240, 432)
FIELDS = ("tab_a", "tab_b", "swap", "mode", "pos_y", "pos_x", "coef_y", "coef_x", "affine")


def _mask():
    m = np.zeros(SRC, np.uint8)
    m[60:130, 100:300] = 255
    return m


def launch():
    import torch
    from mumpy_hip import augment as A, ops
    dev = torch.device("cuda:0")
    reps, rounds, warm = 100, 25, 4
    nclips = 3 * SAMPLES
    g = np.random.default_rng(1)
    frames = torch.from_numpy(g.integers(0, 256, (nclips, T) + SRC + (3,), dtype=np.uint8)).to(dev)
    masks = torch.from_numpy(np.stack([_mask()] * SAMPLES)).to(dev)
    out, target = torch.empty(nclips, T, 3, L, L, device=dev), torch.empty(nclips, L * L, device=dev)
    MIXES = {"mixed 3/2/1": ("RandomCrop", "RandomScaleCrop", "OriginalRandomCrop", "RandomRotate", "RandomCrop", "RandomScaleCrop"),
             "mixed 3/1/2": ("RandomCrop", "RandomRotate", "OriginalRandomCrop", "RandomScaleCrop", "RandomCrop", "RandomRotate")}

    def draws(kind):
        """One seeded FullDraw per sample: all of one shape operation, or a mix.  The strategy draws modes 0 / 1 / 2 with frequencies
        1/2, 1/4, 1/4, i.e. 3, 1.5 and 1.5 of 6 samples: the two mixes (3 / 2 / 1 and 3 / 1 / 2) bracket it."""
        r, res = np.random.default_rng(7), []
        for s in range(SAMPLES):
            want = MIXES.get(kind, (kind,) * SAMPLES)[s]
            d = A.sample_double_full(r, SRC, L, _mask())
            while d.shape != want:
                d = A.sample_double_full(r, SRC, L, _mask())
            res.append(d)
        return res

    def variant(kind, entry):
        by_sample = [A.clip_warp_params(SRC, L, d) for d in draws(kind)]
        recs = [by_sample[c % SAMPLES] for c in range(nclips)]          # clip c belongs to sample c % 6, as it reads mask c % 6
        arrays = [torch.from_numpy(np.stack([np.asarray(getattr(p, f)) for p in recs]).astype(np.float32 if f == "affine" else np.int32))
                  .to(dev) for f in FIELDS]
        print(f"{kind} / {entry}: modes {[int(p.mode) for p in by_sample]}, swap {[int(p.swap) for p in by_sample]}", flush=True)
        if entry == "stage":
            return lambda: ops.augment_stage_u8(frames, *arrays[:3], masks=masks, out=out, target=target)
        return lambda: ops.augment_warp_u8(frames, *arrays, masks=masks, out=out, target=target)

    variants = {"stage_u8 (parent's entry), crops' tables": variant("RandomCrop", "stage"),
                "warp_u8, all mode 0 (RandomCrop)": variant("RandomCrop", "warp"),
                "warp_u8, all mode 1 (RandomScaleCrop)": variant("RandomScaleCrop", "warp"),
                "warp_u8, all mode 2 (RandomRotate)": variant("RandomRotate", "warp"),
                "warp_u8, mixed 3/2/1 (modes 0/1/2 by sample)": variant("mixed 3/2/1", "warp"),
                "warp_u8, mixed 3/1/2 (modes 0/1/2 by sample)": variant("mixed 3/1/2", "warp"),
                "stage_u8 (parent's entry), the 3/2/1 batch's tables": variant("mixed 3/2/1", "stage")}
    graphs, side = {}, torch.cuda.Stream()
    for name, fn in variants.items():
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        graphs[name] = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graphs[name]):
            for _ in range(reps):
                fn()
    torch.cuda.synchronize()
    times, names = {n: [] for n in graphs}, list(graphs)
    for r in range(warm + rounds):
        for n in (names if r % 2 == 0 else names[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                graphs[n].replay()
            e1.record()
            e1.synchronize()
            if r >= warm:
                times[n].append(e0.elapsed_time(e1) * 1000.0 / (10 * reps))
    results = {n: dict(median_us=round(statistics.median(v), 3), min_us=round(min(v), 3), max_us=round(max(v), 3)) for n, v in times.items()}
    for n, r in results.items():
        print(f"{n:55s} median {r['median_us']:8.3f} us   [{r['min_us']:.3f} .. {r['max_us']:.3f}]", flush=True)
    return dict(device=torch.cuda.get_device_name(0), results=results)


def host():
    from mumpy_hip import augment as A
    mask, r = _mask(), np.random.default_rng(3)
    per_shape = {s: [] for s in A.SHAPE_LIST}
    for _ in range(4000):
        t0 = time.perf_counter()
        d = A.sample_double_full(r, SRC, L, mask)
        A.clip_warp_params(SRC, L, d)
        per_shape[d.shape].append((time.perf_counter() - t0) * 1000.0)
    results = {s: dict(n=len(v), median_ms=round(statistics.median(v), 4), p90_ms=round(float(np.percentile(v, 90)), 4), max_ms=round(max(v), 4))
               for s, v in per_shape.items()}
    everything = [x for v in per_shape.values() for x in v]
    results["all"] = dict(n=len(everything), mean_ms=round(statistics.fmean(everything), 4), median_ms=round(statistics.median(everything), 4))
    # where RandomScaleCrop's time goes at the largest side: the upscaled mask's bounding box, whole upscale against edge scans
    cm = A.canvas_mask(mask, *A.clip_tables(SRC, L, "id"))
    A.cubic_taps(L, 1024)
    box = {}
    for label, fn in (("full_upscale_ms", lambda: A.find_corners(A.upscaled_mask(cm, 1024))), ("edge_scans_ms", lambda: A.upscaled_corners(cm, 1024)),
                      ("scale_crop_params_ms", lambda: A.scale_crop_params(L, 1024, (100, 90, 900, 1000)))):
        v = []
        for _ in range(15):
            t0 = time.perf_counter()
            fn()
            v.append((time.perf_counter() - t0) * 1000.0)
        box[label] = dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
    results["S=1024"] = box
    for k, v in results.items():
        print(k, v, flush=True)
    return dict(cpu_threads=1, results=results)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "launch"
    report = dict(mode=mode, shape=dict(samples=SAMPLES, T=T, L=L, src=SRC), **{"launch": launch, "host": host}[mode]())
    out_dir = os.environ.get("MUMPY_PROFILE_OUT", os.path.join(ROOT, "profile_out"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"augment_warp_{mode}.json"), "w") as f:
        json.dump(report, f, indent=1)
