"""Measurements behind profiles/augment_input.md.

    python tools/augment_input_profile.py launch     # GPU: time per launch of the input stage against the eval staging kernels
    python tools/augment_input_profile.py host       # CPU: per-clip host time of a PIL restatement of the reference's loader path
                                                     #      against clip_tables + staging the uint8 bytes; H2D bytes per step

launch: nclips = 6, T = 5, L = 224 from 224 x 224 and 240 x 432 sources.  Every variant is captured as a graph of 100 back-to-back
launches; a sample is 10 replays between two events; the variants alternate (order reversed every round) in one process, 4 warm-up
rounds, 25 timed ones; median and range over the rounds, in microseconds per launch.
host: a sample is one training sample of 3 sequences x T = 5 frames + the centre mask, already decoded (decoding is out of scope)."""
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "multilateral-temporal-view-pyramid-transformer-for-video-inpainting-detection_amd"))
NCLIPS, T, L = 6, 5, 224
SOURCES = ((224, 224), (240, 432))
BOX = (30, 17, 201, 190)


def launch():
    import torch
    from mumpy_hip import augment as A, ops
    dev = torch.device("cuda:0")
    reps, rounds, warm = 100, 25, 4
    lib = ops._lib()
    m3, s3 = (ctypes.c_float * 3)(*ops.EVAL_MEAN), (ctypes.c_float * 3)(*ops.EVAL_STD)
    results = {}
    for hs, ws in SOURCES:
        g = np.random.default_rng(hs)
        frames = torch.from_numpy(g.integers(0, 256, (NCLIPS, T, hs, ws, 3), dtype=np.uint8)).to(dev)
        masks = torch.from_numpy(g.integers(0, 2, (2, hs, ws), dtype=np.uint8)).to(dev)
        out, target = torch.empty(NCLIPS, T, 3, L, L, device=dev), torch.empty(NCLIPS, L * L, device=dev)
        ytab, xtab = ops._nearest_table(hs, L, dev), ops._nearest_table(ws, L, dev)

        def stage(op, box, with_masks=False):
            p = [A.clip_tables((hs, ws), L, op if isinstance(op, str) else op[k % len(op)], box) for k in range(NCLIPS)]
            ta, tb, sw = (torch.from_numpy(np.stack([np.asarray(q[k]) for q in p]).astype(np.int32)).to(dev) for k in range(3))
            return lambda: ops.augment_stage_u8(frames, ta, tb, sw, masks=masks if with_masks else None, out=out,
                                                target=target if with_masks else None)

        def eval_resize():
            assert lib.mumpy_resize_normalize_u8_fwd(frames.data_ptr(), out.data_ptr(), ytab.data_ptr(), xtab.data_ptr(), NCLIPS * T, hs, ws,
                                                     L, L, m3, s3, torch.cuda.current_stream().cuda_stream) == 0

        variants = {"eval resize_normalize_u8": eval_resize, "(a) identity": stage("id", None), "(b) hflip + crop": stage("hflip", BOX),
                    "(c) rot90": stage("rot90", None), "(c) rot90 + crop": stage("rot90", BOX),
                    "id / rot90 / hflip / rot270 by clip": stage(("id", "rot90", "hflip", "rot270"), None),
                    "(a) identity, with masks": stage("id", None, True), "(c) rot90, with masks": stage("rot90", None, True)}
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
        results[f"{hs}x{ws}"] = {n: dict(median_us=round(statistics.median(v), 3), min_us=round(min(v), 3), max_us=round(max(v), 3))
                                 for n, v in times.items()}
        for n, r in results[f"{hs}x{ws}"].items():
            print(f"{hs}x{ws}  {n:40s} median {r['median_us']:7.3f} us   [{r['min_us']:.3f} .. {r['max_us']:.3f}]", flush=True)
    return dict(device=torch.cuda.get_device_name(0), results=results)


def host():
    import torch
    from PIL import Image, ImageOps
    from mumpy_hip import augment as A, ops
    import warnings
    warnings.filterwarnings("ignore", message="The given NumPy array is not writable")          # np.asarray(PIL image), as the loader passes it
    torch.set_num_threads(1)                                    # one DataLoader worker
    mean, std = torch.tensor(ops.EVAL_MEAN).view(3, 1, 1), torch.tensor(ops.EVAL_STD).view(3, 1, 1)

    def transform(arr):                                         # ToTensor + Normalize
        return (torch.from_numpy(arr).permute(2, 0, 1).float().div(255.0) - mean) / std

    def pil_sample(imgs, annot, op, box):
        """universaldataset.py:66-120 after decoding: the un-augmented branch the loader always runs, then the augmented one."""
        origin = [im.resize((L, L), Image.NEAREST) for im in imgs]
        origin_annot = annot.resize((L, L), Image.NEAREST)
        plain = [transform(np.array(im.resize((L, L), Image.NEAREST))) for im in imgs]
        aug = [op(im) for im in origin + [origin_annot]]
        if box is not None:
            aug = [im.crop(box) for im in aug]
        res = [transform(np.asarray(im.resize((L, L), Image.NEAREST))) for im in aug[:-1]]
        m = np.asarray(aug[-1].resize((L, L), Image.NEAREST)).copy()
        m[m > 0] = 1
        return torch.stack(res[:T]), torch.stack(res[T:2 * T]), torch.stack(res[2 * T:]), torch.from_numpy(m.astype(np.float32).reshape(1, -1)), plain

    results = {}
    for hs, ws in SOURCES:
        g = np.random.default_rng(ws)
        frames = g.integers(0, 256, (3, T, hs, ws, 3), dtype=np.uint8)
        mask = g.integers(0, 2, (hs, ws), dtype=np.uint8) * 255
        imgs, annot = [Image.fromarray(f) for f in frames.reshape(-1, hs, ws, 3)], Image.fromarray(mask)
        stage_f, stage_m = np.empty_like(frames), np.empty_like(mask)
        cases = {"identity": (lambda im: im, "id", None), "hflip + crop": (ImageOps.mirror, "hflip", BOX),
                 "rot90": (lambda im: im.rotate(90, expand=True), "rot90", None)}
        res = {}
        for name, (pil_op, op, box) in cases.items():
            def ours():
                t = A.clip_tables((hs, ws), L, op, box)         # one draw per sample: the three clips share the tables
                np.copyto(stage_f, frames)
                np.copyto(stage_m, mask)
                return t
            row = {}
            for label, fn in (("pil_ms_per_clip", lambda: pil_sample(imgs, annot, pil_op, box)), ("tables_and_staging_ms_per_clip", ours)):
                fn()
                v = []
                for _ in range(15):
                    t0 = time.perf_counter()
                    fn()
                    v.append((time.perf_counter() - t0) * 1000.0 / 3)          # 3 clips per sample
                row[label] = dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
            res[name] = row
            print(f"{hs}x{ws}  {name:14s} PIL path {row['pil_ms_per_clip']['median']:8.3f} ms/clip [{row['pil_ms_per_clip']['min']:.3f} .. "
                  f"{row['pil_ms_per_clip']['max']:.3f}]   tables + uint8 staging {row['tables_and_staging_ms_per_clip']['median']:7.4f} ms/clip "
                  f"[{row['tables_and_staging_ms_per_clip']['min']:.4f} .. {row['tables_and_staging_ms_per_clip']['max']:.4f}]", flush=True)
        b = 2                                                    # samples per step: 6 clips
        res["h2d_bytes_per_step"] = dict(fp32_clips_and_targets=b * (3 * T * 3 * L * L * 4 + L * L * 4),
                                         uint8_frames_masks_tables=b * (3 * T * hs * ws * 3 + hs * ws) + 3 * b * (2 * L + 1) * 4)
        print(f"{hs}x{ws}  H2D bytes per step (2 samples): {res['h2d_bytes_per_step']}", flush=True)
        results[f"{hs}x{ws}"] = res
    return dict(cpu_threads=1, results=results)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "launch"
    report = dict(mode=mode, shape=dict(nclips=NCLIPS, T=T, L=L), **{"launch": launch, "host": host}[mode]())
    out_dir = os.environ.get("MUMPY_PROFILE_OUT", os.path.join(ROOT, "profile_out"))
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"augment_input_{mode}.json"), "w") as f:
        json.dump(report, f, indent=1)
