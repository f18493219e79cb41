"""Whole-video inference on the device: sliding clips, the per-frame mask bank, F1 / IoU.

The reference takes a video of N frames and produces one forgery mask per frame: it builds one clip per frame -- the frame plus its
k = T // 2 neighbours on each side, clamped at the ends (dataloaders/universaldataloader.py:41-48) --, runs each clip, keeps the
centre frame's mask, writes mask * 255 (test.py:86-111) and scores every frame with the per-image F1 / IoU of measure.py:57-62, 86-89.
Its CPU workers copy and resize every frame T times.  Here each frame is uploaded once; from there to the metric vector nothing leaves
the device, and per batch of clips the host uploads two small tables and replays one graph (`VideoPredictor`):

    clip_window_u8 (gather + resize + normalise out of the resident video) -> fused_forward -> mask_score_u8 (bank + counts)

Annotations may arrive at their own size (`VideoPredictor(gt_hw=...)`): measure.py:21-40 resizes each to 224 x 224 with Pillow's 8-bit
BILINEAR before it thresholds, and ops.resize_bilinear_u8 does that on the device, bit for bit.  `bilinear_taps` builds Pillow's
coefficient tables and `bilinear_resize` is the numpy statement of the whole resize.  Not covered: a palette image's conversion to
'L' (the caller's `.convert('L')`), RGB images, the other filters, `box=` and `reducing_gap=`.

The threshold need not be chosen before the pass: `VideoPredictor(sweep=...)` also counts, per frame, how many pixels exceed each
threshold of a table (ops.score_exceed, inside the same graph) and sums F1 / IoU per threshold (ops.sweep_metrics);
evaluate.finalize_sweep turns that into the best threshold and a pixel-level AUC.  `sweep_table` builds the table and
`exceed_counts` reads the four counts of one threshold out of the exceed rows.

The host half (`clip_frame_indices`, `batch_plan`, `bilinear_taps`, `bilinear_resize`, `sweep_table`, `exceed_counts`) imports and
runs without a GPU."""
import os

import numpy as np
import torch

from .graph import GraphedForward

SIDE = 224                       # the model's input side (inputRes of the reference's loaders)


def clip_frame_indices(nframes: int, T: int) -> np.ndarray:
    """(nframes, T) int32: row i holds clamp(j, 0, nframes - 1) for j = i - k .. i + k, k = T // 2 -- the comprehension of
    universaldataloader.py:41-46.  An even T is refused: the reference's rule yields T + 1 frames there.
    Column k of row i is i, the frame the mask belongs to: test.py names the saved file after that frame and measure.py scores it
    against that frame's annotation.  (universaldataset.py:130 returns targets[1] as the clip's annotation, which is the centre frame
    only for T = 3; this module follows measure.py.)"""
    nframes, T = int(nframes), int(T)
    if nframes < 1 or T < 1:
        raise ValueError(f"clip_frame_indices: nframes={nframes} and T={T} must be at least 1")
    if T % 2 == 0:
        raise ValueError(f"clip_frame_indices: T={T} is even; the reference's window i - T//2 .. i + T//2 holds T + 1 frames then")
    k = T // 2
    j = np.arange(nframes)[:, None] + np.arange(-k, k + 1)[None, :]
    return np.clip(j, 0, nframes - 1).astype(np.int32)


def batch_plan(nframes: int, T: int, batch: int):
    """-> (idx (nb, batch, T) int32, dest (nb, batch) int32), nb = ceil(nframes / batch): batch b runs the clips of frames
    b * batch .. ; dest is the frame each clip's mask belongs to.  The tail of the last batch is padded with copies of the last clip
    (valid indices) whose dest is -1: they write nothing and count for nothing."""
    batch = int(batch)
    if batch < 1:
        raise ValueError(f"batch_plan: batch={batch} must be at least 1")
    rows = clip_frame_indices(nframes, T)
    nb = -(-nframes // batch)
    pad = nb * batch - nframes
    idx = np.concatenate([rows, np.repeat(rows[-1:], pad, axis=0)]).reshape(nb, batch, T)
    dest = np.concatenate([np.arange(nframes, dtype=np.int32), np.full(pad, -1, np.int32)]).reshape(nb, batch)
    return np.ascontiguousarray(idx), np.ascontiguousarray(dest)


PRECISION_BITS = 22             # Pillow's 8-bit resampling: coefficients are fixed point with 22 fractional bits (Resample.c)
GT_MAX_RATIO = 32               # 2 * 32 + 1 taps = MUMPY_RESIZE_KMAX_CAP of include/mumpy_hip_ext6.h


def bilinear_taps(n_in: int, n_out: int):
    """Pillow's BILINEAR coefficients of an n_in -> n_out resize of 8-bit images, any ratio: (start (n_out,), count (n_out,),
    coef (n_out, ksize)) int32.  Output position i reads input start[i] .. start[i] + count[i] - 1; coef[i, count[i]:] is 0.
    precompute_coeffs + normalize_coeffs_8bpc restated for the triangle filter, in double and in Pillow's order: the filter is
    stretched by max(n_in / n_out, 1) (the antialiasing of a downscale), so ksize = 2 * ceil(that) + 1 grows with the ratio; the
    weights of a row are divided by their sum, then trunc(0.5 + w * 2^22).  n_in == n_out gives the identity -- coef[:, 0] = 2^22 and
    zeros --, which is what the pass Pillow skips for an unchanged side amounts to."""
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f"bilinear_taps: n_in={n_in} and n_out={n_out} must be at least 1")
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support = fs
    ksize = 2 * int(np.ceil(support)) + 1
    start, count = np.zeros(n_out, np.int32), np.zeros(n_out, np.int32)
    coef = np.zeros((n_out, ksize), np.int32)
    for i in range(n_out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) / fs)) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            coef[i, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        start[i], count[i] = xmin, xmax
    return start, count, coef


def _resample_rows(img, start, count, coef):
    """One pass of Pillow's 8-bit resample along axis 0 of img (n_in, ...) -> (len(start), ...) int64 in [0, 255]."""
    n_in = img.shape[0]
    acc = np.full((len(start),) + img.shape[1:], 1 << (PRECISION_BITS - 1), np.int64)
    tail = (1,) * (img.ndim - 1)
    for k in range(coef.shape[1]):
        c = np.where(k < count, coef[:, k], 0).astype(np.int64)
        acc += c.reshape(-1, *tail) * img[np.clip(start.astype(np.int64) + k, 0, n_in - 1)]
    return np.clip(acc >> PRECISION_BITS, 0, 255)


def bilinear_resize(img_u8, out_hw) -> np.ndarray:
    """Image.resize((w, h), Image.BILINEAR) of an 8-bit single-channel image (H, W) -- or of a stack (..., H, W) --, restated in
    integers: the horizontal pass, its result rounded to uint8, then the vertical pass; each is
    clip((2^21 + sum coef * src) >> 22, 0, 255) with the taps of `bilinear_taps`.  The numpy statement of ops.resize_bilinear_u8."""
    img = np.asarray(img_u8)
    if img.dtype != np.uint8 or img.ndim < 2:
        raise ValueError(f"bilinear_resize: needs a uint8 image (..., H, W), got {img.dtype} {img.shape}")
    oh, ow = (int(v) for v in out_hw)
    img = img.astype(np.int64)
    horiz = np.moveaxis(_resample_rows(np.moveaxis(img, -1, 0), *bilinear_taps(img.shape[-1], ow)), 0, -1)
    vert = _resample_rows(np.moveaxis(horiz, -2, 0), *bilinear_taps(img.shape[-2], oh))
    return np.ascontiguousarray(np.moveaxis(vert, 0, -2)).astype(np.uint8)


SWEEP_MAX_THRESHOLDS = 1023     # MUMPY_SWEEP_MAX_THRESHOLDS of include/mumpy_hip_ext7.h


def sweep_table(thresholds=None) -> np.ndarray:
    """The threshold table of a sweep, float32 (K,).  The default is the 255 values i / 256, i = 1 .. 255: exact in float32, and
    0.5 -- the reference's threshold (test.py:108) -- is one of them.  A caller's list is converted to float32 and refused unless it
    then holds 1 to 1023 finite, strictly ascending values (two values that collapse in float32 are refused: they would be one
    operating point listed twice)."""
    if thresholds is None:
        return (np.arange(1, 256, dtype=np.float32) / np.float32(256.0)).astype(np.float32)
    with np.errstate(over="ignore"):
        t = np.asarray(thresholds, dtype=np.float64).astype(np.float32)
    if t.ndim != 1 or not 1 <= t.size <= SWEEP_MAX_THRESHOLDS:
        raise ValueError(f"sweep_table: needs a list of 1 to {SWEEP_MAX_THRESHOLDS} thresholds, got shape {t.shape}")
    if not np.isfinite(t).all():
        raise ValueError("sweep_table: every threshold must be finite in float32")
    if not (np.diff(t) > 0).all():
        raise ValueError("sweep_table: the thresholds must be strictly ascending after the conversion to float32")
    return np.ascontiguousarray(t)


def exceed_counts(exceed, k: int):
    """The (n, 4) counts {inter, sum p, sum g, union} of threshold k out of exceed (n, 2, K + 1) as ops.score_exceed writes it --
    what ops.mask_score_u8 counts from the mask at thr = table[k], and what ops.frame_metrics / the metric formulas take.  Works
    on a numpy array (-> int64) and on a tensor (-> int32, on its device)."""
    if exceed.ndim != 3 or exceed.shape[1] != 2 or exceed.shape[2] < 2:
        raise ValueError(f"exceed_counts: needs exceed of shape (n, 2, K + 1), got {tuple(exceed.shape)}")
    last = exceed.shape[2] - 1
    k = int(k)
    if not 0 <= k < last:
        raise ValueError(f"exceed_counts: k={k} is outside the table's 0 .. {last - 1}")
    on_device = isinstance(exceed, torch.Tensor)
    e = exceed.to(torch.int64) if on_device else np.asarray(exceed).astype(np.int64)
    inter, sp, sg = e[:, 1, k], e[:, 0, k] + e[:, 1, k], e[:, 1, last]
    cols = [inter, sp, sg, sp + sg - inter]
    return torch.stack(cols, 1).to(torch.int32).contiguous() if on_device else np.stack(cols, 1)


class VideoPredictor(GraphedForward):
    """One forgery mask per frame of a video, and the F1 / IoU sums over its frames, without leaving the device.

        vp = VideoPredictor(encoder, decoder, T=3, src_hw=(240, 432))
        masks = vp.predict(frames_u8, gt_u8)            # (N, 224, 224) uint8, values 0 / 255, on the device
        f1, iou, n = evaluate.finalize_metrics(vp.metric_vector())

    gt_hw=(Hg, Wg): predict takes the annotations at their own size and resizes them on the device as measure.py does (see predict);
    gt_hw=None (the default) takes them at 224 x 224 and launches nothing more.

    sweep=True (the 255 thresholds of `sweep_table()`) or a list of thresholds: the predictor also owns the table on the device,
    exceed (max_frames, 2, K + 1) int32, sweep_acc (K, 3) float64 and sweep_pooled (2, K + 1) int64; the captured forward ends with
    ops.score_exceed(logits, gt, dest, table, exceed), and a predict with gt_u8 ends with ops.sweep_metrics(..., accumulate=True)
    beside frame_metrics.  `sweep_vector()` is what evaluate.finalize_sweep takes.  thr, the masks, the bank, counts and the metric
    vector are not affected; sweep=None (the default) allocates nothing and captures exactly the three steps below.

    It owns the frame bank (max_frames, Hs, Ws, 3), the index table (batch, T) and dest table (batch,), the clip batch
    (batch, T, 3, 224, 224), the mask and annotation banks (max_frames, 224 * 224), the counts bank (max_frames, 4), the accumulator
    of 3 doubles, and pinned host staging for the two tables.  With graph=True ONE graph is captured per predictor, holding
    ops.clip_window_u8 into the clip batch, pipeline.fused_forward(..., with_mask=True) and ops.mask_score_u8; warm-up, capture
    stream and the re-capture after a weight change are GraphedForward's.  Per batch the host uploads the two tables and replays.
    graph=False issues the same three steps eagerly.

    The reference's own test.py saves only clip 0 of each batch, so it works at batch size 1 only; this class returns every frame's
    mask at any `batch`.  As in the reference, the forward couples the clips of one batch (SwinDAttention pairs windows across the
    batch, see mumpy_hip/distributed.py): what comes out at `batch` = B is the model run at batch size B on these clips in this
    order, the padding clips of the tail (copies of the last clip) included, and the GEMM kernels are chosen by the batch's row
    count -- so results at different `batch` values are not bit for bit the same.

    coupling="batch" (the default) is that behaviour: the same launches and the same bits as before the option existed.
    coupling="clip" runs every forward, eager or captured, under ops.clip_coupling_as("clip"): the cross-view attention pairs
    windows inside each clip (the grouped kernels of include/mumpy_hip_ext8.h on the full batch), so every clip is computed as the
    reference's batch-size-1 test.py computes it.  A frame's mask then depends neither on `batch`, nor on which clips share its
    batch or in what order, nor on the tail's padding clips -- up to the fp32 rounding of the GEMM routes, which are still chosen
    by the batch's row count (logits agree to ~1e-6 relative, not bit for bit).  The predictor sets the switch around its own
    forwards only and leaves the global ops.clip_coupling() as it found it.

    perturb=("jpeg", q), ("blur", r) or a list of those, applied in order: every predict first runs that post-processing once, in
    place, on the uploaded video at its own size (ops.jpeg_roundtrip_u8 / ops.gaussian_blur_u8: Pillow's save(format="JPEG",
    quality=q) + re-open and ImageFilter.GaussianBlur(r), bit for bit), before the first batch -- what an unperturbed predictor
    computes when it is fed the frames Pillow processed on the host.  A robustness table is
    `for q in (90, 70, 50): VideoPredictor(..., perturb=("jpeg", q)).predict(frames, gt)`.  The nine photometric kinds of
    mumpy_hip.photometric -- ("contrast", 1.4), ("equalize", None), ... -- may stand anywhere in the list, mixed with the two
    (ops.photometric_u8: Pillow's ImageOps / ImageEnhance, bit for bit, statistics per frame).  The predictor owns the tables and a
    workspace of perturb_chunk frames; a bad spec is refused here.  perturb=None (the default) allocates nothing and launches
    nothing: the captured graph, the masks, the bank, the counts and the metric vector are what they were without the option.

    clean=dict(min_area=..., max_hole=..., connectivity=8): after the last batch of a predict, ONE launch (ops.mask_clean_u8,
    include/mumpy_postprocess.h) removes every connected component below min_area pixels from each frame's mask and then fills every
    hole of up to max_hole pixels (max_hole < 0: every hole; mumpy_hip.postprocess.clean is the numpy statement), bank[:n] ->
    clean_bank[:n], and predict returns the cleaned masks.  The predictor then also owns clean_bank (max_frames, 224 * 224) uint8,
    clean_counts (max_frames, 4), clean_stats (max_frames, 8), clean_acc (3,) float64, the parameter rows and the workspace; with
    annotations one more ops.frame_metrics sums the cleaned masks' F1 / IoU into clean_acc (`metric_vector(clean=True)`), and
    `clean_statistics()` is the (n, 8) table of mumpy_hip.postprocess.STATS.  bank, counts, metric_vector() and the sweep stay the
    raw ones, bit for bit.  A bad setting is refused here; clean=None (the default) allocates nothing and launches nothing.  Not
    covered: cleaned masks per threshold of a sweep, filtering across frames."""

    def __init__(self, encoder, decoder, T, src_hw, batch=8, max_frames=1024, thr=0.5, graph=True, gt_hw=None, gt_chunk=64,
                 sweep=None, coupling="batch", perturb=None, perturb_chunk=64, clean=None):
        from .perturb import check_spec, jpeg_tables
        from .postprocess import check_spec as check_clean
        clean = check_clean(clean, "VideoPredictor: clean", (SIDE, SIDE))      # refuses a bad setting
        if coupling not in ("batch", "clip"):
            raise ValueError(f"VideoPredictor: coupling must be \"batch\" or \"clip\", got {coupling!r}")
        steps = check_spec(perturb, "VideoPredictor: perturb")      # refuses a bad spec
        if steps and int(perturb_chunk) < 1:
            raise ValueError(f"VideoPredictor: perturb_chunk={perturb_chunk} must be at least 1")
        T, batch, max_frames = int(T), int(batch), int(max_frames)
        clip_frame_indices(1, T)                                     # refuses an even T
        model_t = int(encoder.configs[-1]["num_frames"])
        if T != model_t:
            raise ValueError(f"VideoPredictor: T={T}, but the encoder was built for clips of {model_t} frames")
        if batch < 1 or max_frames < 1:
            raise ValueError(f"VideoPredictor: batch={batch} and max_frames={max_frames} must be at least 1")
        hs, ws = (int(v) for v in src_hw)
        self.gt_hw = None if gt_hw is None else tuple(int(v) for v in gt_hw)
        self.gt_chunk = int(gt_chunk)
        if self.gt_hw is not None and (len(self.gt_hw) != 2 or min(self.gt_hw) < 1 or self.gt_chunk < 1):
            raise ValueError(f"VideoPredictor: gt_hw={gt_hw} must be (Hg, Wg) with both at least 1, and gt_chunk={gt_chunk} at least 1")
        if self.gt_hw is not None and max(self.gt_hw) > GT_MAX_RATIO * SIDE:
            raise ValueError(f"VideoPredictor: gt_hw={gt_hw} is more than {GT_MAX_RATIO} times {SIDE} (the resize kernel's tap cap)")
        if sweep is not None and not isinstance(sweep, bool) and isinstance(sweep, (str, bytes, int, float)):
            raise ValueError(f"VideoPredictor: sweep={sweep!r} must be None, True or a list of thresholds")
        table = None if sweep is None or sweep is False else sweep_table(None if sweep is True else sweep)    # refuses a bad list
        dev = next(encoder.parameters()).device
        if dev.type != "cuda":
            raise RuntimeError("VideoPredictor: the model is not on a GPU (there is no CPU path)")
        self.T, self.batch, self.max_frames, self.src_hw, self.thr, self.graphed = T, batch, max_frames, (hs, ws), float(thr), bool(graph)
        npix = SIDE * SIDE
        nb = -(-max_frames // batch)
        self.frames = torch.zeros(max_frames, hs, ws, 3, device=dev, dtype=torch.uint8)
        self.idx = torch.zeros(batch, T, device=dev, dtype=torch.int32)
        self.dest = torch.full((batch,), -1, device=dev, dtype=torch.int32)          # the warm-up runs write nothing
        self.bank = torch.zeros(max_frames, npix, device=dev, dtype=torch.uint8)
        self.gt = torch.zeros(max_frames, npix, device=dev, dtype=torch.uint8)
        self.counts = torch.zeros(max_frames, 4, device=dev, dtype=torch.int32)
        self.acc = torch.zeros(3, device=dev, dtype=torch.float64)
        self._idx_host = torch.zeros(nb, batch, T, dtype=torch.int32).pin_memory()   # a whole video's plan: no slot is reused while
        self._dest_host = torch.zeros(nb, batch, dtype=torch.int32).pin_memory()     # an upload out of it may still be in flight
        self._uploaded = None
        # sweep: the table (uploaded once), the per-frame exceed counts and the two accumulators; nothing of it exists without
        self.table = self.exceed = self.sweep_acc = self.sweep_pooled = None
        if table is not None:
            k = len(table)
            self.table = torch.from_numpy(table).to(dev)
            self.exceed = torch.zeros(max_frames, 2, k + 1, device=dev, dtype=torch.int32)
            self.sweep_acc = torch.zeros(k, 3, device=dev, dtype=torch.float64)
            self.sweep_pooled = torch.zeros(2, k + 1, device=dev, dtype=torch.int64)
        # annotations that arrive from the host at their own size pass through this, gt_chunk frames at a time (1080p annotations
        # of a whole video would cost max_frames * Hg * Wg bytes)
        self._gt_stage = None if self.gt_hw is None else \
            torch.zeros(min(self.gt_chunk, max_frames), *self.gt_hw, device=dev, dtype=torch.uint8)
        if self.gt_hw is not None:
            from . import ops
            ops._bilinear_tables(*self.gt_hw, SIDE, SIDE, dev)      # uploaded here, not in the first predict
        # perturb: per step its device-side setting (one table pair, or one box row per frame of a chunk), and one workspace
        self.perturb, self._perturb_ws = [], None
        if steps:
            from . import ops
            chunk = min(int(perturb_chunk), max_frames)
            lib, need = ops._lib(), [16]
            for kind, value in steps:
                if kind == "jpeg":
                    need.append(int(lib.mumpy_jpeg_roundtrip_workspace_bytes(chunk, hs, ws)))
                    self.perturb.append((kind, value, ops.jpeg_tables_u16(jpeg_tables(value)[None], dev),
                                         torch.zeros(chunk, device=dev, dtype=torch.int32)))
                elif kind == "blur":
                    need.append(int(lib.mumpy_gaussian_blur_workspace_bytes(chunk, hs, ws)))
                    self.perturb.append((kind, value, ops.blur_params(value, chunk, dev), None))
                else:                                                # a photometric kind: one row per frame of a chunk
                    need.append(int(lib.mumpy_photometric_workspace_bytes(chunk, hs, ws)))
                    self.perturb.append((kind, value, ops.photometric_params((kind, value), chunk, dev), None))
            if min(need) < 0:
                raise ValueError(f"VideoPredictor: perturb: frames of {hs}x{ws} are refused: {lib.mumpy_last_error().decode()}")
            self._perturb_ws = torch.empty(max(need), device=dev, dtype=torch.uint8)
            self._perturb_chunk = chunk
        # clean: the cleaned bank with its counts, statistics and accumulator, the rows and the workspace; nothing of it exists without
        self.clean = clean
        if clean is not None:
            from . import ops
            self.clean_bank = torch.zeros(max_frames, npix, device=dev, dtype=torch.uint8)
            self.clean_counts = torch.zeros(max_frames, 4, device=dev, dtype=torch.int32)
            self.clean_stats = torch.zeros(max_frames, 8, device=dev, dtype=torch.int32)
            self.clean_acc = torch.zeros(3, device=dev, dtype=torch.float64)
            self._clean_params = ops.mask_clean_params(clean, max_frames, dev)
            self._clean_ws = ops.mask_clean_workspace(max_frames, SIDE, SIDE, dev)
            self._clean_n = 0
        clips = torch.zeros(batch, T, 3, SIDE, SIDE, device=dev, dtype=torch.float32)
        if self.graphed:
            super().__init__(encoder, decoder, clips, with_mask=True, coupling=coupling)     # static_x is the clip batch
        else:
            self.encoder, self.decoder, self.with_mask, self.static_x, self.coupling = encoder, decoder, True, clips, coupling

    def _fwd(self):
        from . import ops
        from .pipeline import fused_forward
        ops.clip_window_u8(self.frames, self.idx, (SIDE, SIDE), out=self.static_x)
        with ops.clip_coupling_as(self.coupling):                    # eager, warm-up and capture alike; restored on the way out
            logits, mask, feats = fused_forward(self.encoder, self.decoder, self.static_x, with_mask=True, thr=self.thr)
        ops.mask_score_u8(mask, self.dest, self.bank, gt=self.gt, counts=self.counts)
        if self.table is not None:
            ops.score_exceed(logits, self.gt, self.dest, self.table, self.exceed)
        return logits, mask, feats

    def __call__(self, frames_u8, gt_u8=None):
        return self.predict(frames_u8, gt_u8)

    def _run_batch(self):
        if not self.graphed:
            with torch.no_grad():
                return self._fwd()
        if self._stale():
            self._capture()
        self.graph.replay()
        return self.static_out

    @staticmethod
    def _u8(t, name, shape):
        t = torch.as_tensor(t)
        if t.dtype != torch.uint8 or tuple(t.shape) != tuple(shape):
            raise ValueError(f"VideoPredictor.predict: {name} must be uint8 of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}")
        return t

    def predict(self, frames_u8, gt_u8=None, on_batch=None):
        """frames_u8 (N, Hs, Ws, 3) uint8, on the host or the device, 1 <= N <= max_frames (N need not be a multiple of `batch`)
        -> masks (N, 224, 224) uint8 with values 0 / 255 on the device: a view of the bank (of clean_bank in a predictor built with
        clean=: the cleaned masks), valid until the next call.
        gt_u8 (N, 224, 224) uint8 (> 0 counts as forged), already resized by the caller -- or, in a predictor built with
        gt_hw=(Hg, Wg), (N, Hg, Wg) uint8 at the annotations' own size, on the host or the device, holding the bytes
        Image.open(...).convert('L') gives: measure.py's Image.resize((224, 224), BILINEAR) then runs on the device, bit for bit
        (ops.resize_bilinear_u8), before the first batch.  The frame metrics of the N frames are added into the accumulator
        (`metric_vector`).
        on_batch(b, logits, mask): called after batch b was issued, with the forward's static output buffers (logits (batch, 1, 224,
        224) float32 and the 0 / 1 mask) -- the next batch overwrites them.
        Everything is checked before anything is launched."""
        from . import ops
        frames_u8 = torch.as_tensor(frames_u8)
        if frames_u8.dim() != 4 or frames_u8.shape[0] == 0:
            raise ValueError(f"VideoPredictor.predict: frames must be (N, Hs, Ws, 3) with N >= 1, got {tuple(frames_u8.shape)}")
        n = frames_u8.shape[0]
        if n > self.max_frames:
            raise ValueError(f"VideoPredictor.predict: {n} frames, but the banks hold max_frames={self.max_frames}")
        frames_u8 = self._u8(frames_u8, "frames", (n, *self.src_hw, 3))
        if gt_u8 is not None:
            gt_u8 = self._u8(gt_u8, "gt", (n, *(self.gt_hw or (SIDE, SIDE))))
            if self.gt_hw is not None and gt_u8.is_cuda and not gt_u8.is_contiguous():
                raise ValueError("VideoPredictor.predict: gt on the device must be contiguous (it is resized where it is, never copied)")
        idx, dest = batch_plan(n, self.T, self.batch)
        nb = idx.shape[0]
        if self._uploaded is not None:
            self._uploaded.synchronize()                             # the last video's uploads have left the staging
        self._idx_host[:nb].copy_(torch.from_numpy(idx))
        self._dest_host[:nb].copy_(torch.from_numpy(dest))
        self.frames[:n].copy_(frames_u8, non_blocking=True)
        if self.perturb:
            self._perturb_frames(n)
        if gt_u8 is not None and self.gt_hw is None:
            self.gt[:n].copy_(gt_u8.reshape(n, SIDE * SIDE), non_blocking=True)
        elif gt_u8 is not None:
            self._resize_gt(gt_u8, n)
        for b in range(nb):
            self.idx.copy_(self._idx_host[b], non_blocking=True)
            self.dest.copy_(self._dest_host[b], non_blocking=True)
            out = self._run_batch()
            if on_batch is not None:
                on_batch(b, out[0], out[1])
        self._uploaded = torch.cuda.Event()
        self._uploaded.record()
        if gt_u8 is not None:
            ops.frame_metrics(self.counts, n, SIDE * SIDE, acc=self.acc, accumulate=True)
            if self.table is not None:
                ops.sweep_metrics(self.exceed, n, SIDE * SIDE, acc=self.sweep_acc, pooled=self.sweep_pooled, accumulate=True)
        if self.clean is not None:
            scored = gt_u8 is not None
            ops.mask_clean_u8(self.bank[:n], self._clean_params[:n], out=self.clean_bank[:n], gt=self.gt[:n] if scored else None,
                              counts=self.clean_counts[:n] if scored else None, stats=self.clean_stats[:n], workspace=self._clean_ws,
                              hw=(SIDE, SIDE))
            if scored:
                ops.frame_metrics(self.clean_counts, n, SIDE * SIDE, acc=self.clean_acc, accumulate=True)
            self._clean_n = n
            return self.clean_bank[:n].view(n, SIDE, SIDE)
        return self.bank[:n].view(n, SIDE, SIDE)

    def _perturb_frames(self, n):
        """frames[:n] through every step of `perturb`, in place, issued on the current stream ahead of the first batch, one pair of
        launches per step and chunk of perturb_chunk frames (the workspace holds one chunk)."""
        from . import ops
        for kind, _, setting, sel in self.perturb:
            for i in range(0, n, self._perturb_chunk):
                part = self.frames[i:min(i + self._perturb_chunk, n)]
                m = part.shape[0]
                if kind == "jpeg":
                    ops.jpeg_roundtrip_u8(part, setting, sel=sel[:m], out=part, workspace=self._perturb_ws)
                elif kind == "blur":
                    ops.gaussian_blur_u8(part, setting[:m], out=part, workspace=self._perturb_ws)
                else:
                    ops.photometric_u8(part, setting[:m], out=part, workspace=self._perturb_ws)

    def _resize_gt(self, gt_u8, n):
        """gt[:n] = Image.resize((224, 224), BILINEAR) of the annotations (ops.resize_bilinear_u8), issued on the current stream ahead
        of the first batch: a device tensor straight from the caller's memory, a host tensor through the staging buffer, one upload
        and one launch per gt_chunk frames (stream order keeps a chunk's upload behind the launch that read the one before)."""
        from . import ops
        bank = self.gt[:n].view(n, SIDE, SIDE)
        if gt_u8.is_cuda:
            ops.resize_bilinear_u8(gt_u8, (SIDE, SIDE), out=bank)
            return
        step = self._gt_stage.shape[0]
        for i in range(0, n, step):
            m = min(step, n - i)
            self._gt_stage[:m].copy_(gt_u8[i:i + m], non_blocking=True)
            ops.resize_bilinear_u8(self._gt_stage[:m], (SIDE, SIDE), out=bank[i:i + m])

    def metric_vector(self, clean=False) -> torch.Tensor:
        """The device [sum F1, sum IoU, n] over every frame scored since the last reset: what evaluate.finalize_metrics takes.
        clean=True: the same sums of the cleaned masks (only in a predictor built with clean=)."""
        if clean and self.clean is None:
            raise RuntimeError("VideoPredictor.metric_vector: this predictor was built without clean=")
        return self.clean_acc if clean else self.acc

    def clean_statistics(self) -> torch.Tensor:
        """(n, 8) int32 on the device, a view: per frame of the last predict the columns of mumpy_hip.postprocess.STATS -- components
        found, kept, pixels removed, holes filled, pixels filled, the largest kept component, 0, status (0).  Only with clean=."""
        if self.clean is None:
            raise RuntimeError("VideoPredictor.clean_statistics: this predictor was built without clean=")
        return self.clean_stats[:self._clean_n]

    def sweep_vector(self):
        """(table (K,) float32, sweep_acc (K, 3) float64, sweep_pooled (2, K + 1) int64) on the device: the thresholds, per threshold
        [sum F1, sum IoU, n] and the pooled exceed counts over every frame scored since the last reset -- what
        evaluate.finalize_sweep takes.  Only in a predictor built with sweep=."""
        if self.table is None:
            raise RuntimeError("VideoPredictor.sweep_vector: this predictor was built without sweep=")
        return self.table, self.sweep_acc, self.sweep_pooled

    def reset_metrics(self) -> None:
        self.acc.zero_()
        if self.clean is not None:
            self.clean_acc.zero_()
        if self.table is not None:
            self.sweep_acc.zero_()
            self.sweep_pooled.zero_()

    def write_masks(self, dirname, frame_numbers, clean=None) -> None:
        """Saves the masks of the last predict as '%04d_instance_%02d.png' % (frame_number, 0) (test.py:109-111), one per entry of
        frame_numbers.  The one place that copies masks to the host.  clean=None saves the cleaned masks when the predictor was built
        with clean= and the raw ones otherwise; clean=False the raw ones; clean=True needs a predictor built with clean=."""
        if clean and self.clean is None:
            raise RuntimeError("VideoPredictor.write_masks: this predictor was built without clean=")
        bank = self.clean_bank if (self.clean is not None and clean is not False) else self.bank
        from PIL import Image
        frame_numbers = [int(f) for f in frame_numbers]
        if not 1 <= len(frame_numbers) <= self.max_frames:
            raise ValueError(f"VideoPredictor.write_masks: {len(frame_numbers)} frame numbers for banks of {self.max_frames} frames")
        masks = bank[:len(frame_numbers)].view(-1, SIDE, SIDE).cpu().numpy()
        os.makedirs(dirname, exist_ok=True)
        for f, m in zip(frame_numbers, masks):
            Image.fromarray(m).save(os.path.join(dirname, "%04d_instance_%02d.png" % (f, 0)))
