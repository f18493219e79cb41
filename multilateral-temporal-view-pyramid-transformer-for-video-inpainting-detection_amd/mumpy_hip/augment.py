"""The training input stage on the device: uint8 clips in, augmented + normalized fp32 clips and 0/1 targets out.

The reference loads a training sample on CPU workers (universaldataset.py:55-120): every frame is resized with PIL (NEAREST under the
pinned pillow==4.0.0), one augmentation is drawn per sample and applied to every frame and to the centre mask
(utils/randaugment.py), everything is resized to the input size again, turned into float tensors and normalized, and the target is
`mask > 0` (universaldataset.py:141-144).  The augmentations the reference has switched on are exact index permutations:

  * Identity, HFlip, VFlip and PsccAug (90-degree rotations, optionally followed by a top-bottom flip): the dihedral group D4 of the
    square L x L canvas;
  * RandomCrop / OriginalRandomCrop (the Double strategy): a crop box of the transformed canvas, resized back to L x L (NEAREST).

With out[y, x] = canvas[u, v] every such pipeline folds into two index tables of L entries and one swap bit per clip (`clip_tables`),
and the whole stage is one gather launch with the arithmetic of ops.normalize_u8 (`ops.augment_stage_u8`,
mumpy_augment_stage_u8_fwd of include/mumpy_hip_ext3.h).  RandomRotate (a bilinear warp) and RandomScaleCrop (a CUBIC resize)
interpolate and are not expressible this way: asking for them raises.

This module is host code (numpy + the library's host helper mumpy_resize_nearest_table) and imports without a GPU; only
AugmentedInput touches the device.  The samplers follow the reference's distributions, not its RNG stream."""
import collections
import ctypes
import functools

import numpy as np

# op -> (swap, reverse u, reverse v) with out[y, x] = canvas[u, v]; u walks y (x when swapped), v walks x (y when swapped)
OPS = {
    "id": (0, 0, 0),            # Identity, PsccAug 0
    "hflip": (0, 0, 1),         # HFlip (ImageOps.mirror), PsccAug 6 (rotate 180 + top-bottom flip)
    "vflip": (0, 1, 0),         # VFlip (ImageOps.flip), PsccAug 4
    "rot90": (1, 0, 1),         # PsccAug 1: rotate(90, expand=True), counter-clockwise
    "rot180": (0, 1, 1),        # PsccAug 2
    "rot270": (1, 1, 0),        # PsccAug 3
    "rot90+tb": (1, 0, 0),      # PsccAug 5: the transpose
    "rot270+tb": (1, 1, 1),     # PsccAug 7: the anti-transpose; the reference never draws it (np.random.randint(0, 7))
}
PSCC_OPS = ("id", "rot90", "rot180", "rot270", "vflip", "rot90+tb", "hflip", "rot270+tb")
# augment_list() (randaugment.py:542-576): seven equally likely entries under OneAugmentStrategy
SINGLE_LIST = ("id", "id", "id", "id", "hflip", "vflip", "pscc")
# none_shape_change_augment_list() / shape_change_augment_list() (randaugment.py:579-613): the Double strategy draws one of each
DOUBLE_LIST = ("hflip", "vflip", "pscc")
SHAPE_LIST = ("RandomCrop", "RandomRotate", "OriginalRandomCrop", "RandomScaleCrop")
FOLDABLE_SHAPE_OPS = ("RandomCrop", "OriginalRandomCrop")

Draw = collections.namedtuple("Draw", "entry pscc op")          # list entry 0..6, PsccAug index (None unless entry is PsccAug), op name


@functools.lru_cache(maxsize=4096)
def _nearest(src: int, dst: int):
    """Pillow's NEAREST source indices of a src -> dst resize: the library's host helper (its double-accumulator walk decides ties)."""
    from .lib import load_library
    lib = load_library()
    host = (ctypes.c_int32 * dst)()
    rc = lib.mumpy_resize_nearest_table(src, dst, host)
    if rc:
        raise RuntimeError(f"mumpy_resize_nearest_table failed ({rc}): {lib.mumpy_last_error().decode()}")
    t = np.frombuffer(host, dtype=np.int32).copy()
    t.setflags(write=False)
    return t


def nearest_table(src: int, dst: int) -> np.ndarray:
    return _nearest(int(src), int(dst))


def check_box(box, L):
    l, t, r, b = (int(v) for v in box)
    if not (0 <= l < r <= L and 0 <= t < b <= L):
        raise ValueError(f"augment: crop box {tuple(box)} must satisfy 0 <= l < r <= {L} and 0 <= t < b <= {L}")
    return l, t, r, b


def clip_tables(src_hw, L, op="id", box=None):
    """(tab_a, tab_b, swap) of one clip: int32 tables of L entries for
        source (Hs, Ws) --NEAREST--> L x L canvas --op (D4)--> [--crop box=(l, t, r, b)--NEAREST--> L x L]
    so that out[y, x] = source[tab_a[y], tab_b[x]] (swap 0) or source[tab_a[x], tab_b[y]] (swap 1)."""
    hs, ws = (int(v) for v in src_hw)
    L = int(L)
    if op not in OPS:
        raise ValueError(f"augment: unknown operation {op!r}; one of {sorted(OPS)}")
    if hs < 1 or ws < 1 or L < 1:
        raise ValueError(f"augment: bad sizes {hs}x{ws} -> {L}")
    ry, rx = nearest_table(hs, L), nearest_table(ws, L)
    if box is None:
        cy = cx = np.arange(L, dtype=np.int64)
    else:
        l, t, r, b = check_box(box, L)
        cy, cx = t + nearest_table(b - t, L).astype(np.int64), l + nearest_table(r - l, L).astype(np.int64)
    swap, rev_u, rev_v = OPS[op]
    pu, pv = (cx, cy) if swap else (cy, cx)
    u = L - 1 - pu if rev_u else pu
    v = L - 1 - pv if rev_v else pv
    return np.ascontiguousarray(ry[u], dtype=np.int32), np.ascontiguousarray(rx[v], dtype=np.int32), np.int32(swap)


def gather(img, tab_a, tab_b, swap, channels_last=False):
    """The host statement of what the kernel reads: img (..., Hs, Ws) or, channels_last, (..., Hs, Ws, C) -> (..., L, L[, C]) with
    the kernel's clamp and its reading of the swap word (bit 0)."""
    img = np.asarray(img)
    hs, ws = img.shape[-3:-1] if channels_last else img.shape[-2:]
    a = np.clip(np.asarray(tab_a, dtype=np.int64), 0, hs - 1)
    b = np.clip(np.asarray(tab_b, dtype=np.int64), 0, ws - 1)
    rows, cols = (a[None, :], b[:, None]) if int(swap) & 1 else (a[:, None], b[None, :])
    return img[..., rows, cols, :] if channels_last else img[..., rows, cols]


def canvas_mask(mask_u8, tab_a, tab_b, swap):
    """The mask as the crop operations see it: resized to the canvas and D4-transformed -- the gather of the host mask (Hs, Ws) through
    the tables of `clip_tables(src_hw, L, op)` (no box)."""
    return gather(mask_u8, tab_a, tab_b, swap)


# ------------------------------------------------------------------------------------------------ the reference's draws
def sample_single(rng) -> Draw:
    """OneAugmentStrategy over augment_list(): one of seven entries, four of them Identity; PsccAug then draws its index from 0..6."""
    entry = int(rng.integers(0, len(SINGLE_LIST)))
    if SINGLE_LIST[entry] != "pscc":
        return Draw(entry, None, SINGLE_LIST[entry])
    k = int(rng.integers(0, 7))
    return Draw(entry, k, PSCC_OPS[k])


def find_corners(mask):
    """FindCorners (randaugment.py:194-202): None for an empty mask, else (left - 1, top - 1, right + 1, bottom + 1) of the bounding
    box of the non-zero pixels."""
    mask = np.asarray(mask)
    rows, cols = np.flatnonzero(mask.any(axis=1)), np.flatnonzero(mask.any(axis=0))
    if rows.size == 0 or cols.size == 0:
        return None
    return int(cols[0]) - 1, int(rows[0]) - 1, int(cols[-1]) + 1, int(rows[-1]) + 1


def original_random_crop_box(v, L, rng):
    """OriginalRandomCrop (randaugment.py:263-288): a square of side int(v), placed by its top-left corner, by its bottom-right corner
    (which then stays off the last row / column) or centred, each with probability 1/3."""
    size, L = int(v), int(L)
    if not 1 <= size <= L - 1:
        raise ValueError(f"augment: crop side {size} must lie in [1, {L - 1}]")
    how = int(rng.integers(0, 3))
    if how == 0:
        l, t = int(rng.integers(0, L - size + 1)), int(rng.integers(0, L - size + 1))
    elif how == 1:
        l, t = int(rng.integers(size, L)) - size, int(rng.integers(size, L)) - size
    else:
        l = t = (L - size) // 2
    return check_box((l, t, l + size, t + size), L)


def random_crop_box(cmask, v, L, rng):
    """RandomCrop (randaugment.py:291-309) on the canvas mask: a box around the mask's bounding box, each side drawn uniformly between
    the canvas edge and the (one pixel widened) bounding box; OriginalRandomCrop when the mask is empty.  As in the reference the right
    / bottom side is exclusive and never beyond L - 1, so a mask that touches the last column / row loses that column / row."""
    L = int(L)
    corners = find_corners(cmask)
    if corners is None:
        return original_random_crop_box(v, L, rng)
    left, top, right, bottom = corners
    l = int(rng.integers(0, left - 1)) if left > 1 else 0
    r = int(rng.integers(right + 1, L - 1)) if right + 1 < L - 1 else L - 1
    t = int(rng.integers(0, top - 1)) if top > 1 else 0
    b = int(rng.integers(bottom + 1, L - 1)) if bottom + 1 < L - 1 else L - 1
    return check_box((l, t, r, b), L)


def sample_double(rng, src_hw, L, mask_u8=None, shape_ops=None, v_range=(20.0, 220.0)):
    """DoubleAugmentStrategy: one of HFlip / VFlip / PsccAug, then one shape operation with v ~ U(v_range) -> (op, box).
    The reference's shape list holds RandomRotate and RandomScaleCrop, which interpolate; the whole list (shape_ops=None) is therefore
    refused, and the caller restricts it to a subset of ("RandomCrop", "OriginalRandomCrop").  mask_u8: the host mask (Hs, Ws) RandomCrop
    looks at (None: an empty mask)."""
    if shape_ops is None or not set(shape_ops) <= set(FOLDABLE_SHAPE_OPS) or not shape_ops:
        bad = sorted(set(SHAPE_LIST if shape_ops is None else shape_ops) - set(FOLDABLE_SHAPE_OPS))
        raise NotImplementedError(
            f"augment: the Double strategy's shape operations {bad} are interpolating warps (RandomRotate: a bilinear rotation, "
            f"RandomScaleCrop: a CUBIC resize) and do not fold into index tables; pass shape_ops restricted to {FOLDABLE_SHAPE_OPS}")
    first = DOUBLE_LIST[int(rng.integers(0, len(DOUBLE_LIST)))]
    op = PSCC_OPS[int(rng.integers(0, 7))] if first == "pscc" else first
    shape = tuple(shape_ops)[int(rng.integers(0, len(shape_ops)))]
    v = float(rng.uniform(*v_range))
    if shape == "OriginalRandomCrop":
        return op, original_random_crop_box(v, L, rng)
    hs, ws = src_hw
    cm = np.zeros((L, L), np.uint8) if mask_u8 is None else canvas_mask(mask_u8, *clip_tables((hs, ws), L, op))
    return op, random_crop_box(cm, v, L, rng)


# ------------------------------------------------------------------------------------------------ the device side
class AugmentedInput:
    """Fills the clip tensor `x` (B, T, 3, L, L) and the `target` tensor (B * L * L elements) of a training step in place from uint8
    frames, e.g. GraphedTrainStep.x / .target:

        inp = AugmentedInput(step.x, step.target, src_hw=(240, 432), nmasks=2)
        inp.load(frames_u8, masks_u8, [clip_tables((240, 432), 224, op, box) for op, box in draws]);  loss3 = step.step()-style replay

    frames_u8 (B, T, Hs, Ws, 3) and masks_u8 (nmasks, Hs, Ws) are uint8, on the host or on the device; clip b reads mask b % nmasks
    (the reference's cat([masks] * 3) over the sequences of a sample).  params: one (tab_a, tab_b, swap) per clip, or the three
    stacked arrays.  The object owns pinned host staging (two sets, used alternately) and the device buffers for frames, masks,
    tables and swap words; load() allocates nothing, uploads with non_blocking=True and launches once on the current stream.  The
    only wait is the host's, for the upload issued two loads earlier from the same staging set -- long finished in a training loop.
    The tables live in device memory, so a captured launch (`launch()`) replays with the parameters uploaded last."""

    def __init__(self, x, target, src_hw, nmasks=None, mean=None, std=None):
        import torch
        from . import ops
        if not x.is_cuda or x.dtype != torch.float32 or x.dim() != 5 or x.shape[2] != 3 or x.shape[3] != x.shape[4] or not x.is_contiguous():
            raise RuntimeError("AugmentedInput: x must be a contiguous float32 GPU tensor (B, T, 3, L, L)")
        b, t, _, L, _ = x.shape
        hs, ws = (int(v) for v in src_hw)
        if target is not None:
            if not target.is_cuda or target.dtype != torch.float32 or not target.is_contiguous() or target.numel() != b * L * L:
                raise RuntimeError(f"AugmentedInput: target must be a contiguous float32 GPU tensor of {b} x {L * L} elements")
            if nmasks is None or nmasks < 1 or b % nmasks:
                raise ValueError(f"AugmentedInput: nmasks={nmasks} must divide the {b} clips")
        self.x, self.target, self.src_hw, self.L, self.nclips, self.T = x, target, (hs, ws), L, b, t
        self.nmasks = int(nmasks) if target is not None else 0
        self.mean, self.std = ops.EVAL_MEAN if mean is None else mean, ops.EVAL_STD if std is None else std
        dev, u8, i32 = x.device, torch.uint8, torch.int32
        self.frames = torch.empty(b, t, hs, ws, 3, dtype=u8, device=dev)
        self.masks = torch.empty(self.nmasks, hs, ws, dtype=u8, device=dev) if target is not None else None
        self.params = torch.empty(2 * b * L + b, dtype=i32, device=dev)          # [tab_a | tab_b | swap]: one upload
        self.tab_a, self.tab_b, self.swap = self.params[:b * L].view(b, L), self.params[b * L:2 * b * L].view(b, L), self.params[2 * b * L:]
        self._stage = [dict(frames=torch.empty(b, t, hs, ws, 3, dtype=u8).pin_memory(),
                            masks=torch.empty(self.nmasks, hs, ws, dtype=u8).pin_memory() if target is not None else None,
                            params=torch.empty(2 * b * L + b, dtype=i32).pin_memory(), done=torch.cuda.Event()) for _ in range(2)]
        self._turn = 0

    def _upload(self, dst, src, pinned, what):
        import torch
        src = torch.as_tensor(src)
        if src.dtype != dst.dtype or tuple(src.shape) != tuple(dst.shape):
            raise RuntimeError(f"AugmentedInput.load: {what} must be {dst.dtype} of shape {tuple(dst.shape)}, got {src.dtype} {tuple(src.shape)}")
        if src.is_cuda:
            dst.copy_(src, non_blocking=True)
        else:
            pinned.copy_(src)
            dst.copy_(pinned, non_blocking=True)

    def load(self, frames_u8, masks_u8, params):
        import torch
        b, L = self.nclips, self.L
        st = self._stage[self._turn]
        self._turn ^= 1
        st["done"].synchronize()                 # host-side only: the upload of two loads ago has left this staging set
        if len(params) == 3 and hasattr(params[0], "ndim") and params[0].ndim == 2:          # the three stacked arrays
            ta, tb, sw = params
        else:                                                                                 # one (tab_a, tab_b, swap) per clip
            ta, tb, sw = (np.stack([np.asarray(p[k]) for p in params]) for k in range(3))
        ta, tb, sw = np.asarray(ta), np.asarray(tb), np.asarray(sw)
        if ta.shape != (b, L) or tb.shape != (b, L) or sw.shape != (b,):
            raise RuntimeError(f"AugmentedInput.load: the tables must be ({b}, {L}) and the swap words ({b},), got {ta.shape}, {tb.shape}, {sw.shape}")
        host = st["params"].numpy()
        host[:b * L], host[b * L:2 * b * L], host[2 * b * L:] = ta.reshape(-1), tb.reshape(-1), sw
        self.params.copy_(st["params"], non_blocking=True)
        self._upload(self.frames, frames_u8, st["frames"], "frames")
        if self.target is not None:
            if masks_u8 is None:
                raise RuntimeError("AugmentedInput.load: this input was built with a target and needs masks")
            self._upload(self.masks, masks_u8, st["masks"], "masks")
        elif masks_u8 is not None:
            raise RuntimeError("AugmentedInput.load: this input was built without a target and takes no masks")
        st["done"].record()
        self.launch()

    def launch(self):
        """The one kernel launch on the current stream, reading the device-resident parameters (capturable)."""
        from . import ops
        ops.augment_stage_u8(self.frames, self.tab_a, self.tab_b, self.swap, masks=self.masks, out=self.x,
                             target=None if self.target is None else self.target.view(self.nclips, self.L * self.L),
                             mean=self.mean, std=self.std)
