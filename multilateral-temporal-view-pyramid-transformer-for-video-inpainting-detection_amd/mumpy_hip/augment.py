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
interpolate and are not expressible this way: `sample_double` refuses them.  They run as modes 2 and 1 of a second kernel that
interpolates on the canvas those tables describe (`ops.augment_warp_u8`, mumpy_augment_warp_u8_fwd of include/mumpy_hip_ext4.h):
`sample_double_full` draws from the whole list, `clip_warp_params` builds the kernel's rows, AugmentedInput(warp=True) runs them.
RandomScaleCrop is Pillow's 8-bit BICUBIC restated in integers, bit for bit; RandomRotate is a plain fp32 bilinear warp, not
cv2.warpAffine's fixed-point one -- how far the two differ is not measured.

The affine group of the same file (ShearX .. Rotate) and Cutout, which the reference lists beside those and keeps commented out, move
the mask with the frames and are not index tables of this kind either (a shear has no per-axis table, a rotation by 17 degrees no
swap bit): they run before this stage, on the canvas, as mumpy_hip.geometric / ops.geometric_u8 (include/mumpy_geometric.h) behind
AugmentedInput(perturb=True, geometric=True), bit for bit Pillow's fixed-point walk.

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


# ------------------------------------------------------------------------------------------------ the interpolating operations
# RandomScaleCrop and RandomRotate do not permute pixels; they run on the device as modes 1 and 2 of mumpy_augment_warp_u8_fwd
# (include/mumpy_hip_ext4.h), which reads the L x L canvas through the tables of clip_tables and interpolates on it.  The rows below
# are that kernel's per-clip parameters.
MODE_GATHER, MODE_CUBIC, MODE_AFFINE = 0, 1, 2
PRECISION_BITS = 22                    # Pillow's 8-bit resample: coefficients in 22-bit fixed point, each pass clip8((2^21 + sum) >> 22)

WarpParams = collections.namedtuple("WarpParams", "tab_a tab_b swap mode pos_y pos_x coef_y coef_x affine")
# op: the D4 operation drawn first; shape: the entry of SHAPE_LIST; box: the crop box on the canvas (the crops) or on the S x S upscale
# (RandomScaleCrop; None: no box); S, angle: RandomScaleCrop's side, RandomRotate's angle (None otherwise)
FullDraw = collections.namedtuple("FullDraw", "op shape box S angle")


@functools.lru_cache(maxsize=4096)
def _cubic(n_in: int, n_out: int):
    if n_in < 1 or n_out < n_in:
        raise ValueError(f"augment: cubic_taps restates Pillow's BICUBIC for n_out >= n_in >= 1 only (4 taps), got {n_in} -> {n_out}")
    scale = float(n_in) / n_out                          # <= 1: the filter is not widened, its support stays 2
    a = -0.5
    center = (np.arange(n_out, dtype=np.float64) + 0.5) * scale
    lo = np.maximum(np.trunc(center - 2.0 + 0.5), 0.0)
    hi = np.minimum(np.trunc(center + 2.0 + 0.5), float(n_in))
    assert (hi - lo <= 4.0).all()
    pos = lo[:, None] + np.arange(4.0)
    x = np.abs(pos - center[:, None] + 0.5)
    w = np.where(x < 1.0, ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0, np.where(x < 2.0, (((x - 5.0) * x + 8.0) * x - 4.0) * a, 0.0))
    w = np.where(pos < hi[:, None], w, 0.0)                # the taps Pillow drops at the right / bottom edge
    ww = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]        # Pillow's own order of summation
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    start = lo.astype(np.int32)
    coef = np.trunc(np.where(w < 0.0, -0.5, 0.5) + w * (1 << PRECISION_BITS)).astype(np.int32)
    start.setflags(write=False)
    coef.setflags(write=False)
    return start, coef


def cubic_taps(n_in, n_out):
    """Pillow's BICUBIC coefficients of an n_in -> n_out resize of 8-bit images, n_out >= n_in: (start (n_out,), coef (n_out, 4)) int32.
    Output position i reads input start[i] .. start[i] + 3; a tap Pillow drops at an edge is a zero coefficient.  Centre
    (i + 0.5) * n_in / n_out, support 2, a = -0.5, weights normalised in double, then trunc(+-0.5 + w * 2^22)."""
    return _cubic(int(n_in), int(n_out))


def _clip8(acc):
    return np.clip((acc + (1 << (PRECISION_BITS - 1))) >> PRECISION_BITS, 0, 255)


def _resample_rows(img, start, coef):
    """One pass of Pillow's 8-bit resample along axis 0 of img (n_in, ...) integer -> (len(start), ...) int64 in [0, 255]."""
    n_in = img.shape[0]
    acc = np.zeros((len(start),) + img.shape[1:], np.int64)
    tail = (1,) * (img.ndim - 1)
    for k in range(4):
        acc += coef[:, k].astype(np.int64).reshape(-1, *tail) * img[np.clip(start.astype(np.int64) + k, 0, n_in - 1)]
    return _clip8(acc)


def cubic_resize(img, out_hw):
    """Image.resize(BICUBIC) of an 8-bit image (H, W[, C]) to out_hw >= (H, W), restated: the horizontal pass, then the vertical."""
    img = np.asarray(img).astype(np.int64)
    oh, ow = (int(v) for v in out_hw)
    horiz = np.moveaxis(_resample_rows(np.moveaxis(img, 1, 0), *cubic_taps(img.shape[1], ow)), 0, 1)
    return _resample_rows(horiz, *cubic_taps(img.shape[0], oh)).astype(np.uint8)


def upscaled_mask(cmask, S):
    """The canvas mask (L, L) as RandomScaleCrop's CornerCrop sees it: resized to S x S with CUBIC, in the kernel's integer arithmetic."""
    return cubic_resize(cmask, (S, S))


def _upscaled_part(cmask, S, ys, xs):
    """upscaled_mask(cmask, S)[ys][:, xs] without forming the rest."""
    cm = np.asarray(cmask).astype(np.int64)
    L = cm.shape[0]
    start, coef = cubic_taps(L, S)
    rows = np.unique(np.clip(start[ys].astype(np.int64)[:, None] + np.arange(4), 0, L - 1))            # the canvas rows these ys read
    horiz = np.zeros((L, len(xs)), np.int64)
    horiz[rows] = np.moveaxis(_resample_rows(np.moveaxis(cm[rows], 1, 0), start[xs], coef[xs]), 0, 1)
    return _resample_rows(horiz, start[ys], coef[ys])


def upscaled_corners(cmask, S, chunk=8):
    """find_corners(upscaled_mask(cmask, S)) from row and column "any" tests: rows and columns of the upscale are formed a few at a
    time from each side of the region the mask's bounding box can reach, until one holds a positive pixel."""
    cm = np.asarray(cmask)
    rows, cols = np.flatnonzero(cm.any(axis=1)), np.flatnonzero(cm.any(axis=0))
    if rows.size == 0:
        return None
    start, _ = cubic_taps(cm.shape[0], S)
    reach = lambda lo, hi: np.flatnonzero((start + 3 >= lo) & (start <= hi))          # upscale positions with a tap in [lo, hi]
    ys, xs = reach(rows[0], rows[-1]), reach(cols[0], cols[-1])

    def first(cand, axis):
        for k in range(0, len(cand), chunk):
            c = cand[k:k + chunk]
            hit = (_upscaled_part(cm, S, c, xs) if axis == 0 else _upscaled_part(cm, S, ys, c)).any(axis=1 - axis)
            if hit.any():
                return int(c[np.flatnonzero(hit)[0]])
        return None
    top = first(ys, 0)
    if top is None:
        return None
    return first(xs, 1) - 1, top - 1, first(xs[::-1], 1) + 1, first(ys[::-1], 0) + 1


def corner_crop_box(up_mask, rng):
    """CornerCrop (randaugment.py:377-395) on the S x S upscaled mask: random_crop_box's draw with side S; None for an empty mask
    (the reference then keeps the upscale whole)."""
    return _corner_box(find_corners(up_mask), np.shape(up_mask)[0], rng)


def _corner_box(corners, S, rng):
    if corners is None:
        return None
    left, top, right, bottom = corners
    S = int(S)
    l = int(rng.integers(0, left - 1)) if left > 1 else 0
    r = int(rng.integers(right + 1, S - 1)) if right + 1 < S - 1 else S - 1
    t = int(rng.integers(0, top - 1)) if top > 1 else 0
    b = int(rng.integers(bottom + 1, S - 1)) if bottom + 1 < S - 1 else S - 1
    return check_box((l, t, r, b), S)


def scale_crop_params(L, S, box=None):
    """The mode-1 rows (pos_y, coef_y, pos_x, coef_x) of RandomScaleCrop on an L x L canvas: CUBIC to S x S, CornerCrop's box
    (l, t, r, b) of the upscale resized back to S x S with NEAREST (None: no crop), the loader's NEAREST to L x L.  The two NEAREST
    steps pick rows ty = t + near(b - t -> S)[near(S -> L)] of the upscale (columns alike), whose taps are the rows returned."""
    L, S = int(L), int(S)
    start, coef = cubic_taps(L, S)
    back = nearest_table(S, L).astype(np.int64)
    if box is None:
        ty = tx = back
    else:
        l, t, r, b = check_box(box, S)
        ty, tx = t + nearest_table(b - t, S).astype(np.int64)[back], l + nearest_table(r - l, S).astype(np.int64)[back]
    return start[ty].copy(), coef[ty].copy(), start[tx].copy(), coef[tx].copy()


def rotate_params(L, angle):
    """The mode-2 rows (pos_y, pos_x, affine) of RandomRotate (randaugment.py:434-474) by an integer angle in degrees: affine maps
    the rotated image's pixel (u, w) to the canvas about c = L / 2,
        sx = cos(u - c) - sin(w - c) + c,    sy = sin(u - c) + cos(w - c) + c       (the inverse of cv2.getRotationMatrix2D's map),
    and pos_* pick the centre crop of side int(crop_mult * L) resized back to L with NEAREST.  The crop angle is the angle folded
    into [0, 90] degrees; for 0 .. 179 that is the reference's own expression, which leaves that range for larger angles."""
    L, angle = int(L), int(angle)
    th = np.deg2rad(float(angle % 360))
    al, be, c = np.cos(th), np.sin(th), L / 2
    fold = angle % 180
    tc = np.deg2rad(float(180 - fold if fold > 90 else fold))
    crop_mult = (np.cos(tc) + np.sin(tc) * np.tan(tc)) / (np.tan(tc) + 1.0)
    side = int(crop_mult * L)
    if not 1 <= side <= L:
        raise ValueError(f"augment: rotation by {angle} degrees leaves a crop of side {side} of {L}")
    pos = (int((L - side) / 2) + nearest_table(side, L)).astype(np.int32)
    affine = np.array([al, -be, c - al * c + be * c, be, al, c - be * c - al * c, 0.0, 0.0], np.float32)
    return pos, pos.copy(), affine


def sample_double_full(rng, src_hw, L, mask_u8, base_size=512, v_range=(20.0, 220.0)):
    """DoubleAugmentStrategy with its whole shape list: one of HFlip / VFlip / PsccAug, then one of RandomCrop, RandomRotate,
    OriginalRandomCrop, RandomScaleCrop with equal probability and v ~ U(v_range) -> FullDraw, which clip_warp_params turns into the
    kernel's rows.  RandomRotate takes int(v) degrees; 180, where the reference's crop has no extent, is drawn again.  RandomScaleCrop
    draws its side uniformly in [base_size // 2, 2 * base_size] and its box from the upscaled mask.  mask_u8: the host mask (Hs, Ws)
    the crops look at (None: an empty mask)."""
    first = DOUBLE_LIST[int(rng.integers(0, len(DOUBLE_LIST)))]
    op = PSCC_OPS[int(rng.integers(0, 7))] if first == "pscc" else first
    shape = SHAPE_LIST[int(rng.integers(0, len(SHAPE_LIST)))]
    v = float(rng.uniform(*v_range))
    if shape == "RandomRotate":
        while int(v) == 180:
            v = float(rng.uniform(*v_range))
        return FullDraw(op, shape, None, None, int(v))
    if shape == "OriginalRandomCrop":
        return FullDraw(op, shape, original_random_crop_box(v, L, rng), None, None)
    cm = np.zeros((L, L), np.uint8) if mask_u8 is None else canvas_mask(mask_u8, *clip_tables(src_hw, L, op))
    if shape == "RandomCrop":
        return FullDraw(op, shape, random_crop_box(cm, v, L, rng), None, None)
    S = int(rng.integers(base_size // 2, 2 * base_size + 1))
    if S < L:
        raise ValueError(f"augment: RandomScaleCrop drew side {S} below the canvas side {L}; the downscaling cubic is not restated")
    return FullDraw(op, shape, _corner_box(upscaled_corners(cm, S), S, rng), S, None)


def clip_warp_params(src_hw, L, draw) -> WarpParams:
    """The per-clip arrays of mumpy_augment_warp_u8_fwd for a FullDraw; one record serves every clip of the sample."""
    L = int(L)
    zl, zc, za = np.zeros(L, np.int32), np.zeros((L, 4), np.int32), np.zeros(8, np.float32)
    if draw.shape == "RandomScaleCrop":
        py, cy, px, cx = scale_crop_params(L, draw.S, draw.box)
        return WarpParams(*clip_tables(src_hw, L, draw.op), np.int32(MODE_CUBIC), py, px, cy, cx, za)
    if draw.shape == "RandomRotate":
        py, px, aff = rotate_params(L, draw.angle)
        return WarpParams(*clip_tables(src_hw, L, draw.op), np.int32(MODE_AFFINE), py, px, zc, zc, aff)
    if draw.shape not in FOLDABLE_SHAPE_OPS:
        raise ValueError(f"augment: unknown shape operation {draw.shape!r}")
    return WarpParams(*clip_tables(src_hw, L, draw.op, draw.box), np.int32(MODE_GATHER), zl, zl, zc, zc, za)


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
    The tables live in device memory, so a captured launch (`launch()`) replays with the parameters uploaded last.
    warp=True: the launch is ops.augment_warp_u8, the parameter block holds every array of that call (still one upload), and a clip's
    entry of params is either such a triple (a gather) or the WarpParams of clip_warp_params.
    perturb=True: ordinary post-processing as an augmentation (mumpy_hip.perturb; the reference's JPEGCompression and
    RandomGaussianBlur act on the frame after its first img.resize(inputRes), universaldataset.py:67).  The object additionally owns
    the canvas (B, T, L, L, 3) uint8 and the mask canvas (nmasks, L, L), one quantisation-table pair per clip, the per-frame table
    choice and box rows -- all in the one parameter block, still one upload -- and the kernels' workspace; launch() becomes
    ops.resize_nearest_u8 source -> canvas (frames and masks), ops.jpeg_roundtrip_u8 and ops.gaussian_blur_u8 in place on the canvas,
    then the stage above reading the canvas: all of it capturable.  The per-clip tables are then CANVAS-relative --
    clip_tables((L, L), L, op, box), clip_warp_params((L, L), L, draw) -- because the object does the source -> canvas resize itself.
    load(..., perturb=[None | ("jpeg", q) | ("blur", r) per clip]): all T frames of a clip share the clip's setting; masks are never
    perturbed.  perturb=False (the default) is the object as it was: the same buffers, the same single launch.
    photometric=True (needs perturb=True): the nine photometric kinds of mumpy_hip.photometric as well -- one {kind, value, 0, 0} row
    per frame more in the parameter block (still one upload) and one more in-place launch on the canvas after the blur
    (ops.photometric_u8); load(perturb=[...]) then also takes ("contrast", 1.4), ("equalize", None), ... per clip.  Statistics are per
    frame, as Pillow's are per image.  photometric=False (the default) is the object as it was: the same block, the same launches.
    geometric=True (needs perturb=True): the affine kinds and Cutout of mumpy_hip.geometric as well, the first operations that move
    the MASK with the frames.  The object additionally owns a second frame canvas and a second mask canvas (a gather cannot run in
    place), one {mode, a0 .. a5, 0} row per frame and one per mask more in the parameter block (still one upload); after the
    photometric launch (after the blur without one) launch() runs ops.geometric_u8 canvas -> second canvas, the same on the mask canvas
    with channels=1, and the final stage reads the second canvases.  load(perturb=[...]) then also takes ("shear_x", 0.2),
    ("rotate", -30), ... per clip: all T frames and the clip's mask share the clip's matrix, so clips that share a mask (b % nmasks)
    must carry the same affine setting.  ("cutout", v) fills the rectangles of mumpy_hip.geometric.cutout_rects in the frames and
    leaves the mask alone; their placement reads the canvas mask on the host (`canvas_mask`), so the masks must arrive on the host,
    and load(..., rng=) supplies the generator.  geometric=False (the default) is the object as it was."""

    def __init__(self, x, target, src_hw, nmasks=None, mean=None, std=None, warp=False, perturb=False, photometric=False,
                 geometric=False):
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
        # one parameter block, one upload: [tab_a | tab_b | swap], or with warp every array of mumpy_augment_warp_u8_fwd -- the ones
        # loaded 16 bytes at a time first (L % 4 == 0 keeps each of them aligned), affine as the bits of its float32
        self.warp = bool(warp)
        shapes = dict(tab_a=(b, L), tab_b=(b, L), pos_y=(b, L), pos_x=(b, L), coef_y=(b, L, 4), coef_x=(b, L, 4), affine=(b, 8), swap=(b,),
                      mode=(b,))
        self._fields = tuple(shapes) if self.warp else ("tab_a", "tab_b", "swap")
        self.perturb, self.photometric, self.geometric = bool(perturb), bool(photometric), bool(geometric)
        if self.photometric and not self.perturb:
            raise ValueError("AugmentedInput: photometric=True needs perturb=True (the operations act on the canvas)")
        if self.geometric and not self.perturb:
            raise ValueError("AugmentedInput: geometric=True needs perturb=True (the operations act on the canvas)")
        if self.perturb:
            # qtab: (b, 2, 64) uint16 = 64 words per clip; blur: {r, ww, fw, on} per frame; sel: the clip's table or -1 per frame.
            # qtab and blur are loaded 16 bytes at a time: they go in front of the first one-word-per-clip array
            shapes.update(qtab=(b, 64), blur=(b * t, 4), sel=(b * t,))
            at = self._fields.index("swap")
            self._fields = self._fields[:at] + ("qtab", "blur") + self._fields[at:] + ("sel",)
        if self.photometric:                                          # {kind, value, 0, 0} per frame, loaded 16 bytes at a time too
            shapes.update(photo=(b * t, 4))
            at = self._fields.index("swap")
            self._fields = self._fields[:at] + ("photo",) + self._fields[at:]
        if self.geometric:                                            # {mode, a0 .. a5, 0} per frame and per mask, 16 bytes at a time
            shapes.update(geo=(b * t, 8), geo_mask=(self.nmasks, 8))
            at = self._fields.index("swap")
            self._fields = self._fields[:at] + ("geo", "geo_mask") + self._fields[at:]
        self._where, n = {}, 0
        for name in self._fields:
            self._where[name] = (n, n + int(np.prod(shapes[name])), shapes[name])
            n += int(np.prod(shapes[name]))
        self.params = torch.empty(n, dtype=i32, device=dev)
        for name, (lo, hi, shape) in self._where.items():
            view = self.params[lo:hi]
            setattr(self, name, (view.view(torch.float32) if name == "affine" else view).view(shape))
        self._stage = [dict(frames=torch.empty(b, t, hs, ws, 3, dtype=u8).pin_memory(),
                            masks=torch.empty(self.nmasks, hs, ws, dtype=u8).pin_memory() if target is not None else None,
                            params=torch.empty(n, dtype=i32).pin_memory(), done=torch.cuda.Event()) for _ in range(2)]
        self._turn = 0
        if self.perturb:
            self.qtab = self.qtab.view(torch.int16).view(b, 2, 64)         # the bits of the kernel's uint16
            self.canvas = torch.empty(b, t, L, L, 3, dtype=u8, device=dev)
            self.mask_canvas = torch.empty(self.nmasks, L, L, dtype=u8, device=dev) if target is not None else None
            lib = ops._lib()
            need = [int(lib.mumpy_jpeg_roundtrip_workspace_bytes(b * t, L, L)), int(lib.mumpy_gaussian_blur_workspace_bytes(b * t, L, L))]
            if self.photometric:
                need.append(int(lib.mumpy_photometric_workspace_bytes(b * t, L, L)))
            if min(need) < 0:
                raise RuntimeError(f"AugmentedInput: a canvas of {L}x{L} is refused: {lib.mumpy_last_error().decode()}")
            self._perturb_ws = torch.empty(max(need), dtype=u8, device=dev)
            if self.geometric:
                self.canvas2 = torch.empty_like(self.canvas)
                self.mask_canvas2 = torch.empty_like(self.mask_canvas) if target is not None else None
            ops._nearest_table(hs, L, dev), ops._nearest_table(ws, L, dev)  # uploaded here, not inside a capture

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

    def _perturb_rows(self, perturb, masks_u8=None, rng=None):
        """-> (qtab (b, 64) words, blur (b * T, 4), sel (b * T,), photo (b * T, 4), geo (b * T, 8), geo_mask (nmasks, 8)) int32 of one
        setting per clip (None: the clip passes through)."""
        from . import geometric as G
        from .perturb import box_params, check_spec, jpeg_tables
        from .photometric import params_row
        b, t = self.nclips, self.T
        perturb = [None] * b if perturb is None else list(perturb)
        if len(perturb) != b:
            raise ValueError(f"AugmentedInput.load: perturb needs one entry per clip ({b}), got {len(perturb)}")
        qtab = np.ones((b, 2, 64), np.uint16)
        blur = np.tile(np.array([0, 1 << 24, 0, 0], np.int64), (b, t, 1))
        sel = np.full((b, t), -1, np.int32)
        photo = np.zeros((b, t, 4), np.int32)
        geo, geo_mask = np.zeros((b, t, 8), np.int32), np.zeros((self.nmasks, 8), np.int32)
        moved = {}                                                    # mask -> (the first clip that reads it, its affine setting)
        for c, spec in enumerate(perturb):
            steps = check_spec(spec, "AugmentedInput.load: perturb", geometric=self.geometric)
            if len(steps) > 1:
                raise ValueError("AugmentedInput.load: one setting per clip, (\"jpeg\", q) or (\"blur\", r), not a list")
            for kind, value in steps:
                if kind == "jpeg":
                    qtab[c], sel[c] = jpeg_tables(value), c
                elif kind == "blur":
                    blur[c] = box_params(value)
                elif kind == "cutout":
                    geo[c] = self._cutout_rows(c, value, masks_u8, rng)
                elif kind in G.AFFINE_KINDS:
                    geo[c] = G.params_row(kind, value, (self.L, self.L))
                elif not self.photometric:
                    raise ValueError(f"AugmentedInput.load: perturb: ({kind!r}, ...) needs an input built with photometric=True")
                else:
                    photo[c] = params_row(kind, value)
            if self.geometric and self.nmasks:                        # the mask moves with the frames: one matrix per mask
                affine = steps[0] if steps and steps[0][0] in G.AFFINE_KINDS else None
                first, other = moved.setdefault(c % self.nmasks, (c, affine))
                if other != affine:
                    raise ValueError(f"AugmentedInput.load: perturb: clips {first} and {c} share mask {c % self.nmasks} and must carry the "
                                     f"same affine setting, got {other!r} and {affine!r}")
                geo_mask[c % self.nmasks] = geo[c, 0] if affine else 0
        return (qtab.reshape(b, 128).view(np.int32), blur.astype(np.int32).reshape(b * t, 4), sel.reshape(b * t), photo.reshape(b * t, 4),
                geo.reshape(b * t, 8), geo_mask)

    def _cutout_rows(self, c, v, masks_u8, rng):
        """The T rows of clip c for ("cutout", v): the reference's rectangles on the canvas, placed against the clip's canvas mask."""
        import torch
        from . import geometric as G
        if self.target is None or masks_u8 is None:
            raise ValueError("AugmentedInput.load: perturb: (\"cutout\", v) places its rectangles against the mask and needs an input "
                             "built with a target")
        if isinstance(masks_u8, torch.Tensor) and masks_u8.is_cuda:
            raise ValueError("AugmentedInput.load: perturb: (\"cutout\", v) reads the mask on the host to place its rectangles; pass "
                             "masks_u8 as a host array, not a device tensor")
        if rng is None:
            raise ValueError("AugmentedInput.load: perturb: (\"cutout\", v) draws its rectangles and needs rng= (a numpy Generator)")
        mask = np.asarray(masks_u8)[c % self.nmasks]
        if mask.shape != self.src_hw:
            raise RuntimeError(f"AugmentedInput.load: masks must be ({self.nmasks}, {self.src_hw[0]}, {self.src_hw[1]}), got "
                               f"{np.asarray(masks_u8).shape}")
        L = self.L
        cmask = canvas_mask(mask, nearest_table(self.src_hw[0], L), nearest_table(self.src_hw[1], L), 0)
        rects = G.cutout_rects(cmask, v, self.T, rng)
        rows = np.zeros((self.T, 8), np.int32)
        for k, r in enumerate(rects):
            rows[k] = G.params_row("cutout", r, (L, L))
        return rows

    def load(self, frames_u8, masks_u8, params, perturb=None, rng=None):
        import torch
        b, L = self.nclips, self.L
        if perturb is not None and not self.perturb:
            raise RuntimeError("AugmentedInput.load: perturb= needs an input built with perturb=True")
        extra = dict(zip(("qtab", "blur", "sel", "photo", "geo", "geo_mask"), self._perturb_rows(perturb, masks_u8, rng))) if self.perturb else {}
        if not self.photometric:
            extra.pop("photo", None)
        if not self.geometric:
            extra.pop("geo", None), extra.pop("geo_mask", None)
        st = self._stage[self._turn]
        self._turn ^= 1
        st["done"].synchronize()                 # host-side only: the upload of two loads ago has left this staging set
        if len(params) == 3 and hasattr(params[0], "ndim") and params[0].ndim == 2:          # the three stacked arrays
            cols = dict(zip(("tab_a", "tab_b", "swap"), (np.asarray(p) for p in params)))
        else:                                                          # one (tab_a, tab_b, swap) or, with warp, one WarpParams per clip
            if any(len(p) != 3 for p in params) and not self.warp:
                raise RuntimeError("AugmentedInput.load: a WarpParams record needs an input built with warp=True")
            fields = WarpParams._fields if any(len(p) != 3 for p in params) else ("tab_a", "tab_b", "swap")
            gather0 = (np.int32(MODE_GATHER), np.zeros(L, np.int32), np.zeros(L, np.int32), np.zeros((L, 4), np.int32),
                       np.zeros((L, 4), np.int32), np.zeros(8, np.float32))
            rows = [tuple(p) + gather0 if len(p) == 3 and len(fields) != 3 else p for p in params]
            cols = {name: np.stack([np.asarray(r[k]) for r in rows]) for k, name in enumerate(fields)}
        cols.update(extra)
        ta, tb, sw = cols["tab_a"], cols["tab_b"], cols["swap"]
        if ta.shape != (b, L) or tb.shape != (b, L) or sw.shape != (b,):
            raise RuntimeError(f"AugmentedInput.load: the tables must be ({b}, {L}) and the swap words ({b},), got {ta.shape}, {tb.shape}, {sw.shape}")
        host = st["params"].numpy()
        for name, (lo, hi, shape) in self._where.items():
            if name not in cols:                                       # triples only: every clip is a gather
                host[lo:hi] = 0
            elif cols[name].shape != shape:
                raise RuntimeError(f"AugmentedInput.load: {name} must be {shape}, got {cols[name].shape}")
            else:
                (host[lo:hi].view(np.float32) if name == "affine" else host[lo:hi])[:] = cols[name].reshape(-1)
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
        target = None if self.target is None else self.target.view(self.nclips, self.L * self.L)
        frames, masks = self.frames, self.masks
        if self.perturb:
            frames, masks, side = self.canvas, self.mask_canvas, (self.L, self.L)
            ops.resize_nearest_u8(self.frames, side, out=frames)
            if masks is not None:
                ops.resize_nearest_u8(self.masks, side, out=masks, channels=1)
            ops.jpeg_roundtrip_u8(frames, self.qtab, sel=self.sel, out=frames, workspace=self._perturb_ws)
            ops.gaussian_blur_u8(frames, self.blur, out=frames, workspace=self._perturb_ws)
            if self.photometric:
                ops.photometric_u8(frames, self.photo, out=frames, workspace=self._perturb_ws)
            if self.geometric:
                frames = ops.geometric_u8(frames, self.geo, out=self.canvas2)
                if masks is not None:
                    masks = ops.geometric_u8(masks, self.geo_mask, out=self.mask_canvas2, channels=1)
        if self.warp:
            ops.augment_warp_u8(frames, self.tab_a, self.tab_b, self.swap, self.mode, self.pos_y, self.pos_x, self.coef_y, self.coef_x,
                                self.affine, masks=masks, out=self.x, target=target, mean=self.mean, std=self.std)
        else:
            ops.augment_stage_u8(frames, self.tab_a, self.tab_b, self.swap, masks=masks, out=self.x, target=target,
                                 mean=self.mean, std=self.std)
