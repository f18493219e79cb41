"""The geometric group of the reference's augmentation file, restated bit for bit: ShearX / ShearY / TranslateX / TranslateY /
TranslateXAbs / TranslateYAbs / Rotate (utils/randaugment.py:20-86) and Cutout / CutoutAbs (:209-260) of Pillow on uint8 images.

These are the first operations of that file that move the MASK together with the frames (affine_transform transforms both with the
same six numbers; Cutout reads the mask to place its rectangles and leaves it alone).  ops.geometric_u8 runs them on the device
(csrc/geometric.hip); this module is the numpy statement and the host half of the arguments:

    affine_matrix(kind, value, hw)     the six doubles the reference hands to Pillow (Image.rotate's matrix for "rotate")
    params_row(kind, value, hw)        the int32[8] row of one image: the one place that encodes a row
    apply_row(img, row)                what the kernel computes from a row
    affine(img, kind, value)           apply_row of params_row: Image.transform(size, AFFINE, m, NEAREST, fillcolor=0) / Image.rotate
    cutout(img, rect)                  ImageDraw.rectangle(rect, 0): corners truncated, filled inclusively, clipped to the image
    cutout_rects(canvas_mask, v, T, rng)  the reference's placement of T rectangles, quirks included
    draw(rng, kinds), check_kind(kind, value)

Pillow's Geometry.c takes one of two integer-exact paths for a NEAREST affine transform.  With m[1] == 0 and m[3] == 0 (the
translations, a zero shear) it walks the columns and rows in double precision -- xo = m[2] + m[0] * 0.5, then xin = (xo < 0 ? -1 :
(int) xo) and xo += m[0] per column, the same per row; for m[0] = m[4] = 1 that is an integer shift, which params_row derives by
running the walk and checking it (mode SHIFT).  Everything else (shear, rotate) takes the 16.16 fixed-point walk affine_fixed as long
as the four transformed corners stay within +-32768 (check_fixed): FIX(v) = floor(v * 65536 + 0.5), a0, a1, a3, a4 = FIX(m[0]),
FIX(m[1]), FIX(m[3]), FIX(m[4]), a2 = FIX(m[2] + m[0] / 2 + m[1] / 2), a5 = FIX(m[5] + m[3] / 2 + m[4] / 2), and output (x, y)
reads source ((a2 + a0 x + a1 y) >> 16, (a5 + a3 x + a4 y) >> 16) or stays at the fill colour 0 when either index is out of range
(mode FIXED16).  Pillow's third, double-precision path (corners beyond +-32768) is not offered: params_row refuses.

numpy only: imports and runs without a GPU.  DESIGN.md ("Geometric operations") gives the arithmetic."""
import math

import numpy as np

MODES = {"none": 0, "fixed16": 1, "shift": 2, "rect": 3}
MODE_NONE, MODE_FIXED16, MODE_SHIFT, MODE_RECT = 0, 1, 2, 3
AFFINE_KINDS = ("shear_x", "shear_y", "translate_x", "translate_y", "translate_x_abs", "translate_y_abs", "rotate")
KINDS = AFFINE_KINDS + ("cutout",)

# the reference's asserts (randaugment.py:33-77, 210).  The Abs kinds assert 0 <= v <= 10 BEFORE the sign flip that every affine kind
# then applies with probability 0.5; a value here is the one that reaches Pillow, after the flip, so it lies in +-10.
LIMITS = {"shear_x": (-0.3, 0.3), "shear_y": (-0.3, 0.3), "translate_x": (-0.45, 0.45), "translate_y": (-0.45, 0.45),
          "translate_x_abs": (-10.0, 10.0), "translate_y_abs": (-10.0, 10.0), "rotate": (-180.0, 180.0), "cutout": (0.0, 0.2)}
# the ranges of augment_list() (randaugment.py:542-576), drawn before the sign flip
RANGES = {"shear_x": (0.0, 0.3), "shear_y": (0.0, 0.3), "translate_x": (0.0, 0.33), "translate_y": (0.0, 0.33),
          "translate_x_abs": (0.0, 10.0), "translate_y_abs": (0.0, 10.0), "rotate": (0.0, 180.0), "cutout": (0.0, 0.2)}
SIZE_MAX = 8192                     # the kernel's bound on H and W
INT32 = (-(1 << 31), (1 << 31) - 1)


def _check(img_u8, who):
    img = np.asarray(img_u8)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"{who}: needs a uint8 image (H, W) or (H, W, C) with H, W >= 1, got {img.dtype} {img.shape}")
    return img


def _hw(hw, who):
    h, w = (int(v) for v in hw)
    if h < 1 or w < 1:
        raise ValueError(f"{who}: bad image size {h}x{w}")
    return h, w


def _number(value, who):
    if isinstance(value, (str, bytes, bool)) or not isinstance(value, (int, float, np.integer, np.floating)) or not math.isfinite(value):
        raise ValueError(f"{who} needs a finite number, got {value!r}")
    return float(value)


def check_kind(kind, value, who="geometric"):
    """-> (kind, float(value)), refused unless the kind is one of KINDS and the value a finite number inside the reference's assert
    for it (LIMITS; the Abs kinds: see there)."""
    if kind not in KINDS:
        raise ValueError(f"{who}: kind={kind!r} must be one of {list(KINDS)}")
    v = _number(value, f"{who}: {kind}")
    lo, hi = LIMITS[kind]
    if not lo <= v <= hi:
        raise ValueError(f"{who}: {kind} needs a finite value in {lo} .. {hi}, got {value!r}")
    return kind, v


def rotate_matrix(angle, hw):
    """The matrix Image.rotate(angle) hands to Image.transform for an image of (H, W) -- cos and sin rounded to 15 decimals, about
    (w / 2, h / 2) -- and for its three exits, which are exact transposes, the matrix whose fixed-point walk is that transpose:
    angle % 360 == 0 (a copy), == 180 (ROTATE_180), 90 / 270 on a square image (ROTATE_90 / ROTATE_270)."""
    h, w = _hw(hw, "rotate_matrix")
    angle = float(angle) % 360.0
    if angle == 0:
        return (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    if angle == 180:
        return (-1.0, 0.0, float(w), 0.0, -1.0, float(h))
    if angle in (90, 270) and w == h:
        return (0.0, -1.0, float(w), 1.0, 0.0, 0.0) if angle == 90 else (0.0, 1.0, 0.0, -1.0, 0.0, float(h))
    cx, cy = w / 2, h / 2
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(float(v) for v in m)


def affine_matrix(kind, value, hw):
    """The six doubles (a, b, c, d, e, f) the reference hands to Pillow for one affine kind on an image of hw = (H, W): output (x, y)
    reads source (a x + b y + c, d x + e y + f).  The translate fractions are multiplied by the width / height as the reference
    multiplies them (one double product).  Any finite value is taken (Pillow takes any); check_kind holds the reference's asserts."""
    if kind not in AFFINE_KINDS:
        raise ValueError(f"affine_matrix: kind={kind!r} must be one of {list(AFFINE_KINDS)}")
    v = _number(value, f"affine_matrix: {kind}")
    h, w = _hw(hw, "affine_matrix")
    if kind == "shear_x":
        return (1.0, v, 0.0, 0.0, 1.0, 0.0)
    if kind == "shear_y":
        return (1.0, 0.0, 0.0, v, 1.0, 0.0)
    if kind in ("translate_x", "translate_x_abs"):
        return (1.0, 0.0, v * w if kind == "translate_x" else v, 0.0, 1.0, 0.0)
    if kind in ("translate_y", "translate_y_abs"):
        return (1.0, 0.0, 0.0, 0.0, 1.0, v * h if kind == "translate_y" else v)
    return rotate_matrix(v, (h, w))


def fix16(v):
    """Geometry.c: FIX(v) = FLOOR(v * 65536.0 + 0.5), with FLOOR(v) = v >= 0 ? (int) v : (int) floor(v)."""
    return int(math.floor(v * 65536.0 + 0.5))


def check_fixed(m, hw):
    """Geometry.c: check_fixed over the four corners (0, 0), (w, h), (0, h), (w, 0): every transformed coordinate within +-32768."""
    h, w = hw
    return all(abs(x * m[0] + y * m[1] + m[2]) < 32768.0 and abs(x * m[3] + y * m[4] + m[5]) < 32768.0
               for x, y in ((0, 0), (w, h), (0, h), (w, 0)))


def fixed16_words(m, hw):
    """(a0 .. a5) of affine_fixed, refused where Pillow would leave that path (check_fixed) or a word left 32 bits."""
    if not check_fixed(m, hw):
        raise ValueError(f"geometric: matrix {tuple(m)} on {hw[0]}x{hw[1]} fails Pillow's check_fixed (a corner beyond +-32768): Pillow "
                         f"would take its double-precision path, which is not offered")
    a = (fix16(m[0]), fix16(m[1]), fix16(m[2] + m[0] * 0.5 + m[1] * 0.5), fix16(m[3]), fix16(m[4]), fix16(m[5] + m[3] * 0.5 + m[4] * 0.5))
    if any(not INT32[0] <= v <= INT32[1] for v in a):
        raise ValueError(f"geometric: matrix {tuple(m)}: a 16.16 word leaves 32 bits")
    return a


def scale_walk(m, hw):
    """Geometry.c: ImagingScaleAffine's double walk -> (xin (W,), yin (H,)) int64, -1 where COORD gives a negative coordinate."""
    h, w = hw

    def walk(o, step, n):
        out = np.empty(n, np.int64)
        for k in range(n):
            out[k] = -1 if o < 0.0 or o >= 2.0 ** 62 else int(o)
            o += step
        return out
    return walk(m[2] + m[0] * 0.5, m[0], w), walk(m[5] + m[4] * 0.5, m[4], h)


def constant_shift(m, hw):
    """(dx, dy) with xin = x + dx and yin = y + dy wherever Pillow's double walk lands inside the image and x + dx / y + dy outside
    it wherever the walk does not, for a matrix (1, 0, tx, 0, 1, ty).  ValueError if the walk is no such shift (the sums of a walk
    round: tx + 0.5 just below an integer can step over it)."""
    if not (m[0] == 1 and m[1] == 0 and m[3] == 0 and m[4] == 1):
        raise ValueError(f"geometric: {tuple(m)} is no translation")
    h, w = hw
    if not (abs(m[2]) < 2.0 ** 31 - 1 and abs(m[5]) < 2.0 ** 31 - 1):
        raise ValueError(f"geometric: translation {m[2]}, {m[5]} leaves 32 bits")
    out = []
    for t, idx, n in ((m[2], scale_walk(m, hw)[0], w), (m[5], scale_walk(m, hw)[1], h)):
        d = int(math.floor(t + 0.5))
        want = np.arange(n, dtype=np.int64) + d
        inside, winside = (idx >= 0) & (idx < n), (want >= 0) & (want < n)
        if not (np.array_equal(inside, winside) and np.array_equal(idx[inside], want[inside])):
            raise ValueError(f"geometric: Pillow's walk from {t!r} over {n} pixels is not the constant shift {d}")
        out.append(d)
    return tuple(out)


def clip_rect(rect, hw):
    """ImageDraw.rectangle's reading of (x0, y0, x1, y1): refused if x1 < x0 or y1 < y0 (as Pillow refuses), corners truncated toward
    zero, filled inclusively, clipped to the image -> inclusive integers, or None when nothing is left."""
    h, w = hw
    x0, y0, x1, y1 = (float(v) for v in rect)
    if not all(math.isfinite(v) for v in (x0, y0, x1, y1)):
        raise ValueError(f"cutout: rectangle {tuple(rect)} must be finite")
    if x1 < x0 or y1 < y0:
        raise ValueError(f"cutout: rectangle {tuple(rect)} needs x1 >= x0 and y1 >= y0")
    big = float(1 << 30)
    x0, y0, x1, y1 = (int(min(max(v, -big), big)) for v in (x0, y0, x1, y1))
    x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
    return None if x0 > x1 or y0 > y1 else (x0, y0, x1, y1)


def params_row(kind, value=None, hw=None) -> np.ndarray:
    """int32[8] {mode, a0, a1, a2, a3, a4, a5, 0} of one image of hw = (H, W):
        NONE     copy ("none" / None)
        FIXED16  the six 16.16 words of affine_fixed (shears with v != 0, every rotate)
        SHIFT    {dx, dy}: source (x + dx, y + dy) (the translations and a zero shear: Pillow's scale path, walked and checked here)
        RECT     {x0, y0, x1, y1} inclusive and clipped, filled with 0 ("cutout", value = the rectangle); an empty one is NONE.
    A rotate whose matrix has b = d = 0 (0 and 180 degrees) goes to Pillow's scale path or a transpose; it is encoded FIXED16 after
    the fixed-point walk is checked against that."""
    row = np.zeros(8, np.int32)
    if kind in ("none", None):
        return row
    h, w = _hw(hw, "params_row")
    if h > SIZE_MAX or w > SIZE_MAX:
        raise ValueError(f"params_row: {h}x{w} is above {SIZE_MAX} a side")
    if kind == "cutout":
        r = clip_rect(value, (h, w))
        if r is not None:
            row[:5] = (MODE_RECT,) + r
        return row
    m = affine_matrix(kind, value, (h, w))
    if kind != "rotate" and m[1] == 0 and m[3] == 0:
        row[:3] = (MODE_SHIFT,) + constant_shift(m, (h, w))
        return row
    row[:7] = (MODE_FIXED16,) + fixed16_words(m, (h, w))
    if m[1] == 0 and m[3] == 0:                                       # rotate by 0 or 180: the fixed walk must be the exact flip
        xs, ys = _fixed_sources(row, (h, w))
        fx, fy = (np.arange(w), np.arange(h)) if m[0] > 0 else (w - 1 - np.arange(w), h - 1 - np.arange(h))
        if not (np.array_equal(xs, np.broadcast_to(fx[None, :], (h, w))) and np.array_equal(ys, np.broadcast_to(fy[:, None], (h, w)))):
            raise ValueError(f"params_row: rotate {value!r} on {h}x{w}: the fixed-point walk is not Pillow's transpose")
    return row


def _fixed_sources(row, hw):
    h, w = hw
    a = [int(v) for v in row[1:7]]
    x, y = np.arange(w, dtype=np.int64)[None, :], np.arange(h, dtype=np.int64)[:, None]
    return (a[2] + a[0] * x + a[1] * y) >> 16, (a[5] + a[3] * x + a[4] * y) >> 16


def apply_row(img_u8, row):
    """What the kernel computes for one image from its row (64-bit integers, as the kernel walks): out-of-range pixels 0, an unknown
    mode copies."""
    img = _check(img_u8, "apply_row")
    row = np.asarray(row)
    if row.shape != (8,) or row.dtype != np.int32:
        raise ValueError(f"apply_row: needs an int32 row of 8 words, got {row.dtype} {row.shape}")
    h, w = img.shape[:2]
    mode = int(row[0])
    out = img.copy()
    if mode == MODE_RECT:
        x0, y0, x1, y1 = (int(v) for v in row[1:5])
        x0, y0, x1, y1 = max(x0, 0), max(y0, 0), min(x1, w - 1), min(y1, h - 1)
        if x0 <= x1 and y0 <= y1:
            out[y0:y1 + 1, x0:x1 + 1] = 0
        return out
    if mode == MODE_FIXED16:
        xs, ys = _fixed_sources(row, (h, w))
    elif mode == MODE_SHIFT:
        xs = np.broadcast_to(np.arange(w, dtype=np.int64)[None, :] + int(row[1]), (h, w))
        ys = np.broadcast_to(np.arange(h, dtype=np.int64)[:, None] + int(row[2]), (h, w))
    else:
        return out
    ok = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
    out[...] = 0
    out[ok] = img[ys[ok], xs[ok]]
    return out


def affine(img_u8, kind, value):
    """Image.transform(size, AFFINE, affine_matrix(kind, value), resample=NEAREST, fillcolor=0) -- Image.rotate(value, fillcolor=0)
    for "rotate" -- of an image (H, W, C) or (H, W), bit for bit: the row of params_row applied."""
    img = _check(img_u8, "affine")
    if kind not in AFFINE_KINDS:
        raise ValueError(f"affine: kind={kind!r} must be one of {list(AFFINE_KINDS)}")
    return apply_row(img, params_row(kind, value, img.shape[:2]))


def cutout(img_u8, rect):
    """ImageDraw.Draw(img).rectangle(rect, 0) on a copy: rect = (x0, y0, x1, y1), floats truncated, both corners inside the fill."""
    img = _check(img_u8, "cutout")
    return apply_row(img, params_row("cutout", rect, img.shape[:2]))


def _uniform(rng, low, high=1.0):
    """np.random.uniform(low, high) as the legacy generator computes it, low > high included: low + (high - low) * u."""
    return low + (high - low) * float(rng.random())


def cutout_rects(canvas_mask, v, T, rng):
    """Cutout / CutoutAbs (randaugment.py:209-260) restated: one rectangle (x0, y0, x1, y1) per frame of a clip of T frames, as the
    reference hands it to ImageDraw.rectangle (x0, y0 integers, x1, y1 floats); [] for v <= 0, where the reference returns the pair
    untouched.  canvas_mask (H, W) is the mask the frames travel with.  Kept as the reference has them:
      * `v = v * img.size[0]` sits INSIDE the frame loop, so the side compounds: frame 0 gets v w, frame 1 v w w, frame k v w^(k+1);
      * np.random.uniform(w) is uniform(low=w, high=1.0): a draw between 1 and w, not between 0 and w;
      * with a non-empty mask one axis is placed beside the mask's box (FindCorners) -- left of it if there is more room on the left,
        else right of it; above it or below it likewise -- and the other over the whole side; uniform(0, left - v) and
        uniform(right, w - v) may run backwards or below zero;
      * x0 = int(max(0, x0 - v / 2)), x1 = min(w, x0 + v): the rectangle starts half a side before the drawn point and Pillow fills
        x1 inclusively.
    The distributions are the reference's, the random stream is `rng`'s (numpy Generator)."""
    from .augment import find_corners
    check_kind("cutout", v, "cutout_rects")
    mask = np.asarray(canvas_mask)
    if mask.ndim != 2 or mask.shape[0] < 1 or mask.shape[1] < 1:
        raise ValueError(f"cutout_rects: needs a mask (H, W), got {mask.shape}")
    h, w = mask.shape
    v = float(v)
    if v <= 0.0:
        return []
    corners = find_corners(mask)
    rects = []
    for _ in range(int(T)):
        v = v * w
        if corners is None:
            x0, y0 = _uniform(rng, w), _uniform(rng, h)
        else:
            left, top, right, bottom = corners
            if float(rng.random()) > 0.5:
                x0 = _uniform(rng, 0, left - v) if left > w - right else _uniform(rng, right, w - v)
                y0 = _uniform(rng, h)
            else:
                x0 = _uniform(rng, 0, w)
                y0 = _uniform(rng, 0, top - v) if top > h - bottom else _uniform(rng, bottom, h - v)
        x0, y0 = int(max(0, x0 - v / 2.)), int(max(0, y0 - v / 2.))
        rects.append((x0, y0, min(w, x0 + v), min(h, y0 + v)))
    return rects


def draw(rng, kinds=KINDS):
    """One condition (kind, value), the kind uniform over `kinds`, the value uniform over the reference's list range for it (RANGES)
    and, for the affine kinds, negated with probability 0.5 as every one of them does: the reference's distributions, not its RNG
    stream.  ("cutout", v) still needs its rectangles: cutout_rects."""
    kinds = tuple(kinds)
    if not kinds or any(k not in KINDS for k in kinds):
        raise ValueError(f"draw: kinds={kinds!r} must be a non-empty choice of {list(KINDS)}")
    kind = kinds[int(rng.integers(0, len(kinds)))]
    v = float(rng.uniform(*RANGES[kind]))
    if kind in AFFINE_KINDS and float(rng.random()) > 0.5:
        v = -v
    return kind, v
