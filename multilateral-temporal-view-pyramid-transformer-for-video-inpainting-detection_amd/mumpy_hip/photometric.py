"""The photometric half of the reference's augmentation file, restated bit for bit: ImageOps.autocontrast / invert / equalize /
solarize / posterize and ImageEnhance.Contrast / Color / Brightness / Sharpness of Pillow on RGB images.

The reference ships all nine (utils/randaugment.py:89-110, 129-191) and leaves them commented out of its lists (:557-565, :587-597),
as it does the JPEG round trip and the blur of mumpy_hip/perturb.py.  ops.photometric_u8 runs the same arithmetic on the device
(csrc/photometric.hip); this module is its numpy statement and the host half of its arguments:

    autocontrast(img) ... sharpness(img, v)   one function per kind, (H, W, 3) uint8 -> the same
    apply(img, kind, value)                   the dispatcher, by name or by code
    KINDS                                     name -> the integer code the kernels read (0: pass through)
    params_row(kind, value)                   the int32[4] row of one image: the one place that encodes a row
    draw(rng, kinds)                          one condition out of the reference's ranges

Seven kinds are one 256-entry table per channel once the image's histogram or mean luminance is known; color and sharpness are per
pixel.  The four float kinds go through Image.blend, whose product and sum are two float32 roundings (no fused multiply-add: a Pillow
compiled with contraction would differ, and tests/test_photometric_host.py would show it against the installed Pillow).

numpy only: imports and runs without a GPU.  DESIGN.md ("Photometric operations") gives the arithmetic and what is pinned to which
Pillow."""
import math

import numpy as np

KINDS = {"none": 0, "autocontrast": 1, "invert": 2, "equalize": 3, "solarize": 4, "posterize": 5, "contrast": 6, "color": 7,
         "brightness": 8, "sharpness": 9}
NAMES = {v: k for k, v in KINDS.items()}
VALUELESS = ("autocontrast", "equalize", "invert")
FACTOR = ("contrast", "color", "brightness", "sharpness")
FACTOR_MAX = 16.0

f32 = np.float32


def _check(img_u8, who):
    img = np.asarray(img_u8)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError(f"{who}: needs a uint8 image (H, W, 3) with H, W >= 1, got {img.dtype} {img.shape}")
    return img


def _gather(img, tables):
    """tables (3, 256) or (256,) uint8: out[..., c] = tables[c][img[..., c]]"""
    tables = np.broadcast_to(np.asarray(tables, np.uint8), (3, 256))
    return np.stack([tables[c][img[..., c]] for c in range(3)], -1)


def _clip8(t):
    """float32 array -> bytes as Pillow clips: 0 if <= 0, 255 if >= 255, else truncated"""
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def blend(degenerate, image, v):
    """Image.blend(degenerate, image, v) on integer arrays: t = float32(d) + float32(v) * float32(i - d), the product and the sum
    rounded to float32 one after the other.  Pillow truncates t for 0 <= v <= 1 and clips it otherwise; inside that range t lies
    between d and i, where the two agree."""
    d, i = np.asarray(degenerate, np.int32), np.asarray(image, np.int32)
    prod = (f32(v) * (i - d).astype(f32)).astype(f32)
    return _clip8((d.astype(f32) + prod).astype(f32))


def luminance(img):
    """convert("L") of an RGB image: (19595 R + 38470 G + 7471 B + 32768) >> 16"""
    p = img.astype(np.int64)
    return (19595 * p[..., 0] + 38470 * p[..., 1] + 7471 * p[..., 2] + 32768) >> 16


def invert(img_u8):
    return _gather(_check(img_u8, "invert"), 255 - np.arange(256))


def solarize_threshold(v) -> int:
    """i < v in float for an integer i is i < ceil(v): the integer the kernels compare with."""
    v = float(v)
    if not 0 <= v <= 256:
        raise ValueError(f"solarize: threshold={v} must be in 0 .. 256")
    return int(math.ceil(v))


def solarize(img_u8, v):
    i = np.arange(256)
    return _gather(_check(img_u8, "solarize"), np.where(i < solarize_threshold(v), i, 255 - i))


def posterize_bits(v) -> int:
    bits = int(v)
    if bits != v or not 0 <= bits <= 8:
        raise ValueError(f"posterize: bits={v!r} must be an integer in 0 .. 8")
    return bits


def posterize(img_u8, v):
    return _gather(_check(img_u8, "posterize"), np.arange(256) & ~(2 ** (8 - posterize_bits(v)) - 1) & 255)


def autocontrast_table(h):
    """h (256,) counts of one channel -> its table"""
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(max(int(i * scale + offset), 0), 255) for i in range(256)])


def autocontrast(img_u8):
    img = _check(img_u8, "autocontrast")
    return _gather(img, [autocontrast_table(np.bincount(img[..., c].ravel(), minlength=256)) for c in range(3)])


def equalize_table(h):
    """h (256,) counts of one channel -> its table.  Three identity exits; an entry saturates at 255."""
    h = [int(v) for v in h]
    histo = [v for v in h if v]
    if len(histo) <= 1:
        return np.arange(256)
    step = (sum(histo) - histo[-1]) // 255
    if not step:
        return np.arange(256)
    out, n = [], step // 2
    for i in range(256):
        out.append(min(n // step, 255))
        n += h[i]
    return np.array(out)


def equalize(img_u8):
    img = _check(img_u8, "equalize")
    return _gather(img, [equalize_table(np.bincount(img[..., c].ravel(), minlength=256)) for c in range(3)])


def _factor(v, who):
    v = float(v)
    if not math.isfinite(v) or not 0 <= v <= FACTOR_MAX:
        raise ValueError(f"{who}: factor={v} must be finite and in 0 .. {FACTOR_MAX:g}")
    return v


def brightness(img_u8, v):
    return _gather(_check(img_u8, "brightness"), blend(0, np.arange(256), _factor(v, "brightness")))


def contrast_mean(img) -> int:
    """int(mean(L) + 0.5) in integers: (2 sum + n) // (2 n).  A quotient comes no nearer to .5 than 1 / (2 n), far above the rounding
    of the double division Pillow does."""
    L = luminance(img)
    return int((2 * int(L.sum()) + L.size) // (2 * L.size))


def contrast(img_u8, v):
    img = _check(img_u8, "contrast")
    return _gather(img, blend(contrast_mean(img), np.arange(256), _factor(v, "contrast")))


def color(img_u8, v):
    img = _check(img_u8, "color")
    return blend(luminance(img)[..., None], img, _factor(v, "color"))


SMOOTH_WEIGHTS = (1, 1, 1, 1, 5, 1, 1, 1, 1)
SMOOTH_KERNEL = np.array([f32(w) / f32(13) for w in SMOOTH_WEIGHTS], f32).reshape(3, 3)


def smooth(img_u8):
    """Image.filter(ImageFilter.SMOOTH): the sum starts at 0.5f and takes the row terms of y + 1, y, y - 1 one after another, a row
    term being p[x-1] k0 + p[x] k1 + p[x+1] k2 with every product and sum rounded to float32; clipped; the one-pixel border, and an
    image with a side below 3, are copied."""
    img = _check(img_u8, "smooth")
    H, W = img.shape[:2]
    out = img.copy()
    if H < 3 or W < 3:
        return out
    p = img.astype(f32)
    ss = np.full((H - 2, W - 2, 3), 0.5, f32)
    for dy, krow in ((2, SMOOTH_KERNEL[2]), (1, SMOOTH_KERNEL[1]), (0, SMOOTH_KERNEL[0])):
        r = p[dy:dy + H - 2]
        a, b, c = (r[:, 0:W - 2] * krow[0]).astype(f32), (r[:, 1:W - 1] * krow[1]).astype(f32), (r[:, 2:W] * krow[2]).astype(f32)
        ss = (ss + ((a + b).astype(f32) + c).astype(f32)).astype(f32)
    out[1:-1, 1:-1] = _clip8(ss)
    return out


def sharpness(img_u8, v):
    img = _check(img_u8, "sharpness")
    return blend(smooth(img), img, _factor(v, "sharpness"))


_FUNCS = {"autocontrast": autocontrast, "invert": invert, "equalize": equalize, "solarize": solarize, "posterize": posterize,
          "contrast": contrast, "color": color, "brightness": brightness, "sharpness": sharpness}


def check_kind(kind, value, who="photometric"):
    """-> (name, value) with the value as the kind takes it (None, a float, the posterize bit count), refused otherwise."""
    if kind not in _FUNCS:
        raise ValueError(f"{who}: kind={kind!r} must be one of {sorted(_FUNCS)}")
    if kind in VALUELESS:
        if value is not None:
            raise ValueError(f"{who}: {kind} takes no value, got {value!r}")
        return kind, None
    if value is None or isinstance(value, (str, bytes)):
        raise ValueError(f"{who}: {kind} needs a number, got {value!r}")
    if kind == "posterize":
        return kind, posterize_bits(value)
    if kind == "solarize":
        solarize_threshold(value)
        return kind, float(value)
    return kind, _factor(value, f"{who}: {kind}")


def apply(img_u8, kind, value=None):
    """One operation by name or by code; "none" / 0 returns a copy."""
    kind = NAMES.get(kind, kind) if not isinstance(kind, str) else kind
    if kind == "none":
        return _check(img_u8, "apply").copy()
    kind, value = check_kind(kind, value, "apply")
    return _FUNCS[kind](img_u8) if value is None else _FUNCS[kind](img_u8, value)


def params_row(kind, value=None) -> np.ndarray:
    """int32[4] {code, value, 0, 0}: the bits of the float32 factor for contrast, color, brightness and sharpness, ceil(threshold)
    for solarize, the bit count for posterize, 0 for the rest."""
    row = np.zeros(4, np.int32)
    if kind in ("none", 0, None):
        return row
    kind, value = check_kind(NAMES.get(kind, kind) if not isinstance(kind, str) else kind, value, "params_row")
    row[0] = KINDS[kind]
    if kind == "posterize":
        row[1] = value
    elif kind == "solarize":
        row[1] = solarize_threshold(value)
    elif kind in FACTOR:
        row[1] = np.array([value], f32).view(np.int32)[0]
    return row


SOLARIZE_RANGE = (0.0, 110.0)       # randaugment.py:557-565, 587-597
POSTERIZE_RANGE = (3.0, 8.0)
FACTOR_RANGE = (0.5, 1.5)


def draw(rng, kinds=tuple(_FUNCS)):
    """One condition (kind, value), the kind uniform over `kinds`: the reference's ranges, not its RNG stream."""
    kinds = tuple(kinds)
    if not kinds or any(k not in _FUNCS for k in kinds):
        raise ValueError(f"draw: kinds={kinds!r} must be a non-empty choice of {sorted(_FUNCS)}")
    kind = kinds[int(rng.integers(0, len(kinds)))]
    if kind in VALUELESS:
        return kind, None
    if kind == "solarize":
        return kind, float(rng.uniform(*SOLARIZE_RANGE))
    if kind == "posterize":
        return kind, int(rng.uniform(*POSTERIZE_RANGE))
    return kind, float(rng.uniform(*FACTOR_RANGE))
