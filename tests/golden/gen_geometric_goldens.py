"""Regenerates tests/golden/geometric.npz: what Pillow itself gives for the affine group and for Cutout's rectangle fill (Pillow only;
the project's code is not imported), with the Pillow version that produced the bytes.

  small cases (1x1, 2x5, 7x9, 19x21), RGB and single-channel: the input and Pillow's output for every entry of CASES and RECTS;
  one 64x48 RGB case per entry of BIG_CASES: the sha256 of Pillow's output (the input is regenerated from its seed).

    python tests/golden/gen_geometric_goldens.py
"""
import hashlib
import os

import numpy as np
import PIL
from PIL import Image, ImageDraw

SMALL = ((1, 1), (2, 5), (7, 9), (19, 21))
CASES = (("shear_x", 0.13), ("shear_x", -0.3), ("shear_y", 0.05), ("shear_y", -0.3), ("translate_x", 0.2501), ("translate_x", -0.45),
         ("translate_y", 0.1), ("translate_y", -0.33), ("translate_x_abs", 3), ("translate_y_abs", -7.5), ("rotate", 17.3),
         ("rotate", -30), ("rotate", 90), ("rotate", 180), ("rotate", 270), ("rotate", -179.5))
RECTS = ((2, 1, 5.7, 3.2), (0, 0, 3.9, 2), (4, 3, 21, 19), (30, 30, 40.5, 41))
BIG = (64, 48)
BIG_CASES = (("shear_x", 0.3), ("shear_y", -0.13), ("translate_x", 0.33), ("translate_y_abs", 10), ("rotate", 45), ("rotate", 89.9),
             ("rotate", 123.4))


def image(hw, channels, seed):
    """Noise over a ramp, never 0: a pixel the operation left at the fill colour cannot be mistaken for one it moved."""
    h, w = hw
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([yy * 5 + xx * 2, 255 - xx * 3 - yy, (yy * xx) % 256], -1)
    a = (1 + np.clip(base + g.integers(-24, 25, (h, w, 3)), 0, 254)).astype(np.uint8)
    return a if channels == 3 else np.ascontiguousarray(a[..., 1])


def pil_geometric(a, kind, value):
    """One affine kind as the reference calls Pillow (utils/randaugment.py:20-86), the sign flip already in `value`: fill colour 0 for
    frames (FILL_COLOR) and masks (IGNORE_LABEL) alike."""
    im = Image.fromarray(a)
    fill = 0 if a.ndim == 2 else (0, 0, 0)
    w, h = im.size
    if kind == "rotate":
        return np.array(im.rotate(value, resample=Image.NEAREST, fillcolor=fill))
    m = {"shear_x": (1, value, 0, 0, 1, 0), "shear_y": (1, 0, 0, value, 1, 0), "translate_x": (1, 0, value * w, 0, 1, 0),
         "translate_y": (1, 0, 0, 0, 1, value * h), "translate_x_abs": (1, 0, value, 0, 1, 0), "translate_y_abs": (1, 0, 0, 0, 1, value)}[kind]
    return np.array(im.transform(im.size, Image.AFFINE, m, resample=Image.NEAREST, fillcolor=fill))


def pil_cutout(a, rect):
    """CutoutAbs's drawing call: ImageDraw.Draw(img).rectangle(xy, (0, 0, 0)) on a copy."""
    im = Image.fromarray(a).copy()
    ImageDraw.Draw(im).rectangle(tuple(rect), 0 if a.ndim == 2 else (0, 0, 0))
    return np.array(im)


def key(hw, channels, kind, value):
    v = "_".join(str(x) for x in value) if isinstance(value, tuple) else str(value)
    return f"{kind}_{hw[0]}x{hw[1]}x{channels}_{v}"


def main():
    out = {"pillow_version": np.array(PIL.__version__), "big_seed": np.array(17)}
    for k, hw in enumerate(SMALL):
        for c in (1, 3):
            a = image(hw, c, 300 + k)
            out[f"in_{hw[0]}x{hw[1]}x{c}"] = a
            for kind, value in CASES:
                out[key(hw, c, kind, value)] = pil_geometric(a, kind, value)
            for rect in RECTS:
                out[key(hw, c, "cutout", rect)] = pil_cutout(a, rect)
    big = image(BIG, 3, 17)
    for kind, value in BIG_CASES:
        out["sha256_" + key(BIG, 3, kind, value)] = np.array(hashlib.sha256(pil_geometric(big, kind, value).tobytes()).hexdigest())
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "geometric.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
