"""Regenerates tests/golden/photometric.npz: what Pillow itself gives for the nine photometric operations (Pillow only; the project's
code is not imported), with the Pillow version that produced the bytes.

  small cases (3x3, 7x9, 19x21): the input and Pillow's output for every entry of CASES;
  one 224x224 case per entry of BIG_CASES: the sha256 of Pillow's output (the input is regenerated from its seed).

    python tests/golden/gen_photometric_goldens.py
"""
import hashlib
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageOps

SMALL = ((3, 3), (7, 9), (19, 21))
CASES = (("autocontrast", None), ("invert", None), ("equalize", None), ("solarize", 0.5), ("solarize", 109.7), ("posterize", 0),
         ("posterize", 3), ("posterize", 7)) + tuple((k, f) for k in ("contrast", "color", "brightness", "sharpness") for f in (0.3, 1.3, 2.5))
BIG = (224, 224)
BIG_CASES = (("autocontrast", None), ("equalize", None), ("solarize", 77.5), ("posterize", 4), ("contrast", 1.4), ("color", 0.6),
             ("brightness", 1.7), ("sharpness", 1.9))


def image(hw, seed):
    """A ramp with noise of +-24 squeezed into 20 .. 230: neither flat nor full range, every channel different."""
    h, w = hw
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([yy * 5 + xx * 2, 255 - xx * 3 - yy, (yy * xx) % 256], -1)
    return (20 + np.clip(base + g.integers(-24, 25, (h, w, 3)), 0, 255) * 210 // 255).astype(np.uint8)


def pil_photometric(a, kind, value=None):
    im = Image.fromarray(a)
    if kind in ("autocontrast", "invert", "equalize"):
        out = getattr(ImageOps, kind)(im)
    elif kind in ("solarize", "posterize"):
        out = getattr(ImageOps, kind)(im, value)
    else:
        out = getattr(ImageEnhance, kind.capitalize())(im).enhance(value)
    return np.array(out)


def key(hw, kind, value):
    return f"{kind}_{hw[0]}x{hw[1]}" + ("" if value is None else f"_{value}")


def main():
    out = {"pillow_version": np.array(PIL.__version__), "big_seed": np.array(11)}
    for k, hw in enumerate(SMALL):
        a = image(hw, 200 + k)
        out[f"in_{hw[0]}x{hw[1]}"] = a
        for kind, value in CASES:
            out[key(hw, kind, value)] = pil_photometric(a, kind, value)
    big = image(BIG, 11)
    for kind, value in BIG_CASES:
        out["sha256_" + key(BIG, kind, value)] = np.array(hashlib.sha256(pil_photometric(big, kind, value).tobytes()).hexdigest())
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "photometric.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
