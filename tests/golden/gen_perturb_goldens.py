"""Regenerates tests/golden/perturb.npz: what Pillow itself gives for the JPEG round trip and the Gaussian blur (Pillow only; the
project's code is not imported), with the Pillow and libjpeg versions that produced the bytes.

  small cases (16x16, 19x21, 24x40): the input and Pillow's output at quality 30, 75, 100 and radius 0.3, 2.5, 5;
  one 224x224 case per operation: the sha256 of Pillow's output (the input is regenerated from its seed).

    python tests/golden/gen_perturb_goldens.py
"""
import hashlib
import io
import os

import numpy as np
import PIL
from PIL import Image, ImageFilter, features

SMALL = ((16, 16), (19, 21), (24, 40))
QUALITIES = (30, 75, 100)
RADII = (0.3, 2.5, 5.0)
BIG, BIG_QUALITY, BIG_RADIUS = (224, 224), 50, 2.0


def image(hw, seed):
    """A smooth ramp with noise of +-24: neither flat nor white noise, every channel different."""
    h, w = hw
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([yy * 5 + xx * 2, 255 - xx * 3 - yy, (yy * xx) % 256], -1)
    return np.clip(base + g.integers(-24, 25, (h, w, 3)), 0, 255).astype(np.uint8)


def pil_jpeg(a, q):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", quality=int(q))
    buf.seek(0)
    return np.array(Image.open(buf))


def pil_blur(a, r):
    return np.array(Image.fromarray(a).filter(ImageFilter.GaussianBlur(radius=r)))


def main():
    out = {"pillow_version": np.array(PIL.__version__), "libjpeg_version": np.array(str(features.version("jpg"))),
           "libjpeg_turbo": np.array(bool(features.check_feature("libjpeg_turbo")))}
    for k, hw in enumerate(SMALL):
        a = image(hw, 100 + k)
        name = f"{hw[0]}x{hw[1]}"
        out[f"in_{name}"] = a
        for q in QUALITIES:
            out[f"jpeg_{name}_q{q}"] = pil_jpeg(a, q)
        for r in RADII:
            out[f"blur_{name}_r{r}"] = pil_blur(a, r)
    big = image(BIG, 7)
    out["big_seed"] = np.array(7)
    out["big_jpeg_sha256"] = np.array(hashlib.sha256(pil_jpeg(big, BIG_QUALITY).tobytes()).hexdigest())
    out["big_blur_sha256"] = np.array(hashlib.sha256(pil_blur(big, BIG_RADIUS).tobytes()).hexdigest())
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "perturb.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, Pillow {PIL.__version__}, libjpeg {features.version('jpg')}")


if __name__ == "__main__":
    main()
