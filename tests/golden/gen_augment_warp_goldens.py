"""Generate tests/golden/augment_warp.npz from the REAL reference's RandomScaleCrop, on CPU.

    python tests/golden/gen_augment_warp_goldens.py [--ref /root/reference] [--out tests/golden]

Runs RandomScaleCrop (utils/randaugment.py:398-428: a CUBIC upscale to S x S, then CornerCrop's box around the upscaled mask resized
back to S x S) on seeded 28 x 28 uint8 clips of 3 frames plus a mask, alone and after a D4 operation as the Double strategy composes
them, followed by the loader's `resize(inputRes)` (universaldataset.py:111-112) with Image.NEAREST spelled out.  S is forced by
wrapping random.randint; the box is recorded by wrapping Image.Image.crop; CornerCrop's own draws (np.random.randint) are seeded.
v = 20 <= S, so the function's padding branch is not taken -- as in the reference's recipes, where v <= 220 < 256 <= S.

Stand-ins: those of gen_augment_goldens.py (an empty `cv2`, the stub `configs.davis.config`), plus two for today's Pillow:
Image.CUBIC = Image.BICUBIC (the constant was removed), and Image.Image.resize wrapped so that a call without `resample` means
NEAREST, the default of the pillow==4.0.0 the reference pins -- CornerCrop relies on it.  RandomRotate has no golden: it needs the
real cv2.  tests/test_augment_warp_host.py and tests/test_augment_warp.py read only the .npz."""
import argparse
import os
import random
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from gen_augment_goldens import install_stubs          # noqa: E402

L = 28


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    sys.path.insert(0, install_stubs())             # in front: the stand-in `configs` wins over the reference's
    Image.CUBIC = Image.BICUBIC
    real_resize = Image.Image.resize

    def resize(self, size, resample=None, *a, **kw):
        return real_resize(self, size, Image.NEAREST if resample is None else resample, *a, **kw)
    Image.Image.resize = resize
    import utils.randaugment as RA

    rng = np.random.default_rng(20241)
    frames = rng.integers(0, 256, (3, L, L, 3), dtype=np.uint8)
    mask = np.zeros((L, L), np.uint8)
    mask[9:17, 6:19] = rng.choice(np.array([0, 1, 37, 255], np.uint8), (8, 13))
    mask[9, 6] = mask[16, 18] = 255                   # the bounding box is rows 9..16, columns 6..18 whatever was drawn
    zero = np.zeros((L, L), np.uint8)

    boxes = []
    real_crop = Image.Image.crop

    def crop(self, box=None):
        boxes.append(tuple(int(v) for v in box))
        return real_crop(self, box)
    Image.Image.crop = crop

    def forced_pscc(p, k):
        real = np.random.randint
        np.random.randint = lambda lo, hi=None, *a, **kw: k
        try:
            return RA.PsccAug(p, 0.5)
        finally:
            np.random.randint = real

    def scale_crop(p, S):
        real = random.randint
        random.randint = lambda a, b: S
        try:
            return RA.RandomScaleCrop(p, 20.0)
        finally:
            random.randint = real

    D4 = {"none": lambda p: p, "hflip": lambda p: RA.HFlip(p, 1), "pscc1": lambda p: forced_pscc(p, 1)}
    cases = [("none", 32, 0), ("none", 57, 0), ("none", 100, 0), ("none", 64, 1), ("pscc1", 57, 0), ("hflip", 100, 0)]
    random.seed(11)
    np.random.seed(11)
    rec = dict(d4=[], S=[], zero_mask=[], box=[], out_frames=[], out_mask=[])
    for d4, S, zm in cases:
        boxes.clear()
        imgs, m = scale_crop(D4[d4](([Image.fromarray(f) for f in frames], Image.fromarray(zero if zm else mask))), S)
        assert all(i.size == (S, S) for i in imgs) and m.size == (S, S)
        assert bool(zm) == (not boxes) and len(set(boxes)) <= 1, (d4, S, boxes)               # one box for every frame and the mask
        rec["d4"].append(d4); rec["S"].append(S); rec["zero_mask"].append(zm)
        rec["box"].append(boxes[0] if boxes else (-1, -1, -1, -1))
        rec["out_frames"].append(np.stack([np.asarray(i.resize((L, L), Image.NEAREST)) for i in imgs]))
        rec["out_mask"].append(np.asarray(m.resize((L, L), Image.NEAREST)).copy())
    Image.Image.crop, Image.Image.resize = real_crop, real_resize
    out = os.path.join(args.out, "augment_warp.npz")
    np.savez_compressed(out, frames=frames, mask=mask, d4=np.array(rec["d4"]), S=np.array(rec["S"], np.int32),
                        zero_mask=np.array(rec["zero_mask"], np.int32), box=np.array(rec["box"], np.int32),
                        out_frames=np.stack(rec["out_frames"]), out_mask=np.stack(rec["out_mask"]))
    print(f"wrote {out}: {len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
