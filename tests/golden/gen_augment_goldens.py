"""Generate tests/golden/augment.npz from the REAL reference's augmentation functions, on CPU.

    python tests/golden/gen_augment_goldens.py [--ref /root/reference] [--out tests/golden]

Runs HFlip, VFlip, PsccAug, RandomCrop and OriginalRandomCrop of the reference's utils/randaugment.py on seeded 28 x 28 uint8 clips of
3 frames plus a mask (and an all-zero mask for RandomCrop's fallback), followed by the loader's `resize(inputRes)`
(universaldataset.py:111-112) -- with Image.NEAREST spelled out, the default of the pillow==4.0.0 the reference pins (today's Pillow
defaults to BICUBIC).  Every PsccAug index 0..6 is forced by wrapping np.random.randint; every crop box is recorded by wrapping
Image.Image.crop; OriginalRandomCrop's three placements are forced by wrapping the first random.randint.  The Double strategy's
composition (a D4 operation, then a crop that looks at the transformed mask) is recorded for a few pairs.

Stand-ins, written to a temp dir (own code): an empty `cv2` (imported by randaugment.py, used only by operations that are switched
off), and `configs.davis.config` exposing only cfg.DATASET.IGNORE_LABEL / FILL_COLOR -- the real module reads a YAML database file at
import through packages that are absent here.  tests/test_augment_host.py reads only the .npz."""
import argparse
import os
import random
import sys
import tempfile

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
L = 28

STUB_CFG = '''
class _NS:
    pass
cfg = _NS()
cfg.DATASET = _NS()
cfg.DATASET.IGNORE_LABEL = 0
cfg.DATASET.FILL_COLOR = (0, 0, 0)
'''


def install_stubs():
    d = tempfile.mkdtemp(prefix="mumpy_aug_stubs_")
    os.makedirs(os.path.join(d, "configs", "davis"))
    open(os.path.join(d, "cv2.py"), "w").close()
    open(os.path.join(d, "configs", "__init__.py"), "w").close()
    open(os.path.join(d, "configs", "davis", "__init__.py"), "w").close()
    with open(os.path.join(d, "configs", "davis", "config.py"), "w") as f:
        f.write(STUB_CFG)
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    sys.path.insert(0, args.ref)
    sys.path.insert(0, install_stubs())             # in front: the stand-in `configs` wins over the reference's
    import utils.randaugment as RA

    rng = np.random.default_rng(20240)
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

    def pair(m):
        return [Image.fromarray(f) for f in frames], Image.fromarray(m)

    def forced_pscc(p, k):
        real = np.random.randint
        np.random.randint = lambda lo, hi=None, *a, **kw: k
        try:
            return RA.PsccAug(p, 0.5)
        finally:
            np.random.randint = real

    def forced_original_crop(p, v, how):
        real, calls = random.randint, []

        def randint(a, b):
            calls.append((a, b))
            return how if len(calls) == 1 else real(a, b)
        random.randint = randint
        try:
            return RA.OriginalRandomCrop(p, v)
        finally:
            random.randint = real

    def finish(p):                                    # the loader's resize back to the input size + np.asarray
        imgs, m = p
        return (np.stack([np.asarray(i.resize((L, L), Image.NEAREST)) for i in imgs]),
                np.asarray(m.resize((L, L), Image.NEAREST)).copy())

    D4 = {"none": lambda p: p, "hflip": lambda p: RA.HFlip(p, 1), "vflip": lambda p: RA.VFlip(p, 1)}
    for k in range(7):
        D4[f"pscc{k}"] = lambda p, k=k: forced_pscc(p, k)
    CROPS = {"none": lambda p, v: p, "random": RA.RandomCrop, "orig0": lambda p, v: forced_original_crop(p, v, 0),
             "orig1": lambda p, v: forced_original_crop(p, v, 1), "orig2": lambda p, v: forced_original_crop(p, v, 2)}
    cases = [(d, "none", 0, 0.0) for d in D4 if d != "none"]                                  # every D4 operation alone
    cases += [("none", "random", 0, 14.0), ("none", "random", 1, 13.9), ("none", "orig0", 0, 11.0), ("none", "orig1", 0, 20.7),
              ("none", "orig2", 0, 9.0)]                                                      # every crop alone (zero mask: fallback)
    cases += [("pscc1", "random", 0, 14.0), ("pscc3", "random", 0, 14.0), ("pscc5", "random", 0, 14.0), ("vflip", "random", 0, 14.0),
              ("hflip", "orig1", 0, 17.0), ("pscc2", "random", 1, 10.0)]                      # the Double strategy's compositions
    random.seed(7)
    np.random.seed(7)
    rec = dict(d4=[], crop=[], zero_mask=[], v=[], box=[], out_frames=[], out_mask=[])
    for d4, cr, zm, v in cases:
        boxes.clear()
        of, om = finish(CROPS[cr](D4[d4](pair(zero if zm else mask)), v))
        assert (cr == "none") == (not boxes) and len(set(boxes)) <= 1, (d4, cr, boxes)       # one box for every frame and the mask
        rec["d4"].append(d4); rec["crop"].append(cr); rec["zero_mask"].append(zm); rec["v"].append(v)
        rec["box"].append(boxes[0] if boxes else (-1, -1, -1, -1)); rec["out_frames"].append(of); rec["out_mask"].append(om)
    Image.Image.crop = real_crop
    out = os.path.join(args.out, "augment.npz")
    np.savez_compressed(out, frames=frames, mask=mask, d4=np.array(rec["d4"]), crop=np.array(rec["crop"]),
                        zero_mask=np.array(rec["zero_mask"], np.int32), v=np.array(rec["v"], np.float64),
                        box=np.array(rec["box"], np.int32), out_frames=np.stack(rec["out_frames"]), out_mask=np.stack(rec["out_mask"]))
    print(f"wrote {out}: {len(cases)} cases, {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
