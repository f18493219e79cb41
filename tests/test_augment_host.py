"""CPU only: the host half of the device-side training input stage (mumpy_hip/augment.py, include/mumpy_hip_ext3.h).

  * clip_tables against Pillow itself: an id-image (the pixel's index packed into RGB, so a wrong pick always shows) goes through
    resize(NEAREST) -> ImageOps.mirror / flip / rotate(90k, expand=True) / transpose(FLIP_TOP_BOTTOM) -> crop -> resize(NEAREST) and
    must equal the gather through the tables exactly;
  * the tables reproduce every output recorded from the reference's own HFlip / VFlip / PsccAug / RandomCrop / OriginalRandomCrop
    (tests/golden/augment.npz, written by tests/golden/gen_augment_goldens.py);
  * the samplers follow the reference's distributions (5 standard deviations of the binomial over 70,000 seeded draws) and the box
    contract;
  * the header declares the entry with the pinned argument names;
  * every refusal of mumpy_augment_stage_u8_fwd, with nothing launched (sign convention of tests/test_abi_refusals.py; needs no GPU and
    must not run where one is visible)."""
import ctypes
import functools
import os

import numpy as np
import pytest
from PIL import Image, ImageOps

from abi_surface import names_of
from conftest import GOLDEN, have_gpu

ENTRY = "mumpy_augment_stage_u8_fwd"
EINVAL, EALIGN, ENULL, ERANGE = -1, -2, -3, -4
SOURCES = [(37, 50), (240, 432), (28, 28), (300, 301)]          # (Hs, Ws)
SIDES = [28, 224]


def A():
    from mumpy_hip import augment
    return augment


# ------------------------------------------------------------------------------------------------ clip_tables against Pillow
def _id_image(hs, ws):
    idx = np.arange(hs * ws, dtype=np.uint32).reshape(hs, ws)
    return np.stack([idx & 255, (idx >> 8) & 255, (idx >> 16) & 255], -1).astype(np.uint8)


def _pil_op(img, op):
    """The reference's own calls (randaugment.py:113-127, 515-539)."""
    if op == "id":
        return img
    if op == "hflip":
        return ImageOps.mirror(img)
    if op == "vflip":
        return ImageOps.flip(img)
    k, tb = {"rot90": (90, False), "rot180": (180, False), "rot270": (270, False), "rot90+tb": (90, True), "rot270+tb": (270, True)}[op]
    img = img.rotate(k, expand=True)
    return img.transpose(Image.FLIP_TOP_BOTTOM) if tb else img


def _boxes(L):
    return [None, (L // 4, L // 7, L - L // 5, L - L // 3), (0, L // 2, L - 3, L), (L // 2, L // 3, L // 2 + 5, L // 3 + 3)]


@pytest.mark.parametrize("L", SIDES)
@pytest.mark.parametrize("src", SOURCES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_clip_tables_are_pillows_pipeline(src, L):
    """8 operations x {no box, interior box, box touching two edges, 5 x 3 box}: exact equality with Pillow."""
    hs, ws = src
    ident = _id_image(hs, ws)
    canvas = Image.fromarray(ident).resize((L, L), Image.NEAREST)
    assert len(A().OPS) == 8
    for op in A().OPS:
        moved = _pil_op(canvas, op)
        assert moved.size == (L, L)
        for box in _boxes(L):
            ref = moved if box is None else moved.crop(box)
            ref = np.asarray(ref.resize((L, L), Image.NEAREST))
            ta, tb, sw = A().clip_tables(src, L, op, box)
            assert ta.dtype == tb.dtype == np.int32 and ta.shape == tb.shape == (L,) and int(sw) in (0, 1)
            assert 0 <= ta.min() and ta.max() < hs and 0 <= tb.min() and tb.max() < ws
            got = A().gather(ident, ta, tb, sw, channels_last=True)
            assert np.array_equal(got, ref), (op, box)


def test_psccaug_six_is_the_mirror_and_the_box_contract_is_enforced():
    """rotate(180) + FLIP_TOP_BOTTOM (PsccAug 6) is ImageOps.mirror: one table entry serves both."""
    img = Image.fromarray(_id_image(28, 28))
    six = img.rotate(180, expand=True).transpose(Image.FLIP_TOP_BOTTOM)
    assert np.array_equal(np.asarray(six), np.asarray(ImageOps.mirror(img))) and A().PSCC_OPS[6] == "hflip"
    assert A().PSCC_OPS[:6] == ("id", "rot90", "rot180", "rot270", "vflip", "rot90+tb") and A().PSCC_OPS[7] == "rot270+tb"
    for bad in [(-1, 0, 5, 5), (0, 0, 29, 5), (5, 0, 5, 5), (6, 0, 5, 5), (0, 9, 5, 9), (0, 0, 5, 29), (0, -1, 5, 5)]:
        with pytest.raises(ValueError):
            A().clip_tables((28, 28), 28, "id", bad)
    with pytest.raises(ValueError):
        A().clip_tables((28, 28), 28, "rot45")


# ------------------------------------------------------------------------------------------------ the reference's recorded outputs
@functools.lru_cache(maxsize=None)
def _golden():
    return np.load(os.path.join(GOLDEN, "augment.npz"))


def _golden_op(name):
    return "id" if name == "none" else (A().PSCC_OPS[int(name[4:])] if name.startswith("pscc") else name)


def test_tables_reproduce_the_references_recorded_outputs():
    g = _golden()
    n = len(g["d4"])
    assert n >= 20 and {f"pscc{k}" for k in range(7)} | {"hflip", "vflip"} <= set(g["d4"].tolist())
    assert {"random", "orig0", "orig1", "orig2"} <= set(g["crop"].tolist())
    assert any(g["zero_mask"][i] and g["crop"][i] == "random" for i in range(n))                 # RandomCrop's empty-mask fallback
    for i in range(n):
        op, crop = _golden_op(str(g["d4"][i])), str(g["crop"][i])
        box = None if crop == "none" else tuple(int(v) for v in g["box"][i])
        mask = np.zeros_like(g["mask"]) if g["zero_mask"][i] else g["mask"]
        t = A().clip_tables((28, 28), 28, op, box)
        assert np.array_equal(A().gather(g["frames"], *t, channels_last=True), g["out_frames"][i]), (i, op, crop, box)
        assert np.array_equal(A().gather(mask, *t), g["out_mask"][i]), (i, op, crop, box)
        if crop == "none":
            continue
        # the recorded box is one the restated draw can produce from the same transformed mask
        l, tp, r, b = box
        corners = A().find_corners(A().canvas_mask(mask, *A().clip_tables((28, 28), 28, op)))
        if crop != "random" or corners is None:
            side = int(g["v"][i])
            assert (r - l, b - tp) == (side, side) and 0 <= l and 0 <= tp and r <= 28 and b <= 28
            if crop == "orig2":
                assert (l, tp) == ((28 - side) // 2, (28 - side) // 2)
        else:
            left, top, right, bottom = corners
            assert l in (range(0, left - 1) if left > 1 else (0,)) and tp in (range(0, top - 1) if top > 1 else (0,))
            assert r in (range(right + 1, 27) if right + 1 < 27 else (27,)) and b in (range(bottom + 1, 27) if bottom + 1 < 27 else (27,))


# ------------------------------------------------------------------------------------------------ the samplers
def _within_5_sigma(count, n, p):
    return abs(count - n * p) <= 5.0 * (n * p * (1.0 - p)) ** 0.5


def test_sample_single_follows_the_references_distribution():
    n = 70000
    rng = np.random.default_rng(12345)
    entries, pscc = np.zeros(7, np.int64), np.zeros(8, np.int64)
    for _ in range(n):
        d = A().sample_single(rng)
        entries[d.entry] += 1
        assert d.op in A().OPS
        if d.entry == 6:
            pscc[d.pscc] += 1
            assert d.op == A().PSCC_OPS[d.pscc]
        else:
            assert d.pscc is None and d.op == ("id" if d.entry < 4 else ("hflip", "vflip")[d.entry - 4])
    assert all(_within_5_sigma(int(c), n, 1 / 7) for c in entries), entries
    assert pscc[7] == 0 and all(_within_5_sigma(int(c), n, 1 / 49) for c in pscc[:7]), pscc


def test_crop_boxes_keep_the_contract_and_contain_the_mask():
    """Masks whose bounding box stays off the last row and column: like the reference, RandomCrop's right / bottom side is exclusive
    and never beyond L - 1, so a mask touching the last column loses it (restated faithfully, not tested as containment)."""
    rng = np.random.default_rng(99)
    for L in (28, 224):
        for trial in range(300):
            y0, x0 = (int(v) for v in rng.integers(0, L - 2, 2))
            y1, x1 = int(rng.integers(y0, L - 1)), int(rng.integers(x0, L - 1))               # inclusive corners, <= L - 2
            cm = np.zeros((L, L), np.uint8)
            cm[y0, x0] = cm[y1, x1] = 255
            l, t, r, b = A().check_box(A().random_crop_box(cm, 0.0, L, rng), L)
            assert l <= x0 and x1 < r and t <= y0 and y1 < b, ((y0, x0, y1, x1), (l, t, r, b))
            v = float(rng.uniform(1.0, L - 1))
            for box in (A().original_random_crop_box(v, L, rng), A().random_crop_box(np.zeros((L, L), np.uint8), v, L, rng)):
                l, t, r, b = A().check_box(box, L)
                assert r - l == b - t == int(v)
    with pytest.raises(ValueError):
        A().original_random_crop_box(28.0, 28, rng)                  # the reference's own randint(crop, w - 1) has no value then


def test_double_strategy_is_refused_whole_and_runs_restricted_to_the_crops():
    rng = np.random.default_rng(5)
    with pytest.raises(NotImplementedError) as e:
        A().sample_double(rng, (240, 432), 224)
    assert "RandomRotate" in str(e.value) and "RandomScaleCrop" in str(e.value)
    with pytest.raises(NotImplementedError):
        A().sample_double(rng, (240, 432), 224, shape_ops=("RandomCrop", "RandomRotate"))
    mask = np.zeros((240, 432), np.uint8)
    mask[60:130, 100:300] = 1
    seen = set()
    for _ in range(200):
        op, box = A().sample_double(rng, (240, 432), 224, mask, shape_ops=("RandomCrop", "OriginalRandomCrop"))
        assert op in A().OPS and op != "rot270+tb"                   # PsccAug 0 is the identity; index 7 is never drawn
        A().check_box(box, 224)
        seen.add(op)
    assert seen == set(A().OPS) - {"rot270+tb"}


# ------------------------------------------------------------------------------------------------ the header's pinned names
def test_ext3_header_declares_the_pinned_argument_names():
    """(tests/test_abi.py holds the header to its binding and to both libraries.)"""
    ext3 = names_of("mumpy_hip_ext3.h")
    assert "mumpy_ext3_version" in ext3
    assert ext3[ENTRY] == ["frames", "masks", "out", "target", "tab_a", "tab_b", "swap", "nclips", "T", "nmasks", "Hs", "Ws", "L", "mean3",
                           "std3", "stream"]


# ------------------------------------------------------------------------------------------------ refusals, without a GPU
@pytest.mark.skipif(have_gpu(), reason="with a device present a valid tuple of fake addresses would really launch")
def test_refusals_need_no_gpu():
    """A valid tuple of fake, 16-byte aligned, never dereferenced addresses passes every host check (rc > 0: the launch reaches a
    runtime without a device); the same tuple with one rule broken is refused (rc < 0) with the stated code and a message of this
    call's own.  mean3 / std3 are real host arrays: the entry reads them."""
    from mumpy_hip.lib import load_library
    lib = load_library()
    fn = getattr(lib, ENTRY)
    P = [0x100000 * (i + 1) for i in range(7)]
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    z3 = (ctypes.c_float * 3)(0.5, 0.0, 0.5)
    names = ["frames", "masks", "out", "target", "tab_a", "tab_b", "swap", "nclips", "T", "nmasks", "Hs", "Ws", "L", "mean3", "std3", "stream"]
    ok = dict(zip(names, (P[0], P[1], P[2], P[3], P[4], P[5], P[6], 6, 2, 2, 5, 7, 8, f3, f3, None)))
    nomask = dict(ok, masks=None, target=None)

    def call(base, **over):
        a = dict(base, **over)
        return int(fn(*[a[k] for k in names]))

    def refused(code, base=ok, **over):
        assert lib.mumpy_add_fwd(None, None, None, 16, None) < 0        # the message is sticky per thread: leave a known one
        stale = lib.mumpy_last_error()
        rc = call(base, **over)
        err = lib.mumpy_last_error()
        assert rc == code and err != stale and b"augment_stage_u8" in err, (over, rc, err)

    assert call(ok) > 0 and call(nomask) > 0
    assert call(nomask, nmasks=0) > 0 and call(nomask, nmasks=-5) > 0    # without masks nmasks is ignored
    assert call(ok, nclips=0) == 0 and call(nomask, nclips=0) == 0       # the accepted no-op
    for p in ("frames", "out", "tab_a", "tab_b", "swap", "mean3", "std3"):
        refused(ENULL, **{p: None})
    refused(ENULL, masks=None)                                           # exactly one of masks / target
    refused(ENULL, target=None)
    for k, v in (("T", 0), ("T", -1), ("Hs", 0), ("Ws", 0), ("Hs", -1), ("Ws", -1), ("L", 0), ("L", 2), ("L", 6), ("L", 9), ("L", -4),
                 ("nclips", -1), ("nmasks", 0), ("nmasks", -1), ("nmasks", 4), ("std3", z3)):
        refused(EINVAL, **{k: v})
    for p in ("out", "target", "tab_a", "tab_b"):
        refused(EALIGN, **{p: ok[p] + 4})
    assert call(ok, frames=ok["frames"] + 1, masks=ok["masks"] + 1, swap=ok["swap"] + 4) > 0        # bytes / words: no alignment rule
    refused(ERANGE, nclips=1 << 31, nmasks=1)                            # the frame index
    refused(ERANGE, nclips=1 << 30, nmasks=1)                            # nclips * T = 2^31
    refused(ERANGE, nclips=1 << 62, nmasks=1)
    refused(ERANGE, Hs=26755, Ws=26755)                                  # 3 * Hs * Ws >= 2^31
    refused(ERANGE, L=26756)                                             # 3 * L * L >= 2^31
    assert call(ok, Hs=26754, Ws=26754) > 0 and call(ok, nclips=(1 << 30) - 2) > 0                  # just inside
