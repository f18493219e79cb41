"""CPU only: the host half of the interpolating augmentations of the device-side input stage (mumpy_hip/augment.py,
include/mumpy_hip_ext4.h).

  * cubic_taps, composed into a two-pass resize in numpy, is Pillow's Image.resize(BICUBIC) bit for bit; no position has more than 4
    taps; downscaling is refused;
  * `warp_reference`, the numpy statement of the kernel's three modes written here (tests/test_augment_warp.py holds the kernel to it),
    fed with scale_crop_params reproduces every output recorded from the reference's own RandomScaleCrop
    (tests/golden/augment_warp.npz, written by tests/golden/gen_augment_warp_goldens.py): frames, mask and box;
  * corner_crop_box keeps the reference's bounds; sample_double_full follows its distribution; rotate_params at angle 0 and its range;
  * the header declares exactly the entry and its version function, with the pinned argument names;
  * every refusal of mumpy_augment_warp_u8_fwd, with nothing launched (sign convention of tests/test_abi_refusals.py; needs no GPU and
    must not run where one is visible)."""
import ctypes
import functools
import os

import numpy as np
import pytest
from PIL import Image

from abi_surface import names_of
from conftest import GOLDEN, have_gpu

ENTRY = "mumpy_augment_warp_u8_fwd"
EINVAL, EALIGN, ENULL, ERANGE = -1, -2, -3, -4
GOLDEN_OPS = {"none": "id", "hflip": "hflip", "pscc1": "rot90"}


def A():
    from mumpy_hip import augment
    return augment


# ------------------------------------------------------------------------------------------------ the numpy statement of the kernel
def _clip8(acc):
    return np.clip((acc + (1 << 21)) >> 22, 0, 255)


def warp_reference(src, p, channels_last=False):
    """What mumpy_augment_warp_u8_fwd forms from one source plane stack `src` (..., Hs, Ws[, C]) uint8 under the per-clip record `p`
    (fields of augment.WarpParams) -> (values (..., L, L[, C]) float64, exact) where `exact` says that the values are the 8-bit result
    itself (modes 0, 1 and 3); in mode 2 they are the real-valued blend of the definition, evaluated in double from the float32
    parameters, and the kernel's pixel is floor(value + 0.5)."""
    canvas = A().gather(src, p.tab_a, p.tab_b, p.swap, channels_last=channels_last).astype(np.int64)
    if channels_last:
        canvas = np.moveaxis(canvas, -1, -3)                                   # (..., C, L, L)
    L = canvas.shape[-1]
    mode = int(p.mode) & 3
    if mode == 1:
        rows = np.clip(np.asarray(p.pos_y, np.int64)[:, None] + np.arange(4), 0, L - 1)          # (L, 4)
        cols = np.clip(np.asarray(p.pos_x, np.int64)[:, None] + np.arange(4), 0, L - 1)
        cy, cx = np.asarray(p.coef_y, np.int64), np.asarray(p.coef_x, np.int64)
        acc = 0
        for j in range(4):
            h = sum(cx[:, i][None, :] * canvas[..., rows[:, j], :][..., cols[:, i]] for i in range(4))
            acc = acc + cy[:, j][:, None] * _clip8(h)
        val, exact = _clip8(acc).astype(np.float64), True
    elif mode == 2:
        m = np.asarray(p.affine, np.float32).astype(np.float64)
        u, w = np.asarray(p.pos_x, np.float64)[None, :], np.asarray(p.pos_y, np.float64)[:, None]
        sx, sy = m[0] * u + m[1] * w + m[2], m[3] * u + m[4] * w + m[5]
        x0, y0 = np.floor(sx), np.floor(sy)
        fx, fy = sx - x0, sy - y0

        def corner(dy, dx):
            yy, xx = (y0 + dy).astype(np.int64), (x0 + dx).astype(np.int64)
            inside = (yy >= 0) & (yy <= L - 1) & (xx >= 0) & (xx <= L - 1)
            return np.where(inside, canvas[..., np.clip(yy, 0, L - 1), np.clip(xx, 0, L - 1)], 0).astype(np.float64)
        val = (1 - fy) * ((1 - fx) * corner(0, 0) + fx * corner(0, 1)) + fy * ((1 - fx) * corner(1, 0) + fx * corner(1, 1))
        exact = False
    else:
        val, exact = canvas.astype(np.float64), True
    return (np.moveaxis(val, -3, -1) if channels_last else val), exact


def gather_params(triple, L):
    ta, tb, sw = triple
    return A().WarpParams(ta, tb, sw, np.int32(0), np.zeros(L, np.int32), np.zeros(L, np.int32), np.zeros((L, 4), np.int32),
                          np.zeros((L, 4), np.int32), np.zeros(8, np.float32))


def scale_crop_record(src_hw, L, op, S, box):
    return A().clip_warp_params(src_hw, L, A().FullDraw(op, "RandomScaleCrop", box, S, None))


def rotate_record(src_hw, L, op, angle):
    return A().clip_warp_params(src_hw, L, A().FullDraw(op, "RandomRotate", None, None, angle))


# ------------------------------------------------------------------------------------------------ the cubic against Pillow
def _two_pass(img, n_out):
    """The full resize from cubic_taps alone: horizontal pass, then vertical pass."""
    start, coef = A().cubic_taps(img.shape[0], n_out)
    assert start.dtype == coef.dtype == np.int32 and start.shape == (n_out,) and coef.shape == (n_out, 4)
    idx = np.clip(start.astype(np.int64)[:, None] + np.arange(4), 0, img.shape[0] - 1)
    x = img.astype(np.int64).reshape(img.shape[0], img.shape[1], -1)
    horiz = _clip8(sum(coef[:, k].astype(np.int64)[None, :, None] * x[:, idx[:, k]] for k in range(4)))
    vert = _clip8(sum(coef[:, k].astype(np.int64)[:, None, None] * horiz[idx[:, k]] for k in range(4)))
    return vert.astype(np.uint8).reshape((n_out, n_out) + img.shape[2:])


@pytest.mark.parametrize("n_in,n_out", [(28, 28), (28, 29), (28, 57), (28, 128), (224, 256), (224, 1024)])
def test_cubic_taps_are_pillows_bicubic_bit_for_bit(n_in, n_out):
    g = np.random.default_rng(n_in * 10000 + n_out)
    for img in (g.integers(0, 256, (n_in, n_in, 3), dtype=np.uint8), g.integers(0, 256, (n_in, n_in), dtype=np.uint8),
                g.choice(np.array([0, 255], np.uint8), (n_in, n_in))):                       # RGB, L, and L at full contrast (ringing)
        ref = np.asarray(Image.fromarray(img).resize((n_out, n_out), Image.BICUBIC))
        assert np.array_equal(_two_pass(img, n_out), ref)
        assert np.array_equal(A().cubic_resize(img, (n_out, n_out)), ref)
    start, coef = A().cubic_taps(n_in, n_out)
    # no more than 4 taps: Pillow's own bounds never span more
    center = (np.arange(n_out) + 0.5) * n_in / n_out
    lo, hi = np.maximum((center - 1.5).astype(np.int64), 0), np.minimum((center + 2.5).astype(np.int64), n_in)
    assert int((hi - lo).max()) <= 4 and np.array_equal(start, lo)
    assert all((coef[i, hi[i] - lo[i]:] == 0).all() for i in range(n_out))                  # a dropped tap is a zero coefficient
    assert int(np.abs(coef.astype(np.int64)).sum(axis=1).max()) * 255 < 2 ** 31             # the 32-bit sums of the kernel fit


def test_downscaling_cubic_is_refused():
    for n_in, n_out in ((28, 27), (224, 112), (2, 1)):
        with pytest.raises(ValueError):
            A().cubic_taps(n_in, n_out)
    with pytest.raises(ValueError):
        A().scale_crop_params(28, 27)


# ------------------------------------------------------------------------------------------------ the reference's recorded outputs
@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(GOLDEN, "augment_warp.npz"))


def golden_cases():
    """[(record, mask (28, 28), out_frames (3, 28, 28, 3), out_mask (28, 28))] of the recorded cases."""
    g = golden()
    out = []
    for i in range(len(g["d4"])):
        box = None if g["zero_mask"][i] else tuple(int(v) for v in g["box"][i])
        rec = scale_crop_record((28, 28), 28, GOLDEN_OPS[str(g["d4"][i])], int(g["S"][i]), box)
        out.append((rec, np.zeros_like(g["mask"]) if g["zero_mask"][i] else g["mask"], g["out_frames"][i], g["out_mask"][i]))
    return out


def test_scale_crop_params_reproduce_the_references_recorded_outputs():
    g = golden()
    assert sorted(zip(g["S"].tolist(), g["zero_mask"].tolist(), g["d4"].tolist())) == sorted(
        [(32, 0, "none"), (57, 0, "none"), (100, 0, "none"), (64, 1, "none"), (57, 0, "pscc1"), (100, 0, "hflip")])
    ringing = []
    for i, (rec, mask, out_frames, out_mask) in enumerate(golden_cases()):
        assert int(rec.mode) == 1
        got, exact = warp_reference(g["frames"], rec, channels_last=True)
        assert exact and np.array_equal(got, out_frames), i
        got, _ = warp_reference(mask, rec)
        assert np.array_equal(got, out_mask), i
        # the recorded box is one the restated draw can produce from the same upscaled mask
        op, S = GOLDEN_OPS[str(g["d4"][i])], int(g["S"][i])
        cm = A().canvas_mask(mask, *A().clip_tables((28, 28), 28, op))
        up = A().upscaled_mask(cm, S)
        assert np.array_equal(up, np.asarray(Image.fromarray(cm).resize((S, S), Image.BICUBIC)))
        corners = A().find_corners(up)
        assert corners == A().upscaled_corners(cm, S)
        if g["zero_mask"][i]:
            assert corners is None and A().corner_crop_box(up, np.random.default_rng(0)) is None
            assert not out_mask.any()
            continue
        left, top, right, bottom = corners
        l, t, r, b = (int(v) for v in g["box"][i])
        assert l in (range(0, left - 1) if left > 1 else (0,)) and t in (range(0, top - 1) if top > 1 else (0,))
        assert r in (range(right + 1, S - 1) if right + 1 < S - 1 else (S - 1,))
        assert b in (range(bottom + 1, S - 1) if bottom + 1 < S - 1 else (S - 1,))
        ringing.append(int((out_mask > 0).sum()))
    assert min(ringing) > int((g["mask"] > 0).sum())           # the cubic's ringing is part of the target: more positives than the mask has


def test_upscaled_corners_need_no_full_upscale():
    g = np.random.default_rng(8)
    for k in range(12):
        cm = ((g.random((28, 28)) < (0.0, 0.01, 0.05)[k % 3]) * g.integers(1, 256, (28, 28))).astype(np.uint8)
        for S in (28, 29, 57, 128):
            assert A().upscaled_corners(cm, S) == A().find_corners(A().upscaled_mask(cm, S)), (k, S)


# ------------------------------------------------------------------------------------------------ the samplers
def test_corner_crop_box_stays_inside_the_references_bounds():
    rng = np.random.default_rng(31)
    for trial in range(1000):
        S = int(rng.integers(8, 80))
        up = np.zeros((S, S), np.uint8)
        y0, x0 = (int(v) for v in rng.integers(0, S, 2))
        y1, x1 = int(rng.integers(y0, S)), int(rng.integers(x0, S))
        up[y0, x0] = up[y1, x1] = 1 + trial % 255
        left, top, right, bottom = x0 - 1, y0 - 1, x1 + 1, y1 + 1
        assert A().find_corners(up) == (left, top, right, bottom)
        l, t, r, b = A().check_box(A().corner_crop_box(up, rng), S)
        assert l in (range(0, left - 1) if left > 1 else (0,)) and t in (range(0, top - 1) if top > 1 else (0,))
        assert r in (range(right + 1, S - 1) if right + 1 < S - 1 else (S - 1,))
        assert b in (range(bottom + 1, S - 1) if bottom + 1 < S - 1 else (S - 1,))
    assert A().corner_crop_box(np.zeros((9, 9), np.uint8), rng) is None


def test_sample_double_full_follows_the_references_distribution():
    n, L, src = 4000, 224, (30, 54)
    rng = np.random.default_rng(77)
    mask = np.zeros(src, np.uint8)
    mask[8:17, 12:38] = 255
    counts, angles, sides = dict.fromkeys(A().SHAPE_LIST, 0), set(), set()
    for k in range(n):
        d = A().sample_double_full(rng, src, L, mask)
        counts[d.shape] += 1
        assert d.op in A().OPS and d.op != "rot270+tb"
        if d.shape == "RandomRotate":
            assert d.angle != 180 and 20 <= d.angle <= 219 and d.box is None and d.S is None
            angles.add(d.angle)
        elif d.shape == "RandomScaleCrop":
            assert 256 <= d.S <= 1024 and d.box is not None and d.angle is None
            A().check_box(d.box, d.S)
            sides.add(d.S)
        else:
            A().check_box(d.box, L)
        if k % 40 == 0:                                         # the record -> kernel rows, for every kind of draw
            p = A().clip_warp_params(src, L, d)
            assert int(p.mode) == {"RandomScaleCrop": 1, "RandomRotate": 2}.get(d.shape, 0)
            assert p.pos_y.shape == p.pos_x.shape == (L,) and p.coef_y.shape == p.coef_x.shape == (L, 4) and p.affine.shape == (8,)
            assert all(a.dtype == np.int32 for a in p[:8]) and p.affine.dtype == np.float32
    sigma = (n * 0.25 * 0.75) ** 0.5
    assert all(abs(c - n / 4) <= 4.0 * sigma for c in counts.values()), counts
    assert {179, 181} <= angles and min(sides) < 300 and max(sides) > 980
    with pytest.raises(NotImplementedError):                     # the older sampler keeps refusing the whole list
        A().sample_double(rng, src, L)
    empty = A().sample_double_full(np.random.default_rng(3), src, L, None)
    assert empty.shape in A().SHAPE_LIST


def test_rotate_params_identity_range_and_crop():
    for L in (28, 36, 224):
        pos_y, pos_x, aff = A().rotate_params(L, 0)
        assert np.array_equal(pos_y, np.arange(L)) and np.array_equal(pos_x, np.arange(L))          # the full canvas
        assert np.array_equal(aff, np.array([1, 0, 0, 0, 1, 0, 0, 0], np.float32))                  # the identity map
        for angle in range(180):
            pos_y, pos_x, aff = A().rotate_params(L, angle)
            assert np.isfinite(aff).all() and pos_y.dtype == pos_x.dtype == np.int32 and aff.dtype == np.float32
            assert 0 <= pos_y.min() and pos_y.max() <= L - 1 and np.array_equal(pos_y, pos_x)
            # randaugment.py:441-460 in its own words
            ac = angle % 180
            if angle > 90:
                ac = 180 - ac
            th = ac * np.pi / 180
            side = int((np.cos(th) + np.sin(th) * np.tan(th)) / (np.tan(th) + 1) * L)
            x0 = int((L - side) / 2)
            assert pos_x[0] == x0 and pos_x[-1] == x0 + A().nearest_table(side, L)[-1] and pos_x[-1] <= x0 + side - 1
            c, t = L / 2, np.deg2rad(angle)
            want = [np.cos(t), -np.sin(t), c - np.cos(t) * c + np.sin(t) * c, np.sin(t), np.cos(t), c - np.sin(t) * c - np.cos(t) * c]
            assert np.allclose(aff[:6], want, rtol=2.0 ** -23, atol=1e-7) and not aff[6:].any()           # float32 of the double value
    # a quarter turn maps the centre to itself and (c + 1, c) to (c, c + 1)
    _, _, aff = A().rotate_params(28, 90)
    m = aff[:6].astype(np.float64).reshape(2, 3)
    assert np.allclose(m @ [14, 14, 1], [14, 14], atol=1e-5) and np.allclose(m @ [15, 14, 1], [14, 15], atol=1e-5)


# ------------------------------------------------------------------------------------------------ the header's pinned names
def test_ext4_header_declares_exactly_the_pinned_names():
    """(tests/test_abi.py holds the header to its binding and to both libraries.)"""
    assert names_of("mumpy_hip_ext4.h") == {"mumpy_ext4_version": [], ENTRY: [
        "frames", "masks", "out", "target", "tab_a", "tab_b", "swap", "mode", "pos_y", "pos_x", "coef_y", "coef_x", "affine", "nclips",
        "T", "nmasks", "Hs", "Ws", "L", "mean3", "std3", "stream"]}


# ------------------------------------------------------------------------------------------------ refusals, without a GPU
@pytest.mark.skipif(have_gpu(), reason="with a device present a valid tuple of fake addresses would really launch")
def test_refusals_need_no_gpu():
    """A valid tuple of fake, 16-byte aligned, never dereferenced addresses passes every host check (rc > 0: the launch reaches a
    runtime without a device); the same tuple with one rule broken is refused (rc < 0) with the stated code and a message of this
    call's own.  mean3 / std3 are real host arrays: the entry reads them."""
    from mumpy_hip.lib import load_library
    lib = load_library()
    fn = getattr(lib, ENTRY)
    ptrs = ["frames", "masks", "out", "target", "tab_a", "tab_b", "swap", "mode", "pos_y", "pos_x", "coef_y", "coef_x", "affine"]
    names = ptrs + ["nclips", "T", "nmasks", "Hs", "Ws", "L", "mean3", "std3", "stream"]
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    z3 = (ctypes.c_float * 3)(0.5, 0.0, 0.5)
    ok = dict(zip(names, [0x100000 * (i + 1) for i in range(len(ptrs))] + [6, 2, 2, 5, 7, 8, f3, f3, None]))
    nomask = dict(ok, masks=None, target=None)

    def call(base, **over):
        a = dict(base, **over)
        return int(fn(*[a[k] for k in names]))

    def refused(code, base=ok, **over):
        assert lib.mumpy_add_fwd(None, None, None, 16, None) < 0        # the message is sticky per thread: leave a known one
        stale = lib.mumpy_last_error()
        rc = call(base, **over)
        err = lib.mumpy_last_error()
        assert rc == code and err != stale and b"augment_warp_u8" in err, (over, rc, err)

    assert call(ok) > 0 and call(nomask) > 0
    assert call(nomask, nmasks=0) > 0 and call(nomask, nmasks=-5) > 0    # without masks nmasks is ignored
    assert call(ok, nclips=0) == 0 and call(nomask, nclips=0) == 0       # the accepted no-op
    for p in set(ptrs) - {"masks", "target"} | {"mean3", "std3"}:
        refused(ENULL, **{p: None})
    refused(ENULL, masks=None)                                           # exactly one of masks / target
    refused(ENULL, target=None)
    for k, v in (("T", 0), ("T", -1), ("Hs", 0), ("Ws", 0), ("Hs", -1), ("Ws", -1), ("L", 0), ("L", 2), ("L", 6), ("L", 9), ("L", -4),
                 ("nclips", -1), ("nmasks", 0), ("nmasks", -1), ("nmasks", 4), ("std3", z3)):
        refused(EINVAL, **{k: v})
    for p in ("out", "target", "tab_a", "tab_b", "pos_y", "pos_x", "coef_y", "coef_x"):
        refused(EALIGN, **{p: ok[p] + 4})
    assert call(ok, frames=ok["frames"] + 1, masks=ok["masks"] + 1, swap=ok["swap"] + 4, mode=ok["mode"] + 4,
                affine=ok["affine"] + 4) > 0                             # bytes / single words: no alignment rule
    refused(ERANGE, nclips=1 << 31, nmasks=1)                            # the frame index
    refused(ERANGE, nclips=1 << 30, nmasks=1)                            # nclips * T = 2^31
    refused(ERANGE, nclips=1 << 62, nmasks=1)
    refused(ERANGE, Hs=26755, Ws=26755)                                  # 3 * Hs * Ws >= 2^31
    refused(ERANGE, L=26756)                                             # 3 * L * L >= 2^31
    assert call(ok, Hs=26754, Ws=26754) > 0 and call(ok, nclips=(1 << 30) - 2) > 0                  # just inside
