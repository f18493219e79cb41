"""CPU only: the host half of scoring against native-size annotations (mumpy_hip/video.py::bilinear_taps / bilinear_resize,
include/mumpy_hip_ext6.h).

  * `bilinear_resize`, the numpy statement of the kernel, IS Pillow's Image.resize(BILINEAR) of an 8-bit image: zero differing bytes
    on downscales from 1.07 x to 8.6 x, upscales, the identity, ragged and per-axis different ratios, for random bytes, a sparse
    0 / 255 mask (every byte at a mask edge) and a block of a single small value (the rounding around 0 that `> 0` then sees);
  * the taps stay inside the source, fit their table, and their fixed-point weights sum to 1 within one unit per tap;
  * the header declares exactly the entry and its version function, with the pinned argument names and limits;
  * every refusal named in the header, with nothing launched (sign convention of tests/test_abi_refusals.py: needs no GPU and must
    not run where one is visible; tests/test_annot_resize.py runs the same table against real buffers)."""

import numpy as np
import pytest

from abi_surface import define, names_of
from conftest import have_gpu

EINVAL, EALIGN, ENULL, ERANGE = -1, -2, -3, -4
ENTRY = "mumpy_resize_bilinear_u8_fwd"
ARGS = ["src", "out", "ystart", "ycount", "ycoef", "xstart", "xcount", "xcoef", "n", "Hs", "Ws", "H", "W", "ykmax", "xkmax", "stream"]
POINTERS = ARGS[:8]
TABLES = ARGS[2:8]
KMAX_CAP, BAND_BYTES = 65, 49152

SIZES = [((240, 432), (224, 224)), ((480, 854), (224, 224)), ((720, 1280), (224, 224)), ((1080, 1920), (224, 224)),
         ((224, 224), (224, 224)), ((224, 300), (224, 224)), ((100, 150), (224, 224)), ((225, 223), (224, 224)), ((7, 5), (224, 224)),
         ((37, 53), (16, 32))]
KINDS = ["random", "mask", "block"]


def V():
    from mumpy_hip import video
    return video


def annotation(kind, hw, seed):
    """A test image (H, W) uint8: random bytes; a 2 %-dense 0 / 255 mask; a block of one value in 1 .. 3 on zeros."""
    g = np.random.default_rng(seed)
    h, w = hw
    if kind == "random":
        return g.integers(0, 256, (h, w), dtype=np.uint8)
    if kind == "mask":
        return ((g.random((h, w)) < 0.02) * 255).astype(np.uint8)
    a = np.zeros((h, w), np.uint8)
    a[h // 4:h // 2 + 1, w // 3:w // 2 + 1] = 1 + seed % 3
    return a


def pil_resize(img, out_hw):
    from PIL import Image
    return np.array(Image.fromarray(img).resize((out_hw[1], out_hw[0]), Image.BILINEAR))


# ------------------------------------------------------------------------------------------------ the resize is Pillow's
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("src,dst", SIZES, ids=[f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in SIZES])
def test_bilinear_resize_is_pillows_bit_for_bit(src, dst, kind):
    img = annotation(kind, src, seed=src[0] + src[1] + KINDS.index(kind))
    assert img.any()
    got, want = V().bilinear_resize(img, dst), pil_resize(img, dst)
    assert got.dtype == np.uint8 and got.shape == want.shape == dst
    assert int((got != want).sum()) == 0, f"{int((got != want).sum())} of {got.size} bytes differ from Image.resize(BILINEAR)"


def test_bilinear_resize_of_a_stack_is_per_image():
    imgs = np.stack([annotation(k, (37, 53), seed=i) for i, k in enumerate(KINDS)])
    got = V().bilinear_resize(imgs, (16, 32))
    assert got.shape == (3, 16, 32) and all(np.array_equal(got[i], pil_resize(imgs[i], (16, 32))) for i in range(3))
    with pytest.raises(ValueError):
        V().bilinear_resize(imgs.astype(np.float32), (16, 32))


# ------------------------------------------------------------------------------------------------ the taps
@pytest.mark.parametrize("n_in,n_out", [(1080, 224), (1920, 224), (854, 224), (4320, 224), (432, 224), (225, 224), (223, 224),
                                        (5, 224), (7, 16), (53, 32), (1, 7), (9, 1), (224, 224), (1, 1)])
def test_tap_properties(n_in, n_out):
    start, count, coef = V().bilinear_taps(n_in, n_out)
    ksize = 2 * int(np.ceil(max(n_in / n_out, 1.0))) + 1
    assert start.dtype == count.dtype == coef.dtype == np.int32
    assert start.shape == count.shape == (n_out,) and coef.shape == (n_out, ksize)
    assert (start >= 0).all() and (count >= 1).all() and (start.astype(np.int64) + count <= n_in).all() and (count <= ksize).all()
    assert (coef >= 0).all()                                         # the triangle filter has no negative lobe
    assert all((coef[i, count[i]:] == 0).all() for i in range(n_out))
    assert (np.abs(coef.astype(np.int64).sum(1) - (1 << 22)) <= count).all()      # each weight is rounded once: half a unit per tap
    assert (np.diff(start) >= 0).all()                              # the bands of the kernel rely on it: later rows read later rows
    if n_in == n_out:
        assert np.array_equal(start, np.arange(n_in)) and (coef[:, 0] == 1 << 22).all() and (coef[:, 1:] == 0).all()


def test_the_kernels_cap_covers_4320_pixel_sources():
    assert V().bilinear_taps(4320, 224)[2].shape[1] == 41 <= KMAX_CAP
    assert V().bilinear_taps(V().GT_MAX_RATIO * 224, 224)[2].shape[1] == KMAX_CAP
    for bad in ((0, 5), (5, 0), (-1, 5)):
        with pytest.raises(ValueError):
            V().bilinear_taps(*bad)


# ------------------------------------------------------------------------------------------------ the header's pinned names and limits
def test_ext6_header_declares_exactly_the_pinned_names_and_limits():
    """(tests/test_abi.py holds the header to its binding and to both libraries.)"""
    assert names_of("mumpy_hip_ext6.h") == {ENTRY: ARGS, "mumpy_ext6_version": []}
    assert define("mumpy_hip_ext6.h", "MUMPY_RESIZE_KMAX_CAP") == KMAX_CAP
    assert define("mumpy_hip_ext6.h", "MUMPY_RESIZE_BAND_BYTES") == BAND_BYTES


# ------------------------------------------------------------------------------------------------ refusals
OFF = lambda k: ("off", k)           # the valid pointer moved by k bytes
VALID = dict(n=2, Hs=5, Ws=7, H=8, W=8, ykmax=3, xkmax=3, stream=None)
ALSO_VALID = [dict(src=OFF(1), out=OFF(3)),                          # bytes: no alignment rule
              dict(ykmax=KMAX_CAP, xkmax=KMAX_CAP), dict(ykmax=1, xkmax=1),
              dict(Hs=1000, ykmax=3, W=BAND_BYTES // 4),             # the widest band that fits
              dict(Hs=2, ykmax=41, W=BAND_BYTES // 2)]               # ... a short source needs no more rows than it has
NOOPS = [dict(n=0)]
REFUSED = ([(ENULL, {p: None}) for p in POINTERS]
           + [(EINVAL, {k: v}) for k, v in (("Hs", 0), ("Hs", -1), ("Ws", 0), ("Ws", -3), ("H", 0), ("H", -1), ("W", 0), ("W", -4), ("n", -1),
                                            ("ykmax", 0), ("ykmax", -1), ("ykmax", KMAX_CAP + 1), ("xkmax", 0), ("xkmax", KMAX_CAP + 1))]
           + [(EINVAL, dict(Hs=1000, ykmax=3, W=BAND_BYTES // 4 + 1)), (EINVAL, dict(Hs=2, ykmax=41, W=BAND_BYTES // 2 + 1))]
           + [(EALIGN, {p: OFF(2)}) for p in TABLES]
           + [(ERANGE, {"n": 1 << 31}), (ERANGE, {"n": 1 << 62}), (ERANGE, {"n": 1 << 28}),          # n * H = 2^31
              (ERANGE, {"Hs": 46341, "Ws": 46341}), (ERANGE, {"H": 46341, "W": 46341}), (ERANGE, {"H": (1 << 31) - 1, "W": 1}),
              (ERANGE, {"W": (1 << 31) - 1, "H": 1})])


def sweep_refusals(lib, pointers, launches, before_refusals=None):
    """pointers: {name: address} of the entry's device pointers.  launches: True where a valid call really runs (rc == 0), False where
    it reaches a runtime without a device (rc > 0).  Every refusal must give its code and a message of this call's own.
    before_refusals(): called between the valid calls and the refused ones."""
    fn = getattr(lib, ENTRY)
    ok = dict(pointers, **VALID)
    assert set(ok) == set(ARGS)

    def call(over):
        a = dict(ok)
        for k, v in over.items():
            a[k] = ok[k] + v[1] if isinstance(v, tuple) else v
        return int(fn(*[a[k] for k in ARGS]))

    for over in [{}] + ALSO_VALID:
        rc = call(over)
        assert (rc == 0) if launches else (rc > 0), (over, rc, lib.mumpy_last_error())
    if before_refusals is not None:
        before_refusals()
    for over in NOOPS:
        assert call(over) == 0, over
    for code, over in REFUSED:
        assert lib.mumpy_add_fwd(None, None, None, 16, None) < 0        # the message is sticky per thread: leave a known one
        stale = lib.mumpy_last_error()
        rc = call(over)
        err = lib.mumpy_last_error()
        assert rc == code and err != stale and b"resize_bilinear_u8" in err, (over, rc, err)
    return len(REFUSED)


@pytest.mark.skipif(have_gpu(), reason="with a device present a valid tuple of fake addresses would really launch")
def test_refusals_need_no_gpu():
    """A valid tuple of fake, 16-byte aligned, never dereferenced addresses passes every host check (rc > 0: the launch reaches a
    runtime without a device); the same tuple with one rule broken is refused with the stated code."""
    from mumpy_hip.lib import load_library
    assert sweep_refusals(load_library(), {p: 0x1000000 * (i + 1) for i, p in enumerate(POINTERS)}, launches=False) >= 30
