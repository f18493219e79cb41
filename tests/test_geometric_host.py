"""CPU only: the host half of the geometric operations (mumpy_hip.geometric; include/mumpy_geometric.h).

  * the numpy statements against Pillow itself, bit for bit (every comparison here is array_equal), over sizes 1x1 .. 240x432, one and
    three channels, every affine kind, and against tests/golden/geometric.npz, which records the Pillow version its bytes came from --
    a different Pillow on another machine shows up there, by version, not as a kernel bug;
  * cutout against ImageDraw.rectangle; cutout_rects: bounds, the compounding side, both branches;
  * params_row (the encoding, the constant-shift check and the check_fixed refusal by constructed cases), draw, check_kind, check_spec;
  * the header's pinned names, its record lib.GEOMETRIC and the exports of both libraries;
  * every refusal of the new entry through the C ABI (nothing is launched for a refused call, so this is safe without a device)."""
import hashlib
import math
import os

import numpy as np
import pytest

from abi_surface import names_of
from conftest import ROOT
from gen_geometric_goldens import BIG, BIG_CASES, CASES, RECTS, SMALL, image, key, pil_cutout, pil_geometric
from mumpy_hip import geometric as G
from mumpy_hip import perturb as PT

SIZES = [(1, 1), (2, 5), (3, 3), (7, 9), (19, 21), (64, 48), (224, 224), (240, 432)]
SHEARS = (0, 0.05, -0.05, 0.13, -0.13, 0.3, -0.3)
FRACTIONS = (0, 0.1, -0.1, 0.2501, -0.2501, 0.33, -0.33, 0.45, -0.45)
ABS = (0, 3, -7.5, 10)
ANGLES = (0, 1, 17.3, -30, 45, 89.9, 90, 123.4, 180, 270, -179.5)
EINVAL, EALIGN, ENULL, ERANGE = -1, -2, -3, -4
HEADER = "mumpy_geometric.h"
ARGS = {"mumpy_geometric_u8_fwd": ["src", "dst", "params", "nimg", "H", "W", "C", "stream"]}
MODES = {"none": 0, "fixed16": 1, "shift": 2, "rect": 3}


def all_cases():
    return [(k, v) for k in ("shear_x", "shear_y") for v in SHEARS] + [(k, v) for k in ("translate_x", "translate_y") for v in FRACTIONS] + \
        [(k, v) for k in ("translate_x_abs", "translate_y_abs") for v in ABS] + [("rotate", v) for v in ANGLES]


# ------------------------------------------------------------------------------------------------ the numpy statements are Pillow's
@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
@pytest.mark.parametrize("channels", [1, 3])
def test_every_affine_statement_is_pillows_bit_for_bit(hw, channels):
    a = image(hw, channels, seed=hw[0] * 1000 + hw[1])
    before = a.copy()
    assert set(k for k, _ in all_cases()) == set(G.AFFINE_KINDS)
    for kind, v in all_cases():
        want, got = pil_geometric(a, kind, v), G.affine(a, kind, v)
        assert got.dtype == np.uint8 and got.shape == a.shape and np.array_equal(got, want), \
            f"{kind} {v} on {hw}x{channels}: {int((got != want).sum())} of {want.size} bytes differ from Pillow"
    assert np.array_equal(a, before)


def test_the_golden_file_agrees_and_names_its_pillow():
    import PIL
    z = np.load(os.path.join(ROOT, "tests", "golden", "geometric.npz"))
    version = str(z["pillow_version"])
    for k, hw in enumerate(SMALL):
        for c in (1, 3):
            a = z[f"in_{hw[0]}x{hw[1]}x{c}"]
            assert np.array_equal(a, image(hw, c, 300 + k))
            for kind, v in CASES:
                assert np.array_equal(G.affine(a, kind, v), z[key(hw, c, kind, v)]), f"{kind} {v} {hw}x{c} (golden of Pillow {version})"
            for rect in RECTS:
                assert np.array_equal(G.cutout(a, rect), z[key(hw, c, "cutout", rect)]), f"cutout {rect} {hw}x{c} (golden of Pillow {version})"
    big = image(BIG, 3, int(z["big_seed"]))
    for kind, v in BIG_CASES:
        got = hashlib.sha256(G.affine(big, kind, v).tobytes()).hexdigest()
        assert got == str(z["sha256_" + key(BIG, 3, kind, v)]), f"{kind} {v} 64x48 (golden of Pillow {version})"
    assert version.split(".")[0].isdigit() and PIL.__version__                    # recorded; the installed one is compared above


def test_the_rotate_matrix_is_image_rotates():
    """The matrix of a general angle is checked through Pillow's own transform; the exits are the exact transposes."""
    from PIL import Image
    for hw in ((7, 9), (19, 21), (12, 12)):
        a = image(hw, 3, 4)
        im = Image.fromarray(a)
        for angle in (1, 17.3, -30, 45, 89.9, 123.4, -179.5, 90, 270):
            m = G.rotate_matrix(angle, hw)
            want = np.array(im.rotate(angle, fillcolor=(0, 0, 0)))
            assert np.array_equal(np.array(im.transform(im.size, Image.AFFINE, m, resample=Image.NEAREST, fillcolor=(0, 0, 0))), want), (hw, angle)
    assert G.rotate_matrix(0, (5, 7)) == G.rotate_matrix(360, (5, 7)) == (1, 0, 0, 0, 1, 0)
    assert G.rotate_matrix(180, (5, 7)) == G.rotate_matrix(-180, (5, 7)) == (-1, 0, 7, 0, -1, 5)
    assert G.rotate_matrix(90, (6, 6)) == (0, -1, 6, 1, 0, 0) and G.rotate_matrix(-90, (6, 6)) == (0, 1, 0, -1, 0, 6)
    a = image((6, 6), 1, 2)
    assert np.array_equal(G.affine(a, "rotate", 90), np.rot90(a, 1)) and np.array_equal(G.affine(a, "rotate", 270), np.rot90(a, 3))
    assert np.array_equal(G.affine(a, "rotate", 180), a[::-1, ::-1]) and np.array_equal(G.affine(a, "rotate", 0), a)
    c, s = round(math.cos(-math.radians(30)), 15), round(math.sin(-math.radians(30)), 15)
    m = G.affine_matrix("rotate", 30, (10, 20))
    assert m[:2] == (c, s) and m[3:5] == (-s, c) and m[2] == c * -10.0 + s * -5.0 + 0.0 + 10.0


def test_affine_matrix_is_what_the_reference_hands_over():
    assert G.affine_matrix("shear_x", 0.2, (5, 7)) == (1, 0.2, 0, 0, 1, 0)
    assert G.affine_matrix("shear_y", -0.2, (5, 7)) == (1, 0, 0, -0.2, 1, 0)
    assert G.affine_matrix("translate_x", 0.2501, (5, 7)) == (1, 0, 0.2501 * 7, 0, 1, 0)
    assert G.affine_matrix("translate_y", 0.2501, (5, 7)) == (1, 0, 0, 0, 1, 0.2501 * 5)
    assert G.affine_matrix("translate_x_abs", -7.5, (5, 7)) == (1, 0, -7.5, 0, 1, 0)
    assert G.affine_matrix("translate_y_abs", 3, (5, 7)) == (1, 0, 0, 0, 1, 3)
    for bad in (("cutout", 0.1), ("shear", 0.1), ("shear_x", None), ("shear_x", float("nan")), ("rotate", float("inf")), ("rotate", "3")):
        with pytest.raises(ValueError):
            G.affine_matrix(*bad, (5, 7))


# ------------------------------------------------------------------------------------------------ cutout
CUT_RECTS = {"interior": (2, 1, 5, 3), "float corners": (2.9, 1.2, 5.7, 3.99), "left edge": (0, 4, 3.5, 6), "top edge": (5, 0, 8, 2.2),
             "right edge": (17, 3, 21, 9), "bottom edge": (3, 15.5, 9, 19), "past both": (12, 10, 30.5, 44), "one pixel": (20, 18, 20.9, 18.2),
             "whole": (0, 0, 21, 19), "outside right": (21, 3, 25, 9), "outside below": (2, 19, 9, 30.5), "far outside": (30, 30, 40.5, 41)}


@pytest.mark.parametrize("name", list(CUT_RECTS))
def test_cutout_is_imagedraws_rectangle(name):
    rect = CUT_RECTS[name]
    for c in (1, 3):
        a = image((19, 21), c, 8)
        want, got = pil_cutout(a, rect), G.cutout(a, rect)
        assert np.array_equal(got, want), f"{name} {rect}: {int((got != want).sum())} bytes differ from ImageDraw"
        assert ("outside" in name) == np.array_equal(got, a)


def test_cutout_refuses_what_pillow_refuses():
    a = image((7, 9), 3, 1)
    for bad in ((5, 2, 4, 6), (1, 5, 3, 4), (0, 0, float("nan"), 3), (0, 0, float("inf"), 3)):
        with pytest.raises(ValueError):
            G.cutout(a, bad)
    for bad in ((5, 2, 4, 6), (1, 5, 3, 4)):
        with pytest.raises(ValueError):
            pil_cutout(a, bad)


def _box_mask(L=28):
    m = np.zeros((L, L), np.uint8)
    m[5:9, 3:12] = 255                                                   # find_corners -> (2, 4, 12, 9): more room right of and below it
    return m


@pytest.mark.parametrize("mask", ["empty", "box"])
def test_cutout_rects_follow_the_reference(mask):
    L, T, v = 28, 3, 0.1
    m = np.zeros((L, L), np.uint8) if mask == "empty" else _box_mask(L)
    g = np.random.default_rng(11)
    sides_x, sides_y, beside = set(), set(), 0
    for _ in range(300):
        rects = G.cutout_rects(m, v, T, g)
        assert len(rects) == T
        for k, (x0, y0, x1, y1) in enumerate(rects):
            side = v * float(L) ** (k + 1)                               # v = v * w inside the frame loop: 2.8, 78.4, 2195.2
            assert isinstance(x0, int) and isinstance(y0, int) and 0 <= x0 <= x1 <= L and 0 <= y0 <= y1 <= L
            assert x1 == min(L, x0 + side) and y1 == min(L, y0 + side)
            clipped = G.clip_rect((x0, y0, x1, y1), (L, L))
            assert clipped is None or (0 <= clipped[0] <= clipped[2] <= L - 1 and 0 <= clipped[1] <= clipped[3] <= L - 1)
            if k == 0:
                sides_x.add(round(x1 - x0, 6)), sides_y.add(round(y1 - y0, 6))
                # the box leaves more room on its right and below: x from uniform(12, 25.2) or y from uniform(9, 25.2), less 1.4
                beside += x0 >= 10 or y0 >= 7
        assert rects[1][2:] == (L, L) and rects[2][:2] == (0, 0) and rects[2][2:] == (L, L)      # the compounded side covers the rest
    assert 2.8 in sides_x and 2.8 in sides_y
    if mask == "box":
        assert beside == 300
    assert G.cutout_rects(m, 0.0, T, g) == []
    for bad in (-0.1, 0.21, float("nan"), None):
        with pytest.raises(ValueError):
            G.cutout_rects(m, bad, T, g)


def test_the_references_uniform_calls_are_kept():
    """np.random.uniform(w) is uniform(low=w, high=1.0), a draw between 1 and w; uniform(0, left - v) runs backwards for a wide side."""
    g = np.random.default_rng(3)
    one = np.array([G._uniform(g, 28) for _ in range(2000)])
    assert one.min() > 1.0 and one.max() <= 28.0 and one.min() < 1.5 and one.max() > 27.5
    back = np.array([G._uniform(g, 0, -5.0) for _ in range(500)])
    assert back.min() >= -5.0 and back.max() <= 0.0
    m = np.zeros((28, 28), np.uint8)
    firsts = [G.cutout_rects(m, 0.001, 1, g)[0] for _ in range(500)]                   # a side of 0.028: the corner is the drawn point
    assert all(0 <= r[0] <= 27 and 0 <= r[1] <= 27 and r[2] == r[0] + 0.028 * 1.0 for r in firsts)


# ------------------------------------------------------------------------------------------------ params_row, draw, check_kind
def test_params_row_encodes_the_four_modes():
    assert G.MODES == MODES and (G.MODE_NONE, G.MODE_FIXED16, G.MODE_SHIFT, G.MODE_RECT) == (0, 1, 2, 3)
    z = np.zeros(8, np.int32)
    for row in (G.params_row("none"), G.params_row(None)):
        assert row.dtype == np.int32 and np.array_equal(row, z)
    fix = lambda v: int(math.floor(v * 65536.0 + 0.5))                           # noqa: E731
    assert G.params_row("shear_x", 0.13, (19, 21)).tolist() == [1, 65536, fix(0.13), fix(0.5 + 0.065), 0, 65536, 32768, 0]
    assert G.params_row("shear_y", -0.3, (19, 21)).tolist() == [1, 65536, 0, 32768, fix(-0.3), 65536, fix(0.5 - 0.15), 0]
    assert G.params_row("rotate", 180, (19, 21)).tolist() == [1, -65536, 0, fix(21 - 0.5), 0, -65536, fix(19 - 0.5), 0]
    assert G.params_row("rotate", 0, (19, 21)).tolist() == [1, 65536, 0, 32768, 0, 65536, 32768, 0]
    assert G.params_row("shear_x", 0, (19, 21)).tolist() == [2, 0, 0, 0, 0, 0, 0, 0]                       # Pillow's scale path
    assert G.params_row("translate_x", 0.2501, (19, 21)).tolist() == [2, 5, 0, 0, 0, 0, 0, 0]             # floor(5.2521 + 0.5)
    assert G.params_row("translate_x", -0.45, (19, 21)).tolist() == [2, -9, 0, 0, 0, 0, 0, 0]             # floor(-9.45 + 0.5)
    assert G.params_row("translate_y_abs", -7.5, (19, 21)).tolist() == [2, 0, -7, 0, 0, 0, 0, 0]          # floor(-7.5 + 0.5)
    assert G.params_row("translate_y", 0.45, (1, 1)).tolist() == [2, 0, 0, 0, 0, 0, 0, 0]
    assert G.params_row("cutout", (2, 1, 5.7, 3.2), (19, 21)).tolist() == [3, 2, 1, 5, 3, 0, 0, 0]
    assert G.params_row("cutout", (4, 3, 21, 19), (19, 21)).tolist() == [3, 4, 3, 20, 18, 0, 0, 0]
    assert np.array_equal(G.params_row("cutout", (30, 30, 40.5, 41), (19, 21)), z)                         # empty: a copy
    for bad in (("shear", 0.1, (5, 5)), ("shear_x", 0.1, (0, 5)), ("shear_x", 0.1, (5, 8193)), ("shear_x", None, (5, 5))):
        with pytest.raises(ValueError):
            G.params_row(*bad)


def test_apply_row_copies_for_none_an_unknown_mode_and_an_empty_rectangle():
    a = image((7, 9), 3, 2)
    for row in ([0] * 8, [57, 1, 2, 3, 4, 5, 6, 0], [-3, 0, 0, 0, 0, 0, 0, 0], [3, 5, 5, 4, 6, 0, 0, 0], [3, 9, 0, 12, 3, 0, 0, 0]):
        out = G.apply_row(a, np.array(row, np.int32))
        assert np.array_equal(out, a) and out is not a
    assert not G.apply_row(a, np.array([2, 9, 0, 0, 0, 0, 0, 0], np.int32)).any()            # shifted out whole: all zeros
    assert not G.apply_row(a, np.array([2, 0, -7, 0, 0, 0, 0, 0], np.int32)).any()
    big = np.array([1, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 0], np.int32)
    assert G.apply_row(a, big).shape == a.shape                                              # any row is safe: 64-bit walk


def test_the_constant_shift_check_refuses_a_walk_that_steps_over_an_integer():
    """tx + 0.5 = 1 - 2^-53: the walk's first coordinate truncates to 0, its second, 2 - 2^-53 rounded to even, is 2.0: columns 0 and
    1 read sources 0 and 2, which is no shift.  Pillow does exactly that; the SHIFT mode cannot say it, so the row is refused."""
    from PIL import Image
    t = math.nextafter(1.0, 0.0) - 0.5
    assert G.scale_walk((1.0, 0.0, t, 0.0, 1.0, 0.0), (1, 5))[0].tolist() == [0, 2, 3, 4, 5]
    a = image((1, 5), 1, 0)
    pil = np.array(Image.fromarray(a).transform((5, 1), Image.AFFINE, (1, 0, t, 0, 1, 0), resample=Image.NEAREST, fillcolor=0))
    assert pil[0].tolist() == [a[0, 0], a[0, 2], a[0, 3], a[0, 4], 0]
    with pytest.raises(ValueError, match="constant shift"):
        G.params_row("translate_x_abs", t, (1, 5))
    with pytest.raises(ValueError, match="constant shift"):
        G.params_row("translate_y_abs", t, (5, 1))
    assert G.params_row("translate_x_abs", t, (1, 1)).tolist()[:3] == [2, 0, 0]              # one column: nothing to step over
    assert G.constant_shift((1.0, 0.0, 0.5, 0.0, 1.0, -0.5), (4, 4)) == (1, 0)
    with pytest.raises(ValueError):
        G.constant_shift((1.0, 0.1, 0.5, 0.0, 1.0, -0.5), (4, 4))


def test_check_fixed_refuses_what_pillow_would_walk_in_doubles():
    m = (1.0, 0.3, 32766.0, 0.0, 1.0, 0.0)
    assert G.check_fixed(m, (1, 1)) and not G.check_fixed(m, (5, 5))                         # the corner (5, 5) lands at 32772.5
    assert G.fixed16_words(m, (1, 1))[2] == 32766 * 65536 + 42598          # FIX(32766 + 0.5 + 0.15)
    with pytest.raises(ValueError, match="check_fixed"):
        G.fixed16_words(m, (5, 5))
    assert not G.check_fixed((1.0, 0.3, 0.0, 0.0, 1.0, -32768.0), (5, 5))
    assert G.check_fixed(G.affine_matrix("rotate", 45, (8192, 8192)), (8192, 8192))          # every offered kind passes at the largest size
    assert G.fix16(-0.3) == -19661 and G.fix16(0.5) == 32768 and G.fix16(-0.5) == -32768 and G.fix16(-1e-9) == 0


def test_check_kind_holds_the_references_asserts():
    for kind, lo, hi in (("shear_x", -0.3, 0.3), ("shear_y", -0.3, 0.3), ("translate_x", -0.45, 0.45), ("translate_y", -0.45, 0.45),
                         ("translate_x_abs", -10, 10), ("translate_y_abs", -10, 10), ("rotate", -180, 180), ("cutout", 0, 0.2)):
        assert G.check_kind(kind, lo) == (kind, float(lo)) and G.check_kind(kind, hi) == (kind, float(hi))
        assert isinstance(G.check_kind(kind, np.float32(0.1))[1], float)
        for bad in (math.nextafter(lo, -math.inf), math.nextafter(hi, math.inf), float("nan"), float("inf"), -float("inf"), None, "0.1", True):
            with pytest.raises(ValueError):
                G.check_kind(kind, bad)
    with pytest.raises(ValueError):
        G.check_kind("shear", 0.1)
    assert set(G.KINDS) == set(G.AFFINE_KINDS) | {"cutout"} and len(G.AFFINE_KINDS) == 7


def test_draw_stays_inside_the_references_ranges():
    g = np.random.default_rng(5)
    seen = {k: [] for k in G.KINDS}
    for _ in range(4000):
        kind, v = G.draw(g)
        assert G.check_kind(kind, v) == (kind, v)
        seen[kind].append(v)
    top = {"shear_x": 0.3, "shear_y": 0.3, "translate_x": 0.33, "translate_y": 0.33, "translate_x_abs": 10, "translate_y_abs": 10,
           "rotate": 180, "cutout": 0.2}
    for kind, vs in seen.items():
        vs = np.array(vs)
        assert len(vs) > 300 and np.abs(vs).max() <= top[kind] and np.abs(vs).max() > 0.9 * top[kind]
        neg = (vs < 0).mean()
        assert (neg == 0) if kind == "cutout" else (0.4 < neg < 0.6)                         # the sign flips with probability 0.5
    assert all(G.draw(g, ("rotate",))[0] == "rotate" for _ in range(5))
    for bad in ((), ("jpeg",), ("rotate", "none")):
        with pytest.raises(ValueError):
            G.draw(g, bad)


def test_check_spec_takes_the_new_kinds_only_when_asked():
    specs = [("shear_x", 0.2), ("shear_y", -0.3), ("translate_x", 0.45), ("translate_y", -0.1), ("translate_x_abs", 10),
             ("translate_y_abs", -7.5), ("rotate", -30), ("cutout", 0.1)]
    for s in specs:
        assert PT.check_spec(s, geometric=True) == [(s[0], float(s[1]))]
        with pytest.raises(ValueError):
            PT.check_spec(s)                                                                 # the default refuses them: an unknown kind
        with pytest.raises(ValueError):
            PT.check_spec(s, "who")
    assert PT.check_spec([("jpeg", 70), ("rotate", 17)], geometric=True) == [("jpeg", 70), ("rotate", 17.0)]
    assert PT.check_spec(("contrast", 1.4), geometric=True) == PT.check_spec(("contrast", 1.4)) == [("contrast", 1.4)]
    for bad in (("shear_x", 0.31), ("rotate", 181), ("cutout", -0.1), ("cutout", None), ("translate_x", float("nan")), ("shear", 0.1)):
        with pytest.raises(ValueError):
            PT.check_spec(bad, geometric=True)


def test_the_video_predictor_still_refuses_the_new_kinds():
    import inspect
    from mumpy_hip import video
    src = inspect.getsource(video)
    assert "check_spec(" in src and "geometric=True" not in src


# ------------------------------------------------------------------------------------------------ header, binding, exports
def test_the_header_declares_exactly_the_pinned_names():
    import abi_surface as S
    assert names_of(HEADER) == dict(ARGS, mumpy_geometric_version=[])
    for mode, code in MODES.items():
        assert S.define(HEADER, f"MUMPY_GEO_{mode.upper()}") == code == G.MODES[mode]
    assert not HEADER.startswith("mumpy_hip")


def test_header_binding_and_exports_agree():
    import ctypes
    import abi_surface as S
    from mumpy_hip import lib as L
    s = L.GEOMETRIC
    assert s.header == HEADER and s not in L.SURFACES and s is not L.PERTURB and s is not L.PHOTOMETRIC
    declared = S.decls(HEADER)
    shipped, tuning = L.load_library(), ctypes.CDLL(L.tuning_library_path())
    for name in declared:
        assert hasattr(shipped, name) and hasattr(tuning, name), f"{name} declared in {HEADER} but not exported"
    assert set(s.signatures) == set(declared) - {s.version_fn}
    for name, args in s.signatures.items():
        assert getattr(shipped, name).argtypes == args
        got, want = [S.ckind(t) for t in args], [S.kind(a) for a in declared[name].args]
        assert got == want, f"{name}: binding {got} vs header {want}"
        got, want = S.ckind(getattr(shipped, name).restype), S.kind(declared[name].ret)
        assert got == want, f"{name}: binding returns {got}, header {want}"
    assert declared[s.version_fn] == S.Decl("int", [])
    getattr(tuning, s.version_fn).restype = ctypes.c_int
    assert S.define(HEADER, "MUMPY_GEOMETRIC_VERSION") == s.version == getattr(shipped, s.version_fn)() == \
        getattr(tuning, s.version_fn)() == 1


def test_no_name_of_this_header_lives_in_another():
    import abi_surface as S
    from mumpy_hip import lib as L
    for other in L.SURFACES + [L.PERTURB, L.PHOTOMETRIC]:
        assert not set(S.decls(HEADER)) & set(S.decls(other.header)), other.header
        assert not set(L.GEOMETRIC.signatures) & set(other.signatures), other.header
        assert other.version_fn != L.GEOMETRIC.version_fn


def test_a_stale_library_is_refused_by_this_headers_name(monkeypatch):
    from mumpy_hip import lib as L
    monkeypatch.setattr(L, "_LIB", None)
    monkeypatch.setattr(L, "GEOMETRIC", L.GEOMETRIC._replace(version=2))
    with pytest.raises(RuntimeError) as e:
        L.load_library()
    assert HEADER in str(e.value) and "rebuild" in str(e.value) and L._LIB is None


# ------------------------------------------------------------------------------------------------ refusals through the C ABI
A = 4096                                     # a fake, 16-byte aligned, never dereferenced address: every call below is refused
B_ = 1 << 40                                 # a second one, far from the first
ENTRY = "mumpy_geometric_u8_fwd"


def _lib():
    from mumpy_hip.lib import load_library
    return load_library()


def _valid():
    return dict(src=A, dst=B_, params=A, nimg=2, H=19, W=21, C=3, stream=None)


def _refused(code, word, **change):
    lib = _lib()
    args = dict(_valid(), **change)
    assert list(args) == ARGS[ENTRY]
    rc = getattr(lib, ENTRY)(*args.values())
    msg = lib.mumpy_last_error().decode()
    assert rc == code, f"{ENTRY}({change}): rc={rc}, expected {code}: {msg}"
    assert word in msg, f"{ENTRY}({change}): message {msg!r} lacks {word!r}"


def test_refusals():
    for p in ("src", "dst", "params"):
        _refused(ENULL, "null", **{p: None})
    for off in (4, 8, 12, 1):
        _refused(EALIGN, "aligned", params=A + off)
    _refused(EINVAL, "nimg", nimg=-1)
    _refused(EINVAL, "0x21", H=0)
    _refused(EINVAL, "19x0", W=0)
    _refused(EINVAL, "-19x21", H=-19)
    for c in (0, 2, 4, -1):
        _refused(EINVAL, f"C={c}", C=c)
    _refused(ERANGE, "2^31", nimg=1 << 31)
    _refused(ERANGE, "8192", H=8193, W=1)
    _refused(ERANGE, "8192", H=1, W=8193)
    _refused(ERANGE, "2^24", H=4097, W=4096)
    _refused(ERANGE, "2^24", H=8192, W=8192)
    _refused(EINVAL, "overlaps", dst=A)                                          # in place
    nbytes = 2 * 19 * 21 * 3
    for off in (1, 19 * 21 * 3, nbytes - 1):                                     # partial overlap, either way round
        _refused(EINVAL, "overlaps", dst=A + off)
        _refused(EINVAL, "overlaps", src=B_ + off)
    _refused(EINVAL, "overlaps", dst=A + 19 * 21 - 1, nimg=1, C=1)


def test_zero_images_is_a_valid_call_that_launches_nothing():
    assert _lib().mumpy_geometric_u8_fwd(A, B_, A, 0, 8, 8, 3, None) == 0
    assert _lib().mumpy_geometric_u8_fwd(A, A, A, 0, 8, 8, 1, None) == 0
