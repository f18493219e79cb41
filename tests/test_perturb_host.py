"""CPU only: the host half of the two ordinary perturbations (mumpy_hip.perturb; include/mumpy_perturb.h).

  * the numpy statements of the JPEG round trip and the Gaussian blur against Pillow itself, bit for bit (every comparison here is
    array_equal: both operations are integer arithmetic inside Pillow), and against tests/golden/perturb.npz, which records the
    Pillow / libjpeg versions its bytes came from -- a different Pillow on another machine shows up there, not as a kernel bug;
  * jpeg_tables against the tables Pillow reports; box_params at radius 0; the ranges of draw;
  * every refusal of the new entries through the C ABI (nothing is launched for a refused call, so this is safe without a device);
  * the header's pinned names, its record lib.PERTURB and the exports of both libraries."""
import hashlib
import io
import os

import numpy as np
import pytest
from PIL import Image, ImageFilter

from abi_surface import names_of
from conftest import ROOT
from mumpy_hip import perturb as P

JPEG_SIZES = [(1, 1), (2, 2), (8, 8), (16, 16), (3, 50), (17, 33), (19, 21), (24, 40), (224, 224), (240, 432)]
JPEG_QUALITIES = (1, 10, 30, 49, 50, 51, 75, 90, 95, 99, 100)
BLUR_SIZES = [(1, 9), (9, 1), (5, 7), (16, 16), (19, 21), (64, 48), (224, 224)]
BLUR_RADII = (0, 0.1, 0.3, 0.5, 0.77, 1, 1.5, 2, 2.5, 3.3, 4.999, 5, 7.3, 12)
EINVAL, EALIGN, ENULL, ERANGE = -1, -2, -3, -4

ARGS = {
    "mumpy_jpeg_roundtrip_workspace_bytes": ["nimg", "H", "W"],
    "mumpy_jpeg_roundtrip_u8_fwd": ["src", "dst", "qtab", "sel", "workspace", "workspace_bytes", "nimg", "ntab", "H", "W", "stream"],
    "mumpy_gaussian_blur_workspace_bytes": ["nimg", "H", "W"],
    "mumpy_gaussian_blur_u8_fwd": ["src", "dst", "params", "workspace", "workspace_bytes", "nimg", "H", "W", "stream"],
    "mumpy_resize_nearest_u8_fwd": ["src", "dst", "ytab", "xtab", "nimg", "Hs", "Ws", "H", "W", "C", "stream"],
}


def pil_jpeg(a, q):
    buf = io.BytesIO()
    Image.fromarray(a).save(buf, format="JPEG", quality=int(q))
    buf.seek(0)
    im = Image.open(buf)
    return np.array(im), im.quantization


def pil_blur(a, r):
    return np.array(Image.fromarray(a).filter(ImageFilter.GaussianBlur(radius=r)))


def contents(hw, seed):
    """noise, a smooth ramp with +-6 noise, a flat image, a 0 / 255 checkerboard"""
    h, w = hw
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    ramp = np.stack([yy * 3 + xx, 255 - xx * 2, yy + xx * 2], -1) + g.integers(-6, 7, (h, w, 3))
    return {"noise": g.integers(0, 256, (h, w, 3), dtype=np.uint8), "ramp": np.clip(ramp, 0, 255).astype(np.uint8),
            "flat": np.full((h, w, 3), (200, 17, 90), np.uint8),
            "checker": np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, -1)}


# ------------------------------------------------------------------------------------------------ the numpy statements are Pillow's
@pytest.mark.parametrize("hw", JPEG_SIZES, ids=[f"{h}x{w}" for h, w in JPEG_SIZES])
def test_jpeg_roundtrip_is_pillows_bit_for_bit(hw):
    for name, a in contents(hw, seed=hw[0] * 1000 + hw[1]).items():
        for q in JPEG_QUALITIES:
            want, _ = pil_jpeg(a, q)
            got = P.jpeg_roundtrip(a, q)
            assert got.dtype == np.uint8 and np.array_equal(got, want), \
                f"{name} {hw} q={q}: {int((got != want).sum())} of {want.size} bytes differ from Pillow"


@pytest.mark.parametrize("q", [1, 30, 49, 50, 51, 75, 95, 100])
def test_jpeg_tables_are_the_ones_pillow_reports(q):
    _, qt = pil_jpeg(np.zeros((8, 8, 3), np.uint8), q)
    t = P.jpeg_tables(q)
    assert t.shape == (2, 64) and t.dtype == np.uint16
    assert t[0].tolist() == list(qt[0]) and t[1].tolist() == list(qt[1])
    assert np.array_equal(P.jpeg_roundtrip(contents((19, 21), 3)["noise"], t), P.jpeg_roundtrip(contents((19, 21), 3)["noise"], q))


@pytest.mark.parametrize("bad", [0, 101, -5, 50.5, 1000])
def test_a_quality_outside_1_to_100_is_refused(bad):
    with pytest.raises(ValueError):
        P.jpeg_tables(bad)
    with pytest.raises(ValueError):
        P.jpeg_roundtrip(np.zeros((8, 8, 3), np.uint8), bad)
    with pytest.raises(ValueError):
        P.check_spec(("jpeg", bad))


@pytest.mark.parametrize("hw", BLUR_SIZES, ids=[f"{h}x{w}" for h, w in BLUR_SIZES])
def test_gaussian_blur_is_pillows_bit_for_bit(hw):
    a = contents(hw, seed=hw[0] * 77 + hw[1])["noise"]
    for r in BLUR_RADII:
        want, got = pil_blur(a, r), P.gaussian_blur(a, r)
        assert got.dtype == np.uint8 and np.array_equal(got, want), f"{hw} radius {r}: {int((got != want).sum())} bytes differ from Pillow"


def test_box_params_at_radius_zero_says_off_and_elsewhere_on():
    assert P.box_params(0)[3] == 0 and P.box_params(0.0)[3] == 0
    a = contents((9, 9), 1)["noise"]
    assert np.array_equal(P.gaussian_blur(a, 0), a)
    for r in (0.1, 2.5, 12):
        rr, ww, fw, on = P.box_params(r)
        assert on == 1 and rr >= 0 and 0 < ww <= 1 << 24 and 0 <= fw and (2 * rr + 1) * ww + 2 * fw <= 1 << 24
        assert np.array_equal(P.gaussian_blur(a, (rr, ww, fw, on)), P.gaussian_blur(a, r))
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            P.box_params(bad)


def test_draw_stays_inside_the_references_ranges():
    g = np.random.default_rng(5)
    seen = {"jpeg": [], "blur": []}
    for _ in range(2000):
        kind, v = P.draw(g)
        seen[kind].append(v)
    assert min(len(v) for v in seen.values()) > 800
    assert all(isinstance(q, int) and 30 <= q < 100 for q in seen["jpeg"]) and {30, 99} <= set(seen["jpeg"])
    assert all(0.0 <= r < 5.0 for r in seen["blur"])
    assert {P.draw(g, kinds=("jpeg",))[0] for _ in range(20)} == {"jpeg"}
    assert {P.draw(g, kinds=("blur",))[0] for _ in range(20)} == {"blur"}
    for bad in ((), ("noise",), ("jpeg", "sharpen")):
        with pytest.raises(ValueError):
            P.draw(g, kinds=bad)
    for spec in seen["jpeg"][:5]:
        assert P.check_spec(("jpeg", spec)) == [("jpeg", spec)]


def test_check_spec():
    assert P.check_spec(None) == []
    assert P.check_spec(("blur", 2)) == [("blur", 2.0)]
    assert P.check_spec([("blur", 1.0), ("jpeg", 70)]) == [("blur", 1.0), ("jpeg", 70)]
    for bad in ("jpeg", ("jpeg",), ("sharpen", 3), [("jpeg", 70), "blur"], ("blur", -1.0), 7, [("jpeg", 0)]):
        with pytest.raises(ValueError):
            P.check_spec(bad)


# ------------------------------------------------------------------------------------------------ the stored Pillow outputs
def test_the_statements_reproduce_the_stored_pillow_outputs():
    """tests/golden/perturb.npz holds what ONE Pillow gave (its version is in the file).  The statements must reproduce it; if this
    machine's Pillow does not, the message says so -- that is a Pillow difference, not an arithmetic one."""
    import PIL
    from gen_perturb_goldens import BIG, BIG_QUALITY, BIG_RADIUS, QUALITIES, RADII, SMALL, image
    path = os.path.join(ROOT, "tests", "golden", "perturb.npz")
    assert os.path.getsize(path) < 100 * 1024
    gold = np.load(path)
    made_by = f"Pillow {gold['pillow_version']} / libjpeg {gold['libjpeg_version']} (this machine: Pillow {PIL.__version__})"
    for hw in SMALL:
        name = f"{hw[0]}x{hw[1]}"
        a = gold[f"in_{name}"]
        for q in QUALITIES:
            assert np.array_equal(P.jpeg_roundtrip(a, q), gold[f"jpeg_{name}_q{q}"]), f"jpeg {name} q={q} vs the bytes of {made_by}"
        for r in RADII:
            assert np.array_equal(P.gaussian_blur(a, r), gold[f"blur_{name}_r{r}"]), f"blur {name} r={r} vs the bytes of {made_by}"
    big = image(BIG, int(gold["big_seed"]))
    assert hashlib.sha256(P.jpeg_roundtrip(big, BIG_QUALITY).tobytes()).hexdigest() == str(gold["big_jpeg_sha256"]), made_by
    assert hashlib.sha256(P.gaussian_blur(big, BIG_RADIUS).tobytes()).hexdigest() == str(gold["big_blur_sha256"]), made_by


# ------------------------------------------------------------------------------------------------ header and binding
HEADER = "mumpy_perturb.h"


def test_the_header_declares_exactly_the_pinned_names():
    assert names_of(HEADER) == dict(ARGS, mumpy_perturb_version=[])


def test_header_binding_and_exports_agree():
    """What tests/test_abi.py checks for every header of the mumpy_hip.h family, for this one: every declared name is exported by
    both libraries; the bound names are the declared ones minus the version function; every bound argument and the return type have
    the ctypes kind of the C declaration; the version agrees everywhere; load_library has bound it."""
    import ctypes
    import abi_surface as S
    from mumpy_hip import lib as L
    s = L.PERTURB
    assert s.header == HEADER and s not in L.SURFACES and not set(s.signatures) & set(L.SIGNATURES)
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
    assert S.define(HEADER, "MUMPY_PERTURB_VERSION") == s.version == getattr(shipped, s.version_fn)() == getattr(tuning, s.version_fn)() == 1


def test_no_name_of_this_header_lives_in_another():
    import abi_surface as S
    from mumpy_hip import lib as L
    for other in L.SURFACES:
        assert not set(S.decls(HEADER)) & set(S.decls(other.header)), other.header
        assert other.version_fn != L.PERTURB.version_fn


def test_a_stale_library_is_refused_by_this_headers_name(monkeypatch):
    from mumpy_hip import lib as L
    monkeypatch.setattr(L, "_LIB", None)
    monkeypatch.setattr(L, "PERTURB", L.PERTURB._replace(version=2))
    with pytest.raises(RuntimeError) as e:
        L.load_library()
    assert HEADER in str(e.value) and "rebuild" in str(e.value) and L._LIB is None


# ------------------------------------------------------------------------------------------------ refusals through the C ABI
A = 4096                                     # a fake, 16-byte aligned, never dereferenced address: every call below is refused


def _lib():
    from mumpy_hip.lib import load_library
    return load_library()


def _valid(entry):
    lib = _lib()
    if entry == "mumpy_jpeg_roundtrip_u8_fwd":
        return dict(src=A, dst=A, qtab=A, sel=A, workspace=A, workspace_bytes=int(lib.mumpy_jpeg_roundtrip_workspace_bytes(2, 19, 21)),
                    nimg=2, ntab=1, H=19, W=21, stream=None)
    if entry == "mumpy_gaussian_blur_u8_fwd":
        return dict(src=A, dst=A, params=A, workspace=A, workspace_bytes=int(lib.mumpy_gaussian_blur_workspace_bytes(2, 19, 21)),
                    nimg=2, H=19, W=21, stream=None)
    return dict(src=A, dst=A + (1 << 20), ytab=A, xtab=A, nimg=2, Hs=37, Ws=41, H=16, W=16, C=3, stream=None)


def _refused(entry, code, word, **change):
    lib = _lib()
    args = dict(_valid(entry), **change)
    assert list(args) == ARGS[entry]
    rc = getattr(lib, entry)(*args.values())
    msg = lib.mumpy_last_error().decode()
    assert rc == code, f"{entry}({change}): rc={rc}, expected {code}: {msg}"
    assert word in msg, f"{entry}({change}): message {msg!r} lacks {word!r}"


def test_workspace_queries():
    lib = _lib()
    assert lib.mumpy_jpeg_roundtrip_workspace_bytes(1, 16, 16) == 16 * 16 + 2 * 8 * 8
    assert lib.mumpy_jpeg_roundtrip_workspace_bytes(3, 19, 21) == 3 * ((19 * 21 + 2 * 10 * 11 + 15) // 16 * 16)
    assert lib.mumpy_jpeg_roundtrip_workspace_bytes(0, 5, 5) == 0
    assert lib.mumpy_gaussian_blur_workspace_bytes(3, 19, 21) == (3 * 19 * 21 * 3 + 15) // 16 * 16
    for fn in (lib.mumpy_jpeg_roundtrip_workspace_bytes, lib.mumpy_gaussian_blur_workspace_bytes):
        assert fn(-1, 8, 8) == EINVAL and fn(1, 0, 8) == EINVAL and fn(1, 8, 0) == EINVAL
        assert fn(1 << 31, 8, 8) == ERANGE and fn(1, 1 << 15, 1 << 15) == ERANGE
    assert lib.mumpy_gaussian_blur_workspace_bytes(1, 10923, 4) == ERANGE and lib.mumpy_gaussian_blur_workspace_bytes(1, 4, 10923) == ERANGE
    assert lib.mumpy_gaussian_blur_workspace_bytes(1, 10922, 4) > 0


def test_jpeg_roundtrip_refusals():
    e = "mumpy_jpeg_roundtrip_u8_fwd"
    for p in ("src", "dst", "qtab", "sel", "workspace"):
        _refused(e, ENULL, "null", **{p: None})
    for p, off in (("qtab", 8), ("workspace", 4), ("sel", 2)):
        _refused(e, EALIGN, "aligned", **{p: A + off})
    _refused(e, EINVAL, "nimg", nimg=-1)
    _refused(e, EINVAL, "0x21", H=0)
    _refused(e, EINVAL, "19x0", W=0)
    _refused(e, EINVAL, "ntab", ntab=0)
    _refused(e, EINVAL, "workspace", workspace_bytes=_valid(e)["workspace_bytes"] - 1)
    _refused(e, EINVAL, "workspace", workspace_bytes=0)
    _refused(e, ERANGE, "2^31", H=1 << 15, W=1 << 15, workspace_bytes=1 << 62)
    _refused(e, ERANGE, "2^31", nimg=1 << 31, workspace_bytes=1 << 62)


def test_gaussian_blur_refusals():
    e = "mumpy_gaussian_blur_u8_fwd"
    for p in ("src", "dst", "params", "workspace"):
        _refused(e, ENULL, "null", **{p: None})
    for p in ("params", "workspace"):
        _refused(e, EALIGN, "aligned", **{p: A + 4})
    _refused(e, EINVAL, "nimg", nimg=-1)
    _refused(e, EINVAL, "0x21", H=0)
    _refused(e, EINVAL, "19x0", W=0)
    _refused(e, EINVAL, "workspace", workspace_bytes=_valid(e)["workspace_bytes"] - 1)
    _refused(e, ERANGE, "2^31", nimg=1 << 31, workspace_bytes=1 << 62)
    _refused(e, ERANGE, "LDS", W=10923, workspace_bytes=1 << 62)
    _refused(e, ERANGE, "LDS", H=10923, workspace_bytes=1 << 62)


def test_resize_nearest_refusals():
    e = "mumpy_resize_nearest_u8_fwd"
    for p in ("src", "dst", "ytab", "xtab"):
        _refused(e, ENULL, "null", **{p: None})
    for p in ("ytab", "xtab"):
        _refused(e, EALIGN, "aligned", **{p: A + 2})
    for change in (dict(nimg=-1), dict(Hs=0), dict(Ws=0), dict(H=0), dict(W=0), dict(C=0), dict(C=5)):
        _refused(e, EINVAL, "bad sizes", **change)
    _refused(e, ERANGE, "2^31", Hs=1 << 15, Ws=1 << 15)
    _refused(e, ERANGE, "2^31", nimg=1 << 31)


def test_zero_images_is_a_valid_call_that_launches_nothing():
    lib = _lib()
    assert lib.mumpy_jpeg_roundtrip_u8_fwd(A, A, A, A, A, 0, 0, 1, 8, 8, None) == 0
    assert lib.mumpy_gaussian_blur_u8_fwd(A, A, A, A, 0, 0, 8, 8, None) == 0
    assert lib.mumpy_resize_nearest_u8_fwd(A, A + 64, A, A, 0, 8, 8, 4, 4, 3, None) == 0
