"""CPU only: the host half of the nine photometric operations (mumpy_hip.photometric; include/mumpy_photometric.h).

  * the numpy statements against Pillow itself, bit for bit (every comparison here is array_equal), over sizes 1x1 .. 240x432, four
    contents and ten factors, and against tests/golden/photometric.npz, which records the Pillow version its bytes came from -- a
    different Pillow on another machine shows up there, by version, not as a kernel bug;
  * the corners: solarize thresholds, posterize 0 .. 8 bits, equalize's three identity exits and its saturation at 255, autocontrast
    on a flat channel, SMOOTH on small images and on random 3x3 neighbourhoods;
  * params_row, the ranges of draw, what check_spec accepts and refuses;
  * the header's pinned names, its record lib.PHOTOMETRIC and the exports of both libraries;
  * every refusal of the new entry through the C ABI (nothing is launched for a refused call, so this is safe without a device)."""
import hashlib
import os

import numpy as np
import pytest
from PIL import Image, ImageFilter

from abi_surface import names_of
from conftest import ROOT
from gen_photometric_goldens import pil_photometric
from mumpy_hip import perturb as PT
from mumpy_hip import photometric as P

SIZES = [(1, 1), (2, 5), (3, 3), (7, 9), (19, 21), (64, 48), (224, 224), (240, 432)]
FACTORS = (0, 0.1, 0.3, 0.5, 0.77, 1, 1.3, 1.5, 1.9, 2.5)
THRESHOLDS = (0, 0.5, 109.7, 128, 256)
EINVAL, EALIGN, ENULL, ERANGE = -1, -2, -3, -4

ARGS = {
    "mumpy_photometric_workspace_bytes": ["nimg", "H", "W"],
    "mumpy_photometric_u8_fwd": ["src", "dst", "params", "workspace", "workspace_bytes", "nimg", "H", "W", "stream"],
}
KINDS = {"none": 0, "autocontrast": 1, "invert": 2, "equalize": 3, "solarize": 4, "posterize": 5, "contrast": 6, "color": 7,
         "brightness": 8, "sharpness": 9}


def contents(hw, seed):
    """noise, narrow-range noise (90 .. 139), a flat image, a ramp"""
    h, w = hw
    g = np.random.default_rng(seed)
    ramp = np.arange(h * w * 3).reshape(h, w, 3) * 255 // max(h * w * 3 - 1, 1)
    return {"noise": g.integers(0, 256, (h, w, 3), dtype=np.uint8), "narrow": g.integers(90, 140, (h, w, 3), dtype=np.uint8),
            "flat": np.full((h, w, 3), (200, 17, 90), np.uint8), "ramp": ramp.astype(np.uint8)}


def all_cases():
    return [(k, None) for k in P.VALUELESS] + [("solarize", t) for t in THRESHOLDS] + [("posterize", b) for b in range(9)] + \
        [(k, f) for k in P.FACTOR for f in FACTORS]


# ------------------------------------------------------------------------------------------------ the numpy statements are Pillow's
@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_every_statement_is_pillows_bit_for_bit(hw):
    for name, a in contents(hw, seed=hw[0] * 1000 + hw[1]).items():
        before = a.copy()
        for kind, v in all_cases():
            want, got = pil_photometric(a, kind, v), P.apply(a, kind, v)
            assert got.dtype == np.uint8 and got.shape == a.shape and np.array_equal(got, want), \
                f"{kind} {v} on {name} {hw}: {int((got != want).sum())} of {want.size} bytes differ from Pillow"
        assert np.array_equal(a, before)


def test_apply_by_code_and_pass_through():
    a = contents((7, 9), 3)["noise"]
    assert np.array_equal(P.apply(a, "none"), a) and np.array_equal(P.apply(a, 0), a) and P.apply(a, 0) is not a
    for kind, code in KINDS.items():
        if kind != "none":
            v = None if kind in P.VALUELESS else 3
            assert np.array_equal(P.apply(a, code, v), P.apply(a, kind, v))
    for bad in ("sharpen", 10, -1):
        with pytest.raises(ValueError):
            P.apply(a, bad, 1.0)
    with pytest.raises(ValueError):
        P.apply(a[..., :2], "invert")
    with pytest.raises(ValueError):
        P.apply(a.astype(np.int32), "invert")


def test_posterize_zero_bits_is_black_and_eight_is_the_image():
    a = contents((7, 9), 4)["noise"]
    assert not P.posterize(a, 0).any() and np.array_equal(P.posterize(a, 8), a)
    assert np.array_equal(P.solarize(a, 256), a) and np.array_equal(P.solarize(a, 0), 255 - a)


def test_equalize_identity_exits_and_saturation():
    ident = np.arange(256)
    one_bin = np.zeros(256, np.int64)
    one_bin[40] = 500
    assert np.array_equal(P.equalize_table(one_bin), ident)                      # at most one non-empty bin
    few = np.zeros(256, np.int64)
    few[[3, 200]] = (100, 900)                                                   # step = (1000 - 900) // 255 = 0
    assert np.array_equal(P.equalize_table(few), ident)
    a = contents((19, 21), 5)["noise"]                                           # 399 pixels: step 1, entries run past 255
    t = P.equalize_table(np.bincount(a[..., 0].ravel(), minlength=256))
    h = np.bincount(a[..., 0].ravel(), minlength=256)
    raw = np.concatenate([[0], np.cumsum(h)[:-1]])                               # step == 1, n starts at 0
    assert (399 - h[np.nonzero(h)[0][-1]]) // 255 == 1 and raw.max() > 255
    assert t.max() == 255 and np.array_equal(t, np.minimum(raw, 255)) and not np.array_equal(t, raw % 256)
    assert np.array_equal(P.equalize(a), pil_photometric(a, "equalize"))
    flat = contents((7, 9), 5)["flat"]
    assert np.array_equal(P.equalize(flat), flat) and np.array_equal(pil_photometric(flat, "equalize"), flat)


def test_autocontrast_on_a_flat_channel_keeps_it():
    a = contents((7, 9), 6)["narrow"]
    a[..., 1] = 93
    got = P.autocontrast(a)
    assert np.array_equal(got[..., 1], a[..., 1]) and np.array_equal(got, pil_photometric(a, "autocontrast"))
    assert got[..., 0].min() == 0 and got[..., 0].max() >= 254                   # the top entry is truncated, not rounded


def test_smooth_is_pillows_on_small_images_and_random_neighbourhoods():
    for hw in [(1, 1), (1, 9), (9, 1), (2, 5), (5, 2), (3, 3), (3, 4), (7, 9)]:
        for name, a in contents(hw, seed=hw[0] * 17 + hw[1]).items():
            want = np.array(Image.fromarray(a).filter(ImageFilter.SMOOTH))
            assert np.array_equal(P.smooth(a), want), f"SMOOTH {name} {hw}"
    g = np.random.default_rng(7)
    blocks = g.integers(0, 256, (4000, 3, 3, 3), dtype=np.uint8)
    blocks[:200] = g.choice(np.array([0, 1, 254, 255], np.uint8), (200, 3, 3, 3))
    for a in blocks:
        assert np.array_equal(P.smooth(a), np.array(Image.fromarray(a).filter(ImageFilter.SMOOTH)))
    assert P.SMOOTH_KERNEL.dtype == np.float32 and P.SMOOTH_KERNEL[1, 1] == np.float32(5) / np.float32(13)


def test_the_blend_rounds_the_product_and_the_sum_separately():
    """A fused multiply-add would give another byte somewhere in this sweep; the statement is held to the two-rounding form."""
    i, d = np.meshgrid(np.arange(256), np.arange(256))
    fused_differs = 0
    for v in (0.1, 0.3, 0.77, 1.1, 1.3, 1.9):                                    # 1.1f: d = 12, i = 2 is 1.0 in two roundings, 0.99999976 fused
        got = P.blend(d, i, v)
        two = np.float32(d) + (np.float32(v) * np.float32(i - d)).astype(np.float32)
        assert np.array_equal(got, np.clip(np.trunc(two.astype(np.float32)), 0, 255).astype(np.uint8))
        one = np.float64(d) + np.float64(np.float32(v)) * np.float64(i - d)                 # exact, then one rounding
        fused_differs += int((np.clip(np.trunc(one.astype(np.float32)), 0, 255).astype(np.uint8) != got).sum())
    assert fused_differs > 0


# ------------------------------------------------------------------------------------------------ the stored Pillow outputs
def test_the_statements_reproduce_the_stored_pillow_outputs():
    """tests/golden/photometric.npz holds what ONE Pillow gave (its version is in the file).  The statements must reproduce it; if
    this machine's Pillow does not, the message says so -- that is a Pillow difference, not an arithmetic one."""
    import PIL
    from gen_photometric_goldens import BIG, BIG_CASES, CASES, SMALL, image, key
    path = os.path.join(ROOT, "tests", "golden", "photometric.npz")
    assert os.path.getsize(path) < 100 * 1024
    gold = np.load(path)
    made_by = f"Pillow {gold['pillow_version']} (this machine: Pillow {PIL.__version__})"
    for hw in SMALL:
        a = gold[f"in_{hw[0]}x{hw[1]}"]
        for kind, v in CASES:
            assert np.array_equal(P.apply(a, kind, v), gold[key(hw, kind, v)]), f"{kind} {v} {hw} vs the bytes of {made_by}"
    big = image(BIG, int(gold["big_seed"]))
    for kind, v in BIG_CASES:
        assert hashlib.sha256(P.apply(big, kind, v).tobytes()).hexdigest() == str(gold["sha256_" + key(BIG, kind, v)]), \
            f"{kind} {v} {BIG} vs {made_by}"


# ------------------------------------------------------------------------------------------------ rows, draw, check_spec
def test_kinds_and_params_row():
    assert P.KINDS == KINDS
    assert P.params_row("none").tolist() == [0, 0, 0, 0] and P.params_row("invert").tolist() == [2, 0, 0, 0]
    assert P.params_row("posterize", 3).tolist() == [5, 3, 0, 0]
    assert P.params_row("solarize", 109.7).tolist() == [4, 110, 0, 0] and P.params_row("solarize", 110).tolist() == [4, 110, 0, 0]
    assert P.params_row("solarize", 109.00000001).tolist() == [4, 110, 0, 0] and P.params_row("solarize", 0).tolist() == [4, 0, 0, 0]
    for kind in P.FACTOR:
        row = P.params_row(kind, 1.4)
        assert row.dtype == np.int32 and row.shape == (4,) and row[0] == KINDS[kind] and row[2] == row[3] == 0
        assert row[1:2].view(np.float32)[0] == np.float32(1.4)
    for bad in (("invert", 1.0), ("contrast", None), ("contrast", -0.1), ("color", 16.5), ("sharpness", float("nan")),
                ("brightness", float("inf")), ("solarize", 256.5), ("solarize", -1), ("posterize", 9), ("posterize", 2.5),
                ("sharpen", 3), ("contrast", "1")):
        with pytest.raises(ValueError):
            P.params_row(*bad)


def test_draw_stays_inside_the_references_ranges():
    g = np.random.default_rng(5)
    seen = {k: [] for k in KINDS if k != "none"}
    for _ in range(4500):
        kind, v = P.draw(g)
        seen[kind].append(v)
    assert min(len(v) for v in seen.values()) > 350
    assert all(v is None for k in P.VALUELESS for v in seen[k])
    assert all(isinstance(v, float) and 0 <= v < 110 for v in seen["solarize"])
    assert all(isinstance(v, int) for v in seen["posterize"]) and set(seen["posterize"]) == {3, 4, 5, 6, 7}
    assert all(isinstance(v, float) and 0.5 <= v < 1.5 for k in P.FACTOR for v in seen[k])
    assert {P.draw(g, kinds=("color",))[0] for _ in range(20)} == {"color"}
    for bad in ((), ("noise",), ("none",), ("jpeg",)):
        with pytest.raises(ValueError):
            P.draw(g, kinds=bad)
    for kind, vals in seen.items():
        assert PT.check_spec((kind, vals[0])) == [(kind, vals[0])]
    assert PT.draw.__defaults__ == (("jpeg", "blur"),)
    assert {PT.draw(g)[0] for _ in range(50)} == {"jpeg", "blur"}
    assert {PT.draw(g, kinds=("jpeg", "equalize"))[0] for _ in range(50)} == {"jpeg", "equalize"}


def test_check_spec_takes_the_new_kinds_and_still_refuses_the_rest():
    assert PT.check_spec(("contrast", 1.4)) == [("contrast", 1.4)]
    assert PT.check_spec([("jpeg", 70), ("contrast", 1), ("blur", 2), ("equalize", None), ("posterize", 4.0), ("solarize", 128)]) == \
        [("jpeg", 70), ("contrast", 1.0), ("blur", 2.0), ("equalize", None), ("posterize", 4), ("solarize", 128.0)]
    assert PT.check_spec([("autocontrast", None), ("invert", None), ("color", 0), ("brightness", 16), ("sharpness", 0.5)]) == \
        [("autocontrast", None), ("invert", None), ("color", 0.0), ("brightness", 16.0), ("sharpness", 0.5)]
    for bad in (("sharpen", 3), ("blur",), "contrast", "equalize", ("equalize",), ("equalize", 1), ("invert", 0), ("autocontrast", 0.5),
                ("contrast", None), ("contrast", -0.5), ("contrast", 16.01), ("color", float("nan")), ("brightness", float("inf")),
                ("solarize", 257), ("solarize", -0.5), ("solarize", None), ("posterize", 9), ("posterize", -1), ("posterize", 3.5),
                ("none", None), ("contrast", 1.0, 2.0), [("jpeg", 70), "contrast"], (7, 1.0)):
        with pytest.raises(ValueError):
            PT.check_spec(bad)


# ------------------------------------------------------------------------------------------------ header and binding
HEADER = "mumpy_photometric.h"


def test_the_header_declares_exactly_the_pinned_names():
    import abi_surface as S
    assert names_of(HEADER) == dict(ARGS, mumpy_photometric_version=[])
    for kind, code in KINDS.items():
        assert S.define(HEADER, f"MUMPY_PHOTO_{kind.upper()}") == code


def test_header_binding_and_exports_agree():
    import ctypes
    import abi_surface as S
    from mumpy_hip import lib as L
    s = L.PHOTOMETRIC
    assert s.header == HEADER and s not in L.SURFACES and s is not L.PERTURB
    assert not set(s.signatures) & (set(L.SIGNATURES) | set(L.PERTURB.signatures))
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
    assert S.define(HEADER, "MUMPY_PHOTOMETRIC_VERSION") == s.version == getattr(shipped, s.version_fn)() == \
        getattr(tuning, s.version_fn)() == 1


def test_no_name_of_this_header_lives_in_another():
    import abi_surface as S
    from mumpy_hip import lib as L
    for other in L.SURFACES + [L.PERTURB]:
        assert not set(S.decls(HEADER)) & set(S.decls(other.header)), other.header
        assert other.version_fn != L.PHOTOMETRIC.version_fn


def test_a_stale_library_is_refused_by_this_headers_name(monkeypatch):
    from mumpy_hip import lib as L
    monkeypatch.setattr(L, "_LIB", None)
    monkeypatch.setattr(L, "PHOTOMETRIC", L.PHOTOMETRIC._replace(version=2))
    with pytest.raises(RuntimeError) as e:
        L.load_library()
    assert HEADER in str(e.value) and "rebuild" in str(e.value) and L._LIB is None


# ------------------------------------------------------------------------------------------------ refusals through the C ABI
A = 4096                                     # a fake, 16-byte aligned, never dereferenced address: every call below is refused
ENTRY = "mumpy_photometric_u8_fwd"


def _lib():
    from mumpy_hip.lib import load_library
    return load_library()


def _valid():
    return dict(src=A, dst=A, params=A, workspace=A, workspace_bytes=int(_lib().mumpy_photometric_workspace_bytes(2, 19, 21)),
                nimg=2, H=19, W=21, stream=None)


def _refused(code, word, **change):
    lib = _lib()
    args = dict(_valid(), **change)
    assert list(args) == ARGS[ENTRY]
    rc = getattr(lib, ENTRY)(*args.values())
    msg = lib.mumpy_last_error().decode()
    assert rc == code, f"{ENTRY}({change}): rc={rc}, expected {code}: {msg}"
    assert word in msg, f"{ENTRY}({change}): message {msg!r} lacks {word!r}"


def test_workspace_query():
    fn = _lib().mumpy_photometric_workspace_bytes
    one = fn(1, 19, 21)
    assert one >= 3 * 256 + (3 * 256 + 1) * 4 + 19 * 21 * 3 and one % 16 == 0          # a table, one slab of statistics, a copy
    assert fn(3, 19, 21) == 3 * one and fn(0, 5, 5) == 0
    assert fn(1, 1080, 1920) < 2 * 1080 * 1920 * 3
    assert fn(-1, 8, 8) == EINVAL and fn(1, 0, 8) == EINVAL and fn(1, 8, 0) == EINVAL and fn(1, -3, 8) == EINVAL
    assert fn(1 << 31, 8, 8) == ERANGE and fn(1, 4097, 4096) == ERANGE and fn(1, 1 << 15, 1 << 15) == ERANGE
    assert fn(1, 4096, 4096) > 0 and fn(1, 1, 1 << 24) > 0


def test_refusals():
    for p in ("src", "dst", "params", "workspace"):
        _refused(ENULL, "null", **{p: None})
    for p in ("params", "workspace"):
        _refused(EALIGN, "aligned", **{p: A + 4})
    _refused(EINVAL, "nimg", nimg=-1)
    _refused(EINVAL, "0x21", H=0)
    _refused(EINVAL, "19x0", W=0)
    _refused(EINVAL, "-19x21", H=-19)
    _refused(EINVAL, "workspace", workspace_bytes=_valid()["workspace_bytes"] - 1)
    _refused(EINVAL, "workspace", workspace_bytes=0)
    _refused(ERANGE, "2^24", H=4097, W=4096, workspace_bytes=1 << 62)
    _refused(ERANGE, "2^31", nimg=1 << 31, workspace_bytes=1 << 62)
    nbytes = 2 * 19 * 21 * 3
    for off in (1, 19 * 21 * 3, nbytes - 1):                                     # partial overlap, either way round
        _refused(EINVAL, "overlaps", dst=A + off)
        _refused(EINVAL, "overlaps", src=A + off)


def test_zero_images_is_a_valid_call_that_launches_nothing():
    assert _lib().mumpy_photometric_u8_fwd(A, A, A, A, 0, 0, 8, 8, None) == 0
