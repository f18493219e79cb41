"""CPU only: the host half of mask cleaning (mumpy_hip.postprocess; include/mumpy_postprocess.h).

  * the numpy statement `clean` against scipy.ndimage (label with the matching structure, bincount, border test; importorskip only
    there) and, unconditionally, against tests/golden/mask_clean.npz, which records the scipy version its bytes came from: every
    pattern x connectivity x setting of tests/golden/gen_mask_clean_goldens.py, array_equal throughout;
  * max_hole = -1 against binary_fill_holes; the order of the two steps; areas exactly at each threshold; bytes other than 0 / 255;
  * params_row, check_spec; the header's pinned names, its record lib.POSTPROCESS and the exports of both libraries;
  * every refusal of the new entries through the C ABI (nothing is launched for a refused call, so this is safe without a device)."""
import hashlib
import os

import numpy as np
import pytest

from abi_surface import names_of
from conftest import ROOT
from gen_mask_clean_goldens import BIG, CONNS, PATTERNS, SIZES, SMALL, pattern, scipy_clean, settings, size_key
from mumpy_hip import postprocess as P

EINVAL, EALIGN, ENULL, ERANGE = -1, -2, -3, -4
HEADER = "mumpy_postprocess.h"
ARGS = {"mumpy_mask_clean_workspace_bytes": ["nimg", "H", "W"],
        "mumpy_mask_clean_u8_fwd": ["mask", "out", "gt", "counts", "stats", "params", "workspace", "workspace_bytes", "nimg", "H", "W",
                                    "stream"]}


# ------------------------------------------------------------------------------------------------ the numpy statement is scipy's
@pytest.mark.parametrize("hw", SIZES, ids=size_key)
def test_clean_is_the_scipy_construction(hw):
    pytest.importorskip("scipy.ndimage")
    for name in PATTERNS:
        m = pattern(name, hw)
        before = m.copy()
        for conn in CONNS:
            for min_area, max_hole in settings(hw):
                want, want_stats = scipy_clean(m, min_area, max_hole, conn)
                got, stats = P.clean(m, min_area, max_hole, conn)
                assert got.dtype == np.uint8 and got.shape == m.shape and stats.dtype == np.int32 and stats.shape == (8,)
                assert np.array_equal(got, want), f"{name} {hw} conn {conn} ({min_area}, {max_hole}): {int((got != want).sum())} pixels differ"
                assert np.array_equal(stats, want_stats), f"{name} {hw} conn {conn} ({min_area}, {max_hole}): {stats} vs {want_stats}"
                assert set(np.unique(got)) <= {0, 255}
        assert np.array_equal(m, before)


@pytest.mark.parametrize("hw", SIZES, ids=size_key)
def test_the_golden_file_agrees_and_names_its_scipy(hw):
    z = np.load(os.path.join(ROOT, "tests", "golden", "mask_clean.npz"))
    version = str(z["scipy_version"])
    assert version.split(".")[0].isdigit() and tuple(z["patterns"]) == PATTERNS and tuple(z["conns"]) == CONNS
    stats = z["stats_" + size_key(hw)]
    for i, name in enumerate(PATTERNS):
        m = pattern(name, hw)
        if hw != BIG:
            assert np.array_equal(z["in_" + size_key(hw)][i].reshape(hw), m)
        for j, conn in enumerate(CONNS):
            for k, (min_area, max_hole) in enumerate(settings(hw)):
                got, got_stats = P.clean(m, min_area, max_hole, conn)
                what = f"{name} {hw} conn {conn} ({min_area}, {max_hole}) (golden of scipy {version})"
                assert np.array_equal(got_stats, stats[i, j, k]), what
                if hw == BIG:
                    assert hashlib.sha256(got.tobytes()).hexdigest() == str(z["sha256_" + size_key(hw)][i, j, k]), what
                else:
                    assert np.array_equal(np.packbits(got.ravel() != 0), z["bits_" + size_key(hw)][i, j, k]), what


def test_label_is_scipys_label():
    ndi = pytest.importorskip("scipy.ndimage")
    for hw in SMALL + ((64, 48),):
        for name in PATTERNS:
            m = pattern(name, hw)
            for conn in CONNS:
                want, n = ndi.label(m != 0, structure=np.ones((3, 3)) if conn == 8 else None)
                got, k = P.label(m, conn)
                assert k == n and got.dtype == np.int32 and np.array_equal(got, want), (name, hw, conn)
    for bad in (6, 0, None, True):
        with pytest.raises(ValueError):
            P.label(np.zeros((4, 4), np.uint8), bad)
    with pytest.raises(ValueError):
        P.label(np.zeros((2, 4, 4), np.uint8))


def test_the_named_patterns_are_what_they_say():
    assert P.label(pattern("checkerboard", BIG), 4)[1] == 25088 and P.label(pattern("checkerboard", BIG), 8)[1] == 1
    s = pattern("spiral", BIG)
    assert int((s != 0).sum()) == 25312 and P.label(s, 4)[1] == 1
    d = pattern("diagonal_squares", (16, 16))
    assert P.label(d, 4)[1] == 2 and P.label(d, 8)[1] == 1
    r = pattern("rings", (48, 35))
    assert P.label(r, 8)[1] >= 3 and P.label(255 - r, 4)[1] >= 3                   # an object in a hole in an object in a hole
    for hw in ((16, 16), (48, 35), BIG):
        edge, diag = pattern("hole_to_border", hw), pattern("hole_diagonal_to_border", hw)
        for conn in CONNS:
            assert P.clean(edge, 0, -1, conn)[1][3] == 0                           # open through the channel under either rule
        assert P.clean(diag, 0, -1, 8)[1][3] == 1 and P.clean(diag, 0, -1, 4)[1][3] == 0      # a diagonal opens it for 8-connected background


def test_every_hole_filled_is_binary_fill_holes():
    ndi = pytest.importorskip("scipy.ndimage")
    for hw in SMALL + ((64, 48),):
        for name in PATTERNS:
            m = pattern(name, hw)
            assert np.array_equal(P.clean(m, 0, -1, 8)[0] != 0, ndi.binary_fill_holes(m != 0)), (name, hw, 8)
            assert np.array_equal(P.clean(m, 0, -1, 4)[0] != 0, ndi.binary_fill_holes(m != 0, structure=np.ones((3, 3)))), (name, hw, 4)


def _order_case():
    m = np.zeros((16, 16), np.uint8)
    m[2:11, 2:11] = 255
    m[3:10, 3:10] = 0                                                            # a 7 x 7 hole ...
    m[6, 6] = 255                                                                # ... with a one-pixel island
    return m


def test_small_objects_go_before_holes_are_measured():
    m = _order_case()
    for conn in CONNS:
        out, stats = P.clean(m, 2, 48, conn)                                     # the island goes: the hole has 49 pixels, stays open
        assert stats.tolist() == [2, 1, 1, 0, 0, 32, 0, 0] and out[6, 6] == 0 and not out[3:10, 3:10].any()
        out, stats = P.clean(m, 2, 49, conn)
        assert stats.tolist() == [2, 1, 1, 1, 49, 32, 0, 0] and (out[2:11, 2:11] == 255).all() and int((out != 0).sum()) == 81
        out, stats = P.clean(m, 0, 48, conn)                                     # the island kept: the hole has 48 pixels and fills
        assert stats.tolist() == [2, 2, 0, 1, 48, 32, 0, 0] and (out[2:11, 2:11] == 255).all()
        out, stats = P.clean(m, 0, 47, conn)
        assert stats.tolist() == [2, 2, 0, 0, 0, 32, 0, 0] and np.array_equal(out, m)


def test_an_area_at_a_threshold_is_kept_and_filled():
    m = np.zeros((16, 16), np.uint8)
    m[1:3, 1:4] = 255                                                            # an object of 6 pixels
    m[6:12, 6:12] = 255
    m[8:10, 8:11] = 0                                                            # a hole of 6 pixels
    for conn in CONNS:
        assert P.clean(m, 6, 0, conn)[0][1, 1] == 255 and P.clean(m, 6, 0, conn)[1].tolist() == [2, 2, 0, 0, 0, 30, 0, 0]
        assert P.clean(m, 7, 0, conn)[0][1, 1] == 0 and P.clean(m, 7, 0, conn)[1].tolist() == [2, 1, 6, 0, 0, 30, 0, 0]
        assert P.clean(m, 0, 6, conn)[0][8, 8] == 255 and P.clean(m, 0, 6, conn)[1].tolist() == [2, 2, 0, 1, 6, 30, 0, 0]
        assert P.clean(m, 0, 5, conn)[0][8, 8] == 0
        assert np.array_equal(P.clean(m, 1, 0, conn)[0], m) and np.array_equal(P.clean(m, -5, 0, conn)[0], m)
        assert not P.clean(m, 2 ** 31 - 1, -2 ** 31, conn)[0].any()              # everything removed; nothing is left to have holes
        assert np.array_equal(P.clean(m, -2 ** 31, 2 ** 31 - 1, conn)[0] != 0, P.clean(m, 0, -1, conn)[0] != 0)


def test_any_non_zero_byte_is_foreground_and_an_odd_connectivity_means_8():
    m = _order_case()
    g = np.random.default_rng(2)
    odd = np.where(m != 0, g.integers(1, 255, m.shape), 0).astype(np.uint8)
    assert (odd[m != 0] != 255).any()
    for conn in CONNS:
        a, b = P.clean(m, 2, 49, conn), P.clean(odd, 2, 49, conn)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    d = pattern("diagonal_squares", (16, 16))
    for word in (0, 6, -4, 2 ** 31 - 1):
        assert np.array_equal(P.clean(d, 17, 0, word)[0], P.clean(d, 17, 0, 8)[0])
    assert not P.clean(d, 17, 0, 4)[0].any() and P.clean(d, 17, 0, 8)[0].any()
    for bad in (m.astype(np.int32), m[None], m.astype(bool)):
        with pytest.raises(ValueError):
            P.clean(bad, 0, 0, 8)


def test_params_row_and_check_spec():
    assert P.STATS == ("found", "kept", "pixels_removed", "holes_filled", "pixels_filled", "largest_kept", "reserved", "status")
    row = P.params_row(20, -1, 4)
    assert row.dtype == np.int32 and row.tolist() == [20, -1, 4, 0] and P.params_row(0, 50).tolist() == [0, 50, 8, 0]
    assert P.params_row(-2 ** 31, 2 ** 31 - 1, 8).tolist() == [-2 ** 31, 2 ** 31 - 1, 8, 0]
    assert P.params_row(np.int64(3), np.int32(4), 8).tolist() == [3, 4, 8, 0]
    for bad in ((1.5, 0, 8), (0, "3", 8), (0, None, 8), (True, 0, 8), (0, 0, 6), (0, 0, 0), (0, 0, None), (2 ** 31, 0, 8), (0, -2 ** 31 - 1, 8)):
        with pytest.raises(ValueError):
            P.params_row(*bad)
    assert P.check_spec(None) is None
    assert P.check_spec(dict(min_area=20, max_hole=50)) == (20, 50, 8)
    assert P.check_spec(dict(min_area=0, max_hole=-1, connectivity=4), "who") == (0, -1, 4)
    assert P.check_spec(dict(min_area=224 * 224, max_hole=0)) == (224 * 224, 0, 8)
    assert P.check_spec(dict(min_area=256, max_hole=0), "who", (16, 16)) == (256, 0, 8)
    assert P.check_spec(dict(min_area=-3, max_hole=-7)) == (-3, -7, 8)                       # min_area <= 1 removes nothing
    for bad in (dict(min_area=224 * 224 + 1, max_hole=0), dict(min_area=2.0, max_hole=0),
                dict(min_area=2, max_hole=1.5), dict(min_area=2, max_hole=None), dict(min_area=2), dict(max_hole=2),
                dict(min_area=2, max_hole=0, connectivity=6), dict(min_area=2, max_hole=0, connectivity="8"),
                dict(min_area=2, max_hole=0, conn=8), (2, 0, 8), "8", 5, dict(min_area=True, max_hole=0)):
        with pytest.raises(ValueError, match="who"):
            P.check_spec(bad, "who")
    with pytest.raises(ValueError):
        P.check_spec(dict(min_area=257, max_hole=0), "who", (16, 16))


def test_counts_row_is_the_mask_score_layout():
    p = np.array([[255, 0, 255, 0]], np.uint8)
    g = np.array([[7, 9, 0, 0]], np.uint8)
    assert P.counts_row(p, g).tolist() == [1, 2, 2, 3]


def test_the_module_needs_neither_scipy_nor_torch():
    import subprocess
    import sys
    code = ("import sys; sys.modules['scipy'] = None; sys.modules['torch'] = None\n"
            "import importlib.util as u\n"
            f"s = u.spec_from_file_location('pp', {P.__file__!r}); m = u.module_from_spec(s); s.loader.exec_module(m)\n"
            "import numpy as np; a = np.zeros((4, 4), np.uint8); a[1:3, 1:3] = 255\n"
            "assert m.clean(a, 5, 0, 8)[1].tolist() == [1, 0, 4, 0, 0, 0, 0, 0]\n")
    assert subprocess.run([sys.executable, "-c", code]).returncode == 0


# ------------------------------------------------------------------------------------------------ header, binding, exports
def test_the_header_declares_exactly_the_pinned_names():
    import abi_surface as S
    assert names_of(HEADER) == dict(ARGS, mumpy_postprocess_version=[])
    assert S.define(HEADER, "MUMPY_MASK_CLEAN_MAX_PIXELS") == 224 * 224 == P.MAX_PIXELS
    assert not HEADER.startswith("mumpy_hip")


def test_header_binding_and_exports_agree():
    import ctypes
    import abi_surface as S
    from mumpy_hip import lib as L
    s = L.POSTPROCESS
    assert s.header == HEADER and s not in L.SURFACES and s not in (L.PERTURB, L.PHOTOMETRIC, L.GEOMETRIC)
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
    assert S.define(HEADER, "MUMPY_POSTPROCESS_VERSION") == s.version == getattr(shipped, s.version_fn)() == \
        getattr(tuning, s.version_fn)() == 1


def test_no_name_of_this_header_lives_in_another():
    import abi_surface as S
    from mumpy_hip import lib as L
    for other in L.SURFACES + [L.PERTURB, L.PHOTOMETRIC, L.GEOMETRIC]:
        assert not set(S.decls(HEADER)) & set(S.decls(other.header)), other.header
        assert not set(L.POSTPROCESS.signatures) & set(other.signatures), other.header
        assert other.version_fn != L.POSTPROCESS.version_fn


def test_a_stale_library_is_refused_by_this_headers_name(monkeypatch):
    from mumpy_hip import lib as L
    monkeypatch.setattr(L, "_LIB", None)
    monkeypatch.setattr(L, "POSTPROCESS", L.POSTPROCESS._replace(version=2))
    with pytest.raises(RuntimeError) as e:
        L.load_library()
    assert HEADER in str(e.value) and "rebuild" in str(e.value) and L._LIB is None


# ------------------------------------------------------------------------------------------------ refusals through the C ABI
A = 1 << 20                                  # fake, 16-byte aligned, never dereferenced addresses, far apart: every call is refused
B_, G_, C_, S_, P_, W_ = (k << 40 for k in range(1, 7))
ENTRY = "mumpy_mask_clean_u8_fwd"
NIMG, H, W = 3, 5, 48


def _lib():
    from mumpy_hip.lib import load_library
    return load_library()


def _need(nimg=NIMG, h=H, w=W):
    return _lib().mumpy_mask_clean_workspace_bytes(nimg, h, w)


def _valid():
    return dict(mask=A, out=B_, gt=G_, counts=C_, stats=S_, params=P_, workspace=W_, workspace_bytes=_need(), nimg=NIMG, H=H, W=W,
                stream=None)


def _refused(code, word, **change):
    lib = _lib()
    args = dict(_valid(), **change)
    assert list(args) == ARGS[ENTRY]
    rc = getattr(lib, ENTRY)(*args.values())
    msg = lib.mumpy_last_error().decode()
    assert rc == code, f"{ENTRY}({change}): rc={rc}, expected {code}: {msg}"
    assert word in msg, f"{ENTRY}({change}): message {msg!r} lacks {word!r}"


def test_workspace_bytes():
    lib = _lib()
    assert _need() == NIMG * H * W * 4 > 0 and _need(0) == 0 and _need(1, 224, 224) == 4 * 224 * 224
    assert _need(100000, 1, 16) == _need(1 << 30, 1, 16) > 0                     # the launch's grid is capped; the workspace with it
    for args, code in (((-1, H, W), EINVAL), ((1, 0, 16), EINVAL), ((1, 16, 0), EINVAL), ((1, -4, -4), EINVAL), ((1, 3, 5), EINVAL),
                       ((1, 7, 8), EINVAL), ((1, 224, 225), ERANGE), ((1, 1, 224 * 224 + 16), ERANGE), ((1, 1 << 16, 1 << 16), ERANGE),
                       ((1 << 31, H, W), ERANGE)):
        assert lib.mumpy_mask_clean_workspace_bytes(*args) == code, args
        assert lib.mumpy_last_error().decode()


def test_refusals():
    for p in ("mask", "out", "params", "workspace"):
        _refused(ENULL, "null", **{p: None})
    _refused(ENULL, "null gt or counts", gt=None)
    _refused(ENULL, "null gt or counts", counts=None)
    for p in ("mask", "out", "gt", "params", "workspace"):
        for off in (1, 4, 8):
            _refused(EALIGN, "aligned", **{p: _valid()[p] + off})
    _refused(EINVAL, "nimg", nimg=-1)
    _refused(EINVAL, "0x48", H=0)
    _refused(EINVAL, "5x0", W=0)
    _refused(EINVAL, "-5x48", H=-5)
    _refused(EINVAL, "multiple of 16", H=3, W=5)
    _refused(EINVAL, "multiple of 16", H=7, W=8)
    _refused(ERANGE, "2^31", nimg=1 << 31)
    _refused(ERANGE, "pixels", H=224, W=225)
    _refused(ERANGE, "pixels", H=1 << 16, W=1 << 16)                             # the product is taken in 64 bits
    nbytes = NIMG * H * W
    for off in (16, H * W, nbytes - 16):                                         # partial overlap, either way round
        _refused(EINVAL, "overlaps", out=A + off)
        _refused(EINVAL, "overlaps", mask=B_ + off)
    _refused(EINVAL, "too small", workspace_bytes=_need() - 1)
    _refused(EINVAL, "too small", workspace_bytes=0)
    _refused(EINVAL, "too small", workspace_bytes=-1)


def test_zero_images_is_a_valid_call_that_launches_nothing():
    lib = _lib()
    assert lib.mumpy_mask_clean_u8_fwd(A, B_, G_, C_, S_, P_, None, 0, 0, H, W, None) == 0
    assert lib.mumpy_mask_clean_u8_fwd(A, A, None, None, None, P_, None, 0, 0, 224, 224, None) == 0
