"""CPU: every public header of include/ against its record in lib.SURFACES and against the exports of the shipped and the tuning
library; the version-mismatch path of load_library.  No compute calls (no GPU here)."""
import ctypes
import glob
import itertools
import os

import pytest

import abi_surface as S
from conftest import ROOT
from mumpy_hip import lib as L

# literals, so that a header and its record cannot drift together unnoticed (mumpy_hip.h: 2 since mumpy_layernorm_bwd grew dx_add /
# accumulate; ext2: 2 since the fused-MLP entries)
VERSIONS = {"mumpy_hip.h": 2, "mumpy_hip_ext.h": 1, "mumpy_hip_ext2.h": 2, "mumpy_hip_ext3.h": 1, "mumpy_hip_ext4.h": 1,
            "mumpy_hip_ext5.h": 1, "mumpy_hip_ext6.h": 1, "mumpy_hip_ext7.h": 1, "mumpy_hip_ext8.h": 1, "mumpy_hip_ext9.h": 1,
            "mumpy_hip_ext10.h": 1}
HAND_BOUND = {"mumpy_hip.h": {"mumpy_last_error", "mumpy_last_route"}}          # load_library binds these two itself


def test_header_declares_expected_entry_points():
    d = S.decls("mumpy_hip.h")
    for name in ("mumpy_window_attention_fwd", "mumpy_deform_sample_fwd", "mumpy_deform_attention_fwd", "mumpy_faf_fwd",
                 "mumpy_patch_embed_fwd", "mumpy_linear_fwd", "mumpy_layernorm_fwd", "mumpy_last_error"):
        assert name in d


@pytest.mark.parametrize("s", L.SURFACES, ids=[s.header for s in L.SURFACES])
def test_surface_header_binding_and_exports_agree(s):
    """Per header: every declared name is exported by both libraries; the bound names are the declared ones minus the version
    function (and what load_library binds by hand); every bound argument and the return type have the ctypes kind of the C
    declaration (a float/double or int/int64 slip corrupts the call); the version agrees everywhere."""
    assert os.path.exists(L.library_path()) and os.path.exists(L.tuning_library_path()), "build with `python __graft_entry__.py`"
    declared = S.decls(s.header)
    shipped, tuning = L.load_library(), ctypes.CDLL(L.tuning_library_path())
    for name in declared:
        assert hasattr(shipped, name) and hasattr(tuning, name), f"{name} declared in {s.header} but not exported"
    assert set(s.signatures) == set(declared) - {s.version_fn} - HAND_BOUND.get(s.header, set())
    for name, args in s.signatures.items():
        got, want = [S.ckind(t) for t in args], [S.kind(a) for a in declared[name].args]
        assert got == want, f"{name}: binding {got} vs header {want}"
        got, want = S.ckind(getattr(shipped, name).restype), S.kind(declared[name].ret)
        assert got == want, f"{name}: binding returns {got}, header {want}"
    assert declared[s.version_fn] == S.Decl("int", [])
    getattr(tuning, s.version_fn).restype = ctypes.c_int
    in_header = S.define(s.header, s.version_fn.upper())                        # mumpy_ext2_version <-> MUMPY_EXT2_VERSION
    assert in_header == s.version == getattr(shipped, s.version_fn)() == getattr(tuning, s.version_fn)() == VERSIONS[s.header]


def test_no_name_lives_in_two_surfaces_and_no_header_is_forgotten():
    for a, b in itertools.combinations(L.SURFACES, 2):
        assert not set(S.decls(a.header)) & set(S.decls(b.header)), f"declared in {a.header} and {b.header}"
        assert not set(a.signatures) & set(b.signatures), f"bound for {a.header} and {b.header}"
        assert a.version_fn != b.version_fn
    assert len(L.SIGNATURES) == sum(len(s.signatures) for s in L.SURFACES) and L.ABI_VERSION == L.SURFACES[0].version
    on_disk = sorted(os.path.basename(p) for p in glob.glob(os.path.join(ROOT, "include", "mumpy_hip*.h")))
    assert on_disk == sorted(s.header for s in L.SURFACES) == sorted(VERSIONS)


def test_version_mismatch_fails_loudly(monkeypatch):
    """A library whose answer for one header differs from the binding's record is refused by name, with the way out."""
    stale = L.SURFACES[4]
    monkeypatch.setattr(L, "_LIB", None)
    monkeypatch.setattr(L, "SURFACES", [s._replace(version=s.version + 1) if s is stale else s for s in L.SURFACES])
    with pytest.raises(RuntimeError) as e:
        L.load_library()
    msg = str(e.value)
    assert stale.header in msg and "rebuild" in msg and L.library_path() in msg
    assert str(stale.version) in msg and str(stale.version + 1) in msg
    assert L._LIB is None                                                       # nothing half-loaded is kept


def test_argument_validation_without_gpu():
    """Rejected arguments return negative codes before anything is launched, so this is safe on a CPU box."""
    from mumpy_hip.lib import load_library
    lib = load_library()
    rc = lib.mumpy_layernorm_fwd(None, None, None, None, 4, 96, 1e-5, None)
    assert rc == -3 and b"null" in lib.mumpy_last_error()
    rc = lib.mumpy_linear_fwd(16, 16, None, None, 16, 4, 100, 96, 0, None)        # N % 32 != 0
    assert rc == -1
    rc = lib.mumpy_window_attention_fwd(16, 16, 16, None, None, 0, 1, 10, 14, 96, 0, 0.1, None)   # grid not /7
    assert rc == -1
    rc = lib.mumpy_temporal_attention_fwd(16, 16, 4, 17, 768, 12, 0.125, None)    # T > 16
    assert rc == -4


def test_missing_library_fails_loudly(monkeypatch, tmp_path):
    import mumpy_hip.lib as L
    monkeypatch.setattr(L, "_LIB", None)
    monkeypatch.setenv("MUMPY_HIP_LIB", str(tmp_path / "nope.so"))
    with pytest.raises(RuntimeError, match="no CPU/torch fallback"):
        L.load_library()


@pytest.mark.parametrize("src,dst", [(432, 224), (240, 224), (1920, 224), (1080, 224), (224, 224), (37, 224), (854, 448)])
def test_resize_nearest_table_is_pillows(src, dst):
    """The host helper behind mumpy_resize_normalize_u8_fwd reproduces PIL's NEAREST source indices (incl. the exact ties
    that Pillow's double accumulator decides, e.g. 1920 -> 224): checked against PIL resizing an index ramp."""
    import numpy as np
    from PIL import Image
    from mumpy_hip.lib import load_library
    lib = load_library()
    tab = (ctypes.c_int32 * dst)()
    assert lib.mumpy_resize_nearest_table(src, dst, tab) == 0
    ramp = np.arange(src, dtype=np.int32).reshape(1, src)                     # mode "I": pixel value = source column
    pil = np.array(Image.fromarray(ramp, mode="I").resize((dst, 1), Image.NEAREST)).reshape(-1)
    assert list(tab) == pil.tolist()


def test_shipped_library_reads_no_environment_and_the_tuning_build_exists():
    """The shipped libmumpy_hip.so is built without the tuning hooks (mumpy_tuning_build() == 0: no getenv in the library, the
    planner is a pure function of the shape); the diagnostics build that tools/ and the variant tests select with MUMPY_HIP_LIB is
    a separate file with the same exported symbols."""
    import os
    import subprocess
    from mumpy_hip.lib import library_path, load_library, tuning_library_path
    assert load_library().mumpy_tuning_build() == 0
    nm = subprocess.run(["nm", "-D", "--undefined-only", library_path()], capture_output=True, text=True).stdout
    assert "getenv" not in nm
    assert os.path.exists(tuning_library_path()), "run `python __graft_entry__.py` (builds both libraries)"
    t = ctypes.CDLL(tuning_library_path())
    assert t.mumpy_tuning_build() == 1 and t.mumpy_abi_version() == load_library().mumpy_abi_version()


def test_gemm_planner_matches_the_recorded_values():
    """mumpy_linear_workspace_bytes and mumpy_linear_ln_tiles are pure host functions of the shape (the planner of csrc/gemm.hip at
    256 CUs: the MI355X's count, and the fall-back without a device).  Their values over an M x N x K sweep are recorded in
    tests/golden/gemm_planner.json; a change of the launch layer must not move any of them."""
    import json
    from mumpy_hip.lib import load_library
    lib = load_library()
    with open(os.path.join(ROOT, "tests", "golden", "gemm_planner.json")) as f:
        gold = json.load(f)
    shapes = [(m, n, k) for m in gold["M"] for n in gold["N"] for k in gold["K"]]
    assert len(shapes) == 640 == len(gold["workspace_bytes"]) == len(gold["ln_tiles"])
    assert [int(lib.mumpy_linear_workspace_bytes(*s)) for s in shapes] == gold["workspace_bytes"]
    assert [int(lib.mumpy_linear_ln_tiles(*s)) for s in shapes] == gold["ln_tiles"]


def test_gemm_bwd_planner_matches_the_recorded_values():
    """mumpy_linear_bwd_workspace_bytes and mumpy_conv2d_wgrad_workspace_bytes are pure host functions of the shape (the planner and
    the workspace layout of csrc/gemm_bwd.hip).  Their values over the sweeps of tests/golden/gemm_bwd_planner.json were recorded
    before the launch layer of that file was refactored; a change of it must not move any of them."""
    import json
    from mumpy_hip.lib import load_library
    lib = load_library()
    with open(os.path.join(ROOT, "tests", "golden", "gemm_bwd_planner.json")) as f:
        gold = json.load(f)
    lin, conv = gold["linear_bwd"], gold["conv2d_wgrad"]
    shapes = [(m, n, k) for m in lin["M"] for n in lin["N"] for k in lin["K"]]
    assert len(shapes) == 832 == len(lin["workspace_bytes"])
    assert [int(lib.mumpy_linear_bwd_workspace_bytes(*s)) for s in shapes] == lin["workspace_bytes"]
    convs = [(b, h, w, ci, co, kh, kw) for b in conv["B"] for h, w in conv["HW"] for ci, co in conv["CinCout"] for kh, kw in conv["taps"]]
    assert len(convs) == 192 == len(conv["workspace_bytes"])
    assert [int(lib.mumpy_conv2d_wgrad_workspace_bytes(*s)) for s in convs] == conv["workspace_bytes"]
