"""The fused MLP of the training tape (include/mumpy_hip_ext2.h, version 2): mumpy_linear_gelu_dual_fwd writes z = x W^T + b and
a = gelu(z) from one launch, mumpy_linear_gelu_bwd takes gelu'(z) into the dX product of fc2's backward; ops.set_mlp_fusion /
MUMPY_MLP_FUSED routes the three MLP sites of mumpy_hip.autograd through autograd.MlpFn.

CPU: header, binding, exports and version; every refusal, with nothing launched; the switch.  GPU, per op: every forward route the
planner gives a GELU launch and both wave tiles of the backward, split and unsplit, against float64 and against the unfused
launches; memory discipline under tests/guarded_alloc.py.  GPU, tape: the three blocks, the full model and the graphed step with the
switch on against off.

Tolerances.  2e-5 (conftest.rel_err) against float64 is the bar of test_hip_linear_bwd_one_call / test_hip_linear_bwd_bf16_operands /
test_hip_gelu_fwd_bwd for the same products and the same erf approximation.  Against the unfused pair dz differs by at most a few
fp32 roundings of the same expression (1e-6); dW and db are the same launches on the same operands (bitwise)."""
import contextlib
import functools
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import guarded_alloc as GA
from conftest import ROOT, rel_err
from weight_fill import fill_module_, seeded_randn

gpu = pytest.mark.gpu
PKG = os.path.join(ROOT, "multilateral-temporal-view-pyramid-transformer-for-video-inpainting-detection_amd")
FWD, BWD, WSQ = "mumpy_linear_gelu_dual_fwd", "mumpy_linear_gelu_bwd", "mumpy_linear_gelu_bwd_workspace_bytes"
EINVAL, EALIGN, ENULL, ERANGE = -1, -2, -3, -4
MATH_BF16 = 0x100

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")


@contextlib.contextmanager
def _modes(fused=None, math=None):
    from mumpy_hip import ops
    f0, m0 = ops.mlp_fusion(), ops.matrix_math()
    try:
        if fused is not None:
            ops.set_mlp_fusion(fused)
        if math is not None:
            ops.set_matrix_math(math)
        yield
    finally:
        ops.set_mlp_fusion(f0)
        ops.set_matrix_math(m0)


def _route():
    from mumpy_hip.lib import load_library
    return load_library().mumpy_last_route().decode()


# ------------------------------------------------------------------ CPU: header, binding, exports, version
def test_header_declares_the_pinned_argument_names():
    """(tests/test_abi.py holds mumpy_hip_ext2.h, version 2, to its binding and to both libraries.)"""
    from abi_surface import names_of
    ext2 = names_of("mumpy_hip_ext2.h")
    assert {FWD, BWD, WSQ} <= set(ext2)
    assert ext2[FWD] == ["x", "W", "bias", "z", "a", "M", "N", "K", "math", "workspace", "workspace_bytes", "stream"]
    assert ext2[BWD] == ["a", "z", "W", "dy", "dz", "dW", "db", "M", "N", "K", "accumulate", "workspace", "workspace_bytes", "stream"]


def test_refusals_need_no_gpu():
    """Every refusal the header states returns its code with a message of this entry and launches nothing: each tuple below is
    refused, so the stand-in addresses are never dereferenced, with or without a device."""
    from mumpy_hip.lib import load_library
    lib = load_library()
    fwd, bwd, wsq = getattr(lib, FWD), getattr(lib, BWD), getattr(lib, WSQ)
    P = [0x100000 * (i + 1) for i in range(8)]                  # distinct, 16-byte aligned, far apart, never dereferenced
    m, n, k = 64, 128, 32

    def refused(fn, who, ok, i, v, code):
        assert lib.mumpy_add_fwd(None, None, None, 16, None) < 0        # the message is sticky per thread: leave a known one
        stale = lib.mumpy_last_error()
        rc = fn(*(ok[:i] + (v,) + ok[i + 1:]))
        err = lib.mumpy_last_error()
        assert rc == code and err != stale and who in err, (who, i, v, rc, err)

    # ---- forward: x, W, bias, z, a, M, N, K, math, workspace, workspace_bytes, stream
    need_f = lib.mumpy_linear_workspace_bytes(37, 3072, 768)
    assert need_f > 0
    ok = (P[0], P[1], P[2], P[3], P[4], m, n, k, 0, None, 0, None)
    for i in (0, 1, 3, 4):
        refused(fwd, b"linear_gelu_dual", ok, i, None, ENULL)
    for i in (0, 1, 2, 3, 4, 9):
        refused(fwd, b"linear_gelu_dual", ok, i, P[5] + 4, EALIGN)
    for math in (0x200, 0x400, 0x300, 1, -1, 0x101):             # the split-precision modes, an act bit, garbage
        refused(fwd, b"linear_gelu_dual", ok, 8, math, EINVAL)
    refused(fwd, b"linear_gelu_dual", ok, 6, n + 1, EINVAL)      # N % 32
    refused(fwd, b"linear_gelu_dual", ok, 7, k + 1, EINVAL)      # K % 32
    refused(fwd, b"linear_gelu_dual", ok, 5, -1, EINVAL)
    refused(fwd, b"linear_gelu_dual", ok, 5, 1 << 31, ERANGE)    # the M range of the forward GEMMs
    refused(fwd, b"linear_gelu_dual", ok, 4, P[3], EINVAL)       # z == a
    refused(fwd, b"linear_gelu_dual", ok, 10, -1, EINVAL)
    deep = (P[0], P[1], P[2], P[3], P[4], 37, 3072, 768, 0, P[5], need_f - 1, None)
    refused(fwd, b"linear_gelu_dual", deep, 10, need_f - 1, EINVAL)      # a workspace that is too small
    assert fwd(*(ok[:5] + (0,) + ok[6:])) == 0                   # empty batch: accepted, nothing to do

    # ---- backward: a, z, W, dy, dz, dW, db, M, N, K, accumulate, workspace, workspace_bytes, stream
    mb, nb, kb = 50, 768, 3072
    need = wsq(mb, nb, kb)
    assert need == lib.mumpy_linear_bwd_workspace_bytes(mb, nb, kb) > 0
    assert wsq(0, nb, kb) == 0 and wsq(mb, 0, kb) == 0 and wsq(mb, nb, -1) == 0
    ok = (P[0], P[1], P[2], P[3], P[4], P[5], P[6], mb, nb, kb, 0, P[7], need, None)
    refused(bwd, b"linear_gelu_bwd", ok, 3, None, ENULL)         # dy
    refused(bwd, b"linear_gelu_bwd", ok, 1, None, ENULL)         # z is required when dz is wanted
    refused(bwd, b"linear_gelu_bwd", ok, 2, None, ENULL)         # ... and W
    refused(bwd, b"linear_gelu_bwd", ok, 0, None, ENULL)         # a is required when dW is wanted
    nothing = ok[:4] + (None, None, None) + ok[7:]
    refused(bwd, b"linear_gelu_bwd", nothing, 4, None, ENULL)    # no gradient asked for
    for i in (0, 1, 2, 3, 4, 5, 6, 11):
        refused(bwd, b"linear_gelu_bwd", ok, i, P[7] + 0x1000004, EALIGN)
    refused(bwd, b"linear_gelu_bwd", ok, 8, nb + 1, EINVAL)      # N % 32
    refused(bwd, b"linear_gelu_bwd", ok, 9, kb + 1, EINVAL)      # K % 32
    refused(bwd, b"linear_gelu_bwd", ok, 7, -1, EINVAL)
    refused(bwd, b"linear_gelu_bwd", ok, 7, (1 << 31) - 256, EINVAL)     # the M range of mumpy_linear_bwd
    refused(bwd, b"linear_gelu_bwd", ok, 10, 4, EINVAL)          # unknown accumulate bits
    refused(bwd, b"linear_gelu_bwd", ok, 10, 0x200, EINVAL)      # a split-precision mode
    refused(bwd, b"linear_gelu_bwd", ok, 12, need - 1, EINVAL)   # workspace too small
    refused(bwd, b"linear_gelu_bwd", ok, 1, P[0], EINVAL)        # z == a
    for other in (0, 1, 3):                                      # dz aliasing a, z, dy -- the same address, and overlapping ranges
        refused(bwd, b"linear_gelu_bwd", ok, 4, ok[other], EINVAL)
        refused(bwd, b"linear_gelu_bwd", ok, 4, ok[other] + 64, EINVAL)
        refused(bwd, b"linear_gelu_bwd", ok, 4, ok[other] - 64, EINVAL)
    assert bwd(*(ok[:7] + (0,) + ok[8:])) == 0                   # empty batch


def test_switch_default_setter_and_bad_values():
    from mumpy_hip import autograd as AG, ops
    assert os.environ.get("MUMPY_MLP_FUSED", "") in ("", "0", "1")
    before = ops.mlp_fusion()
    assert before is (os.environ.get("MUMPY_MLP_FUSED", "") == "1")
    try:
        ops.set_mlp_fusion(True)
        assert ops.mlp_fusion() is True
        ops.set_mlp_fusion(False)
        assert ops.mlp_fusion() is False
        for bad in ("1", "on", None, 2, 1.0):
            with pytest.raises(ValueError):
                ops.set_mlp_fusion(bad)
        assert ops.mlp_fusion() is False
        math, attn, cva = ops.matrix_math(), ops.attention_math(), ops.cva_math()      # independent of the other switches
        ops.set_mlp_fusion(True)
        assert (ops.matrix_math(), ops.attention_math(), ops.cva_math()) == (math, attn, cva)
    finally:
        ops.set_mlp_fusion(before)
    assert hasattr(AG, "MlpFn")


@pytest.mark.parametrize("value,ok", [("", False), ("0", False), ("1", True), ("2", None), ("true", None), ("on", None)])
def test_switch_environment_in_a_fresh_process(value, ok):
    env = dict(os.environ, MUMPY_MLP_FUSED=value, PYTHONPATH=os.pathsep.join([PKG, os.environ.get("PYTHONPATH", "")]))
    r = subprocess.run([sys.executable, "-c", "from mumpy_hip import ops; print('FUSED', ops.mlp_fusion())"], env=env,
                       capture_output=True, text=True, timeout=300)
    if ok is None:
        assert r.returncode != 0 and "MUMPY_MLP_FUSED" in r.stderr and "ValueError" in r.stderr, (r.stdout, r.stderr[-500:])
    else:
        assert r.returncode == 0 and f"FUSED {ok}" in r.stdout, (r.stdout, r.stderr[-500:])


# ------------------------------------------------------------------ GPU, per op: the forward
# (math, M, K) with N = 4 K -> the route.  Small shapes that reach each route the planner gives an act = GELU launch, from a
# host-side scan of it (K = 32 .. 1536 in 14 steps; M = 1 .. 400 in steps of 7, .. 4200 in steps of 25, .. 34000 in steps of 333;
# with and without the workspace): the tiled 64x64 kernel whole and split-K 2 / 3 / 4 (+ its reduce), the 8-wave 128x128 tile (a
# band of M where 128x128 tiles fill too little of a round for the persistent kernel and 64x64 tiles need one round more), the
# 128x128 LDS-DMA tile, the persistent kernel's whole-tile schedule at each of its P and its split schedule; in bf16 operand mode
# the two tiles of that family and its split-K.  37 and 130 are ragged everywhere; 1100 = 8 x 128 + 76, 1800 = 14 x 128 + 8 and
# 700 = 5 x 128 + 60 end inside a tile; 1000, 4000 and 7840 are no multiple of 128 either.
FWD_CASES = [
    ("fp32", 37, 32, "tiled tile=2 ks=1 np=0 addr=dense dual=z"),
    ("fp32", 130, 64, "tiled tile=2 ks=1 np=0 addr=dense dual=z"),
    ("fp32", 37, 768, "tiled tile=2 ks=2 np=0 addr=dense dual=z"),
    ("fp32", 130, 1536, "tiled tile=2 ks=3 np=0 addr=dense dual=z"),
    ("fp32", 1, 1536, "tiled tile=2 ks=4 np=0 addr=dense dual=z"),
    ("fp32", 1100, 768, "tiled tile=0 ks=1 np=0 addr=dense dual=z"),
    ("fp32", 1800, 1024, "tiled tile=3 ks=1 np=0 addr=dense dual=z"),
    ("fp32", 1000, 1024, "ws sched=whole P=1 ln=none addr=dense dual=z"),
    ("fp32", 7840, 384, "ws sched=whole P=2 ln=none addr=dense dual=z"),
    ("fp32", 4000, 256, "ws sched=whole P=4 ln=none addr=dense dual=z"),
    ("fp32", 7840, 128, "ws sched=whole P=8 ln=none addr=dense dual=z"),
    ("fp32", 700, 1024, "ws sched=split P=4 ln=none addr=dense dual=z"),
    ("bf16", 37, 32, "tiled tile=2 ks=1 np=1 addr=dense dual=z"),
    ("bf16", 37, 768, "tiled tile=2 ks=2 np=1 addr=dense dual=z"),
    ("bf16", 130, 1536, "tiled tile=2 ks=3 np=1 addr=dense dual=z"),
    ("bf16", 1100, 768, "tiled tile=0 ks=1 np=1 addr=dense dual=z"),
    ("bf16", 1000, 1024, "tiled tile=0 ks=1 np=1 addr=dense dual=z"),
]


@functools.lru_cache(maxsize=None)
def _fwd_inputs(m, k):
    n = 4 * k
    return seeded_randn(3100 + k, m, k), seeded_randn(3200 + k, n, k) / k ** 0.5, seeded_randn(3300 + k, n)


@gpu
@pytest.mark.parametrize("math,m,k,route", FWD_CASES)
def test_dual_forward_every_route(math, m, k, route):
    from mumpy_hip import ops
    x, w, b = _fwd_inputs(m, k)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    x0, w0, b0 = xd.clone(), wd.clone(), bd.clone()
    with _modes(math=math):
        z, a = ops.linear_gelu_dual(xd, wd, bd)
        got = _route()
        z_plain = ops.linear(xd, wd, bd)
        a_plain = ops.linear(xd, wd, bd, act=ops.ACT_GELU)
        sibling = _route()
        z2, a2 = ops.linear_gelu_dual(xd, wd, bd)
    torch.cuda.synchronize()
    assert got == route
    assert z.shape == a.shape == (m, 4 * k) and z.dtype == a.dtype == torch.float32
    assert torch.equal(z, z_plain)
    assert sibling + " dual=z" == got and torch.equal(a, a_plain)           # the same plan, the same arithmetic in the same epilogue
    assert torch.equal(z, z2) and torch.equal(a, a2)
    assert torch.equal(xd, x0) and torch.equal(wd, w0) and torch.equal(bd, b0)
    xr, wr = (x.bfloat16().double(), w.bfloat16().double()) if math == "bf16" else (x.double(), w.double())
    zr = xr @ wr.t() + b.double()
    ez, ea = rel_err(z.cpu(), zr), rel_err(a.cpu(), F.gelu(zr))
    print(f"dual fwd {math} M={m} K={k}: {got}: rel err z {ez:.2e}, a {ea:.2e}")
    assert ez < 2e-5 and ea < 2e-5


@gpu
@pytest.mark.parametrize("math,m,k", [(c[0], c[1], c[2]) for c in FWD_CASES if (c[1], c[2]) != (130, 64)])
def test_dual_forward_memory_discipline(monkeypatch, math, m, k):
    """Under the guard, both fill patterns: the bands around z, a and the workspace stay intact, every element of both outputs is
    written, x, W and bias are unchanged, and the results are bitwise those of the unguarded run.  Every route of FWD_CASES: the
    z stores of the unsplit tiled kernels at ragged M, of both 128x128 tiles, of the split-K combine, and of the persistent kernel
    (whole and split schedule) through the residual's descriptor."""
    from mumpy_hip import ops
    host = dict(zip("xwb", _fwd_inputs(m, k)))
    with _modes(math=math):
        first = ops.linear_gelu_dual(*(host[n].to(DEV) for n in "xwb"))

        def body(guard):
            t = {n: guard.tensor(v) for n, v in host.items()}
            z, a = ops.linear_gelu_dual(t["x"], t["w"], t["b"])
            return {"z": z, "a": a}, [], None

        runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set()
    for outs in runs:
        assert not torch.isnan(outs["z"]).any() and not torch.isnan(outs["a"]).any()
        assert torch.equal(outs["z"], first[0]) and torch.equal(outs["a"], first[1])


# ------------------------------------------------------------------ GPU, per op: the backward
# (M, C, hidden) -> (dX product, dW product) as "wave tile x split", by hand from plan() of csrc/gemm_bwd.hip
BWD_CASES = {(37, 32, 128): ("32x1", "32x1"), (50, 768, 3072): ("32x6", "64x1"), (392, 768, 3072): ("64x5", "64x3"),
             (1000, 64, 256): ("32x1", "32x8"), (6272, 128, 512): ("64x1", "32x40")}


@functools.lru_cache(maxsize=None)
def _bwd_inputs(m, c, hid):
    z = seeded_randn(4100 + c, m, hid) * 1.5
    return F.gelu(z), z, seeded_randn(4200 + c, c, hid) / hid ** 0.5, seeded_randn(4300 + c, m, c)


def _gelu_grad64(z):
    z = z.double()
    return 0.5 * (1.0 + torch.erf(z / 2.0 ** 0.5)) + z * torch.exp(-0.5 * z * z) / (2.0 * torch.pi) ** 0.5


def _parse_xgemm(route):
    m = re.fullmatch(r"xgemm np=(\d) addr=dense dx=(\S+) dw=(\S+) reduce=(\S+)( gate=gelu)?", route)
    assert m, route
    return m.groups()


@gpu
@pytest.mark.parametrize("math", ["fp32", "bf16"])
@pytest.mark.parametrize("case", sorted(BWD_CASES))
def test_gated_backward_against_float64_and_the_unfused_pair(case, math):
    from mumpy_hip import ops
    m, c, hid = case
    a, z, w, dy = _bwd_inputs(*case)
    ad, zd, wd, dyd = (t.to(DEV) for t in (a, z, w, dy))
    keep = [t.clone() for t in (ad, zd, wd, dyd)]
    ar, wr, dyr = (t.bfloat16().double() for t in (a, w, dy)) if math == "bf16" else (t.double() for t in (a, w, dy))
    ref_dz, ref_dw, ref_db = (dyr @ wr) * _gelu_grad64(z), dyr.t() @ ar, dyr.sum(0)
    if math == "fp32":                                           # ... which is float64 autograd of gelu(z) @ W.T + b
        z64, w64 = z.double().requires_grad_(True), w.double().requires_grad_(True)
        b64 = torch.zeros(c, dtype=torch.float64, requires_grad=True)
        (F.gelu(z64) @ w64.t() + b64).backward(dy.double())
        assert rel_err(ref_dz, z64.grad) < 1e-9 and rel_err(ref_dw, w64.grad) < 1e-6 and rel_err(ref_db, b64.grad) < 1e-12
        ref_dz, ref_dw = z64.grad, w64.grad
    with _modes(math=math):
        dz, dw, db = ops.linear_gelu_bwd(ad, zd, wd, dyd, need_dz=True, need_dw=True, need_db=True)
        route = _route()
        again = ops.linear_gelu_bwd(ad, zd, wd, dyd, need_dz=True, need_dw=True, need_db=True)
        da, dw_p, db_p = ops.linear_bwd(ad, wd, dyd, need_dx=True, need_dw=True, need_db=True)
        sibling = _route()
        dz_p = ops.gelu_bwd(zd, da)
        gw, gb = seeded_randn(4, c, hid).to(DEV), seeded_randn(5, c).to(DEV)
        gw0, gb0 = gw.clone(), gb.clone()
        acc = ops.linear_gelu_bwd(ad, zd, wd, dyd, need_dz=False, need_dw=True, need_db=True, dw_out=gw, db_out=gb)
        only_dz = ops.linear_gelu_bwd(ad, zd, wd, dyd, need_dz=True, need_dw=False, need_db=False)
    torch.cuda.synchronize()
    np_, dx, dwr, red, gate = _parse_xgemm(route)
    assert (dx, dwr) == BWD_CASES[case] and gate and np_ == ("1" if math == "bf16" else "0") and route == sibling + " gate=gelu"
    assert red == {0: "none", 1: "one", 2: "two-in-one"}[int(not dx.endswith("x1")) + int(not dwr.endswith("x1"))]
    errs = rel_err(dz.cpu(), ref_dz), rel_err(dw.cpu(), ref_dw), rel_err(db.cpu(), ref_db)
    pair = rel_err(dz.cpu(), dz_p.cpu().double())
    bitwise = bool(torch.equal(dz, dz_p))
    print(f"gated bwd {math} {case}: {route}: rel err dz {errs[0]:.2e} dW {errs[1]:.2e} db {errs[2]:.2e}; "
          f"dz vs linear_bwd + gelu_bwd {pair:.2e}, bitwise: {bitwise}")
    assert max(errs) < 2e-5
    assert torch.equal(dw, dw_p) and torch.equal(db, db_p)
    assert pair < 1e-6
    assert bitwise                                               # measured: the same expression, rounded the same way, on all ten
    assert all(torch.equal(p, q) for p, q in zip((dz, dw, db), again))
    assert acc == (None, None, None)
    assert rel_err(gw.cpu(), gw0.cpu().double() + ref_dw) < 2e-5 and rel_err(gb.cpu(), gb0.cpu().double() + ref_db) < 2e-5
    assert torch.equal(only_dz[0], dz) and only_dz[1] is None and only_dz[2] is None
    assert all(torch.equal(p, q) for p, q in zip((ad, zd, wd, dyd), keep))


def test_backward_cases_cover_both_wave_tiles_split_and_unsplit():
    """Of each product: wave tile 32 and 64, each unsplit and split (the per-op test asserts that the route strings say this)."""
    for which in (0, 1):
        seen = {(v[which].split("x")[0], v[which].endswith("x1")) for v in BWD_CASES.values()}
        assert seen == {("32", True), ("32", False), ("64", True), ("64", False)}, (which, seen)


@gpu
@pytest.mark.parametrize("math", ["fp32", "bf16"])
@pytest.mark.parametrize("case", sorted(BWD_CASES))
def test_gated_backward_memory_discipline(monkeypatch, math, case):
    """Under the guard, both patterns: bands intact, every element of dz, dW and db written, a, z, W and dy unchanged, results bitwise
    those of the unguarded run.  Every case of BWD_CASES in both arithmetic forms: the gate in the reduce (dX split) and on the
    accumulators (unsplit), both wave tiles."""
    from mumpy_hip import ops
    host = dict(zip(("a", "z", "w", "dy"), _bwd_inputs(*case)))
    with _modes(math=math):
        first = ops.linear_gelu_bwd(*(host[n].to(DEV) for n in ("a", "z", "w", "dy")), need_dz=True, need_dw=True, need_db=True)

        def body(guard):
            t = {n: guard.tensor(v) for n, v in host.items()}
            dz, dw, db = ops.linear_gelu_bwd(t["a"], t["z"], t["w"], t["dy"], need_dz=True, need_dw=True, need_db=True)
            return {"dz": dz, "dw": dw, "db": db}, [], None

        runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set()
    for outs in runs:
        assert all(not torch.isnan(t).any() for t in outs.values())
        assert all(torch.equal(outs[n], f) for n, f in zip(("dz", "dw", "db"), first))


# ------------------------------------------------------------------ GPU, tape: the blocks
def _swin(shift, dp):
    from models.modules.swinTransformer import SwinTransformerBlock
    from mumpy_hip.autograd import swin_block_train
    blk = fill_module_(SwinTransformerBlock(dim=96, input_resolution=(14, 14), num_heads=3, window_size=7, shift_size=shift, drop_path=dp))
    return blk, [seeded_randn(5001, 2, 196, 96)], lambda b, x: swin_block_train(b, x)


def _global(dp):
    from models.modules.blocks import Block
    from mumpy_hip.autograd import global_block_train
    blk = fill_module_(Block(dim=768, heads=12, mlp_dim=3072, dropout=0.0, drop_path=dp))
    return blk, [seeded_randn(5002, 49, 3, 768)], lambda b, x: global_block_train(b, x)


def _cross(dp):
    from models.encoder.multiTemporalViewEncoder import CrossSwinBlock
    from mumpy_hip.autograd import cross_swin_block_train
    blk = fill_module_(CrossSwinBlock(96, 128, (14, 14), 3, temporal_dims=1, drop_path=dp), "csb/")
    return blk, [seeded_randn(5003, 2, 196, 96), seeded_randn(5004, 2, 196, 128)], lambda b, x1, x2: cross_swin_block_train(b, x1, x2)[0]


BLOCKS = {"swin_s0": lambda dp: _swin(0, dp), "swin_s3": lambda dp: _swin(3, dp), "global": _global, "cross": _cross}


def _fn_names(y):
    names, todo, seen = set(), [y.grad_fn], set()
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.add(type(f).__name__)
        todo.extend(g for g, _ in f.next_functions)
    return names


def _block_run(which, fused, slots, dp):
    """-> ({name: CPU tensor} of the output, the input gradients and every parameter gradient, tape node names, whether every fused fc1
    wrote the z that the unfused tape's ops.linear(x, w, b) writes, bit for bit)."""
    from mumpy_hip import ops
    from mumpy_hip.train import FlatAdamW
    inner, z_same = ops.linear_gelu_dual, []

    def spy(xx, w, b=None):
        z, a = inner(xx, w, b)
        z_same.append(bool(torch.equal(z, ops.linear(xx, w, b))))
        return z, a
    blk, xs, fn = BLOCKS[which](0.3 if dp else 0.0)
    blk = blk.to(DEV)
    blk = blk.train() if dp else blk.eval()
    opt = FlatAdamW(blk.parameters(), lr=0.0, weight_decay=0.0) if slots else None      # adopts the parameters: flat gradient slots
    xg = [x.to(DEV).requires_grad_(True) for x in xs]
    torch.manual_seed(77)                                                              # the stochastic-depth masks
    ops.linear_gelu_dual = spy
    try:
        with _modes(fused=fused, math="fp32"):
            y = fn(blk, *xg)
            names = _fn_names(y)
            (y * seeded_randn(5009, *y.shape).to(DEV)).sum().backward()
    finally:
        ops.linear_gelu_dual = inner
    assert len(z_same) == int(fused)
    out = {"y": y.detach().cpu()}
    out.update({f"dx{i}": x.grad.cpu() for i, x in enumerate(xg)})
    out.update({n: p.grad.detach().cpu().clone() for n, p in blk.named_parameters()})
    if slots:
        assert all(p.grad is p._mumpy_flat_grad for p in blk.parameters())
        out["flat"] = opt.grad.cpu()
    return out, names, all(z_same)


def _compare(tag, on, off, z_same):
    """torch.equal where the parts are bitwise, the 1e-6 bar otherwise.  The parts: dz (bitwise on every case: the per-op test asserts
    it) AND the z the fused fc1 writes against the z of the unfused tape.  The second is not a given: the unfused tape computes z with a launch WITHOUT
    an activation, which the planner may route differently from the GELU launch that the dual-output form is -- at the global
    block's fc1 (M = 147, K = 768, N = 3072) the plain launch takes the 64x64 persistent kernel, unsplit, and the GELU launch the tiled
    kernel with split-K 2, so the two z differ in summation order (measured: the block then differs by 6.2e-7 .. 7.0e-7, above
    half the bar, for this reason and no other: a and dz follow z bit for bit).  Measured here, from the tensors, per block."""
    assert set(on) == set(off)
    worst = max(rel_err(on[n], off[n].double()) if float(off[n].abs().max()) > 0 else float(on[n].abs().max()) for n in on)
    same = all(torch.equal(on[n], off[n]) for n in on)
    print(f"{tag}: switch on vs off: worst rel err {worst:.2e}, bitwise: {same} (fused z == unfused z: {z_same})")
    if z_same:
        assert same, [n for n in on if not torch.equal(on[n], off[n])]
    assert worst < 1e-6


@gpu
@pytest.mark.parametrize("dp", [False, True])
@pytest.mark.parametrize("slots", [False, True])
@pytest.mark.parametrize("which", sorted(BLOCKS))
def test_blocks_switch_on_against_off(which, slots, dp):
    on, names_on, z_same = _block_run(which, True, slots, dp)
    off, names_off, _ = _block_run(which, False, slots, dp)
    assert any("MlpFn" in n for n in names_on) and not any("GeluFn" in n for n in names_on if which != "cross")
    assert any("GeluFn" in n for n in names_off) and not any("MlpFn" in n for n in names_off)
    assert z_same or which == "global"                           # (the one shape here whose plain and GELU launches are routed apart)
    _compare(f"{which} slots={slots} drop_path={dp}", on, off, z_same)


@gpu
@pytest.mark.parametrize("which", sorted(BLOCKS))
def test_no_gelu_node_for_the_mlp_with_the_switch_on(which):
    """With the switch on the MLP is one MlpFn node: no GeluFn node of a block's tape belongs to it.  (The cross-view block keeps
    exactly the GeluFn of its offset network, LayerNorm -> GELU, which is no MLP.)"""
    blk, xs, fn = BLOCKS[which](0.0)
    blk = blk.to(DEV).eval()

    def count(fused):
        with _modes(fused=fused, math="fp32"):
            y = fn(blk, *(x.to(DEV).requires_grad_(True) for x in xs))
        n, todo, seen = {"GeluFn": 0, "MlpFn": 0}, [y.grad_fn], set()
        while todo:
            f = todo.pop()
            if f is None or f in seen:
                continue
            seen.add(f)
            for k in n:
                n[k] += k in type(f).__name__
            todo.extend(g for g, _ in f.next_functions)
        return n
    on, off = count(True), count(False)
    assert on["MlpFn"] == 1 and off["MlpFn"] == 0
    assert off["GeluFn"] == on["GeluFn"] + 1 and on["GeluFn"] == (1 if which == "cross" else 0)


@gpu
def test_fallback_under_a_split_precision_mode_and_the_legacy_route():
    from mumpy_hip import autograd as AG
    blk, xs, fn = BLOCKS["swin_s0"](0.0)
    blk = blk.to(DEV).eval()
    x = xs[0].to(DEV)
    legacy0 = AG.LEGACY_LINEAR_BWD
    for math, legacy in (("bf16x3", False), ("fp32", True)):
        AG.LEGACY_LINEAR_BWD = legacy
        try:
            with _modes(fused=True, math=math):
                xg = x.clone().requires_grad_(True)
                y = fn(blk, xg)
                names = _fn_names(y)
                y.sum().backward()
        finally:
            AG.LEGACY_LINEAR_BWD = legacy0
        assert any("GeluFn" in n for n in names) and not any("MlpFn" in n for n in names)
        assert bool(torch.isfinite(xg.grad).all()) and all(bool(torch.isfinite(p.grad).all()) for p in blk.parameters())
        blk.zero_grad()


@gpu
def test_tape_built_fused_runs_its_backward_after_the_matrix_mode_changed():
    """A tape built with the switch on keeps working when set_matrix_math moves to a split-precision mode before backward(): MlpFn
    then takes the route LinearFn takes there (the forward GEMM on transposed copies, gelu_bwd on its own).  bf16x3 carries
    fp32-level error, so the gradients agree with the all-fp32 run to GRAD_TOL = 2e-4 of tests/test_swin_backward.py."""
    from mumpy_hip import ops
    blk, xs, fn = BLOCKS["swin_s0"](0.0)
    blk = blk.to(DEV).eval()
    grads = []
    for flip in (False, True):
        blk.zero_grad()
        xg = xs[0].to(DEV).requires_grad_(True)
        with _modes(fused=True, math="fp32"):
            y = fn(blk, xg)
            assert any("MlpFn" in n for n in _fn_names(y))
            if flip:
                ops.set_matrix_math("bf16x3")
            (y * seeded_randn(5009, *y.shape).to(DEV)).sum().backward()
        grads.append([xg.grad.cpu()] + [p.grad.cpu().clone() for p in blk.parameters()])
    assert all(rel_err(b, a.double()) < 2e-4 for a, b in zip(*grads))


# ------------------------------------------------------------------ GPU, tape: the full model and the graphed step
# relative L2 of switch-on against switch-off, B = 1, T = 3, eval mode, as measured on MI355X (profiles/mlp_fused_train.md); the
# assertion is four times this.  Not bitwise: the fc1 launches with K >= 768 run split-K 2 as GELU launches and unsplit without an
# activation (see _compare), so their z differ in summation order.
FULL_MODEL_RECORDED = {"logits": 7.585e-07, "enc": 9.989e-07, "cva": 9.373e-07, "dec": 8.597e-07}


def _full_model(fused, log=None):
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from mumpy_hip import ops
    from mumpy_hip.autograd import decoder_train, encoder_train
    from mumpy_hip.train import split_param_groups
    enc = fill_module_(Encoder(num_frames=3)).eval().to(DEV)
    dec = fill_module_(Decoder(input_token_temporal_dims=[1, 1, 3])).eval().to(DEV)
    x, g = seeded_randn(990, 1, 3, 3, 224, 224).to(DEV), seeded_randn(991, 1, 1, 224, 224).to(DEV)
    inner = ops.linear_gelu_dual

    def spy(xx, w, b=None):
        r = inner(xx, w, b)
        log.append(((xx.numel() // xx.shape[-1], xx.shape[-1]), _route()))
        return r
    if log is not None:
        ops.linear_gelu_dual = spy
    try:
        with _modes(fused=fused, math="fp32"):
            fx, vx, dx = encoder_train(enc, x)
            lg, _ = decoder_train(dec, fx, vx, dx)
            (lg * g).sum().backward()
    finally:
        ops.linear_gelu_dual = inner
    groups = {k: torch.cat([p.grad.detach().double().reshape(-1) for p in ps]).cpu() for k, ps in split_param_groups(enc, dec).items()}
    return lg.detach().cpu(), groups


@gpu
def test_full_model_switch_on_against_off():
    log = []
    lg_on, g_on = _full_model(True, log)
    lg_off, g_off = _full_model(False)
    fig = {"logits": float((lg_on.double() - lg_off.double()).norm() / lg_off.double().norm())}
    fig.update({k: float((g_on[k] - g_off[k]).norm() / g_off[k].norm()) for k in g_off})
    print("full model B=1 T=3, switch on vs off, relative L2:", {k: f"{v:.3e}" for k, v in fig.items()})
    print("dual-output launches of the forward:", sorted({(mk, r) for mk, r in log}))
    assert set(fig) == set(FULL_MODEL_RECORDED)
    for k, v in fig.items():
        assert v <= 4.0 * FULL_MODEL_RECORDED[k] and v < 1e-3, (k, v)             # (1e-3: test_hip_full_model_backward_vs_oracle's logits bar)
    exercised = {r for math, _, _, r in FWD_CASES if math == "fp32"}
    assert log and {r for _, r in log} <= exercised, sorted({r for _, r in log} - exercised)


@gpu
def test_graphed_train_step_equals_the_eager_loop_bitwise():
    """config 1 (BaselineEncoder -> BaselineDecoder) with the switch on: warm-up + three replayed steps of GraphedTrainStep leave the
    parameters and AdamW's moments bit for bit where the eager loop of the same launches (constants staged on the device) leaves them."""
    from models.decoder.decoder import BaselineDecoder
    from models.encoder.encoder import BaselineEncoder
    from mumpy_hip import ops
    from mumpy_hip.autograd import baseline_decoder_train, baseline_encoder_train
    from mumpy_hip.train import GraphedTrainStep, build_optimizers
    x = seeded_randn(820, 1, 3, 3, 224, 224).to(DEV)
    target = torch.zeros(1, 1, 224, 224)
    target[:, :, 60:150, 80:190] = 1.0
    target = target.to(DEV)

    def make():
        enc = fill_module_(BaselineEncoder()).eval().to(DEV)
        dec = fill_module_(BaselineDecoder(in_channels=1024)).eval().to(DEV)
        return enc, dec, build_optimizers(enc, dec, lr_cnn=1e-6, lr=1e-5, weight_decay=1e-4, weight_decay_cnn=1e-4)
    warmup, replays = 2, 3
    with _modes(fused=True, math="fp32"):
        enc_e, dec_e, opts_e = make()
        for o in opts_e.values():
            o.enable_device_hyper()
        for _ in range(warmup + replays):
            logits = baseline_decoder_train(dec_e, baseline_encoder_train(enc_e, x))
            logits.backward(ops.mask_loss(logits.detach(), target)[1])
            for o in opts_e.values():
                o.stage_hyper()
                o.step_dev()
                o.zero_grad()
        enc_g, dec_g, opts_g = make()
        names = _fn_names(baseline_decoder_train(dec_g, baseline_encoder_train(enc_g, x)))
        assert any("MlpFn" in n for n in names) and not any("GeluFn" in n for n in names)
        gs = GraphedTrainStep(lambda xx: baseline_decoder_train(dec_g, baseline_encoder_train(enc_g, xx)), opts_g, x, target, warmup=warmup)
        for _ in range(replays):
            gs.step()
    torch.cuda.synchronize()
    for k in opts_e:
        assert opts_g[k].steps == opts_e[k].steps == warmup + replays
        for buf in ("param", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(opts_g[k], buf), getattr(opts_e[k], buf)), (k, buf)
