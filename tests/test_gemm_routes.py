"""Every GEMM kernel on every shape class the launch layer admits for it, not only the (kernel, shape) pairs today's planner
thresholds pick for today's test shapes.

The diagnostics build can force each route (MUMPY_GEMM_FORCE, MUMPY_GEMM_WS, MUMPY_GEMM_WS64, MUMPY_GEMM_WS16, MUMPY_XG_*), but it
reads the variables once per process: tests/gemm_route_worker.py runs one configuration per process, one process after another, and
prints one JSON line per cell (error against its bar, bitwise repeatability, guard rows, and the route mumpy_last_route() reported
against the one the configuration must give).  The CPU tests pin the case table itself: a cell cannot silently disappear.

Stop condition: a worker that dies of a GPU fault, an abort, a segmentation fault or its time limit ends the file -- every later
test fails at once without starting another process on the card.
"""
import json
import os
import re
import subprocess
import sys
import time

import pytest
import torch

from conftest import ROOT

import gemm_route_worker as W

WORKER = os.path.join(ROOT, "tests", "gemm_route_worker.py")
WORKER_TIMEOUT = 300                      # (test_gemm_lds_dma_variant_in_subprocess's; clean runs measured 2-3 s per worker)
_GPU_TROUBLE = []                         # module-level flag: the first worker that faulted / aborted / hung, with what it left

FORWARD = [f"tiled_{t}_{k}" for t, k in W.FORWARD_TILED] + ["ws_whole", "ws_split", "ws64", "s16_tiled", "s16_ws"]
BACKWARD = [f"xg_{w}_{s}" for w in ("w64", "w32") for s in ("nosplit", "split_minc1", "split_minc4")]


# ------------------------------------------------------------------------------------------------------------------ CPU tests
def _listed():
    r = subprocess.run([sys.executable, WORKER, "--list"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return [json.loads(line) for line in r.stdout.splitlines() if line.strip()]


@pytest.fixture(scope="module")
def listed():
    return _listed()


def test_case_table_covers_exactly_what_the_launch_layer_admits(listed):
    """(family, arithmetic, addressing) of the listed cells == the admissibility of launch_linear / mumpy_linear_bf16s_fwd /
    gemm_bwd.hip, written out here: the persistent kernels take fp32, dense or convolution only; the tiled kernels take every
    arithmetic with every way of addressing A; bf16 storage is dense; the backward products are dense or a convolution's."""
    reduced = ["bf16", "bf16x2", "bf16x3"]
    admitted = {("tiled", a, addr) for a in ["fp32"] + reduced for addr in ("dense", "rows", "kseg", "conv")}
    admitted |= {("ws", "fp32", "dense"), ("ws", "fp32", "conv"), ("ws64", "fp32", "dense")}
    admitted |= {("tiled16", "bf16s", "dense"), ("ws16", "bf16s", "dense")}
    admitted |= {("xgemm", a, addr) for a in ("fp32", "bf16") for addr in ("dense", "conv")}
    assert {(c["family"], c["arith"], c["addr"]) for c in listed} == admitted
    assert {c["config"] for c in listed} == set(FORWARD + BACKWARD) == set(W.CONFIGS)
    assert len({(c["config"], c["id"]) for c in listed}) == len(listed)                  # ids are unique per configuration
    per = {}
    for c in listed:
        per.setdefault(c["config"], []).append(c)
    # per configuration: every cell the configuration's family admits, with every epilogue, tap shape and image
    for t, k in W.FORWARD_TILED:
        cells = per[f"tiled_{t}_{k}"]
        assert {(c["arith"], c["addr"]) for c in cells if c["arith"] == "fp32"} == {("fp32", a) for a in ("dense", "rows", "kseg", "conv")}
        want_reduced = {(a, addr) for a in reduced for addr in (("dense", "rows", "kseg", "conv") if t in (0, 2) else ("dense",) if t == 1 else ())}
        assert {(c["arith"], c["addr"]) for c in cells if c["arith"] != "fp32"} == want_reduced
        assert {c["epi"] for c in cells if c["addr"] == "dense"} == {"gelu", "res", "none"}
        convs = [c for c in cells if c["addr"] == "conv" and c["arith"] == "fp32"]
        assert {(c["kh"], c["kw"]) for c in convs} == {(3, 3), (7, 1), (1, 7)} and all(c["h"] != c["w"] for c in convs)
        assert {(c["h"], c["w"], c["kh"]) for c in convs} >= {(h, w, kh) for (h, w) in ((6, 10), (13, 11)) for kh in (3, 7, 1)}
        assert any(c["addr"] == "kseg" and c["b"] == 1 for c in cells)
    for name in ("ws_whole", "ws_split"):
        shapes = {(c["m"], c["n"], c["k"]) for c in per[name] if c["addr"] == "dense" and c["epi"] != "ln"}
        assert (4160, 1056, 96) in shapes and {c["c"] for c in per[name] if c["epi"] == "ln"} == {96, 192, 384, 768}
    assert {(392, 2304, 768), (1568, 384, 384)} <= {(c["m"], c["n"], c["k"]) for c in per["ws_split"] if "m" in c and "k" in c}
    assert {int(re.search(r"P=(\d)", c["route"]).group(1)) for c in per["ws_whole"]} == {1, 2, 4, 8}
    t64 = [((c["m"] + 63) // 64) * ((c["n"] + 63) // 64) for c in per["ws64"]]
    assert max(t64) > 512 and min(t64) < 64 and any(c["epi"] == "gelu" for c in per["ws64"])
    assert any(c["route"].startswith("tiled16 tile=0") for c in per["s16_tiled"]) and any(c["route"].startswith("tiled16 tile=2") for c in per["s16_tiled"])
    assert all(c["route"].startswith("ws16") for c in per["s16_ws"])
    for name in BACKWARD:
        assert {c["epi"] for c in per[name] if c["addr"] == "dense"} == {"all", "dx", "dw_db_acc", "db"}
        assert {(c["m"], c["n"], c["k"]) for c in per[name] if c["addr"] == "dense"} == {(m, n, k) for m in (37, 300, 1000) for n in (96, 160) for k in (96, 160)}
    reduces = {re.search(r"reduce=(\S+)", c["route"]).group(1) for c in listed if c["family"] == "xgemm"}
    assert reduces == {"none", "one", "two-in-one", "taps"}                              # all three reduce forms (+ the taps one)
    wts = {m for c in listed if c["family"] == "xgemm" for m in re.findall(r"d[xw]=(\d+)x", c["route"])}
    assert wts == {"32", "64"}


ROUTE_PATTERNS = [
    r"tiled tile=(?P<tile>[0-3]) ks=(?P<ks>\d+) np=(?P<np>[0-3]) addr=(dense|rows|kseg|conv)",
    r"tiled16 tile=[02] ks=1 np=1 addr=dense",
    r"ws sched=(whole|split) P=[1248] ln=(none|producer|consumer) addr=(dense|conv)",
    r"ws64 P=[124] addr=dense",
    r"ws16 P=[1248] addr=dense",
    r"xgemm np=[01] addr=(dense|conv) dx=(-|(32|64)x\d+) dw=(-|(32|64)x\d+) reduce=(none|one|two-in-one|taps)",
]


def test_expected_routes_parse_and_splits_obey_the_chunk_rule(listed):
    """Every expected route is one of the forms include/mumpy_hip.h documents; a forced split-K factor k is expected only where
    K % (32 k) == 0, and exactly ks = 1 elsewhere; tiles 1 and 3 never appear for the bf16-piece family."""
    seen_dropped = seen_taken = False
    for c in listed:
        ms = [m for m in (re.fullmatch(p, c["route"]) for p in ROUTE_PATTERNS) if m]
        assert len(ms) == 1, c
        if c["family"] != "tiled":
            continue
        m = ms[0]
        want = int(c["env"]["MUMPY_GEMM_FORCE"].split(",")[1])
        k_dim = {"dense": lambda: c["k"], "rows": lambda: c["c"], "kseg": lambda: c["t"] * c["c"],
                 "conv": lambda: c["kh"] * c["kw"] * c["cin"]}[c["addr"]]()
        ks = int(m.group("ks"))
        assert ks == (want if k_dim % (32 * want) == 0 else 1), c
        seen_dropped |= want > 1 and ks == 1
        seen_taken |= ks > 1
        forced_tile = int(c["env"]["MUMPY_GEMM_FORCE"].split(",")[0])
        assert int(m.group("tile")) == (forced_tile if c["arith"] == "fp32" else {0: 0, 3: 0, 1: 2, 2: 2}[forced_tile])
    assert seen_dropped and seen_taken


def test_rounding_helpers_are_round_to_nearest_even():
    """The worker's references round with integer arithmetic of their own: equal to torch.bfloat16 (RNE) on ties, near-ties,
    both signs, zeros and subnormal-free extremes; the two-piece form is the bf16x2 test's."""
    hi = torch.arange(0x3F80, 0x3F90, dtype=torch.int32) << 16                          # 16 consecutive bf16 values from 1.0
    lows = torch.tensor([0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF], dtype=torch.int32)
    bits = (hi[:, None] | lows[None, :]).reshape(-1)                                    # exact ties (0x8000) above even AND odd values
    t = bits.view(torch.float32)
    t = torch.cat([t, -t, t * 2.0 ** -60, t * 2.0 ** 60, torch.zeros(2), torch.randn(4096, generator=torch.Generator().manual_seed(5))])
    assert torch.equal(W.bf16_round(t), t.bfloat16().float())
    ties = bits[(bits & 0xFFFF) == 0x8000].view(torch.float32)
    assert ties.numel() == 16 and not torch.equal(W.bf16_round(ties), (ties.view(torch.int32) & -65536).view(torch.float32))   # not truncation
    p0 = t.bfloat16().float()
    assert torch.equal(W.two_piece(t), p0 + (t - p0).bfloat16().float())
    # the "coherent" operands keep their leading piece and carry positive second and third pieces of ~2^-9 and ~2^-18 relative size
    x = torch.randn(20000, generator=torch.Generator().manual_seed(6))
    co = W.coherent(x)
    p0 = W.bf16_round(co)
    p1 = W.bf16_round(co - p0)
    p2 = (co - p0 - p1).double()
    moved = co != x
    assert float(moved.float().mean()) > 0.99 and torch.equal(p0, x.bfloat16().float())
    assert bool((p1[moved] > 0).all()) and bool((p2[moved] > 0).all())
    assert float((p1 / co.abs())[moved].min()) > 2.0 ** -10 and float((p2 / co.abs().double())[moved].min()) > 2.0 ** -19


# ------------------------------------------------------------------------------------------------------------------ GPU tests
def _run_worker(config):
    if _GPU_TROUBLE:
        pytest.fail(f"not started: an earlier worker ended in a GPU fault, abort or hang: {_GPU_TROUBLE[0]}")
    from mumpy_hip.lib import tuning_library_path
    env = dict(os.environ, MUMPY_HIP_LIB=tuning_library_path(), **W.CONFIGS[config])
    t0 = time.time()
    try:
        r = subprocess.run([sys.executable, WORKER, config], env=env, capture_output=True, text=True, timeout=WORKER_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _GPU_TROUBLE.append(f"{config}: no end after {WORKER_TIMEOUT} s")
        pytest.fail(f"{_GPU_TROUBLE[0]}; last output: {(e.stdout or b'')[-1000:]!r}")
    out = r.stdout + r.stderr
    if r.returncode in (124, 134, 137, 139, -6, -11) or "illegal memory access" in out:
        _GPU_TROUBLE.append(f"{config}: status {r.returncode}: {out[-600:]}")
        pytest.fail(_GPU_TROUBLE[0])
    lines = []
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            lines.append(json.loads(line))
    print(f"{config}: {len(lines) - 1} cells in {time.time() - t0:.1f} s (worker status {r.returncode})")
    for d in lines:
        print(json.dumps(d))
    return r, lines


def _check(config):
    r, lines = _run_worker(config)
    assert lines and lines[-1].get("done"), f"{config}: the worker did not finish: {r.stderr[-2000:]}"
    results, summary = lines[:-1], lines[-1]
    want = W.cases(config)
    assert [d["id"] for d in results] == [c["id"] for c in want]                         # every cell ran
    bad = []
    for d, c in zip(results, want):
        assert d["route"] == c["route"]
        if not (d["got_route"].split(" | ")[0] == c["route"] and d["route_ok"]):
            bad.append((d["id"], "route", d["got_route"], c["route"]))
        if not d["err"] < d["bar"]:
            bad.append((d["id"], "error", d["err"], d["bar"]))
        if d["bitwise"] is not True:
            bad.append((d["id"], "second launch differs"))
        if d["guards"] is not True:
            bad.append((d["id"], "guard rows touched / sentinel left inside / statistics"))
    assert not bad, f"{config}: {len(bad)} failures, first: {bad[:8]}"
    assert summary["flags_zero"] is True and summary["failed"] == [] and r.returncode == 0, (summary, r.stderr[-1000:])


@pytest.mark.gpu
@pytest.mark.parametrize("config", FORWARD)
def test_forward_routes(config):
    """One worker per forced forward configuration: the tiled fp32 kernels in four tile shapes with and without split-K (and the
    bf16-piece family on its two), the persistent 128x128 kernel on whole and split schedules with every P and the LayerNorm
    producer / consumer, the persistent 64x64 kernel (GELU, fewer than 64 tiles, more than 512), and the bf16-storage pair --
    each on dense, strided-rows, segmented-K and non-square 3x3 / 7x1 / 1x7 convolution operands where the launch layer admits it."""
    _check(config)


@pytest.mark.gpu
@pytest.mark.parametrize("config", BACKWARD)
def test_backward_routes(config):
    """mumpy_linear_bwd and mumpy_conv2d_wgrad_nhwc with the 32- or the 64-wave tile forced, unsplit / split as far as it goes with
    MUMPY_XG_MINCHUNKS 1 and 4: every combination of wanted outputs, all reduce forms, fp32 and bf16 operands."""
    _check(config)
