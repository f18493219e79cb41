"""Worker of tests/test_gemm_routes.py: runs every (kernel, shape class) cell of ONE forced GEMM configuration on the GPU.

The planner / kernel hooks of the diagnostics build (MUMPY_GEMM_FORCE, MUMPY_GEMM_WS, MUMPY_GEMM_WS64, MUMPY_GEMM_WS16,
MUMPY_XG_*) are read once per process, so a process can hold one forced configuration: the test file starts this script once
per configuration with MUMPY_HIP_LIB = the diagnostics library and the configuration's variables.  The script sets nothing
itself; it only knows, from the configuration's NAME, which route every cell must take, and compares that with what
mumpy_last_route() reports after the launch -- a force that was dropped (a split whose slabs do not fit, a schedule without its
workspace, the shipped library) is a failed cell, not a silently different test.

    python tests/gemm_route_worker.py --list            the case table of every configuration as JSON lines (no GPU)
    python tests/gemm_route_worker.py <configuration>   run it: one JSON line per cell, then one summary line; exit 1 if a cell failed

Per cell, against a float64 reference computed on the CPU: the error at the bar the suite already uses for that arithmetic
(fp32 and bf16x3: 1e-5 against the exact product; bf16: 2e-5 against the product of the bf16-rounded operands; bf16x2: 2e-5 against
the product of the two-piece-rounded operands; bf16 storage: 2e-5 with an fp32 output, 5e-3 with a bf16 one; LayerNorm folding:
5e-5; backward: 1e-5 fp32, 2e-5 bf16), a second launch that must be bitwise equal, the route, and -- forward -- the output written
into the middle of a buffer whose 64 guard rows either side must keep their sentinel while no sentinel stays inside.

Operands.  Gaussian, W scaled by K^-1/2.  In the fp32 and bf16x3 cells with K >= 384 they are "coherent" instead (coherent()):
every value keeps its leading bf16 piece p0 but sits 0.45 ulp(p0) + 0.45 ulp(p1) above it, so that its second and third pieces
are as large as they get and POSITIVE, and W is positive (odd M: the A operand is the positive one).  On Gaussian data a
lost piece product (a1 b1, a2 b0: 2^-16 ... 2^-18 of |a||b|, random sign) averages down to ~1e-6 of the output scale, under every bar; here those terms have one sign and add up
over K (a2 b0: 4.6e-6 x 0.23 sqrt(K) of the output scale = 2.1e-5 at K = 384, 2.9e-5 at 768; a1 b1: 1e-6 sqrt(K)), while what an
exact three-piece kernel drops (a1 b2, a2 b1, a2 b2: 2^-24 and less) stays ~1e-7.  The bar is unchanged: 1e-5 against the exact
product.  The bf16 and bf16x2 cells keep Gaussian operands: bf16x2 drops a1 b1 by design, and its reference says so.

Workspace.  The dense cells call mumpy_linear_wsz_fwd directly (ops._call) with ONE kept, zeroed 64-MiB workspace
(ops._kept_workspace): ops.linear passes none when mumpy_linear_workspace_bytes is 0, which is the case for every small shape,
so a forced split-K or split schedule would never get its slabs and flags there.  The same buffer serves ops.linear /
ops.linear_ln of the LayerNorm-folding cells.  After the last cell of a persistent configuration ops.check_workspaces() must
pass and the flag page (the first 1024 words) must be zero again.

Bounded waits of the forced split schedule (csrc/gemm_ws.h, read before this was first run on small shapes): a workgroup whose
share of the chunk sequence is empty (first_chunk(b) == first_chunk(b + 1)) returns before any barrier; the roles of a
workgroup meet only in s_barrier, with the same count on every role; the single wait on another workgroup is the owner's poll of
the arrival flags of the FIRST segments of later workgroups (which depend on nothing), it skips the empty workgroups with the same
first_chunk test, and it gives up after 2^24 polls, raising the workspace's sticky status word instead of hanging.  There is no
other loop on memory another workgroup writes.
"""
import argparse
import hashlib
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "multilateral-temporal-view-pyramid-transformer-for-video-inpainting-detection_amd")
for _p in (ROOT, PKG):
    if _p not in sys.path:
        sys.path.insert(0, _p)

NUM_CU = 256
WS_BYTES = 64 << 20
GUARD = 64
SENTINEL32 = 0x7FC0DEAD                  # a quiet NaN with a payload no kernel produces
SENTINEL16 = 0x7FC1                      # (bf16 outputs)

# ---------------------------------------------------------------------------------------------------------------- configurations
FORWARD_TILED = [(0, 1), (0, 2), (1, 1), (2, 1), (2, 3), (3, 1), (3, 2)]
CONFIGS = {}
for _t, _k in FORWARD_TILED:
    CONFIGS[f"tiled_{_t}_{_k}"] = {"MUMPY_GEMM_WS": "0", "MUMPY_GEMM_WS64": "0", "MUMPY_GEMM_FORCE": f"{_t},{_k}"}
CONFIGS["ws_whole"] = {"MUMPY_GEMM_WS64": "0", "MUMPY_GEMM_WS": "1"}
CONFIGS["ws_split"] = {"MUMPY_GEMM_WS64": "0", "MUMPY_GEMM_WS": "3"}
CONFIGS["ws64"] = {"MUMPY_GEMM_WS": "0", "MUMPY_GEMM_WS64": "2"}
CONFIGS["s16_tiled"] = {"MUMPY_GEMM_WS16": "0"}
CONFIGS["s16_ws"] = {"MUMPY_GEMM_WS16": "2"}
# backward: wave tile (MUMPY_XG_WIDE_AT) x split (both targets; MUMPY_XG_MINCHUNKS only matters when something is split)
for _w, _wide_at in (("w64", 1), ("w32", 1000000)):
    CONFIGS[f"xg_{_w}_nosplit"] = {"MUMPY_XG_WIDE_AT": str(_wide_at), "MUMPY_XG_TARGET64": "1", "MUMPY_XG_TARGET32": "1",
                                   "MUMPY_XG_MINCHUNKS": "4"}
    for _minc in (1, 4):
        CONFIGS[f"xg_{_w}_split_minc{_minc}"] = {"MUMPY_XG_WIDE_AT": str(_wide_at), "MUMPY_XG_TARGET64": "100000",
                                                 "MUMPY_XG_TARGET32": "100000", "MUMPY_XG_MINCHUNKS": str(_minc)}

ARITHS = ["fp32", "bf16", "bf16x2", "bf16x3"]
MATH_BITS = {"fp32": 0, "bf16": 0x100, "bf16x3": 0x200, "bf16x2": 0x400}
NP = {"fp32": 0, "bf16": 1, "bf16x2": 2, "bf16x3": 3}
BAR = {"fp32": 1e-5, "bf16x3": 1e-5, "bf16": 2e-5, "bf16x2": 2e-5}
EPIS = ["gelu", "res", "none"]          # bias + GELU; bias + residual; neither

# (M, N, K): M below a 64 tile / ragged against 64 and 128; N ragged against both tile widths; K = 96, 192, 384, 768 gives the
# persistent kernel's P = 8, 4, 2, 1 and admits forced splits 2 and 3 wherever K % (32 k) == 0
DENSE = [(37, 96, 96), (300, 160, 96), (300, 96, 192), (37, 160, 192), (300, 160, 384), (37, 96, 384), (300, 96, 768), (37, 160, 768)]
WS_SECOND_ROUND = (4160, 1056, 96)       # 33 x 9 = 297 tiles of 128 x 128 > 256 workgroups, ragged last row tile
WS64_SECOND_ROUND = (2080, 1056, 96)     # 33 x 17 = 561 tiles of 64 x 64 > 512 slots, ragged last row and column tiles
WS_SPLIT_RECORDED = [(392, 2304, 768), (1568, 384, 384)]      # two of the shapes of profiles/r02_gemm_ws_small_shapes.txt
S16_WIDE = (3200, 1024, 64)              # 25 x 8 = 200 tiles: the bf16-storage tiled kernel's wide tile
# rows: time slice t of a (B, T, n, C) tensor (block stride T n C > n C); (B, T, n, C, N, t)
ROWS = [(3, 3, 37, 96, 160, 1), (2, 2, 150, 192, 96, 1), (3, 2, 100, 768, 160, 0)]
# kseg: linear_time_slices on (B, T, n, C), K = T C; (B, T, n, C, N)
KSEG = [(1, 3, 37, 32, 96), (2, 3, 150, 64, 160), (1, 3, 300, 128, 96), (2, 3, 37, 256, 160)]
IMAGES = [(6, 10), (13, 11)]             # non-square: a swap of H and W in a pixel decode shows
TAPS = [(3, 3), (7, 1), (1, 7)]
CHANNELS = [(32, 32), (32, 96), (128, 32), (128, 96)]        # (Cin, Cout)
CONV_B = 2
BWD_M, BWD_N, BWD_K = [37, 300, 1000], [96, 160], [96, 160]
BWD_WANTS = ["all", "dx", "dw_db_acc", "db"]
WGRAD_CHANNELS = [(32, 96), (128, 32)]


def conv_cases():
    out = []
    for ci, (cin, cout) in enumerate(CHANNELS):
        for ti, (kh, kw) in enumerate(TAPS):
            h, w = IMAGES[(ci + ti) % 2]
            out.append((CONV_B, h, w, cin, cout, kh, kw))
    return out


# ------------------------------------------------------------------------------------------------- the launch layer, as a model
def passes_per_chunk(passes, nk):
    need = (passes + nk - 2) // (nk - 1)
    return 1 if need <= 1 else 2 if need <= 2 else 4 if need <= 4 else 8


def forced_split(k_dim, want):
    """MUMPY_GEMM_FORCE=t,k: the split is taken only when every slice is a whole number of 32-chunks."""
    return want if k_dim % (32 * want) == 0 else 1


def tiled_route(tile, want_ks, arith, addr, k_dim):
    if arith != "fp32":
        tile = {0: 0, 3: 0, 1: 2, 2: 2}[tile]      # the bf16-piece family has the 128x128 and the 64x64 tile only
    return f"tiled tile={tile} ks={forced_split(k_dim, want_ks)} np={NP[arith]} addr={addr}"


def ws_route(split, k_dim, addr, ln="none"):
    p = passes_per_chunk(16, k_dim // 32)
    if split and p < 4:
        p = 4
    return f"ws sched={'split' if split else 'whole'} P={p} ln={ln} addr={addr}"


def ws64_route(k_dim):
    return f"ws64 P={min(4, passes_per_chunk(4, k_dim // 32))} addr=dense"


def s16_route(ws16, m, n, k_dim):
    if ws16 and k_dim % 64 == 0 and k_dim >= 192:
        return f"ws16 P={passes_per_chunk(16, k_dim // 64)} addr=dense"
    wide = ((m + 127) // 128) * ((n + 127) // 128) >= 200
    return f"tiled16 tile={0 if wide else 2} ks=1 np=1 addr=dense"


def xg_plan(env, r, c, kk, taps=1):
    """csrc/gemm_bwd.hip plan(): wave tile and split of one backward product."""
    t128 = ((r + 127) // 128) * ((c + 127) // 128) * taps
    wt = 64 if t128 >= int(env["MUMPY_XG_WIDE_AT"]) else 32
    bt = 2 * wt
    tiles = ((r + bt - 1) // bt) * ((c + bt - 1) // bt) * taps
    nchunks = (kk + 31) // 32
    target = int(env["MUMPY_XG_TARGET64"] if wt == 64 else env["MUMPY_XG_TARGET32"])
    ks = max(1, min(target // tiles, nchunks // int(env["MUMPY_XG_MINCHUNKS"]), 64))
    cps = (nchunks + ks - 1) // ks
    return wt, (nchunks + cps - 1) // cps          # no empty splits


def xg_linear_route(env, arith, m, n, k, want):
    dx = xg_plan(env, m, k, n) if want in ("all", "dx") else None
    dw = xg_plan(env, n, k, m) if want in ("all", "dw_db_acc") else None
    if dx and dw and dx[1] > 1 and dw[1] > 1:
        red = "two-in-one"
    elif (dx and dx[1] > 1) or (dw and dw[1] > 1):
        red = "one"
    else:
        red = "none"
    f = lambda p: "-" if p is None else f"{p[0]}x{p[1]}"
    return f"xgemm np={NP[arith]} addr=dense dx={f(dx)} dw={f(dw)} reduce={red}"


def xg_wgrad_route(env, arith, b, h, w, cin, cout, kh, kw):
    wt, ks = xg_plan(env, cout, cin, b * h * w, kh * kw)
    return f"xgemm np={NP[arith]} addr=conv dx=- dw={wt}x{ks} reduce={'taps' if ks > 1 else 'none'}"


# -------------------------------------------------------------------------------------------------------------- the case table
def _cell(cid, family, arith, addr, epi, route, **kw):
    d = {"id": cid, "family": family, "arith": arith, "addr": addr, "epi": epi, "route": route}
    d.update(kw)
    return d


def _forward_cells(route_of, ariths, addrs, epis_all=True):
    """The shape classes of the forward matrix for one configuration; route_of(arith, addr, K, M, N) -> expected route."""
    cells = []
    for arith in ariths:
        if "dense" in addrs:
            for (m, n, k) in DENSE:
                for epi in EPIS:
                    cells.append(_cell(f"dense-{arith}-{m}x{n}x{k}-{epi}", None, arith, "dense", epi, route_of(arith, "dense", k, m, n),
                                       m=m, n=n, k=k))
        if "rows" in addrs:
            for i, (b, t, rows, c, n, ts) in enumerate(ROWS):
                cells.append(_cell(f"rows-{arith}-{b}x{t}x{rows}x{c}-n{n}", None, arith, "rows", EPIS[i % 3],
                                   route_of(arith, "rows", c, b * rows, n), b=b, t=t, rows=rows, c=c, n=n, ts=ts))
        if "kseg" in addrs:
            for i, (b, t, rows, c, n) in enumerate(KSEG):
                cells.append(_cell(f"kseg-{arith}-{b}x{t}x{rows}x{c}-n{n}", None, arith, "kseg", EPIS[(i + 1) % 3],
                                   route_of(arith, "kseg", t * c, b * rows, n), b=b, t=t, rows=rows, c=c, n=n))
        if "conv" in addrs:
            for i, (b, h, w, cin, cout, kh, kw) in enumerate(conv_cases()):
                cells.append(_cell(f"conv-{arith}-{h}x{w}-{cin}to{cout}-{kh}x{kw}", None, arith, "conv", EPIS[(i + 2) % 3],
                                   route_of(arith, "conv", kh * kw * cin, b * h * w, cout), b=b, h=h, w=w, cin=cin, cout=cout, kh=kh, kw=kw))
    for c in cells:
        c["family"] = c["route"].split()[0]
    return cells


def cases(config):
    env = CONFIGS[config]
    if config.startswith("tiled_"):
        tile, ks = (int(v) for v in env["MUMPY_GEMM_FORCE"].split(","))
        route_of = lambda arith, addr, k, m, n: tiled_route(tile, ks, arith, addr, k)
        cells = _forward_cells(route_of, ["fp32"], ["dense", "rows", "kseg", "conv"])
        # In the reduced modes tiles 0 and 3 are one kernel, and so are 1 and 2 (the launch layer re-routes them): the cells run
        # under tiles 0 and 2; tile 1 keeps the dense ones, which is where a missing re-route leaves columns unwritten.
        if tile in (0, 2):
            cells += _forward_cells(route_of, ARITHS[1:], ["dense", "rows", "kseg", "conv"])
        elif tile == 1:
            cells += _forward_cells(route_of, ARITHS[1:], ["dense"])
        return cells
    if config in ("ws_whole", "ws_split"):
        split = config == "ws_split"
        route_of = lambda arith, addr, k, m, n: ws_route(split, k, addr)
        cells = _forward_cells(route_of, ["fp32"], ["dense", "conv"])
        big = [WS_SECOND_ROUND] + (WS_SPLIT_RECORDED if split else [])
        for i, (m, n, k) in enumerate(big):
            for epi in EPIS:
                cells.append(_cell(f"dense-fp32-{m}x{n}x{k}-{epi}", "ws", "fp32", "dense", epi, ws_route(split, k, "dense"), m=m, n=n, k=k))
        for c in (96, 192, 384, 768):           # one LayerNorm producer + consumer pair per P
            cells.append(_cell(f"lnfold-fp32-300x{c}-n160", "ws", "fp32", "dense", "ln", ws_route(split, c, "dense", "producer"),
                               route2=ws_route(split, c, "dense", "consumer"), m=300, c=c, n=160, gelu=c in (192, 768)))
        return cells
    if config == "ws64":
        cells = _forward_cells(lambda arith, addr, k, m, n: ws64_route(k), ["fp32"], ["dense"])
        m, n, k = WS64_SECOND_ROUND
        for epi in EPIS:
            cells.append(_cell(f"dense-fp32-{m}x{n}x{k}-{epi}", "ws64", "fp32", "dense", epi, ws64_route(k), m=m, n=n, k=k))
        return cells
    if config in ("s16_tiled", "s16_ws"):
        ws16 = config == "s16_ws"
        cells = []
        shapes = [s for s in DENSE if not ws16 or s[2] >= 192]        # (K = 96 is the tiled kernel's in both: run once)
        if not ws16:
            shapes = shapes + [S16_WIDE]
        for (m, n, k) in shapes:
            for epi, out16 in (("gelu", True), ("none", True), ("res", False)):
                route = s16_route(ws16, m, n, k)
                cells.append(_cell(f"dense-bf16s-{m}x{n}x{k}-{epi}-{'out16' if out16 else 'out32'}", route.split()[0], "bf16s", "dense",
                                   epi, route, m=m, n=n, k=k, out16=out16))
        return cells
    if config.startswith("xg_"):
        cells = []
        for arith in ("fp32", "bf16"):
            for m in BWD_M:
                for n in BWD_N:
                    for k in BWD_K:
                        for want in BWD_WANTS:
                            cells.append(_cell(f"bwd-{arith}-{m}x{n}x{k}-{want}", "xgemm", arith, "dense", want,
                                               xg_linear_route(env, arith, m, n, k, want), m=m, n=n, k=k))
            for ci, (cin, cout) in enumerate(WGRAD_CHANNELS):
                for ti, (kh, kw) in enumerate(TAPS):
                    h, w = IMAGES[(ci + ti) % 2]
                    for acc in (False, True):
                        cells.append(_cell(f"wgrad-{arith}-{h}x{w}-{cin}to{cout}-{kh}x{kw}-{'acc' if acc else 'new'}", "xgemm", arith, "conv",
                                           "acc" if acc else "new", xg_wgrad_route(env, arith, CONV_B, h, w, cin, cout, kh, kw),
                                           b=CONV_B, h=h, w=w, cin=cin, cout=cout, kh=kh, kw=kw, acc=acc))
        return cells
    raise KeyError(config)


# ------------------------------------------------------------------------------------------------------------ rounding helpers
def bf16_round(t):
    """fp32 -> the nearest bf16 value (ties to even), as fp32; integer arithmetic on the bit pattern, no torch.bfloat16."""
    i = t.contiguous().view(torch.int32).to(torch.int64) & 0xFFFFFFFF
    i = (i + 0x7FFF + ((i >> 16) & 1)) & 0xFFFF0000
    i = torch.where(i >= (1 << 31), i - (1 << 32), i).to(torch.int32)
    return i.view(torch.float32).reshape(t.shape)


def two_piece(t):
    """The two-piece form of the bf16x2 mode: bf16(t) + bf16(t - bf16(t)), as fp32 (exact: 17 significant bits at most)."""
    p0 = bf16_round(t)
    return p0 + bf16_round(t - p0)


def coherent(t):
    """t moved, inside the rounding interval of its leading bf16 piece p0, to p0 + p1 + p2 with p1 = +0.45 ulp(p0) and
    p2 = +0.45 ulp(p1): every lower piece as large as it gets, and positive whatever the sign of t."""
    p0 = bf16_round(t)

    def up(v):                                       # 0.45 bf16 ulp of v: |v| in [2^(e-1), 2^e) has ulp 2^(e-8)
        return torch.ldexp(torch.full_like(v, 0.45), torch.frexp(v).exponent - 8)
    p1 = bf16_round(up(p0))
    c = p0 + p1 + up(p1)
    ok = (p0 != 0) & (bf16_round(c) == p0) & (bf16_round(c - p0) == p1)      # (not so just above a negative power of two)
    return torch.where(ok, c, t)


def operand_rounding(arith):
    return {"fp32": lambda t: t, "bf16x3": lambda t: t, "bf16": bf16_round, "bf16x2": two_piece, "bf16s": lambda t: t}[arith]


def rel_err(a, b):
    a, b = a.double(), b.double()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def digest(tensors):
    """sha256 of the tensors' bytes in the order given.  Informational (no check reads it): it lets the cells of two libraries be
    compared bit for bit."""
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------------------------- running cells
class Runner:
    def __init__(self, config):
        from mumpy_hip import ops
        from mumpy_hip.lib import load_library
        self.ops, self.lib, self.config = ops, load_library(), config
        self.dev = torch.device("cuda:0")
        self.ws = ops._kept_workspace(WS_BYTES, self.dev)
        self.operands = (None, None)         # (key, tensors) of the shape in hand: its cells are consecutive

    def route(self):
        return self.lib.mumpy_last_route().decode()

    def guarded(self, m, n, dtype=torch.float32):
        """(buffer, view of its middle m rows): 64 sentinel rows either side, sentinels inside until the kernel writes."""
        if dtype == torch.float32:
            buf = torch.full((m + 2 * GUARD, n), SENTINEL32, dtype=torch.int32, device=self.dev).view(torch.float32)
        else:
            buf = torch.full((m + 2 * GUARD, n), SENTINEL16, dtype=torch.int16, device=self.dev).view(torch.bfloat16)
        return buf, buf[GUARD:GUARD + m]

    @staticmethod
    def bits(t):
        return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)

    def guards_ok(self, buf, m):
        b = self.bits(buf)
        s = SENTINEL32 if buf.dtype == torch.float32 else SENTINEL16
        outside = bool((b[:GUARD] == s).all()) and bool((b[GUARD + m:] == s).all())
        inside = not bool((b[GUARD:GUARD + m] == s).any())
        return outside and inside

    def forward_operands(self, cell):
        """-> (A as the (M, K) matrix the GEMM sees, or None for a convolution; source tensor; W; bias; residual; M; N; K)"""
        addr = cell["addr"]
        if addr == "dense":
            m, n, k = cell["m"], cell["n"], cell["k"]
            shape = (m, k)
        elif addr == "rows":
            m, n, k = cell["b"] * cell["rows"], cell["n"], cell["c"]
            shape = (cell["b"], cell["t"], cell["rows"], cell["c"])
        elif addr == "kseg":
            m, n, k = cell["b"] * cell["rows"], cell["n"], cell["t"] * cell["c"]
            shape = (cell["b"], cell["t"], cell["rows"], cell["c"])
        else:
            m, n, k = cell["b"] * cell["h"] * cell["w"], cell["cout"], cell["kh"] * cell["kw"] * cell["cin"]
            shape = (cell["b"], cell["h"], cell["w"], cell["cin"])             # NHWC memory
        co = k >= 384 and cell["arith"] in ("fp32", "bf16x3")                  # "coherent" operands: see the module docstring
        key = (addr, co) + shape + (n, k)
        if self.operands[0] != key:
            g = torch.Generator().manual_seed(1000 + sum((i + 1) * v for i, v in enumerate(shape + (n, k))))
            src = torch.randn(*shape, generator=g)
            w = torch.randn(n, k, generator=g) / k ** 0.5
            if co and m % 2:
                src, w = coherent(src.abs()), coherent(w)                      # (a0 b2 adds up; a2 b0 does where W is the positive one)
            elif co:
                src, w = coherent(src), coherent(w.abs())
            bias, res = torch.randn(n, generator=g), torch.randn(m, n, generator=g)
            self.operands = (key, (src, w, bias, res))
        src, w, bias, res = self.operands[1]
        return src, w, bias, res, m, n, k

    def forward_reference(self, cell, src, w, bias, res, q):
        addr = cell["addr"]
        a, wq = q(src).double(), q(w).double()
        if addr == "dense":
            y = a @ wq.t()
        elif addr == "rows":
            y = a[:, cell["ts"]].reshape(-1, cell["c"]) @ wq.t()
        elif addr == "kseg":
            y = a.permute(0, 2, 1, 3).reshape(a.shape[0] * a.shape[2], -1) @ wq.t()
        else:
            kh, kw, cin = cell["kh"], cell["kw"], cell["cin"]
            w4 = wq.reshape(-1, kh, kw, cin).permute(0, 3, 1, 2)               # (Cout, kh, kw, Cin) -> OIHW
            y = F.conv2d(a.permute(0, 3, 1, 2), w4, padding=(kh // 2, kw // 2)).permute(0, 2, 3, 1).reshape(-1, w4.shape[0])
        if cell["epi"] != "none":
            y = y + bias.double()
        if cell["epi"] == "gelu":
            y = F.gelu(y)
        if cell["epi"] == "res":
            y = y + res.double()
        return y

    def run_forward(self, cell):
        ops, dev = self.ops, self.dev
        src, w, bias, res, m, n, k = self.forward_operands(cell)
        arith, addr, epi = cell["arith"], cell["addr"], cell["epi"]
        storage16 = arith == "bf16s"
        if storage16:
            src, w = src.to(torch.bfloat16), w.to(torch.bfloat16)              # the operands ARE bf16: the reference takes them as stored
            ref = self.forward_reference(cell, src.float(), w.float(), bias, res, lambda t: t)
        else:
            ref = self.forward_reference(cell, src, w, bias, res, operand_rounding(arith))
        xd, wd = src.to(dev), w.to(dev)
        if addr == "conv":
            # the image sits in the middle of a zeroed allocation four image rows larger either side: a loader whose pixel decode
            # is wrong accepts taps up to three rows outside the image, and those reads must stay inside memory this process owns
            pad = 4 * cell["w"] * cell["cin"]
            held = torch.zeros(src.numel() + 2 * pad, device=dev)
            held[pad:pad + src.numel()] = xd.reshape(-1)
            xd = held[pad:pad + src.numel()].view(src.shape)
        bd = bias.to(dev) if epi != "none" else None
        rd = res.to(dev) if epi == "res" else None
        act = (ops.ACT_GELU if epi == "gelu" else ops.ACT_NONE) | MATH_BITS.get(arith, 0)
        out_dtype = torch.bfloat16 if cell.get("out16") else torch.float32
        p, ws, stream = ops._p, self.ws, ops._stream()
        outs, routes, guards = [], [], True
        for _ in range(2):
            buf, y = self.guarded(m, n, out_dtype)
            if storage16:
                ops._call("mumpy_linear_bf16s_fwd", p(xd), p(wd), p(bd), p(rd), p(y), m, n, k, act, 1 if cell["out16"] else 0, stream)
            elif addr == "dense":
                ops._call("mumpy_linear_wsz_fwd", p(xd), p(wd), p(bd), p(rd), p(y), m, n, k, act, p(ws), WS_BYTES, stream)
            elif addr == "rows":
                v = xd[:, cell["ts"]]
                ops._call("mumpy_linear_rows_fwd", v.data_ptr(), cell["rows"], v.stride(0), p(wd), p(bd), p(rd), p(y), m, n, k, act,
                          p(ws), WS_BYTES, stream)
            elif addr == "kseg":
                rows, c, t = cell["rows"], cell["c"], cell["t"]
                ops._call("mumpy_linear_rows_kseg_fwd", p(xd), rows, t * rows * c, c, rows * c, p(wd), p(bd), p(rd), p(y), m, n, k, act,
                          p(ws), WS_BYTES, stream)
            else:
                ops._call("mumpy_conv2d_nhwc_fwd", p(xd), p(wd), p(bd), p(rd), p(y), cell["b"], cell["h"], cell["w"], cell["cin"],
                          cell["cout"], cell["kh"], cell["kw"], act, p(ws), WS_BYTES, stream)
            routes.append(self.route())
            torch.cuda.synchronize()
            guards = guards and self.guards_ok(buf, m)
            outs.append(y)
        bar = (5e-3 if cell["out16"] else 2e-5) if storage16 else BAR[arith]
        return {"err": rel_err(outs[0].float().cpu(), ref), "bar": bar, "bitwise": bool(torch.equal(self.bits(outs[0]), self.bits(outs[1]))),
                "guards": guards, "got_route": routes[0], "route_ok": routes[0] == cell["route"] and routes[1] == cell["route"]}

    def run_lnfold(self, cell):
        """tests/test_hip_parity.py::test_layernorm_folded_into_its_gemms on a small shape, under the forced schedule."""
        ops, dev = self.ops, self.dev
        m, c, n, gelu = cell["m"], cell["c"], cell["n"], cell["gelu"]
        g = torch.Generator().manual_seed(m + n + c)
        h = torch.randn(m, c, generator=g)
        wp, bp = torch.randn(c, c, generator=g) / c ** 0.5, torch.randn(c, generator=g)
        r = torch.randn(m, c, generator=g)
        w, bias = torch.randn(n, c, generator=g) / c ** 0.5, torch.randn(n, generator=g)
        gam, bet = 1.0 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
        was = ops.LN_FOLD_MIN_K
        ops.LN_FOLD_MIN_K = 0
        hd, wpd, bpd, rd = h.to(dev), wp.to(dev), bp.to(dev), r.to(dev)
        try:
            x = ops.linear(hd, wpd, bpd, residual=rd, emit_stats=True)
        finally:
            ops.LN_FOLD_MIN_K = was
        route_p = self.route()
        st = ops.ln_stats_of(x)
        gn = (c + 127) // 128
        ok = st is not None and tuple(st.shape) == (m, gn, 2)
        errs = {}
        if ok:
            # statistics change nothing in x: the same GEMM without them, on the same schedule (ops.linear would pass no workspace
            # for so small a shape and so leave the forced split schedule)
            plain = torch.empty_like(x)
            ops._call("mumpy_linear_wsz_fwd", ops._p(hd), ops._p(wpd), ops._p(bpd), ops._p(rd), ops._p(plain),
                      m, c, c, ops.ACT_NONE, ops._p(self.ws), WS_BYTES, ops._stream())
            ok = self.route() == cell["route"].replace("ln=producer", "ln=none") and bool(torch.equal(x, plain))
            xd = x.cpu().double()
            if c % 128 == 0:
                tiles = xd.reshape(m, gn, -1)
                errs["mean"] = rel_err(st[..., 0].cpu(), tiles.mean(-1))
                errs["m2"] = rel_err(st[..., 1].cpu(), ((tiles - tiles.mean(-1, keepdim=True)) ** 2).sum(-1))
                ok = ok and errs["mean"] < 1e-5 and errs["m2"] < 1e-4
            ref = F.layer_norm(xd, (c,), gam.double(), bet.double(), 1e-5) @ w.double().t() + bias.double()
            if gelu:
                ref = F.gelu(ref)
            wg, cs, bpr = ops.fold_ln_weights(w.to(dev), bias.to(dev), gam.to(dev), bet.to(dev))
            a = ops.ACT_GELU if gelu else ops.ACT_NONE
            got = ops.linear_ln(x, st, wg, cs, bpr, 1e-5, act=a)
            route_c = self.route()
            again = ops.linear_ln(x, st, wg, cs, bpr, 1e-5, act=a)
            torch.cuda.synchronize()
            err, bitwise = rel_err(got.cpu(), ref), bool(torch.equal(got, again))
        else:
            route_c, err, bitwise = "", float("inf"), False
        return {"err": err, "bar": 5e-5, "bitwise": bitwise, "guards": ok, "got_route": route_p + " | " + route_c, "stats_err": errs,
                "route_ok": route_p == cell["route"] and route_c == cell["route2"]}

    def run_bwd(self, cell):
        ops, dev = self.ops, self.dev
        m, n, k, want, arith = cell["m"], cell["n"], cell["k"], cell["epi"], cell["arith"]
        g = torch.Generator().manual_seed(7 * m + 3 * n + k)
        x, w, dy = torch.randn(m, k, generator=g), torch.randn(n, k, generator=g) / k ** 0.5, torch.randn(m, n, generator=g)
        gw, gb = torch.randn(n, k, generator=g), torch.randn(n, generator=g)
        q = operand_rounding(arith)
        xr, wr, dyr = q(x).double(), q(w).double(), q(dy).double()
        # db: with dW it rides in the dW product's launch and sums the dY that launch staged (rounded to bf16 in bf16 mode:
        # test_hip_linear_bwd_bf16_operands); asked for alone it is a plain column sum of the fp32 dY -- no product, nothing rounded
        refs = {"dx": dyr @ wr, "dw": dyr.t() @ xr, "db": dy.double().sum(0) if want == "db" else dyr.sum(0)}
        xd, wd, dyd = x.to(dev), w.to(dev), dy.to(dev)

        def launch():
            if want == "all":
                dx, dw, db = ops.linear_bwd(xd, wd, dyd, need_dx=True, need_dw=True, need_db=True)
                return {"dx": dx, "dw": dw, "db": db}, {}
            if want == "dx":
                dx, dw, db = ops.linear_bwd(xd, wd, dyd, need_dx=True, need_dw=False, need_db=False)
                assert dw is None and db is None
                return {"dx": dx}, {}
            if want == "dw_db_acc":
                bw, bb = gw.to(dev), gb.to(dev)
                assert ops.linear_bwd(xd, wd, dyd, need_dx=False, need_dw=True, need_db=True, dw_out=bw, db_out=bb) == (None, None, None)
                return {"dw": bw, "db": bb}, {"dw": gw.double(), "db": gb.double()}
            dx, dw, db = ops.linear_bwd(None, None, dyd, need_dx=False, need_dw=False, need_db=True)
            assert dx is None and dw is None
            return {"db": db}, {}

        ops.set_matrix_math(arith)
        try:
            got, base = launch()
            route1 = self.route()
            again, _ = launch()
            route2 = self.route()
        finally:
            ops.set_matrix_math("fp32")
        torch.cuda.synchronize()
        err = max(rel_err(t.cpu(), refs[name] + base.get(name, 0.0)) for name, t in got.items())
        bitwise = all(bool(torch.equal(t, again[name])) for name, t in got.items())
        return {"err": err, "bar": 1e-5 if arith == "fp32" else 2e-5, "bitwise": bitwise, "guards": True, "got_route": route1,
                "route_ok": route1 == cell["route"] and route2 == cell["route"], "digest": digest(got[name] for name in sorted(got))}

    def run_wgrad(self, cell):
        ops, dev = self.ops, self.dev
        b, h, w, cin, cout, kh, kw, acc, arith = (cell[v] for v in ("b", "h", "w", "cin", "cout", "kh", "kw", "acc", "arith"))
        g = torch.Generator().manual_seed(b + 5 * h + 11 * w + cin + 3 * cout + kh)
        x, dy = torch.randn(b, cin, h, w, generator=g), torch.randn(b, cout, h, w, generator=g)
        base = torch.randn(cout, kh, kw, cin, generator=g)
        q = operand_rounding(arith)
        wt = torch.zeros(cout, cin, kh, kw, dtype=torch.float64, requires_grad=True)
        F.conv2d(q(x).double(), wt, padding=(kh // 2, kw // 2)).backward(q(dy).double())
        ref = wt.grad.permute(0, 2, 3, 1)
        if acc:
            ref = ref + base.double()
        xd = x.to(dev).contiguous(memory_format=torch.channels_last)
        dyd = dy.to(dev).contiguous(memory_format=torch.channels_last)

        def launch():
            if acc:
                buf = base.to(dev)
                assert ops.conv2d_wgrad(xd, dyd, kh, kw, dw_out=buf) is None
                return buf
            return ops.conv2d_wgrad(xd, dyd, kh, kw)

        ops.set_matrix_math(arith)
        try:
            got = launch()
            route1 = self.route()
            again = launch()
            route2 = self.route()
        finally:
            ops.set_matrix_math("fp32")
        torch.cuda.synchronize()
        return {"err": rel_err(got.cpu(), ref), "bar": 1e-5 if arith == "fp32" else 2e-5, "bitwise": bool(torch.equal(got, again)),
                "guards": True, "got_route": route1, "route_ok": route1 == cell["route"] and route2 == cell["route"], "digest": digest([got])}

    def run(self, cell):
        if cell["epi"] == "ln":
            return self.run_lnfold(cell)
        if cell["id"].startswith("bwd-"):
            return self.run_bwd(cell)
        if cell["id"].startswith("wgrad-"):
            return self.run_wgrad(cell)
        return self.run_forward(cell)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?")
    ap.add_argument("--list", action="store_true")
    args = ap.parse_args()
    if args.list:
        for name in CONFIGS:
            for cell in cases(name):
                print(json.dumps(dict(cell, config=name, env=CONFIGS[name])))
        return 0
    t0 = time.time()
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 8)))
    runner = Runner(args.config)
    assert runner.lib.mumpy_tuning_build() == 1, "the forced configurations need the diagnostics build (MUMPY_HIP_LIB)"
    for name, value in CONFIGS[args.config].items():
        assert os.environ.get(name) == value, f"configuration {args.config} needs {name}={value}"
    failed, n = [], 0
    for cell in cases(args.config):
        r = runner.run(cell)
        r["ok"] = bool(r["err"] < r["bar"] and r["bitwise"] and r["guards"] and r["route_ok"])
        print(json.dumps(dict(r, id=cell["id"], route=cell["route"])), flush=True)
        n += 1
        if not r["ok"]:
            failed.append(cell["id"])
    torch.cuda.synchronize()
    runner.ops.check_workspaces()                       # raises if a split launch gave up waiting for a part
    flags_zero = not bool(runner.ws[:1024].view(torch.int32).any())
    print(json.dumps({"done": True, "config": args.config, "cells": n, "failed": failed, "flags_zero": flags_zero,
                      "seconds": round(time.time() - t0, 1)}), flush=True)
    return 0 if not failed and flags_zero else 1


if __name__ == "__main__":
    sys.exit(main())
