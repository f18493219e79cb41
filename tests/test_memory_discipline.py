"""Memory discipline of every operator family: guard bands intact, outputs fully written, inputs kept, values independent of where
the buffers sit.  The per-operator tests elsewhere compare VALUES; three kinds of mistake pass them: a store one row or one tile past
an output or a workspace (the caching allocator packs a usually dead neighbour there), an output element that is never stored
(torch.empty hands back the block of the previous, correct call), and a kernel that modifies an input.  tests/guarded_alloc.py
intercepts the allocations mumpy_hip.ops / mumpy_hip.autograd already make and surrounds each with 4 KB bands of a fill pattern.

CPU tests (no GPU): the proxy reproduces shapes / strides / dtypes, and the harness FAILS on a band write, an unwritten row, a
modified input and a written `partial` region, and passes when an op legitimately stores the fill pattern.  They are the proof that
the harness can fail; no kernel is ever made to write out of bounds for that.  Three of them pin down what patterns A and B alone
cannot see and the per-block third pass of tests/guarded_alloc.py can: a store past an output whose value was loaded from past an
input -- summed (op_stray_sum), copied verbatim (op_stray_copy), and the db reduce of mumpy_dwconv5_window_bwd with the column bound
it had before its fix, restated on the host at (n, cg) = (6, 32) (op_window_db_reduce; the old kernel is never rebuilt or run).
Under 0xFF and under 0x7F every band compares intact, under per-block bytes the output's block is named.

GPU test (marked gpu test by test, because this file also holds the CPU tests): one parametrised test over CASES.  Each case runs
its call unguarded, then under the guard with pattern 0xFF (NaN), with pattern 0x7F (3.39e38) and with per-block bytes 0x3B..0x3F,
in one process on the current stream, and asserts (a) bands, (b) full writes (decided by the first two), (c) inputs kept, and that
all three guarded results are BITWISE equal to the unguarded one.  Values are not re-checked.  Shapes: parametrisations an existing
test already launches, the smallest and most ragged of each family (the test each comes from is named at the case) -- and, for the
cross-view chain, the four side-view widths C = 96, 192, 384, 768 (group width 32, 64, 128, 256) at the smallest window counts:
dwconv5_window(_bwd) at (n, cg) with n in {1, 6}, deform_sample_bwd and deform_attention_bwd (fp32 and bf16) at (windows, r) = (2, 3)
and with groups = 2 at (4, 3) for C = 96 and 768, deform_offsets / deform_sample_kv / deform_out_combine at C = 384 and 768; the
values of the two backward ops at these widths are held by tests/test_swin_backward.py (..._side_view_widths, against fp64).
Three families differ from a literal reading of their issue: the 7 x 7
window-attention backward runs with shift 0 only (the existing tests force shift 0 on a one-window grid; the shifted backward is
covered at 14 x 14), the fused cross-view GEMMs run at (C, side, r) = (96, 14, 1) and (192, 14, 3) (the existing set has no
(96, 14, 3)), and deform_offsets runs in the one-window form its own test uses.

GPU test of the whole model (test_whole_model_under_the_guard): the three-view model's eval forward (fp32; bf16 storage with bf16
window and cross-view attention) at B = 1 and its training tape (fp32 at B = 1; bf16 window and cross-view attention, fused MLP and
per-clip pairing at B = 2), T = 3, with the proxy in mumpy_hip.ops, mumpy_hip.autograd and the three models.* modules that allocate.
Each configuration runs twice unguarded (bitwise equal: the precondition) and once per pass; every band of every block must be
intact after a device-wide synchronise, the clip and the target unchanged, the logits and every parameter gradient bitwise those of
the unguarded run.  Check (b) is not applied: intermediates are not outputs.  Seen on an MI355X (launches through ops._call; guarded
blocks, the same under every pass, clip and target included):
    eval-fp32-b1                               727 launches,   766 blocks
    eval-bf16-storage-b1                       731 launches,   772 blocks
    train-fp32-b1                             1693 launches,  3505 blocks   (logits + 1177 parameter gradients compared)
    train-bf16-attention-fused-mlp-clip-b2    1561 launches,  3442 blocks   (the same)
All of it passed as found: no kernel or wrapper needed a fix.  On a band failure the configuration runs once more with the damaged
blocks watched after every launch (_watching_call; its report path has a CPU test beside it) and the failure names the first entry
point after which a band changed, with its scalar arguments.

`partial` exemptions (regions an op must NOT write; they must still hold the pattern):
  * gn_resample/out_coff: channels [0, 256) of the 384-channel map -- the op writes the slice [256, 384) of a concatenated map;
  * set_channels/first-slice: channels [256, 320) -- the complement of the slice that one call fills;
  * copy_rows/strided-slice: channels [0, 256) -- set_channels(cat, 256, view) fills [256, 2560) only.
Padding that a kernel zero-fills counts as written and is checked as such: avgpool2_pad's channels [C, Cpad), transpose's columns
[R, Rp), expand_relpos_bias's rows / key columns >= 49.
Unguarded allocation sites: Tensor.new_zeros in autograd.py (channel padding of the generic final-conv backward), torch.full in
ops.compact_attn_mask (host table), and the temporaries of tensor methods (.contiguous(), .sum(), slicing copies, and in the
whole-model test everything torch's own autograd and torch.cat / repeat / reshape allocate); an op's result that such a method
produced (deform_sample_bwd's dpos = part.sum(...), at every width: UNGUARDED_RESULTS) is compared bitwise only -- an unwritten
element of the guarded buffer behind it is NaN under pattern A and breaks that comparison.
What the harness sees since the third pass: a store within 4 KB of a buffer whatever its value was computed from, another block's
band included.  What it still cannot see: out-of-bounds READS that reach no result (one that reaches a result changes it between
the passes and breaks the bitwise comparison), writes further than 4 KB from a buffer, a stray store whose value was loaded from
the band of the very block it lands in, and a verbatim copy between the bands of two blocks whose allocations lie a multiple of
five apart (five bytes in the cycle).
Out of scope: graph capture / replay, ops.background, the multi-stream pipeline, tests/gemm_route_worker.py (it has guard rows)."""
import contextlib
import functools
import os
import types
from collections import namedtuple

import numpy as np
import pytest
import torch

import guarded_alloc as GA
from conftest import GOLDEN
from weight_fill import fill_module_, seeded_randn

gpu = pytest.mark.gpu


# ================================================================================================ CPU: the harness itself
def _fake_module():
    """A stand-in for mumpy_hip.ops: a namespace whose `torch` the guard swaps, and 'ops' that allocate through it."""
    fake = types.SimpleNamespace(torch=torch)

    def op_full(x):
        out = fake.torch.empty_like(x)
        out.copy_(x * 2)
        return out

    def op_skips_row(x):
        out = fake.torch.empty(x.shape, dtype=x.dtype)
        out[:-1] = x[:-1] * 2
        return out

    def op_scribbles(x):
        x[0, 0] = 7.0
        return op_full(x)

    def op_slice(x, out, coff, overrun=0):
        out[:, coff:coff + x.shape[1] + overrun] = 1.0
        return out

    def past(t):
        """The element just past the end of a dense tensor: the first one of the band behind its block."""
        return t.as_strided((1,), (1,), t.storage_offset() + t.numel())

    def op_stray_sum(x):
        """One wrong bound shared by a load and a store: x[n] + x[0] lands one element past out."""
        out = op_full(x)
        past(out).copy_(past(x) + x.reshape(-1)[:1])
        return out

    def op_stray_copy(x):
        """... and a verbatim copy from the input's band into the output's band."""
        out = op_full(x)
        past(out).copy_(past(x))
        return out

    def op_window_db_reduce(part, n, c, bound):
        """Host restatement of the db launch of window_partial_reduce (csrc/deform_bwd.hip): part is the (n, 26 c) image of per-window
        partials, the launch starts at column 25 c of each row and runs (c + 63) / 64 blocks of 64 columns, db[i] = sum_n part[n][25 c
        + i] in ascending n for every column i < bound.  bound = "count" is the kernel (i < c); bound = "width" is what it was before
        its fix (i < 26 c, the row stride): at c = 32 the one block stores 32 floats past db, the last of its terms loaded from past
        the end of part."""
        db = fake.torch.empty(c, dtype=torch.float32)
        width = 26 * c
        cols = min((c + 63) // 64 * 64, {"count": c, "width": width}[bound])
        src = part.as_strided((n, cols), (width, 1), part.storage_offset() + 25 * c)
        acc = src[0].clone()
        for k in range(1, n):
            acc = acc + src[k]
        db.as_strided((cols,), (1,), db.storage_offset()).copy_(acc)
        return db

    fake.op_full, fake.op_skips_row, fake.op_scribbles, fake.op_slice = op_full, op_skips_row, op_scribbles, op_slice
    fake.op_stray_sum, fake.op_stray_copy, fake.op_window_db_reduce = op_stray_sum, op_stray_copy, op_window_db_reduce
    return fake


REQUESTS = [
    ("contiguous", lambda T: T.empty(3, 5, 7, dtype=torch.float32)),
    ("size-tuple", lambda T: T.empty((4, 6), dtype=torch.float32, device="cpu")),
    ("channels_last", lambda T: T.empty(2, 8, 5, 3, dtype=torch.float32, memory_format=torch.channels_last)),
    ("empty_nhwc", lambda T: T.empty(2, 5, 3, 8, dtype=torch.float32).permute(0, 3, 1, 2)),
    ("permuted-empty_like", lambda T: T.empty_like(torch.zeros(2, 5, 3, 8).permute(0, 3, 1, 2))),
    ("channels_last-empty_like", lambda T: T.empty_like(torch.zeros(2, 8, 5, 3).contiguous(memory_format=torch.channels_last))),
    ("degenerate-nhwc", lambda T: T.empty(1, 1, 1, 32, dtype=torch.float32).permute(0, 3, 1, 2)),
    ("bf16", lambda T: T.empty(37, 96, dtype=torch.bfloat16)),
    ("uint8", lambda T: T.empty(2, 1, 13, 11, dtype=torch.uint8)),
    ("int32", lambda T: T.empty(2401, dtype=torch.int32)),
    ("odd-bytes", lambda T: T.empty(3, dtype=torch.uint8)),
    ("no-elements", lambda T: T.empty(0, 96, dtype=torch.float32)),
    ("zeros", lambda T: T.zeros(33, 7, dtype=torch.float32)),
    ("zeros-1d", lambda T: T.zeros(1024, dtype=torch.float32, device="cpu")),
]


@pytest.mark.parametrize("name,request_", REQUESTS, ids=[r[0] for r in REQUESTS])
@pytest.mark.parametrize("pattern", GA.PATTERNS)
def test_proxy_reproduces_the_real_allocation(name, request_, pattern):
    guard = GA.Guard(pattern)
    got, want = request_(guard.torch), request_(torch)
    assert got.shape == want.shape and got.stride() == want.stride() and got.dtype == want.dtype and got.device == want.device
    assert got.data_ptr() % 16 == 0
    assert GA._bytes(got).shape == (*got.shape, got.element_size()) and GA._bytes(got).dtype == torch.uint8
    a = guard.log[-1]
    assert a.raw.dtype == torch.uint8 and a.lo == GA.BAND and a.raw.numel() - a.hi >= GA.BAND and (a.raw.numel() - 2 * GA.BAND) % 16 == 0
    assert bool((a.raw[:a.lo] == pattern).all()) and bool((a.raw[a.hi:] == pattern).all())
    if name.startswith("zeros"):
        assert not got.any()
    else:
        assert bool((a.raw == pattern).all())
    if got.numel():
        got.fill_(1)                                   # the whole view lies inside the interior
    assert guard.band_hits() == []


def test_patterns_read_as_nan_and_as_a_huge_value():
    a, b = GA.Guard(GA.PATTERN_A), GA.Guard(GA.PATTERN_B)
    assert bool(a.torch.empty(4, dtype=torch.float32).isnan().all()) and bool(a.torch.empty(4, dtype=torch.bfloat16).isnan().all())
    assert bool((b.torch.empty(4, dtype=torch.float32) > 3.3e38).all())


def test_proxy_is_installed_per_module_only(monkeypatch):
    fake = _fake_module()
    fake._KEPT_WS, fake._RETIRED_WS, resets = {"k": 1}, [2], []
    fake.reset_workspaces = lambda: resets.append(len(fake._KEPT_WS))
    real_empty = torch.empty
    guard = GA.Guard(GA.PATTERN_A)
    with guard.installed(monkeypatch, fake):
        assert fake.torch is guard.torch and torch.empty is real_empty and fake.torch.float32 is torch.float32
        assert fake._KEPT_WS == {} and fake._RETIRED_WS == []           # kept workspaces are reallocated inside the guard
        fake.op_full(torch.ones(2, 2))
        assert len(guard.log) == 1
    assert fake.torch is torch and fake._KEPT_WS == {"k": 1} and fake._RETIRED_WS == [2]
    assert resets == [1, 1]                                              # reset_workspaces before entering and after leaving


def _body(fake, op, x, **kw):
    def body(guard):
        return {"y": getattr(fake, op)(guard.tensor(x))}, kw.get("inplace", ()), None
    return body


def test_harness_passes_a_clean_op(monkeypatch):
    fake, x = _fake_module(), seeded_randn(1, 6, 5)
    runs, unguarded = GA.run_both(monkeypatch, [fake], _body(fake, "op_full", x))
    assert len(runs) == len(GA.PASSES) == 3 and all(GA.same_bits(r["y"], x * 2) for r in runs) and unguarded == set()

    def body(guard):                                                     # a result that a tensor method allocated is reported as unseen
        return {"y": fake.op_full(guard.tensor(x)).sum(0)}, (), None
    assert GA.run_both(monkeypatch, [fake], body)[1] == {"y"}


@pytest.mark.parametrize("where", ["front", "behind", "slack"])
def test_a_write_into_a_band_fails_check_a(monkeypatch, where):
    fake, x = _fake_module(), seeded_randn(1, 3, 5)                       # 60 bytes: 4 bytes of slack up to the multiple of 16

    def body(guard):
        y = fake.op_full(guard.tensor(x))
        a = guard.log[-1]
        a.raw[{"front": a.lo - 1, "behind": a.raw.numel() - 1, "slack": a.hi}[where]] = 0
        return {"y": y}, (), None
    with pytest.raises(AssertionError, match="guard band overwritten"):
        GA.run_both(monkeypatch, [fake], body)


def test_an_unwritten_row_fails_check_b_in_both_patterns(monkeypatch):
    fake, x = _fake_module(), seeded_randn(1, 6, 5)
    masks = []
    for pattern in GA.PATTERNS:                                          # each pattern on its own sees the row ...
        guard = GA.Guard(pattern)
        with guard.installed(monkeypatch, fake):
            guard.check({"y": fake.op_skips_row(guard.tensor(x))})
        masks.append(guard.unwritten["y"])
        assert masks[-1].tolist() == [[False] * 5] * 5 + [[True] * 5]
    with pytest.raises(AssertionError, match=r"y: 5 of 30 elements never written .* first at \[5, 0\], last at \[5, 4\]"):
        GA.run_both(monkeypatch, [fake], _body(fake, "op_skips_row", x))          # ... and together they decide


def test_an_op_that_stores_the_fill_pattern_passes(monkeypatch):
    """What the two-pattern rule is for: y[2, 3] is legitimately NaN with all bits set, the very bytes of pattern A."""
    fake = _fake_module()
    x = seeded_randn(1, 6, 5)
    x[2, 3] = torch.tensor([-1], dtype=torch.int32).view(torch.float32)[0]
    guard = GA.Guard(GA.PATTERN_A)
    with guard.installed(monkeypatch, fake):
        fake.torch.empty(1)
        y = fake.torch.empty_like(x)
        y.copy_(x)
        guard.check({"y": y})
    assert int(guard.unwritten["y"].sum()) == 1 and bool(guard.unwritten["y"][2, 3])     # one pattern alone cannot tell

    def body(guard):
        y = fake.torch.empty_like(x)
        y.copy_(guard.tensor(x))
        return {"y": y}, (), None
    GA.run_both(monkeypatch, [fake], body)


def test_a_modified_input_fails_check_c(monkeypatch):
    fake, x = _fake_module(), seeded_randn(1, 6, 5)
    with pytest.raises(AssertionError, match=r"input 0 \(6, 5\) torch.float32 was modified"):
        GA.run_both(monkeypatch, [fake], _body(fake, "op_scribbles", x))

    def body(guard):                                                     # the same op with its operand declared in-place passes
        xd = guard.tensor(x)
        return {"y": fake.op_scribbles(xd)}, (xd,), None
    GA.run_both(monkeypatch, [fake], body)


@pytest.mark.parametrize("overrun", [0, 1])
def test_a_declared_partial_region_must_stay_untouched(monkeypatch, overrun):
    fake, x = _fake_module(), torch.ones(4, 3)

    def body(guard):
        out = fake.torch.empty(4, 8, dtype=torch.float32)
        fake.op_slice(guard.tensor(x), out, 2, overrun)
        return {"out": out}, (), {"out": ((slice(None), slice(5, 8)), "the op fills columns [2, 5) ...")}
    if overrun:
        with pytest.raises(AssertionError, match="declared-untouched region .* was written \\(4 elements"):
            GA.run_both(monkeypatch, [fake], body)
    else:                                                                # columns [0, 2) are neither declared nor written
        with pytest.raises(AssertionError, match="out: 8 of 32 elements never written"):
            GA.run_both(monkeypatch, [fake], body)

    def body_ok(guard):
        out = fake.torch.empty(4, 8, dtype=torch.float32)
        fake.op_slice(guard.tensor(torch.ones(4, 6)), out, 2, 0)
        return {"out": out}, (), {"out": ((slice(None), slice(0, 2)), "the op fills columns [2, 8)")}
    GA.run_both(monkeypatch, [fake], body_ok)


# ------------------------------------------------------------------------------------------------ CPU: the per-block third pass
def test_per_block_bytes_differ_between_neighbours_and_read_as_ordinary_numbers():
    guard = GA.Guard(GA.CYCLE)
    assert GA.PASSES == (GA.PATTERN_A, GA.PATTERN_B, GA.CYCLE) and GA.CYCLE == (0x3B, 0x3C, 0x3D, 0x3E, 0x3F)
    made = []
    for i in range(13):                                                  # proxy allocations and tensor() blocks, interleaved
        announced = guard.pattern                                        # the byte the next block gets
        if i % 3 == 1:
            made.append(("tensor", guard.tensor(seeded_randn(i, 3, 5))))
        elif i % 3 == 2:
            made.append(("zeros", guard.torch.zeros(7, dtype=torch.float32)))
        else:
            made.append(("empty", guard.torch.empty(2, 9, dtype=torch.bfloat16 if i % 2 else torch.float32)))
        assert guard.log[-1].fill == announced
    fills = [a.fill for a in guard.log]
    assert len(fills) == 13 and set(fills) == set(GA.CYCLE)
    assert all(x != y for x, y in zip(fills, fills[1:]))                 # consecutive allocations never share a byte
    for (kind, view), a in zip(made, guard.log):
        assert bool((a.raw[:a.lo] == a.fill).all()) and bool((a.raw[a.hi:] == a.fill).all())
        if kind == "empty":                                              # the interior carries the block's byte too ...
            assert bool((a.raw == a.fill).all())
            assert bool(((view.float() > 2.8e-3) & (view.float() < 0.75)).all())          # ... an ordinary magnitude in fp32 and bf16
        assert a.site == ("Guard.tensor" if kind == "tensor" else "test_per_block_bytes_differ_between_neighbours_and_read_as_ordinary_numbers")
    assert guard.band_hits() == []
    guard.check({"y": made[0][1]})                                       # (a) and (c) only: nothing said about the unwritten output
    assert guard.unwritten == {} and guard.unguarded == set()
    a, b = guard.log[3], guard.log[4]
    b.raw[b.lo - 4:b.lo] = a.fill                                        # the neighbour's byte in a band is a hit ...
    assert guard.band_hits() == [(4, b.site, tuple(b.view.shape), 4, 0)] and guard.band_hits(only=[3]) == []
    with pytest.raises(AssertionError, match=r"guard band overwritten \(per-block bytes 0x3b..0x3f\)"):
        guard.check({})
    b.raw[b.lo - 4:b.lo] = b.fill                                        # ... the block's own is not
    assert guard.band_hits() == []


def test_allocations_are_tagged_with_the_innermost_function_of_a_proxied_module(monkeypatch):
    mod = types.ModuleType("somepkg.fakeops")
    exec("def outer(n):\n    return inner(n)\n\n\ndef inner(n):\n    return torch.empty(n), helper.op_full(torch.zeros(n))\n", mod.__dict__)
    mod.torch, mod.helper = torch, _fake_module()                        # helper's functions live in this file: their frames are passed over
    guard = GA.Guard(GA.PATTERN_A)
    with guard.installed(monkeypatch, mod, mod.helper):
        mod.outer(4)
        guard.tensor(torch.ones(2))
    assert [a.site for a in guard.log] == ["fakeops.inner", "fakeops.inner", "fakeops.inner", "Guard.tensor"]
    guard.log[1].raw[0] = 0
    assert guard.band_hits() == [(1, "fakeops.inner", (4,), 1, 0)]
    with pytest.raises(AssertionError, match=r"guard band overwritten \(pattern 0xff\).*\(1, 'fakeops.inner', \(4,\), 1, 0\)"):
        guard.check({})


def _one_pass(monkeypatch, fake, pattern, run):
    """run(guard) under one pattern alone -> the guard, after its own checks (a) and (c)."""
    guard = GA.Guard(pattern)
    with guard.installed(monkeypatch, fake):
        outputs = run(guard)
        assert guard.band_hits() == []
        guard.check(outputs)
    return guard


@pytest.mark.parametrize("op", ["op_stray_sum", "op_stray_copy"])
def test_a_store_fed_by_a_stray_load_passes_patterns_a_and_b_and_fails_the_third_pass(monkeypatch, op):
    """The blind spot as a fact: both patterns absorb the addition (NaN + x is the same NaN, 3.39e38 + x rounds back), and a copy
    carries the pattern over, so the element written past `out` holds the band's own bytes.  Per-block bytes tell the two bands
    apart."""
    fake, x = _fake_module(), seeded_randn(1, 6, 5)
    for pattern in GA.PATTERNS:
        guard = _one_pass(monkeypatch, fake, pattern, lambda g: {"y": getattr(fake, op)(g.tensor(x))})
        out = guard.log[1]
        assert bool((out.raw[out.hi:out.hi + 4] == pattern).all())       # the stray store happened, and wrote the pattern
    with pytest.raises(AssertionError, match=rf"guard band overwritten \(per-block bytes.*\[\(1, 'op_full', \(6, 5\), 0, [1-4]\)\]"):
        GA.run_both(monkeypatch, [fake], _body(fake, op, x))             # names the output's block: index 1, after the input's
    guard = GA.Guard(GA.CYCLE)
    with guard.installed(monkeypatch, fake):
        getattr(fake, op)(guard.tensor(x))
    (hit,) = guard.band_hits()
    assert hit[0] == 1 and hit[3] == 0 and hit[4] >= 1 and guard.log[0].fill != guard.log[1].fill


def test_the_old_dwconv5_db_reduce_bound_passes_patterns_a_and_b_and_fails_the_third_pass(monkeypatch):
    """(n, cg) = (6, 32), the stage-1 launch of the model: with the column bound i < 26 c the reduce stores 32 floats past db, each a
    sum whose last term comes from past the end of the partials.  Patterns A and B leave every band intact; the third pass names db.
    With the kernel's bound (i < c) all three pass."""
    fake, n, c = _fake_module(), 6, 32
    part = seeded_randn(7, n, 26 * c)

    def body(bound):
        return lambda g: ({"db": fake.op_window_db_reduce(g.tensor(part), n, c, bound)}, (), None)
    for pattern in GA.PATTERNS:
        guard = _one_pass(monkeypatch, fake, pattern, lambda g: body("width")(g)[0])
        db = guard.log[1]
        assert db.view.shape == (c,) and bool((db.raw[db.hi:db.hi + 128] == pattern).all())
        assert torch.allclose(db.view, part[:, 25 * c:].sum(0), rtol=1e-5, atol=1e-6)              # db itself is right all along
    with pytest.raises(AssertionError, match=r"guard band overwritten \(per-block bytes.*\[\(1, 'op_window_db_reduce', \(32,\), 0, 128\)\]"):
        GA.run_both(monkeypatch, [fake], body("width"))
    runs, unguarded = GA.run_both(monkeypatch, [fake], body("count"))
    assert unguarded == set() and all(GA.same_bits(r["db"], runs[0]["db"]) for r in runs)


# ================================================================================================ GPU: the case table
Case = namedtuple("Case", "id build inplace partial")
CASES = []


def case(id_, inplace=(), partial=None):
    """Registers build() -> (inputs {name: CPU tensor}, call(ops, t) -> {name: output}); t.<name> are the device tensors.  inplace:
    names of inputs the op updates; partial: {output: (index, reason)}."""
    def deco(build):
        CASES.append(Case(id_, build, tuple(inplace), partial or {}))
        return build
    return deco


class _T(dict):
    __getattr__ = dict.__getitem__


def _nhwc(x):
    """Logical (B,C,H,W) with exactly the NHWC strides the kernels address (also for degenerate sizes)."""
    return x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)


def _bias_pad(table):
    """(169, nH) -> the (nH, 64, 64) padded bias of ops.expand_relpos_bias, on the CPU."""
    from models.modules.swinTransformer import relative_position_index
    nh = table.shape[1]
    b = torch.zeros(nh, 64, 64)
    b[:, :, 49:] = -1e30
    b[:, :49, :49] = table[relative_position_index(7, 7).reshape(-1)].reshape(49, 49, nh).permute(2, 0, 1)
    return b


def _shift_mask(hs, w, shift):
    """-> {"tab": ..., "ids": ...} CPU operands of the shifted window attention (empty dict for shift 0)."""
    if not shift:
        return {}
    from models.modules.swinTransformer import build_shift_mask
    from mumpy_hip import ops
    tab, ids = ops.compact_attn_mask(build_shift_mask(hs, w, 7, shift))
    return {"tab": tab, "ids": ids}


# ---------------------------------------------------------------------------------------------------------------- norms
for _c in (96, 4096):                                                    # test_layernorm: 37 rows
    @case(f"layernorm/c{_c}")
    def _(c=_c):
        i = {"x": seeded_randn(c, 37, c) * 3 + 1, "g": seeded_randn(c + 1, c), "b": seeded_randn(c + 2, c)}
        return i, lambda ops, t: {"y": ops.layernorm(t.x, t.g, t.b)}

for _rows, _c in ((37, 96), (1000, 384)):                                # test_layernorm_offset_rows / test_layernorm_bf16_output
    @case(f"layernorm_bf16/{_rows}x{_c}")
    def _(rows=_rows, c=_c):
        i = {"x": seeded_randn(31, rows, c) * 3 + 1, "g": seeded_randn(32, c), "b": seeded_randn(33, c)}
        return i, lambda ops, t: {"y": ops.layernorm_bf16(t.x, t.g, t.b)}


@case("patch_merge_ln/42x14x96")                                         # test_patch_merging / test_patch_merge_layernorm_offset_rows
def _():
    i = {"x": seeded_randn(40, 1, 42 * 14, 96), "g": 1 + 0.1 * seeded_randn(41, 384), "b": 0.1 * seeded_randn(42, 384)}
    return i, lambda ops, t: {"y": ops.patch_merge_ln(t.x, t.g, t.b, 1, 42, 14, 96)}


@functools.lru_cache(maxsize=None)
def _tokenizer():
    from models.encoder.multiTemporalViewEncoder import CrossThreeViewTokenize
    from models.factory.modelFactory import multiswin_view_configs
    return fill_module_(CrossThreeViewTokenize(multiswin_view_configs(3)).eval(), "tok/")


for _v in range(3):                                                      # test_tokenizer: T = 3, the three views' tubelets
    @case(f"patch_embed/tokenizer-t3-view{_v + 1}")
    def _(v=_v):
        tk = _tokenizer()
        proj, norm = getattr(tk, f"project{v + 1}"), getattr(tk, f"norm{v + 1}")
        w = proj.weight.detach()
        i = {"x": seeded_randn(50, 1, 3, 3, 224, 224), "wt": w.reshape(w.shape[0], -1).t().contiguous(), "bias": proj.bias.detach(),
             "g": norm.weight.detach(), "b": norm.bias.detach()}
        return i, lambda ops, t: {"y": ops.patch_embed(t.x, t.wt, t.bias, t.g, t.b, w.shape[2], norm.eps)}


def _ln_bwd_inputs(rows, c):
    return {"x": seeded_randn(1, rows, c) * 2 + 0.5, "g": 1 + 0.1 * seeded_randn(2, c), "dy": seeded_randn(4, rows, c)}


for _rows, _c in ((5, 1024), (37, 128)):                                 # test_hip_layernorm_bwd
    @case(f"layernorm_bwd/{_rows}x{_c}")
    def _(rows=_rows, c=_c):
        def call(ops, t):
            dx, dg, db = ops.layernorm_bwd(t.x, t.g, t.dy, 1e-5)
            return {"dx": dx, "dg": dg, "db": db}
        return _ln_bwd_inputs(rows, c), call

    @case(f"layernorm_bwd/{_rows}x{_c}-dx_add-accumulate", inplace=("gacc", "bacc"))
    def _(rows=_rows, c=_c):
        i = dict(_ln_bwd_inputs(rows, c), extra=seeded_randn(6, rows, c), gacc=torch.full((c,), 0.5), bacc=torch.full((c,), -2.0))

        def call(ops, t):
            dx, r1, r2 = ops.layernorm_bwd(t.x, t.g, t.dy, 1e-5, dx_add=t.extra, dg_out=t.gacc, db_out=t.bacc)
            assert r1 is None and r2 is None
            return {"dx": dx, "gacc": t.gacc, "bacc": t.bacc}
        return i, call


# ---------------------------------------------------------------------------------------- GEMM wrappers that own index logic
for _m, _n, _k in ((1, 128, 32), (129, 288, 96)):                        # test_linear
    for _act, _res in ((0, False), (1, True)):
        @case(f"linear/{_m}x{_n}x{_k}-{'gelu-residual' if _act else 'plain'}")
        def _(m=_m, n=_n, k=_k, act=_act, res=_res):
            i = {"x": seeded_randn(m, m, k), "w": seeded_randn(n, n, k) / k ** 0.5, "b": seeded_randn(k, n)}
            if res:
                i["r"] = seeded_randn(m + n, m, n)
            return i, lambda ops, t: {"y": ops.linear(t.x, t.w, t.b, act=act, residual=t.get("r"))}


@case("linear_time_slices/3x9x49x96->64")                                # test_linear_time_slices_segmented_k
def _():
    b, tt, n, c, nout = 3, 9, 49, 96, 64
    i = {"x": seeded_randn(60 + c, b, tt, n, c), "w": seeded_randn(61, nout, tt * c) / (tt * c) ** 0.5, "bias": seeded_randn(62, nout),
         "res": seeded_randn(63, b * n, nout)}
    return i, lambda ops, t: {"y": ops.linear_time_slices(t.x, t.w, t.bias, residual=t.res)}


@case("linear_rows/strided-time-slices")                                 # test_linear_rows_strided_time_slices, its first two links
def _():
    b, tt, n, c, nout = 3, 5, 196, 128, 256
    w = seeded_randn(2, nout, c, tt) / (c * tt) ** 0.5
    i = {"x": seeded_randn(1, b, tt, n, c), "w0": w[:, :, 0].contiguous(), "w1": w[:, :, 1].contiguous(), "bias": seeded_randn(3, nout)}

    def call(ops, t):
        y0 = ops.linear_rows(t.x[:, 0], t.w0, t.bias)
        return {"y0": y0, "y1": ops.linear_rows(t.x[:, 1], t.w1, None, residual=y0)}
    return i, call


@case("linear_ln/2000x1024x3072-emit_stats")                             # test_layernorm_folded_into_its_gemms, its last case
def _():
    from mumpy_hip import ops as _ops
    m, c, n, shift = 2000, 1024, 3072, 3.0
    kp = c if _ops.linear_ln_tiles(m, c, c) > 0 else 4 * c
    assert _ops.linear_ln_tiles(m, c, kp) > 0 and _ops.linear_ln_tiles(m, n, c) > 0, "shapes must run on the persistent kernel"
    g = torch.Generator().manual_seed(m + n)
    h = torch.randn(m, kp, generator=g)
    wp, bp = torch.randn(c, kp, generator=g) / kp ** 0.5, torch.randn(c, generator=g)
    r = torch.randn(m, c, generator=g) + shift
    w, bias = torch.randn(n, c, generator=g) / c ** 0.5, torch.randn(n, generator=g)
    gam, bet = 1.0 + 0.2 * torch.randn(c, generator=g), 0.2 * torch.randn(c, generator=g)
    wg, cs, bpr = _ops.fold_ln_weights(w, bias, gam, bet)
    i = {"h": h, "wp": wp, "bp": bp, "r": r, "wg": wg, "cs": cs, "bpr": bpr}

    def call(ops, t):
        x = ops.linear(t.h, t.wp, t.bp, residual=t.r, emit_stats=True)
        st = ops.ln_stats_of(x)
        assert st is not None and st.shape == (m, (c + 127) // 128, 2)
        return {"x": x, "stats": st, "y": ops.linear_ln(x, st, t.wg, t.cs, t.bpr, 1e-5)}
    return i, call


for _m, _n, _k, _act, _res in ((200, 96, 64, 0, True), (6272, 192, 96, 1, False)):          # test_linear_bf16_storage
    @case(f"linear_bf16s/{_m}x{_n}x{_k}")
    def _(m=_m, n=_n, k=_k, act=_act, res=_res):
        i = {"x": seeded_randn(m + n, m, k).bfloat16(), "w": (seeded_randn(m + n + 1, n, k) / k ** 0.5).bfloat16(), "b": seeded_randn(m + n + 2, n)}
        if res:
            i["r"] = seeded_randn(m + n + 3, m, n)

        def call(ops, t):
            out = {"y32": ops.linear_bf16s(t.x, t.w, t.b, act=act, residual=t.get("r"), out_bf16=False)}
            if not res:
                out["y16"] = ops.linear_bf16s(t.x, t.w, t.b, act=act, out_bf16=True)
            return out
        return i, call


def _linear_bwd_inputs():
    m, n, k = 50, 96, 96                                                 # test_hip_linear_bwd_one_call
    return {"x": seeded_randn(1, m, k), "w": seeded_randn(2, n, k) / k ** 0.5, "dy": seeded_randn(3, m, n)}


@case("linear_bwd/50x96x96")
def _():
    def call(ops, t):
        dx, dw, db = ops.linear_bwd(t.x, t.w, t.dy, need_dx=True, need_dw=True, need_db=True)
        return {"dx": dx, "dw": dw, "db": db, "only_dx": ops.linear_bwd(t.x, t.w, t.dy, need_dx=True, need_dw=False, need_db=False)[0]}
    return _linear_bwd_inputs(), call


@case("linear_bwd/50x96x96-accumulate", inplace=("gw", "gb"))
def _():
    i = dict(_linear_bwd_inputs(), gw=seeded_randn(4, 96, 96), gb=seeded_randn(5, 96))

    def call(ops, t):
        assert ops.linear_bwd(t.x, t.w, t.dy, need_dx=False, need_dw=True, need_db=True, dw_out=t.gw, db_out=t.gb) == (None, None, None)
        return {"gw": t.gw, "gb": t.gb}
    return i, call


@case("conv2d_nhwc/32->32-1x7-14x14")                                    # test_conv2d_nhwc
def _():
    b, cin, cout, kh, kw, h = 2, 32, 32, 1, 7, 14
    w = seeded_randn(cout + kh, cout, cin, kh, kw) / (cin * kh * kw) ** 0.5
    i = {"x": _nhwc(seeded_randn(cin + h, b, cin, h, h)), "w": w.permute(0, 2, 3, 1).contiguous(), "bias": seeded_randn(3, cout),
         "res": _nhwc(seeded_randn(4, b, cout, h, h))}
    return i, lambda ops, t: {"y": ops.conv2d_nhwc(t.x, t.w, t.bias, residual=t.res)}


def _wgrad_inputs():
    b, cin, cout, h, w = 2, 64, 32, 9, 11                                # test_hip_conv2d_wgrad_one_launch
    return {"x": _nhwc(seeded_randn(1, b, cin, h, w)), "dy": _nhwc(seeded_randn(2, b, cout, h, w))}


@case("conv2d_wgrad/2x64->32-3x3-9x11")
def _():
    return _wgrad_inputs(), lambda ops, t: {"dw": ops.conv2d_wgrad(t.x, t.dy, 3, 3)}


@case("conv2d_wgrad/2x64->32-3x3-9x11-accumulate", inplace=("acc",))
def _():
    def call(ops, t):
        assert ops.conv2d_wgrad(t.x, t.dy, 3, 3, dw_out=t.acc) is None
        return {"acc": t.acc}
    return dict(_wgrad_inputs(), acc=torch.full((32, 3, 3, 64), 0.25)), call


for _shape in ((32, 3, 3, 64), (7, 5, 3, 130)):                          # test_hip_conv_weight_dgrad_and_channels_last_slots
    @case("conv_weight_dgrad/" + "x".join(map(str, _shape)))
    def _(shape=_shape):
        return {"w": seeded_randn(40, *shape)}, lambda ops, t: {"y": ops.conv_weight_dgrad(t.w)}


# ------------------------------------------------------------------------------------------------------- window attention
def _wa_inputs(b, hs, w, c, shift, seed, bf16=False, dout=False):
    qkv = seeded_randn(seed, b, hs * w, 3 * c)
    i = {"qkv": qkv.bfloat16() if bf16 else qkv, "bias": _bias_pad(seeded_randn(701, 169, c // 32) * 0.2), **_shift_mask(hs, w, shift)}
    if dout:
        i["dout"] = seeded_randn(seed + 1, b, hs * w, c)
    return i


for _b, _hs, _w, _c, _s in ((1, 7, 7, 32, 0), (2, 14, 14, 64, 3)):       # test_window_attention_peaked_rows
    @case(f"window_attention/{_b}x{_hs}x{_w}x{_c}-shift{_s}")
    def _(b=_b, hs=_hs, w=_w, c=_c, s=_s):
        return (_wa_inputs(b, hs, w, c, s, 21),
                lambda ops, t: {"y": ops.window_attention(t.qkv, t.bias, b, hs, w, c, s, 32 ** -0.5, t.get("tab"), t.get("ids"))})

for _s in (0, 3):
    @case(f"window_attention_bf16/2x28x14x96-shift{_s}")                  # test_window_attention_bf16_storage
    def _(s=_s):
        return (_wa_inputs(2, 28, 14, 96, s, 700 + s, bf16=True),
                lambda ops, t: {"y": ops.window_attention_bf16(t.qkv, t.bias, 2, 28, 14, 96, s, 32 ** -0.5, t.get("tab"), t.get("ids"), math="fp32")})

    @case(f"window_attention_bf16mm/2x14x14x64-shift{_s}")                # test_bf16mm_layout_bit_exact
    def _(s=_s):
        return (_wa_inputs(2, 14, 14, 64, s, 900 + s, bf16=True),
                lambda ops, t: {"y": ops.window_attention_bf16(t.qkv, t.bias, 2, 14, 14, 64, s, 32 ** -0.5, t.get("tab"), t.get("ids"), math="bf16")})

for _b, _hs, _w, _c, _s in ((3, 7, 7, 32, 0), (2, 14, 14, 96, 3)):       # test_window_attention_bf16mm_train.CASES
    @case(f"window_attention_mm16/{_b}x{_hs}x{_w}x{_c}-shift{_s}")
    def _(b=_b, hs=_hs, w=_w, c=_c, s=_s):
        return (_wa_inputs(b, hs, w, c, s, 1201),
                lambda ops, t: {"y": ops.window_attention_mm16(t.qkv, t.bias, b, hs, w, c, s, 32 ** -0.5, t.get("tab"), t.get("ids"))})


def _wa_bwd_case(b, hs, w, c, s, math, acc):
    def build():
        from models.modules.swinTransformer import relative_position_index
        from mumpy_hip import ops as _ops
        rpi = relative_position_index(7, 7)
        i = dict(_wa_inputs(b, hs, w, c, s, 20, dout=True), idx32=_ops.rel_index32(rpi), csr=_ops.rel_index_csr(rpi))
        if acc:
            i["dtable"] = seeded_randn(77, 169, c // 32)

        def call(ops, t):
            args = (t.qkv, t.dout, t.bias, t.idx32, b, hs, w, c, s, 32 ** -0.5, t.get("tab"), t.get("ids"))
            if acc:
                d, none = ops.window_attention_bwd(*args, dtable_out=t.dtable, rel_csr=t.csr, math=math)
                assert none is None
                return {"dqkv": d, "dtable": t.dtable}
            d_scan, t_scan = ops.window_attention_bwd(*args, math=math)
            d_csr, t_csr = ops.window_attention_bwd(*args, rel_csr=t.csr, math=math)
            return {"dqkv_scan": d_scan, "dtable_scan": t_scan, "dqkv_csr": d_csr, "dtable_csr": t_csr}
        return i, call
    return build


# test_hip_window_attention_bwd_vs_oracle ((3,7,7,32): shift 0, as every test of a one-window grid), test_window_attention_peaked_rows
# ((2,14,14,64) shift 3), test_window_attention_bf16mm_train (math="bf16"; dtable_out at (2,280,56,128) there, at these shapes by the tape)
for _b, _hs, _w, _c, _s in ((3, 7, 7, 32, 0), (2, 14, 14, 64, 3)):
    for _math in ("fp32", "bf16") if _c == 32 else ("fp32",):
        case(f"window_attention_bwd/{_b}x{_hs}x{_w}x{_c}-shift{_s}-{_math}")(_wa_bwd_case(_b, _hs, _w, _c, _s, _math, False))
        case(f"window_attention_bwd/{_b}x{_hs}x{_w}x{_c}-shift{_s}-{_math}-dtable_out", inplace=("dtable",))(
            _wa_bwd_case(_b, _hs, _w, _c, _s, _math, True))


# ----------------------------------------------------------------------------------------------------- cross-view chain
for _c in (96, 384, 768):                                                # test_deform_offset_network_layernorm_offset_rows; 384, 768: the deep stages
    @case(f"deform_offsets/1x7x7x{_c}")
    def _(c=_c):
        from models.modules.deformableAttention import SwinDAttention
        sd = fill_module_(SwinDAttention(c, c // 32, 0.0, n_groups=3).eval(), "sda_r1/").state_dict()
        i = {"q": seeded_randn(60, 1, 49, c), "dw_w": sd["conv_offset.0.weight"], "dw_b": sd["conv_offset.0.bias"],
             "ln_g": sd["conv_offset.1.norm.weight"], "ln_b": sd["conv_offset.1.norm.bias"], "pw_w": sd["conv_offset.3.weight"]}
        i = {k: v.detach().clone() for k, v in i.items()}
        return i, lambda ops, t: {"pos": ops.deform_offsets(t.q, t.dw_w, t.dw_b, t.ln_g, t.ln_b, t.pw_w, 1, 7, 7, c)}


@case("deform_sample/window-form-3x49x96")                                # test_deform_sampling_hits_zero_padding
def _():
    i = {"x2": seeded_randn(5, 3, 49, 96), "pos": torch.rand(3, 3, 49, 2, generator=torch.Generator().manual_seed(9)) * 2.8 - 1.4}
    return i, lambda ops, t: {"y": ops.deform_sample(t.x2, t.pos, 3, 7, 7, 96, 3)}


# test_deform_fused_gemms_match_the_unfused_kernels + test_cva_bf16mm: b = 2, raster; (384, 14, 3) and (768, 7, 3) are the side views'
# stages 3 and 4 at their own map sizes, for the two fused GEMMs only
for _c, _side, _r, _whole_chain in ((96, 14, 1, True), (192, 14, 3, True), (384, 14, 3, False), (768, 7, 3, False)):
    def _cva_inputs(c=_c, side=_side, r=_r):
        b = 2
        nq = b * (side // 7) ** 2
        return {"x2": seeded_randn(50 + c, b, r * side * side, c),
                "pos": torch.rand(nq, 3, 49, 2, generator=torch.Generator().manual_seed(51 + c)) * 2.6 - 1.3,       # some corners outside
                "wkv": seeded_randn(52, 2 * c, c) / c ** 0.5, "bkv": seeded_randn(53, 2 * c), "o": seeded_randn(54 + c, nq, 49, c),
                "x1": seeded_randn(55 + c, b, side * side, c), "wout": seeded_randn(56, c, c) / c ** 0.5, "bout": seeded_randn(57, c)}

    if _whole_chain:
        @case(f"deform_sample/c{_c}-side{_side}-r{_r}")
        def _(c=_c, side=_side, r=_r, inputs=_cva_inputs):
            i = {k: v for k, v in inputs().items() if k in ("x2", "pos")}
            return i, lambda ops, t: {"y": ops.deform_sample(t.x2, t.pos, 2, r * side, side, c, t.pos.shape[0])}

    for _math in ("fp32", "bf16"):
        @case(f"deform_sample_kv/c{_c}-side{_side}-r{_r}-{_math}")
        def _(c=_c, side=_side, r=_r, math=_math, inputs=_cva_inputs):
            i = {k: v for k, v in inputs().items() if k in ("x2", "pos", "wkv", "bkv")}
            return i, lambda ops, t: {"kv": ops.deform_sample_kv(t.x2, t.pos, t.wkv, t.bkv, 2, r * side, side, c, t.pos.shape[0], math=math)}

        @case(f"deform_out_combine/c{_c}-side{_side}-{_math}")
        def _(c=_c, side=_side, math=_math, inputs=_cva_inputs):
            i = {k: v for k, v in inputs().items() if k in ("o", "x1", "wout", "bout")}
            return i, lambda ops, t: {"y": ops.deform_out_combine(t.o, t.wout, t.bout, t.x1, 2, side, side, c, math=math)}

    if _whole_chain:
        @case(f"deform_combine/c{_c}-side{_side}")
        def _(c=_c, side=_side, inputs=_cva_inputs):
            i = inputs()
            i = {"x1": i["x1"], "yt": seeded_randn(58 + c, *i["o"].shape)}
            return i, lambda ops, t: {"y": ops.deform_combine(t.x1, t.yt, 2, side, side, c)}

for _math in ("fp32", "bf16"):                                           # test_core_mm16_accuracy_...: (b, h, w, c, r) = (2, 14, 14, 96, 3)
    @case(f"deform_attention/2x14x14x96-r3-{_math}")
    def _(math=_math):
        from mumpy_hip import ops as _ops
        b, h, w, c, r = 2, 14, 14, 96, 3
        b1w = b * (h // 7) * (w // 7)
        i = {"q": seeded_randn(600 + c + r + 1, b, h * w, c), "kv": seeded_randn(601 + c + r + 1, b1w * r, 49, 2 * c), "pad": _ops.pad_mask()}
        return i, lambda ops, t: {"y": ops.deform_attention(t.q, t.kv, t.pad, b, h, w, c, r, 32 ** -0.5, math=math)}


def _sample_bwd_case(nq, r, c, groups):
    def build():
        i = {"x2": seeded_randn(110, nq * r, 49, c), "pos": (seeded_randn(111, nq, 3, 49, 2) * 0.7).clamp(-1.3, 1.3), "ds": seeded_randn(112, nq * r, 49, c)}

        def call(ops, t):
            dx2, dpos = ops.deform_sample_bwd(t.x2, t.pos, t.ds, groups=groups)
            return {"dx2": dx2, "dpos": dpos}
        return i, call
    return build


def _attention_bwd_case(b1, r, c, math, groups):
    def build():
        i = {"q": seeded_randn(120, b1, 49, c), "kv": seeded_randn(121, b1 * r, 49, 2 * c), "do": seeded_randn(122, b1, 49, c)}

        def call(ops, t):
            dq, dkv = ops.deform_attention_bwd(t.q, t.kv, t.do, r, 32 ** -0.5, math=math, groups=groups)
            return {"dq": dq, "dkv": dkv}
        return i, call
    return build


case("deform_sample_bwd/nq2-r3-c192")(_sample_bwd_case(2, 3, 192, 1))               # test_hip_deform_sample_bwd
case("deform_attention_bwd/b1-r5-c96")(_attention_bwd_case(1, 5, 96, "fp32", 1))    # test_hip_deform_attention_bwd
# the four side-view widths (group width C / 3 = 32, 64, 128, 256) at (windows, r) = (2, 3), and per-clip pairing (groups = 2) at
# (4, 3) for the narrowest and the widest: test_hip_deform_{sample,attention}_bwd_side_view_widths hold the values.
# deform_sample_bwd has one arithmetic form; deform_attention_bwd runs both.
for _c in (96, 192, 384, 768):
    for _nq, _g in ((2, 1), (4, 2)) if _c in (96, 768) else ((2, 1),):
        _tag = f"-groups{_g}" if _g > 1 else ""
        if (_nq, _c) != (2, 192):
            case(f"deform_sample_bwd/nq{_nq}-r3-c{_c}{_tag}")(_sample_bwd_case(_nq, 3, _c, _g))
        for _math in ("fp32", "bf16"):
            case(f"deform_attention_bwd/b{_nq}-r3-c{_c}-{_math}{_tag}")(_attention_bwd_case(_nq, 3, _c, _math, _g))


for _n, _c in ((3, 256), (6, 32), (1, 32), (1, 64), (6, 64), (1, 128), (6, 128), (1, 256), (6, 256)):
    # test_hip_dwconv5_window_fwd_bwd; (n, cg) with cg = C / 3 of the four side-view widths at one window and at six
    @case(f"dwconv5_window/{_n}x{_c}")
    def _(n=_n, c=_c):
        i = {"x": seeded_randn(100, n, 49, c), "w": (seeded_randn(101, c, 1, 5, 5) / 5).reshape(c, 25), "b": seeded_randn(102, c)}
        return i, lambda ops, t: {"u": ops.dwconv5_window(t.x, t.w, t.b)}

    @case(f"dwconv5_window_bwd/{_n}x{_c}")
    def _(n=_n, c=_c):
        i = {"x": seeded_randn(100, n, 49, c), "w": (seeded_randn(101, c, 1, 5, 5) / 5).reshape(c, 25), "du": seeded_randn(103, n, 49, c)}

        def call(ops, t):
            dx, dw, db = ops.dwconv5_window_bwd(t.x, t.w, t.du)
            return {"dx": dx, "dw": dw, "db": db}
        return i, call


# --------------------------------------------------------------------------------------------------------------- temporal
for _t in (1, 2, 16):                                                    # test_temporal_attention_lengths: s = 7
    @case(f"temporal_attention/s7-t{_t}")
    def _(tt=_t):
        return {"qkv": seeded_randn(tt, 7, tt, 3 * 768)}, lambda ops, t: {"y": ops.temporal_attention(t.qkv, 7, tt, 768, 12, 64 ** -0.5)}


@case("temporal_attention/s98-t3-tq1+probs+bwd")                         # test_temporal_attention_peaked_rows
def _():
    s, tt, c, heads, scale = 98, 3, 768, 12, 64 ** -0.5
    i = {"qkv": seeded_randn(tt + 1, s, tt, 3 * c), "dout": seeded_randn(70 + tt, s, tt, c)}

    def call(ops, t):
        return {"y_q1": ops.temporal_attention(t.qkv, s, tt, c, heads, scale, tq=1),
                "probs": ops.attention_probs(t.qkv, t.qkv[..., c:], s, heads, tt, tt, c // heads, (tt * 3 * c, 3 * c), (tt * 3 * c, 3 * c), scale),
                "dqkv": ops.temporal_attention_bwd(t.qkv, t.dout, s, tt, c, heads, scale)}
    return i, call


# ----------------------------------------------------------------------------------------------------------- decoder glue
@case("gn_stats+gn_apply/1x256x7x9-g32")                                 # test_groupnorm_act_offset_groups (GN_SHAPES[3])
def _():
    i = {"x": _nhwc(seeded_randn(263, 1, 256, 7, 9) * 1.5), "g": 1 + 0.1 * seeded_randn(1, 256), "b": 0.1 * seeded_randn(2, 256)}

    def call(ops, t):
        xn, partial, nsplit = ops.gn_stats(t.x, 32)
        return {"partial": partial, "y": ops.gn_apply_resample(xn, (partial, nsplit, t.g, t.b, 32, 1e-5), act=1)}
    return i, call


def _tail_inputs():
    return {"x": _nhwc(seeded_randn(5, 2, 128, 28, 28)), "g": seeded_randn(6, 128), "b": seeded_randn(7, 128)}


@case("gn_resample/mean4+EP_ADD_MUL+EP_MUL")                             # test_decoder_tail_fusion
def _():
    i = dict(_tail_inputs(), ea=_nhwc(seeded_randn(8, 2, 128, 56, 56)), eb=_nhwc(seeded_randn(9, 2, 128, 56, 56)))

    def call(ops, t):
        xn, partial, nsplit = ops.gn_stats(t.x, 8)
        gn = (partial, nsplit, t.g, t.b, 8, 1e-5)
        return {"partial": partial, "mean4": ops.gn_apply_resample(xn, gn, act=1, mean4=True, scale=2, align_corners=True),
                "add_mul": ops.gn_apply_resample(xn, gn, act=1, scale=2, align_corners=True, ep_mode=ops.EP_ADD_MUL, ep_a=t.ea, ep_b=t.eb),
                "mul": ops.gn_apply_resample(xn, gn, act=1, scale=2, align_corners=True, ep_mode=ops.EP_MUL, ep_a=t.ea)}
    return i, call


@case("gn_resample/out_coff", partial={"cat": ((slice(None), slice(0, 256)), "the op writes the channel slice [256, 384) of a concatenated map")})
def _():
    def call(ops, t):                                                    # test_decoder_tail_fusion
        cat = ops.empty_nhwc(2, 384, 56, 56, t.x.device)
        ops.gn_apply_resample(t.x, None, scale=2, align_corners=False, out=cat, out_coff=256)
        return {"cat": cat}
    return {"x": _tail_inputs()["x"]}, call


for _scale, _align in ((2, True), (2, False), (4, False)):               # test_bilinear_resample_modes
    @case(f"bilinear/x{_scale}-align{int(_align)}")
    def _(scale=_scale, align=_align):
        return ({"x": _nhwc(seeded_randn(scale, 2, 64, 14, 14))},
                lambda ops, t: {"y": ops.gn_apply_resample(t.x, None, scale=scale, align_corners=align)})


@case("avgpool2_pad/nchw-9->32")                                         # test_decoder_wiring_kernels; channels [9, 32) are zero-filled: written
def _():
    return {"x": seeded_randn(31, 2, 9, 224, 224)}, lambda ops, t: {"y": ops.avgpool2_pad(t.x, 32, nchw_in=True)}


@case("avgpool2_pad/nhwc-128")
def _():
    return {"x": _nhwc(seeded_randn(32, 2, 128, 28, 28))}, lambda ops, t: {"y": ops.avgpool2_pad(t.x)}


@case("set_channels/first-slice", partial={"cat": ((slice(None), slice(256, 320)), "one call fills the slice [0, 256) of the 320 channels")})
def _():
    def call(ops, t):                                                    # test_decoder_wiring_kernels
        cat = ops.empty_nhwc(2, 320, 14, 14, t.a.device)
        ops.set_channels(cat, 0, t.a)
        return {"cat": cat}
    return {"a": _nhwc(seeded_randn(33, 2, 256, 14, 14))}, call


@case("set_channels/both-slices")
def _():
    def call(ops, t):
        cat = ops.empty_nhwc(2, 320, 14, 14, t.a.device)
        ops.set_channels(cat, 0, t.a)
        ops.set_channels(cat, 256, t.bq)                                 # NCHW-contiguous source: normalised to NHWC first
        return {"cat": cat}
    return {"a": _nhwc(seeded_randn(33, 2, 256, 14, 14)), "bq": seeded_randn(34, 2, 64, 14, 14)}, call


@case("copy_rows/strided-slice", partial={"cat": ((slice(None), slice(0, 256)), "set_channels(cat, 256, view) fills channels [256, 2560)")})
def _():
    def call(ops, t):                                                    # the pitched 3-of-T token slice of test_decoder_wiring_kernels
        view = t.g.reshape(3, 49, 5 * 768)[:, :, :2304].reshape(3, 7, 7, 2304).permute(0, 3, 1, 2)
        if not t.g.is_contiguous() or view.data_ptr() != t.g.data_ptr():         # (an error of the caller, not an assert:
            raise RuntimeError("the view must be a pitched alias of a dense g")   # tests/test_ops_handoff.py counts it as a refusal)
        cat = ops.empty_nhwc(3, 256 + 2304, 7, 7, t.g.device)
        ops.set_channels(cat, 256, view)
        return {"cat": cat}
    return {"g": seeded_randn(35, 3 * 49, 5 * 768)}, call


@case("merge_views/2x49-t115")                                           # test_decoder_wiring_kernels
def _():
    i = {"v0": seeded_randn(36, 2, 49, 768), "v1": seeded_randn(37, 2, 49, 768), "v2": seeded_randn(38, 2, 5 * 49, 1024)}
    return i, lambda ops, t: {"y": ops.merge_views([t.v0, t.v1, t.v2], [1, 1, 5])}


@case("trunk_head/2x128x7x7")                                            # test_decoder_wiring_kernels
def _():
    i = {"g": _nhwc(seeded_randn(39, 2, 128, 7, 7)), "f": _nhwc(seeded_randn(40, 2, 128, 7, 7)),
         "gcn": _nhwc(seeded_randn(41, 2, 32, 14, 14)), "fr": _nhwc(seeded_randn(42, 2, 32, 14, 14))}
    return i, lambda ops, t: {"z": ops.trunk_head(t.g, t.f, t.gcn, t.fr)}


for _b, _h, _w in ((2, 13, 11), (1, 1, 1)):                              # test_hip_final_conv_backward (forward + backward)
    def _fc_inputs(b=_b, h=_h, w=_w):
        return {"x": _nhwc(seeded_randn(50, b, 32, h, w)), "w": (seeded_randn(51, 1, 32, 3, 3) / 17.0).permute(0, 2, 3, 1).contiguous(),
                "bias": seeded_randn(52, 1), "dy": seeded_randn(53, b, 1, h, w)}

    for _mask in (False, True):
        @case(f"final_conv/{_b}x{_h}x{_w}{'-mask' if _mask else ''}")
        def _(mask=_mask, inputs=_fc_inputs):
            i = {k: v for k, v in inputs().items() if k != "dy"}

            def call(ops, t):
                if mask:
                    logits, m = ops.final_conv(t.x, t.w, t.bias, with_mask=True)
                    return {"logits": logits, "mask": m}
                return {"logits": ops.final_conv(t.x, t.w, t.bias)}
            return i, call

    @case(f"final_conv_bwd/{_b}x{_h}x{_w}")
    def _(inputs=_fc_inputs):
        i = {k: v for k, v in inputs().items() if k != "bias"}

        def call(ops, t):
            dx, dw, db = ops.final_conv_bwd(t.x, t.w, t.dy)
            return {"dx": dx, "dw": dw, "db": db}
        return i, call


@case("sigmoid_threshold/2x1x224x224")                                   # test_sigmoid_threshold
def _():
    z = seeded_randn(4, 2, 1, 224, 224)
    z[0, 0, 0, :4] = torch.tensor([0.0, 1e-7, -1e-7, 30.0])
    return {"z": z}, lambda ops, t: {"mask": ops.sigmoid_threshold(t.z)}


def _gn_bwd_inputs():
    b, c, h, w = 1, 64, 7, 9                                             # test_hip_groupnorm_relu_bwd / GN_BWD_SHAPES[1]
    return {"z": _nhwc(seeded_randn(30, b, c, h, w) * 2 + 0.3), "g": 1 + 0.1 * seeded_randn(31, c), "b": 0.1 * seeded_randn(32, c),
            "dy": _nhwc(seeded_randn(33, b, c, h, w))}


@case("gn_bwd/1x64x7x9-g8")
def _():
    def call(ops, t):
        z, partial, nsplit = ops.gn_stats(t.z, 8)
        dz, dg, db = ops.gn_bwd(z, (partial, nsplit), t.g, t.b, t.dy, 8, 1e-5, ops.ACT_RELU)
        return {"dz": dz, "dg": dg, "db": db}
    return _gn_bwd_inputs(), call


@case("gn_bwd/1x64x7x9-g8-accumulate", inplace=("gs", "bs"))
def _():
    def call(ops, t):
        z, partial, nsplit = ops.gn_stats(t.z, 8)
        dz, r1, r2 = ops.gn_bwd(z, (partial, nsplit), t.g, t.b, t.dy, 8, 1e-5, ops.ACT_RELU, dg_out=t.gs, db_out=t.bs)
        assert r1 is None and r2 is None
        return {"dz": dz, "gs": t.gs, "bs": t.bs}
    return dict(_gn_bwd_inputs(), gs=seeded_randn(34, 64), bs=seeded_randn(35, 64)), call


for _scale, _align in ((2, False), (2, True), (4, False)):               # test_hip_upsample_bwd_scales
    @case(f"upsample_bwd/x{_scale}-align{int(_align)}")
    def _(scale=_scale, align=_align):
        return ({"dy": _nhwc(seeded_randn(61, 2, 32, 7 * scale, 7 * scale))},
                lambda ops, t: {"dx": ops.upsample_bwd(t.dy, scale, align)})


@case("scale_samples/6x49x32")                                           # test_hip_drop_path_train_mode
def _():
    i = {"x": seeded_randn(40, 6, 49, 32), "scale": torch.tensor([0.0, 1.25, 1.25, 0.0, 1.25, 1.25])}
    return i, lambda ops, t: {"y": ops.scale_samples(t.x, t.scale)}


# ---------------------------------------------------------------------------------------------------------- input staging
@case("normalize_u8/2x3x224x224")                                        # test_normalize_u8_input_staging
def _():
    frames = torch.randint(0, 256, (2, 3, 224, 224, 3), generator=torch.Generator().manual_seed(3), dtype=torch.uint8)
    return {"frames": frames}, lambda ops, t: {"y": ops.normalize_u8(t.frames)}


@case("normalize_u8/resize-100x37")                                      # test_resize_normalize_u8_input_staging
def _():
    frames = torch.randint(0, 256, (2, 3, 100, 37, 3), generator=torch.Generator().manual_seed(137), dtype=torch.uint8)
    return {"frames": frames}, lambda ops, t: {"y": ops.normalize_u8(t.frames, size=(224, 224))}


# -------------------------------------------------------------------------------------------------------------------- FAF
@case("faf/b1-t3-frame1")                                                # test_faf: all nine planes, band-skipped tiles included
def _():
    from models.modules.dct import FAF
    ss = [int(v) for v in np.load(os.path.join(GOLDEN, "ops.npz"))["faf/x/seed_shape"]]
    faf = FAF()
    i = {"x": seeded_randn(ss[0], *ss[1:]), "d": faf._host[0], "dt": faf._host[1]}
    return i, lambda ops, t: {"y": ops.faf(t.x, t.d, t.dt, 1, faf.lo_hi, faf.mid_lo, faf.mid_hi)}


# ---------------------------------------------------------------------------------------------------------- small helpers
@case("gelu+gelu_bwd/4096")                                              # test_hip_gelu_fwd_bwd
def _():
    i = {"x": seeded_randn(5, 4096) * 3, "dy": seeded_randn(6, 4096)}
    return i, lambda ops, t: {"y": ops.gelu(t.x), "dx": ops.gelu_bwd(t.x, t.dy)}


for _r, _c in ((1, 7), (1000, 333)):                                     # test_hip_transpose_and_col_sum
    @case(f"transpose+col_sum/{_r}x{_c}")
    def _(r=_r, c=_c):                                                    # pad columns [R, Rp) of the padded form are zero-filled: written
        return {"x": seeded_randn(7, r, c)}, lambda ops, t: {"t": ops.transpose(t.x), "t32": ops.transpose(t.x, 32), "sum": ops.col_sum(t.x)}


@case("patch_gather/1x2x2x4-both-ways")                                  # test_hip_patch_gather_both_ways
def _():
    i = {"x": seeded_randn(43, 1, 4, 4), "m": seeded_randn(44, 1, 1, 16)}
    return i, lambda ops, t: {"fwd": ops.patch_gather(t.x, 1, 2, 2, 4), "inv": ops.patch_gather(t.m, 1, 2, 2, 4, inverse=True)}


@case("add/7x196x96")                                                    # test_add
def _():
    return {"a": seeded_randn(1, 7, 196, 96), "b": seeded_randn(2, 7, 196, 96)}, lambda ops, t: {"y": ops.add(t.a, t.b)}


for _nh in (3, 24):                                                      # test_relpos_bias_expand
    @case(f"expand_relpos_bias/nh{_nh}")
    def _(nh=_nh):
        from models.modules.swinTransformer import relative_position_index
        from mumpy_hip import ops as _ops
        i = {"table": seeded_randn(900 + nh, 169, nh), "idx": _ops.rel_index32(relative_position_index(7, 7))}
        return i, lambda ops, t: {"bias": ops.expand_relpos_bias(t.table, t.idx)}


# ---------------------------------------------------------------------------------------------------------- training tail
for _grad in (True, False):                                              # test_hip_mask_loss_extremes (+ need_grad=False as in test_hip_mask_loss_matches_reference)
    @case(f"mask_loss/2x1x32x32-{'grad' if _grad else 'loss-only'}")
    def _(grad=_grad):
        target = torch.zeros(2, 1, 1024)
        target[1, 0, :100] = 1.0

        def call(ops, t):
            loss3, dz = ops.mask_loss(t.z, t.target, need_grad=grad)
            return {"loss3": loss3, "dz": dz} if grad else {"loss3": loss3}
        return {"z": seeded_randn(9, 2, 1, 32, 32) * 40.0, "target": target}, call

for _n in (1, 3, 1023):          # test_hip_adamw_matches_torch / test_hip_sgd_matches_torch / test_hip_rmsprop_matches_torch: two steps each
    @case(f"adamw_step/n{_n}", inplace=("p", "m", "v"))
    def _(n=_n):
        def call(ops, t):
            for step in (1, 2):
                ops.adamw_step(t.p, t.g, t.m, t.v, step, lr=3e-3, weight_decay=1e-2, grad_scale=0.5)
            return {"p": t.p, "m": t.m, "v": t.v}
        return {"p": seeded_randn(21, n), "g": seeded_randn(101, n), "m": torch.zeros(n), "v": torch.zeros(n)}, call

    for _mom, _nes in ((0.0, False), (0.9, False), (0.9, True)):
        @case(f"sgd_step/n{_n}-momentum{_mom}{'-nesterov' if _nes else ''}", inplace=("p", "buf") if _mom else ("p",))
        def _(n=_n, mom=_mom, nes=_nes):
            i = {"p": seeded_randn(21, n), "g": seeded_randn(101, n)}
            if mom:
                i["buf"] = torch.zeros(n)

            def call(ops, t):
                for _ in (1, 2):
                    ops.sgd_step(t.p, t.g, t.get("buf"), lr=3e-2, momentum=mom, weight_decay=1e-2, nesterov=nes, grad_scale=0.5)
                return {k: t[k] for k in ("p", "buf") if k in t}
            return i, call

    for _mom in (0.0, 0.9):
        @case(f"rmsprop_step/n{_n}-momentum{_mom}", inplace=("p", "sq", "buf") if _mom else ("p", "sq"))
        def _(n=_n, mom=_mom):
            i = {"p": seeded_randn(22, n), "g": seeded_randn(201, n), "sq": torch.zeros(n)}
            if mom:
                i["buf"] = torch.zeros(n)

            def call(ops, t):
                for _ in (1, 2):
                    ops.rmsprop_step(t.p, t.g, t.sq, t.get("buf"), lr=3e-3, momentum=mom, weight_decay=1e-2, grad_scale=0.5)
                return {k: t[k] for k in ("p", "sq", "buf") if k in t}
            return i, call


# ================================================================================================ GPU: the one test
# results that a tensor method allocated, not the proxy: compared bitwise, invisible to check (b) (see the docstring)
UNGUARDED_RESULTS = {c.id: {"dpos"} for c in CASES if c.id.startswith("deform_sample_bwd/")}
_HIP_ERROR = []          # the first case whose run raised inside the library: nothing more is launched in this process after it


def test_case_ids_are_unique_and_partials_carry_a_reason():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    for c in CASES:
        for name, (index, reason) in c.partial.items():
            assert isinstance(reason, str) and len(reason) > 10, (c.id, name)


def _outside(mask_shape, index):
    keep = torch.ones(mask_shape, dtype=torch.bool)
    keep[index] = False
    return keep


@gpu
@pytest.mark.parametrize("case_", CASES, ids=[c.id for c in CASES])
def test_memory_discipline(case_, monkeypatch):
    if _HIP_ERROR:
        pytest.fail(f"not run: the case {_HIP_ERROR[0]} hit an error inside a launch earlier in this process")
    from mumpy_hip import autograd, ops
    dev = torch.device("cuda:0")
    inputs, call = case_.build()
    assert set(case_.inplace) <= set(inputs)
    try:
        plain = call(ops, _T({k: v.to(dev) for k, v in inputs.items()}))              # 1. unguarded
        torch.cuda.synchronize()
        plain = {k: v.cpu() for k, v in plain.items()}

        def body(guard):                                                              # 2. + 3. under the guard, both patterns
            t = _T({k: guard.tensor(v) for k, v in inputs.items()})
            return call(ops, t), [t[k] for k in case_.inplace], case_.partial
        runs, unguarded = GA.run_both(monkeypatch, [ops, autograd], body, device=dev, sync=torch.cuda.synchronize)
    except RuntimeError as e:
        if any(s in str(e) for s in ("HIP", "hip", "rc=")):                           # a launch failed: the usual rule, stop here
            _HIP_ERROR.append(case_.id)
        raise
    assert unguarded == UNGUARDED_RESULTS.get(case_.id, set())                        # every other output was seen by check (b)
    assert len(runs) == len(GA.PASSES)
    for pattern, outs in zip(GA.PASSES, runs):                                        # placement independence, bit for bit
        assert set(outs) == set(plain)
        for name, out in outs.items():
            got, want = GA._bytes(out.cpu()), GA._bytes(plain[name])
            if name in case_.partial:
                keep = _outside(out.shape, case_.partial[name][0])
                got, want = got[keep], want[keep]
            assert got.shape == want.shape
            diff = (got != want).any(-1)
            assert not bool(diff.any()), (f"{name}: {int(diff.sum())} of {diff.numel()} elements differ from the unguarded run under "
                                          f"{GA.pass_name(pattern)}; first at {diff.nonzero()[0].tolist()}")


# ================================================================================================ GPU: the whole model
# (id, training tape?, batch, switches).  T = 3 throughout: the smallest clip that launches every kernel of its mode.
ModelConfig = namedtuple("ModelConfig", "id train batch storage attn cva mlp coupling")
MODEL_CONFIGS = [
    ModelConfig("eval-fp32-b1", False, 1, "fp32", "fp32", "fp32", False, "batch"),
    ModelConfig("eval-bf16-storage-b1", False, 1, "bf16", "bf16", "bf16", False, "batch"),
    ModelConfig("train-fp32-b1", True, 1, "fp32", "fp32", "fp32", False, "batch"),
    ModelConfig("train-bf16-attention-fused-mlp-clip-b2", True, 2, "fp32", "bf16", "bf16", True, "clip"),
]
MODEL_T = 3
MODEL_MODULES = ("mumpy_hip.ops", "mumpy_hip.autograd", "models.modules.swinTransformer", "models.modules.blocks",
                 "models.encoder.multiTemporalViewEncoder")


@functools.lru_cache(maxsize=None)
def _three_view_model():
    """Encoder and Decoder as tests/test_swin_backward._hip_full_backward builds them, once for the four configurations."""
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    enc = fill_module_(Encoder(num_frames=MODEL_T)).eval().cuda()
    dec = fill_module_(Decoder(input_token_temporal_dims=[1, 1, MODEL_T])).eval().cuda()
    return enc, dec


@contextlib.contextmanager
def _model_switches(cfg):
    """The process-wide switches of one configuration; every one of them is put back on the way out, also on failure."""
    from mumpy_hip import ops
    before = (ops.storage(), ops.matrix_math(), ops.attention_math(), ops.cva_math(), ops.mlp_fusion(), ops.clip_coupling())
    try:
        ops.set_storage(cfg.storage)
        ops.set_attention_math(cfg.attn)
        ops.set_cva_math(cfg.cva)
        ops.set_mlp_fusion(cfg.mlp)
        ops.set_clip_coupling(cfg.coupling)
        yield
    finally:
        ops.set_storage(before[0])
        ops.set_matrix_math(before[1])
        ops.set_attention_math(before[2])
        ops.set_cva_math(before[3])
        ops.set_mlp_fusion(before[4])
        ops.set_clip_coupling(before[5])


def _scalars(args):
    """The scalar arguments of a launch: everything that is not an address (tensor, workspace and stream handles are 64-bit values)."""
    return tuple(a for a in args if isinstance(a, float) or (isinstance(a, int) and abs(a) < 1 << 32))


def _watching_call(real_call, launches, first, guard=None, watch=None, sync=lambda: None):
    """ops._call, counted in launches[0].  With watch (indices of guarded blocks): after every launch the device is synchronised and
    the bands of those blocks -- the ones that exist by then; allocation order is deterministic, so the indices of an earlier run
    carry over -- are looked at, until one has changed: first[0] = (entry point, its scalar arguments, band_hits)."""
    def call(name, *args, work=0.0):
        real_call(name, *args, work=work)
        launches[0] += 1
        if watch and not first:
            sync()
            hits = guard.band_hits(only=[i for i in watch if i < len(guard.log)])
            if hits:
                first.append((name, _scalars(args), hits))
    return call


def test_the_watching_call_names_the_first_launch_that_damaged_a_band():
    """CPU: the report path of test_whole_model_under_the_guard, on a fake launch that writes past its output on its third call."""
    guard, launches, first, bufs = GA.Guard(GA.CYCLE), [0], [], []

    def fake_launch(name, address, n, scale, table, stream, work=0.0):
        out = guard.torch.empty(n, dtype=torch.float32)
        bufs.append(out)
        out.fill_(scale)
        if len(bufs) == 3:
            out.as_strided((1,), (1,), out.storage_offset() + n).fill_(scale)         # one element too far
    call = _watching_call(fake_launch, launches, first, guard, watch=[2, 3])
    for i in range(5):
        call(f"entry{i}", 0x7F0000001000 + i, 4 + i, 0.5, None, 0x55550000AAAA, work=1.0)
    assert launches == [5] and len(guard.log) == 5
    assert first == [("entry2", (6, 0.5), [(2, "fake_launch", (6,), 0, 4)])]                # addresses and handles are left out
    quiet = []
    call = _watching_call(lambda name, *a, work=0.0: None, launches, quiet, guard, watch=[0, 1])
    call("entry5", 1, 2)
    assert quiet == [] and launches == [6]                                                   # undamaged blocks report nothing


def _model_run(monkeypatch, cfg, x, target, guard=None, watch=None):
    """One forward (and backward) of the configuration -> ({"logits": ..., "grad/<name>": ...} as copies, launches, first damaging
    launch or None).  guard: run with its proxy installed in MODEL_MODULES, x and target in guarded blocks.  watch: indices of
    guarded blocks; after every launch the device is synchronised and their bands are looked at, and the first launch after which
    one changed is returned as (entry point, scalar arguments, band_hits)."""
    import importlib
    from mumpy_hip import ops, state
    from mumpy_hip.autograd import decoder_train, encoder_train
    enc, dec = _three_view_model()
    params = [(f"{which}.{n}", p) for which, mod in (("enc", enc), ("dec", dec)) for n, p in mod.named_parameters()]
    for _, p in params:
        p.grad = None
    state.bump_weights_epoch()                                           # derived weights are rebuilt inside this run's allocations
    launches, first = [0], []
    counting_call = _watching_call(ops._call, launches, first, guard, watch, torch.cuda.synchronize)

    def run(xd, td):
        if cfg.train:
            fx, vx, dx = encoder_train(enc, xd, coupling="clip" if cfg.coupling == "clip" else None)
            lg, _ = decoder_train(dec, fx, vx, dx)
            lg.backward(ops.mask_loss(lg.detach(), td)[1])
        else:
            with torch.no_grad():
                lg, _ = dec(*enc(xd))
        torch.cuda.synchronize()                                         # side streams included
        out = {"logits": lg.detach().clone()}                            # copies outside the guard, compared on the device
        if cfg.train:
            assert all(p.grad is not None for _, p in params)
            out.update({f"grad/{n}": p.grad.detach().clone() for n, p in params})
        return out
    try:
        with monkeypatch.context() as m, _model_switches(cfg):
            m.setattr(ops, "_call", counting_call)
            if guard is None:
                out = run(x.cuda(), target.cuda())
            else:
                with guard.installed(monkeypatch, *(importlib.import_module(n) for n in MODEL_MODULES)):
                    out = run(guard.tensor(x), guard.tensor(target))
    finally:
        for _, p in params:
            p.grad = None
        state.bump_weights_epoch()                                       # nothing derived inside a guard outlives it in use
    return out, launches[0], first[0] if first else None


def _first_difference(a, b):
    assert list(a) == list(b)
    return next((n for n in a if not GA.same_bits(a[n], b[n])), None)


MODEL_COUNTS = {}        # id -> (launches, [guarded blocks per pass]); printed by the test, quoted in the module docstring


@gpu
@pytest.mark.parametrize("cfg", MODEL_CONFIGS, ids=[c.id for c in MODEL_CONFIGS])
def test_whole_model_under_the_guard(cfg, monkeypatch):
    """The three-view model's own forward and training tape, every allocation of MODEL_MODULES in a guarded block: after each of the
    three passes every band of every block is intact (kept GEMM workspaces and side-stream allocations included; the device is
    synchronised first), the clip and the target are unchanged, and the logits -- on the tape also every parameter gradient -- are
    bitwise those of the unguarded run.  Precondition: two unguarded runs are bitwise equal.  Check (b) is not applied:
    intermediates are not outputs.  On a band failure the configuration runs once more with the damaged blocks watched after every
    launch, and the failure names the first entry point after which a band changed."""
    if _HIP_ERROR:
        pytest.fail(f"not run: the case {_HIP_ERROR[0]} hit an error inside a launch earlier in this process")
    dev = torch.device("cuda:0")
    x = seeded_randn(990, cfg.batch, MODEL_T, 3, 224, 224)
    target = (torch.rand(cfg.batch, 1, 224, 224, generator=torch.Generator().manual_seed(7)) < 0.1).float()
    try:
        plain, launches, _ = _model_run(monkeypatch, cfg, x, target)
        again, launches2, _ = _model_run(monkeypatch, cfg, x, target)
        assert launches == launches2 and _first_difference(plain, again) is None, \
            f"two unguarded runs differ; first at {_first_difference(plain, again)}"
        blocks = []
        for pattern in GA.PASSES:
            guard = GA.Guard(pattern, dev)
            out, n, _ = _model_run(monkeypatch, cfg, x, target, guard=guard)
            blocks.append(len(guard.log))
            hits = guard.band_hits()
            if hits:
                _, _, first = _model_run(monkeypatch, cfg, x, target, guard=GA.Guard(pattern, dev), watch=[h[0] for h in hits])
                pytest.fail(f"guard band overwritten ({GA.pass_name(pattern)}): [(block, site, shape, bytes in front, bytes behind)] = "
                            f"{hits[:8]}{' ...' if len(hits) > 8 else ''}; first launch after which one of them changed: {first}")
            guard.check({})                                              # (a) again, and (c): the clip and the target are unchanged
            assert n == launches, f"{n} launches under the guard, {launches} without"
            differs = _first_difference(plain, out)
            assert differs is None, f"{differs} differs from the unguarded run under {GA.pass_name(pattern)}"
            del guard, out
    except RuntimeError as e:
        if any(s in str(e) for s in ("HIP", "hip", "rc=")):
            _HIP_ERROR.append(f"whole model/{cfg.id}")
        raise
    MODEL_COUNTS[cfg.id] = (launches, blocks)
    print(f"whole model {cfg.id}: {launches} launches, guarded blocks per pass {blocks}, {len(plain)} tensors compared")
