"""Guard-banded allocations for the memory-discipline tests (tests/test_memory_discipline.py).

A `Guard` owns a proxy that stands in for the name `torch` INSIDE the project's modules only (`Guard.installed` swaps the
module attribute with monkeypatch; the global torch module is never patched).  The proxy forwards every attribute to the real
torch except `empty`, `empty_like` and `zeros`: each of those allocates one uint8 block of BAND + nbytes (rounded up to 16) + BAND
bytes filled with a byte pattern and returns the interior as an as_strided view with the shape, strides and dtype the real call
would have produced (taken from a device="meta" twin, so memory_format=torch.channels_last and empty_like of a permuted view keep
their strides).  BAND is a multiple of 256, so the interior keeps the 16-byte alignment the kernels require.  Every allocation
is logged as (raw block, interior byte range, view).

Two fill patterns: 0xFF bytes read as NaN in fp32 and in bf16 -- a kernel that READS an element nothing wrote carries the NaN
into its result, where the value checks see it -- and 0x7F bytes read as 3.39e38.  An element counts as unwritten if and only
if it holds pattern A after a run under pattern A AND pattern B after a second run under pattern B: that separates "never stored"
from "legitimately stored that bit pattern".

A third pass fills every block with a byte of its own, cycling through CYCLE = 0x3B .. 0x3F (fp32 and bf16 readings 0.0029 .. 0.747,
ordinary finite magnitudes); consecutive allocations -- tensor() blocks included -- never share a byte, each block's byte is kept
in Alloc.fill and band_hits() compares every band with its own block's byte.  What it is for: patterns A and B both ABSORB an
addition (NaN + x is the same NaN, 3.39e38 + O(1) rounds back to 3.39e38), so a stray store whose value was computed from a stray
load -- one wrong bound shared by the load and the store of a reduce, an epilogue or a copy -- writes the band's own pattern into
the neighbouring band and leaves nothing to find.  Under per-block bytes a value loaded from one block's band and stored into
another block's band, summed, scaled or copied verbatim, does not reproduce the target's byte.  The third pass decides nothing
about check (b); it asserts (a) and (c), and the callers compare its outputs bitwise like those of the other two.  `run_both`
does the three runs.

Every allocation carries its site: module.function of the innermost frame on the stack whose module has the proxy installed
(tensor() blocks are tagged "Guard.tensor").  Failure messages print it with the block's index in the log and its shape.

`Guard.check(outputs, inplace, partial)` asserts
  (a) every band of every logged block is intact (outputs, scratch buffers and the kept GEMM workspaces alike);
  (b) every element of every output is written, except a declared `partial` region, which must still hold the pattern;
  (c) every tensor placed with `Guard.tensor` and not named in `inplace` is bitwise unchanged.

Limits, stated rather than measured: BAND = 4096 bytes on each side.  The harness sees near misses within 4 KB of a buffer --
one row, one tile too far -- now also when the stored value came from a stray load in ANOTHER block's band.  It does not see:
wild writes beyond the band; out-of-bounds READS that reach no result (one that does reach a result changes that result between
the passes, which the callers' bitwise comparisons see); a stray store whose value was loaded from the band of the SAME block it
lands in (a copy within one block's bands reproduces the byte); and, with five bytes in the cycle, a verbatim copy between the
bands of two blocks allocated a multiple of five apart.
Allocations the proxy cannot see pass through unguarded: Tensor.new_zeros (autograd.py, the channel padding of the generic final
convolution's backward), torch.full (ops.compact_attn_mask, a host-side table) and whatever tensor METHODS allocate
(.contiguous(), .to(), .sum(), ...)."""
import contextlib
import sys
from collections import namedtuple

import torch as _torch

BAND = 4096                          # bytes on each side of every block; a multiple of 256
PATTERN_A, PATTERN_B = 0xFF, 0x7F    # NaN in fp32 / bf16; 3.39e38
PATTERNS = (PATTERN_A, PATTERN_B)     # the two that decide "unwritten"
CYCLE = (0x3B, 0x3C, 0x3D, 0x3E, 0x3F)   # the third pass: one byte per block, fp32 / bf16 readings 0.0029 .. 0.747 (nothing absorbs an addition)
PASSES = (PATTERN_A, PATTERN_B, CYCLE)   # what run_both runs, in this order

# interior = raw[lo:hi]; raw[:lo] and raw[hi:] are the bands; fill = the byte of this block; site = who allocated it
Alloc = namedtuple("Alloc", "raw lo hi view fill site")


def pass_name(pattern):
    return f"pattern {pattern:#x}" if isinstance(pattern, int) else f"per-block bytes {pattern[0]:#x}..{pattern[-1]:#x}"


def _extent(size, stride):
    """Elements spanned by a strided tensor (0 when it has no elements)."""
    if any(s == 0 for s in size):
        return 0
    return 1 + sum((s - 1) * st for s, st in zip(size, stride))


def _bytes(t):
    """The elements of t as bytes, logical shape + (itemsize,)."""
    c = t.detach().contiguous().reshape(-1)          # (flattened first: a "contiguous" tensor with size-1 dims may carry any strides there)
    return c.view(_torch.uint8).reshape(*t.shape, c.element_size())


def same_bits(a, b):
    """Bitwise equality (torch.equal calls NaN != NaN and -0.0 == 0.0)."""
    return a.shape == b.shape and a.dtype == b.dtype and bool(_torch.equal(_bytes(a), _bytes(b)))


class _TorchProxy:
    """Forwards to the real torch; empty / empty_like / zeros go through the guard."""

    def __init__(self, guard):
        self.__dict__["_guard"] = guard

    def __getattr__(self, name):
        return getattr(_torch, name)

    def __setattr__(self, name, value):
        raise AttributeError("the torch proxy is read-only")

    def empty(self, *args, **kw):
        return self._guard._like_meta(_torch.empty(*args, **{**kw, "device": "meta"}), kw.get("device"))

    def empty_like(self, t, **kw):
        return self._guard._like_meta(_torch.empty_like(t, **{**kw, "device": "meta"}), kw.get("device", t.device))

    def zeros(self, *args, **kw):
        out = self._guard._like_meta(_torch.empty(*args, **{**kw, "device": "meta"}), kw.get("device"))
        out.zero_()
        return out


class Guard:
    def __init__(self, pattern, device="cpu"):
        """pattern: one byte for every block (PATTERN_A, PATTERN_B), or a tuple of bytes to cycle through block by block (CYCLE)."""
        self.cycle = None if isinstance(pattern, int) else tuple(pattern)
        assert BAND % 256 == 0 and all(0 <= p < 256 for p in (self.cycle or (pattern,)))
        assert self.cycle is None or len(set(self.cycle)) == len(self.cycle) >= 2           # consecutive blocks never share a byte
        self._pattern, self.device = pattern, _torch.device(device)
        self.log = []                # every allocation made through the proxy or through tensor()
        self.placed = []             # (view, snapshot of its interior bytes) of tensor()
        self.unwritten = None        # after check(): one boolean mask per output (element still holds the pattern)
        self.unguarded = None        # after check(): names of the outputs that live in no logged block (check (b) cannot see them)
        self.torch = _TorchProxy(self)

    @property
    def pattern(self):
        """The byte the NEXT allocation is filled with (the same for every block under patterns A and B)."""
        return self._pattern if self.cycle is None else self.cycle[len(self.log) % len(self.cycle)]

    @property
    def name(self):
        return pass_name(self._pattern)

    # ---------------------------------------------------------------- allocation
    def _site(self):
        """module.function of the innermost frame whose module has this guard's proxy as its `torch`; without one (the fake modules
        of the CPU tests) the function that called into this file."""
        f, caller = sys._getframe(1), None
        while f is not None:
            g = f.f_globals
            if g.get("torch") is self.torch:
                return f"{str(g.get('__name__', '?')).rsplit('.', 1)[-1]}.{f.f_code.co_name}"
            if caller is None and g.get("__name__") != __name__:
                caller = f.f_code.co_name
            f = f.f_back
        return caller or "?"

    def _alloc(self, size, stride, dtype, device, site=None):
        item = _torch.empty((), dtype=dtype, device="meta").element_size()
        nbytes = _extent(size, stride) * item
        fill = self.pattern
        raw = _torch.full((BAND + (nbytes + 15) // 16 * 16 + BAND,), fill, dtype=_torch.uint8, device=device)
        view = raw[BAND:BAND + nbytes].view(dtype).as_strided(tuple(size), tuple(stride))
        self.log.append(Alloc(raw, BAND, BAND + nbytes, view, fill, site or self._site()))
        return view

    def _like_meta(self, meta, device):
        return self._alloc(meta.shape, meta.stride(), meta.dtype, _torch.device("cpu" if device is None else device))

    def tensor(self, t):
        """A copy of the (CPU) tensor t in a guarded block on the guard's device, with t's strides when t is dense (channels_last and
        permuted tensors keep their layout), and a bitwise snapshot for check (c)."""
        t = t.detach()
        if _extent(t.shape, t.stride()) != t.numel():
            t = t.contiguous()
        view = self._alloc(t.shape, t.stride(), t.dtype, self.device, site="Guard.tensor")
        view.copy_(t)
        a = self.log[-1]
        self.placed.append((view, a.raw[a.lo:a.hi].clone()))
        return view

    @contextlib.contextmanager
    def installed(self, monkeypatch, *modules):
        """The proxy as the name `torch` of each module, for the duration of the block.  A module that keeps GEMM workspaces
        (mumpy_hip.ops) gets empty registries meanwhile, so that the workspaces are reallocated inside the guard and no guarded view
        outlives the block."""
        with monkeypatch.context() as m:
            for mod in modules:
                m.setattr(mod, "torch", self.torch)
                if hasattr(mod, "_KEPT_WS"):
                    mod.reset_workspaces()
                    m.setattr(mod, "_KEPT_WS", {})
                    m.setattr(mod, "_RETIRED_WS", [])
            yield self
        for mod in modules:
            if hasattr(mod, "_KEPT_WS"):
                mod.reset_workspaces()

    # ---------------------------------------------------------------- checks
    def _block_of(self, t):
        p = t.data_ptr()
        for a in self.log:
            base = a.raw.data_ptr()
            if a.raw.device == t.device and base + a.lo <= p < base + max(a.hi, a.lo + 1):
                return a
        return None

    def band_hits(self, only=None):
        """[(index in the log, site, shape of the view, bytes changed in front, bytes changed behind)] of the blocks whose bands no
        longer hold their block's byte; only: the indices to look at (default: every block)."""
        which = range(len(self.log)) if only is None else sorted(only)
        if not which:
            return []
        counts = [_torch.stack([(a.raw[:a.lo] != a.fill).sum(), (a.raw[a.hi:] != a.fill).sum()]) for a in (self.log[i] for i in which)]
        by_device = {}
        for i, c in zip(which, counts):                      # one transfer per device
            by_device.setdefault(c.device, []).append((i, c))
        hits = []
        for pairs in by_device.values():
            for (i, _), (f, b) in zip(pairs, _torch.stack([c for _, c in pairs]).tolist()):
                if f or b:
                    hits.append((i, self.log[i].site, tuple(self.log[i].view.shape), int(f), int(b)))
        return sorted(hits)

    def check(self, outputs, inplace=(), partial=None, prior=None):
        """outputs: {name: tensor}.  inplace: tensors from tensor() that the op may modify.  partial: {name: (index, reason)} -- the
        region `output[index]` (logical indexing) must NOT be written.  prior: the Guard of the run under the other pattern; with it
        check (b) is decided (an element must hold the pattern in both runs to count as unwritten), without it the candidates are only
        recorded in self.unwritten.  A guard with per-block bytes asserts (a) and (c) only: patterns A and B decide (b)."""
        partial = partial or {}
        assert set(partial) <= set(outputs), "partial names an output that does not exist"
        hits = self.band_hits()                                                                       # (a)
        assert not hits, f"guard band overwritten ({self.name}): [(block, site, shape, bytes in front, bytes behind)] = {hits}"
        self.unwritten, self.unguarded = {}, set()
        for name, out in outputs.items() if self.cycle is None else ():                               # (b)
            holds = (_bytes(out) == self._pattern).all(-1)
            if self._block_of(out) is None:
                assert name not in partial, f"{name}: a partial region needs an output that lives in a guarded block"
                holds = _torch.zeros_like(holds)             # not allocated through the proxy: nothing to say about it
                self.unguarded.add(name)
            if name in partial:
                index = partial[name][0]
                region = _torch.zeros_like(holds)
                region[index] = True
                assert bool(holds[region].all()), (f"{name}: declared-untouched region {index} was written "
                                                   f"({int((~holds[region]).sum())} elements; {self.name})")
                holds = holds & ~region
            self.unwritten[name] = holds.cpu()
        if prior is not None:
            assert self.cycle is None and prior.cycle is None
            assert prior.unwritten is not None and prior.pattern != self.pattern and set(prior.unwritten) == set(self.unwritten)
            for name, holds in self.unwritten.items():
                never = holds & prior.unwritten[name]
                if bool(never.any()):
                    where = never.nonzero()
                    raise AssertionError(f"{name}: {int(never.sum())} of {never.numel()} elements never written "
                                         f"(they hold the fill pattern under both patterns); first at {where[0].tolist()}, "
                                         f"last at {where[-1].tolist()}")
        skip = {t.data_ptr() for t in inplace}                                                        # (c)
        for i, (view, snap) in enumerate(self.placed):
            if view.data_ptr() in skip and view.numel():
                continue
            a = self._block_of(view) if view.numel() else None
            if a is not None:
                assert bool(_torch.equal(a.raw[a.lo:a.hi], snap)), f"input {i} {tuple(view.shape)} {view.dtype} was modified ({self.name})"


def run_both(monkeypatch, modules, body, device="cpu", sync=None):
    """body(guard) -> (outputs, inplace, partial), run once per entry of PASSES with the proxy installed in `modules`: patterns A and
    B assert (a), (b) and (c), the per-block pass (a) and (c).  Returns the output dicts of all passes, in the order of PASSES (for
    the caller's bitwise comparison with the unguarded run), and the names of the outputs check (b) could not see."""
    results, prior = [], None
    for pattern in PASSES:
        guard = Guard(pattern, device)
        with guard.installed(monkeypatch, *modules):
            outputs, inplace, partial = body(guard)
            if sync is not None:
                sync()
            guard.check(outputs, inplace, partial, prior=prior if guard.cycle is None else None)
        results.append(outputs)
        if guard.cycle is None:
            prior = guard
    return results, prior.unguarded
