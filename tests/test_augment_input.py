"""GPU: the training input stage (ops.augment_stage_u8 / mumpy_augment_stage_u8_fwd, mumpy_hip.augment.AugmentedInput).

The kernel is a gather through per-clip index tables followed by the arithmetic of normalize_u8_kernel, so its reference is code that
exists without it: the uint8 frames gathered on the CPU through the same tables (mumpy_hip.augment.gather, itself pinned against
Pillow and against the reference's recorded outputs in tests/test_augment_host.py), then ops.normalize_u8 -- equal BIT FOR BIT -- and
oracle.stage_frames of the gathered frames at the bar of test_resize_normalize_u8_input_staging (rel_err < 1e-6, no element off by
more than 1e-5).  Targets are exact 0/1 values.  Shapes: L = 28 (one block per few rows, several clips per block) and 224 (the
model's), sources 37 x 50 (ragged, smaller and larger than L) and 240 x 432 (config 4's footage), L = 4 from a 1 x 3 source as the
smallest case the entry accepts."""
import numpy as np
import pytest
import torch

import guarded_alloc as GA
from conftest import rel_err
from oracle import mumpy_oracle as O

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")


def _mods():
    from mumpy_hip import augment, ops
    return augment, ops


def _boxed(L):
    return (L // 4, L // 7, L - L // 5, L - L // 3)


def _dev_params(params):
    ta, tb, sw = (np.stack([np.asarray(p[k]) for p in params]) for k in range(3))
    return (torch.from_numpy(ta.astype(np.int32)).to(DEV), torch.from_numpy(tb.astype(np.int32)).to(DEV),
            torch.from_numpy(sw.astype(np.int32)).to(DEV))


def _host_gather(frames, params):
    """frames (nclips, T, Hs, Ws, 3) uint8 numpy -> (nclips, T, L, L, 3): each clip through its own tables."""
    A, _ = _mods()
    return np.stack([A.gather(frames[c], *params[c], channels_last=True) for c in range(frames.shape[0])])


def _check_frames(out, frames, params):
    _, ops = _mods()
    moved = torch.from_numpy(np.ascontiguousarray(_host_gather(frames, params)))
    want = ops.normalize_u8(moved.to(DEV)).cpu()
    got = out.cpu()
    assert got.shape == want.shape
    assert GA.same_bits(got, want), f"{int((got != want).sum())} of {got.numel()} elements differ from gather + normalize_u8"
    ref = O.stage_frames(moved)
    assert rel_err(got, ref) < 1e-6
    assert int(((got - ref).abs() > 1e-5).sum()) == 0


@pytest.mark.parametrize("L", [28, 224])
@pytest.mark.parametrize("src", [(37, 50), (240, 432)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_augment_stage_is_gather_plus_normalize_bit_for_bit(src, L):
    """Every operation x {no box, one box}, three clips with different parameters per launch, T = 2."""
    A, ops = _mods()
    hs, ws = src
    combos = [(op, box) for op in A.OPS for box in (None, _boxed(L))]
    assert len(combos) == 16
    g = np.random.default_rng(hs * 1000 + L)
    frames = g.integers(0, 256, (3, 2, hs, ws, 3), dtype=np.uint8)
    fd = torch.from_numpy(frames).to(DEV)
    for k in range(0, 18, 3):                                    # 6 launches of 3 clips: each of the 16 combinations at least once
        params = [A.clip_tables(src, L, *combos[(k + c) % 16]) for c in range(3)]
        out = ops.augment_stage_u8(fd, *_dev_params(params))
        assert out.shape == (3, 2, 3, L, L) and out.dtype == torch.float32
        _check_frames(out, frames, params)


def test_augment_stage_smallest_shape():
    A, ops = _mods()
    frames = np.random.default_rng(1).integers(0, 256, (3, 2, 1, 3, 3), dtype=np.uint8)
    params = [A.clip_tables((1, 3), 4, op, box) for op, box in (("rot90", None), ("hflip", (1, 0, 4, 3)), ("rot270+tb", (0, 1, 2, 2)))]
    _check_frames(ops.augment_stage_u8(torch.from_numpy(frames).to(DEV), *_dev_params(params)), frames, params)


def test_targets_are_the_gathered_masks():
    """nmasks = 2, nclips = 6: clip c reads mask c % 2; mask values {0, 1, 37, 255} all above 0 count as 1."""
    A, ops = _mods()
    hs, ws, L = 37, 50, 28
    g = np.random.default_rng(7)
    frames = g.integers(0, 256, (6, 2, hs, ws, 3), dtype=np.uint8)
    masks = g.choice(np.array([0, 1, 37, 255], np.uint8), (2, hs, ws))
    combos = [("id", None), ("rot90", _boxed(L)), ("vflip", None), ("rot270", None), ("hflip", _boxed(L)), ("rot90+tb", (0, 3, 9, 28))]
    params = [A.clip_tables((hs, ws), L, op, box) for op, box in combos]
    fd, md, (ta, tb, sw) = torch.from_numpy(frames).to(DEV), torch.from_numpy(masks).to(DEV), _dev_params(params)
    out, target = ops.augment_stage_u8(fd, ta, tb, sw, masks=md)
    want = np.stack([(A.gather(masks[c % 2], *params[c]) > 0).astype(np.float32).reshape(-1) for c in range(6)])
    assert target.shape == (6, L * L) and GA.same_bits(target.cpu(), torch.from_numpy(want))
    assert 0.2 < want.mean() < 0.9                                # both values occur
    _check_frames(out, frames, params)
    # in place, and a run without masks writes no target
    out2, tgt2 = torch.full_like(out, 3.0), torch.full_like(target, 7.0)
    r = ops.augment_stage_u8(fd, ta, tb, sw, masks=md, out=out2, target=tgt2)
    assert r[0].data_ptr() == out2.data_ptr() and r[1].data_ptr() == tgt2.data_ptr()
    assert GA.same_bits(out2, out) and GA.same_bits(tgt2, target)
    tgt2.fill_(7.0)
    out3 = ops.augment_stage_u8(fd, ta, tb, sw, out=out2.fill_(3.0))
    assert isinstance(out3, torch.Tensor) and GA.same_bits(out3, out) and bool((tgt2 == 7.0).all())
    # never a silent copy
    with pytest.raises(RuntimeError):
        ops.augment_stage_u8(fd, ta, tb, sw, out=torch.empty(6, 2, 3, L, L + 4, device=DEV)[..., :L])
    with pytest.raises(RuntimeError):
        ops.augment_stage_u8(fd, ta, tb, sw, masks=md, target=torch.empty(6, L * L, device=DEV, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        ops.augment_stage_u8(fd, ta.long(), tb, sw)
    with pytest.raises(RuntimeError):
        ops.augment_stage_u8(fd, ta, tb, sw, target=tgt2)


def test_clamp_and_swap_bit_are_part_of_the_contract():
    """Table entries in [-3, Hs + 5] read as clamped indices and swap words 2, 3, -1, 0x7ffffffe as their bit 0.  The frames passed
    are a contiguous copy of the interior of a larger block of real data; the expectation is the clamped gather of that copy."""
    A, ops = _mods()
    hs, ws, L = 11, 9, 12
    g = np.random.default_rng(3)
    big = g.integers(0, 256, (4, 2, hs + 8, ws + 8, 3), dtype=np.uint8)
    bigm = g.choice(np.array([0, 1, 37, 255], np.uint8), (2, hs + 8, ws + 8))
    frames, masks = np.ascontiguousarray(big[:, :, 4:4 + hs, 4:4 + ws]), np.ascontiguousarray(bigm[:, 4:4 + hs, 4:4 + ws])
    words = [2, 3, -1, 0x7ffffffe]
    params = [(g.integers(-3, hs + 6, L).astype(np.int32), g.integers(-3, ws + 6, L).astype(np.int32), np.int32(w)) for w in words]
    for p in params:
        p[0][:2], p[1][:2] = (-3, hs + 5), (ws + 5, -3)           # both ends occur
    fd = torch.from_numpy(big).to(DEV)[:, :, 4:4 + hs, 4:4 + ws].contiguous()
    md = torch.from_numpy(bigm).to(DEV)[:, 4:4 + hs, 4:4 + ws].contiguous()
    out, target = ops.augment_stage_u8(fd, *_dev_params(params), masks=md)
    _check_frames(out, frames, params)
    want = np.stack([(A.gather(masks[c % 2], *params[c]) > 0).astype(np.float32).reshape(-1) for c in range(4)])
    assert GA.same_bits(target.cpu(), torch.from_numpy(want))
    for c, w in enumerate(words):                                 # ... and the words mean their bit 0
        same = A.gather(frames[c], params[c][0], params[c][1], w & 1, channels_last=True)
        assert np.array_equal(same, _host_gather(frames, params)[c])


def test_memory_discipline_of_the_input_stage(monkeypatch):
    """tests/guarded_alloc.py as tests/test_memory_discipline.py uses it: bands intact, every element of out / target written,
    frames, masks, tables and swap words bitwise unchanged, results independent of where the buffers sit."""
    A, ops = _mods()
    hs, ws, L = 37, 50, 28
    g = np.random.default_rng(11)
    frames = torch.from_numpy(g.integers(0, 256, (4, 2, hs, ws, 3), dtype=np.uint8))
    masks = torch.from_numpy(g.choice(np.array([0, 1, 37, 255], np.uint8), (2, hs, ws)))
    params = [A.clip_tables((hs, ws), L, op, box) for op, box in (("id", None), ("rot90", _boxed(L)), ("rot180", _boxed(L)), ("rot270+tb", None))]
    ta, tb, sw = (t.cpu() for t in _dev_params(params))

    def call(f, m, a, b, s):
        out, target = ops.augment_stage_u8(f, a, b, s, masks=m)
        return {"out": out, "target": target}
    plain = {k: v.cpu() for k, v in call(*(t.to(DEV) for t in (frames, masks, ta, tb, sw))).items()}

    def body(guard):
        return call(*(guard.tensor(t) for t in (frames, masks, ta, tb, sw))), (), None
    runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set()
    for outs in runs:
        assert set(outs) == set(plain) and all(GA.same_bits(outs[k].cpu(), plain[k]) for k in plain)


def test_augmented_input_loads_in_place_and_replays_with_new_parameters():
    A, ops = _mods()
    hs, ws, L, b, t = 37, 50, 28, 6, 2
    g = np.random.default_rng(21)
    x, target = torch.zeros(b, t, 3, L, L, device=DEV), torch.zeros(b, L * L, device=DEV)
    inp = A.AugmentedInput(x, target, (hs, ws), nmasks=2)
    px, pt = x.data_ptr(), target.data_ptr()

    def draw(seed):
        r = np.random.default_rng(seed)
        ops_ = [A.sample_single(r).op for _ in range(b - 2)] + ["rot90", "rot270"]
        boxes = [None if c % 2 else A.original_random_crop_box(float(r.uniform(5, 20)), L, r) for c in range(b)]
        return [A.clip_tables((hs, ws), L, op, box) for op, box in zip(ops_, boxes)]

    def expect(frames, masks, params):
        return np.stack([(A.gather(masks[c % 2], *params[c]) > 0).astype(np.float32).reshape(-1) for c in range(b)])

    data = []
    for seed in (1, 2):                                           # the second load takes device tensors
        frames = g.integers(0, 256, (b, t, hs, ws, 3), dtype=np.uint8)
        masks = g.choice(np.array([0, 1, 37, 255], np.uint8), (2, hs, ws))
        data.append((frames, masks, draw(seed)))
    frames, masks, params = data[0]
    inp.load(torch.from_numpy(frames), torch.from_numpy(masks), params)
    assert (x.data_ptr(), target.data_ptr()) == (px, pt)
    _check_frames(x, frames, params)
    assert GA.same_bits(target.cpu(), torch.from_numpy(expect(frames, masks, params)))
    frames, masks, params = data[1]
    fd, md = torch.from_numpy(frames).to(DEV), torch.from_numpy(masks).to(DEV)
    stacked = tuple(np.stack([p[k] for p in params]) for k in range(3))
    count = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]          # cumulative: sees a temporary that was freed again
    before = count()
    inp.load(fd, md, stacked)
    assert count() == before, "AugmentedInput.load allocated device memory"
    assert (x.data_ptr(), target.data_ptr()) == (px, pt)
    _check_frames(x, frames, params)
    assert GA.same_bits(target.cpu(), torch.from_numpy(expect(frames, masks, params)))

    # the launch alone, captured; new tables uploaded afterwards are what the replay reads
    # (captured as torch.cuda.graph does it, but on a stream of the HIGH-priority pool: torch hands pool streams out round-robin and
    # mumpy_hip.streams keys its fork/join side streams by their handles, so a normal-priority stream drawn here -- the context
    # manager draws one of its own on first use -- would change which handles every later test of the process is given)
    side = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        inp.launch()
        graph.capture_end()
    new = draw(3)
    assert any(not np.array_equal(n[0], p[0]) or int(n[2]) != int(p[2]) for n, p in zip(new, params))
    for dst, src in zip((inp.tab_a, inp.tab_b, inp.swap), _dev_params(new)):
        dst.copy_(src)
    x.zero_(); target.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _check_frames(x, frames, new)
    assert GA.same_bits(target.cpu(), torch.from_numpy(expect(frames, masks, new)))
    with pytest.raises(RuntimeError):
        inp.load(torch.from_numpy(frames[:, :, :-1]), torch.from_numpy(masks), params)
