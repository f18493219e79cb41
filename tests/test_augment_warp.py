"""GPU: the input stage with the interpolating augmentations (ops.augment_warp_u8 / mumpy_augment_warp_u8_fwd,
AugmentedInput(warp=True)).

One launch carries six clips that mix the three modes and both values of the swap bit; T = 2, nmasks = 2.  The reference of every
mode is `warp_reference` of tests/test_augment_warp_host.py, the numpy statement of include/mumpy_hip_ext4.h, which that file pins
against Pillow and against outputs recorded from the reference's own RandomScaleCrop:
  * mode 0 equals ops.augment_stage_u8 bitwise;
  * mode 1 equals ops.normalize_u8 of the numpy-warped uint8 frames bitwise, the target equals warped mask > 0 -- also on the recorded
    cases themselves;
  * mode 2 is fp32 on the device and fp64 in the statement: a pixel must be floor(ref + 0.5), unless ref lies within 1e-2 of a
    half-integer, where it may be the neighbour (fp32 coordinates are off by < 1e-4 px, times 255 grey levels, with margin); at most 5 %
    of a case's pixels may use that exception (uniform noise has 0 - 2.9 % of its pixels in the band).  Targets alike around 0.5.
Shapes: L = 28 (one partial 32-tile) and 36 (2 x 2 tiles, partial), sources 19 x 23 and 28 x 28, S in {L, L + 1, 57, 128}, angles
{0, 1, 37, 90, 135, 179}; six launches per shape cover every S and every angle under both swap values."""
import functools

import numpy as np
import pytest
import torch

import guarded_alloc as GA
from test_augment_warp_host import gather_params, golden, golden_cases, rotate_record, scale_crop_record, warp_reference

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")

ANGLES = (0, 1, 37, 90, 135, 179)
FIELDS = ("tab_a", "tab_b", "swap", "mode", "pos_y", "pos_x", "coef_y", "coef_x", "affine")
SHAPES = [((19, 23), 28), ((19, 23), 36), ((28, 28), 28), ((28, 28), 36)]


def _mods():
    from mumpy_hip import augment, ops
    return augment, ops


def _stack(records):
    """Per-clip records -> the nine stacked host arrays in the order of ops.augment_warp_u8."""
    return [np.stack([np.asarray(getattr(r, f)) for r in records]).astype(np.float32 if f == "affine" else np.int32) for f in FIELDS]


def _dev(arrays):
    return [torch.from_numpy(a).to(DEV) for a in arrays]


def _records(src, L, k):
    """Launch k of a shape: clips 0, 1 gather, 2, 3 resample, 4, 5 rotate; of each pair one clip has the swap bit."""
    A, _ = _mods()
    sides = (L, L + 1, 57, 128)
    s0, s1 = sides[k % 4], sides[(k + 1) % 4]
    box = (s1 // 5, s1 // 9, s1 - s1 // 4, s1 - 2)
    return [gather_params(A.clip_tables(src, L, "vflip", (L // 4, L // 7, L - L // 5, L - L // 3)), L),
            gather_params(A.clip_tables(src, L, ("rot90", "rot270+tb")[k % 2]), L),
            scale_crop_record(src, L, ("hflip", "id")[k % 2], s0, None),
            scale_crop_record(src, L, ("rot270", "rot90+tb")[k % 2], s1, box),
            rotate_record(src, L, ("rot180", "id")[k % 2], ANGLES[k]),
            rotate_record(src, L, ("rot90", "rot270")[k % 2], ANGLES[(k + 3) % 6])]


@functools.lru_cache(maxsize=None)
def _launches(src, L):
    """The six launches of one shape, run once: [(records, frames, masks, out (6, 2, 3, L, L), target (6, L * L))] on the host."""
    _, ops = _mods()
    g = np.random.default_rng(src[0] * 100 + L)
    runs = []
    for k in range(6):
        frames = g.integers(0, 256, (6, 2) + src + (3,), dtype=np.uint8)
        masks = g.choice(np.array([0, 1, 37, 255], np.uint8), (2,) + src)
        records = _records(src, L, k)
        out, target = ops.augment_warp_u8(torch.from_numpy(frames).to(DEV), *_dev(_stack(records)), masks=torch.from_numpy(masks).to(DEV))
        assert out.shape == (6, 2, 3, L, L) and target.shape == (6, L * L) and out.dtype == target.dtype == torch.float32
        runs.append((records, frames, masks, out.cpu(), target.cpu()))
    return runs


def _normalized(u8_nhwc):
    """ops.normalize_u8 of uint8 frames (N, L, L, 3) -> (N, 3, L, L) on the host."""
    _, ops = _mods()
    return ops.normalize_u8(torch.from_numpy(np.ascontiguousarray(u8_nhwc)).to(DEV)).cpu()


@pytest.mark.parametrize("src,L", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_mode_0_is_the_gather_stage_bitwise(src, L):
    _, ops = _mods()
    for records, frames, masks, out, target in _launches(src, L):
        ta, tb, sw = _dev(_stack(records)[:3])
        want_out, want_target = ops.augment_stage_u8(torch.from_numpy(frames).to(DEV), ta, tb, sw, masks=torch.from_numpy(masks).to(DEV))
        for c in (0, 1):
            assert int(records[c].mode) == 0
            assert GA.same_bits(out[c], want_out[c].cpu()) and GA.same_bits(target[c], want_target[c].cpu())
    # an all-gather launch, mode words 0 and 3 with arbitrary upper bits: the whole output is the gather stage's
    arrays = _stack([records[c % 2] for c in range(6)])
    arrays[3] = np.array([0, 3, 4, 7, -4, 0x7ffffffc], np.int32)
    fd, md = torch.from_numpy(frames).to(DEV), torch.from_numpy(masks).to(DEV)
    got_out, got_target = ops.augment_warp_u8(fd, *_dev(arrays), masks=md)
    want_out, want_target = ops.augment_stage_u8(fd, *_dev(arrays[:3]), masks=md)
    assert GA.same_bits(got_out, want_out) and GA.same_bits(got_target, want_target)
    assert isinstance(ops.augment_warp_u8(fd, *_dev(arrays)), torch.Tensor)                  # without masks: no target


@pytest.mark.parametrize("src,L", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_mode_1_is_pillows_resample_bitwise(src, L):
    positive = []
    for records, frames, masks, out, target in _launches(src, L):
        for c in (2, 3):
            assert int(records[c].mode) == 1
            warped, exact = warp_reference(frames[c], records[c], channels_last=True)
            assert exact and GA.same_bits(out[c], _normalized(warped.astype(np.uint8)))
            wmask, _ = warp_reference(masks[c % 2], records[c])
            assert GA.same_bits(target[c], torch.from_numpy((wmask > 0).astype(np.float32).reshape(-1)))
            positive.append(float((wmask > 0).mean()))
    assert 0.0 < min(positive) and max(positive) < 1.0            # both target values occur in every case


def test_mode_1_with_taps_wider_than_the_staged_patch():
    """The kernel stages a 40 x 40 canvas patch per 32 x 32 tile and reads the source directly when a tile's taps span more.  The host's
    rows never do; rows in shuffled order at L = 48 (2 x 2 tiles, partial) do, along y, along x, or both -- the same definition holds."""
    A, ops = _mods()
    src, L = (19, 23), 48
    g = np.random.default_rng(48)
    frames = g.integers(0, 256, (4, 2) + src + (3,), dtype=np.uint8)
    masks = g.choice(np.array([0, 1, 37, 255], np.uint8), (2,) + src)
    records = []
    for c, (op, shuffle_y, shuffle_x) in enumerate((("id", 1, 0), ("rot90", 0, 1), ("hflip", 1, 1), ("rot270", 1, 1))):
        r = scale_crop_record(src, L, op, 57, None)
        oy, ox = (g.permutation(L) if s else np.arange(L) for s in (shuffle_y, shuffle_x))
        records.append(r._replace(pos_y=r.pos_y[oy], coef_y=r.coef_y[oy], pos_x=r.pos_x[ox], coef_x=r.coef_x[ox]))
        assert max(np.ptp(records[-1].pos_y[:32]), np.ptp(records[-1].pos_x[:32])) + 4 > 40          # rows or columns spanned by tile (0, 0)
    out, target = ops.augment_warp_u8(torch.from_numpy(frames).to(DEV), *_dev(_stack(records)), masks=torch.from_numpy(masks).to(DEV))
    for c in range(4):
        warped, _ = warp_reference(frames[c], records[c], channels_last=True)
        assert GA.same_bits(out[c].cpu(), _normalized(warped.astype(np.uint8))), c
        wmask, _ = warp_reference(masks[c % 2], records[c])
        assert GA.same_bits(target[c].cpu(), torch.from_numpy((wmask > 0).astype(np.float32).reshape(-1))), c


def test_mode_1_reproduces_the_references_recorded_outputs():
    """The six recorded RandomScaleCrop cases as one launch: 28 x 28 sources, T = 3, every clip with the mask of its case."""
    _, ops = _mods()
    cases = golden_cases()
    frames = np.stack([golden()["frames"]] * len(cases))
    masks = np.stack([m for _, m, _, _ in cases])
    out, target = ops.augment_warp_u8(torch.from_numpy(frames).to(DEV), *_dev(_stack([r for r, _, _, _ in cases])),
                                      masks=torch.from_numpy(masks).to(DEV))
    for c, (_, _, out_frames, out_mask) in enumerate(cases):
        assert GA.same_bits(out[c].cpu(), _normalized(out_frames)), c
        assert GA.same_bits(target[c].cpu(), torch.from_numpy((out_mask > 0).astype(np.float32).reshape(-1))), c


@functools.lru_cache(maxsize=None)
def _levels():
    """normalize_u8 of every 8-bit value: (3, 256) float32."""
    ramp = np.repeat(np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1), 3, axis=3)
    return _normalized(ramp)[0].reshape(3, 256)


def _pixels(out_c):
    """(T, 3, L, L) float32 -> the 8-bit values the kernel normalized; every element must be the image of one, bit for bit."""
    levels = _levels()
    v = torch.stack([torch.bucketize(out_c[:, ch].contiguous(), levels[ch]) for ch in range(3)], 1).clamp_(0, 255)
    back = torch.stack([levels[ch][v[:, ch]] for ch in range(3)], 1)
    assert GA.same_bits(back, out_c), "an output element is not the normalization of an 8-bit value"
    return v.numpy()


@pytest.mark.parametrize("src,L", SHAPES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_mode_2_is_the_bilinear_warp_of_the_definition(src, L):
    seen = set()
    for k, (records, frames, masks, out, target) in enumerate(_launches(src, L)):
        for c in (4, 5):
            assert int(records[c].mode) == 2
            ref, exact = warp_reference(frames[c], records[c], channels_last=True)                    # (T, L, L, 3) float64
            assert not exact and 0.0 <= ref.min() and ref.max() <= 255.0
            ref = np.moveaxis(ref, -1, 1)
            got = _pixels(out[c])
            near = np.abs(ref - np.floor(ref) - 0.5) <= 1e-2
            plain = got == np.floor(ref + 0.5)
            ok = plain | (near & ((got == np.floor(ref)) | (got == np.floor(ref) + 1)))
            angle = ANGLES[k] if c == 4 else ANGLES[(k + 3) % 6]
            print(f"{src} L={L} angle={angle} swap={int(records[c].swap)}: {int((~plain).sum())} of {plain.size} pixels use the "
                  f"half-integer exception, {int(near.sum())} lie in the band, {int((~ok).sum())} fail")
            assert ok.all(), (angle, int((~ok).sum()))
            assert (~plain).mean() <= 0.05
            mref, _ = warp_reference(masks[c % 2], records[c])
            tgot = target[c].numpy().reshape(L, L)
            assert set(np.unique(tgot).tolist()) <= {0.0, 1.0}
            tplain = tgot == (np.floor(mref + 0.5) > 0)
            assert (tplain | (np.abs(mref - 0.5) <= 1e-2)).all() and (~tplain).mean() <= 0.05
            if angle == 0:                                        # the identity map on the full canvas: the gather itself
                A, _ = _mods()
                assert np.array_equal(got, np.moveaxis(A.gather(frames[c], *records[c][:3], channels_last=True), -1, 1))
            seen.add((angle, int(records[c].swap)))
    assert seen == {(a, s) for a in ANGLES for s in (0, 1)}


def test_garbage_parameters_stay_inside_the_buffers(monkeypatch):
    """Tables, positions and coefficients of random int32 words (half of them small, so that the taps also land inside), random mode
    words, affine rows with NaN, +-Inf and 1e30: under tests/guarded_alloc.py the bands stay intact, every element of out / target is
    written, frames, masks and every parameter array stay bitwise unchanged -- and every output is finite."""
    _, ops = _mods()
    (hs, ws), L, n = (19, 23), 36, 8
    g = np.random.default_rng(5)

    def words(shape):
        wild = g.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int64)
        return np.where(g.random(shape) < 0.5, wild, g.integers(-6, L + 6, shape)).astype(np.int32)
    affine = g.normal(0.0, 1.0, (n, 8)).astype(np.float32)
    affine[0, 0], affine[1, 2], affine[2, 5], affine[3, 5], affine[4, 2] = np.nan, np.inf, -np.inf, 1e30, -1e30
    mode = (g.integers(-2 ** 29, 2 ** 29, n) * 4 + np.array([2, 2, 2, 2, 2, 1, 0, 3])).astype(np.int32)
    arrays = [words((n, L)), words((n, L)), words((n,)), mode, words((n, L)), words((n, L)), words((n, L, 4)), words((n, L, 4)), affine]
    assert [int(m) & 3 for m in mode] == [2, 2, 2, 2, 2, 1, 0, 3] and {int(s) & 1 for s in arrays[2]} == {0, 1}
    inputs = [torch.from_numpy(g.integers(0, 256, (n, 2, hs, ws, 3), dtype=np.uint8)),
              torch.from_numpy(g.integers(0, 256, (2, hs, ws), dtype=np.uint8))] + [torch.from_numpy(a) for a in arrays]

    def body(guard):
        f, m, *rest = (guard.tensor(t) for t in inputs)
        out, target = ops.augment_warp_u8(f, *rest, masks=m)
        return {"out": out, "target": target}, (), None
    runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set()
    for outs in runs:
        assert bool(torch.isfinite(outs["out"]).all()) and bool(torch.isfinite(outs["target"]).all())
        assert set(np.unique(outs["target"].cpu().numpy()).tolist()) <= {0.0, 1.0}
    assert len(runs) == len(GA.PASSES)
    assert all(GA.same_bits(runs[0][k].cpu(), outs[k].cpu()) for outs in runs[1:] for k in runs[0])   # independent of the fill around them
    # the affine clips whose rows hold a NaN, an infinity or 1e30 see nothing but border; the others see mask
    assert all(float(runs[0]["target"][c].abs().max()) == 0.0 for c in range(5)) and float(runs[0]["target"][5:].max()) == 1.0


def test_augmented_input_warp_matches_the_old_path_and_replays_a_later_load():
    A, ops = _mods()
    src, L, b, t = (19, 23), 28, 6, 2
    g = np.random.default_rng(21)
    data = [(torch.from_numpy(g.integers(0, 256, (b, t) + src + (3,), dtype=np.uint8)),
             torch.from_numpy(g.choice(np.array([0, 1, 37, 255], np.uint8), (2,) + src))) for _ in range(2)]
    triples = [A.clip_tables(src, L, op, box) for op, box in
               (("id", None), ("rot90", (3, 2, 20, 25)), ("vflip", None), ("rot270", None), ("hflip", (0, 5, 28, 21)), ("rot90+tb", None))]

    # old-style triples: the same bits as the warp=False object
    x0, t0 = torch.zeros(b, t, 3, L, L, device=DEV), torch.zeros(b, L * L, device=DEV)
    x1, t1 = torch.zeros_like(x0), torch.zeros_like(t0)
    A.AugmentedInput(x0, t0, src, nmasks=2).load(*data[0], triples)
    inp = A.AugmentedInput(x1, t1, src, nmasks=2, warp=True)
    inp.load(*data[0], triples)
    assert GA.same_bits(x1, x0) and GA.same_bits(t1, t0) and bool(x0.abs().sum() > 0)
    inp.load(*data[0], tuple(np.stack([p[k] for p in triples]) for k in range(3)))                  # ... and the three stacked arrays
    assert GA.same_bits(x1, x0) and GA.same_bits(t1, t0)
    with pytest.raises(RuntimeError):
        A.AugmentedInput(x0, t0, src, nmasks=2).load(*data[0], _records(src, L, 2))              # records need warp=True

    # the launch alone, captured (on a stream of the high-priority pool, as tests/test_augment_input.py explains); a later load()
    # uploads new frames, masks and a parameter block that mixes triples and records, and the replay reads them
    side = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        inp.launch()
        graph.capture_end()
    records = _records(src, L, 2)
    mixed = [triples[1], records[2], records[3], records[4], records[5], triples[4]]
    count = lambda: torch.cuda.memory_stats()["allocation.all.allocated"]          # cumulative: sees a temporary that was freed again
    before = count()
    inp.load(*data[1], mixed)
    assert count() == before, "AugmentedInput.load allocated device memory"
    full = [gather_params(triples[1], L)] + records[2:6] + [gather_params(triples[4], L)]
    want_x, want_t = ops.augment_warp_u8(data[1][0].to(DEV), *_dev(_stack(full)), masks=data[1][1].to(DEV))
    assert GA.same_bits(x1, want_x) and GA.same_bits(t1, want_t) and not GA.same_bits(x1, x0)
    x1.zero_(); t1.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert GA.same_bits(x1, want_x) and GA.same_bits(t1, want_t)
