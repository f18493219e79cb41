"""GPU: the geometric operations of include/mumpy_geometric.h (ops.geometric_u8; csrc/geometric.hip) and
AugmentedInput(perturb=True, geometric=True).

The oracle of the kernel is the numpy statement mumpy_hip.geometric.apply_row (tests/test_geometric_host.py holds it to Pillow, bit
for bit), plus one direct Pillow comparison per kind.  The oracle of the input stage is the host chain: `gather` source ->
canvas, the numpy statement on the canvas, then the final stage's reference (the host gather through the clip's tables +
ops.normalize_u8, and the gathered mask > 0 as the target).  Every comparison is array_equal / torch.equal / same_bits.

Shapes, nine images each, one and three channels: 1x1 (a tail and nothing else), 2x5, 7x9 and 19x21 (W % 4 != 0: a byte-stored tail
in every row, and rows that start off a 4-byte boundary), 64x48 and 224x224 (whole dwords only; 224x224 takes 13 chunks of quads per
image).  One launch mixes every mode: NONE, both shears, a rotation, a translation, a shift that moves the whole image out, a
rectangle, an empty rectangle and a mode outside the table."""
import numpy as np
import pytest
import torch

import guarded_alloc as GA
from gen_geometric_goldens import image, pil_cutout, pil_geometric
from mumpy_hip import geometric as G

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")

SHAPES = [(1, 1), (2, 5), (7, 9), (19, 21), (64, 48), (224, 224)]
NIMG = 9


def _ops():
    from mumpy_hip import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stack(hw, channels, seed):
    return np.stack([image(hw, channels, seed + k) for k in range(NIMG)])


def _mixed_rows(hw):
    h, w = hw
    rect = (w // 4, h // 3, w // 4 + w / 2.0 + 0.7, h // 3 + h / 3.0 + 0.2)
    rows = [G.params_row("none"), G.params_row("shear_x", 0.3, hw), G.params_row("shear_y", -0.13, hw), G.params_row("rotate", 17.3, hw),
            G.params_row("translate_y", -0.33, hw), np.array([G.MODE_SHIFT, w, 0, 0, 0, 0, 0, 0], np.int32),
            G.params_row("cutout", rect, hw), np.array([G.MODE_RECT, 3, 2, 2, 5, 0, 0, 0], np.int32),
            np.array([57, 65536, 7, 9, 11, 65536, 13, 0], np.int32)]
    assert len(rows) == NIMG and [int(r[0]) for r in rows] == [0, 1, 1, 1, 2, 2, 3, 3, 57]
    return np.stack(rows)


def _want(imgs, rows):
    return np.stack([G.apply_row(a, r) for a, r in zip(imgs, rows)])


@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("hw", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_one_launch_of_every_mode_is_the_numpy_statement(hw, channels):
    ops = _ops()
    imgs, rows = _stack(hw, channels, seed=hw[0] * 31 + hw[1]), _mixed_rows(hw)
    want = _want(imgs, rows)
    assert np.array_equal(want[0], imgs[0]) and not want[5].any() and np.array_equal(want[7], imgs[7]) and np.array_equal(want[8], imgs[8])
    src = _dev(imgs)
    out = ops.geometric_u8(src, _dev(rows), channels=channels)
    assert out.shape == src.shape and out.dtype == torch.uint8
    got = out.cpu().numpy()
    bad = [i for i in range(NIMG) if not np.array_equal(got[i], want[i])]
    assert not bad, f"images {bad} (modes {[int(rows[i][0]) for i in bad]}) differ from the numpy statement"
    assert np.array_equal(src.cpu().numpy(), imgs)
    assert torch.equal(ops.geometric_u8(src, rows, channels=channels), out)                  # host rows are uploaded by the wrapper


CASES = [("shear_x", 0.3), ("shear_x", -0.05), ("shear_y", 0.13), ("shear_y", -0.3), ("translate_x", 0.2501), ("translate_x", -0.45),
         ("translate_y", 0.33), ("translate_x_abs", -7.5), ("translate_y_abs", 10), ("rotate", 0), ("rotate", 1), ("rotate", -30),
         ("rotate", 89.9), ("rotate", 90), ("rotate", 123.4), ("rotate", 180), ("rotate", 270), ("rotate", -179.5)]


@pytest.mark.parametrize("hw,channels", [((37, 53), 3), ((37, 53), 1), ((40, 40), 3)], ids=["37x53x3", "37x53x1", "40x40x3"])
def test_each_kind_is_pillows(hw, channels):
    ops = _ops()
    a = image(hw, channels, 9)
    rect = (5, 3, 20.7, 11.2)
    rows = np.stack([G.params_row(k, v, hw) for k, v in CASES] + [G.params_row("cutout", rect, hw)])
    want = np.stack([pil_geometric(a, k, v) for k, v in CASES] + [pil_cutout(a, rect)])
    got = ops.geometric_u8(_dev(np.stack([a] * len(rows))), rows, channels=channels).cpu().numpy()
    bad = [(CASES + [("cutout", rect)])[i] for i in range(len(rows)) if not np.array_equal(got[i], want[i])]
    assert not bad, f"{bad} differ from Pillow"


@pytest.mark.parametrize("channels", [1, 3])
def test_memory_discipline(monkeypatch, channels):
    """tests/guarded_alloc.py on the entry itself, every buffer in a guarded block: the bands around dst, src and params stay intact,
    every byte of dst is written (dst is prefilled with the guard's byte, under two different bytes), src and params are bitwise
    unchanged, and the runs agree bit for bit."""
    ops = _ops()
    hw = (19, 21)
    imgs, rows = torch.from_numpy(_stack(hw, channels, seed=40)), torch.from_numpy(_mixed_rows(hw))

    def body(guard):
        src = guard.tensor(imgs)
        out = guard.torch.empty(imgs.shape, dtype=torch.uint8, device=DEV)
        ops._call("mumpy_geometric_u8_fwd", ops._p(src), ops._p(out), ops._p(guard.tensor(rows)), NIMG, hw[0], hw[1], channels, ops._stream())
        return {"out": out}, (), None
    runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set() and len(runs) == len(GA.PASSES) and all(torch.equal(runs[0]["out"], outs["out"]) for outs in runs[1:])
    assert np.array_equal(runs[0]["out"].cpu().numpy(), _want(imgs.numpy(), rows.numpy()))


def test_a_sentinel_in_dst_is_overwritten_everywhere_and_two_runs_agree():
    ops = _ops()
    for hw, channels in (((7, 9), 3), ((19, 21), 1), ((64, 48), 3)):
        imgs, rows = _stack(hw, channels, seed=3), _mixed_rows(hw)
        want = _want(imgs, rows)
        src, drows = _dev(imgs), _dev(rows)
        outs = []
        for sentinel in (0xA5, 0x00, 0xFF):
            out = torch.full(src.shape, sentinel, dtype=torch.uint8, device=DEV)
            ops.geometric_u8(src, drows, out=out, channels=channels)
            outs.append(out)
            assert np.array_equal(out.cpu().numpy(), want), (hw, channels, sentinel)
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]) and np.array_equal(src.cpu().numpy(), imgs)


def test_a_captured_launch_follows_later_rows():
    """The rows are rewritten on the device before the replay, which follows them.  (Captured as tests/test_perturb.py does it: on a
    stream of the high-priority pool.)"""
    ops = _ops()
    hw = (24, 40)
    imgs = np.stack([image(hw, 3, 6 + k) for k in range(3)])
    src = _dev(imgs)
    first = np.stack([G.params_row("shear_x", 0.2, hw), G.params_row("none"), G.params_row("cutout", (3, 4, 20.5, 11), hw)])
    second = np.stack([G.params_row("rotate", -30, hw), G.params_row("translate_x", 0.33, hw), G.params_row("none")])
    rows = _dev(first)
    out = torch.empty_like(src)
    ops.geometric_u8(src, rows, out=out)
    assert np.array_equal(out.cpu().numpy(), _want(imgs, first))
    side = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        ops.geometric_u8(src, rows, out=out)
        graph.capture_end()
    rows.copy_(_dev(second))
    out.fill_(9)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want = _want(imgs, second)
    assert np.array_equal(out.cpu().numpy(), want) and not np.array_equal(want, _want(imgs, first))


def test_the_wrapper_refuses_before_launch():
    ops = _ops()
    src = _dev(_stack((16, 16), 3, seed=1))
    rows = _dev(np.zeros((NIMG, 8), np.int32))
    for bad in (src.cpu(), src.float(), src[:, :, :8], src[..., :2]):
        with pytest.raises(RuntimeError):
            ops.geometric_u8(bad, rows)
    with pytest.raises(RuntimeError, match="overlaps"):                           # in place
        ops.geometric_u8(src, rows, out=src)
    both = torch.zeros(src.numel() + 48, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="overlaps"):                           # out is src shifted by one row
        ops.geometric_u8(both[:src.numel()].view(src.shape), rows, out=both[48:].view(src.shape))
    with pytest.raises(RuntimeError):
        ops.geometric_u8(src, rows, out=torch.empty(NIMG, 16, 16, 4, dtype=torch.uint8, device=DEV)[..., :3])
    with pytest.raises(RuntimeError, match=r"\(9, 8\)"):
        ops.geometric_u8(src, torch.zeros(NIMG, 8, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match=r"\(9, 8\)"):
        ops.geometric_u8(src, torch.zeros(NIMG - 1, 8, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match=r"\(9, 8\)"):
        ops.geometric_u8(src, np.zeros((NIMG, 4), np.int32))
    with pytest.raises(RuntimeError, match="channels=2"):
        ops.geometric_u8(src, rows, channels=2)
    with pytest.raises(RuntimeError):                                             # (9, 16, 16, 3) read as single-channel images of 16 x 3
        ops.geometric_u8(src, rows, channels=1)
    mask = src[..., 0].contiguous()
    assert ops.geometric_u8(mask, rows, channels=1).shape == mask.shape
    lib = ops._lib()
    odd = torch.zeros(NIMG * 8 + 4, dtype=torch.int32, device=DEV)[1:NIMG * 8 + 1].view(NIMG, 8)       # 4 bytes off a 16-byte boundary
    with pytest.raises(RuntimeError, match="aligned"):
        ops.geometric_u8(src, odd)
    assert "aligned" in lib.mumpy_last_error().decode()


# ------------------------------------------------------------------------------------------------ the training input stage
B, T, L, SH, SW = 2, 2, 28, 19, 21
DRAWS = [("id", None), ("rot90", (2, 1, 25, 23))]


def _clips(seed=3):
    g = np.random.default_rng(seed)
    frames = np.stack([np.stack([image((SH, SW), 3, int(g.integers(1 << 20))) for _ in range(T)]) for _ in range(B)])
    masks = np.zeros((B, SH, SW), np.uint8)
    masks[0, 4:9, 3:10] = 255
    masks[1, 10:16, 12:19] = 255
    return frames, masks


def _input(geometric=True, nmasks=B, photometric=False):
    from mumpy_hip.augment import AugmentedInput
    x = torch.full((B, T, 3, L, L), float("nan"), device=DEV)
    target = torch.full((B * L * L,), float("nan"), device=DEV)
    return AugmentedInput(x, target, (SH, SW), nmasks=nmasks, perturb=True, photometric=photometric, geometric=geometric), x, target


def _tabs():
    from mumpy_hip.augment import clip_tables
    return [clip_tables((L, L), L, op, box) for op, box in DRAWS]


def _canvas(frames, masks):
    from mumpy_hip.augment import clip_tables, gather
    ta, tb, sw = clip_tables((SH, SW), L, "id")
    return gather(frames, ta, tb, sw, channels_last=True).copy(), gather(masks, ta, tb, sw).copy()


def _stage_on(canvas, mcanvas):
    """The final stage's reference (tests/test_augment_input.py): each clip gathered through its tables on the host, then
    ops.normalize_u8; the target is the gathered mask > 0."""
    from mumpy_hip.augment import gather
    tabs = _tabs()
    moved = np.stack([gather(canvas[c], *tabs[c], channels_last=True) for c in range(B)])
    want_t = np.stack([(gather(mcanvas[c % len(mcanvas)], *tabs[c]) > 0).astype(np.float32).reshape(-1) for c in range(B)])
    return _ops().normalize_u8(_dev(moved)), torch.from_numpy(want_t).to(DEV)


def test_an_input_with_geometric_settings_equals_the_stage_on_a_numpy_moved_canvas():
    """Clip 0 is sheared (its T frames and its mask under one matrix), rotated, translated; clip 1 gets cutout rectangles placed
    against its host mask (the mask stays), or passes through."""
    frames, masks = _clips()
    inp, x, target = _input()
    canvas, mcanvas = _canvas(frames, masks)
    clean_x, clean_t = _stage_on(canvas, mcanvas)
    for k, settings in enumerate(([("shear_x", 0.2), ("cutout", 0.1)], [("rotate", -30), None], [None, ("translate_y", 0.33)],
                                  [("cutout", 0.15), ("shear_y", -0.3)])):
        inp.load(frames, masks, _tabs(), perturb=settings, rng=np.random.default_rng(50 + k))
        want_c, want_m = canvas.copy(), mcanvas.copy()
        rng = np.random.default_rng(50 + k)                                       # the same stream: the same rectangles
        for c, s in enumerate(settings):
            if s is None:
                continue
            if s[0] == "cutout":
                rects = G.cutout_rects(mcanvas[c], s[1], T, rng)
                assert len(rects) == T
                want_c[c] = np.stack([G.cutout(f, r) for f, r in zip(canvas[c], rects)])
                assert not np.array_equal(want_c[c][0], canvas[c][0])
            else:
                want_c[c] = np.stack([G.affine(f, *s) for f in canvas[c]])
                want_m[c] = G.affine(mcanvas[c], *s)
                assert not np.array_equal(want_m[c], mcanvas[c])
        want_x, want_t = _stage_on(want_c, want_m)
        torch.cuda.synchronize()
        assert GA.same_bits(x, want_x) and not GA.same_bits(x, clean_x), settings
        assert GA.same_bits(target.view(B, L * L), want_t), settings
        for c, s in enumerate(settings):
            if s is None:
                assert GA.same_bits(x[c], clean_x[c]) and GA.same_bits(target.view(B, L * L)[c], clean_t[c])
            elif s[0] == "cutout":
                assert GA.same_bits(target.view(B, L * L)[c], clean_t[c])         # Cutout leaves the mask alone
    inp.load(frames, masks, _tabs())                                              # a later load without settings undoes it all
    torch.cuda.synchronize()
    assert GA.same_bits(x, clean_x) and GA.same_bits(target.view(B, L * L), clean_t)


def test_a_replayed_input_follows_the_rows_of_a_second_load():
    frames, masks = _clips()
    inp, x, target = _input(photometric=True)
    inp.load(frames, masks, _tabs(), perturb=[("shear_x", 0.2), ("contrast", 1.4)])
    side = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        inp.launch()
        graph.capture_end()
    frames2, masks2 = _clips(seed=8)
    inp.load(frames2, masks2, _tabs(), perturb=[None, ("rotate", 45)])
    torch.cuda.synchronize()
    x.zero_(); target.zero_()
    graph.replay()
    torch.cuda.synchronize()
    canvas, mcanvas = _canvas(frames2, masks2)
    canvas[1], mcanvas[1] = np.stack([G.affine(f, "rotate", 45) for f in canvas[1]]), G.affine(mcanvas[1], "rotate", 45)
    want_x, want_t = _stage_on(canvas, mcanvas)
    assert GA.same_bits(x, want_x) and GA.same_bits(target.view(B, L * L), want_t)


def test_clips_that_share_a_mask_must_share_their_affine_setting():
    frames, masks = _clips()
    inp, x, target = _input(nmasks=1)
    with pytest.raises(ValueError, match="clips 0 and 1 share mask 0"):
        inp.load(frames, masks[:1], _tabs(), perturb=[("shear_x", 0.2), ("shear_x", 0.1)])
    with pytest.raises(ValueError, match="clips 0 and 1 share mask 0"):
        inp.load(frames, masks[:1], _tabs(), perturb=[("shear_x", 0.2), None])
    with pytest.raises(ValueError, match="clips 0 and 1 share mask 0"):
        inp.load(frames, masks[:1], _tabs(), perturb=[("cutout", 0.1), ("rotate", 5)], rng=np.random.default_rng(0))
    inp.load(frames, masks[:1], _tabs(), perturb=[("rotate", 17), ("rotate", 17)])                    # the same setting: taken
    canvas, mcanvas = _canvas(frames, masks[:1])
    canvas = np.stack([np.stack([G.affine(f, "rotate", 17) for f in clip]) for clip in canvas])
    want_x, want_t = _stage_on(canvas, np.stack([G.affine(mcanvas[0], "rotate", 17)] * B))
    torch.cuda.synchronize()
    assert GA.same_bits(x, want_x) and GA.same_bits(target.view(B, L * L), want_t)


def test_cutout_needs_host_masks_and_a_generator():
    frames, masks = _clips()
    inp, _, _ = _input()
    with pytest.raises(ValueError, match="host"):
        inp.load(frames, torch.from_numpy(masks).to(DEV), _tabs(), perturb=[("cutout", 0.1), None], rng=np.random.default_rng(0))
    with pytest.raises(ValueError, match="rng"):
        inp.load(frames, masks, _tabs(), perturb=[("cutout", 0.1), None])
    inp.load(frames, torch.from_numpy(masks).to(DEV), _tabs(), perturb=[("shear_x", 0.1), None])      # device masks are fine otherwise
    for bad in (("shear_x", 0.31), ("rotate", 200), ("cutout", 0.3), ("shear", 0.1)):
        with pytest.raises(ValueError):
            inp.load(frames, masks, _tabs(), perturb=[bad, None], rng=np.random.default_rng(0))


def test_geometric_false_is_the_object_as_it_was(monkeypatch):
    from mumpy_hip.augment import AugmentedInput
    ops = _ops()
    frames, masks = _clips()
    off, x0, t0 = _input(False)
    on, x1, t1 = _input(True)
    words = 2 * B * L + B * 64 + B * T * 4 + B + B * T                            # tab_a, tab_b, qtab, blur, swap, sel
    assert off.params.numel() == words and on.params.numel() == words + B * T * 8 + B * 8
    assert not hasattr(off, "canvas2") and not hasattr(off, "mask_canvas2") and not hasattr(off, "geo") and not hasattr(off, "geo_mask")
    assert on.canvas2.shape == on.canvas.shape and on.mask_canvas2.shape == on.mask_canvas.shape
    assert on.geo.shape == (B * T, 8) and on.geo_mask.shape == (B, 8) and on.geo.data_ptr() % 16 == 0 and on.geo_mask.data_ptr() % 16 == 0
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a, **kw: (calls.append(name), real(name, *a, **kw))[1])
    off.load(frames, masks, _tabs(), perturb=[("jpeg", 50), None])
    was = list(calls)
    del calls[:]
    on.load(frames, masks, _tabs(), perturb=[("jpeg", 50), None])
    torch.cuda.synchronize()
    assert "mumpy_geometric_u8_fwd" not in was and len(was) == 5
    assert calls == was[:4] + ["mumpy_geometric_u8_fwd"] * 2 + was[4:] and GA.same_bits(x1, x0) and GA.same_bits(t1, t0)
    with pytest.raises(ValueError):                                               # a new kind needs geometric=True
        off.load(frames, masks, _tabs(), perturb=[("shear_x", 0.2), None])
    with pytest.raises(ValueError):                                               # ... which needs perturb=True
        AugmentedInput(x0, None, (SH, SW), geometric=True)
    nomask = AugmentedInput(x0, None, (SH, SW), perturb=True, geometric=True)     # no target: frames only
    assert nomask.mask_canvas2 is None and nomask.geo_mask.shape == (0, 8)
    nomask.load(frames, None, _tabs(), perturb=[("rotate", 90), None])
    canvas, mcanvas = _canvas(frames, masks)
    canvas[0] = np.stack([np.rot90(f, 1) for f in canvas[0]])
    torch.cuda.synchronize()
    assert GA.same_bits(x0, _stage_on(canvas, mcanvas)[0])
    with pytest.raises(ValueError, match="target"):
        nomask.load(frames, None, _tabs(), perturb=[("cutout", 0.1), None], rng=np.random.default_rng(0))
