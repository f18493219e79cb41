"""GPU: the JPEG round trip, the Gaussian blur and the NEAREST gather of include/mumpy_perturb.h (ops.jpeg_roundtrip_u8,
ops.gaussian_blur_u8, ops.resize_nearest_u8; csrc/perturb.hip).

The oracle is the numpy statement of mumpy_hip.perturb (tests/test_perturb_host.py holds it to Pillow, bit for bit), plus one direct
Pillow comparison per operation.  Every comparison is array_equal: the arithmetic is integer.

JPEG shapes: 16x16 (one MCU); 8x8 and 2x2 (an even height that is no multiple of 16: the chroma plane's own last row is repeated,
not the input's); 24x40; 19x21 and 17x33 (odd sizes, clamped edges); 1x1; 224x224; 240x432 (one image).  Blur shapes: 1x9, 9x1, 5x7
(windows wider than the image), 16x16, 19x21, 224x224 with mixed on / off, and images of 700, 1400 and 5500 rows, where the column
tile narrows from 16 to 8, 4 and 1 columns so that its H rows still fit LDS."""
import numpy as np
import pytest
import torch

import guarded_alloc as GA
from mumpy_hip import perturb as P
from test_perturb_host import contents, pil_blur, pil_jpeg

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")

JPEG_SHAPES = [(16, 16, 3), (8, 8, 3), (2, 2, 3), (24, 40, 3), (19, 21, 3), (17, 33, 3), (1, 1, 3), (224, 224, 3), (240, 432, 1)]
QUALITIES = (30, 50, 99, 100)


def _ops():
    from mumpy_hip import ops
    return ops


def _stack(hw, n, seed):
    c = contents(hw, seed)
    return np.stack([c["noise"], c["ramp"], c["checker"]][:n])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ JPEG
@pytest.mark.parametrize("h,w,n", JPEG_SHAPES, ids=[f"{h}x{w}x{n}" for h, w, n in JPEG_SHAPES])
def test_jpeg_roundtrip_is_the_numpy_statement(h, w, n):
    ops = _ops()
    imgs = _stack((h, w), n, seed=h * 31 + w)
    src = _dev(imgs)
    for q in QUALITIES + (1,):
        use = imgs[:1] if q == 1 else imgs                           # quality 1 on the noise image: the decoder's clamp
        want = np.stack([P.jpeg_roundtrip(a, q) for a in use])
        out = ops.jpeg_roundtrip_u8(src[:len(use)], q)
        assert out.shape == (len(use), h, w, 3) and out.dtype == torch.uint8
        got = out.cpu().numpy()
        assert np.array_equal(got, want), f"q={q}: {int((got != want).sum())} of {want.size} bytes differ from the numpy statement"
        assert np.array_equal(src.cpu().numpy(), imgs)               # a distinct dst leaves src alone
        buf = src[:len(use)].clone()                                 # in place equals out of place
        assert ops.jpeg_roundtrip_u8(buf, q, out=buf).data_ptr() == buf.data_ptr() and torch.equal(buf, out)


def test_jpeg_roundtrip_is_pillows():
    ops = _ops()
    imgs = _stack((37, 53), 3, seed=9)
    want = np.stack([pil_jpeg(a, 75)[0] for a in imgs])
    assert np.array_equal(ops.jpeg_roundtrip_u8(_dev(imgs), 75).cpu().numpy(), want)


def test_sel_mixes_tables_and_copies_through():
    """Two tables, and images that pass through: sel < 0, and sel >= ntab, which the host cannot refuse."""
    ops = _ops()
    imgs = np.concatenate([_stack((19, 21), 3, seed=4), _stack((19, 21), 3, seed=5)])
    tabs = ops.jpeg_tables_u16(np.stack([P.jpeg_tables(40), P.jpeg_tables(90)]), DEV)
    sel = [0, 1, -1, 1, 2, 0]
    want = np.stack([a if s not in (0, 1) else P.jpeg_roundtrip(a, (40, 90)[s]) for a, s in zip(imgs, sel)])
    src = _dev(imgs)
    out = ops.jpeg_roundtrip_u8(src, tabs, sel=torch.tensor(sel, dtype=torch.int32, device=DEV))
    assert np.array_equal(out.cpu().numpy(), want)
    buf = src.clone()
    ops.jpeg_roundtrip_u8(buf, tabs, sel=torch.tensor(sel, dtype=torch.int32, device=DEV), out=buf)
    assert torch.equal(buf, out)


def test_the_wrappers_chunk_over_images_without_a_workspace(monkeypatch):
    ops = _ops()
    imgs = np.concatenate([_stack((19, 21), 3, seed=k) for k in range(3)])[:7]
    src = _dev(imgs)
    whole_j, whole_b = ops.jpeg_roundtrip_u8(src, 60), ops.gaussian_blur_u8(src, 1.5)
    monkeypatch.setattr(ops, "PERTURB_CHUNK_BYTES", 3 * 19 * 21 * 3)                    # room for two (blur) / five (JPEG) images
    assert torch.equal(ops.jpeg_roundtrip_u8(src, 60), whole_j) and torch.equal(ops.gaussian_blur_u8(src, 1.5), whole_b)
    assert np.array_equal(whole_j.cpu().numpy(), np.stack([P.jpeg_roundtrip(a, 60) for a in imgs]))


# ------------------------------------------------------------------------------------------------ blur
BLUR_CASES = [((1, 9), (5,)), ((9, 1), (5,)), ((5, 7), (5,)), ((16, 16), (0.1, 0.77, 2.5, 5)), ((19, 21), (0.1, 0.77, 2.5, 5))]


@pytest.mark.parametrize("hw,radii", BLUR_CASES, ids=[f"{h}x{w}" for (h, w), _ in BLUR_CASES])
def test_gaussian_blur_is_the_numpy_statement(hw, radii):
    ops = _ops()
    imgs = _stack(hw, 3, seed=hw[0] * 13 + hw[1])
    src = _dev(imgs)
    for r in radii:
        want = np.stack([P.gaussian_blur(a, r) for a in imgs])
        out = ops.gaussian_blur_u8(src, r)
        got = out.cpu().numpy()
        assert np.array_equal(got, want), f"radius {r}: {int((got != want).sum())} of {want.size} bytes differ from the numpy statement"
        assert np.array_equal(src.cpu().numpy(), imgs)
        buf = src.clone()
        assert ops.gaussian_blur_u8(buf, r, out=buf).data_ptr() == buf.data_ptr() and torch.equal(buf, out)


def test_gaussian_blur_224_with_mixed_settings():
    ops = _ops()
    imgs = _stack((224, 224), 3, seed=2)
    radii = [2.0, None, 4.999]
    want = np.stack([a if r is None else P.gaussian_blur(a, r) for a, r in zip(imgs, radii)])
    src = _dev(imgs)
    params = ops.blur_params(radii, 3, DEV)
    assert params[:, 3].tolist() == [1, 0, 1]
    out = ops.gaussian_blur_u8(src, params)
    assert np.array_equal(out.cpu().numpy(), want)
    buf = src.clone()
    ops.gaussian_blur_u8(buf, params, out=buf)
    assert torch.equal(buf, out)


@pytest.mark.parametrize("h,w", [(700, 9), (1400, 6), (5500, 2)])
def test_gaussian_blur_on_images_taller_than_the_widest_column_tile(h, w):
    ops = _ops()
    img = np.random.default_rng(h).integers(0, 256, (1, h, w, 3), dtype=np.uint8)
    out = ops.gaussian_blur_u8(_dev(img), 3.3)
    assert np.array_equal(out.cpu().numpy()[0], P.gaussian_blur(img[0], 3.3))


def test_gaussian_blur_is_pillows():
    ops = _ops()
    imgs = _stack((37, 53), 3, seed=10)
    assert np.array_equal(ops.gaussian_blur_u8(_dev(imgs), 2.5).cpu().numpy(), np.stack([pil_blur(a, 2.5) for a in imgs]))


# ------------------------------------------------------------------------------------------------ resize
@pytest.mark.parametrize("src,size", [((37, 37), (16, 16)), ((240, 432), (224, 224))], ids=["37-16", "240x432-224x224"])
def test_resize_nearest_is_pillows(src, size):
    from PIL import Image
    ops = _ops()
    imgs = np.random.default_rng(src[0]).integers(0, 256, (2, *src, 3), dtype=np.uint8)
    want = np.stack([np.array(Image.fromarray(a).resize((size[1], size[0]), Image.NEAREST)) for a in imgs])
    sd = _dev(imgs)
    out = ops.resize_nearest_u8(sd, size)
    assert out.shape == (2, *size, 3) and np.array_equal(out.cpu().numpy(), want) and np.array_equal(sd.cpu().numpy(), imgs)
    masks = np.ascontiguousarray(imgs[..., 1])
    want1 = np.stack([np.array(Image.fromarray(a).resize((size[1], size[0]), Image.NEAREST)) for a in masks])
    out1 = ops.resize_nearest_u8(_dev(masks), size, channels=1)
    assert out1.shape == (2, *size) and np.array_equal(out1.cpu().numpy(), want1)
    with pytest.raises(RuntimeError):
        ops.resize_nearest_u8(sd, size, out=sd.view(-1)[:2 * size[0] * size[1] * 3].view(2, *size, 3))      # overlaps the source


# ------------------------------------------------------------------------------------------------ memory discipline
@pytest.mark.parametrize("op", ["jpeg", "blur", "resize"])
def test_memory_discipline(monkeypatch, op):
    """tests/guarded_alloc.py on the entries themselves, every buffer in a guarded block and the workspace of exactly the queried
    size: the bands around dst, src, the settings and the workspace stay intact (no workspace byte beyond the query is written),
    every byte of dst is written, src and the settings are bitwise unchanged."""
    ops = _ops()
    h, w = 19, 21
    imgs = torch.from_numpy(_stack((h, w), 3, seed=21))
    tabs = torch.from_numpy(np.stack([P.jpeg_tables(35), P.jpeg_tables(80)]).astype(np.int16))
    sel = torch.tensor([1, -1, 0], dtype=torch.int32)
    params = torch.tensor([list(P.box_params(5)), [0, 1 << 24, 0, 0], list(P.box_params(0.77))], dtype=torch.int32)

    def body(guard):
        src = guard.tensor(imgs)
        if op == "resize":
            from mumpy_hip.augment import nearest_table
            yt, xt = (guard.tensor(torch.from_numpy(nearest_table(n, 16).copy())) for n in (h, w))
            out = guard.torch.empty(3, 16, 16, 3, dtype=torch.uint8, device=DEV)
            ops._call("mumpy_resize_nearest_u8_fwd", ops._p(src), ops._p(out), ops._p(yt), ops._p(xt), 3, h, w, 16, 16, 3, ops._stream())
            return {"out": out}, (), None
        out = guard.torch.empty(3, h, w, 3, dtype=torch.uint8, device=DEV)
        if op == "jpeg":
            nbytes = int(ops._lib().mumpy_jpeg_roundtrip_workspace_bytes(3, h, w))
            ws = guard.torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            ops._call("mumpy_jpeg_roundtrip_u8_fwd", ops._p(src), ops._p(out), ops._p(guard.tensor(tabs)), ops._p(guard.tensor(sel)),
                      ops._p(ws), nbytes, 3, 2, h, w, ops._stream())
        else:
            nbytes = int(ops._lib().mumpy_gaussian_blur_workspace_bytes(3, h, w))
            ws = guard.torch.empty(nbytes, dtype=torch.uint8, device=DEV)
            ops._call("mumpy_gaussian_blur_u8_fwd", ops._p(src), ops._p(out), ops._p(guard.tensor(params)), ops._p(ws), nbytes, 3, h, w,
                      ops._stream())
        return {"out": out}, (), None
    runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set() and len(runs) == len(GA.PASSES) and all(torch.equal(runs[0]["out"], outs["out"]) for outs in runs[1:])
    a = imgs.numpy()
    if op == "jpeg":
        want = np.stack([P.jpeg_roundtrip(a[0], 80), a[1], P.jpeg_roundtrip(a[2], 35)])
    elif op == "blur":
        want = np.stack([P.gaussian_blur(a[0], 5), a[1], P.gaussian_blur(a[2], 0.77)])
    else:
        from mumpy_hip.augment import nearest_table
        want = a[:, nearest_table(h, 16)][:, :, nearest_table(w, 16)]
    assert np.array_equal(runs[0]["out"].cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ capture
def test_captured_launches_follow_later_settings():
    """A JPEG launch and a blur launch in one graph; sel, qtab and params are rewritten on the device before the replay, which
    follows them.  (Captured as tests/test_annot_resize.py does it: on a stream of the high-priority pool.)"""
    ops = _ops()
    imgs = _stack((24, 40), 3, seed=6)
    src = _dev(imgs)
    tabs = ops.jpeg_tables_u16(np.stack([P.jpeg_tables(30), P.jpeg_tables(85)]), DEV)
    sel = torch.tensor([0, 1, -1], dtype=torch.int32, device=DEV)
    params = ops.blur_params([1.0, None, 2.5], 3, DEV)
    mid, out = torch.empty_like(src), torch.empty_like(src)
    ws = torch.empty(int(ops._lib().mumpy_gaussian_blur_workspace_bytes(3, 24, 40)), dtype=torch.uint8, device=DEV)

    def run():
        ops.jpeg_roundtrip_u8(src, tabs, sel=sel, out=mid, workspace=ws)
        ops.gaussian_blur_u8(mid, params, out=out, workspace=ws)

    def expect(qs, rs):
        j = [a if q is None else P.jpeg_roundtrip(a, q) for a, q in zip(imgs, qs)]
        return np.stack([a if r is None else P.gaussian_blur(a, r) for a, r in zip(j, rs)])
    run()
    assert np.array_equal(out.cpu().numpy(), expect([30, 85, None], [1.0, None, 2.5]))
    side = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        run()
        graph.capture_end()
    sel.copy_(torch.tensor([-1, 0, 1], dtype=torch.int32))
    tabs.copy_(ops.jpeg_tables_u16(np.stack([P.jpeg_tables(55), P.jpeg_tables(99)]), DEV))
    params.copy_(ops.blur_params([None, 0.5, 4.0], 3, DEV))
    out.fill_(9)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want = expect([None, 55, 99], [None, 0.5, 4.0])
    assert np.array_equal(out.cpu().numpy(), want) and not np.array_equal(want, expect([30, 85, None], [1.0, None, 2.5]))


# ------------------------------------------------------------------------------------------------ the wrappers' checks
def test_the_wrappers_refuse_what_would_need_a_copy():
    ops = _ops()
    src = _dev(_stack((16, 16), 3, seed=1))
    for fn, setting in ((ops.jpeg_roundtrip_u8, 50), (ops.gaussian_blur_u8, 1.0)):
        for bad in (src.cpu(), src.float(), src[:, :, :8], src[..., :2]):
            with pytest.raises(RuntimeError):
                fn(bad, setting)
        with pytest.raises(RuntimeError):
            fn(src, setting, out=torch.empty(3, 16, 16, 4, dtype=torch.uint8, device=DEV)[..., :3])
        both = torch.zeros(src.numel() + 48, dtype=torch.uint8, device=DEV)
        with pytest.raises(RuntimeError):                                          # out is src shifted by one row: partial overlap
            fn(both[:src.numel()].view(src.shape), setting, out=both[48:].view(src.shape))
        with pytest.raises(RuntimeError):
            fn(src, setting, workspace=torch.empty(16, dtype=torch.uint8, device=DEV))
    for bad in (0, 101):
        with pytest.raises(ValueError):
            ops.jpeg_roundtrip_u8(src, bad)
    with pytest.raises(RuntimeError):
        ops.jpeg_roundtrip_u8(src, 50, sel=torch.zeros(2, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        ops.gaussian_blur_u8(src, torch.zeros(3, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        ops.jpeg_roundtrip_u8(src, torch.ones(1, 2, 64, dtype=torch.int32, device=DEV))
