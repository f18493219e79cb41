"""GPU: the nine photometric operations of include/mumpy_photometric.h (ops.photometric_u8; csrc/photometric.hip).

The oracle is the numpy statement of mumpy_hip.photometric (tests/test_photometric_host.py holds it to Pillow, bit for bit), plus one
direct Pillow comparison per kind.  Every comparison is array_equal.

Shapes, three images each (noise, narrow-range noise, a ramp): 1x1, 1x9, 9x1, 2x5 (no interior: sharpness copies), 3x3 (one interior
pixel), 7x9, 19x21 (odd sizes: images 1 and 2 start off a 16-byte boundary, and a last group of fewer than 16 pixels), 64x48,
224x224; one 240x432 image; one 700x33 image, whose 1444 pixel groups take three slabs of statistics and three chunks of the apply
launch.  The factors hold 1.1, where d = 12, i = 2 tells a fused multiply-add from the two roundings Pillow does."""
import numpy as np
import pytest
import torch

import guarded_alloc as GA
from gen_photometric_goldens import pil_photometric
from mumpy_hip import photometric as P
from test_photometric_host import contents

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")

SHAPES = [(1, 1, 3), (1, 9, 3), (9, 1, 3), (2, 5, 3), (3, 3, 3), (7, 9, 3), (19, 21, 3), (64, 48, 3), (224, 224, 3), (240, 432, 1),
          (700, 33, 1)]
CASES = [("autocontrast", None), ("invert", None), ("equalize", None), ("solarize", 0), ("solarize", 0.5), ("solarize", 109.7),
         ("solarize", 256), ("posterize", 0), ("posterize", 3), ("posterize", 8)] + \
        [(k, f) for k in P.FACTOR for f in (0, 0.3, 0.77, 1, 1.1, 1.9, 2.5)]
ALL_KINDS = [("autocontrast", None), ("invert", None), ("equalize", None), ("solarize", 77.5), ("posterize", 2), ("contrast", 1.4),
             ("color", 0.6), ("brightness", 1.7), ("sharpness", 1.9)]


def _ops():
    from mumpy_hip import ops
    return ops


def _stack(hw, n, seed):
    c = contents(hw, seed)
    return np.stack([c["noise"], c["narrow"], c["ramp"]][:n])


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rows(settings):
    return torch.from_numpy(np.stack([P.params_row(*(s or ("none", None))) for s in settings])).to(DEV)


def _want(imgs, settings):
    return np.stack([a if s is None else P.apply(a, *s) for a, s in zip(imgs, settings)])


@pytest.mark.parametrize("h,w,n", SHAPES, ids=[f"{h}x{w}x{n}" for h, w, n in SHAPES])
def test_every_kind_is_the_numpy_statement(h, w, n):
    ops = _ops()
    imgs = _stack((h, w), n, seed=h * 31 + w)
    src = _dev(imgs)
    for kind, v in CASES:
        want = np.stack([P.apply(a, kind, v) for a in imgs])
        out = ops.photometric_u8(src, (kind, v))
        assert out.shape == (n, h, w, 3) and out.dtype == torch.uint8
        got = out.cpu().numpy()
        assert np.array_equal(got, want), f"{kind} {v}: {int((got != want).sum())} of {want.size} bytes differ from the numpy statement"
        buf = src.clone()                                            # in place equals out of place
        assert ops.photometric_u8(buf, (kind, v), out=buf).data_ptr() == buf.data_ptr() and torch.equal(buf, out), f"{kind} {v} in place"
    assert np.array_equal(src.cpu().numpy(), imgs)                   # a distinct dst leaves src alone


def test_one_call_mixes_all_kinds_with_pass_through_and_an_unknown_kind():
    ops = _ops()
    settings = ALL_KINDS[:4] + [None] + ALL_KINDS[4:] + [None]
    imgs = np.concatenate([_stack((19, 21), 3, seed=k) for k in range(4)])[:len(settings)]
    rows = _rows(settings)
    rows[-1] = torch.tensor([57, 0x3FC00000, 0, 0], dtype=torch.int32)           # outside the table: copied through
    want = _want(imgs, settings)
    src = _dev(imgs)
    out = ops.photometric_u8(src, rows)
    assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(src.cpu().numpy(), imgs)
    buf = src.clone()
    ops.photometric_u8(buf, rows, out=buf)
    assert torch.equal(buf, out)
    rows[-1, 0] = -3
    assert torch.equal(ops.photometric_u8(src, rows), out)
    per_image = ops.photometric_params(settings, len(settings), DEV)
    assert torch.equal(ops.photometric_u8(src, per_image), out)


@pytest.mark.parametrize("kind,v", ALL_KINDS, ids=[k for k, _ in ALL_KINDS])
def test_each_kind_is_pillows(kind, v):
    ops = _ops()
    imgs = _stack((37, 53), 3, seed=9)
    want = np.stack([pil_photometric(a, kind, v) for a in imgs])
    assert np.array_equal(ops.photometric_u8(_dev(imgs), (kind, v)).cpu().numpy(), want)


def test_the_result_does_not_depend_on_the_workspace_and_repeats():
    ops = _ops()
    settings = ALL_KINDS + [None]
    imgs = np.concatenate([_stack((64, 48), 3, seed=k) for k in range(4)])[:len(settings)]
    src, rows = _dev(imgs), _rows(settings)
    nbytes = int(ops._lib().mumpy_photometric_workspace_bytes(len(settings), 64, 48))
    outs = []
    for fill in (0, 255, 0x5A):
        ws = torch.full((nbytes,), fill, dtype=torch.uint8, device=DEV)
        outs.append(ops.photometric_u8(src, rows, workspace=ws))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
    assert np.array_equal(outs[0].cpu().numpy(), _want(imgs, settings))


def test_the_wrapper_chunks_over_images_without_a_workspace(monkeypatch):
    ops = _ops()
    settings = (ALL_KINDS + [None])[:7]
    imgs = np.concatenate([_stack((19, 21), 3, seed=k) for k in range(3)])[:7]
    src, rows = _dev(imgs), _rows(settings)
    whole = ops.photometric_u8(src, rows)
    one = int(ops._lib().mumpy_photometric_workspace_bytes(1, 19, 21))
    monkeypatch.setattr(ops, "PERTURB_CHUNK_BYTES", 2 * one + 8)                 # two images per launch
    assert torch.equal(ops.photometric_u8(src, rows), whole)
    assert np.array_equal(whole.cpu().numpy(), _want(imgs, settings))


def test_memory_discipline(monkeypatch):
    """tests/guarded_alloc.py on the entry itself, every buffer in a guarded block and the workspace of exactly the queried size: the
    bands around dst, src, params and the workspace stay intact (no workspace byte beyond the query is written), every byte of dst
    is written, src and params are bitwise unchanged."""
    ops = _ops()
    h, w = 19, 21
    settings = ALL_KINDS + [None]
    n = len(settings)
    imgs = torch.from_numpy(np.concatenate([_stack((h, w), 3, seed=30 + k) for k in range(4)])[:n])
    rows = torch.from_numpy(np.stack([P.params_row(*(s or ("none", None))) for s in settings]))

    def body(guard):
        src = guard.tensor(imgs)
        out = guard.torch.empty(n, h, w, 3, dtype=torch.uint8, device=DEV)
        nbytes = int(ops._lib().mumpy_photometric_workspace_bytes(n, h, w))
        ws = guard.torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        ops._call("mumpy_photometric_u8_fwd", ops._p(src), ops._p(out), ops._p(guard.tensor(rows)), ops._p(ws), nbytes, n, h, w,
                  ops._stream())
        return {"out": out}, (), None
    runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set() and len(runs) == len(GA.PASSES) and all(torch.equal(runs[0]["out"], outs["out"]) for outs in runs[1:])
    assert np.array_equal(runs[0]["out"].cpu().numpy(), _want(imgs.numpy(), settings))


def test_a_captured_launch_follows_later_settings():
    """params are rewritten on the device before the replay, which follows them.  (Captured as tests/test_perturb.py does it: on a
    stream of the high-priority pool.)"""
    ops = _ops()
    imgs = _stack((24, 40), 3, seed=6)
    src = _dev(imgs)
    first, second = [("contrast", 1.4), None, ("sharpness", 0.2)], [("equalize", None), ("color", 1.5), None]
    rows = _rows(first)
    out = torch.empty_like(src)
    ws = torch.empty(int(ops._lib().mumpy_photometric_workspace_bytes(3, 24, 40)), dtype=torch.uint8, device=DEV)
    ops.photometric_u8(src, rows, out=out, workspace=ws)
    assert np.array_equal(out.cpu().numpy(), _want(imgs, first))
    side = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        ops.photometric_u8(src, rows, out=out, workspace=ws)
        graph.capture_end()
    rows.copy_(_rows(second))
    out.fill_(9)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    want = _want(imgs, second)
    assert np.array_equal(out.cpu().numpy(), want) and not np.array_equal(want, _want(imgs, first))


def test_the_wrapper_refuses_what_would_need_a_copy():
    ops = _ops()
    src = _dev(_stack((16, 16), 3, seed=1))
    for bad in (src.cpu(), src.float(), src[:, :, :8], src[..., :2]):
        with pytest.raises(RuntimeError):
            ops.photometric_u8(bad, ("invert", None))
    with pytest.raises(RuntimeError):
        ops.photometric_u8(src, ("invert", None), out=torch.empty(3, 16, 16, 4, dtype=torch.uint8, device=DEV)[..., :3])
    both = torch.zeros(src.numel() + 48, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):                                            # out is src shifted by one row: partial overlap
        ops.photometric_u8(both[:src.numel()].view(src.shape), ("invert", None), out=both[48:].view(src.shape))
    with pytest.raises(RuntimeError):
        ops.photometric_u8(src, ("invert", None), workspace=torch.empty(16, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError):
        ops.photometric_u8(src, torch.zeros(3, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError):
        ops.photometric_u8(src, torch.zeros(2, 4, dtype=torch.int32, device=DEV))
    for bad in (("contrast", None), ("invert", 1), ("sharpen", 1.0), ("posterize", 9)):
        with pytest.raises(ValueError):
            ops.photometric_u8(src, bad)
