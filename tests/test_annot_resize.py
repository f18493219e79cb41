"""GPU: Pillow's BILINEAR resize of annotations on the device (include/mumpy_hip_ext6.h, ops.resize_bilinear_u8) and
VideoPredictor(gt_hw=...), which scores a video against annotations that arrive at their own size.

The oracle is Pillow itself, bit for bit (tests/test_annot_resize_host.py holds the numpy statement to it as well); for the predictor
it is a second predictor that is fed the same annotations resized by Pillow on the host.

Shapes.  The kernel gives a workgroup a band of 16 output rows of one image (fewer where the band's intermediate rows would not fit
its 48 KiB) and walks the band's source rows in quads:
  7x5 -> 16x16        an upscale, 3 taps, one band of one image
  37x53 -> 16x32      ragged, a different ratio per axis
  61x854 -> 8x224     the DAVIS width (not a multiple of 4), 9 horizontal / 17 vertical taps
  30x1920 -> 4x224    19 horizontal taps
  224x224 -> same     the identity
  200x20 -> 40x16     bands of 16, 16 and 8 rows; 87 of the 200 source rows fit a band, so hostile tables reach the row cap
  200x300 -> 20x600   16 rows would need 103 KB: the band shrinks to 4 rows, five bands
each with n = 1 and n = 3 distinct images."""
import numpy as np
import pytest
import torch

import guarded_alloc as GA
from test_annot_resize_host import ARGS, ENTRY, KMAX_CAP, BAND_BYTES, POINTERS, pil_resize, sweep_refusals

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")

CASES = [((7, 5), (16, 16)), ((37, 53), (16, 32)), ((61, 854), (8, 224)), ((30, 1920), (4, 224)), ((224, 224), (224, 224)),
         ((200, 20), (40, 16)), ((200, 300), (20, 600))]
IDS = [f"{s[0]}x{s[1]}-{d[0]}x{d[1]}" for s, d in CASES]


def _ops():
    from mumpy_hip import ops
    return ops


def _images(n, hw, seed):
    """n distinct images: random bytes, then a sparse 0 / 255 mask, then a block of 2 on zeros."""
    g = np.random.default_rng(seed)
    h, w = hw
    imgs = [g.integers(0, 256, (h, w), dtype=np.uint8), ((g.random((h, w)) < 0.05) * 255).astype(np.uint8), np.zeros((h, w), np.uint8)]
    imgs[2][h // 4:h // 2 + 1, w // 3:w // 2 + 1] = 2
    return np.stack(imgs[:n])


def _pil(imgs, size):
    return np.stack([pil_resize(a, size) for a in imgs])


def _taps(src, size):
    from mumpy_hip.video import bilinear_taps
    return [torch.from_numpy(a) for a in bilinear_taps(src[0], size[0]) + bilinear_taps(src[1], size[1])]


def _raw(src, out, tabs, size):
    """The entry itself, on the caller's buffers and tables."""
    ops = _ops()
    n, hs, ws = src.shape
    ops._call(ENTRY, *[ops._p(t) for t in (src, out, *tabs)], n, hs, ws, size[0], size[1], tabs[2].shape[1], tabs[5].shape[1],
              ops._stream())
    return out


# ------------------------------------------------------------------------------------------------ the kernel is Pillow's resize
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("src,size", CASES, ids=IDS)
def test_resize_is_pillows_bit_for_bit(src, size, n):
    ops = _ops()
    imgs = _images(n, src, seed=src[0] * 7 + n)
    want = _pil(imgs, size)
    sd = torch.from_numpy(imgs).to(DEV)
    out = ops.resize_bilinear_u8(sd, size)
    assert out.shape == (n, *size) and out.dtype == torch.uint8 and out.is_cuda
    got = out.cpu().numpy()
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} bytes differ from Image.resize(BILINEAR)"
    assert np.array_equal(sd.cpu().numpy(), imgs)
    # in place, and never a silent copy
    buf = torch.full_like(out, 77)
    assert ops.resize_bilinear_u8(sd, size, out=buf).data_ptr() == buf.data_ptr() and torch.equal(buf, out)
    with pytest.raises(RuntimeError):
        ops.resize_bilinear_u8(sd.float(), size)
    with pytest.raises(RuntimeError):
        ops.resize_bilinear_u8(sd.cpu(), size)
    with pytest.raises(RuntimeError):
        ops.resize_bilinear_u8(sd, size, out=torch.empty(n, size[0], size[1] + 4, device=DEV, dtype=torch.uint8)[..., :size[1]])
    with pytest.raises(RuntimeError):
        ops.resize_bilinear_u8(torch.from_numpy(np.ascontiguousarray(imgs.transpose(0, 2, 1))).to(DEV).transpose(1, 2), size)
    with pytest.raises(RuntimeError):
        ops.resize_bilinear_u8(sd[0], size)


# ------------------------------------------------------------------------------------------------ memory discipline
def _hostile(tabs, src, which):
    """Tables nobody validated: starts of -5 and n_in + 5, counts of -1 and kmax + 7 (`edges`); rows of one band that lie the whole
    source apart, every count over the cap and weights that wrap the sum (`spread`)."""
    tabs = [t.clone() for t in tabs]
    for (s, c, k), n_in in zip((tabs[:3], tabs[3:]), src):
        kmax = k.shape[1]
        if which == "edges":
            s[0], s[1], c[2], c[3] = -5, n_in + 5, -1, kmax + 7
            s[4], c[4], s[5], c[5] = n_in + 5, kmax + 7, -5, kmax + 7
        else:
            s[0::2], s[1::2] = 0, n_in + 5
            c[:] = kmax + 7
            k[:] = 2 ** 31 - 1
    return tabs


@pytest.mark.parametrize("tables", ["pillow", "edges", "spread"])
@pytest.mark.parametrize("src,size", [CASES[1], CASES[5], CASES[6]], ids=[IDS[1], IDS[5], IDS[6]])
def test_memory_discipline(monkeypatch, src, size, tables):
    """tests/guarded_alloc.py as tests/test_memory_discipline.py uses it, on the entry itself so that the tables sit in guarded blocks
    too: the bands around out, src and the six tables stay intact, every byte of out is written, src and the tables are bitwise
    unchanged -- with Pillow's tables (then out is Pillow's, wherever the buffers sit) and with hostile ones, which by the header's
    contract are clamped: in bounds, no fault, unspecified bytes."""
    ops = _ops()
    imgs = torch.from_numpy(_images(3, src, seed=11))
    tabs = _taps(src, size)
    if tables != "pillow":
        tabs = _hostile(tabs, src, tables)

    def body(guard):
        out = guard.torch.empty(3, *size, dtype=torch.uint8, device=DEV)
        return {"out": _raw(guard.tensor(imgs), out, [guard.tensor(t) for t in tabs], size)}, (), None
    runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set()
    assert len(runs) == len(GA.PASSES)
    assert all(torch.equal(runs[0]["out"], outs["out"]) for outs in runs[1:])     # the same bytes wherever the buffers sit, hostile or not
    if tables == "pillow":
        assert np.array_equal(runs[0]["out"].cpu().numpy(), _pil(imgs.numpy(), size))


def test_the_binding_allocates_out_inside_the_guard(monkeypatch):
    """... and ops.resize_bilinear_u8 as users call it (its tables are cached outside the guard)."""
    ops = _ops()
    src, size = CASES[2]
    imgs = torch.from_numpy(_images(3, src, seed=5))

    def body(guard):
        return {"out": ops.resize_bilinear_u8(guard.tensor(imgs), size)}, (), None
    runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set()
    for outs in runs:
        assert np.array_equal(outs["out"].cpu().numpy(), _pil(imgs.numpy(), size))


# ------------------------------------------------------------------------------------------------ capture
def test_captured_launch_replays_on_new_bytes():
    """One launch, captured; the replay resizes what src holds THEN.  (Captured as tests/test_augment_input.py does it: on a stream
    of the high-priority pool, so that no normal-priority pool stream is drawn here.)"""
    ops = _ops()
    src, size = CASES[1]
    a, b = _images(3, src, seed=1), _images(3, src, seed=2)
    sd = torch.from_numpy(a).to(DEV)
    out = ops.resize_bilinear_u8(sd, size)                           # the tables of this shape are uploaded here, outside the capture
    assert np.array_equal(out.cpu().numpy(), _pil(a, size))
    side = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        ops.resize_bilinear_u8(sd, size, out=out)
        graph.capture_end()
    sd.copy_(torch.from_numpy(b))
    out.fill_(9)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), _pil(b, size)) and not np.array_equal(_pil(a, size), _pil(b, size))


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_of_the_header_launches_nothing():
    """The table of tests/test_annot_resize_host.py against real buffers, each large enough for every valid tuple of the table: the
    valid tuples run (rc == 0), every broken one is refused with its MUMPY_E* code and a message of its own -- and no buffer changes."""
    from mumpy_hip.lib import load_library
    wmax = BAND_BYTES // 2
    sizes = {"src": (2 * 1000 * 7, torch.uint8), "out": (2 * 8 * wmax, torch.uint8), "ystart": (8, torch.int32), "ycount": (8, torch.int32),
             "ycoef": (8 * KMAX_CAP, torch.int32), "xstart": (wmax, torch.int32), "xcount": (wmax, torch.int32),
             "xcoef": (max(wmax * 3, 8 * KMAX_CAP), torch.int32)}
    assert list(sizes) == POINTERS == ARGS[:8]
    bufs = {k: torch.zeros(n + 64, device=DEV, dtype=dt) for k, (n, dt) in sizes.items()}      # (64 elements of slack: moved pointers)
    snap = {}

    def before_refusals():
        torch.cuda.synchronize()
        for k, t in bufs.items():
            t.view(torch.uint8).fill_(0x5A)
            snap[k] = t.view(torch.uint8).clone()
    n = sweep_refusals(load_library(), {k: t.data_ptr() for k, t in bufs.items()}, launches=True, before_refusals=before_refusals)
    torch.cuda.synchronize()
    assert n >= 30 and snap and all(torch.equal(t.view(torch.uint8), snap[k]) for k, t in bufs.items())


# ------------------------------------------------------------------------------------------------ end to end
HS, WS, BATCH, GT_HW = 30, 26, 4, (61, 107)                          # the model fixture and sizes of tests/test_video_stage.py


@pytest.fixture(scope="module")
def predictors():
    """Seeded weights, the three-view model at T = 3 and, per mode, a predictor that takes annotations at 61 x 107 and one that takes
    them at 224 x 224.  Every graphed predictor owns a capture stream and fork/join side streams under it; the entries they add to
    mumpy_hip.streams' registry are taken out again afterwards, so that the rest of the process finds it as it was."""
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from mumpy_hip import streams
    from mumpy_hip.video import VideoPredictor
    from weight_fill import fill_module_
    from mumpy_hip.pipeline import fused_forward
    from mumpy_hip.video import batch_plan
    before = set(streams._SIDE)
    enc, dec = fill_module_(Encoder()).eval().to(DEV), fill_module_(Decoder()).eval().to(DEV)
    idx, _ = batch_plan(5, 3, BATCH)                                 # thr: the sigmoid of the first batch's median logit, so that
    clips = torch.from_numpy(_video()[0]).to(DEV)[torch.from_numpy(idx[0]).long().to(DEV)]        # the masks hold both values
    thr = float(torch.sigmoid(fused_forward(enc, dec, _ops().normalize_u8(clips, size=(224, 224)))[0]).median())
    assert 0.0 < thr < 1.0
    made = {}

    def get(graph, native, **kw):
        key = (graph, native, tuple(sorted(kw.items())))
        if key not in made:
            made[key] = VideoPredictor(enc, dec, T=3, src_hw=(HS, WS), batch=BATCH, max_frames=16, thr=thr, graph=graph,
                                       gt_hw=GT_HW if native else None, **kw)
        return made[key]
    yield get
    torch.cuda.synchronize()
    made.clear()
    for key in set(streams._SIDE) - before:
        del streams._SIDE[key]


def _video(n=5):
    g = np.random.default_rng(77)
    frames = g.integers(0, 256, (n, HS, WS, 3), dtype=np.uint8)
    gt = ((g.random((n, *GT_HW)) < 0.3) * 255).astype(np.uint8)
    gt[1] = g.integers(0, 4, GT_HW)                                  # small values: `> 0` after the resize sees the rounding
    gt[2] = 0                                                        # a frame without annotation
    return frames, gt


@pytest.mark.parametrize("graph", [True, False], ids=["graph", "eager"])
def test_native_annotations_score_like_pillow_resized_ones(predictors, graph):
    frames, gt = _video()
    resized = _pil(gt, (224, 224))
    native, plain = predictors(graph, True), predictors(graph, False)
    native.reset_metrics(); plain.reset_metrics()
    m_native = native.predict(frames, gt).clone()
    m_plain = plain.predict(frames, resized).clone()
    torch.cuda.synchronize()
    assert torch.equal(m_native, m_plain) and np.unique(m_native.cpu().numpy()).tolist() == [0, 255]
    assert torch.equal(native.gt[:5], plain.gt[:5]) and np.array_equal(native.gt[:5].cpu().numpy().reshape(5, 224, 224), resized)
    assert torch.equal(native.counts[:5], plain.counts[:5])
    assert GA.same_bits(native.metric_vector(), plain.metric_vector()) and float(native.metric_vector()[2]) == 5.0
    assert int(native.counts[:5, 2].sum()) > 0                       # annotated pixels were counted at all
    # annotations that are already on the device are resized where they are: the same bits
    native.reset_metrics()
    m_dev = native.predict(torch.from_numpy(frames).to(DEV), torch.from_numpy(gt).to(DEV)).clone()
    torch.cuda.synchronize()
    assert torch.equal(m_dev, m_plain) and torch.equal(native.gt[:5], plain.gt[:5])
    assert GA.same_bits(native.metric_vector(), plain.metric_vector())


def test_a_gt_of_the_wrong_size_raises_before_any_launch(predictors):
    frames, gt = _video()
    native = predictors(False, True)
    native.predict(frames, gt)
    torch.cuda.synchronize()
    state = [t.clone() for t in (native.frames, native.gt, native.bank, native.counts, native.acc)]
    other = np.zeros_like(frames)
    for bad in (np.zeros((5, 224, 224), np.uint8), np.zeros((5, GT_HW[0], GT_HW[1] + 1), np.uint8), np.zeros((4, *GT_HW), np.uint8),
                np.zeros((5, *GT_HW), np.float32), np.zeros((5, *GT_HW, 1), np.uint8)):
        with pytest.raises(ValueError):
            native.predict(other, bad)
    with pytest.raises(ValueError):                                  # on the device: read where it is, so it must be dense
        native.predict(other, torch.zeros(5, GT_HW[1], GT_HW[0], dtype=torch.uint8, device=DEV).transpose(1, 2))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(state, (native.frames, native.gt, native.bank, native.counts, native.acc)))
    from mumpy_hip.video import VideoPredictor
    for kw in (dict(gt_hw=(0, 5)), dict(gt_hw=(61,)), dict(gt_hw=(61, 107), gt_chunk=0), dict(gt_hw=(224 * 32 + 1, 10))):
        with pytest.raises(ValueError):
            VideoPredictor(native.encoder, native.decoder, T=3, src_hw=(HS, WS), graph=False, **kw)


def test_host_annotations_longer_than_the_staging_chunk(predictors):
    """gt_chunk=2 against 5 frames: three uploads through the staging buffer, the last of one frame."""
    frames, gt = _video()
    chunked, native = predictors(False, True, gt_chunk=2), predictors(False, True)
    assert chunked._gt_stage.shape == (2, *GT_HW) and native._gt_stage.shape == (16, *GT_HW)      # (never more than max_frames)
    chunked.reset_metrics(); native.reset_metrics()
    m_host = chunked.predict(frames, gt).clone()
    m_dev = native.predict(frames, torch.from_numpy(gt).to(DEV)).clone()
    torch.cuda.synchronize()
    assert torch.equal(m_host, m_dev) and torch.equal(chunked.gt[:5], native.gt[:5]) and torch.equal(chunked.counts[:5], native.counts[:5])
    assert GA.same_bits(chunked.metric_vector(), native.metric_vector())
    assert np.array_equal(chunked.gt[:5].cpu().numpy().reshape(5, 224, 224), _pil(gt, (224, 224)))
