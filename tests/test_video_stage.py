"""GPU: whole-video inference on the device (include/mumpy_hip_ext5.h, ops.clip_window_u8 / mask_score_u8 / frame_metrics,
mumpy_hip.video.VideoPredictor).

The oracles are the numpy statements of tests/test_video_host.py (checked there on hand-made cases) and code that exists without
the new kernels: ops.normalize_u8 of the gathered frames for the window (bit for bit), pipeline.fused_forward on the same clip batches
for the predictor (bit for bit: the same shapes, so the same kernels).

Shapes.  Window: 3 frames, T = 3, 10 x 13 -> 8 x 12 (a few blocks, both tables non-trivial); the identity size on an 8 x 12 source (the
output width must be a multiple of 4, so 10 x 13 has no identity case); 240 x 432 -> 224 x 224 (the model's: ~900 blocks).  Score:
npix = 64 (4 of a workgroup's 256 threads hold pixels), 16 * 257 (ragged over the threads) and 224 * 224 (the model's: every thread
walks several chunks, all four waves reduce).  Metrics: 5 frames and 300 (more frames than threads)."""
import numpy as np
import pytest
import torch

import guarded_alloc as GA
from test_video_host import (ARGS, REFUSALS, masks_metrics_reference, metrics_reference, score_reference, sweep_refusals,
                             window_reference)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")

IDX = [[-5, 0, 1], [0, 1, 2], [1, 2, 99], [2, 2, 0]]                  # -5 and 99 clamp


def _ops():
    from mumpy_hip import ops
    return ops


# ------------------------------------------------------------------------------------------------ the window
@pytest.mark.parametrize("src,size,nclips", [((10, 13), (8, 12), 4), ((8, 12), (8, 12), 4), ((240, 432), (224, 224), 2)],
                         ids=["10x13-8x12", "identity-8x12", "240x432-224x224"])
def test_clip_window_is_gather_plus_normalize_bit_for_bit(src, size, nclips):
    ops = _ops()
    frames = np.random.default_rng(src[0]).integers(0, 256, (3, *src, 3), dtype=np.uint8)
    idx = np.array(IDX[:nclips], np.int32)
    fd, idd = torch.from_numpy(frames).to(DEV), torch.from_numpy(idx).to(DEV)
    out = ops.clip_window_u8(fd, idd, size)
    assert out.shape == (nclips, 3, 3, *size) and out.dtype == torch.float32
    want = ops.normalize_u8(fd[torch.from_numpy(np.clip(idx, 0, 2).astype(np.int64)).to(DEV)], size=size)
    assert GA.same_bits(out, want), f"{int((out != want).sum())} of {out.numel()} elements differ from normalize_u8(frames[idx])"
    moved, ref = window_reference(frames, idx, size)
    assert np.array_equal(moved, window_reference(frames, np.clip(idx, 0, 2), size)[0])
    assert np.abs(out.cpu().numpy().astype(np.float64) - ref).max() <= 1e-5          # the bar of test_resize_normalize_u8_input_staging
    # in place, other statistics, and never a silent copy
    buf = torch.full_like(out, 3.0)
    r = ops.clip_window_u8(fd, idd, size, out=buf, mean=(0.1, 0.2, 0.3), std=(0.5, 0.25, 2.0))
    assert r.data_ptr() == buf.data_ptr()
    assert GA.same_bits(buf, ops.normalize_u8(fd[idd.clamp(0, 2).long()], mean=(0.1, 0.2, 0.3), std=(0.5, 0.25, 2.0), size=size))
    with pytest.raises(RuntimeError):
        ops.clip_window_u8(fd, idd.long(), size)
    with pytest.raises(RuntimeError):
        ops.clip_window_u8(fd, idd, size, out=torch.empty(nclips, 3, 3, size[0], size[1] + 4, device=DEV)[..., :size[1]])
    with pytest.raises(RuntimeError):
        ops.clip_window_u8(fd.cpu(), idd, size)


def test_memory_discipline_of_the_window(monkeypatch):
    """tests/guarded_alloc.py as tests/test_memory_discipline.py uses it: bands intact, every element of out written, frames and
    frame_idx bitwise unchanged, the result independent of where the buffers sit."""
    ops = _ops()
    frames = torch.from_numpy(np.random.default_rng(2).integers(0, 256, (3, 10, 13, 3), dtype=np.uint8))
    idx = torch.tensor(IDX, dtype=torch.int32)
    plain = ops.clip_window_u8(frames.to(DEV), idx.to(DEV), (8, 12)).cpu()

    def body(guard):
        return {"out": ops.clip_window_u8(guard.tensor(frames), guard.tensor(idx), (8, 12))}, (), None
    runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set()
    for outs in runs:
        assert GA.same_bits(outs["out"].cpu(), plain)


# ------------------------------------------------------------------------------------------------ bank and counts
@pytest.mark.parametrize("npix", [64, 16 * 257, 224 * 224])
def test_mask_score_bank_and_counts_are_exact(npix):
    ops = _ops()
    g = np.random.default_rng(npix)
    nclips, nbank = 4, 5
    mask = g.choice(np.array([0, 0, 1, 1, 200], np.uint8), (nclips, npix))
    gt = g.choice(np.array([0, 0, 1, 37, 255], np.uint8), (nbank, npix))
    dest = np.array([3, -1, 0, 5], np.int32)                         # -1 and 5 (= nbank) are dropped
    bank0, counts0 = np.full((nbank, npix), 9, np.uint8), np.full((nbank, 4), -7, np.int32)
    md, gd, dd = (torch.from_numpy(a).to(DEV) for a in (mask, gt, dest))
    bank, counts = torch.from_numpy(bank0).to(DEV), torch.from_numpy(counts0).to(DEV)
    rb, rc = ops.mask_score_u8(md.view(nclips, 1, -1), dd, bank, gt=gd, counts=counts)
    assert rb.data_ptr() == bank.data_ptr() and rc.data_ptr() == counts.data_ptr()
    wb, wc = score_reference(mask, dest, bank0, gt, counts0)
    assert np.array_equal(bank.cpu().numpy(), wb) and np.array_equal(counts.cpu().numpy(), wc)
    assert (wb[[1, 2, 4]] == 9).all() and (wc[[1, 2, 4]] == -7).all()                 # rows no valid dest names keep the sentinel
    assert set(np.unique(bank.cpu().numpy()[[0, 3]]).tolist()) == {0, 255}            # bank values are only 0 / 255
    assert np.array_equal(md.cpu().numpy(), mask) and np.array_equal(gd.cpu().numpy(), gt) and np.array_equal(dd.cpu().numpy(), dest)
    # without an annotation no counts are touched (none can even be passed), the bank is the same
    bank2 = torch.from_numpy(bank0).to(DEV)
    r = ops.mask_score_u8(md, dd, bank2)
    assert isinstance(r, torch.Tensor) and r.data_ptr() == bank2.data_ptr() and np.array_equal(bank2.cpu().numpy(), wb)
    assert np.array_equal(counts.cpu().numpy(), wc)
    rb3, rc3 = ops.mask_score_u8(md, dd, torch.from_numpy(bank0).to(DEV), gt=gd)      # counts allocated: zero where nothing was written
    want3 = score_reference(mask, dest, bank0, gt, np.zeros((nbank, 4), np.int32))[1]
    assert np.array_equal(rc3.cpu().numpy(), want3)
    with pytest.raises(RuntimeError):
        ops.mask_score_u8(md, dd, bank2, counts=counts)
    with pytest.raises(RuntimeError):
        ops.mask_score_u8(md, dd.long(), bank2)
    with pytest.raises(RuntimeError):
        ops.mask_score_u8(md[:, :npix - 16], dd, bank2)
    with pytest.raises(RuntimeError):
        ops.mask_score_u8(md, dd, bank2, gt=gd[:4])


# ------------------------------------------------------------------------------------------------ metrics
def _counts(g, n, npix):
    sp, sg = g.integers(0, npix // 2, n), g.integers(0, npix // 2, n)
    inter = (g.random(n) * np.minimum(sp, sg)).astype(np.int64)
    c = np.stack([inter, sp, sg, sp + sg - inter], 1).astype(np.int32)
    c[0] = [0, 0, 40, 40]            # an empty prediction
    c[1] = [0, 30, 0, 30]            # an empty annotation
    c[2] = [0, 0, 0, 0]              # both empty
    c[3] = [77, 77, 77, 77]          # a perfect match
    return c


@pytest.mark.parametrize("n", [5, 300])
def test_frame_metrics_in_fp64(n):
    """Against metrics_reference to 1e-12 relative: the arithmetic is the same fp64 and only the order of the sum over the frames
    differs (n * 2^-53 < 1e-13 for n = 300)."""
    ops = _ops()
    npix = 224 * 224
    c = _counts(np.random.default_rng(n), n + 3, npix)               # three more rows than are scored
    cd = torch.from_numpy(c).to(DEV)
    want = metrics_reference(c[:n], npix)
    acc = ops.frame_metrics(cd, n, npix)
    got = acc.cpu().numpy()
    assert acc.dtype == torch.float64 and acc.shape == (3,) and got[2] == n
    assert np.all(np.abs(got - want) <= 1e-12 * np.abs(want)), (got, want)
    again = ops.frame_metrics(cd, n, npix)
    assert GA.same_bits(acc, again)                                  # two runs: the same bits
    buf = torch.full((3,), 5.0, device=DEV, dtype=torch.float64)
    assert ops.frame_metrics(cd, n, npix, acc=buf).data_ptr() == buf.data_ptr() and GA.same_bits(buf, acc)      # overwrites
    ops.frame_metrics(cd, 4, npix, acc=buf, accumulate=True)                                                    # adds
    want2 = want + metrics_reference(c[:4], npix)
    assert np.all(np.abs(buf.cpu().numpy() - want2) <= 1e-12 * np.abs(want2)) and float(buf[2]) == n + 4
    ops.frame_metrics(cd, 0, npix, acc=buf, accumulate=True)                                                    # no frames: adds nothing
    assert np.all(np.abs(buf.cpu().numpy() - want2) <= 1e-12 * np.abs(want2))
    assert ops.frame_metrics(cd, 0, npix).cpu().tolist() == [0.0, 0.0, 0.0]
    with pytest.raises(RuntimeError):
        ops.frame_metrics(cd, n + 4, npix)
    with pytest.raises(RuntimeError):
        ops.frame_metrics(cd, n, npix, accumulate=True)
    with pytest.raises(RuntimeError):
        ops.frame_metrics(cd, n, npix, acc=torch.zeros(3, device=DEV))


# ------------------------------------------------------------------------------------------------ refusals
SLACK = 256                          # bytes behind every buffer: a pointer moved by a few bytes still reads and writes inside it


def _buffers(entry):
    """Real device buffers for the valid tuple of REFUSALS[entry], each with SLACK bytes behind it."""
    v = REFUSALS[entry][1]
    if entry == "mumpy_clip_window_u8_fwd":
        sizes = {"frames": (v["nframes"] * v["Hs"] * v["Ws"] * 3, torch.uint8), "out": (v["nclips"] * v["T"] * 3 * v["H"] * v["W"], torch.float32),
                 "frame_idx": (v["nclips"] * v["T"], torch.int32), "ytab": (v["H"], torch.int32), "xtab": (v["W"], torch.int32)}
    elif entry == "mumpy_mask_score_u8_fwd":
        sizes = {"mask": (v["nclips"] * v["npix"], torch.uint8), "gt": (v["nbank"] * v["npix"], torch.uint8), "dest": (v["nclips"], torch.int32),
                 "bank": (v["nbank"] * v["npix"], torch.uint8), "counts": (v["nbank"] * 4, torch.int32)}
    else:
        sizes = {"counts": (v["nscored"] * 4, torch.int32), "acc3": (3, torch.float64)}
    assert set(sizes) | set(v) == set(ARGS[entry])
    return {k: torch.zeros(n + SLACK // torch.empty((), dtype=dt).element_size(), device=DEV, dtype=dt) for k, (n, dt) in sizes.items()}


@pytest.mark.parametrize("entry", sorted(REFUSALS))
def test_every_refusal_of_the_header_launches_nothing(entry):
    """The table of tests/test_video_host.py against real buffers: the valid tuples run (rc == 0), every broken one is refused with
    its MUMPY_E* code and a message of its own -- and no buffer changes: nothing was launched."""
    from mumpy_hip.lib import load_library
    bufs = _buffers(entry)
    if "dest" in bufs:
        bufs["dest"].fill_(-1)
    snap = {}

    def before_refusals():
        torch.cuda.synchronize()
        for k, t in bufs.items():
            t.view(torch.uint8).fill_(0x5A)
            snap[k] = t.view(torch.uint8).clone()
    n = sweep_refusals(load_library(), entry, {k: t.data_ptr() for k, t in bufs.items()}, launches=True, before_refusals=before_refusals)
    torch.cuda.synchronize()
    assert n >= 8 and snap and all(torch.equal(t.view(torch.uint8), snap[k]) for k, t in bufs.items())


# ------------------------------------------------------------------------------------------------ end to end
HS, WS, BATCH = 30, 26, 4


@pytest.fixture(scope="module")
def video_model():
    """Seeded weights, the three-view model at T = 3, and ONE graphed predictor for the file (each owns a capture stream and the
    fork/join side streams under it, which come from torch's pool and are never handed back).  thr is the sigmoid of the median
    logit of the first batch, so that the masks hold both values."""
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from mumpy_hip.pipeline import fused_forward
    from mumpy_hip.video import VideoPredictor, batch_plan
    from weight_fill import fill_module_
    ops = _ops()
    enc, dec = fill_module_(Encoder()).eval().to(DEV), fill_module_(Decoder()).eval().to(DEV)
    g = np.random.default_rng(2024)
    frames = {n: g.integers(0, 256, (n, HS, WS, 3), dtype=np.uint8) for n in (7, 5)}
    idx, _ = batch_plan(7, 3, BATCH)
    x = ops.normalize_u8(torch.from_numpy(frames[7]).to(DEV)[torch.from_numpy(idx[0]).long().to(DEV)], size=(224, 224))
    thr = float(torch.sigmoid(fused_forward(enc, dec, x)[0]).median())
    assert 0.0 < thr < 1.0
    graphed = VideoPredictor(enc, dec, T=3, src_hw=(HS, WS), batch=BATCH, max_frames=16, thr=thr, graph=True)
    eager = VideoPredictor(enc, dec, T=3, src_hw=(HS, WS), batch=BATCH, max_frames=16, thr=thr, graph=False)
    return {"enc": enc, "dec": dec, "thr": thr, "frames": frames, "graphed": graphed, "eager": eager}


def _run(vp, frames, gt=None):
    """-> (masks, [(logits, mask) per batch]) of one predict, cloned."""
    seen = []
    masks = vp.predict(frames, gt, on_batch=lambda b, logits, mask: seen.append((b, logits.clone(), mask.clone())))
    torch.cuda.synchronize()
    assert [b for b, _, _ in seen] == list(range(len(seen)))
    return masks.clone(), [(lg, m) for _, lg, m in seen]


def _expect(vm, frames):
    """fused_forward on the same clip batches in the same order -> ([(logits, mask) per batch], masks (N, 224, 224) 0 / 255)."""
    from mumpy_hip.pipeline import fused_forward
    from mumpy_hip.video import batch_plan
    ops = _ops()
    n = len(frames)
    idx, dest = batch_plan(n, 3, BATCH)
    fd = torch.from_numpy(frames).to(DEV)
    per, masks = [], torch.zeros(n, 224, 224, dtype=torch.uint8, device=DEV)
    for b in range(idx.shape[0]):
        x = ops.normalize_u8(fd[torch.from_numpy(idx[b]).long().to(DEV)], size=(224, 224))
        logits, mask, _ = fused_forward(vm["enc"], vm["dec"], x, with_mask=True, thr=vm["thr"])
        per.append((logits.clone(), mask.clone()))
        for c, d in enumerate(dest[b].tolist()):
            if d >= 0:
                masks[d] = mask[c, 0] * 255
    torch.cuda.synchronize()
    return per, masks


def _same(got, want):
    assert len(got) == len(want)
    for (lg, m), (wl, wm) in zip(got, want):
        assert GA.same_bits(lg, wl) and GA.same_bits(m, wm)


def test_video_predictor_end_to_end(video_model, tmp_path):
    vm, vp, eager = video_model, video_model["graphed"], video_model["eager"]
    f7, f5 = vm["frames"][7], vm["frames"][5]
    gt = (np.random.default_rng(9).integers(0, 3, (7, 224, 224)) * 100).astype(np.uint8)
    gt[6] = 0                                                        # one frame without annotation
    want_per, want_masks = _expect(vm, f7)
    assert len(want_per) == 2                                        # one full batch, then a tail of 3 plus a padding clip

    masks, per = _run(vp, torch.from_numpy(f7), torch.from_numpy(gt))
    graph = vp.graph
    _same(per, want_per)
    assert masks.shape == (7, 224, 224) and masks.dtype == torch.uint8 and masks.is_cuda and GA.same_bits(masks, want_masks)
    values = np.unique(masks.cpu().numpy())
    assert values.tolist() == [0, 255]                               # both occur (thr is the median logit's sigmoid)
    want_metric = masks_metrics_reference(masks.cpu().numpy(), gt)
    got_metric = vp.metric_vector().cpu().numpy()
    assert got_metric[2] == 7                                        # the padding clip is not counted
    assert np.all(np.abs(got_metric - want_metric) <= 1e-12 * np.abs(want_metric)), (got_metric, want_metric)

    # graph=False: the same three steps, the same bits
    masks_e, per_e = _run(eager, torch.from_numpy(f7).to(DEV), torch.from_numpy(gt).to(DEV))      # (frames already on the device)
    _same(per_e, per)
    assert GA.same_bits(masks_e, masks) and GA.same_bits(eager.metric_vector(), vp.metric_vector())

    # a second video through the same predictor: the replay follows the uploaded tables; without gt nothing is scored
    want_per5, want_masks5 = _expect(vm, f5)
    masks5, per5 = _run(vp, f5)                                      # (numpy frames)
    _same(per5, want_per5)
    assert masks5.shape == (5, 224, 224) and GA.same_bits(masks5, want_masks5) and vp.graph is graph
    assert not GA.same_bits(masks5, masks[:5])
    assert GA.same_bits(vp.metric_vector(), eager.metric_vector())
    # ... with gt the accumulator runs across the videos, until it is reset
    vp.predict(f5, gt[:5])
    both = want_metric + masks_metrics_reference(masks5.cpu().numpy(), gt[:5])
    got = vp.metric_vector().cpu().numpy()
    assert got[2] == 12 and np.all(np.abs(got - both) <= 1e-12 * np.abs(both))
    from mumpy_hip.evaluate import finalize_metrics
    f1, iou, cnt = finalize_metrics(vp.metric_vector())
    assert cnt == 12 and abs(f1 - both[0] / 12) < 1e-12 and abs(iou - both[1] / 12) < 1e-12
    vp.reset_metrics()
    assert vp.metric_vector().cpu().tolist() == [0.0, 0.0, 0.0]

    # the files test.py:109-111 writes
    from PIL import Image
    vp.write_masks(str(tmp_path), [3, 4, 10, 11, 12])
    assert sorted(p.name for p in tmp_path.iterdir()) == ["%04d_instance_00.png" % f for f in (3, 4, 10, 11, 12)]
    assert np.array_equal(np.array(Image.open(tmp_path / "0010_instance_00.png")), masks5[2].cpu().numpy())

    # refusals, before anything is launched
    bank = vp.bank.clone()
    for bad in (np.zeros((17, HS, WS, 3), np.uint8), np.zeros((0, HS, WS, 3), np.uint8), np.zeros((5, HS + 1, WS, 3), np.uint8),
                np.zeros((5, HS, WS, 3), np.float32), np.zeros((5, HS, WS), np.uint8)):
        with pytest.raises(ValueError):
            vp.predict(bad)
    with pytest.raises(ValueError):
        vp.predict(f5, gt[:4])
    torch.cuda.synchronize()
    assert GA.same_bits(vp.bank, bank)
    from mumpy_hip.video import VideoPredictor
    for T in (5, 2):                                                 # not the encoder's T; even
        with pytest.raises(ValueError):
            VideoPredictor(vm["enc"], vm["dec"], T=T, src_hw=(HS, WS), graph=False)


def test_video_predictor_follows_load_state_dict(video_model):
    from weight_fill import fill_state_dict_
    vm, vp, enc = video_model, video_model["graphed"], video_model["enc"]
    f5 = vm["frames"][5]
    old = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    before, per_before = _run(vp, f5)
    try:
        enc.load_state_dict(fill_state_dict_({k: v.clone() for k, v in old.items()}, salt="other"), strict=True)
        want_per, want_masks = _expect(vm, f5)
        after, per = _run(vp, f5)
        _same(per, want_per)
        assert GA.same_bits(after, want_masks)
        assert not GA.same_bits(per[0][0], per_before[0][0])
    finally:
        enc.load_state_dict(old, strict=True)
    again, per_again = _run(vp, f5)
    _same(per_again, per_before)
    assert GA.same_bits(again, before)
