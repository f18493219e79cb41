"""GPU: mask cleaning on the device (ops.mask_clean_u8; csrc/mask_clean.hip; include/mumpy_postprocess.h) and
VideoPredictor(clean=...).

The oracle is the numpy statement mumpy_hip.postprocess.clean, which tests/test_postprocess_host.py holds to scipy.ndimage and to
tests/golden/mask_clean.npz.  Every comparison is torch.equal / array_equal.

One stack per size holds every pattern of tests/golden/gen_mask_clean_goldens.py twice, under two different rows of ROWS, so one launch
mixes connectivities, thresholds, a connectivity word that is neither 4 nor 8 and INT32_MIN / INT32_MAX thresholds.  The sizes are the
smallest at which the kernel takes another path: 1x16 and 2x8 (one pixel per lane, rows without a row above / of 8), 16x16, 5x48,
48x35 (two pixels per lane: the chunk links; W no multiple of the wave size) and 224x224 (49 pixels per lane, 100,352 B of LDS, the
raised dynamic-LDS cap).  The numpy results of a size are computed once and shared."""
import functools

import numpy as np
import pytest
import torch

import guarded_alloc as GA
from gen_mask_clean_goldens import PATTERNS, SIZES, pattern, size_key
from mumpy_hip import postprocess as P

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1
GRID = 256                                                   # the launch's grid cap: a stack above it walks the images grid-stride


def _rows(hw):
    """{min_area, max_hole, connectivity word}: both connectivities under every setting of the host test, words that are neither 4 nor
    8 (they mean 8), and the int32 extremes (nothing removed + every hole of any size; everything removed)."""
    n = hw[0] * hw[1]
    return [(0, 0, 8), (1, 0, 4), (2, 48, 8), (20, 50, 4), (n, -1, 8), (0, -1, 4), (2, 3, 6), (I32_MIN, I32_MAX, 4), (I32_MAX, I32_MIN, 8),
            (3, -1, -7), (0, -1, 8), (5, 5, 4), (2, 48, 4), (20, 50, 8), (0, -1, I32_MAX), (2, 1, 0), (n, -1, 4)]


def _ops():
    from mumpy_hip import ops
    return ops


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                    # a copy: the shared cases are read-only


@functools.lru_cache(maxsize=None)
def _case(hw):
    """-> masks (2 * npat, H, W), gt, rows (.., 4) int32, and the numpy statement's out, counts, stats.  Read-only."""
    rows = _rows(hw)
    names = list(PATTERNS) * 2
    masks = np.stack([pattern(name, hw, seed=k) for k, name in enumerate(names)])
    params = np.array([rows[(k + 7 * (k // len(PATTERNS))) % len(rows)] + (0,) for k in range(len(names))], np.int64).astype(np.int32)
    g = np.random.default_rng(hw[0] * 7 + hw[1])
    gt = (g.integers(0, 3, masks.shape) * 100).astype(np.uint8)
    gt[1] = 0
    res = [P.clean(m, int(r[0]), int(r[1]), int(r[2])) for m, r in zip(masks, params)]
    out = np.stack([r[0] for r in res])
    stats = np.stack([r[1] for r in res])
    counts = np.stack([P.counts_row(o, t) for o, t in zip(out, gt)])
    for a in (masks, gt, params, out, counts, stats):
        a.setflags(write=False)
    return masks, gt, params, out, counts, stats


@pytest.mark.parametrize("hw", SIZES, ids=size_key)
def test_one_launch_of_mixed_rows_is_the_numpy_statement(hw):
    ops = _ops()
    masks, gt, params, want, want_counts, want_stats = _case(hw)
    assert {4, 8} < set(params[:, 2].tolist()) and I32_MIN in params[:, :2] and I32_MAX in params[:, :2]
    src, dgt, rows = _dev(masks), _dev(gt), _dev(params)
    out, counts, stats = ops.mask_clean_u8(src, rows, gt=dgt)
    torch.cuda.synchronize()
    assert out.shape == src.shape and out.dtype == torch.uint8 and counts.shape == (len(masks), 4) and stats.shape == (len(masks), 8)
    got, got_stats = out.cpu().numpy(), stats.cpu().numpy()
    assert (got_stats[:, 7] == 0).all(), f"status column {got_stats[:, 7].tolist()}: a loop bound was reached"
    bad = [(i, (PATTERNS * 2)[i], params[i].tolist()) for i in range(len(masks)) if not np.array_equal(got[i], want[i])]
    assert not bad, f"{hw}: images {bad} differ from the numpy statement"
    assert torch.equal(out, _dev(want)) and torch.equal(stats, _dev(want_stats)), (got_stats, want_stats)
    assert torch.equal(counts, _dev(want_counts))
    assert np.array_equal(src.cpu().numpy(), masks) and np.array_equal(dgt.cpu().numpy(), gt)
    assert want.any() and (want != (masks != 0) * 255).any()                                  # the stack is no identity


@pytest.mark.parametrize("hw", SIZES, ids=size_key)
def test_in_place_gives_the_same_bytes_and_host_rows_are_uploaded(hw):
    ops = _ops()
    masks, gt, params, want, _, want_stats = _case(hw)
    src = _dev(masks)
    out, stats = ops.mask_clean_u8(src, params.copy(), out=src)                                        # host rows; no gt: no counts
    assert out is src and torch.equal(src, _dev(want)) and torch.equal(stats, _dev(want_stats))


def test_a_stack_above_the_grid_walks_grid_stride():
    ops = _ops()
    hw, n = (1, 16), 3 * GRID + 5
    g = np.random.default_rng(5)
    masks = ((g.random((n, *hw)) < 0.6) * 255).astype(np.uint8)
    rows = _rows(hw)
    params = np.array([rows[k % len(rows)] + (0,) for k in range(n)], np.int64).astype(np.int32)
    gt = (g.integers(0, 2, masks.shape) * 255).astype(np.uint8)
    res = [P.clean(m, int(r[0]), int(r[1]), int(r[2])) for m, r in zip(masks, params)]
    assert ops._lib().mumpy_mask_clean_workspace_bytes(n, *hw) == GRID * 16 * 4                # the grid is capped, the walk is not
    out, counts, stats = ops.mask_clean_u8(_dev(masks), params, gt=_dev(gt))
    assert torch.equal(out, _dev(np.stack([r[0] for r in res]))) and torch.equal(stats, _dev(np.stack([r[1] for r in res])))
    assert torch.equal(counts, _dev(np.stack([P.counts_row(r[0], t) for r, t in zip(res, gt)])))


@pytest.mark.parametrize("hw", [(5, 48), (48, 35)], ids=size_key)
def test_memory_discipline(monkeypatch, hw):
    """tests/guarded_alloc.py on the entry itself, every buffer and the workspace in a guarded block: the bands stay intact, every
    byte of out, counts and stats is written (under two different fill bytes), mask, gt and params are bitwise unchanged, and the
    runs agree bit for bit."""
    ops = _ops()
    masks, gt, params, want, want_counts, want_stats = _case(hw)
    n = len(masks)
    need = ops._lib().mumpy_mask_clean_workspace_bytes(n, *hw)
    assert need == n * hw[0] * hw[1] * 4

    def body(guard):
        src, dgt, rows = guard.tensor(torch.from_numpy(masks.copy())), guard.tensor(torch.from_numpy(gt.copy())), \
            guard.tensor(torch.from_numpy(params.copy()))
        out = guard.torch.empty(masks.shape, dtype=torch.uint8, device=DEV)
        counts = guard.torch.empty((n, 4), dtype=torch.int32, device=DEV)
        stats = guard.torch.empty((n, 8), dtype=torch.int32, device=DEV)
        ws = guard.torch.empty(need, dtype=torch.uint8, device=DEV)
        ops._call("mumpy_mask_clean_u8_fwd", ops._p(src), ops._p(out), ops._p(dgt), ops._p(counts), ops._p(stats), ops._p(rows),
                  ops._p(ws), need, n, hw[0], hw[1], ops._stream())
        return {"out": out, "counts": counts, "stats": stats}, (), None
    runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set() and len(runs) == len(GA.PASSES)
    for outs in runs:
        assert np.array_equal(outs["out"].cpu().numpy(), want) and np.array_equal(outs["counts"].cpu().numpy(), want_counts) and \
            np.array_equal(outs["stats"].cpu().numpy(), want_stats)


def test_sentinels_in_out_are_overwritten_and_two_runs_agree():
    ops = _ops()
    hw = (16, 16)
    masks, gt, params, want, want_counts, want_stats = _case(hw)
    src, dgt, rows = _dev(masks), _dev(gt), _dev(params)
    ws = ops.mask_clean_workspace(len(masks), *hw, DEV)
    got = []
    for sentinel in (0xA5, 0x5A):
        out = torch.full(src.shape, sentinel, dtype=torch.uint8, device=DEV)
        counts = torch.full((len(masks), 4), sentinel, dtype=torch.int32, device=DEV)
        stats = torch.full((len(masks), 8), sentinel, dtype=torch.int32, device=DEV)
        ws.fill_(sentinel)                                                                     # the kernel zeroes what it needs itself
        ops.mask_clean_u8(src, rows, out=out, gt=dgt, counts=counts, stats=stats, workspace=ws)
        assert np.array_equal(out.cpu().numpy(), want) and np.array_equal(counts.cpu().numpy(), want_counts) and \
            np.array_equal(stats.cpu().numpy(), want_stats), hex(sentinel)
        got.append((out, counts, stats))
    assert all(torch.equal(a, b) for a, b in zip(*got)) and np.array_equal(src.cpu().numpy(), masks)


def test_a_captured_launch_follows_later_rows_and_masks():
    """Rows and mask are rewritten on the device before the replay, which follows them.  (Captured as tests/test_geometric.py does
    it: on a stream of the high-priority pool.)"""
    ops = _ops()
    hw = (48, 35)
    masks, _, params, want, _, want_stats = _case(hw)
    n = len(PATTERNS)
    src, rows = _dev(masks[:n]), _dev(params[:n])
    out = torch.empty_like(src)
    stats = torch.empty(n, 8, dtype=torch.int32, device=DEV)
    ws = ops.mask_clean_workspace(n, *hw, DEV)
    ops.mask_clean_u8(src, rows, out=out, stats=stats, workspace=ws)
    assert np.array_equal(out.cpu().numpy(), want[:n])
    side = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        ops.mask_clean_u8(src, rows, out=out, stats=stats, workspace=ws)
        graph.capture_end()
    src.copy_(_dev(masks[n:]))
    rows.copy_(_dev(params[n:]))
    out.fill_(9)
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want[n:]) and np.array_equal(stats.cpu().numpy(), want_stats[n:])
    assert not np.array_equal(want[n:], want[:n])


def test_the_counts_feed_frame_metrics_like_mask_score_of_the_cleaned_mask():
    ops = _ops()
    hw = (48, 35)
    masks, gt, params, want, _, _ = _case(hw)
    n, npix = len(masks), hw[0] * hw[1]
    _, counts, _ = ops.mask_clean_u8(_dev(masks), params.copy(), gt=_dev(gt))
    got = ops.frame_metrics(counts, n, npix)
    dest = torch.arange(n, dtype=torch.int32, device=DEV)
    bank = torch.zeros(n, npix, dtype=torch.uint8, device=DEV)
    _, ref_counts = ops.mask_score_u8(_dev((want != 0).astype(np.uint8)), dest, bank, gt=_dev(gt).view(n, npix))
    assert torch.equal(counts, ref_counts) and torch.equal(bank.view(n, *hw), _dev(want))
    assert GA.same_bits(got, ops.frame_metrics(ref_counts, n, npix))


def test_the_wrapper_refuses_before_launch():
    ops = _ops()
    hw = (16, 16)
    masks, gt, params, _, _, _ = _case(hw)
    n = len(masks)
    src, dgt, rows = _dev(masks), _dev(gt), _dev(params)
    for bad in (src.cpu(), src.float(), src[:, :, :8], src[0], masks):
        with pytest.raises(RuntimeError):
            ops.mask_clean_u8(bad, rows)
    both = torch.zeros(src.numel() + 256, dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match="overlaps"):                                        # out is mask shifted by one image
        ops.mask_clean_u8(both[:src.numel()].view(src.shape), rows, out=both[256:].view(src.shape))
    with pytest.raises(RuntimeError, match=rf"\({n}, 4\)"):
        ops.mask_clean_u8(src, torch.zeros(n, 4, dtype=torch.int64, device=DEV))
    with pytest.raises(RuntimeError, match=rf"\({n}, 4\)"):
        ops.mask_clean_u8(src, torch.zeros(n - 1, 4, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match=rf"\({n}, 4\)"):
        ops.mask_clean_u8(src, np.zeros((n, 8), np.int32))
    with pytest.raises(RuntimeError, match="counts= needs gt"):
        ops.mask_clean_u8(src, rows, counts=torch.zeros(n, 4, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError):
        ops.mask_clean_u8(src, rows, gt=dgt[:-1])
    with pytest.raises(RuntimeError):
        ops.mask_clean_u8(src, rows, stats=torch.zeros(n, 4, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match="workspace"):
        ops.mask_clean_u8(src, rows, workspace=torch.zeros(64, dtype=torch.uint8, device=DEV))
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops.mask_clean_u8(torch.zeros(2, 3, 5, dtype=torch.uint8, device=DEV), np.zeros((2, 4), np.int32))
    with pytest.raises(RuntimeError, match="pixels"):
        ops.mask_clean_u8(torch.zeros(1, 224, 225, dtype=torch.uint8, device=DEV), np.zeros((1, 4), np.int32))
    with pytest.raises(RuntimeError, match="hw="):
        ops.mask_clean_u8(src.view(n, 256), rows, hw=(16, 15))
    odd = torch.zeros(n * 4 + 4, dtype=torch.int32, device=DEV)[1:n * 4 + 1].view(n, 4)       # 4 bytes off a 16-byte boundary
    with pytest.raises(RuntimeError, match="aligned"):
        ops.mask_clean_u8(src, odd)
    flat, _ = ops.mask_clean_u8(src.view(n, 256), rows, hw=hw)                                 # the bank's layout
    assert flat.shape == (n, 256) and torch.equal(flat.view(src.shape), ops.mask_clean_u8(src, rows)[0])
    p = ops.mask_clean_params(dict(min_area=3, max_hole=-1, connectivity=4), 5, DEV)
    assert p.dtype == torch.int32 and p.cpu().tolist() == [[3, -1, 4, 0]] * 5
    assert ops.mask_clean_params((2, 48), 2, DEV).cpu().tolist() == [[2, 48, 8, 0]] * 2
    assert ops.mask_clean_params([(2, 48, 4), dict(min_area=1, max_hole=0)], 2, DEV).cpu().tolist() == [[2, 48, 4, 0], [1, 0, 8, 0]]
    with pytest.raises(RuntimeError, match="3 images"):
        ops.mask_clean_params([(2, 48, 4)], 3, DEV)
    with pytest.raises(ValueError):
        ops.mask_clean_params((2, 48, 5), 3, DEV)


# ------------------------------------------------------------------------------------------------ the predictor
HS, WS, BATCH, NF = 30, 26, 4, 7
CLEAN = dict(min_area=20, max_hole=50, connectivity=8)


@pytest.fixture(scope="module")
def predictors():
    """Seeded weights and two eager predictors that differ in clean= alone (built as tests/test_video_stage.py builds its model);
    thr is the sigmoid of the median logit of the first batch, so that the masks hold both values in small pieces."""
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from mumpy_hip.pipeline import fused_forward
    from mumpy_hip.video import VideoPredictor, batch_plan
    from weight_fill import fill_module_
    ops = _ops()
    enc, dec = fill_module_(Encoder()).eval().to(DEV), fill_module_(Decoder()).eval().to(DEV)
    g = np.random.default_rng(77)
    frames = g.integers(0, 256, (NF, HS, WS, 3), dtype=np.uint8)
    gt = (g.integers(0, 3, (NF, 224, 224)) * 100).astype(np.uint8)
    idx, _ = batch_plan(NF, 3, BATCH)
    x = ops.normalize_u8(torch.from_numpy(frames).to(DEV)[torch.from_numpy(idx[0]).long().to(DEV)], size=(224, 224))
    thr = float(torch.sigmoid(fused_forward(enc, dec, x)[0]).median())
    kw = dict(T=3, src_hw=(HS, WS), batch=BATCH, max_frames=8, thr=thr, graph=False)
    return {"raw": VideoPredictor(enc, dec, **kw), "clean": VideoPredictor(enc, dec, clean=CLEAN, **kw), "frames": frames, "gt": gt,
            "enc": enc, "dec": dec, "kw": kw}


def test_the_predictor_cleans_after_the_last_batch_and_leaves_the_raw_results_alone(predictors, tmp_path):
    from test_video_host import masks_metrics_reference
    raw, vp, frames, gt = predictors["raw"], predictors["clean"], predictors["frames"], predictors["gt"]
    assert NF % BATCH != 0
    raw.reset_metrics(), vp.reset_metrics()
    raw_masks = raw.predict(frames, gt).clone()
    cleaned = vp.predict(frames, gt)
    torch.cuda.synchronize()
    # the raw side is bit for bit the clean=None predictor's
    assert GA.same_bits(vp.bank, raw.bank) and GA.same_bits(vp.counts, raw.counts) and GA.same_bits(vp.metric_vector(), raw.metric_vector())
    # the cleaned masks are the numpy statement on the raw bank
    res = [P.clean(m, CLEAN["min_area"], CLEAN["max_hole"], CLEAN["connectivity"]) for m in raw_masks.cpu().numpy()]
    want, want_stats = np.stack([r[0] for r in res]), np.stack([r[1] for r in res])
    assert cleaned.shape == (NF, 224, 224) and cleaned.data_ptr() == vp.clean_bank.data_ptr()
    assert np.array_equal(cleaned.cpu().numpy(), want) and not np.array_equal(want, raw_masks.cpu().numpy())
    assert np.array_equal(vp.clean_statistics().cpu().numpy(), want_stats)
    assert np.array_equal(vp.clean_counts[:NF].cpu().numpy(), np.stack([P.counts_row(o, t) for o, t in zip(want, gt)]))
    want_metric = masks_metrics_reference(want, gt)
    got_metric = vp.metric_vector(clean=True).cpu().numpy()
    assert got_metric[2] == NF and np.all(np.abs(got_metric - want_metric) <= 1e-12 * np.abs(want_metric)), (got_metric, want_metric)
    assert not GA.same_bits(vp.metric_vector(clean=True), vp.metric_vector())
    # without annotations nothing is scored; a shorter video gives a shorter table
    before = vp.metric_vector(clean=True).clone()
    short = vp.predict(frames[:3])
    torch.cuda.synchronize()
    assert short.shape == (3, 224, 224) and vp.clean_statistics().shape == (3, 8) and GA.same_bits(vp.metric_vector(clean=True), before)
    # saved masks: the cleaned ones by default, the raw ones on request
    from PIL import Image
    vp.write_masks(str(tmp_path / "c"), [1, 2, 3])
    vp.write_masks(str(tmp_path / "r"), [1, 2, 3], clean=False)
    assert np.array_equal(np.array(Image.open(tmp_path / "c" / "0002_instance_00.png")), short[1].cpu().numpy())
    assert np.array_equal(np.array(Image.open(tmp_path / "r" / "0002_instance_00.png")), vp.bank[1].view(224, 224).cpu().numpy())
    vp.reset_metrics()
    assert vp.metric_vector(clean=True).cpu().tolist() == [0.0, 0.0, 0.0] and vp.metric_vector().cpu().tolist() == [0.0, 0.0, 0.0]


def test_clean_none_is_the_predictor_as_it_was(predictors, monkeypatch):
    from mumpy_hip.video import VideoPredictor
    ops = _ops()
    raw, vp = predictors["raw"], predictors["clean"]
    assert raw.clean is None
    for name in ("clean_bank", "clean_counts", "clean_stats", "clean_acc", "_clean_params", "_clean_ws"):
        assert not hasattr(raw, name) and hasattr(vp, name), name
    assert vp.clean_bank.shape == (8, 224 * 224) and vp.clean_counts.shape == (8, 4) and vp.clean_stats.shape == (8, 8) and \
        vp.clean_acc.shape == (3,) and vp.clean_acc.dtype == torch.float64
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a, **kw: (calls.append(name), real(name, *a, **kw))[1])
    raw.predict(predictors["frames"], predictors["gt"])
    was = [c for c in calls if "clean" in c or "frame_metrics" in c]
    del calls[:]
    vp.predict(predictors["frames"], predictors["gt"])
    torch.cuda.synchronize()
    now = [c for c in calls if "clean" in c or "frame_metrics" in c]
    assert was == ["mumpy_frame_metrics_fwd"] and now == ["mumpy_frame_metrics_fwd", "mumpy_mask_clean_u8_fwd", "mumpy_frame_metrics_fwd"]
    for call in (raw.clean_statistics, lambda: raw.metric_vector(clean=True), lambda: raw.write_masks("unused", [1], clean=True)):
        with pytest.raises(RuntimeError, match="without clean="):
            call()
    for bad in (dict(min_area=224 * 224 + 1, max_hole=0), dict(min_area=2, max_hole=0, connectivity=6), dict(min_area=2.5, max_hole=0),
                (20, 50), dict(min_area=2)):
        with pytest.raises(ValueError, match="VideoPredictor: clean"):
            VideoPredictor(predictors["enc"], predictors["dec"], clean=bad, **predictors["kw"])
