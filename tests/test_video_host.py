"""CPU only: the host half of whole-video inference (mumpy_hip/video.py, include/mumpy_hip_ext5.h).

  * clip_frame_indices is the comprehension of the reference's loader (dataloaders/universaldataloader.py:41-46), its centre column is
    the frame itself, an even T is refused; batch_plan pads the tail with valid clips whose dest is -1;
  * the header declares exactly the three entries and its version function, with the pinned argument names;
  * `window_reference`, `score_reference` and `metrics_reference`, the numpy statements of the three kernels written here from
    universaldataset.py:75-79 (PIL NEAREST) + test.py:22-25, test.py:100-111 and measure.py:57-62, 86-89 (tests/test_video_stage.py
    holds the kernels to them), checked on hand-made cases;
  * every refusal named in the header, with nothing launched (sign convention of tests/test_abi_refusals.py: needs no GPU and must
    not run where one is visible; tests/test_video_stage.py runs the same table against real buffers)."""
import ctypes

import numpy as np
import pytest

from abi_surface import names_of
from conftest import have_gpu

EINVAL, EALIGN, ENULL, ERANGE = -1, -2, -3, -4
EVAL_MEAN, EVAL_STD = (0.4776, 0.479, 0.4465), (0.230, 0.2085, 0.2324)      # test.py:23-24
ARGS = {
    "mumpy_clip_window_u8_fwd": ["frames", "out", "frame_idx", "ytab", "xtab", "nclips", "T", "nframes", "Hs", "Ws", "H", "W", "mean3",
                                 "std3", "stream"],
    "mumpy_mask_score_u8_fwd": ["mask", "gt", "dest", "bank", "counts", "nclips", "npix", "nbank", "stream"],
    "mumpy_frame_metrics_fwd": ["counts", "nscored", "npix", "acc3", "accumulate", "stream"],
}


def V():
    from mumpy_hip import video
    return video


# ------------------------------------------------------------------------------------------------ the numpy statements of the kernels
def nearest_table(src, dst):
    """Pillow's NEAREST source indices (Geometry.c, ImagingScaleAffine: a double accumulator that starts at half a step)."""
    a = src / dst
    xo, tab = a * 0.5, []
    for _ in range(dst):
        tab.append(min(int(xo), src - 1))
        xo += a
    return np.array(tab, np.int64)


def window_reference(frames, frame_idx, size, mean=EVAL_MEAN, std=EVAL_STD):
    """frames (nframes, Hs, Ws, 3) uint8, frame_idx (nclips, T) -> (gathered (nclips, T, H, W, 3) uint8, out (nclips, T, 3, H, W)
    float32): the clamped frame gather, `img.resize(inputRes)` with PIL NEAREST, ToTensor and Normalize, in float32 in that order."""
    frames = np.asarray(frames)
    src = frames[np.clip(np.asarray(frame_idx, np.int64), 0, frames.shape[0] - 1)]
    moved = src[:, :, nearest_table(frames.shape[1], size[0])][:, :, :, nearest_table(frames.shape[2], size[1])]
    m, s = np.asarray(mean, np.float32).reshape(3, 1, 1), np.asarray(std, np.float32).reshape(3, 1, 1)
    out = (np.moveaxis(moved, -1, -3).astype(np.float32) / np.float32(255.0) - m) / s
    return moved, out.astype(np.float32)


def score_reference(mask, dest, bank, gt=None, counts=None):
    """-> (bank, counts) after mumpy_mask_score_u8_fwd: copies of bank (nbank, npix) and counts (nbank, 4) with the rows named by a
    valid dest replaced; every other row as it was."""
    mask = np.asarray(mask).reshape(len(dest), -1)
    bank = np.array(bank, copy=True)
    counts = None if counts is None else np.array(counts, copy=True)
    for c, d in enumerate(np.asarray(dest).tolist()):
        if not 0 <= d < bank.shape[0]:
            continue
        p = mask[c] != 0
        bank[d] = np.where(p, 255, 0)
        if gt is not None:
            g = np.asarray(gt)[d] > 0
            counts[d] = [(p & g).sum(), p.sum(), g.sum(), (p | g).sum()]
    return bank, counts


def metrics_reference(counts, npix):
    """[sum F1, sum IoU, n] in float64 over the rows of counts: measure.py:57-62, 86-89 (recall's denominator is sum(gt + 1e-6) over
    all pixels, as written there)."""
    c = np.asarray(counts, np.float64).reshape(-1, 4)
    inter, sp, sg, union = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    recall = inter / (sg + 1e-6 * npix)
    precision = inter / (sp + 1e-6)
    f1 = 2 * precision * recall / (precision + recall + 1e-6)
    iou = (inter + 1e-5) / (union + 1e-5)
    return np.array([f1.sum(), iou.sum(), float(len(c))], np.float64)


def masks_metrics_reference(pred, gt):
    """metrics_reference of predicted masks (N, ...) (non-zero = forged) against annotations (N, ...) (> 0 = forged)."""
    p, g = np.asarray(pred).reshape(len(pred), -1) != 0, np.asarray(gt).reshape(len(gt), -1) > 0
    counts = np.stack([(p & g).sum(1), p.sum(1), g.sum(1), (p | g).sum(1)], 1)
    return metrics_reference(counts, p.shape[1])


# ------------------------------------------------------------------------------------------------ frame tables
@pytest.mark.parametrize("T", [1, 3, 5, 9])
@pytest.mark.parametrize("N", [1, 2, 3, 7])
def test_clip_frame_indices_are_the_loaders_comprehension(N, T):
    got = V().clip_frame_indices(N, T)
    k = T // 2
    want = [[min(max(j, 0), N - 1) for j in range(i - k, i + k + 1)] for i in range(N)]          # universaldataloader.py:46
    assert got.dtype == np.int32 and got.shape == (N, T) and got.tolist() == want
    assert np.array_equal(got[:, T // 2], np.arange(N))              # the frame the mask belongs to


def test_even_T_is_refused():
    for T in (2, 4, 8):
        with pytest.raises(ValueError):
            V().clip_frame_indices(5, T)
    with pytest.raises(ValueError):
        V().clip_frame_indices(0, 3)
    with pytest.raises(ValueError):
        V().batch_plan(5, 3, 0)


def test_padding_plan_has_every_frame_once():
    idx, dest = V().batch_plan(7, 3, 4)
    assert idx.shape == (2, 4, 3) and dest.shape == (2, 4) and idx.dtype == dest.dtype == np.int32
    valid = dest[dest >= 0]
    assert sorted(valid.tolist()) == list(range(7)) and len(valid) == 7              # exactly 7 valid dest values, each once
    assert dest.reshape(-1).tolist() == [0, 1, 2, 3, 4, 5, 6, -1]
    assert idx.min() >= 0 and idx.max() <= 6                                             # the padding clip's indices are valid
    assert np.array_equal(idx.reshape(-1, 3)[:7], V().clip_frame_indices(7, 3))
    for n, b in ((8, 4), (1, 8), (5, 1)):
        idx, dest = V().batch_plan(n, 5, b)
        assert idx.shape == (-(-n // b), b, 5) and sorted(dest[dest >= 0].tolist()) == list(range(n))
        assert set(dest[dest < 0].tolist()) <= {-1} and 0 <= idx.min() and idx.max() <= n - 1


# ------------------------------------------------------------------------------------------------ the references, by hand
def test_window_reference_by_hand():
    frames = np.arange(3 * 2 * 4 * 3, dtype=np.uint8).reshape(3, 2, 4, 3) * 3
    moved, out = window_reference(frames, [[-5, 0, 1], [1, 2, 99]], (2, 4))
    assert np.array_equal(moved[0], frames[[0, 0, 1]]) and np.array_equal(moved[1], frames[[1, 2, 2]])          # the clamp, identity size
    assert out.shape == (2, 3, 3, 2, 4) and out.dtype == np.float32
    v = frames[2, 1, 3, 1]
    assert out[1, 2, 1, 1, 3] == np.float32((np.float32(v) / np.float32(255) - np.float32(0.479)) / np.float32(0.2085))
    assert nearest_table(4, 2).tolist() == [1, 3] and nearest_table(2, 4).tolist() == [0, 0, 1, 1] and nearest_table(7, 7).tolist() == list(range(7))
    moved, _ = window_reference(frames, [[1]], (4, 2))
    assert np.array_equal(moved[0, 0], frames[1][[0, 0, 1, 1]][:, [1, 3]])


def test_score_and_metrics_references_by_hand():
    npix = 16
    g = np.zeros((4, npix), np.uint8)
    g[0, :4] = 255; g[1, :4] = 1; g[3, :8] = 7
    mask = np.zeros((5, npix), np.uint8)
    mask[1, 2:6] = 1                    # -> frame 1: overlaps the annotation in 2 pixels
    mask[2, :5] = 1                     # -> frame 2: an empty annotation
    mask[3, :8] = 200                   # -> frame 3: a perfect match (any non-zero byte is "forged")
    mask[4, :] = 1                      # dropped: dest -1
    dest = [0, 1, 2, 3, -1]             # clip 0 -> frame 0: an empty prediction
    bank0, counts0 = np.full((4, npix), 9, np.uint8), np.full((4, 4), -7, np.int32)
    bank, counts = score_reference(mask, dest, bank0, g, counts0)
    assert set(np.unique(bank).tolist()) == {0, 255} and bank[3].tolist() == [255] * 8 + [0] * 8
    assert counts.tolist() == [[0, 0, 4, 4], [2, 4, 4, 6], [0, 5, 0, 5], [8, 8, 8, 8]]
    assert (bank0 == 9).all() and (counts0 == -7).all()                               # the reference copies
    b2, c2 = score_reference(mask[:2], [7, -1], bank0, g, counts0)                        # nothing valid: nothing written
    assert np.array_equal(b2, bank0) and np.array_equal(c2, counts0)
    b3, c3 = score_reference(mask, dest, bank0)                                           # no annotation: no counts
    assert c3 is None and np.array_equal(b3, bank)
    per = [metrics_reference(counts[i], npix) for i in range(4)]
    assert per[0][0] == 0.0 and abs(per[0][1] - 1e-5 / (4 + 1e-5)) < 1e-18               # an empty prediction: F1 0
    assert per[2][0] == 0.0 and np.isfinite(per[2]).all() and abs(per[2][1] - 1e-5 / (5 + 1e-5)) < 1e-18     # an empty annotation: F1 0, not NaN
    P, R = 8 / (8 + 1e-6), 8 / (8 + 1e-6 * npix)
    assert abs(per[3][0] - 2 * P * R / (P + R + 1e-6)) < 1e-15 and 0.99999 < per[3][0] < 1.0 and per[3][1] == 1.0   # a perfect match
    P, R = 2 / (4 + 1e-6), 2 / (4 + 1e-6 * npix)
    assert abs(per[1][0] - 2 * P * R / (P + R + 1e-6)) < 1e-15 and abs(per[1][1] - (2 + 1e-5) / (6 + 1e-5)) < 1e-15
    total = metrics_reference(counts, npix)
    assert total[2] == 4.0 and abs(total[0] - sum(p[0] for p in per)) < 1e-15 and abs(total[1] - sum(p[1] for p in per)) < 1e-15
    both_empty = metrics_reference([[0, 0, 0, 0]], npix)
    assert both_empty.tolist() == [0.0, 1.0, 1.0]
    assert np.array_equal(masks_metrics_reference(bank, g), total)


def test_metrics_reference_is_eval_metric_vector():
    """... the formulas as mumpy_hip.distributed.eval_metric_vector already states them."""
    import torch
    from mumpy_hip.distributed import eval_metric_vector
    r = np.random.default_rng(5)
    p, g = r.integers(0, 2, (6, 64)).astype(np.uint8), (r.integers(0, 3, (6, 64)) * 100).astype(np.uint8)
    p[0] = 0; g[1] = 0; p[2] = g[2] > 0
    want = eval_metric_vector(torch.from_numpy(p), torch.from_numpy(g)).numpy()
    got = masks_metrics_reference(p * 255, g)
    assert np.allclose(got, want, rtol=1e-14, atol=0) and got[2] == 6


# ------------------------------------------------------------------------------------------------ the header's pinned names
def test_ext5_header_declares_exactly_the_pinned_names():
    """(tests/test_abi.py holds the header to its binding and to both libraries.)"""
    assert names_of("mumpy_hip_ext5.h") == dict(ARGS, mumpy_ext5_version=[])


# ------------------------------------------------------------------------------------------------ refusals
F3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
Z3 = (ctypes.c_float * 3)(0.5, 0.0, 0.5)
OFF = lambda k: ("off", k)           # the valid pointer moved by k bytes
# entry -> (tag in the message, valid scalars, [further valid tuples], [accepted no-ops], [(code, overrides)])
REFUSALS = {
    "mumpy_clip_window_u8_fwd": (
        b"clip_window_u8", dict(nclips=2, T=3, nframes=3, Hs=5, Ws=7, H=8, W=8, mean3=F3, std3=F3, stream=None),
        [dict(frames=OFF(1), frame_idx=OFF(4), ytab=OFF(4))],                            # bytes / single words: no alignment rule
        [dict(nclips=0)],
        [(ENULL, {p: None}) for p in ("frames", "out", "frame_idx", "ytab", "xtab", "mean3", "std3")]
        + [(EINVAL, {k: v}) for k, v in (("nframes", 0), ("nframes", -1), ("T", 0), ("T", -1), ("Hs", 0), ("Ws", 0), ("H", 0), ("W", 0),
                                         ("Hs", -1), ("W", 6), ("W", 9), ("W", -4), ("nclips", -1), ("std3", Z3))]
        + [(EALIGN, {"out": OFF(4)}), (EALIGN, {"xtab": OFF(4)})]
        + [(ERANGE, {"nframes": 1 << 31}), (ERANGE, {"nclips": 1 << 31}), (ERANGE, {"nclips": 1 << 30}), (ERANGE, {"nclips": 1 << 62}),
           (ERANGE, {"Hs": 26755, "Ws": 26755}), (ERANGE, {"H": 26756, "W": 26756})]),
    "mumpy_mask_score_u8_fwd": (
        b"mask_score_u8", dict(nclips=2, npix=32, nbank=3, stream=None),
        [dict(gt=None, counts=None), dict(dest=OFF(4), counts=OFF(4))],
        [dict(nclips=0)],
        [(ENULL, {p: None}) for p in ("mask", "dest", "bank", "gt", "counts")]           # gt / counts: exactly one of the two given
        + [(EINVAL, {k: v}) for k, v in (("npix", 0), ("npix", 24), ("npix", 40), ("npix", -16), ("nbank", 0), ("nbank", -1), ("nclips", -1))]
        + [(EALIGN, {p: OFF(8)}) for p in ("mask", "bank", "gt")]
        + [(ERANGE, {"nclips": 1 << 31}), (ERANGE, {"nbank": 1 << 31}), (ERANGE, {"npix": 1 << 31})]),
    "mumpy_frame_metrics_fwd": (
        b"frame_metrics", dict(nscored=3, npix=32, accumulate=0, stream=None),
        [dict(accumulate=1), dict(nscored=0), dict(counts=OFF(4))],
        [],
        [(ENULL, {"counts": None}), (ENULL, {"acc3": None}), (EINVAL, {"nscored": -1}), (EINVAL, {"npix": 0}), (EINVAL, {"npix": -1}),
         (EALIGN, {"acc3": OFF(4)}), (ERANGE, {"nscored": 1 << 31}), (ERANGE, {"npix": 1 << 31})]),
}


def sweep_refusals(lib, entry, pointers, launches, before_refusals=None):
    """pointers: {name: address} of the entry's device pointers.  launches: True where a valid call really runs (rc == 0), False where
    it reaches a runtime without a device (rc > 0).  Every refusal must give its code and a message of this call's own.
    before_refusals(): called between the valid calls and the refused ones."""
    tag, scalars, valid, noops, cases = REFUSALS[entry]
    names, fn = ARGS[entry], getattr(lib, entry)
    ok = dict(pointers, **scalars)
    assert set(ok) == set(names)

    def call(over):
        a = dict(ok)
        for k, v in over.items():
            a[k] = ok[k] + v[1] if isinstance(v, tuple) else v
        return int(fn(*[a[k] for k in names]))

    for over in [{}] + valid:
        rc = call(over)
        assert (rc == 0) if launches else (rc > 0), (entry, over, rc, lib.mumpy_last_error())
    if before_refusals is not None:
        before_refusals()
    for over in noops:
        assert call(over) == 0, (entry, over)
    for code, over in cases:
        assert lib.mumpy_add_fwd(None, None, None, 16, None) < 0        # the message is sticky per thread: leave a known one
        stale = lib.mumpy_last_error()
        rc = call(over)
        err = lib.mumpy_last_error()
        assert rc == code and err != stale and tag in err, (entry, over, rc, err)
    return len(cases)


@pytest.mark.skipif(have_gpu(), reason="with a device present a valid tuple of fake addresses would really launch")
@pytest.mark.parametrize("entry", sorted(REFUSALS))
def test_refusals_need_no_gpu(entry):
    """A valid tuple of fake, 16-byte aligned, never dereferenced addresses passes every host check (rc > 0: the launch reaches a
    runtime without a device); the same tuple with one rule broken is refused with the stated code.  mean3 / std3 are real host
    arrays: the entry reads them."""
    from mumpy_hip.lib import load_library
    ptrs = [n for n in ARGS[entry] if n not in REFUSALS[entry][1]]
    assert sweep_refusals(load_library(), entry, {p: 0x100000 * (i + 1) for i, p in enumerate(ptrs)}, launches=False) >= 8
