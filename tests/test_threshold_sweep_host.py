"""CPU only: the host half of scoring a video at every mask threshold in one pass (mumpy_hip/video.py::sweep_table / exceed_counts,
mumpy_hip/evaluate.py::finalize_sweep, include/mumpy_hip_ext7.h).

  * `exceed_reference` and `sweep_reference`, the numpy statements of the two kernels, checked by hand on a 16-pixel case (a pixel
    whose probability EQUALS a threshold does not exceed it; an all-background frame).  exceed_reference takes float32
    probabilities, not logits: __expf is the device's (tests/test_threshold_sweep.py holds the kernel to code that runs there);
  * exceed_counts at every k is {inter, sum p, sum g, union} of thresholding the probabilities directly;
  * sweep_table: the default values bitwise, every refusal;
  * finalize_sweep: the means, the tie rule of `best`, an AUC of exactly 1.0, 0.5 and 0.0, nan with an empty class;
  * the header declares exactly the two entries and its version function, with the pinned argument names and limit;
  * every refusal named in the header, with nothing launched (sign convention of tests/test_abi_refusals.py: needs no GPU and must
    not run where one is visible; tests/test_threshold_sweep.py runs the same table against real buffers);
  * the two ops wrappers under tests/handoff_audit.py's recorder: a valid call hands exactly the buffers given, a shorter exceed, a
    wrong dtype and a non-contiguous in-place buffer are refused before the first launch;
  * VideoPredictor(sweep=...) refuses a bad table before it looks for a device."""
import types

import numpy as np
import pytest
import torch

import handoff_audit as HA
import test_video_host as TVH
from abi_surface import define, names_of
from conftest import have_gpu
from test_video_host import metrics_reference, sweep_refusals

EINVAL, EALIGN, ENULL, ERANGE = -1, -2, -3, -4
KMAX = 1023
ARGS = {
    "mumpy_score_exceed_fwd": ["logits", "gt", "dest", "thr_tab", "exceed", "nclips", "npix", "nbank", "K", "stream"],
    "mumpy_sweep_metrics_fwd": ["exceed", "nscored", "npix", "K", "acc", "pooled", "accumulate", "stream"],
}


def V():
    from mumpy_hip import video
    return video


# ------------------------------------------------------------------------------------------------ the numpy statements of the kernels
def exceed_reference(p, gt, dest, table, exceed):
    """-> exceed after mumpy_score_exceed_fwd: a copy of exceed (nbank, 2, K + 1) with the rows named by a valid dest replaced, every
    other row as it was.  p (nclips, npix) float32 PROBABILITIES; the comparison is the strict float32 `>` (NaN exceeds nothing)."""
    p = np.asarray(p, np.float32).reshape(len(dest), -1)
    table = np.asarray(table, np.float32)
    out, K = np.array(exceed, copy=True), len(table)
    assert out.shape[1:] == (2, K + 1)
    for c, d in enumerate(np.asarray(dest).tolist()):
        if not 0 <= d < out.shape[0]:
            continue
        g = np.asarray(gt)[d] > 0
        for cls in (0, 1):
            sel = p[c][g == bool(cls)]
            with np.errstate(invalid="ignore"):
                out[d, cls, :K] = (sel[:, None] > table[None, :]).sum(0)
            out[d, cls, K] = sel.size
    return out


def sweep_reference(exceed, npix):
    """-> (acc (K, 3) float64, pooled (2, K + 1) int64) of mumpy_sweep_metrics_fwd over all rows of exceed: metrics_reference of
    exceed_counts per threshold, and the column sums."""
    exceed = np.asarray(exceed)
    K = exceed.shape[2] - 1
    acc = np.stack([metrics_reference(V().exceed_counts(exceed, k), npix) for k in range(K)]) if len(exceed) else \
        np.zeros((K, 3), np.float64)
    return acc, exceed.astype(np.int64).sum(0)


def direct_counts(p, g, t):
    """{inter, sum p, sum g, union} per row of thresholding the probabilities p (n, npix) at t against g (n, npix) > 0."""
    with np.errstate(invalid="ignore"):
        m = np.asarray(p, np.float32) > np.float32(t)
    g = np.asarray(g) > 0
    return np.stack([(m & g).sum(1), m.sum(1), g.sum(1), (m | g).sum(1)], 1).astype(np.int64)


# ------------------------------------------------------------------------------------------------ the references, by hand
TABLE3 = np.array([0.25, 0.5, 0.75], np.float32)


def test_exceed_and_sweep_references_by_hand():
    npix = 16
    gt = np.zeros((3, npix), np.uint8)
    gt[0, :4] = 255; gt[0, 4:6] = 1                   # frame 0: six forged pixels
    gt[1, :] = 0                                      # frame 1: all background
    p = np.zeros((3, npix), np.float32)
    #           forged:  > all   == .5   == .75  < all   > .25   nan        background: > all, == .25, > .5, rest 0
    p[0, :10] = [0.9, 0.5, 0.75, 0.1, 0.3, np.nan, 0.8, 0.25, 0.6, 0.0]
    p[1, :3] = [0.3, 0.6, 1.0]                        # -> frame 1
    p[2, :] = 1.0                                     # dropped: dest -1
    sentinel = np.full((3, 2, 4), -7, np.int32)
    got = exceed_reference(p, gt, [0, 1, -1], TABLE3, sentinel)
    # frame 0, forged {.9, .5, .75, .1, .3, nan}: > .25: .9 .5 .75 .3 = 4; > .5: .9 .75 = 2 (.5 itself is not exceeded); > .75: .9 = 1
    # frame 0, background {.8, .25, .6, 0 x 7}: > .25: .8 .6 = 2 (.25 itself is not); > .5: 2; > .75: 1
    assert got[0].tolist() == [[2, 2, 1, 10], [4, 2, 1, 6]]
    assert got[1].tolist() == [[3, 2, 1, 16], [0, 0, 0, 0]]                               # all background: class 1 is empty
    assert (got[2] == -7).all() and (sentinel == -7).all()                                # no dest names row 2; the reference copies
    assert np.array_equal(exceed_reference(p, gt, [7, -1, 3], TABLE3, sentinel), sentinel)        # nothing valid: nothing written
    c = V().exceed_counts(got[:2], 1)                                                     # thr 0.5
    assert c.tolist() == [[2, 4, 6, 8], [0, 2, 0, 2]] and c.dtype == np.int64
    for k, t in enumerate(TABLE3):
        assert np.array_equal(V().exceed_counts(got[:2], k), direct_counts(p[:2], gt[:2], t))
    acc, pooled = sweep_reference(got[:2], npix)
    assert acc.shape == (3, 3) and pooled.dtype == np.int64 and pooled.tolist() == [[5, 4, 2, 26], [4, 2, 1, 6]]
    P, R = 2 / (4 + 1e-6), 2 / (6 + 1e-6 * npix)                                          # frame 0 at 0.5; frame 1 has F1 0
    assert abs(acc[1, 0] - 2 * P * R / (P + R + 1e-6)) < 1e-15 and acc[1, 2] == 2.0
    assert abs(acc[1, 1] - ((2 + 1e-5) / (8 + 1e-5) + 1e-5 / (2 + 1e-5))) < 1e-15
    assert np.array_equal(acc[1], metrics_reference([[2, 4, 6, 8], [0, 2, 0, 2]], npix))
    empty = sweep_reference(got[:0], npix)
    assert empty[0].tolist() == [[0.0] * 3] * 3 and empty[1].tolist() == [[0] * 4] * 2
    for bad_k in (-1, 3):
        with pytest.raises(ValueError):
            V().exceed_counts(got, bad_k)
    with pytest.raises(ValueError):
        V().exceed_counts(got[:, :1], 0)


@pytest.mark.parametrize("K", [1, 37, 255])
def test_exceed_counts_are_the_counts_of_thresholding_directly(K):
    g = np.random.default_rng(K)
    n, npix = 5, 16 * 9
    table = V().sweep_table() if K == 255 else V().sweep_table(np.sort(g.random(K)))
    assert len(table) == K
    p = g.random((n, npix)).astype(np.float32)
    p[0, :K] = table[:npix]                                          # probabilities that equal thresholds
    p[1, 0] = np.nan
    gt = g.choice(np.array([0, 1, 100, 255], np.uint8), (n, npix))
    gt[2] = 0
    exceed = exceed_reference(p, gt, list(range(n)), table, np.zeros((n, 2, K + 1), np.int32))
    assert exceed.min() >= 0 and exceed.max() <= npix and np.array_equal(exceed[:, 0, K] + exceed[:, 1, K], np.full(n, npix))
    assert (np.diff(exceed[:, :, :K], axis=2) <= 0).all()           # an ascending table: counts descend
    for k in range(K):
        assert np.array_equal(V().exceed_counts(exceed, k), direct_counts(p, gt, table[k])), k
    dev = V().exceed_counts(torch.from_numpy(exceed), K // 2)        # the tensor form: int32, what ops.frame_metrics takes
    assert dev.dtype == torch.int32 and dev.is_contiguous() and np.array_equal(dev.numpy(), V().exceed_counts(exceed, K // 2))


# ------------------------------------------------------------------------------------------------ the table
def test_default_table_bitwise():
    t = V().sweep_table()
    assert t.dtype == np.float32 and t.shape == (255,) and t.flags["C_CONTIGUOUS"]
    want = np.array([i / 256 for i in range(1, 256)], np.float64)   # exact in double and in float32: 8 fraction bits
    assert np.array_equal(t.astype(np.float64), want) and t.tobytes() == want.astype(np.float32).tobytes()
    assert t[127] == np.float32(0.5) and (np.diff(t) == np.float32(1 / 256)).all()
    assert np.array_equal(V().sweep_table(None), t)


def test_table_conversion_and_refusals():
    t = V().sweep_table([0.1, 0.5, 0.9])
    assert t.dtype == np.float32 and t.tolist() == [np.float32(0.1), np.float32(0.5), np.float32(0.9)]
    assert V().sweep_table([0.5]).tolist() == [0.5]
    assert len(V().sweep_table(np.linspace(0.001, 0.999, KMAX))) == KMAX
    assert V().sweep_table(np.array([0.25, 0.75], np.float64)).dtype == np.float32
    for bad in ([],                                                  # empty
                np.linspace(0.001, 0.999, KMAX + 1),                 # 1024 values
                [0.1, float("nan"), 0.9], [0.1, float("inf")], [1e300],      # not finite (1e300 is inf in float32)
                [0.5, 0.4], [0.1, 0.5, 0.5, 0.9],                    # descending; not strictly ascending
                [0.5, 0.5 + 1e-9],                                   # distinct doubles that collapse in float32
                [[0.1, 0.2]]):                                       # not a list
        with pytest.raises(ValueError):
            V().sweep_table(bad)


# ------------------------------------------------------------------------------------------------ finalize_sweep
def _pooled(fp, tp, neg, pos):
    return np.array([list(fp) + [neg], list(tp) + [pos]], np.int64)


def test_finalize_sweep_means_and_tie_rule():
    from mumpy_hip.evaluate import finalize_sweep
    table = np.array([0.2, 0.4, 0.6, 0.8], np.float32)
    acc = np.array([[1.0, 2.0, 4.0], [3.0, 1.0, 4.0], [3.0, 2.5, 4.0], [0.5, 0.0, 4.0]], np.float64)       # F1 ties at 0.4 and 0.6
    r = finalize_sweep(table, acc, _pooled([8, 4, 2, 1], [9, 8, 6, 2], 10, 10))
    assert r["n"] == 4 and np.array_equal(r["thresholds"], table) and r["thresholds"].dtype == np.float32
    assert r["f1"].tolist() == [0.25, 0.75, 0.75, 0.125] and r["iou"].tolist() == [0.5, 0.25, 0.625, 0.0]
    assert r["best"] == (float(np.float32(0.4)), 0.75, 0.25)        # the lowest threshold wins the tie
    assert isinstance(r["auc"], float) and 0.5 < r["auc"] < 1.0
    r1 = finalize_sweep(torch.from_numpy(table), torch.from_numpy(acc), torch.from_numpy(_pooled([8, 4, 2, 1], [9, 8, 6, 2], 10, 10)))
    assert r1["best"] == r["best"] and r1["auc"] == r["auc"]         # tensors or arrays
    r0 = finalize_sweep(table, np.zeros((4, 3)), np.zeros((2, 5), np.int64))       # nothing scored: finite means, no AUC
    assert r0["n"] == 0 and r0["f1"].tolist() == [0.0] * 4 and r0["best"][0] == float(np.float32(0.2)) and np.isnan(r0["auc"])
    for bad in ((table, acc[:3], _pooled([1] * 4, [1] * 4, 2, 2)), (table, acc, _pooled([1] * 3, [1] * 3, 2, 2)), (table[None], acc, acc)):
        with pytest.raises(ValueError):
            finalize_sweep(*bad)


def test_finalize_sweep_auc_exact_cases():
    from mumpy_hip.evaluate import finalize_sweep
    table = np.array([0.25, 0.5, 0.75], np.float32)
    acc = np.ones((3, 3))
    auc = lambda fp, tp, neg=8, pos=4: finalize_sweep(table, acc, _pooled(fp, tp, neg, pos))["auc"]
    assert auc([8, 0, 0], [4, 4, 0]) == 1.0                          # a threshold that separates the classes: the point (0, 1)
    assert auc([6, 4, 2], [3, 2, 1]) == 0.5                          # TPR == FPR everywhere: the diagonal
    assert auc([8, 8, 0], [4, 0, 0]) == 0.0                          # the point (1, 0): every score inverted
    assert np.isnan(auc([0, 0, 0], [3, 2, 1], neg=0)) and np.isnan(auc([6, 4, 2], [0, 0, 0], pos=0))
    # by hand: points (1, 1) (.75, 1) (.25, .5) (0, .25) (0, 0): .25 * 1 + .5 * .75 + .25 * .375 + 0
    assert abs(auc([6, 2, 0], [4, 2, 1]) - (0.25 + 0.375 + 0.09375)) < 1e-15


# ------------------------------------------------------------------------------------------------ the header's pinned names and limit
def test_ext7_header_declares_exactly_the_pinned_names_and_limit():
    """(tests/test_abi.py holds the header to its binding and to both libraries.)"""
    assert names_of("mumpy_hip_ext7.h") == dict(ARGS, mumpy_ext7_version=[])
    assert define("mumpy_hip_ext7.h", "MUMPY_SWEEP_MAX_THRESHOLDS") == KMAX
    from mumpy_hip import ops
    assert ops.SWEEP_MAX_THRESHOLDS == V().SWEEP_MAX_THRESHOLDS == KMAX


# ------------------------------------------------------------------------------------------------ refusals
OFF = TVH.OFF
# entry -> (tag in the message, valid scalars, [further valid tuples], [accepted no-ops], [(code, overrides)]): the layout of
# tests/test_video_host.py::REFUSALS, walked by its sweep_refusals
REFUSALS = {
    "mumpy_score_exceed_fwd": (
        b"score_exceed", dict(nclips=2, npix=32, nbank=3, K=5, stream=None),
        [dict(dest=OFF(4)), dict(K=1), dict(K=KMAX)],                                    # dest: single words, no alignment rule
        [dict(nclips=0)],
        [(ENULL, {p: None}) for p in ("logits", "gt", "dest", "thr_tab", "exceed")]
        + [(EINVAL, {k: v}) for k, v in (("npix", 0), ("npix", 24), ("npix", 40), ("npix", -16), ("nbank", 0), ("nbank", -1), ("nclips", -1),
                                         ("K", 0), ("K", -1), ("K", KMAX + 1))]
        + [(EALIGN, {"logits": OFF(4)}), (EALIGN, {"gt": OFF(8)}), (EALIGN, {"thr_tab": OFF(4)}), (EALIGN, {"exceed": OFF(8)})]
        + [(ERANGE, {"nclips": 1 << 31}), (ERANGE, {"nclips": 1 << 62}), (ERANGE, {"nbank": 1 << 31}), (ERANGE, {"npix": 1 << 31}),
           (ERANGE, {"nbank": 1 << 20, "K": KMAX}), (ERANGE, {"nbank": 1 << 29, "K": 1})]),          # nbank * 2 * (K + 1) = 2^31
    "mumpy_sweep_metrics_fwd": (
        b"sweep_metrics", dict(nscored=3, npix=32, K=5, accumulate=0, stream=None),
        [dict(accumulate=1), dict(nscored=0), dict(pooled=None), dict(exceed=OFF(4)), dict(K=1), dict(K=KMAX)],
        [],
        [(ENULL, {"exceed": None}), (ENULL, {"acc": None})]
        + [(EINVAL, {k: v}) for k, v in (("nscored", -1), ("npix", 0), ("npix", -1), ("K", 0), ("K", -1), ("K", KMAX + 1))]
        + [(EALIGN, {"acc": OFF(4)}), (EALIGN, {"pooled": OFF(4)})]
        + [(ERANGE, {"nscored": 1 << 31}), (ERANGE, {"nscored": 1 << 62}), (ERANGE, {"npix": 1 << 31}),
           (ERANGE, {"nscored": 1 << 20, "K": KMAX})]),
}


def walk_refusals(monkeypatch, lib, entry, pointers, launches, before_refusals=None):
    """sweep_refusals of tests/test_video_host.py over this file's table (its two dictionaries hold these entries for the walk only)."""
    with monkeypatch.context() as m:
        m.setitem(TVH.ARGS, entry, ARGS[entry])
        m.setitem(TVH.REFUSALS, entry, REFUSALS[entry])
        return sweep_refusals(lib, entry, pointers, launches, before_refusals)


@pytest.mark.skipif(have_gpu(), reason="with a device present a valid tuple of fake addresses would really launch")
@pytest.mark.parametrize("entry", sorted(REFUSALS))
def test_refusals_need_no_gpu(entry, monkeypatch):
    """A valid tuple of fake, 16-byte aligned, never dereferenced addresses passes every host check (rc > 0: the launch reaches a
    runtime without a device); the same tuple with one rule broken is refused with the stated code."""
    from mumpy_hip.lib import load_library
    ptrs = [n for n in ARGS[entry] if n not in REFUSALS[entry][1]]
    n = walk_refusals(monkeypatch, load_library(), entry, {p: 0x100000 * (i + 1) for i, p in enumerate(ptrs)}, launches=False)
    assert n >= 12 and entry not in TVH.REFUSALS and entry not in TVH.ARGS


# ------------------------------------------------------------------------------------------------ what ops hands over
class OnGpu(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the ops wrappers' checks pass, and the recorder launches nothing."""
    is_cuda = property(lambda self: True)


def _gpu(t):
    return torch.Tensor._make_subclass(OnGpu, t)


def _record(monkeypatch, fn):
    from mumpy_hip import ops
    monkeypatch.setattr(ops, "_stream", lambda: None)                # no device: there is no stream to ask for
    return HA.record(monkeypatch, ops, lambda: fn(ops), on_gpu=lambda t: isinstance(t, OnGpu))


def _exceed_inputs(K=5, nclips=3, npix=32, nbank=4):
    g = torch.Generator().manual_seed(7)
    return types.SimpleNamespace(
        logits=_gpu(torch.randn(nclips, 1, 4, npix // 4, generator=g)), gt=_gpu(torch.randint(0, 2, (nbank, npix), generator=g, dtype=torch.uint8)),
        dest=_gpu(torch.tensor([2, -1, 0][:nclips], dtype=torch.int32)), table=_gpu(torch.linspace(0.1, 0.9, K)),
        exceed=_gpu(torch.zeros(nbank, 2, K + 1, dtype=torch.int32)), acc=_gpu(torch.zeros(K, 3, dtype=torch.float64)),
        pooled=_gpu(torch.zeros(2, K + 1, dtype=torch.int64)))


def _refused_before_any_launch(monkeypatch, fn):
    log, _, error, launched = _record(monkeypatch, fn)
    assert isinstance(error, RuntimeError) and not log and launched == 0, (error, log)


def test_score_exceed_hands_exactly_the_buffers_given(monkeypatch):
    t = _exceed_inputs()
    log, result, error, _ = _record(monkeypatch, lambda ops: ops.score_exceed(t.logits, t.gt, t.dest, t.table, t.exceed))
    assert error is None and result is t.exceed and len(log) == 1
    assert log[0].name == "mumpy_score_exceed_fwd" and log[0].scalars == ("ptr",) * 5 + (3, 32, 4, 5, None)       # K from the table
    given = [t.logits, t.gt, t.dest, t.table, t.exceed]
    assert [p.storage for p in log[0].ptrs] == [x.untyped_storage().data_ptr() for x in given]
    assert [(p.dtype, p.shape, p.contiguous, p.gpu) for p in log[0].ptrs] == [(x.dtype, tuple(x.shape), True, True) for x in given]
    assert not HA.inplace_problems(log, {"exceed": t.exceed})
    wide = _gpu(torch.zeros(4, 2, 12, dtype=torch.int32))
    for bad in (dict(exceed=t.exceed[:3]),                                              # a shorter exceed
                dict(exceed=_gpu(torch.zeros(4, 2, 5, dtype=torch.int32))),              # ... or one threshold short
                dict(exceed=_gpu(t.exceed.long())), dict(exceed=wide[:, :, ::2]),        # wrong dtype; not contiguous
                dict(exceed=torch.zeros(4, 2, 6, dtype=torch.int32)),                    # on the host
                dict(table=_gpu(t.table.double())), dict(table=_gpu(torch.zeros(0))), dict(table=_gpu(torch.zeros(KMAX + 1))),
                dict(table=_gpu(torch.zeros(2, 5))), dict(table=_gpu(torch.zeros(10))[::2]),
                dict(dest=_gpu(t.dest.long())), dict(dest=t.dest[:2]), dict(gt=t.gt[:3]), dict(gt=_gpu(t.gt.int())),
                dict(logits=t.logits[:2]), dict(logits=_gpu(t.logits.double())), dict(logits=t.logits[..., :4]),
                dict(logits=_gpu(torch.zeros(3, 64))[:, ::2])):
        a = dict(vars(t), **bad)
        _refused_before_any_launch(monkeypatch, lambda ops: ops.score_exceed(a["logits"], a["gt"], a["dest"], a["table"], a["exceed"]))


def test_sweep_metrics_hands_exactly_the_buffers_given(monkeypatch):
    t = _exceed_inputs()
    log, result, error, _ = _record(monkeypatch, lambda ops: ops.sweep_metrics(t.exceed, 3, 32, acc=t.acc, pooled=t.pooled, accumulate=True))
    assert error is None and result[0] is t.acc and result[1] is t.pooled and len(log) == 1
    assert log[0].name == "mumpy_sweep_metrics_fwd" and log[0].scalars == ("ptr", 3, 32, 5, "ptr", "ptr", 1, None)
    given = [t.exceed, t.acc, t.pooled]
    assert [p.storage for p in log[0].ptrs] == [x.untyped_storage().data_ptr() for x in given]
    assert not HA.inplace_problems(log, {"acc": t.acc, "pooled": t.pooled})
    log, result, error, _ = _record(monkeypatch, lambda ops: ops.sweep_metrics(t.exceed, 4, 32, acc=t.acc))      # no pooled: a null pointer
    assert error is None and result is t.acc and log[0].scalars == ("ptr", 4, 32, 5, "ptr", None, 0, None)
    wide = _gpu(torch.zeros(5, 6, dtype=torch.float64))
    for bad in (dict(nscored=5), dict(nscored=-1),                                       # more frames than exceed has rows
                dict(exceed=t.exceed[:2]),                                               # a shorter exceed
                dict(exceed=_gpu(t.exceed.long())), dict(exceed=_gpu(torch.zeros(4, 2, 12, dtype=torch.int32))[:, :, ::2]),
                dict(exceed=_gpu(torch.zeros(4, 3, 6, dtype=torch.int32))), dict(exceed=_gpu(torch.zeros(4, 2, 1, dtype=torch.int32))),
                dict(acc=t.acc[:4]), dict(acc=_gpu(t.acc.float())), dict(acc=wide[:, ::2]), dict(acc=torch.zeros(5, 3, dtype=torch.float64)),
                dict(pooled=t.pooled[:, :5]), dict(pooled=_gpu(t.pooled.int())), dict(pooled=_gpu(torch.zeros(6, 2, dtype=torch.int64)).t()),
                dict(acc=None, accumulate=True), dict(pooled=True, accumulate=True)):    # accumulate needs the caller's buffers
        a = dict(exceed=t.exceed, nscored=3, acc=t.acc, pooled=t.pooled, accumulate=False)
        a.update(bad)
        _refused_before_any_launch(monkeypatch, lambda ops: ops.sweep_metrics(a["exceed"], a["nscored"], 32, acc=a["acc"], pooled=a["pooled"],
                                                                              accumulate=a["accumulate"]))


# ------------------------------------------------------------------------------------------------ the predictor's arguments
def test_video_predictor_refuses_a_bad_sweep_before_it_needs_a_device():
    enc = types.SimpleNamespace(configs=[{"num_frames": 3}], parameters=lambda: iter([torch.zeros(1)]))
    make = lambda sweep: V().VideoPredictor(enc, None, T=3, src_hw=(30, 26), batch=4, max_frames=16, graph=False, sweep=sweep)
    for bad in ([], [0.5, 0.4], [0.1, float("nan")], np.linspace(0.001, 0.999, KMAX + 1), [0.5, 0.5], 0.5, "0.5", 3):
        with pytest.raises(ValueError):
            make(bad)
    for good in (None, True, [0.25, 0.5], np.array([0.5])):         # accepted: the next thing missing is the device
        with pytest.raises(RuntimeError, match="not on a GPU"):
            make(good)
