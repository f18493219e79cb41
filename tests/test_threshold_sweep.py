"""GPU: a whole video scored at every mask threshold in one pass (include/mumpy_hip_ext7.h, ops.score_exceed / sweep_metrics,
mumpy_hip.video.VideoPredictor(sweep=...)).

The oracle of the exceed kernel is code that exists without it and runs on the device, never numpy: ops.final_conv(..., with_mask=True,
thr=t_k) gives the logits and the mask at each threshold, ops.mask_score_u8 counts the mask against the annotation, and the new kernel
on the same logits must give the same integers at every k (`==`).  The metrics kernel is held to the numpy statements of
tests/test_threshold_sweep_host.py (the same fp64 arithmetic, only the order of the sum over frames differs) and to
ops.frame_metrics of the same counts.

Shapes.  Exceed: npix = 64 (8 x 8: 4 of a workgroup's 256 threads hold pixels), 16 * 257 (ragged over the threads), 224 * 224 (the
model's: every thread walks several chunks); K = 1 (no interior bin), 37, 255 (the default table) and 1023 (the cap: every thread of
the suffix sum owns four bins), the last at npix = 64 only.  Metrics: 5 frames and 300 (more frames than threads), K = 3 and 255."""
import numpy as np
import pytest
import torch

import guarded_alloc as GA
from test_threshold_sweep_host import ARGS, REFUSALS, exceed_reference, sweep_reference, walk_refusals
from test_video_host import masks_metrics_reference

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")

NCLIPS, NBANK = 4, 6
DEST = [3, -1, 0, 99]                                                # -1 and 99 are dropped: rows 0 and 3 are written
SENTINEL = -7


def _ops():
    from mumpy_hip import ops
    return ops


def _video():
    from mumpy_hip import video
    return video


def _table(K):
    if K == 1:
        return _video().sweep_table([0.5])
    if K == 255:
        return _video().sweep_table()
    if K == 1023:
        return _video().sweep_table(np.linspace(0.001, 0.999, 1023))
    return _video().sweep_table(np.sort(np.random.default_rng(K).random(K)))


def _features(h, w, nclips=NCLIPS, seed=0):
    """Features (nclips, 32, h, w) NHWC and a 3 x 3 weight scaled so that the logits span about +-6 (288 products of unit normals
    with weights of standard deviation 2 / sqrt(288): a standard deviation of 2)."""
    g = torch.Generator().manual_seed(1000 * h + w + seed)
    x = torch.randn(nclips, 32, h, w, generator=g).to(DEV).contiguous(memory_format=torch.channels_last)
    wt = (torch.randn(1, 3, 3, 32, generator=g) * (2.0 / 288 ** 0.5)).to(DEV)
    bias = torch.tensor([0.1], device=DEV)
    return x, wt, bias


def _gt(nbank, npix, seed):
    return torch.from_numpy(np.random.default_rng(seed).choice(np.array([0, 1, 100, 255], np.uint8), (nbank, npix))).to(DEV)


def oracle_rows(x, wt, bias, gt_per_clip, table):
    """-> (logits (nclips, npix), rows (nclips, 2, K + 1) int32 on the host): per threshold the mask final_conv emits and the counts
    mask_score_u8 takes from it against gt_per_clip (nclips, npix), rearranged as exceed rows."""
    ops = _ops()
    nclips, npix, K = x.shape[0], gt_per_clip.shape[1], len(table)
    ident = torch.arange(nclips, dtype=torch.int32, device=DEV)
    bank = torch.empty(nclips, npix, dtype=torch.uint8, device=DEV)
    counts = torch.zeros(K, nclips, 4, dtype=torch.int32, device=DEV)
    logits = None
    for k in range(K):
        lg, mask = ops.final_conv(x, wt, bias, with_mask=True, thr=float(table[k]))
        assert logits is None or GA.same_bits(lg, logits)            # the logits do not depend on thr
        logits = lg
        ops.mask_score_u8(mask, ident, bank, gt=gt_per_clip, counts=counts[k])
    c = counts.cpu().numpy().astype(np.int64)                        # (K, nclips, {inter, sum p, sum g, union})
    rows = np.zeros((nclips, 2, K + 1), np.int64)
    rows[:, 1, :K] = c[:, :, 0].T
    rows[:, 0, :K] = (c[:, :, 1] - c[:, :, 0]).T
    rows[:, 1, K] = c[0, :, 2]
    rows[:, 0, K] = npix - c[0, :, 2]
    assert (c[:, :, 3] == c[:, :, 1] + c[:, :, 2] - c[:, :, 0]).all() and (c[:, :, 2] == c[0, :, 2]).all()
    return logits.reshape(nclips, npix), rows.astype(np.int32)


# ------------------------------------------------------------------------------------------------ the exceed kernel
CASES = [(hw, K) for hw in ((8, 8), (16, 257), (224, 224)) for K in (1, 37, 255)] + [((8, 8), 1023)]


@pytest.mark.parametrize("hw,K", CASES, ids=[f"{h}x{w}-K{K}" for (h, w), K in CASES])
def test_exceed_rows_are_the_counts_of_the_mask_at_every_threshold(hw, K):
    ops = _ops()
    h, w = hw
    npix = h * w
    table = _table(K)
    assert len(table) == K
    x, wt, bias = _features(h, w)
    gt = _gt(NBANK, npix, seed=npix + K)
    dest = torch.tensor(DEST, dtype=torch.int32, device=DEV)
    valid = {c: d for c, d in enumerate(DEST) if 0 <= d < NBANK}     # clip -> row
    gt_per_clip = torch.stack([gt[valid.get(c, 0)] for c in range(NCLIPS)]).contiguous()
    logits, want = oracle_rows(x, wt, bias, gt_per_clip, table)
    if K > 1:                                                        # the logits spread and the thresholds bite
        assert float(logits.min()) < -2 and float(logits.max()) > 2 and len(np.unique(want[:, :, :K])) > min(K, npix) // 4
    td = torch.from_numpy(table).to(DEV)
    snap = [t.clone() for t in (logits, gt, dest, td)]
    exceed = torch.full((NBANK, 2, K + 1), SENTINEL, dtype=torch.int32, device=DEV)
    r = ops.score_exceed(logits.view(NCLIPS, 1, h, w), gt, dest, td, exceed)
    assert r.data_ptr() == exceed.data_ptr()
    got = exceed.cpu().numpy()
    for c, d in valid.items():
        assert np.array_equal(got[d], want[c]), (d, np.argwhere(got[d] != want[c])[:5])
    others = [d for d in range(NBANK) if d not in valid.values()]
    assert others == [1, 2, 4, 5] and (got[others] == SENTINEL).all()                     # rows no valid dest names keep the sentinel
    assert all(GA.same_bits(a, b) for a, b in zip((logits, gt, dest, td), snap))          # the inputs are only read
    # garbage in the buffer: valid rows are overwritten, nothing is accumulated; two runs give the same bits
    again = torch.from_numpy(np.random.default_rng(1).integers(-2 ** 31, 2 ** 31, (NBANK, 2, K + 1)).astype(np.int32)).to(DEV)
    before = again.clone()
    ops.score_exceed(logits, gt, dest, td, again)
    assert GA.same_bits(again[[0, 3]], exceed[[0, 3]]) and GA.same_bits(again[others], before[others])


SPECIAL = [float("nan"), float("inf"), float("-inf"), 0.0, -0.0, 100.0, -100.0, 1e30, -1e30]


def test_special_logits():
    """Zero weights and the logit as the bias, so that the oracle still applies.  The table is [0.25, 0.5, 0.75], npix = 16."""
    ops = _ops()
    table = _video().sweep_table([0.25, 0.5, 0.75])
    x = torch.zeros(1, 32, 4, 4, device=DEV).contiguous(memory_format=torch.channels_last)
    wt = torch.zeros(1, 3, 3, 32, device=DEV)
    n, npix = len(SPECIAL), 16
    gt = _gt(n, npix, seed=3)
    logits, want = [], []
    for i, z in enumerate(SPECIAL):
        lg, rows = oracle_rows(x, wt, torch.tensor([z], device=DEV), gt[i:i + 1], table)
        logits.append(lg)
        want.append(rows[0])
    logits, want = torch.cat(logits).contiguous(), np.stack(want)
    lz = logits[:, 0].cpu().numpy()
    assert np.isnan(lz[0]) and lz[1] == np.inf and lz[2] == -np.inf and lz[5] == 100 and lz[8] == np.float32(-1e30)
    logits[4] = -0.0                                                 # 0 * 0 + (-0) is +0 in the convolution: the sign is set here
    assert bool(torch.signbit(logits[4]).all()) and not bool(torch.signbit(logits[3]).any())
    exceed = torch.full((n, 2, 4), SENTINEL, dtype=torch.int32, device=DEV)
    ops.score_exceed(logits, gt, torch.arange(n, dtype=torch.int32, device=DEV), torch.from_numpy(table).to(DEV), exceed)
    got = exceed.cpu().numpy()
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    g1 = (gt > 0).sum(1).cpu().numpy()
    tot = np.stack([npix - g1, g1], 1)                               # (n, class)
    assert (got[0, :, :3] == 0).all() and np.array_equal(got[0, :, 3], tot[0])            # NaN exceeds nothing
    for i in (1, 5, 7):                                              # +inf, 100, 1e30: p = 1 exceeds everything
        assert np.array_equal(got[i, :, :3], np.repeat(tot[i][:, None], 3, 1)), i
    for i in (2, 6, 8):                                              # -inf, -100, -1e30: p = 0 exceeds nothing
        assert (got[i, :, :3] == 0).all(), i
    for i in (3, 4):                                                 # +-0: p = 0.5 exceeds 0.25 and does not exceed 0.5
        assert np.array_equal(got[i, :, 0], tot[i]) and (got[i, :, 1:3] == 0).all(), i


def _int32_fill(pattern):
    return int(np.array([pattern] * 4, np.uint8).view(np.int32)[0])


@pytest.mark.parametrize("garbage", [False, True], ids=["ascending", "garbage-table-and-dest"])
def test_memory_discipline_of_the_exceed_kernel(monkeypatch, garbage):
    """tests/guarded_alloc.py as test_memory_discipline_of_the_window uses it: bands intact, every element of a valid row written,
    the other rows untouched, the inputs bitwise unchanged, the result independent of where the buffers sit.  With a garbage table
    (shuffled, with NaN) and garbage dest the same holds, and every value written lies in [0, npix]."""
    ops = _ops()
    h, w, K = 16, 257, 37
    npix = h * w
    g = np.random.default_rng(11)
    table = _table(K)
    dest_list = DEST
    if garbage:
        table = g.permutation(table)
        table[[0, 5, K - 1]] = np.nan
        dest_list = [5, -2 ** 31, 2 ** 31 - 1, 1]
    valid_rows = sorted(d for d in dest_list if 0 <= d < NBANK)
    others = [d for d in range(NBANK) if d not in valid_rows]
    x, wt, bias = _features(h, w, seed=1)
    logits = ops.final_conv(x, wt, bias).reshape(NCLIPS, npix).cpu()
    gt, dest, tab = _gt(NBANK, npix, seed=5).cpu(), torch.tensor(dest_list, dtype=torch.int32), torch.from_numpy(table)
    plain = torch.full((NBANK, 2, K + 1), SENTINEL, dtype=torch.int32, device=DEV)
    ops.score_exceed(logits.to(DEV), gt.to(DEV), dest.to(DEV), tab.to(DEV), plain)
    plain = plain.cpu()
    assert (plain[others] == SENTINEL).all()
    assert int(plain[valid_rows].min()) >= 0 and int(plain[valid_rows].max()) <= npix
    assert bool((plain[valid_rows][:, 0, K] + plain[valid_rows][:, 1, K] == npix).all())

    def body(guard):
        ex = guard.tensor(torch.full((NBANK, 2, K + 1), _int32_fill(guard.pattern), dtype=torch.int32))
        ops.score_exceed(guard.tensor(logits), guard.tensor(gt), guard.tensor(dest), guard.tensor(tab), ex)
        return {"exceed": ex}, (ex,), {"exceed": (others, "rows no valid dest names")}
    runs, unguarded = GA.run_both(monkeypatch, [ops], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set()
    for outs in runs:
        assert GA.same_bits(outs["exceed"][valid_rows].cpu(), plain[valid_rows])


# ------------------------------------------------------------------------------------------------ the metrics kernel
def _random_exceed(n, npix, K, seed):
    g = np.random.default_rng(seed)
    table = _table(K) if K != 3 else np.array([0.25, 0.5, 0.75], np.float32)
    p = g.random((n, npix)).astype(np.float32) ** 2
    gt = (g.random((n, npix)) < 0.2).astype(np.uint8) * 255
    p[gt > 0] = np.sqrt(p[gt > 0])                                   # forged pixels score higher: the metrics are not trivial
    gt[0] = 0                                                        # an empty annotation
    p[1] = 0.0                                                       # an empty prediction at every threshold
    p[2] = np.where(gt[2] > 0, 1.0, 0.0)                             # a perfect match at every threshold
    return exceed_reference(p, gt, list(range(n)), table, np.zeros((n, 2, K + 1), np.int32))


def _close(got, want):
    return bool(np.all(np.abs(got - want) <= 1e-12 * np.abs(want)))


@pytest.mark.parametrize("n,K", [(5, 3), (5, 255), (300, 3), (300, 255)])
def test_sweep_metrics_in_fp64(n, K):
    """acc against sweep_reference to 1e-12 relative: the arithmetic is the same fp64 and only the order of the sum over the frames
    differs (300 * 2^-53 < 1e-13, the argument of test_frame_metrics_in_fp64); pooled exactly."""
    ops = _ops()
    npix = 16 * 24
    ex = _random_exceed(n + 3, npix, K, seed=n + K)                  # three more rows than are scored
    exd = torch.from_numpy(ex).to(DEV)
    want_acc, want_pooled = sweep_reference(ex[:n], npix)
    acc, pooled = ops.sweep_metrics(exd, n, npix, pooled=True)
    assert acc.dtype == torch.float64 and acc.shape == (K, 3) and pooled.dtype == torch.int64 and pooled.shape == (2, K + 1)
    got = acc.cpu().numpy()
    assert (got[:, 2] == n).all() and _close(got, want_acc), np.abs(got - want_acc).max()
    assert np.array_equal(pooled.cpu().numpy(), want_pooled)
    for k in sorted({0, K // 2, K - 1}):                             # row k is frame_metrics of the counts at threshold k
        fm = ops.frame_metrics(_video().exceed_counts(exd[:n], k), n, npix).cpu().numpy()
        assert _close(got[k], fm), (k, got[k], fm)
    acc2, pooled2 = ops.sweep_metrics(exd, n, npix, pooled=True)
    assert GA.same_bits(acc, acc2) and GA.same_bits(pooled, pooled2)                      # two runs: the same bits
    assert GA.same_bits(exd.cpu(), torch.from_numpy(ex))                                  # exceed is only read
    # overwrite, then accumulate, then no frames
    a = torch.full((K, 3), 5.0, device=DEV, dtype=torch.float64)
    p = torch.full((2, K + 1), 5, device=DEV, dtype=torch.int64)
    ra, rp = ops.sweep_metrics(exd, n, npix, acc=a, pooled=p)
    assert ra.data_ptr() == a.data_ptr() and rp.data_ptr() == p.data_ptr() and GA.same_bits(a, acc) and GA.same_bits(p, pooled)
    ops.sweep_metrics(exd, 4, npix, acc=a, pooled=p, accumulate=True)
    acc4, pooled4 = sweep_reference(ex[:4], npix)
    assert _close(a.cpu().numpy(), want_acc + acc4) and (a[:, 2] == n + 4).all()
    assert np.array_equal(p.cpu().numpy(), want_pooled + pooled4)
    ops.sweep_metrics(exd, 0, npix, acc=a, pooled=p, accumulate=True)
    assert _close(a.cpu().numpy(), want_acc + acc4) and np.array_equal(p.cpu().numpy(), want_pooled + pooled4)
    z, zp = ops.sweep_metrics(exd, 0, npix, pooled=True)
    assert not z.any() and not zp.any()
    # without pooled: the same acc, nothing else written
    only = ops.sweep_metrics(exd, n, npix)
    assert isinstance(only, torch.Tensor) and GA.same_bits(only, acc)
    assert GA.same_bits(ops.sweep_metrics(exd, n, npix, acc=torch.zeros_like(acc)), acc)
    # refusals of the wrapper
    for bad in (dict(nscored=n + 4), dict(acc=torch.zeros(K - 1 or 2, 3, device=DEV, dtype=torch.float64)),
                dict(acc=torch.zeros(K, 3, device=DEV)), dict(pooled=torch.zeros(2, K, device=DEV, dtype=torch.int64)),
                dict(pooled=torch.zeros(2, K + 1, device=DEV, dtype=torch.int32)), dict(accumulate=True),
                dict(accumulate=True, acc=a, pooled=True), dict(exceed=exd[:, :, :-1]), dict(exceed=exd.cpu())):
        kw = dict(exceed=exd, nscored=n, acc=None, pooled=None, accumulate=False)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            ops.sweep_metrics(kw["exceed"], kw["nscored"], npix, acc=kw["acc"], pooled=kw["pooled"], accumulate=kw["accumulate"])


# ------------------------------------------------------------------------------------------------ refusals
SLACK = 256                          # bytes behind every buffer: a pointer moved by a few bytes still reads and writes inside it
KCAP = 1023                          # the buffers are sized for the longest valid table of REFUSALS


def _buffers(entry):
    v = REFUSALS[entry][1]
    if entry == "mumpy_score_exceed_fwd":
        sizes = {"logits": (v["nclips"] * v["npix"], torch.float32), "gt": (v["nbank"] * v["npix"], torch.uint8), "dest": (v["nclips"], torch.int32),
                 "thr_tab": (KCAP, torch.float32), "exceed": (v["nbank"] * 2 * (KCAP + 1), torch.int32)}
    else:
        sizes = {"exceed": (v["nscored"] * 2 * (KCAP + 1), torch.int32), "acc": (KCAP * 3, torch.float64), "pooled": (2 * (KCAP + 1), torch.int64)}
    assert set(sizes) | set(v) == set(ARGS[entry])
    return {k: torch.zeros(n + SLACK // torch.empty((), dtype=dt).element_size(), device=DEV, dtype=dt) for k, (n, dt) in sizes.items()}


@pytest.mark.parametrize("entry", sorted(REFUSALS))
def test_every_refusal_of_the_header_launches_nothing(entry, monkeypatch):
    """The table of tests/test_threshold_sweep_host.py against real buffers: the valid tuples run (rc == 0), every broken one is
    refused with its MUMPY_E* code and a message of its own -- and no buffer changes: nothing was launched."""
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
    n = walk_refusals(monkeypatch, load_library(), entry, {k: t.data_ptr() for k, t in bufs.items()}, launches=True,
                      before_refusals=before_refusals)
    torch.cuda.synchronize()
    assert n >= 12 and snap and all(torch.equal(t.view(torch.uint8), snap[k]) for k, t in bufs.items())


# ------------------------------------------------------------------------------------------------ the predictor
HS, WS, BATCH = 30, 26, 4


def _next_pool_stream():
    return torch.cuda.Stream(device=DEV).cuda_stream


@pytest.fixture(scope="module")
def sweep_model():
    """Seeded weights, the three-view model at T = 3 (the fixture of tests/test_video_stage.py), and three predictors: graphed with
    a sweep, eager with, eager without.  ONE graphed predictor: each owns a capture stream and the fork/join side streams under it,
    which come from torch's round-robin pool of 32 and stay in mumpy_hip.streams' registry; whether a later capture of the process
    still finds free ones depends on both.  So the entries this predictor adds are taken out again afterwards (as
    tests/test_annot_resize.py does) and the pool's pointer is walked on to where it stood, and the rest of the process finds both
    as if this file had not run.  thr is the sigmoid of the median logit of the first batch, so that the masks hold both values;
    the table is [thr / 2, float32(thr), (1 + thr) / 2]: its middle row is the predictor's own threshold."""
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from mumpy_hip import streams
    from mumpy_hip.pipeline import fused_forward
    from mumpy_hip.video import VideoPredictor, batch_plan
    from weight_fill import fill_module_
    ops = _ops()
    registry = set(streams._SIDE)
    cycle = [_next_pool_stream()]                                    # one turn of the pool, and the first handle once more
    while len(cycle) < 2 or cycle[-1] != cycle[0]:
        cycle.append(_next_pool_stream())
        assert len(cycle) <= 257, "torch's stream pool does not repeat"
    enc, dec = fill_module_(Encoder()).eval().to(DEV), fill_module_(Decoder()).eval().to(DEV)
    g = np.random.default_rng(2024)
    frames = {n: g.integers(0, 256, (n, HS, WS, 3), dtype=np.uint8) for n in (7, 5)}
    idx, _ = batch_plan(7, 3, BATCH)
    x = ops.normalize_u8(torch.from_numpy(frames[7]).to(DEV)[torch.from_numpy(idx[0]).long().to(DEV)], size=(224, 224))
    thr = float(torch.sigmoid(fused_forward(enc, dec, x)[0]).median())
    assert 0.0 < thr < 1.0
    table = [thr / 2, float(np.float32(thr)), (1 + thr) / 2]
    kw = dict(T=3, src_hw=(HS, WS), batch=BATCH, max_frames=16, thr=thr)
    graphed = VideoPredictor(enc, dec, graph=True, sweep=table, **kw)
    yield {"thr": thr, "table": table, "frames": frames, "graphed": graphed,
           "plain": VideoPredictor(enc, dec, graph=False, **kw),
           "eager": VideoPredictor(enc, dec, graph=False, sweep=table, **kw)}
    torch.cuda.synchronize()
    for key in set(streams._SIDE) - registry:
        del streams._SIDE[key]
    for _ in range(len(cycle)):                                      # until the next handle out is cycle[0] again
        if _next_pool_stream() == cycle[-2]:
            break
    else:
        raise AssertionError("the stream pool's pointer was not found again")


def test_video_predictor_sweep(sweep_model):
    from mumpy_hip.evaluate import finalize_metrics, finalize_sweep
    sm, vp, plain, eager = sweep_model, sweep_model["graphed"], sweep_model["plain"], sweep_model["eager"]
    video, npix = _video(), 224 * 224
    f7, f5 = sm["frames"][7], sm["frames"][5]
    gt = (np.random.default_rng(9).integers(0, 3, (7, 224, 224)) * 100).astype(np.uint8)
    gt[6] = 0                                                        # one frame without annotation
    assert plain.table is None and plain.exceed is None and plain.sweep_acc is None and plain.sweep_pooled is None
    with pytest.raises(RuntimeError):
        plain.sweep_vector()
    table, acc, pooled = vp.sweep_vector()
    assert table.dtype == torch.float32 and table.cpu().tolist() == [float(np.float32(t)) for t in sm["table"]]
    assert vp.exceed.shape == (16, 2, 4) and acc.shape == (3, 3) and acc.dtype == torch.float64
    assert pooled.shape == (2, 4) and pooled.dtype == torch.int64 and not acc.any() and not pooled.any()
    assert not vp.exceed.any()                                       # the warm-up and the capture wrote nothing: dest is -1

    masks = vp.predict(torch.from_numpy(f7), torch.from_numpy(gt)).clone()
    torch.cuda.synchronize()
    graph = vp.graph
    assert sorted(np.unique(masks.cpu().numpy()).tolist()) == [0, 255]
    # the middle row of the table is the predictor's own threshold: the same counts, exactly
    assert torch.equal(video.exceed_counts(vp.exceed[:7], 1), vp.counts[:7])
    ex = vp.exceed[:7].cpu().numpy().astype(np.int64)
    assert (ex[:, 0, 3] + ex[:, 1, 3] == npix).all() and np.array_equal(ex[:, 1, 3], (gt.reshape(7, -1) > 0).sum(1))
    assert (np.diff(ex[:, :, :3], axis=2) <= 0).all() and (ex[:, :, 0] > ex[:, :, 2]).any()
    assert not vp.exceed[7:].any()                                   # the padding clip wrote nothing
    metric, sweep_acc = vp.metric_vector().cpu().numpy(), acc.cpu().numpy()
    assert (sweep_acc[:, 2] == 7).all() and metric[2] == 7           # the padding clip is not counted
    assert np.all(np.abs(sweep_acc[1] - metric) <= 1e-12 * np.abs(metric)), (sweep_acc[1], metric)
    want_acc, want_pooled = sweep_reference(ex, npix)
    assert np.all(np.abs(sweep_acc - want_acc) <= 1e-12 * np.abs(want_acc)) and np.array_equal(pooled.cpu().numpy(), want_pooled)
    # sweep=None (an eager predictor; graph=False gives the graph's bits, below and in tests/test_video_stage.py): the same masks
    # and the same metric vector, bit for bit
    masks_p = plain.predict(torch.from_numpy(f7), torch.from_numpy(gt))
    torch.cuda.synchronize()
    assert GA.same_bits(masks_p, masks) and GA.same_bits(plain.metric_vector(), vp.metric_vector()) and GA.same_bits(plain.counts, vp.counts)
    # graph=False: the same bits
    masks_e = eager.predict(torch.from_numpy(f7).to(DEV), torch.from_numpy(gt).to(DEV))
    torch.cuda.synchronize()
    assert GA.same_bits(masks_e, masks) and GA.same_bits(eager.exceed, vp.exceed)
    assert GA.same_bits(eager.sweep_acc, vp.sweep_acc) and GA.same_bits(eager.sweep_pooled, vp.sweep_pooled)

    # without gt nothing is added
    keep_acc, keep_pooled, keep_metric = acc.clone(), pooled.clone(), vp.metric_vector().clone()
    masks5 = vp.predict(f5).clone()
    torch.cuda.synchronize()
    assert GA.same_bits(acc, keep_acc) and GA.same_bits(pooled, keep_pooled) and GA.same_bits(vp.metric_vector(), keep_metric)
    assert vp.graph is graph and not GA.same_bits(masks5, masks[:5])
    # a second video accumulates
    vp.predict(f5, gt[:5])
    torch.cuda.synchronize()
    assert vp.graph is graph                                         # one capture serves every video
    assert torch.equal(video.exceed_counts(vp.exceed[:5], 1), vp.counts[:5])
    ex5 = vp.exceed[:5].cpu().numpy().astype(np.int64)
    acc5, pooled5 = sweep_reference(ex5, npix)
    both = want_acc + acc5
    got = acc.cpu().numpy()
    assert (got[:, 2] == 12).all() and np.all(np.abs(got - both) <= 1e-12 * np.abs(both))
    assert np.array_equal(pooled.cpu().numpy(), want_pooled + pooled5)
    both_metric = masks_metrics_reference(masks.cpu().numpy(), gt) + masks_metrics_reference(masks5.cpu().numpy(), gt[:5])
    assert np.all(np.abs(got[1] - both_metric) <= 1e-12 * np.abs(both_metric))
    r = finalize_sweep(*vp.sweep_vector())
    f1, iou, cnt = finalize_metrics(vp.metric_vector())
    assert r["n"] == cnt == 12 and np.allclose(r["f1"], both[:, 0] / 12, rtol=1e-12, atol=0) and np.allclose(r["iou"], both[:, 1] / 12, rtol=1e-12, atol=0)
    assert abs(r["f1"][1] - f1) <= 1e-12 * f1 and abs(r["iou"][1] - iou) <= 1e-12 * iou
    assert r["best"][0] == float(r["thresholds"][int(np.argmax(r["f1"]))]) and 0.0 <= r["auc"] <= 1.0
    assert GA.same_bits(acc, torch.from_numpy(got).to(DEV))          # finalize_sweep reduces copies
    vp.reset_metrics()
    assert not acc.any() and not pooled.any() and vp.metric_vector().cpu().tolist() == [0.0, 0.0, 0.0]
