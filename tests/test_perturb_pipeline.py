"""GPU: the two ordinary perturbations inside the device paths -- VideoPredictor(perturb=...) and AugmentedInput(perturb=True).

The oracle of the predictor is an unperturbed predictor that is fed the frames Pillow processed on the host: masks, bank, counts and
metric vector must agree bit for bit.  The oracle of the input stage is the existing stage (ops.augment_stage_u8) run on a canvas
that numpy resized and perturbed (mumpy_hip.perturb, which tests/test_perturb_host.py holds to Pillow).  The model is the three-view
model at T = 3 with seeded weights, as tests/test_annot_resize.py builds it."""
import numpy as np
import pytest
import torch

import guarded_alloc as GA
from mumpy_hip import perturb as P
from test_perturb_host import pil_blur, pil_jpeg

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")

HS, WS, N, BATCH = 48, 64, 7, 4


def _ops():
    from mumpy_hip import ops
    return ops


def _video():
    g = np.random.default_rng(123)
    yy, xx = np.mgrid[0:HS, 0:WS]
    base = np.stack([yy * 4 + xx, 255 - xx * 3, (yy * xx) % 256], -1)
    frames = np.stack([np.clip(base + g.integers(-40, 41, (HS, WS, 3)) + 9 * k, 0, 255) for k in range(N)]).astype(np.uint8)
    gt = ((g.random((N, 224, 224)) < 0.3) * 255).astype(np.uint8)
    return frames, gt


def _pil(frames, steps):
    out = frames
    for kind, v in steps:
        out = np.stack([pil_jpeg(a, v)[0] if kind == "jpeg" else pil_blur(a, v) for a in out])
    return out


@pytest.fixture(scope="module")
def predictors():
    """Seeded weights and predictors on demand.  thr is the sigmoid of the first batch's median logit, so that the masks hold both
    values.  Every graphed predictor owns a capture stream and fork/join side streams under it, which come from torch's round-robin
    pool of 32 and stay in mumpy_hip.streams' registry; whether a later capture of the process still finds free ones depends on
    both (tests/test_threshold_sweep.py).  The perturbation runs ahead of the forward and outside its graph, so this file needs no
    forked forward: every forward of this file, on either side of a comparison, runs with streams.SERIAL (the branches in order on
    one stream), which takes no side stream at all; the capture streams it does draw are paid back by walking the pool's pointer
    on to where it stood."""
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from mumpy_hip import streams
    from mumpy_hip.pipeline import fused_forward
    from mumpy_hip.video import VideoPredictor, batch_plan
    from weight_fill import fill_module_
    before, serial = set(streams._SIDE), streams.SERIAL
    streams.SERIAL = True
    cycle = [_next_pool_stream()]                                    # one turn of the pool, and the first handle once more
    while len(cycle) < 2 or cycle[-1] != cycle[0]:
        cycle.append(_next_pool_stream())
        assert len(cycle) <= 257, "torch's stream pool does not repeat"
    enc, dec = fill_module_(Encoder()).eval().to(DEV), fill_module_(Decoder()).eval().to(DEV)
    idx, _ = batch_plan(N, 3, BATCH)
    clips = torch.from_numpy(_video()[0]).to(DEV)[torch.from_numpy(idx[0]).long().to(DEV)]
    thr = float(torch.sigmoid(fused_forward(enc, dec, _ops().normalize_u8(clips, size=(224, 224)))[0]).median())
    assert 0.0 < thr < 1.0
    made = {}

    def get(graph, **kw):
        key = (graph, repr(sorted(kw.items())))
        if key not in made:
            made[key] = VideoPredictor(enc, dec, T=3, src_hw=(HS, WS), batch=BATCH, max_frames=8, thr=thr, graph=graph, **kw)
        return made[key]
    get.models = (enc, dec, thr)
    yield get
    torch.cuda.synchronize()
    made.clear()
    streams.SERIAL = serial
    assert set(streams._SIDE) == before                              # no side stream was taken
    for _ in range(len(cycle)):                                      # until the next handle out is cycle[0] again
        if _next_pool_stream() == cycle[-2]:
            break
    else:
        raise AssertionError("the stream pool's pointer was not found again")


def _next_pool_stream():
    return torch.cuda.Stream(device=DEV).cuda_stream


def _same_results(a, b):
    assert torch.equal(a.bank[:N], b.bank[:N]) and torch.equal(a.counts[:N], b.counts[:N])
    assert GA.same_bits(a.metric_vector(), b.metric_vector()) and float(a.metric_vector()[2]) == float(N)


@pytest.mark.parametrize("graph,spec", [(True, ("jpeg", 50)), (False, ("jpeg", 50)), (False, ("blur", 2.0)),
                                        (False, [("blur", 1.0), ("jpeg", 70)])], ids=["jpeg50-graph", "jpeg50", "blur2", "blur1+jpeg70"])
def test_a_perturbed_predictor_equals_a_plain_one_fed_pillows_frames(predictors, graph, spec):
    frames, gt = _video()
    steps = P.check_spec(spec)
    processed = _pil(frames, steps)
    assert not np.array_equal(processed, frames)
    pert, plain = predictors(graph, perturb=spec, perturb_chunk=3), predictors(graph)      # chunks of 3, 3 and 1 frames
    pert.reset_metrics(); plain.reset_metrics()
    m_pert = pert.predict(frames, gt).clone()
    m_plain = plain.predict(processed, gt).clone()
    torch.cuda.synchronize()
    assert np.array_equal(pert.frames[:N].cpu().numpy(), processed)               # the uploaded video, perturbed in place
    assert torch.equal(m_pert, m_plain) and np.unique(m_pert.cpu().numpy()).tolist() == [0, 255]
    _same_results(pert, plain)
    # ... and it is not what the unperturbed video gives
    plain.reset_metrics()
    m_clean = plain.predict(frames, gt).clone()
    torch.cuda.synchronize()
    assert not torch.equal(m_clean, m_pert)
    # frames that are already on the device: the caller's tensor is left alone
    fd = torch.from_numpy(frames).to(DEV)
    pert.reset_metrics()
    assert torch.equal(pert.predict(fd, gt), m_plain) and np.array_equal(fd.cpu().numpy(), frames)


def test_perturb_none_is_the_default_predictor(predictors, monkeypatch):
    """perturb=None allocates nothing and launches nothing: the same launches go into the captured graph (every node of it is one
    call through the binding, so the calls made while capturing count its nodes), and the same bits come out."""
    ops = _ops()
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a, **kw: (calls.append(name), real(name, *a, **kw))[1])
    built = []
    for vp in (predictors(True), predictors(True, perturb=None)):                 # (the fixture's plain predictor: no stream more)
        del calls[:]
        vp._capture()                                                             # warm-up and capture, counted
        built.append((vp, list(calls)))
    assert built[0][1] == built[1][1] and len(built[0][1]) > 100
    assert not any("jpeg" in n or "blur" in n or "nearest" in n for n in built[0][1])
    frames, gt = _video()
    for vp, _ in built:
        assert vp.perturb == [] and vp._perturb_ws is None
        vp.reset_metrics()
        del calls[:]
        vp.predict(frames, gt)
        assert calls == ["mumpy_frame_metrics_fwd"]                               # the replays launch nothing through the binding
    torch.cuda.synchronize()
    _same_results(built[1][0], built[0][0])
    eager = predictors(False, perturb=[])                                         # an empty list is no perturbation either
    assert eager.perturb == [] and eager._perturb_ws is None


def test_a_bad_spec_is_refused_in_the_constructor(predictors):
    from mumpy_hip.video import VideoPredictor
    enc, dec, thr = predictors.models
    for bad in ("jpeg", ("jpeg", 0), ("jpeg", 101), ("blur", -1.0), ("sharpen", 2), [("jpeg", 50), ("blur",)], 5):
        with pytest.raises(ValueError):
            VideoPredictor(enc, dec, T=3, src_hw=(HS, WS), graph=False, perturb=bad)
    with pytest.raises(ValueError):
        VideoPredictor(enc, dec, T=3, src_hw=(HS, WS), graph=False, perturb=("jpeg", 50), perturb_chunk=0)


# ------------------------------------------------------------------------------------------------ the training input stage
B, T, SH, SW, L = 2, 3, 30, 44, 16


def _clips(seed=3):
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:SH, 0:SW]
    base = np.stack([yy * 6 + xx * 2, 255 - xx * 4, (yy * xx) % 256], -1)
    frames = np.clip(base[None, None] + g.integers(-50, 51, (B, T, SH, SW, 3)), 0, 255).astype(np.uint8)
    masks = ((g.random((B, SH, SW)) < 0.4) * 255).astype(np.uint8)
    return frames, masks


def _input(perturb, warp=False):
    from mumpy_hip.augment import AugmentedInput
    x = torch.full((B, T, 3, L, L), float("nan"), device=DEV)
    target = torch.full((B * L * L,), float("nan"), device=DEV)
    return AugmentedInput(x, target, (SH, SW), nmasks=B, perturb=perturb, warp=warp), x, target


DRAWS = [[("id", None), ("rot90", None)], [("hflip", (2, 1, 13, 12)), ("id", (0, 3, 9, 16))]]


def _canvas(frames, masks):
    from mumpy_hip.augment import nearest_table
    ry, rx = nearest_table(SH, L), nearest_table(SW, L)
    return frames[:, :, ry][:, :, :, rx], masks[:, ry][:, :, rx]


def _stage_on(canvas, mask_canvas, draws):
    """The existing stage on a host-made canvas, with canvas-relative tables."""
    from mumpy_hip.augment import clip_tables
    ops = _ops()
    tabs = [clip_tables((L, L), L, op, box) for op, box in draws]
    ta, tb, sw = (torch.from_numpy(np.stack([np.asarray(t[k]) for t in tabs])).to(DEV) for k in range(3))
    return ops.augment_stage_u8(torch.from_numpy(np.ascontiguousarray(canvas)).to(DEV), ta, tb, sw,
                                masks=torch.from_numpy(np.ascontiguousarray(mask_canvas)).to(DEV))


@pytest.mark.parametrize("draws", DRAWS, ids=["id+rot90", "crops"])
def test_perturb_true_with_every_clip_off_is_the_plain_stage(draws):
    from mumpy_hip.augment import clip_tables
    frames, masks = _clips()
    plain, x0, t0 = _input(False)
    plain.load(frames, masks, [clip_tables((SH, SW), L, op, box) for op, box in draws])
    pert, x1, t1 = _input(True)
    pert.load(frames, masks, [clip_tables((L, L), L, op, box) for op, box in draws], perturb=[None, None])
    torch.cuda.synchronize()
    assert not torch.isnan(x0).any() and GA.same_bits(x1, x0) and GA.same_bits(t1, t0)
    pert.load(frames, masks, [clip_tables((L, L), L, op, box) for op, box in draws])              # perturb omitted: every clip off
    torch.cuda.synchronize()
    assert GA.same_bits(x1, x0) and GA.same_bits(t1, t0)
    with pytest.raises(RuntimeError):
        plain.load(frames, masks, [clip_tables((SH, SW), L, op, box) for op, box in draws], perturb=[None, None])
    with pytest.raises(ValueError):
        pert.load(frames, masks, [clip_tables((L, L), L, op, box) for op, box in draws], perturb=[None])
    with pytest.raises(ValueError):
        pert.load(frames, masks, [clip_tables((L, L), L, op, box) for op, box in draws], perturb=[("jpeg", 0), None])


def _expected(frames, masks, draws, settings):
    canvas, mcanvas = _canvas(frames, masks)
    canvas = canvas.copy()
    for c, s in enumerate(settings):
        if s is not None:
            fn = P.jpeg_roundtrip if s[0] == "jpeg" else P.gaussian_blur
            canvas[c] = np.stack([fn(f, s[1]) for f in canvas[c]])
    return _stage_on(canvas, mcanvas, draws)


@pytest.mark.parametrize("warp", [False, True], ids=["stage", "warp"])
def test_per_clip_settings_equal_the_stage_on_a_numpy_perturbed_canvas(warp):
    from mumpy_hip.augment import clip_tables
    frames, masks = _clips()
    draws = DRAWS[1]
    tabs = [clip_tables((L, L), L, op, box) for op, box in draws]
    inp, x, target = _input(True, warp=warp)
    clean_x, clean_t = _expected(frames, masks, draws, [None, None])
    for settings in ([("jpeg", 40), None], [None, ("blur", 1.5)], [("blur", 0.6), ("jpeg", 95)]):
        inp.load(frames, masks, tabs, perturb=settings)
        want_x, want_t = _expected(frames, masks, draws, settings)
        torch.cuda.synchronize()
        assert GA.same_bits(x, want_x) and not GA.same_bits(x, clean_x)
        assert GA.same_bits(target.view(B, L * L), want_t) and GA.same_bits(want_t, clean_t)         # masks are never perturbed
        off = [c for c, s in enumerate(settings) if s is None]
        assert all(GA.same_bits(x[c], clean_x[c]) for c in off)


def test_a_replay_after_a_second_load_follows_its_settings():
    from mumpy_hip.augment import clip_tables
    frames, masks = _clips()
    draws = DRAWS[0]
    tabs = [clip_tables((L, L), L, op, box) for op, box in draws]
    inp, x, target = _input(True)
    inp.load(frames, masks, tabs, perturb=[("jpeg", 40), None])
    side = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        inp.launch()
        graph.capture_end()
    frames2, masks2 = _clips(seed=8)
    second = [("blur", 2.0), ("jpeg", 65)]
    inp.load(frames2, masks2, tabs, perturb=second)
    torch.cuda.synchronize()
    x.zero_(); target.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want_x, want_t = _expected(frames2, masks2, draws, second)
    assert GA.same_bits(x, want_x) and GA.same_bits(target.view(B, L * L), want_t)
    assert not GA.same_bits(want_x, _expected(frames2, masks2, draws, [("jpeg", 40), None])[0])
