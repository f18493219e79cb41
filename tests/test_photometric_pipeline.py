"""GPU: the photometric operations inside the device paths -- VideoPredictor(perturb=...) with the new kinds and
AugmentedInput(perturb=True, photometric=True).

The oracle of the predictor is an unperturbed predictor that is fed the frames Pillow processed on the host: masks, bank, counts and
metric vector must agree bit for bit, eager and graphed.  The oracle of the input stage is the existing stage (ops.augment_stage_u8)
run on a canvas that numpy resized and processed (mumpy_hip.photometric, which tests/test_photometric_host.py holds to Pillow).
The video, the seeded model and the predictor fixture (with its care for torch's stream pool) are those of
tests/test_perturb_pipeline.py."""
import numpy as np
import pytest
import torch

import guarded_alloc as GA
from gen_photometric_goldens import pil_photometric
from mumpy_hip import perturb as PT
from mumpy_hip import photometric as P
from test_perturb_host import pil_blur, pil_jpeg
from test_perturb_pipeline import (B, DRAWS, L, N, SH, SW, T, _canvas, _clips, _ops, _same_results, _stage_on, _video,  # noqa: F401
                                   predictors)

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    DEV = torch.device("cuda:0")


def _pil(frames, steps):
    out = frames
    for kind, v in steps:
        fn = (lambda a: pil_jpeg(a, v)[0]) if kind == "jpeg" else (lambda a: pil_blur(a, v)) if kind == "blur" else \
            (lambda a: pil_photometric(a, kind, v))
        out = np.stack([fn(a) for a in out])
    return out


SPECS = [[("jpeg", 70), ("contrast", 1.4)], ("equalize", None)]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("spec", SPECS, ids=["jpeg70+contrast1.4", "equalize"])
def test_a_predictor_with_the_new_kinds_equals_a_plain_one_fed_pillows_frames(predictors, graph, spec):
    frames, gt = _video()
    processed = _pil(frames, PT.check_spec(spec))
    assert not np.array_equal(processed, frames)
    pert, plain = predictors(graph, perturb=spec, perturb_chunk=3), predictors(graph)      # chunks of 3, 3 and 1 frames
    pert.reset_metrics(); plain.reset_metrics()
    m_pert = pert.predict(frames, gt).clone()
    m_plain = plain.predict(processed, gt).clone()
    torch.cuda.synchronize()
    assert np.array_equal(pert.frames[:N].cpu().numpy(), processed)               # the uploaded video, processed in place
    assert torch.equal(m_pert, m_plain) and np.unique(m_pert.cpu().numpy()).tolist() == [0, 255]
    _same_results(pert, plain)
    fd = torch.from_numpy(frames).to(DEV)                                         # frames on the device: the caller's tensor is left alone
    pert.reset_metrics()
    assert torch.equal(pert.predict(fd, gt), m_plain) and np.array_equal(fd.cpu().numpy(), frames)


def test_every_new_kind_runs_in_one_list_in_order(predictors):
    frames, _ = _video()
    spec = [("sharpness", 1.8), ("blur", 0.8), ("color", 0.4), ("solarize", 140), ("posterize", 5), ("autocontrast", None),
            ("brightness", 1.2), ("invert", None)]
    vp = predictors(False, perturb=spec, perturb_chunk=4)
    vp.predict(frames)
    torch.cuda.synchronize()
    assert np.array_equal(vp.frames[:N].cpu().numpy(), _pil(frames, PT.check_spec(spec)))


def test_specs_of_the_old_kinds_launch_what_they_did(predictors, monkeypatch):
    ops = _ops()
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a, **kw: (calls.append(name), real(name, *a, **kw))[1])
    frames, _ = _video()
    vp = predictors(False, perturb=[("blur", 1.0), ("jpeg", 70)], perturb_chunk=3)
    vp.predict(frames)
    assert not any("photometric" in n for n in calls)
    assert [n for n in calls if "blur" in n or "jpeg" in n] == ["mumpy_gaussian_blur_u8_fwd"] * 3 + ["mumpy_jpeg_roundtrip_u8_fwd"] * 3
    want = max(int(ops._lib().mumpy_gaussian_blur_workspace_bytes(3, 48, 64)), int(ops._lib().mumpy_jpeg_roundtrip_workspace_bytes(3, 48, 64)))
    assert vp._perturb_ws.numel() == want
    del calls[:]
    vp = predictors(False, perturb=("contrast", 1.4), perturb_chunk=3)
    vp.predict(frames)
    assert [n for n in calls if "photometric" in n or "blur" in n or "jpeg" in n] == ["mumpy_photometric_u8_fwd"] * 3


def test_a_bad_spec_is_refused_in_the_constructor(predictors):
    from mumpy_hip.video import VideoPredictor
    enc, dec, thr = predictors.models
    for bad in (("contrast", None), ("contrast", 17), ("equalize", 1), ("posterize", 9), ("solarize", 300), ("sharpen", 2),
                [("jpeg", 50), ("invert",)], "equalize"):
        with pytest.raises(ValueError):
            VideoPredictor(enc, dec, T=3, src_hw=(48, 64), graph=False, perturb=bad)


# ------------------------------------------------------------------------------------------------ the training input stage
def _input(photometric, perturb=True, warp=False):
    from mumpy_hip.augment import AugmentedInput
    x = torch.full((B, T, 3, L, L), float("nan"), device=DEV)
    target = torch.full((B * L * L,), float("nan"), device=DEV)
    return AugmentedInput(x, target, (SH, SW), nmasks=B, perturb=perturb, warp=warp, photometric=photometric), x, target


def _expected(frames, masks, draws, settings):
    canvas, mcanvas = _canvas(frames, masks)
    canvas = canvas.copy()
    for c, s in enumerate(settings):
        if s is not None:
            fn = PT.jpeg_roundtrip if s[0] == "jpeg" else PT.gaussian_blur if s[0] == "blur" else None
            canvas[c] = np.stack([fn(f, s[1]) if fn else P.apply(f, *s) for f in canvas[c]])
    return _stage_on(canvas, mcanvas, draws)


@pytest.mark.parametrize("warp", [False, True], ids=["stage", "warp"])
def test_per_clip_settings_equal_the_stage_on_a_numpy_processed_canvas(warp):
    from mumpy_hip.augment import clip_tables
    frames, masks = _clips()
    draws = DRAWS[1]
    tabs = [clip_tables((L, L), L, op, box) for op, box in draws]
    inp, x, target = _input(True, warp=warp)
    clean_x, clean_t = _expected(frames, masks, draws, [None, None])
    for settings in ([("contrast", 1.4), None], [("invert", None), ("equalize", None)], [("sharpness", 1.5), ("jpeg", 60)],
                     [("blur", 0.7), ("color", 0.5)], [("autocontrast", None), ("solarize", 100.5)],
                     [("posterize", 3), ("brightness", 0.6)], [None, ("color", 1.5)]):
        inp.load(frames, masks, tabs, perturb=settings)
        want_x, want_t = _expected(frames, masks, draws, settings)
        torch.cuda.synchronize()
        assert GA.same_bits(x, want_x) and not GA.same_bits(x, clean_x), settings
        assert GA.same_bits(target.view(B, L * L), want_t) and GA.same_bits(want_t, clean_t)         # masks are never touched
        off = [c for c, s in enumerate(settings) if s is None]
        assert all(GA.same_bits(x[c], clean_x[c]) for c in off)


@pytest.mark.parametrize("draws", DRAWS, ids=["id+rot90", "crops"])
def test_photometric_true_with_every_clip_off_is_the_plain_stage(draws):
    from mumpy_hip.augment import clip_tables
    frames, masks = _clips()
    plain, x0, t0 = _input(False, perturb=False)
    plain.load(frames, masks, [clip_tables((SH, SW), L, op, box) for op, box in draws])
    inp, x1, t1 = _input(True)
    tabs = [clip_tables((L, L), L, op, box) for op, box in draws]
    inp.load(frames, masks, tabs, perturb=[("invert", None), ("contrast", 0.5)])   # ... and a later load with every clip off undoes it
    inp.load(frames, masks, tabs, perturb=[None, None])
    torch.cuda.synchronize()
    assert not torch.isnan(x0).any() and GA.same_bits(x1, x0) and GA.same_bits(t1, t0)
    inp.load(frames, masks, tabs)
    torch.cuda.synchronize()
    assert GA.same_bits(x1, x0) and GA.same_bits(t1, t0)


def test_photometric_false_is_the_object_as_it_was(monkeypatch):
    from mumpy_hip.augment import AugmentedInput, clip_tables
    ops = _ops()
    frames, masks = _clips()
    tabs = [clip_tables((L, L), L, op, box) for op, box in DRAWS[0]]
    off, x0, _ = _input(False)
    on, x1, _ = _input(True)
    words = 2 * B * L + B * 64 + B * T * 4 + B + B * T                            # tab_a, tab_b, qtab, blur, swap, sel
    assert off.params.numel() == words and on.params.numel() == words + B * T * 4
    assert not hasattr(off, "photo") and on.photo.shape == (B * T, 4) and on.photo.data_ptr() % 16 == 0
    assert off._perturb_ws.numel() == max(int(ops._lib().mumpy_jpeg_roundtrip_workspace_bytes(B * T, L, L)),
                                          int(ops._lib().mumpy_gaussian_blur_workspace_bytes(B * T, L, L)))
    calls = []
    real = ops._call
    monkeypatch.setattr(ops, "_call", lambda name, *a, **kw: (calls.append(name), real(name, *a, **kw))[1])
    off.load(frames, masks, tabs, perturb=[("jpeg", 50), None])
    was = list(calls)
    del calls[:]
    on.load(frames, masks, tabs, perturb=[("jpeg", 50), None])
    torch.cuda.synchronize()
    assert "mumpy_photometric_u8_fwd" not in was and len(was) == 5
    assert calls == was[:4] + ["mumpy_photometric_u8_fwd"] + was[4:] and GA.same_bits(x1, x0)
    with pytest.raises(ValueError):                                               # a new kind needs photometric=True
        off.load(frames, masks, tabs, perturb=[("contrast", 1.4), None])
    with pytest.raises(ValueError):                                               # ... which needs perturb=True
        AugmentedInput(x0, None, (SH, SW), photometric=True)
    with pytest.raises(ValueError):
        on.load(frames, masks, tabs, perturb=[("contrast", 17), None])
    with pytest.raises(ValueError):
        on.load(frames, masks, tabs, perturb=[[("contrast", 1.4), ("invert", None)], None])


def test_a_replay_after_a_second_load_follows_its_settings():
    from mumpy_hip.augment import clip_tables
    frames, masks = _clips()
    draws = DRAWS[0]
    tabs = [clip_tables((L, L), L, op, box) for op, box in draws]
    inp, x, target = _input(True)
    inp.load(frames, masks, tabs, perturb=[("contrast", 1.4), None])
    side = torch.cuda.Stream(priority=-1)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        graph.capture_begin()
        inp.launch()
        graph.capture_end()
    frames2, masks2 = _clips(seed=8)
    second = [("blur", 2.0), ("sharpness", 0.3)]
    inp.load(frames2, masks2, tabs, perturb=second)
    torch.cuda.synchronize()
    x.zero_(); target.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want_x, want_t = _expected(frames2, masks2, draws, second)
    assert GA.same_bits(x, want_x) and GA.same_bits(target.view(B, L * L), want_t)
    assert not GA.same_bits(want_x, _expected(frames2, masks2, draws, [("contrast", 1.4), None])[0])
