"""GPU: per-clip cross-view pairing (include/mumpy_hip_ext8.h, ops.set_clip_coupling, VideoPredictor(coupling="clip")).

The oracle of every grouped kernel is the FROZEN entry, run on each group's slice of the batch: a grouped launch with G groups must
give, bit for bit, the concatenation of the frozen entry's results on the G slices (a kernel computes a window from the same values
in the same order whatever else the launch holds), G = 1 must be the frozen entry on the whole batch, and so must any G when r = 1.
Module, whole model and predictor are held to the CPU oracle run clip by clip -- and the batch-coupled forward of the same library
must MISS that oracle, or the input could not tell the two pairings apart.

Kernel shapes, (B, H, W, Hs2): (2, 7, 7, 21), (3, 14, 7, 42), (3, 14, 14, 70), (4, 7, 14, 7) -- 1, 2, 4 and 2 q windows per clip,
r = 3, 3, 5 and 1 -- at C = 96 and 192, and one stage-0 sized launch (2, 56, 56, 168) at C = 96.  All of them run the attention
core in its split form (units <= 1,024), so the core has one more case, (6, 56, 56, 168) at C = 96: 1,152 units, the whole form,
against per-clip launches in the split form."""
import numpy as np
import pytest
import torch

import guarded_alloc as GA
from conftest import rel_err, rms_err
from weight_fill import fill_module_, seeded_randn

pytestmark = pytest.mark.gpu
TOL = 1e-3          # the whole-model parity bar
TIGHT = 5e-5        # single operators and modules in fp32 (tests/test_hip_parity.py)
K_ORACLE = 2.0      # the bf16-MFMA route against the parent's bf16 route (tests/test_cva_bf16mm.py)
SCALE = 32 ** -0.5

if torch.cuda.is_available():
    from oracle import mumpy_oracle as O
    DEV = torch.device("cuda:0")

SHAPES = [(2, 7, 7, 21), (3, 14, 7, 42), (3, 14, 14, 70), (4, 7, 14, 7)]
CASES = [(c, *s) for c in (96, 192) for s in SHAPES] + [(96, 2, 56, 56, 168)]
WHOLE_FORM = (96, 6, 56, 56, 168)
ENTRIES = ["sample", "sample_kv", "sample_kv_mm16", "attention", "attention_mm16"]


def _ops():
    from mumpy_hip import ops
    return ops


# ------------------------------------------------------------------------------------------------ the five entries
def _inputs(entry, c, b, h, w, hs2):
    """CPU inputs of one launch: q grid (b, h, w), kv grid (b, hs2, w).  The sampling positions reach outside the window."""
    nq, nkv = b * (h // 7) * (w // 7), b * (hs2 // 7) * (w // 7)
    seed = 1000 * c + 100 * b + h + w + hs2
    if entry.startswith("sample"):
        g = torch.Generator().manual_seed(seed)
        t = {"x2": seeded_randn(seed + 1, b, hs2 * w, c), "pos": torch.rand(nq, 3, 49, 2, generator=g) * 2.6 - 1.3}
        if entry != "sample":
            t["wkv"], t["bkv"] = seeded_randn(seed + 2, 2 * c, c) / c ** 0.5, seeded_randn(seed + 3, 2 * c)
        return t
    return {"q": seeded_randn(seed + 4, b, h * w, c), "kv": seeded_randn(seed + 5, nkv, 49, 2 * c), "pad": _ops().pad_mask()}


def _launch(entry, t, b, h, w, hs2, c, groups):
    """The op on tensors t (a dict of device tensors); groups=None calls it without the keyword, as before it existed."""
    ops = _ops()
    kw = {} if groups is None else {"groups": groups}
    nq = b * (h // 7) * (w // 7)
    if entry == "sample":
        return ops.deform_sample(t["x2"], t["pos"], b, hs2, w, c, nq, **kw)
    if entry.startswith("sample_kv"):
        return ops.deform_sample_kv(t["x2"], t["pos"], t["wkv"], t["bkv"], b, hs2, w, c, nq,
                                    math="bf16" if entry.endswith("mm16") else "fp32", **kw)
    return ops.deform_attention(t["q"], t["kv"], t["pad"], b, h, w, c, hs2 // h, SCALE,
                                math="bf16" if entry.endswith("mm16") else "fp32", **kw)


def _slice(t, g, groups, b):
    """Group g's share of the inputs: clips g b/G .. (g + 1) b/G - 1 and their windows (copies: fresh, aligned buffers)."""
    out = {}
    for k, v in t.items():
        if k in ("wkv", "bkv", "pad"):
            out[k] = v
        else:
            n = v.shape[0] // groups
            out[k] = v[g * n:(g + 1) * n].clone()
    return out


def _frozen_by_slices(entry, t, c, b, h, w, hs2, groups):
    return torch.cat([_launch(entry, _slice(t, g, groups, b), b // groups, h, w, hs2, c, None) for g in range(groups)])


def _guarded(monkeypatch, entry, cpu, c, b, h, w, hs2, groups):
    """The grouped launch under tests/guarded_alloc.py: bands intact, every element of the output written, inputs unchanged.
    -> the output of each guarded run (one per pass of GA.PASSES)."""
    def body(guard):
        return {"out": _launch(entry, {k: guard.tensor(v) for k, v in cpu.items()}, b, h, w, hs2, c, groups)}, (), None
    runs, unguarded = GA.run_both(monkeypatch, [_ops()], body, device=DEV, sync=torch.cuda.synchronize)
    assert unguarded == set()
    return [r["out"] for r in runs]


def _same(a, b):
    return a.shape == b.shape and torch.equal(a, b) and bool(torch.isfinite(a).all())


@pytest.mark.parametrize("c,b,h,w,hs2", CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("entry", ENTRIES)
def test_grouped_launch_is_the_frozen_entry_clip_by_clip(monkeypatch, entry, c, b, h, w, hs2):
    cpu = _inputs(entry, c, b, h, w, hs2)
    dev = {k: v.to(DEV) for k, v in cpu.items()}
    per_clip = _frozen_by_slices(entry, dev, c, b, h, w, hs2, b)           # the frozen entry, one launch per clip
    whole = _launch(entry, dev, b, h, w, hs2, c, None)                     # the frozen entry on the batch: coupled
    for out in _guarded(monkeypatch, entry, cpu, c, b, h, w, hs2, b):      # G = B
        assert _same(out, per_clip)
    assert _same(_launch(entry, dev, b, h, w, hs2, c, 1), whole)           # G = 1
    if hs2 == h:                                                           # r = 1: the two rules coincide
        assert _same(per_clip, whole)
    else:
        assert not torch.equal(per_clip, whole)                            # ... and otherwise the case tells them apart


@pytest.mark.parametrize("entry", ["attention", "attention_mm16"])
def test_attention_core_whole_form_against_split_form_clips(entry):
    """1,152 units: the fp32 launch on the batch takes the one-wave form, the per-clip launches (192 units) the split form; the two
    are documented as bitwise equal, and the mm16 kernel has one form."""
    c, b, h, w, hs2 = WHOLE_FORM
    from mumpy_hip.lib import load_library
    lib = load_library()
    assert lib.mumpy_deform_attention_plan(b, h, w, c, 3) == 0 and lib.mumpy_deform_attention_plan(1, h, w, c, 3) == 1
    dev = {k: v.to(DEV) for k, v in _inputs(entry, c, b, h, w, hs2).items()}
    out = _launch(entry, dev, b, h, w, hs2, c, b)
    assert _same(out, _frozen_by_slices(entry, dev, c, b, h, w, hs2, b))
    assert not torch.equal(out, _launch(entry, dev, b, h, w, hs2, c, None))


@pytest.mark.parametrize("c", [96, 192])
@pytest.mark.parametrize("entry", ENTRIES)
def test_two_groups_of_two_clips(monkeypatch, entry, c):
    """B = 4, G = 2 (r = 3, two q windows per clip): the frozen entry on the two halves -- neither per-clip nor batch-wide."""
    b, h, w, hs2 = 4, 7, 14, 21
    cpu = _inputs(entry, c, b, h, w, hs2)
    dev = {k: v.to(DEV) for k, v in cpu.items()}
    halves = _frozen_by_slices(entry, dev, c, b, h, w, hs2, 2)
    for out in _guarded(monkeypatch, entry, cpu, c, b, h, w, hs2, 2):
        assert _same(out, halves)
    assert not torch.equal(halves, _launch(entry, dev, b, h, w, hs2, c, None))
    assert not torch.equal(halves, _frozen_by_slices(entry, dev, c, b, h, w, hs2, 4))
    q_of, out_of = _ops().cva_pairing(b * 6, b * 2, 2)                      # the host statement agrees on which halves pair
    assert q_of.max() == b * 2 - 1 and set(q_of[:12]) == {0, 1, 2, 3} and set(out_of[:12]) == {0, 1, 2, 3}


def test_ops_refuse_a_bad_grouping_on_real_buffers():
    """... before any launch: the output of a refused call does not exist, and the next valid call is unaffected."""
    ops = _ops()
    c, b, h, w, hs2 = 96, 3, 14, 7, 42
    dev = {k: v.to(DEV) for k, v in _inputs("sample", c, b, h, w, hs2).items()}
    for groups in (0, 2, 4, 6, -3):
        with pytest.raises(ValueError, match="groups"):
            _launch("sample", dev, b, h, w, hs2, c, groups)
    assert _same(_launch("sample", dev, b, h, w, hs2, c, 3), _frozen_by_slices("sample", dev, c, b, h, w, hs2, 3))


# ------------------------------------------------------------------------------------------------ the module
def _windows(x, hs, w):
    """(hs*w, C) raster tokens of one clip -> (nW, 49, C), window-major (window_partition, swin:54-66)."""
    c = x.shape[-1]
    return x.view(hs // 7, 7, w // 7, 7, c).permute(0, 2, 1, 3, 4).reshape(-1, 49, c)


@pytest.fixture(scope="module")
def module_case():
    """SwinDAttention with filled weights (proj_out is not the zero it is initialised to), B = 3 clips of two q windows, and the
    oracle run on each clip alone, for r = 3 and 5."""
    from models.modules.deformableAttention import SwinDAttention
    m = fill_module_(SwinDAttention(96, 3, 0.0, n_groups=3).eval(), "clipc/")
    assert float(m.proj_out.weight.detach().abs().max()) > 0
    sd = {"d." + k: v.detach().clone() for k, v in m.state_dict().items()}
    b, h, w, c = 3, 7, 14, 96
    cases = {}
    with torch.no_grad():
        for r in (3, 5):
            x1, x2 = seeded_randn(310 + r, b, h * w, c), seeded_randn(320 + r, b, r * h * w, c)
            ref = torch.cat([O.swin_dattention(_windows(x1[i], h, w), _windows(x2[i], r * h, w), sd, "d") for i in range(b)])
            cases[r] = (x1.to(DEV), x2.to(DEV), ref)
    return m.to(DEV), (b, h, w, c), cases


def _module_out(m, x1, x2, b, h, w, r, c):
    """attend_raster -> y (nq, 49, C) in the reference's layout: the flat (C, 49) image re-read as (49, C) (deform:403)."""
    with torch.no_grad():
        yt = m.attend_raster(x1, x2, b, h, w, r * h)
    return yt.transpose(1, 2).reshape(-1, 49, c).cpu()


@pytest.mark.parametrize("r", [3, 5])
@pytest.mark.parametrize("route", ["fused", "unfused"])
def test_module_fp32_routes_match_the_per_clip_oracle(monkeypatch, module_case, route, r):
    import models.modules.deformableAttention as DA
    ops = _ops()
    m, (b, h, w, c), cases = module_case
    x1, x2, ref = cases[r]
    if route == "unfused":
        monkeypatch.setitem(DA.FUSED, "sample_kv", False)
        monkeypatch.setitem(DA.FUSED, "out_combine", False)
    assert (ops.cva_math(), ops.matrix_math(), ops.storage(), ops.clip_coupling()) == ("fp32", "fp32", "fp32", "batch")
    was, ops.PROFILE = ops.PROFILE, {}
    try:
        with ops.clip_coupling_as("clip"):
            clip = _module_out(m, x1, x2, b, h, w, r, c)
        names = set(ops.PROFILE)
    finally:
        ops.PROFILE = was
    torch.cuda.synchronize()
    grouped = {"fused": {"mumpy_deform_sample_kv_grouped_fwd", "mumpy_deform_attention_grouped_fwd"},
               "unfused": {"mumpy_deform_sample_grouped_fwd", "mumpy_deform_attention_grouped_fwd"}}[route]
    assert grouped <= names and not any(n.startswith("mumpy_deform_") and "grouped" not in n and "offsets" not in n for n in names)
    batch = _module_out(m, x1, x2, b, h, w, r, c)
    e_clip, e_batch = rel_err(clip, ref), rel_err(batch, ref)
    print(f"SwinDAttention {route} r={r}: rel_err vs per-clip oracle: clip {e_clip:.3e}, batch {e_batch:.3e}")
    assert e_clip < TIGHT
    assert e_batch > TIGHT                                                 # the input tells the two pairings apart


@pytest.mark.parametrize("r", [3, 5])
def test_module_bf16_route_matches_the_per_clip_oracle(module_case, r):
    """The yardstick of tests/test_cva_bf16mm.py: rms error against the oracle within K_ORACLE x that of the parent's bf16 route
    (bf16 matrix math, cva switch off) -- both under the clip setting here, both against the per-clip oracle."""
    ops = _ops()
    m, (b, h, w, c), cases = module_case
    x1, x2, ref = cases[r]
    before = (ops.cva_math(), ops.matrix_math())
    try:
        ops.set_matrix_math("bf16")
        with ops.clip_coupling_as("clip"):
            e_parent = rms_err(_module_out(m, x1, x2, b, h, w, r, c), ref)
            ops.set_cva_math("bf16")
            e_new = rms_err(_module_out(m, x1, x2, b, h, w, r, c), ref)
        e_batch = rms_err(_module_out(m, x1, x2, b, h, w, r, c), ref)
    finally:
        ops.set_cva_math(before[0])
        ops.set_matrix_math(before[1])
    print(f"SwinDAttention bf16 r={r}: rms_err vs per-clip oracle: clip {e_new:.3e}, parent route {e_parent:.3e}, batch {e_batch:.3e}")
    assert e_new <= K_ORACLE * e_parent
    assert e_batch > K_ORACLE * e_parent


def test_forward_keeps_the_reference_pairing_and_takes_groups(module_case):
    """forward(x1, x2) has the reference's signature and no clip boundaries: it pairs over all windows whatever the switch says;
    groups= is explicit.  The attention maps of the visualisation path follow the same grouping."""
    ops = _ops()
    m, (b, h, w, c), cases = module_case
    x1, x2, ref = cases[3]
    x1w = torch.stack([_windows(x1[i], h, w) for i in range(b)]).reshape(-1, 49, c).contiguous()
    x2w = torch.stack([_windows(x2[i], 3 * h, w) for i in range(b)]).reshape(-1, 49, c).contiguous()
    with torch.no_grad():
        plain = m(x1w, x2w)[0]
        with ops.clip_coupling_as("clip"):
            assert torch.equal(m(x1w, x2w)[0], plain)
        y, maps = m(x1w, x2w, return_attention=True, groups=b)
        per_clip = [m(x1w[2 * i:2 * i + 2].contiguous(), x2w[6 * i:6 * i + 6].contiguous(), return_attention=True) for i in range(b)]
    assert rel_err(y.cpu(), ref) < TIGHT and rel_err(plain.cpu(), ref) > TIGHT
    # (not bitwise: the proj_q / proj_out GEMMs pick their kernel by the row count, which differs between 6 windows and 2)
    assert maps.shape == (2 * b, 3 * 3, 49, 49)
    assert rel_err(y.cpu(), torch.cat([p[0] for p in per_clip]).cpu()) < TIGHT
    assert rel_err(maps.cpu(), torch.cat([p[1] for p in per_clip]).cpu()) < TIGHT


# ------------------------------------------------------------------------------------------------ whole model, graph, predictor
HS, WS, NFRAMES, BATCH = 240, 432, 6, 4


def _next_pool_stream():
    return torch.cuda.Stream(device=DEV).cuda_stream


@pytest.fixture(scope="module")
def model():
    """Seeded weights, the three-view model at T = 3, the B = 3 input of tests/test_clip_coupling_host.py, and the oracle on each of
    its clips alone (computed once, never modified).  The captures of this file (one GraphedForward, one graphed predictor) take
    streams from torch's round-robin pool and leave entries in mumpy_hip.streams' registry; as tests/test_threshold_sweep.py does,
    the entries are taken out again afterwards and the pool's pointer is walked on to where it stood."""
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from mumpy_hip import streams
    registry = set(streams._SIDE)
    cycle = [_next_pool_stream()]                                    # one turn of the pool, and the first handle once more
    while len(cycle) < 2 or cycle[-1] != cycle[0]:
        cycle.append(_next_pool_stream())
        assert len(cycle) <= 257, "torch's stream pool does not repeat"
    enc, dec = fill_module_(Encoder().eval()), fill_module_(Decoder().eval())
    sde = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    sdd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    x = seeded_randn(77, 3, 3, 3, 224, 224)
    with torch.no_grad():
        refs = [O.full_forward(sde, sdd, x[i:i + 1]) for i in range(3)]
    ref_logits, ref_feats = torch.cat([r[0] for r in refs]), torch.cat([r[1] for r in refs])
    yield {"enc": enc.to(DEV), "dec": dec.to(DEV), "x": x.to(DEV), "logits": ref_logits, "feats": ref_feats, "cache": {}}
    torch.cuda.synchronize()
    for key in set(streams._SIDE) - registry:
        del streams._SIDE[key]
    for _ in range(len(cycle)):                                      # until the next handle out is cycle[0] again
        if _next_pool_stream() == cycle[-2]:
            break
    else:
        raise AssertionError("the stream pool's pointer was not found again")


def _forward(model, x, coupling):
    from mumpy_hip.pipeline import fused_forward
    ops = _ops()
    with torch.no_grad(), ops.clip_coupling_as(coupling):
        logits, feats = fused_forward(model["enc"], model["dec"], x)
    return logits.clone(), feats.clone()


def test_whole_model_under_clip_coupling_is_the_oracle_clip_by_clip(model):
    ops = _ops()
    assert ops.clip_coupling() == "batch"
    logits, feats = _forward(model, model["x"], "clip")
    coupled, _ = _forward(model, model["x"], "batch")
    alone, _ = _forward(model, model["x"][1:2], "clip")
    assert ops.clip_coupling() == "batch"
    fig = {"logits rel": rel_err(logits.cpu(), model["logits"]), "logits rms": rms_err(logits.cpu(), model["logits"]),
           "feats rel": rel_err(feats.cpu(), model["feats"]), "feats rms": rms_err(feats.cpu(), model["feats"]),
           "coupled rel": rel_err(coupled.cpu(), model["logits"]), "clip 1 of 3 vs alone": rel_err(logits[1:2].cpu(), alone.cpu())}
    print("fused_forward B=3 T=3 vs per-clip oracle: " + ", ".join(f"{k} {v:.3e}" for k, v in fig.items()))
    assert fig["logits rel"] < TOL and fig["logits rms"] < TOL
    assert fig["feats rel"] < TOL and fig["feats rms"] < TOL
    assert fig["coupled rel"] > 3e-3
    assert fig["clip 1 of 3 vs alone"] < TOL
    assert torch.equal(_forward(model, model["x"][1:2], "batch")[0], alone)    # a batch of one: the two settings coincide


def test_graph_keeps_the_coupling_it_was_captured_with(model):
    from mumpy_hip.graph import GraphedForward
    ops = _ops()
    eager, _ = _forward(model, model["x"], "clip")
    coupled, _ = _forward(model, model["x"], "batch")
    assert ops.clip_coupling() == "batch"
    g = GraphedForward(model["enc"], model["dec"], model["x"], coupling="clip")      # captured while the switch says "batch"
    assert g.coupling == "clip" and ops.clip_coupling() == "batch"
    assert torch.equal(g(model["x"])[0], eager) and not torch.equal(eager, coupled)
    try:
        for mode in ("clip", "batch"):
            ops.set_clip_coupling(mode)
            assert torch.equal(g(model["x"])[0], eager)                    # a replay launches what was captured
    finally:
        ops.set_clip_coupling("batch")
    with pytest.raises(ValueError, match="coupling"):
        GraphedForward(model["enc"], model["dec"], model["x"], coupling="x")


@pytest.mark.parametrize("graph", [True, False], ids=["graphed", "eager"])
def test_predictor_frames_are_batch_size_one_results(model, graph):
    """N = 6 frames at batch = 4: the second batch carries two padding clips.  Every frame's logits equal, within TOL, an eager B = 1
    forward of that frame's clip -- whatever shares its batch."""
    from mumpy_hip.video import VideoPredictor, batch_plan
    ops = _ops()
    rng = np.random.default_rng(6)
    frames = torch.from_numpy(rng.integers(0, 256, (NFRAMES, HS, WS, 3), dtype=np.uint8))
    gt = torch.from_numpy((rng.random((NFRAMES, 224, 224)) < 0.3).astype(np.uint8) * 255)
    idx, dest = batch_plan(NFRAMES, 3, BATCH)
    assert dest.shape == (2, BATCH) and (dest[1] < 0).sum() == 2
    if "alone" not in model["cache"]:                                     # the B = 1 forwards, once for both parametrisations
        fd = frames.to(DEV)
        alone = {}
        for bi in range(dest.shape[0]):
            for j in range(BATCH):
                if dest[bi, j] >= 0:
                    clip = ops.clip_window_u8(fd, torch.from_numpy(idx[bi, j:j + 1].astype(np.int32)).to(DEV), (224, 224))
                    alone[int(dest[bi, j])] = _forward(model, clip, "batch")[0][0].cpu()
        model["cache"]["alone"] = alone
    alone = model["cache"]["alone"]
    assert sorted(alone) == list(range(NFRAMES))
    assert ops.clip_coupling() == "batch"
    vp = VideoPredictor(model["enc"], model["dec"], T=3, src_hw=(HS, WS), batch=BATCH, max_frames=8, graph=graph, coupling="clip")
    assert vp.coupling == "clip" and ops.clip_coupling() == "batch"
    seen = {}

    def on_batch(bi, logits, mask):
        for j in range(BATCH):
            if dest[bi, j] >= 0:
                seen[int(dest[bi, j])] = logits[j].clone()
    masks = vp.predict(frames, gt, on_batch=on_batch)
    assert ops.clip_coupling() == "batch"                                  # the global switch is as it was
    assert masks.shape == (NFRAMES, 224, 224) and sorted(seen) == list(range(NFRAMES))
    errs = [rel_err(seen[f].cpu(), alone[f]) for f in range(NFRAMES)]
    print(f"VideoPredictor(coupling='clip', graph={graph}): per-frame logits rel_err vs B=1: " + " ".join(f"{e:.2e}" for e in errs))
    assert max(errs) < TOL
    mv = vp.metric_vector().cpu()
    assert bool(torch.isfinite(mv).all()) and float(mv[2]) == NFRAMES
    with pytest.raises(ValueError, match="coupling"):
        VideoPredictor(model["enc"], model["dec"], T=3, src_hw=(HS, WS), coupling="frame")


def test_training_tape_refuses_the_clip_setting_before_any_launch(model):
    from mumpy_hip import autograd
    ops = _ops()
    was, ops.PROFILE = ops.PROFILE, {}
    try:
        with ops.clip_coupling_as("clip"):
            with pytest.raises(RuntimeError, match="per-clip"):
                autograd.encoder_train(model["enc"], model["x"])
            with pytest.raises(RuntimeError, match="per-clip"):
                autograd.DeformAttentionFn.apply(model["x"], model["x"], SCALE)
            with pytest.raises(RuntimeError, match="per-clip"):
                autograd.DeformSampleFn.apply(model["x"], model["x"])
        launched = set(ops.PROFILE)
    finally:
        ops.PROFILE = was
    assert launched == set() and ops.clip_coupling() == "batch"
