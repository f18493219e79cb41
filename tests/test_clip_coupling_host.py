"""CPU only: the host half of per-clip cross-view pairing (ops.cva_pairing, ops.set_clip_coupling, include/mumpy_hip_ext8.h).

  * ops.cva_pairing, the host statement of the kernels' index rule, against a torch statement of the reference applied clip by clip:
    an index tensor sent through `.repeat(r)` (deform:330) and the `(b t) -> b t` regrouping whose t axis is summed (deform:394-395);
  * the header declares exactly the pinned names, each grouped entry its frozen sibling's arguments plus `int groups`;
  * every grouped entry refuses null pointers and a bad grouping with a negative code, nothing launched (the calls made here are
    refusals only, so the test is safe with or without a device);
  * the switch: values, the environment variable in a fresh process, the context manager, the constructors' refusals;
  * the oracle on the input the GPU tests use: the batch-coupled forward is far from the per-clip one (the input discriminates)."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from abi_surface import decls, kind, names_of
from conftest import PKG, ROOT, rel_err, rms_err

EINVAL, ENULL = -1, -3
SAMPLE = ["x2", "pos", "out", "B", "Hs2", "W", "C", "nq", "groups", "stream"]
SAMPLE_KV = ["x2", "pos", "Wkv", "bkv", "kv", "B", "Hs2", "W", "C", "nq", "groups", "stream"]
CORE = ["q", "kv", "padmask", "out", "B", "H", "W", "C", "r", "scale", "groups", "stream"]
ARGS = {
    "mumpy_deform_sample_grouped_fwd": SAMPLE,
    "mumpy_deform_sample_kv_grouped_fwd": SAMPLE_KV,
    "mumpy_deform_sample_kv_mm16_grouped_fwd": SAMPLE_KV,
    "mumpy_deform_attention_grouped_fwd": CORE,
    "mumpy_deform_attention_mm16_grouped_fwd": CORE,
}
FROZEN = {name: name.replace("_grouped", "") for name in ARGS}


def _ops():
    from mumpy_hip import ops
    return ops


# ------------------------------------------------------------------------------------------------ the rule
def reference_pairing(B, nqc, r):
    """(q_of_kv, out_of_kv) of B clips of nqc q windows and r nqc kv windows each, every clip sent through the reference alone:
    x1.repeat(ratio, ...) tiles the clip's q windows r times (deform:330), and `(b t) c h w -> b t c h w` with t = ratio followed
    by the sum over t adds kv results b t + 0 .. b t + r - 1 into output b (deform:394-395)."""
    q_of, out_of = [], []
    for clip in range(B):
        q_local = torch.arange(nqc).repeat(r)                              # the q window each of the r nqc kv windows meets
        slots = torch.arange(r * nqc).reshape(nqc, r)                      # (b t) -> b t: row b holds the kv results summed into b
        out_local = torch.empty(r * nqc, dtype=torch.int64)
        for b in range(nqc):
            out_local[slots[b]] = b
        q_of.append(q_local + clip * nqc)
        out_of.append(out_local + clip * nqc)
    return torch.cat(q_of).numpy(), torch.cat(out_of).numpy()


@pytest.mark.parametrize("B,nqc,r", list(itertools.product([1, 2, 3, 4], [1, 2, 4, 16, 64], [1, 2, 3, 5, 9])))
def test_cva_pairing_is_the_reference_clip_by_clip(B, nqc, r):
    ops = _ops()
    nq, nkv = B * nqc, B * nqc * r
    q_ref, out_ref = reference_pairing(B, nqc, r)
    q, out = ops.cva_pairing(nkv, nq, B)
    assert q.dtype == np.int64 and out.dtype == np.int64 and q.shape == out.shape == (nkv,)
    assert np.array_equal(q, q_ref) and np.array_equal(out, out_ref)
    q1, out1 = ops.cva_pairing(nkv, nq, 1)                                 # G = 1: today's rule
    assert np.array_equal(q1, np.arange(nkv) % nq) and np.array_equal(out1, np.arange(nkv) // r)
    qb, outb = reference_pairing(1, nq, r)                                 # ... which is the reference on the whole batch
    assert np.array_equal(q1, qb) and np.array_equal(out1, outb)
    assert np.array_equal(ops.cva_pairing(nkv, nq)[0], q1)                 # the default
    if r == 1:
        assert np.array_equal(q, q1) and np.array_equal(q, np.arange(nkv))
    elif B > 1:
        assert not np.array_equal(q, q1)


def test_cva_pairing_intermediate_groups_and_refusals():
    ops = _ops()
    for nqc, r in ((1, 3), (2, 3), (4, 5), (16, 2)):
        q, out = ops.cva_pairing(4 * nqc * r, 4 * nqc, 2)                  # B = 4, G = 2: two halves of two clips each
        qh, outh = reference_pairing(1, 2 * nqc, r)
        assert np.array_equal(q, np.concatenate([qh, qh + 2 * nqc])) and np.array_equal(out, np.concatenate([outh, outh + 2 * nqc]))
    for nkv, nq, g in ((12, 4, 3), (12, 4, 0), (12, 4, -1), (12, 5, 1), (12, 0, 1), (0, 4, 1), (12, 4, 8)):
        with pytest.raises(ValueError):
            ops.cva_pairing(nkv, nq, g)


# ------------------------------------------------------------------------------------------------ the header's pinned names
def test_ext8_grouped_entries_are_their_frozen_siblings_plus_groups():
    """Exactly the pinned names, and each grouped entry takes its frozen sibling's arguments plus `int groups` before the stream
    (tests/test_abi.py holds the header to its binding and to both libraries)."""
    assert names_of("mumpy_hip_ext8.h") == dict(ARGS, mumpy_ext8_version=[])
    ext8, frozen = decls("mumpy_hip_ext8.h"), decls("mumpy_hip.h")
    for name in ARGS:
        sib = frozen[FROZEN[name]].args
        assert [kind(a) for a in ext8[name].args] == [kind(a) for a in sib[:-1]] + ["int", "ptr"], name
        assert ext8[name].args[-2] == "int groups"


# ------------------------------------------------------------------------------------------------ refusals through the C ABI
P = 4096                                                                    # a fake, 16-byte aligned, never dereferenced address


def _call(lib, entry, **over):
    """The entry with a tuple that passes every host check (r = 3, two clips) except for the overrides."""
    if entry in ("mumpy_deform_attention_grouped_fwd", "mumpy_deform_attention_mm16_grouped_fwd"):
        v = dict(q=P, kv=P, padmask=P, out=P, B=2, H=7, W=14, C=96, r=3, scale=0.17, groups=2, stream=None)
    else:
        v = {n: P for n in ARGS[entry] if n[0] in "xpoWbk"}
        v.update(B=2, Hs2=21, W=14, C=96, nq=4, groups=2, stream=None)
    v.update(over)
    return getattr(lib, entry)(*[v[n] for n in ARGS[entry]])


@pytest.mark.parametrize("entry", sorted(ARGS))
def test_grouped_entries_refuse_before_launch(entry):
    """Rejected arguments return negative codes before anything is launched, as tests/test_abi.py::test_argument_validation_without_gpu
    has it for the frozen surface: every call here is a refusal."""
    from mumpy_hip.lib import load_library
    lib = load_library()
    core = "attention" in entry
    for ptr in [n for n in ARGS[entry] if n[0] in "xpoWbkq" and n not in ("B", "W")]:
        assert _call(lib, entry, **{ptr: None}) == ENULL and b"null" in lib.mumpy_last_error(), ptr
    tag = entry[len("mumpy_"):-len("_fwd")].encode()
    for bad in (0, -1, -2):
        assert _call(lib, entry, groups=bad) == EINVAL and tag in lib.mumpy_last_error() and b"groups" in lib.mumpy_last_error()
    # groups does not divide nq: 3 q windows (attention: B = 3 clips of one), G = 2
    assert (_call(lib, entry, B=3, H=7, W=7, groups=2) if core else _call(lib, entry, B=2, nq=3, groups=2)) == EINVAL
    assert b"divide" in lib.mumpy_last_error()
    # groups divides nq but not B: 3 clips of two q windows, G = 2
    assert (_call(lib, entry, B=3, groups=2) if core else _call(lib, entry, B=3, Hs2=14, W=14, nq=6, groups=2)) == EINVAL
    assert b"divide" in lib.mumpy_last_error()
    assert _call(lib, entry, groups=4) == EINVAL                           # 4 divides nq = 4 but not B = 2
    if not core:                                                           # nq must divide nkv once there is more than one group
        assert _call(lib, entry, B=2, Hs2=21, W=7, nq=4, groups=2) == EINVAL and b"multiple" in lib.mumpy_last_error()
    # what the sibling refuses is refused with the sibling's code
    assert _call(lib, entry, C=100) == EINVAL and _call(lib, entry, W=15) == EINVAL


def test_ops_refuse_a_bad_grouping_without_a_device():
    """The wrappers restate the refusals ahead of every tensor check, so they need no GPU."""
    ops = _ops()
    x = torch.zeros(1)
    for groups in (0, -1, 2.0, True, None, 4, 3):
        with pytest.raises(ValueError, match="groups"):
            ops.deform_sample(x, x, 2, 21, 14, 96, 4, groups=groups)
        with pytest.raises(ValueError, match="groups"):
            ops.deform_sample_kv(x, x, x, x, 2, 21, 14, 96, 4, groups=groups)
        with pytest.raises(ValueError, match="groups"):
            ops.deform_attention(x, x, x, 2, 7, 14, 96, 3, 0.17, groups=groups)


# ------------------------------------------------------------------------------------------------ the switch
def _child(env_value):
    env = dict(os.environ)
    env.pop("MUMPY_CLIP_COUPLING", None)
    if env_value is not None:
        env["MUMPY_CLIP_COUPLING"] = env_value
    code = f"import sys; sys.path[:0] = [{ROOT!r}, {PKG!r}]; from mumpy_hip import ops; print('MODE=' + ops.clip_coupling())"
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)


def test_clip_coupling_switch_and_environment():
    ops = _ops()
    if not os.environ.get("MUMPY_CLIP_COUPLING"):
        assert ops.clip_coupling() == "batch"
    before = ops.clip_coupling()
    try:
        ops.set_clip_coupling("clip")
        assert ops.clip_coupling() == "clip"
        for bad in ("frame", "", None, 1, "CLIP"):
            with pytest.raises(ValueError):
                ops.set_clip_coupling(bad)
            assert ops.clip_coupling() == "clip"                           # a bad value leaves the switch unchanged
        ops.set_clip_coupling("batch")
        assert ops.clip_coupling() == "batch"
        other = (ops.cva_math(), ops.matrix_math(), ops.storage(), ops.attention_math())
        ops.set_clip_coupling("clip")                                      # it touches no other switch
        assert (ops.cva_math(), ops.matrix_math(), ops.storage(), ops.attention_math()) == other
    finally:
        ops.set_clip_coupling(before)
    for value, mode in ((None, "batch"), ("", "batch"), ("batch", "batch"), ("clip", "clip")):
        r = _child(value)                                                  # fresh processes: they import the package, no GPU
        assert r.returncode == 0 and "MODE=" + mode in r.stdout, r.stderr[-2000:]
    r = _child("frame")
    assert r.returncode != 0 and "ValueError" in r.stderr and "MUMPY_CLIP_COUPLING" in r.stderr and "MODE=" not in r.stdout


def test_clip_coupling_context_manager_restores():
    ops = _ops()
    before = ops.clip_coupling()
    try:
        ops.set_clip_coupling("batch")
        with ops.clip_coupling_as("clip"):
            assert ops.clip_coupling() == "clip"
            with ops.clip_coupling_as("batch"):
                assert ops.clip_coupling() == "batch"
            assert ops.clip_coupling() == "clip"
            with ops.clip_coupling_as(None):                               # None: the body follows the switch as it stands
                assert ops.clip_coupling() == "clip"
        assert ops.clip_coupling() == "batch"
        with pytest.raises(KeyError):
            with ops.clip_coupling_as("clip"):
                assert ops.clip_coupling() == "clip"
                raise KeyError("from the body")
        assert ops.clip_coupling() == "batch"                              # restored on the way out of an exception
        with pytest.raises(ValueError):
            ops.clip_coupling_as("x")
        assert ops.clip_coupling() == "batch"
    finally:
        ops.set_clip_coupling(before)


def test_constructors_refuse_an_unknown_coupling():
    """Before anything is allocated or looked at: no model, no device."""
    from mumpy_hip.graph import GraphedForward
    from mumpy_hip.video import VideoPredictor
    ops = _ops()
    before = ops.clip_coupling()
    for bad in ("x", "", 1):
        with pytest.raises(ValueError, match="coupling"):
            VideoPredictor(None, None, T=3, src_hw=(240, 432), coupling=bad)
        with pytest.raises(ValueError, match="coupling"):
            GraphedForward(None, None, None, coupling=bad)
    with pytest.raises(ValueError, match="coupling"):
        VideoPredictor(None, None, T=3, src_hw=(240, 432), coupling=None)    # the predictor's default is explicit: "batch"
    assert ops.clip_coupling() == before


def test_training_tape_refuses_clip_coupling_without_a_device():
    from mumpy_hip import autograd
    ops = _ops()
    with ops.clip_coupling_as("clip"):
        with pytest.raises(RuntimeError, match="per-clip"):
            autograd.encoder_train(None, None)


# ------------------------------------------------------------------------------------------------ the oracle: the input discriminates
def test_oracle_batch_coupling_differs_from_per_clip_on_the_test_input():
    """O.full_forward on the B = 3, T = 3 input of tests/test_clip_coupling.py, against the same call on each clip alone: the logits
    differ by far more than the 1e-3 parity bar (measured 9.3e-3 rel_err, 5.5e-3 rms_err), so a forward that matches the per-clip
    oracle within 1e-3 cannot be the batch-coupled one."""
    from models.decoder.decoder import Decoder
    from models.encoder.encoder import Encoder
    from oracle import mumpy_oracle as O
    from weight_fill import fill_module_, seeded_randn
    enc, dec = fill_module_(Encoder().eval()), fill_module_(Decoder().eval())
    sde = {k: v.detach().clone() for k, v in enc.state_dict().items()}
    sdd = {k: v.detach().clone() for k, v in dec.state_dict().items()}
    x = seeded_randn(77, 3, 3, 3, 224, 224)
    with torch.no_grad():
        batch = O.full_forward(sde, sdd, x)[0]
        clips = torch.cat([O.full_forward(sde, sdd, x[i:i + 1])[0] for i in range(3)])
    rel, rms = rel_err(batch, clips), rms_err(batch, clips)
    flips = float(((batch > 0) != (clips > 0)).float().mean())
    print(f"oracle, batch-coupled vs per-clip: logits rel_err {rel:.3e}, rms_err {rms:.3e}, mask bits that flip {100 * flips:.3f} %")
    assert rel > 3e-3
