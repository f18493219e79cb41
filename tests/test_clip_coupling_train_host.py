"""CPU only: the host half of training with per-clip cross-view pairing (include/mumpy_hip_ext9.h, ops.cva_pairing_members, the
groups= argument of ops.deform_sample_bwd / ops.deform_attention_bwd, encoder_train(coupling=)).

  * the header declares exactly the pinned names, each grouped entry its frozen sibling's arguments plus `int groups`;
  * every grouped backward entry refuses null pointers and a bad grouping with a negative code, nothing launched (the calls made
    here are refusals only, so the test is safe with or without a device);
  * the backward ops refuse a bad groups before they look at a tensor;
  * ops.cva_pairing_members, the inverse the bf16 q kernel walks, against ops.cva_pairing;
  * encoder_train: an unknown coupling is a ValueError, and the default call still refuses the global "clip" setting."""
import numpy as np
import pytest
import torch

from abi_surface import decls, kind, names_of

EINVAL, ENULL = -1, -3
SAMPLE = ["x2", "pos", "dsampled", "dx2", "dpos_part", "B2", "C", "nq", "groups", "stream"]
CORE = ["q", "kv", "dout", "dq_part", "dkv", "workspace", "workspace_bytes", "B1w", "r", "C", "scale", "groups", "stream"]
ARGS = {
    "mumpy_deform_sample_grouped_bwd": SAMPLE,
    "mumpy_deform_attention_grouped_bwd": CORE,
    "mumpy_deform_attention_mm16_grouped_bwd": [a if a != "dq_part" else "dq" for a in CORE],
}
FROZEN = {name: (name.replace("_grouped", ""), "mumpy_hip_ext2.h" if "mm16" in name else "mumpy_hip.h") for name in ARGS}


def _ops():
    from mumpy_hip import ops
    return ops


# ------------------------------------------------------------------------------------------------ the header's pinned names
def test_ext9_grouped_entries_are_their_frozen_siblings_plus_groups():
    """Exactly the pinned names, and each grouped entry takes its frozen sibling's arguments plus `int groups` before the stream
    (tests/test_abi.py holds the header to its binding and to both libraries)."""
    assert names_of("mumpy_hip_ext9.h") == dict(ARGS, mumpy_ext9_version=[])
    ext9 = decls("mumpy_hip_ext9.h")
    for name in ARGS:
        sib_name, sib_header = FROZEN[name]
        sib = decls(sib_header)[sib_name].args
        assert [kind(a) for a in ext9[name].args] == [kind(a) for a in sib[:-1]] + ["int", "ptr"], name
        assert ext9[name].args[-2] == "int groups"


# ------------------------------------------------------------------------------------------------ refusals through the C ABI
P = 4096                                                                    # a fake, 16-byte aligned, never dereferenced address


def _call(lib, entry, **over):
    """The entry with a tuple that passes every host check (two groups of two q windows, r = 3) except for the overrides."""
    if entry == "mumpy_deform_sample_grouped_bwd":
        v = dict(x2=P, pos=P, dsampled=P, dx2=P, dpos_part=P, B2=12, C=96, nq=4, groups=2, stream=None)
    else:
        v = {n: P for n in ARGS[entry][:6]}
        v.update(workspace_bytes=1 << 30, B1w=4, r=3, C=96, scale=0.17, groups=2, stream=None)
    v.update(over)
    return getattr(lib, entry)(*[v[n] for n in ARGS[entry]])


@pytest.mark.parametrize("entry", sorted(ARGS))
def test_grouped_backward_entries_refuse_before_launch(entry):
    """Rejected arguments return negative codes before anything is launched, as tests/test_clip_coupling_host.py has it for the
    forward entries: every call here is a refusal."""
    from mumpy_hip.lib import load_library
    lib = load_library()
    core = "attention" in entry
    for ptr in ARGS[entry][:6 if core else 5]:
        assert _call(lib, entry, **{ptr: None}) == ENULL and b"null" in lib.mumpy_last_error(), ptr
    tag = entry[len("mumpy_"):].encode()
    for bad in (0, -1, -2):
        assert _call(lib, entry, groups=bad) == EINVAL and tag in lib.mumpy_last_error() and b"groups" in lib.mumpy_last_error()
    # groups does not divide nq: 3 q windows, G = 2; 4 q windows, G = 3 and G = 8
    assert (_call(lib, entry, B1w=3) if core else _call(lib, entry, B2=9, nq=3)) == EINVAL
    assert b"divide" in lib.mumpy_last_error()
    for bad in (3, 8):
        assert _call(lib, entry, groups=bad) == EINVAL and b"divide" in lib.mumpy_last_error()
    if not core:                                                           # nq must divide nkv once there is more than one group
        assert _call(lib, entry, B2=14) == EINVAL and b"multiple" in lib.mumpy_last_error()
    # what the sibling refuses is refused with the sibling's code
    assert _call(lib, entry, C=100) == EINVAL
    if core:
        assert _call(lib, entry, r=0) == EINVAL and _call(lib, entry, workspace_bytes=16) == EINVAL
        assert _call(lib, entry, groups=1, r=0) == EINVAL                  # ... also on the way to the frozen launch
    else:
        assert _call(lib, entry, B2=0) == EINVAL and _call(lib, entry, groups=1, nq=0) == EINVAL


def test_backward_ops_refuse_a_bad_grouping_without_a_device():
    """The wrappers restate the refusals ahead of every tensor check, so they need no GPU."""
    ops = _ops()
    x, pos, q = torch.zeros(1), torch.zeros(4, 3, 49, 2), torch.zeros(4, 49, 96)
    for groups in (0, -1, 2.0, True, None, 3, 8):
        with pytest.raises(ValueError, match="groups"):
            ops.deform_sample_bwd(x, pos, x, groups=groups)
        for math in ("fp32", "bf16"):
            with pytest.raises(ValueError, match="groups"):
                ops.deform_attention_bwd(q, x, x, 3, 0.17, math=math, groups=groups)
    with pytest.raises(ValueError, match="math"):
        ops.deform_attention_bwd(q, x, x, 3, 0.17, math="fp16", groups=2)


# ------------------------------------------------------------------------------------------------ the inverse rule
@pytest.mark.parametrize("nkv,nq,groups", [(6, 2, 1), (6, 2, 2), (18, 6, 3), (18, 6, 1), (18, 6, 6), (40, 8, 2), (40, 8, 8), (8, 8, 4),
                                           (8, 8, 1), (8, 8, 8), (12, 4, 2), (12, 4, 4), (36, 4, 2), (5, 1, 1), (640, 128, 2)])
def test_cva_pairing_members_is_the_inverse_of_cva_pairing(nkv, nq, groups):
    ops = _ops()
    r = nkv // nq
    members = ops.cva_pairing_members(nkv, nq, groups)
    assert isinstance(members, np.ndarray) and members.dtype == np.int64 and members.shape == (nq, r)
    q_of, out_of = ops.cva_pairing(nkv, nq, groups)
    for qw in range(nq):
        assert members[qw].tolist() == np.nonzero(q_of == qw)[0].tolist()  # exactly the kv windows of qw, ascending
    assert sorted(members.reshape(-1).tolist()) == list(range(nkv))        # every kv window in exactly one row
    if groups == 1:
        assert np.array_equal(members, np.arange(nq)[:, None] + np.arange(r)[None, :] * nq)
        assert np.array_equal(members, ops.cva_pairing_members(nkv, nq))   # the default
    if r == 1:
        assert np.array_equal(members[:, 0], np.arange(nq))
    nqg = nq // groups                                                     # the formula of the device helper (csrc/cva_pairing.h)
    for qw in range(nq):
        g, j = qw // nqg, qw % nqg
        assert members[qw].tolist() == [g * r * nqg + j + m * nqg for m in range(r)]


def test_cva_pairing_members_refusals():
    ops = _ops()
    for nkv, nq, g in ((12, 4, 3), (12, 4, 0), (12, 4, -1), (12, 5, 1), (12, 0, 1), (0, 4, 1), (12, 4, 8)):
        with pytest.raises(ValueError):
            ops.cva_pairing_members(nkv, nq, g)


# ------------------------------------------------------------------------------------------------ the tape's argument
def test_encoder_train_coupling_argument_without_a_device():
    from mumpy_hip import autograd
    ops = _ops()
    for bad in ("bogus", "", 1, "CLIP", True):
        with pytest.raises(ValueError, match="coupling"):
            autograd.encoder_train(None, None, coupling=bad)
    before = ops.clip_coupling()
    with ops.clip_coupling_as("clip"):
        with pytest.raises(ValueError, match="coupling"):                  # ... whatever the switch says
            autograd.encoder_train(None, None, coupling="bogus")
        with pytest.raises(RuntimeError, match="per-clip"):                # the default call does not follow the switch: it refuses
            autograd.encoder_train(None, None)
        with pytest.raises(RuntimeError, match="per-clip") as info:
            autograd.encoder_train(None, None, coupling="batch")
        assert "coupling=" in str(info.value)                              # the message points at the argument
    assert ops.clip_coupling() == before
