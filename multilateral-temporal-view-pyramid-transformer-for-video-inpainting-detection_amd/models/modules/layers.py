"""Small host-side helpers the reference takes from timm / ml_collections (neither is a dependency here)."""
import collections.abc

import torch
import torch.nn as nn

from mumpy_hip.state import derived_seen, weights_epoch


def to_2tuple(x):
    if isinstance(x, collections.abc.Iterable) and not isinstance(x, str):
        return tuple(x)
    return (x, x)


def trunc_normal_(tensor, mean=0.0, std=1.0, a=-2.0, b=2.0):
    return nn.init.trunc_normal_(tensor, mean=mean, std=std, a=a, b=b)


class DropPath(nn.Module):
    """Stochastic depth.  Identity in eval mode (the inference forward).  The training path (mumpy_hip.autograd
    .drop_path_train) reads `drop_prob` and applies the per-sample mask itself; calling this module in train mode with a
    non-zero rate is refused so that a forward-only call cannot silently skip it."""

    def __init__(self, drop_prob: float = 0.0):
        super().__init__()
        self.drop_prob = float(drop_prob)

    def forward(self, x):
        if self.training and self.drop_prob > 0.0:
            raise NotImplementedError("the inference forward has no stochastic depth: call .eval(), or train through "
                                      "mumpy_hip.autograd (swin_block_train / baseline_encoder_train)")
        return x

    def extra_repr(self):
        return f"drop_prob={self.drop_prob}"


def refuse_stochastic_depth(module):
    """The inference forwards fold the residual add into the GEMM epilogue and never call `drop_path`; in train mode with a
    non-zero rate that would silently skip stochastic depth, so they refuse instead (training goes through mumpy_hip.autograd)."""
    if module.training and getattr(module.drop_path, "drop_prob", 0.0) > 0.0:
        raise NotImplementedError("the inference forward has no stochastic depth: call .eval(), or train through "
                                  "mumpy_hip.autograd (swin_block_train / encoder_train / baseline_encoder_train)")


class ConfigDict(dict):
    """Nested dict with attribute access: the part of ml_collections.ConfigDict the factory and the encoder use
    (item access `cfg["patches"].size`, attribute access `cfg.window_size`)."""

    def __init__(self, d=None):
        super().__init__()
        for k, v in (d or {}).items():
            self[k] = ConfigDict(v) if isinstance(v, dict) and not isinstance(v, ConfigDict) else v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v


class Derived:
    """Cache of a tensor derived from parameters/buffers (transposed weights, expanded bias tables, compacted masks).

    The key is, per source, (storage address, tensor version, device), plus mumpy_hip.state.weights_epoch when any source is an
    nn.Parameter (trainable or frozen).  Followed by themselves, because torch moves the version or the address: load_state_dict,
    a torch.optim step, any in-place op under no_grad (an EMA update, nn.init.*_), `p.data = new`, .to() / .cuda() / .double().
    Followed through the epoch: FlatAdamW / FlatSGD / FlatRMSprop steps (a HIP kernel rewrites the weights; they bump it).
    NOT seen: an in-place edit through `.data` (p.data.mul_(), p.data.copy_()) -- `.data` has a version counter of its own -- and
    an nn.Parameter object swapped for another one while nothing calls the module.  After those call
    mumpy_hip.state.bump_weights_epoch().  Buffer-only keys (attn_mask, relative_position_index) ignore the epoch: no optimizer
    writes them, and rebuilding the compacted mask synchronises with the host, which a captured training step must not do.

    The cache keeps an alias of each source it was built from, so a storage it has seen stays allocated until the next rebuild
    and a replacement (`p.data = new`, a .to() round trip) can never come back at the same address with the same version.
    A copy of the owning module (copy.deepcopy, pickling) starts with an empty cache."""

    def __init__(self):
        self._key = None
        self._val = None
        self._sources = ()
        self._held = ()

    def __reduce__(self):
        return (Derived, ())

    @staticmethod
    def _key_of(sources):
        epoch = weights_epoch[0] if any(isinstance(s, nn.Parameter) for s in sources) else 0
        return (epoch,) + tuple((s.data_ptr(), s._version, s.device) for s in sources)

    @property
    def key(self):
        """What the cached value was built from; a value built later has another key."""
        return self._key

    def current(self):
        """True while the sources of the last get() are what the cached value was built from (fn is not called)."""
        return self._key is not None and self._key == self._key_of(self._sources)

    def get(self, sources, fn):
        seen = derived_seen[0]
        if seen is not None:               # a GraphedForward is warming up: it re-checks these keys before every replay
            seen.append(self)
        key = self._key_of(sources)
        if key != self._key:
            with torch.no_grad():
                self._val = fn()
            self._key = key
            self._sources = tuple(sources)
            self._held = tuple(s.detach() for s in sources)
        return self._val
