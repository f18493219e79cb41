"""A recorder of what mumpy_hip.ops hands to the C ABI (tests/test_ops_handoff.py), beside tests/guarded_alloc.py.

`Recorder.installed(monkeypatch, ops)` replaces two functions of the module for the duration of one call:
  * `ops._p`    returns a `Handed`: an int (the address, so that ctypes tables of pointers can still be packed) that carries the
                tensor itself; `None` stays `None`;
  * `ops._call` appends a `Launch` to `Recorder.log` and returns.  It NEVER calls the library, so in record mode nothing is
                launched, however wrong the arguments are.  Workspace-size queries and the host-only `*_hyper` helpers do not go
                through `_call`; they still reach the library, where they are pure host functions.

A `Launch` keeps the entry name, the scalar arguments (`scalars`: one item per argument position; a pointer position holds "ptr"
or None for a null pointer, a ctypes table of pointers ("ptrs", count), any other ctypes array its values) and, per pointer, a `Ptr`
with the handed tensor's dtype, whether it is on the GPU, contiguity, shape / strides, byte size and the data_ptr() of its storage.
A pointer inside a ctypes table is found again through the addresses `_p` handed out during the same recording.

`judge(valid, mutated, error, kind)` is the verdict of a mutated call against the valid call's hand-off, in this order:
  1. refused          the call raised RuntimeError / ValueError / TypeError and nothing had been recorded: passes.  A refusal after a
                      recorded launch FAILS: the real wrapper would have launched already.  "Before" is counted per wrapper: the
                      recorder also wraps the module's public functions, and a case body that calls gelu and then gelu_bwd is
                      refused cleanly when gelu_bwd raises before ITS first launch (gelu, a complete and valid call, has run);
  2. re-dimensioned   entry names or scalars differ: the wrapper took a dimension from the mutated tensor.  Passes for kind "short"
                      only;
  3. same launch      names and scalars identical: every pointer must be a GPU tensor of the valid hand-off's dtype and at least its
                      byte size, and contiguous -- unless the valid call handed a strided view at that position on purpose (its
                      strides travel as scalars: linear_rows, copy_rows, attention_probs), in which case shape and strides must be
                      the valid ones.
`inplace_problems(launches, tensors)` is rule 4: the storage of every in-place input of the caller must be among the storages
handed; a copy is a lost result."""
import contextlib
import ctypes
import types
from collections import namedtuple

import torch

Ptr = namedtuple("Ptr", "pos dtype gpu contiguous shape strides nbytes storage")
Launch = namedtuple("Launch", "name scalars ptrs")
REFUSALS = (RuntimeError, ValueError, TypeError)


class Handed(int):
    """data_ptr() of a tensor, with the tensor."""

    def __new__(cls, tensor):
        self = super().__new__(cls, tensor.data_ptr())
        self.tensor = tensor
        return self


def _describe(pos, t, on_gpu):
    return Ptr(pos, t.dtype, bool(on_gpu(t)), bool(t.is_contiguous()), tuple(t.shape), tuple(t.stride()),
               t.numel() * t.element_size(), t.untyped_storage().data_ptr())


class Recorder:
    def __init__(self, on_gpu=lambda t: t.is_cuda):
        self.log, self.on_gpu, self._by_address = [], on_gpu, {}
        self._depth, self._mark, self.launched_by_refusing_call = 0, 0, None

    def _tracked(self, fn):
        """fn with the launches of the outermost wrapper call counted: what had been launched when that call raised."""
        def wrapper(*args, **kw):
            if self._depth == 0:
                self._mark = len(self.log)
            self._depth += 1
            try:
                return fn(*args, **kw)
            except BaseException:
                if self._depth == 1:
                    self.launched_by_refusing_call = len(self.log) - self._mark
                raise
            finally:
                self._depth -= 1
        return wrapper

    def _p(self, t):
        if t is None:
            return None
        h = Handed(t)
        self._by_address[int(h)] = t                   # keeps the tensor alive: no address is reused within one recording
        return h

    def _call(self, name, *args, work=0.0):
        scalars, ptrs = [], []
        for pos, a in enumerate(args):
            if isinstance(a, Handed):
                scalars.append("ptr")
                ptrs.append(_describe(pos, a.tensor, self.on_gpu))
            elif isinstance(a, ctypes.Array) and a._type_ is ctypes.c_void_p:
                scalars.append(("ptrs", len(a)))
                for j, address in enumerate(a):
                    if address is None or address not in self._by_address:
                        raise AssertionError(f"{name}: pointer {j} of the table at position {pos} did not pass through ops._p")
                    ptrs.append(_describe((pos, j), self._by_address[address], self.on_gpu))
            elif isinstance(a, ctypes.Array):
                scalars.append(tuple(a))
            elif a is None or isinstance(a, (bool, int, float)):
                scalars.append(a)
            else:
                raise AssertionError(f"{name}: argument {pos} is a {type(a).__name__}: a tensor address that did not pass through ops._p?")
        self.log.append(Launch(name, tuple(scalars), tuple(ptrs)))

    @contextlib.contextmanager
    def installed(self, monkeypatch, module):
        with monkeypatch.context() as m:
            m.setattr(module, "_p", self._p)
            m.setattr(module, "_call", self._call)
            for name, fn in list(vars(module).items()):
                if isinstance(fn, types.FunctionType) and not name.startswith("_"):
                    m.setattr(module, name, self._tracked(fn))
            yield self


def record(monkeypatch, module, fn, on_gpu=lambda t: t.is_cuda):
    """-> (launches, result or None, the refusal raised or None, launches the refusing wrapper call had made).  Any other exception
    propagates.  A refusal raised outside every wrapper (in the case body) counts everything recorded before it."""
    rec = Recorder(on_gpu)
    with rec.installed(monkeypatch, module):
        try:
            return rec.log, fn(), None, 0
        except REFUSALS as e:
            return rec.log, None, e, len(rec.log) if rec.launched_by_refusing_call is None else rec.launched_by_refusing_call


def signature(launches):
    return [(launch.name, launch.scalars) for launch in launches]


def judge(valid, mutated, error, kind, launched=0):
    """-> (verdict, problems): verdict "refused" / "re-dimensioned" / "same launch"; the triple passes iff problems == [].
    launched: how many launches the wrapper call that raised `error` had recorded itself (the last ones of `mutated`)."""
    if error is not None:
        if launched:
            return "refused", [f"refused only after {launched} recorded launch(es) (first {mutated[-launched].name}): {error}"]
        return "refused", []
    if signature(valid) != signature(mutated):
        if kind == "short":
            return "re-dimensioned", []
        diff = next((i for i, (a, b) in enumerate(zip(signature(valid), signature(mutated))) if a != b), min(len(valid), len(mutated)))
        return "re-dimensioned", [f"a {kind} mutation changed the launches (first difference at launch {diff}: "
                                  f"{signature(valid)[diff:diff + 1]} -> {signature(mutated)[diff:diff + 1]})"]
    problems = []
    for v, m in zip(valid, mutated):
        for pv, pm in zip(v.ptrs, m.ptrs):
            where = f"{v.name} argument {pv.pos}"
            if not pm.gpu:
                problems.append(f"{where}: handed a tensor that is not on the GPU")
            if pm.dtype != pv.dtype:
                problems.append(f"{where}: handed {pm.dtype}, the launch reads / writes {pv.dtype}")
            if pm.nbytes < pv.nbytes:
                problems.append(f"{where}: handed {pm.nbytes} bytes, the launch addresses {pv.nbytes}")
            if pv.contiguous and not pm.contiguous:
                problems.append(f"{where}: handed a non-contiguous tensor (strides {pm.strides}) that the kernel addresses as dense")
            if not pv.contiguous and (pm.shape, pm.strides) != (pv.shape, pv.strides):
                problems.append(f"{where}: a strided view by design, handed with shape / strides {pm.shape} / {pm.strides} instead of "
                                f"{pv.shape} / {pv.strides}")
    return "same launch", problems


def inplace_problems(launches, tensors):
    """Rule 4.  tensors: {name: the caller's tensor} of the inputs the op updates in place."""
    handed = {p.storage for launch in launches for p in launch.ptrs}
    return [f"in-place input {name}: no launch was handed the caller's storage (a copy: the result is lost)"
            for name, t in tensors.items() if t.untyped_storage().data_ptr() not in handed]
