"""hipGraph capture of the whole forward (encoder + decoder): ~700 kernel launches become one graph launch, which
removes the Python/ctypes launch overhead that would otherwise bound small-batch throughput.  Every kernel in
libmumpy_hip.so is capture-safe by construction (no allocation, no sync, explicit stream)."""
import torch


class GraphedForward:
    def __init__(self, encoder, decoder, example: torch.Tensor, warmup: int = 2, with_mask: bool = False, coupling=None):
        """with_mask=True captures Decoder.predict_mask: outputs are (logits, uint8 mask, feats), the thresholded mask
        of test.py:100-108 coming out of the same last kernel.
        coupling: "batch" or "clip" -- warm-up and capture run under ops.clip_coupling_as(coupling), whatever the global switch
        says, and leave the switch as they found it.  None: whatever ops.clip_coupling() says now.  Either way the value is kept
        in self.coupling and a re-capture (weights moved) uses it again: a graph never changes its pairing."""
        from . import ops
        if coupling not in (None, "batch", "clip"):
            raise ValueError(f"GraphedForward: coupling must be \"batch\", \"clip\" or None, got {coupling!r}")
        self.coupling = ops.clip_coupling() if coupling is None else coupling
        self.encoder, self.decoder, self.with_mask = encoder, decoder, with_mask
        self.static_x = example.clone()
        self._warmup = warmup
        # every tensor whose ADDRESS the captured launches bake in directly: re-pointing one (`p.data = new`, .to()) needs a new capture
        self._tensors = [t for m in (encoder, decoder) for t in list(m.parameters()) + list(m.buffers())]
        self._capture()

    def _capture(self):
        """The graph bakes in the addresses of the weights AND of the tensors derived from them (transposed tokenizer
        weights, padded relative-position bias, concatenated k|v weights, LayerNorm-folded GEMM operands, KRSC convolution
        images -- models.modules.layers.Derived).  The eager path rebuilds a derived tensor when its sources change; a replay
        makes no eager call, so an old graph would go on reading the old derived tensor (or its freed memory) next to the new
        raw weights.  The capture therefore remembers (1) every Derived cache the warm-up consulted, (2) the address of every
        parameter and buffer and (3) the weights epoch, and __call__ re-captures when any of them has moved.  See __call__ for
        what that follows by itself."""
        from . import state
        # warm-up and capture run on the SAME side stream: the per-stream kept workspaces of the GEMMs (ops._kept_workspace)
        # and the fork/join side streams (keyed by their parent) that the warm-up created are then the ones the captured
        # launches use -- captured on another stream, every GEMM would record a zero-fill of a fresh 17 MB workspace
        # (0.86 ms per forward of fill kernels in the first round-2 profile)
        if getattr(self, "_side", None) is None:
            from .streams import new_distinct_stream       # never a handle that a fork/join side stream already wraps
            self._side = new_distinct_stream(self.static_x.device, (torch.cuda.current_stream().cuda_stream,))
        side = self._side
        seen, state.derived_seen[0] = state.derived_seen[0], []
        try:
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad():          # warm the derived-table caches off the graph
                for _ in range(max(self._warmup, 1)):               # (at least once: this run also lists the caches)
                    self._fwd()
            torch.cuda.current_stream().wait_stream(side)
        finally:
            seen, state.derived_seen[0] = state.derived_seen[0], seen
        derived = list({id(d): d for d in seen}.values())
        from .streams import quiesce_collectives
        quiesce_collectives()                                # device idle; RCCL's watchdog has nothing left to poll (streams.py)
        self.graph = torch.cuda.CUDAGraph()
        # capture_error_mode="thread_local": with a process group alive (one rank per GPU) RCCL's watchdog thread polls events
        # while this thread captures; in the default "global" mode such a call from ANOTHER thread invalidates the capture
        with torch.no_grad(), torch.cuda.graph(self.graph, stream=side, capture_error_mode="thread_local"):
            self.static_out = self._fwd()
        self.weights_epoch = state.weights_epoch[0]
        self._addresses = [t.data_ptr() for t in self._tensors]
        self._derived = [(d, d.key) for d in derived]              # the values the graph reads are the ones built under these keys

    def _stale(self) -> bool:
        from . import state
        if state.weights_epoch[0] != self.weights_epoch:           # a HIP optimizer step or an announced .data edit
            return True
        for d, key in self._derived:                               # a source of a derived tensor moved (version or address), or an
            if d.key != key or not d.current():                    # eager call in between has already rebuilt it somewhere else
                return True
        for t, a in zip(self._tensors, self._addresses):           # a raw weight was re-pointed
            if t.data_ptr() != a:
                return True
        return False

    def _fwd(self):
        from . import ops
        from .pipeline import fused_forward
        with ops.clip_coupling_as(self.coupling):                  # warm-up and capture only: a replay launches what was captured
            return fused_forward(self.encoder, self.decoder, self.static_x, with_mask=self.with_mask)

    def __call__(self, x: torch.Tensor):
        """Returns the static (logits, feats) buffers; contents are overwritten by the next call.

        Weight changes are followed without any call: a torch.optim step, an in-place op under no_grad (EMA, nn.init.*_),
        load_state_dict on the model or on any submodule, `p.data = new`, .to() round trips, and the flat HIP optimizers'
        steps.  The check is host-only (keys of the derived caches, addresses of the parameters; no kernel, no sync) and runs
        while the previous replay is still on the GPU.  An in-place edit through `.data` (p.data.mul_()) or a swapped
        nn.Parameter object is invisible to torch and to this check: call mumpy_hip.state.bump_weights_epoch() after it.
        Mode switches (ops.set_storage, set_matrix_math, set_attention_math, set_cva_math, set_clip_coupling) after capture are
        not followed."""
        if self._stale():
            self._capture()
        self.static_x.copy_(x, non_blocking=True)
        self.graph.replay()
        return self.static_out
