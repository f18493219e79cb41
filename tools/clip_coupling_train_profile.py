#!/usr/bin/env python3
"""What training with per-clip cross-view pairing (encoder_train(coupling="clip"), include/mumpy_hip_ext9.h) costs next to the
batch-coupled step.  usage: clip_coupling_train_profile.py [batch] [frames] [--bf16] [--rounds N] [--reps N]

Two GraphedTrainSteps over two copies of the same seeded model (taped forward, mask loss, backward, fused AdamW): one with the
default, batch-coupled tape -- whose cross-view launches are the frozen entries, the instantiations and arguments of the commit
before the grouped backward existed -- and one with coupling="clip".  The two graphs replay alternately, ROUNDS rounds of REPS steps
each; prints the median and the range of the per-step time of both, and their ratio.
--bf16: bf16 matrix math and the bf16-MFMA cross-view attention (config 5's arithmetic), forward and backward."""
import os, sys, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests", "golden"),
                os.path.join(ROOT, "multilateral-temporal-view-pyramid-transformer-for-video-inpainting-detection_amd")]
from weight_fill import fill_module_, seeded_randn
from models.decoder.decoder import Decoder
from models.encoder.encoder import Encoder
from mumpy_hip import ops
from mumpy_hip.autograd import decoder_train, encoder_train
from mumpy_hip.train import GraphedTrainStep, build_optimizers

argv = sys.argv[1:]


def _opt(name, default):
    if name in argv:
        i = argv.index(name)
        v = int(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


ROUNDS, REPS = _opt("--rounds", 12), _opt("--reps", 5)
BF16 = "--bf16" in argv
args = [a for a in argv if not a.startswith("--")]
B = int(args[0]) if args else 2
T = int(args[1]) if len(args) > 1 else 5
dev = torch.device("cuda:0")
if BF16:
    ops.set_matrix_math("bf16")
    ops.set_cva_math("bf16")
x = seeded_randn(1, B, T, 3, 224, 224).to(dev)
target = (torch.rand(B, 1, 224, 224, device=dev, generator=torch.Generator(device=dev).manual_seed(7)) < 0.1).float()
steps, keep = {}, []
for coupling in ("batch", "clip"):
    enc = fill_module_(Encoder(num_frames=T)).eval().to(dev)
    dec = fill_module_(Decoder(input_token_temporal_dims=[1, 1, T])).eval().to(dev)
    opts = build_optimizers(enc, dec, lr_cnn=1e-6, lr=1e-5, lr_cva=1e-6, weight_decay=1e-4, weight_decay_cnn=1e-4)

    def fwd(xx, enc=enc, dec=dec, coupling=coupling):
        return decoder_train(dec, *encoder_train(enc, xx, coupling=None if coupling == "batch" else coupling))[0]
    steps[coupling] = GraphedTrainStep(fwd, opts, x, target)
    # GraphedTrainStep holds the optimizers (hence the flat parameter buffers), not the forward closure: the MODULES -- whose buffers,
    # index images and compacted shift masks the captured launches point at -- live exactly as long as the caller keeps them
    keep.append((enc, dec, opts, fwd))
    for _ in range(2):
        loss = steps[coupling].step()
    torch.cuda.synchronize()
    print(f"{coupling}: captured; loss after the warm-up steps {[round(float(v), 4) for v in loss]}", flush=True)
times = {k: [] for k in steps}
for _ in range(ROUNDS):
    for k, gs in steps.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(REPS):
            gs.step()
        e1.record(); torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) / REPS)
med = {k: sorted(v)[len(v) // 2] for k, v in times.items()}
print(f"graphed train step, B={B}, T={T}, {ops.matrix_math()} matrix math, cva {ops.cva_math()}: "
      + ", ".join(f"{k} {med[k]:.2f} ms [{min(v):.2f}..{max(v):.2f}]" for k, v in times.items())
      + f"; clip / batch = {med['clip'] / med['batch']:.4f}  (medians of {ROUNDS} alternating rounds of {REPS} replayed steps)")
