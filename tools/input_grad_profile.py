"""What the gradient with respect to the input clip costs (include/mumpy_hip_ext10.h, encoder_train(input_grad=True),
mumpy_hip.inputgrad) -> profiles/input_gradient.md.

  --mode step     the taped forward + backward of loss = sum(logits * g) at B = 2 and B = 8, T = 5, fp32, eager, device events
                  around synchronised work, two alternating rounds: without input gradient, and with input_grad=True.  On a tree
                  that has no input_grad argument (the commit before it) the second variant is x.requires_grad_() through the old
                  tape: its ATen fold of the tokenizer part, no FAF part.
  --mode pgd      one PGD iteration (taped forward, mask loss, backward to dx, pgd_step) graphed and eager, beside a plain
                  forward + backward with parameter gradients, at B = 2, T = 5.
  --mode kernels  the three new launches and faf_fwd, 20 calls each at B = 2 and B = 8: run it under
                  `rocprofv3 --kernel-trace --stats -- python tools/input_grad_profile.py --mode kernels` for the kernel times.
  --mode bf16     dx at B = 2, T = 5 under each of the three bf16 switches against the fp32 tape's dx, per frame.
"""
import argparse
import inspect
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "multilateral-temporal-view-pyramid-transformer-for-video-inpainting-detection_amd"),
                os.path.join(ROOT, "tests", "golden")]

from models.decoder.decoder import Decoder  # noqa: E402
from models.encoder.encoder import Encoder  # noqa: E402
from mumpy_hip import autograd as A, ops  # noqa: E402
from weight_fill import fill_module_, seeded_randn  # noqa: E402

DEV = "cuda"
HAS_INPUT_GRAD = "input_grad" in inspect.signature(A.encoder_train).parameters


def model(t):
    enc = fill_module_(Encoder(num_frames=t)).eval().to(DEV)
    dec = fill_module_(Decoder(input_token_temporal_dims=[1, 1, t])).eval().to(DEV)
    return enc, dec


def timed(fn, iters):
    """ms per call: events around `iters` calls, the device idle before and after."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def drop_grads(*mods):
    for m in mods:
        for p in m.parameters():
            p.grad = None


def mode_step(args):
    for b in (2, 8):
        t = 5
        enc, dec = model(t)
        x, g = seeded_randn(990, b, t, 3, 224, 224).to(DEV), seeded_randn(991, b, 1, 224, 224).to(DEV)

        def step(with_x):
            xx = x.clone().requires_grad_() if with_x else x
            kw = dict(input_grad=True) if with_x and HAS_INPUT_GRAD else {}
            lg, _ = A.decoder_train(dec, *A.encoder_train(enc, xx, **kw))
            (lg * g).sum().backward()
            drop_grads(enc, dec)
        names = {False: "no input gradient", True: "input_grad=True" if HAS_INPUT_GRAD else "x.requires_grad_() on the old tape (ATen fold, no FAF part)"}
        for w in (False, True):
            for _ in range(args.warmup):
                step(w)
        for rnd in range(2):
            for w in (False, True):
                print(f"step B={b} T={t} round {rnd}: {names[w]}: {timed(lambda: step(w), args.iters):.2f} ms", flush=True)
        del enc, dec
        torch.cuda.empty_cache()


def mode_pgd(args):
    from mumpy_hip.inputgrad import PGDAttack
    b, t = 2, 5
    enc, dec = model(t)
    x = (seeded_randn(990, b, t, 3, 224, 224) * 0.5).to(DEV)
    target = (torch.rand(b, 1, 224, 224, generator=torch.Generator().manual_seed(7)) < 0.1).float().to(DEV)
    graphed = PGDAttack(enc, dec, x, target, 4 / 255, 1 / 255, graph=True)
    eager = PGDAttack(enc, dec, x, target, 4 / 255, 1 / 255, graph=False)

    def plain():
        lg, _ = A.decoder_train(dec, *A.encoder_train(enc, x))
        lg.backward(ops.mask_loss(lg.detach(), target)[1])
        drop_grads(enc, dec)
    for _ in range(args.warmup):
        eager.run(1)
        plain()
    for rnd in range(2):
        print(f"pgd B={b} T={t} round {rnd}: one iteration graphed {timed(lambda: graphed.run(1), args.iters):.2f} ms "
              f"(includes the copy of x into x_adv and the clone of the result), eager {timed(lambda: eager.run(1), args.iters):.2f} ms, "
              f"plain forward + loss + backward with parameter gradients {timed(plain, args.iters):.2f} ms", flush=True)
    print(f"pgd B={b} T={t}: {args.iters} iterations in one run(): graphed {timed(lambda: graphed.run(args.iters), 1) / args.iters:.2f} ms "
          f"per iteration, eager {timed(lambda: eager.run(args.iters), 1) / args.iters:.2f} ms per iteration", flush=True)


def mode_kernels(args):
    from models.modules.dct import FAF
    from mumpy_hip.inputgrad import pgd_bounds
    faf = FAF()
    d, dt = faf._mats(torch.device(DEV))
    eps3, lo3, hi3 = pgd_bounds(4 / 255)
    t = 5
    for b in (2, 8):
        x = seeded_randn(1, b, t, 3, 224, 224).to(DEV)
        dout = seeded_randn(2, b, 9, 224, 224).to(DEV)
        cols = [torch.randn(b * ((t - tv) // tv + 1) * 56 * 56, 48 * tv + (-48 * tv) % 32, device=DEV) for tv in (t, t - 1, 1)]
        xa, dxf = x.clone(), dout[:, :3].contiguous()
        for name, fn in (("faf_fwd", lambda: faf.forward_frame(x, 1)),
                         ("faf_bwd", lambda: ops.faf_bwd(dout, d, dt, faf.lo_hi, faf.mid_lo, faf.mid_hi)),
                         ("tokenize_dx", lambda: ops.tokenize_dx(cols, (t, t - 1, 1), b, t, 224, 224, dxf=dxf, frame=1)),
                         ("pgd_step", lambda: ops.pgd_step(xa, x, x, 0.02, eps3, lo3, hi3))):
            fn()
            print(f"kernels B={b} T={t}: {name}: {timed(fn, 20) * 1e3:.1f} us per call (events around 20 calls, launch gaps included)", flush=True)


def mode_bf16(args):
    """The node under the bf16 switches: per-frame max-norm distance of dx from the fp32 tape's dx (no bar is set on it)."""
    b, t = 2, 5
    enc, dec = model(t)
    x, g = seeded_randn(990, b, t, 3, 224, 224).to(DEV), seeded_randn(991, b, 1, 224, 224).to(DEV)

    def dx_of():
        xx = x.clone().requires_grad_()
        lg, _ = A.decoder_train(dec, *A.encoder_train(enc, xx, input_grad=True))
        (lg * g).sum().backward()
        drop_grads(enc, dec)
        return xx.grad
    ref = dx_of()
    for name, on, off in (("set_matrix_math('bf16')", lambda: ops.set_matrix_math("bf16"), lambda: ops.set_matrix_math("fp32")),
                          ("set_attention_math('bf16')", lambda: ops.set_attention_math("bf16"), lambda: ops.set_attention_math("fp32")),
                          ("set_cva_math('bf16')", lambda: ops.set_cva_math("bf16"), lambda: ops.set_cva_math("fp32"))):
        on()
        try:
            dx = dx_of()
        finally:
            off()
        errs = [float((dx[:, f] - ref[:, f]).abs().max() / ref[:, f].abs().max()) for f in range(t)]
        print(f"bf16 B={b} T={t}: {name}: per-frame rel distance of dx from the fp32 tape {['%.2e' % e for e in errs]}", flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["step", "pgd", "kernels", "bf16"], required=True)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    {"step": mode_step, "pgd": mode_pgd, "kernels": mode_kernels, "bf16": mode_bf16}[a.mode](a)
