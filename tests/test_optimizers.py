"""The reference's other two optimizer branches (utils/utils.py:252-261: SGD with momentum 0.9, RMSprop) on flat buffers, their
choice per parameter group (-optim / -optim_cnn, train.py:209-213), and gradient accumulation in the replayed training step
(train.py:115-120, scripts/train_youtube.sh: --accumulation_steps=8).  CPU tests pin the host logic and the state_dict layouts;
the `gpu` tests run the fused HIP updates against torch.optim and the replayed step against the eager loop."""
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import rel_err
from weight_fill import seeded_randn


def _net():
    """Odd sizes (16-B slot padding) and a spatial convolution (channels_last slot)."""
    return torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.Linear(5, 3), torch.nn.Linear(3, 2))


def _fake_grads(params, seed):
    for i, p in enumerate(params):
        p.grad = seeded_randn(seed + i, *p.shape)


# ----------------------------------------------------------------------------------------------------------- CPU
def test_get_optimizer_maps_the_reference_names():
    """utils/utils.py:252-261: 'sgd' -> SGD(momentum=0.9), 'adam' -> AdamW, 'rmsprop' -> RMSprop; weight decay passed on."""
    from mumpy_hip.train import FlatAdamW, FlatRMSprop, FlatSGD, get_optimizer
    o = get_optimizer("sgd", 1e-3, _net().parameters(), weight_decay=1e-4)
    assert type(o) is FlatSGD and (o.lr, o.momentum, o.weight_decay, o.nesterov) == (1e-3, 0.9, 1e-4, False)
    assert o.momentum_buffer is not None and o.momentum_buffer.numel() == o.param.numel()
    o = get_optimizer("adam", 2e-3, _net().parameters(), weight_decay=1e-4)
    assert type(o) is FlatAdamW and (o.lr, o.weight_decay, o.betas, o.eps) == (2e-3, 1e-4, (0.9, 0.999), 1e-8)
    o = get_optimizer("rmsprop", 3e-3, _net().parameters(), weight_decay=1e-4)
    assert type(o) is FlatRMSprop and (o.lr, o.weight_decay, o.alpha, o.eps, o.momentum) == (3e-3, 1e-4, 0.99, 1e-8, 0.0)
    assert o.momentum_buffer is None                                   # only the state the update needs
    assert FlatSGD(_net().parameters(), lr=0.1).momentum_buffer is None
    with pytest.raises(ValueError, match="adagrad"):
        get_optimizer("adagrad", 1e-3, _net().parameters())


def test_build_optimizers_picks_optim_and_optim_cnn():
    """train.py:209-213: the decoder uses -optim, the encoder and its "cva" group -optim_cnn; rates and decays as before."""
    from models.decoder.decoder import BaselineDecoder
    from mumpy_hip.train import FlatAdamW, FlatRMSprop, FlatSGD, build_optimizers

    class Enc(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.block = torch.nn.Linear(4, 4)
            self.cva = torch.nn.Linear(4, 2)

    def make():
        return Enc(), BaselineDecoder(in_channels=32, features=[32] * 5)
    kw = dict(lr_cnn=1e-6, lr=1e-5, lr_cva=2e-6, weight_decay=1e-3, weight_decay_cnn=1e-4)
    opts = build_optimizers(*make(), optim="sgd", optim_cnn="rmsprop", **kw)
    assert {k: type(v) for k, v in opts.items()} == {"dec": FlatSGD, "enc": FlatRMSprop, "cva": FlatRMSprop}
    assert (opts["dec"].lr, opts["dec"].weight_decay, opts["dec"].momentum) == (1e-5, 1e-3, 0.9)
    assert (opts["enc"].lr, opts["enc"].weight_decay) == (1e-6, 1e-4)
    assert (opts["cva"].lr, opts["cva"].weight_decay) == (2e-6, 1e-3)
    opts = build_optimizers(*make(), **kw)                              # defaults: AdamW everywhere, as before
    assert {k: type(v) for k, v in opts.items()} == {"dec": FlatAdamW, "enc": FlatAdamW, "cva": FlatAdamW}
    assert [(o.lr, o.weight_decay) for o in (opts["enc"], opts["dec"], opts["cva"])] == [(1e-6, 1e-4), (1e-5, 1e-3), (2e-6, 1e-3)]


@pytest.mark.parametrize("kind", ["sgd", "sgd_nesterov", "rmsprop", "rmsprop_momentum"])
def test_flat_state_dicts_are_torch_layouts(tmp_path, kind):
    """FlatSGD / FlatRMSprop state_dicts load into torch.optim.SGD / RMSprop, and a state dict torch wrote after a few steps
    loads back bit-exactly -- both directions through checkpoint.save_checkpoint / load_optimizer_states (weights-only)."""
    from mumpy_hip import checkpoint as C
    from mumpy_hip.train import FlatRMSprop, FlatSGD
    torch.manual_seed(4)
    if kind.startswith("sgd"):
        nest = kind == "sgd_nesterov"
        flat = lambda ps: FlatSGD(ps, lr=9.0)                                               # noqa: E731
        ref_cls, ref_kw = torch.optim.SGD, dict(lr=2e-2, momentum=0.9, weight_decay=1e-4, nesterov=nest)
        keys = ["momentum_buffer"]
    else:
        mom = 0.9 if kind == "rmsprop_momentum" else 0.0
        flat = lambda ps: FlatRMSprop(ps, lr=9.0)                                           # noqa: E731
        ref_cls, ref_kw = torch.optim.RMSprop, dict(lr=2e-2, weight_decay=1e-4, momentum=mom, alpha=0.95, eps=1e-6)
        keys = ["square_avg"] + (["momentum_buffer"] if mom else [])
    net = _net()
    torch_opt = ref_cls(net.parameters(), **ref_kw)
    for s in range(3):
        _fake_grads(net.parameters(), 10 * s)
        torch_opt.step()
    enc = torch.nn.Linear(2, 2)
    C.save_checkpoint(str(tmp_path / "t"), enc, enc, epoch=1, optimizers={"dec": torch_opt})
    sd_torch = C.load_optimizer_states(str(tmp_path / "t"), epoch=1)["dec"]
    mine = flat(_net().parameters())
    mine.load_state_dict(sd_torch)                                                         # torch -> flat
    g = sd_torch["param_groups"][0]
    assert (mine.lr, mine.weight_decay, mine.momentum) == (g["lr"], g["weight_decay"], g["momentum"])
    if kind.startswith("sgd"):
        assert mine.nesterov == g["nesterov"]
    else:
        assert (mine.alpha, mine.eps, mine.steps) == (0.95, 1e-6, 3)
    back = mine.state_dict()
    assert set(back["param_groups"][0]) == set(g)
    for i in range(len(mine.params)):
        assert set(back["state"][i]) == set(sd_torch["state"][i])
        for k in keys:
            assert torch.equal(back["state"][i][k], sd_torch["state"][i][k])
    for i, (p, o) in enumerate(zip(mine.params, mine.offsets)):                             # and the flat buffers themselves
        assert torch.equal(mine._slot(getattr(mine, keys[0]), p, o), sd_torch["state"][i][keys[0]])
    mine.steps, mine.sched_it, mine.lr = 7, 5, 1.5e-2
    C.save_checkpoint(str(tmp_path / "f"), enc, enc, epoch=2, optimizers={"enc": mine})
    sd_mine = C.load_optimizer_states(str(tmp_path / "f"), epoch=2)["enc"]
    twin = ref_cls(_net().parameters(), lr=1.0)
    twin.load_state_dict({k: v for k, v in sd_mine.items() if k != "mumpy"})               # flat -> torch
    assert twin.param_groups[0]["lr"] == 1.5e-2
    for i, p in enumerate(twin.param_groups[0]["params"]):
        for k in keys:
            assert torch.equal(twin.state[p][k], sd_torch["state"][i][k])
    again = flat(_net().parameters())
    again.load_state_dict(sd_mine)
    assert (again.steps, again.sched_it, again.base_lr) == (7, 5, 2e-2)     # base rate: the torch file's, kept by `mine`


def test_sgd_state_dict_before_the_first_step_has_no_state():
    from mumpy_hip.train import FlatSGD
    sd = FlatSGD(_net().parameters(), lr=0.1, momentum=0.9).state_dict()
    assert sd["state"] == {}
    ref = torch.optim.SGD(_net().parameters(), lr=0.1, momentum=0.9)
    assert set(sd["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])
    ref.load_state_dict({k: v for k, v in sd.items() if k != "mumpy"})


def test_loading_another_optimizers_state_dict_is_refused():
    from mumpy_hip.train import FlatAdamW, FlatRMSprop, FlatSGD
    adam_sd = FlatAdamW(_net().parameters(), lr=1e-3).state_dict()
    with pytest.raises(ValueError, match="AdamW.*SGD|SGD.*AdamW"):
        FlatSGD(_net().parameters(), lr=0.1, momentum=0.9).load_state_dict(adam_sd)
    with pytest.raises(ValueError, match="AdamW.*RMSprop|RMSprop.*AdamW"):
        FlatRMSprop(_net().parameters(), lr=0.1).load_state_dict(adam_sd)
    with pytest.raises(ValueError, match="SGD.*AdamW|AdamW.*SGD"):
        FlatAdamW(_net().parameters(), lr=0.1).load_state_dict(torch.optim.SGD(_net().parameters(), lr=0.1).state_dict())


def test_sgd_rejects_dampening_and_nesterov_without_momentum_before_launch():
    """Rejected arguments return MUMPY_EINVAL (-1) before anything is launched: safe without a GPU."""
    import ctypes
    from mumpy_hip.lib import load_library
    lib = load_library()
    assert lib.mumpy_sgd_step(None, None, None, 4, 0.1, 0.9, 0.1, 0.0, 0, 1.0, None) == -1
    assert b"dampening" in lib.mumpy_last_error()
    assert lib.mumpy_sgd_step(None, None, None, 4, 0.1, 0.0, 0.0, 0.0, 1, 1.0, None) == -1
    out = (ctypes.c_float * 8)()
    assert lib.mumpy_sgd_hyper(out, 0.1, 0.9, 0.5, 0.0, 0, 1.0) == -1
    assert lib.mumpy_sgd_hyper(out, 0.25, 0.9, 0.0, 1e-4, 1, 0.5) == 0
    assert list(out)[:4] == [0.5, torch.tensor(1e-4).item(), torch.tensor(0.9).item(), 0.25]   # fp32 of each double
    assert lib.mumpy_rmsprop_hyper(out, 0.25, 0.99, 1e-8, 0.0, 0.0, 1.0) == 0
    assert out[3] == torch.tensor(1 - 0.99, dtype=torch.float64).float().item()
    with pytest.raises(ValueError):
        from mumpy_hip.train import FlatSGD
        FlatSGD(_net().parameters(), lr=0.1, nesterov=True)


# ----------------------------------------------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 262147])
@pytest.mark.parametrize("momentum,nesterov", [(0.0, False), (0.9, False), (0.9, True)])
def test_hip_sgd_matches_torch(n, momentum, nesterov):
    """torch.optim.SGD (what utils/utils.py:254 builds) for 5 steps, weight decay and a gradient scale included.
    (Nesterov without momentum is rejected by torch and by the kernel alike.)"""
    from mumpy_hip import ops
    p0 = seeded_randn(21, n)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.SGD([ref], lr=3e-2, momentum=momentum, weight_decay=1e-2, nesterov=nesterov)
    p = p0.cuda()
    buf = torch.zeros(n, device="cuda") if momentum else None
    for step in range(1, 6):
        g = seeded_randn(100 + step, n)
        ref.grad = g * 0.5
        opt.step()
        ops.sgd_step(p, g.cuda(), buf, lr=3e-2, momentum=momentum, weight_decay=1e-2, nesterov=nesterov, grad_scale=0.5)
    assert rel_err(p.cpu(), ref.data) < 2e-6
    if momentum:
        assert rel_err(buf.cpu(), opt.state[ref]["momentum_buffer"]) < 2e-6


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 1023, 262147])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
def test_hip_rmsprop_matches_torch(n, momentum):
    """torch.optim.RMSprop (utils/utils.py:260, torch defaults: alpha 0.99, eps 1e-8) for 5 steps, weight decay and a
    gradient scale included."""
    from mumpy_hip import ops
    p0 = seeded_randn(22, n)
    ref = torch.nn.Parameter(p0.clone())
    opt = torch.optim.RMSprop([ref], lr=3e-3, momentum=momentum, weight_decay=1e-2)
    p, sq = p0.cuda(), torch.zeros(n, device="cuda")
    buf = torch.zeros(n, device="cuda") if momentum else None
    for step in range(1, 6):
        g = seeded_randn(200 + step, n)
        ref.grad = g * 0.5
        opt.step()
        ops.rmsprop_step(p, g.cuda(), sq, buf, lr=3e-3, momentum=momentum, weight_decay=1e-2, grad_scale=0.5)
    st = opt.state[ref]
    assert rel_err(p.cpu(), ref.data) < 2e-6 and rel_err(sq.cpu(), st["square_avg"]) < 2e-6
    if momentum:
        assert rel_err(buf.cpu(), st["momentum_buffer"]) < 2e-6


def _make_flat(kind, params, lr):
    from mumpy_hip.train import FlatRMSprop, FlatSGD
    if kind == "sgd":
        return FlatSGD(params, lr=lr, weight_decay=1e-4, momentum=0.9)
    if kind == "sgd_nesterov":
        return FlatSGD(params, lr=lr, weight_decay=1e-4, momentum=0.9, nesterov=True)
    if kind == "rmsprop":
        return FlatRMSprop(params, lr=lr, weight_decay=1e-4)
    return FlatRMSprop(params, lr=lr, weight_decay=1e-4, momentum=0.9)


def _state_bufs(o):
    return [b for b in (getattr(o, "momentum_buffer", None), getattr(o, "square_avg", None)) if b is not None]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sgd", "sgd_nesterov", "rmsprop_momentum"])
def test_step_dev_equals_step(kind):
    """After stage_hyper, the capturable step_dev (constants from device memory) is bitwise the eager step."""
    torch.manual_seed(2)
    a, b = _net().cuda(), _net().cuda()
    b.load_state_dict(a.state_dict())
    oa, ob = _make_flat(kind, a.parameters(), 1e-2), _make_flat(kind, b.parameters(), 1e-2)
    ob.enable_device_hyper()
    for s, lr in enumerate([1e-2, 1e-2, 5e-3]):
        ga = seeded_randn(40 + s, oa.grad.numel()).cuda()
        oa.grad.copy_(ga); ob.grad.copy_(ga)
        oa.lr = ob.lr = lr
        oa.step(grad_scale=0.5)
        ob.stage_hyper(0.5)
        ob.step_dev()
    torch.cuda.synchronize()
    assert oa.steps == ob.steps == 3
    assert torch.equal(oa.param, ob.param)
    assert all(torch.equal(x, y) for x, y in zip(_state_bufs(oa), _state_bufs(ob)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sgd", "sgd_nesterov", "rmsprop", "rmsprop_momentum"])
def test_flat_optimizers_train_like_torch(kind):
    """FlatSGD / FlatRMSprop over a module == per-tensor torch.optim.SGD / RMSprop, with the polynomial schedule stepping both
    (as test_flat_adamw_trains_like_torch_adamw)."""
    from mumpy_hip.train import polynomial_lr
    torch.manual_seed(3)
    net = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3)).cuda()
    twin = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3)).cuda()
    twin.load_state_dict(net.state_dict())
    opt = _make_flat(kind, net.parameters(), 1e-2)
    if kind.startswith("sgd"):
        ref = torch.optim.SGD(twin.parameters(), lr=1e-2, weight_decay=1e-4, momentum=0.9, nesterov=opt.nesterov, foreach=False)
    else:
        ref = torch.optim.RMSprop(twin.parameters(), lr=1e-2, weight_decay=1e-4, momentum=opt.momentum, foreach=False)
    x = seeded_randn(5, 16, 7).cuda()
    for it in range(1, 9):
        for model in (net, twin):
            model(x).square().mean().backward()                  # autograd writes into the flat gradient views
        assert all(p.grad.data_ptr() >= opt.grad.data_ptr() for p in net.parameters())
        opt.step()
        ref.step()
        opt.zero_grad()
        ref.zero_grad()
        lr = opt.scheduler_step(iter_max=6)
        for gparam in ref.param_groups:
            gparam["lr"] = polynomial_lr(1e-2, gparam["lr"], it, 6)
        assert lr == ref.param_groups[0]["lr"]
    for a, b in zip(net.parameters(), twin.parameters()):
        assert rel_err(a.detach().cpu(), b.detach().cpu()) < 1e-5


def _decoder_case():
    from weight_fill import fill_module_
    from models.decoder.decoder import BaselineDecoder
    dev = torch.device("cuda:0")
    target = (seeded_randn(401, 2, 1, 224, 224) > 1.0).float().to(dev)

    def make(kind, lr):
        dec = fill_module_(BaselineDecoder(in_channels=64, features=[128] * 5)).eval().to(dev)
        return dec, _make_flat(kind, dec.parameters(), lr)
    return dev, target, make


@pytest.mark.gpu
@pytest.mark.parametrize("two_graphs", [False, True])
def test_graphed_train_step_with_sgd_equals_eager_steps(two_graphs):
    """GraphedTrainStep drives FlatSGD unchanged: the replayed trajectory (SGD constants staged in device memory) equals
    eager steps, learning-rate changes included (as test_graphed_train_step_equals_eager_steps for AdamW)."""
    from mumpy_hip import ops
    from mumpy_hip.autograd import baseline_decoder_train
    from mumpy_hip.train import GraphedTrainStep
    dev, target, make = _decoder_case()
    x = seeded_randn(400, 2, 64, 7, 7).to(dev)
    lrs = [1e-3, 1e-3, 1e-3, 5e-4, 2.5e-4, 1e-4]
    dec_e, opt_e = make("sgd", lrs[0])
    for lr in lrs:                                                        # eager reference trajectory
        opt_e.lr = lr
        logits = baseline_decoder_train(dec_e, x)
        loss3, dl = ops.mask_loss(logits.detach(), target)
        logits.backward(dl)
        opt_e.step()
        opt_e.zero_grad()
    dec_g, opt_g = make("sgd", lrs[0])
    gs = GraphedTrainStep(lambda xx: baseline_decoder_train(dec_g, xx), [opt_g], x, target, warmup=3, all_reduce=two_graphs)
    for lr in lrs[3:]:
        opt_g.lr = lr
        gs.step()
        assert gs.updated
    torch.cuda.synchronize()
    assert opt_g.steps == opt_e.steps == len(lrs)
    assert rel_err(opt_g.param.cpu(), opt_e.param.cpu()) < 1e-5
    assert rel_err(opt_g.momentum_buffer.cpu(), opt_e.momentum_buffer.cpu()) < 1e-5


@pytest.mark.gpu
@pytest.mark.parametrize("all_reduce", [False, True])
@pytest.mark.parametrize("kind", ["sgd", "rmsprop"])
@pytest.mark.parametrize("k", [2, 3])
def test_graphed_train_step_accumulates_like_the_eager_loop(k, kind, all_reduce):
    """GraphedTrainStep(accumulation_steps=k): every step() is one micro-batch (its own x), the loss gradient scaled by 1/k and
    accumulated; every k-th micro-batch -- counted across warm-up and replays -- runs the update.  Equals the eager loop of
    INTEGRATION 2b (loss_scale = 1/k, update when (iteration + 1) % k == 0), learning-rate changes included."""
    from mumpy_hip import ops
    from mumpy_hip.autograd import baseline_decoder_train
    from mumpy_hip.train import GraphedTrainStep
    dev, target, make = _decoder_case()
    total, warmup = 4 * k, 3
    n_warm = max(warmup, k)
    xs = [seeded_randn(500 + i, 2, 64, 7, 7).to(dev) for i in range(total)]
    xs[:n_warm] = [xs[0]] * n_warm                         # the warm-up micro-batches replay the constructor's x
    lrs = [1e-3, 5e-4, 2.5e-4, 1e-4]                       # one rate per update
    dec_e, opt_e = make(kind, lrs[0])
    for i, x in enumerate(xs):                             # eager reference
        logits = baseline_decoder_train(dec_e, x)
        loss_e, dl = ops.mask_loss(logits.detach(), target, loss_scale=1.0 / k)
        logits.backward(dl)
        if (i + 1) % k == 0:
            opt_e.lr = lrs[i // k]
            opt_e.step()
            opt_e.zero_grad()
    dec_g, opt_g = make(kind, lrs[0])
    gs = GraphedTrainStep(lambda xx: baseline_decoder_train(dec_g, xx), [opt_g], xs[0], target, warmup=warmup,
                          all_reduce=all_reduce, accumulation_steps=k)
    assert gs.graph_update is not None and gs.iteration == n_warm
    assert opt_g.steps == n_warm // k
    for i in range(n_warm, total):
        opt_g.lr = lrs[i // k]
        loss_g = gs.step(xs[i])
        assert gs.updated == ((i + 1) % k == 0)
    torch.cuda.synchronize()
    assert gs.iteration == total
    assert opt_g.steps == opt_e.steps == total // k
    assert rel_err(opt_g.param.cpu(), opt_e.param.cpu()) < 1e-5
    for a, b in zip(_state_bufs(opt_g), _state_bufs(opt_e)):
        assert rel_err(a.cpu(), b.cpu()) < 1e-5
    assert rel_err(loss_g.cpu(), loss_e.cpu()) < 1e-5      # [total / k, iou, focal]
    assert float(opt_g.grad.abs().max()) == 0.0            # the cycle ended with an update: gradients reset


@pytest.mark.gpu
def test_checkpoint_resume_with_sgd_continues_the_same_trajectory(tmp_path):
    """save -> load -> continue == never having stopped, for FlatSGD: parameters, momentum buffer, step and scheduler counters."""
    from mumpy_hip import checkpoint as C
    from mumpy_hip.train import FlatSGD

    def make():
        torch.manual_seed(8)
        return torch.nn.Sequential(torch.nn.Linear(9, 8), torch.nn.GELU(), torch.nn.Linear(8, 4)).cuda()

    x = seeded_randn(6, 32, 9).cuda()

    def run(net, opt, n):
        for _ in range(n):
            net(x).square().mean().backward()
            opt.step()
            opt.zero_grad()
            opt.scheduler_step(iter_max=20)

    a = make(); oa = FlatSGD(a.parameters(), lr=1e-2, weight_decay=1e-3, momentum=0.9)
    run(a, oa, 10)                                                        # the uninterrupted run
    b = make(); ob = FlatSGD(b.parameters(), lr=1e-2, weight_decay=1e-3, momentum=0.9)
    run(b, ob, 4)
    C.save_checkpoint(str(tmp_path), b, b, epoch=0, optimizers={"dec": ob})
    c = make(); oc = FlatSGD(c.parameters(), lr=123.0)                    # a fresh process: wrong rate, no momentum buffer
    e, _, _ = C.load_checkpoint(str(tmp_path), epoch=0)
    c.load_state_dict(e, strict=True)
    oc.load_state_dict(C.load_optimizer_states(str(tmp_path), epoch=0)["dec"])
    run(c, oc, 6)
    assert torch.equal(oc.param, oa.param) and torch.equal(oc.momentum_buffer, oa.momentum_buffer)
    assert (oc.steps, oc.sched_it, oc.lr, oc.momentum) == (oa.steps, oa.sched_it, oa.lr, 0.9)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _sgd_ddp_worker(rank, world, port, q):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from conftest import PKG  # noqa: F401
    from weight_fill import fill_module_
    from models.modules.swinTransformer import SwinTransformerBlock
    from mumpy_hip import distributed as D
    from mumpy_hip.autograd import swin_block_train
    from mumpy_hip.train import FlatSGD
    D.init_process_group("gloo")
    dev = torch.device("cuda:0")
    blk = fill_module_(SwinTransformerBlock(dim=96, input_resolution=(14, 14), num_heads=3, window_size=7, shift_size=3)).to(dev)
    opt = FlatSGD(blk.parameters(), lr=1e-2, weight_decay=1e-4, momentum=0.9)
    x = seeded_randn(300 + rank, 2, 196, 96).to(dev)               # this rank's micro-batch
    g = seeded_randn(310 + rank, 2, 196, 96).to(dev)
    swin_block_train(blk, x).backward(g)
    scale = opt.all_reduce_grads(bucket_bytes=1 << 16)               # several buckets
    opt.step(grad_scale=scale)
    q.put((rank, opt.param.cpu().numpy(), opt.momentum_buffer.cpu().numpy()))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_two_rank_sgd_step_matches_accumulated_single_process():
    """Two ranks (gloo, sharing the one GPU), one Swin block, one FlatSGD step after the bucketed all-reduce: both replicas are
    identical and equal one process that accumulated both micro-batches' gradients and stepped with grad_scale = 1/2."""
    from weight_fill import fill_module_
    from models.modules.swinTransformer import SwinTransformerBlock
    from mumpy_hip.autograd import swin_block_train
    from mumpy_hip.train import FlatSGD
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_sgd_ddp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = {r: (torch.from_numpy(a), torch.from_numpy(b)) for r, a, b in (q.get(timeout=300) for _ in procs)}
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    dev = torch.device("cuda:0")
    blk = fill_module_(SwinTransformerBlock(dim=96, input_resolution=(14, 14), num_heads=3, window_size=7, shift_size=3)).to(dev)
    opt = FlatSGD(blk.parameters(), lr=1e-2, weight_decay=1e-4, momentum=0.9)
    for rank in range(2):                                            # autograd accumulates into the flat gradient views
        swin_block_train(blk, seeded_randn(300 + rank, 2, 196, 96).to(dev)).backward(seeded_randn(310 + rank, 2, 196, 96).to(dev))
    opt.step(grad_scale=0.5)
    assert rel_err(res[0][0], opt.param.cpu()) < 1e-6
    assert rel_err(res[0][1], opt.momentum_buffer.cpu()) < 1e-6
