"""Time stage 1 on the GPU: one fp16 Stage1Trainer step at the reference crop (4 x 3 x 256 x 256), and the codebook layer's new launches
(csrc/vq_train.hip) alone against the same step's glare_vq_nearest_f32 launch, on the step's own token count (4 x 64 x 64) and on
the largest the layer is specified for (8 x 16 275).  Device events around repeated launches on preallocated buffers; every shape is
warmed up first.  `python tools/stage1_time.py [--out profiles/stage1_step.txt]`

`--gan`: instead, the same step with and without the patch discriminator (disc_start = 0) in one session, and every launch the discriminator
adds timed alone at the step's shapes (8 = 4 real + 4 fake images, two batch groups); for the four 64-to-512-channel conv layers the share of
the dense 16-bit peak their forward, data-gradient and weight-gradient launches reach.
`python tools/stage1_time.py --gan [--out profiles/stage1_gan_step.txt]`

`--lpips`: the same step without the term, with the LPIPS term (losses.LPIPSLoss on seeded weights), with the discriminator, and with both,
in one session; then the LPIPS head's two kernels alone at every tap of that step (the largest: 4 x 256 x 256 x 64) in GB/s of the bytes
they must move (forward: a and b read once; backward: a and b read, da written).
`python tools/stage1_time.py --lpips [--out profiles/stage1_lpips_step.txt]`"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from glare_amd import _lib  # noqa: E402
from glare_amd import modules as M  # noqa: E402
from glare_amd._lib import check, ptr, stream_handle  # noqa: E402
from glare_amd.synthetic import seeded_init_  # noqa: E402
from glare_amd.train import Stage1Trainer  # noqa: E402


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def launches(N, K, reps):
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(N)
    z, E, gr = (torch.randn(n, 3, generator=g).to(dev) for n in (N, K, N))
    idx, zq, st, dz = torch.empty(N, dtype=torch.int64, device=dev), torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
    s, gl, de = torch.empty(1, device=dev), torch.full((1,), 65536.0, device=dev), torch.empty(K, 3, device=dev)
    lib = _lib.lib()
    nws = lib.glare_vq_train_workspace_bytes(N, K)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    cz, ce = 2 * 0.25 / (3 * N), 2.0 / (3 * N)
    near = lambda: check(lib.glare_vq_nearest_f32(ptr(z), ptr(E), N, K, 3, ptr(idx), ptr(zq), stream_handle()), "vq_nearest")
    fwd = lambda: check(lib.glare_vq_loss_sum_f32(ptr(z), ptr(zq), N, 3, ptr(st), ptr(s), ptr(ws), nws, stream_handle()), "vq_loss_sum")
    bwd = lambda: check(lib.glare_vq_backward_f32(ptr(z), ptr(zq), ptr(idx), ptr(gr), ptr(gl), N, K, 3, cz, ce, ptr(dz), ptr(de), ptr(ws), nws,
                                                  stream_handle()), "vq_backward")
    bwd_dz = lambda: check(lib.glare_vq_backward_f32(ptr(z), ptr(zq), ptr(idx), ptr(gr), ptr(gl), N, K, 3, cz, ce, ptr(dz), None, ptr(ws), nws,
                                                     stream_handle()), "vq_backward")
    near()
    return {"vq_nearest": timed(near, reps), "vq_loss_sum": timed(fwd, reps), "vq_backward": timed(bwd, reps), "vq_backward dz only": timed(bwd_dz, reps)}


PEAK_TFLOPS = 2500.0      # dense bf16 / fp16 MFMA peak of one MI355X (spec)


def gan(args):
    """The fp16 step at 4 x 3 x 256^2 without and with the discriminator, then D's launches one by one."""
    from glare_amd import ops
    from glare_amd import train_ops as T

    dev = torch.device("cuda", 0)
    lines = ["stage 1 with the patch discriminator on %s (tools/stage1_time.py --gan; device events, warmed up, ms; one session)"
             % torch.cuda.get_device_name(0)]
    x = torch.rand(4, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(dev)
    res = {}
    for name in ("plain", "gan"):
        torch.manual_seed(0)
        disc = M.NLayerDiscriminator().to(dev) if name == "gan" else None
        tr = Stage1Trainer(seeded_init_(M.VQModel().train(), 1).to(dev), precision="fp16", discriminator=disc, disc_start=0)
        tr.opt.scale.fill_(1024.0)
        if disc is not None:
            tr.opt_d.scale.fill_(1024.0)
        res[name] = timed(lambda: tr.step_tensor(x), args.steps, warm=3)
        lines.append("Stage1Trainer.step_tensor fp16, 4 x 3 x 256 x 256, %-5s (eager, %d steps): %.2f ms per step, generator steps applied %d of %d%s"
                     % (name, args.steps, res[name], tr.opt.t, args.steps + 3, "" if disc is None else ", discriminator %d" % tr.opt_d.t))
        del tr
    lines.append("the discriminator's share of the step: %.2f ms = %.1f %% (the parent commit measured 34.3 ms for the plain step on another day:"
                 " quoted, not compared)" % (res["gan"] - res["plain"], 100 * (res["gan"] - res["plain"]) / res["gan"]))
    lines.append("")
    lines.append("the discriminator's launches alone, 8 x 3 x 256 x 256 (real + fake), fp16, %d launches each:" % args.reps)
    lines.append("  %-34s %9s %9s %8s" % ("launch", "ms", "GFLOP", "of peak"))
    total = 0.0
    with ops.use_precision("fp16"), torch.no_grad():
        g = torch.Generator().manual_seed(1)
        layers = ((3, 64, 2, 256), (64, 128, 2, 128), (128, 256, 2, 64), (256, 512, 1, 32), (512, 1, 1, 31))
        for i, (cin, cout, stride, side) in enumerate(layers, 1):
            xin = torch.rand(8, side, side, cin, generator=g).to(dev)
            if cin != 3:
                xin = xin.to(ops.act_dtype())
            w = (torch.randn(cout, cin, 4, 4, generator=g) * 0.02).to(dev)
            o = T.conv4x4_out(side, stride)
            g16 = torch.randn(8, o, o, max(cout, 8), generator=g).to(dev).to(ops.act_dtype())
            gf = 2.0 * 8 * o * o * 16 * cin * cout / 1e9
            rows = [("conv%d %d->%d s%d forward" % (i, cin, cout, stride), lambda: T.conv4x4_forward(xin, w, stride=stride, lrelu=i == 1, out_f32=i == 5)),
                    ("conv%d data gradient" % i, lambda: T.conv4x4_dgrad(g16, w, (8, side, side, cin), stride=stride, out_f32=cin == 3)),
                    ("conv%d weight gradient" % i, lambda: T.conv4x4_weight_grad(xin, g16, cout, stride))]
            for label, fn in rows:
                ms = timed(fn, args.reps)
                total += ms
                peak = "%7.2f%%" % (100 * gf / ms / PEAK_TFLOPS) if 64 <= cin and cout >= 64 else "       -"
                lines.append("  %-34s %9.4f %9.3f %s" % (label, ms, gf, peak))
            if 2 <= i <= 4:
                y = torch.randn(8, o, o, cout, generator=g).to(dev).to(ops.act_dtype())
                ga, be = torch.ones(cout, device=dev), torch.zeros(cout, device=dev)
                _, saved = T.batchnorm_forward(y, ga, be, groups=2)
                for label, fn in (("batchnorm%d + lrelu forward (4 launches)" % i, lambda: T.batchnorm_forward(y, ga, be, groups=2)),
                                  ("batchnorm%d + lrelu backward (3)" % i, lambda: T.batchnorm_backward(y, y, saved, ga, be, groups=2))):
                    ms = timed(fn, args.reps)
                    total += ms
                    lines.append("  %-34s %9.4f %9s %s" % (label, ms, "-", "       -"))
        logits = torch.randn(4, 30, 30, 1, generator=g).to(dev)
        ms = timed(lambda: T.hinge_loss(logits, "real"), args.reps)
        total += 3 * ms
        lines.append("  %-34s %9.4f %9s %s" % ("hinge reduction (2 launches), x 3", ms, "-", "       -"))
    lines.append("  sum of the launches above (the weight-gradient rows include im2col_t, transpose, GEMM and the packs): %.3f ms" % total)
    return lines


def seeded_lpips(dev, seed=1):
    """LPIPSLoss on name-seeded weights in a regime where every tap carries signal (filters at He's gain, non-negative heads)."""
    import math

    from glare_amd import losses

    net = seeded_init_(losses.LPIPSLoss(), seed)
    const = losses.LPIPSLoss().state_dict()
    with torch.no_grad():
        for k, v in net.state_dict().items():
            if k.startswith("scaling_layer."):
                v.copy_(const[k])
            elif k.startswith("net.") and k.endswith(".weight"):
                v.mul_(math.sqrt(6.0))
            elif k.startswith("lin"):
                v.copy_(v.abs() * math.sqrt(v.shape[1]))
    return net.to(dev)


def lpips(args):
    """The fp16 step at 4 x 3 x 256^2: plain, + LPIPS, + discriminator, + both; then the head's kernels per tap."""
    from glare_amd import ops
    from glare_amd import train_ops as T

    dev = torch.device("cuda", 0)
    lines = ["stage 1 with the LPIPS term on %s (tools/stage1_time.py --lpips; device events, warmed up, ms; one session)"
             % torch.cuda.get_device_name(0)]
    x = torch.rand(4, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(dev)
    res = {}
    for name, with_lpips, with_gan in (("plain", False, False), ("lpips", True, False), ("gan", False, True), ("lpips + gan", True, True)):
        torch.manual_seed(0)
        disc = M.NLayerDiscriminator().to(dev) if with_gan else None
        tr = Stage1Trainer(seeded_init_(M.VQModel().train(), 1).to(dev), precision="fp16", discriminator=disc, disc_start=0,
                           perceptual=seeded_lpips(dev) if with_lpips else None)
        tr.opt.scale.fill_(1024.0)
        if disc is not None:
            tr.opt_d.scale.fill_(1024.0)
        res[name] = timed(lambda: tr.step_tensor(x), args.steps, warm=3)
        lines.append("Stage1Trainer.step_tensor fp16, 4 x 3 x 256 x 256, %-11s (eager, %d steps): %.2f ms per step, generator steps applied %d of %d"
                     % (name, args.steps, res[name], tr.opt.t, args.steps + 3))
        del tr
    lines.append("the LPIPS term's share: %.2f ms without the discriminator, %.2f ms with it" % (res["lpips"] - res["plain"], res["lpips + gan"] - res["gan"]))
    lines.append("the parent commit's profiles/stage1_gan_step.txt has 34.4 ms (plain) / 39.3 ms (gan) from another session: re-measured above, quoted not compared")
    lines.append("")
    lines.append("the LPIPS head's kernels alone at the step's taps, fp16, %d launches each (forward: 2 launches; GB/s of the bytes that must move):" % args.reps)
    lines.append("through the Python wrappers (train_ops: three allocations per forward, one per backward) | the C entry points on preallocated buffers")
    lines.append("  %-22s %10s %10s %10s %10s | %10s %10s %10s %10s" % (("tap B x H x W x C",) + ("fwd ms", "fwd GB/s", "bwd ms", "bwd GB/s") * 2))
    from glare_amd import _lib

    with ops.use_precision("fp16"), torch.no_grad():
        lib, sh = _lib.lib(), _lib.stream_handle
        g = torch.Generator().manual_seed(1)
        for side, C in ((256, 64), (128, 128), (64, 256), (32, 512), (16, 512)):
            a = torch.relu(torch.randn(4, side, side, C, generator=g)).to(dev).to(ops.act_dtype())
            b = torch.relu(torch.randn(4, side, side, C, generator=g)).to(dev).to(ops.act_dtype())
            w, gi = torch.rand(C, generator=g).to(dev), torch.full((4,), 256.0, device=dev)
            fwd = timed(lambda: T.lpips_head(a, b, w), args.reps)
            bwd = timed(lambda: T.lpips_head_backward(a, b, w, gi), args.reps)
            nbytes = a.numel() * 2
            nws = lib.glare_lpips_head_workspace_bytes(4, side * side, C)
            ws, out, da = torch.empty(nws, dtype=torch.uint8, device=dev), torch.empty(4, device=dev), torch.empty_like(a)
            p = lambda t: t.data_ptr()
            cfwd = timed(lambda: lib.glare_lpips_head_bf16(p(a), p(b), p(w), 4, side * side, C, T.LPIPS_EPS, p(out), p(ws), nws, sh()), args.reps)
            cbwd = timed(lambda: lib.glare_lpips_head_backward_bf16(p(a), p(b), p(w), 4, side * side, C, T.LPIPS_EPS, p(gi), p(da), sh()), args.reps)
            assert torch.equal(out, T.lpips_head(a, b, w)) and torch.equal(da, T.lpips_head_backward(a, b, w, gi))
            lines.append("  %-22s %10.4f %10.0f %10.4f %10.0f | %10.4f %10.0f %10.4f %10.0f" % (
                "4 x %d x %d x %d" % (side, side, C), fwd, 2 * nbytes / fwd / 1e6, bwd, 3 * nbytes / bwd / 1e6,
                cfwd, 2 * nbytes / cfwd / 1e6, cbwd, 3 * nbytes / cbwd / 1e6))
    lines.append("(the project's other streaming passes on this box: GroupNorm apply 4.8-5.3 TB/s, VERDICT r06; the forward is its two launches together;")
    lines.append(" from the third tap down the launches move under 17 MB and are launch-bound)")
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--gan", action="store_true", help="time the step with and without the patch discriminator, and its launches alone")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--lpips", action="store_true", help="time the step with and without the LPIPS term (and --gan on top), and the head's kernels")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
    if args.gan or args.lpips:
        text = "\n".join((lpips if args.lpips else gan)(args)) + "\n"
        print(text, end="")
        if args.out:
            with open(args.out, "w") as f:
                f.write(text)
        return
    dev = torch.device("cuda", 0)
    lines = ["stage 1 on %s (tools/stage1_time.py; device events, warmed up, ms)" % torch.cuda.get_device_name(0)]
    tr = Stage1Trainer(seeded_init_(M.VQModel().train(), 1).to(dev), precision="fp16")
    tr.opt.scale.fill_(1024.0)
    x = torch.rand(4, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(dev)
    ms = timed(lambda: tr.step_tensor(x), args.steps, warm=3)
    lines.append("Stage1Trainer.step_tensor fp16, 4 x 3 x 256 x 256 (eager, %d steps): %.2f ms per step, %d steps applied of %d"
                 % (args.steps, ms, tr.opt.t, args.steps + 3))
    for N, reps in ((4 * 64 * 64, 200), (8 * 16275, 50)):
        t = launches(N, 8192, reps)
        lines.append("codebook layer, N = %d tokens, K = 8192 (%d launches each):" % (N, reps))
        lines += ["  %-22s %8.4f ms" % (k, v) for k, v in t.items()]
        lines.append("  new launches / vq_nearest: %.2f" % ((t["vq_loss_sum"] + t["vq_backward"]) / t["vq_nearest"]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
