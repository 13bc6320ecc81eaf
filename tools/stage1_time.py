"""Time stage 1 on the GPU: one fp16 Stage1Trainer step at the reference crop (4 x 3 x 256 x 256), and the codebook layer's new launches
(csrc/vq_train.hip) alone against the same step's glare_vq_nearest_f32 launch, on the step's own token count (4 x 64 x 64) and on
the largest the layer is specified for (8 x 16 275).  Device events around repeated launches on preallocated buffers; every shape is
warmed up first.  `python tools/stage1_time.py [--out profiles/stage1_step.txt]`"""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=30)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs an MI355X"
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
