"""Time stage 1's semantic guidance term on the GPU (profiles/vq_semantic.txt).  Device events, every shape warmed up first.

  kernels   python tools/semantic_bench.py kernels
            glare_vq_semantic_bf16 / _f16 alone at N = 4 x 64 x 64 tokens (loss and the three unit gradients, two launches), its feature
            bytes per second against the HBM roof, and the scale launch; then the same quantity through the ops the tree had before
            the kernel existed, unfused: autograd.conv2d_small 3 -> 256 with ReLU into autograd.mse_loss, forward plus backward.
  step      python tools/semantic_bench.py step [--semantic] [--tree DIR]
            one fp16 Stage1Trainer step at 2 x 3 x 256 x 256 without or with the term (seeded VGG19 weights), ms per step; --tree DIR
            imports glare_amd from another checkout (the parent commit, built), so that one session can alternate the three.
Each mode prints JSON lines."""
import argparse
import json
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=("kernels", "step"))
ap.add_argument("--semantic", action="store_true")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--steps", type=int, default=40)
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.tree))

from glare_amd import _lib, ops  # noqa: E402
from glare_amd import autograd as A  # noqa: E402
from glare_amd import modules as M  # noqa: E402
from glare_amd.synthetic import seeded_init_  # noqa: E402
from glare_amd.train import Stage1Trainer  # noqa: E402

HBM_TBS = 6.29          # measured float4-copy bandwidth of one MI355X (spec 8.0)
DEV = torch.device("cuda", 0)


def timed(fn, reps, warm=10):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / reps          # us


def seeded_vgg19(seed=4):
    g = torch.Generator().manual_seed(seed)
    sd, cin = {}, 3
    for idx, cout in ((0, 64), (2, 64), (5, 128), (7, 128), (10, 256), (12, 256), (14, 256), (16, 256)):
        sd["features.%d.weight" % idx] = torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (cin * 9)) ** 0.5
        sd["features.%d.bias" % idx] = torch.randn(cout, generator=g) * 0.05
        cin = cout
    return sd


def kernels():
    B, h, w, C = 4, 64, 64, 256
    N = B * h * w
    g = torch.Generator().manual_seed(0)
    q, W, b = torch.randn(N, 3, generator=g).to(DEV), (torch.randn(C, 3, generator=g) * 0.5).to(DEV), (torch.randn(C, generator=g) * 0.1).to(DEV)
    for prec in ("fp16", "bf16"):
        with ops.use_precision(prec):
            feat = torch.randn(N, C, generator=g).abs().to(DEV).to(ops.act_dtype())
            lib = _lib.lib()
            nws = lib.glare_vq_semantic_workspace_bytes(N, C)
            ws = torch.empty(nws, dtype=torch.uint8, device=DEV)
            loss, dq, dW, db = torch.empty(1, device=DEV), torch.empty_like(q), torch.empty_like(W), torch.empty_like(b)
            p, sh = _lib.ptr, _lib.stream_handle
            fused = lambda: _lib.check(lib.glare_vq_semantic_bf16(p(q), p(W), p(b), p(feat), N, C, p(loss), p(dq), p(dW), p(db), p(ws), nws, sh()), "fused")
            gq, gW, gb, gs = torch.empty_like(dq), torch.empty_like(dW), torch.empty_like(db), torch.full((1,), 256.0, device=DEV)
            scale = lambda: _lib.check(lib.glare_vq_semantic_scale_f32(p(gs), N, p(dq), p(dW), p(db), p(gq), p(gW), p(gb), sh()), "scale")
            t_fused, t_scale = timed(fused, args.reps), timed(scale, args.reps)
            # one workgroup's worth of tokens: what the two launches cost when there is next to nothing to read
            small = lambda: _lib.check(lib.glare_vq_semantic_bf16(p(q), p(W), p(b), p(feat), 64, C, p(loss), p(dq), p(dW), p(db), p(ws), nws, sh()), "fused")
            t_small = timed(small, args.reps)
            node_q, node_W, node_b = q.view(B, h, w, 3).clone().requires_grad_(True), W.view(C, 3, 1, 1).clone().requires_grad_(True), b.clone().requires_grad_(True)
            featn = feat.view(B, h, w, C)

            def node():
                for t in (node_q, node_W, node_b):
                    t.grad = None
                (A.vq_semantic(node_q, node_W, node_b, featn) * 256.0).backward()

            def unfused():
                for t in (node_q, node_W, node_b):
                    t.grad = None
                s = A.conv2d_small(node_q, node_W, node_b, layout="nhwc", act="relu")
                (A.mse_loss(s, featn) * 256.0).backward()

            rec = {"precision": prec, "tokens": N, "fused_call_us": round(t_fused, 2), "scale_call_us": round(t_scale, 2), "fused_call_us_at_64_tokens": round(t_small, 2),
                   "feat_bytes": feat.numel() * 2, "feat_TB_per_s": round(feat.numel() * 2 / (t_fused * 1e-6) / 1e12, 3),
                   "share_of_hbm_roof_%.2f_TB_per_s" % HBM_TBS: round(feat.numel() * 2 / (t_fused * 1e-6) / 1e12 / HBM_TBS, 3),
                   "autograd_node_fwd_bwd_us": round(timed(node, args.reps), 2)}
            try:
                unfused()
                torch.cuda.synchronize()
                rec["unfused_fwd_bwd_us"] = round(timed(unfused, args.reps), 2)
                node()
                ref = [t.grad.clone() for t in (node_q, node_W, node_b)]
                unfused()
                rel = lambda a, r: float((a.double() - r.double()).norm() / r.double().norm())
                rec["unfused_vs_fused_gradient_rel_l2"] = [round(rel(t.grad, r), 5) for t, r in zip((node_q, node_W, node_b), ref)]
            except Exception as e:      # the existing ops cannot express it: say so
                rec["unfused_fwd_bwd_us"] = None
                rec["unfused_cannot"] = "%s: %s" % (type(e).__name__, str(e)[:300])
            print(json.dumps(rec), flush=True)


def step():
    x = torch.rand(2, 3, 256, 256, generator=torch.Generator().manual_seed(0)).to(DEV)
    kw = {}
    if args.semantic:
        from glare_amd import losses

        net = losses.SemanticTarget()
        losses.load_vgg19(net, seeded_vgg19())
        kw = {"semantic": net.to(DEV), "semantic_weight": 0.1}
    tr = Stage1Trainer(seeded_init_(M.VQModel().train(), 1).to(DEV), precision="fp16", **kw)
    tr.opt.scale.fill_(1024.0)
    ms = timed(lambda: tr.step_tensor(x), args.steps, warm=8) / 1e3
    print(json.dumps({"tree": os.path.abspath(args.tree), "semantic": bool(args.semantic), "batch": "2x3x256x256", "steps": args.steps,
                      "ms_per_step": round(ms, 3), "loss": float(tr.step_tensor(x))}), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs an MI355X"
    kernels() if args.mode == "kernels" else step()
