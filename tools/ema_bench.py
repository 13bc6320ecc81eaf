"""Times what the EMA codebook costs (profiles/ema_step.txt).  python tools/ema_bench.py MODE [--size small|default] [--tree DIR]
  kernels     glare_vq_ema_stats_f32 and glare_vq_ema_update_f32 alone at K = 8192 codes and N = 512 (2 x 64^2) and N = 16384 (4 x 256^2)
              tokens, beside glare_vq_backward_f32's dE walk they stand in for; device events around 200 back-to-back calls, five repeats
  fit | fit-ema | fit-ema-restart
              `python -m glare_amd.fit stage1` for 50 steps on a synthetic folder -- plain, with --codebook-ema 0.99, with
              --codebook-ema 0.99 --codebook-restart 10: the driver's own ms per step of each 10-step window and after the first 20 steps
              --size small: 2 x 64^2 (--batch 2, GT_size 64); default: the driver's default batch, 4 x 256^2
--tree DIR: import glare_amd from DIR instead of this checkout (`fit` against another commit's build in the same session)."""
import json
import os
import sys
import tempfile

mode = sys.argv[1]
size = sys.argv[sys.argv.index("--size") + 1] if "--size" in sys.argv else "default"
tree = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
import numpy as np  # noqa: E402
import torch  # noqa: E402

dev = torch.device("cuda", 0)


def events_ms(fn, calls=200):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


if mode == "kernels":
    from glare_amd import _lib

    K = 8192
    lib = _lib.main_lib()
    s, p = _lib.stream_handle(), _lib.ptr
    res = {"mode": mode, "K": K, "sizes": []}
    for N in (512, 16384):
        g = torch.Generator().manual_seed(0)
        z, zq, gz = (torch.randn(N, 3, generator=g).to(dev) for _ in range(3))
        idx = torch.randint(0, K, (N,), generator=g).to(dev)
        stats = torch.empty(K, 4, device=dev)
        cs, ea, cb, de = torch.zeros(K, device=dev), torch.randn(K, 3, device=dev), torch.randn(K, 3, device=dev), torch.empty(K, 3, device=dev)
        gl = torch.ones(1, device=dev)
        nws = lib.glare_vq_ema_workspace_bytes(N, K)
        ws = torch.empty(nws, dtype=torch.uint8, device=dev)
        nwt = lib.glare_vq_train_workspace_bytes(N, K)
        wt = torch.empty(nwt, dtype=torch.uint8, device=dev)
        calls = {"ema_stats_us": lambda: lib.glare_vq_ema_stats_f32(p(idx), p(z), N, K, 3, p(stats), p(ws), nws, s),
                 "ema_update_us": lambda: lib.glare_vq_ema_update_f32(p(stats), K, 3, 0.99, 1e-5, p(cs), p(ea), p(cb), p(ws), nws, s),
                 "backward_dE_only_us": lambda: lib.glare_vq_backward_f32(p(z), p(zq), p(idx), p(gz), p(gl), N, K, 3, 1e-3, 1e-3, None, p(de),
                                                                          p(wt), nwt, s)}
        rec = {"N": N, "ema_workspace_bytes": nws}
        for name, call in calls.items():
            assert call() == 0, name
            for _ in range(20):
                call()
            torch.cuda.synchronize()
            rec[name] = [round(1e3 * events_ms(call), 2) for _ in range(5)]
        res["sizes"].append(rec)
else:
    from PIL import Image

    from glare_amd import fit

    rng = np.random.default_rng(4)
    with tempfile.TemporaryDirectory() as tmp:
        root, out = os.path.join(tmp, "data"), os.path.join(tmp, "run")
        for split, count in (("our485", 8), ("eval15", 1)):
            for sub in ("low", "high"):
                os.makedirs(os.path.join(root, split, sub))
                for i in range(count):
                    Image.fromarray(rng.integers(0, 256, size=(300, 320, 3), dtype=np.uint8)).save(os.path.join(root, split, sub, "%02d.png" % i))
        argv = ["stage1", "--root", root, "--out", out, "--niter", "50", "--save-freq", "1000", "--no-val"]
        if size == "small":
            opt = os.path.join(tmp, "opt.json")
            with open(opt, "w") as f:
                json.dump({"datasets": {"train": {"GT_size": 64}}}, f)
            argv += ["--opt", opt, "--batch", "2"]
        extra = {"fit": [], "fit-ema": ["--codebook-ema", "0.99"], "fit-ema-restart": ["--codebook-ema", "0.99", "--codebook-restart", "10"]}[mode]
        recs = fit.main(argv + extra)
    res = {"mode": mode, "size": size, "tree": tree, "ms_per_step_windows": [round(r["ms_per_step"], 3) for r in recs[:-1]],
           "ms_per_step_after_20": round(recs[-1]["ms_per_step_after_20"], 3), "loss": recs[-2]["loss"],
           "codebook_restarted": [r.get("codebook_restarted") for r in recs[:-1]]}
print(json.dumps(res), flush=True)
