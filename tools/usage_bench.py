"""Times what codebook usage adds (profiles/vq_usage.txt).  python tools/usage_bench.py MODE [--tree DIR]
  kernels     the two entry points of csrc/vq_usage.hip at the test split's size: G = 8 latents of n = 15 000 tokens (a 400 x 600 image is
              100 x 150 tokens), K = 8192; device events around 200 back-to-back calls, five repeats
  evaluate    glare_amd.evaluate.score_checkpoint("stage1") over 15 images of 400 x 600 (eval15's shape), name-seeded weights: images / s
  step-off | step-on | step-plain
              one stage-1 training step at the driver's default shape (4 x 3 x 256 x 256, fp16): Stage1Trainer(codebook_usage=False / True),
              or built without the keyword (what another checkout given by --tree understands); ms / step over 30 steps after 8
--tree DIR: import glare_amd from DIR instead of this checkout (an A/B against another commit's build in the same call)."""
import json
import os
import sys
import time

mode = sys.argv[1]
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

    G, n, K = 8, 15000, 8192
    lib = _lib.main_lib()
    g = torch.Generator().manual_seed(0)
    # a used-codebook shape: most tokens on a few hundred codes, the rest spread
    idx = torch.where(torch.rand(G, n, generator=g) < 0.7, torch.randint(0, 300, (G, n), generator=g), torch.randint(0, K, (G, n), generator=g)).to(dev)
    counts = torch.empty(G, K, dtype=torch.int64, device=dev)
    oor = torch.empty(G, dtype=torch.int64, device=dev)
    total = torch.zeros(K, dtype=torch.int64, device=dev)
    nws = lib.glare_vq_usage_workspace_bytes(G, n, K)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    out = [torch.empty(G, dtype=torch.int64, device=dev) for _ in range(2)] + [torch.empty(G, dtype=torch.float64, device=dev) for _ in range(2)]
    s = _lib.stream_handle()
    p = _lib.ptr
    use = lambda: lib.glare_vq_usage_i64(p(idx), G, n, K, p(counts), p(oor), p(total), p(ws), nws, s)
    stats = lambda: lib.glare_vq_usage_stats(p(counts), G, K, p(out[0]), p(out[1]), p(out[2]), p(out[3]), s)
    assert use() == 0 and stats() == 0
    for _ in range(20):
        use(), stats()
    torch.cuda.synchronize()
    res = {"mode": mode, "G": G, "n": n, "K": K, "workspace_bytes": nws,
           "usage_i64_us": [round(1e3 * events_ms(use), 2) for _ in range(5)], "usage_stats_us": [round(1e3 * events_ms(stats), 2) for _ in range(5)],
           "active": out[1].tolist(), "perplexity": [round(v, 3) for v in out[3].tolist()]}
elif mode == "evaluate":
    from glare_amd import checkpoint, evaluate
    from glare_amd.synthetic import synthetic_gt

    net, _ = checkpoint.build_nets("stage1", device=dev)
    gts = synthetic_gt(15, 400, 600)
    rates = []
    for _ in range(3):                                   # the first pass packs the filters and loads the code objects
        report = {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = evaluate.score_checkpoint("stage1", net, None, gts, gts, batch=8, report=report)
        torch.cuda.synchronize()
        rates.append(round(len(rows) / (time.perf_counter() - t0), 2))
    res = {"mode": mode, "images": 15, "size": [400, 600], "batch": 8, "images_per_s": rates, "codebook": report["codebook"],
           "mean_psnr": float(np.mean([r["PSNR"] for r in rows]))}
else:
    from glare_amd import modules as M
    from glare_amd.synthetic import seeded_init_
    from glare_amd.train import Stage1Trainer

    kw = {"step-off": {"codebook_usage": False}, "step-on": {"codebook_usage": True}, "step-plain": {}}[mode]
    tr = Stage1Trainer(seeded_init_(M.VQModel().train(), 6).to(dev), precision="fp16", **kw)
    x = torch.rand(4, 3, 256, 256, generator=torch.Generator().manual_seed(10)).to(dev)
    for _ in range(8):
        loss = tr.step_tensor(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(30):
        loss = tr.step_tensor(x)
    torch.cuda.synchronize()
    res = {"mode": mode, "tree": tree, "ms_per_step": round(1e3 * (time.perf_counter() - t0) / 30, 3), "loss": float(loss),
           "terms": sorted(tr.last_terms)}
print(json.dumps(res), flush=True)
