"""Times what the codebook restart adds (profiles/vq_restart.txt).  python tools/restart_bench.py MODE [--tree DIR]
  kernels     glare_vq_restart_f32 (four launches) at the stage-1 step's size, N = 8192 tokens (2 x 256^2) and K = 8192 codes, about 98 % of
              the window dead as in a fresh run; device events around 200 back-to-back calls, five repeats (the window is zero after
              the first call: every later call finds every code dead, the most rows the call can write)
  fit | fit-restart
              `python -m glare_amd.fit stage1` at 2 x 256^2 for 50 steps on a synthetic folder, without the option / with
              --codebook-restart 10: the driver's own ms per step of each 10-step window and after the first 20 steps
--tree DIR: import glare_amd from DIR instead of this checkout (`fit` against another commit's build in the same session)."""
import json
import os
import sys
import tempfile

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

    N, K = 8192, 8192
    lib = _lib.main_lib()
    g = torch.Generator().manual_seed(0)
    z = torch.randn(N, 3, generator=g).to(dev)
    cb, m, v = (torch.randn(K, 3, generator=g).to(dev) for _ in range(3))
    window = (torch.rand(K, generator=g) < 0.02).long().to(dev)
    out = torch.empty(2, dtype=torch.int64, device=dev)
    nws = lib.glare_vq_restart_workspace_bytes(K)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    s, p = _lib.stream_handle(), _lib.ptr
    call = lambda: lib.glare_vq_restart_f32(p(window), 0, p(z), N, K, 3, 7919, p(cb), p(m), p(v), out.data_ptr(), out.data_ptr() + 8, p(ws), nws, s)
    assert call() == 0
    first = out.tolist()
    for _ in range(20):
        call()
    torch.cuda.synchronize()
    res = {"mode": mode, "N": N, "K": K, "workspace_bytes": nws, "first_call_dead_restarted": first, "later_calls_dead_restarted": out.tolist(),
           "restart_f32_us": [round(1e3 * events_ms(call), 2) for _ in range(5)]}
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
        argv = ["stage1", "--root", root, "--out", out, "--batch", "2", "--niter", "50", "--save-freq", "1000", "--no-val"]
        recs = fit.main(argv + (["--codebook-restart", "10"] if mode == "fit-restart" else []))
    res = {"mode": mode, "tree": tree, "ms_per_step_windows": [round(r["ms_per_step"], 3) for r in recs[:-1]],
           "ms_per_step_after_20": round(recs[-1]["ms_per_step_after_20"], 3), "loss": recs[-2]["loss"],
           "codebook_restarted": [r.get("codebook_restarted") for r in recs[:-1]]}
print(json.dumps(res), flush=True)
