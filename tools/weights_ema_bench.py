"""Times what the weight average costs (profiles/weights_ema.txt).  python tools/weights_ema_bench.py MODE [--rounds R] [--tree DIR]
  kernels   glare_weight_ema_f32 (seeded: the averaging form) and glare_swap_f32 alone over buffers of the two trained sizes -- stage 3's
            deformable decoder and stage 1's VQModel -- and over the first one 4 bytes off the vector phase; device events around 100
            back-to-back calls, five repeats; bytes moved over the time
  stage3    `python -m glare_amd.fit stage3 --graph` (2 x 256^2, name-seeded nets) for 120 steps on a synthetic folder, R rounds in this
            process, each round the run without the option and then with --weights-ema 0.999: the driver's own ms per step of every
            20-step window and after the first 20 steps, and the last loss
  stage1    the same for `python -m glare_amd.fit stage1 --gan --disc-start 0` (4 x 256^2), 60 steps, 10-step windows
--tree DIR: import glare_amd from DIR instead of this checkout (a build of the parent commit in the same session); a tree without the
option runs the plain form only."""
import json
import os
import sys
import tempfile

mode = sys.argv[1]
rounds = int(sys.argv[sys.argv.index("--rounds") + 1]) if "--rounds" in sys.argv else 3
tree = sys.argv[sys.argv.index("--tree") + 1] if "--tree" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
import numpy as np  # noqa: E402
import torch  # noqa: E402

dev = torch.device("cuda", 0)


def events_ms(fn, calls=100):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


if mode == "kernels":
    from glare_amd import _lib
    from glare_amd import modules as M

    lib = _lib.main_lib()
    s = _lib.stream_handle()
    sizes = {"stage3 deformable_decoder": sum(p.numel() for n, p in M.VQLLFLOWDeformable().named_parameters() if n.startswith("deformable_decoder.")),
             "stage1 VQModel": sum(p.numel() for p in M.VQModel().parameters())}
    res = {"mode": mode, "threads": 256, "max_workgroups": 2048, "sizes": []}
    flag = torch.ones(1, dtype=torch.int32, device=dev)
    for name, n in sizes.items():
        for off in ((0, 1) if name.startswith("stage3") else (0,)):
            e, w = torch.randn(n + 4, device=dev), torch.randn(n + 4, device=dev)
            pe, pw = e.data_ptr(), w.data_ptr() + 4 * off
            calls = {"weight_ema_us": (lambda: lib.glare_weight_ema_f32(pe, pw, n, 0.999, 1.0 - float(np.float32(0.999)), flag.data_ptr(), s), 12),
                     "swap_us": (lambda: lib.glare_swap_f32(pe, pw, n, s), 16)}
            rec = {"buffer": name, "n": n, "w_offset_elements": off, "workgroups": min(2048, -(-(n // 4) // 256))}
            for key, (call, bytes_per) in calls.items():
                assert call() == 0, key
                for _ in range(10):
                    call()
                torch.cuda.synchronize()
                rec[key] = [round(1e3 * events_ms(call), 2) for _ in range(5)]
                rec[key.replace("_us", "_TBps")] = round(bytes_per * n / (min(rec[key]) * 1e-6) / 1e12, 3)
            res["sizes"].append(rec)
else:
    from PIL import Image

    from glare_amd import fit

    has_option = hasattr(fit, "check_weights_ema_option")
    niter, window = (120, 20) if mode == "stage3" else (60, 10)
    rng = np.random.default_rng(4)
    res = {"mode": mode, "tree": tree, "runs": []}
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "data")
        for split, count in (("our485", 8), ("eval15", 1)):
            for sub in ("low", "high"):
                os.makedirs(os.path.join(root, split, sub))
                for i in range(count):
                    Image.fromarray(rng.integers(0, 256, size=(300, 320, 3), dtype=np.uint8)).save(os.path.join(root, split, sub, "%02d.png" % i))
        opt = os.path.join(tmp, "opt.json")
        with open(opt, "w") as f:
            json.dump({"logger": {"print_freq": window}}, f)
        for r in range(rounds):
            for ema in ((False, True) if has_option else (False,)):
                out = os.path.join(tmp, "run_%d_%d" % (r, ema))
                argv = [mode, "--root", root, "--out", out, "--opt", opt, "--niter", str(niter), "--save-freq", "100000", "--no-val"]
                argv += ["--graph"] if mode == "stage3" else ["--gan", "--disc-start", "0"]
                recs = fit.main(argv + (["--weights-ema", "0.999"] if ema else []))
                res["runs"].append({"round": r, "weights_ema": 0.999 if ema else None,
                                    "ms_per_step_windows": [round(x["ms_per_step"], 3) for x in recs[:-1]],
                                    "ms_per_step_after_20": round(recs[-1]["ms_per_step_after_20"], 3), "loss": recs[-2]["loss"]})
print(json.dumps(res), flush=True)
