"""What profiles/niqe.txt holds: the four NIQE kernels (csrc/niqe.hip) timed one by one at 400x600 and at about 4 MP, with the bytes
each must move over its time against the HBM rate, the whole metrics.niqe() call, and enhance.run with and without --niqe on one folder.

    python tools/probes/niqe_profile.py kernels [reps]        device events around `reps` back-to-back launches of each kernel
    python tools/probes/niqe_profile.py trace                 a few launches of each, for `rocprofv3 --kernel-trace --stats -- python ...`
    python tools/probes/niqe_profile.py enhance               enhance.run on a folder of 8 seeded 400x600 images, flag off / on, alternating

The pristine model is the synthetic one of the tests (tests/niqe_fp64.py): the times do not depend on its values."""
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import niqe_fp64 as N  # noqa: E402
from glare_amd import enhance, metrics  # noqa: E402
from glare_amd.synthetic import synthetic_pair  # noqa: E402

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12          # B/s: the specification, and what a float4 copy reaches on this chip
SIZES = ((1, 400, 600), (8, 400, 600), (1, 1536, 2688))
WINDOW = N.synthetic_params()["gaussian_window"]


def _stages(img):
    """[(kernel, launch, bytes it must read + write)] on one uint8 batch; the launches reuse their inputs."""
    B, h, w, _ = img.shape
    y = metrics.niqe_luma(img)
    H, W = y.shape[1:]
    n, y2 = metrics.niqe_mscn(y, WINDOW), metrics.niqe_halve(y)
    n2 = metrics.niqe_mscn(y2, WINDOW)
    px, nb = B * H * W, B * (H // 96) * (W // 96)
    return [("niqe_luma_kernel", lambda: metrics.niqe_luma(img), 3 * px + 4 * px),        # the cropped pixels, uint8 in, fp32 out
            ("niqe_mscn_kernel (scale 1)", lambda: metrics.niqe_mscn(y, WINDOW), 8 * px),
            ("niqe_moments_kernel (96x96)", lambda: metrics.niqe_block_moments(n), 4 * px + 200 * nb),
            ("niqe_halve_kernel", lambda: metrics.niqe_halve(y), 4 * px + px),
            ("niqe_mscn_kernel (scale 2)", lambda: metrics.niqe_mscn(y2, WINDOW), 2 * px),
            ("niqe_moments_kernel (48x48)", lambda: metrics.niqe_block_moments(n2, 48, 48), px + 200 * nb)]


def kernels(reps):
    for B, h, w in SIZES:
        img = torch.from_numpy(np.ascontiguousarray(np.concatenate([synthetic_pair(1, h, w, seed=500 + b)[1] for b in range(B)]))).cuda()
        print("\n%d x %dx%d (cropped to %dx%d, %.2f MP, %d blocks per image)" % (B, h, w, h // 96 * 96, w // 96 * 96, B * (h // 96 * 96) * (w // 96 * 96) / 1e6,
                                                                               (h // 96) * (w // 96)))
        total = 0.0
        for name, launch, nbytes in _stages(img):
            for _ in range(5):
                launch()
            torch.cuda.synchronize()
            best = float("inf")
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    launch()
                e1.record()
                torch.cuda.synchronize()
                best = min(best, e0.elapsed_time(e1) * 1e3 / reps)
            total += best
            rate = nbytes / (best * 1e-6)
            print("  %-30s %8.2f us per launch (incl. its output allocation and launch gap)  %7.2f MB  %6.1f GB/s = %4.1f %% of %.2f TB/s (copy rate), %4.1f %% of spec"
                  % (name, best, nbytes / 1e6, rate / 1e9, 100 * rate / HBM_COPY, HBM_COPY / 1e12, 100 * rate / HBM_SPEC))
        params = metrics._niqe_params(N.synthetic_params(), "synthetic")
        metrics.niqe(img, params)
        t = []
        for _ in range(5):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            metrics.niqe(img, params)
            t.append(time.perf_counter() - t0)
        print("  sum of the six launches %.1f us; metrics.niqe() on the device tensor, host clock, 5 calls: %s ms (launches, the copy of the moments, "
              "the fp64 host part)" % (total, " ".join("%.2f" % (x * 1e3) for x in t)))


def trace():
    for B, h, w in SIZES:
        img = torch.from_numpy(np.ascontiguousarray(np.concatenate([synthetic_pair(1, h, w, seed=500 + b)[1] for b in range(B)]))).cuda()
        for _, launch, _ in _stages(img):
            for _ in range(20):
                launch()
        torch.cuda.synchronize()


def enhance_ab():
    from PIL import Image

    device = torch.device("cuda", torch.cuda.current_device())
    netG, net_vq = enhance.load_nets(device=device)
    params = metrics._niqe_params(N.synthetic_params(), "synthetic")
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "photos")
        os.makedirs(src)
        for i in range(8):
            Image.fromarray(synthetic_pair(1, 400, 600, seed=600 + i)[0][0]).save(os.path.join(src, "img%d.png" % i))
        for rep in range(3):
            for flag in (None, params):
                r = enhance.run([src], os.path.join(tmp, "out"), netG, net_vq, device=device, niqe=flag)
                print(json.dumps({"niqe": flag is not None, "rep": rep, "seconds": r["seconds"], "images_per_sec": r["images_per_sec"],
                                  "niqe_seconds": r.get("niqe_seconds"), "niqe_mean": r.get("niqe_mean"), "niqe_in_mean": r.get("niqe_in_mean")}))


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs an MI355X"
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    if mode == "kernels":
        kernels(int(sys.argv[2]) if len(sys.argv) > 2 else 200)
    elif mode == "trace":
        trace()
    else:
        enhance_ab()
