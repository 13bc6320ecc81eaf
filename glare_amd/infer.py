"""Dataset-style inference driver: the GLARE counterpart of code/infer_dataset_lol.py:113-163 on the HIP
path, data-parallel over the GPUs of one node.

    python -m glare_amd.infer --images 32                      # 1 GPU, synthetic 400x600 pairs
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 -m glare_amd.infer --images 32

Per image, exactly the reference's harness steps (glare_amd/harness.py): reflect-pad, /255, log -> network ->
crop, clamp, GT-mean gain, PSNR.  Unlike the reference's one-image-per-iteration loop (one H2D + one D2H +
a full host sync per image), images are batched (default 8) and each rank enhances its own contiguous slice;
the only collective is the final gather of the per-image PSNRs to rank 0 (RCCL).
There are no datasets or checkpoints offline: inputs are synthetic LOL-shaped pairs, weights name-seeded."""
import argparse
import os
import time
import json

import numpy as np
import torch

from . import harness, parallel
from .synthetic import synthetic_gt, synthetic_lowlight


def enhance_batch(netG, net_vq, imgs_u8, device, precision=None):
    """uint8 [n,H,W,3] (host) -> network outputs [n,3,H+20,W+20] on the device (before the GT gain), via the fused NHWC
    graph.  The images cross PCIe once, as uint8; padding / log transform run on the device (csrc/harness.hip).
    precision: None = the entry point's default (fp16), or "bf16" / "fp16"."""
    # imgs_u8: a numpy array, or a (pinned) uint8 torch tensor -- then the copy is asynchronous on the current stream and the host
    # runs ahead instead of waiting for the stream to drain (a pageable H2D copy blocks until everything queued before it is done)
    src = imgs_u8 if isinstance(imgs_u8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(imgs_u8))
    lr = harness.preprocess_device(src.to(device, non_blocking=True))
    with torch.no_grad():
        out = netG.reverse_flow_nhwc(net_vq, lr, precision=precision)["out"]
    return out


def load_lol_pairs(root, layout="v1"):
    """uint8 (low, high) stacks of the test split of a LOL folder: layout "v1" = `<root>/eval15/{low,high}` (glare_amd.data.LoL_Dataset),
    "v2" = `<root>/{Synthetic,Real_captured}/Test/{low,high}` (LoL_Dataset_v2); all images one size."""
    from .data import LAYOUTS

    ds = LAYOUTS[layout]({"root": root}, train=False)
    lows = np.stack([p[0] for p in ds.pairs])
    gts = np.stack([p[1] for p in ds.pairs])
    return lows, gts


def run(n_images, batch=8, h=400, w=600, seed=1234, root=None, net_g=None, net_vq=None, pairs=None, with_ssim=False, precision=None,
        with_lpips=False, lpips_weights=None, nets=None, layout="v1"):
    """Synthetic LOL-shaped pairs by default; `root` = a LOL dataset folder (eval15 split), `net_g` / `net_vq` = checkpoint
    files in the reference's format (glare_amd.checkpoint) -- without them the weights are name-seeded; `pairs` = (lows, gts)
    uint8 stacks [n,h,w,3] supplied by the caller.  with_ssim / with_lpips: the loop's other two metrics (infer_dataset_lol.py:152-153)
    as further columns of the result; lpips_weights: a state dict saved from `lpips.LPIPS(net='alex')` (its AlexNet + linear heads cannot be
    downloaded here: without the file the LPIPS net is name-seeded and the column only exercises the path); nets = (netG, net_vq)
    module instances supplied by the caller (tests).
    The LAST column of the per-rank result is the overflow flag: the number of non-finite values of the network output inside the
    image's crop, counted on the device before the clamp; it is dropped from the returned array and reported as `run.nonfinite_values`."""
    from . import checkpoint

    rank, world, device = parallel.init_from_env()
    assert device.type == "cuda", "glare_amd.infer needs an MI355X: the HIP kernels are the only implementation"
    netG, net_vq_m = nets if nets is not None else checkpoint.build_nets("stage3")
    if net_g:
        checkpoint.load_network(net_g, netG, strict=False)       # VQLLFLOWD_model.py:53-63 loads with strict=False
    if net_vq:
        checkpoint.load_network(net_vq, net_vq_m, strict=False)
    netG, net_vq = netG.to(device), net_vq_m.to(device)
    lpips_net = None
    if with_lpips:
        from . import metrics

        lpips_net = metrics.build_lpips_alex(lpips_weights, device)
    ncols = 1 + int(with_ssim) + int(with_lpips)          # metric columns; one more (the overflow flag) rides along inside this function
    if pairs is not None:
        lows, gts = pairs
        n_images, h, w = lows.shape[0], lows.shape[1], lows.shape[2]
    elif root:
        lows, gts = load_lol_pairs(root, layout)
        n_images, h, w = lows.shape[0], lows.shape[1], lows.shape[2]
    else:
        lows = synthetic_lowlight(n_images, h, w, seed=seed)
        gts = synthetic_gt(n_images, h, w, seed=seed + 1)

    # the host images in PINNED memory (once, outside the timed region: the dataset loader's job), so that every batch's H2D copy is an
    # asynchronous DMA on its own stream; from pageable memory each copy stalled the host behind the previous batch (53 -> 5x images/s)
    base, top = parallel.shard_range(n_images, rank, world)        # only this rank's slice is pinned
    lows_p = torch.from_numpy(np.ascontiguousarray(lows[base:top])).pin_memory()
    gts_p = torch.from_numpy(np.ascontiguousarray(gts[base:top])).pin_memory()

    def psnr_slice(lo, hi, prec=precision):        # global image indices inside [base, top)
        out = enhance_batch(netG, net_vq, lows_p[lo - base:hi - base], device, prec)
        gt = gts_p[lo - base:hi - base].to(device, non_blocking=True)
        restored, vals, bad = harness.postprocess_device(out, h, w, gt, want_nonfinite=True)   # crop, clamp, GT-mean gain, PSNR + overflow flag
        cols = [vals]
        if with_ssim:                                                  # + SSIM (calculate_ssim, infer_dataset_lol.py:152)
            cols.append(harness.ssim_device(restored, gt))
        if with_lpips:                                                 # + LPIPS (measure.lpips on the two uint8 images, :153)
            from . import metrics

            a, b = metrics.to_lpips_input(harness.to_ubyte_device(restored)), metrics.to_lpips_input(gt)
            cols.append(lpips_net(a, b).view(-1).double())
        cols.append(bad.double())
        return torch.stack(cols, dim=1)

    if top > base:
        psnr_slice(base, min(base + batch, top))                  # warm-up on this rank's first batch: weight packing, workspace growth
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    local = parallel.run_sharded(n_images, psnr_slice, rank, world, batch=batch, streams=2)
    if local is None:
        local = torch.zeros(0, ncols + 1, dtype=torch.float64, device=device)
    # fp16 (the default) has fp16's range: a checkpoint whose activations pass 65504 yields inf / NaN where bf16 would not.  The
    # PSNRs come back to the host anyway; an image whose value is not finite is enhanced again in bf16 (fp32 range, same kernels)
    # bf16 misses the end-to-end tolerance 10x: a re-run image is a flagged exception, listed BY INDEX in the
    # output (`bf16_rerun_images`), not a silent substitution
    # Round 6: the trigger is the DEVICE-SIDE count of non-finite output values before the clamp, not only a non-finite PSNR -- the
    # clamp maps +inf to 1.0, so an overflowed image could come back with a finite figure
    run.bf16_reruns = 0
    run.bf16_rerun_images = []
    run.nonfinite_values = {}
    flagged = (~torch.isfinite(local[:, 0])) | (local[:, -1] > 0) if local.numel() else None
    if flagged is not None and bool(flagged.any()):
        lo0, _ = parallel.shard_range(n_images, rank, world)
        for j in flagged.nonzero().flatten().tolist():
            run.nonfinite_values[lo0 + j] = int(local[j, -1].item())
            if precision != "bf16":
                local[j] = psnr_slice(lo0 + j, lo0 + j + 1, "bf16")[0]
                run.bf16_reruns += 1
                run.bf16_rerun_images.append(lo0 + j)
    local = local[:, :ncols].contiguous()
    torch.cuda.synchronize()
    run.last_seconds = time.perf_counter() - t0                   # host uint8 in -> PSNR on the device, this rank's share
    full = parallel.gather_results(local, n_images, rank, world)
    if world > 1:      # which images were re-run, from every rank (a few integers)
        lists = [None] * world
        torch.distributed.all_gather_object(lists, (run.bf16_rerun_images, run.nonfinite_values))
        run.bf16_rerun_images = sorted(i for l, _ in lists for i in l)
        run.bf16_reruns = len(run.bf16_rerun_images)
        run.nonfinite_values = {k: v for _, d in lists for k, v in d.items()}
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()
    if full is None:
        return None
    return full.cpu().numpy() if ncols > 1 else full.view(-1).cpu().numpy()   # several metrics: columns (PSNR[, SSIM][, LPIPS])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=16)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=400)
    ap.add_argument("--width", type=int, default=600)
    ap.add_argument("--root", default=None, help="LOL dataset folder (uses <root>/eval15/{low,high}/*.png)")
    ap.add_argument("--layout", choices=("v1", "v2"), default="v1", help="v2: <root>/{Synthetic,Real_captured}/Test/{low,high}/*.png")
    ap.add_argument("--net-g", default=None, help="net_G checkpoint (reference format)")
    ap.add_argument("--net-vq", default=None, help="VQGAN checkpoint (reference format)")
    ap.add_argument("--ssim", action="store_true", help="also report SSIM (utils2.calculate_ssim) per image")
    ap.add_argument("--lpips", action="store_true", help="also report LPIPS-alex (Measure.lpips) per image")
    ap.add_argument("--lpips-weights", default=None, help="state dict of lpips.LPIPS(net='alex') (torch.save); without it the net is name-seeded")
    ap.add_argument("--precision", choices=("fp16", "bf16"), default=None,
                    help="16-bit format of activations and filters (default fp16, the reference's autocast dtype; images whose fp16 "
                         "result is not finite are re-run in bf16)")
    args = ap.parse_args()
    res = run(args.images, args.batch, args.height, args.width, root=args.root, net_g=args.net_g, net_vq=args.net_vq, with_ssim=args.ssim,
              precision=args.precision, with_lpips=args.lpips, lpips_weights=args.lpips_weights, layout=args.layout)
    if res is not None:
        world = int(os.environ.get("WORLD_SIZE", "1"))
        multi = args.ssim or args.lpips
        psnrs = res[:, 0] if multi else res
        extra = {"mean_ssim": float(np.mean(res[:, 1])), "ssim": [round(float(v), 5) for v in res[:, 1]]} if args.ssim else {}
        if args.lpips:
            col = res[:, 2 if args.ssim else 1]
            extra.update({"mean_lpips": float(np.mean(col)), "lpips": [round(float(v), 5) for v in col],
                          "lpips_weights": args.lpips_weights or "name-seeded (the package's weights are not available offline)"})
        print(json.dumps({"images": int(len(psnrs)), "mean_psnr": float(np.mean(psnrs)), "psnr": [round(float(v), 4) for v in psnrs], **extra,
                          "images_per_sec_incl_host_transfers": round(len(psnrs) / run.last_seconds, 2), "ranks": world,
                          "host_transfers_counted": "per batch: the asynchronous H2D copy of the uint8 inputs and GTs from PINNED host memory + the "
                                                    "D2H of the metrics; the one-off pageable -> pinned staging of this rank's images happens before "
                                                    "the clock starts (the dataset loader's job; rounds 1-4 timed a pageable .to(device) per batch)",
                          # images whose fp16 result was not finite and whose figure therefore comes from the bf16 precision (which
                          # misses the end-to-end tolerance): flagged per image, empty on every input this build has seen
                          "bf16_rerun_images": run.bf16_rerun_images,
                          # the overflow flag: per flagged image, how many values of the network output inside its crop were inf / NaN
                          # BEFORE the clamp (counted on the device, csrc/harness.hip) in the precision first tried
                          "nonfinite_output_values": {str(k): v for k, v in sorted(run.nonfinite_values.items())}}))


if __name__ == "__main__":
    main()
