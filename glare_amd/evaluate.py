"""Score every checkpoint of a training run on the test split: the GLARE counterpart of code/test_stage2.py and
code/test_stage3.py on the HIP path -- the step between `glare_amd.fit stage2` and `stage3` that names the checkpoint to go on with
(confs/train_stage3_LOL.yml:109, "best checkpoint in stage2"), and the same after stage 3.

    python -m glare_amd.evaluate stage2|stage3 --run RUN --root LOLdataset [--layout v1|v2] [--net-vq F] [--out DIR]
                                 [--lpips --lpips-weights F] [--select COL] [--precision fp16|bf16] [--save-images]

The networks are built once; every `RUN/models/*_G.pth`, in natural order, is loaded into the same module instances
(test_stage2.py:110-116), scored, written to `<out>/<name>.csv` (one row per image) and appended to `<out>/results-<stage>.txt`
(`<name> <means>`); a checkpoint whose CSV exists is not scored again (:126-127).  The last line printed is one JSON object.

Per image (score_checkpoint), with the test images crossing PCIe once as uint8 and pad / log / crop / gain / uint8 / squared error
on the device (csrc/harness.hip):
  stage 3 (test_stage3.py:157-205): reflect pad 20 px bottom / left, log, the network, crop; `PSNR` and `SSIM` on the clamped,
    GT-mean-scaled float image (:189-202, what glare_amd.infer reports), `1_PSNR` on the uint8 image rgb(clamp(out * mean_gt /
    mean_out)) with mean_out over the RAW output (:183-185, :203); `LPIPS` (:205) on request.
  stage 2 (test_stage2.py:133-180): reflect pad bottom / right to even sides, log, LLFlowVQGAN2.enhance_nhwc (conditional encoder,
    reverse flow, codebook, the VQGAN decoder's RGB head); `PSNR` on rgb(out) (:179), `Adjust_PSNR` on rgb(clamp(out * mean_gt /
    mean_out)) (:169-177); `LPIPS` / `Adjust_LPIPS` on request.  The reference pads to even sides only and then compares the
    PADDED output with the ground truth, which works where nothing was padded and the sides are multiples of 4 (the decoder's x4);
    here the window of the image is scored and a padded side that is no multiple of 4 raises ValueError before any launch.
PSNR of two uint8 images is skimage's peak_signal_noise_ratio (Measure.psnr): 10 log10(255^2 / mse), inf for equal images.
NOT built: the `SSIM` / `Adjust_SSIM` / `1_SSIM` columns of Measure.ssim (code/Measure.py:32-41).  It calls
skimage.structural_similarity(..., multichannel=True) on 2-D arrays, an argument current scikit-image no longer has, and
scikit-image is not available to pin what it computed; stage 3's `SSIM` column is calculate_ssim (test_stage3.py:202), which is.
Rows are written in dataset order (the reference prepends each new row).  Without checkpoints the weights are name-seeded."""
import argparse
import csv
import glob
import json
import math
import os
import time

import numpy as np

from . import harness
from .enhance import check_size, natural_key, write_image

# per-image metric columns in the reference's names and order (test_stage2.py:175-180, test_stage3.py:197-205), without Measure.ssim's
COLUMNS = {"stage2": ("Adjust_PSNR", "Adjust_LPIPS", "PSNR", "LPIPS"), "stage3": ("PSNR", "SSIM", "1_PSNR", "LPIPS")}
LEAD = {"stage2": ("conf", "heat", "name"), "stage3": ("conf", "name")}
LOWER_IS_BETTER = ("LPIPS", "Adjust_LPIPS")
WARM_SIDE = 32          # the side of the one-image pass that rebuilds every packed filter after a checkpoint swap


def columns(stage, with_lpips=False):
    return tuple(c for c in COLUMNS[stage] if with_lpips or "LPIPS" not in c)


def stage2_pads(h, w):
    """(top, bottom, left, right) of test_stage2.py:142-145 (pad_factor 2, bottom / right); ValueError for a padded side the stage-2
    graph cannot take: its decoder returns 4 * (side // 4) pixels, an image smaller than the ground truth."""
    pads = (0, -h % 2, 0, -w % 2)
    hp, wp = h + pads[1], w + pads[3]
    if hp % 4 or wp % 4 or hp < 4 or wp < 4:
        raise ValueError("stage 2: the image size %dx%d pads to %dx%d, not a multiple of 4 on both sides: the VQGAN decoder would "
                         "return %dx%d" % (h, w, hp, wp, hp // 4 * 4, wp // 4 * 4))
    return pads


def _device_rows(stage, netG, net_hq, low_d, gt_d, precision, lpips_net, want_images):
    """One batch on the device -> ({column: host float64 [n]}, non-finite counts [n], {image kind: uint8 device tensor})."""
    import torch

    n, h, w, _ = low_d.shape
    images = {}
    with torch.no_grad():
        if stage == "stage3":
            out = netG.reverse_flow_nhwc(net_hq, harness.preprocess_device(low_d), precision=precision)["out"].float().contiguous()
            window = (0, harness.PAD, h, w)
            restored, psnr, bad = harness.postprocess_device(out, h, w, gt_d, want_nonfinite=True)      # GT-mean protocol (:189-201)
            cols = {"PSNR": psnr, "SSIM": harness.ssim_device(restored, gt_d)}
            adj, sse = harness.score_device(out, gt_d, harness.adjust_gain_device(out, gt_d, window), window)     # :183-185, :203
            cols["1_PSNR"] = sse
            if lpips_net is not None or want_images:
                saved = harness.to_ubyte_device(restored)                # img_as_ubyte(restored): what :205 measures and :209 saves
                images = {"": saved, "adjust": adj}
        else:
            pads = stage2_pads(h, w)
            lr = harness.preprocess_unpaired_device(low_d, pads, harness.PAD_REFLECT101)
            out = netG.enhance_nhwc(net_hq, lr, precision=precision)["out"].float().contiguous()
            window = (0, 0, h, w)
            _, bad = harness.postprocess_unpaired_device(out, pads, h, w, want_nonfinite=True)          # the overflow flag only
            raw, sse_raw = harness.score_device(out, gt_d, None, window)                                   # rgb(lr_out), :179
            adj, sse_adj = harness.score_device(out, gt_d, harness.adjust_gain_device(out, gt_d, window), window)  # :169-177
            cols = {"Adjust_PSNR": sse_adj, "PSNR": sse_raw}
            images = {"no-adjust": raw, "adjust": adj}
        if lpips_net is not None:
            from . import metrics

            ref = metrics.to_lpips_input(gt_d)
            for col, kind in (("LPIPS", "" if stage == "stage3" else "no-adjust"),) + ((("Adjust_LPIPS", "adjust"),) if stage == "stage2" else ()):
                cols[col] = lpips_net(metrics.to_lpips_input(images[kind]), ref).view(-1).double()
    host = {}
    for c, v in cols.items():
        v = v.cpu().numpy()
        host[c] = np.array([harness.psnr_u8(s, 3 * h * w) for s in v]) if v.dtype == np.int64 else v.astype(np.float64)
    return host, bad.cpu().numpy(), (images if want_images else {})


def score_checkpoint(stage, netG, net_hq, lows, gts, batch=8, precision=None, lpips_net=None, device=None, report=None, keep_images=False):
    """Per-image rows ({column: float}, dataset order) of one set of weights on uint8 pairs `lows`, `gts` [n,h,w,3] (one size).
    An image whose fp16 output holds inf / NaN before the clamp is scored again in bf16 and listed in report["bf16_rerun_images"]
    (as glare_amd.infer does).  keep_images: report["images"] = {kind: uint8 [n,h,w,3]} of what --save-images writes (stage 2:
    "no-adjust" and "adjust"; stage 3: "" = img_as_ubyte(restored), and "adjust").  Raises ValueError before any launch for a size
    outside the envelope of the kernels (glare_amd.enhance.check_size) or, in stage 2, of the graph (stage2_pads)."""
    import torch

    from . import ops

    assert stage in COLUMNS, stage
    lows, gts = np.ascontiguousarray(lows), np.ascontiguousarray(gts)
    assert lows.dtype == np.uint8 and gts.dtype == np.uint8 and lows.ndim == 4 and lows.shape == gts.shape and lows.shape[3] == 3
    n, h, w, _ = lows.shape
    batch = max(1, min(batch, n))
    if stage == "stage2":
        pads = stage2_pads(h, w)
        check_size(h + pads[1], w + pads[3], batch)
    else:
        check_size(h + harness.PAD, w + harness.PAD, batch)
    assert torch.cuda.is_available(), "glare_amd.evaluate needs an MI355X: the HIP kernels are the only implementation"
    device = device or torch.device("cuda", torch.cuda.current_device())
    precision = ops.inference_precision(precision)
    lows_p, gts_p = torch.from_numpy(lows).pin_memory(), torch.from_numpy(gts).pin_memory()

    def run(lo, hi, prec):
        return _device_rows(stage, netG, net_hq, lows_p[lo:hi].to(device, non_blocking=True), gts_p[lo:hi].to(device, non_blocking=True),
                            prec, lpips_net, keep_images)

    rows, reruns, kept = [None] * n, [], {}
    for lo in range(0, n, batch):
        hi = min(lo + batch, n)
        cols, bad, images = run(lo, hi, precision)
        images = {k: v.cpu().numpy() for k, v in images.items()}
        for j in range(hi - lo):
            flagged = int(bad[j]) > 0 or not all(math.isfinite(cols[c][j]) or cols[c][j] == math.inf for c in cols)
            if flagged and precision != "bf16":       # fp16 overflow: bf16 has fp32's range, same kernels; a flagged exception
                c1, _, im1 = run(lo + j, lo + j + 1, "bf16")
                for c in cols:
                    cols[c][j] = c1[c][0]
                for k in images:
                    images[k][j] = im1[k][0].cpu().numpy()
                reruns.append(lo + j)
            rows[lo + j] = {c: float(cols[c][j]) for c in columns(stage, lpips_net is not None)}
        for k, v in images.items():
            kept.setdefault(k, []).append(v)
    if report is not None:
        report["bf16_rerun_images"] = reruns
        if keep_images:
            report["images"] = {k: np.concatenate(v) for k, v in kept.items()}
    return rows


# ---- the sweep ----------------------------------------------------------------------------------------------------------------
def list_checkpoints(run_or_files):
    """A run folder -> its models/*_G.pth in natural order (natsorted(os.listdir(.../models)), test_stage2.py:110); a list of
    files -> the same order."""
    if isinstance(run_or_files, (str, os.PathLike)):
        files = glob.glob(os.path.join(run_or_files, "models", "*_G.pth"))
    else:
        files = list(run_or_files)
    return sorted(files, key=natural_key)


def format_measurements(meas):
    """format_measurements of the test scripts (test_stage2.py:197-203)."""
    return ", ".join("%s: %s" % (k, "%0.4f" % v if isinstance(v, float) else v) for k, v in meas.items())


def load_checkpoint(path, netG):
    """Weights of `path` into the SAME module instance (model.load_network, test_stage2.py:114) and every cached fold / packed filter
    of it dropped.  strict: a file that does not fit the network would leave the previous checkpoint's weights to be scored under
    this one's name.  (The inference graphs pack through HipModule._packed only; a trainer's ops.PackCache re-packs on entry.)"""
    from . import checkpoint

    checkpoint.load_network(path, netG, strict=True)
    netG.invalidate()


def warm(stage, netG, net_hq, precision=None, device=None):
    """One WARM_SIDE x WARM_SIDE image through the stage's graph: every fold and packed filter is rebuilt here (they do not depend
    on the image size), so that the sweep can time the re-pack of a checkpoint swap apart from the scoring."""
    import torch

    lr = torch.zeros(1, 3, WARM_SIDE, WARM_SIDE, dtype=torch.float32, device=device)
    with torch.no_grad():
        if stage == "stage2":
            netG.enhance_nhwc(net_hq, lr, precision=precision)
        else:
            netG.reverse_flow_nhwc(net_hq, lr, precision=precision)


def build_nets(stage, net_vq=None, device=None):
    """(netG, net_hq) of the stage as glare_amd.fit builds them, in eval mode: name-seeded, the VQGAN from `net_vq` if given."""
    from . import checkpoint

    return checkpoint.build_nets(stage, net_vq=net_vq, device=device)


def _read_csv_means(path, cols):
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    return {c: float(np.mean([float(r[c]) for r in rows])) for c in cols if rows and c in rows[0]}


def sweep(stage, run_or_files, out_dir, lows, gts, names=None, nets=None, select="PSNR", precision=None, batch=8, lpips_net=None,
          save_images=False, conf=None, score_fn=None, load_fn=None, warm_fn=None, sync=None, device=None, log=None):
    """Scores every checkpoint of `run_or_files` (list_checkpoints) on the pairs and returns the dict of the closing JSON line.
    nets: (netG, net_hq) instances every checkpoint is loaded into.  select: the column that names the best checkpoint (highest;
    lowest for the LPIPS columns); a column the stage does not produce raises ValueError before anything is scored.
    score_fn / load_fn / warm_fn / sync: the device calls (default score_checkpoint, load_checkpoint, warm, torch.cuda.synchronize)."""
    cols = columns(stage, lpips_net is not None)
    if select not in cols:
        raise ValueError("--select %s: %s produces the columns %s" % (select, stage, ", ".join(cols)))
    files = list_checkpoints(run_or_files)
    n = len(lows)
    names = list(names) if names is not None else ["%d.png" % i for i in range(n)]
    conf = conf or "train_%s_LOL" % stage
    if nets is None:
        import torch

        device = device or torch.device("cuda", torch.cuda.current_device())
        nets = build_nets(stage, device=device)
    netG, net_hq = nets
    if score_fn is None:
        import torch

        sync = sync or torch.cuda.synchronize
    score_fn, load_fn, warm_fn, sync = score_fn or score_checkpoint, load_fn or load_checkpoint, warm_fn or warm, sync or (lambda: None)
    os.makedirs(out_dir, exist_ok=True)
    results_path = os.path.join(out_dir, "results-%s.txt" % stage)
    done = []
    for path in files:
        name = os.path.splitext(os.path.basename(path))[0]
        csv_path = os.path.join(out_dir, name + ".csv")
        if os.path.isfile(csv_path):                                  # resumed sweep (test_stage2.py:126-127)
            done.append({"name": name, "means": _read_csv_means(csv_path, cols), "skipped": True})
            continue
        t0 = time.perf_counter()
        load_fn(path, netG)
        warm_fn(stage, netG, net_hq, precision, device)
        sync()
        t1 = time.perf_counter()
        report = {}
        rows = score_fn(stage, netG, net_hq, lows, gts, batch=batch, precision=precision, lpips_net=lpips_net, device=device, report=report,
                        keep_images=save_images)
        sync()
        t2 = time.perf_counter()
        lead = {"conf": conf, "heat": 0, "name": None}
        with open(csv_path + "_", "w", newline="") as f:              # under a temporary name: a CSV that exists is complete
            wr = csv.DictWriter(f, fieldnames=LEAD[stage] + cols)
            wr.writeheader()
            for nm, row in zip(names, rows):
                wr.writerow({**{k: (nm if k == "name" else lead[k]) for k in LEAD[stage]}, **{c: repr(row[c]) for c in cols}})
        os.replace(csv_path + "_", csv_path)
        means = {c: float(np.mean([r[c] for r in rows])) for c in cols}
        with open(results_path, "a") as f:
            f.write("%s %s\n" % (name, format_measurements(means)))
        for kind, imgs in report.get("images", {}).items():
            for nm, im in zip(names, imgs):
                write_image(os.path.join(out_dir, name, kind, nm), im)
        rec = {"name": name, "means": means, "skipped": False, "seconds_load_repack": round(t1 - t0, 4), "seconds_scoring": round(t2 - t1, 4),
               "bf16_rerun_images": [names[i] for i in report.get("bf16_rerun_images", [])]}
        done.append(rec)
        if log:
            log(rec)
    scored = [d for d in done if not d["skipped"]]
    ranked = [d for d in done if select in d["means"] and not math.isnan(d["means"][select])]
    best = None
    if ranked:
        pick = min if select in LOWER_IS_BETTER else max
        b = pick(ranked, key=lambda d: d["means"][select])
        best = {"name": b["name"], "column": select, "value": b["means"][select]}
    mean = lambda key: round(float(np.mean([d[key] for d in scored])), 4) if scored else None
    secs = sum(d["seconds_scoring"] for d in scored)
    return {"stage": stage, "images": n, "checkpoints": done, "best": best, "select": select,
            "seconds_per_checkpoint": {"load_repack": mean("seconds_load_repack"), "scoring": mean("seconds_scoring")},
            "images_per_sec_scoring": round(n * len(scored) / secs, 2) if secs > 0 else None,
            "bf16_rerun_images": {d["name"]: d["bf16_rerun_images"] for d in scored if d["bf16_rerun_images"]},
            "timed": "load_repack: file -> weights on the device + one %dx%d image through the graph (every fold and packed filter rebuilt); "
                     "scoring: uint8 pairs on the host -> per-image rows back on the host" % (WARM_SIDE, WARM_SIDE)}


def main(argv=None):
    from . import data as D

    ap = argparse.ArgumentParser(description="Score every checkpoint of a training run on the test split.")
    ap.add_argument("stage", choices=sorted(COLUMNS))
    ap.add_argument("--run", required=True, help="run folder of glare_amd.fit: <run>/models/<iter>_G.pth")
    ap.add_argument("--root", required=True, help="dataset folder (v1: <root>/eval15/{low,high}; v2: see --layout)")
    ap.add_argument("--layout", choices=sorted(D.LAYOUTS), default="v1")
    ap.add_argument("--net-vq", default=None, help="VQGAN checkpoint (reference format); without it the weights are name-seeded")
    ap.add_argument("--out", default=None, help="output folder (default <run>/results-<stage>)")
    ap.add_argument("--lpips", action="store_true", help="also the LPIPS-alex columns")
    ap.add_argument("--lpips-weights", default=None, help="state dict of lpips.LPIPS(net='alex') (torch.save); without it the net is name-seeded")
    ap.add_argument("--select", default="PSNR", help="the column that names the best checkpoint (default PSNR)")
    ap.add_argument("--precision", choices=("fp16", "bf16"), default=None,
                    help="16-bit format of activations and filters (default fp16; images whose fp16 output is not finite are re-run in bf16)")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--save-images", action="store_true", help="write the scored uint8 images under <out>/<name>/")
    args = ap.parse_args(argv)
    import torch

    if args.select not in columns(args.stage, args.lpips):
        ap.error("--select %s: %s produces %s" % (args.select, args.stage, ", ".join(columns(args.stage, args.lpips))))
    assert torch.cuda.is_available(), "glare_amd.evaluate needs an MI355X: the HIP kernels are the only implementation"
    device = torch.device("cuda", torch.cuda.current_device())
    ds = D.LAYOUTS[args.layout]({"root": args.root}, train=False)
    lows, gts = np.stack([p[0] for p in ds.pairs]), np.stack([p[1] for p in ds.pairs])
    names = [p[2] + ".png" for p in ds.pairs]
    lpips_net = None
    if args.lpips:
        from . import metrics

        lpips_net = metrics.build_lpips_alex(args.lpips_weights, device)
    nets = build_nets(args.stage, args.net_vq, device)
    res = sweep(args.stage, args.run, args.out or os.path.join(args.run, "results-%s" % args.stage), lows, gts, names, nets, args.select,
                args.precision, max(1, args.batch), lpips_net, args.save_images, device=device)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
