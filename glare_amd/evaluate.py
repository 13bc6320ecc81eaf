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
Rows are written in dataset order (the reference prepends each new row).  Without checkpoints the weights are name-seeded.

    python -m glare_amd.evaluate stage1 --run RUN --root LOLdataset [...]          (no --net-vq: the run's own files are the VQGAN)
    python -m glare_amd.evaluate stage3 --run RUN --root LOLdataset --ema          (the averaged weights of `fit --weights-ema`: *_G_ema.pth)

scores every `RUN/models/*_VQ.pth` of `glare_amd.fit stage1`, the file `--net-vq` takes everywhere else, by the prior's own
reconstruction of the ground truth (stage1_reconstruct, the protocol of fit.make_validate_stage1): pad bottom / right by symmetric
reflection to multiples of 4, / 255, encode_nhwc, decode_nhwc(straight_through=True), uint8 of the image's own window.  Columns:
`PSNR` (psnr_u8), `SSIM` (calculate_ssim on that uint8 image), `codes` = the distinct codes the image's latent uses, `LPIPS` on request.
Per checkpoint the use of the codebook over every token of the split -- {tokens, active, active_fraction, perplexity} (quantize.py:83-85),
counted on the device (csrc/vq_usage.hip, metrics.CodebookUsage) -- goes into the record, the closing JSON and the results-stage1.txt
line, and `<out>/<name>.codes.npy` holds the int64 [K] counts (what basicsr/active_codebook.py plots)."""
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
COLUMNS = {"stage1": ("PSNR", "SSIM", "codes", "LPIPS"), "stage2": ("Adjust_PSNR", "Adjust_LPIPS", "PSNR", "LPIPS"),
           "stage3": ("PSNR", "SSIM", "1_PSNR", "LPIPS")}
LEAD = {"stage1": ("conf", "name"), "stage2": ("conf", "heat", "name"), "stage3": ("conf", "name")}
CHECKPOINT_TAG = {"stage1": "VQ", "stage2": "G", "stage3": "G"}       # <iter>_<tag>.pth: what glare_amd.fit writes for the stage
LOWER_IS_BETTER = ("LPIPS", "Adjust_LPIPS")
NO_EMA_FILES = ("--ema: %s holds no *_%s_ema.pth: the averaged weights are written by a run trained with `glare_amd.fit ... --weights-ema DECAY`; "
                "without --ema the run's own weights are scored")
NET_VQ_REFUSAL = "--net-vq is not a stage1 option: the run's own <iter>_VQ.pth files are the VQGAN that is scored"
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


def stage1_pads(h, w):
    """(top, bottom, left, right): bottom / right up to multiples of 4, the encoder's stride."""
    return (0, -h % 4, 0, -w % 4)


def stage1_reconstruct(net, highs, precision=None):
    """The stage-1 protocol on uint8 ground-truth images `highs` [n,h,w,3] (host): padded bottom / right by symmetric reflection to
    multiples of 4, / 255, VQModel.encode_nhwc, decode_nhwc(want_image=True, straight_through=True) as stages 2 and 3 call them ->
    (img fp32 NCHW [n,3,hp,wp], gt uint8 [n,h,w,3], u8 = rgb(img) of the image's own window, sse int64 [n], idx int64 [n * hp/4 * wp/4]),
    all on the device and nothing read back.  PSNR: harness.psnr_u8(sse, 3 h w).  The caller sets eval mode and no_grad."""
    import torch

    from . import ops

    highs = np.asarray(highs)
    assert highs.dtype == np.uint8 and highs.ndim == 4 and highs.shape[3] == 3, (highs.dtype, highs.shape)
    n, h, w, _ = highs.shape
    _, pb, _, pr = stage1_pads(h, w)
    padded = np.pad(highs, [(0, 0), (0, pb), (0, pr), (0, 0)], "symmetric")
    with ops.use_precision(ops.inference_precision(precision)):
        x = torch.from_numpy(np.ascontiguousarray(padded.transpose(0, 3, 1, 2)).astype(np.float32) / 255).cuda()
        idx, img, _ = net.decode_nhwc(net.encode_nhwc(x), want_image=True, straight_through=True)
        img = img.float().contiguous()
        gt = torch.from_numpy(np.array(highs)).cuda()                            # (a copy: the dataset's arrays are read-only)
        u8, sse = harness.score_device(img, gt, window=(0, 0, h, w))
    return img, gt, u8, sse, idx


def _device_rows_stage1(net, highs, precision, lpips_net, want_images, usage):
    """One stage-1 batch -> ({column: host float64 [n]}, non-finite counts [n], {image kind: uint8 device tensor}, counts int64 [n, K] on
    the device: what this batch added to `usage`)."""
    import torch

    from . import ops

    n, h, w, _ = highs.shape
    with torch.no_grad():
        img, gt, u8, sse, idx = stage1_reconstruct(net, highs, precision)
        _, bad = harness.postprocess_unpaired_device(img, (0, 0, 0, 0), h, w, want_nonfinite=True)            # the overflow flag only
        counts, _ = usage.update(idx, groups=n)
        cols = {"PSNR": sse, "SSIM": harness.ssim_device(u8.float() / 255, gt), "codes": ops.vq_usage_stats(counts)[1].double()}
        if lpips_net is not None:
            from . import metrics

            cols["LPIPS"] = lpips_net(metrics.to_lpips_input(u8), metrics.to_lpips_input(gt)).view(-1).double()
    host = {}
    for c, v in cols.items():
        v = v.cpu().numpy()
        host[c] = np.array([harness.psnr_u8(s, 3 * h * w) for s in v]) if v.dtype == np.int64 else v.astype(np.float64)
    return host, bad.cpu().numpy(), ({"": u8} if want_images else {}), counts


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
    if stage == "stage1":
        pads = stage1_pads(h, w)
        check_size(h + pads[1], w + pads[3], batch)
    elif stage == "stage2":
        pads = stage2_pads(h, w)
        check_size(h + pads[1], w + pads[3], batch)
    else:
        check_size(h + harness.PAD, w + harness.PAD, batch)
    assert torch.cuda.is_available(), "glare_amd.evaluate needs an MI355X: the HIP kernels are the only implementation"
    device = device or torch.device("cuda", torch.cuda.current_device())
    precision = ops.inference_precision(precision)
    usage = None
    if stage == "stage1":           # the prior reconstructs the ground truth: `lows` is not read
        from . import metrics

        usage = metrics.CodebookUsage(netG.quantize.n_e, device)

        def run(lo, hi, prec):
            return _device_rows_stage1(netG, gts[lo:hi], prec, lpips_net, keep_images, usage)
    else:
        lows_p, gts_p = torch.from_numpy(lows).pin_memory(), torch.from_numpy(gts).pin_memory()

        def run(lo, hi, prec):
            return _device_rows(stage, netG, net_hq, lows_p[lo:hi].to(device, non_blocking=True), gts_p[lo:hi].to(device, non_blocking=True),
                                prec, lpips_net, keep_images) + (None,)

    rows, reruns, kept = [None] * n, [], {}
    for lo in range(0, n, batch):
        hi = min(lo + batch, n)
        cols, bad, images, counts = run(lo, hi, precision)
        images = {k: v.cpu().numpy() for k, v in images.items()}
        for j in range(hi - lo):
            flagged = int(bad[j]) > 0 or not all(math.isfinite(cols[c][j]) or cols[c][j] == math.inf for c in cols)
            if flagged and precision != "bf16":       # fp16 overflow: bf16 has fp32's range, same kernels; a flagged exception
                if usage is not None:
                    usage.discard(counts[j])          # the re-run's indices are the ones that count
                c1, _, im1, _ = run(lo + j, lo + j + 1, "bf16")
                for c in cols:
                    cols[c][j] = c1[c][0]
                for k in images:
                    images[k][j] = im1[k][0].cpu().numpy()
                reruns.append(lo + j)
            rows[lo + j] = {c: float(cols[c][j]) for c in columns(stage, lpips_net is not None)}
        for k, v in images.items():
            kept.setdefault(k, []).append(v)
    if report is not None:
        if usage is not None:
            report["codebook"] = usage.stats()
            report["codes"] = usage.counts().cpu().numpy()
        report["bf16_rerun_images"] = reruns
        if keep_images:
            report["images"] = {k: np.concatenate(v) for k, v in kept.items()}
    return rows


# ---- the sweep ----------------------------------------------------------------------------------------------------------------
def list_checkpoints(run_or_files, stage="stage2", ema=False):
    """A run folder -> its models/*_G.pth (stage1: *_VQ.pth) in natural order (natsorted(os.listdir(.../models)), test_stage2.py:110);
    a list of files -> the same order.  ema: the averaged weights of `glare_amd.fit --weights-ema` instead, models/*_G_ema.pth (*_VQ_ema.pth):
    the two sets never mix, neither glob matches the other's names."""
    if isinstance(run_or_files, (str, os.PathLike)):
        files = glob.glob(os.path.join(run_or_files, "models", "*_%s%s.pth" % (CHECKPOINT_TAG[stage], "_ema" if ema else "")))
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
        if stage == "stage1":
            from . import ops

            with ops.use_precision(ops.inference_precision(precision)):
                netG.decode_nhwc(netG.encode_nhwc(lr), want_image=True, straight_through=True)
        elif stage == "stage2":
            netG.enhance_nhwc(net_hq, lr, precision=precision)
        else:
            netG.reverse_flow_nhwc(net_hq, lr, precision=precision)


def build_nets(stage, net_vq=None, device=None):
    """(netG, net_hq) of the stage as glare_amd.fit builds them, in eval mode: name-seeded, the VQGAN from `net_vq` if given."""
    from . import checkpoint

    if stage == "stage1" and net_vq:
        raise ValueError(NET_VQ_REFUSAL)
    return checkpoint.build_nets(stage, net_vq=net_vq, device=device)


USAGE_KEYS = ("tokens", "active", "active_fraction", "perplexity")     # the `codebook` block of a stage-1 record


def _usage_block(codes):
    """The `codebook` block from a host histogram (a resumed sweep's `<name>.codes.npy`), in float64."""
    from . import metrics

    return metrics.usage_block_host(codes)


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
    files = list_checkpoints(run_or_files, stage)
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
        codes_path = os.path.join(out_dir, name + ".codes.npy")       # stage 1: the int64 [K] use of the codebook over the split
        if os.path.isfile(csv_path):                                  # resumed sweep (test_stage2.py:126-127)
            done.append({"name": name, "means": _read_csv_means(csv_path, cols), "skipped": True})
            if stage == "stage1" and os.path.isfile(codes_path):
                done[-1]["codebook"] = _usage_block(np.load(codes_path))
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
        means = {c: float(np.mean([r[c] for r in rows])) for c in cols}
        codebook = None
        if report.get("codes") is not None:                          # written before the CSV: a CSV that exists has its counts beside it
            codes = np.asarray(report["codes"], dtype=np.int64)
            np.save(codes_path, codes)
            codebook = {k: v for k, v in (report.get("codebook") or _usage_block(codes)).items() if k in USAGE_KEYS}
        os.replace(csv_path + "_", csv_path)
        with open(results_path, "a") as f:
            usage_text = ", " + format_measurements({"codebook_" + k: v for k, v in codebook.items()}) if codebook else ""
            f.write("%s %s%s\n" % (name, format_measurements(means), usage_text))
        for kind, imgs in report.get("images", {}).items():
            for nm, im in zip(names, imgs):
                write_image(os.path.join(out_dir, name, kind, nm), im)
        rec = {"name": name, "means": means, "skipped": False, "seconds_load_repack": round(t1 - t0, 4), "seconds_scoring": round(t2 - t1, 4),
               "bf16_rerun_images": [names[i] for i in report.get("bf16_rerun_images", [])]}
        if codebook:
            rec["codebook"] = codebook
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
    usage = {"codebook": {d["name"]: d["codebook"] for d in done if "codebook" in d}} if stage == "stage1" else {}
    return {"stage": stage, "images": n, "checkpoints": done, "best": best, "select": select, **usage,
            "seconds_per_checkpoint": {"load_repack": mean("seconds_load_repack"), "scoring": mean("seconds_scoring")},
            "images_per_sec_scoring": round(n * len(scored) / secs, 2) if secs > 0 else None,
            "bf16_rerun_images": {d["name"]: d["bf16_rerun_images"] for d in scored if d["bf16_rerun_images"]},
            "timed": "load_repack: file -> weights on the device + one %dx%d image through the graph (every fold and packed filter rebuilt); "
                     "scoring: uint8 pairs on the host -> per-image rows back on the host" % (WARM_SIDE, WARM_SIDE)}


def main(argv=None):
    from . import data as D

    ap = argparse.ArgumentParser(description="Score every checkpoint of a training run on the test split.")
    ap.add_argument("stage", choices=sorted(COLUMNS))
    ap.add_argument("--run", required=True, help="run folder of glare_amd.fit: <run>/models/<iter>_G.pth (stage1: <iter>_VQ.pth)")
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
    ap.add_argument("--ema", action="store_true", help="score the averaged weights of a run trained with --weights-ema, <run>/models/<iter>_G_ema.pth "
                                                        "(stage1: <iter>_VQ_ema.pth), instead; the default output folder is <run>/results-<stage>-ema")
    args = ap.parse_args(argv)
    if args.stage == "stage1" and args.net_vq:
        ap.error(NET_VQ_REFUSAL)
    run = args.run
    if args.ema:
        run = list_checkpoints(args.run, args.stage, ema=True)
        if not run:
            ap.error(NO_EMA_FILES % (os.path.join(args.run, "models"), CHECKPOINT_TAG[args.stage]))
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
    res = sweep(args.stage, run, args.out or os.path.join(args.run, "results-%s%s" % (args.stage, "-ema" if args.ema else "")), lows, gts, names, nets, args.select,
                args.precision, max(1, args.batch), lpips_net, args.save_images, device=device)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
