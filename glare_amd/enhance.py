"""Unpaired enhancement: photos of any size, no ground truth, enhanced images written back out -- the GLARE counterpart of
code/infer_unpaired.py:91-136 on the HIP path.

    python -m glare_amd.enhance photos/ more/img.png --out enhanced/ [--net-g G.pth --net-vq VQ.pth --precision fp16 --batch 8]
                                [--tile 512 --tile-overlap 64] [--niqe niqe_pris_params.npz]

Per image, the reference's steps: read as RGB uint8 (cv2.imread, :47), auto_padding to a multiple of 16 with cv2.BORDER_REFLECT
(:81-88), /255, log(clamp(x + 1e-3, min=1e-3)) (:39, :122), the network (get_sr, :128), crop + clamp + rgb() -- which truncates
(:42, :129-130) -- and imwrite under the same basename (:136).  Padding, the log transform, the crop and the uint8 conversion run on
the device (csrc/harness.hip): images cross PCIe as uint8 both ways.  Images of one padded shape are enhanced in batches; the size
envelope of the kernels (SIZE_TABLE) is checked before anything is launched; with --tile, an image larger than a tile is enhanced
as overlapping tiles that are feathered together on the device, so its size is bounded by memory alone.  Without checkpoints the
weights are name-seeded."""
import argparse
import glob
import json
import os
import re
import time

import numpy as np

from . import harness

# ---- the size envelope ------------------------------------------------------------------------------------------------------
# Extents of the inference graph that the kernels address through 32-bit buffer offsets or 31-bit block counts, in bytes (or
# blocks) per PADDED full-resolution pixel.  Every row names the C check it mirrors; the product returns GLARE_ERR_UNSUPPORTED /
# GLARE_ERR_INVALID (or, for the DCN, leaves its fast path) above the limit.  An extent is
#     ceil64(Hp * Wp) * (per_image + per_more_image * (B - 1)) + const
# (ceil64: the DCN's offset planes are padded to 64 pixels; applied to every row, so each is an upper bound).  Derived from the layer
# list (ch = 128, ch_mult = (1, 2, 4), attention at 1/4 resolution with 512 channels, WarpBlock DCN: dg = 4, 3 x 3) and checked
# against every launch of a run by tests/test_gpu_enhance.py.
# (name, C check, per_image, per_more_image, const, limit; an extent must stay < limit)
SIZE_TABLE = (
    # the two decoders' first ResnetBlock at full resolution reads the upsampled 256-channel map: 256 ch x 2 B
    ("conv source, one image", "conv_igemm.hip:392-394  H*W*pitch*2 < 0x7ff00000", 512, 0, 0, 0x7ff00000),
    # the full-resolution WarpBlock: x = the VQ decoder's 128-channel feature, 16-bit, the whole batch
    ("DCN x, whole batch", "dcn.hip:771-781  B*H*W*pitch*2 < 2^31-1", 256, 256, 0, 0x7fffffff),
    # conv_offset's planar fp32 output [B][3*dg*9 = 108][plane]: the offsets are its first 72 planes, the mask the last 36
    ("DCN offsets, whole batch", "dcn.hip:773-781  ((B-1)*108 + 72)*plane*4 < 2^31-1", 288, 432, 0, 0x7fffffff),
    ("DCN mask, whole batch", "dcn.hip:774-781  ((B-1)*108 + 36)*plane*4 < 2^31-1", 144, 432, 0, 0x7fffffff),
    # attention at 1/4 resolution (N = Hp*Wp/16 tokens): q and k interleaved, ldk = 1024 (AttnBlock's d512 form), 16-bit
    ("attention K, one image", "attn.hip:712  (N*ldk + 512)*2 < 0x7ff00000", 128, 0, 1024, 0x7ff00000),
    ("attention V^T, one image", "attn.hip:712  512*v_pitch*2 < 0x7ff00000", 64, 0, 65536, 0x7ff00000),
    ("attention K/V (shared), one image", "attn.hip:674  (N*ldkv + 512)*2 < 0x7ff00000", 64, 0, 1024, 0x7ff00000),
    ("conv1x1 pixels, one image", "conv1x1.hip:403/466  pixels_per_image <= 2^31-1", 1, 0, 0, 0x80000000),
)


def _extent(row, hp, wp, batch):
    _, _, per, more, const, _ = row
    px = (hp * wp + 63) // 64 * 64
    return px * (per + more * (batch - 1)) + const


def check_size(hp, wp, batch=1, name=None):
    """Raises ValueError, before any launch, when a batch of `batch` images padded to hp x wp crosses a row of SIZE_TABLE."""
    for row in SIZE_TABLE:
        e = _extent(row, hp, wp, batch)
        if e >= row[5]:
            raise ValueError("%s: padded size %dx%d (batch %d) is outside the size envelope: %s = %d B, limit %d B (%s)"
                             % (name or "image", hp, wp, batch, row[0], e, row[5], row[1]))


def max_batch(hp, wp, cap=1 << 16):
    """The largest batch of hp x wp padded images that check_size accepts (0: not even one)."""
    b = 0
    while b < cap:
        try:
            check_size(hp, wp, b + 1)
        except ValueError:
            break
        b += 1
    return b


# ---- the tile plan ----------------------------------------------------------------------------------------------------------
# An image with a side longer than `tile` is enhanced as overlapping windows of one shape that are feathered back together
# (DESIGN.md "Tiled enhancement"): each window stays inside the size envelope and near the token count the network was trained at.
def plan_axis(L, tile, overlap):
    """One axis of the plan -> (starts, length, keep0): the image coordinate of each window's first pixel, the windows' common
    length, and the offset inside the first window at which image coordinate 0 lies.  L <= tile: one window [-p1, L + p2) with
    auto_padding's (p1, p2) -- the axis exactly as the untiled path pads it.  L > tile: windows of `tile` pixels every tile - overlap,
    the last one shifted back to end at L; every window lies inside the image, nothing is padded, up to three cover a coordinate."""
    if L < 1 or tile < 16 or tile % 16 != 0 or overlap < 16 or tile < 2 * overlap:
        raise ValueError("tile plan: L = %d, tile = %d, overlap = %d (need L >= 1, tile a multiple of 16, overlap >= 16, tile >= 2 * overlap)"
                         % (L, tile, overlap))
    if L <= tile:
        p1, p2 = harness.auto_padding(L, L)[:2]
        return [-p1], L + p1 + p2, p1
    stride = tile - overlap
    n = -(-(L - overlap) // stride)
    return [min(i * stride, L - tile) for i in range(n)], tile, 0


def axis_weights(L, starts, length, overlap):
    """The blend table of one axis -> (first int32 [L], count int32 [L], weight fp32 [L,3]): per image coordinate the first window
    that covers it, the number of covering windows (consecutive, <= 3) and their weights.  Window i of n ramps over the REQUESTED
    overlap O, whatever its actual overlap with the neighbour: r_i(x) = min(1, (x + 0.5 - s_i) / O if i > 0, (s_i + length - x - 0.5) / O
    if i < n - 1); weight = r_i / sum_k r_k in fp64, rounded once to fp32 (a lone window: exactly 1)."""
    n = len(starts)
    x = np.arange(L, dtype=np.float64)
    r = np.zeros((n, L), dtype=np.float64)
    for i, s in enumerate(starts):
        ri = np.ones(L, dtype=np.float64)
        if i > 0:
            ri = np.minimum(ri, (x + 0.5 - s) / overlap)
        if i < n - 1:
            ri = np.minimum(ri, (s + length - x - 0.5) / overlap)
        r[i] = np.where((x >= s) & (x < s + length), ri, 0.0)
    cover = r > 0
    count = cover.sum(axis=0)
    first = cover.argmax(axis=0)
    assert count.min() >= 1 and count.max() <= 3, "tile plan: a coordinate is covered by %d..%d windows" % (count.min(), count.max())
    norm = r / r.sum(axis=0)
    weight = np.zeros((L, 3), dtype=np.float32)
    cols = np.arange(L)
    for a in range(3):
        sel = count > a
        weight[sel, a] = norm[np.minimum(first + a, n - 1), cols][sel].astype(np.float32)
    return first.astype(np.int32), count.astype(np.int32), weight


def plan_tiles(h, w, tile=512, overlap=64, name=None):
    """The plan of an h x w image: window origins per axis (ys, xs), the windows' shape (th, tw), where image coordinate (0, 0) lies
    in the first window (keep) and the two blend tables.  check_size() refuses a window shape outside the envelope before any launch."""
    ys, th, ky = plan_axis(h, tile, overlap)
    xs, tw, kx = plan_axis(w, tile, overlap)
    check_size(th, tw, 1, name)
    return {"h": h, "w": w, "tile": tile, "overlap": overlap, "ys": ys, "xs": xs, "th": th, "tw": tw, "keep": (ky, kx),
            "row_table": axis_weights(h, ys, th, overlap), "col_table": axis_weights(w, xs, tw, overlap)}


def enhance_tiled(img_u8, netG=None, net_vq=None, tile=512, overlap=64, precision=None, batch=8, tile_fn=None, blend_fn=None,
                  device=None, report=None, name=None):
    """uint8 [h,w,3] of any size -> the enhanced uint8 [h,w,3], through overlapping windows of plan_tiles(h, w, tile, overlap).

    The image is uploaded once as uint8; its windows are gathered on the device into the log domain (harness.tile_gather_device), run
    through netG.reverse_flow_nhwc in batches of min(batch, max_batch(th, tw)) -- all windows share one shape --, their fp32 outputs
    stay on the device and one launch blends, clamps and truncates them to uint8 (harness.tile_blend_device).  If any window value
    inside the image is inf / NaN and the precision is not bf16, all windows run again in bf16 (report["bf16_rerun"] = True).
    tile_fn(lr fp32 [n,3,th,tw] log domain, precision) -> network outputs of the same shape, and blend_fn(outputs [N,3,th,tw], plan) ->
    (uint8 [h,w,3], non-finite count) replace the network and the blend with host code (both or neither); the windows are then cut
    by harness.tile_gather.  report: a dict that receives "tiles" = [n_ty, n_tx], "tile_shape", "nonfinite" and "bf16_rerun"."""
    assert img_u8.dtype == np.uint8 and img_u8.ndim == 3 and img_u8.shape[2] == 3, (name, img_u8.dtype, img_u8.shape)
    if (tile_fn is None) != (blend_fn is None):
        raise ValueError("enhance_tiled: tile_fn and blend_fn replace the device path together")
    h, w = img_u8.shape[:2]
    plan = plan_tiles(h, w, tile, overlap, name)
    th, tw = plan["th"], plan["tw"]
    origins = [(y, x) for y in plan["ys"] for x in plan["xs"]]
    n = len(origins)
    bs = max(1, min(batch, max_batch(th, tw)))
    if tile_fn is not None:
        lr = harness.tile_gather(img_u8, origins, th, tw)

        def once(prec):
            outs = np.concatenate([np.asarray(tile_fn(lr[s:s + bs], prec), dtype=np.float32) for s in range(0, n, bs)])
            return blend_fn(outs, plan)
    else:
        import torch

        device = device or torch.device("cuda", torch.cuda.current_device())
        src = _stack([img_u8])
        img_d = (src if isinstance(src, torch.Tensor) else torch.from_numpy(src))[0].to(device, non_blocking=True)      # uint8, once
        origins_d = torch.tensor(origins, dtype=torch.int32).to(device)
        tables = harness.tile_blend_tables(plan, device)

        def once(prec):
            outs = torch.empty(n, 3, th, tw, dtype=torch.float32, device=device)
            with torch.no_grad():
                for s in range(0, n, bs):
                    lr = harness.tile_gather_device(img_d, origins_d[s:s + bs], th, tw)
                    outs[s:s + bs].copy_(netG.reverse_flow_nhwc(net_vq, lr, precision=prec)["out"])
            u8, _, bad = harness.tile_blend_device(outs, plan, tables)
            return u8.cpu().numpy(), int(bad.cpu())

    out, bad = once(precision)
    rerun = int(bad) > 0 and precision != "bf16"       # fp16 overflow: bf16 has fp32's range, same kernels
    if rerun:
        out, bad = once("bf16")
    if report is not None:
        report.update(tiles=[len(plan["ys"]), len(plan["xs"])], tile_shape=[th, tw], nonfinite=int(bad), bf16_rerun=rerun)
    return out


# ---- reading and writing ----------------------------------------------------------------------------------------------------
def natural_key(path):
    """natsort's order for plain file names: digit runs compare as numbers (img2 before img10)."""
    return [(0, int(t), "") if t.isdigit() else (1, 0, t) for t in re.split(r"(\d+)", os.path.basename(path)) if t != ""]


def list_inputs(paths):
    """Files and folders -> file list; a folder means <dir>/*.* in natural order (fiFindByWildcard, infer_unpaired.py:17-18)."""
    out = []
    for p in paths:
        if os.path.isdir(p):
            out += sorted((f for f in glob.glob(os.path.join(p, "*.*")) if os.path.isfile(f)), key=natural_key)
        else:
            out.append(p)
    return out


# PIL modes cv2.imread(IMREAD_COLOR) turns into 8-bit BGR that PIL converts to RGB the same way: 8-bit gray (+ alpha), palette, colour
_CONVERTIBLE = {"RGB", "RGBA", "RGBX", "L", "LA", "P", "PA", "1", "CMYK", "YCbCr"}


def read_image(path):
    """-> (uint8 [H,W,3] RGB, None) or (None, reason).  EXIF orientation applied (cv2's IMREAD_COLOR does), gray -> 3 channels,
    alpha dropped; modes that do not convert to 8-bit RGB faithfully (16-bit, float) are refused."""
    from PIL import Image, ImageOps

    try:
        with Image.open(path) as im:
            im.load()
            mode = im.mode
            if mode not in _CONVERTIBLE:
                return None, "unsupported image mode %s" % mode
            im = ImageOps.exif_transpose(im)
            if mode in ("RGBA", "LA", "PA") or (mode == "P" and "transparency" in im.info):
                im = im.convert("RGBA").convert("RGB")      # alpha dropped, not composited (cv2.imread's IMREAD_COLOR)
            else:
                im = im.convert("RGB")
            return np.ascontiguousarray(np.asarray(im, dtype=np.uint8)), None
    except Exception as e:          # not an image, truncated, unknown format
        return None, "cannot read: %s" % (str(e) or type(e).__name__)


def write_image(path, img):
    from PIL import Image

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    ext = os.path.splitext(path)[1].lower()
    kw = {"quality": 95} if ext in (".jpg", ".jpeg") else {}        # cv2.IMWRITE_JPEG_QUALITY defaults to 95
    Image.fromarray(img).save(path, **kw)


# ---- the network call -------------------------------------------------------------------------------------------------------
def device_enhance_fn(netG, net_vq, device):
    """enhance_fn over the HIP path: pinned uint8 [n,H,W,3] + pads -> (uint8 [n,h,w,3] on the host, int32 [n] non-finite counts).
    The uint8 batch crosses PCIe as uint8; pad, log, network, crop and rgb() run on the device."""
    import torch

    def fn(batch_u8, pads, precision):
        h, w = batch_u8.shape[1], batch_u8.shape[2]
        src = batch_u8 if isinstance(batch_u8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(batch_u8))
        lr = harness.preprocess_unpaired_device(src.to(device, non_blocking=True), pads)
        with torch.no_grad():
            out = netG.reverse_flow_nhwc(net_vq, lr, precision=precision)["out"]
        u8, bad = harness.postprocess_unpaired_device(out, pads, h, w, want_nonfinite=True)
        return u8.cpu().numpy(), bad.cpu().numpy()

    return fn


def enhance_images(imgs, netG=None, net_vq=None, precision=None, batch=8, enhance_fn=None, names=None, device=None, report=None,
                   tile=None, overlap=64, tile_fn=None, blend_fn=None):
    """uint8 HWC arrays of any sizes -> the enhanced uint8 arrays, same shapes, same order.

    Images are grouped by padded shape and each group runs in batches of at most `batch`, capped by max_batch() (the DCN fast path's
    whole-batch extents).  check_size() refuses an image outside the envelope with ValueError before anything is launched.
    enhance_fn(batch_u8 [n,H,W,3], pads, precision) -> (uint8 [n,H,W,3], nonfinite [n]): the network call (default: the HIP path
    over netG / net_vq).  An image whose fp16 output holds inf / NaN before the clamp is run again in bf16 and named in
    report["bf16_rerun_images"] (as glare_amd.infer does).  report: a dict that receives that list and per-image padded sizes.
    tile: an image with a side longer than `tile` goes through enhance_tiled(tile, overlap, tile_fn, blend_fn) instead -- one image at
    a time, its windows batched; report["tiles"] maps its name to [n_ty, n_tx] and its "padded" entry is the windows' shape.  Without
    `tile` nothing is tiled and such an image is refused as before."""
    names = list(names) if names is not None else ["#%d" % i for i in range(len(imgs))]
    shapes, tiled = [], {}
    for i, (nm, im) in enumerate(zip(names, imgs)):
        assert im.dtype == np.uint8 and im.ndim == 3 and im.shape[2] == 3, (nm, im.dtype, im.shape)
        if tile is not None and max(im.shape[:2]) > tile:
            tiled[i] = plan_tiles(im.shape[0], im.shape[1], tile, overlap, nm)       # raises before any launch, as check_size does
            shapes.append((tiled[i]["th"], tiled[i]["tw"], None))
            continue
        pads = harness.auto_padding(im.shape[0], im.shape[1])
        hp, wp = im.shape[0] + pads[0] + pads[1], im.shape[1] + pads[2] + pads[3]
        check_size(hp, wp, 1, nm)
        shapes.append((hp, wp, pads))
    if enhance_fn is None and len(tiled) < len(imgs):
        import torch

        device = device or torch.device("cuda", torch.cuda.current_device())
        enhance_fn = device_enhance_fn(netG, net_vq, device)
    groups = {}
    for i, im in enumerate(imgs):
        if i not in tiled:
            groups.setdefault((im.shape[0], im.shape[1]), []).append(i)
    results = [None] * len(imgs)
    reruns, per_size, tiles = [], {}, {}
    for i, plan in tiled.items():
        t0 = time.perf_counter()
        rep = {}
        results[i] = enhance_tiled(imgs[i], netG, net_vq, tile, overlap, precision, batch, tile_fn, blend_fn, device, rep, names[i])
        tiles[names[i]] = rep["tiles"]
        if rep["bf16_rerun"]:
            reruns.append(names[i])
        per_size["%dx%d" % imgs[i].shape[:2]] = round(time.perf_counter() - t0, 4)       # the result is a host array: synchronous
    for (h, w), idx in groups.items():
        t0 = time.perf_counter()
        hp, wp, pads = shapes[idx[0]]
        bs = max(1, min(batch, max_batch(hp, wp)))
        for s in range(0, len(idx), bs):
            part = idx[s:s + bs]
            stack = _stack([imgs[i] for i in part])
            out, bad = enhance_fn(stack, pads, precision)
            for j, i in enumerate(part):
                results[i] = out[j]
                if int(bad[j]) > 0 and precision != "bf16":       # fp16 overflow: bf16 has fp32's range, same kernels
                    results[i] = enhance_fn(_stack([imgs[i]]), pads, "bf16")[0][0]
                    reruns.append(names[i])
        per_size["%dx%d" % (h, w)] = round((time.perf_counter() - t0) / len(idx), 4)   # enhance_fn hands back host arrays: synchronous
    if report is not None:
        report["seconds_per_image_by_size"] = per_size
        report["bf16_rerun_images"] = [n for n in names if n in reruns]
        report["padded"] = [list(s[:2]) for s in shapes]
        report["tiles"] = tiles
    return results


def _stack(ims):
    """uint8 [n,H,W,3], in pinned host memory when a GPU is there (the H2D copy is then an asynchronous DMA)."""
    a = np.stack(ims)
    try:
        import torch

        if torch.cuda.is_available():
            return torch.from_numpy(a).pin_memory()
    except Exception:
        pass
    return a


# ---- the driver -------------------------------------------------------------------------------------------------------------
def load_nets(net_g=None, net_vq=None, device=None):
    """The two networks as glare_amd.infer builds them: name-seeded, checkpoints (reference format) loaded with strict=False."""
    from . import checkpoint

    return checkpoint.build_nets("stage3", net_g=net_g, net_vq=net_vq, device=device)


def run(inputs, out_dir, netG=None, net_vq=None, precision=None, batch=8, enhance_fn=None, device=None, tile=None, overlap=64,
        tile_fn=None, blend_fn=None, niqe=None, niqe_fn=None):
    """Enhance every readable image of `inputs` (files and folders) into out_dir under its basename; -> the result dict of the
    JSON line (per-image name / size / padded size, "tiles": [n_ty, n_tx] for an image enhanced in tiles, skipped files with reasons,
    bf16 re-runs, seconds, images/s, MP/s).  tile / overlap: as enhance_images.
    niqe: a NIQE pristine model (metrics.load_niqe_params).  Every image entry then gains "niqe_in" (the input) and "niqe" (the enhanced
    image, assembled where it was tiled) -- null with a "niqe_reason" where an image has no score -- and the line "niqe_in_mean",
    "niqe_mean" (over the scored images) and "niqe_seconds"; scoring runs after the timed region, which stays what it is without it.
    niqe_fn(list of uint8 images) -> list of (score or None, reason or None) replaces metrics.niqe_scores."""
    files = list_inputs(inputs)
    imgs, names, skipped = [], [], []
    for f in files:
        img, why = read_image(f)
        if img is None:
            skipped.append({"name": os.path.basename(f), "reason": why})
        else:
            imgs.append(img)
            names.append(os.path.basename(f))
    sync = lambda: None
    if enhance_fn is None and tile_fn is None:
        import torch

        sync = torch.cuda.synchronize
        if imgs:                      # warm-up at the smallest shape: weight packing, workspace growth, kernel loading
            small = min(imgs, key=lambda a: a.shape[0] * a.shape[1])
            enhance_images([small], netG, net_vq, precision, 1, device=device, tile=tile, overlap=overlap)
        sync()
    report = {}
    t0 = time.perf_counter()
    outs = enhance_images(imgs, netG, net_vq, precision, batch, enhance_fn, names, device, report, tile, overlap, tile_fn, blend_fn)
    sync()
    secs = time.perf_counter() - t0          # uint8 on the host -> uint8 back on the host (excluding decode / encode of the files)
    for nm, o in zip(names, outs):
        write_image(os.path.join(out_dir, nm), o)
    mp = sum(a.shape[0] * a.shape[1] for a in imgs) / 1e6
    tiles = report.get("tiles", {})
    res = {"images": [dict({"name": n, "size": [int(a.shape[0]), int(a.shape[1])], "padded": p}, **({"tiles": tiles[n]} if n in tiles else {}))
                       for n, a, p in zip(names, imgs, report.get("padded", []))],
            "skipped": skipped, "bf16_rerun_images": report.get("bf16_rerun_images", []),
            "seconds": round(secs, 4), "seconds_per_image_by_size": report.get("seconds_per_image_by_size", {}), "images_per_sec": round(len(imgs) / secs, 3) if imgs and secs > 0 else 0.0,
            "megapixels_per_sec": round(mp / secs, 3) if imgs and secs > 0 else 0.0,
            "timed": "uint8 in pinned host memory -> uint8 back on the host, one warm-up image first; file decode / encode excluded"}
    if niqe is not None:
        if niqe_fn is None:
            from . import metrics

            niqe_fn = lambda ims: metrics.niqe_scores(ims, niqe)
        t1 = time.perf_counter()
        scored = {"niqe_in": niqe_fn(imgs), "niqe": niqe_fn(outs)}       # each ends in a copy to the host: synchronous
        res["niqe_seconds"] = round(time.perf_counter() - t1, 4)
        for key, pairs in scored.items():
            for entry, (score, why) in zip(res["images"], pairs):
                entry[key] = score
                if score is None:
                    entry.setdefault("niqe_reason", why)
            vals = [s for s, _ in pairs if s is not None]
            res[key + "_mean"] = sum(vals) / len(vals) if vals else None
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description="Enhance low-light photos of any size (no ground truth needed).")
    ap.add_argument("inputs", nargs="+", help="image files and / or folders (a folder: <dir>/*.* in natural order)")
    ap.add_argument("--out", required=True, help="output folder; each image is written under its own basename")
    ap.add_argument("--net-g", default=None, help="net_G checkpoint (reference format); without it the weights are name-seeded")
    ap.add_argument("--net-vq", default=None, help="VQGAN checkpoint (reference format)")
    ap.add_argument("--precision", choices=("fp16", "bf16"), default=None,
                    help="16-bit format of activations and filters (default fp16; images whose fp16 output is not finite are re-run in bf16)")
    ap.add_argument("--batch", type=int, default=8, help="images of one padded size per launch (capped by the size envelope)")
    ap.add_argument("--tile", type=int, default=None, metavar="N",
                    help="enhance an image with a side longer than N pixels as overlapping N x N tiles that are feathered together (a multiple of 16, "
                         "e.g. 512); without it such an image must fit the kernels' size envelope (about 4 MP)")
    ap.add_argument("--tile-overlap", type=int, default=64, metavar="O", help="overlap of neighbouring tiles in pixels (>= 16, at most N / 2)")
    ap.add_argument("--niqe", default=None, metavar="PARAMS.npz",
                    help="score every input and every enhanced image with NIQE on the device (lower is better); PARAMS.npz is the pristine "
                         "model, basicsr's niqe_pris_params.npz")
    args = ap.parse_args(argv)
    import torch

    niqe = None
    if args.niqe is not None:
        from . import metrics

        niqe = metrics.load_niqe_params(args.niqe)          # a bad file is refused before the networks are built

    assert torch.cuda.is_available(), "glare_amd.enhance needs an MI355X: the HIP kernels are the only implementation"
    device = torch.device("cuda", torch.cuda.current_device())
    netG, net_vq = load_nets(args.net_g, args.net_vq, device)
    res = run(args.inputs, args.out, netG, net_vq, args.precision, max(1, args.batch), device=device, tile=args.tile, overlap=args.tile_overlap,
              niqe=niqe)
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    main()
