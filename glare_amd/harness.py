"""Pre/post-processing of the inference harness (host side, as in the reference).

Mirrors code/infer_dataset_lol.py:113-153: reflect-pad 20 px at the bottom and the left (`impad`,
:71-72), HWC uint8 -> NCHW float /255 (`t`, :42), log(clamp(x + 1e-3, min=1e-3)) (:127-128,
`log_low: true`); after the network: crop `[:, :, :h, 20:]`, clamp to [0,1], GT-mean gain with the
cv2.COLOR_BGR2GRAY weights applied to RGB-ordered data (:142-144), PSNR (utils/utils2.py:32-36)."""
import math

import numpy as np
import torch

from . import _lib

PAD = 20


# ---- device versions (csrc/harness.hip): batched, uint8 in, PSNR out ------------------------------------------
def preprocess_device(imgs_u8):
    """uint8 device tensor [B,H,W,3] -> fp32 [B,3,H+20,W+20] in the log domain (same arithmetic as preprocess())."""
    _lib.require_cuda(imgs_u8)
    assert imgs_u8.dtype == torch.uint8 and imgs_u8.dim() == 4 and imgs_u8.shape[3] == 3 and imgs_u8.is_contiguous()
    B, H, W, _ = imgs_u8.shape
    out = torch.empty(B, 3, H + PAD, W + PAD, dtype=torch.float32, device=imgs_u8.device)
    _lib.check(_lib.lib().glare_harness_preprocess_u8(_lib.ptr(imgs_u8), B, H, W, PAD, _lib.ptr(out), _lib.stream_handle()),
               "glare_harness_preprocess_u8")
    return out


def postprocess_device(out_nchw, h, w, gts_u8=None, want_nonfinite=False):
    """network output [B,3,Hp,Wp] (device) -> (restored float [B,h,w,3], psnr float64 [B] or None), all on the device.
    want_nonfinite: a third result, int32 [B] = inf / NaN values of the network output inside each crop BEFORE the clamp (which maps
    +inf to 1.0 and would hide an fp16 overflow behind a finite PSNR)."""
    _lib.require_cuda(out_nchw, gts_u8)
    out_nchw = out_nchw.float().contiguous()
    B, _, Hp, Wp = out_nchw.shape
    lib = _lib.lib()
    nws = lib.glare_harness_postprocess_workspace_bytes(B)
    ws = torch.empty(nws, dtype=torch.uint8, device=out_nchw.device)
    restored = torch.empty(B, h, w, 3, dtype=torch.float32, device=out_nchw.device)
    psnr_t = None
    if gts_u8 is not None:
        assert gts_u8.dtype == torch.uint8 and tuple(gts_u8.shape) == (B, h, w, 3) and gts_u8.is_contiguous()
        psnr_t = torch.empty(B, dtype=torch.float64, device=out_nchw.device)
    bad = torch.empty(B, dtype=torch.int32, device=out_nchw.device) if want_nonfinite else None
    _lib.check(lib.glare_harness_postprocess_flagged_f32(_lib.ptr(out_nchw), _lib.ptr(gts_u8), B, h, w, Hp, Wp, PAD, _lib.ptr(restored),
                                                         _lib.ptr(psnr_t), _lib.ptr(bad), _lib.ptr(ws), nws,
                                                         _lib.stream_handle()), "glare_harness_postprocess_flagged_f32")
    if want_nonfinite:
        return restored, psnr_t, bad
    return restored, psnr_t


def to_ubyte_device(restored):
    """restored float [..] in [0,1] (device) -> uint8 of the same shape: img_as_ubyte, the image the reference's loop saves."""
    _lib.require_cuda(restored)
    restored = restored.float().contiguous()
    out = torch.empty(restored.shape, dtype=torch.uint8, device=restored.device)
    _lib.check(_lib.main_lib().glare_harness_to_ubyte(_lib.ptr(restored), restored.numel(), _lib.ptr(out),
                                                      _lib.stream_handle()), "glare_harness_to_ubyte")
    return out


def ssim_device(restored, gts_u8):
    """SSIM as the reference's evaluation loop computes it (calculate_ssim(img_as_ubyte(target), img_as_ubyte(restored)),
    utils2.py:42-89 / infer_dataset_lol.py:152): restored float [B,h,w,3] in [0,1] and the uint8 ground truth, both on the device
    -> float64 [B] (device).  11x11 Gaussian (sigma 1.5) window at the valid positions, per channel, averaged."""
    from . import train_ops as T

    _lib.require_cuda(restored, gts_u8)
    assert restored.dtype == torch.float32 and gts_u8.dtype == torch.uint8 and restored.shape == gts_u8.shape
    restored, gts_u8 = restored.contiguous(), gts_u8.contiguous()
    B = restored.shape[0]
    x, y = torch.empty_like(restored), torch.empty_like(restored)
    _lib.check(_lib.lib().glare_harness_ubyte_planes_f32(_lib.ptr(restored), _lib.ptr(gts_u8), restored.numel(), _lib.ptr(x), _lib.ptr(y),
                                                         _lib.stream_handle()), "glare_harness_ubyte_planes_f32")
    g = np.exp(-((np.arange(11) - 5.0) ** 2) / (2 * 1.5 ** 2))
    g = (g / g.sum()).tolist()                                   # cv2.getGaussianKernel(11, 1.5)
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    vals = [T.ssim_forward(x[b:b + 1], y[b:b + 1], g, C1, C2)[1][0:1] for b in range(B)]   # mean ssim_map of one image
    return torch.cat(vals).double()


# ---- the checkpoint sweep's "adjust" protocol (code/test_stage2.py:169-180, code/test_stage3.py:183-185, :203-204) --------------
def _score_args(out_nchw, gts_u8, window):
    _lib.require_cuda(out_nchw, gts_u8)
    assert out_nchw.dtype == torch.float32 and out_nchw.dim() == 4 and out_nchw.shape[1] == 3 and out_nchw.is_contiguous()
    B, _, Hp, Wp = out_nchw.shape
    top, left, h, w = (0, 0, Hp, Wp) if window is None else window
    assert gts_u8.dtype == torch.uint8 and tuple(gts_u8.shape) == (B, h, w, 3) and gts_u8.is_contiguous()
    lib = _lib.main_lib()
    nws = lib.glare_harness_score_workspace_bytes(B)
    return lib, (B, Hp, Wp, top, left, h, w), torch.empty(max(nws, 1), dtype=torch.uint8, device=out_nchw.device), nws


def adjust_gain_device(out_nchw, gts_u8, window=None):
    """network output fp32 [B,3,Hp,Wp] and the uint8 ground truth [B,h,w,3] (device) -> fp32 [B] (device): mean_gt / mean_out of
    the window (top, left, h, w) (default: the whole tensor), mean_out over the RAW values (same arithmetic as adjust_gain())."""
    lib, (B, Hp, Wp, top, left, h, w), ws, nws = _score_args(out_nchw, gts_u8, window)
    gain = torch.empty(B, dtype=torch.float32, device=out_nchw.device)
    _lib.check(lib.glare_harness_adjust_gain_f32(_lib.ptr(out_nchw), _lib.ptr(gts_u8), B, Hp, Wp, top, left, h, w, _lib.ptr(gain), _lib.ptr(ws),
                                                 nws, _lib.stream_handle()), "glare_harness_adjust_gain_f32")
    return gain


def score_device(out_nchw, gts_u8, gain=None, window=None):
    """-> (uint8 [B,h,w,3] = rgb(out * gain) of the window, int64 [B] = sum (out_u8 - gt_u8)^2), both on the device; gain: fp32 [B]
    (adjust_gain_device) or None = 1.  PSNR: psnr_u8(sse, 3 h w) on the host."""
    lib, (B, Hp, Wp, top, left, h, w), ws, nws = _score_args(out_nchw, gts_u8, window)
    if gain is not None:
        _lib.require_cuda(gain)
        assert gain.dtype == torch.float32 and tuple(gain.shape) == (B,) and gain.is_contiguous()
    u8 = torch.empty(B, h, w, 3, dtype=torch.uint8, device=out_nchw.device)
    sse = torch.empty(B, dtype=torch.int64, device=out_nchw.device)
    _lib.check(lib.glare_harness_score_u8(_lib.ptr(out_nchw), _lib.ptr(gain), _lib.ptr(gts_u8), B, Hp, Wp, top, left, h, w, _lib.ptr(u8),
                                          _lib.ptr(sse), _lib.ptr(ws), nws, _lib.stream_handle()), "glare_harness_score_u8")
    return u8, sse


# ---- unpaired enhancement (code/infer_unpaired.py:81-136): any size, no GT, uint8 out --------------------------------
PAD_REFLECT101, PAD_SYMMETRIC = (_lib.constants()["GLARE_PAD_" + n] for n in ("REFLECT101", "SYMMETRIC"))     # include/glare_hip.h


def auto_padding(h, w, times=16):
    """(h1, h2, w1, w2) of auto_padding (infer_unpaired.py:81-88): up to the next multiple of `times`, split top / bottom and
    left / right with the odd pixel at the bottom / right -- a side that is already a multiple gets times/2 + times/2."""
    h1, w1 = (times - h % times) // 2, (times - w % times) // 2
    return h1, (times - h % times) - h1, w1, (times - w % times) - w1


def preprocess_unpaired_device(imgs_u8, pads=None, mode=PAD_SYMMETRIC):
    """uint8 device tensor [B,H,W,3] -> fp32 [B,3,Hp,Wp] in the log domain, padded by `pads` = (top, bottom, left, right)
    (default auto_padding) with cv2.BORDER_REFLECT (mode PAD_SYMMETRIC) or numpy 'reflect' (PAD_REFLECT101)."""
    _lib.require_cuda(imgs_u8)
    assert imgs_u8.dtype == torch.uint8 and imgs_u8.dim() == 4 and imgs_u8.shape[3] == 3 and imgs_u8.is_contiguous()
    B, H, W, _ = imgs_u8.shape
    t, b, l, r = auto_padding(H, W) if pads is None else pads
    out = torch.empty(B, 3, H + t + b, W + l + r, dtype=torch.float32, device=imgs_u8.device)
    _lib.check(_lib.main_lib().glare_harness_preprocess_pad_u8(_lib.ptr(imgs_u8), B, H, W, t, b, l, r, mode, _lib.ptr(out),
                                                               _lib.stream_handle()), "glare_harness_preprocess_pad_u8")
    return out


def postprocess_unpaired_device(out_nchw, pads, h, w, want_nonfinite=False):
    """network output [B,3,Hp,Wp] (device) -> uint8 [B,h,w,3] (device): the window at (pads[0], pads[2]), clamped and TRUNCATED to
    uint8 as rgb() does (infer_unpaired.py:42, :129-130).  want_nonfinite: also int32 [B], the inf / NaN values of each window
    before the clamp (the overflow flag of glare_amd.infer)."""
    _lib.require_cuda(out_nchw)
    out_nchw = out_nchw.float().contiguous()
    B, _, Hp, Wp = out_nchw.shape
    lib = _lib.main_lib()
    u8 = torch.empty(B, h, w, 3, dtype=torch.uint8, device=out_nchw.device)
    bad = ws = None
    nws = 0
    if want_nonfinite:
        nws = lib.glare_harness_postprocess_workspace_bytes(B)
        ws = torch.empty(nws, dtype=torch.uint8, device=out_nchw.device)
        bad = torch.empty(B, dtype=torch.int32, device=out_nchw.device)
    _lib.check(lib.glare_harness_postprocess_u8(_lib.ptr(out_nchw), B, Hp, Wp, pads[0], pads[2], h, w, _lib.ptr(u8), _lib.ptr(bad),
                                                _lib.ptr(ws), nws, _lib.stream_handle()),
               "glare_harness_postprocess_u8")
    return (u8, bad) if want_nonfinite else u8


# ---- tiled enhancement (glare_amd.enhance.enhance_tiled): overlapping windows of one image, feathered together --------------------
def tile_gather_device(img_u8, origins, th, tw, mode=PAD_SYMMETRIC):
    """uint8 device tensor [H,W,3] and int32 device tensor [n,2] of window origins (y0, x0; may be negative) -> fp32 [n,3,th,tw] in
    the log domain; coordinates outside the image fold as preprocess_unpaired_device pads, and the arithmetic is the same."""
    _lib.require_cuda(img_u8, origins)
    assert img_u8.dtype == torch.uint8 and img_u8.dim() == 3 and img_u8.shape[2] == 3 and img_u8.is_contiguous()
    assert origins.dtype == torch.int32 and origins.dim() == 2 and origins.shape[1] == 2 and origins.is_contiguous()
    H, W, _ = img_u8.shape
    n = origins.shape[0]
    out = torch.empty(n, 3, th, tw, dtype=torch.float32, device=img_u8.device)
    _lib.check(_lib.main_lib().glare_harness_tile_gather_u8(_lib.ptr(img_u8), H, W, _lib.ptr(origins), n, th, tw, mode, _lib.ptr(out),
                                                            _lib.stream_handle()), "glare_harness_tile_gather_u8")
    return out


def tile_blend_tables(plan, device):
    """The device-side tables of a tile plan (enhance.plan_tiles) as tile_blend_device takes them.  Checked here, on the host: every
    window an axis table names for a coordinate holds that coordinate, so the kernel reads inside the tile buffer."""
    tabs = []
    for starts, length, (first, count, weight), L in ((plan["ys"], plan["th"], plan["row_table"], plan["h"]),
                                                      (plan["xs"], plan["tw"], plan["col_table"], plan["w"])):
        s = np.asarray(starts, dtype=np.int64)
        first, count = np.asarray(first, dtype=np.int64), np.asarray(count, dtype=np.int64)
        assert first.shape == count.shape == (L,) and np.asarray(weight).shape == (L, 3)
        assert (count >= 1).all() and (count <= 3).all() and (first >= 0).all() and (first + count <= len(s)).all()
        x = np.arange(L)
        for a in range(3):
            sel = count > a
            lo = s[np.minimum(first + a, len(s) - 1)]
            assert ((x >= lo) & (x < lo + length))[sel].all(), "a blend table names a window that does not hold the coordinate"
        fc = np.ascontiguousarray(np.stack([first, count], axis=1).astype(np.int32))
        tabs.append((torch.from_numpy(s.astype(np.int32)).to(device), torch.from_numpy(fc).to(device),
                     torch.from_numpy(np.ascontiguousarray(weight, dtype=np.float32)).to(device)))
    return tabs


def tile_blend_device(tiles, plan, tables=None, want_f32=False):
    """network outputs fp32 [n_ty*n_tx,3,th,tw] (device) of the windows of `plan` -> (uint8 [h,w,3], fp32 [h,w,3] or None, int32 [1]),
    all on the device: the feathered blend of the clamped windows truncated to uint8 as rgb() does, the blended value before that
    (want_f32), and the number of raw inf / NaN window values inside the image."""
    _lib.require_cuda(tiles)
    n_ty, n_tx, th, tw, h, w = len(plan["ys"]), len(plan["xs"]), plan["th"], plan["tw"], plan["h"], plan["w"]
    assert tiles.dtype == torch.float32 and tuple(tiles.shape) == (n_ty * n_tx, 3, th, tw) and tiles.is_contiguous()
    (y0, rfc, rwt), (x0, cfc, cwt) = tables if tables is not None else tile_blend_tables(plan, tiles.device)
    lib = _lib.main_lib()
    nws = lib.glare_harness_tile_blend_workspace_bytes()
    ws = torch.empty(nws, dtype=torch.uint8, device=tiles.device)
    u8 = torch.empty(h, w, 3, dtype=torch.uint8, device=tiles.device)
    f32 = torch.empty(h, w, 3, dtype=torch.float32, device=tiles.device) if want_f32 else None
    bad = torch.empty(1, dtype=torch.int32, device=tiles.device)
    _lib.check(lib.glare_harness_tile_blend_f32(_lib.ptr(tiles), n_ty, n_tx, th, tw, _lib.ptr(y0), _lib.ptr(x0), h, w, _lib.ptr(rfc),
                                                _lib.ptr(rwt), _lib.ptr(cfc), _lib.ptr(cwt), _lib.ptr(u8), _lib.ptr(f32), _lib.ptr(bad),
                                                _lib.ptr(ws), nws, _lib.stream_handle()), "glare_harness_tile_blend_f32")
    return u8, f32, bad


def tile_gather(img_u8, origins, th, tw):
    """Host restatement of tile_gather_device (symmetric fold): uint8 [H,W,3] and (y0, x0) origins -> fp32 [n,3,th,tw], log domain."""
    H, W = img_u8.shape[:2]

    def fold(i, n):                                   # cv2.BORDER_REFLECT at any distance: period 2n
        p = np.mod(i, 2 * n)
        return np.where(p < n, p, 2 * n - 1 - p)

    wins = [img_u8[fold(y0 + np.arange(th), H)][:, fold(x0 + np.arange(tw), W)] for y0, x0 in origins]
    x = torch.from_numpy(np.ascontiguousarray(np.stack(wins).transpose(0, 3, 1, 2)).astype(np.float32)) / 255
    return torch.log(torch.clamp(x + 1e-3, min=1e-3))


def preprocess_unpaired(img_u8, pads=None):
    """Host restatement: uint8 [H,W,3] -> fp32 [1,3,Hp,Wp] in the log domain, auto_padding with numpy 'symmetric' (=
    cv2.BORDER_REFLECT), t() (:39) and log_low (:122)."""
    t, b, l, r = auto_padding(*img_u8.shape[:2]) if pads is None else pads
    img = np.pad(img_u8, [(t, b), (l, r), (0, 0)], "symmetric")
    x = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)[None]).astype(np.float32)) / 255
    return torch.log(torch.clamp(x + 1e-3, min=1e-3))


def rgb_u8(x):
    """Host restatement of rgb() (infer_unpaired.py:42): float array -> uint8 = (clip(x, 0, 1) * 255) in fp32, TRUNCATED; a NaN
    becomes 0 (fminf / fmaxf on the device; numpy's cast of a NaN is undefined)."""
    x = np.asarray(x, dtype=np.float32)
    x = np.where(np.isnan(x), np.float32(0), x)
    return (np.clip(x, np.float32(0), np.float32(1)) * np.float32(255)).astype(np.uint8)


def _window(out_nchw, window):
    out_nchw = np.asarray(out_nchw, dtype=np.float32)
    top, left, h, w = (0, 0) + out_nchw.shape[2:] if window is None else window
    return out_nchw[:, :, top:top + h, left:left + w]


def adjust_gain(out_nchw, gts_u8, window=None):
    """Host restatement of the test scripts' gain (test_stage2.py:169-171, test_stage3.py:183-185) in fp64: float array
    [B,3,Hp,Wp] and uint8 [B,h,w,3] -> fp32 [B] = mean_gt / mean_out.  mean_out is `lr_out.reshape(B, -1).mean(1)` of the window's
    RAW values (nothing is clamped first); mean_gt the gray mean of the ground truth / 255 with gray_mean()'s weights."""
    x = _window(out_nchw, window).astype(np.float64)
    g = np.asarray(gts_u8).astype(np.float64)
    mean_out = x.reshape(x.shape[0], -1).mean(axis=1)
    mean_gt = (0.114 * g[..., 0] + 0.587 * g[..., 1] + 0.299 * g[..., 2]).reshape(g.shape[0], -1).mean(axis=1) / 255
    with np.errstate(divide="ignore", invalid="ignore"):
        return (mean_gt / mean_out).astype(np.float32)


def score_u8(out_nchw, gts_u8, gain=None, window=None):
    """Host restatement of glare_harness_score_u8: -> (uint8 [B,h,w,3] = rgb_u8(out * gain) of the window, int64 [B] = the sum of
    squared differences to the uint8 ground truth).  The product is taken in fp32, as the device (and torch, on the fp32 output) does."""
    x = _window(out_nchw, window)
    if gain is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            x = x * np.asarray(gain, dtype=np.float32).reshape(-1, 1, 1, 1)
    u8 = np.ascontiguousarray(rgb_u8(x).transpose(0, 2, 3, 1))
    d = u8.astype(np.int64) - np.asarray(gts_u8).astype(np.int64)
    return u8, (d * d).reshape(d.shape[0], -1).sum(axis=1)


def psnr_u8(sse, n):
    """skimage.metrics.peak_signal_noise_ratio of two uint8 images (Measure.psnr, code/Measure.py:43-45) from their sum of squared
    differences over n values: 10 log10(255^2 / (sse / n)) in fp64, inf at sse = 0 (as it returns)."""
    sse = int(sse)
    return math.inf if sse == 0 else 10 * math.log10(255.0 ** 2 / (sse / n))


def preprocess(img_u8):
    """uint8 [H,W,3] -> fp32 [1,3,H+20,W+20] in the log domain."""
    img = np.pad(img_u8, [(0, PAD), (PAD, 0), (0, 0)], "reflect")
    t = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1)[None]).astype(np.float32)) / 255
    return torch.log(torch.clamp(t + 1e-3, min=1e-3))


def preprocess_batch(imgs_u8):
    return torch.cat([preprocess(im) for im in imgs_u8], dim=0)


def gray_mean(img):
    img = np.asarray(img, dtype=np.float32)
    return float((0.114 * img[..., 0] + 0.587 * img[..., 1] + 0.299 * img[..., 2]).mean())


def postprocess(out_nchw, h, gt_u8=None):
    """network output [1,3,H+20,W+20] -> float [H,W,3] in [0,1]; with gt: mean-gray gain first."""
    r = torch.clamp(out_nchw[:, :, :h, PAD:], 0, 1).detach().cpu().permute(0, 2, 3, 1).squeeze(0).numpy()
    if gt_u8 is not None:
        r = np.clip(r * (gray_mean(gt_u8 / 255) / gray_mean(r)), 0, 1)
    return r


def psnr(img1, img2):
    mse = float(np.mean((img1 - img2) ** 2))
    return 100.0 if mse == 0 else 10 * math.log10(1 / mse)
