"""GPU: unpaired enhancement of any-size images (glare_amd.enhance; code/infer_unpaired.py:81-136) -- the two harness kernels against
their host restatements, the full path against the fp32 oracle on unpaired-padded inputs, batch invariance, a 1080p image, the
largest 16:9 image the size envelope admits, the table of the envelope against every launch of a run, and the CLI."""
import json
import os

import numpy as np
import pytest
import torch

from glare_amd import enhance, harness, ops
from glare_amd.synthetic import synthetic_pair

pytestmark = pytest.mark.gpu

from test_gpu_precision import audit_flips, e2e_metrics, rel, setup  # noqa: E402
from tolerances import within  # noqa: E402


def _nets():
    og, ov, pg, pv, _, _ = setup("representative", 36, 28, 33)      # trained-like weights (shared with the other-sizes test)
    return og, ov, pg, pv


_PAD_CASES = [(21, 37, None), (5, 7, None), (5, 7, (9, 6, 13, 2)), (128, 192, None)]


@pytest.mark.parametrize("h,w,pads,mode", [c + (m,) for m in (harness.PAD_SYMMETRIC, harness.PAD_REFLECT101) for c in _PAD_CASES]
                         + [(1, 3, (4, 5, 6, 7), harness.PAD_SYMMETRIC)])      # a one-pixel side repeats (cv2's fold)
def test_pad_encode_kernel_equals_host(h, w, pads, mode):
    rng = np.random.default_rng(h * 1000 + w)
    imgs = rng.integers(0, 256, (3, h, w, 3), dtype=np.uint8)
    p = harness.auto_padding(h, w) if pads is None else pads
    got = harness.preprocess_unpaired_device(torch.from_numpy(imgs).cuda(), p, mode).cpu()
    for b in range(3):
        if mode == harness.PAD_SYMMETRIC:
            want = harness.preprocess_unpaired(imgs[b], p)
        else:
            padded = np.pad(imgs[b], [(p[0], p[1]), (p[2], p[3]), (0, 0)], "reflect")
            x = torch.from_numpy(np.ascontiguousarray(padded.transpose(2, 0, 1)[None]).astype(np.float32)) / 255
            want = torch.log(torch.clamp(x + 1e-3, min=1e-3))
        assert got[b:b + 1].shape == want.shape
        torch.testing.assert_close(got[b:b + 1], want, rtol=3e-7, atol=3e-7)     # one ulp of logf


@pytest.mark.parametrize("B,Hp,Wp,pads,h,w", [(3, 16, 16, (3, 4, 5, 2), 9, 9), (2, 32, 48, (8, 8, 8, 8), 16, 32), (5, 13, 11, (0, 0, 0, 0), 13, 11),
                                              (1, 16, 16, (7, 8, 7, 8), 1, 1)])
def test_postprocess_u8_is_rgb_of_the_crop_bit_for_bit(B, Hp, Wp, pads, h, w):
    g = torch.Generator().manual_seed(Hp * Wp + B)
    x = torch.rand(B, 3, Hp, Wp, generator=g, dtype=torch.float64).mul(1.4).sub(0.2).float()
    k = torch.randint(0, 256, x.shape, generator=g).float() / 255          # on k/255 and one ulp either side
    sel = torch.rand(x.shape, generator=g)
    x = torch.where(sel < 0.3, k, x)
    x = torch.where((sel >= 0.3) & (sel < 0.4), torch.nextafter(k, torch.tensor(2.0)), x)
    x = torch.where((sel >= 0.4) & (sel < 0.5), torch.nextafter(k, torch.tensor(-1.0)), x)
    flat = x.view(-1)
    spec = torch.randint(0, flat.numel(), (max(3, flat.numel() // 50),), generator=g)
    for j, i in enumerate(spec.tolist()):
        flat[i] = (float("nan"), float("inf"), float("-inf"))[j % 3]
    u8, bad = harness.postprocess_unpaired_device(x.cuda(), pads, h, w, want_nonfinite=True)
    crop = x[:, :, pads[0]:pads[0] + h, pads[2]:pads[2] + w].permute(0, 2, 3, 1).numpy()
    assert np.array_equal(u8.cpu().numpy(), harness.rgb_u8(crop))
    assert bad.cpu().tolist() == [int((~np.isfinite(crop[b])).sum()) for b in range(B)]
    assert np.array_equal(harness.postprocess_unpaired_device(x.cuda(), pads, h, w).cpu().numpy(), u8.cpu().numpy())


@pytest.mark.parametrize("h,w", [(201, 299), (128, 192)])
def test_end_to_end_unpaired_against_oracle(h, w, capsys):
    og, ov, pg, pv = _nets()
    img = synthetic_pair(1, h, w, seed=44)[0][0]
    pads = harness.auto_padding(h, w)
    lr = harness.preprocess_unpaired(img)
    threads = torch.get_num_threads()
    torch.set_num_threads(min(32, os.cpu_count() or 1))
    try:
        with torch.no_grad():
            ref = og.stages(ov, lr)
    finally:
        torch.set_num_threads(threads)
    lr_dev = harness.preprocess_unpaired_device(torch.from_numpy(img[None].copy()).cuda())
    torch.testing.assert_close(lr_dev.cpu(), lr, rtol=3e-7, atol=3e-7)
    with torch.no_grad():
        r = pg.reverse_flow_nhwc(pv, lr_dev)
    agree = float((r["indices"].cpu() == ref["indices"]).float().mean())
    lat = float(rel(ops.nhwc_to_nchw(r["latent"]).cpu(), ref["latent"]))
    flips, ratio = audit_flips(r, ref, ov)
    m = e2e_metrics(r["out"].cpu(), ref["out"], lr.shape[2])
    u8 = harness.postprocess_unpaired_device(r["out"], pads, h, w).cpu().numpy()[0]
    want = harness.rgb_u8(torch.clamp(ref["out"], 0, 1)[0, :, pads[0]:pads[0] + h, pads[2]:pads[2] + w].permute(1, 2, 0).numpy())
    mad = float(np.abs(u8.astype(np.int32) - want.astype(np.int32)).mean())
    with capsys.disabled():
        print("\n[unpaired %dx%d -> %dx%d] latent rel %.2e | %d flips of %d, worst ratio %.3f | PSNR(ours,oracle) %.2f dB | uint8 mean |diff| %.4f,"
              " max %d" % (h, w, lr.shape[2], lr.shape[3], lat, flips, ref["indices"].numel(), ratio, m["psnr_vs_oracle"], mad,
                           int(np.abs(u8.astype(int) - want.astype(int)).max())))
    assert u8.shape == img.shape
    within(lat, 5.5e-5)
    assert (1.0 - agree) * ref["indices"].numel() <= 6.5
    within(mad, 0.14)                  # measured 0.0669 / 0.0676 (max 2 LSB): truncation puts ~1 LSB on near-boundary values


def test_batch_of_4_equals_four_single_runs():
    _, _, pg, pv = _nets()
    imgs = list(synthetic_pair(4, 56, 90, seed=61)[0])
    ops.ATTENTION_KEY_SPLITS_OVERRIDE = 1          # B = 1 and B = 4 otherwise split the keys differently (summation order)
    try:
        four = enhance.enhance_images(imgs, pg, pv, batch=4)
        ones = [enhance.enhance_images([im], pg, pv, batch=1)[0] for im in imgs]
    finally:
        ops.ATTENTION_KEY_SPLITS_OVERRIDE = None
    for a, b, im in zip(four, ones, imgs):
        assert a.shape == im.shape and a.dtype == np.uint8
        assert np.array_equal(a, b)


def test_1080p_image_is_finite_and_repeatable():
    _, _, pg, pv = _nets()
    img = synthetic_pair(1, 1080, 1920, seed=71)[0][0]
    fn = enhance.device_enhance_fn(pg, pv, torch.device("cuda"))
    pads = harness.auto_padding(1080, 1920)
    a, bad = fn(img[None], pads, None)
    b, _ = fn(img[None], pads, None)
    assert a.shape == (1, 1080, 1920, 3) and int(bad[0]) == 0
    assert np.array_equal(a, b)


def _probe_extents(monkeypatch):
    """Wraps the ops whose C entry points carry the checks of enhance.SIZE_TABLE: -> list of (row name, B, extent) of a run."""
    seen = []
    conv2d, grouped, d512, kv512 = ops.conv2d, ops.conv2d_grouped, ops.attention_d512, ops.attention_kv512
    dcn, dcn_fused = ops.mdcn_forward_nhwc, ops.mdcn_forward_nhwc_fused

    def conv_src(x, B):
        seen.append(("conv source, one image", 1, x.shape[1] * x.shape[2] * x.shape[3] * 2))

    def w_conv2d(x, pc, **kw):
        conv_src(x, x.shape[0])
        if kw.get("x2") is not None:
            conv_src(kw["x2"], x.shape[0])
        return conv2d(x, pc, **kw)

    def w_grouped(x, pcs, **kw):
        conv_src(x, x.shape[0])
        return grouped(x, pcs, **kw)

    def w_d512(q, k, v_t, N, ldq=None, ldk=None, *a, **kw):
        seen.append(("attention K, one image", 1, (N * (ldk or k.shape[-1]) + 512) * 2))
        seen.append(("attention V^T, one image", 1, 512 * v_t.shape[2] * 2))
        return d512(q, k, v_t, N, ldq, ldk, *a, **kw)

    def w_kv512(q, kv, N, ldq=None, ldkv=None, *a, **kw):
        seen.append(("attention K/V (shared), one image", 1, (N * (ldkv or kv.shape[-1]) + 512) * 2))
        return kv512(q, kv, N, ldq, ldkv, *a, **kw)

    def dcn_rows(x, om, pd):
        B, planes, plane = x.shape[0], om.shape[1], om.shape[2]
        K = pd.kh * pd.kw
        seen.append(("DCN x, whole batch", B, x.numel() * 2))
        seen.append(("DCN offsets, whole batch", B, ((B - 1) * planes * plane + 2 * pd.dg * K * plane) * 4))
        seen.append(("DCN mask, whole batch", B, ((B - 1) * planes * plane + pd.dg * K * plane) * 4))

    def w_dcn(x, om, pd, *a, **kw):
        dcn_rows(x, om, pd)
        return dcn(x, om, pd, *a, **kw)

    def w_dcn_fused(x, om, pd, *a, **kw):
        dcn_rows(x, om, pd)
        return dcn_fused(x, om, pd, *a, **kw)

    for name, f in (("conv2d", w_conv2d), ("conv2d_grouped", w_grouped), ("attention_d512", w_d512), ("attention_kv512", w_kv512),
                    ("mdcn_forward_nhwc", w_dcn), ("mdcn_forward_nhwc_fused", w_dcn_fused)):
        monkeypatch.setattr(ops, name, f)
    return seen


def test_size_table_bounds_every_launch(monkeypatch, capsys):
    """Every extent of the table's rows, as the launches of a real run (B = 1 and B = 2) compute it, is within the table's figure:
    the table is complete for the graph (and the envelope test below shows it is not too loose)."""
    _, _, pg, pv = _nets()
    rows = {r[0]: r for r in enhance.SIZE_TABLE}
    worst = {}
    for B in (1, 2):
        seen = _probe_extents(monkeypatch)
        imgs = list(synthetic_pair(B, 72, 104, seed=81)[0])
        enhance.enhance_images(imgs, pg, pv, batch=B)
        monkeypatch.undo()
        hp, wp = 80, 112
        kinds = set()
        for name, b, e in seen:
            kinds.add(name)
            bound = enhance._extent(rows[name], hp, wp, b)
            assert e <= bound, (name, b, e, bound)
            worst[(name, b)] = max(worst.get((name, b), 0), e / (hp * wp))
        assert {"conv source, one image", "DCN x, whole batch", "DCN offsets, whole batch"} <= kinds <= set(rows), kinds
    with capsys.disabled():
        print("\n[size table, bytes per padded pixel as launched at 80x112] " +
              "; ".join("%s B=%d: %.1f" % (n, b, v) for (n, b), v in sorted(worst.items())))


def test_largest_16_9_image_of_the_envelope_runs():
    _, _, pg, pv = _nets()
    hp = 16
    while True:
        wn = (hp + 16) * 16 // 9 // 16 * 16
        try:
            enhance.check_size(hp + 16, wn)
        except ValueError:
            break
        hp += 16
    wp = hp * 16 // 9 // 16 * 16
    enhance.check_size(hp, wp)
    h, w = hp - 16, wp - 16                            # multiples of 16: auto_padding adds 8 + 8
    img = synthetic_pair(1, h, w, seed=91)[0][0]
    fn = enhance.device_enhance_fn(pg, pv, torch.device("cuda"))
    out, bad = fn(img[None], harness.auto_padding(h, w), None)
    print("envelope image %dx%d (padded %dx%d = %.2f MP)" % (h, w, hp, wp, hp * wp / 1e6))
    assert out.shape == (1, h, w, 3) and int(bad[0]) == 0


def test_cli_on_a_folder_of_mixed_sizes(tmp_path, capsys):
    from PIL import Image

    src, out = tmp_path / "photos", tmp_path / "out"
    src.mkdir()
    sizes = {"b2.png": (40, 60), "b10.jpg": (33, 47), "a.png": (64, 64)}
    for i, (n, (h, w)) in enumerate(sizes.items()):
        Image.fromarray(synthetic_pair(1, h, w, seed=100 + i)[0][0]).save(src / n)
    res = enhance.main([str(src), "--out", str(out), "--batch", "4"])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert [r["name"] for r in line["images"]] == ["a.png", "b2.png", "b10.jpg"] == [r["name"] for r in res["images"]]
    assert line["skipped"] == [] and line["bf16_rerun_images"] == [] and line["images_per_sec"] > 0
    for n, (h, w) in sizes.items():
        assert np.asarray(Image.open(out / n)).shape == (h, w, 3)
