"""CPU: the unpaired harness around the network (glare_amd.enhance, glare_amd.harness): auto_padding, the symmetric pad, rgb()'s
truncation, the size envelope and the folder driver with a stub network call (code/infer_unpaired.py:39-136)."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

from glare_amd import enhance, harness


def ref_auto_padding(h, w, times=16):       # infer_unpaired.py:81-88, the arithmetic as written
    h1, w1 = (times - h % times) // 2, (times - w % times) // 2
    h2, w2 = (times - h % times) - h1, (times - w % times) - w1
    return [h1, h2, w1, w2]


@pytest.mark.parametrize("h", list(range(1, 71)) + [400, 600, 1080, 1920])
def test_auto_padding_matches_the_reference_formula(h):
    for w in list(range(1, 71)) + [400, 600, 1080, 1920]:
        p = harness.auto_padding(h, w)
        assert list(p) == ref_auto_padding(h, w)
        assert (h + p[0] + p[1]) % 16 == 0 and (w + p[2] + p[3]) % 16 == 0
    if h % 16 == 0:
        assert harness.auto_padding(h, 32)[:2] == (8, 8)      # a side already a multiple of 16 still gets 8 + 8


def border_reflect(i, n):
    """cv2.borderInterpolate(i, n, BORDER_REFLECT), as OpenCV documents it: fedcba|abcdefgh|hgfedcb, any distance."""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i - 1 if i < 0 else 2 * n - i - 1
    return i


@pytest.mark.parametrize("h,w", [(5, 7), (1, 3), (2, 2), (21, 37), (16, 32), (3, 1)])
def test_symmetric_pad_is_cv2_border_reflect(h, w):
    rng = np.random.default_rng(h * 100 + w)
    img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for pads in (harness.auto_padding(h, w), (9, 13, 11, 6)):      # incl. pads longer than the image
        t, b, l, r = pads
        want = np.empty((h + t + b, w + l + r, 3), np.uint8)
        for y in range(h + t + b):
            for x in range(w + l + r):
                want[y, x] = img[border_reflect(y - t, h), border_reflect(x - l, w)]
        got = np.pad(img, [(t, b), (l, r), (0, 0)], "symmetric")
        assert np.array_equal(got, want), pads
        enc = harness.preprocess_unpaired(img, pads)
        assert enc.shape == (1, 3, h + t + b, w + l + r)
        ref = torch.log(torch.clamp(torch.from_numpy(want.transpose(2, 0, 1)[None].astype(np.float32)) / 255 + 1e-3, min=1e-3))
        assert torch.equal(enc, ref)


def test_rgb_u8_truncates():
    f = np.float32
    k = np.arange(256, dtype=np.float32) / f(255)
    below = np.nextafter(k, f(-1))
    x = np.array([0.999, 1.0, -0.5, 1.5, 0.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    assert harness.rgb_u8(x).tolist() == [254, 255, 0, 255, 0, 255, 0, 0]
    want = (np.clip(k, 0, 1) * f(255)).astype(np.uint8)                   # rgb() of infer_unpaired.py:42, fp32
    assert np.array_equal(harness.rgb_u8(k), want)
    assert np.array_equal(harness.rgb_u8(below), (np.clip(below, 0, 1) * f(255)).astype(np.uint8))
    assert (harness.rgb_u8(below)[1:].astype(int) <= np.arange(1, 256)).all()   # never rounds up
    assert harness.rgb_u8(np.float32(0.5)) == 127                           # img_as_ubyte would give 128


def test_size_envelope():
    p = harness.auto_padding(1080, 1920)
    enhance.check_size(1080 + p[0] + p[1], 1920 + p[2] + p[3])              # 1088 x 1936
    p = harness.auto_padding(1440, 2560)
    enhance.check_size(1440 + p[0] + p[1], 2560 + p[2] + p[3])
    with pytest.raises(ValueError) as ei:
        enhance.check_size(2176, 3856, name="uhd.png")                     # 4K UHD, padded
    msg = str(ei.value)
    assert "uhd.png" in msg and "2176x3856" in msg and "conv_igemm.hip" in msg and "limit" in msg
    # the largest single image: every row of the table below its limit, the binding row one pixel row further
    hp = 16
    while True:
        try:
            enhance.check_size(hp + 16, (hp + 16) * 16 // 9 // 16 * 16)
        except ValueError:
            break
        hp += 16
    assert 1088 <= hp and hp * (hp * 16 // 9 // 16 * 16) < 0x7ff00000 // 512
    # batches: LOL (400 x 600 -> 416 x 608) runs batches of 8; the DCN's whole-batch extents cap them
    assert enhance.max_batch(416, 608) >= 8
    assert enhance.max_batch(1088, 1936) >= 1
    b = enhance.max_batch(416, 608)
    enhance.check_size(416, 608, b)
    with pytest.raises(ValueError, match="DCN"):
        enhance.check_size(416, 608, b + 1)


def test_natural_order():
    files = ["img10.png", "img2.png", "img1.png", "a.png", "img2b.png"]
    assert sorted(files, key=enhance.natural_key) == ["a.png", "img1.png", "img2.png", "img2b.png", "img10.png"]


def _stub(calls):
    """A stand-in network: the 'enhanced' image is 255 - input, through the real harness arithmetic on the host."""
    def fn(batch_u8, pads, precision):
        a = np.asarray(batch_u8)
        calls.append((a.shape, tuple(pads), precision))
        return 255 - a, np.zeros(a.shape[0], np.int32)
    return fn


def test_driver_on_a_folder(tmp_path):
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (20, 30, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(src / "img10.png")
    Image.fromarray(rgb).save(src / "img2.png")
    Image.fromarray(rgb[:, :, 0]).save(src / "gray.png")                      # L
    Image.fromarray(rgb[:, :, 0]).convert("LA").save(src / "gray_alpha.png")  # LA
    rgba = np.concatenate([rgb, np.full((20, 30, 1), 7, np.uint8)], axis=2)
    Image.fromarray(rgba).save(src / "rgba.png")                              # RGBA
    tall = rng.integers(0, 256, (17, 9, 3), dtype=np.uint8)
    ex = Image.fromarray(tall).getexif()
    ex[0x0112] = 6                                                            # orientation: rotate 90 CW to display
    Image.fromarray(tall).save(src / "rotated.jpg", exif=ex, quality=100)
    (src / "notes.txt").write_text("not an image")
    Image.fromarray((rng.integers(0, 65535, (8, 8))).astype(np.uint16)).save(src / "deep.png")   # 16-bit gray

    calls = []
    res = enhance.run([str(src)], str(out), enhance_fn=_stub(calls))
    json.dumps(res)
    names = [r["name"] for r in res["images"]]
    assert names == ["gray.png", "gray_alpha.png", "img2.png", "img10.png", "rgba.png", "rotated.jpg"]
    skipped = {s["name"]: s["reason"] for s in res["skipped"]}
    assert set(skipped) == {"notes.txt", "deep.png"} and "mode" in skipped["deep.png"]
    sizes = {r["name"]: tuple(r["size"]) for r in res["images"]}
    assert sizes["rotated.jpg"] == (9, 17)                                   # EXIF orientation applied
    assert all(sizes[n] == (20, 30) for n in names if n != "rotated.jpg")
    assert {tuple(r["padded"]) for r in res["images"]} == {(32, 32), (16, 32)}
    # images of one size run as one batch, the others on their own
    assert sorted(c[0] for c in calls) == [(1, 9, 17, 3), (5, 20, 30, 3)]
    assert (5, 20, 30, 3) in [c[0] for c in calls] and all(c[1] == harness.auto_padding(*c[0][1:3]) for c in calls)
    for n in names:
        o = np.asarray(Image.open(out / n))
        assert o.shape == sizes[n] + (3,)
    assert np.array_equal(np.asarray(Image.open(out / "img2.png")), 255 - rgb)
    assert np.array_equal(np.asarray(Image.open(out / "gray.png")), 255 - np.repeat(rgb[:, :, :1], 3, axis=2))
    assert np.array_equal(np.asarray(Image.open(out / "rgba.png")), 255 - rgb)    # alpha dropped
    assert res["bf16_rerun_images"] == [] and res["seconds"] >= 0
    assert set(os.listdir(out)) == set(names)


def test_driver_reruns_nonfinite_images_in_bf16():
    imgs = [np.full((10, 12, 3), v, np.uint8) for v in (1, 2, 3)]
    calls = []

    def fn(batch_u8, pads, precision):
        a = np.asarray(batch_u8)
        calls.append((a.shape[0], precision))
        bad = np.array([int(im[0, 0, 0] == 2 and precision != "bf16") for im in a], np.int32)
        return a + (10 if precision == "bf16" else 0), bad

    rep = {}
    outs = enhance.enhance_images(imgs, enhance_fn=fn, names=["a", "b", "c"], report=rep)
    assert rep["bf16_rerun_images"] == ["b"] and calls == [(3, None), (1, "bf16")]
    assert [int(o[0, 0, 0]) for o in outs] == [1, 12, 3]


def test_envelope_is_enforced_before_any_launch():
    calls = []
    with pytest.raises(ValueError, match="big.png"):
        enhance.enhance_images([np.zeros((10, 10, 3), np.uint8), np.zeros((2200, 3900, 3), np.uint8)], enhance_fn=_stub(calls),
                               names=["ok.png", "big.png"])
    assert calls == []
