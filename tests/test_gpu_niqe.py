"""GPU: the whole NIQE score (glare_amd.metrics.niqe) with the synthetic pristine model against the fp64 restatement
(tests/niqe_fp64.py), and `enhance.run(..., niqe=...)` on the device.

The bar for |gpu - fp64| is not chosen: it is the largest deviation, over the images below, of the restatement run with the published
implementation's float32 storage (niqe_fp64.niqe(storage=np.float32): the second scale's image, mu, window (*) y^2, their squares, sigma
and n as float32 arrays) from the fp64 restatement -- that implementation's own noise, with no margin on top.  The kernels' variance
about the centre pixel and their fp64 sums should sit well inside it."""
import numpy as np
import pytest
import torch

import niqe_fp64 as N
from glare_amd import enhance, metrics
from glare_amd.synthetic import synthetic_pair

pytestmark = pytest.mark.gpu

PARAMS = N.synthetic_params()


def _images():
    """name -> uint8 [h, w, 3]: six seeded 192 x 288 images (three low-light, three normal-light), one 200 x 300 for the crop, one with a
    constant quarter -- the first block and the 16 pixels around it that its filters reach, so that n is 0 all over it at both scales:
    a block without features, and a neighbour that is mostly flat -- and a batch of two."""
    imgs = {}
    for k in range(3):
        low, normal = synthetic_pair(1, 192, 288, seed=300 + k)
        imgs["low%d" % k], imgs["normal%d" % k] = low[0], normal[0]
    imgs["crop 200x300"] = synthetic_pair(1, 200, 300, seed=310)[1][0]
    flat = synthetic_pair(1, 192, 288, seed=311)[1][0].copy()
    flat[:112, :160] = (90, 120, 60)
    imgs["constant quarter"] = flat
    pair = synthetic_pair(2, 96, 192, seed=312)[1]
    imgs["batch[0]"], imgs["batch[1]"] = pair[0], pair[1]
    return imgs


@pytest.fixture(scope="module")
def reference():
    """(images, fp64 scores, the bar), computed once."""
    imgs = _images()
    exact = {k: N.niqe(v, PARAMS) for k, v in imgs.items()}
    stored = {k: N.niqe(v, PARAMS, storage=np.float32) for k, v in imgs.items()}
    assert all(v is not None and np.isfinite(v) for v in exact.values())
    dev = {k: abs(stored[k] - exact[k]) for k in imgs}
    bar = max(dev.values())
    print("\nNIQE fp64 scores: " + ", ".join("%s %.6f" % kv for kv in exact.items()))
    print("float32-storage deviation: " + ", ".join("%s %.3g" % kv for kv in dev.items()) + " -> bar %.3g" % bar)
    return imgs, exact, bar


def test_scores_are_within_the_published_implementations_own_noise(reference):
    imgs, exact, bar = reference
    singles = [k for k in imgs if not k.startswith("batch")]
    got = dict(zip(singles, metrics.niqe([imgs[k] for k in singles], PARAMS)))                  # a list of mixed sizes, host arrays
    batch = metrics.niqe(torch.from_numpy(np.stack([imgs["batch[0]"], imgs["batch[1]"]])).cuda(), PARAMS)      # a device tensor [2,h,w,3]
    got.update({"batch[0]": batch[0], "batch[1]": batch[1]})
    worst = 0.0
    for k in imgs:
        assert isinstance(got[k], float), k
        err = abs(got[k] - exact[k])
        worst = max(worst, err)
        print("NIQE %-18s gpu %.9f fp64 %.9f |diff| %.3g (bar %.3g)" % (k, got[k], exact[k], err, bar))
    print("NIQE worst |gpu - fp64| %.3g, bar %.3g, ratio %.3f" % (worst, bar, worst / bar))
    assert worst <= bar


def test_nan_rows_are_left_out_as_the_restatement_leaves_them(reference):
    imgs, exact, _ = reference
    f = N.features(imgs["constant quarter"], PARAMS)
    nan_rows = np.isnan(f).any(axis=1)
    assert f.shape == (6, 36) and nan_rows.tolist() == [True] + [False] * 5           # column-major: the first block
    m1, m2 = metrics.niqe_moments_device(torch.from_numpy(imgs["constant quarter"][None]).cuda(), PARAMS["gaussian_window"])
    f1, _ = metrics.niqe_features(m1[0], 96 * 96)
    f2, _ = metrics.niqe_features(m2[0], 48 * 48)
    assert np.array_equal(np.isnan(np.concatenate([f1, f2], axis=1)).any(axis=1), nan_rows)


def test_an_image_with_fewer_than_two_blocks_has_no_score():
    small = synthetic_pair(1, 100, 150, seed=320)[1][0]
    assert metrics.niqe([small], PARAMS) == [None]
    (score, why), = metrics.niqe_scores([small], PARAMS)
    assert score is None and "fewer than 2 whole" in why
    mixed = metrics.niqe([small, synthetic_pair(1, 96, 192, seed=321)[1][0]], PARAMS)
    assert mixed[0] is None and isinstance(mixed[1], float)


def test_two_runs_give_identical_bits(reference):
    imgs, _, _ = reference
    batch = [imgs[k] for k in imgs]
    assert metrics.niqe(batch, PARAMS) == metrics.niqe(batch, PARAMS)


def test_enhance_run_scores_inputs_and_outputs(tmp_path):
    """Two small images through the name-seeded networks, as the CLI test of test_gpu_enhance.py sets them up: finite scores of the input
    and of the enhanced image, and the enhanced files byte-equal to a run without the flag."""
    from PIL import Image

    src = tmp_path / "photos"
    src.mkdir()
    for i, (name, (h, w)) in enumerate({"a.png": (96, 192), "b.png": (100, 200)}.items()):
        Image.fromarray(synthetic_pair(1, h, w, seed=330 + i)[0][0]).save(src / name)
    device = torch.device("cuda", torch.cuda.current_device())
    netG, net_vq = enhance.load_nets(device=device)
    plain = enhance.run([str(src)], str(tmp_path / "plain"), netG, net_vq, device=device)
    scored = enhance.run([str(src)], str(tmp_path / "scored"), netG, net_vq, device=device, niqe=metrics._niqe_params(PARAMS, "synthetic"))
    assert "niqe_mean" not in plain and all("niqe" not in e for e in plain["images"])
    for e in scored["images"]:
        assert np.isfinite(e["niqe"]) and np.isfinite(e["niqe_in"]) and "niqe_reason" not in e
        assert (tmp_path / "plain" / e["name"]).read_bytes() == (tmp_path / "scored" / e["name"]).read_bytes()
        out = np.asarray(Image.open(tmp_path / "scored" / e["name"]))
        assert e["niqe"] == metrics.niqe([out], PARAMS)[0]                              # NIQE sees the image that was written
    assert scored["niqe_mean"] == pytest.approx(np.mean([e["niqe"] for e in scored["images"]]))
    assert scored["niqe_in_mean"] == pytest.approx(np.mean([e["niqe_in"] for e in scored["images"]]))
    assert scored["niqe_seconds"] > 0


def test_metrics_cli_scores_a_folder_in_natural_order(tmp_path, capsys):
    import json

    from PIL import Image

    src = tmp_path / "other_method"
    src.mkdir()
    imgs = {"img10.png": synthetic_pair(1, 96, 192, seed=340)[1][0], "img2.png": synthetic_pair(1, 192, 96, seed=341)[1][0],
            "tiny.png": synthetic_pair(1, 40, 60, seed=342)[1][0]}
    for name, im in imgs.items():
        Image.fromarray(im).save(src / name)
    (src / "notes.txt").write_text("not an image")
    np.savez(tmp_path / "params.npz", **PARAMS)
    res = metrics.main(["niqe", str(src), "--params", str(tmp_path / "params.npz")])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == json.loads(json.dumps(res))
    assert [e["name"] for e in line["images"]] == ["img2.png", "img10.png", "tiny.png"] and [s["name"] for s in line["skipped"]] == ["notes.txt"]
    want = metrics.niqe([imgs["img2.png"], imgs["img10.png"]], PARAMS)
    assert [e["niqe"] for e in line["images"]] == want + [None] and "fewer than 2 whole" in line["images"][2]["niqe_reason"]
    assert line["scored"] == 2 and line["niqe_mean"] == pytest.approx(np.mean(want)) and line["niqe_seconds"] > 0
