"""CPU: NIQE's host side.  The fp64 restatement (tests/niqe_fp64.py) against the reference's own colour conversion and MATLAB
bicubic resize, executed in place (basicsr/utils/matlab_functions.py; skipped where the reference tree is absent); the product's
moments -> features -> score against the restatement on identical moments; the loader's and the C entries' refusals; and the
`--niqe` plumbing of glare_amd.enhance through a stub network and a stub scorer."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest

import niqe_fp64 as N
from glare_amd import _lib, enhance, metrics
from oracle import refimport

MATLAB = os.path.join(refimport.REF_ROOT, "defor_cuda_ext", "basicsr", "utils", "matlab_functions.py")
needs_reference = pytest.mark.skipif(not os.path.isfile(MATLAB), reason="the reference tree is not present")
U = 2.0 ** -24


def _matlab():
    spec = importlib.util.spec_from_file_location("ref_matlab_functions", MATLAB)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@needs_reference
@pytest.mark.parametrize("h,w", [(8, 10), (96, 192), (192, 288)])
def test_half_size_filter_is_the_reference_imresize(h, w):
    """The reference holds the image and both passes in float32; with taps that are exact in float32 and sum |tap| = 304 / 256:
    the input cast costs U, a pass of 8 products and 7 additions at most 8 U sum |tap v|, and the second pass carries the first one's
    error through sum |tap|.  On values <= 1 that is e1 = (1 + 8) T U after the H pass and e2 = T e1 + 8 T^2 U after the W pass,
    T = 1.1875: 24 U, times 255 on the 0..255 scale."""
    y = np.random.default_rng(h * w).integers(16, 236, (h, w)).astype(np.float64)
    ref = _matlab().imresize(y / 255.0, 0.5, antialiasing=True).astype(np.float64) * 255.0
    got = N.halve(y / 255.0) * 255.0
    T = float(np.abs(N.TAPS).sum())
    bound = 255.0 * (T * (9 * T * U) + 8 * T * T * U)
    err = float(np.abs(got - ref).max())
    print("halve %dx%d: max |restatement - imresize| %.3g, bound %.3g" % (h, w, err, bound))
    assert got.shape == ref.shape == (h // 2, w // 2)
    assert err <= bound


@needs_reference
def test_taps_and_indices_are_what_calculate_weights_indices_returns():
    weights, indices, s, e = _matlab().calculate_weights_indices(192, 96, 0.5, "cubic", 4, True)
    assert (s, e) == (3, 3) and tuple(weights.shape) == (96, 8)
    assert np.array_equal(weights.numpy().astype(np.float64), np.tile(N.TAPS, (96, 1)))
    # indices address the image extended by s reflected pixels in front: output j reads inputs 2 j - 3 .. 2 j + 4
    assert np.array_equal(indices.numpy().astype(np.int64) - s, 2 * np.arange(96)[:, None] - 3 + np.arange(8)[None, :])


@needs_reference
def test_luma_over_all_colours_against_rgb2ycbcr():
    """rgb2ycbcr(img / 255, y_only=True) * 255 and round(), as the published calculate_niqe takes its luma, in float32; the integer rule
    may differ from it only where the exact value lies within 1e-4 of a half-integer (|remainder - 127500| <= 25 of 255000)."""
    rgb2ycbcr = _matlab().rgb2ycbcr
    g = np.arange(256, dtype=np.uint8)
    differ = near = 0
    for r in range(0, 256, 16):
        c = np.stack(np.meshgrid(g[r:r + 16], g, g, indexing="ij"), axis=-1).reshape(-1, 3)
        ref = (rgb2ycbcr(c.astype(np.float32) / np.float32(255.0), y_only=True) * 255.0).round().astype(np.int64)
        rem = N.luma_numerator(c) % 255000
        close = np.abs(rem - 127500) <= 25
        bad = N.luma(c) != ref
        assert not (bad & ~close).any()
        differ += int(bad.sum())
        near += int(close.sum())
    print("luma: %d of 2^24 colours differ from the reference's float32 path, %d lie within 1e-4 of a half-integer" % (differ, near))
    assert differ <= near <= 3330


def test_luma_rounds_ties_to_even():
    g = np.arange(256)
    c = np.stack(np.meshgrid(g, g, [0, 85, 170, 255], indexing="ij"), axis=-1).reshape(-1, 3)
    rem = N.luma_numerator(c) % 255000
    tie = c[rem == 127500]
    assert tie.shape[0] > 0
    y = N.luma(tie)
    assert (y % 2 == 0).all()                                  # half to even
    exact = 16 + N.luma_numerator(tie) / 255000.0
    assert np.array_equal(np.abs(y - exact), np.full(tie.shape[0], 0.5))


def _moment_sets(rng):
    """Moments of blocks of n with different tails, computed by the restatement: [n_blocks, 5, 5] for 96- and 48-blocks."""
    base = rng.standard_normal((192, 288))
    n = np.sign(base) * np.abs(base) ** np.repeat(np.repeat(np.array([[0.6, 1.0, 1.7], [2.4, 1.0, 0.8]]), 96, 0), 96, 1)
    return N.block_moments(n).reshape(-1, 5, 5), N.block_moments(n[::2, ::2], 48, 48).reshape(-1, 5, 5), n


def test_host_part_equals_the_restatement_on_identical_moments():
    params = N.synthetic_params()
    m1, m2, n = _moment_sets(np.random.default_rng(11))
    for m, count in ((m1, 96 * 96), (m2, 48 * 48)):
        want, kw = N.features_from_moments(m, count)
        got, kg = metrics.niqe_features(m, count)
        assert np.array_equal(kg, kw) and len(set(kw[:, 0].tolist())) > 2              # the same grid index, and not one index
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    want, _ = N.score_from_features(np.concatenate([N.features_from_moments(m1, 9216)[0], N.features_from_moments(m2, 2304)[0]], 1), params)
    got, why = metrics.niqe_from_moments(m1, m2, metrics._niqe_params(params, "synthetic"))
    assert why is None and got == pytest.approx(want, rel=1e-10)
    # the moments are those of the blocks: the features of a block computed directly agree with the route through the moments
    direct = [N.aggd(N.map_moments(v), 9216) for v in N.block_maps(n[:96, :96])]
    assert [d[3] for d in direct] == metrics.niqe_features(m1, 9216)[1][0].tolist()


def test_empty_sides_give_nan_rows_and_too_few_rows_give_no_score():
    params = metrics._niqe_params(N.synthetic_params(), "synthetic")
    rng = np.random.default_rng(12)
    m1, m2, _ = _moment_sets(rng)
    pos = np.abs(rng.standard_normal((96, 96))) + 0.1                     # no negative value: map 0 has an empty left side
    mp = N.block_moments(pos).reshape(5, 5)
    assert mp[0, 0] == 0 and mp[0, 1] == 9216
    m1 = m1.copy()
    m1[2] = mp
    m1[4] = 0.0                                                           # a constant block: n = 0, both sides empty
    got, kg = metrics.niqe_features(m1, 9216)
    want, kw = N.features_from_moments(m1, 9216)
    assert np.array_equal(kg, kw) and np.array_equal(np.isnan(got), np.isnan(want))
    assert np.isnan(got[2]).any() and np.isnan(got[4]).any() and not np.isnan(got[[0, 1, 3, 5]]).any()
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=0)
    s_want, _ = N.score_from_features(np.concatenate([want, N.features_from_moments(m2, 2304)[0]], 1), params)
    s_got, why = metrics.niqe_from_moments(m1, m2, params)
    assert why is None and s_got == pytest.approx(s_want, rel=1e-10)      # nanmean over 6 rows, covariance over 4
    m1[[0, 1, 3]] = 0.0                                                   # one row without NaN is left
    s_got, why = metrics.niqe_from_moments(m1, m2, params)
    assert s_got is None and "fewer than 2 blocks" in why
    assert N.score_from_features(np.concatenate([N.features_from_moments(m1, 9216)[0], N.features_from_moments(m2, 2304)[0]], 1), params)[0] is None
    assert metrics.niqe_mean([None, 2.0, 4.0]) == 3.0 and metrics.niqe_mean([None]) is None


def test_grid_index_is_the_argmin_with_the_first_on_ties():
    g, rho, _ = metrics._niqe_table()
    assert g.size == 9801 and g[0] == 0.2 and abs(g[-1] - 10.0) < 1e-12
    np.testing.assert_allclose(rho, N.RHO, rtol=1e-13)
    R = np.concatenate([[-1.0, 0.0, rho[0], rho[-1], 5.0, np.nan, np.inf], (rho[:-1] + rho[1:]) / 2, rho[::97] * (1 + 1e-9),
                        np.random.default_rng(3).uniform(0.0, 1.0, 500)])
    with np.errstate(invalid="ignore"):
        want = np.array([int(np.argmin((rho - r) ** 2)) for r in R])
    assert np.array_equal(metrics.niqe_grid_index(R), want)


def test_loader_refuses_by_name(tmp_path):
    p = N.synthetic_params()
    np.savez(tmp_path / "ok.npz", **p)
    got = metrics.load_niqe_params(tmp_path / "ok.npz")
    assert got["mu_pris_param"].shape == (36,) and got["cov_pris_param"].shape == (36, 36) and got["gaussian_window"].shape == (7, 7)
    np.savez(tmp_path / "row.npz", **dict(p, mu_pris_param=p["mu_pris_param"][None]))
    assert np.array_equal(metrics.load_niqe_params(tmp_path / "row.npz")["mu_pris_param"], p["mu_pris_param"])
    for key in p:
        np.savez(tmp_path / "missing.npz", **{k: v for k, v in p.items() if k != key})
        with pytest.raises(ValueError, match=key):
            metrics.load_niqe_params(tmp_path / "missing.npz")
    for key, bad in (("mu_pris_param", np.zeros(35)), ("mu_pris_param", np.zeros((36, 1))), ("cov_pris_param", np.zeros((36, 35))),
                     ("gaussian_window", np.zeros((5, 5))), ("gaussian_window", np.full((7, 7), np.nan))):
        np.savez(tmp_path / "bad.npz", **dict(p, **{key: bad}))
        with pytest.raises(ValueError, match=key):
            metrics.load_niqe_params(tmp_path / "bad.npz")


def test_window_sums():
    w = N.synthetic_params()["gaussian_window"]
    assert metrics.niqe_window_sums(w) == (1.0, 0.0)                       # normalised to within its own rounding
    s0, oms0 = metrics.niqe_window_sums(w * 0.75)
    assert abs(s0 - 0.75) < 1e-15 and abs(oms0 - 0.25) < 1e-15


def test_header_types_the_niqe_entries_and_they_refuse_before_launching():
    c = ctypes
    sigs = _lib.signatures()
    assert sigs["glare_niqe_luma_u8"] == (c.c_int, [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_void_p])
    assert sigs["glare_niqe_mscn_f32"] == (c.c_int, [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_float, c.c_float, c.c_void_p, c.c_void_p])
    assert sigs["glare_niqe_block_moments_f32"] == (c.c_int, [c.c_void_p] + [c.c_int] * 5 + [c.c_void_p] * 2)
    assert sigs["glare_niqe_halve_f32"] == (c.c_int, [c.c_void_p, c.c_int, c.c_int, c.c_int, c.c_void_p, c.c_void_p])
    K = _lib.constants()
    assert K["GLARE_NIQE_BLOCK"] == 96 == metrics.NIQE_BLOCK and K["GLARE_NIQE_MAX_BLOCK"] == 96 * 96
    lib = _lib.lib()
    assert lib.glare_version() >= 131
    buf = (c.c_double * 64)()                                  # host memory: every call below returns before it would be read
    p = c.addressof(buf)
    INV, UNS = _lib.ERR_INVALID, _lib.ERR_UNSUPPORTED
    luma = lib.glare_niqe_luma_u8
    assert luma(None, 1, 96, 96, p, None) == INV and luma(p, 1, 96, 96, None, None) == INV
    assert luma(p, 0, 96, 96, p, None) == INV and luma(p, 1, 95, 200, p, None) == INV and luma(p, 1, 200, 95, p, None) == INV
    assert luma(p, 1, 96, 96, (p & ~15) + 4, None) == INV and luma(p, 65536, 96, 96, p & ~15, None) == UNS
    win = _lib.host_f32([1.0 / 49] * 49)
    mscn = lib.glare_niqe_mscn_f32
    assert mscn(None, 1, 8, 8, win, 1.0, 0.0, p, None) == INV and mscn(p, 1, 8, 8, None, 1.0, 0.0, p, None) == INV
    assert mscn(p, 1, 8, 8, win, 1.0, 0.0, None, None) == INV and mscn(p, 1, 0, 8, win, 1.0, 0.0, p, None) == INV
    assert mscn(p, 1, 8, 8, _lib.host_f32([float("nan")] * 49), 1.0, 0.0, p, None) == INV
    assert mscn(p, 1, 8, 8, win, float("inf"), 0.0, p, None) == INV and mscn(p, 65536, 8, 8, win, 1.0, 0.0, p, None) == UNS
    mom = lib.glare_niqe_block_moments_f32
    assert mom(None, 1, 96, 96, 96, 96, p, None) == INV and mom(p, 1, 96, 96, 96, 96, None, None) == INV
    assert mom(p, 1, 96, 100, 96, 96, p, None) == INV and mom(p, 1, 24, 36, 0, 12, p, None) == INV and mom(p, 1, 24, 36, 48, 12, p, None) == INV
    assert mom(p, 1, 192, 192, 96, 97, p, None) == INV and mom(p, 1, 194, 96, 97, 96, p, None) == UNS and mom(p, 1, 192, 192, 192, 96, p, None) == UNS
    halve = lib.glare_niqe_halve_f32
    assert halve(None, 1, 8, 8, p, None) == INV and halve(p, 1, 8, 8, None, None) == INV
    for h, w in ((7, 8), (8, 9), (2, 8), (8, 2), (0, 8), (3, 3)):
        assert halve(p, 1, h, w, p, None) == INV
    assert halve(p, 65536, 8, 8, p, None) == UNS


def _stub_enhance(batch_u8, pads, precision):
    a = np.asarray(batch_u8)
    return (255 - a).astype(np.uint8), np.zeros(a.shape[0], dtype=np.int32)


def test_enhance_niqe_keys_appear_only_with_the_flag(tmp_path):
    from PIL import Image

    src = tmp_path / "photos"
    src.mkdir()
    rng = np.random.default_rng(21)
    for name, (h, w) in (("a.png", (96, 192)), ("b.png", (40, 60)), ("c.png", (96, 192))):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(src / name)
    calls = []

    def scorer(images):
        calls.append([im.copy() for im in images])
        return [(float(im.mean()), None) if im.shape[0] >= 96 else (None, "too small") for im in images]

    plain = enhance.run([str(src)], str(tmp_path / "plain"), enhance_fn=_stub_enhance)
    scored = enhance.run([str(src)], str(tmp_path / "scored"), enhance_fn=_stub_enhance, niqe={"stub": True}, niqe_fn=scorer)
    added_line, added_image = {"niqe_in_mean", "niqe_mean", "niqe_seconds"}, {"niqe_in", "niqe", "niqe_reason"}
    timing = {"seconds", "seconds_per_image_by_size", "images_per_sec", "megapixels_per_sec"}
    assert not (added_line & set(plain)) and not any(added_image & set(e) for e in plain["images"])
    assert set(scored) - set(plain) == added_line
    assert {k: v for k, v in plain.items() if k not in timing | {"images"}} == {k: v for k, v in scored.items() if k not in timing | added_line | {"images"}}
    for a, b in zip(plain["images"], scored["images"]):
        assert a == {k: v for k, v in b.items() if k not in added_image}
    for name in ("a.png", "b.png", "c.png"):
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "scored" / name).read_bytes()
    # the scorer saw the inputs, then the enhanced images; a missing score is null with its reason and stays out of the means
    assert len(calls) == 2 and all(np.array_equal(255 - i, o) for i, o in zip(*calls))
    by = {e["name"]: e for e in scored["images"]}
    assert by["b.png"]["niqe"] is None and by["b.png"]["niqe_in"] is None and by["b.png"]["niqe_reason"] == "too small"
    assert "niqe_reason" not in by["a.png"] and by["a.png"]["niqe"] == pytest.approx(255 - by["a.png"]["niqe_in"])
    assert scored["niqe_mean"] == pytest.approx((by["a.png"]["niqe"] + by["c.png"]["niqe"]) / 2)
    assert scored["niqe_in_mean"] == pytest.approx((by["a.png"]["niqe_in"] + by["c.png"]["niqe_in"]) / 2)
    assert scored["niqe_seconds"] >= 0


def test_cli_flags_exist():
    with pytest.raises(SystemExit):
        metrics.main(["niqe", "some/folder"])                 # --params is required
    with pytest.raises(SystemExit):
        enhance.main(["x", "--out", "y", "--niqe"])           # the flag takes the model's path
