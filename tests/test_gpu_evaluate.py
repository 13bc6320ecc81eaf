"""GPU: the checkpoint sweep (glare_amd.evaluate; code/test_stage2.py, code/test_stage3.py) -- the two harness kernels of the
"adjust" protocol against their numpy restatements, the stage-2 image path against the module calls it replaces, a checkpoint swap
inside the same module instances against fresh ones, and the stage-3 rows against glare_amd.infer."""
import numpy as np
import pytest
import torch

from glare_amd import _lib, checkpoint, evaluate, harness, ops
from glare_amd import modules as M
from glare_amd.fit import default_options
from glare_amd.modules._base import to_nchw
from glare_amd.synthetic import seeded_init_, synthetic_gt, synthetic_lowlight
from scoring_fp64 import output_and_gt as _output          # the generator, shared with test_gpu_scoring_edges.py

pytestmark = pytest.mark.gpu

# (B, Hp, Wp, window): odd sizes -- rows that start at any byte of a 4-byte word, tail lanes, words that straddle two images
# (3 * 29 * 41 = 3567 bytes per image); and one image smaller than a workgroup
_SHAPES = [(3, 37, 53, (2, 5, 29, 41)), (1, 9, 11, (1, 2, 5, 7))]


@pytest.mark.parametrize("B,Hp,Wp,window", _SHAPES)
def test_score_kernel_equals_the_host_restatement_bit_for_bit(B, Hp, Wp, window):
    x, gt_full = _output(B, Hp, Wp)
    top, left, h, w = window
    gt = gt_full[:, :h, :w].contiguous()
    gains = torch.tensor([0.7, float("inf"), 2.1][:B], dtype=torch.float32)          # inf: 0 * inf = NaN -> 0
    xd, gd = x.cuda(), gt.cuda()
    for gain in (None, gains):
        u8, sse = harness.score_device(xd, gd, None if gain is None else gain.cuda(), window)
        want_u8, want_sse = harness.score_u8(x.numpy(), gt.numpy(), None if gain is None else gain.numpy(), window)
        assert u8.dtype == torch.uint8 and tuple(u8.shape) == (B, h, w, 3) and sse.dtype == torch.int64
        assert np.array_equal(u8.cpu().numpy(), want_u8)
        assert sse.cpu().tolist() == want_sse.tolist()
    # gain = NULL is the arithmetic of glare_harness_postprocess_u8
    pads = (top, Hp - top - h, left, Wp - left - w)
    assert torch.equal(harness.score_device(xd, gd, None, window)[0], harness.postprocess_unpaired_device(xd, pads, h, w))
    # the whole tensor as the window, and equal images: sse = 0 -> inf
    same = harness.score_device(xd, harness.score_device(xd, gt_full.cuda())[0])[1]
    assert same.cpu().tolist() == [0] * B and harness.psnr_u8(same[0].item(), 3 * Hp * Wp) == float("inf")


@pytest.mark.parametrize("B,Hp,Wp,window", _SHAPES)
def test_gain_kernel_matches_fp64_and_is_deterministic(B, Hp, Wp, window):
    """Tolerance: two fp64 sums of these values in different orders, rounded to fp32, land at most 1 ulp apart (6e-8 relative);
    1e-6 leaves margin.  The values are finite and their mean is far from 0 (about 1.1)."""
    x, gt_full = _output(B, Hp, Wp, special=False)
    x = x + 0.6                                    # 0.4 .. 1.8: the raw mean (about 1.1) and the clamped one differ
    top, left, h, w = window
    gt = gt_full[:, :h, :w].contiguous()
    xd, gd = x.cuda(), gt.cuda()
    g1 = harness.adjust_gain_device(xd, gd, window)
    g2 = harness.adjust_gain_device(xd, gd, window)
    want = harness.adjust_gain(x.numpy(), gt.numpy(), window)
    assert g1.dtype == torch.float32 and tuple(g1.shape) == (B,)
    got = g1.cpu().numpy()
    print("gain", got, want, np.abs(got / want - 1).max())
    assert np.all(np.abs(got.astype(np.float64) / want.astype(np.float64) - 1) <= 1e-6)
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))
    # raw values, not clamped ones: the clamped mean differs by far more than the tolerance on these inputs
    clamped = harness.adjust_gain(np.clip(x.numpy(), 0, 1), gt.numpy(), window)
    assert np.all(np.abs(clamped / want - 1) > 1e-3)
    # a NaN anywhere in the window makes the mean, and the gain, NaN (as torch's mean does)
    xn = x.clone()
    xn[0, 1, top + h - 1, left + w - 1] = float("nan")
    assert torch.isnan(harness.adjust_gain_device(xn.cuda(), gd, window)[0])


def test_invalid_arguments_are_refused_before_any_launch():
    B, Hp, Wp = 2, 12, 10
    x = torch.rand(B, 3, Hp, Wp, device="cuda")
    gt = torch.zeros(B, 8, 8, 3, dtype=torch.uint8, device="cuda")
    u8 = torch.full((B, 8, 8, 3), 7, dtype=torch.uint8, device="cuda")
    sse = torch.full((B,), -5, dtype=torch.int64, device="cuda")
    gain = torch.full((B,), -3.0, device="cuda")
    lib = _lib.main_lib()
    nws = lib.glare_harness_score_workspace_bytes(B)
    ws = torch.empty(nws, dtype=torch.uint8, device="cuda")
    s = _lib.stream_handle()
    p = _lib.ptr
    for b, top, left, h, w in ((B, 5, 0, 8, 8), (B, 0, 3, 8, 8), (B, -1, 0, 8, 8), (B, 0, 0, 0, 8), (0, 0, 0, 8, 8), (65536, 0, 0, 8, 8)):
        assert lib.glare_harness_score_u8(p(x), None, p(gt), b, Hp, Wp, top, left, h, w, p(u8), p(sse), p(ws), nws, s) == _lib.ERR_INVALID
        assert lib.glare_harness_adjust_gain_f32(p(x), p(gt), b, Hp, Wp, top, left, h, w, p(gain), p(ws), nws, s) == _lib.ERR_INVALID
    assert lib.glare_harness_score_u8(p(x), None, p(gt), B, Hp, Wp, 0, 0, 8, 8, p(u8), p(sse), p(ws), nws - 1, s) == _lib.ERR_WORKSPACE
    assert lib.glare_harness_score_u8(p(x), None, None, B, Hp, Wp, 0, 0, 8, 8, p(u8), p(sse), p(ws), nws, s) == _lib.ERR_INVALID
    torch.cuda.synchronize()
    assert bool((u8 == 7).all()) and sse.tolist() == [-5] * B and gain.tolist() == [-3.0] * B        # nothing was launched
    with pytest.raises(_lib.GlareError) as ei:                 # the wrapper hands the status on
        harness.score_device(x, gt, None, (5, 0, 8, 8))
    assert ei.value.status == _lib.ERR_INVALID


def _stage2_nets(seed=2):
    netG = seeded_init_(M.LLFlowVQGAN2(opt=default_options("stage2")).eval(), seed).cuda()
    return netG, seeded_init_(M.VQModel().eval(), 1).cuda()


def _stage3_nets(seed=0):
    return seeded_init_(M.VQLLFLOWDeformable().eval(), seed).cuda(), seeded_init_(M.VQModel().eval(), 1).cuda()


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
def test_stage2_image_path_equals_the_module_calls_it_replaces(precision):
    netG, net_hq = _stage2_nets()
    lows = torch.from_numpy(synthetic_lowlight(2, 44, 60, seed=5)).cuda()
    lr = harness.preprocess_unpaired_device(lows, (0, 0, 0, 0), harness.PAD_REFLECT101)
    with torch.no_grad(), ops.use_precision(precision):
        z, _ = netG(lr=lr, reverse=True)                       # LLFlowVQGAN2.forward(reverse=True): NCHW latent
        ref, _, ref_feats = net_hq.decode(z)                   # VQModel.decode: NCHW -> codebook -> decoder, image fp32 NCHW
    with torch.no_grad():
        got = netG.enhance_nhwc(net_hq, lr, precision=precision)
    assert tuple(got["out"].shape) == (2, 3, 44, 60) and got["out"].dtype == torch.float32
    assert torch.equal(to_nchw(got["latent"]), z)
    assert torch.equal(got["indices"].view(-1), net_hq.last_indices.view(-1))
    assert torch.equal(got["out"], ref)
    assert bool(torch.isfinite(ref).all()) and float(ref.std()) > 0
    with ops.use_precision(precision):                         # to_nchw takes 16-bit tensors of the precision in use
        for a, b in zip(got["code_feats"], ref_feats):
            assert torch.equal(to_nchw(a), b)


@pytest.mark.parametrize("stage", ["stage2", "stage3"])
def test_checkpoint_swap_in_place_equals_fresh_instances(tmp_path, stage):
    """The test of the cache invalidation: every fold and packed filter of checkpoint A must be gone when B is scored."""
    make = _stage2_nets if stage == "stage2" else _stage3_nets
    seed_a, seed_b = (2, 12) if stage == "stage2" else (0, 10)
    files = {}
    for seed in (seed_a, seed_b):
        files[seed] = str(tmp_path / ("%d_G.pth" % seed))
        checkpoint.save_network(make(seed)[0], files[seed])
    lows, gts = synthetic_lowlight(2, 40, 60, seed=5), synthetic_gt(2, 40, 60, seed=6)
    netG, net_hq = make(seed_a)
    evaluate.load_checkpoint(files[seed_a], netG)
    rep_a, rep_b, rep_f = {}, {}, {}
    rows_a = evaluate.score_checkpoint(stage, netG, net_hq, lows, gts, report=rep_a, keep_images=True)
    evaluate.load_checkpoint(files[seed_b], netG)
    evaluate.warm(stage, netG, net_hq, None, torch.device("cuda"))
    rows_b = evaluate.score_checkpoint(stage, netG, net_hq, lows, gts, report=rep_b, keep_images=True)
    fresh, fresh_hq = make(seed_b)
    rows_f = evaluate.score_checkpoint(stage, fresh, fresh_hq, lows, gts, report=rep_f, keep_images=True)
    assert len(rows_b) == 2 and tuple(rows_b[0]) == evaluate.columns(stage)
    assert rows_b == rows_f
    assert set(rep_b["images"]) == set(rep_f["images"]) == ({"no-adjust", "adjust"} if stage == "stage2" else {"", "adjust"})
    for kind in rep_b["images"]:
        assert rep_b["images"][kind].shape == (2, 40, 60, 3) and np.array_equal(rep_b["images"][kind], rep_f["images"][kind])
    assert all(ra != rb for ra, rb in zip(rows_a, rows_b))
    assert not np.array_equal(rep_a["images"]["adjust"], rep_b["images"]["adjust"])
    assert rep_b["bf16_rerun_images"] == rep_f["bf16_rerun_images"]


def test_stage3_rows_equal_infer_and_the_host_adjust_protocol():
    from glare_amd import infer

    netG, net_hq = _stage3_nets()
    lows, gts = synthetic_lowlight(2, 40, 60, seed=5), synthetic_gt(2, 40, 60, seed=6)
    report = {}
    rows = evaluate.score_checkpoint("stage3", netG, net_hq, lows, gts, report=report, keep_images=True)
    want = np.asarray(infer.run(2, pairs=(lows, gts), nets=(netG, net_hq), with_ssim=True)).reshape(2, 2)
    assert [r["PSNR"] for r in rows] == want[:, 0].tolist()
    assert [r["SSIM"] for r in rows] == want[:, 1].tolist()
    assert report["bf16_rerun_images"] == infer.run.bf16_rerun_images == []
    # 1_PSNR: rgb(clamp(out * mean_gt / mean_out)) against the uint8 ground truth, on the downloaded raw output
    with torch.no_grad():
        out = netG.reverse_flow_nhwc(net_hq, harness.preprocess_device(torch.from_numpy(lows).cuda()))["out"].float().contiguous()
    window = (0, harness.PAD, 40, 60)
    gain = harness.adjust_gain_device(out, torch.from_numpy(gts).cuda(), window).cpu().numpy()
    host_gain = harness.adjust_gain(out.cpu().numpy(), gts, window)
    assert np.all(np.abs(gain.astype(np.float64) / host_gain.astype(np.float64) - 1) <= 1e-6)
    u8, sse = harness.score_u8(out.cpu().numpy(), gts, gain, window)
    assert [r["1_PSNR"] for r in rows] == [harness.psnr_u8(s, 3 * 40 * 60) for s in sse]
    assert np.array_equal(report["images"]["adjust"], u8)
    assert all(np.isfinite(r["1_PSNR"]) and r["1_PSNR"] > 0 for r in rows)
