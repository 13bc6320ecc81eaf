"""Training steps on the HIP path: stage 1 (the VQGAN prior: reconstruction + codebook objective), stage 2 (row a12: conditional
encoder + flow, NLL objective), stage 3 (row a13) and the data-parallel plumbing they share.

Reference: LLFlowModel.optimize_parameters (code/models/LLFlow_model.py:181-250) with its optimizer setup (:90-122):
torch.optim.Adam over two parameter groups -- the flow ("other", lr_G, weight_decay_G) and the conditional encoder
(names containing '.RRDB.', lr_RRDB or lr_G, weight decay 1e-5); the `beta1` / `beta2` keys it passes are not Adam's
`betas`, so torch's defaults (0.9, 0.999) apply.  `scaler.scale(loss).backward(); scaler.step(opt); scaler.update()`
(:236-241): bf16 activations keep fp32's range, so the loss is not scaled -- but GradScaler's other job is: a step whose
gradients hold an inf / NaN is skipped, decided on the device (FlatAdam.step), and the scale / growth tracker are kept as the
reference's scaler would keep them.

MI355X design: parameters, gradients and both Adam moments of a group live in four flat fp32 buffers (module parameters
and their .grad are views), so the optimizer is ONE kernel launch per group and the data-parallel gradient mean is ONE
RCCL all-reduce per group over xGMI (106 MB at stage 2) instead of nn.DataParallel's per-step replicate / scatter /
gather through GPU 0 (LLFlow_model.py:72-75).
"""
import contextlib
import os

import torch
import torch.distributed as dist

from . import autograd as A
from . import checkpoint, losses, ops
from . import train_ops as T
from .modules import encoder_decoder as ED


class FlatGroup:
    """Flat fp32 storage for a parameter group: w / grad / exp_avg / exp_avg_sq; parameters become views."""

    def __init__(self, params, lr, weight_decay=0.0, device=None, never_used=()):
        """never_used: parameters the training graph never reaches (they never get a gradient: torch.optim.Adam keeps no
        state for them and applies no weight decay).  Declared STATICALLY so that the set of parameters Adam updates is
        the same on every rank and every step: a rank-local `p.grad is None` test is not -- stage 2's `train_gt_ratio`
        branch leaves `RRDB.color_conv` without a gradient on the ranks that drew `mean = gt`, and those ranks would skip an
        update the others apply to the all-reduced gradient.  (With nn.DataParallel the reference sums the replicas'
        gradients on one device: a parameter moves whenever any replica used it -- the same rule.)"""
        self.params = [p for p in params if p.requires_grad]
        skip = {id(p) for p in never_used}
        self.has_grad = [id(p) not in skip for p in self.params]
        self.lr, self.weight_decay = float(lr), float(weight_decay)
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device if self.params else torch.device(device or "cpu")
        self.w = torch.empty(n, dtype=torch.float32, device=dev)
        self.g = torch.zeros_like(self.w)
        self.m = torch.zeros_like(self.w)
        self.v = torch.zeros_like(self.w)
        self._early = None          # the armed early all-reduce of the step in progress (arm_early_all_reduce)
        off = 0
        for p in self.params:
            k = p.numel()
            self.w[off:off + k].copy_(p.data.reshape(-1))
            p.data = self.w[off:off + k].view(p.shape)
            off += k

    def zero_grad(self):
        """Gradients are left None: autograd then hands over each gradient tensor without an accumulation kernel per
        parameter; collect() gathers them into the flat buffer with a few concatenations."""
        for p in self.params:
            p.grad = None

    def active_ranges(self):
        """[lo, hi) element ranges of the flat buffer that Adam updates: everything but the `never_used` parameters.
        torch.optim.Adam (the reference's optimizer) skips a parameter whose .grad is None -- no moment update, no weight
        decay, no state entry: the parameters the graph never uses (flowUpsamplerNet.f, deformable_decoder.{scale,bias,enc,
        conv_out}) must not move under weight decay.  Merged, these are 1-3 ranges, i.e. 1-3 Adam launches per group."""
        out, off = [], 0
        for p, used in zip(self.params, self.has_grad):
            k = p.numel()
            if used:
                if out and out[-1][1] == off:
                    out[-1][1] = off + k
                else:
                    out.append([off, off + k])
            off += k
        return [(a, b) for a, b in out]

    def collect(self, chunk=64, grads=None):
        """grads: {id(param): gradient tensor or None} -- the gradients as a multi-grad hook receives them (arm_early_all_reduce),
        BEFORE AccumulateGrad has stored them in .grad; None = read .grad."""
        gof = (lambda p: p.grad) if grads is None else (lambda p: grads.get(id(p)))
        for i, p in enumerate(self.params):
            if gof(p) is not None and not self.has_grad[i]:
                raise RuntimeError("a parameter declared never_used received a gradient (index %d, shape %s)" % (i, tuple(p.shape)))
        off = 0
        for i in range(0, len(self.params), chunk):
            ps = self.params[i:i + chunk]
            n = sum(p.numel() for p in ps)
            if all(gof(p) is None for p in ps):
                self.g[off:off + n].zero_()
            else:
                # runs of parameters WITH a gradient are concatenated into their slot, runs without one zeroed in place (one launch per
                # run; a torch.zeros_like per missing parameter inside the cat was 38 launches of a stage-3 step)
                o2, run, run_off, miss_off = off, [], off, None
                for p in ps + [None]:                                   # (the sentinel closes the last run)
                    gp = gof(p) if p is not None else None
                    if p is not None and gp is not None:
                        if miss_off is not None:
                            self.g[miss_off:o2].zero_()
                            miss_off, run_off = None, o2
                        run.append(gp.reshape(-1).to(torch.float32))
                    else:
                        if run:
                            torch.cat(run, out=self.g[run_off:o2])
                            run = []
                        if p is not None and miss_off is None:
                            miss_off = o2
                    if p is not None:
                        o2 += p.numel()
                if miss_off is not None:
                    self.g[miss_off:o2].zero_()
            off += n
        if grads is not None:     # inside the backward pass: AccumulateGrad has yet to run for these parameters, and a .grad that
            return                # aliases the flat buffer would be accumulated INTO, under the exchange (finish_early_all_reduce re-points)
        self._expose_grads()

    def _expose_grads(self):
        """.grad of every parameter = its view of the flat gradient buffer; parameters the graph never reaches keep None, as in torch."""
        off = 0
        for p, used in zip(self.params, self.has_grad):
            k = p.numel()
            p.grad = self.g[off:off + k].view(p.shape) if used else None
            off += k

    def arm_early_all_reduce(self):
        """Data-parallel steps only: start THIS group's gradient exchange the moment its last gradient exists, while the backward
        pass of the layers in front of it is still running -- stage 2's flow group (53 MB) is complete when FlowNLLFn.backward and
        the fold nodes return, and the conditional encoder's whole backward (the larger half of the step) then hides the ring
        all-reduce over xGMI.  The reference reduces everything through GPU 0 after backward (nn.DataParallel, LLFlow_model.py:
        71-74).  Call before `loss.backward()`; FlatAdam.step() picks the result up (and falls back to the blocking path if the
        hook never fired).  No-op at world size 1, so the single-GPU step and its hipGraph capture are untouched."""
        stale, self._early = self._early, None
        if stale is not None:          # a backward that raised between arm and step(): its hook must not fire on a later backward
            stale["handle"].remove()   # (a stray collect + all_reduce would desynchronise the ranks' collective order)
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1) or not self.params:
            return
        used = [p for p, u in zip(self.params, self.has_grad) if u]
        state = {"fired": False, "work": None}

        def fire(grads):
            state["fired"] = True
            by_id = {id(p): g for p, g in zip(used, grads)}
            self.collect(grads=by_id)
            state["work"] = self.all_reduce(async_op=True)

        state["handle"] = torch.autograd.graph.register_multi_grad_hook(used, fire, mode="all")
        self._early = state

    def finish_early_all_reduce(self):
        """-> the world size if the early exchange ran (the flat gradient buffer then holds the all-reduced sum and every .grad is
        its view), else None (nothing armed, or the hook did not fire: the caller collects and reduces as usual)."""
        state, self._early = self._early, None
        if state is None:
            return None
        state["handle"].remove()
        if not state["fired"]:
            return None
        work = state["work"]
        if work is not None and not isinstance(work, int):
            work.wait()
        for i, (p, used) in enumerate(zip(self.params, self.has_grad)):   # collect()'s check, which the hook's id-keyed dict cannot make:
            if not used and p.grad is not None:                            # a never_used parameter must not have received a gradient
                raise RuntimeError("a parameter declared never_used received a gradient (index %d, shape %s)" % (i, tuple(p.shape)))
        self._expose_grads()                              # AccumulateGrad has since stored the LOCAL gradient tensors in .grad
        return dist.get_world_size()

    def all_reduce(self, async_op=False):
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            if self.g.is_cuda and dist.get_backend() == "gloo":
                # test rigs only (two ranks on one GPU cannot use RCCL): the same exchange bounced through host memory
                host = self.g.cpu()
                dist.all_reduce(host)
                self.g.copy_(host)
            elif async_op:
                return dist.all_reduce(self.g, async_op=True)   # the caller waits on the returned work (finish_early_all_reduce)
            else:
                dist.all_reduce(self.g)        # sum (RCCL over xGMI); the 1/world of the mean is folded into the Adam kernel
            return dist.get_world_size()
        return 1


class FlatAdam:
    """torch.optim.Adam over flat groups with ALL optimizer state on the device -- step count, bias corrections, an lr multiplier,
    GradScaler's found_inf / scale / growth tracker: a step has no host-side state and no host synchronisation (the Python launch
    loop runs ahead of the GPU; the whole step replays from a hipGraph, GraphedStep).  `device_state` is accepted and ignored (Trainer)."""

    def __init__(self, groups, betas=(0.9, 0.999), eps=1e-8, device_state=True, loss_scaling=False, weights_ema=None):
        """loss_scaling: fp16 training -- `scale_loss()` multiplies the loss by the scale before backward and step() divides it out
        of the gradients (scaler.scale / scaler.unscale_, LLFlow_model.py:236-241); bf16 training keeps fp32's range and only runs
        the scaler's bookkeeping.
        weights_ema: a decay d in [0, 1) keeps an exponential moving average of every group's weights on the device (BaseModel.model_ema,
        basicsr/models/base_model.py:85-92; csrc/weight_ema.hip); None (the default) is off: nothing is allocated or launched, and a step is
        what it was, bit for bit.  On: each non-empty group gets `ema` (fp32, the size of `w`) and the optimizer `ema_seeded` (int32 [1], 0).
        At the end of EVERY step(), skipped by the GradScaler or not (the weights did not move then and the average keeps decaying toward
        them, as model_ema called every iteration does), one launch per group over the WHOLE buffer: ema_1 = w_1, the weights after the
        first step (a fresh flow's data-dependent ActNorm initialisation is inside the seed), ema_t = d ema_{t-1} + (1 - d) w_t after
        that; then the flag is filled with 1 on the device, so a captured step holds the same launches on every replay.  The average of a
        parameter Adam never updates is that parameter, up to the rule's own roundings (Trainer.ema_state_dict takes those live).  Ranks
        hold identical weights: no communication."""
        self.groups, self.betas, self.eps = groups, betas, eps
        self.weights_ema = None if weights_ema is None else float(weights_ema)
        assert self.weights_ema is None or 0.0 <= self.weights_ema < 1.0, weights_ema
        self.loss_scaling = bool(loss_scaling)
        dev = next(g.w.device for g in groups if g.w.numel())
        # GradScaler's state (torch.cuda.amp.GradScaler defaults, LLFlow_model.py:120): found_inf of the step in progress, the
        # scale and the growth tracker
        self.found_inf = torch.zeros(1, dtype=torch.int32, device=dev)
        self.scale = torch.full((1,), 65536.0, dtype=torch.float32, device=dev)
        self.growth_tracker = torch.zeros(1, dtype=torch.int32, device=dev)
        self.growth_factor, self.backoff_factor, self.growth_interval = 2.0, 0.5, 2000
        self.step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self.state3 = torch.tensor([1.0, 1.0, 1.0], dtype=torch.float32, device=dev)   # bc1, sqrt(bc2), lr multiplier
        self.ema_seeded = None
        if self.weights_ema is not None:
            for g in groups:
                if g.w.numel():
                    g.ema = torch.empty_like(g.w)          # holds nothing until the first step seeds it (ema_seeded)
            self.ema_seeded = torch.zeros(1, dtype=torch.int32, device=dev)

    def ema_tensors(self):
        """Every tensor the weight average lives in (GraphedStep snapshots them around its warm-up steps); [] when it is off."""
        if self.weights_ema is None:
            return []
        return [g.ema for g in self.groups if g.w.numel()] + [self.ema_seeded]

    @property
    def t(self):
        return int(self.step_dev.item())       # a host read: for checkpoints / tests, never inside a step

    @t.setter
    def t(self, v):
        self.step_dev.fill_(int(v))

    def set_lr_scale(self, s):
        """Scheduler hook: lr_effective = group lr * s (a device scalar the kernels read)."""
        self.state3[2] = float(s)

    def zero_grad(self):
        for g in self.groups:
            g.zero_grad()

    def scale_loss(self, loss):
        """scaler.scale(loss): a device-side multiply (no host read of the scale); the identity without loss scaling."""
        return loss * self.scale.to(loss.dtype).reshape(()) if self.loss_scaling else loss

    def step(self):
        """scaler.step(optimizer); scaler.update() (LLFlow_model.py:240-241): gather + all-reduce the gradients, then ONE Adam
        step over every group -- unless an inf / NaN sits anywhere in them (checked AFTER the all-reduce, so every rank
        decides alike): then nothing moves, the step count stays and the scale backs off.  `last_step_skipped()` reads the flag
        (a host synchronisation) for callers that want to log it."""
        self.found_inf.zero_()
        worlds = []
        for g in self.groups:
            if g.w.numel() == 0:
                worlds.append(1)
                continue
            early = g.finish_early_all_reduce()      # the exchange that started during the backward pass, if one was armed
            if early is None:
                g.collect()
                early = g.all_reduce()
            worlds.append(early)
            T.grad_nonfinite_(g.g, self.found_inf)
        T.adam_prepare_guarded_(self.step_dev, self.state3, self.betas, self.found_inf)
        for g, world in zip(self.groups, worlds):
            if g.w.numel() == 0:
                continue
            for lo, hi in g.active_ranges():       # never-used parameters are skipped, as torch.optim.Adam does
                T.adam_step_dev_guarded_(g.w[lo:hi], g.g[lo:hi], g.m[lo:hi], g.v[lo:hi], self.state3, g.lr, self.betas, self.eps,
                                         g.weight_decay, 1.0 / world, self.found_inf, self.scale if self.loss_scaling else None)
        T.gradscaler_update_(self.scale, self.growth_tracker, self.found_inf, self.growth_factor, self.backoff_factor,
                             self.growth_interval)
        if self.weights_ema is not None:           # on skipped steps too: no host decision, the same launches every step
            for g in self.groups:
                if g.w.numel():
                    T.weight_ema_(g.ema, g.w, self.weights_ema, self.ema_seeded)
            self.ema_seeded.fill_(1)

    def last_step_skipped(self):
        return bool(int(self.found_inf.item()))

    def scaler_state_dict(self):
        """What torch.cuda.amp.GradScaler.state_dict() holds (checkpoint.save_training_state)."""
        return {"scale": float(self.scale.item()), "growth_factor": self.growth_factor, "backoff_factor": self.backoff_factor,
                "growth_interval": self.growth_interval, "_growth_tracker": int(self.growth_tracker.item())}

    def load_scaler_state_dict(self, sd):
        if not sd:
            return
        self.scale.fill_(float(sd.get("scale", 65536.0)))
        self.growth_tracker.fill_(int(sd.get("_growth_tracker", 0)))
        self.growth_factor = float(sd.get("growth_factor", 2.0))
        self.backoff_factor = float(sd.get("backoff_factor", 0.5))
        self.growth_interval = int(sd.get("growth_interval", 2000))


# Parameters the reference constructs but its graphs never call (they never receive a gradient, so torch.optim.Adam never
# touches them): the 320 -> 384 conv of FlowUpsamplerNet (FlowUpsamplerNet.py:113-116) and, in MultiScaleDecoder2, the
# fuse / scale / shift layers of the unused gating path and its own conv_out (deformableDecoder_arch.py:490-523).
STAGE2_NEVER_USED = ("flowUpsamplerNet.f.",)
STAGE3_NEVER_USED = ("deformable_decoder.scale.", "deformable_decoder.bias.", "deformable_decoder.enc.", "deformable_decoder.conv_out.")
# ... and, in VQModel, the 3 -> 256 conv of the semantic branch: `encode` returns vgg_feat = None (VQModel_arch.py:74-79), so `decode`
# never calls it (:81-91).
STAGE1_NEVER_USED = ("conv_semantic.",)


DISC_KEY = "discriminator"   # stage 1 with a discriminator: its Adam and GradScaler state dicts, one more top-level key of a `.state` file
GAN_TERMS = ("g_loss", "d_weight", "d_loss")
USAGE_TERMS = ("codebook_active", "codebook_perplexity")      # Stage1Trainer(codebook_usage=True)
RESTART_KEY = "codebook_restart"   # Stage1Trainer(codebook_restart=P): {"window": int64 [K], "every": P, "threshold": T}, one more key of a `.state` file
RESTART_TERMS = ("codebook_restarted",)
SEMANTIC_TERMS = ("semantic_loss",)                            # Stage1Trainer(semantic=...): the semantic guidance part of codebook_loss
RESTART_OFFSET_STEP = 7919         # the r-th restart of a run takes its tokens from offset r * 7919 (a prime: successive restarts start apart)


def exchange_restart_inputs(window, z):
    """World size > 1: what a restart step needs for every rank to re-seed the same rows with the same values -- `window` (int64 [K],
    each rank's own histogram) is all-reduced with SUM in place, `z` ([N, 3] latents) becomes rank 0's.  -> (window, z).  The identity at
    world size 1 or without a process group.  Plain torch.distributed calls (they take CPU tensors under gloo); with more than one rank
    this has run under gloo only."""
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return window, z
    dist.all_reduce(window)                      # SUM
    z = z.contiguous()
    dist.broadcast(z, src=0)
    return window, z


EMA_KEY = "codebook_ema"           # Stage1Trainer(codebook_ema=d): {"cluster_size": fp32 [K], "embed_avg": fp32 [K, 3], "decay": d, "eps": eps}
EMA_MAX_TOKENS = 1 << 24           # the fp32 count n_k of csrc/vq_ema.hip stays exact up to here, summed over ranks too
EMA_SEED_SIZE = 1.0                # cluster_size of a code the restart re-seeds under EMA: the mean of one token


def exchange_ema_stats(stats, n_tokens=None):
    """World size > 1: the ranks' per-code statistics (fp32 [K, 4] of ops.vq_ema_stats: sums and counts of this rank's n_tokens tokens) are
    all-reduced with SUM in place, so every rank's EMA update sees the whole batch and all codebooks stay alike; world * n_tokens must
    not pass 2^24 (the summed count is an fp32 integer).  -> stats.  The identity at world size 1 or without a process group.  A plain
    torch.distributed call (fp32 sums in the backend's order); with more than one rank this has run under gloo only."""
    if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
        return stats
    assert n_tokens is None or dist.get_world_size() * int(n_tokens) <= EMA_MAX_TOKENS, (dist.get_world_size(), n_tokens)
    dist.all_reduce(stats)                       # SUM
    return stats


def two_group_adam(params, lr, weight_decay, never_used=(), second=(), second_lr=None, second_weight_decay=0.0, betas=(0.9, 0.999),
                   precision="fp16", weights_ema=None):
    """FlatAdam in the layout of the reference's optimizer: always the two groups [other, RRDB] (LLFlow_model.py:110-118,
    VQLLFLOWD_model.py:113-121).  The second group is EMPTY wherever the conditional encoder is not trained (stage 2 with train_RRDB:
    false / before train_RRDB_delay, stage 3, and stage 1 and its discriminator, which have no such encoder), exactly as in the
    reference's optimizer -- so `.state` files are interchangeable (glare_amd/checkpoint.py).  fp16 scales the loss.  weights_ema: FlatAdam's."""
    return FlatAdam([FlatGroup(params, lr, weight_decay, never_used=never_used),
                     FlatGroup(second, lr if second_lr is None else second_lr, second_weight_decay, device=params[0].device)],
                    betas=betas, loss_scaling=precision == "fp16", weights_ema=weights_ema)


WEIGHTS_EMA_KEY = "weights_ema"    # Trainer(weights_ema=d): {"decay": d}, one more key of a `.state` file (the average itself is a network file)
EMA_SUFFIX = "_ema"                # <iter>_<checkpoint_tag>_ema.pth
EMA_RESUME_REFUSAL = ("--weights-ema: %s does not exist: a resumed run continues the average from the file written beside the weights (the "
                      ".state file was written without --weights-ema, or the file was removed); resume without --weights-ema, or put the file back")
EMA_UNSEEDED_REFUSAL = "ema_weights(): no step has seeded the average yet (it starts as the weights after the first step)"


class _AveragedNetwork:
    """What checkpoint.save_network needs of a network, over a trainer's averaged weights."""

    def __init__(self, trainer):
        self.state_dict = trainer.ema_state_dict


def _frozen(net):
    for p in net.parameters():
        p.requires_grad_(False)
    return net.eval()


class Trainer:
    """What the three stages' trainers share, and the ONE interface everything around a trainer talks to (glare_amd.fit, GraphedStep,
    glare_amd.checkpoint): a new stage or objective term overrides members here instead of being recognised by its callers.

    A trainer has `.netG` (the network it trains and the file <iter>_<checkpoint_tag>.pth holds), `.opt` (its FlatAdam), `.pack_cache`,
    `.precision` and `.last_terms` (the terms of the last step's loss, device tensors).  `step_tensor(gt, lq=None, branch=None)` is the step
    without any host synchronisation and returns the loss as a device tensor; `step()` is its float.

    precision: the 16-bit format of activations and activation gradients.  "fp16" (the default) is the reference's own AMP form
    (`@autocast()` forward + `scaler.scale(loss).backward()`, LLFlowVQGAN_arch.py:36, LLFlow_model.py:236-241): IEEE-half
    activations, the loss multiplied by the device-resident GradScaler scale, and the precision every gradient-parity bound of
    tests/test_gpu_train.py is stated in.  "bf16" (fp32 range, no loss scaling, ~1 % faster) rounds every stored tensor 8x
    coarser and carries NO gradient-parity claim (AFT decoder on the pipeline's inputs: 8 % median / 32 % max against fp16's
    2 % / 5 %).

    The subclasses' `device_state=` keyword is accepted and ignored: the optimizer's state lives on the device in every mode (the
    host-state mode it once selected would have cost a synchronisation per step)."""

    checkpoint_tag = "G"                          # glare_amd.fit: <out>/models/<iter>_G.pth
    perceptual, perceptual_weight = None, 1.0     # the frozen loss network of an objective with a perceptual term, and its factor
    weights_ema = None                            # the decay of the averaged weights (FlatAdam), None: no average is kept

    def __init__(self, netG, packed, precision, params, lr, weight_decay, weights_ema=None, **adam):
        """packed: the parameters whose packed filters live across steps; params, lr, weight_decay, **adam: two_group_adam's.
        weights_ema: a decay in [0, 1) keeps an exponential moving average of the trained weights (FlatAdam); a checkpoint then has a
        second network file <iter>_<checkpoint_tag>_ema.pth (ema_state_dict), and ema_weights() runs anything under the average."""
        assert precision in ("bf16", "fp16")
        self.precision, self.netG, self.last_terms = precision, netG, {}
        self.opt = two_group_adam(params, lr, weight_decay, precision=precision, weights_ema=weights_ema, **adam)
        self.weights_ema = self.opt.weights_ema
        self.pack_cache = ops.PackCache(packed)

    def step_tensor(self, gt_img, lr_img=None, branch=None):
        """gt_img: fp32 NCHW ground-truth crop in [0, 1]; lr_img: fp32 NCHW low-light crop (log domain); branch: a key of
        graph_branches(), None = draw_branch()."""
        raise NotImplementedError

    def step(self, *args, **kwargs):
        """step_tensor() with the loss read back: one host synchronisation."""
        return float(self.step_tensor(*args, **kwargs))

    # ---- what the training driver asks (glare_amd.fit) ----
    def extra_networks(self):
        """{suffix: module}: further networks of a checkpoint, written as <iter>_<suffix>.pth beside <iter>_<checkpoint_tag>.pth.  With
        weights_ema: <iter>_<checkpoint_tag>_ema.pth, the averaged weights under the network's own key names (the suffix ends in `_ema`, so
        glare_amd.evaluate's `*_<tag>.pth` glob does not take it for a checkpoint of its own)."""
        return {} if self.weights_ema is None else {self.checkpoint_tag + EMA_SUFFIX: _AveragedNetwork(self)}

    def extra_state(self):
        """Further top-level entries of a `.state` file (the reference's resume reads its five keys by name and ignores any other)."""
        return {} if self.weights_ema is None else {WEIGHTS_EMA_KEY: {"decay": self.weights_ema}}

    # ---- the averaged weights (weights_ema) ----
    def _averaged_params(self):
        """[(parameter, its slice of the group's `ema`)] over the parameters Adam updates.  A parameter declared
        never_used is not listed: it never moves by Adam, and what else writes it (the EMA codebook of stage 1) is taken live."""
        out = []
        for g in self.opt.groups:
            off = 0
            for p, used in zip(g.params, g.has_grad):
                k = p.numel()
                if used and k:
                    out.append((p, g.ema[off:off + k]))
                off += k
        return out

    def ema_seeded(self):
        """Has a step seeded the average (or a resume loaded it)?  A host read."""
        return self.weights_ema is not None and bool(int(self.opt.ema_seeded.item()))

    def ema_state_dict(self):
        """netG.state_dict() with every trained parameter's tensor replaced by its average; buffers, frozen and never-used parameters are
        the live ones.  Before the first step there is no average yet: the live weights."""
        sd = self.netG.state_dict()
        if not self.ema_seeded():
            return sd
        avg = {p.data_ptr(): e.view(p.shape) for p, e in self._averaged_params()}
        return type(sd)((k, avg[v.data_ptr()] if v.data_ptr() in avg and v.shape == avg[v.data_ptr()].shape else v) for k, v in sd.items())

    def load_ema_weights(self, path):
        """The resume side of <iter>_<checkpoint_tag>_ema.pth: the file's tensors into the `ema` buffers (whatever it does not name
        starts from the live weights) and the flag set.  A missing file is refused by name."""
        assert self.weights_ema is not None, "load_ema_weights: the trainer was built without weights_ema"
        if not os.path.exists(path):
            raise ValueError(EMA_RESUME_REFUSAL % path)
        sd = torch.load(path, map_location="cpu")
        sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
        names = {p.data_ptr(): k for k, p in self.netG.named_parameters()}
        for g in self.opt.groups:
            if g.w.numel():
                g.ema.copy_(g.w)
        for p, e in self._averaged_params():
            name = names.get(p.data_ptr())
            if name in sd:
                e.copy_(sd[name].reshape(-1).to(e.device, torch.float32))
        self.opt.ema_seeded.fill_(1)

    def _swap_averaged(self):
        for g in self.opt.groups:
            if g.w.numel():
                for lo, hi in g.active_ranges():       # what Adam updates; the rest stays live, as in ema_state_dict()
                    T.swap_(g.w[lo:hi], g.ema[lo:hi])
        self.invalidate()

    @contextlib.contextmanager
    def ema_weights(self):
        """`with trainer.ema_weights():` -- the network holds the averaged weights inside (w and ema exchanged in place, no third buffer;
        packed inference weights dropped on the way in and out) and the live ones, bit for bit, after.  No training step inside."""
        if not self.ema_seeded():
            raise RuntimeError(EMA_UNSEEDED_REFUSAL)
        self._swap_averaged()
        try:
            yield self
        finally:
            self._swap_averaged()

    def load_extra_state(self, state):
        """The resume side of extra_state(): `state` is the whole `.state` dict."""

    def objective_tag(self):
        """None, or a string naming the part of the objective that travels in no checkpoint (the frozen loss network and its factor): the
        `.state` file records it, and a resume under another one is refused."""
        return None if self.perceptual is None else "%s x %g" % (type(self.perceptual).__name__, self.perceptual_weight)

    def on_resume(self, step):
        """Called with the step count of the `.state` file a run resumes from."""

    def log_terms(self):
        """The keys of `last_terms` a log record carries beside the loss."""
        return () if self.perceptual is None else ("percep_loss",)

    # ---- what the graph capture asks (GraphedStep) ----
    def graph_branches(self):
        """The keys of every kernel sequence the step can take: a capture covers them all up front.  One for a step without a host-side
        decision."""
        return (False,)

    def draw_branch(self):
        """The step's host-side random decision: the key of graph_branches() this step takes."""
        return False

    def init_forward(self, gt_img, lr_img, branch):
        """Whatever data-dependent initialisation the FIRST training forward performs, on its own: no tape kept, nothing updated."""

    def invalidate(self):
        """Drops the packed inference weights that a step made stale."""
        self.netG.invalidate()


class Stage2Trainer(Trainer):
    """One optimisation step of the flow objective: a7 (frozen VQGAN encoder, no tape) -> a1 -> a4 -> mean NLL -> backward ->
    gradient mean over ranks -> Adam."""

    def __init__(self, netG, net_hq, lr_G=5e-4, lr_RRDB=None, weight_decay_G=0.0, train_rrdb=True, device_state=False, precision="fp16",
                 weights_ema=None):
        self.net_hq = _frozen(net_hq)
        rrdb = [p for n, p in netG.named_parameters() if n.startswith("RRDB.")]
        other = [p for n, p in netG.named_parameters() if not n.startswith("RRDB.")]
        if not train_rrdb:  # train_RRDB_delay (LLFlow_model.py:142-150): the encoder joins after a fraction of the run
            for p in rrdb:
                p.requires_grad_(False)
        never = [p for n, p in netG.named_parameters() if n.startswith(STAGE2_NEVER_USED)]
        super().__init__(netG.train(), [p for p in netG.parameters() if p.requires_grad], precision, other, lr_G, weight_decay_G,
                         never_used=never, second=rrdb if train_rrdb else [], second_lr=lr_RRDB, second_weight_decay=1e-5, weights_ema=weights_ema)

    def graph_branches(self):
        """mean = color_map, and mean = gt where it can be drawn (train_gt_ratio > 0: 0.2 in confs/train_stage2_LOL.yml, 0 in LOL.yml)."""
        return (False, True) if float(self.netG.train_gt_ratio) > 0.0 else (False,)

    def draw_branch(self):
        """The step's one host-side random decision (LLFlowVQGAN_arch.py:95): is the Gaussian's mean the ground truth?"""
        return self.netG._mean_is_gt(None)

    def init_forward(self, gt_img, lr_img, branch):
        """The forward half of a step only (what initialises a fresh flow's ActNorms)."""
        flow = self.netG.flowUpsamplerNet
        with ops.use_precision(self.precision), torch.no_grad():
            if flow.needs_actnorm_init():                      # exactly what train_nll() does first (LLFlowVQGAN_arch.train_nll)
                with ops.auto_cout_tile():
                    gt_latent = self.net_hq.encode_nhwc(gt_img)
                enc0 = self.netG.RRDB.forward_nhwc(lr_img)
                flow.initialize_actnorms_nhwc(gt_latent.detach(), enc0["cond_feat"])

    def step_tensor(self, gt_img, lr_img=None, branch=None, *, mean_is_gt=None):
        """branch (or, by keyword, mean_is_gt): None = draw with probability train_gt_ratio as the reference does; True / False =
        forced (GraphedStep draws before choosing a graph)."""
        branch = mean_is_gt if branch is None else branch
        flag = self.draw_branch() if branch is None else bool(branch)
        with ops.use_precision(self.precision):
            with torch.no_grad(), ops.auto_cout_tile():
                gt_latent = self.net_hq.encode_nhwc(gt_img)            # LLFlow_model.py:200-201
            self.opt.zero_grad()
            with self.pack_cache:
                nll = self.netG.train_nll(gt_latent, lr_img, mean_is_gt=flag)   # :215
                loss = nll.mean()
                self.opt.groups[0].arm_early_all_reduce()              # N > 1: the flow group's all-reduce runs under the encoder's backward
                self.opt.scale_loss(loss).backward()                   # :236  scaler.scale(loss).backward()
            self.opt.step()                                            # :240-241  scaler.step(); scaler.update()
        self.invalidate()                                          # packed inference weights are stale now
        return loss.detach()


class Stage3Trainer(Trainer):
    """One optimisation step of stage 3 (row a13, VQLLFLOWDModel.optimize_parameters, VQLLFLOWD_model.py:187-232): the
    conditional encoder, the flow (reverse) and the VQGAN decoder run without a tape exactly as in inference
    (VQLLFLOWDeformable_arch.py:231-248); only `deformable_decoder` is trained.  Loss (:217-223): L1 + 0.01 * VGG16-feature
    perceptual + 0.2 * (1 - MS-SSIM(normalize=True)).  The perceptual network's weights are the caller's (`perceptual=`): the
    reference downloads torchvision's pretrained VGG16, which is not available offline; pass None to train on L1 + MS-SSIM."""

    def __init__(self, netG, net_hq, lr_G=5e-5, weight_decay_G=0.0, perceptual=None, use_msssim=True, device_state=False, precision="fp16",
                 frozen_fp32_class=False, weights_ema=None):
        """frozen_fp32_class: run the FROZEN conditional encoder + flow in the fp32-class inference form (hi / lo operand pairs, three
        MFMA passes per conv) instead of the single-pass fp16 form.  Default False: the reference runs these nets under `@autocast()`
        in the stage-3 step (VQLLFLOWDeformable_arch.py:222-248), i.e. single-pass fp16 is ITS arithmetic; the fp32-class form serves
        inference's index contract and costs the step ~3.5 ms (23.0 -> 19.5 ms at 1 x 256^2, round 4 / 5)."""
        self.frozen_fp32_class, self.perceptual, self.use_msssim = bool(frozen_fp32_class), perceptual, use_msssim
        self.net_hq = _frozen(net_hq)
        for n, p in netG.named_parameters():
            p.requires_grad_(n.startswith("deformable_decoder."))
        dd = [p for n, p in netG.named_parameters() if n.startswith("deformable_decoder.")]
        never = [p for n, p in netG.named_parameters() if n.startswith(STAGE3_NEVER_USED)]
        super().__init__(netG, dd, precision, dd, lr_G, weight_decay_G, never_used=never, second_weight_decay=1e-5, weights_ema=weights_ema)

    def invalidate(self):
        """Only the deformable decoder's packed inference weights go stale; the frozen nets keep theirs."""
        self.netG.deformable_decoder.invalidate()

    def step_tensor(self, gt_img, lr_img=None, branch=None):
        G = self.netG
        with ops.use_precision(self.precision):
            with torch.no_grad(), ops.auto_cout_tile(), ED.fp32_class(self.frozen_fp32_class):
                enc = G.RRDB.forward_nhwc(lr_img)
                lat = G.flowUpsamplerNet.decode_nhwc(enc["color_map"], enc["cond_feat"])
                _, _, feats = self.net_hq.decode_nhwc(lat, want_image=False)
            self.opt.zero_grad()
            with self.pack_cache:
                rec = G.deformable_decoder.train_nhwc(lat, feats, enc["mid_feat"], whole_batch_mean=True)
                loss, self.last_terms = stage3_loss(rec, gt_img, self.perceptual, self.use_msssim)
                self.opt.scale_loss(loss).backward()
            self.opt.step()
        self.invalidate()
        return loss.detach()


class Stage1Trainer(Trainer):
    """One optimisation step of stage 1, the VQGAN prior itself (VQModel.forward + configure_optimizers, VQModel_arch.py:98-101,
    148-157): x -> encoder -> quant_conv -> codebook (straight-through) -> post_quant_conv -> decoder, every layer with a tape.
    Loss: mean |xrec - x| + codebook_weight * qloss (+ perceptual_weight * perceptual(xrec, x) when a perceptual network is passed).
    x is the ground-truth crop in [0, 1] -- what `net_hq.encode` is fed in stages 2 and 3.  The L1 is plain, not `l1_clamp_loss`: a
    clamp would zero the gradient wherever the reconstruction leaves [0, 1].

    The reference's `self.loss` is taming's VQLPIPSWithDiscriminator (`self.loss(qloss, x, xrec, optimizer_idx, global_step,
    last_layer=self.get_last_layer())`, VQModel_arch.py:110-160), which is not part of the reference tree.  All three of its parts are
    built: LPIPS behind `perceptual=losses.LPIPSLoss()` (the VGG16 trunk and the heads are the caller's files, losses.load_vgg16: the
    pretrained weights cannot be fetched offline, as in stage 3), the patch discriminator with the hinge loss and the adaptive weight
    behind `discriminator=`.  With a discriminator D the step at global step t is
        nll      = l1 (+ perceptual)                       g_loss = -mean D(xrec)
        d_weight = clamp(|d nll / d W_last| / (|d g_loss / d W_last| + 1e-4), 0, 1e4) * disc_weight, detached; W_last = decoder.conv_out.weight
        loss     = nll + d_weight f g_loss + codebook_weight qloss            f = disc_factor if t >= disc_start else 0
        d_loss   = f 0.5 (mean relu(1 - D(x)) + mean relu(1 + D(xrec.detach())))          D's own Adam (betas (0.5, 0.9), lr_G) and GradScaler
    from ONE pass through D over [x; xrec] as two batch groups (BatchNorm statistics per half, as two calls): the fake half's logits
    serve g_loss and d_loss alike, the generator's term takes only the data gradient of that pass (autograd.data_grad_only), D's term only
    its parameter gradients.  Both gradients at xrec are pushed through conv_out's weight gradient once each for the two norms and the
    generator is backpropagated ONCE from their weighted sum -- the arithmetic of the reference's two backward passes.  D sees the xrec of
    this step's generator forward (Lightning's loop runs the generator forward again after its update).  While t < disc_start nothing of D
    is launched and the generator's update is today's, bit for bit.  The optimizer is the reference's: Adam, betas (0.5, 0.9), one group
    over encoder, decoder, quantize, quant_conv and post_quant_conv (:148-157)."""

    checkpoint_tag = "VQ"                            # glare_amd.fit: <out>/models/<iter>_VQ.pth, the file `--net-vq` takes

    def __init__(self, net, lr_G=1e-4, weight_decay_G=0.0, codebook_weight=1.0, perceptual=None, perceptual_weight=1.0,
                 device_state=False, precision="fp16", discriminator=None, disc_start=10000, disc_weight=0.8, disc_factor=1.0,
                 codebook_usage=False, codebook_restart=0, restart_threshold=0, codebook_ema=None, ema_eps=1e-5, semantic=None,
                 semantic_weight=0.1, weights_ema=None):
        """lr_G: a starting point, not a tuned value (the reference sets `self.learning_rate` from a config it does not ship).
        discriminator: an NLayerDiscriminator on the net's device, or None (no GAN term: the step and every file are what they were);
        disc_start / disc_weight / disc_factor: taming's defaults for the VQGAN configs.
        codebook_usage: every step also puts `codebook_active` (int64: the distinct codes the step's indices select) and
        `codebook_perplexity` (fp64, quantize.py:83-85) of that forward pass into last_terms -- three small launches (csrc/vq_usage.hip), no
        host synchronisation; off (the default), the step launches and records what it always did.  Usage is not state: nothing of it
        is written to a `.state` file.
        codebook_restart: P > 0 revives dead codes every P steps (csrc/vq_restart.hip); 0 (the default) is off, and the step then launches
        and records exactly what it always did.  A code no token selects gets dE = 0 and never moves again -- at the reference's
        initialisation (uniform(-1/8192, 1/8192)) that is most of the codebook.  On: every step adds its indices' histogram to a persistent
        int64 [K] window (`restart_window`; the one ops.vq_usage call codebook_usage makes too), and after `opt.step()` of every step whose
        new global_step is a multiple of P, the codes with window count <= restart_threshold are overwritten, in ascending order, with evenly
        strided rows of this step's `net.last_latent`, starting at token (global_step // P) * 7919; their Adam moments are zeroed, the
        window restarts from zero, and `last_terms["codebook_restarted"]` holds the number of rows written (a device zero on the other
        steps).  All of it on the device: no count is read back.  The restart depends on no gradient, so a step the GradScaler skipped
        restarts all the same.  Adam's step count is ONE device scalar shared by every parameter: a re-seeded row starts again from zero
        moments but under the run's global bias correction (1 - beta^t, t the run's step count), not a fresh t = 1 -- late in a
        run its first update is about (1 - beta1) / sqrt(1 - beta2) lr (1.58 lr at this stage's betas) where a new parameter's is lr.  The window is state: it travels in the `.state` file with P
        and the threshold, and a resume under other values is refused.  World size > 1: exchange_restart_inputs.
        codebook_ema: a decay d in (0, 1) moves the codebook by the reference's EmbeddingEMA rule instead of a gradient (quantize.py:345-358,
        426-437; csrc/vq_ema.hip); None (the default) is off: nothing new is launched, and the step and every file are what they were, bit
        for bit.  On: the embedding stops requiring a gradient and is declared `never_used` -- Adam keeps its moments at zero, applies no
        update and no weight decay -- the codebook term becomes beta mean((z_q.detach() - z)^2) alone (dE is not computed), and
        `cluster_size` (fp32 [K], zeros) and `embed_avg` (fp32 [K, 3], the codebook's clone, :336-339) become trainer state.  After
        `opt.step()` of every step, skipped by the GradScaler or not (no gradient is involved): stats of this step's indices and latents
        (ops.vq_ema_stats), exchange_ema_stats, ops.vq_ema_update with (d, ema_eps) -- the reference's arithmetic: the step's lookup used the
        old rows, the backward never reads the codebook.  A code nothing selects only decays: from cluster_size = 0 its smoothed size is
        about eps and its row embed_avg / ~eps, far from every latent, and it stays dead.  So use it with codebook_restart: on the restart
        steps, AFTER that step's EMA update, ops.vq_restart_ema re-seeds codebook and embed_avg rows alike and sets their cluster_size to
        1.0.  Both tensors travel in the `.state` file with d and eps; a resume under other values, or with the key and the option not
        both present, is refused.  <iter>_VQ.pth keeps VQModel's keys.
        semantic: a loaded losses.SemanticTarget (VGG19 down to relu3_4, the caller's file: losses.load_vgg19), or None (the default) --
        off: nothing new is launched, and the step and every file are what they were, bit for bit.  On: the reference's semantic guidance
        term (VQModel_arch.py:85-88, `emb_loss += 0.1 * F.mse_loss(conv_semantic(quant), vgg_feat)`; fed as the ancestor's HQ pre-training
        stage feeds it, the extractor on the input under no_grad).  Both step forms compute vgg_feat = semantic(x) once per step and hand it
        to VQModel.train_nhwc, where the term rides in qloss -- so codebook_weight multiplies it as it multiplies emb_loss there, and the
        GAN step needs nothing else.  `last_terms["codebook_loss"]` is reported as it is computed, INCLUDING the term;
        `last_terms["semantic_loss"]` = codebook_weight * semantic_weight * mse is the part of it (not a further summand of the total).
        `conv_semantic.*` is then NOT declared never_used for this trainer: it trains in the same Adam group (the flat layout always held
        it, so the `.state` layout does not change).  The reference's configure_optimizers list (:150-155) omits conv_semantic because the
        branch is dead there (its forward passes no vgg_feat); the ancestor optimises all of net_g.  The term's gradient reaches the
        encoder and quant_conv through the straight-through output and never a codebook row, so it goes together with codebook_ema,
        codebook_restart, the discriminator and LPIPS.  The loss network is in no checkpoint: objective_tag() names it with its weight, and
        a resume under another objective is refused.
        weights_ema: Trainer's.  The generator alone is averaged: the discriminator's optimizer gets no average.  Under codebook_ema the
        codebook is outside what Adam updates, so it is not averaged either: <iter>_VQ_ema.pth and ema_weights() carry the live one."""
        self.semantic, self.semantic_weight = semantic, float(semantic_weight)
        self.codebook_usage = bool(codebook_usage)
        self.codebook_ema, self.ema_eps = (None if codebook_ema is None else float(codebook_ema)), float(ema_eps)
        assert self.codebook_ema is None or (0.0 < self.codebook_ema < 1.0 and self.ema_eps >= 0.0), (codebook_ema, ema_eps)
        self.codebook_restart, self.restart_threshold = int(codebook_restart), int(restart_threshold)
        assert self.codebook_restart >= 0 and self.restart_threshold >= 0, (codebook_restart, restart_threshold)
        self.restart_window = None                   # off: ops.vq_usage is handed no total, as ever
        self.codebook_weight, self.perceptual, self.perceptual_weight = float(codebook_weight), perceptual, float(perceptual_weight)
        for p in net.parameters():
            p.requires_grad_(True)
        named = list(net.named_parameters())
        never = [] if semantic is not None else [p for n, p in named if n.startswith(STAGE1_NEVER_USED)]
        E = net.quantize.embedding.weight
        if self.codebook_ema is not None:            # in the flat layout as ever (one `.state` layout), outside what Adam updates
            never.append(E)
        super().__init__(net.train(), [p for n, p in named if not n.startswith(STAGE1_NEVER_USED)], precision, [p for _, p in named], lr_G,
                         weight_decay_G, never_used=never, betas=(0.5, 0.9), weights_ema=weights_ema)
        self.net = self.netG                         # `netG`: the name the driver and the checkpoint code read
        if semantic is not None:
            net.semantic_weight = self.semantic_weight
        self.discriminator, self.opt_d = discriminator, None
        self.disc_start, self.disc_weight, self.disc_factor = int(disc_start), float(disc_weight), float(disc_factor)
        self.global_step = 0                         # Lightning's global_step: steps taken so far (on_resume restores it)
        self.cluster_size = self.embed_avg = None
        if self.codebook_ema is not None:
            E.requires_grad_(False)                  # autograd.VQStraightThroughFn then computes no dE
            net.quantize.ema_update = True           # VectorQuantizer2.loss_weights(): (beta, 0)
            self.cluster_size = torch.zeros(E.shape[0], dtype=torch.float32, device=E.device)
            self.embed_avg = E.detach().clone()
        if self.codebook_restart:
            # the parameters are views of FlatGroup.w: the embedding's rows of w, exp_avg and exp_avg_sq sit at one static offset
            g0, off = self.opt.groups[0], 0
            for p in g0.params:
                if p is E:
                    break
                off += p.numel()
            else:
                raise RuntimeError("the codebook is not a parameter of the optimizer's first group")
            self._restart_rows = tuple(t[off:off + E.numel()].view(E.shape) for t in (g0.w, g0.m, g0.v))
            assert self._restart_rows[0].data_ptr() == E.data_ptr()
            self.restart_window = torch.zeros(E.shape[0], dtype=torch.int64, device=E.device)
            self._restart_none = torch.zeros((), dtype=torch.int64, device=E.device)
        if discriminator is not None:
            discriminator.train()
            for p in discriminator.parameters():
                p.requires_grad_(True)
            dparams = list(discriminator.parameters())
            self.opt_d = two_group_adam(dparams, lr_G, 0.0, betas=(0.5, 0.9), precision=precision)
            self._zero = torch.zeros((), dtype=torch.float32, device=dparams[0].device)

    def extra_networks(self):
        """<iter>_D.pth: taming's NLayerDiscriminator state dict."""
        return dict(super().extra_networks(), **({} if self.discriminator is None else {"D": self.discriminator}))

    def extra_state(self):
        """D's Adam and GradScaler state, the restart's window with its two settings, and the EMA's two tensors with theirs, travel as
        further keys of the `.state` file."""
        extra = super().extra_state()
        if self.discriminator is not None:
            extra[DISC_KEY] = {"optimizer": checkpoint.adam_state_dict(self.opt_d), "scaler": self.opt_d.scaler_state_dict()}
        if self.codebook_restart:
            extra[RESTART_KEY] = {"window": self.restart_window.cpu().clone(), "every": self.codebook_restart,
                                  "threshold": self.restart_threshold}
        if self.codebook_ema is not None:
            extra[EMA_KEY] = {"cluster_size": self.cluster_size.cpu().clone(), "embed_avg": self.embed_avg.cpu().clone(),
                              "decay": self.codebook_ema, "eps": self.ema_eps}
        return extra

    def load_extra_state(self, state):
        if self.discriminator is not None:
            assert DISC_KEY in state, "--gan: the .state file carries no discriminator optimizer (it was written without --gan)"
            checkpoint.load_adam_state_dict(self.opt_d, state[DISC_KEY]["optimizer"])
            self.opt_d.load_scaler_state_dict(state[DISC_KEY]["scaler"])
        saved = state.get(RESTART_KEY)
        if self.codebook_restart:
            assert saved is not None, ("--codebook-restart: the .state file carries no restart window (it was written without "
                                       "--codebook-restart)")
            assert (int(saved["every"]), int(saved["threshold"])) == (self.codebook_restart, self.restart_threshold), (
                "--codebook-restart: the .state file was written with --codebook-restart %d --restart-threshold %d and this run has %d and %d: "
                "the window would be read against another rule partway through; name the same values again"
                % (saved["every"], saved["threshold"], self.codebook_restart, self.restart_threshold))
            self.restart_window.copy_(saved["window"])
        else:
            assert saved is None, ("the .state file carries a restart window (it was written with --codebook-restart %d) and this run has "
                                   "no --codebook-restart: name it again" % saved["every"])
        saved = state.get(EMA_KEY)
        if self.codebook_ema is not None:
            assert saved is not None, ("--codebook-ema: the .state file carries no cluster_size / embed_avg (it was written without "
                                       "--codebook-ema, by a run whose codebook followed its gradient)")
            assert (float(saved["decay"]), float(saved["eps"])) == (self.codebook_ema, self.ema_eps), (
                "--codebook-ema: the .state file was written with --codebook-ema %r --ema-eps %r and this run has %r and %r: the averages "
                "would go on under another rule partway through; name the same values again"
                % (saved["decay"], saved["eps"], self.codebook_ema, self.ema_eps))
            self.cluster_size.copy_(saved["cluster_size"])
            self.embed_avg.copy_(saved["embed_avg"])
        else:
            assert saved is None, ("the .state file carries an EMA codebook's state (it was written with --codebook-ema %r --ema-eps %r) and "
                                   "this run has no --codebook-ema: name both again" % (saved["decay"], saved["eps"]))

    def on_resume(self, step):
        self.global_step = step                      # what `disc_start` and the restart's period are compared with

    def objective_tag(self):
        tags = [t for t in (Trainer.objective_tag(self), None if self.semantic is None else
                            "%s x %g" % (type(self.semantic).__name__, self.semantic_weight)) if t is not None]
        return " + ".join(tags) or None

    def log_terms(self):
        return ((GAN_TERMS if self.discriminator is not None else ()) + super().log_terms() + (SEMANTIC_TERMS if self.semantic is not None else ())
                + (USAGE_TERMS if self.codebook_usage else ()) + (RESTART_TERMS if self.codebook_restart else ()))

    def _forward(self, gt):
        """The taped autoencoder on the step's batch; with the semantic term, its target first: (xrec, qloss, idx)."""
        if self.semantic is None:
            return self.net.train_nhwc(gt)
        return self.net.train_nhwc(gt, self.semantic(ops.nchw_to_nhwc(gt, bf16=False)))

    def _semantic_terms(self):
        return {} if self.semantic is None else {"semantic_loss": self.net.last_semantic * (self.codebook_weight * self.semantic_weight)}

    def _usage_terms(self, idx):
        """{codebook_active, codebook_perplexity} of one forward pass's indices, device tensors.  With the restart on, the same
        histogram call adds the step's counts to its window."""
        counts, _, _ = ops.vq_usage(idx, self.net.quantize.n_e, total=self.restart_window)
        _, active, _, perplexity = ops.vq_usage_stats(counts)
        return {"codebook_active": active[0], "codebook_perplexity": perplexity[0]}

    def _codebook_terms(self, idx):
        """What follows `opt.step()` for the codebook's bookkeeping: the EMA update, the usage terms, the restart's window and, on its
        steps, the restart itself (after that step's EMA update).  Every option off: nothing is launched and {} comes back."""
        if self.codebook_ema is not None:
            E = self.net.quantize.embedding.weight.data
            stats = exchange_ema_stats(ops.vq_ema_stats(idx, self.net.last_latent, E.shape[0]), idx.numel())
            ops.vq_ema_update(stats, self.cluster_size, self.embed_avg, E, self.codebook_ema, self.ema_eps)
        terms = self._usage_terms(idx) if self.codebook_usage else {}
        if not self.codebook_restart:
            return terms
        if not self.codebook_usage:
            ops.vq_usage(idx, self.net.quantize.n_e, total=self.restart_window)
        terms["codebook_restarted"] = self._restart_none
        if self.global_step % self.codebook_restart == 0:          # global_step: already this step's new count
            w, m, v = self._restart_rows
            window, z = exchange_restart_inputs(self.restart_window, self.net.last_latent)
            offset = (self.global_step // self.codebook_restart) * RESTART_OFFSET_STEP
            if self.codebook_ema is not None:
                _, terms["codebook_restarted"] = ops.vq_restart_ema(window, z, w, self.embed_avg, self.cluster_size, offset,
                                                                    self.restart_threshold, EMA_SEED_SIZE)
            else:
                _, terms["codebook_restarted"] = ops.vq_restart(window, z, w, offset, self.restart_threshold, m, v)
        return terms

    def invalidate(self):
        self.net.invalidate()
        if self.discriminator is not None:
            self.discriminator.invalidate()

    def get_last_layer(self):
        """VQModel.get_last_layer (VQModel_arch.py:159-160): the weight the adaptive GAN weight takes its two gradient norms at."""
        return self.net.decoder.conv_out.weight

    def step_tensor(self, gt_img, lr_img=None, branch=None):
        """lr_img is ignored (the driver hands both halves of a pair)."""
        gt = gt_img.float().contiguous()
        t, self.global_step = self.global_step, self.global_step + 1
        if self.discriminator is not None and t >= self.disc_start and self.disc_factor != 0.0:
            return self._gan_step(gt)
        with ops.use_precision(self.precision):
            self.opt.zero_grad()
            with self.pack_cache:
                xrec, qloss, idx = self._forward(gt)
                loss, self.last_terms = stage1_loss(xrec, gt, qloss, self.codebook_weight, self.perceptual, self.perceptual_weight)
                self.opt.scale_loss(loss).backward()
            self.opt.step()
        self.net.invalidate()                        # packed inference weights are stale now
        self.last_terms.update(self._semantic_terms())
        self.last_terms.update(self._codebook_terms(idx))     # (the search reads embedding.weight itself: nothing packed goes stale)
        if self.discriminator is not None:           # before disc_start: f = 0, nothing of D launched, its parameters and optimizer untouched
            self.last_terms.update(g_loss=self._zero, d_weight=self._zero, d_loss=self._zero)
        return loss.detach()

    def _disc_logits(self, gt_nchw, xrec_nhwc):
        """One pass of D over [x; xrec] as two batch groups -> (logits of the real half, of the fake half), fp32 [B, oh, ow, 1]."""
        both = torch.cat([ops.nchw_to_nhwc(gt_nchw, bf16=False), xrec_nhwc])      # 3-channel images: an image-sized copy
        logits = self.discriminator.train_nhwc(both, groups=2)
        B = gt_nchw.shape[0]
        return logits[:B], logits[B:]

    def _gan_step(self, gt):
        f = self.disc_factor
        with ops.use_precision(self.precision):
            self.opt.zero_grad()
            self.opt_d.zero_grad()
            self.opt_d.state3[2:3].copy_(self.opt.state3[2:3])       # D's lr follows the generator's schedule (one device scalar)
            with self.pack_cache:
                xrec, qloss, idx = self._forward(gt)
                # the two gradients at xrec, on a detached leaf: nll's and, through D (data gradients only), g_loss's.  Both carry the
                # generator's loss scale s (fp16: 1 / n of a mean is an fp16 subnormal unscaled), divided out of the norms below
                xr = xrec.detach().requires_grad_(True)
                nll, terms = stage1_loss(xr, gt, None, self.codebook_weight, self.perceptual, self.perceptual_weight)
                s = self.opt.scale.reshape(()) if self.opt.loss_scaling else None
                scaled = (lambda v: v * s) if s is not None else (lambda v: v)
                (g_nll,) = torch.autograd.grad(scaled(nll), xr)
                logits_real, logits_fake = self._disc_logits(gt, xr)
                g_loss = A.hinge_loss(logits_fake, "generator")
                with A.data_grad_only():
                    (g_gan,) = torch.autograd.grad(scaled(g_loss), xr, retain_graph=True)
                w_last = self.get_last_layer()
                (dw_nll,) = torch.autograd.grad(xrec, w_last, grad_outputs=g_nll, retain_graph=True)
                (dw_gan,) = torch.autograd.grad(xrec, w_last, grad_outputs=g_gan, retain_graph=True)
                n_nll, n_gan = dw_nll.float().norm(), dw_gan.float().norm()
                if s is not None:
                    n_nll, n_gan = n_nll / s, n_gan / s
                d_weight = (n_nll / (n_gan + 1e-4)).clamp(0.0, 1e4).detach() * self.disc_weight
                cb = qloss * self.codebook_weight
                # one backward of the generator from the weighted sum of the two gradients at xrec, and the codebook term
                torch.autograd.backward([xrec, scaled(cb)], [g_nll + (d_weight * f) * g_gan, None])
                # the discriminator: parameter gradients only, from the same pass
                d_loss = (A.hinge_loss(logits_real, "real") + A.hinge_loss(logits_fake, "fake")) * (0.5 * f)
                torch.autograd.backward(self.opt_d.scale_loss(d_loss), inputs=self.opt_d.groups[0].params)
            self.opt.step()
            self.opt_d.step()
        self.invalidate()
        loss = nll.detach() + d_weight * f * g_loss.detach() + cb.detach()
        terms["codebook_loss"] = cb
        terms.update(g_loss=g_loss.detach(), d_weight=d_weight, d_loss=d_loss.detach())
        terms.update(self._semantic_terms())
        terms.update(self._codebook_terms(idx))
        self.last_terms = terms
        return loss

    def discriminator_step(self, gt_img, xrec_nhwc):
        """One update of D alone on (x, a given reconstruction): d_loss = disc_factor 0.5 (mean relu(1 - D(x)) + mean relu(1 + D(xrec))).
        The generator is not touched.  Returns d_loss as a device tensor."""
        gt = gt_img.float().contiguous()
        with ops.use_precision(self.precision):
            self.opt_d.zero_grad()
            logits_real, logits_fake = self._disc_logits(gt, xrec_nhwc.detach().float().contiguous())
            d_loss = (A.hinge_loss(logits_real, "real") + A.hinge_loss(logits_fake, "fake")) * (0.5 * self.disc_factor)
            self.opt_d.scale_loss(d_loss).backward()
            self.opt_d.step()
        self.discriminator.invalidate()
        self.last_logits = (logits_real.detach(), logits_fake.detach())
        return d_loss.detach()


def stage1_loss(xrec_nhwc, gt_nchw, qloss, codebook_weight=1.0, perceptual=None, perceptual_weight=1.0):
    """total = mean |xrec - x| + codebook_weight * qloss (+ perceptual_weight * perceptual(xrec, x)) on the NHWC fp32 reconstruction.
    Returns (total, {term: float-able tensor})."""
    terms = {"l1_loss": A.l1_loss(xrec_nhwc, gt_nchw)}
    if qloss is not None:                # None: the reconstruction terms alone (the GAN step's nll)
        terms["codebook_loss"] = qloss * codebook_weight
    if perceptual is not None:
        terms["percep_loss"] = perceptual(xrec_nhwc, ops.nchw_to_nhwc(gt_nchw, bf16=False)) * perceptual_weight
    return sum(terms.values()), terms


def stage3_loss(rec_nhwc, gt_nchw, perceptual=None, use_msssim=True):
    """total = l1 + 0.01 * percep + 0.2 * (1 - msssim(sr, gt, normalize=True)) on the NHWC fp32 network output
    (VQLLFLOWD_model.py:209-223).  Returns (total, {term: float-able tensor})."""
    gt_nchw = gt_nchw.float().contiguous()
    terms = {"l1_loss": A.l1_clamp_loss(rec_nhwc, gt_nchw)}
    if perceptual is not None or use_msssim:
        sr = A.clamp01(rec_nhwc)
        gt_nhwc = ops.nchw_to_nhwc(gt_nchw, bf16=False)
        if perceptual is not None:
            terms["percep_loss"] = perceptual(sr, gt_nhwc) * 0.01
        if use_msssim:
            terms["ssim_loss"] = (1 - losses.msssim(sr, gt_nhwc, normalize=True)) * 0.2
    return sum(terms.values()), terms


class GraphedStep:
    """A training step captured once into a hipGraph (torch.cuda.CUDAGraph) and replayed: the ~5 000 kernel launches of a step
    at the reference's crop sizes are launch-bound from Python, the graph removes the host from the loop.  Needs fixed input
    shapes; inputs are copied into static buffers.  World size 1 only (a collective inside the captured region is not attempted).

    A step with a host-side decision that changes the captured kernel sequence (stage 2: mean = ground truth with probability
    train_gt_ratio, LLFlowVQGAN_arch.py:95) has one graph per branch (Trainer.graph_branches), all captured up front (capture_all):
    the decision is drawn on the host BEFORE the replay (Trainer.draw_branch) and selects the graph."""

    def __init__(self, trainer, gt_img, lr_img, warmup=3):
        self.trainer = trainer
        self.gt, self.lr = gt_img.clone(), lr_img.clone()
        self.warmup = warmup
        self.graphs = {}
        self.capture_all()

    def capture_all(self):
        """Warm up and capture EVERY branch now (stage 2: mean = color_map and mean = gt), never lazily mid-training: a capture
        bakes in host state of that moment -- the packed-filter job table of the PackCache (a branch that packs a filter the
        other never touched must have done so BEFORE any graph holds the table), allocator pools, lazily built folds.  Call again
        after `resume_training` / loading weights: the old graphs are dropped."""
        self.graphs = {}
        branches = self.trainer.graph_branches()
        self._warm_up(branches)
        self.trainer.invalidate()
        for b in branches:
            self._capture(b)

    def _warm_up(self, branches):
        # The warm-up runs REAL steps (allocator pools, lazy folds, the PackCache's job table must exist before the capture), on the
        # batch cloned at construction: the training state is snapshotted around it and put back, so that capturing -- at construction
        # or again after `resume_training` / a weight load -- never advances the optimisation (it used to apply
        # warmup x branches Adam updates on a stale batch and move the step counter and the scaler's tracker).  Only a FRESH flow's
        # ActNorm initialisation (a property of the first training forward, FlowActNorms.py:82-83) deliberately survives.
        opt = self.trainer.opt
        snap = [(t, t.clone()) for g in opt.groups for t in (g.w, g.m, g.v)]
        snap += [(t, t.clone()) for t in (opt.step_dev, opt.state3, opt.scale, opt.growth_tracker)]
        snap += [(t, t.clone()) for t in opt.ema_tensors()]      # the warm-up steps must neither seed nor advance the weight average
        actnorms = [m for m in self.trainer.netG.modules() if hasattr(m, "inited") and hasattr(m, "logs")]
        # "fresh" as FlowActNorms.py:36-38 defines it: not yet initialised AND still all-zero (a seeded / loaded ActNorm is only marked)
        fresh = {id(m) for m in actnorms if not m.inited and not bool((m.bias != 0).any())}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            keep = []
            if fresh:
                # The data-dependent initialisation happens inside the FIRST training forward (FlowActNorms.py:82-83).  It is run here on
                # its own -- a forward without backward or optimizer step -- and cloned BEFORE any warm-up step: cloned after the warm-up
                # (as this code did) the values put back were the initialisation PLUS warmup x branches Adam updates on the construction
                # batch, with their moments and the step counter rewound to zero.
                self.trainer.init_forward(self.gt, self.lr, branches[0])
                keep = [(t, t.clone()) for m in actnorms if id(m) in fresh for t in (m.bias.data, m.logs.data)]
            for _ in range(self.warmup):            # allocator / lazy-init warm-up outside the capture, every branch
                for b in branches:
                    self.trainer.step_tensor(self.gt, self.lr, b)
            for t, v in snap:
                t.copy_(v)
            for t, v in keep:                       # the parameters live inside the restored flat buffers: put the initialisation back
                t.copy_(v)
        torch.cuda.current_stream().wait_stream(side)

    def _capture(self, branch):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            loss = self.trainer.step_tensor(self.gt, self.lr, branch)
        self.graphs[branch] = (g, loss)
        # the capture only RECORDS: it must not advance the optimizer.  (Capturing runs no kernels, and the optimizer's step
        # counter lives on the device, so nothing to undo.)

    def step_tensor(self, gt_img, lr_img, mean_is_gt=None):
        branch = self.trainer.draw_branch() if mean_is_gt is None else bool(mean_is_gt)
        self.gt.copy_(gt_img)
        self.lr.copy_(lr_img)
        if branch not in self.graphs:    # a forced branch the configuration itself cannot draw (tests): captured on first use --
            self._capture(branch)        # safe, the PackCache keeps superseded job tables alive for the graphs that hold them
        g, loss = self.graphs[branch]
        g.replay()
        # the host code inside step_tensor (its invalidate()) ran at capture time only: packed inference weights built since then (a
        # validation pass between steps) would be stale after this replay
        self.trainer.invalidate()
        return loss

    def step(self, gt_img, lr_img):
        return float(self.step_tensor(gt_img, lr_img))
