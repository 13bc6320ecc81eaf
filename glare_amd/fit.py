"""Training driver: the loop around `Stage1Trainer` / `Stage2Trainer` / `Stage3Trainer` (code/train_stage2.py,
code/train_stage3.py:138-300 over models/base_model.py:46-83 and models/lr_scheduler.py:8-34), fed by a device-resident dataset
(glare_amd.data.DeviceLoLDataset).

    python -m glare_amd.fit stage1 --root LOLdataset --out prior [--net-vq start.pth]
    python -m glare_amd.fit stage3 --root LOLdataset --out run --net-g stage2_G.pth --net-vq vqgan.pkl
    python -m glare_amd.fit stage3 --root LOLdataset --out run --resume run/training_state/500.state
    python -m glare_amd.fit stage1 --root LOLdataset --out prior --vgg16 vgg16.pth --lpips-heads vgg.pth [--gan]
    python -m glare_amd.fit stage3 --root LOLdataset --out run --net-g stage2_G.pth --net-vq vqgan.pkl --vgg16 vgg16.pth
    python -m glare_amd.fit stage1 --root LOLdataset --out prior --codebook-usage        (log the codebook's use; glare_amd.evaluate stage1 scores the run)
    python -m glare_amd.fit stage1 --root LOLdataset --out prior --codebook-restart 100  (every 100 steps, re-seed the codes nothing selected)
    python -m glare_amd.fit stage1 --root LOLdataset --out prior --codebook-ema 0.99 --codebook-restart 100   (an EMA codebook, no gradient)
    python -m glare_amd.fit stage1 --root LOLdataset --out prior --vgg19 vgg19-dcbb9e9d.pth [--semantic-weight 0.1]   (semantic guidance)
    python -m glare_amd.fit stage3 --root LOLdataset --out run --net-g stage2_G.pth --net-vq vqgan.pkl --weights-ema 0.999   (averaged weights)

Stage 1 trains the VQGAN prior itself (VQModel_arch.py:98-101, 148-157) on the ground-truth half of the pairs and writes
<out>/models/<iter>_VQ.pth under the reference's VQModel key names: what `--net-vq` of stages 2 and 3, `evaluate` and `enhance` load.
--vgg16 / --lpips-heads add the perceptual terms of the reference's objectives from the user's weight files (stage 1: LPIPS on VGG16, both
files; stage 3: the VGG16-feature loss, --vgg16 alone; losses.load_vgg16 refuses a file that lacks a tensor).  The loss networks are frozen and
are written to no checkpoint: a resumed run names the same files again (the .state records that the run had the term, and a resume
without it, or with another --perceptual-weight, is refused).
--vgg19 adds stage 1's semantic guidance term (VQModel_arch.py:85-88: the codes through conv_semantic against VGG19 relu3_4 of the input)
from the user's VGG19 file (losses.load_vgg19, strict); the same rules hold for it: frozen, in no checkpoint, named again on a resume.
--weights-ema keeps an exponential moving average of the trained weights on the device (every stage; BaseModel.model_ema of the stage-1
lineage, basicsr/models/base_model.py:85-92): every checkpoint gains <iter>_G_ema.pth (stage 1: <iter>_VQ_ema.pth), a plain state dict under
the network's own key names, every validation a second result `val_ema` scored under the averaged weights, and a resume continues the
average from that file (and is refused, by the file's name, where it is missing).
The reference ships no stage-1 configuration (its prior is a download): `lr_G` 1e-4 is a starting point, not a tuned value.

What is mirrored: the option keys and their per-stage values, the seeding, the index order of the reference's DataLoader, the
augmentation draws, the learning-rate schedule with its warm-up override, the checkpoint cadence and the two checkpoint files
(glare_amd.checkpoint: interchangeable with the reference's).  What is not: its logging stack (one JSON line per print_freq
instead) and its validation block (dead code at the shipped val_freq; validation here is glare_amd.infer over the test split).
World size 1."""
import argparse
import copy
import json
import os
import random
import time
from collections import Counter

import numpy as np
import torch

from . import checkpoint, train

# confs/train_stage2_LOL.yml / confs/train_stage3_LOL.yml, the keys this driver reads, restated
_COMMON_TRAIN = {"manual_seed": 10, "weight_decay_G": 0, "beta1": 0.9, "beta2": 0.99, "lr_scheme": "MultiStepLR", "warmup_iter": 10,
                 "lr_steps_rel": [0.5, 0.75, 0.9, 0.95], "lr_gamma": 0.5, "val_freq": 0}
_COMMON_DATA = {"use_shuffle": True, "use_flip": True, "use_crop": True, "use_rot": False, "noise_prob": 0, "noise_level": 5, "log_low": True,
                "gamma_aug": False}
DEFAULTS = {
    # no file of the reference: its stage-1 network and optimizer are VQModel_arch.py:98-101, 148-157 (Adam, betas (0.5, 0.9)); crop,
    # batch, lr and schedule are this driver's starting point
    "stage1": {"name": "train_stage1_LOL", "model": "VQModel", "train_gt_ratio": 0.0,
               "datasets": {"train": dict(_COMMON_DATA, batch_size=4, GT_size=256), "val": {"log_low": True}},
               "network_G": {"train_RRDB": False},
               "train": dict(_COMMON_TRAIN, beta1=0.5, beta2=0.9, lr_G=1e-4, niter=80000, codebook_weight=1.0),
               "logger": {"print_freq": 10, "save_checkpoint_freq": 1000}},
    "stage2": {"name": "train_stage2_LOL", "model": "LLFlow", "train_gt_ratio": 0.2,
               "datasets": {"train": dict(_COMMON_DATA, batch_size=4, GT_size=320), "val": {"log_low": True}},
               "network_G": {"train_RRDB": False},
               "train": dict(_COMMON_TRAIN, lr_G=5e-4, niter=80000),
               "logger": {"print_freq": 10, "save_checkpoint_freq": 1000}},
    "stage3": {"name": "train_stage3_LOL", "model": "VQLLFLOWD", "train_gt_ratio": 0.0,
               "datasets": {"train": dict(_COMMON_DATA, batch_size=2, GT_size=256), "val": {"log_low": True}},
               "network_G": {"train_RRDB": False},
               "train": dict(_COMMON_TRAIN, lr_G=5e-5, niter=40000),
               "logger": {"print_freq": 5, "save_checkpoint_freq": 500}},
}
DISC_KEY = train.DISC_KEY    # --gan: {"optimizer": Adam state dict, "scaler": GradScaler state dict} of the discriminator (Stage1Trainer)
STATE_KEY = "glare_fit"      # the extra key of a `.state` file: RNG states and the place in the epoch (the reference ignores it)
STEADY_FROM = 20             # the closing summary's ms per step leaves out this many steps


def default_options(stage):
    return copy.deepcopy(DEFAULTS[stage])


def merge_options(opt, override):
    """Nested dict update: `override` wins key by key (an --opt file names only what it changes)."""
    for k, v in override.items():
        if isinstance(v, dict) and isinstance(opt.get(k), dict):
            merge_options(opt[k], v)
        else:
            opt[k] = v
    return opt


def load_options_file(path):
    if path.endswith((".yml", ".yaml")):
        try:
            import yaml
        except ImportError:
            raise RuntimeError("%s: PyYAML is not installed; pass the options as a .json file" % path)
        with open(path) as f:
            return yaml.safe_load(f)
    with open(path) as f:
        return json.load(f)


def set_random_seed(seed):
    """utils/util.py set_random_seed."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)


class MultiStepSchedule:
    """`MultiStepLR_Restart` at the shipped settings (restarts [0], weights [1], no inverse steps) = torch's MultiStepLR in its
    chainable form, plus BaseModel.update_learning_rate's warm-up override, over the groups of a FlatAdam.  `lrs` is what
    `optimizer.param_groups[i]['lr']` holds in the reference; it reaches the kernels as ONE device scalar (FlatAdam.set_lr_scale:
    every group's lr moves by the same factor).  state_dict() carries torch's field names, so a `.state` file round-trips.

    As in the reference, the override writes the group's lr and the scheduler then keeps multiplying THAT value: after the warm-up the
    lr stays at initial_lr * (warmup_iter - 1) / warmup_iter until the first milestone."""

    def __init__(self, opt, milestones, gamma, warmup_iter=-1):
        self.opt = opt
        self.milestones = Counter(int(m) for m in milestones)
        self.gamma = gamma
        self.warmup_iter = warmup_iter
        self.base_lrs = [g.lr for g in opt.groups]
        self.lrs = list(self.base_lrs)
        self.last_epoch = 0            # torch's constructor performs the initial step
        self._step_count = 1
        self._last_lr = list(self.lrs)
        self._scale = None

    def update(self, cur_iter):
        """update_learning_rate(cur_iter, warmup_iter): one scheduler step, then the warm-up override; returns group 0's lr."""
        self.last_epoch += 1
        self._step_count += 1
        if self.last_epoch in self.milestones:
            self.lrs = [lr * self.gamma ** self.milestones[self.last_epoch] for lr in self.lrs]
        self._last_lr = list(self.lrs)
        if cur_iter < self.warmup_iter:
            self.lrs = [v / self.warmup_iter * cur_iter for v in self.base_lrs]
        self.apply()
        return self.lrs[0]

    def apply(self):
        scale = self.lrs[0] / self.base_lrs[0] if self.base_lrs[0] else 0.0
        if scale != self._scale:             # a device write only when the factor moves: the warm-up steps and the milestones
            self.opt.set_lr_scale(scale)
            self._scale = scale

    def state_dict(self):
        return {"milestones": Counter(self.milestones), "gamma": self.gamma, "base_lrs": list(self.base_lrs), "last_epoch": self.last_epoch,
                "_step_count": self._step_count, "_get_lr_called_within_step": False, "_last_lr": list(self._last_lr)}

    def load_state_dict(self, sd):
        self.milestones, self.gamma = Counter(sd["milestones"]), sd["gamma"]
        self.base_lrs, self.last_epoch, self._step_count = list(sd["base_lrs"]), sd["last_epoch"], sd["_step_count"]
        self._last_lr = list(sd.get("_last_lr", self.base_lrs))

    # a `.state` file holds each group's CURRENT lr in its optimizer entry (torch's param_groups[i]['lr']); FlatGroup.lr is the base
    def _swap_in_current(self):
        for g, lr in zip(self.opt.groups, self.lrs):
            g.lr = lr

    def _swap_in_base(self):
        for g, lr in zip(self.opt.groups, self.base_lrs):
            g.lr = lr

    def adopt_loaded(self):
        """After checkpoint.resume_training: the groups' lr just loaded is the current one."""
        self.lrs = [g.lr for g in self.opt.groups]
        self._swap_in_base()
        self._scale = None
        self.apply()


def make_schedule(opt, options):
    tr = options["train"]
    assert tr.get("lr_scheme", "MultiStepLR") == "MultiStepLR", "only MultiStepLR is built"
    niter = int(tr["niter"])
    return MultiStepSchedule(opt, [int(x * niter) for x in tr["lr_steps_rel"]], tr["lr_gamma"], tr.get("warmup_iter", -1))


def epoch_batches(n, batch_size):
    """The index batches of one epoch, in the order `DataLoader(dataset, batch_size, shuffle=True, drop_last=True)` yields them
    for the same state of torch's default generator: its iterator draws a base seed first, then the RandomSampler seeds its own
    generator -- two draws per epoch."""
    torch.empty((), dtype=torch.int64).random_()
    sampler = torch.utils.data.BatchSampler(torch.utils.data.RandomSampler(range(n)), batch_size, drop_last=True)
    return [list(map(int, b)) for b in sampler]


def _rng_state():
    py = random.getstate()
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    return {"python": [py[0], list(py[1]), py[2]], "numpy": [kind, torch.from_numpy(keys.astype(np.int64)), int(pos), int(has_gauss), float(cached)],
            "torch": torch.get_rng_state()}


def _set_rng_state(st):
    py = st["python"]
    random.setstate((py[0], tuple(py[1]), py[2]))
    kind, keys, pos, has_gauss, cached = st["numpy"]
    np.random.set_state((kind, keys.numpy().astype(np.uint32), pos, has_gauss, cached))
    torch.set_rng_state(st["torch"])


def _sync():
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def fit(options, trainer, dataset, out_dir, step_fn=None, batch_fn=None, resume=None, validate_fn=None, log=None):
    """The loop.  trainer: a train.Trainer; dataset: `len()` and `.batch(indices)`.  step_fn(gt, lq) -> loss (device
    tensor, default trainer.step_tensor) and batch_fn(indices) -> (gt, lq) (default dataset.batch) are injectable, as is
    validate_fn(iter) -> dict.  Returns the list of records it logged (one per print_freq, plus the closing summary)."""
    step_fn = step_fn or trainer.step_tensor
    batch_fn = batch_fn or dataset.batch
    log = log or (lambda rec: print(json.dumps(rec), flush=True))
    tr, lg = options["train"], options["logger"]
    niter, batch_size = int(tr["niter"]), int(options["datasets"]["train"]["batch_size"])
    print_freq, save_freq, val_freq = int(lg["print_freq"]), int(lg["save_checkpoint_freq"]), int(tr.get("val_freq") or 0)
    n = len(dataset)
    assert n >= batch_size, "%d training pairs cannot fill a batch of %d (drop_last)" % (n, batch_size)
    os.makedirs(os.path.join(out_dir, "models"), exist_ok=True)
    os.makedirs(os.path.join(out_dir, "training_state"), exist_ok=True)
    trainer.opt.betas = (tr["beta1"], tr["beta2"])          # FlatAdam's own default is torch's 0.999
    sched = make_schedule(trainer.opt, options)
    set_random_seed(tr["manual_seed"])
    epoch, step, order, done = 0, 0, None, 0
    percep = trainer.objective_tag()                               # the loss network travels in no file; which one it was does
    if resume:
        st = torch.load(resume, map_location="cpu", weights_only=False) if isinstance(resume, str) else resume
        if STATE_KEY in st and st[STATE_KEY].get("perceptual") != percep:
            raise ValueError(PERCEPTUAL_RESUME_REFUSAL % (st[STATE_KEY].get("perceptual") or "no perceptual term", percep or "none"))
        epoch, step = checkpoint.resume_training(st, trainer, [sched])
        sched.adopt_loaded()
        if STATE_KEY in st:                  # written by this driver: continue the exact index / augmentation sequence
            _set_rng_state(st[STATE_KEY]["rng"])
            order, done = st[STATE_KEY]["epoch_order"], st[STATE_KEY]["batches_done"]
        trainer.on_resume(step)
        trainer.load_extra_state(st)

    def save(epoch, step, order, done):
        # <iter>_G.pth (stage 1: <iter>_VQ.pth, the file `--net-vq` takes) and whatever further networks the trainer has (--gan: <iter>_D.pth)
        for tag, net in {trainer.checkpoint_tag: trainer.netG, **trainer.extra_networks()}.items():
            checkpoint.save_network(net, os.path.join(out_dir, "models", "%d_%s.pth" % (step, tag)))
        extra = {STATE_KEY: {"rng": _rng_state(), "epoch_order": order, "batches_done": done}, **trainer.extra_state()}
        if percep:   # (a run without the term writes the state it always wrote)
            extra[STATE_KEY]["perceptual"] = percep
        sched._swap_in_current()
        try:
            checkpoint.save_training_state(os.path.join(out_dir, "training_state", "%d.state" % step), trainer, epoch, step, [sched],
                                           extra=extra)
        finally:
            sched._swap_in_base()

    records, first = [], step
    t_win, n_win, t_batch, t_steady, last_loss, saved_at = time.perf_counter(), 0, 0.0, None, None, None
    while step < niter:
        if order is None:
            order, done = epoch_batches(n, batch_size), 0
        while done < len(order) and step < niter:
            indices = order[done]
            done += 1
            step += 1
            lr = sched.update(step)
            t0 = time.perf_counter()
            gt, lq = batch_fn(indices)
            t_batch += time.perf_counter() - t0
            last_loss = step_fn(gt, lq)
            n_win += 1
            rec = None
            if step % print_freq == 0 or step == niter:
                loss = float(last_loss)                     # the window's one device -> host read
                now = time.perf_counter()
                rec = {"epoch": epoch, "iter": step, "lr": lr, "loss": loss, "ms_per_step": 1e3 * (now - t_win) / n_win,
                       "ms_batch": 1e3 * t_batch / n_win}
                rec.update((k, float(trainer.last_terms[k])) for k in trainer.log_terms())
            if step - first == STEADY_FROM:
                _sync()
                t_steady = time.perf_counter()
            if validate_fn is not None and ((val_freq and step % val_freq == 0) or step == niter):
                rec = rec or {"epoch": epoch, "iter": step, "lr": lr}
                rec["val"] = validate_fn(step)
                if trainer.weights_ema is not None:         # the same score under the averaged weights
                    with trainer.ema_weights():
                        rec["val_ema"] = validate_fn(step)
            if step % save_freq == 0 or step == niter:
                save(epoch, step, order, done)
                saved_at = step
            if rec is not None:
                records.append(rec)
                log(rec)
                t_win, n_win, t_batch = time.perf_counter(), 0, 0.0       # validation and checkpoint time stay out of the next window
        if done >= len(order):
            order, epoch = None, epoch + 1
    _sync()
    summary = {"done": True, "iter": step, "epochs": epoch, "last_checkpoint": saved_at}
    if t_steady is not None and step - first > STEADY_FROM:
        summary["ms_per_step_after_%d" % STEADY_FROM] = 1e3 * (time.perf_counter() - t_steady) / (step - first - STEADY_FROM)
    records.append(summary)
    log(summary)
    return records


# ---- the command ---------------------------------------------------------------------------------------------------------------
def check_perceptual_options(stage, vgg16=None, lpips_heads=None, perceptual_weight=None):
    """The refusals of --vgg16 / --lpips-heads / --perceptual-weight: ValueError with the reason, before anything is built."""
    if stage == "stage2" and (vgg16 or lpips_heads or perceptual_weight is not None):
        raise ValueError(PERCEPTUAL_STAGE2_REFUSAL)
    if stage == "stage3" and (lpips_heads or perceptual_weight is not None):
        raise ValueError(PERCEPTUAL_STAGE3_REFUSAL)
    if stage == "stage1" and bool(vgg16) != bool(lpips_heads):
        raise ValueError(LPIPS_REFUSAL)
    if stage == "stage1" and perceptual_weight is not None and not vgg16:
        raise ValueError("--perceptual-weight needs --vgg16 and --lpips-heads: without them stage1 has no perceptual term to weigh")


def check_semantic_options(stage, vgg19=None, semantic_weight=None):
    """The refusals of --vgg19 / --semantic-weight: ValueError with the reason, before anything is built."""
    if stage != "stage1" and (vgg19 or semantic_weight is not None):
        raise ValueError(SEMANTIC_REFUSAL)
    if semantic_weight is not None and not vgg19:
        raise ValueError("--semantic-weight needs --vgg19: without the VGG19 file stage1 has no semantic term to weigh")


def check_restart_options(stage, codebook_restart=0, restart_threshold=None):
    """The refusals of --codebook-restart / --restart-threshold: ValueError with the reason, before anything is built."""
    if stage != "stage1" and (codebook_restart or restart_threshold is not None):
        raise ValueError(CODEBOOK_RESTART_REFUSAL)
    if codebook_restart is not None and int(codebook_restart) < 0:
        raise ValueError("--codebook-restart takes the number of steps between two restarts (0: off), not %d" % codebook_restart)
    if restart_threshold is not None and not codebook_restart:
        raise ValueError("--restart-threshold needs --codebook-restart: without it no code is ever re-seeded")
    if restart_threshold is not None and int(restart_threshold) < 0:
        raise ValueError("--restart-threshold is a token count (a code is dead at <= that many selections in a window), not %d" % restart_threshold)


def check_weights_ema_option(weights_ema=None):
    """The refusal of --weights-ema: ValueError with the reason, before anything is built."""
    if weights_ema is not None and not 0.0 <= float(weights_ema) < 1.0:
        raise ValueError(WEIGHTS_EMA_REFUSAL % (weights_ema,))


def check_ema_options(stage, codebook_ema=None, ema_eps=None):
    """The refusals of --codebook-ema / --ema-eps: ValueError with the reason, before anything is built."""
    if stage != "stage1" and (codebook_ema is not None or ema_eps is not None):
        raise ValueError(CODEBOOK_EMA_REFUSAL)
    if codebook_ema is not None and not 0.0 < float(codebook_ema) < 1.0:
        raise ValueError("--codebook-ema takes the decay of the moving average, a number in (0, 1) such as 0.99, not %r" % (codebook_ema,))
    if ema_eps is not None and codebook_ema is None:
        raise ValueError("--ema-eps needs --codebook-ema: without it the codebook follows its gradient and no cluster size is smoothed")
    if ema_eps is not None and not float(ema_eps) >= 0.0:
        raise ValueError("--ema-eps is the smoothing added to every cluster size (default 1e-5), not %r" % (ema_eps,))


def build_perceptual(stage, device, vgg16=None, lpips_heads=None):
    """The frozen loss network of the stage from the user's files (losses.load_vgg16, strict; `.loaded_keys`: what it loaded), or None
    without --vgg16."""
    from . import losses

    if not vgg16:
        return None
    net = losses.LPIPSLoss() if stage == "stage1" else losses.PerceptualNetwork()
    net.loaded_keys = losses.load_vgg16(net, vgg16, lpips_heads)
    return net.to(device).eval()


def build_semantic(device, vgg19=None):
    """Stage 1's frozen VGG19 relu3_4 extractor from the user's file (losses.load_vgg19, strict; `.loaded_keys`: what it loaded), or None
    without --vgg19."""
    from . import losses

    if not vgg19:
        return None
    net = losses.SemanticTarget()
    net.loaded_keys = losses.load_vgg19(net, vgg19)
    return net.to(device).eval()


def build_trainer(stage, options, device, net_g=None, net_vq=None, graph=False, precision="fp16", gan=False, net_d=None, vgg16=None,
                  lpips_heads=None, perceptual_weight=None, codebook_usage=False, codebook_restart=0, restart_threshold=None,
                  codebook_ema=None, ema_eps=None, vgg19=None, semantic_weight=None, weights_ema=None):
    """Networks (name-seeded unless checkpoint files are given, as glare_amd.infer) and the stage's trainer.  gan (stage 1 only): with the
    patch discriminator (taming's initialisation under the run's seed, or the `_D.pth` file net_d).  vgg16 / lpips_heads: the weight
    files of the perceptual term (stage 1: LPIPS, both files; stage 3: the VGG16-feature loss, the backbone alone); perceptual_weight:
    stage 1's factor on it (default 1.0).  The loss network is frozen and is written to no checkpoint: a resumed run names the files again.
    codebook_usage, codebook_restart / restart_threshold, codebook_ema / ema_eps (stage 1 only): Stage1Trainer's; off, the trainer is built
    without the keywords.  vgg19 / semantic_weight (stage 1 only): the VGG19 file of the semantic guidance term and its factor (default 0.1);
    frozen and in no checkpoint like the perceptual network.  weights_ema (every stage): Trainer's decay of the averaged weights."""
    from . import modules as M

    check_perceptual_options(stage, vgg16, lpips_heads, perceptual_weight)
    check_semantic_options(stage, vgg19, semantic_weight)
    tr = options["train"]
    perceptual = build_perceptual(stage, device, vgg16, lpips_heads)       # None without the options: the trainers' own default
    if stage == "stage1" and graph:
        raise ValueError(GRAPH_REFUSAL)
    if stage != "stage1" and gan:
        raise ValueError(GAN_REFUSAL)
    if stage != "stage1" and codebook_usage:
        raise ValueError(CODEBOOK_USAGE_REFUSAL)
    check_restart_options(stage, codebook_restart, restart_threshold)
    check_ema_options(stage, codebook_ema, ema_eps)
    check_weights_ema_option(weights_ema)
    averaged = {} if weights_ema is None else {"weights_ema": float(weights_ema)}
    netG, net_hq = checkpoint.build_nets(stage, True, net_g, net_vq, options, device)
    if stage == "stage1":
        disc = None
        if gan:
            set_random_seed(tr["manual_seed"])       # N(0, 0.02) / N(1, 0.02): the same discriminator for the same seed
            disc = M.NLayerDiscriminator()
            if net_d:
                checkpoint.load_network(net_d, disc, strict=True)
            disc = disc.to(device)
        return train.Stage1Trainer(netG, lr_G=tr["lr_G"], weight_decay_G=tr.get("weight_decay_G", 0),
                                   codebook_weight=tr.get("codebook_weight", 1.0), precision=precision, discriminator=disc,
                                   disc_start=tr.get("disc_start", 10000), disc_weight=tr.get("disc_weight", 0.8),
                                   disc_factor=tr.get("disc_factor", 1.0), perceptual=perceptual,
                                   perceptual_weight=1.0 if perceptual_weight is None else float(perceptual_weight),
                                   **({"codebook_usage": True} if codebook_usage else {}),
                                   **({"codebook_restart": int(codebook_restart), "restart_threshold": int(restart_threshold or 0)}
                                      if codebook_restart else {}),
                                   **({"codebook_ema": float(codebook_ema), "ema_eps": 1e-5 if ema_eps is None else float(ema_eps)}
                                      if codebook_ema is not None else {}),
                                   **({"semantic": build_semantic(device, vgg19),
                                       "semantic_weight": 0.1 if semantic_weight is None else float(semantic_weight)} if vgg19 else {}),
                                   **averaged)
    if stage == "stage2":
        return train.Stage2Trainer(netG, net_hq, lr_G=tr["lr_G"], lr_RRDB=tr.get("lr_RRDB"), weight_decay_G=tr.get("weight_decay_G", 0),
                                   train_rrdb=bool(options["network_G"].get("train_RRDB", False)), precision=precision, **averaged)
    return train.Stage3Trainer(netG, net_hq, lr_G=tr["lr_G"], weight_decay_G=tr.get("weight_decay_G", 0), precision=precision,
                               perceptual=perceptual, **averaged)


CODEBOOK_USAGE_REFUSAL = ("--codebook-usage is a stage1 option: stage1 is the stage that trains the codebook (stages 2 and 3 read a frozen one; "
                          "glare_amd.evaluate stage1 reports the use of a finished prior's)")
CODEBOOK_RESTART_REFUSAL = ("--codebook-restart / --restart-threshold are stage1 options: stage1 is the stage that trains the codebook (stages 2 "
                            "and 3 read a frozen one, which has no dead codes to revive)")
CODEBOOK_EMA_REFUSAL = ("--codebook-ema / --ema-eps are stage1 options: stage1 is the stage that trains the codebook (stages 2 and 3 read a "
                        "frozen one, which nothing updates)")
SEMANTIC_REFUSAL = ("--vgg19 / --semantic-weight are stage1 options: the semantic guidance term belongs to the VQGAN prior's codebook loss "
                    "(VQModel_arch.py:85-88); stages 2 and 3 read a frozen prior")
WEIGHTS_EMA_REFUSAL = ("--weights-ema takes the decay of the moving average of the trained weights, a number in [0, 1) such as 0.999, not %r")
GAN_REFUSAL = "--gan is a stage1 option: the patch discriminator belongs to the VQGAN prior's objective (stages 2 and 3 train no GAN term)"
LPIPS_REFUSAL = ("stage1's perceptual term is LPIPS and needs both files: --vgg16 (the VGG16 backbone) and --lpips-heads (the five linear "
                 "heads, taming's / the lpips package's vgg.pth); one without the other would leave half the network at its initialisation")
PERCEPTUAL_STAGE3_REFUSAL = ("--lpips-heads / --perceptual-weight are stage1 options: stage3's perceptual term is the VGG16-feature MSE with its "
                             "fixed factor 0.01 (VQLLFLOWD_model.py:217-223) and takes --vgg16 alone")
PERCEPTUAL_RESUME_REFUSAL = ("the .state file was written by a run with %s and this one has %s: the objective would change partway through "
                             "the run; name the same --vgg16 / --lpips-heads / --perceptual-weight / --vgg19 / --semantic-weight again (the loss networks are in "
                             "no checkpoint)")
PERCEPTUAL_STAGE2_REFUSAL = "--vgg16 / --lpips-heads / --perceptual-weight are stage1 / stage3 options: stage2's objective is the flow's NLL alone"
GRAPH_REFUSAL = "--graph is not available for stage1: its step is not captured into a hipGraph (GraphedStep covers stages 2 and 3)"


def graphed_fns(trainer, dataset):
    """(step_fn, batch_fn) that replay the step from a hipGraph: the GraphedStep is built on the first batch (after any resume, as
    its capture_all() asks), and from then on batch() writes straight into its static inputs."""
    box = []

    def batch_fn(indices):
        return dataset.batch(indices, out_gt=box[0].gt, out_lq=box[0].lr) if box else dataset.batch(indices)

    def step_fn(gt, lq):
        if not box:
            box.append(train.GraphedStep(trainer, gt, lq))
        g = box[0]
        return g.step_tensor(g.gt, g.lr)

    return step_fn, batch_fn


def make_validate(trainer, test_ds, precision, batch=8):
    """PSNR / SSIM of the test split through the inference path (glare_amd.infer.run), images grouped by size."""
    from . import infer

    groups = {}
    for low, high, _ in test_ds.pairs:
        groups.setdefault(low.shape, []).append((low, high))

    def validate(step):
        was_training = trainer.netG.training
        trainer.netG.eval()
        rows = []
        try:
            for pairs in groups.values():
                lows, gts = np.stack([p[0] for p in pairs]), np.stack([p[1] for p in pairs])
                rows.append(np.asarray(infer.run(len(pairs), batch=batch, pairs=(lows, gts), nets=(trainer.netG, trainer.net_hq), with_ssim=True,
                                                 precision=precision)).reshape(len(pairs), 2))
        finally:
            trainer.netG.train(was_training)
        rows = np.concatenate(rows)
        return {"images": int(len(rows)), "psnr": float(rows[:, 0].mean()), "ssim": float(rows[:, 1].mean())}

    return validate


def make_validate_stage1(trainer, test_ds, precision):
    """Mean PSNR of decode(encode(gt)) over the test split's ground-truth images, through the inference kernels (VQModel.encode_nhwc /
    decode_nhwc as stages 2 and 3 call them); an image whose sides are no multiple of 4 (the encoder's stride) is padded at the
    bottom / right by reflection and scored on its own window.  uint8 PSNR as glare_amd.evaluate (harness.score_device / psnr_u8): the
    protocol is evaluate.stage1_reconstruct, one image at a time.  A trainer built with codebook_usage=True also gets `codebook`, the use of
    the codebook over every token of the split ({tokens, active, active_fraction, perplexity}, metrics.CodebookUsage)."""
    from . import evaluate, harness, metrics

    def validate(step):
        net = trainer.netG
        was_training = net.training
        net.eval()
        vals = []
        usage = metrics.CodebookUsage(net.quantize.n_e, next(net.parameters()).device) if getattr(trainer, "codebook_usage", False) else None
        try:
            with torch.no_grad():
                for _, high, _ in test_ds.pairs:
                    h, w = high.shape[:2]
                    _, _, _, sse, idx = evaluate.stage1_reconstruct(net, high[None], precision)
                    if usage is not None:
                        usage.update(idx)
                    vals.append(harness.psnr_u8(int(sse[0]), 3 * h * w))
        finally:
            net.train(was_training)
        res = {"images": len(vals), "psnr": float(np.mean(vals))}
        if usage is not None:
            res["codebook"] = {k: v for k, v in usage.stats().items() if k in evaluate.USAGE_KEYS}
        return res

    return validate


def parse_args(argv=None):
    """The command line -> (args, options): the stage's defaults, the --opt file over them, the single-key switches over that."""
    from . import data as D

    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("stage", choices=("stage1", "stage2", "stage3"))
    ap.add_argument("--root", required=True, help="dataset folder (v1: <root>/our485|eval15/{low,high}; v2: see --layout)")
    ap.add_argument("--out", required=True, help="run folder: <out>/models/<iter>_G.pth, <out>/training_state/<iter>.state")
    ap.add_argument("--layout", choices=sorted(D.LAYOUTS), default="v1")
    ap.add_argument("--opt", default=None, help="options file (.json; .yml where PyYAML is installed) overriding the stage's defaults")
    ap.add_argument("--niter", type=int, default=None)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--save-freq", type=int, default=None)
    ap.add_argument("--val-freq", type=int, default=None, help="validate every N steps (default 0: only after the last step)")
    ap.add_argument("--resume", default=None, help="a .state file; the weights come from models/<iter>_G.pth (stage1: <iter>_VQ.pth) next to it "
                                                   "unless --net-g (stage1: --net-vq) is given")
    ap.add_argument("--net-g", default=None, help="net_G checkpoint (reference format)")
    ap.add_argument("--net-vq", default=None, help="VQGAN checkpoint (reference format); stage1: the weights to start from")
    ap.add_argument("--graph", action="store_true", help="replay the step from a hipGraph (GraphedStep; stages 2 and 3)")
    ap.add_argument("--precision", choices=("fp16", "bf16"), default="fp16")
    ap.add_argument("--gan", action="store_true", help="stage1: add the patch discriminator (hinge loss, adaptive weight); writes <iter>_D.pth")
    ap.add_argument("--disc-start", type=int, default=None, help="--gan: first step whose loss has the GAN term (default 10000)")
    ap.add_argument("--disc-weight", type=float, default=None, help="--gan: factor on the adaptive weight (default 0.8)")
    ap.add_argument("--vgg16", default=None, help="VGG16 weights (torchvision's vgg16 state dict; also PerceptualNetwork's or LPIPS's key form): "
                                                  "stage1 with --lpips-heads: the LPIPS term; stage3: the VGG16-feature perceptual term")
    ap.add_argument("--lpips-heads", default=None, help="stage1: the LPIPS linear heads (taming's / the lpips package's vgg.pth)")
    ap.add_argument("--perceptual-weight", type=float, default=None, help="stage1: factor on the LPIPS term (default 1.0)")
    ap.add_argument("--vgg19", default=None, help="stage1: VGG19 weights (torchvision's vgg19 state dict, vgg19-dcbb9e9d.pth; also the key form "
                                                  "vgg_net.convX_Y): adds the semantic guidance term on the codebook (relu3_4)")
    ap.add_argument("--semantic-weight", type=float, default=None, help="--vgg19: factor on the semantic term inside the codebook loss (default 0.1)")
    ap.add_argument("--codebook-usage", action="store_true", help="stage1: log codebook_active / codebook_perplexity of every step's indices, and "
                                                                   "the test split's codebook use with the closing validation")
    ap.add_argument("--codebook-restart", type=int, default=0, metavar="P",
                    help="stage1: every P steps, re-seed the codes that no token selected since the last restart from the step's encoder outputs")
    ap.add_argument("--restart-threshold", type=int, default=None, metavar="T",
                    help="--codebook-restart: a code is dead when at most T tokens selected it in the window (default 0)")
    ap.add_argument("--codebook-ema", type=float, default=None, metavar="DECAY",
                    help="stage1: move the codebook by an exponential moving average of the latents that select each code (decay in (0, 1), "
                         "e.g. 0.99) instead of its gradient; use with --codebook-restart, a code nothing selects is thrown far away")
    ap.add_argument("--ema-eps", type=float, default=None, metavar="EPS", help="--codebook-ema: the smoothing of the cluster sizes (default 1e-5)")
    ap.add_argument("--weights-ema", type=float, default=None, metavar="DECAY",
                    help="keep an exponential moving average of the trained weights on the device (decay in [0, 1), e.g. 0.999): every checkpoint "
                         "gains <iter>_G_ema.pth (stage1: <iter>_VQ_ema.pth) and every validation `val_ema`")
    ap.add_argument("--no-val", action="store_true", help="skip the closing validation")
    args = ap.parse_args(argv)
    if args.codebook_usage and args.stage != "stage1":
        ap.error(CODEBOOK_USAGE_REFUSAL)
    if args.graph and args.stage == "stage1":
        ap.error(GRAPH_REFUSAL)
    if args.gan and args.stage != "stage1":
        ap.error(GAN_REFUSAL)
    if not args.gan and (args.disc_start is not None or args.disc_weight is not None):
        ap.error("--disc-start / --disc-weight need --gan")
    try:
        check_restart_options(args.stage, args.codebook_restart, args.restart_threshold)
        check_ema_options(args.stage, args.codebook_ema, args.ema_eps)
        check_weights_ema_option(args.weights_ema)
        check_perceptual_options(args.stage, args.vgg16, args.lpips_heads, args.perceptual_weight)
        check_semantic_options(args.stage, args.vgg19, args.semantic_weight)
    except ValueError as e:
        ap.error(str(e))

    options = default_options(args.stage)
    if args.opt:
        merge_options(options, load_options_file(args.opt))
    for value, (section, key) in ((args.niter, ("train", "niter")), (args.val_freq, ("train", "val_freq")),
                                  (args.save_freq, ("logger", "save_checkpoint_freq")), (args.disc_start, ("train", "disc_start")),
                                  (args.disc_weight, ("train", "disc_weight"))):
        if value is not None:
            options[section][key] = value
    if args.batch is not None:
        options["datasets"]["train"]["batch_size"] = args.batch
    return args, options


def main(argv=None):
    from . import data as D

    args, options = parse_args(argv)
    assert torch.cuda.is_available(), "glare_amd.fit needs an MI355X: the HIP kernels are the only implementation"
    device = torch.device("cuda", 0)
    net_g, net_vq, net_d = args.net_g, args.net_vq, None
    resume, net_ema = None, None
    if args.resume:
        resume = torch.load(args.resume, map_location="cpu", weights_only=False)
        models = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(args.resume))), "models")
        if args.stage == "stage1":
            net_vq = net_vq or os.path.join(models, "%d_VQ.pth" % resume["iter"])
            net_d = os.path.join(models, "%d_D.pth" % resume["iter"]) if args.gan else None
        elif net_g is None:
            net_g = os.path.join(models, "%d_G.pth" % resume["iter"])
        if args.weights_ema is not None:      # the average continues from the file written beside the weights
            net_ema = os.path.join(models, "%d_%s%s.pth" % (resume["iter"], "VQ" if args.stage == "stage1" else "G", train.EMA_SUFFIX))
            if not os.path.exists(net_ema):
                raise ValueError(train.EMA_RESUME_REFUSAL % net_ema)
    train_opt = dict(options["datasets"]["train"], root=args.root)
    host_ds = D.LAYOUTS[args.layout](train_opt, train=True, all_opt=options)
    dataset = D.DeviceLoLDataset(host_ds, device)
    trainer = build_trainer(args.stage, options, device, net_g, net_vq, args.graph, args.precision, gan=args.gan, net_d=net_d,
                            vgg16=args.vgg16, lpips_heads=args.lpips_heads, perceptual_weight=args.perceptual_weight,
                            codebook_usage=args.codebook_usage, codebook_restart=args.codebook_restart, restart_threshold=args.restart_threshold,
                            codebook_ema=args.codebook_ema, ema_eps=args.ema_eps, vgg19=args.vgg19, semantic_weight=args.semantic_weight,
                            weights_ema=args.weights_ema)
    if net_ema:
        trainer.load_ema_weights(net_ema)
    if args.vgg16:        # the opening line of a run with a perceptual term: which files it was built from
        print(json.dumps({"perceptual": type(trainer.perceptual).__name__, "vgg16": args.vgg16, "lpips_heads": args.lpips_heads,
                          "tensors_loaded": len(trainer.perceptual.loaded_keys)}), flush=True)
    if args.vgg19:        # ... and of a run with the semantic term
        print(json.dumps({"semantic": type(trainer.semantic).__name__, "vgg19": args.vgg19, "semantic_weight": trainer.semantic_weight,
                          "tensors_loaded": len(trainer.semantic.loaded_keys)}), flush=True)
    step_fn, batch_fn = graphed_fns(trainer, dataset) if args.graph else (None, None)
    validate_fn = None
    # stage 3 scores the inference path, stage 1 the prior's own reconstruction of the ground truth; stage 2 has nothing to score
    if args.stage in ("stage1", "stage3") and not args.no_val:
        test_ds = D.LAYOUTS[args.layout](dict(options["datasets"].get("val", {}), root=args.root), train=False, all_opt=options)
        if len(test_ds):
            validate_fn = (make_validate_stage1 if args.stage == "stage1" else make_validate)(trainer, test_ds, args.precision)
    return fit(options, trainer, dataset, args.out, step_fn=step_fn, batch_fn=batch_fn, resume=resume, validate_fn=validate_fn)


if __name__ == "__main__":
    main()
