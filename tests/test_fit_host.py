"""CPU: the host side of the training driver (glare_amd.fit) and of the device-resident dataset (glare_amd.data): augmentation
draws and the lookup table against LoL_Dataset bit for bit, the lr schedule against stock torch (and the reference's scheduler
where it is present), the index order against a DataLoader, the loop's mechanics / checkpoints / resume with stub step and batch
functions, `.state` interchange, the v2 folder layout."""
import itertools
import os
import random
import types

import numpy as np
import pytest
import torch
from PIL import Image

from glare_amd import checkpoint, fit, train
from glare_amd import data as D

SIZES = [(40, 56), (33, 47), (24, 24), (64, 48), (37, 37), (50, 50)]      # one smaller than the 32-crop, odd sizes, squares


def make_v1(root, split, sizes, seed=0):
    rng = np.random.default_rng(seed)
    for sub in ("low", "high"):
        os.makedirs(os.path.join(root, split, sub), exist_ok=True)
    for i, (h, w) in enumerate(sizes):
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(root, split, "low", "%02d.png" % i))
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(os.path.join(root, split, "high", "%02d.png" % i))


def test_draws_and_lookup_table_equal_the_dataset_bit_for_bit(tmp_path):
    """1. draw_augmentation + crop / flip / rot90 restated in numpy + the 256-entry table == LoL_Dataset.__getitem__, 200 seeded draws
    per option combination."""
    make_v1(str(tmp_path / "mixed"), "our485", SIZES)
    make_v1(str(tmp_path / "square"), "our485", [(37, 37), (50, 50), (40, 40)])
    assert torch.equal(D.lq_lookup_table(False), torch.arange(256).float().div(255))
    combos = 0
    for use_crop, use_flip, use_rot, center, log_low in itertools.product((False, True), (False, True), (False, True), (None, 20), (False, True)):
        # rotation and center_crop need square inputs (center_crop asserts it): without the random crop, the square folder
        square_only = not use_crop and (use_rot or center)
        root = str(tmp_path / ("square" if square_only else "mixed"))
        opt = {"root": root, "use_crop": use_crop, "use_flip": use_flip, "use_rot": use_rot, "GT_size": 32, "log_low": log_low, "noise_prob": 0}
        if center:
            opt["center_crop_hr_size"] = center
        ds = D.LoL_Dataset(opt, train=True)
        if use_crop and center:          # the 32-crop of an image smaller than 32 is not square: center_crop asserts in both
            items = [i for i, p in enumerate(ds.pairs) if min(p[0].shape[:2]) >= 32]
        else:
            items = list(range(len(ds)))
        lut = D.lq_lookup_table(log_low)
        for n in range(200):
            item = items[n % len(items)]
            np.random.seed(1000 + n)
            s = ds[item]
            after_ds = np.random.get_state()[1].copy(), np.random.get_state()[2]
            np.random.seed(1000 + n)
            draw = D.draw_augmentation(ds, item)
            after_draw = np.random.get_state()[1], np.random.get_state()[2]
            assert np.array_equal(after_ds[0], after_draw[0]) and after_ds[1] == after_draw[1]       # same number of draws
            low, high, _ = ds.pairs[item]
            lo, hi = D.apply_augmentation(low, *draw), D.apply_augmentation(high, *draw)
            gt = torch.from_numpy(np.ascontiguousarray(hi.transpose(2, 0, 1))).float().div(255)
            lq = lut[torch.from_numpy(np.ascontiguousarray(lo.transpose(2, 0, 1))).long()]
            assert torch.equal(s["GT"], gt) and torch.equal(s["LQ"], lq), (opt, item, draw)
        combos += 1
    assert combos == 32


def _torch_lrs(niter, warmup, rels, gamma, lr0, make):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([{"params": [p]}, {"params": []}], lr=lr0, betas=(0.9, 0.99))
    for g in opt.param_groups:
        g["initial_lr"] = g["lr"]
    sch = make(opt, [int(r * niter) for r in rels], gamma)
    out = []
    for it in range(1, niter + 1):
        sch.step()                                                  # base_model.py:67-79
        if it < warmup:
            for g in opt.param_groups:
                g["lr"] = g["initial_lr"] / warmup * it
        out.append(opt.param_groups[0]["lr"])
    return out, sch, opt


def _stub_opt(lr=5e-5):
    scales = []
    groups = [types.SimpleNamespace(params=[], lr=lr, weight_decay=0.0), types.SimpleNamespace(params=[], lr=lr, weight_decay=1e-5)]
    return types.SimpleNamespace(groups=groups, betas=(0.9, 0.999), eps=1e-8, t=0, set_lr_scale=scales.append, scales=scales,
                                 scaler_state_dict=lambda: dict(checkpoint.GRAD_SCALER_STATE), load_scaler_state_dict=lambda sd: None)


class _StubTrainer(train.Trainer):
    """The least a driver needs, built without a device: an optimizer and a network; every member of the interface at its default."""

    def __init__(self, opt, netG=None):
        self.opt, self.netG = opt, netG


def _options(niter=200, batch=2, save=10, print_freq=5):
    o = fit.default_options("stage3")
    o["train"]["niter"], o["datasets"]["train"]["batch_size"] = niter, batch
    o["logger"]["save_checkpoint_freq"], o["logger"]["print_freq"] = save, print_freq
    return o


def _our_lrs(niter=200):
    opt = _stub_opt()
    sch = fit.make_schedule(opt, _options(niter))
    return [sch.update(it) for it in range(1, niter + 1)], sch, opt


def test_lr_sequence_equals_stock_multisteplr_with_the_warmup_override():
    """2. exact equality with torch.optim.Adam + MultiStepLR + the override, niter 200, warm-up 10."""
    ours, sch, opt = _our_lrs()
    ref, tsch, _ = _torch_lrs(200, 10, [0.5, 0.75, 0.9, 0.95], 0.5, 5e-5,
                              lambda o, m, g: torch.optim.lr_scheduler.MultiStepLR(o, m, gamma=g))
    assert ours == ref
    assert ours[0] == 5e-5 / 10 and ours[8] == 5e-5 / 10 * 9 and ours[9] == ours[8]        # the override's value sticks after the warm-up
    assert ours[99] == ours[98] * 0.5 and ours[-1] == ours[8] * 0.5 ** 4
    assert opt.scales[-1] == ours[-1] / 5e-5 and len(opt.scales) == 9 + 4                 # device writes only when the factor moves
    ts, os_ = tsch.state_dict(), sch.state_dict()
    assert os_["last_epoch"] == ts["last_epoch"] == 200 and os_["_step_count"] == ts["_step_count"] and os_["milestones"] == ts["milestones"]
    assert os_["base_lrs"] == ts["base_lrs"] and os_["_last_lr"] == ts["_last_lr"] and os_["gamma"] == ts["gamma"]


@pytest.mark.reference
def test_lr_sequence_equals_the_reference_scheduler():
    from oracle import refimport as R

    if not R.available():
        pytest.skip("reference tree not present")
    R.install()
    from models.lr_scheduler import MultiStepLR_Restart

    ours, _, _ = _our_lrs()
    ref, _, _ = _torch_lrs(200, 10, [0.5, 0.75, 0.9, 0.95], 0.5, 5e-5,
                           lambda o, m, g: MultiStepLR_Restart(o, m, restarts=[], weights=[], gamma=g, clear_state=[], lr_steps_invese=[]))
    assert ours == ref


class _Dummy(torch.utils.data.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


@pytest.mark.parametrize("n,batch", [(11, 2), (23, 4), (6, 6)])
def test_index_order_equals_the_dataloader(n, batch):
    """3. per epoch, for the same seed: DataLoader(shuffle=True, drop_last=True) with num_workers 0, as the reference builds it."""
    torch.manual_seed(10)
    loader = torch.utils.data.DataLoader(_Dummy(n), batch_size=batch, shuffle=True, drop_last=True, num_workers=0)
    ref = [[b.tolist() for b in loader] for _ in range(3)]
    torch.manual_seed(10)
    ours = [fit.epoch_batches(n, batch) for _ in range(3)]
    assert ours == ref and len(ours[0]) == n // batch
    assert ours[0] != ours[1]


class _Stub:
    """A dataset of 7 'images' whose batch() draws as DeviceLoLDataset does, and a step that consumes Python's `random` as stage 2 does."""

    def __init__(self, tmp, trainer=None):
        self.ds = types.SimpleNamespace(pairs=[[np.zeros((40 + i, 50, 3), np.uint8)] * 2 + ["x"] for i in range(7)], use_crop=True, crop_size=32,
                                        center_crop_hr_size=None, use_flip=True, use_rot=True)
        self.trainer = trainer or _StubTrainer(_stub_opt(), torch.nn.Linear(2, 2))
        self.trace, self.out = [], str(tmp)

    def __len__(self):
        return 7

    def batch(self, indices):
        self.cur = (tuple(indices),) + tuple((y0, x0, f, k) for y0, x0, _, f, k in (D.draw_augmentation(self.ds, i) for i in indices))
        return None, None

    def step(self, gt, lq):
        self.trace.append(self.cur + (random.random(), self.trainer.opt.scales[-1]))
        return torch.tensor(float(len(self.trace)))

    def run(self, niter, save=10):
        recs = []
        fit.fit(_options(niter=niter, save=save), self.trainer, self, self.out, step_fn=self.step, batch_fn=self.batch, log=recs.append)
        return recs


def test_loop_mechanics_checkpoint_cadence_and_exact_resume(tmp_path):
    """4. 30 steps straight == 17 steps, resume, 13 more: the same (indices, y0, x0, flip, k), Python-random draws and lr factors."""
    a = _Stub(tmp_path / "a")
    recs = a.run(30)
    assert len(a.trace) == 30 and [r["iter"] for r in recs[:-1]] == list(range(5, 31, 5)) and recs[-1]["done"] and recs[-1]["iter"] == 30
    assert recs[0]["loss"] == 5.0 and set(recs[0]) == {"epoch", "iter", "lr", "loss", "ms_per_step", "ms_batch"}
    assert recs[-2]["epoch"] == (30 - 1) // 3                                   # 7 images, batch 2, drop_last: 3 steps per epoch
    for sub, ext in (("models", "_G.pth"), ("training_state", ".state")):
        assert sorted(os.listdir(os.path.join(a.out, sub))) == sorted("%d%s" % (i, ext) for i in (10, 20, 30))
    assert len({t[0] for t in a.trace}) > 10 and len({t[1] for t in a.trace}) > 10      # the order and the draws do vary

    b = _Stub(tmp_path / "b")
    # milestones come from niter: the interrupted run is a 30-step run stopped at 17, not a 17-step run
    opts = _options(niter=30, save=17)

    def stop_at_17(gt, lq):
        if len(b.trace) == 17:
            raise KeyboardInterrupt
        return b.step(gt, lq)

    with pytest.raises(KeyboardInterrupt):
        fit.fit(opts, b.trainer, b, b.out, step_fn=stop_at_17, batch_fn=b.batch, log=lambda r: None)
    assert os.path.exists(os.path.join(b.out, "training_state", "17.state"))
    c = _Stub(tmp_path / "b")
    random.seed(999), np.random.seed(999), torch.manual_seed(999)                # the resumed process starts from other RNG states
    recs = []
    fit.fit(_options(niter=30, save=10), c.trainer, c, c.out, step_fn=c.step, batch_fn=c.batch, log=recs.append,
            resume=os.path.join(b.out, "training_state", "17.state"))
    assert len(c.trace) == 13 and recs[0]["iter"] == 20 and recs[-1]["iter"] == 30
    assert b.trace[:17] == a.trace[:17]
    assert c.trace == a.trace[17:]


class _Recorder(_StubTrainer):
    """Overrides every member of train.Trainer's interface and records the calls."""

    checkpoint_tag = "MAIN"

    def __init__(self, tag="Stub x 2", branches=("a", "b")):
        super().__init__(_stub_opt(), torch.nn.Linear(2, 2))
        self.side, self.tag, self.branches, self.calls, self.value = torch.nn.Linear(3, 1), tag, branches, [], 0.0
        self.next_branch = branches[0]

    def step_tensor(self, gt_img, lr_img=None, branch=None):
        self.calls.append(("step", branch))
        self.value += 1.5
        self.last_terms = {"aux": torch.tensor(self.value), "unlogged": torch.tensor(-1.0)}
        return torch.tensor(self.value * 2)

    def extra_networks(self):
        return {"SIDE": self.side}

    def extra_state(self):
        return {"stub_extra": {"value": self.value}}

    def load_extra_state(self, state):
        self.calls.append(("load_extra_state", state["stub_extra"]))

    def objective_tag(self):
        return self.tag

    def on_resume(self, step):
        self.calls.append(("on_resume", step))

    def log_terms(self):
        return ("aux",)

    def graph_branches(self):
        return self.branches

    def draw_branch(self):
        self.calls.append(("draw_branch",))
        return self.next_branch

    def init_forward(self, gt_img, lr_img, branch):
        self.calls.append(("init_forward", branch))

    def invalidate(self):
        self.calls.append(("invalidate",))


def test_driver_asks_the_trainer_and_nothing_else(tmp_path):
    """The loop's files, `.state` entries, record keys and resume go through train.Trainer's members: (a) the extra network file and
    the extra `.state` entry appear under the trainer's names and come back through load_extra_state; (b) on_resume gets the resumed
    step; (c) a resume under another objective_tag() is refused; (d) a trainer that overrides nothing writes what it always wrote."""
    tr = _Recorder()
    a = _Stub(tmp_path / "a", tr)
    opts = _options(niter=30, save=7)

    def stop_at_9(gt, lq):
        if sum(c[0] == "step" for c in tr.calls) == 9:
            raise KeyboardInterrupt
        return tr.step_tensor(gt, lq)

    recs = []
    with pytest.raises(KeyboardInterrupt):
        fit.fit(opts, tr, a, a.out, step_fn=stop_at_9, batch_fn=a.batch, log=recs.append)
    # (a) the names are the trainer's
    assert sorted(os.listdir(os.path.join(a.out, "models"))) == ["7_MAIN.pth", "7_SIDE.pth"]
    assert os.listdir(os.path.join(a.out, "training_state")) == ["7.state"]
    side = torch.load(os.path.join(a.out, "models", "7_SIDE.pth"), map_location="cpu")
    assert set(side) == set(tr.side.state_dict()) and all(torch.equal(v, tr.side.state_dict()[k]) for k, v in side.items())
    main = torch.load(os.path.join(a.out, "models", "7_MAIN.pth"), map_location="cpu")
    assert all(torch.equal(v, tr.netG.state_dict()[k]) for k, v in main.items())
    st = torch.load(os.path.join(a.out, "training_state", "7.state"), map_location="cpu", weights_only=False)
    assert set(st) == {"epoch", "iter", "schedulers", "optimizers", "scaler", fit.STATE_KEY, "stub_extra"}
    assert st["stub_extra"] == {"value": 7 * 1.5} and st[fit.STATE_KEY]["perceptual"] == "Stub x 2"
    assert set(recs[0]) == {"epoch", "iter", "lr", "loss", "ms_per_step", "ms_batch", "aux"} and recs[0]["aux"] == 5 * 1.5 and recs[0]["loss"] == 15.0
    # ... and come back through the load member with the saved content; (b) on_resume receives the resumed step
    tr2 = _Recorder()
    b = _Stub(tmp_path / "a", tr2)
    recs = []
    fit.fit(_options(niter=12, save=7), tr2, b, b.out, batch_fn=b.batch, log=recs.append, resume=os.path.join(a.out, "training_state", "7.state"))
    assert [c for c in tr2.calls if c[0] != "step"] == [("on_resume", 7), ("load_extra_state", {"value": 7 * 1.5})]
    assert tr2.calls.count(("step", None)) == 5 and recs[-1]["iter"] == 12           # the default step_fn is the trainer's step_tensor
    # (c) another objective: refused, in the words of PERCEPTUAL_RESUME_REFUSAL
    for other, shown in (("Stub x 3", "Stub x 3"), (None, "none")):
        tr3 = _Recorder(tag=other)
        with pytest.raises(ValueError) as e:
            fit.fit(_options(niter=12, save=7), tr3, _Stub(tmp_path / "a", tr3), a.out, log=recs.append, resume=os.path.join(a.out, "training_state", "7.state"))
        assert str(e.value) == fit.PERCEPTUAL_RESUME_REFUSAL % ("Stub x 2", shown) and tr3.calls == []
    # (d) nothing overridden: the file set and the record keys of test_loop_mechanics_checkpoint_cadence_and_exact_resume
    d = _Stub(tmp_path / "d")
    recs = d.run(30)
    assert set(recs[0]) == {"epoch", "iter", "lr", "loss", "ms_per_step", "ms_batch"}
    for sub, ext in (("models", "_G.pth"), ("training_state", ".state")):
        assert sorted(os.listdir(os.path.join(d.out, sub))) == sorted("%d%s" % (i, ext) for i in (10, 20, 30))
    st = torch.load(os.path.join(d.out, "training_state", "30.state"), map_location="cpu", weights_only=False)
    assert set(st) == {"epoch", "iter", "schedulers", "optimizers", "scaler", fit.STATE_KEY}
    assert set(st[fit.STATE_KEY]) == {"rng", "epoch_order", "batches_done"}


def test_graphed_step_covers_the_trainers_branches_and_invalidates_after_every_replay(monkeypatch):
    """GraphedStep's bookkeeping without a device (the warm-up and the capture themselves replaced): capture_all covers exactly
    graph_branches(), step_tensor replays the branch draw_branch() returned, invalidate() follows every replay."""
    tr = _Recorder(branches=("a", "b", "c"))

    class _Graph:
        def __init__(self, branch):
            self.branch = branch

        def replay(self):
            tr.calls.append(("replay", self.branch))

    def capture(self, branch):
        tr.calls.append(("capture", branch))
        self.graphs[branch] = (_Graph(branch), torch.tensor(float(ord(branch))))

    monkeypatch.setattr(train.GraphedStep, "_warm_up", lambda self, branches: tr.calls.append(("warm_up", tuple(branches))))
    monkeypatch.setattr(train.GraphedStep, "_capture", capture)
    gt, lq = torch.arange(6.0).reshape(1, 1, 2, 3), -torch.arange(6.0).reshape(1, 1, 2, 3)
    gs = train.GraphedStep(tr, torch.zeros_like(gt), torch.zeros_like(lq))
    assert tr.calls == [("warm_up", ("a", "b", "c")), ("invalidate",), ("capture", "a"), ("capture", "b"), ("capture", "c")]
    assert set(gs.graphs) == {"a", "b", "c"}
    for branch in ("c", "a", "c", "b"):
        del tr.calls[:]
        tr.next_branch = branch
        loss = gs.step_tensor(gt, lq)
        assert tr.calls == [("draw_branch",), ("replay", branch), ("invalidate",)] and float(loss) == ord(branch)
        assert torch.equal(gs.gt, gt) and torch.equal(gs.lr, lq)
    del tr.calls[:]
    gs.capture_all()                                   # again (after a resume): the old graphs are dropped, the same set is captured
    assert [c for c in tr.calls if c[0] == "capture"] == [("capture", b) for b in ("a", "b", "c")] and set(gs.graphs) == {"a", "b", "c"}


def test_state_file_interchanges_with_checkpoint_and_stock_torch(tmp_path):
    """5. the driver's `.state` loads with checkpoint.resume_training; schedulers[0] loads into a stock MultiStepLR; the optimizer
    entry carries the CURRENT lr, as torch's param_groups do."""
    a = _Stub(tmp_path)
    o = _options(niter=30, save=25)
    o["train"]["lr_steps_rel"] = [0.5]
    fit.fit(o, a.trainer, a, a.out, step_fn=a.step, batch_fn=a.batch, log=lambda r: None)
    path = os.path.join(a.out, "training_state", "25.state")
    other = _StubTrainer(_stub_opt(lr=1.0))
    sch = fit.make_schedule(other.opt, o)
    epoch, it = checkpoint.resume_training(path, other, [sch])
    assert (epoch, it) == (8, 25) and sch.last_epoch == 25
    st = torch.load(path, map_location="cpu", weights_only=False)
    assert set(st) == {"epoch", "iter", "schedulers", "optimizers", "scaler", fit.STATE_KEY}
    assert st["optimizers"][0]["param_groups"][0]["lr"] == 5e-5 / 10 * 9 * 0.5 and st["optimizers"][0]["param_groups"][0]["betas"] == (0.9, 0.99)
    assert a.trainer.opt.groups[0].lr == 5e-5                                   # ... and the trainer keeps its base lr
    p = torch.nn.Parameter(torch.zeros(1))
    stock = torch.optim.lr_scheduler.MultiStepLR(torch.optim.Adam([{"params": [p]}, {"params": []}], lr=5e-5), [15], gamma=0.5)
    stock.load_state_dict(st["schedulers"][0])
    assert stock.last_epoch == 25 and stock.milestones == {15: 1} and stock.get_last_lr() == st["schedulers"][0]["_last_lr"]
    stock.optimizer.param_groups[0]["lr"] = st["optimizers"][0]["param_groups"][0]["lr"]
    stock.step()
    sch.adopt_loaded()
    assert sch.update(26) == stock.optimizer.param_groups[0]["lr"]
    assert other.opt.groups[0].lr == 5e-5 and other.opt.scales[-1] == pytest.approx(0.9 * 0.5, rel=1e-12)


def test_v2_layout_pairs_by_sorted_position_and_noise_is_refused(tmp_path):
    """6. <root>/{Synthetic,Real_captured}/{Train,Test}/{Low,Normal | low,high}, sorted, paired by position."""
    rng = np.random.default_rng(3)
    made = {}
    for sub, split, low_dir, high_dir, lows, highs in (("Synthetic", "Train", "Low", "Normal", ["b_low.png", "a_low.png"], ["n2.png", "n1.png"]),
                                                       ("Real_captured", "Train", "Low", "Normal", ["low9.png"], ["normal9.png"]),
                                                       ("Synthetic", "Test", "low", "high", ["t1.png"], ["t1.png"]),
                                                       ("Real_captured", "Test", "low", "high", ["z.png", "y.png"], ["q.png", "p.png"])):
        for d, names in ((low_dir, lows), (high_dir, highs)):
            os.makedirs(tmp_path / sub / split / d, exist_ok=True)
            for nm in names:
                img = rng.integers(0, 256, size=(20, 28, 3), dtype=np.uint8)
                Image.fromarray(img).save(tmp_path / sub / split / d / nm)
                made[(sub, split, d, nm)] = img
        (tmp_path / sub / split / low_dir / "notes.txt").write_text("ignored")
    tr = D.LoL_Dataset_v2({"root": str(tmp_path), "log_low": True}, train=True)
    assert [p[2] for p in tr.pairs] == ["n1", "n2", "normal9"]
    assert np.array_equal(tr.pairs[0][0], made[("Synthetic", "Train", "Low", "a_low.png")]) and np.array_equal(tr.pairs[0][1], made[("Synthetic", "Train", "Normal", "n1.png")])
    assert np.array_equal(tr.pairs[2][0], made[("Real_captured", "Train", "Low", "low9.png")])
    te = D.LoL_Dataset_v2({"root": str(tmp_path)}, train=False)
    assert [p[2] for p in te.pairs] == ["t1", "p", "q"] and np.array_equal(te.pairs[1][0], made[("Real_captured", "Test", "low", "y.png")])
    s = tr[1]
    assert torch.equal(s["GT"], D.to_tensor(made[("Synthetic", "Train", "Normal", "n2.png")])) and s["GT_path"] == "n2"
    assert torch.equal(s["LQ"], D.lq_lookup_table(True)[torch.from_numpy(made[("Synthetic", "Train", "Low", "b_low.png")].transpose(2, 0, 1).copy()).long()])
    assert D.LAYOUTS == {"v1": D.LoL_Dataset, "v2": D.LoL_Dataset_v2}
    noisy = D.LoL_Dataset_v2({"root": str(tmp_path), "noise_prob": 0.3, "noise_level": 5}, train=True)
    with pytest.raises(ValueError, match="noise_prob"):
        D.DeviceLoLDataset(noisy, "cpu")


def test_device_dataset_refuses_what_cannot_share_a_batch(tmp_path):
    make_v1(str(tmp_path), "our485", [(40, 56), (33, 47)])
    with pytest.raises(ValueError, match="use_crop"):
        D.DeviceLoLDataset(D.LoL_Dataset({"root": str(tmp_path)}, train=True), "cpu")
    make_v1(str(tmp_path / "same"), "our485", [(40, 56), (40, 56)])
    with pytest.raises(ValueError, match="use_rot"):
        D.DeviceLoLDataset(D.LoL_Dataset({"root": str(tmp_path / "same"), "use_rot": True}, train=True), "cpu")


def test_options_defaults_and_overrides(tmp_path):
    s2, s3 = fit.default_options("stage2"), fit.default_options("stage3")
    assert (s2["datasets"]["train"]["batch_size"], s2["datasets"]["train"]["GT_size"], s2["train"]["lr_G"], s2["train"]["niter"],
            s2["logger"]["save_checkpoint_freq"]) == (4, 320, 5e-4, 80000, 1000)
    assert (s3["datasets"]["train"]["batch_size"], s3["datasets"]["train"]["GT_size"], s3["train"]["lr_G"], s3["train"]["niter"],
            s3["logger"]["save_checkpoint_freq"]) == (2, 256, 5e-5, 40000, 500)
    for o in (s2, s3):
        assert (o["train"]["beta1"], o["train"]["beta2"], o["train"]["warmup_iter"], o["train"]["manual_seed"]) == (0.9, 0.99, 10, 10)
        assert o["train"]["lr_steps_rel"] == [0.5, 0.75, 0.9, 0.95] and o["train"]["lr_gamma"] == 0.5 and not o["network_G"]["train_RRDB"]
        d = o["datasets"]["train"]
        assert d["use_flip"] and d["use_crop"] and d["log_low"] and not d["noise_prob"]
    (tmp_path / "o.json").write_text('{"train": {"niter": 7}, "datasets": {"train": {"use_rot": true}}}')
    m = fit.merge_options(s3, fit.load_options_file(str(tmp_path / "o.json")))
    assert m["train"]["niter"] == 7 and m["train"]["lr_G"] == 5e-5 and m["datasets"]["train"]["use_rot"] and m["datasets"]["train"]["GT_size"] == 256
    s3["train"]["niter"] = 1
    assert fit.DEFAULTS["stage3"]["train"]["niter"] == 40000
