"""LOL dataset loader (host side): mirrors `LoL_Dataset` (code/data/LoL_dataset.py:409-502) and its helpers
`random_crop` (:640-661), `random_flip` (:615-621), `random_rotation` (:631-637) with the same folder layout
(`<root>/our485|eval15/{low,high}/*.png`), option keys, sample dict and random-number call sequence, so that a seeded run draws
the crops / flips / rotations the reference draws.  PNG decoding is PIL (RGB order, what the reference gets from
cv2.imread + COLOR_BGR2RGB); the histogram-equalised side input (`concat_histeq` / `histeq_as_input`, off in every shipped
config) is not built.  The tensors it yields feed glare_amd.train.{Stage2Trainer,Stage3Trainer}.step and glare_amd.infer."""
import os
import random

import numpy as np
import torch


def random_crop(hr, lr, size_hr):
    """Same square crop from both images; np.random.randint is called for rows, then columns (LoL_dataset.py:640-661)."""
    sx, sy = lr.shape[0], lr.shape[1]
    x0 = np.random.randint(low=0, high=(sx - size_hr) + 1) if sx > size_hr else 0
    y0 = np.random.randint(low=0, high=(sy - size_hr) + 1) if sy > size_hr else 0
    return hr[x0:x0 + size_hr, y0:y0 + size_hr, :], lr[x0:x0 + size_hr, y0:y0 + size_hr, :]


def center_crop(img, size):
    assert img.shape[0] == img.shape[1], img.shape      # the reference asserts on dims 1/2 of an HWC image (:667); same intent
    border = (img.shape[0] - size) // 2
    return img[border:img.shape[0] - border, border:img.shape[1] - border, :]


def random_flip(hr, lr):
    keep = np.random.choice([True, False])
    return (hr, lr) if keep else (np.flip(hr, 1).copy(), np.flip(lr, 1).copy())


def random_rotation(hr, lr):
    k = np.random.choice([0, 1, 3])
    return np.rot90(hr, k, axes=(0, 1)).copy(), np.rot90(lr, k, axes=(0, 1)).copy()


def to_tensor(img_u8):
    """torchvision ToTensor on a uint8 HWC array: CHW float32 / 255."""
    return torch.from_numpy(np.ascontiguousarray(img_u8.transpose(2, 0, 1))).float().div(255)


class LoL_Dataset(torch.utils.data.Dataset):
    def __init__(self, opt, train, all_opt=None):
        from PIL import Image

        all_opt = all_opt or {}
        assert not all_opt.get("concat_histeq", False) and not all_opt.get("histeq_as_input", False), "histogram-equalised input: not built"
        self.opt = opt
        self.log_low = opt.get("log_low", False)
        self.use_flip, self.use_rot, self.use_crop = opt.get("use_flip", False), opt.get("use_rot", False), opt.get("use_crop", False)
        self.use_noise = opt.get("noise_prob", False)
        self.noise_prob = opt["noise_prob"] if self.use_noise else None
        self.noise_level = opt.get("noise_level", 0)
        self.center_crop_hr_size = opt.get("center_crop_hr_size", None)
        self.crop_size = opt.get("GT_size", None)
        self.root = os.path.join(opt["root"], "our485" if train else "eval15")
        self.pairs = []
        for f_name in filter(lambda x: "png" in x, os.listdir(os.path.join(self.root, "low"))):
            low = np.asarray(Image.open(os.path.join(self.root, "low", f_name)).convert("RGB"))
            high = np.asarray(Image.open(os.path.join(self.root, "high", f_name)).convert("RGB"))
            self.pairs.append([low, high, f_name.split(".")[0]])

    def __len__(self):
        return len(self.pairs)

    def __getitem__(self, item):
        lr, hr, f_name = self.pairs[item]
        if self.use_crop:
            hr, lr = random_crop(hr, lr, self.crop_size)
        if self.center_crop_hr_size:
            hr, lr = center_crop(hr, self.center_crop_hr_size), center_crop(lr, self.center_crop_hr_size)
        if self.use_flip:
            hr, lr = random_flip(hr, lr)
        if self.use_rot:
            hr, lr = random_rotation(hr, lr)
        hr, lr = to_tensor(hr), to_tensor(lr)
        if self.use_noise and random.random() < self.noise_prob:
            lr = torch.randn(lr.shape) * (self.noise_level / 255) + lr
        if self.log_low:
            lr = torch.log(torch.clamp(lr + 1e-3, min=1e-3))
        return {"LQ": lr, "GT": hr, "LQ_path": f_name, "GT_path": f_name}


class LoL_Dataset_v2(LoL_Dataset):
    """The LOL-v2 layout (`LoL_Dataset_v2`, LoL_dataset.py:505-554): `<root>/{Synthetic,Real_captured}/{Train,Test}/` with the
    folders `Low` / `Normal` in Train and `low` / `high` in Test; both listings sorted and paired BY POSITION (the two sides' file
    names differ), the pair named after the normal-light file.  Options, transforms and sample dict are LoL_Dataset's;
    `gamma_aug` and the histogram-equalised side input are not built."""

    def __init__(self, opt, train, all_opt=None):
        from PIL import Image

        all_opt = all_opt or {}
        assert not all_opt.get("concat_histeq", False) and not all_opt.get("histeq_as_input", False), "histogram-equalised input: not built"
        assert not opt.get("gamma_aug", False), "gamma_aug: not built"
        self.opt = opt
        self.log_low = opt.get("log_low", False)
        self.use_flip, self.use_rot, self.use_crop = opt.get("use_flip", False), opt.get("use_rot", False), opt.get("use_crop", False)
        self.use_noise = opt.get("noise_prob", False)
        self.noise_prob = opt["noise_prob"] if self.use_noise else None
        self.noise_level = opt.get("noise_level", 0)
        self.center_crop_hr_size = opt.get("center_crop_hr_size", None)
        self.crop_size = opt.get("GT_size", None)
        self.root = opt["root"]
        self.pairs = []
        low_dir, high_dir = ("Low", "Normal") if train else ("low", "high")
        for sub_data in ("Synthetic", "Real_captured"):
            folder = os.path.join(self.root, sub_data, "Train" if train else "Test")
            lows = sorted(f for f in os.listdir(os.path.join(folder, low_dir)) if "png" in f)
            highs = sorted(f for f in os.listdir(os.path.join(folder, high_dir)) if "png" in f)
            if len(highs) < len(lows):          # the reference indexes the normal-light list by the low list's positions
                raise IndexError("%s: %d low images, %d normal-light images" % (folder, len(lows), len(highs)))
            for f_low, f_high in zip(lows, highs):
                low = np.asarray(Image.open(os.path.join(folder, low_dir, f_low)).convert("RGB"))
                high = np.asarray(Image.open(os.path.join(folder, high_dir, f_high)).convert("RGB"))
                self.pairs.append([low, high, f_high.split(".")[0]])


LAYOUTS = {"v1": LoL_Dataset, "v2": LoL_Dataset_v2}


def _crop_hw(S):
    return (S, S) if isinstance(S, int) else tuple(S)


def draw_augmentation(ds, item):
    """The random decisions of `ds[item]` WITHOUT touching a pixel: (y0, x0, S, flip, k) -- the sample is
    rot90(flip(img[y0:y0 + S, x0:x0 + S]) if flip, k).  Makes LoL_Dataset.__getitem__'s np.random calls in its order (rows then columns
    of random_crop, each only when the image is larger than the crop; the flip's choice; the rotation's choice), so a seeded run
    draws what the dataset -- and the reference -- draws.  center_crop_hr_size is folded into the origin.  S is an int for a
    square crop, else (height, width): an image smaller than GT_size keeps its own side, as random_crop's slice does."""
    H, W = ds.pairs[item][0].shape[:2]
    y0 = x0 = 0
    ch, cw = H, W
    if ds.use_crop:
        size = ds.crop_size
        y0 = np.random.randint(low=0, high=(H - size) + 1) if H > size else 0
        x0 = np.random.randint(low=0, high=(W - size) + 1) if W > size else 0
        ch, cw = min(size, H), min(size, W)
    if ds.center_crop_hr_size:
        assert ch == cw, (ch, cw)                     # center_crop's own assertion
        border = (ch - ds.center_crop_hr_size) // 2
        y0, x0 = y0 + border, x0 + border
        ch = cw = ch - 2 * border
    flip = 0
    if ds.use_flip:
        flip = 0 if np.random.choice([True, False]) else 1
    k = int(np.random.choice([0, 1, 3])) if ds.use_rot else 0
    return int(y0), int(x0), (int(ch) if ch == cw else (int(ch), int(cw))), flip, k


def apply_augmentation(img, y0, x0, S, flip, k):
    """numpy restatement of the decisions on one HWC image (host twin of csrc/train_data.hip)."""
    ch, cw = _crop_hw(S)
    img = img[y0:y0 + ch, x0:x0 + cw, :]
    if flip:
        img = np.flip(img, 1)
    return np.rot90(img, k, axes=(0, 1))


def lq_lookup_table(log_low):
    """fp32 [256]: what the dataset makes of a low-image byte -- its own torch expression, evaluated once."""
    x = torch.arange(256).float().div(255)
    return torch.log(torch.clamp(x + 1e-3, min=1e-3)) if log_low else x


class DeviceLoLDataset:
    """A LoL_Dataset / LoL_Dataset_v2 held on the device as uint8 (LOL: 485 pairs, ~700 MB); `batch()` assembles a training batch with
    ONE kernel launch (csrc/train_data.hip) straight into fp32 NCHW buffers -- bit-identical to collating `host_dataset[i]`."""

    RING = 8        # pinned row tables in flight: the host runs ahead of the stream, a table is reused only after its copy has run

    def __init__(self, host_dataset, device):
        from . import _lib

        ds = host_dataset
        if ds.use_noise:
            raise ValueError("noise_prob = %r: the reference draws this noise with torch.randn on the host, a device-resident "
                             "dataset cannot reproduce it; set noise_prob to 0" % (ds.opt.get("noise_prob"),))
        shapes = [p[0].shape for p in ds.pairs]
        assert all(p[0].shape == p[1].shape and p[0].dtype == np.uint8 and p[0].shape[2] == 3 for p in ds.pairs)
        if not ds.use_crop and len(set(shapes)) > 1:
            raise ValueError("use_crop is off and the images differ in size: they cannot share a batch")
        if ds.use_rot and not ds.use_crop and any(s[0] != s[1] for s in shapes):
            raise ValueError("use_rot without use_crop needs square images (a rotated sample would not fit the batch)")
        self.ds, self.device, self._lib = ds, torch.device(device), _lib
        self.hw = [(s[0], s[1]) for s in shapes]
        sizes = [3 * h * w for h, w in self.hw]
        self.offsets = [int(o) for o in np.cumsum([0] + sizes[:-1])]
        self.n_bytes = int(sum(sizes))
        self.low = torch.from_numpy(np.concatenate([p[0].reshape(-1) for p in ds.pairs])).to(self.device)
        self.high = torch.from_numpy(np.concatenate([p[1].reshape(-1) for p in ds.pairs])).to(self.device)
        self.lut = lq_lookup_table(ds.log_low).to(self.device)
        self.row_ints = _lib.constants()["GLARE_TRAIN_ROW_INTS"]
        self._tables = {}            # B -> (pinned [RING + 1, B, R], device [B, R], events, next slot); slot RING serves captures
        self.last_draws = None

    def __len__(self):
        return len(self.ds)

    def _table(self, B):
        if B not in self._tables:
            pinned = torch.empty(self.RING + 1, B, self.row_ints, dtype=torch.int32).pin_memory()
            self._tables[B] = [pinned, torch.empty(B, self.row_ints, dtype=torch.int32, device=self.device), [None] * self.RING, 0]
        return self._tables[B]

    def rows(self, indices, draws):
        """int32 [B, GLARE_TRAIN_ROW_INTS] of include/glare_hip.h for these samples and decisions."""
        out = np.empty((len(indices), self.row_ints), dtype=np.int64)
        for b, (i, (y0, x0, S, flip, k)) in enumerate(zip(indices, draws)):
            ch, cw = _crop_hw(S)
            off = int(self.offsets[i])
            out[b] = (off & 0xffffffff, off >> 32, self.hw[i][0], self.hw[i][1], y0, x0, ch, cw, flip, k)
        return (out & 0xffffffff).astype(np.uint32).view(np.int32)        # negative values (tests of the error paths) keep their bits

    def check_rows(self, rows, out_h, out_w):
        """The host checks of glare_train_batch_u8, for rows written into a table that a CAPTURED launch reads at replay."""
        for off_lo, off_hi, H, W, y0, x0, ch, cw, flip, k in rows.tolist():
            off = (off_lo & 0xffffffff) | (off_hi << 32)
            ok = H > 0 and W > 0 and 0 <= off and off + 3 * H * W <= self.n_bytes and y0 >= 0 and x0 >= 0 and ch > 0 and cw > 0
            ok = ok and y0 + ch <= H and x0 + cw <= W and flip in (0, 1) and k in (0, 1, 3) and (k == 0 or ch == cw) and (ch, cw) == (out_h, out_w)
            if not ok:
                raise ValueError("invalid batch row %r for a %d x %d batch" % ((off, H, W, y0, x0, ch, cw, flip, k), out_h, out_w))

    def batch(self, indices, out_gt=None, out_lq=None, draws=None):
        """(GT, LQ), fp32 [B,3,S,S] on the device, for `indices` in order; written into out_gt / out_lq when given (the static inputs
        of a GraphedStep).  draws: the (y0, x0, S, flip, k) per sample, default draw_augmentation(ds, i) per index in order.  Never
        synchronises with the device in steady state: the rows go through a ring of pinned tables, copied non-blocking.
        Under stream capture the launch reads a table of its own; `update_captured()` rewrites it before a replay."""
        indices = [int(i) for i in indices]
        if draws is None:
            draws = [draw_augmentation(self.ds, i) for i in indices]
        self.last_draws = draws
        B = len(indices)
        oh, ow = _crop_hw(draws[0][2])
        rows = self.rows(indices, draws)
        pinned, dev_rows, events, nxt = tab = self._table(B)
        capturing = torch.cuda.is_current_stream_capturing()
        slot = self.RING if capturing else nxt
        if not capturing and events[slot] is not None:
            events[slot].synchronize()                      # RING batches ago: long done, unless the host is that far ahead
        host_rows = pinned[slot]
        host_rows.numpy()[:] = rows
        if out_gt is None:
            out_gt = torch.empty(B, 3, oh, ow, dtype=torch.float32, device=self.device)
        if out_lq is None:
            out_lq = torch.empty(B, 3, oh, ow, dtype=torch.float32, device=self.device)
        for t in (out_gt, out_lq):
            assert t.dtype == torch.float32 and tuple(t.shape) == (B, 3, oh, ow) and t.is_contiguous() and t.device == self.low.device, \
                (t.dtype, tuple(t.shape), (B, 3, oh, ow))
        _lib = self._lib
        with torch.cuda.device(self.device):
            dev_rows.copy_(host_rows, non_blocking=True)
            if not capturing:
                events[slot] = torch.cuda.Event()
                events[slot].record()
                tab[3] = (slot + 1) % self.RING
            _lib.check(_lib.lib().glare_train_batch_u8(_lib.ptr(self.low), _lib.ptr(self.high), self.n_bytes, host_rows.data_ptr(),
                                                       _lib.ptr(dev_rows), B, oh, ow, _lib.ptr(self.lut), _lib.ptr(out_gt), _lib.ptr(out_lq),
                                                       _lib.stream_handle()), "glare_train_batch_u8")
        return out_gt, out_lq

    def update_captured(self, indices, draws=None):
        """New samples for the batch() launch that was captured with len(indices) samples: validates and rewrites the pinned table
        its copy node reads.  The replay then yields this batch in the captured output buffers."""
        indices = [int(i) for i in indices]
        if draws is None:
            draws = [draw_augmentation(self.ds, i) for i in indices]
        self.last_draws = draws
        rows = self.rows(indices, draws)
        self.check_rows(rows, *_crop_hw(draws[0][2]))
        self._table(len(indices))[0][self.RING].numpy()[:] = rows
