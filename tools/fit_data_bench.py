"""Data time per training step: (a) LoL_Dataset + DataLoader's default collate + .to(device), what the reference's loader does on
the CPU of the training process (num_workers 0, pageable memory), against (b) glare_amd.data.DeviceLoLDataset.batch (one launch of
csrc/train_data.hip).  Host wall clock around the calls plus a final synchronise, divided by the steps.

    python tools/fit_data_bench.py make DIR [pairs]           # a LOL-shaped folder of random 400x600 pairs
    python tools/fit_data_bench.py stage2|stage3 DIR [steps] [host|device]     (default: both, device first)"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from glare_amd import data as D
from glare_amd import fit


def make(root, pairs):
    from PIL import Image

    rng = np.random.default_rng(0)
    for split, n in (("our485", pairs), ("eval15", 2)):
        for sub, top in (("low", 60), ("high", 256)):
            os.makedirs(os.path.join(root, split, sub), exist_ok=True)
            for i in range(n):
                Image.fromarray(rng.integers(0, top, size=(400, 600, 3), dtype=np.uint8)).save(os.path.join(root, split, sub, "%03d.png" % i))


def timed(next_batch, steps, warmup=20):
    for _ in range(warmup):
        next_batch()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        next_batch()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / steps


def main():
    if sys.argv[1] == "make":
        return make(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 48)
    stage, root = sys.argv[1], sys.argv[2]
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 200
    which = sys.argv[4:] or ["device", "host"]
    opt = dict(fit.default_options(stage)["datasets"]["train"], root=root)
    B, S = opt["batch_size"], opt["GT_size"]
    dev = torch.device("cuda", 0)
    ds = D.LoL_Dataset(opt, train=True)
    fit.set_random_seed(10)
    for w in which:
        if w == "device":
            dds = D.DeviceLoLDataset(ds, dev)
            order = iter(())

            def next_batch():
                nonlocal order
                idx = next(order, None)
                if idx is None:
                    order = iter(fit.epoch_batches(len(ds), B))
                    idx = next(order)
                return dds.batch(idx)
        else:
            loader = torch.utils.data.DataLoader(ds, batch_size=B, shuffle=True, num_workers=0, drop_last=True)
            it = iter(())

            def next_batch():
                nonlocal it
                item = next(it, None)
                if item is None:
                    it = iter(loader)
                    item = next(it)
                return item["GT"].to(dev), item["LQ"].to(dev)
        print("%s %d x %dx%d, %d pairs, %s: %.3f ms per batch" % (stage, B, S, S, len(ds), "DeviceLoLDataset.batch" if w == "device" else
                                                                    "LoL_Dataset + collate + .to(device)", timed(next_batch, steps)), flush=True)


if __name__ == "__main__":
    main()
