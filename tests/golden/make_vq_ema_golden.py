"""Writes tests/golden/vq_ema.npz and tests/golden/vq_ema_large.npz: for each seeded case (K codes, N tokens per update) the inputs of
three successive EMA updates and the three tensors of the reference's own EmbeddingEMA (code/models/modules/quantize.py:331-358, on CPU)
after each -- cluster_size_ema_update, embed_avg_ema_update and weight_update fed the one-hot statistics formed as
EMAVectorQuantizer.forward forms them (:422, :428, :431).  (EMAVectorQuantizer itself cannot be constructed, :365-366.)  Every case has
codes no update selects.  The largest case has a file of its own: with it one file would pass the size limit for a committed file.
Needs the reference tree; run from the repository root:  python tests/golden/make_vq_ema_golden.py"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from oracle import refimport  # noqa: E402

CASES = [(64, 512), (64, 2000), (300, 512), (300, 2000), (8192, 512), (8192, 2000)]      # (K, N)
LARGE = [(8192, 2000)]             # -> vq_ema_large.npz
UPDATES = 3
DECAY, EPS = 0.99, 1e-5
SEED0 = 200


def inputs(K, N, seed):
    """-> (weight fp32 [K,3], idx int64 [UPDATES,N], z fp32 [UPDATES,N,3]): a standard-normal codebook (the reference's own init, :336) and
    latents; indices over a fixed three quarters of the codes with a skewed law, so that some codes gather long sums and a quarter of the
    codebook (at least) is never selected."""
    rng = np.random.default_rng(seed)
    weight = rng.standard_normal((K, 3)).astype(np.float32)
    alive = rng.permutation(K)[:max(1, (3 * K) // 4)]
    p = 1.0 / (1.0 + np.arange(alive.size))
    idx = rng.choice(alive, size=(UPDATES, N), p=p / p.sum()).astype(np.int64)
    z = rng.standard_normal((UPDATES, N, 3)).astype(np.float32)
    return weight, idx, z


def run_reference(K, weight, idx, z):
    """-> (cluster_size [UPDATES,K], embed_avg [UPDATES,K,3], weight [UPDATES,K,3]) fp32: the module's tensors after each update."""
    refimport.install()
    from models.modules.quantize import EmbeddingEMA

    emb = EmbeddingEMA(K, 3, decay=DECAY, eps=EPS)
    out = ([], [], [])
    with torch.no_grad():
        emb.weight.copy_(torch.from_numpy(weight))
        emb.embed_avg.copy_(emb.weight)                                    # :339, embed_avg = weight.clone()
        for u in range(UPDATES):
            z_flattened = torch.from_numpy(z[u])
            encodings = F.one_hot(torch.from_numpy(idx[u]), K).type(z_flattened.dtype)      # :422
            emb.cluster_size_ema_update(encodings.sum(0))                  # :428-429
            emb.embed_avg_ema_update(encodings.transpose(0, 1) @ z_flattened)               # :431-432
            emb.weight_update(K)                                           # :434
            for dst, t in zip(out, (emb.cluster_size, emb.embed_avg, emb.weight)):
                dst.append(t.detach().numpy().copy())
    return tuple(np.stack(a) for a in out)


def main():
    small, large = {"decay": np.float64(DECAY), "eps": np.float64(EPS)}, {"decay": np.float64(DECAY), "eps": np.float64(EPS)}
    for i, (K, N) in enumerate(CASES):
        weight, idx, z = inputs(K, N, SEED0 + i)
        cs, ea, w = run_reference(K, weight, idx, z)
        never = K - np.unique(idx).size
        assert never > 0 and cs.dtype == ea.dtype == w.dtype == np.float32
        dst = large if (K, N) in LARGE else small
        tag = "K%d_N%d" % (K, N)
        dst.update({"weight0_" + tag: weight, "idx_" + tag: idx.astype(np.int32), "z_" + tag: z, "cluster_size_" + tag: cs,
                    "embed_avg_" + tag: ea, "weight_" + tag: w})
        print(tag, "never selected", never, "active per update", [int(np.unique(r).size) for r in idx], "max |weight|", float(np.abs(w).max()))
    np.savez_compressed(os.path.join(HERE, "vq_ema.npz"), **small)
    np.savez_compressed(os.path.join(HERE, "vq_ema_large.npz"), **large)


if __name__ == "__main__":
    main()
