"""Writes tests/golden/vq_usage.npz: for each seeded case of tests/usage_fp64.py (CASES) the indices the reference's own
VectorQuantizer.forward selects (code/models/modules/quantize.py:34-90, on CPU), its fp32 perplexity (:83-85) and the int64 counts of its
one-hot matrix.  Needs the reference tree; run from the repository root:  python tests/golden/make_vq_usage_golden.py"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import usage_fp64 as U  # noqa: E402
from oracle import refimport  # noqa: E402

SEED0 = 100


def run_reference(case, seed):
    """-> (idx int64 [N], perplexity fp32 scalar, counts int64 [K]) of the reference class on the seeded case."""
    refimport.install()
    from models.modules.quantize import VectorQuantizer

    z, cb = U.reference_case(case, seed)
    vq = VectorQuantizer(case[0], 3, 0.25)
    with torch.no_grad():
        vq.embedding.weight.copy_(cb)
        _, _, (perplexity, one_hot, idx) = vq(z)
    return idx.view(-1).numpy().astype(np.int64), np.float32(perplexity.item()), one_hot.sum(0).numpy().astype(np.int64)


def main():
    out = {"n_cases": np.int64(len(U.CASES))}
    for i, case in enumerate(U.CASES):
        idx, perplexity, counts = run_reference(case, SEED0 + i)
        assert counts.sum() == idx.size and int(idx.max()) < 2 ** 31
        out.update({"K_%d" % i: np.int64(case[0]), "idx_%d" % i: idx.astype(np.int32), "perplexity_%d" % i: perplexity, "counts_%d" % i: counts})
        print(case, "active", int((counts > 0).sum()), "perplexity", float(perplexity))
    np.savez_compressed(os.path.join(HERE, "vq_usage.npz"), **out)


if __name__ == "__main__":
    main()
