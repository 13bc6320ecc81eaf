"""A checkpoint sweep (glare_amd.evaluate) without a dataset or a training run: N name-seeded checkpoints of one stage over 15
synthetic 400x600 pairs, after one un-timed pass -- the closing JSON line carries seconds per checkpoint (load + re-pack, scoring) and
images/s of the scoring part.

    python tools/evaluate_sweep.py stage2|stage3 [checkpoints, default 4]"""
import json
import os
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from glare_amd import checkpoint, evaluate  # noqa: E402
from glare_amd.synthetic import seeded_init_, synthetic_gt, synthetic_lowlight  # noqa: E402

stage = sys.argv[1]
n_ckpt = int(sys.argv[2]) if len(sys.argv) > 2 else 4
dev = torch.device("cuda", 0)
lows, gts = synthetic_lowlight(15, 400, 600, seed=1234), synthetic_gt(15, 400, 600, seed=1235)
with tempfile.TemporaryDirectory() as d:
    os.makedirs(os.path.join(d, "models"))
    netG, net_hq = evaluate.build_nets(stage, device=dev)
    for k in range(n_ckpt):
        seeded_init_(netG, 20 + k)
        checkpoint.save_network(netG, os.path.join(d, "models", "%d_G.pth" % (1000 * (k + 1))))
    # one un-timed pass first (kernel loading, allocator pools), as glare_amd.infer warms up before its clock
    evaluate.score_checkpoint(stage, netG, net_hq, lows[:8], gts[:8])
    res = evaluate.sweep(stage, d, os.path.join(d, "out"), lows, gts, nets=(netG, net_hq), device=dev)
print(json.dumps(res))
