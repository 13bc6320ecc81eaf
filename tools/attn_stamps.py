#!/usr/bin/env python
"""Cycle table of one key tile of attn_kv_fwd_kernel: where a wave's ~3 500 cycles per 32-key tile go.

    GLARE_DEFS="-DATTN_KV_PLACE=0,0,0,0,0,0,0,0,8,0,0,0,0,0,0,0,0" python tools/attn_stamps.py [--build-only] [--tag NAME]

Builds glare_amd/csrc/attn.hip ALONE with -DGLARE_ATTN_STAMPS (plus whatever GLARE_DEFS holds: the placement table under test) into
tools/scratch/ -- a diagnostic library of its own, never libglare_hip*.so -- in which the kernel reads the clock at the phase boundaries
of one tile (the middle one) per workgroup: wait + barrier, K.Q^T, softmax, P.V, loop overhead.  Runs it at the path's shape (B = 8,
N = 16 275, fp16) on random-normal data after >= 2 s of back-to-back launches, so that the clock is the loaded one, and prints the median
cycles per phase over every wave of the launch.  The stamps fence the schedule: read the SHARES of this build; its run time is not the
product kernel's (that is tools/kbench.py attn).  --build-only compiles and stops (no GPU needed)."""
import argparse
import ctypes
import hashlib
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "glare_amd", "csrc")
OUT_DIR = os.path.join(ROOT, "tools", "scratch")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
PHASES = ("wait+barrier", "K.Q^T", "softmax", "P.V", "loop overhead")


def build(precision, verbose=True, reuse=False):
    defs = os.environ.get("GLARE_DEFS", "").split()
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-DGLARE_ATTN_STAMPS"] + defs
    if precision == "fp16":
        flags.append("-DGLARE_ACT_F16")
    tag = hashlib.sha1(" ".join(flags).encode()).hexdigest()[:10]
    os.makedirs(OUT_DIR, exist_ok=True)
    lib = os.path.join(OUT_DIR, "libattn_stamps_%s.so" % tag)
    deps = [os.path.join(CSRC, f) for f in ("attn.hip", "common.h", "f16_names.h")] + [os.path.join(ROOT, "include", "glare_hip.h")]
    if not os.path.exists(lib) or not reuse and any(os.path.getmtime(d) > os.path.getmtime(lib) for d in deps if os.path.exists(d)):
        cmd = [HIPCC] + flags + ["-shared", os.path.join(CSRC, "attn.hip"), "-o", lib]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return lib


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--no-rebuild", action="store_true", help="use the library of an earlier --build-only with the same flags as it is")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=105 * 155)
    ap.add_argument("--precision", choices=("bf16", "fp16"), default="fp16")
    ap.add_argument("--pair", action="store_true", help="the hi / lo output form (attn_kv_fwd_kernel<true>)")
    ap.add_argument("--warm-s", type=float, default=2.0, help="seconds of back-to-back launches before the stamped one")
    ap.add_argument("--tag", default=None, help="name of this schedule in the printed table")
    a = ap.parse_args()
    lib_path = build(a.precision, reuse=a.no_rebuild)
    if a.build_only:
        print(lib_path)
        return
    import torch

    sys.path.insert(0, ROOT)
    from glare_amd import _lib

    lib = ctypes.CDLL(lib_path, mode=ctypes.RTLD_LOCAL)
    _lib._bind(lib, half=a.precision == "fp16")      # typed from the header, like the product libraries: the ABI is the same
    launch = getattr(lib, "glare_attention_kv512_pair_" + ("f16" if a.precision == "fp16" else "bf16"))

    B, N, C = a.batch, a.tokens, 512
    dt = torch.float16 if a.precision == "fp16" else torch.bfloat16
    g = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(B, N, C, device="cuda", generator=g).to(dt)
    q = (torch.randn(B, N, C, device="cuda", generator=g) * 0.3).to(dt)
    out = torch.empty(B, N, C, dtype=dt, device="cuda")
    out_lo = torch.empty_like(out) if a.pair else None
    # the diagnostic build stamps into the workspace argument, which a launch without key splits does not use otherwise:
    # 6 stamps per wave, 4 waves per workgroup of 128 query rows
    nbytes = B * ((N + 127) // 128) * 4 * 6 * 8
    stamps = torch.zeros(nbytes // 8, dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def run(ws=None, ws_bytes=0):
        rc = launch(q.data_ptr(), C, x.data_ptr(), C, out.data_ptr(), None if out_lo is None else out_lo.data_ptr(), C, B, N, 1, ws, ws_bytes,
                    stream)
        if rc != 0:
            raise RuntimeError("launch failed: %d" % rc)

    t0, n = time.time(), 0
    while time.time() - t0 < a.warm_s:      # back-to-back: a few launches queued ahead, the device never idles
        for _ in range(4):
            run()
        torch.cuda.synchronize()
        n += 4
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    run(stamps.data_ptr(), nbytes)
    e.record()
    torch.cuda.synchronize()
    st = stamps.view(-1, 6).cpu()
    st = st[(st[:, 0] != 0) & (st[:, 5] != 0)]
    d = (st[:, 1:] - st[:, :-1]).tolist()
    total = (st[:, 5] - st[:, 0]).tolist()
    name = a.tag or os.environ.get("GLARE_DEFS", "") or "default placement"
    print("== %s   (B=%d N=%d %s%s; %d waves stamped, %d warm-up launches, stamped launch %.3f ms)"
          % (name, B, N, a.precision, " pair" if a.pair else "", len(total), n, s.elapsed_time(e)))
    print("%-14s %8s %7s" % ("phase", "median", "share"))
    tot = median(total)
    for i, ph in enumerate(PHASES):
        m = median([r[i] for r in d])
        print("%-14s %8d %6.1f%%" % (ph, m, 100.0 * m / tot))
    print("%-14s %8d   (clock counts of s_memtime; every phase includes one stamp's own cost)" % ("tile", tot))


if __name__ == "__main__":
    sys.exit(main())
