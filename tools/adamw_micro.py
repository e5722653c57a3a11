"""Micro-benchmark of the fused AdamW + cosine-schedule launch on config B's flat parameter buffer (GPU box).

usage: [FMD_LIB=...] python tools/adamw_micro.py [--n 113008257] [--iters 20] [--ema]
Prints us/launch and the achieved HBM rate at the algorithmic 28 B/param (read p, g, m, v; write p, m, v).

--ema: three variants, alternated launch by launch, each launch timed by its own pair of HIP events after a
write over a buffer larger than the 256 MiB Infinity Cache (median and min..max over --iters):
  adamw_sched                      28 B/param
  adamw_sched_ema                  36 B/param (+ read and write of ema)
  adamw_sched + _foreach_lerp_     the unfused alternative: the old launch, then torch._foreach_lerp_(ema, p, 1 - d)
"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "flow-matching-and-diffusion-models_amd")]

import torch  # noqa: E402

from fmdiff.runtime import ops  # noqa: E402


def ema_compare(a, dev):
    p, g, m, v = (torch.randn(a.n, device=dev) * 0.01 for _ in range(4))
    v.abs_()
    ema = p.clone()
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    hp = (1e-4, 500, 100000)

    def plain():
        ops.adamw_sched(p, g, m, v, ctr, *hp)

    def fused():
        ops.adamw_sched(p, g, m, v, ctr, *hp, ema=ema, ema_decay=0.9999, ema_warmup=True)

    def unfused():
        ops.adamw_sched(p, g, m, v, ctr, *hp)
        torch._foreach_lerp_([ema], [p], 1e-4)

    variants = (("adamw_sched", plain, 28), ("adamw_sched_ema", fused, 36), ("adamw_sched+foreach_lerp", unfused, 40))
    times = {name: [] for name, _, _ in variants}
    for it in range(a.iters + 3):
        for name, fn, _ in variants:
            flush.fill_(it & 0xFF)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if it >= 3:   # the first rounds load code objects and warm the allocator
                times[name].append(e0.elapsed_time(e1) * 1e3)
    med = {}
    for name, _, nbytes in variants:
        ts = times[name]
        med[name] = statistics.median(ts)
        print(f"{name} n={a.n}: median {med[name]:.1f} us (min {min(ts):.1f}, max {max(ts):.1f}, {len(ts)} launches), "
              f"{nbytes * a.n / med[name] / 1e3:.0f} GB/s at {nbytes} B/param", flush=True)
    base = med["adamw_sched"]
    print(f"fused/plain {med['adamw_sched_ema'] / base:.3f} (bytes alone: {36 / 28:.3f}); "
          f"unfused/plain {med['adamw_sched+foreach_lerp'] / base:.3f}; "
          f"fused/unfused {med['adamw_sched_ema'] / med['adamw_sched+foreach_lerp']:.3f}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=113008257)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--ema", action="store_true", help="compare the launch with and without the fused EMA")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.ema:
        return ema_compare(a, dev)
    p, g, m, v = (torch.randn(a.n, device=dev) * 0.01 for _ in range(4))
    v.abs_()
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    for _ in range(5):
        ops.adamw_sched(p, g, m, v, ctr, 1e-4, 500, 100000)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.iters):
        ops.adamw_sched(p, g, m, v, ctr, 1e-4, 500, 100000)
    e1.record()
    torch.cuda.synchronize()
    us = e0.elapsed_time(e1) / a.iters * 1e3
    print(f"adamw_sched n={a.n}: {us:.1f} us/launch, {28 * a.n / us / 1e3:.0f} GB/s", flush=True)


if __name__ == "__main__":
    main()
