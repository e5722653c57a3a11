"""Per-call time of each piece of one quantizer training step (HIP events, 300 calls after 3 warm-up calls, inputs
rotating through 320 MB), at the shapes of tools/bench_vq_train.py:

    python tools/bench_vq_train_pieces.py [--collapsed] [--out profiles/vq_train_pieces.jsonl]

Inputs are clustered around the codebook (z = e_j + 0.05 n, j uniform: balanced segments) or, with
``--collapsed``, around code 0 alone: every row chooses one code, the segmented sum's worst case.  One JSON line
per shape: the longest segment and microseconds per call of ``ops.vq_quantize``, ``vq_residual``,
``vq_ema_update`` (both launches), ``vq_backward``, ``vq_codebook_grad`` and the torch transposition of ``g_zq``.
"""
import argparse
import json
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "flow-matching-and-diffusion-models_amd"))
from fmdiff.runtime import ops  # noqa: E402

SHAPES = ((4096, 16384, 256), (8192, 16384, 256), (8192, 512, 64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--collapsed", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = []
    for M, K, D in SHAPES:
        g = torch.Generator(device="cuda").manual_seed(M + K + D)
        e = torch.randn(K, D, generator=g, device="cuda")
        cs, w = torch.ones(K, device="cuda"), e.clone()
        n = int(320e6 / (4 * M * D)) + 1
        zs = [e[torch.randint(0, 1 if a.collapsed else K, (M,), generator=g, device="cuda")][None]
              + 0.05 * torch.randn(1, M, D, generator=g, device="cuda") for _ in range(n)]
        gz = torch.randn(1, M, D, generator=g, device="cuda")
        gl = torch.tensor([0.7], device="cuda")
        q = ops.vq_quantize(zs[0], D, e, 0.25, False)
        r = ops.vq_residual(zs[0], D, q.codes, e)
        pieces = {
            "vq_quantize": lambda z: ops.vq_quantize(z, D, e, 0.25, False),
            "vq_residual": lambda z: ops.vq_residual(z, D, q.codes, e),
            "vq_ema_update": lambda z: ops.vq_ema_update(z, D, q.codes, q.hist, e, cs, w, 0.99, 1e-5),
            "vq_backward": lambda z: ops.vq_backward(r, D, None, None, gz, gl, 0.25),
            "vq_codebook_grad": lambda z: ops.vq_codebook_grad(z, D, q.codes, q.hist, e, gl),
            "g_zq transpose (torch)": lambda z: gz.view(1, D, M).movedim(1, -1).contiguous(),
        }
        rec = dict(M=M, K=K, D=D, collapsed=a.collapsed, longest=int(q.hist.max()))
        for name, fn in pieces.items():
            for i in range(3):
                fn(zs[i % n])
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(300):
                fn(zs[i % n])
            t1.record()
            torch.cuda.synchronize()
            rec[name + " us"] = round(t0.elapsed_time(t1) * 1e3 / 300, 2)
        out.append(json.dumps(rec))
        print(out[-1], flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
