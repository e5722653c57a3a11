"""Generate the quantizer-training golden fixture from the reference itself.

Run in the build container only (the reference never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_vq_train_golden.py

Runs the reference ``nn.modules.vae.codebook`` quantizers (pure PyTorch, CPU, fp32) with the ``_stats`` patch of
``make_vq_golden.py`` (the reference's ``forward`` cannot finish without it).  For every shape of ``SHAPES``,
``(N, spatial, K, D)``:

* four chained training-mode steps of ``VectorQuantizerEMA`` (decay 0.99, eps 1e-5, beta 0.25) from a state with a
  strictly positive ``ema_cluster_size`` (ones, or ``rand * 4``), ``ema_w = embedding`` and a seeded normal
  ``embedding``.  Step ``s`` quantises ``z_s = embedding_s[j_s] + 0.05 * std(embedding_s) * noise`` drawn around
  the reference's embedding at that step, so every row is decided (its fp64 gap exceeds twice
  ``vq_bounds.row_bound``; the first of 64 seeds for which that holds at all four steps is taken) and the argmin
  is ``j_s``.  Recorded: ``z_s``, the four outputs, and
  the three buffers as ``state{s}`` (before step ``s``) ... ``state{s+1}`` (after it); ``state0.ema_w`` equals
  ``state0.embedding`` and is not stored;
* one backward of each quantizer at ``state0`` on ``z_0``: ``(z_q * g_zq).sum() + 0.7 * vq_loss`` with a seeded
  ``g_zq``; recorded ``g_zq`` and ``z.grad`` (``embedding.grad`` of the classic quantizer is asserted ``None``).

A codebook of 512 x 64 is 128 KiB and five states of two such buffers pass the 1 MiB limit of a committed file,
so the record is split over two files: ``vq_train_golden.pt`` holds everything but states 2 to 4 of the larger
shape, which are in ``vq_train_golden_b.pt``.  Tensors only; load with ``weights_only=True``.
"""
from __future__ import annotations

import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join("/root/reference", "src"))
sys.path.insert(0, os.path.dirname(HERE))

from nn.modules.vae.codebook import VectorQuantizer, VectorQuantizerEMA  # noqa: E402  (reference)

import vq_bounds as vb  # noqa: E402

SHAPES = {"a": (3, (5, 7), 100, 8), "b": (2, (8, 8), 512, 64)}
BETA, DECAY, EPS, G_LOSS, STEPS = 0.25, 0.99, 1e-5, 0.7, 4


def _patch_stats(quantizer_cls):
    """Run the reference's own ``_stats`` with an index order of the right rank (the identity)."""
    original = quantizer_cls.__mro__[1]._stats

    def _stats(self, encodings, indices, z, order, inverse, **kw):
        return original(self, encodings, indices, z, order, tuple(range(z.ndim - 1)), **kw)

    quantizer_cls._stats = _stats


def _state(q):
    return {k: getattr(q, k).detach().clone() for k in ("embedding", "ema_cluster_size", "ema_w")}


class Undecided(Exception):
    pass


def record(tag, N, sp, K, D, seed):
    g = vb.gen(f"vq_train/{tag}/s{seed}")
    M = vb_rows(N, sp)
    q = VectorQuantizerEMA(K, D, BETA, decay=DECAY, eps=EPS).train()
    with torch.no_grad():
        q.embedding.copy_(torch.randn(K, D, generator=g))
        q.ema_w.copy_(q.embedding)
        q.ema_cluster_size.copy_(torch.ones(K) if tag == "a" else torch.rand(K, generator=g) * 4.0)
        assert float(q.ema_cluster_size.min()) > 0.0
    out = {}
    states = [_state(q)]
    for s in range(STEPS):
        emb = q.embedding.detach().clone()
        j = torch.randint(0, K, (M,), generator=g)
        flat = emb[j] + 0.05 * emb.std() * torch.randn(M, D, generator=g)
        ref = vb.reference(flat, emb)
        if not (bool((ref["gap"] > 2.0 * vb.row_bound(ref)).all()) and torch.equal(ref["idx"], j)):
            raise Undecided(f"{tag} seed {seed} step {s}")
        z = flat.view(N, *sp, D).movedim(-1, 1).contiguous()
        if s == 0:
            out.update(backward(tag, z, states[0], K, D, g))
        with torch.no_grad():
            z_q, vq_loss, perplexity, codes = q(z)
        assert torch.equal(codes.reshape(-1), j), (tag, s)
        out.update({f"{tag}.z{s}": z, f"{tag}.z_q{s}": z_q.clone(), f"{tag}.vq_loss{s}": vq_loss.clone(),
                    f"{tag}.perplexity{s}": perplexity.clone(), f"{tag}.codes{s}": codes.clone()})
        states.append(_state(q))
    for s, st in enumerate(states):
        for k, v in st.items():
            if s == 0 and k == "ema_w":
                assert torch.equal(v, st["embedding"])
                continue
            out[f"{tag}.state{s}.{k}"] = v
    return out


def vb_rows(N, sp):
    M = N
    for v in sp:
        M *= v
    return M


def backward(tag, z, st, K, D, g):
    out = {}
    g_zq = torch.randn(z.shape, generator=g)
    out[f"{tag}.g_zq"] = g_zq
    for qt in ("classic", "ema"):
        if qt == "classic":
            q = VectorQuantizer(K, D, BETA).train()
            with torch.no_grad():
                q.embedding.copy_(st["embedding"])
        else:
            q = VectorQuantizerEMA(K, D, BETA, decay=DECAY, eps=EPS).train()
            with torch.no_grad():
                for k, v in st.items():
                    getattr(q, k).copy_(v)
        zz = z.clone().requires_grad_()
        z_q, vq_loss, _, _ = q(zz)
        ((z_q * g_zq).sum() + G_LOSS * vq_loss).backward()
        if qt == "classic":
            assert q.embedding.grad is None
        out[f"{tag}.{qt}.z_grad"] = zz.grad.clone()
    return out


def main():
    torch.set_num_threads(8)
    _patch_stats(VectorQuantizer)
    _patch_stats(VectorQuantizerEMA)
    out = {}
    for tag, (N, sp, K, D) in SHAPES.items():
        # rand * 4 cluster sizes hold a few values near 0, whose codes grow by 1 / size in the first step and
        # widen row_bound with them: take the first seed whose four steps leave every row decided (a property of
        # the inputs and the fp64 reference, not of any kernel)
        for seed in range(64):
            try:
                out.update(record(tag, N, sp, K, D, seed))
                print(tag, "seed", seed)
                break
            except Undecided as e:
                print("skipped:", e)
        else:
            raise SystemExit(f"no decided trajectory for {tag}")
    out["hyper"] = torch.tensor([BETA, DECAY, EPS, G_LOSS], dtype=torch.float64)
    second = {k: out.pop(k) for k in list(out) if k[:9] in ("b.state2.", "b.state3.", "b.state4.")}
    for name, part in (("vq_train_golden.pt", out), ("vq_train_golden_b.pt", second)):
        path = os.path.join(HERE, name)
        torch.save(part, path)
        print("wrote", name, os.path.getsize(path), "bytes", {k: tuple(v.shape) for k, v in part.items()})
        assert os.path.getsize(path) < 1_000_000


if __name__ == "__main__":
    main()
