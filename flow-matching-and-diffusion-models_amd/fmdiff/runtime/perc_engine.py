"""Fused HIP execution of the VGG perceptual loss (``fmdiff.nn.losses.perceptual.VGGPerceptualLoss``): forward and
the data gradient to the reconstruction.

The loss is ``sum_l w_l mean |f_l(rec) - f_l(target)|`` over the outputs of tapped ReLUs of a frozen stack of
``Conv2d(3x3, stride 1, padding 1) -> ReLU [-> MaxPool2d(2, 2)]`` (reference ``src/nn/losses/vae.py:22-72``).  The
walker runs the reconstruction and the target as ONE batch of 2 N images (recon first):

    perc_stage -> per conv: ops.conv (two-term gather, fp32 result) -> perc_tap_fwd (tapped) | bn_act_fwd(slope 0)

and stops behind the last tap.  ``perc_tap_fwd`` is the ReLU, the L1 term and, where a pool follows, the 2x2 max pool
in one pass over the conv's output (csrc/perceptual.hip).

The forward runs on two-term bf16 operands, as the discriminators do (``disc_engine``) and for the same reason, only
sharper: ReLU's derivative jumps from 1 to 0 and the L1 sign adds a second kink, so a plain bf16 forward is 6 - 11 %
off the fp32 gradient at the input.  The backward carries bf16 gradients through the plain bf16
weight layout (``ops.conv(transposed=True)``) over the recon half only; the stack is frozen, so no weight-gradient
work is ever queued, and the split weights are built once and rebuilt only when a weight's version counter moves.

Only the recon rows of each conv output are kept for the backward (a copy, so that the 2 N-image tensor is freed),
plus an int8 sign per tapped element; under ``torch.no_grad()`` nothing is kept.  Everything a forward leaves for its
backward lives in a ``PercState`` owned by the call.
"""
from __future__ import annotations

from typing import List, Optional

import torch

from . import ops
from .disc_engine import _DiscWeights, _pad8
from .engine import LayerEngine

F32 = torch.float32


class _PercWeights(_DiscWeights):
    """The split layouts of a frozen stack, plus their halo tiles (``ops.conv`` would otherwise re-tile per call).
    ``invalidate`` marks every entry stale; the next forward rebuilds what it reaches."""

    def invalidate(self):
        self._force.update(self._c.keys())

    def split_tiled(self, w: torch.Tensor, cp: int, kpad=None):
        key = (id(w), "split_tiled", cp, kpad)
        if not self._fresh(key, self._ver(w)):
            e = self._c.get(key)
            buf = ops.tile_weights(self.split(w, cp, kpad), out=None if e is None else e["buf"])
            self._c[key] = dict(kind="split_tiled", src=w, buf=buf, ver=self._ver(w))
            self._force.discard(key)
        return self._c[key]["buf"]


class _Layer:
    """One saved conv of a forward: what its backward reads (``y``: the recon rows of its fp32 output)."""
    __slots__ = ("spec", "y", "sgn", "cin")

    def __init__(self, spec, y, sgn, cin):
        self.spec, self.y, self.sgn, self.cin = spec, y, sgn, cin


class PercState:
    """Everything one forward leaves for its backward (owned by the call, not by the engine)."""
    __slots__ = ("layers", "raw", "mode", "weights")

    def __init__(self, raw, mode, weights):
        self.layers: List[_Layer] = []
        self.raw, self.mode, self.weights = raw, mode, weights


class PercEngine(LayerEngine):
    def __init__(self, module):
        super().__init__(module, dims1=False)
        self.wc = _PercWeights()

    def check(self, recon, target):
        """Host arithmetic only: shapes, sizes of every feature map, devices.  Returns the staged size."""
        m = self.m
        if recon.dim() != 4 or recon.shape[1] not in (1, 3):
            raise ValueError(f"VGGPerceptualLoss: images [N, 1 or 3, H, W], got {tuple(recon.shape)}")
        if tuple(target.shape) != tuple(recon.shape):
            raise ValueError(f"VGGPerceptualLoss: recon {tuple(recon.shape)} and target {tuple(target.shape)} differ")
        hw = m.resize or tuple(int(v) for v in recon.shape[2:])
        m.feature_sizes(hw)   # raises ValueError for an input too small for the stack
        ops._need_cuda(recon, "VGGPerceptualLoss")
        ops._need_cuda(target, "VGGPerceptualLoss")
        if torch.cuda.is_current_stream_capturing():
            raise NotImplementedError("VGGPerceptualLoss: hipGraph capture is not built (the walk is eager)")
        for p in m.features.parameters():
            if p.device != recon.device or target.device != recon.device:
                raise RuntimeError(f"VGGPerceptualLoss: weights on {p.device}, recon on {recon.device}, target on "
                                   f"{target.device}: one device")
        return hw

    def forward(self, recon, target, mode: str = "identity", save: bool = True, plan_out: Optional[list] = None):
        """``recon``, ``target``: fp32 NCHW; ``mode``: the image map of ``recon`` (``ops.IMAGE_MODES``).  Returns
        (loss, the per-tap values as one device tensor, PercState or None).  ``plan_out``: a list that receives the
        ``ConvPlan`` and split count of every conv."""
        m = self.m
        hw = self.check(recon, target)
        specs = m.layer_specs()
        recon = recon.detach().contiguous().float()
        target = target.detach().contiguous().float()
        N, dev = recon.shape[0], recon.device
        ntap = sum(s.tap is not None for s in specs)
        values = torch.empty((ntap,), device=dev, dtype=F32)
        loss = torch.empty((), device=dev, dtype=F32)
        st = PercState(recon, mode, [s.weight for s in specs]) if save else None
        h = ops.perc_stage(recon, target, mode, None if hw == tuple(recon.shape[2:]) else hw)
        for i, spec in enumerate(specs):
            conv = spec.conv
            Cp, K = h.shape[-1] // 2, conv.out_channels
            Kp = _pad8(K)
            kpad = Kp if Kp != K else None
            w = self.wc.split(conv.weight, Cp, kpad)
            tiled = None
            if ops.halo_eligible(h.shape[0], h.shape[1], h.shape[1], h.shape[2], Kp, Cin=4 * Cp):
                tiled = self.wc.split_tiled(conv.weight, Cp, kpad)
            bias = conv.bias if Kp == K else self.wc.padded(conv.bias, Kp)
            po = [] if plan_out is not None else None
            # (hi + lo)(w_hi + w_lo) in one launch: the two-source gather reads the activation twice
            y, _ = ops.conv(h, Kp, w, src1=h, ks=3, stride=1, pad=1, bias=bias, out_f32=True, wgt_tiled=tiled,
                            plan_out=po)
            if plan_out is not None:
                plan_out.append((i, tuple(y.shape), po[0], po[1]))
            last = i == len(specs) - 1
            sgn = None
            if spec.tap is not None:
                h, sgn, _ = ops.perc_tap_fwd(y, K, pool=spec.pool, want_out=not last, save=save, weight=spec.weight,
                                             value=values[spec.tap], loss=loss, first=spec.tap == 0)
            else:
                h = ops.bn_act_fwd(y, None, None, 0.0, split=True)
            if save:
                st.layers.append(_Layer(spec, y[:N].clone(), sgn, Cp))
        return loss, values, st

    def backward(self, st: PercState, g_loss):
        """``g_loss``: the device scalar gradient of the loss.  Returns the fp32 NCHW gradient of the raw recon."""
        g = g_loss.detach().reshape(1).float().contiguous()
        dy = None
        for i in range(len(st.layers) - 1, -1, -1):
            L = st.layers[i]
            spec, conv = L.spec, L.spec.conv
            K = conv.out_channels
            if spec.tap is not None:
                dy = ops.perc_tap_bwd(L.y, L.sgn, K, g, weight=spec.weight, g_below=dy,
                                      pool=spec.pool and dy is not None)
            else:
                dy = ops.bn_act_bwd(dy, L.y, slope=0.0)
            Kp = dy.shape[-1]
            wt = self.wc.get(conv.weight, 1, Kp if Kp != K else None, L.cin if conv.weight.shape[1] != L.cin else None)
            dy, _ = ops.conv(dy, L.cin, wt, ks=3, stride=1, pad=1, transposed=True, out_hw_=tuple(L.y.shape[1:3]))
        return ops.perc_stage_bwd(dy, st.raw, st.mode)


class _PercFunction(torch.autograd.Function):
    """raw recon -> loss; the target and the frozen stack receive no gradient."""

    @staticmethod
    def forward(fctx, recon, target, engine, mode, values_out):
        loss, values, st = engine.forward(recon, target, mode, save=True)
        fctx.engine, fctx.state = engine, st
        values_out.append(values)
        return loss

    @staticmethod
    def backward(fctx, g):
        st = fctx.state
        if st is None:
            raise RuntimeError("perceptual loss backward called twice on one forward")
        dx = fctx.engine.backward(st, g)
        fctx.state = None
        return dx, None, None, None, None


def perc_apply(module, recon, target, mode: str = "identity"):
    """(loss, per-tap values) of ``module`` for the raw fp32 NCHW ``recon`` mapped by ``mode`` against ``target``;
    the loss is connected by autograd to ``recon``."""
    eng = get_perc_engine(module)
    eng.check(recon, target)
    if mode not in ops.IMAGE_MODES:
        raise ValueError(f"image map {mode!r}: one of {sorted(ops.IMAGE_MODES)}")
    if not (torch.is_grad_enabled() and recon.requires_grad):
        loss, values, _ = eng.forward(recon, target, mode, save=False)
        return loss, values
    values = []
    loss = _PercFunction.apply(recon, target, eng, mode, values)
    return loss, values[0]


def get_perc_engine(module) -> PercEngine:
    eng = getattr(module, "_fmd_perc_engine", None)
    if eng is None:
        eng = PercEngine(module)
        object.__setattr__(module, "_fmd_perc_engine", eng)
    return eng
