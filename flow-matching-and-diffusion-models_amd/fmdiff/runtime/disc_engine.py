"""Fused HIP execution of the GAN discriminators (``fmdiff.nn.modules.vae.discriminators``): forward and backward.

A discriminator is a stack of ``conv -> [BatchNorm2d] -> [LeakyReLU]`` layers (reference
``src/nn/modules/vae/discriminators.py:26-39``, ``src/nn/losses/vae.py:85-98``).  The walker runs each layer as

    image_stage (first layer only) -> ops.conv -> ops.bn_stats_f32 -> ops.bn_fold -> ops.bn_act_fwd

with the convolutions on the generic implicit GEMM (4x4 kernels: the halo kernels are 3x3), the weight gradients on
the grouped queue (``LayerEngine._wg`` / ``_join``) and the data gradients as transposed gathers.  BatchNorm and
LeakyReLU are csrc/batchnorm.hip.

The forward runs on two-term bf16 operands.  LeakyReLU's derivative jumps at 0, so the 2^-9 a bf16 operand moves a
pre-activation by flips the branch of the elements next to the kink, and the gradient's error grows like the square
root of the flipped fraction: a plain bf16 forward is 8 - 14 % off the fp32 gradient at the input (DESIGN.md
section 4).  So an activation v is carried as hi = bf16(v) and lo = bf16(v - hi) side by side in one bf16 tensor
``[N, H, W, 2 C]``, a weight likewise, and one conv launch over the two-source gather ``[hi | lo | hi | lo]`` with
the weights ``[w_hi | w_hi | w_lo | w_lo]`` forms (hi + lo)(w_hi + w_lo) on the MFMA with an fp32 result; BatchNorm
reads that fp32 tensor.  The backward needs no such care (its operands carry gradients, not branch decisions): dy and
dx are bf16, the data gradient reads the plain bf16 weight, and the weight gradient reads both terms of its input and
adds the two halves.

Several forwards of one discriminator are alive at once in a GAN step (``real_pred`` and ``fake_pred``), so a
forward returns everything its backward needs in a ``DiscState`` of its own: nothing per call lives on the engine.
"""
from __future__ import annotations

from typing import List

import torch

from . import ops
from .engine import LayerEngine, WeightCache

F32 = torch.float32


def _pad8(n: int) -> int:
    return max(8, -(-n // 8) * 8)


class _DiscWeights(WeightCache):
    """WeightCache whose refresh goes weight by weight through ``ops.prep_weights``: the batched refresh kernel
    (fmd_prep_weights_batch) holds at most 9 taps of a master tile in LDS, and these convs have 16."""

    def invalidate(self):
        for key, e in self._c.items():
            if e["kind"] == "pad":
                e["buf"][: e["src"].numel()].copy_(e["src"].detach().reshape(-1))
            elif e["kind"] == "prep":
                ops.prep_weights(e["src"].detach(), key[1], key[2], key[3], out=e["buf"])
            elif e["kind"] == "split":
                self._split_fill(e["src"], e["master"], e["cp"])
                ops.prep_weights(e["master"], 0, e["kpad"], None, out=e["buf"])
            else:   # nothing else is derived for a discriminator
                raise NotImplementedError(f"discriminator weight cache: entry kind {e['kind']}")
            e["ver"] = self._ver(e["src"])
        self._force.clear()

    @staticmethod
    def _split_fill(w, master, cp):
        """fp32 [K][4 cp][k][k]: w_hi at channel offsets 0 and cp, w_lo = w - bf16(w) at 2 cp and 3 cp (the bf16
        rounding of the layout pass leaves w_hi and bf16(w_lo) there); padding channels stay zero."""
        C = w.shape[1]
        wd = w.detach()
        hi = wd.to(torch.bfloat16).float()
        lo = wd - hi
        for off, t in ((0, hi), (cp, hi), (2 * cp, lo), (3 * cp, lo)):
            master[:, off:off + C].copy_(t)

    def split(self, w: torch.Tensor, cp: int, kpad=None):
        """bf16 forward layout [Kpad][T][4 cp] of ``w`` for the two-term gather [hi | lo | hi | lo] of an input with
        ``cp`` (padded) channels per term."""
        key = (id(w), "split", cp, kpad)
        if not self._fresh(key, self._ver(w)):
            e = self._c.get(key)
            master = e["master"] if e is not None else torch.zeros((w.shape[0], 4 * cp, *w.shape[2:]),
                                                                   device=w.device, dtype=F32)
            self._split_fill(w, master, cp)
            buf = ops.prep_weights(master, 0, kpad, None, out=None if e is None else e["buf"])
            self._c[key] = dict(kind="split", src=w, buf=buf, master=master, cp=cp, kpad=kpad, ver=self._ver(w))
            self._force.discard(key)
        return self._c[key]["buf"]


class _Layer:
    """One saved layer of a forward: what its backward reads."""
    __slots__ = ("spec", "x", "y", "a", "b", "mr")

    def __init__(self, spec, x, y, a, b, mr):
        self.spec, self.x, self.y, self.a, self.b, self.mr = spec, x, y, a, b, mr


class DiscState:
    """Everything one forward leaves for its backward (owned by the call, not by the engine)."""
    __slots__ = ("layers", "raw", "mode", "training", "in_channels", "out_pad")

    def __init__(self, raw, mode, training, in_channels):
        self.layers: List[_Layer] = []
        self.raw, self.mode, self.training, self.in_channels = raw, mode, training, in_channels
        self.out_pad = 8


class DiscEngine(LayerEngine):
    def __init__(self, module):
        super().__init__(module, dims1=False)
        self.wc = _DiscWeights()

    # ------------------------------------------------------------------ checks (host arithmetic only)
    def check(self, x):
        m = self.m
        what = type(m).__name__
        if x.dim() != 4 or x.shape[1] != m.in_channels:
            raise ValueError(f"{what}: input [N, {m.in_channels}, H, W], got {tuple(x.shape)}")
        sizes = m.output_sizes(tuple(x.shape[2:]))   # raises ValueError for an input too small for the stack
        if m.base_channels % 8:
            raise NotImplementedError(f"{what}: base_channels must be a multiple of 8 on the HIP engine")
        ops._need_cuda(x, what)
        for spec, sp in zip(m.layer_specs(), sizes[1:]):
            if spec.norm is not None and m.training and x.shape[0] * sp[0] * sp[1] < 2:
                raise ValueError(f"{what}: BatchNorm in training mode needs more than 1 value per channel")
        return sizes

    def ensure_grads(self):
        for p in self.m.parameters():
            if p.grad is None:
                p.grad = torch.zeros_like(p)

    # ------------------------------------------------------------------ forward
    def forward(self, x, mode: str = "identity", save: bool = True):
        """``x``: fp32 NCHW raw input; ``mode``: the image map fused into the staging (``ops.IMAGE_MODES``).
        Returns (logits fp32 NCHW ``[N, 1, h, w]``, DiscState or None)."""
        m = self.m
        self.check(x)
        training = bool(m.training)
        x = x.contiguous().float()
        st = DiscState(x if mode != "identity" else None, mode, training, m.in_channels) if save else None
        h = ops.image_stage(x, mode, split=True)          # [N, H, W, 2 Cp]: hi | lo
        for spec in m.layer_specs():
            conv, bn = spec.conv, spec.norm
            Cp, K = h.shape[-1] // 2, conv.out_channels
            Kp = _pad8(K)
            w = self.wc.split(conv.weight, Cp, Kp if Kp != K else None)
            bias = conv.bias if Kp == K else self.wc.padded(conv.bias, Kp)
            last = spec.slope is None
            # (hi + lo)(w_hi + w_lo) in one launch: the two-source gather reads the activation twice
            y, _ = ops.conv(h, Kp, w, src1=h, ks=spec.ks, stride=spec.stride, pad=spec.pad, bias=bias, out_f32=True)
            a = b = mr = None
            if bn is not None:
                stats = ops.bn_stats_f32(y) if training else None
                a, b, mr = ops.bn_fold(stats, y.numel() // Kp, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                       bn.num_batches_tracked, eps=bn.eps, momentum=bn.momentum, training=training)
            if save:
                st.layers.append(_Layer(spec, h, y if not last else None, a, b, mr))
            if last:
                if save:
                    st.out_pad = Kp
                return ops.nhwc_to_nchw(y, K), st
            h = ops.bn_act_fwd(y, a, b, spec.slope, split=True)
        raise RuntimeError("discriminator layer table has no output layer")

    # ------------------------------------------------------------------ backward
    def _wgrad(self, conv, x, dy, spec, landed):
        """Weight and bias gradient over both terms of the input ``x`` ([.., 2 Cp]: hi | lo) into temporaries on the
        grouped queue; ``landed`` collects what ``_land`` adds into ``.grad`` once the queue has been flushed."""
        w = conv.weight
        tw = torch.empty((dy.shape[-1], x.shape[-1], *w.shape[2:]), device=w.device, dtype=F32)
        tb = torch.empty((dy.shape[-1],), device=w.device, dtype=F32)
        ops.wgrad(x, dy, tw, db=tb, accumulate=False, ks=spec.ks, stride=spec.stride, pad=spec.pad)
        landed.append((conv, tw, tb))

    @staticmethod
    def _land(landed):
        """dW = the hi half + the lo half of the two-term weight gradient (d/dw of (hi + lo) w), cut to size."""
        for conv, tw, tb in landed:
            w = conv.weight
            K, C, cp = w.shape[0], w.shape[1], tw.shape[1] // 2
            w.grad.add_(tw[:K, :C] + tw[:K, cp:cp + C])
            conv.bias.grad.add_(tb[:K])

    def backward(self, st: DiscState, glogits, need_dx: bool = True, param_grads: bool = True):
        """``glogits``: fp32 NCHW gradient of the logits.  Accumulates into ``.grad`` of every parameter (unless
        ``param_grads`` is False: then no weight-gradient or gamma/beta work is launched) and returns the fp32 NCHW
        gradient of the raw input (None without ``need_dx``)."""
        if param_grads:
            self.ensure_grads()
        dy = ops.nchw_to_nhwc(glogits.contiguous(), st.out_pad)
        dx = None
        landed = []
        try:
            for i in range(len(st.layers) - 1, -1, -1):
                L = st.layers[i]
                spec, conv = L.spec, L.spec.conv
                if L.y is not None:   # through LeakyReLU and BatchNorm to the conv's output
                    bn = spec.norm
                    dy = ops.bn_act_bwd(dy, L.y, L.a, L.b, L.mr, slope=spec.slope, training=st.training,
                                        dgamma=bn.weight.grad if (bn is not None and param_grads) else None,
                                        dbeta=bn.bias.grad if (bn is not None and param_grads) else None,
                                        accumulate=True, skip_param_grads=not param_grads)
                if param_grads:
                    self._wg(lambda L=L, dy=dy: self._wgrad(L.spec.conv, L.x, dy, L.spec, landed))
                if i == 0 and not need_dx:
                    break
                Cin, Kp, K = L.x.shape[-1] // 2, dy.shape[-1], conv.out_channels
                wt = self.wc.get(conv.weight, 1, Kp if Kp != K else None,
                                 Cin if conv.weight.shape[1] != Cin else None)
                dy, _ = ops.conv(dy, Cin, wt, ks=spec.ks, stride=spec.stride, pad=spec.pad, transposed=True,
                                 out_hw_=tuple(L.x.shape[1:-1]))
            if need_dx:
                dx = (ops.nhwc_to_nchw(dy, st.in_channels) if st.mode == "identity" else
                      ops.image_stage_bwd(dy, st.raw, st.mode))
            self._join()
            self._land(landed)
        except BaseException:
            self.drop_saved_state()   # a failed backward leaves nothing behind for the next one
            raise
        return dx


class _DiscFunction(torch.autograd.Function):
    """raw input -> logits; parameter gradients are written into ``.grad`` (as ``_UNetFunction``)."""

    @staticmethod
    def forward(fctx, x, engine, mode, param_grads, *params):
        logits, st = engine.forward(x, mode, save=True)
        fctx.engine, fctx.state, fctx.param_grads = engine, st, param_grads
        return logits

    @staticmethod
    def backward(fctx, g):
        eng, st = fctx.engine, fctx.state
        if st is None:
            raise RuntimeError("discriminator backward called twice on one forward")
        dx = eng.backward(st, g, need_dx=fctx.needs_input_grad[0], param_grads=fctx.param_grads)
        fctx.state = None
        return (dx, None, None, None) + tuple(None for _ in eng.m.parameters())


def disc_apply(module, x, mode: str = "identity", param_grads: bool = True):
    """Logits of ``module`` for the raw fp32 NCHW batch ``x`` mapped by ``mode``, connected by autograd to ``x`` and
    (unless ``param_grads`` is False) to the parameters."""
    eng = get_disc_engine(module)
    eng.check(x)
    if mode not in ops.IMAGE_MODES:
        raise ValueError(f"image map {mode!r}: one of {sorted(ops.IMAGE_MODES)}")
    if not torch.is_grad_enabled():
        return eng.forward(x, mode, save=False)[0]
    return _DiscFunction.apply(x, eng, mode, bool(param_grads), *module.parameters())


def get_disc_engine(module) -> DiscEngine:
    eng = getattr(module, "_fmd_disc_engine", None)
    if eng is None:
        eng = DiscEngine(module)
        object.__setattr__(module, "_fmd_disc_engine", eng)
    return eng
