"""Fused HIP execution of the AutoencoderKL / VQVAE encoder and decoder (config D: encode -> denoise -> decode;
VQVAE: encoder -> HIP quantizer -> decoder, ``vq_forward``).

Walks the reference module trees (``src/nn/modules/vae/encoder.py:139-158``,
``decoder.py:133-160``, ``src/models/vae/kl.py:116-128``) with the layer
methods of ``fmdiff.runtime.engine.LayerEngine``: ResBlocks as two fused implicit-GEMM / halo convs
with GroupNorm+SiLU in the gather and skip + residual in the epilogue, stride-2 / nearest-x2
resampling inside the convs, the mid-block SpatialSelfAttention on the attention kernels, and
GroupNorm -> SiLU -> conv_out on the head kernels.  ``quant_conv`` (1x1, pointwise after conv_out) is
folded into conv_out's weights, so ``encode`` ends in one head launch; ``post_quant_conv`` runs as a
1x1 conv before the decoder (folding it into conv_in would be wrong at the zero-padded border).

AutoencoderKL also trains here (2-D, eager): ``train_encode`` / ``train_decode`` walk the same trunks under a
tape, their backwards run it the way ``UNetEngine.backward`` does, the gradient of the folded conv is unfolded
exactly onto conv_out and quant_conv (``unfold_quant_grads``), and post_quant_conv's backward is one VALU launch
(``ops.pointwise_bwd``, csrc/pointwise_bwd.hip).  ``vae_forward_train`` ties them to autograd.

VQVAE trains on the same walks (``vq_train_forward`` / ``vq_train_backward``, one autograd node,
``vqvae_forward_train``).  Its latent convs are up to 256 channels wide, so post_quant_conv's backward runs on the
MFMA weight-gradient and 1x1 conv kernels, and the quantizer's gradient joins the 1x1's fp32 data gradient in one
launch that writes the encoder head's bf16 operand (``ops.vq_join_bwd``, csrc/vq_train.hip).
Its trunks walk ``like_forward``: the small levels run on the forward-only kernels ``vq_forward`` uses and are
recomputed in the backward (``LayerEngine._replay``), so ``forward_train`` carries ``forward``'s bits.
"""
from __future__ import annotations

import torch

from . import ops
from .engine import CPAD, Act, Ctx, LayerEngine
from ..nn.blocks.residual import ResBlockND
from ..nn.params import Conv, Identity

F32 = torch.float32


class VAEEngine(LayerEngine):
    def __init__(self, module):
        super().__init__(module, dims1=False)   # 2-D models only (spatial_dims checked on entry)
        self._fold = None       # conv_out with quant_conv folded in (_folded_out)
        self._fold_key = None

    def _ctx(self, part, N, dev, save=False, like_forward=False):
        emb = None
        if part.emb_channels is not None:   # the reference feeds zeros (encoder.py:141-144)
            emb = torch.zeros((N, part.emb_channels), device=dev, dtype=F32)
        ctx = Ctx(emb, False, N)
        if save:   # training walks have no embedding (check_trainable): a tape, no demb
            ctx.tape = []
            ctx.like_forward = like_forward
        return ctx

    def _stage(self, x):
        """NCHW fp32 -> NHWC bf16 with CPAD-padded channels."""
        ops._need_cuda(x, type(self.m).__name__)
        Cp = max(CPAD, -(-x.shape[1] // 8) * 8)
        return ops.noise_prepare(None, x.float().contiguous(), None, None, None, Cp)

    def _mid(self, part, h, ctx):
        h = self.res_block(part.mid_block1, [h], ctx)
        if not isinstance(part.mid_attn, Identity):
            h = self.attention(part.mid_attn, h, ctx)
        return self.res_block(part.mid_block2, [h], ctx)

    def _encoder_trunk(self, enc, x, save=False, like_forward=False):
        if enc.spatial_dims != 2:
            raise NotImplementedError("fmdiff VAE engine: spatial_dims=2")
        ctx = self._ctx(enc, x.shape[0], x.device, save, like_forward)
        h = self.conv_layer(enc.conv_in.conv, Act(self._stage(x), need_grad=False), ctx)
        for stage in enc.downs:
            for i, blk in enumerate(stage.blocks):
                h = self.res_block(blk, [h], ctx)
                if i < len(stage.attns):
                    h = self.attention(stage.attns[i], h, ctx)
            if hasattr(stage, "down"):
                h = self._apply(stage.down, h, ctx)
        return self._mid(enc, h, ctx), ctx

    def _decoder_trunk(self, dec, hin: Act, ctx):
        if dec.tanh_out:
            raise NotImplementedError("fmdiff VAE engine: tanh_out decoders")
        h = self.conv_layer(dec.conv_in.conv, hin, ctx)
        h = self._mid(dec, h, ctx)
        for stage in reversed(dec.ups):
            for i, blk in enumerate(stage.blocks):
                h = self.res_block(blk, [h], ctx)
                if i < len(stage.attns):
                    h = self.attention(stage.attns[i], h, ctx)
            if hasattr(stage, "up"):
                h = self._apply(stage.up, h, ctx)
        return self.head(dec.norm_out, dec.conv_out.conv, h, ctx)

    # ------------------------------------------------------------ entry points
    @torch.no_grad()
    def encoder_forward(self, x):
        """Encoder.forward: NCHW fp32 -> NCHW fp32 moments before quant_conv."""
        enc = self.m
        h, ctx = self._encoder_trunk(enc, x)
        out = self.head(enc.norm_out, enc.conv_out.conv, h, ctx)
        return ops.nhwc_to_nchw(out, enc.conv_out.conv.out_channels)

    def _folded_out(self, vae) -> Conv:
        """conv_out followed by the 1x1 quant_conv as one 3x3 conv: W = Wq . Wout, b = Wq bout + bq
        (exact: quant_conv is pointwise after conv_out)."""
        co, qc = vae.encoder.conv_out.conv, vae.quant_conv.conv
        key = tuple((t._version, t.data_ptr()) for t in (co.weight, co.bias, qc.weight, qc.bias))
        if key != self._fold_key:
            if self._fold is None:
                self._fold = Conv(2, co.in_channels, qc.out_channels, 3, padding=1).to(co.weight.device)
            wq = qc.weight.detach().reshape(qc.out_channels, -1)
            self._fold.weight.data.copy_(torch.einsum("oz,zchw->ochw", wq, co.weight.detach()))
            self._fold.bias.data.copy_(wq @ co.bias.detach() + qc.bias.detach())
            self._fold_key = key
        return self._fold

    def _encode_nhwc(self, x):
        """Encoder + folded quant_conv: (fp32 NHWC [B, h, w, Kp], the valid channel count)."""
        vae = self.m
        h, ctx = self._encoder_trunk(vae.encoder, x)
        fold = self._folded_out(vae)
        return self.head(vae.encoder.norm_out, fold, h, ctx), fold.out_channels

    @torch.no_grad()
    def encode_moments(self, x):
        """AutoencoderKL.encode up to the DiagonalGaussian parameters: NCHW fp32 -> [B, 2*embed_dim, h, w]
        (VQVAE.encode: the quantizer's input [B, embed_dim, h, w])."""
        out, K = self._encode_nhwc(x)
        return ops.nhwc_to_nchw(out, K)

    @torch.no_grad()
    def decoder_forward(self, z):
        dec = self.m
        ctx = self._ctx(dec, z.shape[0], z.device)
        out = self._decoder_trunk(dec, Act(self._stage(z), need_grad=False), ctx)
        return ops.nhwc_to_nchw(out, dec.conv_out.conv.out_channels)

    @torch.no_grad()
    def decode(self, z):
        """AutoencoderKL.decode / VQVAE.decode (denorm handled by the caller): post_quant_conv, then the decoder."""
        return self._decode_staged(self._stage(z))

    def _decode_staged(self, zin):
        """post_quant_conv + decoder from the staged latent (NHWC bf16, CPAD-padded channels)."""
        vae = self.m
        dec, pq = vae.decoder, vae.post_quant_conv.conv
        Kp = max(CPAD, -(-pq.out_channels // 8) * 8)
        hz, _ = ops.conv(zin, Kp, self.wc.get(pq.weight, 0, Kp, zin.shape[-1]), ks=1, pad=0,
                         bias=self.wc.padded(pq.bias, Kp))
        ctx = self._ctx(dec, zin.shape[0], zin.device)
        out = self._decoder_trunk(dec, Act(hz, need_grad=False), ctx)
        return ops.nhwc_to_nchw(out, dec.conv_out.conv.out_channels)

    @torch.no_grad()
    def vq_forward(self, x):
        """VQVAE.forward: encoder -> quantizer -> post_quant_conv -> decoder.  The quantizer reads the head's
        fp32 NHWC output in place and writes the decoder's staged operand itself (the bf16 rounding of z_q that
        ``_stage`` would make), so ``rec`` equals ``decode(codebook(encode(x))[0])`` bit for bit.  Returns
        (rec NCHW fp32, ops.VQOut)."""
        vae = self.m
        quant_in, D = self._encode_nhwc(x)
        q = vae.codebook.quantize_nhwc(quant_in, Cpad=max(CPAD, -(-D // 8) * 8))
        return self._decode_staged(q.zq_nhwc), q

    @torch.no_grad()
    def kl_forward(self, x, eps=None, sample=True):
        """AutoencoderKL.forward for training: encoder -> posterior kernel -> post_quant_conv -> decoder.  The
        posterior kernel (``ops.gauss_sample_kl``) reads the head's fp32 NHWC moments in place, samples (``eps``
        fp32 ``[B, embed_dim, h, w]``; None: drawn with ``torch.randn``; ``sample=False``: the mode), sums the KL
        and writes the decoder's staged operand itself (the bf16 rounding of z that ``_stage`` would make), so
        ``rec`` equals ``decode(z)`` bit for bit.  Returns (rec NCHW fp32, z NCHW fp32, kl [B])."""
        mom, K = self._encode_nhwc(x)
        E = K // 2
        if not sample:
            eps = None
        elif eps is None:
            eps = torch.randn((mom.shape[0], E, *mom.shape[1:-1]), device=mom.device, dtype=F32)
        z, kl, zs = ops.gauss_sample_kl(mom, E, eps, Cp=max(CPAD, -(-E // 8) * 8))
        return self._decode_staged(zs), z, kl


    # ------------------------------------------------------------ training (2-D, eager; AutoencoderKL first)
    def check_trainable(self):
        """Refuse what the trunk backward is not built (or not checked) for."""
        vae = self.m
        what = "fmdiff VAE training"
        if not hasattr(vae, "quant_conv"):
            raise NotImplementedError(f"{what}: AutoencoderKL and VQVAE only")
        enc, dec, pq = vae.encoder, vae.decoder, vae.post_quant_conv.conv
        if enc.spatial_dims != 2 or dec.spatial_dims != 2:
            raise NotImplementedError(f"{what}: spatial_dims=2")
        if dec.tanh_out:
            raise NotImplementedError(f"{what}: tanh_out decoders")
        if enc.emb_channels is not None or dec.emb_channels is not None:
            raise NotImplementedError(f"{what}: emb_channels (no reference path to check the embedding against)")
        if any(isinstance(mod, ResBlockND) and float(mod.dropout or 0.0) > 0 for mod in vae.modules()):
            raise NotImplementedError(f"{what}: dropout > 0")
        if hasattr(vae, "codebook"):   # the latent convs on the MFMA routes: the quantizer's own limit
            if pq.in_channels > VQ_MAX_EMBED:
                raise NotImplementedError(f"{what}: embed_dim up to {VQ_MAX_EMBED} (the quantizer kernels), got "
                                          f"{pq.in_channels}")
        elif max(pq.in_channels, pq.out_channels) > ops.POINTWISE_MAXC:
            raise NotImplementedError(f"{what}: z_channels and embed_dim up to {ops.POINTWISE_MAXC} (the latent 1x1 "
                                      f"backward kernel), got {pq.out_channels} and {pq.in_channels}")

    def ensure_grads(self):
        for p in self.m.parameters():
            if p.grad is None:
                p.grad = torch.zeros_like(p)

    def invalidate_weights(self):
        """After an optimizer that writes the parameters through raw pointers (no ``_version`` bump): re-derive
        the bf16 kernel layouts and drop the folded conv_out, which is rebuilt from the masters on its next use."""
        self._fold_key = None
        if self._fold is not None:   # before the layouts: the fold's own bf16 copies are derived from it
            self._folded_out(self.m)
        super().invalidate_weights()

    def _run_backward(self, head_bwd, dpred, tape):
        """What UNetEngine.backward does around its tape: batched GroupNorm folds, the head first, the tape in
        reverse, every weight gradient landed on return."""
        ops.gb_defer()
        try:
            head_bwd(dpred)
            for fn in reversed(tape):
                fn()
            self._join()
        except BaseException:
            self.drop_saved_state()   # a failed backward leaves nothing behind for the next one
            raise
        finally:
            ops.gb_flush()
        self._join()

    def train_encode(self, x, like_forward=False):
        """Encoder + folded quant_conv under a tape: (fp32 NHWC moments [N, h, w, Kp], state for the backward).
        ``like_forward``: the small levels on the forward-only kernels, their backward recomputed
        (``LayerEngine._replay``), so that the moments are ``_encode_nhwc``'s bit for bit."""
        self.check_trainable()
        vae = self.m
        enc = vae.encoder
        h, ctx = self._encoder_trunk(enc, x, save=True, like_forward=like_forward)
        fold = self._folded_out(vae)
        mom = self.head(enc.norm_out, fold, h, ctx)
        head_bwd, self._head_bwd = self._head_bwd, None   # one slot: the decoder's head would overwrite it
        return mom, (ctx, head_bwd)

    def train_encode_backward(self, state, dmom):
        """``dmom``: bf16 NHWC gradient of the moments (padding channels zero).  Accumulates into ``.grad`` of the
        encoder and of quant_conv (the fold's gradient unfolded exactly)."""
        ctx, head_bwd = state
        vae = self.m
        fold = self._fold
        for p in (fold.weight, fold.bias):
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        self._run_backward(head_bwd, dmom, ctx.tape)
        ctx.tape = None
        co, qc = vae.encoder.conv_out.conv, vae.quant_conv.conv
        dwo, dbo, dwq, dbq = unfold_quant_grads(qc.weight.detach().reshape(qc.out_channels, -1), co.weight.detach(),
                                                co.bias.detach(), fold.weight.grad, fold.bias.grad)
        co.weight.grad.add_(dwo)
        co.bias.grad.add_(dbo)
        qc.weight.grad.add_(dwq.view_as(qc.weight))
        qc.bias.grad.add_(dbq)
        fold.weight.grad.zero_()
        fold.bias.grad.zero_()

    def train_decode(self, zs, like_forward=False):
        """post_quant_conv + decoder under a tape from the staged latent: (fp32 NHWC output, state).
        ``like_forward``: as in ``train_encode``; the output is ``_decode_staged``'s bit for bit."""
        self.check_trainable()
        vae = self.m
        dec, pq = vae.decoder, vae.post_quant_conv.conv
        Kp = max(CPAD, -(-pq.out_channels // 8) * 8)
        hz, _ = ops.conv(zs, Kp, self.wc.get(pq.weight, 0, Kp, zs.shape[-1]), ks=1, pad=0,
                         bias=self.wc.padded(pq.bias, Kp))
        ctx = self._ctx(dec, zs.shape[0], zs.device, save=True, like_forward=like_forward)
        hin = Act(hz, need_grad=True)
        out = self._decoder_trunk(dec, hin, ctx)
        head_bwd, self._head_bwd = self._head_bwd, None
        return out, (ctx, head_bwd, hin, zs)

    def train_decode_backward(self, state, dpred):
        """``dpred``: bf16 NHWC gradient of the decoder output.  Accumulates into ``.grad`` of the decoder and of
        post_quant_conv; returns ``g_z``, the fp32 channels-first gradient of the latent."""
        ctx, head_bwd, hin, zs = state
        pq = self.m.post_quant_conv.conv
        self._run_backward(head_bwd, dpred, ctx.tape)
        ctx.tape = None
        g_z, _, _ = ops.pointwise_bwd(hin.grad, zs, pq.weight.detach().reshape(pq.out_channels, pq.in_channels),
                                      dW=pq.weight.grad, db=pq.bias.grad, accumulate=True)
        return g_z

    # ------------------------------------------------------------ training (VQVAE, 2-D, eager)
    def vq_train_forward(self, x):
        """``vq_forward`` under a tape: encoder trunk, head with the folded quant_conv, the quantizer's training
        call (a training-mode EMA codebook has been updated when this returns), post_quant_conv as the MFMA 1x1 on
        the staged z_q, decoder trunk.  Both trunks walk ``like_forward``: in eval mode, and for the classic quantizer,
        rec, vq_loss, perplexity and codes are ``vq_forward``'s bit for bit.  Returns (fp32 NHWC decoder output, ops.VQOut, state for the backward)."""
        self.check_trainable()
        vae = self.m
        quant_in, enc_state = self.train_encode(x, like_forward=True)
        D = vae.codebook.embedding_dim
        q, saved = vae.codebook.quantize_train_saved(quant_in, Cpad=max(CPAD, -(-D // 8) * 8))
        out, dec_state = self.train_decode(q.zq_nhwc, like_forward=True)
        return out, q, (enc_state, dec_state, saved, vae.codebook._latent_coef(), D, quant_in.shape[-1])

    def vq_train_backward(self, state, dpred, g_loss):
        """``dpred``: bf16 NHWC gradient of the decoder output; ``g_loss``: one-element fp32 device tensor, the
        gradient of vq_loss (None: zero).  Decoder tape, then post_quant_conv's backward on the MFMA routes (the
        1x1 weight gradient and the transposed 1x1 as data gradient, stored fp32), then the latent join
        (``ops.vq_join_bwd``) straight into the bf16 operand of the encoder head's backward, then the encoder tape
        and the unfold.  Between the data gradient and the head's backward there is the join kernel and nothing
        else.  Accumulates into ``.grad`` of every trunk parameter; the codebook gets none (as in the reference)."""
        enc_state, (dctx, dec_head_bwd, hin, zs), saved, c, D, Kp = state
        pq = self.m.post_quant_conv.conv
        Z, Zp, Dp = pq.out_channels, hin.t.shape[-1], zs.shape[-1]
        self._run_backward(dec_head_bwd, dpred, dctx.tape)
        dctx.tape = None
        dy = hin.grad   # bf16 [N, h, w, Zp], padding channels zero (conv_in's padded weight rows are zero)
        if Zp == Z and Dp == D:
            ops.wgrad(zs, dy, pq.weight.grad, ks=1, pad=0, db=pq.bias.grad, immediate=True)
        else:   # padded channels: through zeroed fp32 temporaries cut to size, as the head's own weight gradient
            tmpw = torch.zeros((Zp, Dp, 1, 1), device=dy.device, dtype=F32)
            tmpb = torch.zeros((Zp,), device=dy.device, dtype=F32)
            ops.wgrad(zs, dy, tmpw, ks=1, pad=0, db=tmpb, accumulate=False, immediate=True)
            pq.weight.grad.add_(tmpw[:Z, :D])
            pq.bias.grad.add_(tmpb[:Z])
        g, _ = ops.conv(dy, Dp, self.wc.get(pq.weight, 1, Zp, Dp), ks=1, pad=0, transposed=True,
                        out_hw_=tuple(dy.shape[1:-1]), out_f32=True)
        if len(saved) == 1:   # the EMA update has overwritten the codebook: the saved residual z - q
            dz = ops.vq_join_bwd(g, D, saved[0], None, None, g_loss, c, ld_out=Kp)
        else:
            z, codes, e, _ = saved
            dz = ops.vq_join_bwd(g, D, z, codes, e, g_loss, c, ld_out=Kp)
        self.train_encode_backward(enc_state, dz)


def unfold_quant_grads(wq, w_out, b_out, dwf, dbf):
    """Gradients of ``conv_out`` and ``quant_conv`` from those of their fold ``W_f = W_q . W_out``,
    ``b_f = W_q b_out + b_q`` (``VAEEngine._folded_out``).  ``wq`` [O, Z], ``w_out`` [Z, C, kh, kw], ``b_out`` [Z],
    ``dwf`` [O, C, kh, kw], ``dbf`` [O].  Returns ``(dW_out, db_out, dW_q [O, Z], db_q)``; tensors in, tensors out."""
    dw_out = torch.einsum("oz,ochw->zchw", wq, dwf)
    db_out = wq.t() @ dbf
    dwq = torch.einsum("ochw,zchw->oz", dwf, w_out) + dbf[:, None] * b_out[None, :]
    return dw_out, db_out, dwq, dbf.clone()


class _VAEEncodeFunction(torch.autograd.Function):
    """x -> the channels-last fp32 moments; parameter gradients are written into ``.grad`` (as _UNetFunction)."""

    @staticmethod
    def forward(fctx, x, engine, *params):
        mom, state = engine.train_encode(x)
        fctx.engine, fctx.state = engine, state
        return mom

    @staticmethod
    def backward(fctx, gmom):
        eng = fctx.engine
        eng.ensure_grads()
        eng.train_encode_backward(fctx.state, gmom.contiguous().to(torch.bfloat16))
        fctx.state = None
        return (None, None) + tuple(None for _ in eng.m.parameters())


class _VAEDecodeFunction(torch.autograd.Function):
    """(z, its staged bf16 copy) -> rec NCHW fp32.  ``z`` only carries the graph: the decoder reads the staged
    operand.  Backward runs the decoder's tape, then the latent 1x1's backward, and returns ``g_z``."""

    @staticmethod
    def forward(fctx, z, zs, engine, *params):
        out, state = engine.train_decode(zs)
        fctx.engine, fctx.state, fctx.kpad = engine, state, out.shape[-1]
        return ops.nhwc_to_nchw(out, engine.m.decoder.conv_out.conv.out_channels)

    @staticmethod
    def backward(fctx, grec):
        eng = fctx.engine
        eng.ensure_grads()
        g_z = eng.train_decode_backward(fctx.state, ops.nchw_to_nhwc(grec.contiguous(), fctx.kpad))
        fctx.state = None
        return (g_z, None, None) + tuple(None for _ in eng.m.parameters())


def vae_forward_train(module, x, eps=None, sample_posterior=True):
    """AutoencoderKL.forward_train: (rec NCHW fp32, z NCHW fp32, kl [N]), connected to the parameters by autograd."""
    from ..nn.modules.vae import reparameterize_kl
    eng = get_vae_engine(module)
    eng.check_trainable()
    ops._need_cuda(x, f"{type(module).__name__}.forward_train")
    params = list(module.parameters())
    E = module.post_quant_conv.conv.in_channels
    mom = _VAEEncodeFunction.apply(x, eng, *params)
    z, kl, zs = reparameterize_kl(mom, eps, sample_posterior, channels_last=True, embed_dim=E,
                                  staged_channels=max(CPAD, -(-E // 8) * 8))
    rec = _VAEDecodeFunction.apply(z, zs, eng, *params)
    return rec, z, kl


class _VQVAETrainFunction(torch.autograd.Function):
    """x -> (rec NCHW fp32, vq_loss, perplexity, codes): the whole VQVAE training forward as one node, so that the
    latent gradient stays the engine's own bf16 channels-last tensor from the 1x1's data gradient to the encoder
    head (autograd would cast the gradient of an fp32 latent to fp32).  Parameter gradients are written into
    ``.grad``; perplexity and codes carry none."""

    @staticmethod
    def forward(fctx, x, engine, *params):
        out, q, state = engine.vq_train_forward(x)
        fctx.engine, fctx.state, fctx.kpad = engine, state, out.shape[-1]
        fctx.mark_non_differentiable(q.perplexity, q.codes)
        return ops.nhwc_to_nchw(out, engine.m.decoder.conv_out.conv.out_channels), q.vq_loss, q.perplexity, q.codes

    @staticmethod
    def backward(fctx, grec, gloss, *_):
        eng = fctx.engine
        eng.ensure_grads()
        eng.vq_train_backward(fctx.state, ops.nchw_to_nhwc(grec.contiguous(), fctx.kpad),
                              gloss.float().reshape(1))
        fctx.state = None
        return (None, None) + tuple(None for _ in eng.m.parameters())


def vqvae_forward_train(module, x):
    """VQVAE.forward_train: (rec NCHW fp32, vq_loss, perplexity, codes); ``rec`` and ``vq_loss`` are connected to
    the parameters by autograd."""
    eng = get_vae_engine(module)
    eng.check_trainable()
    ops._need_cuda(x, f"{type(module).__name__}.forward_train")
    return _VQVAETrainFunction.apply(x, eng, *module.parameters())


VQ_MAX_EMBED = 256   # widest code the quantizer kernels take (csrc/vq.hip, csrc/vq_train.hip)


def get_vae_engine(module) -> VAEEngine:
    eng = getattr(module, "_fmd_vae_engine", None)
    if eng is None:
        eng = VAEEngine(module)
        object.__setattr__(module, "_fmd_vae_engine", eng)
    return eng
