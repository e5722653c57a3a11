"""AutoencoderKL training on the engine (MI355X): the latent 1x1 backward kernel against its derived bound, gradient
parity of ``forward_train`` with torch autograd over the CPU oracle (``oracle/vae.py``), ``VAETrainStep`` against
the hand-written composition and torch's AdamW, a short descent against the oracle's, and the weight caches.

Gradient tolerances are the project's own for UNet gradients (tests/test_gpu_unet.py): loss
within 1e-2 relative, relative L2 over all parameters < 5e-2, cosine > 0.99 for every tensor whose reference
gradient exceeds 1e-3 of the running total norm.  The oracle's values are kept away from the clamp and sign kinks
(asserted), so no mask can flip under bf16 noise; those paths are pinned by tests/test_gpu_vae_loss.py."""
import json
import math
import os
import warnings

import pytest
import torch
import torch.nn.functional as F

import pointwise_bounds as PB

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
KL_WEIGHT = 1e-3
_CACHE = {}


# ------------------------------------------------------------------ the kernel
def _kernel_case(N, h, w, Z, E):
    key = ("kernel", N, h, w, Z, E)
    if key not in _CACHE:
        g = torch.Generator().manual_seed(1000 * Z + 10 * E + N)
        M = N * h * w
        dy, x = PB.bf16_valued((M, Z), g, 0.5), PB.bf16_valued((M, E), g)
        W = torch.randn((Z, E), generator=g) / 2
        old_w, old_b = torch.randn((Z, E), generator=g), torch.randn((Z,), generator=g)
        _CACHE[key] = (dy, x, W, old_w, old_b, PB.exact(dy, x, W))
    return _CACHE[key]


def _padded(t, N, h, w, ld):
    """[M, C] fp32 -> device bf16 [N, h, w, ld] with NaN in the padding channels."""
    out = torch.full((t.shape[0], ld), float("nan"))
    out[:, :t.shape[1]] = t
    return out.reshape(N, h, w, ld).to(torch.bfloat16).cuda()


@pytest.mark.parametrize("Z,E", [(4, 4), (3, 5), (8, 8), (1, 1)])
@pytest.mark.parametrize("N,h,w", [(3, 5, 7), (2, 33, 32)])
def test_pointwise_bwd_within_the_derived_bound(N, h, w, Z, E):
    """Every output element of ``ops.pointwise_bwd`` within ``2^-24 |v| + gamma_n sum |terms|`` of the exact value
    (tests/pointwise_bounds.py), for both row strides, both layouts of g, store and accumulate; NaN in the padding
    channels of dy and x reaches no output; channels-last padding is exactly zero; two runs are bit-identical."""
    from fmdiff.runtime import ops
    dy, x, W, old_w, old_b, ((ge, dWe, dbe), (ga, dWa, dba)) = _kernel_case(N, h, w, Z, E)
    M = N * h * w
    Wd = W.cuda()
    for ldy, ldx in ((8, 16), (16, 8)):
        dyd, xd = _padded(dy, N, h, w, ldy), _padded(x, N, h, w, ldx)
        assert torch.isnan(dyd).any() == (Z < ldy) and torch.isnan(xd).any() == (E < ldx)
        for cl in (False, True):
            for acc in (False, True):
                dW = old_w.cuda() if acc else torch.full((Z, E), float("nan"), device="cuda")
                db = old_b.cuda() if acc else torch.full((Z,), float("nan"), device="cuda")
                g, _, _ = ops.pointwise_bwd(dyd, xd, Wd, channels_last=cl, ldg=16 if cl else None, dW=dW, db=db,
                                            accumulate=acc)
                dW2 = old_w.cuda() if acc else torch.empty((Z, E), device="cuda")
                db2 = old_b.cuda() if acc else torch.empty((Z,), device="cuda")
                g2, _, _ = ops.pointwise_bwd(dyd, xd, Wd, channels_last=cl, ldg=16 if cl else None, dW=dW2, db=db2,
                                             accumulate=acc)
                assert torch.equal(g, g2) and torch.equal(dW, dW2) and torch.equal(db, db2)
                gc = g.cpu()
                if cl:
                    assert gc.shape == (N, h, w, 16) and (gc[..., E:] == 0).all()
                    gm = gc[..., :E].reshape(M, E)
                else:
                    assert gc.shape == (N, E, h, w)
                    gm = gc.permute(0, 2, 3, 1).reshape(M, E)
                for got, v, at, n, old in ((gm, ge, ga, Z, None), (dW.cpu(), dWe, dWa, M, old_w if acc else None),
                                           (db.cpu(), dbe, dba, M, old_b if acc else None)):
                    assert not torch.isnan(got).any()
                    want = v if old is None else old.double() + v
                    err, bd = (got.double() - want).abs(), PB.bound(v, at, n, old)
                    assert (err <= bd).all(), (ldy, ldx, cl, acc, n, (err / bd.clamp_min(1e-300)).max().item())
    # g alone (no sums, no x) and the sums alone give the same bits
    dyd, xd = _padded(dy, N, h, w, 8), _padded(x, N, h, w, 8)
    ga_, _, _ = ops.pointwise_bwd(dyd, None, Wd)
    dW, db = torch.empty((Z, E), device="cuda"), torch.empty((Z,), device="cuda")
    gb_, _, _ = ops.pointwise_bwd(dyd, xd, Wd, dW=dW, db=db)
    dW3, db3 = torch.empty((Z, E), device="cuda"), torch.empty((Z,), device="cuda")
    assert ops.pointwise_bwd(dyd, xd, Wd, want_g=False, dW=dW3, db=db3)[0] is None
    assert torch.equal(ga_, gb_) and torch.equal(dW, dW3) and torch.equal(db, db3)


def test_pointwise_bwd_refuses_more_than_eight_channels():
    from fmdiff import _lib
    from fmdiff.runtime import ops
    dy = torch.zeros((2, 4, 4, 16), dtype=torch.bfloat16, device="cuda")
    W = torch.zeros((9, 4), device="cuda")
    g = torch.zeros((2, 4, 4, 4), device="cuda")
    L = _lib.lib()
    assert L.fmd_pointwise_bwd_workspace(32, 9, 4) == -1 and L.fmd_pointwise_bwd_workspace(32, 4, 9) == -1
    rc = L.fmd_pointwise_bwd(dy.data_ptr(), 16, None, 0, W.data_ptr(), 2, 16, 9, 4, g.data_ptr(), 0, 0, None, None, 0,
                             None, ops.stream())
    assert rc == -1
    with pytest.raises(ValueError, match="limit"):
        ops.pointwise_bwd(dy, None, W)
    with pytest.raises(ValueError, match="limit"):
        ops.pointwise_bwd(dy, None, torch.zeros((4, 9), device="cuda"))
    torch.cuda.synchronize()


# ------------------------------------------------------------------ the oracle
def _golden():
    if "golden" not in _CACHE:
        G = torch.load(os.path.join(HERE, "golden", "vae_golden.pt"), weights_only=True)
        cfg = json.loads(bytes(G["cfg_json"].tolist()).decode())
        state = {k: v.clone() for k, v in G["state"].items()}
        for k in ("decoder.conv_out.conv.weight", "decoder.conv_out.conv.bias"):
            state[k] = state[k] * 0.25    # keeps |rec| below the clamp of raw_output_to_image
        _CACHE["golden"] = (cfg, state, G["x"].clone())
    return _CACHE["golden"]


SHAPE2_CFG = dict(in_channels=3, out_channels=3, resolution=32, base_ch=32, down_channels=[32, 64], num_res_blocks=1,
                  attn_resolutions=[16], z_channels=3, embed_dim=3, dropout=0.0, use_attention=True, spatial_dims=2,
                  emb_channels=None, use_scale_shift_norm=False, double_z=True, attn_heads=4, attn_dim_head=16)


def _build(cfg, state=None):
    from fmdiff.models.vae import AutoencoderKL
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vae = AutoencoderKL(**cfg)
    if state is not None:
        vae.load_state_dict(state)
    return vae


def _shape2():
    """The second shape: parameters seeded by the recipe of tests/golden/make_vae_golden.py, applied to the fmdiff
    module; the oracle gets them as a state_dict."""
    if "shape2" not in _CACHE:
        vae = _build(SHAPE2_CFG)
        g = torch.Generator().manual_seed(4321)
        with torch.no_grad():
            for name, p in vae.named_parameters():
                fan = p[0].numel() if p.dim() > 1 else 1
                if name.endswith("norm1.weight") or name.endswith("norm2.weight") or ".norm" in name and name.endswith("weight"):
                    p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
                elif p.dim() == 1:
                    p.copy_(0.05 * torch.randn(p.shape, generator=g))
                else:
                    p.copy_(torch.randn(p.shape, generator=g) / math.sqrt(fan))
            for p in (vae.decoder.conv_out.conv.weight, vae.decoder.conv_out.conv.bias):
                p.mul_(0.25)
        x = torch.rand(3, 3, 32, 48, generator=g)
        _CACHE["shape2"] = (SHAPE2_CFG, {k: v.detach().clone() for k, v in vae.state_dict().items()}, x)
    return _CACHE["shape2"]


def _oracle_forward(sd, cfg, x, eps):
    """(rec, kl [N], logvar) of the reference's training forward; ``eps=None``: the mode."""
    from oracle import vae as OV
    mom = OV.encode_moments(sd, cfg, x * 2.0 - 1.0)
    mu, logvar = mom.chunk(2, dim=1)
    lv = logvar.clamp(-30.0, 20.0)
    z = mu if eps is None else mu + torch.exp(0.5 * lv) * eps
    kl = 0.5 * torch.sum(mu.pow(2) + torch.exp(lv) - 1.0 - lv, dim=(1, 2, 3))
    return OV.decode(sd, cfg, z), kl, logvar


def _oracle_loss(rec, kl, target, recon):
    img = (rec.clamp(-1.0, 1.0) + 1.0) * 0.5
    return (F.mse_loss(img, target) if recon == "mse" else F.l1_loss(img, target)) + KL_WEIGHT * kl.mean()


def _oracle_grads(cfg, state, x, eps, recon, target_fn=None):
    """Loss and gradients of torch autograd over the oracle on the CPU, with the conditions on its values that keep
    every clamp mask and sign fixed.  ``target_fn(img_ref) -> target``; default: the input image."""
    sd = {k: v.clone().requires_grad_() for k, v in state.items()}
    rec, kl, logvar = _oracle_forward(sd, cfg, x, eps)
    assert rec.abs().max().item() <= 0.9, rec.abs().max().item()
    assert -30.0 < logvar.min().item() and logvar.max().item() < 20.0
    target = x
    if target_fn is not None:
        img = ((rec.detach().clamp(-1.0, 1.0) + 1.0) * 0.5)
        target = target_fn(img)
        assert (img - target).abs().min().item() >= 0.2
    loss = _oracle_loss(rec, kl, target, recon)
    loss.backward()
    return loss.item(), {k: v.grad for k, v in sd.items()}, target


def _engine_loss(vae, x, eps, recon, target, sample=True):
    from fmdiff.nn.losses import recon_loss
    rec, z, kl = vae.forward_train(vae.image_to_model_range(x), eps, sample_posterior=sample)
    return recon_loss(rec, target, recon) + KL_WEIGHT * kl.mean(), rec, z, kl


def _compare(vae, ref, loss, loss_ref, what):
    num = den = 0.0
    worst = (1.0, None)
    gated = []
    for k, p in vae.named_parameters():
        g = p.grad.double().cpu()
        r = ref[k].double()
        num += (g - r).pow(2).sum().item()
        den += r.pow(2).sum().item()
        if r.norm() > 1e-3 * math.sqrt(den + 1e-30):
            gated.append(k)
            cos = ((g * r).sum() / (g.norm() * r.norm() + 1e-30)).item()
            if cos < worst[0]:
                worst = (cos, k)
    rel = math.sqrt(num / den)
    print(f"[{what}] loss hip={loss:.6f} oracle={loss_ref:.6f}; grad rel L2 {rel:.3e}; worst cosine {worst[0]:.5f} "
          f"({worst[1]}) over {len(gated)} gated tensors")
    assert abs(loss - loss_ref) <= 1e-2 * abs(loss_ref)
    assert rel < 5e-2
    assert worst[0] > 0.99, worst
    return gated


def _parity(cfg, state, x, eps, recon, what, target_fn=None):
    loss_ref, ref, target = _oracle_grads(cfg, state, x, eps, recon, target_fn)
    vae = _build(cfg, state).cuda()
    loss, rec, z, kl = _engine_loss(vae, x.cuda(), None if eps is None else eps.cuda(), recon, target.cuda(),
                                    sample=eps is not None)
    assert rec.shape == x.shape and rec.dtype == torch.float32 and kl.shape == (x.shape[0],)
    loss.backward()
    torch.cuda.synchronize()
    return vae, _compare(vae, ref, loss.item(), loss_ref, what)


def test_gradient_parity_mse_sampled():
    """The fixture model (32^2, channels 32/64/64, mid attention, 144 parameter tensors), mse + 1e-3 KL, seeded eps:
    at this KL weight the quant_conv rows and post_quant_conv clear the cosine gate (asserted)."""
    cfg, state, x = _golden()
    eps = torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(77))
    vae, gated = _parity(cfg, state, x, eps, "mse", "mse, sampled")
    assert len(list(vae.parameters())) == 144
    for k in ("quant_conv.conv.weight", "post_quant_conv.conv.weight", "encoder.conv_out.conv.weight",
              "decoder.conv_in.conv.weight", "encoder.conv_in.conv.weight"):
        assert k in gated, k
    eng = vae._fmd_vae_engine
    assert eng._head_bwd is None and not eng._fold.weight.grad.any() and not eng._fold.bias.grad.any()


def test_gradient_parity_l1_mode():
    """l1 and ``sample_posterior=False`` (no eps: z is the mode); the target is placed a quarter away from the
    oracle's reconstruction so that no sign of img - target can flip."""
    cfg, state, x = _golden()
    _parity(cfg, state, x, None, "l1", "l1, mode",
            target_fn=lambda img: torch.where(img < 0.5, img + 0.25, img - 0.25))


def test_gradient_parity_second_shape():
    """3 image channels, z_channels = embed_dim = 3 (6 valid moment channels + 2 padding), channels 32/64 with
    attention at resolution 16, batch 3, a non-square 32x48 input."""
    cfg, state, x = _shape2()
    eps = torch.randn((3, 3, 16, 24), generator=torch.Generator().manual_seed(5))
    vae, gated = _parity(cfg, state, x, eps, "mse", "second shape")
    assert "quant_conv.conv.weight" in gated and "encoder.conv_out.conv.weight" in gated
    from fmdiff.runtime.vae_engine import get_vae_engine
    mom, _ = get_vae_engine(vae).train_encode((x * 2.0 - 1.0).cuda())
    assert mom.shape == (3, 16, 24, 8) and (mom[..., 6:] == 0).all()


# ------------------------------------------------------------------ the step
TRAIN_CFG = {"recon_type": "mse", "kl_weight": KL_WEIGHT, "gan_weight": 0.0, "perceptual_weight": 0.0}


def test_train_step_equals_the_composition_and_torch_adamw():
    from fmdiff.pipelines.train.vae_lib import VAECriterion, VAETrainStep
    cfg, state, x = _golden()
    lr, wd = 1e-3, 0.01
    xd = x.cuda()
    eps = [torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(s)).cuda() for s in (77, 78)]
    # the hand-written composition
    ref = _build(cfg, state).cuda()
    rec, _, kl = ref.forward_train(ref.image_to_model_range(xd), eps[0])
    out_ref = VAECriterion(TRAIN_CFG)(rec, xd, kl=kl, global_step=0)
    out_ref["loss"].backward()
    # the step
    vae = _build(cfg, state).cuda()
    step = VAETrainStep(vae, TRAIN_CFG, lr=lr, weight_decay=wd)
    out = step.step(xd, eps[0])
    torch.cuda.synchronize()
    assert set(out) == set(out_ref) and step.global_step == 1
    for k in out:
        assert out[k].is_cuda and out[k].dim() == 0 and torch.equal(out[k], out_ref[k].detach()), k
    for (k, p), q in zip(vae.named_parameters(), ref.parameters()):
        assert torch.equal(p.grad, q.grad), k
    # torch's AdamW on the CPU, fed the engine's own gradients
    cpu = {k: torch.nn.Parameter(v.clone()) for k, v in state.items() if k in dict(vae.named_parameters())}
    for k, p in vae.named_parameters():
        cpu[k].grad = p.grad.detach().cpu().clone()
    torch.optim.AdamW(list(cpu.values()), lr=lr, weight_decay=wd).step()
    worst = 0.0
    for k, p in vae.named_parameters():
        tol = 2.0 * state[k].abs() * 2.0 ** -23 + 1e-3 * lr
        worst = max(worst, ((p.detach().cpu() - cpu[k].detach()).abs() / tol).max().item())
    print(f"AdamW vs torch.optim.AdamW on the engine's gradients: worst |error| / tol {worst:.3f}")
    assert worst <= 1.0
    # a second step: nothing left over from the first
    eng = step.eng
    assert eng._head_bwd is None and len(eng._wq) == 0
    out2 = step.step(xd, eps[1])
    torch.cuda.synchronize()
    assert step.global_step == 2 and torch.isfinite(out2["loss"]).item()
    assert out2["loss"].item() < out["loss"].item()
    sd = step.state_dict()
    assert sd["global_step"] == 2 and float(sd["state"][0]["step"]) == 2.0


def test_twelve_steps_descend_like_the_oracle():
    """Twelve steps at lr 1e-3 on the fixed batch, seeded eps per step, against the same steps of the CPU oracle
    under torch.optim.AdamW: the engine reaches at least 80 % of the oracle's decrease of the total loss."""
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    cfg, state, x = _golden()
    steps, lr = 12, 1e-3
    eps = [torch.randn((2, 4, 8, 8), generator=torch.Generator().manual_seed(100 + i)) for i in range(steps)]
    sd = {k: v.clone().requires_grad_() for k, v in state.items()}
    opt = torch.optim.AdamW(list(sd.values()), lr=lr, weight_decay=0.0)
    ref = []
    for i in range(steps):
        opt.zero_grad(set_to_none=True)
        rec, kl, _ = _oracle_forward(sd, cfg, x, eps[i])
        loss = _oracle_loss(rec, kl, x, "mse")
        loss.backward()
        opt.step()
        ref.append(loss.item())
    vae = _build(cfg, state).cuda()
    step = VAETrainStep(vae, TRAIN_CFG, lr=lr, weight_decay=0.0)
    xd = x.cuda()
    outs = [step.step(xd, e.cuda())["loss"] for e in eps]
    got = torch.stack(outs).cpu().tolist()
    print("oracle total loss per step:", " ".join(f"{v:.4f}" for v in ref))
    print("engine total loss per step:", " ".join(f"{v:.4f}" for v in got))
    assert ref[0] - ref[-1] > 0.25 * ref[0]          # the reference itself descends (measured: 49 %)
    assert abs(got[0] - ref[0]) <= 1e-2 * ref[0]
    assert got[0] - got[-1] >= 0.8 * (ref[0] - ref[-1])


# ------------------------------------------------------------------ the caches
def _inference_outputs(vae, x, z, eps):
    from fmdiff.runtime.vae_engine import get_vae_engine
    with torch.no_grad():
        mom = get_vae_engine(vae).encode_moments(x)
        rec = vae.decode(z)
        rk, zk, kl = get_vae_engine(vae).kl_forward(x, eps)
    return mom, rec, rk, zk, kl


def test_caches_survive_training():
    """``encode`` / ``decode`` / ``kl_forward`` give the same bits before and after a ``forward_train`` + backward
    without an optimizer step, and after one ``VAETrainStep.step`` the bits of a fresh model loaded from the updated
    state_dict (the step writes the parameters through raw pointers, which no ``_version`` sees)."""
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    cfg, state, x = _golden()
    g = torch.Generator().manual_seed(9)
    xin = (x * 2.0 - 1.0).cuda()
    z = torch.randn((2, 4, 8, 8), generator=g).cuda()
    eps = torch.randn((2, 4, 8, 8), generator=g).cuda()
    vae = _build(cfg, state).cuda()
    before = _inference_outputs(vae, xin, z, eps)
    loss, *_ = _engine_loss(vae, x.cuda(), eps, "mse", x.cuda())
    loss.backward()
    after = _inference_outputs(vae, xin, z, eps)
    for a, b in zip(before, after):
        assert torch.equal(a, b)
    step = VAETrainStep(vae, TRAIN_CFG, lr=1e-2, weight_decay=0.0)
    moved = _inference_outputs(vae, xin, z, eps)      # the parameters moved into the flat buffer: same values
    for a, b in zip(before, moved):
        assert torch.equal(a, b)
    step.step(x.cuda(), eps)
    stepped = _inference_outputs(vae, xin, z, eps)
    fresh = _build(cfg, {k: v.detach().cpu().clone() for k, v in vae.state_dict().items()}).cuda()
    want = _inference_outputs(fresh, xin, z, eps)
    torch.cuda.synchronize()
    for a, b, c in zip(stepped, want, before):
        assert torch.equal(a, b)
        assert not torch.equal(a, c)                 # and the step did change them
