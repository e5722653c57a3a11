"""The adversarial VAE step (``VAETrainStep`` with a discriminator) against the reference's loop body written out by
hand with the public pieces: the VQVAE fixture model with a base-8 MAGVIT discriminator and the AutoencoderKL fixture
model with a base-8 PatchGAN discriminator, on 2 x 1 x 48 x 64 images (48 x 64: the MAGVIT stack needs 40 pixels a
side), gan_weight 0.5."""
import json
import os
import warnings

import pytest
import torch

import vq_bounds as VB

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
GAN_WEIGHT, LR, WD, DISC_LR = 0.5, 1e-3, 0.01, 2e-3
_CACHE = {}


def _model_case(kind):
    """(constructor, cfg, state, x, eps, training cfg, model cfg): the fixture models of the trunk-training tests
    (decoder.conv_out scaled by 0.25 as there) on a seeded 48 x 64 batch."""
    if kind not in _CACHE:
        g = torch.Generator().manual_seed(77)
        x = torch.rand(2, 1, 48, 64, generator=g)
        if kind == "vq":
            from fmdiff.models.vae import VQVAE as cls
            G, cfg = VB.load_fixture()
            _, state = VB.build_fixture_model(G, cfg, "ema")
            cfg = dict(cfg, quantizer_type="ema")
            eps = None
            tcfg = {"recon_type": "mse", "codebook_weight": 1.0, "gan_weight": GAN_WEIGHT, "disc_lr": DISC_LR}
            mcfg = {"latent_type": "vq"}
        else:
            from fmdiff.models.vae import AutoencoderKL as cls
            G = torch.load(os.path.join(HERE, "golden", "vae_golden.pt"), weights_only=True)
            cfg = json.loads(bytes(G["cfg_json"].tolist()).decode())
            state = G["state"]
            eps = torch.randn(2, cfg["embed_dim"], 12, 16, generator=g)
            tcfg = {"recon_type": "l1", "kl_weight": 1e-3, "gan_weight": GAN_WEIGHT, "disc_lr": DISC_LR}
            mcfg = None
        state = {k: v.clone() for k, v in state.items()}
        for k in ("decoder.conv_out.conv.weight", "decoder.conv_out.conv.bias"):
            state[k] = state[k] * 0.25
        _CACHE[kind] = (cls, cfg, state, x, eps, tcfg, mcfg)
    return _CACHE[kind]


def _vae(kind):
    cls, cfg, state = _model_case(kind)[:3]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = cls(**cfg)
    m.load_state_dict(state)
    return m.cuda().train()


def _disc_state(kind):
    if ("disc", kind) not in _CACHE:
        from fmdiff.nn.modules.vae.discriminators import MagvitDiscriminatorND, PatchGANDiscriminatorND
        torch.manual_seed(31)
        d = (MagvitDiscriminatorND if kind == "vq" else PatchGANDiscriminatorND)(1, 8)
        g = torch.Generator().manual_seed(32)
        sd = {k: v.detach().clone() for k, v in d.state_dict().items()}
        for k in sd:   # BatchNorm away from its defaults
            if k.endswith("running_mean"):
                sd[k] = torch.randn(sd[k].shape, generator=g) * 0.3
            elif k.endswith("running_var") or (sd[k].dim() == 1 and ".conv." not in k and k.endswith("weight")):
                sd[k] = torch.rand(sd[k].shape, generator=g) + 0.5
        _CACHE[("disc", kind)] = sd
    return _CACHE[("disc", kind)]


def _disc(kind):
    from fmdiff.nn.modules.vae.discriminators import MagvitDiscriminatorND, PatchGANDiscriminatorND
    d = (MagvitDiscriminatorND if kind == "vq" else PatchGANDiscriminatorND)(1, 8)
    d.load_state_dict(_disc_state(kind))
    return d.cuda().train()


def _forward(kind, vae, xd, eps):
    if kind == "vq":
        rec, aux = vae.forward_train(vae.image_to_model_range(xd))
        return rec, dict(vq_loss=aux["vq_loss"])
    rec, _, kl = vae.forward_train(vae.image_to_model_range(xd), eps, sample_posterior=True)
    return rec, dict(kl=kl)


def _by_hand(kind, disc_from_gen=True):
    """The sequence of the reference's loop body with the public pieces; returns (vae, disc, totals)."""
    from fmdiff.pipelines.train.vae_lib import VAECriterion
    _, _, _, x, eps, tcfg, mcfg = _model_case(kind)
    xd = x.cuda()
    eps = None if eps is None else eps.cuda()
    vae, disc = _vae(kind), _disc(kind)
    crit = VAECriterion(tcfg, mcfg)
    rec, kw = _forward(kind, vae, xd, eps)
    fake_pred = disc.forward_image(rec, "clamp", param_grads=disc_from_gen)
    out = crit(rec, xd, fake_pred=fake_pred, global_step=0, **kw)
    out["loss"].backward()
    real_pred = disc(xd)
    fake_det = disc.forward_image(rec.detach(), "clamp")
    d = crit.discriminator_loss(real_pred, fake_det)
    d.backward()
    out["d_gan"] = d.detach()
    out["loss"] = out["loss"].detach()
    return vae, disc, out, rec.detach()


def _step(kind, disc=True, tcfg_over=None, **kw):
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    _, _, _, x, eps, tcfg, mcfg = _model_case(kind)
    vae = _vae(kind)
    d = _disc(kind) if disc else None
    tc = dict(tcfg, **(tcfg_over or {}))
    if not disc:
        tc["gan_weight"] = 0.0
    st = VAETrainStep(vae, tc, mcfg, discriminator=d, lr=LR, weight_decay=WD, **kw)
    return vae, d, st, x.cuda(), (None if eps is None else eps.cuda())


def _adamw_check(named, state0, lr, wd, what):
    cpu = {k: torch.nn.Parameter(state0[k].clone()) for k, _ in named}
    for k, p in named:
        cpu[k].grad = p.grad.detach().cpu().clone()
    torch.optim.AdamW(list(cpu.values()), lr=lr, weight_decay=wd).step()
    worst = 0.0
    for k, p in named:
        tol = 2.0 * state0[k].abs() * 2.0 ** -23 + 1e-3 * lr
        worst = max(worst, ((p.detach().cpu() - cpu[k].detach()).abs() / tol).max().item())
    print(f"{what}: AdamW vs torch.optim.AdamW on the engine's gradients, worst |error| / tol {worst:.3f}")
    assert worst <= 1.0, what


@pytest.mark.parametrize("kind", ["vq", "kl"])
def test_active_step_equals_the_sequence_by_hand(kind):
    from fmdiff.nn.losses import generator_hinge_loss
    state0 = _model_case(kind)[2]
    rvae, rdisc, rout, rec = _by_hand(kind)
    vae, disc, st, xd, eps = _step(kind)
    out = st.step(xd, eps)
    torch.cuda.synchronize()
    assert set(out) == set(rout) and st.global_step == 1 and st.disc_step == 1
    for k in out:
        assert out[k].is_cuda and out[k].dim() == 0 and torch.equal(out[k], rout[k]), k
    assert out["d_gan"].item() > 0 and out["g_gan"].item() != 0
    # loss excludes d_gan, includes gan_weight * g_gan
    parts = out["recon"] + (out["vq"] if kind == "vq" else 1e-3 * out["kl"]) + GAN_WEIGHT * out["g_gan"]
    assert abs(out["loss"].item() - parts.item()) <= 1e-5 * abs(parts.item())
    frozen = "codebook."
    for (k, p), (_, q) in zip(vae.named_parameters(), rvae.named_parameters()):
        if not k.startswith(frozen):
            assert torch.equal(p.grad, q.grad), k
    for (k, p), (_, q) in zip(disc.named_parameters(), rdisc.named_parameters()):
        assert torch.equal(p.grad, q.grad), k
    for (k, b), (_, c) in zip(disc.named_buffers(), rdisc.named_buffers()):
        assert torch.equal(b, c), k
    # the discriminator's gradients: gan_weight * d g_gan / d theta + d d_gan / d theta, each obtained alone.  Every
    # destination is written as (0 + A) + B with A and B the same fp32 values the lone passes produce (the kernels
    # are deterministic): one fp32 rounding of A + B, held to 2 * 2^-24 (|A| + |B|) (that rounding plus one)
    da, db = _disc(kind), _disc(kind)
    (GAN_WEIGHT * generator_hinge_loss(da.forward_image(rec, "clamp"))).backward()
    from fmdiff.nn.losses import discriminator_hinge_loss
    discriminator_hinge_loss(db(xd), db.forward_image(rec, "clamp")).backward()
    for (k, p), (_, a), (_, b) in zip(disc.named_parameters(), da.named_parameters(), db.named_parameters()):
        A, Bv = a.grad.double(), b.grad.double()
        assert ((p.grad.double() - (A + Bv)).abs() <= 2 * 2.0 ** -24 * (A.abs() + Bv.abs())).all(), k
        assert A.abs().max().item() > 0 or ".conv.bias" in k, k
    # running statistics: three sequential training-mode updates in the order fake, real, fake
    ds = _disc(kind)
    with torch.no_grad():
        ds.forward_image(rec, "clamp"), ds(xd), ds.forward_image(rec, "clamp")
    for (k, b), (_, c) in zip(disc.named_buffers(), ds.named_buffers()):
        assert torch.equal(b, c), k
        if k.endswith("num_batches_tracked"):
            assert int(b) == 3
    # both AdamW updates
    _adamw_check([(k, p) for k, p in vae.named_parameters() if not k.startswith(frozen)], state0, LR, WD, f"{kind} VAE")
    _adamw_check(list(disc.named_parameters()), _disc_state(kind), DISC_LR, 0.01, f"{kind} discriminator")
    # the weight caches follow the raw-pointer updates: the module equals a fresh one with its state_dict
    fresh = _disc(kind)
    fresh.load_state_dict({k: v.cpu() for k, v in disc.state_dict().items()})
    with torch.no_grad():
        assert torch.equal(disc(xd), fresh(xd))
    # a second step starts with nothing queued
    from fmdiff.runtime.disc_engine import get_disc_engine
    assert st.eng._head_bwd is None and len(st.eng._wq) == 0 and len(get_disc_engine(disc)._wq) == 0
    out2 = st.step(xd, eps)
    torch.cuda.synchronize()
    assert st.global_step == 2 and st.disc_step == 2 and all(torch.isfinite(v).item() for v in out2.values())
    assert len(st.eng._wq) == 0 and len(get_disc_engine(disc)._wq) == 0
    # the optimizer state in torch's form
    sd = st.disc_state_dict()
    cpu = [torch.nn.Parameter(p.detach().cpu().clone()) for p in disc.parameters()]
    opt = torch.optim.AdamW(cpu, lr=1.0)
    opt.load_state_dict(sd)
    assert opt.param_groups[0]["lr"] == DISC_LR and opt.param_groups[0]["weight_decay"] == 0.01
    assert float(opt.state[cpu[0]]["step"]) == 2.0
    m0, v0 = st.disc_m.clone(), st.disc_v.clone()
    st.disc_m.zero_(), st.disc_v.zero_()
    st.load_disc_state_dict(opt.state_dict())
    assert torch.equal(st.disc_m, m0) and torch.equal(st.disc_v, v0) and st.disc_step == 2
    assert "disc" not in "".join(st.state_dict().keys())


@pytest.mark.parametrize("kind", ["vq", "kl"])
def test_without_generator_weight_gradients(kind):
    """disc_grad_from_generator=False: the discriminator's gradients are d_gan's alone, the VAE's keep their bits."""
    rvae, rdisc, rout, rec = _by_hand(kind)
    vae, disc, st, xd, eps = _step(kind, disc_grad_from_generator=False)
    out = st.step(xd, eps)
    for k in out:
        assert torch.equal(out[k], rout[k]), k
    for (k, p), (_, q) in zip(vae.named_parameters(), rvae.named_parameters()):
        if not k.startswith("codebook."):
            assert torch.equal(p.grad, q.grad), k
    from fmdiff.nn.losses import discriminator_hinge_loss
    db = _disc(kind)
    discriminator_hinge_loss(db(xd), db.forward_image(rec, "clamp")).backward()
    differs = False
    for (k, p), (_, b), (_, q) in zip(disc.named_parameters(), db.named_parameters(), rdisc.named_parameters()):
        assert torch.equal(p.grad, b.grad), k
        differs = differs or not torch.equal(p.grad, q.grad)
    assert differs, "the default mode must leave the generator pass's gradients in the discriminator"


@pytest.mark.parametrize("kind", ["vq", "kl"])
def test_inactive_step_is_the_step_without_a_discriminator(kind):
    vae0, _, st0, xd, eps = _step(kind, disc=False)
    out0 = st0.step(xd, eps)
    vae, disc, st, _, _ = _step(kind, tcfg_over={"gan_start_steps": 5})
    before = {k: v.clone() for k, v in disc.state_dict().items()}
    out = st.step(xd, eps)
    torch.cuda.synchronize()
    for k in out0:
        assert torch.equal(out[k], out0[k]), k
    assert out["g_gan"].item() == 0 and out["d_gan"].item() == 0
    for (k, p), (_, q) in zip(vae.state_dict().items(), vae0.state_dict().items()):
        assert torch.equal(p, q), k
    assert torch.equal(st.m, st0.m) and torch.equal(st.v, st0.v)
    for k, v in disc.state_dict().items():
        assert torch.equal(v, before[k]), k
    assert st.disc_step == 0 and not st.disc_m.any() and not st.disc_v.any() and not st.disc_flat.grad.any()
    assert st.disc_state_dict()["state"] == {}


def test_refusals():
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    _, _, _, _, _, tcfg, mcfg = _model_case("vq")
    with pytest.raises(NotImplementedError, match="discriminator"):
        VAETrainStep(_vae("vq"), tcfg, mcfg)
    for over, msg in (({"use_amp": True}, "use_amp"), ({"disc_device": "cuda:1"}, "disc_device"),
                      ({"perceptual_weight": 0.1}, "perceptual")):
        with pytest.raises(NotImplementedError, match=msg):
            VAETrainStep(_vae("vq"), dict(tcfg, **over), mcfg, discriminator=_disc("vq"))
    from fmdiff.nn.modules.vae.discriminators import MagvitDiscriminatorND
    with pytest.raises(ValueError, match="channels"):
        VAETrainStep(_vae("vq"), tcfg, mcfg, discriminator=MagvitDiscriminatorND(3, 8).cuda())
