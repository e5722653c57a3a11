"""CPU checks of the VAE criterion's host side: the trainer's composition (fmdiff.pipelines.train.vae_lib), the
pieces that are deliberately not built, and the absence of a CPU path."""
import pytest
import torch


def _crit(training=None, model=None):
    from fmdiff.pipelines.train.vae_lib import VAECriterion
    return VAECriterion(training or {}, model)


def test_kl_scale_follows_the_reference_schedule():
    c = _crit({"kl_weight": 0.5, "kl_anneal_steps": 10})
    # kl_weight * min(1, max(1, step + 1) / max(1, anneal))
    assert c.kl_scale(0) == 0.5 * (1 / 10)
    assert c.kl_scale(1) == 0.5 * (2 / 10)
    assert c.kl_scale(8) == 0.5 * (9 / 10)          # anneal - 2
    assert c.kl_scale(9) == 0.5                     # anneal - 1: step + 1 == anneal
    assert c.kl_scale(10) == 0.5 and c.kl_scale(11) == 0.5
    assert c.kl_scale(-5) == 0.5 * (1 / 10)         # max(1, step + 1)
    flat = _crit({"kl_weight": 0.25, "kl_anneal_steps": 0})
    for step in (0, 1, 9, 10, 11):
        assert flat.kl_scale(step) == 0.25
    assert _crit().kl_scale(3) == 0.0               # the default kl_weight
    one = _crit({"kl_weight": 2.0, "kl_anneal_steps": 1})
    assert one.kl_scale(0) == 2.0 and one.kl_scale(1) == 2.0


@pytest.mark.parametrize("training,model,want", [
    ({}, {}, 0.0),                                              # latent_type kl, reg_type kl
    ({"reg_type": "VQ"}, {}, 1.0),                              # default codebook_weight 1.0
    ({"codebook_weight": 0.3}, {"latent_type": "vq"}, 0.3),
    ({"codebook_weight": 0.3, "reg_type": "vq"}, {"latent_type": "kl"}, 0.3),
    ({"codebook_weight": 0.3}, {"latent_type": "kl"}, 0.0),
    ({"codebook_weight": 0.0}, {"latent_type": "vq"}, 0.0),
])
def test_effective_codebook_weight(training, model, want):
    assert _crit(training, model).effective_codebook_weight == want


def test_disc_is_active():
    from fmdiff.pipelines.train.vae_lib import _disc_is_active
    d = object()
    assert not _disc_is_active(None, 1.0, 0, None, 5, 5)
    assert not _disc_is_active(d, 0.0, 0, None, 5, 5)
    assert not _disc_is_active(d, -1.0, 0, 0, 5, 5)
    assert _disc_is_active(d, 0.1, 2, None, 2, 0) and not _disc_is_active(d, 0.1, 2, None, 1, 10 ** 6)
    # gan_start_steps, when given, decides alone
    assert _disc_is_active(d, 0.1, 99, 10, 0, 10) and not _disc_is_active(d, 0.1, 0, 10, 99, 9)
    assert _disc_is_active(d, 0.1, 99, 0, 0, 0)
    c = _crit({"gan_weight": 0.5, "gan_start": 3, "gan_start_steps": "7"})
    assert c.gan_start_steps == 7 and c.disc_is_active(d, 0, 7) and not c.disc_is_active(d, 9, 6)


def test_make_scheduler_names():
    from torch.optim.lr_scheduler import CosineAnnealingLR, ExponentialLR, StepLR
    from fmdiff.pipelines.train.vae_lib import _make_scheduler
    opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=0.1)
    assert _make_scheduler(opt, {}) is None
    assert _make_scheduler(opt, {"scheduler": None}) is None
    assert _make_scheduler(opt, {"scheduler": {"name": ""}}) is None
    assert _make_scheduler(opt, {"scheduler": {"name": None, "params": {}}}) is None
    assert isinstance(_make_scheduler(opt, {"scheduler": {"name": "StepLR", "params": {"step_size": 2}}}), StepLR)
    assert isinstance(_make_scheduler(opt, {"scheduler": {"name": "cosineannealinglr", "params": {"T_max": 4}}}),
                      CosineAnnealingLR)
    assert isinstance(_make_scheduler(opt, {"scheduler": {"name": "ExponentialLR", "params": {"gamma": 0.9}}}),
                      ExponentialLR)
    with pytest.raises(ValueError, match="Unsupported scheduler 'onecycle'"):
        _make_scheduler(opt, {"scheduler": {"name": "OneCycle"}})


def test_what_is_not_built_says_so():
    from fmdiff.nn.losses import PatchDiscriminator, PerceptualLoss, bce_focal_loss, focal_loss, recon_loss
    from fmdiff.pipelines.train import vae_lib
    with pytest.raises(NotImplementedError):
        PerceptualLoss()
    with pytest.raises(NotImplementedError):
        PatchDiscriminator(in_channels=1)
    with pytest.raises(NotImplementedError, match="DESIGN"):
        vae_lib.train(None, "x.json")
    with pytest.raises(NotImplementedError):
        _crit({"perceptual_weight": 0.1})
    x = torch.zeros(2, 1, 4, 4)
    for fn in (focal_loss, bce_focal_loss):
        with pytest.raises(NotImplementedError, match="gamma"):
            fn(x, x, gamma=1.5)
    with pytest.raises(ValueError, match="Unsupported recon_type 'huber'"):
        recon_loss(x, x, "huber")
    with pytest.raises(ValueError, match="Unsupported recon_type"):
        _crit({"recon_type": "huber"})


def test_criterion_has_no_cpu_fallback():
    from fmdiff.nn.losses import (bce_focal_loss, discriminator_hinge_loss, focal_loss, generator_hinge_loss,
                                  recon_loss, vq_regularizer)
    from fmdiff.nn.modules.vae import reparameterize_kl
    from fmdiff.runtime import ops
    x = torch.zeros(2, 2, 4, 4)
    calls = [lambda: focal_loss(x, x), lambda: bce_focal_loss(x, x), lambda: discriminator_hinge_loss(x, x),
             lambda: generator_hinge_loss(x), lambda: vq_regularizer(x), lambda: recon_loss(x, x, "l1"),
             lambda: reparameterize_kl(x), lambda: ops.elementwise_loss("l1", x, x),
             lambda: ops.gauss_sample_kl(x.movedim(1, -1).contiguous(), 1),
             lambda: ops.gauss_backward(x.movedim(1, -1).contiguous(), 1, None, None, None),
             lambda: _crit()(x, x)]
    for call in calls:
        with pytest.raises(RuntimeError, match="no CPU path"):
            call()
