"""Host-side checks of the GAN discriminators (no GPU): the CPU oracle of tests/bn_bounds.py reproduces the recorded
reference run (tests/golden/disc_golden.pt, written by tests/golden/make_disc_golden.py), the new modules carry the
reference's state_dict, and what is refused still raises."""
import os

import pytest
import torch

import bn_bounds as B

HERE = os.path.dirname(os.path.abspath(__file__))
F64 = torch.float64


@pytest.fixture(scope="module")
def golden():
    return torch.load(os.path.join(HERE, "golden", "disc_golden.pt"), weights_only=True)


def _cls(name):
    from fmdiff.nn.modules.vae.discriminators import MagvitDiscriminatorND, PatchGANDiscriminatorND
    return {"magvit": MagvitDiscriminatorND, "patchgan": PatchGANDiscriminatorND}[name]


def _sd(G, name):
    pre = f"{name}.sd."
    return {k[len(pre):]: v for k, v in G.items() if k.startswith(pre)}


def _rel(got, ref):
    return (got.double() - ref.double()).abs().max().item() / max(ref.double().abs().max().item(), 1e-30)


@pytest.mark.parametrize("name", ["magvit", "patchgan"])
@pytest.mark.parametrize("dtype", [torch.float32, F64])
def test_oracle_reproduces_the_reference(golden, name, dtype):
    G = golden
    sd = _sd(G, name)
    P = B.oracle_params(sd, dtype)
    x = G[f"{name}.x"].to(dtype).clone().requires_grad_()
    logits, bufs = B.disc_oracle(P, B.TABLES[name], x, training=True, dtype=dtype)
    (logits * G[f"{name}.g"].to(dtype)).sum().backward()
    assert _rel(logits, G[f"{name}.train.logits"]) < 1e-5
    assert _rel(x.grad, G[f"{name}.train.dx"]) < 1e-5
    nb = 0
    for k, v in G.items():
        pre = f"{name}.train.buf."
        if k.startswith(pre):
            key = k[len(pre):]
            nb += 1
            if v.is_floating_point():
                assert _rel(bufs[key], v) < 1e-5, key
            else:
                assert v.dtype == torch.int64 and int(bufs[key]) == int(v) == 1, key
    assert nb == 9
    for k, p in P.items():
        if p.requires_grad:
            ref = G[f"{name}.train.grad.{k}"]
            # a conv bias in front of a BatchNorm has a zero gradient: compare those on the scale of the weights'
            scale = max(ref.abs().max().item(), G[f"{name}.train.grad.{k.replace('bias', 'weight')}"].abs().max().item())
            assert (p.grad.double() - ref.double()).abs().max().item() < 1e-5 * scale, k
    P = B.oracle_params(sd, dtype)
    ev, bufs = B.disc_oracle(P, B.TABLES[name], G[f"{name}.x"].to(dtype), training=False, dtype=dtype)
    assert _rel(ev, G[f"{name}.eval.logits"]) < 1e-5
    for k, v in bufs.items():
        assert torch.equal(v.to(sd[k].dtype), sd[k]), k


@pytest.mark.parametrize("name,cin", [("magvit", 1), ("patchgan", 3)])
def test_state_dict_is_the_reference_s(golden, name, cin):
    sd = _sd(golden, name)
    m = _cls(name)(in_channels=cin, base_channels=8)
    own = m.state_dict()
    assert list(own) == list(sd)
    for k in sd:
        assert own[k].shape == sd[k].shape and own[k].dtype == sd[k].dtype, k
    assert own["model.3.num_batches_tracked"].dtype == torch.int64
    m.load_state_dict(sd)
    back = m.state_dict()
    for k in sd:
        assert torch.equal(back[k], sd[k]), k
    assert [k for k, _ in B.disc_keys(B.TABLES[name])] == [k[:-7] for k in sd if k.endswith(".conv.weight")]


def test_defaults_and_alias():
    from fmdiff.nn.modules.vae import MagvitDiscriminator, MagvitDiscriminatorND, PatchGANDiscriminatorND
    m = MagvitDiscriminator()
    assert isinstance(m, MagvitDiscriminatorND) and m.model[0].conv.weight.shape == (64, 3, 4, 4)
    assert m.model[11].conv.weight.shape == (1, 512, 4, 4) and m.model[11].conv.padding == (0, 0)
    p = PatchGANDiscriminatorND()
    assert p.model[0].conv.weight.shape == (64, 1, 4, 4) and p.model[11].conv.weight.shape == (1, 512, 3, 3)
    assert p.model[8].conv.stride == (2, 2) and m.model[8].conv.stride == (1, 1)
    bn = m.model[3]
    assert isinstance(bn, torch.nn.BatchNorm2d) and bn.eps == 1e-5 and bn.momentum == 0.1 and bn.affine
    assert m.model[1].negative_slope == 0.2
    specs = m.layer_specs()
    assert [(s.ks, s.stride, s.pad, s.norm is not None, s.slope) for s in specs] == [
        (4, 2, 1, False, 0.2), (4, 2, 1, True, 0.2), (4, 2, 1, True, 0.2), (4, 1, 1, True, 0.2), (4, 1, 0, False, None)]


def test_sizes_and_refusals():
    from fmdiff.nn.modules.vae.discriminators import MagvitDiscriminatorND, PatchGANDiscriminatorND
    m = MagvitDiscriminatorND(1, 8)
    assert m.output_sizes((48, 64))[-1] == (2, 4) and m.output_sizes((256, 256))[-1] == (28, 28)
    assert PatchGANDiscriminatorND(3, 8).output_sizes((32, 48))[-1] == (2, 3)
    with pytest.raises(ValueError, match="too small"):
        m.output_sizes((32, 24))          # 4 -> 3 -> 0 in the last two layers
    with pytest.raises(ValueError, match="too small"):
        m(torch.zeros(2, 1, 16, 16))
    with pytest.raises(ValueError):
        m(torch.zeros(2, 3, 64, 64))      # wrong channel count
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(2, 1, 48, 64))
    for cls in (MagvitDiscriminatorND, PatchGANDiscriminatorND):
        with pytest.raises(NotImplementedError, match="spatial_dims"):
            cls(1, 8, spatial_dims=3)
        with pytest.raises(ValueError):
            cls(1, 8, spatial_dims=4)


def test_make_discriminator():
    from fmdiff.models.vae.kl import AutoencoderKL
    from fmdiff.models.vae.vq import VQVAE
    from fmdiff.nn.modules.vae.discriminators import MagvitDiscriminatorND
    kw = dict(in_channels=1, out_channels=1, resolution=16, base_ch=32, ch_mult=(1, 2), num_res_blocks=1,
              z_channels=4, embed_dim=4, use_attention=False)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        d = VQVAE(discriminator_type="magvit", codebook_size=16, **kw).make_discriminator()
        assert isinstance(d, MagvitDiscriminatorND) and d.in_channels == 1 and d.base_channels == 64
        for dt in ("patchgan", "default"):
            with pytest.raises(NotImplementedError, match="PatchGANDiscriminatorND"):
                VQVAE(discriminator_type=dt, codebook_size=16, **kw).make_discriminator()
        with pytest.raises(NotImplementedError, match="PatchGANDiscriminatorND"):
            AutoencoderKL(**kw).make_discriminator()


def test_pinned_refusals_still_raise():
    from fmdiff.nn.losses import PatchDiscriminator
    from fmdiff.pipelines.train import vae_lib
    with pytest.raises(NotImplementedError, match="PatchGANDiscriminatorND"):
        PatchDiscriminator(in_channels=1)
    with pytest.raises(NotImplementedError):
        vae_lib.train(None, "x.json")


def test_entry_points_refuse_bad_shapes_without_a_gpu():
    """The argument checks run on the host before any launch: they answer without a device."""
    from fmdiff import _lib
    try:
        L = _lib.lib()
    except (OSError, RuntimeError) as e:
        pytest.skip(f"library not loadable here: {e}")
    assert L.fmd_bn_act_bwd_workspace(105, 8) == (2 * 8 * 2 + 8 * 2) * 4
    assert L.fmd_bn_act_bwd_workspace(105, 12) == -1 and L.fmd_bn_act_bwd_workspace(0, 8) == -1
    assert L.fmd_bn_fold(None, 1, 12, 100, None, None, 1e-5, 0.1, 1, None, None, None, None, None, None, None) < 0
    assert L.fmd_bn_act_fwd(None, 10, 8, None, None, 0.2, None, None) < 0
    assert L.fmd_image_stage(None, 1, 1, 16, 8, 3, None, None) < 0
