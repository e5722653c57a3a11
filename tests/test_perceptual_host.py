"""CPU checks of the perceptual loss's host side: topology and state-dict keys, load_vgg_state_dict, every refusal,
the three names that must keep refusing, construction of the criterion and the step, and the absence of a CPU path."""
import warnings

import pytest
import torch
import torch.nn as nn

import perc_bounds as PB

SMALL = dict(in_channels=1, out_channels=1, resolution=16, base_ch=32, down_channels=[32, 32], num_res_blocks=1,
             attn_resolutions=[], z_channels=4, embed_dim=4, use_attention=False, attn_heads=4, attn_dim_head=8)


def _vae(**kw):
    from fmdiff.models.vae import AutoencoderKL
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return AutoencoderKL(**{**SMALL, **kw})


def _P(*a, **kw):
    from fmdiff.nn.losses import VGGPerceptualLoss
    return VGGPerceptualLoss(*a, **kw)


def test_default_topology_and_state_dict_keys():
    P = _P()
    convs = [m for m in P.features if isinstance(m, nn.Conv2d)]
    assert [c.out_channels for c in convs] == [64, 64, 128, 128, 256, 256, 256, 512, 512, 512]
    assert len(P.features) == 23 and convs[0].in_channels == 3
    assert [i for i, m in enumerate(P.features) if isinstance(m, nn.MaxPool2d)] == [4, 9, 16]
    idx = [0, 2, 5, 7, 10, 12, 14, 17, 19, 21]     # torchvision vgg16().features
    assert list(P.state_dict()) == [f"features.{i}.{n}" for i in idx for n in ("weight", "bias")]
    assert not any(p.requires_grad for p in P.parameters())
    specs = P.layer_specs()
    assert [(s.tap, s.pool) for s in specs] == [(None, False), (0, True), (None, False), (1, True), (None, False),
                                                (None, False), (2, True), (None, False), (None, False), (3, False)]
    assert P.resize is None and _P(resize=True).resize == (224, 224)
    assert _P(resize=32).resize == (32, 32) and _P(resize=(20, 12)).resize == (20, 12)
    assert P.feature_sizes((224, 224))[-1] == (28, 28)
    # a shorter weight list is filled with 1.0; weights follow the layers in ascending order
    Q = _P(layers=(8, 3), layer_weights=(0.5,))
    assert Q.layers == (3, 8) and Q.layer_weights == (0.5, 1.0)
    assert [s.weight for s in Q.layer_specs() if s.tap is not None] == [0.5, 1.0]
    assert len(Q.layer_specs()) == 4 and not Q.layer_specs()[-1].pool     # the walker stops behind the last tap


def test_load_vgg_state_dict():
    src = PB.build_features(PB.VGG16, 3)
    sd = {f"features.{k}": v for k, v in src.state_dict().items()}
    sd["classifier.0.weight"] = torch.zeros(3, 3)
    for extra in (24, 26, 28):
        sd[f"features.{extra}.weight"] = torch.zeros(512, 512, 3, 3)
        sd[f"features.{extra}.bias"] = torch.zeros(512)
    P = _P()
    v0 = P.features[0].weight._version
    P.load_vgg_state_dict(sd)
    assert P.features[0].weight._version > v0      # what the weight caches key on
    for k, v in src.state_dict().items():
        assert torch.equal(P.state_dict()[f"features.{k}"], v)
    Q = _P()
    Q.load_vgg_state_dict(src.state_dict())        # the keys of vgg16().features
    for k, v in src.state_dict().items():
        assert torch.equal(Q.state_dict()[f"features.{k}"], v)
    assert not any(p.requires_grad for p in Q.parameters())
    bad = dict(sd)
    del bad["features.5.bias"]
    with pytest.raises(KeyError, match=r"features\.5\.bias"):
        _P().load_vgg_state_dict(bad)


def _seq(*mods):
    return nn.Sequential(*mods)


def test_module_refusals():
    c = lambda i, o, **kw: nn.Conv2d(i, o, kw.pop("k", 3), padding=kw.pop("p", 1), **kw)   # noqa: E731
    ok = [c(3, 8), nn.ReLU(), nn.MaxPool2d(2, 2), c(8, 8), nn.ReLU()]
    _P(_seq(*ok), layers=(1, 4))
    cases = [
        (_seq(c(3, 8, k=5, p=2), nn.ReLU()), (1,)),                          # kernel geometry
        (_seq(c(3, 8, stride=2), nn.ReLU()), (1,)),
        (_seq(c(3, 8, bias=False), nn.ReLU()), (1,)),
        (_seq(c(3, 8), nn.ReLU(), nn.MaxPool2d(2, 2), c(8, 8), nn.ReLU()), (4,)),   # pool behind an untapped ReLU
        (_seq(c(3, 8), nn.ReLU(), nn.MaxPool2d(3, 2), c(8, 8), nn.ReLU()), (1, 4)),  # another pool
        (_seq(c(3, 8), nn.ReLU()), (0,)),                                    # the tap is not a ReLU
        (_seq(c(1, 8), nn.ReLU()), (1,)),                                    # the first conv does not read 3 channels
        (_seq(c(3, 8), nn.LeakyReLU(0.2)), (1,)),
        (_seq(c(3, 8), nn.ReLU(), c(4, 8), nn.ReLU()), (3,)),                # widths do not chain
        (_seq(c(3, 8), nn.BatchNorm2d(8), nn.ReLU()), (2,)),
    ]
    for feats, layers in cases:
        with pytest.raises(NotImplementedError):
            _P(feats, layers=layers)
    with pytest.raises(ValueError):
        _P(layers=(3, 8, 15, 22, 29))              # more layers than the stack holds
    with pytest.raises(ValueError):
        _P(layers=())
    with pytest.raises(ValueError):
        _P(resize=0)
    P = _P(PB.build_features(PB.NARROW), resize=False)
    z = torch.zeros(2, 1, 16, 16)
    with pytest.raises(ValueError):
        P(torch.zeros(2, 2, 16, 16), torch.zeros(2, 2, 16, 16))      # 2 channels
    with pytest.raises(ValueError):
        P(z, torch.zeros(2, 1, 16, 12))                                # shapes differ
    with pytest.raises(ValueError, match="too small"):
        P(torch.zeros(2, 1, 4, 16), torch.zeros(2, 1, 4, 16))        # 4 -> 2 -> 1 -> 0 rows
    with pytest.raises(ValueError):
        P.feature_sizes((0, 4))


def test_no_cpu_path():
    from fmdiff.runtime import ops
    P = _P(PB.build_features(PB.NARROW))
    z = torch.zeros(2, 1, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P(z, z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        P.forward_image(z, "clamp", z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.perc_stage(z, z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.perc_stage_bwd(torch.zeros(2, 16, 16, 8, dtype=torch.bfloat16), z)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.perc_tap_fwd(torch.zeros(4, 4, 4, 8), 8)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.perc_tap_bwd(torch.zeros(2, 4, 4, 8), torch.zeros(2, 4, 4, 8, dtype=torch.int8), 8, torch.ones(1))


def test_the_three_pinned_names_still_refuse_and_point_to_the_new_one():
    from fmdiff.nn.losses import PerceptualLoss
    from fmdiff.pipelines.train.vae_lib import VAECriterion, VAETrainStep
    with pytest.raises(NotImplementedError, match="VGGPerceptualLoss"):
        PerceptualLoss()
    with pytest.raises(NotImplementedError, match="VGGPerceptualLoss"):
        VAECriterion({"perceptual_weight": 0.1})
    with pytest.raises(NotImplementedError, match="perceptual"):
        VAETrainStep(_vae(), {"perceptual_weight": 0.1})


def test_criterion_and_step_are_constructible_with_the_module():
    from fmdiff.pipelines.train import vae_lib
    P = _P(PB.build_features(PB.NARROW), resize=32)
    crit = vae_lib.VAECriterion({"perceptual_weight": 0.5, "recon_type": "mse"}, perceptual=P)
    assert crit.perceptual is P and crit.perceptual_weight == 0.5
    step = vae_lib.VAETrainStep(_vae(), {"perceptual_weight": 1.0, "recon_type": "mse"}, perceptual=P)
    assert step.perc is P and step.image_map == "clamp" and not P.training
    assert vae_lib.VAETrainStep(_vae(), {"perceptual_weight": 1.0, "recon_type": "bce"}, perceptual=P).image_map == "sigmoid"
    # weight 0: the module is never called
    assert vae_lib.VAETrainStep(_vae(), {"perceptual_weight": 0.0}, perceptual=P).perc is None
    with pytest.raises(RuntimeError, match="no CPU path"):     # up to the first device call
        step.step(torch.zeros(2, 1, 16, 16))
    with pytest.raises(NotImplementedError, match="use_amp"):
        vae_lib.VAETrainStep(_vae(), {"perceptual_weight": 1.0, "use_amp": True}, perceptual=P)
    with pytest.raises(NotImplementedError, match="perceptual_device"):
        vae_lib.VAETrainStep(_vae(), {"perceptual_weight": 1.0, "perceptual_device": "cuda:1"}, perceptual=P)
    with pytest.raises(ValueError, match="1 or 3 channels"):
        vae_lib.VAETrainStep(_vae(in_channels=2, out_channels=2), {"perceptual_weight": 1.0}, perceptual=P)
    with pytest.raises(NotImplementedError, match="DESIGN"):
        vae_lib.train(None, "x.json")
