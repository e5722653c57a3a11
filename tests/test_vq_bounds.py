"""CPU tests of the vector-quantizer path (csrc/vq.hip): the bound and the emulation the GPU test relies on, the
mutants the assertion must reject, the reference fixture, the modules' state_dict and the VAE factory.

test_gpu_vq.py holds the kernel to  d64(z, e_chosen) - min_k d64(z, e_k) <= 1.5 x bound  per row (vq_bounds.py).
Here the same check runs on a torch emulation of the kernel arithmetic (err / bound <= 1), and on mutants of it.
Which check rejects which mutant (margin 1.5; "near" = the near-minimiser assertion on the case named):

  mutant                rejected by
  single_plane          near: 105x100x8 offset1 (*); 105x1000x24 offset1; 128x512x64 scaled; 200x100x256 offset1;
                        256x16384x256 randn / offset1 / scaled (*)
  no_hn                 near: every shape on randn
  hn_not_halved         near: every shape on randn
  tie_highest           ties: every duplicated pair returns the higher index
  drop_last_split       near: 96x4096x256 and 256x16384x256 (splits > 1) on randn
  pad_hn_zero           ties: the all-zero row picks a padded code (K = 100 / 1000); near: 105x100x8 randn
  skip_last_row_block   near: every shape on randn (M = 105: rows 64..104)

(*) These rejections depend on the seed: a single plane errs on near-tie rows only, and a case holds few of them.
Of the seven seed suffixes tried for vq_bounds.make_inputs the single-plane mutant was rejected on 105x100x8
offset1 with five, and on 256x16384x256 with one (randn), five (offset1) and four (scaled); the suffix in use is
the one that rejects on all four.  The other single_plane rows were read off under that suffix only.  The choice
was made on the mutant, never on the kernel; the GPU test runs the 16384x256 case with four times the rows.
"""
import ctypes
import json
import os
import sys
import warnings

import pytest
import torch

import vq_bounds as vb

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
SHAPES = ((105, 100, 8), (105, 1000, 24), (128, 512, 64), (96, 4096, 256), (256, 16384, 256), (200, 100, 256))
_cache = {}


def _case(shape, dist):
    """Inputs and fp64 reference of one case, computed once and shared (never modified)."""
    key = (shape, dist)
    if key not in _cache:
        z, e, j = vb.make_inputs(*shape, dist)
        _cache[key] = (z, e, j, vb.reference(z, e))
    return _cache[key]


def _rejected(codes, ref, name):
    try:
        vb.check(codes, ref, name)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("dist", vb.DISTRIBUTIONS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_emulation_within_bound_and_bound_not_looser(shape, dist):
    z, e, j, ref = _case(shape, dist)
    bound, loose = vb.row_bound(ref), vb.loose_bound(ref)
    assert bool((bound > 0).all()) and bool((bound <= loose).all()), float((bound / loose).max())
    codes = vb.emulate(z, e)
    r = vb.check(codes, ref, f"{shape} {dist}", margin=1.0)
    print(f"{shape} {dist}: splits {vb.plan(*shape)['splits']} err/bound {r['ratio']:.3f} undecided "
          f"{r['undecided']:.4f} agree {r['agree']:.4f} bound/loose {float((bound / loose).max()):.3f}")
    if j is not None:
        assert torch.equal(codes, j)


def test_plan_reaches_both_split_regimes():
    assert vb.plan(200, 100, 256)["splits"] == 1 and vb.plan(200, 100, 256)["Dpad"] == 256
    assert vb.plan(96, 4096, 256)["splits"] > 1 and vb.plan(1024, 16384, 256)["splits"] > 1
    assert vb.plan(1 << 20, 16384, 64)["splits"] == 1


def test_plan_mirrors_the_library():
    from fmdiff import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfmdiff_hip.so not built (run __graft_entry__.build())")
    try:
        ctypes.CDLL(_lib.LIB_PATH)
    except OSError as e:  # HIP runtime absent on this host
        pytest.skip(f"HIP runtime not loadable here: {e}")
    lib = _lib.lib()
    for M, K, D in SHAPES + ((1024, 16384, 256), (1, 1, 1), (4096, 512, 64), (8192, 16384, 256), vb.TIE_SHAPE):
        p = _lib.VqPlan()
        assert lib.fmd_vq_plan(M, K, D, ctypes.byref(p)) == 0
        mirror = vb.plan(M, K, D)
        assert {k: getattr(p, k) for k in mirror} == mirror, (M, K, D)
        assert lib.fmd_vq_workspace(M, K, D) == 8 * M * p.splits      # O(S M): no M x K matrix
    p = _lib.VqPlan()
    assert lib.fmd_vq_plan(16, 16, 264, ctypes.byref(p)) != 0 and lib.fmd_vq_plan(0, 16, 8, ctypes.byref(p)) != 0
    assert lib.fmd_vq_workspace(16, 16, 264) < 0


MUTANT_CASES = {
    "single_plane": [((105, 100, 8), "offset1"), ((105, 1000, 24), "offset1"), ((128, 512, 64), "scaled"),
                     ((200, 100, 256), "offset1"), ((256, 16384, 256), "randn"), ((256, 16384, 256), "offset1"),
                     ((256, 16384, 256), "scaled")],
    "no_hn": [(s, "randn") for s in SHAPES],
    "hn_not_halved": [(s, "randn") for s in SHAPES],
    "drop_last_split": [((96, 4096, 256), "randn"), ((256, 16384, 256), "randn")],
    "pad_hn_zero": [((105, 100, 8), "randn")],
    "skip_last_row_block": [(s, "randn") for s in SHAPES],
}


@pytest.mark.parametrize("mutant", sorted(MUTANT_CASES))
def test_near_minimiser_assertion_rejects_mutant(mutant):
    for shape, dist in MUTANT_CASES[mutant]:
        z, e, j, ref = _case(shape, dist)
        assert _rejected(vb.emulate(z, e, mutant=mutant), ref, mutant), (mutant, shape, dist)


def test_ties_return_the_lower_index_and_zero_row_the_smallest_norm():
    z, e, expect = vb.make_tie_inputs()
    rows = expect >= 0
    p = vb.plan(*vb.TIE_SHAPE)
    cps = p["codes_per_split"]
    a, b = vb.TIE_PAIRS[3], vb.TIE_PAIRS[4]
    assert a[0] // cps == a[1] // cps and a[0] // vb.CHUNK != a[1] // vb.CHUNK    # two chunks of one split
    assert b[0] // cps != b[1] // cps                                              # two splits
    codes = vb.emulate(z, e)
    assert torch.equal(codes[rows], expect[rows])
    hi = vb.emulate(z, e, mutant="tie_highest")
    for r, (lo, up) in enumerate(vb.TIE_PAIRS):
        assert bool((hi[r * vb.TIE_ROWS:(r + 1) * vb.TIE_ROWS] == up).all()), (lo, up)
    # an all-zero row scores -hn < 0 on every real code and 0 on a padded one whose hn is not +inf
    for K in (100, 1000):
        e2 = e[:K].clone()
        e2[7] = 0.05 * e2[7]
        z0 = torch.zeros(4, e.shape[1])
        assert bool((vb.emulate(z0, e2) == 7).all())
        assert bool((vb.emulate(z0, e2, mutant="pad_hn_zero") != 7).all())


# ------------------------------------------------------------------ fixture, modules, factory
_fixture = vb.load_fixture


@pytest.mark.parametrize("qt", ["ema", "classic"])
def test_restatement_reproduces_the_reference_fixture(qt):
    G, cfg = _fixture()
    z_q, loss, perp, codes = vb.quantizer_restatement(G["quant_in"], G[f"{qt}.codebook.embedding"], cfg["vq_beta"],
                                                      qt == "classic", cfg["vq_ema_eps"])
    assert torch.equal(codes, G[f"{qt}.codes"]) and codes.shape == (2, 8, 8)
    assert float((z_q - G[f"{qt}.z_q"]).abs().max()) <= 1e-6
    assert abs(float(loss) - float(G[f"{qt}.vq_loss"])) <= 1e-6 * abs(float(G[f"{qt}.vq_loss"]))
    assert abs(float(perp) - float(G[f"{qt}.perplexity"])) <= 1e-6 * float(G[f"{qt}.perplexity"])
    # the fixture is a usable case of the kernel-level assertion: few undecided rows under the bound
    flat = G["quant_in"].movedim(1, -1).reshape(-1, cfg["embed_dim"])
    ref = vb.reference(flat, G[f"{qt}.codebook.embedding"])
    r = vb.check(vb.emulate(flat, G[f"{qt}.codebook.embedding"]), ref, f"fixture {qt}", margin=1.0)
    assert r["agree"] == 1.0 and bool((ref["idx"] == G[f"{qt}.codes"].reshape(-1)).all())


@pytest.mark.parametrize("qt", ["ema", "classic"])
def test_state_dict_is_the_references(qt):
    G, cfg = _fixture()
    m, state = vb.build_fixture_model(G, cfg, qt)
    shapes = json.loads(bytes(G[f"{qt}.state_shapes_json"].tolist()).decode())
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == shapes
    assert list(m.state_dict()) == list(shapes)       # the same order too
    for k, v in state.items():
        assert torch.equal(m.state_dict()[k], v), k
    if qt == "ema":
        assert set(dict(m.codebook.named_buffers())) == {"embedding", "ema_cluster_size", "ema_w"}
        assert not list(m.codebook.parameters())
        assert float(m.codebook.ema_cluster_size.sum()) > 0 and not torch.equal(m.codebook.ema_w, m.codebook.embedding)
    else:
        assert [k for k, _ in m.codebook.named_parameters()] == ["embedding"] and not list(m.codebook.buffers())
    assert m.quantizer_type == qt and m.discriminator_type == "patchgan" and m.embed_dim == cfg["embed_dim"]
    with pytest.raises(NotImplementedError):
        m.make_discriminator()


def test_quantizer_refusals_on_the_host():
    from fmdiff.nn.modules.vae import VectorQuantizer, VectorQuantizerEMA
    z = torch.zeros(1, 8, 4, 4)
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        VectorQuantizer(16, 8)(z)
    ema = VectorQuantizerEMA(16, 8)
    assert ema.training and ema.decay == 0.99 and ema.eps == 1e-5 and ema.commitment_cost == 0.25
    with pytest.raises(NotImplementedError, match="EMA codebook update"):
        ema(z)
    with pytest.raises(RuntimeError, match="ROCm device tensors"):
        ema.eval()(z)
    from fmdiff.models.vae import VQVAE
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        with pytest.raises(ValueError, match="Unknown quantizer_type 'fsq'. Expected 'classic' or 'ema'."):
            VQVAE(in_channels=1, out_channels=1, resolution=8, base_ch=32, down_channels=(32,), num_res_blocks=1,
                  use_attention=False, quantizer_type="fsq")
        m3 = VQVAE(in_channels=1, out_channels=1, resolution=8, base_ch=32, down_channels=(32,), num_res_blocks=1,
                   use_attention=False, spatial_dims=3, codebook_size=16)
    with pytest.raises(NotImplementedError, match="spatial_dims=2"):
        m3(torch.zeros(1, 1, 8, 8, 8))
    with pytest.raises(FileNotFoundError, match="Checkpoint not found: /nonexistent.pt"):
        VQVAE(ckpt_path="/nonexistent.pt", in_channels=1, out_channels=1, resolution=8, base_ch=32,
              down_channels=(32,), num_res_blocks=1, use_attention=False)


def _write(tmp_path, name, model, **extra):
    p = tmp_path / name
    p.write_text(json.dumps({"training": {"epochs": 1}, "model": model, **extra}))
    return p


def test_factory_builds_vq_and_kl_from_settings_json(tmp_path):
    from fmdiff.models.generators import VAEFactory
    from fmdiff.models.generators.vaefactory import build_from_json
    from fmdiff.models.vae import VQVAE, AutoencoderKL
    from fmdiff.nn.modules.vae import VectorQuantizer, VectorQuantizerEMA
    from fmdiff.utils.model_utils import build_vae_model
    small = dict(vb.LDCT_VQ, down_channels=[32, 64, 64], z_channels=32, embed_dim=32, codebook_size=512)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VAEFactory().build_from_json(_write(tmp_path, "ldct_vq.json", vb.LDCT_VQ))
        assert isinstance(m, VQVAE) and isinstance(m.codebook, VectorQuantizerEMA)
        assert m.codebook.embedding.shape == (16384, 256) and m.encoder.emb_channels is None
        assert m.encoder.conv_out.conv.out_channels == 256 and m.quant_conv.conv.weight.shape == (256, 256, 1, 1)
        assert isinstance(m.encoder.downs[0].blocks[0].in_layers if hasattr(m.encoder.downs[0].blocks[0], "in_layers")
                          else m.encoder.downs[0].blocks[0], torch.nn.Module) and len(m.encoder.downs) == 4
        m = build_from_json(str(_write(tmp_path, "mnist_vq.json", vb.MNIST_VQ)))
        assert isinstance(m, VQVAE) and isinstance(m.codebook, VectorQuantizer)
        assert m.codebook.embedding.shape == (512, 64) and m.codebook.commitment_cost == 0.25
        kl = dict(small, latent_type="kl", z_channels=4, embed_dim=4)
        for k in ("quantizer_type", "discriminator_type", "vq_beta", "vq_ema_decay", "vq_ema_eps"):
            kl.pop(k)
        m = VAEFactory().build_from_json(_write(tmp_path, "kl.json", kl))
        assert isinstance(m, AutoencoderKL) and m.quant_conv.conv.weight.shape == (8, 8, 1, 1)
        m = VAEFactory().build_from_json(_write(tmp_path, "dflt.json", {k: v for k, v in kl.items()
                                                                       if k != "latent_type"}))
        assert isinstance(m, AutoencoderKL)                        # latent_type defaults to "kl"
        p = _write(tmp_path, "util.json", vb.MNIST_VQ)
        m = build_vae_model({"__config_path__": str(p), "model": vb.MNIST_VQ}, torch.device("cpu"))
        assert isinstance(m, VQVAE) and not m.training
    with pytest.raises(ValueError, match="Missing __config_path__ in config."):
        build_vae_model({"model": vb.MNIST_VQ}, torch.device("cpu"))


def test_factory_error_messages(tmp_path):
    from fmdiff.models.generators import VAEFactory
    f = VAEFactory()
    missing = tmp_path / "nope.json"
    with pytest.raises(FileNotFoundError) as ei:
        f.build_from_json(missing)
    assert str(ei.value) == f"Config not found: {missing}"
    p = tmp_path / "nomodel.json"
    p.write_text(json.dumps({"training": {}}))
    with pytest.raises(ValueError) as ei:
        f.build_from_json(p)
    assert str(ei.value) == "Config must contain a 'model' section."
    with pytest.raises(ValueError) as ei:
        f.build_from_json(_write(tmp_path, "unet.json", dict(vb.MNIST_VQ, model_type="unet")))
    assert str(ei.value) == "Expected model_type 'vae', got 'unet'."
    with pytest.raises(ValueError) as ei:
        f.build_from_json(_write(tmp_path, "fsq.json", dict(vb.MNIST_VQ, latent_type="fsq")))
    assert str(ei.value) == "Unsupported latent_type 'fsq'. Expected one of ['kl', 'vq']."
    with pytest.raises(NotImplementedError):
        f.build_from_json(_write(tmp_path, "bn.json", dict(vb.MNIST_VQ, norm_type="bn")))
    with pytest.raises(NotImplementedError):
        f.build_from_json(_write(tmp_path, "relu.json", dict(vb.MNIST_VQ, act="relu")))
