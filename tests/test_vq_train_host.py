"""CPU checks of the VQVAE training path's host side: the C ABI of the latent join, the absence of a CPU path, the
configurations that are refused and those that are now accepted."""
import ctypes
import os
import re
import warnings

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = dict(in_channels=1, out_channels=1, resolution=16, base_ch=32, down_channels=[32, 32], num_res_blocks=1,
             attn_resolutions=[], z_channels=4, embed_dim=4, use_attention=False, attn_heads=4, attn_dim_head=8,
             codebook_size=32)
VQ_CFG = ({"recon_type": "mse", "codebook_weight": 1.0}, {"latent_type": "vq"})


def _vqvae(**kw):
    from fmdiff.models.vae import VQVAE
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return VQVAE(**{**SMALL, **kw})


def test_join_kernel_is_declared_and_exported():
    from fmdiff import _lib
    src = open(os.path.join(REPO, "include", "fmdiff.h")).read()
    assert re.search(r"\bfmd_vq_join_bwd\s*\(", src)
    assert "fmd_vq_join_bwd" in _lib.SIGNATURES and len(_lib.SIGNATURES["fmd_vq_join_bwd"]) == 16
    assert os.path.exists(_lib.LIB_PATH), "libfmdiff_hip.so not built (run __graft_entry__.build())"
    try:
        L = ctypes.CDLL(_lib.LIB_PATH)
    except OSError as e:  # HIP runtime absent on this host
        pytest.skip(f"HIP runtime not loadable here: {e}")
    assert hasattr(L, "fmd_vq_join_bwd")
    # bad arguments come back as -1 before anything is launched (null pointers: nothing is touched)
    fn = _lib.lib().fmd_vq_join_bwd
    assert fn(None, 8, 4, 1, 8, None, None, None, 0, 0, None, 0.25, 1.0, None, 8, None) == -1


@pytest.mark.parametrize("qt", ["ema", "classic"])
def test_training_has_no_cpu_path(qt):
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    from fmdiff.runtime import ops
    vae = _vqvae(quantizer_type=qt)
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vae.forward_train(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        VAETrainStep(vae, *VQ_CFG, lr=1e-3).step(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.vq_join_bwd(None, 4, torch.zeros(2, 4, 4, 8), None, None, None, 0.25)


@pytest.mark.parametrize("kw,msg", [
    (dict(spatial_dims=3), "spatial_dims"),
    (dict(emb_channels=16), "emb_channels"),
    (dict(dropout=0.1), "dropout"),
])
def test_refused_configurations(kw, msg):
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    vae = _vqvae(**kw)
    x = torch.zeros(2, 1, *(16,) * vae.spatial_dims)
    with pytest.raises(NotImplementedError, match=msg):
        vae.forward_train(x)
    with pytest.raises(NotImplementedError, match=msg):
        VAETrainStep(vae, *VQ_CFG)


def test_wide_latents_are_accepted():
    """The POINTWISE_MAXC limit of the AutoencoderKL path does not apply: the VQ latent convs run on MFMA."""
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    from fmdiff.runtime.vae_engine import get_vae_engine
    for kw in (dict(embed_dim=16), dict(z_channels=20, embed_dim=12), dict(z_channels=256, embed_dim=256)):
        vae = _vqvae(**kw)
        get_vae_engine(vae).check_trainable()
        st = VAETrainStep(vae, *VQ_CFG)
        assert st.vq and st.criterion.effective_codebook_weight == 1.0
    wide = _vqvae(z_channels=8, embed_dim=264)   # beyond the quantizer kernels' 256
    with pytest.raises(NotImplementedError, match="embed_dim"):
        get_vae_engine(wide).check_trainable()


def test_eps_is_refused_for_a_vqvae():
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    st = VAETrainStep(_vqvae(), *VQ_CFG)
    with pytest.raises(ValueError, match="eps"):
        st.step(torch.zeros(2, 1, 16, 16), torch.zeros(2, 4, 8, 8))


def test_classic_codebook_is_outside_the_flat_update():
    """The classic codebook parameter lies behind the trained parameters in the flat buffer; the EMA model has no
    such parameter and its layout is the plain one."""
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    vae = _vqvae(quantizer_type="classic")
    st = VAETrainStep(vae, *VQ_CFG)
    off, n = st.flat.offsets[id(vae.codebook.embedding)]
    assert off == st.n_trained and off + n == st.flat.numel and n == 32 * 4
    ema = VAETrainStep(_vqvae(quantizer_type="ema"), *VQ_CFG)
    assert ema.n_trained == ema.flat.numel
    sd = st.state_dict()
    assert len(sd["param_groups"][0]["params"]) == len(list(vae.parameters()))
