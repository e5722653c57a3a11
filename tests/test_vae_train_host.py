"""CPU checks of the AutoencoderKL training path's host side: the unfold algebra, the C ABI of the latent 1x1
backward, the absence of a CPU path and the configurations that are refused."""
import ctypes
import os
import re
import warnings

import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SMALL = dict(in_channels=1, out_channels=1, resolution=16, base_ch=32, down_channels=[32, 32], num_res_blocks=1,
             attn_resolutions=[], z_channels=4, embed_dim=4, use_attention=False, attn_heads=4, attn_dim_head=8)


def _vae(**kw):
    from fmdiff.models.vae import AutoencoderKL
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return AutoencoderKL(**{**SMALL, **kw})


def test_unfold_matches_autograd_of_conv3x3_then_conv1x1():
    from fmdiff.runtime.vae_engine import unfold_quant_grads
    g = torch.Generator().manual_seed(5)
    O, Z, C = 6, 5, 7
    r = lambda *s: torch.randn(s, generator=g, dtype=torch.float64)
    w_out, b_out, wq, bq = r(Z, C, 3, 3), r(Z), r(O, Z), r(O)
    x, dy = r(2, C, 6, 5), r(2, O, 6, 5)
    # the fold computes the same function ...
    wf = torch.einsum("oz,zchw->ochw", wq, w_out).requires_grad_()
    bf = (wq @ b_out + bq).requires_grad_()
    two = F.conv2d(F.conv2d(x, w_out, b_out, padding=1), wq.reshape(O, Z, 1, 1), bq)
    one = F.conv2d(x, wf, bf, padding=1)
    assert (one - two).abs().max() <= 1e-12 * two.abs().max()
    one.backward(dy)
    # ... and its gradients unfold onto the two convs' own
    leaves = [t.clone().requires_grad_() for t in (w_out, b_out, wq, bq)]
    F.conv2d(F.conv2d(x, leaves[0], leaves[1], padding=1), leaves[2].reshape(O, Z, 1, 1), leaves[3]).backward(dy)
    got = unfold_quant_grads(wq, w_out, b_out, wf.grad, bf.grad)
    for a, l in zip(got, leaves):
        assert a.shape == l.grad.shape
        assert (a - l.grad).abs().max() <= 1e-12 * l.grad.abs().max()
    assert got[3].data_ptr() != bf.grad.data_ptr()   # tensors out: the fold's gradient is zeroed afterwards


def test_pointwise_bwd_is_declared_and_exported():
    from fmdiff import _lib
    src = open(os.path.join(REPO, "include", "fmdiff.h")).read()
    for name in ("fmd_pointwise_bwd", "fmd_pointwise_bwd_workspace"):
        assert re.search(r"\b" + name + r"\s*\(", src), name
        assert name in _lib.SIGNATURES
    assert os.path.exists(_lib.LIB_PATH), "libfmdiff_hip.so not built (run __graft_entry__.build())"
    try:
        L = ctypes.CDLL(_lib.LIB_PATH)
    except OSError as e:  # HIP runtime absent on this host
        pytest.skip(f"HIP runtime not loadable here: {e}")
    assert hasattr(L, "fmd_pointwise_bwd") and hasattr(L, "fmd_pointwise_bwd_workspace")
    ws = _lib.lib().fmd_pointwise_bwd_workspace
    from fmdiff.runtime import ops
    rows = ops.POINTWISE_ROWS
    assert ws(rows, 4, 4) == 20 * 8 and ws(rows + 1, 4, 4) == 2 * 20 * 8 and ws(1, 8, 8) == 72 * 8
    assert ws(100, 9, 4) == -1 and ws(100, 4, 9) == -1 and ws(100, 0, 4) == -1 and ws(0, 4, 4) == -1


def test_training_has_no_cpu_path():
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    from fmdiff.runtime import ops
    vae = _vae()
    x = torch.zeros(2, 1, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        vae.forward_train(x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        VAETrainStep(vae, {"recon_type": "mse", "kl_weight": 1e-3}, lr=1e-3).step(x)
    dy = torch.zeros(2, 4, 4, 8, dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.pointwise_bwd(dy, dy, torch.zeros(4, 4))


@pytest.mark.parametrize("kw,msg", [
    (dict(spatial_dims=3), "spatial_dims"),
    (dict(emb_channels=16), "emb_channels"),
    (dict(dropout=0.1), "dropout"),
    (dict(z_channels=9), "z_channels"),
    (dict(embed_dim=16), "embed_dim"),
])
def test_refused_configurations(kw, msg):
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    vae = _vae(**kw)
    x = torch.zeros(2, 1, *(16,) * vae.spatial_dims)
    with pytest.raises(NotImplementedError, match=msg):
        vae.forward_train(x)
    with pytest.raises(NotImplementedError, match=msg):
        VAETrainStep(vae, {})


def test_tanh_out_is_refused():
    vae = _vae()
    vae.decoder.tanh_out = True
    with pytest.raises(NotImplementedError, match="tanh_out"):
        vae.forward_train(torch.zeros(2, 1, 16, 16))


def test_train_step_refuses_what_is_not_built():
    from fmdiff.pipelines.train import vae_lib
    vae = _vae()
    with pytest.raises(NotImplementedError):
        vae_lib.VAETrainStep(vae, {"gan_weight": 0.5})
    with pytest.raises(NotImplementedError):
        vae_lib.VAETrainStep(vae, {"perceptual_weight": 0.1})
    with pytest.raises(NotImplementedError):
        vae_lib.VAETrainStep(vae, {}, {"latent_type": "vq"})
    with pytest.raises(NotImplementedError, match="DESIGN"):
        vae_lib.train(None, "x.json")


def test_train_step_state_dict_round_trip():
    from fmdiff.pipelines.train.vae_lib import VAETrainStep
    vae = _vae()
    st = VAETrainStep(vae, {"learning_rate": 3e-4, "weight_decay": 0.01})
    assert st.lr == 3e-4 and st.weight_decay == 0.01
    # the parameters are views of the flat buffer, in model.parameters() order
    off = 0
    for p in vae.parameters():
        assert p.data_ptr() == st.flat.data.data_ptr() + 4 * off and p.grad.data_ptr() == st.flat.grad.data_ptr() + 4 * off
        off += p.numel()
    g = torch.Generator().manual_seed(1)
    st.m.copy_(torch.randn(st.m.shape, generator=g))
    st.v.copy_(torch.rand(st.v.shape, generator=g))
    st.global_step = 7
    sd = st.state_dict()
    assert sd["global_step"] == 7 and len(sd["state"]) == len(list(vae.parameters()))
    opt = torch.optim.AdamW(vae.parameters(), lr=1.0)
    opt.load_state_dict({k: sd[k] for k in ("state", "param_groups")})   # torch's own format
    other = VAETrainStep(_vae(), {})
    other.load_state_dict(sd)
    assert other.global_step == 7 and other.lr == 3e-4 and other.weight_decay == 0.01
    assert torch.equal(other.m, st.m) and torch.equal(other.v, st.v)
