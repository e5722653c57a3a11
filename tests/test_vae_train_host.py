"""CPU checks of the AutoencoderKL training path's host side: the unfold algebra, the C ABI of the latent 1x1
backward, the absence of a CPU path, the configurations that are refused, and the flat AdamW state (``FlatParams``)
against ``torch.optim.AdamW``'s own ``state_dict()``."""
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


# ------------------------------------------------------- FlatParams: the one owner of the torch AdamW state format
HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01)


def _two_layer(seed=3):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))


@pytest.fixture(scope="module")
def torch_adamw():
    """A twin under torch.optim.AdamW after two steps on seeded random gradients: (twin, optimizer, state_dict)."""
    twin = _two_layer()
    opt = torch.optim.AdamW(twin.parameters(), lr=1e-3, weight_decay=0.01)
    g = torch.Generator().manual_seed(4)
    for _ in range(2):
        for p in twin.parameters():
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    return twin, opt, opt.state_dict()


def _slices(flat, model):
    out = []
    for p in model.parameters():
        off, n = flat.offsets[id(p)]
        out.append((flat.m[off:off + n].view_as(p), flat.v[off:off + n].view_as(p)))
    return out


def test_flat_adamw_state_against_torch(torch_adamw):
    from fmdiff.pipelines.train.fused import FlatParams
    twin, opt, sd = torch_adamw
    model = _two_layer()
    flat = FlatParams(model)
    assert flat.load_adamw_state_dict(sd) == 2
    for i, (m, v) in enumerate(_slices(flat, model)):
        assert torch.equal(m, sd["state"][i]["exp_avg"]) and torch.equal(v, sd["state"][i]["exp_avg_sq"])
    out = flat.adamw_state_dict(2, **HYPER)
    assert sorted(out) == ["param_groups", "state"] and sorted(out["state"]) == sorted(sd["state"])
    for i, want in sd["state"].items():
        assert sorted(out["state"][i]) == sorted(want)
        for k, t in want.items():
            got = out["state"][i][k]
            assert got.dtype == t.dtype and got.shape == t.shape and got.device == t.device and torch.equal(got, t), k
            assert got.data_ptr() not in (flat.m.data_ptr(), flat.v.data_ptr())
    (group,), (want,) = out["param_groups"], sd["param_groups"]
    assert set(group) == set(want)
    assert group == want   # the values too: torch's defaults, the hyperparameters passed, the parameter indices
    with_lr = flat.adamw_state_dict(2, **HYPER, initial_lr=2e-3)["param_groups"][0]
    assert set(with_lr) == set(want) | {"initial_lr"} and with_lr["initial_lr"] == 2e-3
    torch.optim.AdamW(twin.parameters(), lr=1.0).load_state_dict(out)
    fresh = torch.optim.AdamW(_two_layer().parameters(), lr=1.0)
    fresh.load_state_dict(out)
    for p, (m, v) in zip(fresh.param_groups[0]["params"], _slices(flat, model)):
        assert torch.equal(fresh.state[p]["exp_avg"], m) and torch.equal(fresh.state[p]["exp_avg_sq"], v)
        assert float(fresh.state[p]["step"]) == 2.0
    assert fresh.param_groups[0]["lr"] == 1e-3 and fresh.param_groups[0]["weight_decay"] == 0.01


def test_flat_adamw_load_zeroes_first(torch_adamw):
    from fmdiff.pipelines.train.fused import FlatParams
    sd = torch_adamw[2]
    partial = {"state": {i: e for i, e in sd["state"].items() if i != 1}, "param_groups": sd["param_groups"]}
    model = _two_layer()
    flat = FlatParams(model)
    flat.m.fill_(1.0)
    flat.v.fill_(1.0)
    assert flat.load_adamw_state_dict(partial) == 2
    for i, (m, v) in enumerate(_slices(flat, model)):
        if i == 1:
            assert not m.any() and not v.any()
        else:
            assert torch.equal(m, sd["state"][i]["exp_avg"]) and torch.equal(v, sd["state"][i]["exp_avg_sq"])


def test_flat_adamw_load_takes_string_keys(torch_adamw):
    from fmdiff.pipelines.train.fused import FlatParams
    sd = torch_adamw[2]
    a, b = FlatParams(_two_layer()), FlatParams(_two_layer())
    assert a.load_adamw_state_dict(sd) == 2
    assert b.load_adamw_state_dict({"state": {str(i): e for i, e in sd["state"].items()},
                                    "param_groups": sd["param_groups"]}) == 2
    assert a.m.any() and torch.equal(a.m, b.m) and torch.equal(a.v, b.v)


def test_flat_adamw_state_is_empty_at_step_zero():
    from fmdiff.pipelines.train.fused import FlatParams
    flat = FlatParams(_two_layer())
    flat.m.fill_(1.0)   # whatever the buffers hold: no step, no state, as a fresh torch optimizer
    out = flat.adamw_state_dict(0, **HYPER)
    assert out["state"] == {} and out["param_groups"][0]["params"] == [0, 1, 2, 3]
    assert flat.load_adamw_state_dict(out) == 0 and not flat.m.any()
    assert flat.load_adamw_state_dict(None) == 0
