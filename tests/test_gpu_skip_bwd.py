"""fmd_skip_bwd (csrc/skip_bwd.hip; ops.skip_bwd; Engine.res_block): the skip conv's weight, bias and data gradient
in the GroupNorm-1 backward apply pass, against the launches it replaces on the same bf16 operands.

dx must equal ops.conv1x1_gn_apply bit for bit (same MFMA, k order and rounding).  dW_s / db_s are other sums of
the same exact products: against the fp64 product at the weight-gradient tolerances of test_gpu_wgrad_group.py
(rtol 2e-2, atol 2e-2 max|ref| for dW; 1e-3 for db), against ops.wgrad(ks=1) within the order bound of
skip_bwd_cases.py, and bit-identical run to run.  What the plan refuses falls back to today's launches."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import skip_bwd_cases as sc

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ops():
    from fmdiff.runtime import ops as O
    return O


def _dev(t):
    return t.clone().to(DEV) if t is not None else None


@functools.lru_cache(maxsize=None)
def _today(name, acc0, acc1, accumulate):
    """(dx0, dx1, dW, db) of ops.conv1x1_gn_apply + ops.wgrad(ks=1): the launches the fused pass replaces."""
    O = ops()
    p = sc.problem(name)
    wt = O.prep_weights(p["w"].to(DEV), 1)
    dx0, dx1, dw, db = _dev(p["dx0"]), _dev(p["dx1"]), _dev(p["dw0"]), _dev(p["db0"])
    O.conv1x1_gn_apply(_dev(p["dy"]), wt, _dev(p["dz"]), _dev(p["x0"]), _dev(p["x1"]), _dev(p["P"]), _dev(p["Q"]),
                       _dev(p["R"]), dx0, acc0, dx1, acc1)
    O.wgrad(_dev(p["x0"]), _dev(p["dy"]), dw, src1=_dev(p["x1"]), ks=1, pad=0, db=db, accumulate=accumulate)
    torch.cuda.synchronize()
    return dx0.cpu(), dx1.cpu() if dx1 is not None else None, dw.cpu(), db.cpu()


def _fused(name, acc0, acc1, accumulate, groups=0):
    """The engine's sequence: ops.skip_bwd where its plan takes the problem, else today's two launches."""
    O = ops()
    p = sc.problem(name)
    wt = O.prep_weights(p["w"].to(DEV), 1)
    dx0, dx1, dw, db = _dev(p["dx0"]), _dev(p["dx1"]), _dev(p["dw0"]), _dev(p["db0"])
    a = (_dev(p["dy"]), wt, _dev(p["dz"]), _dev(p["x0"]), _dev(p["x1"]), _dev(p["P"]), _dev(p["Q"]), _dev(p["R"]),
         dx0, acc0, dx1, acc1)
    taken = O.skip_bwd(*a, dw, db, accumulate=accumulate, groups=groups, min_tiles=0)
    if not taken:
        O.conv1x1_gn_apply(*a)
        O.wgrad(a[3], a[0], dw, src1=a[4], ks=1, pad=0, db=db, accumulate=accumulate)
    torch.cuda.synchronize()
    return taken, (dx0.cpu(), dx1.cpu() if dx1 is not None else None, dw.cpu(), db.cpu())


def _check(name, acc0, acc1, accumulate, groups=0, want_taken=None):
    p = sc.problem(name)
    ref = _today(name, acc0, acc1, accumulate)
    taken, got = _fused(name, acc0, acc1, accumulate, groups)
    taken2, again = _fused(name, acc0, acc1, accumulate, groups)
    if want_taken is not None:
        assert taken == taken2 == want_taken
    # dx: bit-identical to fmd_conv_gn_apply
    assert torch.equal(got[0], ref[0]), "dx0 differs from conv1x1_gn_apply"
    if ref[1] is not None:
        assert torch.equal(got[1], ref[1]), "dx1 differs from conv1x1_gn_apply"
    # run to run
    assert torch.equal(got[2], again[2]) and torch.equal(got[3], again[3]), "dW / db differ between two runs"
    assert torch.equal(got[0], again[0])
    # dW / db against the fp64 product of the bf16 operands
    dw_ref, db_ref, _, _ = sc.reference(name)
    dw = (got[2].double() - p["dw0"].double() if accumulate else got[2].double()).reshape(dw_ref.shape)
    db = got[3].double() - p["db0"].double() if accumulate else got[3].double()
    e_w, e_b = (dw - dw_ref).abs().max().item(), (db - db_ref).abs().max().item()
    bw, bb = sc.order_bound(name)
    r_w = ((got[2].double() - ref[2].double()).reshape(bw.shape).abs() / bw).max().item()
    r_b = ((got[3].double() - ref[3].double()).abs() / bb).max().item()
    print(f"{name} acc {acc0}{acc1} accumulate {accumulate} groups {groups} taken {taken}: max|dW - fp64| {e_w:.3e} "
          f"(max|ref| {dw_ref.abs().max().item():.3e}), max|db - fp64| {e_b:.3e}; vs ops.wgrad / order bound: "
          f"dW {r_w:.3e}, db {r_b:.3e}")
    torch.testing.assert_close(dw, dw_ref, rtol=2e-2, atol=2e-2 * dw_ref.abs().max().item())
    torch.testing.assert_close(db, db_ref, rtol=1e-3, atol=1e-3 * db_ref.abs().max().item())
    # ... and against the launch it replaces, within the order bound
    assert r_w <= 1.0 and r_b <= 1.0, (r_w, r_b)
    if not taken:   # the fallback is today's path exactly
        assert torch.equal(got[2], ref[2]) and torch.equal(got[3], ref[3])
    return taken


# M = 288 = 4.5 tiles of 64 pixels, 144 pixels per image: the third tile straddles the images, the fifth is partial.
# min_tiles = 0: these shapes are far below the floor the plan keeps by default (test_default_plan_keeps_its_floor)
@pytest.mark.parametrize("name", ["c128_128", "c256_128", "k256", "refused", "single", "c192"])
@pytest.mark.parametrize("acc0,acc1,accumulate", [(0, 0, True), (1, 0, False), (0, 1, True), (1, 1, False)])
def test_skip_bwd_vs_replaced_launches(name, acc0, acc1, accumulate):
    O = ops()
    p = sc.problem(name)
    plan = O.skip_bwd_plan(p["N"], p["H"] * p["W"], p["C0"], p["C1"], p["Kd"], min_tiles=0)
    if name == "refused":
        assert plan is None
    if p["Kd"] == 128:
        assert plan is not None and plan.c_tile == 128
    _check(name, acc0, acc1 if p["C1"] else 0, accumulate, want_taken=plan is not None)


def test_default_plan_keeps_its_floor():
    """With the default floor (SKIP_BWD_MIN_TILES tiles per pixel group) a small problem is refused and runs
    today's launches; nothing is written by a refused call."""
    O = ops()
    p = sc.problem("c128_128")
    assert O.skip_bwd_plan(p["N"], p["H"] * p["W"], p["C0"], p["C1"], p["Kd"]) is None
    wt = O.prep_weights(p["w"].to(DEV), 1)
    dx0, dx1, dw, db = _dev(p["dx0"]), _dev(p["dx1"]), _dev(p["dw0"]), _dev(p["db0"])
    assert not O.skip_bwd(_dev(p["dy"]), wt, _dev(p["dz"]), _dev(p["x0"]), _dev(p["x1"]), _dev(p["P"]), _dev(p["Q"]),
                          _dev(p["R"]), dx0, 0, dx1, 0, dw, db)
    torch.cuda.synchronize()
    assert torch.equal(dw.cpu(), p["dw0"]) and torch.equal(db.cpu(), p["db0"]) and torch.equal(dx0.cpu(), p["dx0"])


# forced pixel groups: one workgroup per c-tile; 3 over the 5 tiles of M = 288 and over the 8 tiles of M = 512
# (uneven); more groups than tiles (idle workgroups, which must not contribute a slab)
@pytest.mark.parametrize("name,groups", [("g16", 1), ("g16", 3), ("g16", 11), ("c128_128", 3), ("c256_128", 16),
                                         ("single", 2), ("c192", 3)])
def test_skip_bwd_forced_groups(name, groups):
    O = ops()
    p = sc.problem(name)
    M, C = p["M"], p["C0"] + p["C1"]
    plan = O.skip_bwd_plan(p["N"], p["H"] * p["W"], p["C0"], p["C1"], p["Kd"], groups)   # forced: no floor
    tiles = -(-M // 64)
    assert plan.workgroups == groups * -(-C // plan.c_tile)
    assert plan.slabs == min(groups, tiles)
    assert plan.ws_floats == plan.slabs * (p["Kd"] * C + p["Kd"])
    assert _check(name, 1, 0, True, groups=groups, want_taken=True)
    assert _check(name, 0, 1, False, groups=groups, want_taken=True)


# ------------------------------------------------------------------------------------------------ engine
def _build(meta):
    from fmdiff.models.generators import DiffusionUNetFactory
    tr = meta["training"]
    return DiffusionUNetFactory().build(meta["unet"], tr["conditioning"], tr["channels"] or 1)


@functools.lru_cache(maxsize=None)
def _step_inputs(hw):
    g = torch.Generator().manual_seed(3)
    clean = torch.rand(2, 1, hw, hw, generator=g)
    ldct = torch.rand(2, 1, hw, hw, generator=g)
    noise = torch.randn(2, 1, hw, hw, generator=g)
    t = torch.rand(2, generator=g)
    return clean, ldct, noise, t


@functools.lru_cache(maxsize=None)
def _oracle_grads(name, hw):
    """fp32 CPU oracle gradients of one FM train step; computed once per model."""
    import json
    import os
    from oracle import spec as S
    from oracle import train_step as OT
    from oracle import unet as U
    meta = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))[name]
    tr = meta["training"]
    spec = S.derive_spec(meta["unet"], tr["conditioning"], tr["channels"] or 1)
    sd = {k: v.requires_grad_() for k, v in U.seeded_state_dict(spec, meta["seed"]).items()}
    loss, scaled = OT.fm_loss(sd, spec, *_step_inputs(hw), 1000)
    scaled.backward()
    return loss.item(), {k: v.grad.double() for k, v in sd.items()}


def _engine_step(meta, hw, monkeypatch, fused):
    from oracle import spec as S
    from oracle import unet as U
    O = ops()
    monkeypatch.setattr(O, "SKIP_BWD", fused)
    monkeypatch.setattr(O, "SKIP_BWD_MIN_TILES", 0)   # the goldens are far below the floor of the default plan
    calls = []
    real = getattr(O.skip_bwd, "real", O.skip_bwd)

    def counted(dy, *a, **kw):
        # operands of the order bound: dy and the block input (positions as ops.skip_bwd)
        calls.append((dy.detach().clone(), a[2].detach().clone(), a[3].detach().clone() if a[3] is not None else None,
                      a[11].data_ptr()))
        return real(dy, *a, **kw)
    counted.real = real
    monkeypatch.setattr(O, "skip_bwd", counted)
    model = _build(meta).to(DEV)
    tr = meta["training"]
    model.load_state_dict(U.seeded_state_dict(S.derive_spec(meta["unet"], tr["conditioning"], tr["channels"] or 1),
                                              meta["seed"]))
    clean, ldct, noise, t = (v.to(DEV) for v in _step_inputs(hw))
    x_t = (1.0 - t[:, None, None, None]) * clean + t[:, None, None, None] * noise
    pred = model(x_t, (t * 999).long(), context=ldct)
    loss = F.mse_loss(pred, noise - clean)
    loss.backward()
    torch.cuda.synchronize()
    by_ptr = {p.grad.data_ptr(): k for k, p in model.named_parameters()}
    ops_of = {by_ptr[c[3]]: c[:3] for c in calls}
    return loss.item(), {k: p.grad.detach().cpu() for k, p in model.named_parameters()}, ops_of


# fm_step (32^2; 32 / 64 channels: no block is taken, the switch must change nothing) and the config-B family at
# 64^2 (128-channel levels: fused blocks)
@pytest.mark.parametrize("name,hw,fused_blocks", [("fm_step", 32, False), ("ldct_fm_diffusers_b64", 64, True)])
def test_engine_step_skip_bwd_on_vs_off(golden, name, hw, fused_blocks, monkeypatch):
    _, M = golden
    meta = M[name]
    l0, g0, c0 = _engine_step(meta, hw, monkeypatch, False)
    l1, g1, c1 = _engine_step(meta, hw, monkeypatch, True)
    assert not c0 and bool(c1) == fused_blocks, (list(c0), list(c1))
    assert l0 == l1
    skip_w = {k for k in g0 if "skip_connection" in k}
    assert {k for k in c1} <= skip_w
    for k in g0:
        base = k.rsplit(".", 1)[0] + ".weight"
        if base not in c1:   # every gradient but the fused skip convs' weight and bias: bit-identical
            assert torch.equal(g0[k], g1[k]), k
            continue
        dy, x0, x1 = c1[base]
        x = x0 if x1 is None else torch.cat([x0, x1], -1)
        dyf, xf = dy.double().reshape(-1, dy.shape[-1]).cpu(), x.double().reshape(-1, x.shape[-1]).cpu()
        Mp = dyf.shape[0]
        # the order bound of skip_bwd_cases.py on this block's operands
        S = dyf.abs().t() @ xf.abs() if k.endswith("weight") else dyf.abs().sum(0)
        bound = 2 * Mp * sc.U * S
        diff = (g1[k].double() - g0[k].double()).reshape(S.shape).abs()
        print(f"{k}: max diff / bound {(diff / bound).max().item():.3e}")
        assert (diff <= bound).all(), k
    loss_ref, ref = _oracle_grads(name, hw)
    assert abs(l1 - loss_ref) / loss_ref < 1e-2
    num = den = 0.0
    worst = (1.0, "")
    for k, g in g1.items():
        g, r = g.double(), ref[k]
        num += (g - r).pow(2).sum().item()
        den += r.pow(2).sum().item()
        if r.norm() > 1e-3 * math.sqrt(den + 1e-30):
            cos = ((g * r).sum() / (g.norm() * r.norm() + 1e-30)).item()
            if cos < worst[0]:
                worst = (cos, k)
    rel = math.sqrt(num / den)
    print(f"{name}: fused blocks {len(c1)}; grad rel L2 vs oracle {rel:.3e}, worst cosine {worst}")
    assert rel < 5e-2
    assert worst[0] > 0.99, worst
