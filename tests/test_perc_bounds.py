"""tests/perc_bounds.py on the CPU: the closed forms equal torch autograd in fp64, the fp32 emulation of the kernels'
arithmetic lies inside every bound, every mutant misses one, and the oracle is the composition it claims to be."""
import pytest
import torch
import torch.nn.functional as F

import perc_bounds as PB

F64, F32 = torch.float64, torch.float32
STAGE_CASES = [((20, 12), None), ((20, 12), (32, 32)), ((40, 36), (32, 32)), ((12, 20), (224, 224))]


def _images(N, C, hw, seed, mode):
    recon, target = PB.make_images(N, C, hw[0], hw[1], seed)
    if mode == "clamp":      # raw decoder output: outside [-1, 1] too, and exactly -1 and 1
        recon = recon * 3 - 1.5
        recon.view(-1)[:4] = torch.tensor([-1.0, 1.0, -1.0, 1.0])
    elif mode == "sigmoid":
        recon = recon * 8 - 4
    return recon, target


def _g_stage(N, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, hw[0], hw[1], 8, generator=g) * 0.5).to(torch.bfloat16)


def _torch_stage(recon, target, mode, size):
    x = torch.cat([PB.image_map(recon, mode), target])
    if x.shape[1] == 1:
        x = x.repeat(1, 3, 1, 1)
    if size is not None:
        x = F.interpolate(x, size=size, mode="bilinear", align_corners=False)
    return x


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("mode", PB.IMAGE_MODES)
@pytest.mark.parametrize("hw,size", STAGE_CASES[:3])
def test_stage_closed_form_is_torch_in_fp64(C, mode, hw, size):
    recon, target = _images(2, C, hw, 1, mode)
    rd = recon.double().requires_grad_()
    x = _torch_stage(rd, target.double(), mode, size)
    v = PB.stage(recon, target, mode, size)
    assert (v[..., :3].permute(0, 3, 1, 2) - x.detach()).abs().max() < 1e-12
    assert v[..., 3:].abs().max() == 0
    g = _g_stage(2, x.shape[2:], 2)
    (x[:2] * g.double()[..., :3].permute(0, 3, 1, 2)).sum().backward()
    assert (PB.stage_bwd(g, recon, mode) - rd.grad).abs().max() < 1e-12


# every map and channel count at the small sizes, the 224 case once
STAGE_GRID = [(C, mode, hw, size) for hw, size in STAGE_CASES for C in (1, 3) for mode in PB.IMAGE_MODES
              if size != (224, 224) or (C, mode) == (1, "clamp")]


@pytest.mark.parametrize("C,mode,hw,size", STAGE_GRID)
def test_stage_emulation_inside_bounds(C, mode, hw, size):
    recon, target = _images(2, C, hw, 3, mode)
    ref, bound = PB.stage(recon, target, mode, size), PB.stage_bound(recon, target, mode, size)
    emu = PB.stage(recon, target, mode, size, dtype=F32)
    hi = emu.to(torch.bfloat16)
    lo = (emu - hi.float()).to(torch.bfloat16)
    assert ((hi.double() + lo.double() - ref).abs() <= bound).all()
    g = _g_stage(2, ref.shape[1:3], 4)
    rb, bb = PB.stage_bwd(g, recon, mode), PB.stage_bwd_bound(g, recon, mode)
    eb = PB.stage_bwd(g, recon, mode, dtype=F32)
    assert ((eb.double() - rb).abs() <= bb).all()
    assert (bb <= 1e-3 * rb.abs().max()).all()     # the bounds are not vacuous


# shrinking never reaches past the edge (the last destination reads source 38.875 of 0..39): no edge clamp to miss
@pytest.mark.parametrize("mutant,hw,size", [(m, hw, size) for m in ("align_corners", "no_half_pixel", "no_edge_clamp")
                                            for hw, size in STAGE_CASES[1:3] if m != "no_edge_clamp" or hw[0] < size[0]])
def test_stage_mutants_miss(mutant, hw, size):
    recon, target = _images(2, 1, hw, 3, "identity")
    ref, bound = PB.stage(recon, target, "identity", size), PB.stage_bound(recon, target, "identity", size)
    emu = PB.stage(recon, target, "identity", size, dtype=F32, mutant=mutant)
    assert ((emu.double() - ref).abs() > bound).any()
    g = _g_stage(2, ref.shape[1:3], 4)
    rb, bb = PB.stage_bwd(g, recon), PB.stage_bwd_bound(g, recon)
    eb = PB.stage_bwd(g, recon, dtype=F32, mutant=mutant)
    assert ((eb.double() - rb).abs() > bb).any()


TAP_CASES = [(8, 8, (20, 12)), (24, 20, (5, 3)), (64, 64, (2, 2)), (8, 3, (1, 1))]


def _g_below(N, H, W, Cp, pool, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (N, H // 2, W // 2, Cp) if pool else (N, H, W, Cp)
    return (torch.randn(shape, generator=g) * 0.01).to(torch.bfloat16)


TAP_POOL = [(Cp, C, hw, pool) for Cp, C, hw in TAP_CASES for pool in (False, True) if not pool or min(hw) >= 2]
# the pool only shows in the gradient from below
TAP_GRID = [(Cp, C, hw, pool, below) for Cp, C, hw, pool in TAP_POOL for below in (False, True) if below or not pool]


@pytest.mark.parametrize("Cp,C,hw,pool", TAP_POOL)
def test_tap_closed_form_is_torch_in_fp64(Cp, C, hw, pool):
    H, W = hw
    N, wgt, gl = 2, 0.5, 0.75
    y = PB.lattice_y(N, H, W, Cp, C, 5)
    yt = y[..., :C].permute(0, 3, 1, 2).double().requires_grad_()
    x = F.relu(yt)
    val = F.l1_loss(x[:N], x[N:])
    nxt = F.max_pool2d(x, 2, 2) if pool else x
    gb = _g_below(N, H, W, Cp, pool, 6)
    ((gl * wgt) * val + (nxt[:N] * gb.double()[..., :C].permute(0, 3, 1, 2)).sum()).backward()
    value, sgn, out = PB.tap_fwd(y, C, pool)
    assert abs(float(value) - float(val.detach())) < 1e-12
    assert (out[..., :C].permute(0, 3, 1, 2) - nxt.detach()).abs().max() == 0
    full, _ = PB.tap_bwd(y[:N], sgn, C, gl, wgt, gb, pool)
    assert (full[:N, ..., :C].permute(0, 3, 1, 2) - yt.grad[:N]).abs().max() < 1e-12
    assert full[:N, ..., C:].abs().max() == 0 if C < Cp else True
    assert torch.isnan(full[N:]).all()


def test_torch_pool_routes_to_the_first_maximum():
    for win, k in (([[1.0, 1.0], [1.0, 1.0]], 0), ([[0.0, 2.0], [2.0, 2.0]], 1)):
        x = torch.tensor(win).reshape(1, 1, 2, 2).requires_grad_()
        F.max_pool2d(x, 2, 2).sum().backward()
        assert x.grad.reshape(-1).tolist() == [1.0 if i == k else 0.0 for i in range(4)]


@pytest.mark.parametrize("Cp,C,hw,pool,below", TAP_GRID)
def test_tap_emulation_inside_bounds(Cp, C, hw, pool, below):
    H, W = hw
    N, wgt, gl = 2, 0.5, 0.75
    y = PB.lattice_y(N, H, W, Cp, C, 7)
    if H * W * C >= 100:   # every kink is in the input (the 1x1 and 2x2 maps are too small to hold them all)
        assert (y == 0).any() and ((y[:N] == y[N:]) & (y[:N] > 0)).any() and ((y[:N] < 0) & (y[N:] < 0)).any()
    value, sgn, out = PB.tap_fwd(y, C, pool)
    ev, es, eo = PB.tap_fwd(y, C, pool, dtype=F32)
    assert abs(float(ev) - float(value)) <= PB.tap_value_bound(y, C, value)
    assert torch.equal(es, sgn)
    hi = eo.to(torch.bfloat16)
    lo = (eo - hi.float()).to(torch.bfloat16)
    assert ((hi.double() + lo.double() - out).abs() <= PB.tap_out_bound(out)).all()
    gb = _g_below(N, H, W, Cp, pool, 8) if below else None
    ref, parts = PB.tap_bwd(y[:N], sgn, C, gl, wgt, gb, pool)
    emu, _ = PB.tap_bwd(y[:N], sgn, C, gl, wgt, gb, pool, dtype=F32)
    assert ((emu[:N].to(torch.bfloat16).double() - ref[:N]).abs() <= PB.tap_bwd_bound(ref, parts)).all()
    assert torch.isnan(emu[N:]).all()


def _tap_bwd_misses(mutant, pool=True):
    N, Cp, C, H, W = 2, 8, 8, 20, 12
    y = PB.lattice_y(N, H, W, Cp, C, 7)
    _, sgn, _ = PB.tap_fwd(y, C, pool)
    gb = _g_below(N, H, W, Cp, pool, 8)
    ref, parts = PB.tap_bwd(y[:N], sgn, C, 0.75, 0.5, gb, pool)
    emu, _ = PB.tap_bwd(y[:N], sgn, C, 0.75, 0.5, gb, pool, dtype=F32, mutant=mutant)
    return emu, ref, parts


def test_tap_mutants_miss():
    for mutant in ("pool_last_max", "relu_grad_at_zero"):
        emu, ref, parts = _tap_bwd_misses(mutant)
        assert ((emu[:2].double() - ref[:2]).abs() > PB.tap_bwd_bound(ref, parts)).any(), mutant
    emu, ref, _ = _tap_bwd_misses("grad_to_target_half")
    assert not torch.isnan(emu[2:]).all()
    y = PB.lattice_y(2, 20, 12, 24, 20, 7)
    value, sgn, _ = PB.tap_fwd(y, 20, False)
    ev, es, _ = PB.tap_fwd(y, 20, False, dtype=F32, mutant="sign_zero_is_one")
    assert not torch.equal(es, sgn)
    ev, _, _ = PB.tap_fwd(y, 20, False, dtype=F32, mutant="divisor_padded")
    assert abs(float(ev) - float(value)) > PB.tap_value_bound(y, 20, value)


def test_loss_fold_and_reversed_weights():
    values, weights = [0.03, 0.14, 0.08, 0.05], [1.0, 0.5, 0.25, 2.0]
    ref, mag = PB.loss_fold(values, weights)
    emu, _ = PB.loss_fold(values, weights, dtype=F32)
    assert abs(float(emu) - float(ref)) <= PB.loss_fold_bound(mag, 4)
    bad, _ = PB.loss_fold(values, weights, dtype=F32, mutant="weights_reversed")
    assert abs(float(bad) - float(ref)) > PB.loss_fold_bound(mag, 4)


@pytest.mark.parametrize("C,hw,resize", [(1, (16, 24), None), (3, (20, 12), 32)])
def test_oracle_is_the_composition_of_the_closed_forms(C, hw, resize):
    """perc_oracle in fp64 against stage -> conv -> tap_fwd chained by hand (fp64), values and loss."""
    feats = PB.build_features(PB.NARROW, 0).double()
    recon, target = PB.make_images(2, C, hw[0], hw[1], 9)
    layers, weights = (3, 8, 15, 22), (1.0, 0.5)
    loss, values = PB.perc_oracle(feats, recon, target, resize, layers, weights, dtype=F64)
    size = None if resize is None else (resize, resize)
    h = PB.stage(recon, target, "identity", size)[..., :3]
    mine, k = [], 0
    mods = list(feats)
    i = 0
    while i <= layers[-1]:
        conv = mods[i]
        y = F.conv2d(h.permute(0, 3, 1, 2), conv.weight, conv.bias, padding=1).permute(0, 2, 3, 1).contiguous()
        i += 2
        pool = i < len(mods) and isinstance(mods[i], torch.nn.MaxPool2d)
        K = y.shape[-1]
        if i - 1 in layers:
            v, _, h = PB.tap_fwd(y, K, pool)
            mine.append(v)
        else:
            h = y.clamp_min(0)
        i += int(pool)
    assert len(mine) == len(values) == 4
    for a, b in zip(mine, values):
        assert abs(float(a) - float(b.detach())) <= 1e-12 * abs(float(b.detach()))
    want, _ = PB.loss_fold(mine, [1.0, 0.5, 1.0, 1.0])
    assert abs(float(want) - float(loss.detach())) <= 1e-12 * abs(float(loss.detach()))
