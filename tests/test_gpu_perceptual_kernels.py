"""csrc/perceptual.hip on the GPU: every element of every output of the four kernels against the per-output bounds
of tests/perc_bounds.py (fp64 references of the kernels' own inputs), bit-equal repeats, untouched target halves,
and negative return codes with nothing launched for bad arguments."""
import functools

import pytest
import torch

import perc_bounds as PB

pytestmark = pytest.mark.gpu
BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _ops():
    from fmdiff.runtime import ops
    return ops


def _images(N, C, hw, seed, mode):
    recon, target = PB.make_images(N, C, hw[0], hw[1], seed)
    if mode == "clamp":      # raw decoder output: outside [-1, 1] too, and exactly -1 and 1
        recon = recon * 3 - 1.5
        recon.view(-1)[:4] = torch.tensor([-1.0, 1.0, -1.0, 1.0])
    elif mode == "sigmoid":
        recon = recon * 8 - 4
    return recon, target


STAGE_CASES = [((20, 12), None), ((20, 12), (32, 32)), ((40, 36), (32, 32))]
STAGE_GRID = [(C, mode, hw, size) for hw, size in STAGE_CASES for C in (1, 3) for mode in PB.IMAGE_MODES]
STAGE_GRID.append((1, "clamp", (12, 20), (224, 224)))   # the real target: up to 47 readers of a source pixel per axis


@pytest.mark.parametrize("C,mode,hw,size", STAGE_GRID)
def test_stage_forward_and_backward_inside_bounds(C, mode, hw, size):
    ops = _ops()
    N = 2
    recon, target = _images(N, C, hw, 3, mode)
    rd, td = recon.to(DEV), target.to(DEV)
    out = ops.perc_stage(rd, td, mode, size)
    Ho, Wo = size or hw
    assert out.shape == (2 * N, Ho, Wo, 16) and out.dtype == BF16
    assert torch.equal(out, ops.perc_stage(rd, td, mode, size))
    o = out.cpu().double()
    ref, bound = PB.stage(recon, target, mode, size), PB.stage_bound(recon, target, mode, size)
    err = (o[..., :8] + o[..., 8:] - ref).abs()
    print(f"stage max err/bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert (err <= bound).all()
    assert (o[..., 3:8] == 0).all() and (o[..., 11:] == 0).all()
    g = torch.Generator().manual_seed(4)
    gb = (torch.randn(N, Ho, Wo, 8, generator=g) * 0.5).to(BF16)
    dx = ops.perc_stage_bwd(gb.to(DEV), rd, mode)
    assert dx.shape == recon.shape and dx.dtype == F32
    assert torch.equal(dx, ops.perc_stage_bwd(gb.to(DEV), rd, mode))
    rb, bb = PB.stage_bwd(gb, recon, mode), PB.stage_bwd_bound(gb, recon, mode)
    eb = (dx.cpu().double() - rb).abs()
    print(f"stage_bwd max err/bound {float((eb / bb.clamp_min(1e-300)).max()):.3f}")
    assert (eb <= bb).all()
    if mode == "clamp":
        flat, gx = recon.view(-1), dx.cpu().view(-1)
        assert (gx[(flat < -1) | (flat > 1)] == 0).all()
        assert flat[0] == -1 and flat[1] == 1     # the boundary passes the gradient, as torch.clamp


TAP_SHAPES = [(8, 8), (24, 24), (64, 64), (24, 20)]
TAP_GRID = [(Cp, C, hw, pool, below) for Cp, C in TAP_SHAPES for hw in ((20, 12), (5, 3), (2, 2), (1, 1))
            for pool in (False, True) for below in (False, True)
            if (not pool or min(hw) >= 2) and (Cp in (8, 24) and C != 20 or hw in ((20, 12), (5, 3)))]


@pytest.mark.parametrize("Cp,C,hw,pool,below", TAP_GRID)
def test_tap_forward_and_backward_inside_bounds(Cp, C, hw, pool, below):
    ops = _ops()
    H, W = hw
    N, wgt, gl = 2, 0.5, 0.75
    y = PB.lattice_y(N, H, W, Cp, C, 7)
    yd = y.to(DEV)
    value, sgn, out = PB.tap_fwd(y, C, pool)
    nan = float("nan")
    obuf = torch.full((2 * N, *out.shape[1:3], 2 * Cp), nan, device=DEV, dtype=BF16)
    sbuf = torch.full((N, H, W, Cp), 77, device=DEV, dtype=torch.int8)
    loss = torch.full((), 2.0, device=DEV)
    o, s, v = ops.perc_tap_fwd(yd, C, pool=pool, weight=wgt, loss=loss, first=False, out=obuf, sgn=sbuf)
    o2, s2, v2 = ops.perc_tap_fwd(yd, C, pool=pool, weight=wgt)
    assert torch.equal(o, o2) and torch.equal(s, s2) and torch.equal(v, v2)
    assert abs(float(v) - float(value)) <= PB.tap_value_bound(y, C, value)
    assert abs(float(loss) - (2.0 + wgt * float(value))) <= (3 * PB.U * (2.0 + wgt * float(value)) +
                                                             wgt * PB.tap_value_bound(y, C, value))
    assert torch.equal(s.cpu(), sgn)
    oc = o.cpu().double()
    assert not torch.isnan(oc).any()
    assert ((oc[..., :Cp] + oc[..., Cp:] - out).abs() <= PB.tap_out_bound(out)).all()
    # without an operand and without saving: the value alone, the same bits
    o3, s3, v3 = ops.perc_tap_fwd(yd, C, pool=pool, want_out=False, save=False)
    assert o3 is None and s3 is None and torch.equal(v3, v)

    g = torch.Generator().manual_seed(8)
    gb = None
    if below:
        gb = (torch.randn((N, H // 2, W // 2, Cp) if pool else (N, H, W, Cp), generator=g) * 0.01).to(BF16)
    ref, parts = PB.tap_bwd(y[:N], sgn, C, gl, wgt, gb, pool and below)
    buf = torch.full((2 * N, H, W, Cp), nan, device=DEV, dtype=BF16)
    gld = torch.tensor([gl], device=DEV)
    dy = ops.perc_tap_bwd(yd[:N].contiguous(), s, C, gld, weight=wgt, g_below=None if gb is None else gb.to(DEV),
                          pool=pool and below, out=buf[:N])
    dy2 = ops.perc_tap_bwd(yd[:N].contiguous(), s, C, gld, weight=wgt, g_below=None if gb is None else gb.to(DEV),
                           pool=pool and below)
    assert torch.equal(dy, dy2)
    assert torch.isnan(buf[N:]).all()              # the target half is untouched
    d = buf[:N].cpu().double()
    assert not torch.isnan(d).any()
    assert ((d - ref[:N]).abs() <= PB.tap_bwd_bound(ref, parts)).all()
    if pool and below and C == Cp == 8 and hw == (20, 12):
        # the planted ties: [[1, 1], [1, 1]] routes to element 0, [[0, 2], [2, 2]] to element 1
        l1 = gl * wgt / (N * C * H * W)
        for ch, first in ((0, (0, 0)), (1, (0, 1))):
            for pos in ((0, 0), (0, 1), (1, 0), (1, 1)):
                alive = float(y[0, pos[0], pos[1], ch]) > 0
                want = (l1 * float(sgn[0, pos[0], pos[1], ch]) + (float(gb[0, 0, 0, ch]) if pos == first else 0.0)) * alive
                assert abs(float(d[0, pos[0], pos[1], ch]) - want) <= 2.0 ** -8 * abs(want) + 1e-12, (ch, pos)


def test_bad_arguments_are_refused_and_launch_nothing():
    from fmdiff import _lib
    ops = _ops()
    L = _lib.lib()
    st = ops.stream()
    x = torch.rand(2, 1, 8, 8, device=DEV)
    out = torch.full((4, 8, 8, 16), 7.0, device=DEV, dtype=BF16)
    p = lambda t: t.data_ptr()   # noqa: E731
    assert L.fmd_perc_stage(p(x), p(x), 2, 2, 8, 8, 8, 8, 0, p(out), st) < 0          # 2 channels
    assert L.fmd_perc_stage(p(x), p(x), 0, 1, 8, 8, 8, 8, 0, p(out), st) < 0          # empty batch
    assert L.fmd_perc_stage(p(x), p(x), 2, 1, 8, 8, 0, 8, 0, p(out), st) < 0          # empty output
    assert L.fmd_perc_stage(p(x), p(x), 2, 1, 8, 8, 8, 8, 3, p(out), st) < 0          # unknown map
    assert L.fmd_perc_stage(p(x), None, 2, 1, 8, 8, 8, 8, 0, p(out), st) < 0          # no target
    assert L.fmd_perc_stage(p(x), p(x), 2, 1, 8, 8, 8, 8, 0, p(out) + 2, st) < 0      # misaligned
    dx = torch.full((2, 1, 8, 8), 7.0, device=DEV)
    g = torch.zeros(2, 8, 8, 8, device=DEV, dtype=BF16)
    assert L.fmd_perc_stage_bwd(p(g), p(x), 2, 1, 8, 8, 8, 8, 12, 0, p(dx), st) < 0   # Cp not a multiple of 8
    assert L.fmd_perc_stage_bwd(p(g) + 2, p(x), 2, 1, 8, 8, 8, 8, 8, 0, p(dx), st) < 0
    assert L.fmd_perc_stage_bwd(p(g), None, 2, 1, 8, 8, 8, 8, 8, 1, p(dx), st) < 0    # a map needs the raw recon
    y = torch.zeros(4, 4, 4, 8, device=DEV)
    ws = torch.zeros(64, device=DEV, dtype=torch.uint8)
    val = torch.full((), 7.0, device=DEV)
    tout = torch.full((4, 4, 4, 16), 7.0, device=DEV, dtype=BF16)
    assert L.fmd_perc_tap_workspace(2, 4, 4, 12) < 0
    assert L.fmd_perc_tap_fwd(p(y), 2, 4, 4, 12, 8, 0, p(tout), None, p(ws), 1.0, 1, p(val), None, st) < 0
    assert L.fmd_perc_tap_fwd(p(y), 2, 4, 4, 8, 9, 0, p(tout), None, p(ws), 1.0, 1, p(val), None, st) < 0    # C > Cp
    assert L.fmd_perc_tap_fwd(p(y), 2, 0, 4, 8, 8, 0, p(tout), None, p(ws), 1.0, 1, p(val), None, st) < 0    # empty
    assert L.fmd_perc_tap_fwd(p(y), 2, 1, 4, 8, 8, 1, p(tout), None, p(ws), 1.0, 1, p(val), None, st) < 0    # empty pool
    assert L.fmd_perc_tap_fwd(p(y) + 4, 2, 4, 4, 8, 8, 0, p(tout), None, p(ws), 1.0, 1, p(val), None, st) < 0
    assert L.fmd_perc_tap_fwd(p(y), 2, 4, 4, 8, 8, 0, p(tout), None, None, 1.0, 1, p(val), None, st) < 0     # no ws
    sg = torch.zeros(2, 4, 4, 8, device=DEV, dtype=torch.int8)
    dy = torch.full((2, 4, 4, 8), 7.0, device=DEV, dtype=BF16)
    gl = torch.ones(1, device=DEV)
    assert L.fmd_perc_tap_bwd(p(y), p(sg), 2, 4, 4, 12, 8, 0, None, p(gl), 1.0, p(dy), st) < 0
    assert L.fmd_perc_tap_bwd(p(y), None, 2, 4, 4, 8, 8, 0, None, p(gl), 1.0, p(dy), st) < 0
    assert L.fmd_perc_tap_bwd(p(y), p(sg), 2, 4, 4, 8, 8, 0, None, None, 1.0, p(dy), st) < 0
    assert L.fmd_perc_tap_bwd(p(y), p(sg), 2, 4, 4, 8, 8, 0, None, p(gl), 1.0, p(dy) + 2, st) < 0
    torch.cuda.synchronize()
    for t in (out, dx, val, tout, dy):
        assert (t.float() == 7.0).all()
    with pytest.raises(RuntimeError):
        ops.perc_stage(x.cpu(), x.cpu())
    with pytest.raises(RuntimeError):
        ops.perc_tap_fwd(y.cpu(), 8)
    with pytest.raises(ValueError):
        ops.perc_stage(torch.rand(2, 2, 8, 8, device=DEV), torch.rand(2, 2, 8, 8, device=DEV))
