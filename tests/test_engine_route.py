"""CPU test of ``fmdiff.runtime.engine.route3x3``: the one place the engine decides which kernel a 3x3 (3x3x3)
pad-1 conv runs on.

The specification is a frozen copy of the decisions the engine made before the route existed, site by site, as
plain boolean expressions over ``ops.halo_eligible`` / ``ops.s2d_eligible`` / ``ops.d2s_eligible`` (the ``_site_*``
functions below; they never call the route).  The sites were:

* ``conv_layer`` forward: the halo kernel (2-D, and 3-D depth taps, nearest-x2 included) or the space-to-depth
  kernel for a stride-2 conv;
* ``_halo_ok``: ResBlock conv1 / conv2, with the fused GroupNorm prologue (``pro``) and again without it once the
  operand is materialised; ``dgrad3x3`` at stride 1 is the same question with ``pro`` off (the gather reads dy);
* ``dgrad3x3`` at stride 2: the depth-to-space kernel, its gradient grid being the forward conv's output grid;
* ``conv_layer`` backward of a conv on a nearest-x2 input: the 4x4 (4x4x4) stride-2 gather from the upsampled
  grid, which the route answers as a ``ks=4`` query on that grid.

Every point of the sweep is checked against each site whose arguments it can be; a combination no site ever
asked (a prologue on a strided conv, ``transposed`` at stride 1, ...) only has to answer with a known route."""
import itertools

import pytest

from fmdiff.runtime import engine as E
from fmdiff.runtime import ops

NS = (1, 2, 8)
GRIDS = tuple((s, s) for s in (8, 16, 32, 64, 128)) + ((32, 64),)
DEPTHS = (0, 8, 16)
CHANNELS = (32, 64, 128, 256)
BOOLS = (False, True)


# ------------------------------------------------------------------ the frozen copy (parent of this change)
def _site_conv_layer_forward(N_, sp, out_channels, Cin, stride, upsample, weight_cin_is_Cin):
    Ho_ = ops.out_hw(sp[0], 3, stride, 1, upsample)
    if len(sp) == 2:
        halo = stride == 1 and ops.halo_eligible(N_, sp[0], Ho_, ops.out_hw(sp[1], 3, stride, 1, upsample),
                                                 out_channels, upsample=upsample, Cin=Cin)
    else:
        Do_ = 2 * sp[0] if upsample else sp[0]
        halo = E.DEPTH_HALO and stride == 1 and ops.halo_eligible(
            N_ * Do_, sp[1], ops.out_hw(sp[1], 3, 1, 1, upsample), ops.out_hw(sp[2], 3, 1, 1, upsample),
            out_channels, upsample=upsample, Cin=Cin, ztaps=3)
    s2d = E.S2D_HALO and stride == 2 and weight_cin_is_Cin and (
        ops.s2d_eligible(N_, sp[0], sp[1], sp[0] // 2, sp[1] // 2, out_channels, Cin, 3) if len(sp) == 2
        else E.S2D_3D and ops.s2d_eligible(N_, sp[1], sp[2], sp[1] // 2, sp[2] // 2, out_channels, Cin, 3,
                                           sp[0], sp[0] // 2))
    return "s2d" if s2d else "halo" if halo else "igemm"


def _site_halo_ok(N, sp, K, Cin, pro=False):
    if len(sp) == 2:
        return bool(ops.halo_eligible(N, sp[0], sp[0], sp[1], K, Cin=Cin, pro=pro))
    D, H, W = sp
    return bool(E.DEPTH_HALO and ops.halo_eligible(N * D, H, H, W, K, Cin=Cin, pro=pro, ztaps=3))


def _site_dgrad_stride2(N, sp, Cin, dyC, Kpad_is_None, weight_cin_is_Cin, pro, w_dim):
    dy_sp = tuple(ops.out_hw(v, 3, 2, 1, False) for v in sp)   # dy is the stride-2 forward's output
    dy_shape = (N, *dy_sp, dyC)
    return bool(E.S2D_HALO and Kpad_is_None and weight_cin_is_Cin and not pro and (
        ops.d2s_eligible(dy_shape[0], dy_shape[1], dy_shape[2], sp[0], sp[1], Cin, dy_shape[-1])
        if len(sp) == 2 and w_dim == 4 else
        E.S2D_3D and len(sp) == 3 and w_dim == 5 and ops.d2s_eligible(dy_shape[0], dy_shape[2], dy_shape[3], sp[1],
                                                                    sp[2], Cin, dy_shape[-1], dy_shape[1], sp[0])))


def _site_nearest_x2_dgrad(N_, sp, Cin, dyC, weight_cin_is_Cin, dyC_is_weight_K):
    """``sp`` is the conv's input grid before the nearest-x2 copy, as in conv_layer."""
    if len(sp) == 2:
        return bool(E.S2D_HALO and weight_cin_is_Cin and dyC_is_weight_K and ops.s2d_eligible(
            N_, 2 * sp[0], 2 * sp[1], sp[0], sp[1], Cin, dyC, 4))
    return bool(E.S2D_3D and weight_cin_is_Cin and dyC_is_weight_K and ops.s2d_eligible(
        N_, 2 * sp[1], 2 * sp[2], sp[1], sp[2], Cin, dyC, 4, 2 * sp[0], sp[0]))


# ------------------------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("depth_halo,s2d_halo,s2d_3d", list(itertools.product(BOOLS, repeat=3)))
def test_route_equals_the_frozen_decisions(monkeypatch, depth_halo, s2d_halo, s2d_3d):
    monkeypatch.setattr(E, "DEPTH_HALO", depth_halo)
    monkeypatch.setattr(E, "S2D_HALO", s2d_halo)
    monkeypatch.setattr(E, "S2D_3D", s2d_3d)
    seen = {"halo": 0, "s2d": 0, "d2s": 0, "igemm": 0}
    checked = 0
    for N, hw, D, Cin, K, stride in itertools.product(NS, GRIDS, DEPTHS, CHANNELS, CHANNELS, (1, 2)):
        sp = (D, *hw) if D else hw
        for upsample, transposed, pro, exact in itertools.product(BOOLS, repeat=4):
            r = E.route3x3(N, sp, K, Cin, stride=stride, upsample=upsample, transposed=transposed, pro=pro,
                           exact_weight=exact)
            assert r in seen
            seen[r] += 1
            where = (N, sp, K, Cin, stride, upsample, transposed, pro, exact)
            if not transposed and not pro:        # conv_layer forward
                assert r == _site_conv_layer_forward(N, sp, K, Cin, stride, upsample, exact), where
                checked += 1
            if stride == 1 and not upsample and not transposed:
                # ResBlock convs (with / without the prologue); pro off: also dgrad3x3 at stride 1, which never
                # looked at the weight's padding (exact)
                assert (r == "halo") == _site_halo_ok(N, sp, K, Cin, pro=pro), where
                assert r in ("halo", "igemm"), where
                checked += 1
            if stride == 2 and transposed and not upsample:   # dgrad3x3 at stride 2: K = Cin of the forward conv
                for kpad_none, wcin, wdim in itertools.product(BOOLS, BOOLS, (4, 5)):
                    ex = kpad_none and wcin and wdim == len(sp) + 2   # how dgrad3x3 folds them into exact_weight
                    if ex == exact:
                        assert (r == "d2s") == _site_dgrad_stride2(N, sp, K, Cin, kpad_none, wcin, pro, wdim), where
                assert r in ("d2s", "igemm"), where
                checked += 1
        # the nearest-x2 data gradient: a ks=4 query on the upsampled grid sp (every swept size is even)
        if stride == 2:
            lo = tuple(v // 2 for v in sp)
            assert tuple(2 * v for v in lo) == sp
            for wcin, dyk in itertools.product(BOOLS, repeat=2):
                r = E.route3x3(N, sp, K, Cin, stride=2, ks=4, exact_weight=wcin and dyk)
                assert r in ("s2d", "igemm")
                assert (r == "s2d") == _site_nearest_x2_dgrad(N, lo, K, Cin, wcin, dyk), (N, sp, K, Cin, wcin, dyk)
                seen[r] += 1
                checked += 1
    # 864 grids x channels per stride; 4 + 4 site questions at stride 1, 4 + 4 + 4 at stride 2
    assert checked == 864 * 8 + 864 * 12
    # the sweep reaches every route its switches allow (3-D depth taps need DEPTH_HALO only for the 3-D grids)
    assert seen["halo"] and seen["igemm"]
    assert bool(seen["s2d"]) == (s2d_halo or s2d_3d)
    assert bool(seen["d2s"]) == s2d_halo


def test_route_reads_the_switches_at_call_time(monkeypatch):
    """The engine's callers monkeypatch the module switches; the route must see the change."""
    q3 = dict(N=2, sp=(16, 32, 32), K=128, Cin=128)
    monkeypatch.setattr(E, "DEPTH_HALO", True)
    assert E.route3x3(**q3) == "halo"
    monkeypatch.setattr(E, "DEPTH_HALO", False)
    assert E.route3x3(**q3) == "igemm"
    q2 = dict(N=8, sp=(128, 128), K=128, Cin=128, stride=2)
    monkeypatch.setattr(E, "S2D_HALO", True)
    assert E.route3x3(**q2) == "s2d"
    assert E.route3x3(**q2, transposed=True) == "d2s"
    assert E.route3x3(**q2, exact_weight=False) == "igemm"
    monkeypatch.setattr(E, "S2D_HALO", False)
    assert E.route3x3(**q2) == "igemm"
    assert E.route3x3(**q2, transposed=True) == "igemm"


def test_vae_engine_is_a_layer_engine_only():
    from fmdiff.runtime.vae_engine import VAEEngine
    assert issubclass(VAEEngine, E.LayerEngine) and not issubclass(VAEEngine, E.UNetEngine)
    assert issubclass(E.UNetEngine, E.LayerEngine)
    for name in ("forward", "backward", "time_mlp", "set_time_table", "seg_ranges", "backward_param_groups"):
        assert not hasattr(VAEEngine, name), name
