"""Exact-lattice checks of the convolution family ("Convolutions: exact lattice").

Every operand is drawn from a coarse dyadic lattice (x in multiples of 1/4, w in multiples of 1/8, ...), so every
product and every partial sum -- in any order, under any split -- is a multiple of ``step`` below 2^24 * step and
therefore exact in fp32.  The value a kernel holds before its final store then equals the fp64 reference exactly:
a bf16 output must be the round-to-nearest-even of the reference bit for bit, an fp32 output (out_f32, dW, db) the
reference itself.  The reference is fp64 torch (F.conv2d / F.conv3d / conv_transpose / autograd) of the whole op as
``ops.conv`` / ``ops.wgrad`` define it, never another kernel.

This module imports without a GPU: the case table, the seeded generators, the reference, the conditions under which
the argument holds (``conditions``: asserted by the CPU and the GPU tests before anything is compared), the bit
comparison (``assert_bits``), the statistics-row maps, and a plain-torch fp32 emulation with mutants that the CPU
test feeds through the same comparison.  Its last part holds what no lattice can carry -- the SiLU prologue and the
SiLU' epilogue -- to elementwise error bounds on real-valued inputs (BOUND_CASES; derivation there).
"""
from __future__ import annotations

import functools
import types
import zlib

import torch
import torch.nn.functional as F

BF16 = torch.bfloat16

# value lattices: (lowest numerator, highest numerator, denominator)
LATTICES = {
    "fine": dict(x=(-4, 8, 4), w=(-4, 4, 8)),      # x in [-1, 2] step 1/4, w in [-1/2, 1/2] step 1/8
    "coarse": dict(x=(-2, 4, 2), w=(-2, 2, 4)),    # the statistics cases: x step 1/2, w step 1/4
    "coarse_w": dict(x=(-2, 4, 2), w=(-1, 1, 4)),  # statistics behind a prologue (z step 1/4) or a wide reduction
    "int": dict(x=(-3, 12, 1), w=(-4, 4, 8)),      # narrow reductions (C = 8): integer x so that outputs still round
}
PRO_A = (0.5, 1.0, 2.0, -1.0)


# ------------------------------------------------------------------------------------------------------ the cases
def case(name, op, inst, **kw):
    """One row of the table.  ``sp``: stored spatial dims of src0 ((H, W) or (D, H, W)); ``mode``: "fwd", "dgrad"
    (transposed gather: src0 is dY, ``w`` the forward master [C0][K][k..]) or "updgrad" (ks 4: the data gradient of
    conv3x3(nearest_x2)); ``out_sp``: output dims where the op needs them; ``plan``: the (kernel, bco, bpx, tile_rows,
    tickets, combine_launch, stats_rows, fold) fmd_conv_plan must answer; ``epx``: (C0e, C1e) channels of a one- or
    two-source data-gradient epilogue tensor without the SiLU' factor (the statistics' second sum is then sum v x);
    ``splits``: the split count handed to ops.conv (implicit GEMM), ``hsplits``: the one ops.halo_splits must choose
    for a halo row -- both asserted, since the uneven K-step tails the rows name depend on them."""
    d = dict(name=name, op=op, inst=inst, N=3, sp=(5, 7), C0=8, C1=0, K=8, ks=3, stride=1, pad=None, up=False,
             mode="fwd", out_sp=None, pro=False, seg2=None, bias=False, bias2=False, bias_nc=False, resid=False,
             out_f32=False, acc=False, stats=False, splits=1, generic=False, ticket=False, th8=None, th4=None,
             gout=False, lattice="fine", plan=None, smode=None, split=None, dy_wide=0, halo=None,
             tile_rows=None, epx=None, silu=False, epsilu=None, hsplits=1, fold=None)
    assert set(kw) <= set(d), set(kw) - set(d)
    d.update(kw)
    if d["pad"] is None:
        d["pad"] = 1 if d["ks"] in (3, 4) else 0
    c = types.SimpleNamespace(**d)
    c.nd = len(c.sp)
    if c.out_sp is None:
        mul = 2 if c.up else 1
        c.out_sp = tuple((h * mul + 2 * c.pad - c.ks) // c.stride + 1 for h in c.sp)
    return c


IG, H8, H9 = 1, 2, 3   # fmd_conv_plan_t.kernel

CONV_CASES = [
    # ---- implicit GEMM: instances, pack, ragged and two-image pixel tiles, channel seams
    case("ig_k16_pack", "conv", "IG_K16", N=3, sp=(5, 7), C0=8, K=8, bias=True, lattice="int",
         plan=(IG, 16, 256, 0, 0, 0, 0, 0)),
    case("ig_k16_c24_1x1", "conv", "IG_K16", N=5, sp=(6, 10), C0=24, K=16, ks=1, bias=True,
         plan=(IG, 16, 256, 0, 0, 0, 0, 0)),
    case("ig_k64_k24_c24", "conv", "IG_K64", N=3, sp=(5, 7), C0=24, K=24, bias=True,
         plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    case("ig_k64_seam_40_24", "conv", "IG_K64", N=3, sp=(5, 7), C0=40, C1=24, K=64,
         plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    case("ig_px128_k72_c72", "conv", "IG_PX128", N=3, sp=(5, 7), C0=72, K=72, bias=True, splits=1,
         plan=(IG, 128, 128, 0, 0, 0, 0, 0)),
    case("ig_px128_k136_all_epilogues", "conv", "IG_PX128", N=3, sp=(6, 10), C0=40, C1=24, K=136, bias=True,
         bias2=True, bias_nc=True, resid=True, seg2=(40, 24), splits=1, plan=(IG, 128, 128, 0, 0, 0, 0, 0)),
    case("ig_px128_pack_k72", "conv", "IG_PX128", N=3, sp=(5, 7), C0=8, K=72, lattice="int", splits=1,
         plan=(IG, 128, 128, 0, 0, 0, 0, 0)),
    case("ig_s2_odd", "conv", "IG_K64", N=3, sp=(7, 9), C0=24, K=24, stride=2, bias=True,
         plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    case("ig_up_pro", "conv", "IG_K64", N=3, sp=(3, 5), C0=40, C1=24, K=64, up=True, pro=True, bias=True,
         plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    case("ig_out_f32", "conv", "IG_K64", N=3, sp=(5, 7), C0=72, K=24, out_f32=True, bias=True,
         plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    case("ig_acc_bf16", "conv", "IG_K64", N=3, sp=(5, 7), C0=72, K=24, acc=True,
         plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    case("ig_acc_f32", "conv", "IG_PX128", N=3, sp=(5, 7), C0=24, K=72, acc=True, out_f32=True, splits=1,
         plan=(IG, 128, 128, 0, 0, 0, 0, 0)),
    case("ig_stats_k64", "conv", "IG_K64", N=3, sp=(8, 16), C0=24, K=64, bias=True, stats=True, lattice="coarse",
         plan=(IG, 64, 128, 0, 0, 0, 64, 0)),
    case("ig_stats_epx_two_source", "conv", "IG_K64", N=3, sp=(8, 16), C0=24, K=64, stats=True, epx=(40, 24),
         lattice="coarse", plan=(IG, 64, 128, 0, 0, 0, 64, 0)),
    # ---- transposed gathers
    case("ig_t_s1", "conv", "IG_K64", N=3, sp=(5, 7), C0=72, K=24, mode="dgrad", out_sp=(5, 7),
         plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    case("ig_t_1x1", "conv", "IG_PX128", N=3, sp=(5, 7), C0=24, K=72, ks=1, mode="dgrad", out_sp=(5, 7), splits=1,
         plan=(IG, 128, 128, 0, 0, 0, 0, 0)),
    case("ig_t_s2_parity", "conv", "IG_K64", N=3, sp=(4, 6), C0=72, K=24, stride=2, mode="dgrad", out_sp=(8, 12),
         plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    case("ig_t_s2_parity_stats", "conv", "IG_K64", N=3, sp=(8, 16), C0=24, K=24, stride=2, mode="dgrad",
         out_sp=(16, 32), stats=True, lattice="coarse", splits=1, plan=(IG, 64, 128, 0, 0, 0, 64, 0)),
    case("ig_t_s2_odd", "conv", "IG_K64", N=3, sp=(4, 5), C0=72, K=24, stride=2, mode="dgrad", out_sp=(7, 9),
         plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    case("ig_updgrad", "conv", "IG_K64", N=3, sp=(6, 10), C0=72, K=24, ks=4, stride=2, mode="updgrad",
         out_sp=(3, 5), plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    # ---- split-K: parts that do not divide the K-steps, one leaving the last part a single step
    case("ig_px64_split_rows", "conv", "IG_PX64", N=3, sp=(8, 16), C0=136, K=136, bias=True, stats=True, splits=4,
         lattice="coarse", plan=(IG, 128, 64, 0, 0, 1, 16, 0)),     # 27 K-steps in 4 parts of 7: the last has 6
    case("ig_px64_split_rows_epx", "conv", "IG_PX64", N=3, sp=(8, 16), C0=72, K=136, stats=True, splits=5,
         epx=(96, 40), lattice="coarse", plan=(IG, 128, 64, 0, 0, 1, 16, 0)),
    case("ig_px64_split_reduce", "conv", "IG_PX64", N=3, sp=(7, 9), C0=72, K=72, bias=True, bias_nc=True, resid=True,
         splits=5, plan=(IG, 128, 64, 0, 0, 1, 0, 0)),              # 18 K-steps in 5 parts of 4: the last has 2
    case("ig_px32_split", "conv", "IG_PX32", N=3, sp=(3, 5), C0=72, K=136, bias=True, splits=5,
         plan=(IG, 128, 32, 0, 0, 1, 0, 0)),                        # 18 in 5 parts of 4: the last has 2
    case("ig_px128_split_rows", "conv", "IG_PX128", N=5, sp=(16, 28), C0=136, K=72, splits=4, bias=True,
         plan=(IG, 128, 128, 0, 0, 1, 0, 0)),                       # M = 2240 > 2048: 27 in 4 parts of 7
    case("ig_k64_split_c200", "conv", "IG_K64", N=3, sp=(5, 7), C0=200, K=24, splits=5, bias=True,
         plan=(IG, 64, 128, 0, 0, 1, 0, 0)),                        # 36 steps in 5 parts of 8: the last has 4
    case("ig_k16_split_empty_parts", "conv", "IG_K16", N=3, sp=(5, 7), C0=136, K=16, splits=13,
         plan=(IG, 16, 256, 0, 0, 1, 0, 0)),                        # 27 steps in parts of 3: 9 used, 4 parts empty
    case("ig_k64_split_single_tail", "conv", "IG_K64", N=3, sp=(5, 7), C0=40, C1=24, K=64, splits=3, resid=True,
         plan=(IG, 64, 128, 0, 0, 1, 0, 0)),                        # 9 steps in parts of 4: the last is a single step
    case("ig_px64_ticket", "conv", "IG_PX64", N=3, sp=(8, 16), C0=72, K=128, bias=True, stats=True, splits=5,
         ticket=True, lattice="coarse", plan=(IG, 128, 64, 0, 1, 0, 32, 0)),
    case("ig_k64_ticket", "conv", "IG_K64", N=3, sp=(8, 16), C0=136, K=64, bias=True, resid=True, splits=4,
         ticket=True, plan=(IG, 64, 128, 0, 1, 0, 0, 0)),
    case("ig_seg2_split", "conv", "IG_PX32", N=3, sp=(5, 7), C0=72, K=72, seg2=(40, 24), bias=True, bias2=True,
         splits=4, plan=(IG, 128, 32, 0, 0, 1, 0, 0)),              # 18 + 1 steps in parts of 5: the last is 4
    # ---- 3-D at D != H != W
    case("ig_3d_s1_pack", "conv", "IG_K16", N=3, sp=(3, 5, 7), C0=8, K=16, bias=True, lattice="int",
         plan=(IG, 16, 256, 0, 0, 0, 0, 0)),
    case("ig_3d_s1", "conv", "IG_K64", N=3, sp=(3, 5, 7), C0=24, K=24, bias=True, splits=1,
         plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    case("ig_3d_s2", "conv", "IG_K64", N=3, sp=(5, 7, 9), C0=24, K=24, stride=2, splits=1,
         plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    case("ig_3d_up", "conv", "IG_K64", N=3, sp=(2, 3, 5), C0=24, K=24, up=True, splits=1,
         plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    case("ig_3d_t_s2_parity", "conv", "IG_K64", N=3, sp=(2, 3, 5), C0=24, K=24, stride=2, mode="dgrad",
         out_sp=(4, 6, 10), splits=1, plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    # ---- halo kernels: 32 x 48 images (2 x 3 tiles of 16 x 16), 6 images for >= 32 workgroups
    case("h9_r16_c32", "conv", "HALO9_16", N=6, sp=(32, 48), C0=32, K=128, bias=True, th8=0,
         plan=(H9, 0, 0, 16, 0, 0, 0, 0)),
    case("h9_r8_seam_resid", "conv", "HALO9_8", N=6, sp=(32, 48), C0=40, C1=24, K=128, bias=True, resid=True, th4=0,
         plan=(H9, 0, 0, 8, 0, 0, 0, 0)),
    case("h9_r4_c96_stats", "conv", "HALO9_4", N=6, sp=(32, 48), C0=96, K=128, bias=True, stats=True,
         lattice="coarse_w", plan=(H9, 0, 0, 4, 0, 0, 64, 0)),
    case("h9_r16_stats_pro", "conv", "HALO9_16", N=6, sp=(32, 48), C0=32, K=128, bias=True, pro=True, stats=True,
         th8=0, lattice="coarse_w", plan=(H9, 0, 0, 16, 0, 0, 64, 0)),
    case("h9_r8_stats_epx", "conv", "HALO9_8", N=6, sp=(32, 48), C0=32, K=128, stats=True, epx=(128, 0), th4=0,
         lattice="coarse_w", plan=(H9, 0, 0, 8, 0, 0, 64, 0)),
    case("h9_r8_up", "conv", "HALO9_8", N=6, sp=(16, 24), C0=32, K=128, up=True, bias=True, th4=0,
         plan=(H9, 0, 0, 8, 0, 0, 0, 0)),
    case("h9_r4_seg2", "conv", "HALO9_4", N=6, sp=(32, 48), C0=32, K=128, seg2=(40, 24), bias=True, bias2=True,
         plan=(H9, 0, 0, 4, 0, 0, 0, 0)),
    case("h9_split_combine", "conv", "HALO9_16", N=3, sp=(32, 48), C0=160, K=128, bias=True, bias_nc=True, th8=0,
         hsplits=2, plan=(H9, 0, 0, 16, 0, 1, 0, 0)),               # 5 chunks in 2 parts: 3 | 2
    case("h9_split_ticket_stats", "conv", "HALO9_4", N=3, sp=(32, 48), C0=224, K=128, bias=True, stats=True,
         lattice="coarse_w", hsplits=3, plan=(H9, 0, 0, 4, 1, 0, 64, 0)),   # 7 chunks in 3 parts: 3 | 3 | 1
    case("h9_split_ticket_r8", "conv", "HALO9_8", N=3, sp=(32, 48), C0=160, K=128, bias=True, resid=True, th4=0,
         hsplits=2, plan=(H9, 0, 0, 8, 1, 0, 0, 0)),
    case("h8_k192", "conv", "HALO8", N=3, sp=(32, 48), C0=32, K=192, bias=True, resid=True,
         plan=(H8, 0, 0, 0, 0, 0, 0, 0)),
    case("h8_gout_affine", "conv", "HALO8", N=6, sp=(32, 48), C0=40, C1=24, K=128, pro=True, gout=True, bias=True,
         plan=(H8, 0, 0, 0, 0, 0, 0, 0)),
    case("h9_3d_depth_split", "conv", "HALO9_8", N=3, sp=(3, 32, 48), C0=64, K=128, bias=True, hsplits=3,
         plan=(H9, 0, 0, 8, 0, 1, 0, 0)),                           # 9 slices x 2 x 3 tiles; 6 (kz, chunk) in 3 parts
]

S2D_CASES = [
    # 128 workgroups: N (x Do) x (Ho / 16) x (Wo / 16) x (K / 128), which is what sets N = 16 (2-D) here.
    # tile_rows: fmd_conv_s2d (csrc/conv_halo9.hip, "8-row tiles on a one-round grid") runs 8-row tiles while that
    # count is below the th8 threshold (1024); the statistics row map needs it and no plan query reports it
    case("s2d_down", "s2d", "S2D", N=16, sp=(64, 128), C0=32, K=128, stride=2, bias=True),
    case("s2d_down_pro_stats", "s2d", "S2D", N=16, sp=(128, 64), C0=32, K=128, stride=2, bias=True, pro=True,
         stats=True, lattice="coarse_w", tile_rows=8),
    case("s2d_updgrad", "s2d", "S2D", N=16, sp=(64, 128), C0=32, K=128, ks=4, stride=2, mode="updgrad",
         out_sp=(32, 64)),
    case("s2d_updgrad_acc", "s2d", "S2D", N=16, sp=(128, 64), C0=32, K=128, ks=4, stride=2, mode="updgrad",
         out_sp=(64, 32), acc=True),
    case("s2d_3d_down", "s2d", "S2D", N=4, sp=(8, 128, 64), C0=32, K=128, stride=2, bias=True),
    case("d2s_plain", "d2s", "D2S", N=16, sp=(32, 16), C0=128, K=128, stride=2, mode="dgrad", out_sp=(64, 32),
         lattice="int"),
    case("d2s_acc", "d2s", "D2S", N=16, sp=(16, 32), C0=32, K=128, stride=2, mode="dgrad", out_sp=(32, 64), acc=True),
    case("d2s_3d", "d2s", "D2S", N=2, sp=(4, 32, 16), C0=32, K=128, stride=2, mode="dgrad", out_sp=(8, 64, 32),
         lattice="int"),
]

SMALL_CASES = [
    case("small_s2_whole", "small", "SMALL", N=3, sp=(8, 16), C0=64, K=32, stride=2, smode="s2", bias=True,
         bias_nc=True, stats=True, split=1, lattice="coarse"),
    case("small_s2_tiles_plan", "small", "SMALL", N=3, sp=(32, 16), C0=96, C1=32, K=32, stride=2, smode="s2",
         bias=True, split=0),
    case("small_up_plan", "small", "SMALL", N=3, sp=(4, 8), C0=128, K=48, up=True, smode="up", bias=True,
         resid=True, split=0),
    case("small_up_unsplit", "small", "SMALL", N=5, sp=(8, 4), C0=64, K=16, up=True, smode="up", bias=True,
         stats=True, split=1, lattice="coarse"),
]

W = dict(op="wgrad")
WGRAD_CASES = [
    # generic kernel
    case("wg_1x1", inst="WG_GENERIC", N=3, sp=(5, 7), C0=72, K=24, ks=1, splits=3, halo=False, **W),
    case("wg_3x3_s1_k24", inst="WG_GENERIC", N=3, sp=(5, 7), C0=24, K=24, splits=1, halo=False, **W),
    case("wg_3x3_s2_odd", inst="WG_GENERIC", N=3, sp=(7, 9), C0=72, K=24, stride=2, splits=3, halo=False, **W),
    case("wg_up", inst="WG_GENERIC", N=3, sp=(3, 5), C0=72, K=24, up=True, splits=1, halo=False, **W),
    case("wg_merged_c8", inst="WG_GENERIC", N=3, sp=(5, 7), C0=8, K=72, pro=True, splits=3, halo=False, **W),
    case("wg_seam_40_24_pro_acc", inst="WG_GENERIC", N=3, sp=(6, 10), C0=40, C1=24, K=136, pro=True, acc=True,
         splits=37, halo=False, **W),
    case("wg_3d", inst="WG_GENERIC", N=3, sp=(3, 5, 7), C0=24, K=24, splits=3, halo=False, **W),
    case("wg_forced_generic", inst="WG_GENERIC", N=3, sp=(8, 16), C0=64, K=128, splits=37, generic=True, acc=True,
         halo=False, **W),
    # halo kernel
    case("wh_s1", inst="WG_HALO", N=3, sp=(8, 16), C0=64, K=128, splits=1, halo=True, **W),
    case("wh_s1_pro_acc", inst="WG_HALO", N=3, sp=(16, 32), C0=64, K=128, pro=True, acc=True, splits=3,
         halo=True, **W),
    case("wh_s1_37", inst="WG_HALO", N=3, sp=(16, 32), C0=64, K=128, splits=37, halo=True, **W),
    case("wh_up", inst="WG_HALO", N=3, sp=(4, 8), C0=64, K=128, up=True, splits=3, halo=True, **W),
    case("wh_s2d", inst="WG_HALO", N=3, sp=(16, 32), C0=64, K=128, stride=2, splits=3, halo=True, **W),
    case("wh_concat_wide_dy", inst="WG_HALO", N=3, sp=(8, 16), C0=40, C1=24, K=128, dy_wide=64, splits=3,
         halo=True, **W),
]

ALL_CASES = CONV_CASES + S2D_CASES + SMALL_CASES + WGRAD_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)


def group_cases():
    """Three raw-input halo weight gradients of one kernel instance (same ``shape.key``) with unequal splits."""
    return [(BY_NAME["wh_s1"], 1), (BY_NAME["wh_s1_37"], 3), (BY_NAME["wh_concat_wide_dy"], 37)]


# ---------------------------------------------------------------------------------------------------- generators
def _draw(g, shape, lat, dtype=BF16):
    """Lattice values n / den, n uniform in [lo, hi]; ``lat`` a float instead: white noise of that scale (the inputs
    of the tolerance tests this suite is measured against)."""
    if isinstance(lat, float):
        v = torch.randn(shape, generator=g) * lat
        return v.to(BF16).to(dtype)
    lo, hi, den = lat
    return (torch.randint(lo, hi + 1, shape, generator=g).double() / den).to(dtype)


def lattice_step(c):
    """The spacing every product (and so every partial sum and epilogue term) is a multiple of."""
    L = LATTICES[c.lattice]
    sx = 1.0 / L["x"][2]
    if c.pro:
        sx = min(sx / 2, 0.25)      # a in {1/2, 1, 2, -1}, b in multiples of 1/4
    return sx / L["w"][2] if c.op != "wgrad" else sx / L["x"][2]


@functools.lru_cache(maxsize=None)
def generate(name):
    """The seeded CPU operands of case ``name`` (seed: a hash of the name): bf16 activations, fp32 weight masters and
    vectors."""
    c = BY_NAME[name]
    return _operands(c, LATTICES[c.lattice], torch.Generator().manual_seed(zlib.crc32(name.encode())))


def white_noise(c, seed=1):
    """(case, operands): ``c`` on square images with white-noise operands scaled as tests/test_gpu_kernels.py scales
    them -- what the 1.5e-2 max|ref| assertion has been looking at."""
    d = {k: v for k, v in vars(c).items() if k not in ("nd", "name", "op", "inst")}
    d["sp"] = (c.sp[0],) * c.nd
    d["out_sp"] = None if c.mode == "fwd" else (c.out_sp[0],) * c.nd
    c2 = case(c.name, c.op, c.inst, **d)
    fan = (c.C0 + c.C1) * c.ks ** c.nd
    T = _operands(c2, dict(x=1.0, w=fan ** -0.5, v=0.1), torch.Generator().manual_seed(seed))
    if c.pro:
        T["pro_a"] = torch.rand(T["pro_a"].shape, generator=torch.Generator().manual_seed(seed + 1)) + 0.5
    return c2, T


def _operands(c, L, g):
    """Every operand of case ``c`` drawn with generator ``g`` from ``L``: a LATTICES entry, or float scales
    dict(x=, w=, v=) for white noise."""
    vec = L.get("v", (-8, 8, 4))       # fp32 vectors: multiples of 1/4
    pb = L.get("v", (-4, 4, 4))
    N, K, nd = c.N, c.K, c.nd
    T = {}
    T["x0"] = _draw(g, (N, *c.sp, c.C0), L["x"])
    if c.C1:
        T["x1"] = _draw(g, (N, *c.sp, c.C1), L["x"])
    Ct = c.C0 + c.C1
    if c.pro:
        T["pro_a"] = torch.tensor(PRO_A)[torch.randint(0, 4, (N, Ct), generator=g)]
        T["pro_b"] = _draw(g, (N, Ct), pb, torch.float32)
    if c.op == "wgrad":
        T["dy"] = _draw(g, (N, *c.out_sp, K), L["x"])
        if c.acc:
            T["dw0"] = _draw(g, (K, Ct, *(c.ks,) * nd), vec, torch.float32)
            T["db0"] = _draw(g, (K,), vec, torch.float32)
        return T
    wshape = (K, Ct) if c.mode == "fwd" else (Ct, K)
    T["w"] = _draw(g, (*wshape, *((3 if c.ks == 4 else c.ks),) * nd), L["w"], torch.float32)
    if c.seg2:
        T["x2"] = _draw(g, (N, *c.out_sp, c.seg2[0]), L["x"])
        if c.seg2[1]:
            T["x3"] = _draw(g, (N, *c.out_sp, c.seg2[1]), L["x"])
        T["w2"] = _draw(g, (K, sum(c.seg2), *(1,) * nd), L["w"], torch.float32)
    for k in ("bias", "bias2"):
        if getattr(c, k):
            T[k] = _draw(g, (K,), vec, torch.float32)
    if c.bias_nc:
        T["bias_nc"] = _draw(g, (N, K), vec, torch.float32)
    if c.resid:
        T["resid"] = _draw(g, (N, *c.out_sp, K), L["x"])
    if c.epx:
        T["ex0"] = _draw(g, (N, *c.out_sp, c.epx[0]), L["x"])
        if c.epx[1]:
            T["ex1"] = _draw(g, (N, *c.out_sp, c.epx[1]), L["x"])
    if c.acc:
        T["old"] = _draw(g, (N, *c.out_sp, K), L["x"], torch.float32 if c.out_f32 else BF16)
    return T


# ----------------------------------------------------------------------------------------------------- reference
def _cf(t):
    return t.double().movedim(-1, 1)


def _cl(t):
    return t.movedim(1, -1).contiguous()


def _bc(v, nd):
    return v.double().reshape(*v.shape, *(1,) * nd)


def prologue(c, T):
    """fp64 [N][C][sp]: the concatenated input after the affine prologue (what the MFMA operand must hold)."""
    x = _cf(torch.cat([T["x0"], T["x1"]], -1) if "x1" in T else T["x0"])
    if c.pro:
        x = _bc(T["pro_a"], c.nd) * x + _bc(T["pro_b"], c.nd)
    return x


def _ups(x):
    return F.interpolate(x, scale_factor=2, mode="nearest")


def reference(c, T, z=None):
    """fp64 result of the whole op in channels-last layout: {"out"} for convs, {"dw", "db"} for weight gradients.
    ``z`` (fp64 [N][C][sp]): the conv operand in place of the affine prologue's output."""
    nd = c.nd
    conv = F.conv2d if nd == 2 else F.conv3d
    convt = F.conv_transpose2d if nd == 2 else F.conv_transpose3d
    x = prologue(c, T) if z is None else z
    if c.op == "wgrad":
        w = torch.zeros(c.K, c.C0 + c.C1, *(c.ks,) * nd, dtype=torch.float64, requires_grad=True)
        b = torch.zeros(c.K, dtype=torch.float64, requires_grad=True)
        conv(_ups(x) if c.up else x, w, b, stride=c.stride, padding=c.pad).backward(_cf(T["dy"]))
        dw, db = w.grad, b.grad
        if c.acc:
            dw, db = dw + T["dw0"].double(), db + T["db0"].double()
        return dict(dw=dw, db=db)
    w = T["w"].double()
    if c.mode == "fwd":
        y = conv(_ups(x) if c.up else x, w, stride=c.stride, padding=c.pad)
    elif c.mode == "dgrad":
        opad = tuple(o - ((i - 1) * c.stride - 2 * c.pad + c.ks) for i, o in zip(c.sp, c.out_sp))
        y = convt(x, w, stride=c.stride, padding=c.pad, output_padding=opad)
    else:   # the data gradient of conv3x3(nearest_x2(z)) at z
        z = torch.zeros(c.N, c.K, *c.out_sp, dtype=torch.float64, requires_grad=True)
        conv(_ups(z), w, padding=1).backward(x)
        y = z.grad
    assert tuple(y.shape[2:]) == tuple(c.out_sp), (y.shape, c.out_sp)
    if c.seg2:
        x2 = _cf(torch.cat([T["x2"], T["x3"]], -1) if "x3" in T else T["x2"])
        y = y + conv(x2, T["w2"].double())
    for k in ("bias", "bias2"):
        if k in T:
            y = y + T[k].double().reshape(1, -1, *(1,) * nd)
    if "bias_nc" in T:
        y = y + _bc(T["bias_nc"], nd)
    y = _cl(y)
    if "resid" in T:
        y = y + T["resid"].double()
    if "old" in T:
        y = y + T["old"].double()
    return dict(out=y)


def ep_tensor(T):
    """The data-gradient epilogue tensor x (both sources concatenated), or None."""
    if "ex0" not in T:
        return None
    return torch.cat([T["ex0"], T["ex1"]], -1) if "ex1" in T else T["ex0"]


def expected(c, ref):
    """What the kernel must store: RNE to bf16 of the fp64 value, or the value itself for fp32 outputs."""
    return ref.float() if (c.out_f32 or c.op == "wgrad") else ref.to(BF16)


def fold_groups():
    """Taps of the 3-tap kernel that each tap of the folded 4-tap stride-2 kernel sums (csrc/conv_halo9.hip S(u))."""
    return [[2], [1, 2], [0, 1], [0]]


# ---------------------------------------------------------------------------------------------------- conditions
def _is_bf16(t):
    return torch.equal(t.double(), t.to(BF16).double())


def rounding_profile(ref):
    """(fraction of outputs whose bf16 store rounds, fraction that are exact ties) of an fp64 tensor that is exact
    in fp32."""
    f = ref.float()
    assert torch.equal(f.double(), ref)
    low = f.contiguous().view(torch.int32) & 0xFFFF
    return (low != 0).double().mean().item(), (low == 0x8000).double().mean().item()


def conditions(c, T, R):
    """Assert what the exactness argument needs of case ``c`` with operands ``T`` and fp64 reference ``R``; returns
    dict(round=, tie=) for bf16 outputs (the per-instance rounding condition is held by the CPU test)."""
    step = lattice_step(c)
    for k, v in T.items():
        if k == "pro_a":
            assert all(a in PRO_A for a in v.unique().tolist())
        elif v.dtype == torch.float32 and k not in ("w", "w2"):   # fp32 vectors and fp32 accumulation targets
            q = v.double() / step
            assert torch.equal(q, q.round()), f"{c.name}: {k} is off the lattice"
        else:                                                     # MFMA operands: bf16, or masters prep rounds
            assert _is_bf16(v), f"{c.name}: operand {k} does not survive a bf16 round trip"
    z = prologue(c, T)
    assert _is_bf16(z), f"{c.name}: the prologue result a*x+b is not a bf16 value"
    # the cap: with |operands| every partial sum of the real op is bounded by the same sum
    Ta = {k: v.abs() for k, v in T.items()}
    Ra = reference(c, Ta)
    for k, v in Ra.items():
        assert v.abs().max().item() < 2.0 ** 24 * step, f"{c.name}: {k} reaches {v.abs().max().item()} >= 2^24 step"
    for k, v in R.items():
        q = v / step
        assert torch.equal(q, q.round()), f"{c.name}: {k} leaves the lattice"
    if c.op == "wgrad":
        assert (R["dw"].flatten(1).abs().sum(1) > 0).all() and (R["db"] != 0).any()
        return dict(round=None, tie=None)
    w = T["w"]
    taps = w.flatten(2)                                  # [rows][cols][taps]
    red = taps if c.mode == "fwd" else taps.transpose(0, 1)   # reduction channels second
    Cr = red.shape[1]
    assert Cr % 8 == 0
    nz = red.reshape(red.shape[0], Cr // 8, 8, -1).abs().amax(dim=(0, 2))
    assert (nz > 0).all(), f"{c.name}: a (tap, 8-channel chunk) of the weights is all zero"
    if "w2" in T:
        w2 = T["w2"].flatten(1)
        assert (w2.reshape(c.K, -1, 8).abs().amax(dim=(0, 2)) > 0).all(), f"{c.name}: a zero chunk in the 1x1 segment"
    if c.mode == "updgrad":
        S = fold_groups()
        wf = w.double()
        for idx in torch.cartesian_prod(*[torch.arange(4)] * c.nd).tolist():
            sub = wf
            for d, u in enumerate(idx):
                sub = sub.index_select(2 + d, torch.tensor(S[u])).sum(2 + d, keepdim=True)
            assert _is_bf16(sub), f"{c.name}: a folded 4-tap weight is not a bf16 value"
    out = R["out"].reshape(-1, c.K)
    assert (out.abs().amax(1) > 0).all() and (out.abs().amax(0) > 0).all(), f"{c.name}: an all-zero output row"
    if c.stats:
        # a slab row holds at most 64 pixels of one image: the 64 largest v^2 of an (image, channel) bound any row
        e = expected(c, R["out"]).double().reshape(c.N, -1, c.K)
        y, sy = e, step
        if c.epx:
            y, sy = ep_tensor(T).double().reshape(c.N, -1, c.K), 1.0 / LATTICES[c.lattice]["x"][2]
        top = (e * y).abs().topk(min(64, e.shape[1]), dim=1).values.sum(1).max().item()
        assert top / (step * sy) < 2.0 ** 24, f"{c.name}: a row's second sum reaches {top}: statistics inexact"
    if c.out_f32:
        return dict(round=None, tie=None)
    r, t = rounding_profile(R["out"])
    return dict(round=r, tie=t)


# ---------------------------------------------------------------------------------------------------- comparison
def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def mismatches(got, exp):
    return (_bits(got) != _bits(exp)).nonzero()


def assert_bits(got, exp, ref, what):
    """``got`` equals ``exp`` bit for bit; the message names the count and the first indices that differ with got /
    expected / fp64 reference (the pattern usually names the bug)."""
    got, exp = got.detach().cpu(), exp.detach().cpu()
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = mismatches(got, exp)
    if bad.shape[0] == 0:
        return
    lines = [f"{what}: {bad.shape[0]} of {got.numel()} elements differ; first (index: got / expected / fp64 ref):"]
    for ix in bad[:8].tolist():
        ix = tuple(ix)
        lines.append(f"  {ix}: {got[ix].item()!r} / {exp[ix].item()!r} / {ref[ix].item()!r}")
    raise AssertionError("\n".join(lines))


SENTINEL = {BF16: 0x7FC1, torch.float32: 0x7FC00001}   # NaN payloads no kernel produces


def _sentinel(dtype):
    """The sentinel as the signed integer of the dtype's width."""
    s, bits = SENTINEL[dtype], 16 if dtype == BF16 else 32
    return s - (1 << bits) if s >= 1 << (bits - 1) else s


def guarded(shape, dtype, device, init=None):
    """(flat buffer, view of ``shape`` inside it): sentinel-filled, the view optionally set to ``init``, with a guard
    zone of one image's elements (at least 1024) on either side, so that a row or a tile written one image off
    still lands in it.  ``guards_intact`` tells whether anything was written outside the view."""
    n = 1
    for s in shape:
        n *= s
    guard = max(1024, -(-(n // shape[0]) // 8) * 8)
    it = torch.int16 if dtype == BF16 else torch.int32
    buf = torch.full((n + 2 * guard,), _sentinel(dtype), dtype=it, device=device).view(dtype)
    view = buf[guard:guard + n].view(shape)
    if init is not None:
        view.copy_(init)
    return buf, view


def guards_intact(buf, view):
    b = _bits(buf.cpu())
    guard = (buf.numel() - view.numel()) // 2
    s = _sentinel(buf.dtype)
    return bool((b[:guard] == s).all() and (b[guard + view.numel():] == s).all())


def unwritten(view):
    """Elements of a sentinel-filled view that still hold the sentinel."""
    return int((_bits(view.cpu()) == _sentinel(view.dtype)).sum().item())


# ------------------------------------------------------------------------------------------------ statistics rows
def stats_row_map(c, kind, rows, tile_rows=0):
    """Row of the statistics slab that each output pixel (flat, channels-last order) belongs to.

    kind "flat": consecutive ``rows`` pixels (implicit GEMM epilogue, ticketed epilogues, the combine launch's
    16-pixel rows, fmd_conv_small).  "parity": the implicit GEMM's parity classes -- rows stay image-major, class c
    the c-th HWq/rows of an image's rows, each holding that class's pixels in class-raster order (csrc/conv.hip, the
    comment above ``srow``).  "halo": 64-pixel rows = 4 tile rows x 16 columns of a ``tile_rows`` x 16 tile, tiles
    in (image, tile row, tile column) order (csrc/conv_halo9.hip epilogue)."""
    N, osp = c.N, c.out_sp
    M = N
    for s in osp:
        M *= s
    m = torch.arange(M)
    if kind == "flat":
        return m // rows
    if kind == "halo":
        Do = osp[0] if len(osp) == 3 else 1
        Ho, Wo = osp[-2:]
        img = m // (Ho * Wo)                       # (n, z) slices are images of the 2-D tiling
        assert img.max().item() == N * Do - 1 and rows == 64
        y, x = (m // Wo) % Ho, m % Wo
        tile = (img * (Ho // tile_rows) + y // tile_rows) * (Wo // 16) + x // 16
        return tile * (tile_rows // 4) + (y % tile_rows) // 4
    assert kind == "parity"
    HW = 1
    for s in osp:
        HW *= s
    n, r = m // HW, m % HW
    coords, cls, q = [], 0, 0
    for s in osp:                                    # most significant first: (z,) y, x
        HW //= s
        coords.append((r // HW) % s)
    for s, co in zip(osp, coords):
        cls = cls * 2 + (co & 1)
        q = q * (s // 2) + co // 2
    HWq = m.numel() // N // (1 << len(osp))
    rpi = HWq // rows
    return (n * (1 << len(osp)) + cls) * rpi + q // rows


def stats_expected(exp_out, rowmap, K, y=None):
    """fp64 [rows][K][2]: (sum v, sum v^2) -- or (sum v, sum v y) -- of the expected stored output over each row."""
    v = exp_out.double().reshape(-1, K)
    second = v * v if y is None else v * y.double().reshape(-1, K)
    nrows = int(rowmap.max().item()) + 1
    out = torch.zeros(nrows, K, 2, dtype=torch.float64)
    out[..., 0].index_add_(0, rowmap, v)
    out[..., 1].index_add_(0, rowmap, second)
    return out


# ------------------------------------------------------------------------------------- plain-torch emulation
MUTANTS = ["hw_swap", "pad_neighbour", "seam_chunk_dropped", "tap_transposed", "s2_odd_off_by_one", "up_ceil",
           "truncate", "bias_nc_image0", "last_split_dropped", "split_twice", "parity_wrong", "stats_row_shift"]


def _trunc_bf16(v):
    return (v.float().contiguous().view(torch.int32) & ~0xFFFF).view(torch.float32).to(BF16)


def emulate(c, T, mutant=None, splits=3, stats_rows=0, z=None, gmul=None):
    """fp32 emulation of a 2-D conv case (forward gather, or the stride-2 transposed gather by parity classes):
    explicit pixel decode and address arithmetic, 8-channel chunks and taps in reverse order dealt round-robin to
    ``splits`` partial slabs that are then summed last-first -- an order no kernel uses.  ``mutant``: one of MUTANTS
    (ignored where the case has nothing it applies to).  Returns (out, stats or None)."""
    assert c.nd == 2 and c.op in ("conv", "s2d", "small")
    N, K, (Ho, Wo), ks, s, pad = c.N, c.K, c.out_sp, c.ks, c.stride, c.pad
    z = _cl(prologue(c, T)).float() if z is None else z  # [N][Hs][Ws][C]; ``z``: the operand a caller computed
    Hs, Ws, C = z.shape[1:]
    M = N * Ho * Wo
    m = torch.arange(M)
    n, r = m // (Ho * Wo), m % (Ho * Wo)
    oy, ox = (r // Ho, r % Ho) if mutant == "hw_swap" else (r // Wo, r % Wo)
    zf = z.reshape(N * Hs * Ws, C)
    w = T["w"].float()
    slabs = torch.zeros(splits, M, K)
    chunks = [(ky, kx, c0) for ky in reversed(range(ks)) for kx in reversed(range(ks))
              for c0 in reversed(range(0, C, 8))]
    seam = (c.C0 // 8) * 8 if c.C1 else (C // 16) * 8
    for i, (ky, kx, c0) in enumerate(chunks):
        if mutant == "seam_chunk_dropped" and (ky, kx, c0) == (1, 0, seam):
            continue
        if c.mode == "fwd":
            iy, ix = oy * s - pad + ky, ox * s - pad + kx
            Hin, Win = (2 * Hs, 2 * Ws) if c.up else (Hs, Ws)
            hlim = Hin - 1 if (mutant == "s2_odd_off_by_one" and s == 2 and Hin % 2) else Hin
            ok = (iy >= 0) & (iy < hlim) & (ix >= 0) & (ix < Win)
            if mutant == "pad_neighbour":                # the column test forgotten: the flat address wraps a row
                ok = (iy >= 0) & (iy < hlim) & (iy * Win + ix >= 0) & (iy * Win + ix < Hin * Win)
            flat = iy * Win + ix
            iy, ix = flat.clamp(0, Hin * Win - 1) // Win, flat.clamp(0, Hin * Win - 1) % Win
            if c.up:
                iy, ix = ((iy + 1) // 2, (ix + 1) // 2) if mutant == "up_ceil" else (iy // 2, ix // 2)
                iy, ix = iy.clamp(max=Hs - 1), ix.clamp(max=Ws - 1)
            wy, wx = (kx, ky) if (mutant == "tap_transposed" and (ky, kx) == (0, 1)) else (ky, kx)
            wt = w[:, c0:c0 + 8, wy, wx]                 # [K][8]
        else:                                            # transposed gather: out[o] += dy[(o + pad - k) / s] w[:, :, k]
            ty, tx = oy + pad - ky, ox + pad - kx
            ok = (ty % s == 0) & (tx % s == 0) & (ty >= 0) & (tx >= 0) & (ty // s < Hs) & (tx // s < Ws)
            iy, ix = (ty // s).clamp(0, Hs - 1), (tx // s).clamp(0, Ws - 1)
            wt = w[c0:c0 + 8, :, ky, kx].t()             # [K][8]
        src = zf[(n * Hs + iy) * Ws + ix, c0:c0 + 8] * ok[:, None].float()
        slabs[i % splits] += src @ wt.t()
    if c.seg2:
        x2 = torch.cat([T["x2"], T["x3"]], -1) if "x3" in T else T["x2"]
        slabs[0] += x2.float().reshape(M, -1) @ T["w2"].float().reshape(K, -1).t()
    acc = torch.zeros(M, K)
    order = list(reversed(range(splits)))
    if mutant == "last_split_dropped":
        order = order[1:]
    if mutant == "split_twice":
        order = order + [0]
    for i in order:
        acc += slabs[i]
    if c.mode == "dgrad" and s == 2 and mutant == "parity_wrong" and Ho % 2 == 0 and Wo % 2 == 0:
        a4 = acc.reshape(N, Ho // 2, 2, Wo // 2, 2, K)
        acc = a4.transpose(2, 4).reshape(M, K)           # class (a, b) stored where class (b, a) belongs
    for k in ("bias", "bias2"):
        if k in T:
            acc += T[k]
    if "bias_nc" in T:
        acc += T["bias_nc"][torch.zeros_like(n) if mutant == "bias_nc_image0" else n]
    if "resid" in T:
        acc += T["resid"].float().reshape(M, K)
    if "old" in T:
        acc += T["old"].float().reshape(M, K)
    if gmul is not None:                                 # the data-gradient epilogue's factor, fp32 [M][K]
        acc = acc * gmul
    out = acc.reshape(N, Ho, Wo, K)
    out = out if c.out_f32 else (_trunc_bf16(out) if mutant == "truncate" else out.to(BF16))
    st = None
    if stats_rows:
        v = out.float().reshape(M // stats_rows, stats_rows, K)
        st = torch.stack([v.sum(1), (v * v).sum(1)], -1)
        if mutant == "stats_row_shift":
            st = st.roll(1, 0)
    return out, st


# ==================================================== what the lattice cannot carry: SiLU prologue, SiLU' epilogue
# pro = (a, b, True) and ep = (x, x1, a, b) round a transcendental, so these cases get real-valued inputs and an
# elementwise bound in the style of attn_bounds.py / gn_bounds.py.  With u = 2^-24, U = 2^-8 and z = a x + b:
#
#   sigmoidf_(z) = v_rcp_f32(1 + v_exp_f32(-z log2e))           (csrc/common.h)
#     the product z log2e and the constant are each rounded: the exponent moves by <= 2u |z| log2e, i.e. exp by a
#     factor 1 +- 2u|z|; v_exp_f32 is 1 ulp = 2u; the addition u; v_rcp_f32 1 ulp = 2u:
#       eta_s(z) = u (2|z| + 5)                                  relative error of the fp32 sigmoid
#   z itself is fl(fl(a x) + b) (or one fma): |dz| <= 2u (|a x| + |b|)
#   siluf_(z) = z * s: one more rounding, and |silu'| <= 1.1 carries dz:
#       eps_t = |t| (eta_s + u) + 2.2 u (|a x| + |b|)            absolute error of the fp32 t = SiLU(z)
#   silu_grad(z) = s * (1 + z * (1 - s)), g = silu'(z), roundings at the subtraction, the product, the addition, the
#   final product, and |g'| <= 0.5 carries dz:
#       eps_g = |g| (eta_s + 2u) + s^2 |z| eta_s + 2u s |z| (1 - s) + u (|a x| + |b|)
#
# Prologue.  The MFMA operand is bf16(t_fp32).  It equals z* = bf16(t_fp64) unless t_fp64 lies within eps_t of a
# rounding boundary; then it lies from bf16(t - eps_t) to bf16(t + eps_t) (the set F, where these differ by delta:
# one bf16 step, or several where a x + b cancels to a tiny t).  So
#       |out - ref| <= U |ref| + k u conv(|z*|, |w|) + conv(delta, |w|)
# with ref = conv(z*, w) + bias in fp64 and k the length of the longest fp32 addition chain: C taps + 8 (every
# product enters one accumulator chain -- MFMA steps, split partials, bias; the 8 covers the epilogue's additions).
# Weight gradients alike with k = N Ho Wo + 8 and the fp32 store's u |ref| in place of U |ref|.
# Epilogue.  out = bf16(v g_fp32) with v the fp32 conv sum:
#       |out - ref| <= U |ref| + |g| k u conv(|x|, |w|) + |v| eps_g + 2u |ref|
# In-kernel fold (pro_fold on the halo kernel, csrc/conv_halo9.hip): a, b come from the statistics slab inside the
# launch.  The reference folds THE SAME fp32 slab in fp64 (a = gamma / sqrt(var + eps), b = beta - mean a); the
# kernel's a, b differ from it by
#   channel totals: fp32 sums of the E slab rows of an image, any order: <= E u sum_rows|.|; over the group (fp64):
#       e_m = e_G1 / cnt,   e_v = e_G2 / cnt + 2 |m| e_G1 / cnt            (var = G2 / cnt - mean^2 in fp64)
#   rs = rsqrtf((float) var + eps): conversion, eps constant and addition 3u on v = var + eps, rsqrtf <= 2 ulp = 4u:
#       eta_r = e_v / (2 v) + 6u;   a = rs gamma: e_a = |a| (eta_r + u)
#   b = beta - (float) mean * a:    e_b = |m| e_a + |a| e_m + 2u |m a| + u |b|
# and eps_t gains 1.1 (e_a |x| + e_b).
# A case fails above MARGIN x its bound (1.5, as the two earlier bound suites); nothing here was tuned to the GPU.
U16, U32, MARGIN, TINY = 2.0 ** -8, 2.0 ** -24, 1.5, 1e-30

BOUND_CASES = [
    case("b_ig_pro", "conv", "conv_igemm", N=3, sp=(5, 7), C0=40, C1=24, K=64, pro=True, silu=True, bias=True,
         plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    case("b_h8_pro_gout", "conv", "conv3x3_halo", N=6, sp=(32, 48), C0=64, K=128, pro=True, silu=True, gout=True,
         bias=True, plan=(H8, 0, 0, 0, 0, 0, 0, 0)),
    case("b_h9_pro_r4", "conv", "conv3x3_halo9b<4>", N=6, sp=(32, 48), C0=64, K=128, pro=True, silu=True, bias=True,
         plan=(H9, 0, 0, 4, 0, 0, 0, 0)),
    case("b_h9_pro_r16", "conv", "conv3x3_halo9b<16>", N=6, sp=(32, 48), C0=40, C1=24, K=128, pro=True, silu=True,
         bias=True, th8=0, plan=(H9, 0, 0, 16, 0, 0, 0, 0)),
    case("b_h9_fold", "conv", "conv3x3_halo9b in-kernel fold", N=6, sp=(32, 48), C0=64, K=128, silu=True, fold=8,
         bias=True, plan=(H9, 0, 0, 4, 0, 0, 0, 1)),
    case("b_s2d_pro", "s2d", "fmd_conv_s2d", N=16, sp=(64, 128), C0=32, K=128, stride=2, pro=True, silu=True,
         bias=True),
    case("b_wg_pro", "wgrad", "wgrad generic", N=3, sp=(5, 7), C0=40, C1=24, K=24, pro=True, silu=True, splits=3,
         halo=False),
    case("b_wh_pro", "wgrad", "wgrad halo", N=3, sp=(16, 32), C0=64, K=128, pro=True, silu=True, splits=3,
         halo=True),
    case("b_ig_ep_two_source", "conv", "conv_igemm epilogue", N=3, sp=(5, 7), C0=72, K=64, mode="dgrad",
         out_sp=(5, 7), epsilu=(40, 24), plan=(IG, 64, 128, 0, 0, 0, 0, 0)),
    case("b_h9_ep", "conv", "conv3x3_halo9b epilogue", N=6, sp=(32, 48), C0=32, K=128, epsilu=(128, 0),
         plan=(H9, 0, 0, 4, 0, 0, 0, 0)),
]
BOUND_BY_NAME = {c.name: c for c in BOUND_CASES}


@functools.lru_cache(maxsize=None)
def real_operands(name):
    """Activation-like operands: x = randn + a per-channel offset (bf16), weights as test_gpu_kernels.py's ``_w``,
    a in [0.5, 1.5), b ~ 0.2 randn."""
    c = BOUND_BY_NAME[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    fan = (c.C0 + c.C1) * c.ks ** c.nd
    T = _operands(c, dict(x=1.0, w=fan ** -0.5, v=0.1), g)
    for k in ("x0", "x1"):
        if k in T:
            T[k] = (T[k].float() + 0.5 * torch.randn(T[k].shape[-1], generator=g)).to(BF16)
    if c.pro:
        T["pro_a"] = torch.rand(T["pro_a"].shape, generator=g) + 0.5
        T["pro_b"] = torch.randn(T["pro_b"].shape, generator=g) * 0.2
    if c.fold:   # GroupNorm parameters and the statistics slab: fp64 sums of 64-pixel rows, stored in fp32
        C = c.C0
        T["gamma"] = torch.rand(C, generator=g) + 0.5
        T["beta"] = torch.randn(C, generator=g) * 0.2
        rows = T["x0"].double().reshape(-1, FOLD_ROWS, C)
        T["slab"] = torch.stack([rows.sum(1), (rows * rows).sum(1)], -1).float()
    if c.epsilu:
        for k, ce in zip(("ex0", "ex1"), c.epsilu):
            if ce:
                T[k] = (torch.randn(c.N, *c.out_sp, ce, generator=g) + 0.5 * torch.randn(ce, generator=g)).to(BF16)
        T["ep_a"] = torch.rand(c.N, c.K, generator=g) + 0.5
        T["ep_b"] = torch.randn(c.N, c.K, generator=g) * 0.2
    return T


FOLD_ROWS, FOLD_EPS = 64, 1e-5   # pixels per row of the fold case's statistics slab; GroupNorm's eps


def fold_affine(c, T):
    """fp64 [N][C]: (a, b, e_a, e_b) of the GroupNorm affine folded from T["slab"], and the error bounds of the
    in-kernel fp32 fold against it (derivation above)."""
    N, C, G = c.N, c.C0, c.fold
    HW = c.sp[0] * c.sp[1]
    E, Cg = HW // FOLD_ROWS, C // G
    slab = T["slab"].double().reshape(N, E, C, 2)
    tot, etot = slab.sum(1), E * U32 * slab.abs().sum(1)            # [N][C][2]
    grp = lambda v: v.reshape(N, G, Cg, 2).sum(2).repeat_interleave(Cg, dim=1)   # noqa: E731
    cnt = Cg * HW
    Gs, eG = grp(tot), grp(etot)
    m = Gs[..., 0] / cnt
    v = (Gs[..., 1] / cnt - m * m).clamp(min=0) + FOLD_EPS
    e_m = eG[..., 0] / cnt
    e_v = eG[..., 1] / cnt + 2 * m.abs() * e_m
    a = T["gamma"].double() / v.sqrt()
    b = T["beta"].double() - m * a
    e_a = a.abs() * (e_v / (2 * v) + 7 * U32)
    e_b = m.abs() * e_a + a.abs() * e_m + 2 * U32 * (m * a).abs() + U32 * b.abs()
    return a, b, e_a, e_b


def _eta_s(z):
    return U32 * (2 * z.abs() + 5)


def bf16_rne(t):
    """fp64 -> nearest bf16 (ties to even) as fp64.  torch converts through fp32, and a value within half an fp32
    ulp of a bf16 tie would then be rounded twice (about 2^-16 of all elements); such a value is moved one fp32
    step off the tie, towards where the fp64 value lies, first."""
    f = t.float()
    res = t - f.double()
    tie = (f.contiguous().view(torch.int32) & 0xFFFF) == 0x8000
    inf = torch.full_like(f, float("inf"))
    f = torch.where(tie & (res != 0), torch.nextafter(f, torch.where(res > 0, inf, -inf)), f)
    return f.to(BF16).double()


def silu_operand(c, T):
    """fp64 [N][C][sp]: dict(t = SiLU(a x + b), zs = bf16(t), lo / hi = bf16(t -+ eps_t), delta = hi - lo)."""
    x = _cf(torch.cat([T["x0"], T["x1"]], -1) if "x1" in T else T["x0"])
    if c.fold:
        a, b, e_a, e_b = (_bc(v, c.nd) for v in fold_affine(c, T))
    else:
        a, b, e_a, e_b = _bc(T["pro_a"], c.nd), _bc(T["pro_b"], c.nd), 0.0, 0.0
    z = a * x + b
    t = z * torch.sigmoid(z)
    eps = t.abs() * (_eta_s(z) + U32) + 1.1 * (2 * U32 * ((a * x).abs() + b.abs()) + e_a * x.abs() + e_b)
    lo, hi = bf16_rne(t - eps), bf16_rne(t + eps)
    return dict(t=t, zs=bf16_rne(t), lo=lo, hi=hi, delta=hi - lo, eps=eps)


def _plain(c, **over):
    d = {k: v for k, v in vars(c).items() if k not in ("nd", "name", "op", "inst")}
    d.update(over)
    return case(c.name, c.op, c.inst, **d)


def bound_reference(c, T):
    """{name: (fp64 reference, elementwise bound)} of a BOUND_CASES row: "out", or "dw" and "db"."""
    Ta = {k: v.abs() for k, v in T.items()}
    nopro = _plain(c, pro=False)
    if c.silu:
        S = silu_operand(c, T)
        R = reference(nopro, T, z=S["zs"])
        A = reference(nopro, Ta, z=S["zs"].abs())
        only_w = {k: Ta[k] for k in ("w", "dy") if k in Ta}
        Fl = reference(_plain(nopro, bias=False), only_w, z=S["delta"])
        if c.op == "wgrad":
            M = c.N
            for s in c.out_sp:
                M *= s
            k = M + 8
            return {n: (R[n], U32 * R[n].abs() + k * U32 * A[n] + (Fl[n] if n == "dw" else 0.0)) for n in ("dw", "db")}
        k = (c.C0 + c.C1) * c.ks ** c.nd + 8
        return dict(out=(R["out"], U16 * R["out"].abs() + k * U32 * A["out"] + Fl["out"]))
    assert c.epsilu
    v = reference(c, T)["out"]
    A = reference(c, Ta)["out"]
    x = ep_tensor(T).double()
    shp = (c.N, *(1,) * c.nd, c.K)
    a, b = T["ep_a"].double().reshape(shp), T["ep_b"].double().reshape(shp)
    z = a * x + b
    s = torch.sigmoid(z)
    g = s * (1 + z * (1 - s))
    eta = _eta_s(z)
    eps_g = g.abs() * (eta + 2 * U32) + s * s * z.abs() * eta + 2 * U32 * s * z.abs() * (1 - s) \
        + U32 * ((a * x).abs() + b.abs())
    k = c.C0 * c.ks ** c.nd + 8
    ref = v * g
    return dict(out=(ref, U16 * ref.abs() + g.abs() * k * U32 * A + v.abs() * eps_g + 2 * U32 * ref.abs()))


def check_bound(got, ref, bound, name, margin=MARGIN):
    """|got - ref| <= margin * bound elementwise (a NaN fails); returns the largest err / bound."""
    got = got.detach().cpu().double()
    err = (got - ref).abs()
    ratio = torch.nan_to_num(err / (bound + TINY), nan=float("inf"))
    bad = ~(err <= margin * bound + TINY)
    if bool(bad.any()):
        ix = tuple(int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape))
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements outside {margin} x bound; worst at "
                             f"{ix}: got {got[ix].item():.9g} ref {ref[ix].item():.9g} err {err[ix].item():.3e} "
                             f"bound {bound[ix].item():.3e} ratio {ratio[ix].item():.3f}")
    return float(ratio.max())


def check_gout(G, S, name):
    """The halo kernel's prologue side output: z* everywhere outside F; inside it a bf16 value from bf16(t - eps_t) to
    bf16(t + eps_t) (rounding is monotone).  These are the two neighbours of the boundary wherever eps_t is below a
    bf16 step; where a x + b cancels (|z| << |a x|) eps_t spans several steps of the tiny t and so may G.  Returns
    the fraction of elements in F."""
    G = G.detach().cpu().double()
    lo, hi = _cl(S["lo"]), _cl(S["hi"])
    bad = ~((G >= lo) & (G <= hi))
    assert not bool(bad.any()), (f"{name}: {int(bad.sum())} of {G.numel()} elements of G lie outside [bf16(t - eps), "
                                 f"bf16(t + eps)] of t = SiLU(a x + b); first at {tuple(bad.nonzero()[0].tolist())}: "
                                 f"{G[tuple(bad.nonzero()[0].tolist())].item()!r}")
    return float((lo != hi).double().mean())


def emulate_bound_case(c, T, mutant=None):
    """fp32 torch arithmetic of a 2-D conv BOUND_CASES row through ``emulate``: the prologue / epilogue factor in
    fp32 (torch's sigmoid), the operand rounded to bf16.  Mutants: "silu_without_shift" (the prologue forgets b),
    "sigmoid_for_silu_grad" (the epilogue multiplies by sigma(z) alone)."""
    if c.silu:
        x = (torch.cat([T["x0"], T["x1"]], -1) if "x1" in T else T["x0"]).float()
        shp = (c.N, *(1,) * c.nd, x.shape[-1])
        z = T["pro_a"].reshape(shp) * x + (0.0 if mutant == "silu_without_shift" else T["pro_b"].reshape(shp))
        return emulate(_plain(c, pro=False), T, z=(z * torch.sigmoid(z)).to(BF16).float())[0]
    x = ep_tensor(T).float()
    shp = (c.N, *(1,) * c.nd, c.K)
    z = T["ep_a"].reshape(shp) * x + T["ep_b"].reshape(shp)
    s = torch.sigmoid(z)
    g = s if mutant == "sigmoid_for_silu_grad" else s * (1 + z * (1 - s))
    return emulate(c, T, gmul=g.reshape(-1, c.K))[0]
