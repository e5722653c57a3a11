"""Exact-lattice checks of the output head, csrc/head.hip ("Output head: saturated lattice").

The head is GroupNorm-affine -> SiLU -> 3x3(x3) conv to K <= 8 channels and its backward.  The conv suite left SiLU
to error bounds; here it is carried by the lattice, because ``sigmoidf_(z) = rcp(1 + __expf(-z))`` saturates exactly
in fp32: for z >= 32 the exponential is below 2^-25, 1 + e^-z is 1.0f and so is its reciprocal (SiLU = z, SiLU' = 1);
for z = 0 the sigmoid is 0.5 (SiLU = 0, SiLU' = 0.5); for z <= -96 the exponential overflows to +inf, the reciprocal
is 0 (SiLU = -0, SiLU' = -0).  With z = a x + b restricted to SAT the transformed operand t is an integer lattice,
every product and partial sum of head_fwd / head_wgrad / head_dgrad is a multiple of a step below 2^24 steps, and
each kernel's value before its final store equals the fp64 reference in any summation order: out, dW, db bit for bit,
dz its round-to-nearest-even to bf16.  tests/test_gpu_head.py holds the premise itself on the device first.

This module imports without a GPU: the case table with the dispatch rules of head.hip, the seeded generators, the
fp64 torch reference (never another kernel), ``conditions``, the comparison functions shared by the CPU and the GPU
test, a plain-torch fp32 emulation with mutants, and the bound rows (real-valued inputs, SiLU not saturated).
"""
from __future__ import annotations

import functools
import types
import zlib

import torch
import torch.nn.functional as F

from conv_lattice import (BF16, MARGIN, PRO_A, TINY, U16, U32, _eta_s, assert_bits, bf16_rne,  # noqa: F401
                          check_bound, guarded, guards_intact, rounding_profile, silu_operand, unwritten)

Z_DRAW = (-128.0, 0.0, 0.0, 32.0, 40.0, 48.0, 56.0, 64.0)   # the targets z is drawn from (0 twice)
SAT = (-128.0, 0.0, 32.0, 40.0, 48.0, 56.0, 64.0)           # the saturated set

# (lowest numerator, highest numerator, denominator)
LATTICES = {
    "fwd": dict(w=(-4, 4, 8), dp=(-4, 4, 4)),          # head_fwd, head_wgrad: w step 1/8, dpred step 1/4
    "coarse": dict(w=(-4, 4, 8), dp=(-4, 4, 4)),       # head_dgrad with exact statistics (rounds nothing)
    "fine": dict(w=(-63, 63, 64), dp=(-31, 31, 16)),   # head_dgrad whose dz must round: w step 1/64, dpred step 1/16
}
BIAS_LAT, DW0_LAT, DB0_LAT = (-8, 8, 4), (-8, 8, 1), (-8, 8, 4)   # dW0: even integers (numerator x 2 below)

HT, CK, WG_WGRAD, RED_SPLIT = 16, 32, 1024, 32   # csrc/head.hip


# ------------------------------------------------------------------------------------------------------ the cases
def case(name, kern, **kw):
    """One row.  ``kern``: "fwd", "dgrad" or "wgrad"; D = 0: 2-D data; ``lattice``: a LATTICES key; ``bias`` / ``db``:
    False passes None; ``kpad``: dpred[..., K:] holds non-zero lattice values (the kernels mask k >= K themselves)."""
    d = dict(name=name, kern=kern, N=2, D=0, H=32, W=48, C=64, K=1, lattice="fwd", bias=True, db=True, kpad=False)
    assert set(kw) <= set(d), set(kw) - set(d)
    d.update(kw)
    c = types.SimpleNamespace(**d)
    c.nd = 3 if c.D else 2
    c.sp = (c.D, c.H, c.W) if c.D else (c.H, c.W)
    return c


# ---- the dispatch rules of head.hip, from the row's shape
def kt_of(K):
    return 1 if K <= 1 else 2 if K <= 2 else 4 if K <= 4 else 8


def shape_ok(N, D, H, W, C, K):
    return (N > 0 and D >= 0 and H % HT == 0 and W % HT == 0 and C % CK == 0 and 1 <= K <= (2 if D > 0 else 8)
            and N * max(D, 1) * H * W * C < 2 ** 31)


def ntiles(c):
    return c.N * max(c.D, 1) * (c.H // HT) * (c.W // HT)


def chunk_groups(c):
    return 4 if ntiles(c) < 128 and c.C >= 4 * CK else 1


def fwd_rounds(c):
    cg = chunk_groups(c)
    return (c.C // CK + cg - 1) // cg


def wgrad_grid(c):
    """(nwg, tiles_per_wg, workgroups that hold a tile, per_split of slot_sum)."""
    nt = ntiles(c)
    nwg = min(nt, WG_WGRAD)
    tpw = (nt + nwg - 1) // nwg
    return nwg, tpw, (nt + tpw - 1) // tpw, (nwg + RED_SPLIT - 1) // RED_SPLIT


def instance(c):
    kz = 3 if c.D else 1
    if c.kern == "fwd":
        return f"head_fwd<{kt_of(c.K)}, {kz}, {chunk_groups(c)}>"
    return f"head_{c.kern}<{kt_of(c.K)}, {kz}>"


F_, D_, W_ = "fwd", "dgrad", "wgrad"
CASES = [
    # ---- 2-D head_fwd, CG = 1: 2 x 32 x 48 (12 tiles), C = 64; every KT, masked rows at K = 3 and 5
    case("f_k1", F_, K=1),
    case("f_k2_nobias", F_, K=2, bias=False),
    case("f_k3", F_, K=3),
    case("f_k4", F_, K=4),
    case("f_k5", F_, K=5),
    case("f_k8", F_, K=8),
    # ---- CG = 4 at 12 tiles
    case("f_cg4_c128", F_, C=128, K=1),                 # one round
    case("f_cg4_c160_k4", F_, C=160, K=4),              # five chunks: groups 1..3 idle in round 2
    case("f_cg4_c512_k8", F_, C=512, K=8),
    case("f_cg4_c128_k2", F_, C=128, K=2),
    # ---- the switch back to CG = 1
    case("f_cg1_128tiles_c128", F_, N=2, H=128, W=128, C=128, K=1),   # 128 tiles: four serial chunks
    case("f_cg1_c96", F_, C=96, K=1),                   # below 4 * CK
    # ---- N = 3, H != W
    case("f_n3_48x16", F_, N=3, H=48, W=16, K=2),
    case("f_n3_16x80", F_, N=3, H=16, W=80, K=1),
    # ---- 2-D head_dgrad: every KT in a fine and a coarse row
    case("d_k1_fine", D_, K=1, lattice="fine"),
    case("d_k1_coarse_c160", D_, K=1, C=160, lattice="coarse"),
    case("d_k2_fine_c160", D_, K=2, C=160, lattice="fine"),          # second 128-channel block, idle threads
    case("d_k2_coarse_n3", D_, N=3, H=48, W=16, K=2, lattice="coarse"),
    case("d_k4_fine", D_, K=4, lattice="fine"),
    case("d_k4_coarse_c256", D_, K=4, C=256, lattice="coarse"),
    case("d_k8_fine", D_, K=8, lattice="fine"),
    case("d_k6_coarse_kpad", D_, N=3, H=16, W=80, K=6, lattice="coarse", kpad=True),
    # ---- 2-D head_wgrad, dW0 and db0 non-zero throughout
    case("w_k1", W_, K=1),
    case("w_k2_nodb", W_, K=2, db=False),
    case("w_k4_c160", W_, K=4, C=160),
    case("w_k6_kpad", W_, N=3, H=48, W=16, K=6, kpad=True),
    case("w_k8", W_, K=8),
    case("w_40wg_per_split2", W_, N=2, H=64, W=80, C=32, K=2),       # 40 workgroups: slot_sum per_split = 2
    case("w_1083_tiles", W_, N=3, H=304, W=304, C=32, K=1),          # tiles_per_wg = 2; see the table test
    # ---- 3-D on 16 x 32
    case("f3_d1_k1", F_, D=1, H=16, W=32, K=1),                       # both depth neighbours are padding
    case("f3_d2_k2_cg4", F_, D=2, H=16, W=32, C=128, K=2),
    case("f3_d5_k1_cg4", F_, D=5, H=16, W=32, C=128, K=1),
    case("f3_d5_k2", F_, D=5, H=16, W=32, K=2),
    case("d3_d1_k1_fine", D_, D=1, H=16, W=32, K=1, lattice="fine"),
    case("d3_d2_k2_coarse_c128", D_, D=2, H=16, W=32, C=128, K=2, lattice="coarse"),
    case("d3_d5_k2_fine", D_, D=5, H=16, W=32, K=2, lattice="fine"),
    case("d3_d5_k1_coarse_kpad", D_, D=5, H=16, W=32, K=1, lattice="coarse", kpad=True),
    case("w3_d1_k1", W_, D=1, H=16, W=32, K=1),
    case("w3_d2_k2_c128", W_, D=2, H=16, W=32, C=128, K=2),
    case("w3_d5_k2", W_, D=5, H=16, W=32, K=2),
    case("w3_1125_tiles", W_, N=1, D=5, H=240, W=240, C=32, K=2),     # 225 tiles per slice: a workgroup straddles
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---------------------------------------------------------------------------------------------------- generators
def _draw(g, shape, lat, dtype):
    lo, hi, den = lat
    return (torch.randint(lo, hi + 1, shape, generator=g).double() / den).to(dtype)


def _bc(v, nd):
    return v.double().reshape(*v.shape, *(1,) * nd)


def _cf(t):
    return t.double().movedim(-1, 1)


def _cl(t):
    return t.movedim(1, -1).contiguous()


@functools.lru_cache(maxsize=None)
def generate(name):
    """The seeded CPU operands of row ``name``: x0 bf16 [N][sp][C] with a x + b in SAT, pro_a / pro_b fp32 [N][C],
    and what the row's kernel reads of w, bias, dpred, dw0, db0."""
    c = BY_NAME[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    L = LATTICES[c.lattice]
    z = torch.tensor(Z_DRAW, dtype=torch.float64)[torch.randint(0, len(Z_DRAW), (c.N, *c.sp, c.C), generator=g)]
    a = torch.tensor(PRO_A, dtype=torch.float64)[torch.randint(0, 4, (c.N, c.C), generator=g)]
    b = 2.0 * torch.randint(-4, 5, (c.N, c.C), generator=g).double()
    shp = (c.N, *(1,) * c.nd, c.C)
    T = dict(x0=((z - b.reshape(shp)) / a.reshape(shp)).to(BF16), pro_a=a.float(), pro_b=b.float())
    if c.kern != W_:
        T["w"] = _draw(g, (c.K, c.C, *(3,) * c.nd), L["w"], torch.float32)
    if c.kern == F_:
        if c.bias:
            T["bias"] = _draw(g, (c.K,), BIAS_LAT, torch.float32)
        return T
    dp = _draw(g, (c.N, *c.sp, 8), L["dp"], BF16)
    if not c.kpad:
        dp[..., c.K:] = 0
    T["dpred"] = dp
    if c.kern == W_:
        T["dw0"] = 2.0 * _draw(g, (c.K, c.C, *(3,) * c.nd), DW0_LAT, torch.float32)
        if c.db:
            T["db0"] = _draw(g, (c.K,), DB0_LAT, torch.float32)
    return T


# ----------------------------------------------------------------------------------------------------- reference
def saturated(c, T):
    """fp64 [N][C][sp]: z = a x + b and, by the saturation argument, t = SiLU(z) and g = SiLU'(z) as fp32 holds them:
    (z, 1) for z >= 32, (0, 0.5) at 0, (-0, -0) for z <= -96."""
    z = _bc(T["pro_a"], c.nd) * _cf(T["x0"]) + _bc(T["pro_b"], c.nd)
    t = torch.where(z > 0, z, torch.zeros_like(z))
    g = torch.where(z >= 32, 1.0, torch.where(z == 0, 0.5, -0.0)).to(torch.float64)
    return z, t, g


def _conv(nd):
    return F.conv2d if nd == 2 else F.conv3d


def _grads(nd, t, dy, K, w=None):
    """fp64 autograd of conv(t, w, b) (zero padding, depth included) at output gradient ``dy``: (dW, db, dL/dt)."""
    C = t.shape[1]
    wz = (torch.zeros(K, C, *(3,) * nd, dtype=torch.float64) if w is None else w.double().clone()).requires_grad_()
    bz = torch.zeros(K, dtype=torch.float64, requires_grad=True)
    tz = t.clone().requires_grad_()
    _conv(nd)(tz, wz, bz, padding=1).backward(dy)
    return wz.grad, bz.grad, tz.grad


def row_map(c, transposed=False):
    """Statistics row of each pixel (flat, channels-last order), as head.hip documents it: row 4 * tile + q holds
    rows 4q .. 4q + 3 of tile ``tile``; tiles run x, then y, then slice (sl = n * D + z)."""
    m = torch.arange(c.N * max(c.D, 1) * c.H * c.W)
    sl, y, x = m // (c.H * c.W), (m // c.W) % c.H, m % c.W
    tile = (sl * (c.H // HT) + y // HT) * (c.W // HT) + x // HT
    return tile * 4 + ((x if transposed else y) % HT) // 4


def _stats(v, x, rowmap):
    """fp64 [rows][C][2]: (sum v, sum v x) per row, v and x channels-last."""
    C = v.shape[-1]
    v, x = v.double().reshape(-1, C), x.double().reshape(-1, C)
    out = torch.zeros(int(rowmap.max().item()) + 1, C, 2, dtype=torch.float64)
    out[..., 0].index_add_(0, rowmap, v)
    out[..., 1].index_add_(0, rowmap, v * x)
    return out


def reference(c, T):
    """fp64 results of the row's kernel, channels-last: {"out"} | {"dw", "db"} (dW0 / db0 added) | {"dz"}."""
    z, t, g = saturated(c, T)
    if c.kern == F_:
        b = T["bias"].double() if "bias" in T else None
        return dict(out=_cl(_conv(c.nd)(t, T["w"].double(), b, padding=1)))
    dy = _cf(T["dpred"])[:, :c.K]
    if c.kern == W_:
        dw, db, _ = _grads(c.nd, t, dy, c.K)
        return dict(dw=dw + T["dw0"].double(), db=db + T["db0"].double() if "db0" in T else db)
    dldt = _grads(c.nd, t, dy, c.K, T["w"])[2] + 0.0      # + 0.0: an exact zero is +0, as a sum started at +0 is
    return dict(dz=_cl(dldt * g))


def expected(c, T, R):
    """What the kernel must store.  fwd: out fp32 [N][sp][8], channels K.. +0.  wgrad: dw, db fp32.  dgrad: dz =
    bf16 RNE of the reference; stats = fp64 sums of that dz per row, stats_abs the rows' sums of |terms|."""
    if c.kern == F_:
        out = torch.zeros(c.N, *c.sp, 8, dtype=torch.float64)
        out[..., :c.K] = R["out"]
        return dict(out=out.float(), out_ref=out)
    if c.kern == W_:
        return dict(dw=R["dw"].float(), db=R["db"].float(), dw_ref=R["dw"], db_ref=R["db"])
    dz = bf16_rne(R["dz"])
    rm = row_map(c)
    return dict(dz=dz.to(BF16), dz_ref=R["dz"], stats=_stats(dz, T["x0"], rm),
                stats_abs=_stats(dz.abs(), T["x0"].double().abs(), rm))


# ---------------------------------------------------------------------------------------------------- conditions
def _on(v, step):
    q = v.double() / step
    return torch.equal(q, q.round())


def _in(v, lat, mul=1.0):
    lo, hi, den = lat
    q = v.double() * den / mul
    return torch.equal(q, q.round()) and q.min().item() >= lo and q.max().item() <= hi


def steps(c):
    """The spacing of every product and partial sum, per result.  t is a multiple of 8 (dW: 8 x dpred's 1/4); out
    counts in bias's and w's 1/8; dz in w step x dpred step x the 1/2 of SiLU'(0)."""
    L = LATTICES[c.lattice]
    return dict(out=1.0 / 8, dw=2.0, db=1.0 / L["dp"][2], dz=0.5 / (L["w"][2] * L["dp"][2]))


def conditions(c, T, R):
    """Assert what the exactness argument needs of row ``c``; returns dict(round=, tie=) of dz (None elsewhere)."""
    n, L, st = c.name, LATTICES[c.lattice], steps(c)
    assert shape_ok(c.N, c.D, c.H, c.W, c.C, c.K), n
    x = T["x0"]
    assert x.dtype == BF16 and torch.equal(x.double(), x.double().to(BF16).double()), f"{n}: x is not a bf16 value"
    a32, b32 = T["pro_a"], T["pro_b"]
    assert all(v in PRO_A for v in a32.unique().tolist()) and _in(b32, (-4, 4, 1), 2.0), f"{n}: a or b off its set"
    for i in range(c.N):
        for j in range(i):
            assert not (torch.equal(a32[i], a32[j]) and torch.equal(b32[i], b32[j])), f"{n}: samples share an affine"
    # a x + b in fp32, product then sum (an fma gives the same where both are exact)
    shp = (c.N, *(1,) * c.nd, c.C)
    ax = a32.reshape(shp) * x.float()
    z32 = ax + b32.reshape(shp)
    z, t, g = saturated(c, T)
    assert torch.equal(ax.double(), a32.reshape(shp).double() * x.double()) and torch.equal(_cf(z32), z), \
        f"{n}: a x + b is not exact in fp32"
    assert all(v in SAT for v in z.unique().tolist()), f"{n}: z leaves the saturated set"
    assert set(z.unique().tolist()) == set(SAT), f"{n}: a saturated value never occurs"
    assert (z * torch.sigmoid(z) - t).abs().max().item() < 1e-10       # the lattice t is SiLU(z) to fp64 accuracy
    if "w" in T:
        assert _in(T["w"], L["w"]), f"{n}: w off its lattice"
        if c.kern == F_:
            assert torch.equal(T["w"], T["w"].to(BF16).float()), f"{n}: w does not survive head_fwd's bf16 pack"
        nz = T["w"].flatten(2).reshape(c.K, c.C // 8, 8, -1).abs().amax(dim=(0, 2))
        assert (nz > 0).all(), f"{n}: a (tap, 8-channel group) of the weights is all zero"
    if "bias" in T:
        assert _in(T["bias"], BIAS_LAT)
    if "dpred" in T:
        dp = T["dpred"]
        assert dp.dtype == BF16 and _in(dp, L["dp"]), f"{n}: dpred off its lattice"
        tail = dp[..., c.K:]
        if tail.numel():
            assert bool((tail != 0).any()) == c.kpad and (not c.kpad or (tail != 0).double().mean().item() > 0.5), n
    if "dw0" in T:
        assert _in(T["dw0"], DW0_LAT, 2.0) and (T["dw0"] != 0).any()
    if "db0" in T:
        assert _in(T["db0"], DB0_LAT) and (T["db0"] != 0).any()
    # the cap: with |operands| every partial sum of the real op is bounded by the same sum
    Ta = {k: v.abs() for k, v in T.items()}
    Ta["x0"] = _cl(t.abs()).to(BF16)           # |t| through a = 1, b = 0
    Ta["pro_a"], Ta["pro_b"] = torch.ones_like(a32), torch.zeros_like(b32)
    caps = {}
    for k, v in reference(c, Ta).items():
        caps[k] = v.abs().max().item() / st[k]
        assert caps[k] < 2.0 ** 24, f"{n}: {k} reaches {caps[k]:.3g} units >= 2^24"
    for k, v in R.items():
        assert _on(v, st[k]), f"{n}: {k} leaves the lattice"
    prof = dict(round=None, tie=None, caps=caps)
    if c.kern == F_:
        out = R["out"].reshape(-1, c.K)
        assert (out.abs().amax(0) > 0).all(), f"{n}: an all-zero output channel"
    elif c.kern == W_:
        assert (R["dw"] - T["dw0"].double()).flatten(1).abs().amax(1).min().item() > 0, f"{n}: an all-zero dW row"
        assert ((R["db"] - (T["db0"].double() if "db0" in T else 0.0)) != 0).all(), f"{n}: db is zero"
    else:
        E = expected(c, T, R)
        assert (R["dz"].reshape(-1, c.C).abs().amax(0) > 0).all(), f"{n}: an all-zero dz channel"
        r, tie = rounding_profile(R["dz"])
        prof.update(round=r, tie=tie)
        if c.lattice == "fine":
            assert r >= 0.50 and tie >= 0.05, f"{n}: {r:.1%} of dz round, {tie:.1%} ties"
        else:
            # a row holds 64 pixels of one image: the 64 largest |dz x| of an (image, channel) bound any row
            e = (E["dz"].double() * x.double()).abs().reshape(c.N, -1, c.C)
            top = e.topk(64, dim=1).values.sum(1).max().item() / st["dz"]
            prof["caps"]["stats"] = top
            assert top < 2.0 ** 24, f"{n}: a row's second sum reaches {top:.3g} units: statistics inexact"
            assert _on(E["stats"], st["dz"])
    return prof


@functools.lru_cache(maxsize=None)
def problem(name):
    """(operands, fp64 reference, expected stores, profile) of a row, its conditions asserted; computed once."""
    c = BY_NAME[name]
    T = generate(name)
    R = reference(c, T)
    prof = conditions(c, T, R)
    return T, R, expected(c, T, R), prof


# ---------------------------------------------------------------------------------------------------- comparison
STATS_FACTOR = 70   # fine rows: 64 additions of a row's serial sums plus the cross-lane adds, each <= U32 sum|terms|


def check_fwd(c, out, E, what):
    assert_bits(out, E["out"], E["out_ref"], f"{what} out")


def check_wgrad(c, dw, db, E, what):
    assert_bits(dw, E["dw"], E["dw_ref"], f"{what} dW")
    if db is not None:
        assert_bits(db, E["db"], E["db_ref"], f"{what} db")


def check_dgrad(c, dz, stats, E, what):
    assert_bits(dz, E["dz"], E["dz_ref"], f"{what} dz")
    stats = stats.detach().cpu()
    assert tuple(stats.shape) == tuple(E["stats"].shape), (what, stats.shape, E["stats"].shape)
    if c.lattice != "fine":
        assert_bits(stats, E["stats"].float(), E["stats"], f"{what} statistics")
        return
    err = (stats.double() - E["stats"]).abs()
    bad = ~(err <= STATS_FACTOR * U32 * E["stats_abs"])
    if bool(bad.any()):
        ix = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what} statistics: {int(bad.sum())} of {bad.numel()} outside {STATS_FACTOR} u sum|terms|"
                             f"; first {ix}: {stats[ix].item()!r} / {E['stats'][ix].item()!r}, sum|terms| "
                             f"{E['stats_abs'][ix].item()!r}")


def check(c, got, E, what):
    """``got``: the dict ``emulate`` returns, or the kernel's outputs under the same keys."""
    if c.kern == F_:
        check_fwd(c, got["out"], E, what)
    elif c.kern == W_:
        check_wgrad(c, got["dw"], got.get("db"), E, what)
    else:
        check_dgrad(c, got["dz"], got["stats"], E, what)


# ------------------------------------------------------------------------------------- plain-torch emulation
MUTANTS = ["pad_neighbour", "wrong_sample_affine", "depth_pad_wraps", "chunk_dropped", "tap_transposed",
           "dgrad_tap_not_flipped", "kpad_leak", "last_tile_dropped", "empty_slot_stale", "bias_every_depth_pass",
           "overwrite_not_accumulate", "silu_grad_zero_is_one", "stats_from_unrounded_dz", "stats_row_transposed"]
BOUND_MUTANTS = ["silu_without_shift", "sigmoid_for_silu_grad"]


def _sigmoid32(z):
    """1 / (1 + exp(-z)) in fp32, the kernel's formula: exactly 1 for z >= 17, exactly 0 once exp overflows."""
    return 1.0 / (1.0 + torch.exp(-z))


def emulate(c, T, mutant=None):
    """fp32 torch emulation of the row's kernel: t = SiLU(a x + b) rounded to bf16, weights rounded to bf16 in the
    forward only, taps and chunks summed last-first (wgrad: per-workgroup slots summed pairwise), dz stored through
    bf16.  ``mutant``: one of MUTANTS / BOUND_MUTANTS, ignored where the row has nothing it applies to.  Returns the
    kernel's outputs as a dict: out | dw, db | dz, stats."""
    N, Dd, H, W, C, K = c.N, max(c.D, 1), c.H, c.W, c.C, c.K
    KZ, pz = (3, 1) if c.D else (1, 0)
    x = T["x0"].float().reshape(N, Dd, H, W, C)
    a, b = T["pro_a"], T["pro_b"]
    if mutant == "wrong_sample_affine":
        a, b = a.roll(1, 0), b.roll(1, 0)
    z = a[:, None, None, None, :] * x
    if mutant != "silu_without_shift":
        z = z + b[:, None, None, None, :]
    s = _sigmoid32(z)
    t = (z * s).to(BF16).float()
    tp = F.pad(t, (0, 0, 1, 1, 1, 1, pz, pz))
    if mutant == "pad_neighbour":          # the column test forgotten: the flat address wraps into the next row
        tp[:, pz:pz + Dd, 2:H + 1, 0] = t[:, :, :H - 1, W - 1]
        tp[:, pz:pz + Dd, 1:H, W + 1] = t[:, :, 1:, 0]
    if mutant == "depth_pad_wraps" and KZ == 3:   # slice z - 1 of the previous sample where zero belongs
        tp[1:, 0, 1:H + 1, 1:W + 1] = t[:-1, Dd - 1]
    taps = [(kz, ky, kx) for kz in reversed(range(KZ)) for ky in reversed(range(3)) for kx in reversed(range(3))]
    if c.kern == F_:
        w = T["w"].reshape(K, C, KZ, 3, 3).to(BF16).float()
        acc = torch.zeros(N, Dd, H, W, K)
        for kz, ky, kx in taps:
            wy, wx = (kx, ky) if (mutant == "tap_transposed" and (ky, kx) == (0, 1)) else (ky, kx)
            for c0 in reversed(range(0, C, CK)):
                if mutant == "chunk_dropped" and C == 160 and c0 == 128:
                    continue
                acc += tp[:, kz:kz + Dd, ky:ky + H, kx:kx + W, c0:c0 + CK] @ w[:, c0:c0 + CK, kz, wy, wx].t()
        if "bias" in T:
            acc += T["bias"]
        out = torch.zeros(N, *c.sp, 8)
        out[..., :K] = acc.reshape(N, *c.sp, K)
        return dict(out=out)
    dp = T["dpred"].float().reshape(N, Dd, H, W, 8)
    ty, tx = H // HT, W // HT
    if c.kern == W_:
        dpt = dp[..., :K].reshape(N * Dd, ty, HT, tx, HT, K)
        nt = N * Dd * ty * tx
        part = torch.zeros(nt, K, C, KZ, 3, 3)
        for kz, ky, kx in taps:
            src = tp[:, kz:kz + Dd, ky:ky + H, kx:kx + W].reshape(N * Dd, ty, HT, tx, HT, C)
            part[..., kz, ky, kx] = torch.einsum("saybxk,saybxc->sabkc", dpt, src).reshape(nt, K, C)
        bpart = dpt.sum(dim=(2, 4)).reshape(nt, K)
        if mutant == "bias_every_depth_pass" and KZ == 3:   # the bias sums on every depth pass that is not padding
            zz = torch.arange(Dd)
            passes = sum(((zz + kz - 1 >= 0) & (zz + kz - 1 < Dd)).float() for kz in range(3))
            bpart = bpart * passes.repeat(N).repeat_interleave(ty * tx)[:, None]
        if mutant == "last_tile_dropped":
            part[nt - 1], bpart[nt - 1] = 0.0, 0.0
        nwg, tpw, used, _ = wgrad_grid(c)
        wg = torch.arange(nt) // tpw
        slots = torch.zeros(nwg, K, C, KZ, 3, 3).index_add_(0, wg, part)
        bslots = torch.zeros(nwg, K).index_add_(0, wg, bpart)
        if mutant == "empty_slot_stale" and used < nwg:     # what an earlier launch left there
            slots[used:], bslots[used:] = slots[0], bslots[0]
        dw, db = slots.sum(0).reshape(K, C, *(3,) * c.nd), bslots.sum(0)
        if mutant != "overwrite_not_accumulate":
            dw, db = dw + T["dw0"], (db + T["db0"] if "db0" in T else db)
        return dict(dw=dw, db=db if c.db else None)
    w = T["w"].reshape(K, C, KZ, 3, 3)
    Ku = K
    if mutant == "kpad_leak":               # dpred rows K .. KT - 1 meet a neighbouring row's weights
        Ku = kt_of(K)
        w = w[torch.arange(Ku) % K]
    dpp = F.pad(dp[..., :Ku], (0, 0, 1, 1, 1, 1, pz, pz))
    acc = torch.zeros(N, Dd, H, W, C)
    for kz, ky, kx in taps:
        oz, oy, ox = (kz, ky, kx) if mutant == "dgrad_tap_not_flipped" else (2 * pz - kz, 2 - ky, 2 - kx)
        acc += dpp[:, oz:oz + Dd, oy:oy + H, ox:ox + W] @ w[:, :, kz, ky, kx]
    g = s if mutant == "sigmoid_for_silu_grad" else s * (1.0 + z * (1.0 - s))
    if mutant == "silu_grad_zero_is_one":
        g = torch.where(z == 0, torch.ones_like(g), g)
    dz32 = acc * g
    dz = dz32.to(BF16)
    v = dz32 if mutant == "stats_from_unrounded_dz" else dz.float()
    rm = row_map(c, transposed=mutant == "stats_row_transposed")
    stats = torch.zeros(int(rm.max().item()) + 1, C, 2)
    stats[..., 0].index_add_(0, rm, v.reshape(-1, C))
    stats[..., 1].index_add_(0, rm, (v * x).reshape(-1, C))
    return dict(dz=dz.reshape(N, *c.sp, C), stats=stats)


# ================================================================ what the lattice leaves out: SiLU not saturated
# Real-valued inputs as conv_lattice.real_operands draws them, each kernel held to an fp64 reference within MARGIN x
# an elementwise bound.  With u = U32, zs = bf16(SiLU(a x + b)) in fp64, delta the flip width of silu_operand:
#   head_fwd:   |out - ref| <= u |ref| + k u conv(|zs|, |w|) + conv(delta, |w|) + 2^-9 conv(|zs|, |w|),
#               k = 9 KZ C + 8; the last term is the forward's bf16 weights (half a bf16 ulp each), ref uses fp32 w
#   head_wgrad: conv_lattice's b_wh_pro formula with M = every pixel: u |ref| + (M + 8) u grad(|zs|, |dy|) + for dW
#               grad(delta, |dy|)
#   head_dgrad: conv_lattice's epsilu formula with k = 9 KZ K + 8, fp32 weights unrounded:
#               U16 |ref| + |g| k u A + |v| eps_g + 2u |ref|
BOUND_CASES = [
    case("b_fwd", F_, K=3),
    case("b_fwd_cg4", F_, C=128, K=2),
    case("b_dgrad", D_, K=3),
    case("b_wgrad", W_, K=3),
    case("b3_fwd", F_, D=3, H=16, W=32, K=2),
    case("b3_dgrad", D_, D=3, H=16, W=32, K=2),
    case("b3_wgrad", W_, D=3, H=16, W=32, K=2),
]
BOUND_BY_NAME = {c.name: c for c in BOUND_CASES}


@functools.lru_cache(maxsize=None)
def real_operands(name):
    """x = randn + a per-channel offset (bf16), w = randn / sqrt(fan-in), a in [0.5, 1.5), b ~ 0.2 randn, bias ~ 0.1
    randn, dpred ~ 0.5 randn (bf16, channels K.. zero), dW0 / db0 ~ 0.1 randn."""
    c = BOUND_BY_NAME[name]
    g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    fan = c.C * 3 ** c.nd
    T = dict(x0=(torch.randn(c.N, *c.sp, c.C, generator=g) + 0.5 * torch.randn(c.C, generator=g)).to(BF16),
             pro_a=torch.rand(c.N, c.C, generator=g) + 0.5, pro_b=torch.randn(c.N, c.C, generator=g) * 0.2)
    if c.kern != W_:
        T["w"] = torch.randn(c.K, c.C, *(3,) * c.nd, generator=g) * fan ** -0.5
    if c.kern == F_:
        T["bias"] = torch.randn(c.K, generator=g) * 0.1
        return T
    T["dpred"] = (torch.randn(c.N, *c.sp, 8, generator=g) * 0.5).to(BF16)
    T["dpred"][..., c.K:] = 0
    if c.kern == W_:
        T["dw0"] = torch.randn(c.K, c.C, *(3,) * c.nd, generator=g) * 0.1
        T["db0"] = torch.randn(c.K, generator=g) * 0.1
    return T


def bound_reference(c, T):
    """{name: (fp64 reference, elementwise bound)} of a BOUND_CASES row."""
    nd, KZ = c.nd, 3 if c.D else 1
    conv = _conv(nd)
    if c.kern == D_:
        dy = _cf(T["dpred"])[:, :c.K]
        zero = torch.zeros(c.N, c.C, *c.sp, dtype=torch.float64)
        v = _cl(_grads(nd, zero, dy, c.K, T["w"])[2])
        A = _cl(_grads(nd, zero, dy.abs(), c.K, T["w"].abs())[2])
        x = T["x0"].double()
        shp = (c.N, *(1,) * nd, c.C)
        a, b = T["pro_a"].double().reshape(shp), T["pro_b"].double().reshape(shp)
        z = a * x + b
        s = torch.sigmoid(z)
        g = s * (1 + z * (1 - s))
        eta = _eta_s(z)
        eps_g = g.abs() * (eta + 2 * U32) + s * s * z.abs() * eta + 2 * U32 * s * z.abs() * (1 - s) \
            + U32 * ((a * x).abs() + b.abs())
        k = 9 * KZ * c.K + 8
        ref = v * g
        return dict(dz=(ref, U16 * ref.abs() + g.abs() * k * U32 * A + v.abs() * eps_g + 2 * U32 * ref.abs()))
    S = silu_operand(types.SimpleNamespace(nd=nd, fold=None), T)
    if c.kern == F_:
        w = T["w"].double()
        ref = _cl(conv(S["zs"], w, T["bias"].double(), padding=1))
        A = _cl(conv(S["zs"].abs(), w.abs(), padding=1))
        Fl = _cl(conv(S["delta"], w.abs(), padding=1))
        k = 9 * KZ * c.C + 8
        return dict(out=(ref, U32 * ref.abs() + k * U32 * A + Fl + 2.0 ** -9 * A))
    dy = _cf(T["dpred"])[:, :c.K]
    dw, db, _ = _grads(nd, S["zs"], dy, c.K)
    dwa, dba, _ = _grads(nd, S["zs"].abs(), dy.abs(), c.K)
    fl = _grads(nd, S["delta"], dy.abs(), c.K)[0]
    dw, db = dw + T["dw0"].double(), db + T["db0"].double()
    k = c.N * max(c.D, 1) * c.H * c.W + 8
    return dict(dw=(dw, U32 * dw.abs() + k * U32 * dwa + fl), db=(db, U32 * db.abs() + k * U32 * dba))


def check_bounds(c, got, B, what, margin=MARGIN):
    """``check_bound`` of every result of the row (fwd: channels < K); returns {name: largest err / bound}."""
    if c.kern == F_:
        return dict(out=check_bound(got["out"][..., :c.K], *B["out"], f"{what} out", margin))
    return {k: check_bound(got[k], *B[k], f"{what} {k}", margin) for k in B}
