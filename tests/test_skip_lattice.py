"""skip_lattice.py checked on the CPU before any GPU run.

1. The fp64 statement of the skip pass equals autograd of the operation it fuses (a 1x1 conv over the concatenated
   input whose data gradient enters the GroupNorm-backward apply) at 1e-12, and its two roundings are the
   round-to-nearest-even of exact values; the dropout statement equals autograd of dropout(SiLU(a h + b)) under the
   oracle's mask.
2. The conditions hold for every case: every partial sum is exact in fp32, and at least 1 % of the dx elements have a
   conv term its rounding changes, show the double rounding, and are ties of the final rounding.
3. Every case the GPU module runs passes against the fp32 emulation (skip_lattice.Emu): bit equality on the lattice,
   ratio < 1 (no margin) where a bound is used; Emu(perm=True) walks every reduction backwards and changes no bit.
4. Mutants of the emulation are rejected by the same checks at the same shapes, in every case in which the bug can
   show at all (skip_lattice.MUTANTS), and every skip-pass case is rejected under the mutants aimed at the edge it
   exists for (skip_lattice.EDGE).  Rejected / applicable cases:

   mutant               families             rejected   caught by
   conv_not_rounded     gn_apply, skip_bwd     65/65    dx bits (the inner rounding is visible in >= 1 %)
   store_truncated      gn_apply, skip_bwd     65/65    dx bits
   store_half_away      gn_apply, skip_bwd     65/65    dx bits (ties >= 1 %)
   n_from_tile_start    gn_apply, skip_bwd     65/65    dx bits (tiles that straddle images)
   source_per_tile      gn_apply, skip_bwd     30/30    dx bits (seam inside a channel tile)
   acc_swapped          gn_apply, skip_bwd     28/28    NaN from the overwritten destination
   old_ignored          gn_apply, skip_bwd     47/47    dx bits
   r_image0             gn_apply, skip_bwd     65/65    dx bits
   last_tile_dropped    skip_bwd               45/45    dW equal to fp64
   stale_slab           skip_bwd               20/20    dW, db (groups above the tile count)
   db_per_ctile         skip_bwd               36/36    db (C > 128)
   old_dw_dropped       skip_bwd               25/25    dW
   idx_no_channel       dropout_fwd, _bwd      6/6      mask (C > 8)
   idx_nchw             dropout_fwd, _bwd      9/9      mask
   seed_plus_1          dropout_fwd, _bwd      8/8      mask
   salt_ignored         dropout_fwd, _bwd      8/8      mask
   scale_omitted        dropout_fwd, _bwd      8/8      values, bound
   p_for_1mp            dropout_fwd, _bwd      7/7      values, bound (p != 1/2)
   ab_image0            dropout_bwd            2/2      bound
   bwd_mask_shift8      dropout_bwd            2/2      zeros against the forward's
   silu_not_grad        dropout_bwd            2/2      bound
   (the 16.8 M-element grid-stride shape is run under the two index mutants only)

5. What the earlier tolerances see.  The issue behind this suite estimated that the tolerances which held
   fmd_skip_bwd's dW (rtol 2e-2 with atol 2e-2 max|ref| in test_gpu_skip_bwd.py; ``_close`` of test_gpu_kernels.py
   at 1.5e-2 max|ref|) would let a dropped partial last tile pass on the white-noise M = 288 problems of
   skip_bwd_cases.py.  They do not: dropping the tile (32 of 288 pixels) moves dW by 0.33 to 0.42 of max|ref|
   (25 to 29 against 64 to 78), twenty times either tolerance, so both reject it
   (test_old_tolerances_reject_the_dropped_tile asserts that, in place of the assertion that they miss it).  What
   they cannot see is anything below 1.5e-2 max|ref|: a stale slab of small values, one wrong rounding, a wrong
   source behind the seam on a few channels -- which is what the lattice holds to the bit.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import skip_bwd_cases as sc
import skip_lattice as sl

F64 = torch.float64
ALL = sl.case_ids()
SKIP_NAMES = [c.name for c in sl.GNA_CASES + sl.SKIP_CASES]


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-300))


# ------------------------------------------------------------------ 1. the statements vs autograd
@pytest.mark.parametrize("name", ["gna64_k24_seam40", "gna128_k128_vol", "skip_c136_m105"])
def test_skip_statement_equals_autograd(name):
    """conv term, dW and db are the gradients of y = conv1x1(cat(x0, x1)) + bias under dy; the rest of dx is the
    affine P dz + Q x + R (+ old) per (image, channel); the two roundings are RNE of exact values."""
    c, T = sl.BY_NAME[name], sl.generate(name)
    x = T["x"].double().movedim(-1, 1).clone().requires_grad_()
    w = T["w"].double().reshape(c.Kd, c.C, *[1] * len(c.sp)).clone().requires_grad_()
    b = torch.zeros(c.Kd, dtype=F64, requires_grad=True)
    conv = F.conv2d if len(c.sp) == 2 else F.conv3d
    conv(x, w, b).backward(T["dy"].double().movedim(-1, 1))
    R = sl.reference(name, 1, 1 if c.C1 else 0, True)
    assert _rel(R["conv"], x.grad.movedim(1, -1).reshape(c.M, c.C)) < 1e-12
    assert _rel(R["dw"] - T["dw0"].double().reshape(c.Kd, c.C), w.grad.reshape(c.Kd, c.C)) < 1e-12
    assert _rel(R["db"] - T["db0"].double(), b.grad) < 1e-12
    bc = lambda v: v.double().reshape(c.N, *[1] * len(c.sp), c.C)     # noqa: E731
    rest = bc(T["P"]) * T["dz"].double() + bc(T["Q"]) * T["x"].double() + bc(T["R"]) + T["old"].double()
    assert torch.equal(R["s"], R["conv_r"] + rest.reshape(c.M, c.C))
    for exact, rounded in ((R["conv"], R["conv_r"]), (R["s"], R["dx"])):
        assert torch.equal(rounded, exact.float().to(torch.bfloat16).double())    # exact in fp32: torch's RNE
        up = rounded.to(torch.bfloat16)
        assert torch.equal(up.double(), rounded) and bool(((rounded - exact).abs() <= 2.0 ** -8 * exact.abs()).all())


@pytest.mark.parametrize("p", sl.BWD_P)
def test_dropout_statement_equals_autograd(p):
    d = sl.bwd_inputs()
    sh = tuple(d["dy"].shape)
    keep = sl.keep_ref(sl.DROP_SEEDS[0], sl.DROP_SALTS[1], sh, p)
    N, C = d["a"].shape
    a, b = (v.double().reshape(N, 1, 1, C) for v in (d["a"], d["b"]))
    h = d["h"].double().clone().requires_grad_()
    t = F.silu(a * h + b)
    y = t * keep.double() * sl.drop_scale(p)
    y.backward(d["dy"].double())
    ref, bnd = sl.bwd_ref(d, keep, p)
    # d/dh carries the GroupNorm scale a; the kernel's output is the gradient at z = a h + b
    assert _rel(ref * a, h.grad) < 1e-12
    assert bool((bnd[keep] > 0).all()) and bool((bnd[~keep] == 0).all())
    # forward: F.dropout's definition under the same mask
    x = d["dy"].double()
    want = torch.where(keep, x / (1 - float(torch.tensor(p))), 0 * x)
    assert _rel(x * keep.double() * sl.drop_scale(p), want) < 1e-12


def test_oracle_mask_is_a_counter_hash():
    """keep_mask_nhwc is a pure function of (seed, salt, flat index): a larger tensor's mask starts with a smaller's."""
    small = sl.keep_ref(5, 3, (2, 3, 8), 0.5).reshape(-1)
    large = sl.keep_ref(5, 3, (4, 3, 8), 0.5).reshape(-1)
    assert torch.equal(large[:small.numel()], small)
    assert bool(sl.keep_ref(5, 3, (4, 3, 8), 0.0).all())


# ------------------------------------------------------------------ 2. conditions
@pytest.mark.parametrize("name", SKIP_NAMES)
def test_conditions(name):
    sh = sl.conditions(name)
    for acc, (cv, dr, tie) in sh.items():
        print(f"{name} acc {acc}: conv term rounds {cv:.1%}, double rounding visible {dr:.1%}, ties {tie:.1%}")


def test_case_tables():
    for c in sl.GNA_CASES:
        assert c.inst == ("IG_GNA64" if c.C <= 64 else "IG_GNA128")
    assert {c.name for c in sl.GNA_CASES + sl.SKIP_CASES} == set(sl.EDGE)
    for c in sl.SKIP_CASES:
        assert c.Kd == 128 and c.C > 64 and c.M % 64
    tiles = {c.name: -(-c.M // 64) for c in sl.SKIP_CASES}
    assert any(t >= 8 for t in tiles.values()) and any(t < 3 for t in tiles.values())   # G = 8 both ways, 3 > tiles
    N, sp, C = sl.DROP_SHAPES["stride_c64"]
    assert 8192 * 256 < N * sp[0] * sp[1] * C // 8 < 8192 * 256 + 512 and N * sp[0] * sp[1] * C < 2 ** 32
    assert any(t >= 2 ** 31 for t in sl.DROP_SALTS) and all(s * 0x9E3779B9 >= 2 ** 32 for s in sl.DROP_SEEDS)


# ------------------------------------------------------------------ 3. the emulation passes every case
@pytest.mark.parametrize("family,case", ALL, ids=[f"{f}-{c}" for f, c in ALL])
def test_emulation_passes(family, case):
    r = sl.CASES[family][case](sl.Emu(), "cpu")
    if r is not None:
        print(f"{family} {case}: fp32 emulation at {r:.3f} of the bound")
        assert r < 1.0, f"{family} {case}: fp32 emulation at {r:.3f} of the bound"


LATTICE = [(f, c) for f, c in ALL if f in ("gn_apply", "skip_bwd") or (f == "dropout_fwd" and "p0.3" not in c
                                                                      and "stride" not in c)]


@pytest.mark.parametrize("family,case", LATTICE, ids=[f"{f}-{c}" for f, c in LATTICE])
def test_lattice_is_order_independent(family, case):
    """Every reduction walked backwards: bit-equal to the fp64 statement all the same."""
    sl.CASES[family][case](sl.Emu(perm=True), "cpu")


# ------------------------------------------------------------------ 4. mutants
@functools.lru_cache(maxsize=None)
def _rejected(mutant):
    out = {}
    for family, case in sl.mutant_cases(mutant):
        if "stride" in case and mutant not in ("idx_no_channel", "idx_nchw"):
            continue                                     # 16.8 M elements: only the index mutants need the shape
        try:
            sl.CASES[family][case](sl.Emu(mutant=mutant), "cpu")
            out[(family, case)] = False
        except AssertionError:
            out[(family, case)] = True
    return out


@pytest.mark.parametrize("mutant", list(sl.MUTANTS))
def test_mutant_is_rejected_in_every_applicable_case(mutant):
    res = _rejected(mutant)
    assert res, "no applicable case"
    missed = [c for c, ok in res.items() if not ok]
    print(f"{mutant}: rejected {len(res) - len(missed)}/{len(res)}")
    assert not missed, f"{mutant} ({sl.MUTANTS[mutant][0]}) passes in {missed}"


@pytest.mark.parametrize("name", SKIP_NAMES)
def test_every_case_is_rejected_under_the_mutants_aimed_at_its_edge(name):
    assert sl.EDGE[name]
    for mutant in sl.EDGE[name]:
        hit = [k for k, ok in _rejected(mutant).items() if ok and k[1].split("-")[0] == name]
        assert hit, f"{name}: no run of this case is rejected under {mutant}"


# ------------------------------------------------------------------ 5. what the earlier tolerances see
def _close_passes(got, ref, rel=1.5e-2):
    """``_close`` of test_gpu_kernels.py."""
    err = (got.float() - ref.float()).abs().max().item()
    return err <= rel * max(ref.float().abs().max().item(), 1e-6)


@pytest.mark.parametrize("name", ["c128_128", "c256_128", "single", "c192"])
def test_old_tolerances_reject_the_dropped_tile(name):
    """The dropped-tile mutant on the white-noise M = 288 problems test_gpu_skip_bwd.py runs: both tolerances that
    held dW before this suite reject it (module docstring, 5)."""
    p = sc.problem(name)
    res = {}
    for mutant in (None, "last_tile_dropped"):
        dx0, dx1 = p["dx0"].clone(), (p["dx1"].clone() if p["dx1"] is not None else None)
        dw, db = torch.zeros_like(p["dw0"]), torch.zeros_like(p["db0"])
        E = sl.Emu(mutant=mutant)
        assert E.skip_bwd(p["dy"], E.prep_weights(p["w"], 1), p["dz"], p["x0"], p["x1"], p["P"], p["Q"], p["R"], dx0, 0,
                          dx1, 0, dw, db, accumulate=False, groups=3, min_tiles=0)
        res[mutant] = dw.double().reshape(p["Kd"], -1)
    dw_ref = sc.reference(name)[0]
    mx = dw_ref.abs().max().item()

    def old_assert(got):
        try:
            torch.testing.assert_close(got, dw_ref, rtol=2e-2, atol=2e-2 * mx)
            return True
        except AssertionError:
            return False
    assert old_assert(res[None]) and _close_passes(res[None], dw_ref)
    err = (res["last_tile_dropped"] - dw_ref).abs().max().item()
    print(f"{name}: dropped tile: max|dW - fp64| {err:.3f}, max|ref| {mx:.3f}, ratio {err / mx:.3f}; "
          f"assert_close(2e-2) passes {old_assert(res['last_tile_dropped'])}, "
          f"_close(1.5e-2) passes {_close_passes(res['last_tile_dropped'], dw_ref)}")
    assert not old_assert(res["last_tile_dropped"]) and not _close_passes(res["last_tile_dropped"], dw_ref)
