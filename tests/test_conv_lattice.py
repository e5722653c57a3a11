"""The exact-lattice convolution checks of conv_lattice.py, held on the CPU before any GPU run.

1. Every case of the GPU table meets the conditions of the exactness argument (bf16-exact operands, the 2^24 step
   cap, no silent rows or weight chunks), and every kernel instance with bf16 outputs has a case in which at least
   10 % of the outputs round and 5 % are exact ties -- so a wrong rounding mode cannot pass.
2. A plain-torch fp32 emulation that sums in an order no kernel uses passes the same bit comparison; twelve mutants
   of it (the mistakes the table exists to catch) all fail it, while the tolerance the suite used so far --
   1.5e-2 max|ref| on white noise, square images -- lets several of them through.  The table is printed (-s).
"""
import pytest
import torch

import conv_lattice as CL

PROFILE = {}


def _ids(cases):
    return [c.name for c in cases]


@pytest.mark.parametrize("c", CL.ALL_CASES, ids=_ids(CL.ALL_CASES))
def test_case_meets_the_conditions(c):
    T = CL.generate(c.name)
    R = CL.reference(c, T)
    PROFILE[c.name] = CL.conditions(c, T, R)


def test_every_instance_has_a_rounding_case():
    by_inst = {}
    for c in CL.ALL_CASES:
        if c.name not in PROFILE:   # run alone: profile the case here
            T = CL.generate(c.name)
            PROFILE[c.name] = CL.conditions(c, T, CL.reference(c, T))
        p = PROFILE[c.name]
        if p["round"] is not None:
            by_inst.setdefault(c.inst, []).append((c.name, p["round"], p["tie"]))
    assert set(by_inst) >= {"IG_K16", "IG_K64", "IG_PX128", "IG_PX64", "IG_PX32", "HALO9_16", "HALO9_8", "HALO9_4",
                            "HALO8", "S2D", "D2S", "SMALL"}
    for inst, rows in by_inst.items():
        best = max(rows, key=lambda r: min(r[1] / 0.10, r[2] / 0.05))
        print(f"{inst:9s} {len(rows):2d} bf16 cases; most rounding: {best[0]} "
              f"({best[1]:.1%} round, {best[2]:.1%} ties)")
        assert best[1] >= 0.10 and best[2] >= 0.05, (inst, rows)


def test_table_covers_the_tiling_edges():
    """Non-square everywhere; the 40|24 seam on both kernel families and in the 1x1 segment; a K = 136 second cout
    tile; every implicit-GEMM pixel tile; every halo tile height; the round-3 halo kernel."""
    names = set(CL.BY_NAME)
    assert len(names) == len(CL.ALL_CASES)
    for c in CL.ALL_CASES:
        assert len(set(c.sp)) == len(c.sp) == len(set(c.out_sp)), f"{c.name}: a square image"
    seams = [c for c in CL.CONV_CASES if (c.C0, c.C1) == (40, 24)]
    assert any(c.plan[0] == CL.IG for c in seams) and any(c.plan[0] != CL.IG for c in seams)
    assert any(c.seg2 == (40, 24) for c in CL.CONV_CASES)
    assert any(c.K == 136 and c.plan[1:3] == (128, 128) for c in CL.CONV_CASES)
    assert {c.plan[2] for c in CL.CONV_CASES if c.plan[0] == CL.IG} == {256, 128, 64, 32}
    assert {c.plan[3] for c in CL.CONV_CASES if c.plan[0] == CL.H9} == {16, 8, 4}
    assert any(c.plan[0] == CL.H8 for c in CL.CONV_CASES)


# ----------------------------------------------------------------------------------- the emulation and its mutants
EMULATED = ["ig_k64_k24_c24", "ig_k64_seam_40_24", "ig_s2_odd", "ig_up_pro", "ig_px64_split_reduce",
            "ig_k64_split_single_tail", "ig_t_s2_parity", "ig_t_s2_odd", "ig_t_s1", "ig_stats_k64",
            "ig_px128_k136_all_epilogues", "ig_out_f32", "ig_acc_bf16", "ig_t_s2_parity_stats"]


@pytest.mark.parametrize("name", EMULATED)
def test_emulation_is_bit_exact(name):
    """fp32 sums in a scrambled order, three partial slabs: the bits of the fp64 reference -- the exactness argument
    at work on the CPU.  Where the case has statistics: the flat 64-pixel rows against ``stats_expected``."""
    c = CL.BY_NAME[name]
    T = CL.generate(name)
    R = CL.reference(c, T)
    CL.conditions(c, T, R)
    for splits in (1, 3, 7):
        out, st = CL.emulate(c, T, splits=splits, stats_rows=64 if c.stats else 0)
        CL.assert_bits(out, CL.expected(c, R["out"]), R["out"], f"{name} emulated, {splits} slabs")
        if c.stats:
            want = CL.stats_expected(CL.expected(c, R["out"]), CL.stats_row_map(c, "flat", 64), c.K)
            assert torch.equal(st.double(), want)


def test_parity_row_map_partitions_each_image_by_class():
    """stats_row_map "parity" (csrc/conv.hip: rows image-major, class c the c-th share of an image's rows): every
    row holds 64 pixels of one image and one parity class, consecutive in class-raster order."""
    c = CL.BY_NAME["ig_t_s2_parity_stats"]
    rm = CL.stats_row_map(c, "parity", 64)
    Ho, Wo = c.out_sp
    m = torch.arange(rm.numel())
    n, y, x = m // (Ho * Wo), (m // Wo) % Ho, m % Wo
    assert torch.equal(torch.bincount(rm), torch.full((rm.numel() // 64,), 64))
    rpi = Ho * Wo // 64
    assert torch.equal(rm // rpi, n)
    cls = (rm % rpi) // (rpi // 4)
    assert torch.equal(cls, (y & 1) * 2 + (x & 1))
    q = (y // 2) * (Wo // 2) + x // 2
    assert torch.equal((rm % (rpi // 4)), q // 64)


def test_halo_row_map_is_four_tile_rows_by_sixteen_columns():
    c = CL.BY_NAME["h9_r4_c96_stats"]
    for th in (4, 8, 16):
        rm = CL.stats_row_map(c, "halo", 64, th)
        assert torch.equal(torch.bincount(rm), torch.full((rm.numel() // 64,), 64))
        Ho, Wo = c.out_sp
        img = rm.reshape(c.N, Ho, Wo)
        blk = img.reshape(c.N, Ho // 4, 4, Wo // 16, 16)
        assert (blk == blk[:, :, :1, :, :1]).all()           # constant on each 4 x 16 block
        assert img[0, 0, 0] == 0 and img[0, 0, 16] == th // 4   # the next tile to the right follows this tile's rows


MUTANT_CASE = {
    "hw_swap": "ig_k64_k24_c24", "pad_neighbour": "ig_k64_k24_c24", "seam_chunk_dropped": "ig_k64_seam_40_24",
    "tap_transposed": "ig_k64_k24_c24", "s2_odd_off_by_one": "ig_s2_odd", "up_ceil": "ig_up_pro",
    "truncate": "ig_k64_k24_c24", "bias_nc_image0": "ig_px64_split_reduce",
    "last_split_dropped": "ig_k64_split_single_tail", "split_twice": "ig_k64_split_single_tail",
    "parity_wrong": "ig_t_s2_parity", "stats_row_shift": "ig_stats_k64",
}


def _todays_check(c, T, mutant):
    """The assertion of tests/test_gpu_kernels.py: max|err| <= 1.5e-2 max|ref| (fp32 outputs: the same bound, which
    is looser than theirs), statistics at rtol 2e-3 / atol 2e-2 -- against the fp64 reference of the same operands."""
    R = CL.reference(c, T)["out"]
    out, st = CL.emulate(c, T, mutant=mutant, stats_rows=64 if c.stats else 0)
    ok = (out.double() - R).abs().max().item() <= 1.5e-2 * R.abs().max().item()
    if c.stats and ok:
        clean = CL.emulate(c, T, stats_rows=64)[1]
        ok = torch.allclose(st, clean, rtol=2e-3, atol=2e-2)
    return ok


def test_mutants():
    """No mutant survives the bit comparison on the lattice table's own (non-square) case; the table also records
    which of them today's assertion passes on today's inputs (white noise, square images)."""
    assert set(MUTANT_CASE) == set(CL.MUTANTS)
    survivors, passed_today = [], []
    print(f"\n{'mutant':22s} {'case':28s} {'1.5e-2 max, noise, square':26s} bit comparison, lattice, H != W")
    for mutant in CL.MUTANTS:
        c = CL.BY_NAME[MUTANT_CASE[mutant]]
        T = CL.generate(c.name)
        R = CL.reference(c, T)
        rows = 64 if c.stats else 0
        out, st = CL.emulate(c, T, mutant=mutant, stats_rows=rows)
        nbad = CL.mismatches(out, CL.expected(c, R["out"])).shape[0]
        if c.stats:
            want = CL.stats_expected(CL.expected(c, R["out"]), CL.stats_row_map(c, "flat", 64), c.K)
            nbad += int((st.double() != want).sum().item())
        today = all(_todays_check(*CL.white_noise(c, seed), mutant) for seed in (1, 2, 3))
        print(f"{mutant:22s} {c.name:28s} {'PASSES' if today else 'fails':26s} "
              f"{'PASSES' if nbad == 0 else f'fails ({nbad} elements)'}")
        if nbad == 0:
            survivors.append(mutant)
        if today:
            passed_today.append(mutant)
    print(f"today's assertion passes {len(passed_today)} of {len(CL.MUTANTS)}: {passed_today}; "
          f"the bit comparison passes {len(survivors)}")
    assert not survivors, survivors
    # the tolerance check is blind to the H/W swap (square images) and to truncation (4e-3 .. 6e-3 of max)
    assert "hw_swap" in passed_today and "truncate" in passed_today, passed_today


# ------------------------------------------------------- what the lattice cannot carry: the bounds of the SiLU cases
@pytest.mark.parametrize("c", CL.BOUND_CASES, ids=_ids(CL.BOUND_CASES))
def test_bound_cases_are_well_formed(c):
    """Non-square, a finite positive bound everywhere, and the flip set F small but not empty (so the G check of
    the halo kernel exercises both of its branches)."""
    assert len(set(c.sp)) == len(c.sp)
    T = CL.real_operands(c.name)
    for name, (ref, bound) in CL.bound_reference(c, T).items():
        assert torch.isfinite(ref).all() and torch.isfinite(bound).all() and (bound > 0).all(), (c.name, name)
        assert bound.max().item() < 1e-2 * ref.abs().max().item(), (c.name, name)   # tighter than the old tolerance
    if c.silu:
        frac = (CL.silu_operand(c, T)["delta"] > 0).double().mean().item()
        assert 0 < frac < 1e-2, (c.name, frac)   # the fold case: 6e-3 (the in-kernel a, b widen eps_t)


@pytest.mark.parametrize("name,mutant", [("b_ig_pro", "silu_without_shift"),
                                         ("b_ig_ep_two_source", "sigmoid_for_silu_grad")])
def test_bound_emulation_and_mutants(name, mutant):
    """The fp32 emulation is inside the bare bound (margin 1); the prologue mutant (SiLU without the affine shift)
    and the epilogue mutant (sigma for SiLU') are rejected at the margin the GPU test uses."""
    c = CL.BOUND_BY_NAME[name]
    T = CL.real_operands(name)
    ref, bound = CL.bound_reference(c, T)["out"]
    ratio = CL.check_bound(CL.emulate_bound_case(c, T), ref, bound, name, margin=1.0)
    print(f"{name}: emulation max err / bound {ratio:.3f}")
    with pytest.raises(AssertionError):
        CL.check_bound(CL.emulate_bound_case(c, T, mutant), ref, bound, f"{name} {mutant}")


def test_bf16_rne_rounds_fp64_once():
    """A value just off a bf16 tie, by less than half an fp32 ulp: torch's conversion through fp32 lands on the tie
    and rounds to even; bf16_rne rounds the fp64 value itself."""
    tie = 1.0 + 2.0 ** -8
    t = torch.tensor([tie + 2.0 ** -40, tie - 2.0 ** -40, tie, 3.0 + 2.0 ** -7 + 2.0 ** -39, -tie - 2.0 ** -40],
                     dtype=torch.float64)
    assert CL.bf16_rne(t).tolist() == [1.0 + 2.0 ** -7, 1.0, 1.0, 3.0 + 2.0 ** -6, -1.0 - 2.0 ** -7]
    assert t.to(torch.bfloat16).double().tolist()[0] == 1.0   # what the helper exists to avoid
    g = torch.Generator().manual_seed(5)
    r = torch.randn(100000, generator=g, dtype=torch.float64)
    assert torch.equal(CL.bf16_rne(r.float().double()), r.float().to(torch.bfloat16).double())


def test_gout_check_on_the_fp32_prologue():
    """check_gout on what fp32 arithmetic gives for G (torch's sigmoid): inside; without the shift b: rejected."""
    c = CL.BOUND_BY_NAME["b_h8_pro_gout"]
    T = CL.real_operands(c.name)
    S = CL.silu_operand(c, T)
    x = T["x0"].float()
    a, b = T["pro_a"][:, None, None, :], T["pro_b"][:, None, None, :]
    z = a * x + b
    assert 0 < CL.check_gout((z * torch.sigmoid(z)).to(torch.bfloat16), S, "fp32 G") < 5e-3
    with pytest.raises(AssertionError):
        CL.check_gout((a * x * torch.sigmoid(a * x)).to(torch.bfloat16), S, "G without b")


def test_fold_bound_holds_for_the_fp32_fold():
    """The in-kernel fold in fp32 torch arithmetic (fp32 row sums, fp64 group sums, fp32 rsqrt, a and b in fp32):
    a and b inside their derived bounds, the conv output inside the bare bound; a fold that forgets the mean term of
    b is rejected."""
    c = CL.BOUND_BY_NAME["b_h9_fold"]
    T = CL.real_operands(c.name)
    a, b, e_a, e_b = CL.fold_affine(c, T)
    Cg, cnt = c.C0 // c.fold, (c.C0 // c.fold) * c.sp[0] * c.sp[1]
    tot = T["slab"].reshape(c.N, -1, c.C0, 2).sum(1)
    g = tot.double().reshape(c.N, c.fold, Cg, 2).sum(2).repeat_interleave(Cg, dim=1)
    m = g[..., 0] / cnt
    v = (g[..., 1] / cnt - m * m).clamp(min=0)
    a32 = torch.rsqrt(v.float() + torch.tensor(CL.FOLD_EPS, dtype=torch.float32)) * T["gamma"]
    b32 = T["beta"] - m.float() * a32
    assert ((a32.double() - a).abs() <= e_a).all() and ((b32.double() - b).abs() <= e_b).all()
    ref, bound = CL.bound_reference(c, T)["out"]
    x = T["x0"].float()
    for mutant, bb in ((None, b32), ("b_without_mean", T["beta"].expand_as(b32))):
        z = a32[:, None, None, :] * x + bb[:, None, None, :]
        out = CL.emulate(CL._plain(c), T, z=(z * torch.sigmoid(z)).to(torch.bfloat16).float())[0]
        if mutant is None:
            print(f"b_h9_fold: emulation max err / bound {CL.check_bound(out, ref, bound, c.name, margin=1.0):.3f}")
        else:
            with pytest.raises(AssertionError):
                CL.check_bound(out, ref, bound, f"{c.name} {mutant}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_guarded_buffers_see_stray_and_missing_writes(dtype):
    """The sentinel-filled buffers of the GPU tests, on the CPU: a view fully written passes; one element left alone,
    a write just before the view, a write one image past it and a front guard overwritten with one value all show."""
    shape = (3, 5, 7, 24)
    buf, view = CL.guarded(shape, dtype, "cpu")
    assert torch.isnan(buf.float()).all() and CL.guards_intact(buf, view) and CL.unwritten(view) == view.numel()
    view.copy_(torch.ones(shape))
    assert CL.guards_intact(buf, view) and CL.unwritten(view) == 0
    guard = (buf.numel() - view.numel()) // 2
    assert guard >= max(1024, 5 * 7 * 24)
    for at in (guard - 1, guard + view.numel() + 5 * 7 * 24 - 1):
        b2 = buf.clone()
        b2[at] = 1.0
        assert not CL.guards_intact(b2, b2[guard:guard + view.numel()].view(shape))
    b2 = buf.clone()
    b2[:guard] = 2.0
    assert not CL.guards_intact(b2, b2[guard:guard + view.numel()].view(shape))
    buf2, v2 = CL.guarded(shape, dtype, "cpu", init=torch.zeros(shape))
    v2.view(-1)[1:] = 1.0
    assert CL.unwritten(v2) == 0   # init counts as written
    buf3, v3 = CL.guarded(shape, dtype, "cpu")
    v3.view(-1)[1:] = 1.0
    assert CL.unwritten(v3) == 1
