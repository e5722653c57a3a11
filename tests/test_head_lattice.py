"""The saturated-lattice checks of the output head (head_lattice.py), held on the CPU before any GPU run.

1. Every row meets the conditions of the exactness argument, and the table reaches every instance of head_fwd /
   head_dgrad / head_wgrad and every edge the rows name -- asserted from the rows' shapes with head.hip's own
   dispatch rules.
2. A plain-torch fp32 emulation that sums in an order no kernel uses passes the comparison functions of the GPU
   test on every row; each of its fourteen mutants fails them on the row that exists to catch it.  The table (-s)
   also records what the assertion in force so far, 1e-2 max|ref|, makes of each mutant on the same inputs.
3. The bound rows are well formed: the emulation inside the bare bound, two mutants outside 1.5 x.
"""
import pytest
import torch

import head_lattice as HL


def _ids(cases):
    return [c.name for c in cases]


def _rows(kern=None, nd=None):
    return [c for c in HL.CASES if (kern is None or c.kern == kern) and (nd is None or c.nd == nd)]


@pytest.mark.parametrize("c", HL.CASES, ids=_ids(HL.CASES))
def test_row_meets_the_conditions_and_the_emulation_is_bit_exact(c):
    T, R, E, prof = HL.problem(c.name)
    caps = ", ".join(f"{k} {v:.3g}" for k, v in prof["caps"].items())
    rnd = "" if prof["round"] is None else f"; dz {prof['round']:.1%} round, {prof['tie']:.1%} ties"
    print(f"[head-lattice] {c.name:24s} {HL.instance(c):22s} {HL.ntiles(c):5d} tiles; units: {caps}{rnd}")
    HL.check(c, HL.emulate(c, T), E, f"{c.name} emulated")


def test_table_reaches_every_instance():
    inst = {HL.instance(c) for c in HL.CASES}
    want = {f"head_fwd<{kt}, 1, {cg}>" for kt in (1, 2, 4, 8) for cg in (1, 4)}
    want |= {f"head_fwd<{kt}, 3, {cg}>" for kt in (1, 2) for cg in (1, 4)}
    for k in ("dgrad", "wgrad"):
        want |= {f"head_{k}<{kt}, 1>" for kt in (1, 2, 4, 8)} | {f"head_{k}<{kt}, 3>" for kt in (1, 2)}
    assert inst == want, (want - inst, inst - want)
    for c in HL.CASES:
        assert HL.shape_ok(c.N, c.D, c.H, c.W, c.C, c.K), c.name
    # masked rows: K = 3 (KT = 4) and a K in 5..7 (KT = 8) in every 2-D kernel
    for kern in ("fwd", "dgrad", "wgrad"):
        ks = {c.K for c in _rows(kern, 2)}
        assert ks >= {1, 2, 4, 8} and ks & {5, 6, 7}, (kern, ks)
    assert 3 in {c.K for c in _rows("fwd", 2)}
    # dgrad: every KT in a fine and a coarse 2-D row
    for lat in ("fine", "coarse"):
        assert {HL.kt_of(c.K) for c in _rows("dgrad", 2) if c.lattice == lat} == {1, 2, 4, 8}, lat


def test_table_reaches_the_forward_edges():
    B = HL.BY_NAME
    fwd = _rows("fwd")
    # CG = 1 with more than one round of chunks at C >= 128: needs 128 tiles
    c = B["f_cg1_128tiles_c128"]
    assert HL.ntiles(c) == 128 and c.C >= 128 and HL.chunk_groups(c) == 1 and HL.fwd_rounds(c) == 4
    c = B["f_cg1_c96"]
    assert HL.ntiles(c) < 128 and c.C < 4 * HL.CK and HL.chunk_groups(c) == 1 and HL.fwd_rounds(c) == 3
    c = B["f_cg4_c128"]
    assert HL.chunk_groups(c) == 4 and HL.fwd_rounds(c) == 1
    c = B["f_cg4_c160_k4"]
    assert HL.chunk_groups(c) == 4 and c.C // HL.CK == 5 and HL.fwd_rounds(c) == 2     # groups 1..3 idle in round 2
    c = B["f_cg4_c512_k8"]
    assert HL.chunk_groups(c) == 4 and HL.fwd_rounds(c) == 4 and c.K == 8
    assert any(not c.bias for c in fwd) and any(c.bias for c in fwd)
    # N = 3 with H != W both ways, in every kernel some non-square grid
    assert {(c.N, c.H, c.W) for c in fwd} >= {(3, 48, 16), (3, 16, 80)}
    for c in HL.CASES:
        assert c.H != c.W or HL.ntiles(c) >= 128, f"{c.name}: a square image"
    # 3-D: D = 1, 2, 5 and C = 64, 128 in all three kernels; CG = 4 in 3-D
    for kern in ("fwd", "dgrad", "wgrad"):
        r3 = _rows(kern, 3)
        assert {c.D for c in r3} >= {1, 2, 5} and {c.C for c in r3} >= {64, 128} and {c.K for c in r3} == {1, 2}, kern
        assert all((c.H, c.W) == (16, 32) for c in r3 if HL.ntiles(c) < 1000)
    assert any(c.nd == 3 and HL.chunk_groups(c) == 4 for c in fwd)


def test_table_reaches_the_backward_edges():
    B = HL.BY_NAME
    dg = _rows("dgrad", 2)
    assert {c.C for c in dg} >= {64, 160, 256}
    c = B["d_k2_fine_c160"]
    assert (c.C + 127) // 128 == 2 and c.C % 128 == 32      # block 1: channel groups 4..15 idle
    assert any(c.kpad for c in dg) and any(c.kpad for c in _rows("wgrad", 2))
    wg = _rows("wgrad")
    assert any(not c.db for c in wg)
    # per_split = 2 of slot_sum: 33 or more workgroups
    nwg, tpw, used, per_split = HL.wgrad_grid(B["w_40wg_per_split2"])
    assert (nwg, tpw, used, per_split) == (40, 1, 40, 2)
    # the benchmark's 8 x 256^2 head: 2048 tiles, 2 per workgroup -- the 1083-tile row runs the same tiles_per_wg
    bench = HL.case("bench", "wgrad", N=8, H=256, W=256, C=128, K=1)
    assert HL.ntiles(bench) == 2048 and HL.wgrad_grid(bench)[:2] == (1024, 2)
    c = B["w_1083_tiles"]
    nwg, tpw, used, per_split = HL.wgrad_grid(c)
    per_sample = (c.H // 16) * (c.W // 16)
    assert (HL.ntiles(c), per_sample, nwg, tpw, used, per_split) == (1083, 361, 1024, 2, 542, 32)
    assert (180 * tpw) // per_sample == 0 and (180 * tpw + 1) // per_sample == 1     # workgroup 180: samples 0 | 1
    assert min(HL.ntiles(c), 541 * tpw + tpw) - 541 * tpw == 1                        # workgroup 541: one tile
    assert 542 * tpw >= HL.ntiles(c) and nwg - used == 482                            # 542 .. 1023: none
    c = B["w3_1125_tiles"]
    nwg, tpw, used, _ = HL.wgrad_grid(c)
    per_slice = (c.H // 16) * (c.W // 16)
    assert (HL.ntiles(c), per_slice, nwg, tpw, used) == (1125, 225, 1024, 2, 563)
    assert (112 * tpw) // per_slice == 0 and (112 * tpw + 1) // per_slice == 1       # workgroup 112: slices 0 | 1


def test_row_map_partitions_every_image():
    """Every statistics row holds 64 pixels: rows 4q .. 4q + 3 and the 16 columns of one tile of one slice; rows are
    numbered tile-major with tiles running x, then y, then slice."""
    for c in (HL.BY_NAME["d_k2_coarse_n3"], HL.BY_NAME["d_k6_coarse_kpad"], HL.BY_NAME["d3_d5_k2_fine"]):
        rm = HL.row_map(c)
        S = c.N * max(c.D, 1)
        assert torch.equal(torch.bincount(rm), torch.full((S * c.H * c.W // 64,), 64))
        img = rm.reshape(S, c.H, c.W)
        blk = img.reshape(S, c.H // 4, 4, c.W // 16, 16)
        assert (blk == blk[:, :, :1, :, :1]).all()
        tiles = (c.H // 16) * (c.W // 16)
        assert torch.equal(img[:, 0, 0], torch.arange(S) * tiles * 4)
        if c.W > 16:
            assert img[0, 0, 16] == 4 and img[0, 4, 0] == 1
        if c.H > 16:
            assert img[0, 16, 0] == 4 * (c.W // 16)
        assert not torch.equal(HL.row_map(c, transposed=True), rm)


# ----------------------------------------------------------------------------------------------------- the mutants
MUTANT_ROW = {
    "pad_neighbour": "f_n3_48x16", "wrong_sample_affine": "f_k1", "depth_pad_wraps": "f3_d1_k1",
    "chunk_dropped": "f_cg4_c160_k4", "tap_transposed": "f_k3", "dgrad_tap_not_flipped": "d_k2_coarse_n3",
    "kpad_leak": "d_k6_coarse_kpad", "last_tile_dropped": "w_1083_tiles", "empty_slot_stale": "w_1083_tiles",
    "bias_every_depth_pass": "w3_d2_k2_c128", "overwrite_not_accumulate": "w_k1",
    "silu_grad_zero_is_one": "d_k1_coarse_c160", "stats_from_unrounded_dz": "d_k1_fine",
    "stats_row_transposed": "d_k1_coarse_c160",
}


def _old_assertion(c, got, E):
    """The assertion of tests/test_gpu_kernels.py on the same inputs: max|err| <= 1e-2 max|ref| per tensor, the
    statistics as per-sample sums at rtol 1e-4 / atol 1e-3 against sums of the kernel's own dz."""
    def close(a, ref):
        return (a.double() - ref).abs().max().item() <= 1e-2 * ref.abs().max().item()
    if c.kern == "fwd":
        return close(got["out"], E["out_ref"])
    if c.kern == "wgrad":
        return close(got["dw"], E["dw_ref"]) and (got["db"] is None or close(got["db"], E["db_ref"]))
    if not close(got["dz"], E["dz_ref"]):
        return False
    T = HL.generate(c.name)
    s = got["stats"].double().reshape(c.N, -1, c.C, 2).sum(1)
    dz, x = got["dz"].double().reshape(c.N, -1, c.C), T["x0"].double().reshape(c.N, -1, c.C)
    return (torch.allclose(s[..., 0], dz.sum(1), rtol=1e-4, atol=1e-3)
            and torch.allclose(s[..., 1], (dz * x).sum(1), rtol=1e-4, atol=1e-3))


def test_mutants():
    """No mutant survives the comparison functions of the GPU test on its row."""
    assert set(MUTANT_ROW) == set(HL.MUTANTS)
    survivors, old_passes = [], []
    print(f"\n{'mutant':26s} {'row':22s} {'1e-2 max|ref|':14s} lattice comparison")
    for mutant in HL.MUTANTS:
        c = HL.BY_NAME[MUTANT_ROW[mutant]]
        T, R, E, _ = HL.problem(c.name)
        got = HL.emulate(c, T, mutant)
        old = _old_assertion(c, got, E)
        try:
            HL.check(c, got, E, f"{c.name} {mutant}")
            caught, why = False, ""
        except AssertionError as e:
            caught, why = True, str(e).splitlines()[0]
        print(f"{mutant:26s} {c.name:22s} {'PASSES' if old else 'fails':14s} "
              f"{'fails: ' + why if caught else 'PASSES'}")
        if not caught:
            survivors.append(mutant)
        if old:
            old_passes.append(mutant)
    print(f"the old assertion passes {len(old_passes)} of {len(HL.MUTANTS)}: {old_passes}; "
          f"the lattice comparison passes {len(survivors)}")
    assert not survivors, survivors


# ------------------------------------------------------------------------------------------------- the bound rows
@pytest.mark.parametrize("c", HL.BOUND_CASES, ids=_ids(HL.BOUND_CASES))
def test_bound_rows_are_well_formed(c):
    """A finite positive bound everywhere, and the fp32 emulation inside 1.0 x it."""
    T = HL.real_operands(c.name)
    B = HL.bound_reference(c, T)
    for name, (ref, bound) in B.items():
        assert torch.isfinite(ref).all() and torch.isfinite(bound).all() and (bound > 0).all(), (c.name, name)
        print(f"[head-bounds] {c.name} {name}: max bound / max|ref| {bound.max().item() / ref.abs().max().item():.2e}")
    ratios = HL.check_bounds(c, HL.emulate(c, T), B, f"{c.name} emulated", margin=1.0)
    print(f"[head-bounds] {c.name} ({HL.instance(c)}): emulation max err / bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))


@pytest.mark.parametrize("name,mutant", [("b_fwd", "silu_without_shift"), ("b_dgrad", "sigmoid_for_silu_grad")])
def test_bound_mutants_are_rejected(name, mutant):
    assert mutant in HL.BOUND_MUTANTS
    c = HL.BOUND_BY_NAME[name]
    T = HL.real_operands(name)
    with pytest.raises(AssertionError):
        HL.check_bounds(c, HL.emulate(c, T, mutant), HL.bound_reference(c, T), f"{name} {mutant}")
