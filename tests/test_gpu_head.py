"""The output head (csrc/head.hip) on saturated-lattice inputs (tests/head_lattice.py; DESIGN.md section 4, "Output
head: saturated lattice").  The premise test comes first: SiLU saturates exactly in fp32 on the device.  Every row
then asserts the conditions of the exactness argument and holds out, dW and db to the fp64 reference bit for bit,
dz to its round-to-nearest-even, the statistics to the fp64 sums of the expected dz per slab row (fine rows: within
70 u of the row's sum of |terms|) -- all inside sentinel-filled buffers.  The bound rows hold what the lattice leaves
out (SiLU not saturated) to elementwise bounds; the last test holds that a refused shape launches nothing."""
import pytest
import torch

import head_lattice as HL

pytestmark = pytest.mark.gpu
DEV = "cuda"
PREMISE = ("(the exactness argument rests on test_saturation_premise: if that test fails too, this row shows the "
           "premise and not the kernel's indexing)")


def ops():
    from fmdiff.runtime import ops as O
    return O


def _ids(cases):
    return [c.name for c in cases]


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == HL.BF16 else torch.int32)


# ------------------------------------------------------------------------------------------------------ the premise
def test_saturation_premise():
    """One-hot weights (centre tap, one channel per output), no bias: head_fwd must return t = SiLU(a x + b) itself,
    which for every saturated z under every a is z (z >= 32) or 0, bit for bit; head_dgrad with dpred = 1 and unit
    centre weights must return SiLU'(z) = 1, 0.5 or -0.  Derived from IEEE rounding of rcp(1 + exp(-z)): the
    exponential underflows against 1, the reciprocal of 1.0 is 1.0, the exponential overflows to infinity."""
    O = ops()
    N, H, W, C = 4, 16, 16, 32
    sat = torch.tensor(HL.SAT, dtype=torch.float64)
    pix = torch.arange(H * W).reshape(1, H, W, 1)
    ch = torch.arange(C).reshape(1, 1, 1, C)
    z = sat[(pix + ch) % len(HL.SAT)].expand(N, H, W, C)
    a = torch.tensor(HL.PRO_A, dtype=torch.float64).reshape(N, 1).expand(N, C)            # every a: one per sample
    b = (2.0 * ((torch.arange(C) % 9) - 4)).double().reshape(1, C).expand(N, C)           # every even b in [-8, 8]
    x = ((z - b[:, None, None, :]) / a[:, None, None, :]).to(HL.BF16)
    assert torch.equal(a[:, None, None, :] * x.double() + b[:, None, None, :], z)
    xd, pro = x.to(DEV), (a.float().contiguous().to(DEV), b.float().contiguous().to(DEV))
    t = torch.where(z > 0, z, torch.zeros_like(z))
    for c0 in (0, 8):
        w = torch.zeros(8, C, 3, 3)
        w[torch.arange(8), c0 + torch.arange(8), 1, 1] = 1.0
        out = O.head_fwd(xd, pro, w.to(DEV), None, 8).cpu()
        want = t[..., c0:c0 + 8]
        seen = {zv: sorted(set(out[z[..., c0:c0 + 8] == zv].tolist())) for zv in HL.SAT}
        try:
            HL.assert_bits(out, want.float(), want, f"SiLU(z) through head_fwd, channels {c0}..{c0 + 7}")
        except AssertionError as e:
            raise AssertionError(f"{e}\nobserved t per saturated z: {seen}") from None
    w = torch.zeros(1, C, 3, 3)
    w[0, :, 1, 1] = 1.0
    dp = torch.zeros(N, H, W, 8, dtype=HL.BF16)
    dp[..., 0] = 1.0
    dz, st = O.head_dgrad(dp.to(DEV), w.to(DEV), 1, xd, pro)
    g = torch.where(z >= 32, 1.0, torch.where(z == 0, 0.5, -0.0)).double()
    dz = dz.cpu()
    seen = {zv: sorted(set(dz[z == zv].float().tolist())) for zv in HL.SAT}
    try:
        HL.assert_bits(dz, g.to(HL.BF16), g, "SiLU'(z) through head_dgrad")
    except AssertionError as e:
        raise AssertionError(f"{e}\nobserved SiLU' per saturated z: {seen}") from None


# ------------------------------------------------------------------------------------------------- the lattice rows
def _launch(c, T):
    """The row's kernel through ops.head_* into guarded buffers, synchronised, guards and sentinels checked:
    {name: output view}."""
    O = ops()
    t = {k: v.to(DEV) for k, v in T.items()}
    pro = (t["pro_a"], t["pro_b"])
    G = {}
    if c.kern == "fwd":
        G["out"] = HL.guarded((c.N, *c.sp, 8), torch.float32, DEV)
        got = O.head_fwd(t["x0"], pro, t["w"], t.get("bias"), c.K, out=G["out"][1])
        assert got.data_ptr() == G["out"][1].data_ptr()
    elif c.kern == "wgrad":
        G["dw"] = HL.guarded((c.K, c.C, *(3,) * c.nd), torch.float32, DEV, t["dw0"])
        if c.db:
            G["db"] = HL.guarded((c.K,), torch.float32, DEV, t["db0"])
        # ops.head_wgrad takes its workspace from the caching allocator: leave a block of that size full of NaN
        # there, so that a slot the kernel does not write (a workgroup without a tile) cannot read as zero by luck
        from fmdiff import _lib
        n = int(_lib.lib().fmd_head_wgrad_workspace(c.N, c.D, c.H, c.W, c.C, c.K))
        dirty = torch.full((n,), float("nan"), device=DEV)
        torch.cuda.synchronize()
        del dirty
        O.head_wgrad(t["dpred"], c.K, t["x0"], pro, G["dw"][1], G["db"][1] if c.db else None)
    else:
        G["dz"] = HL.guarded((c.N, *c.sp, c.C), HL.BF16, DEV)
        G["stats"] = HL.guarded((c.N * max(c.D, 1) * c.H * c.W // 64, c.C, 2), torch.float32, DEV)
        dz, st = O.head_dgrad(t["dpred"], t["w"], c.K, t["x0"], pro, out=(G["dz"][1], G["stats"][1]))
        assert st.rows == 64 and st.slab.data_ptr() == G["stats"][1].data_ptr()
    torch.cuda.synchronize()
    for k, (buf, view) in G.items():
        assert HL.guards_intact(buf, view), f"{c.name}: written outside {k}"
        assert HL.unwritten(view) == 0, f"{c.name}: {HL.unwritten(view)} elements of {k} never written"
    return {k: v[1] for k, v in G.items()}


@pytest.mark.parametrize("c", HL.CASES, ids=_ids(HL.CASES))
def test_head_lattice_row(c):
    T, R, E, _ = HL.problem(c.name)     # asserts the conditions before anything is compared
    got = _launch(c, T)
    try:
        HL.check(c, got, E, f"{c.name} ({HL.instance(c)})")
    except AssertionError as e:
        raise AssertionError(f"{e}\n{PREMISE}") from None


@pytest.mark.parametrize("name", ["f_cg4_c160_k4", "f_cg1_128tiles_c128", "d_k8_fine", "d3_d5_k2_fine", "w_1083_tiles",
                                  "w_40wg_per_split2", "w3_d5_k2"])
def test_second_call_returns_the_same_bits(name):
    c = HL.BY_NAME[name]
    T = HL.generate(name)
    first, second = _launch(c, T), _launch(c, T)
    for k in first:
        assert torch.equal(_bits(first[k]), _bits(second[k])), f"{name}: {k} differs between two calls"


# --------------------------------------------------------------------------------------------------- the bound rows
@pytest.mark.parametrize("c", HL.BOUND_CASES, ids=_ids(HL.BOUND_CASES))
def test_head_bounds(c):
    """Real-valued inputs, SiLU not saturated: every element within 1.5 x the bound of head_lattice.py (derived from
    csrc/common.h and the kernels' summation lengths, not tuned)."""
    T = HL.real_operands(c.name)
    B = HL.bound_reference(c, T)
    ratios = HL.check_bounds(c, _launch(c, T), B, c.name)
    over = " -- ABOVE THE BARE BOUND: a finding" if max(ratios.values()) > 1 else ""
    print(f"[head-bounds] {c.name} ({HL.instance(c)}): max err / bound " +
          ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) + over)


# ------------------------------------------------------------------------------------------------- refused shapes
REFUSED = [("H24", dict(H=24)), ("C48", dict(C=48)), ("K9", dict(K=9)), ("3d_K3", dict(D=2, H=16, W=32, K=3))]


@pytest.mark.parametrize("kern", ["fwd", "dgrad", "wgrad"])
@pytest.mark.parametrize("what,over", REFUSED, ids=[r[0] for r in REFUSED])
def test_refused_shape_raises_and_launches_nothing(what, over, kern):
    O = ops()
    c = HL.case(what, kern, **over)
    assert not HL.shape_ok(c.N, c.D, c.H, c.W, c.C, c.K)
    x = torch.zeros(c.N, *c.sp, c.C, dtype=HL.BF16, device=DEV)
    pro = (torch.ones(c.N, c.C, device=DEV), torch.zeros(c.N, c.C, device=DEV))
    w = torch.zeros(c.K, c.C, *(3,) * c.nd, device=DEV)
    dp = torch.ones(c.N, *c.sp, 8, dtype=HL.BF16, device=DEV)
    if kern == "fwd":
        G = [HL.guarded((c.N, *c.sp, 8), torch.float32, DEV)]
        with pytest.raises(RuntimeError):
            O.head_fwd(x, pro, w, torch.zeros(c.K, device=DEV), c.K, out=G[0][1])
    elif kern == "dgrad":
        G = [HL.guarded((c.N, *c.sp, c.C), HL.BF16, DEV),
             HL.guarded((max(c.N * max(c.D, 1) * c.H * c.W // 64, 1), c.C, 2), torch.float32, DEV)]
        with pytest.raises(RuntimeError):
            O.head_dgrad(dp, w, c.K, x, pro, out=(G[0][1], G[1][1]))
    else:
        G = [HL.guarded(tuple(w.shape), torch.float32, DEV), HL.guarded((c.K,), torch.float32, DEV)]
        with pytest.raises(RuntimeError):
            O.head_wgrad(dp, c.K, x, pro, G[0][1], G[1][1])
    torch.cuda.synchronize()
    for buf, view in G:
        assert HL.guards_intact(buf, view) and HL.unwritten(view) == view.numel(), f"{what} {kern}: output touched"
