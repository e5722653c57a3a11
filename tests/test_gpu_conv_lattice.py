"""The convolution family on exact-lattice inputs (tests/conv_lattice.py; DESIGN.md section 4, "Convolutions: exact
lattice"): every row first asserts the kernel instance the library plans for it, then holds the output to the fp64
reference bit for bit -- bf16 outputs to its round-to-nearest-even, fp32 outputs (out_f32, dW, db) to the value
itself -- inside a sentinel-filled buffer, and the fused statistics to the fp64 sums of the expected output over
each slab row.  Non-square images throughout; no tolerance anywhere."""
import functools

import pytest
import torch

import conv_lattice as CL

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ops():
    from fmdiff.runtime import ops as O
    return O


@functools.lru_cache(maxsize=None)
def _problem(name):
    """(operands, fp64 reference) of a case, the conditions of the exactness argument asserted; computed once."""
    c = CL.BY_NAME[name]
    T = CL.generate(name)
    R = CL.reference(c, T)
    CL.conditions(c, T, R)
    return T, R


def _ids(cases):
    return [c.name for c in cases]


def _out_buffer(c, T):
    dtype = torch.float32 if c.out_f32 else CL.BF16
    return CL.guarded((c.N, *c.out_sp, c.K), dtype, DEV, T["old"].to(DEV) if c.acc else None)


def _check_out(c, buf, out, R):
    torch.cuda.synchronize()
    assert CL.guards_intact(buf, out), f"{c.name}: written outside the output"
    if not c.acc:
        assert CL.unwritten(out) == 0, f"{c.name}: {CL.unwritten(out)} output elements never written"
    CL.assert_bits(out, CL.expected(c, R["out"]), R["out"], c.name)


def _check_stats(c, st, R, kind, tile_rows=0, y=None):
    rowmap = CL.stats_row_map(c, kind, st.rows, tile_rows)
    want = CL.stats_expected(CL.expected(c, R["out"]), rowmap, c.K, y)
    got = st.slab.cpu().double()
    assert got.shape == want.shape, (c.name, got.shape, want.shape)
    bad = (got != want).nonzero()
    assert bad.shape[0] == 0, (f"{c.name}: {bad.shape[0]} of {got.numel()} statistics differ ({kind} rows of "
                               f"{st.rows}); first (row, k, which): "
                               + "; ".join(f"{tuple(i)}: {got[tuple(i)].item()} / {want[tuple(i)].item()}"
                                           for i in bad[:6].tolist()))


def _common_kw(c, t):
    kw = dict(src1=t.get("x1"), bias=t.get("bias"), bias_nc=t.get("bias_nc"), resid=t.get("resid"))
    if c.pro:
        kw["pro"] = (t["pro_a"], t["pro_b"], c.silu)
    return kw


def _launch_conv(c, T, monkeypatch):
    """ops.conv of a table row into guarded buffers; asserts the planned instance and the part count.  Returns
    (out buffer, out, statistics, plan, the keyword arguments)."""
    O = ops()
    from fmdiff import _lib
    from fmdiff.runtime import tuning
    L = _lib.lib()
    t = {k: v.to(DEV) for k, v in T.items()}
    wk = O.prep_weights(t["w"], {"fwd": 0, "dgrad": 1, "updgrad": 2}[c.mode])
    kw = dict(_common_kw(c, t), ks=c.ks, stride=c.stride, pad=c.pad, upsample=c.up, transposed=c.mode == "dgrad",
              out_hw_=c.out_sp, bias2=t.get("bias2"), out_f32=c.out_f32, accumulate=c.acc, want_stats=c.stats,
              splits=c.splits, force_generic=c.generic)
    if c.epx or c.epsilu:
        kw["ep"] = (t["ex0"], t.get("ex1"), t.get("ep_a"), t.get("ep_b"))
    if c.fold:   # the GroupNorm affine folded inside the launch from the statistics slab
        kw["pro_fold"] = dict(st0=O.Stats(t["slab"], CL.FOLD_ROWS), groups=c.fold, eps=CL.FOLD_EPS, gamma=t["gamma"],
                              beta=t["beta"], silu=True)
    if c.seg2:
        kw.update(src2=t["x2"], src3=t.get("x3"), wgt2=O.prep_weights(t["w2"], 0))
    if c.nd == 3 and c.plan[0] != CL.IG:   # depth taps as chunks: pre-tiled (kz, channel block) weights
        from fmdiff.runtime.engine import WeightCache
        kw["wgt_tiled"] = WeightCache().dtiled(t["w"], 0)
    gbuf = None
    if c.gout:
        gbuf, kw["gout"] = CL.guarded((c.N, *c.sp, c.C0 + c.C1), CL.BF16, DEV)
    if c.ticket:
        monkeypatch.setattr(O, "SPLIT_TICKET", True)
    buf, out = _out_buffer(c, T)
    plans = []
    try:
        if c.th8 is not None:
            assert L.fmd_halo_set_th8_max_workgroups(c.th8) == 0
        if c.th4 is not None:
            assert L.fmd_halo_set_th4_max_workgroups(c.th4) == 0
        got, st = O.conv(t["x0"], c.K, wk, out=out, plan_out=plans, **kw)
    finally:
        L.fmd_halo_set_th8_max_workgroups(tuning.get("HALO_TH8_MAX_WG"))
        L.fmd_halo_set_th4_max_workgroups(tuning.get("HALO_TH4_MAX_WG"))
    p, splits = plans
    plan = (p.kernel, p.bco, p.bpx, p.tile_rows, p.tickets, p.combine_launch, p.stats_rows, p.fold)
    assert plan == c.plan, f"{c.name}: planned {plan}, the row names {c.plan}"
    # the part count the row's K-step arithmetic rests on: as given (implicit GEMM) or as ops.halo_splits chooses
    if p.kernel == CL.IG:
        assert splits == c.splits, f"{c.name}: {splits} parts, the row names {c.splits}"
    else:
        imgs = c.N * (c.out_sp[0] if c.nd == 3 else 1)
        hs = O.halo_splits(imgs, *c.out_sp[-2:], c.K, c.C0 + c.C1, 3 if c.nd == 3 else 1)
        assert splits == hs == c.hsplits, f"{c.name}: {splits} parts (halo_splits {hs}), the row names {c.hsplits}"
    assert got.data_ptr() == out.data_ptr()
    if c.gout:
        kw["gbuf"] = gbuf
    return buf, out, st, p, kw


@pytest.mark.parametrize("c", CL.CONV_CASES, ids=_ids(CL.CONV_CASES))
def test_fmd_conv(c, monkeypatch):
    """fmd_conv through ops.conv: the implicit-GEMM instances and the halo kernels."""
    T, R = _problem(c.name)
    buf, out, st, p, kw = _launch_conv(c, T, monkeypatch)
    _check_out(c, buf, out, R)
    if c.stats:
        assert st is not None and st.rows == p.stats_rows
        par = c.mode == "dgrad" and c.stride == 2 and all(s % 2 == 0 for s in c.out_sp)
        kind = "parity" if par else "flat" if (p.kernel == CL.IG or p.combine_launch) else "halo"
        _check_stats(c, st, R, kind, p.tile_rows, CL.ep_tensor(T))
    if c.gout:
        assert CL.guards_intact(kw["gbuf"], kw["gout"]) and CL.unwritten(kw["gout"]) == 0
        z = CL.prologue(c, T).movedim(1, -1).contiguous()
        CL.assert_bits(kw["gout"], z.to(CL.BF16), z, f"{c.name} gout")


@pytest.mark.parametrize("c", CL.S2D_CASES, ids=_ids(CL.S2D_CASES))
def test_fmd_conv_s2d_d2s(c):
    """fmd_conv_s2d (3x3 stride 2, the 4x4 nearest-x2 data gradient) and fmd_conv_d2s, at the smallest N x tiles
    that gives the kernels' 128 workgroups."""
    O = ops()
    T, R = _problem(c.name)
    t = {k: v.to(DEV) for k, v in T.items()}
    d3 = c.nd == 3
    Ds, Do = (c.sp[0], c.out_sp[0]) if d3 else (0, 0)
    (Hs, Ws), (Ho, Wo) = c.sp[-2:], c.out_sp[-2:]
    if c.op == "d2s":
        assert O.d2s_eligible(c.N, Hs, Ws, Ho, Wo, c.K, c.C0, Ds, Do)
        tiles = c.N * max(Ds, 1) * (Hs // 16) * (Ws // 16) * (8 if d3 else 4) * (c.K // 128)
    else:
        assert O.s2d_eligible(c.N, Hs, Ws, Ho, Wo, c.K, c.C0, c.ks, Ds, Do)
        tiles = c.N * max(Do, 1) * (Ho // 16) * (Wo // 16) * (c.K // 128)
    assert tiles == 128, (c.name, tiles)
    tiled = O.s2d_tile_weights(t["w"], {"fwd": 0, "updgrad": 1, "dgrad": 2}[c.mode])
    buf, out = _out_buffer(c, T)
    kw = _common_kw(c, t)
    del kw["bias_nc"], kw["resid"], kw["src1"]
    got, st = O.conv(t["x0"], c.K, None, ks=c.ks, stride=2, pad=1, transposed=c.mode == "dgrad", out_hw_=c.out_sp,
                     out=out, accumulate=c.acc, want_stats=c.stats, s2d_tiled=tiled, **kw)
    assert got.data_ptr() == out.data_ptr()
    _check_out(c, buf, out, R)
    if c.stats:
        assert st is not None and st.rows == 64
        _check_stats(c, st, R, "halo", c.tile_rows)   # 128 workgroups: a one-round grid runs 8-row tiles


@pytest.mark.parametrize("c", CL.SMALL_CASES, ids=_ids(CL.SMALL_CASES))
def test_fmd_conv_small(c):
    """fmd_conv_small in its modes without GroupNorm (s2, up), unsplit and at the plan's own part count."""
    O = ops()
    T, R = _problem(c.name)
    t = {k: v.to(DEV) for k, v in T.items()}
    shape0 = tuple(T["x0"].shape)
    assert O.conv_small_ok(shape0, c.K, C1=c.C1, mode=c.smode, split=c.split)
    parts = O.conv_small_split(shape0, c.K, C1=c.C1, mode=c.smode, split=c.split)
    assert (parts == 1) if c.split == 1 else (parts > 1), (c.name, parts)
    buf, out = _out_buffer(c, T)
    got, st = O.conv_small(t["x0"], c.K, O.prep_weights(t["w"], 0), mode=c.smode, out=out, want_stats=c.stats,
                           split=c.split, **_common_kw(c, t))
    _check_out(c, buf, out, R)
    if c.stats:
        _check_stats(c, st, R, "flat")


def _wgrad_args(c, T):
    """Positional and keyword arguments of ops.wgrad / ops.wgrad_job with guarded dW / db buffers."""
    t = {k: v.to(DEV) for k, v in T.items()}
    Ct = c.C0 + c.C1
    dwb, dw = CL.guarded((c.K, Ct, *(c.ks,) * c.nd), torch.float32, DEV, t.get("dw0"))
    dbb, db = CL.guarded((c.K,), torch.float32, DEV, t.get("db0"))
    dy, off = t["dy"], c.dy_wide
    if off:   # dY is channels [off, off + K) of a wider tensor whose other channels hold lattice values too
        wide = torch.full((*dy.shape[:-1], c.K + 2 * off), 0.75, dtype=CL.BF16, device=DEV)
        wide[..., off:off + c.K] = dy
        dy = wide
    kw = dict(src1=t.get("x1"), ks=c.ks, stride=c.stride, pad=c.pad, upsample=c.up, db=db, accumulate=c.acc,
              dy_offset=off, force_generic=c.generic, pro=(t["pro_a"], t["pro_b"], c.silu) if c.pro else None)
    return (t["x0"], dy, dw), kw, (dwb, dbb)


def _check_wgrad(c, pos, kw, bufs, R, what):
    torch.cuda.synchronize()
    assert CL.guards_intact(bufs[0], pos[2]) and CL.guards_intact(bufs[1], kw["db"]), f"{what}: written outside dW / db"
    if not c.acc:
        assert CL.unwritten(pos[2]) == 0 and CL.unwritten(kw["db"]) == 0, f"{what}: dW / db not fully written"
    CL.assert_bits(pos[2], R["dw"].float(), R["dw"], f"{what} dW")
    CL.assert_bits(kw["db"], R["db"].float(), R["db"], f"{what} db")


@pytest.mark.parametrize("c", CL.WGRAD_CASES, ids=_ids(CL.WGRAD_CASES))
def test_fmd_wgrad(c):
    """ops.wgrad: dW and db are fp32 and equal the fp64 reference outright, at every split count."""
    O = ops()
    T, R = _problem(c.name)
    pos, kw, bufs = _wgrad_args(c, T)
    assert O.wgrad_job(*pos, **kw).shape.halo == c.halo, f"{c.name}: not the kernel the row names"
    O.wgrad(*pos, splits=c.splits, **kw)
    _check_wgrad(c, pos, kw, bufs, R, c.name)


def test_fmd_wgrad_group():
    """One fmd_wgrad_group launch of three jobs with unequal splits: each job equals its fp64 reference."""
    O = ops()
    rows = CL.group_cases()
    args = [_wgrad_args(c, _problem(c.name)[0]) for c, _ in rows]
    jobs = [O.wgrad_job(*pos, **kw) for pos, kw, _ in args]
    assert len({j.shape.key for j in jobs}) == 1
    O.wgrad_group(jobs, [s for _, s in rows])
    for (c, s), (pos, kw, bufs) in zip(rows, args):
        _check_wgrad(c, pos, kw, bufs, _problem(c.name)[1], f"{c.name} grouped with {s} splits")


# ------------------------------------------------------------------ SiLU prologue, SiLU' epilogue: elementwise bounds
@functools.lru_cache(maxsize=None)
def _bound_problem(name):
    T = CL.real_operands(name)
    return T, CL.bound_reference(CL.BOUND_BY_NAME[name], T)


@pytest.mark.parametrize("c", CL.BOUND_CASES, ids=_ids(CL.BOUND_CASES))
def test_silu_prologue_and_epilogue_bounds(c, monkeypatch):
    """pro = (a, b, True) and ep = (x, x1, a, b) on every kernel that implements them, against the fp64 reference
    with the MFMA operand rounded where the kernel rounds it, within 1.5 x the elementwise bound of conv_lattice.py
    (derived from csrc/common.h, not tuned); the halo kernel's G side output is checked directly."""
    O = ops()
    T, B = _bound_problem(c.name)
    ratios = {}
    if c.op == "wgrad":
        pos, kw, bufs = _wgrad_args(c, T)
        assert O.wgrad_job(*pos, **kw).shape.halo == c.halo
        O.wgrad(*pos, splits=c.splits, **kw)
        torch.cuda.synchronize()
        assert CL.guards_intact(bufs[0], pos[2]) and CL.guards_intact(bufs[1], kw["db"])
        ratios["dw"] = CL.check_bound(pos[2], *B["dw"], f"{c.name} dW")
        ratios["db"] = CL.check_bound(kw["db"], *B["db"], f"{c.name} db")
    elif c.op == "s2d":
        t = {k: v.to(DEV) for k, v in T.items()}
        (Hs, Ws), (Ho, Wo) = c.sp, c.out_sp
        assert O.s2d_eligible(c.N, Hs, Ws, Ho, Wo, c.K, c.C0, c.ks)
        buf, out = _out_buffer(c, T)
        O.conv(t["x0"], c.K, None, ks=3, stride=2, pad=1, out=out, bias=t["bias"],
               pro=(t["pro_a"], t["pro_b"], True), s2d_tiled=O.s2d_tile_weights(t["w"], 0))
        torch.cuda.synchronize()
        assert CL.guards_intact(buf, out) and CL.unwritten(out) == 0
        ratios["out"] = CL.check_bound(out, *B["out"], c.name)
    else:
        buf, out, _, _, kw = _launch_conv(c, T, monkeypatch)
        torch.cuda.synchronize()
        assert CL.guards_intact(buf, out) and CL.unwritten(out) == 0
        ratios["out"] = CL.check_bound(out, *B["out"], c.name)
        if c.gout:
            assert CL.guards_intact(kw["gbuf"], kw["gout"]) and CL.unwritten(kw["gout"]) == 0
            ratios["F"] = CL.check_gout(kw["gout"], CL.silu_operand(c, T), f"{c.name} gout")
    over = " -- ABOVE THE BARE BOUND: a finding" if max(v for k, v in ratios.items() if k != "F") > 1 else ""
    print(f"[conv-bounds] {c.name} ({c.inst}): max err / bound " +
          ", ".join(f"{k} {v:.3f}" if k != "F" else f"fraction of G in F {v:.2e}" for k, v in ratios.items()) + over)
