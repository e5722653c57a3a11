"""fmd_conv_plan (csrc/conv.hip conv_decide): the host-side decision fmd_conv launches by -- kernel family and
instance, whether a split is combined inside the launch, the statistics rows, whether the GroupNorm fold is taken --
queried on descriptors alone (no GPU, placeholder pointers: the plan reads only which pointers are set), and the
Python predicates that must agree with it ahead of time (ops.halo_eligible / halo_splits, ops.igemm_split_tile)."""
import ctypes as C
import itertools

import pytest

from fmdiff import _lib
from fmdiff.runtime import ops, tuning

PTR = 64   # a non-NULL placeholder
HALO, IGEMM, STATS = _lib.CONV_TICKET_HALO, _lib.CONV_TICKET_IGEMM, _lib.CONV_WANT_STATS


@pytest.fixture(scope="module")
def L():
    import os
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfmdiff_hip.so not built (run __graft_entry__.build())")
    try:
        return _lib.lib()
    except OSError as e:   # HIP runtime absent on this host
        pytest.skip(f"HIP runtime not loadable here: {e}")


def desc(N, H, C, K, splits=1, *, tiled=True, up=False, pro=False, D=0, ks=3, stride=1, pad=1, transposed=False,
         Ho=None, **kw):
    """A conv descriptor with H x H (x D) stored input; ``tiled``: halo-tiled weights beside the plain ones."""
    d = _lib.ConvDesc()
    Ho = Ho if Ho is not None else (2 * H if up else H)
    d.N, d.Hs, d.Ws, d.C0, d.Ho, d.Wo, d.K = N, H, H, C, Ho, Ho, K
    d.Ds, d.Do = D, (2 * D if up else D)
    d.ks, d.stride, d.pad, d.upsample, d.transposed = ks, stride, pad, int(up), int(transposed)
    d.src0, d.wgt, d.out = PTR, PTR, PTR
    if tiled:
        d.wgt_tiled = PTR
    if pro:
        d.pro_a, d.pro_b, d.pro_silu = PTR, PTR, 1
    d.splits = splits
    if splits > 1:
        d.ws, d.n_tickets = PTR, ops.SMALL_TICKETS
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def fold(d, rows=64, G=32):
    d.fold_st0, d.fold_rows0, d.fold_G, d.fold_eps, d.pro_silu = PTR, rows, G, 1e-5, 1
    return d


def plan(L, d, allow):
    p = _lib.ConvPlan()
    assert L.fmd_conv_plan(C.byref(d), allow, C.byref(p)) == 0
    return p


def test_ticket_and_rows_decision(L):
    """Which split-K convs combine inside their launch and the statistics rows they then write.  The halo kernel on
    whole 128-cout tiles with 64-pixel rows, never with a G side output, a residual + data-gradient epilogue, 3-D or
    fp32 / accumulating outputs; the implicit GEMM (only when allowed: SPLIT_TICKET) on whole tiles without parity
    classes, one row per wave."""
    def tk(d, allow=HALO):
        p = plan(L, d, allow | STATS)
        return (bool(p.tickets), p.stats_rows) if p.tickets else (False, 0)

    latent = dict(N=8, H=32, C=128, K=128)                       # latent 32^2 ResBlock conv: M = 8192
    p = plan(L, desc(**latent, splits=2), HALO | STATS)
    assert (p.kernel, p.tickets, p.combine_launch, p.stats_rows) == (_lib.CONV_HALO9, 1, 0, 64)
    p = plan(L, desc(**latent, splits=1), HALO | STATS)          # unsplit: nothing to combine
    assert (p.kernel, p.tickets, p.combine_launch, p.stats_rows) == (_lib.CONV_HALO9, 0, 0, 64)
    p = plan(L, desc(8, 32, 128, 64, splits=2), HALO | STATS)    # partial 128-cout tile
    assert (p.kernel, p.tickets, p.combine_launch, p.stats_rows) == (_lib.CONV_HALO9, 0, 1, 16)
    p = plan(L, desc(**latent, splits=2, pro=True, gout=PTR), HALO)   # G side output (the round-3 kernel)
    assert (p.kernel, p.tickets, p.combine_launch) == (_lib.CONV_HALO8, 0, 1)
    assert tk(desc(**latent, splits=2, resid=PTR, ep_x0=PTR))[0] is False
    p = plan(L, desc(1, 32, 128, 128, splits=2, D=8), HALO | STATS)   # 3-D
    assert (p.kernel, p.tickets, p.combine_launch, p.stats_rows) == (_lib.CONV_HALO9, 0, 1, 16)
    assert tk(desc(8, 32, 128, 256, splits=4, out_f32=1))[0] is False
    assert tk(desc(8, 32, 128, 256, splits=4, accumulate=1))[0] is False
    gemm = dict(N=8, H=16, C=256, K=256, tiled=False)            # M = 2048 on the implicit GEMM
    assert tk(desc(**gemm, splits=16))[0] is False                # implicit GEMM: not allowed by default
    p = plan(L, desc(**gemm, splits=16), HALO | IGEMM | STATS)
    assert (p.kernel, p.bco, p.bpx, p.tickets, p.combine_launch, p.stats_rows) == (_lib.CONV_IGEMM, 128, 64, 1, 0, 32)
    assert tk(desc(8, 16, 256, 64, splits=4, tiled=False), HALO | IGEMM) == (True, 64)   # 128-pixel tiles, 2 waves
    assert tk(desc(4, 32, 64, 16, splits=4, tiled=False), HALO | IGEMM) == (True, 64)    # K <= 16: 4 waves x 256
    assert tk(desc(5, 20, 256, 256, splits=8, tiled=False), HALO | IGEMM)[0] is False    # M = 2000: ragged tile
    par = desc(2, 16, 256, 256, splits=8, tiled=False, transposed=True, stride=2, Ho=32)   # parity classes
    assert tk(par, HALO | IGEMM)[0] is False
    assert tk(desc(**gemm, splits=8, transposed=True), HALO | IGEMM)[0] is True
    assert tk(desc(1, 16, 256, 256, splits=8, tiled=False, D=8), HALO | IGEMM)[0] is False   # 3-D
    assert tk(desc(**latent, splits=2), 0)[0] is False            # HALO_TICKET off
    assert tk(desc(**latent, splits=2), IGEMM)[0] is False        # a ticket for the implicit GEMM alone: the halo
    assert plan(L, desc(**latent, splits=2), IGEMM).kernel == _lib.CONV_HALO9   # kernel runs it without


def test_declined_offers_settle_on_a_runnable_form(L):
    """A declined ticket is dropped before the fold, a declined fold comes back as pro_a / pro_b, and a ticket offered
    to the halo kernel alone never lands on the implicit GEMM."""
    small = dict(N=8, H=16, C=256, K=128, splits=4)   # 8 tiles x 4 splits, the smallest halo-eligible split problem
    p = plan(L, fold(desc(**small)), HALO | STATS)
    assert (p.kernel, p.tile_rows, p.tickets, p.fold, p.stats_rows) == (_lib.CONV_HALO9, 4, 1, 1, 64)
    try:
        assert L.fmd_halo_set_th8_max_workgroups(0) == 0   # 16-row tiles only: no in-launch combine
        for allow in (HALO, HALO | IGEMM):
            p = plan(L, desc(**small), allow | STATS)
            assert (p.kernel, p.tile_rows) == (_lib.CONV_HALO9, 16)
            assert (p.tickets, p.combine_launch, p.stats_rows, p.fold) == (0, 1, ops.SPLIT_STATS_ROWS, 0)
            p = plan(L, fold(desc(**small)), allow | STATS)
            assert (p.kernel, p.tile_rows) == (_lib.CONV_HALO9, 16)
            assert (p.tickets, p.combine_launch, p.stats_rows, p.fold) == (0, 1, ops.SPLIT_STATS_ROWS, 1)
    finally:
        L.fmd_halo_set_th8_max_workgroups(tuning.get("HALO_TH8_MAX_WG"))
    p = plan(L, desc(**small, n_tickets=31), HALO | STATS)   # 8 images x 4 four-row tiles need 32 counters
    assert (p.kernel, p.tickets, p.combine_launch, p.stats_rows) == (_lib.CONV_HALO9, 0, 1, ops.SPLIT_STATS_ROWS)
    assert plan(L, desc(**small, n_tickets=32), HALO | STATS).tickets == 1
    p = plan(L, fold(desc(**small, force_generic=1)), HALO | IGEMM | STATS)
    assert (p.kernel, p.fold, p.tickets) == (_lib.CONV_IGEMM, 0, 1)
    p = plan(L, fold(desc(**small, force_generic=1)), HALO | STATS)
    assert (p.kernel, p.fold, p.tickets, p.combine_launch) == (_lib.CONV_IGEMM, 0, 0, 1)
    # a fold the v9b kernel cannot take (partial cout tile, unsplit) comes back as pro_a / pro_b on the round-3 kernel
    p = plan(L, fold(desc(8, 64, 128, 64)), HALO | STATS)
    assert (p.kernel, p.fold, p.stats_rows) == (_lib.CONV_HALO8, 0, 64)
    # a descriptor no kernel runs: only halo tiles, but not a halo problem
    d = desc(1, 8, 128, 128)
    d.wgt = None
    assert L.fmd_conv_plan(C.byref(d), 0, C.byref(_lib.ConvPlan())) == -8


SWEEP_3D = [(1, 8, 32, 128, 128), (1, 8, 16, 256, 256), (2, 8, 64, 32, 64), (1, 8, 128, 32, 16), (1, 8, 16, 1024, 512)]


def test_python_predicates_agree_with_the_plan(L):
    """ops.halo_eligible / halo_splits choose weight layouts and split counts before any descriptor exists, and
    ops.igemm_split_tile sizes the implicit GEMM's split: both must say what the library decides."""
    bad = []
    cases = [(N, 0, H, Cin, K) for N, H, Cin, K in itertools.product(
        (1, 2, 8), (1, 4, 8, 16, 32, 64, 128, 256), (8, 32, 128, 256, 512, 1024), (8, 16, 64, 128, 192, 256, 512))]
    for (N, D, H, Cin, K), up, pro in itertools.product(cases + SWEEP_3D, (False, True), (False, True)):
        if up and H % 2:
            continue
        Hs, Ds = (H // 2, D // 2) if up else (H, D)
        imgs, zt = N * max(D, 1), 3 if D else 1
        # the halo family: tiled weights and the halo split count
        sp = ops.halo_splits(imgs, H, H, K, Cin, zt)
        want = ops.halo_eligible(imgs, Hs, H, H, K, upsample=up, Cin=Cin, pro=pro, ztaps=zt)
        p = plan(L, desc(N, Hs, Cin, K, splits=sp, up=up, pro=pro, D=Ds), HALO | STATS)
        if want != (p.kernel in (_lib.CONV_HALO8, _lib.CONV_HALO9)):
            bad.append(("halo", N, D, H, Cin, K, up, pro, want, p.kernel))
        # the implicit GEMM: plain weights and the split count its tile mirror gives
        M = imgs * H * H
        bco, bpx = ops.igemm_split_tile(K, M)
        sp = ops._choose_splits(M, K, -(-Cin // 64) * (27 if D else 9), bpx, bco)
        p = plan(L, desc(N, Hs, Cin, K, splits=sp, up=up, pro=pro, D=Ds, tiled=False), HALO | STATS)
        tile = (bco, bpx) if sp > 1 else (bco, 256 if K <= 16 else 128)   # the small-pixel tiles only with split-K
        if (p.kernel, p.bco, p.bpx) != (_lib.CONV_IGEMM, *tile):
            bad.append(("igemm", N, D, H, Cin, K, up, pro, sp, tile, (p.kernel, p.bco, p.bpx)))
    assert not bad, bad[:20]
