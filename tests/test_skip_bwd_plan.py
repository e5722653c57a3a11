"""fmd_skip_bwd_plan (csrc/skip_bwd.hip decide): the host-side decision whether a ResBlock's skip-conv backward runs
as the fused pass, and its c-tile, workgroups and workspace -- queried on descriptors alone (no GPU), for the 20
non-identity skips of the config-B train step (batch 8, 256^2) and a sweep of shapes."""
import collections
import ctypes as C
import json
import os

import pytest
import torch

from fmdiff import _lib
from fmdiff.runtime import ops

BATCH = 8
# level (H = W) -> [(Kd, C)]: the 18 up-path blocks and the two channel-changing down-path blocks of config B
CONFIG_B = {
    256: [(128, 256)] * 3,
    128: [(128, 256), (128, 256), (128, 384)],
    64: [(256, 384), (256, 512), (256, 512), (256, 128)],
    32: [(256, 512), (256, 512), (256, 768)],
    16: [(512, 768), (512, 1024), (512, 1024), (512, 256)],
    8: [(512, 1024)] * 3,
}


@pytest.fixture(scope="module")
def L():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libfmdiff_hip.so not built (run __graft_entry__.build())")
    try:
        return _lib.lib()
    except OSError as e:   # HIP runtime absent on this host
        pytest.skip(f"HIP runtime not loadable here: {e}")


def plan(L, N, HW, C0, C1, Kd, groups=0, num_cu=256, min_tiles=0):
    d = _lib.SkipBwdDesc()
    d.N, d.HW, d.C0, d.C1, d.Kd, d.groups, d.num_cu, d.min_tiles = N, HW, C0, C1, Kd, groups, num_cu, min_tiles
    p = _lib.SkipBwdPlan()
    rc = L.fmd_skip_bwd_plan(C.byref(d), C.byref(p))
    assert rc in (0, 1) and bool(p.taken) == (rc == 0)
    return p


def test_table_is_the_models_skip_convs():
    """The table above against the model itself (built on the meta device: shapes only)."""
    from fmdiff.models.generators import DiffusionUNetFactory
    meta = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden_b256.json")))
    tr = meta["training"]
    with torch.device("meta"):
        model = DiffusionUNetFactory().build(meta["unet"], tr["conditioning"], tr["channels"] or 1)
    got = [(m.out_channels, m.channels) for m in model.modules()
           if type(m).__name__ == "ResBlockND" and type(m.skip_connection).__name__ != "Identity"]
    want = [s for lvl in CONFIG_B.values() for s in lvl]
    assert len(got) == 20 and collections.Counter(got) == collections.Counter(want)


def test_config_b_levels(L):
    for hw, shapes in CONFIG_B.items():
        for Kd, Cin in shapes:
            # the up path concatenates h | skip; where the split lies does not enter the plan beyond C0 % 8
            for C0 in (Cin, Cin // 2):
                p = plan(L, BATCH, hw * hw, C0, Cin - C0, Kd, min_tiles=ops.SKIP_BWD_MIN_TILES)
                M = BATCH * hw * hw
                if Kd == 128:   # the 256^2 and 128^2 levels: taken, 128-channel c-tiles
                    assert p.taken and p.c_tile == 128, (hw, Kd, Cin)
                    ntc, tiles = -(-Cin // p.c_tile), -(-M // 64)
                    assert p.workgroups % ntc == 0 and p.workgroups <= tiles * ntc
                    # two resident workgroups per CU, whole multiples of 8 pixel groups
                    assert 2 * 256 - 8 * ntc < p.workgroups <= 2 * 256
                    assert p.slabs == p.workgroups // ntc
                    assert p.ws_floats == p.slabs * (Kd * Cin + Kd)
                else:           # Kd = 256 / 512: not built -- today's launches
                    assert not p.taken, (hw, Kd, Cin)


@pytest.mark.parametrize("N,HW,C0,C1", [(2, 144, 128, 128), (2, 144, 256, 128), (1, 1, 72, 0), (2, 256, 128, 128),
                                         (8, 65536, 128, 128), (3, 4096, 64, 40), (1, 100000, 384, 0)])
def test_workspace_is_what_the_kernel_writes(L, N, HW, C0, C1):
    """One [Kd][C] weight slab and one [Kd] bias row per pixel group that has a tile; never more workgroups than
    pixel tiles x c-tiles; forced groups beyond the tiles launch idle workgroups that own no slab."""
    Kd, Cin, M = 128, C0 + C1, N * HW
    tiles = -(-M // 64)
    p = plan(L, N, HW, C0, C1, Kd)
    assert p.taken
    ntc = -(-Cin // p.c_tile)
    assert p.workgroups <= tiles * ntc and p.slabs == p.workgroups // ntc <= tiles
    assert p.ws_floats == p.slabs * (Kd * Cin + Kd)
    # the allocator ops.skip_bwd uses (the weight-gradient workspace of a 1x1 job with `slabs` splits) covers it
    w = ops._SkipWs(Kd, C0, C1, p.slabs, None)
    assert L.fmd_wgrad_workspace(C.byref(w.d)) == p.ws_floats
    for groups in (1, 3, tiles, tiles + 5):
        q = plan(L, N, HW, C0, C1, Kd, groups)
        assert q.taken and q.workgroups == groups * ntc and q.slabs == min(groups, tiles)
        assert q.ws_floats == q.slabs * (Kd * Cin + Kd)


def test_floor_on_tiles_per_group(L):
    """The default plan takes a block only with at least SKIP_BWD_MIN_TILES (8) pixel tiles per pixel group: the
    levels traced faster fused had 8 (128^2, C = 256), 12 (128^2, C = 384) and 32 (256^2).  Forced groups ignore it."""
    F = ops.SKIP_BWD_MIN_TILES
    assert F == 8
    assert plan(L, 8, 128 * 128, 128, 128, 128, min_tiles=F).taken          # 2048 tiles / 256 groups = 8
    assert plan(L, 8, 128 * 128, 256, 128, 128, min_tiles=F).taken          # 2048 / 168
    assert not plan(L, 4, 128 * 128, 128, 128, 128, min_tiles=F).taken      # 1024 / 256 = 4
    assert not plan(L, 8, 64 * 64, 128, 128, 128, min_tiles=F).taken        # 512 / 256
    assert not plan(L, 2, 144, 128, 128, 128, min_tiles=F).taken            # one tile per group
    assert plan(L, 2, 144, 128, 128, 128, groups=3, min_tiles=F).taken
    assert ops.skip_bwd_plan(8, 64 * 64, 128, 128, 128) is None
    assert ops.skip_bwd_plan(8, 64 * 64, 128, 128, 128, min_tiles=0) is not None


def test_refused_shapes(L):
    assert not plan(L, 2, 144, 128, 0, 256).taken      # Kd != 128
    assert not plan(L, 2, 144, 64, 32, 64).taken
    assert not plan(L, 2, 144, 124, 4, 128).taken      # sources not in whole 16-byte chunks
    assert not plan(L, 0, 144, 128, 0, 128).taken
    assert not plan(L, 2, 144, 32, 32, 128).taken      # C <= 64: the apply pass's 64-channel instance
    assert ops.skip_bwd_plan(2, 144, 128, 0, 256) is None


def test_switch_off_refuses_everything(monkeypatch):
    monkeypatch.setattr(ops, "SKIP_BWD", False)
    assert ops.skip_bwd_plan(8, 65536, 128, 128, 128) is None
