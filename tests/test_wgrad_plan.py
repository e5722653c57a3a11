"""CPU test of the grouped weight-gradient planner (fmdiff/runtime/wgrad_plan.py) on config B's job lists.

Config B (bench.py LDCT_FM_UNET): batch 8 at 256^2, block_out_channels [128, 128, 256, 256, 512, 512], two
ResBlocks per encoder stage and three per decoder stage, 3x3 down / up convs.  Per level the engine queues, in
backward order, the decoder's ResBlock convs (3x3 with GN+SiLU prologue, plus the 1x1 skip), the up conv that
writes the level, and later the encoder's ResBlocks and the down conv that writes the level."""
import pytest

from fmdiff.runtime import wgrad_plan as P

KW = dict(num_cu=256, halo_wg=256, slab_mb=96, gen_slab_mb=48, min_steps=8, cu_mult=4)
N = 8
# level -> (decoder ResBlocks (Cin, Cout), up conv writing the level (C) or None,
#           encoder / middle ResBlocks (Cin, Cout), down conv writing the level (C) or None)
LEVELS = {
    256: ([(256, 128)] * 3, 128, [(128, 128)] * 2, None),
    128: ([(384, 128), (256, 128), (256, 128)], 256, [(128, 128)] * 2, 128),
    64: ([(512, 256), (512, 256), (384, 256)], 256, [(128, 256), (256, 256)], 128),
    32: ([(768, 256), (512, 256), (512, 256)], 512, [(256, 256)] * 2, 256),
    16: ([(1024, 512), (1024, 512), (768, 512)], 512, [(256, 512), (512, 512)], 256),
    8: ([(1024, 512)] * 3, None, [(512, 512)] * 4, 512),
}


def _halo(hw):
    return hw % 16 == 0   # 3x3 on K % 128 == 0, C % 64 == 0 throughout; only the 8^2 level misses the 8x16 tile


MAX_PIX = 131072   # tuning WGRAD_GROUP_MAX_PIX: larger output grids are not queued (config B: the 256^2 level)


def _segments(hw):
    """The queue's contents at each flush while the level is visited.  The decoder is one backward segment, so a
    level's decoder jobs wait together (the grid change flushes them); in the encoder every input block -- one
    ResBlock, or the down conv -- is a backward segment of its own and the engine flushes at each segment end; the
    middle block (the last two 8^2 ResBlocks) is one segment."""
    dec, up, enc, down = LEVELS[hw]
    h = _halo(hw)
    # at the generic levels the GN+SiLU operand is materialised: raw-input jobs
    pro = 2 if h else 0

    def blocks(bl):
        out = []
        for cin, cout in reversed(bl):
            out.append(P.Shape(N, hw, hw, cout, cout, halo=h, pro=pro))
            if cin != cout:
                out.append(P.Shape(N, hw, hw, cout, cin, ks=1, halo=False))
            out.append(P.Shape(N, hw, hw, cout, cin, halo=h, pro=pro))
        return out
    a = blocks(dec)
    if up is not None:
        a = [P.Shape(N, hw, hw, up, up, halo=h)] + a
    segs = [a]
    if hw == 8:
        segs.append(blocks(enc[2:]))   # middle block
        enc = enc[:2]
    segs += [blocks([b]) for b in reversed(enc)]
    if down is not None:
        segs.append([P.Shape(N, hw, hw, down, down, stride=2, halo=h)])
    return segs


def _by_key(jobs):
    d = {}
    for j in jobs:
        d.setdefault(j.key, []).append(j)
    return d


@pytest.mark.parametrize("hw", sorted(LEVELS))
def test_group_plan_per_level(hw):
    for seg in _segments(hw):
        for key, jobs in _by_key(seg).items():
            plan = P.plan_groups(jobs, **KW)
            assert sorted(i for idx, _ in plan for i in idx) == list(range(len(jobs)))   # every job exactly once
            for idx, splits in plan:
                assert 1 <= len(idx) <= P.GROUP_MAX
                assert {jobs[i].key for i in idx} == {key}
                assert isinstance(splits, int) and splits >= 1   # one split count for the whole launch
                if key[0] == "halo":
                    base = sum(jobs[i].halo_base for i in idx)
                    # at most one round of workgroups, or a lone job whose base tiles alone exceed it
                    assert base * splits <= KW["halo_wg"] or (len(idx) == 1 and splits == 1)
                    for i in idx:
                        t = jobs[i].halo_tiles
                        assert (splits - 1) * -(-t // splits) < t   # the last split still owns a tile
                else:
                    for i in idx:
                        st = jobs[i].steps
                        assert (splits - 1) * -(-st // splits) < st


def test_generic_level_needs_no_slab_duplication():
    """The 8^2 decoder (9 generic jobs in one segment, > WGRAD_CU_MULT workgroups per CU unsplit): one split.  The
    encoder's one-ResBlock segments there keep the rule's 2 splits (288 unsplit workgroups each)."""
    dec = _segments(8)[0]
    assert len(dec) == 9
    for jobs in _by_key(dec).values():
        assert all(s == 1 for _, s in P.plan_groups(jobs, **KW))
    for seg in _segments(8)[2:4]:
        for jobs in _by_key(seg).values():
            assert all(s == 2 for _, s in P.plan_groups(jobs, **KW))


def test_groups_cut_at_cap_and_reject_mixed_keys():
    jobs = [P.Shape(2, 16, 16, 128, 64, pro=2)] * (P.GROUP_MAX + 3)
    plan = P.plan_groups(jobs, **KW)
    assert [len(idx) for idx, _ in plan] == [P.GROUP_MAX, 3]
    with pytest.raises(ValueError):
        P.plan_groups([P.Shape(2, 16, 16, 128, 64, pro=2), P.Shape(2, 16, 16, 128, 64, pro=0)], **KW)
    with pytest.raises(ValueError):
        P.plan_groups([P.Shape(2, 16, 16, 128, 64), P.Shape(2, 32, 32, 128, 64)], **KW)


def test_single_rule_matches_the_ungrouped_formulas():
    s = P.Shape(8, 256, 256, 128, 128, pro=2)
    assert s.halo_tiles == 4096 and s.halo_base == 2 and P.single_splits(s, **KW) == 128
    s = P.Shape(8, 16, 16, 512, 1024, pro=2)
    assert s.halo_tiles == 16 and s.halo_base == 64 and P.single_splits(s, **KW) == 4
    s = P.Shape(8, 8, 8, 512, 512, halo=False)
    assert s.generic_tiles == 4 * 4 * 9 and s.steps == 16 and P.single_splits(s, **KW) == 2
    assert P.slab_floats(s, 2) == 2 * 512 * 9 * 512 + 2 * 512


def test_grouped_plan_writes_fewer_slab_bytes_per_step():
    """Planned split-K slab bytes of one config-B step: ungrouped, as shipped (levels above MAX_PIX pixels stay
    ungrouped) and with every level grouped."""
    single = shipped = every = 0
    for hw in LEVELS:
        for seg in _segments(hw):
            alone = P.slab_bytes(seg, [P.single_splits(j, **KW) for j in seg])
            grouped = 0
            for jobs in _by_key(seg).values():
                for idx, splits in P.plan_groups(jobs, **KW):
                    grouped += P.slab_bytes([jobs[i] for i in idx], [splits] * len(idx))
            single += alone
            every += grouped
            shipped += grouped if N * hw * hw <= MAX_PIX else alone
    print(f"planned slab bytes per step: ungrouped {single / 1e9:.2f} GB, as shipped {shipped / 1e9:.2f} GB, "
          f"every level grouped {every / 1e9:.2f} GB")
    assert every < shipped < single
