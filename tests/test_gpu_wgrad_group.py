"""Grouped weight gradients (fmd_wgrad_group; ops.wgrad_group / WgradQueue; the engine's deferral).

A grouped launch changes where a job's workgroups sit in the grid, never what they compute: every job must equal
``ops.wgrad`` with the same splits bit for bit.  The planner then picks fewer splits per job, which only
reassociates the fp32 split sums: those results are held to the tolerances of test_gpu_kernels.py's
test_wgrad_halo_vs_torch (rtol 2e-2, atol 2e-2 max|ref| for dW; 1e-3 for db) and, through the engine, to the
bounds of test_gpu_unet.py's train-step test (relative L2 <= 5e-2 over all parameters, cosine >= 0.99)."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"


def ops():
    from fmdiff.runtime import ops as O
    return O


# ---------------------------------------------------------------------------------------------- problems
# name -> (N, H, W, C0, C1, K, ks, stride, prologue, wide dY, db, accumulate, force_generic); H x W is the input grid
HALO = {   # the smallest shapes the halo kernel takes (2, 4 and 12 pixel tiles), all with the GN+SiLU prologue
    "h_a": (2, 8, 16, 64, 0, 128, 3, 1, True, False, True, True, False),
    "h_b": (2, 16, 16, 64, 64, 256, 3, 1, True, False, False, False, False),
    "h_c": (3, 16, 32, 128, 0, 128, 3, 1, True, True, True, True, False),
    "h_d": (2, 16, 16, 128, 0, 128, 3, 1, True, True, True, True, False),      # h_b's grid: one level with it
}
RAW = {    # raw-input halo jobs (another kernel instance)
    "r_a": (2, 8, 16, 64, 0, 128, 3, 1, False, False, True, False, False),
    "r_c": (3, 16, 32, 128, 0, 128, 3, 1, False, True, False, True, False),
}
S2D = {    # stride 2 on the halo kernel (space-to-depth planes as chunks)
    "s_a": (2, 32, 32, 64, 0, 128, 3, 2, False, False, True, True, False),
    "s_b": (2, 32, 64, 128, 0, 128, 3, 2, False, True, False, False, False),
    "s_c": (2, 32, 32, 128, 0, 256, 3, 2, False, False, True, False, False),    # s_a's grid
}
GENERIC = {
    "g_3x3": (2, 8, 8, 64, 0, 128, 3, 1, False, False, True, True, False),     # 8-wide grid: not a halo problem
    "g_1x1": (2, 8, 8, 64, 64, 128, 1, 1, True, True, True, False, False),
    "g_force": (2, 16, 16, 64, 0, 128, 3, 1, True, False, False, True, True),   # halo-eligible, forced generic
    "g_3x3b": (2, 8, 8, 128, 0, 256, 3, 1, False, False, False, False, False),  # g_3x3's and g_1x1's grid
}
ALL = {**HALO, **RAW, **S2D, **GENERIC}


@functools.lru_cache(maxsize=None)
def _problem(name):
    """Seeded operands (CPU) and the torch reference gradients of problem ``name``; computed once."""
    N, H, W, C0, C1, K, ks, stride, pro, wide, has_db, acc, force = ALL[name]
    g = torch.Generator().manual_seed(1000 + sorted(ALL).index(name))
    C = C0 + C1
    x0 = torch.randn(N, H, W, C0, generator=g).to(torch.bfloat16)
    x1 = torch.randn(N, H, W, C1, generator=g).to(torch.bfloat16) if C1 else None
    x = (torch.cat([x0, x1], -1) if C1 else x0).float().permute(0, 3, 1, 2)
    a = b = None
    if pro:
        a = torch.rand(N, C, generator=g) + 0.5
        b = torch.randn(N, C, generator=g) * 0.2
        x = F.silu(x * a[:, :, None, None] + b[:, :, None, None]).to(torch.bfloat16).float()
    w = (torch.randn(K, C, ks, ks, generator=g) / math.sqrt(C * ks * ks)).requires_grad_()
    bias = torch.zeros(K, requires_grad=True)
    y = F.conv2d(x, w, bias, stride=stride, padding=ks // 2)
    dy = torch.randn(y.shape, generator=g).to(torch.bfloat16).float()
    y.backward(dy)
    dyn = dy.permute(0, 2, 3, 1).contiguous().to(torch.bfloat16)
    off = 0
    if wide:   # dY is channels [64, 64 + K) of a wider tensor (ldy / dy_offset)
        full = torch.zeros(*dyn.shape[:3], K + 128, dtype=torch.bfloat16)
        full[..., 64:64 + K] = dyn
        dyn, off = full, 64
    return dict(x0=x0, x1=x1, a=a, b=b, dy=dyn, off=off, ks=ks, stride=stride, pad=ks // 2, acc=acc, force=force,
                dw0=torch.randn(K, C, ks, ks, generator=g), db0=torch.randn(K, generator=g) if has_db else None,
                dw_ref=w.grad.detach(), db_ref=bias.grad.detach())


def _args(name):
    """(positional, keyword) arguments of ops.wgrad / ops.wgrad_job on the device, with fresh dW / db buffers."""
    p = _problem(name)
    dw = p["dw0"].clone().to(DEV)
    db = p["db0"].clone().to(DEV) if p["db0"] is not None else None
    kw = dict(src1=p["x1"].to(DEV) if p["x1"] is not None else None, ks=p["ks"], stride=p["stride"], pad=p["pad"],
              pro=(p["a"].to(DEV), p["b"].to(DEV), True) if p["a"] is not None else None, db=db,
              accumulate=p["acc"], dy_offset=p["off"], force_generic=p["force"])
    return (p["x0"].to(DEV), p["dy"].to(DEV), dw), kw


@functools.lru_cache(maxsize=None)
def _single(name, splits):
    """dW, db of ops.wgrad with the given splits (the reference of the bit-identity tests); computed once."""
    pos, kw = _args(name)
    ops().wgrad(*pos, splits=splits, **kw)
    return pos[2].cpu(), kw["db"].cpu() if kw["db"] is not None else None


def _group(names, splits):
    O = ops()
    args = [_args(n) for n in names]
    O.wgrad_group([O.wgrad_job(*pos, **kw) for pos, kw in args], splits)
    return [(pos[2].cpu(), kw["db"].cpu() if kw["db"] is not None else None) for pos, kw in args]


def _same(got, ref, what):
    assert torch.equal(got[0], ref[0]), f"{what}: dW differs"
    assert (got[1] is None) == (ref[1] is None)
    if ref[1] is not None:
        assert torch.equal(got[1], ref[1]), f"{what}: db differs"


# ------------------------------------------------------------------------------- 1. bit identity per job
@pytest.mark.parametrize("names,splits", [
    (("h_a", "h_b", "h_c"), (1, 3, 20)),      # 20 > h_c's 12 tiles
    (("h_b", "h_c", "h_a"), (1, 3, 5)),       # 5 > h_a's 2 tiles
    (("h_c", "h_a", "h_b"), (1, 3, 7)),       # 7 > h_b's 4 tiles
    (("r_a", "r_c"), (3, 1)),
    (("s_a", "s_b"), (3, 9)),                 # 9 > s_b's 8 tiles
    (("s_b", "s_a"), (1, 2)),
    (("g_3x3", "g_1x1", "g_force"), (1, 3, 5)),   # g_3x3 / g_1x1: 4 32-pixel steps
    (("g_force", "g_3x3", "g_1x1"), (20, 5, 1)),
])
def test_group_jobs_equal_single_launches(names, splits):
    assert len({ops().wgrad_job(*_args(n)[0], **_args(n)[1]).shape.key for n in names}) == 1
    for n, s, got in zip(names, splits, _group(names, list(splits))):
        _same(got, _single(n, s), f"{n} splits {s}")


def test_mixed_kernel_instances_are_rejected():
    O = ops()
    for names in (("h_a", "r_a"), ("h_a", "g_3x3"), ("r_a", "s_a"), ("h_a", "g_force")):
        args = [_args(n) for n in names]
        before = [pos[2].clone() for pos, _ in args]
        with pytest.raises(RuntimeError):
            O.wgrad_group([O.wgrad_job(*pos, **kw) for pos, kw in args], 2)
        torch.cuda.synchronize()
        for (pos, _), b in zip(args, before):
            assert torch.equal(pos[2], b), "nothing may be launched"


# ------------------------------------------------------------------------------------- 2. group sizes
@pytest.mark.parametrize("n", [1, 2, "cap+3"])
def test_group_sizes(n, monkeypatch):
    from fmdiff import _lib
    from fmdiff.runtime import wgrad_plan
    n = wgrad_plan.GROUP_MAX + 3 if n == "cap+3" else n
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (calls.append((name, a[1]) if name == "fmd_wgrad_group"
                                                                     else None), real(name, *a))[1])
    order = ["h_a", "h_b", "h_c"]
    names = [order[i % 3] for i in range(n)]
    splits = [(1, 3, 5)[(i // 3) % 3] for i in range(n)]
    res = _group(names, splits)
    launched = [c for c in calls if c is not None]
    assert [c[1] for c in launched] == ([n] if n <= wgrad_plan.GROUP_MAX else [wgrad_plan.GROUP_MAX, 3])
    for nm, s, got in zip(names, splits, res):
        _same(got, _single(nm, s), f"{nm} splits {s}")


# --------------------------------------------------------------- 3. planner-chosen splits against torch
@pytest.mark.parametrize("names,knobs,want", [
    # the planner's targets scaled down to a "chip" these small jobs fill, so the group rule -- not the tile count --
    # decides: halo sum of bases 4 + 2 + 4 = 10 -> 24 // 10 = 2 splits (alone: 4 each, all tiles)
    (("h_b", "h_d", "h_b"), dict(WGRAD_HALO_WG=24), 2),
    (("s_a", "s_c"), dict(WGRAD_HALO_WG=48), 2),          # bases 4 + 16: 48 // 20 = 2 (alone 4 and 3)
    # generic: 5 + 1 + 18 workgroups unsplit, 48 wanted -> 2 splits (alone 4, 4 and 3)
    (("g_3x3", "g_1x1", "g_3x3b"), dict(NUM_CU=48, WGRAD_CU_MULT=1, WGRAD_MIN_STEPS=1), 2),
])
def test_planned_group_vs_torch(names, knobs, want, monkeypatch):
    """Same-grid jobs of one kernel instance (a level) planned together by wgrad_plan.plan_groups -- the group rule's
    splits, not each job's own -- against torch, and run to run."""
    O = ops()
    from fmdiff.runtime import wgrad_plan
    for k, v in knobs.items():
        monkeypatch.setattr(O, k, v)
    outs = []
    for _ in range(2):
        args = [_args(n) for n in names]
        jobs = [O.wgrad_job(*pos, **kw) for pos, kw in args]
        plan = wgrad_plan.plan_groups([j.shape for j in jobs], **O._plan_kw())
        assert [idx for idx, _ in plan] == [list(range(len(jobs)))]   # one launch for the level
        (idx, splits), = plan
        assert splits == want and all(j.single_splits() > splits for j in jobs)   # fewer splits than alone
        O.wgrad_group(jobs, splits)
        outs.append([(pos[2].cpu(), kw["db"].cpu() if kw["db"] is not None else None) for pos, kw in args])
    for n, r0, r1 in zip(names, *outs):
        _same(r1, r0, f"{n}: second run")
        p = _problem(n)
        dw = r0[0] - p["dw0"] if p["acc"] else r0[0]
        torch.testing.assert_close(dw, p["dw_ref"], rtol=2e-2, atol=2e-2 * p["dw_ref"].abs().max().item())
        if r0[1] is not None:
            db = r0[1] - p["db0"] if p["acc"] else r0[1]
            torch.testing.assert_close(db, p["db_ref"], rtol=1e-3, atol=1e-3 * p["db_ref"].abs().max().item())


def test_queue_groups_a_level_and_flushes_on_grid_change(monkeypatch):
    """ops.WgradQueue under ops.wgrad_defer: same-grid jobs of one kernel instance leave together with the group
    plan's splits at the flush; a job on another grid or onto a queued dW flushes first; immediate jobs run at once
    after a flush.  Results against torch at the kernel tolerances."""
    O = ops()
    launched = []
    real = O.wgrad_group
    monkeypatch.setattr(O, "wgrad_group", lambda jobs, splits: (launched.append((len(jobs), splits)),
                                                                 real(jobs, splits))[1])
    q = O.WgradQueue()
    names = ["h_b", "h_b", "g_force", "h_a", "h_a"]   # 16x16, 16x16, 16x16 (generic), 8x16, 8x16 (same dW: flush)
    args = [_args(n) for n in names]
    args[4] = ((args[4][0][0], args[4][0][1], args[3][0][2]), dict(args[4][1], db=args[3][1]["db"]))
    with O.wgrad_defer(q):
        for pos, kw in args[:3]:
            O.wgrad(*pos, **kw)
        assert len(q) == 3 and not launched
        O.wgrad(*args[3][0], **args[3][1])            # another grid: the 16x16 level leaves, halo pair together
        assert sorted(n for n, _ in launched) == [1, 2] and len(q) == 1
        O.wgrad(*args[4][0], **args[4][1])            # same dW / db as the queued job: that one leaves first
        assert len(launched) == 3 and len(q) == 1
        O.wgrad(*_args("h_c")[0], **dict(_args("h_c")[1], immediate=True))
        assert len(launched) == 4 and len(q) == 0
    q.flush()
    assert len(launched) == 4
    torch.cuda.synchronize()
    p = _problem("h_a")   # accumulated twice into one buffer
    torch.testing.assert_close(args[3][0][2].cpu() - p["dw0"], 2 * p["dw_ref"], rtol=2e-2,
                               atol=4e-2 * p["dw_ref"].abs().max().item())
    pb = _problem("h_b")  # accumulate off
    for i in (0, 1):
        torch.testing.assert_close(args[i][0][2].cpu(), pb["dw_ref"], rtol=2e-2,
                                   atol=2e-2 * pb["dw_ref"].abs().max().item())


# -------------------------------------------------------------------------------------- 4. engine level
def _build(meta):
    from fmdiff.models.generators import DiffusionUNetFactory
    tr = meta["training"]
    return DiffusionUNetFactory().build(meta["unet"], tr["conditioning"], tr["channels"] or 1)


@functools.lru_cache(maxsize=None)
def _step_inputs(hw):
    g = torch.Generator().manual_seed(3)
    clean = torch.rand(2, 1, hw, hw, generator=g)
    ldct = torch.rand(2, 1, hw, hw, generator=g)
    noise = torch.randn(2, 1, hw, hw, generator=g)
    t = torch.rand(2, generator=g)
    return clean, ldct, noise, t


_ORACLE = {}


def _oracle_grads(name, meta, hw):
    """fp32 CPU oracle gradients of one FM train step; computed once per model."""
    if name not in _ORACLE:
        from oracle import spec as S
        from oracle import train_step as OT
        from oracle import unet as U
        tr = meta["training"]
        spec = S.derive_spec(meta["unet"], tr["conditioning"], tr["channels"] or 1)
        sd = {k: v.requires_grad_() for k, v in U.seeded_state_dict(spec, meta["seed"]).items()}
        loss, scaled = OT.fm_loss(sd, spec, *_step_inputs(hw), 1000)
        scaled.backward()
        _ORACLE[name] = (loss.item(), {k: v.grad.double() for k, v in sd.items()})
    return _ORACLE[name]


def _engine_step(meta, hw, monkeypatch, group, own_splits):
    from oracle import spec as S
    from oracle import unet as U
    O = ops()
    monkeypatch.setattr(O, "WGRAD_GROUP", group)
    monkeypatch.setattr(O, "WGRAD_GROUP_SPLITS", int(own_splits))
    sizes = []
    real = getattr(O.wgrad_group, "real", O.wgrad_group)   # the steps of one test each count their own launches

    def counted(jobs, splits):
        sizes.append(len(jobs))
        real(jobs, splits)
    counted.real = real
    monkeypatch.setattr(O, "wgrad_group", counted)
    model = _build(meta).to(DEV)
    tr = meta["training"]
    model.load_state_dict(U.seeded_state_dict(S.derive_spec(meta["unet"], tr["conditioning"], tr["channels"] or 1),
                                              meta["seed"]))
    clean, ldct, noise, t = (v.to(DEV) for v in _step_inputs(hw))
    x_t = (1.0 - t[:, None, None, None]) * clean + t[:, None, None, None] * noise
    pred = model(x_t, (t * 999).long(), context=ldct)
    loss = F.mse_loss(pred, noise - clean)
    loss.backward()
    torch.cuda.synchronize()
    return loss.item(), {k: p.grad.detach().cpu() for k, p in model.named_parameters()}, sizes


@pytest.mark.parametrize("name,hw", [("fm_step", 32), ("ldct_fm_diffusers_b64", 64)])
def test_engine_grouped_step(golden, name, hw, monkeypatch):
    """One train step of a 2-level EfficientUNetND (concat decoder, 1x1 skips) at 32^2 and of the diffusers-compat
    config-B family at 64^2: grouped with every job's own splits == ungrouped, bit for bit; grouped with the
    planner's splits inside test_gpu_unet.py's train-step bounds against the fp32 oracle."""
    _, M = golden
    meta = M[name]
    l0, g0, s0 = _engine_step(meta, hw, monkeypatch, False, False)
    l1, g1, s1 = _engine_step(meta, hw, monkeypatch, True, True)
    l2, g2, s2 = _engine_step(meta, hw, monkeypatch, True, False)
    assert not s0 and s1 == s2 and max(s1) >= 2, (s0, s1, s2)
    assert l0 == l1
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    loss_ref, ref = _oracle_grads(name, meta, hw)
    assert abs(l2 - loss_ref) / loss_ref < 1e-2
    num = den = 0.0
    worst = (1.0, "")
    for k, g in g2.items():
        g, r = g.double(), ref[k]
        num += (g - r).pow(2).sum().item()
        den += r.pow(2).sum().item()
        if r.norm() > 1e-3 * math.sqrt(den + 1e-30):
            cos = ((g * r).sum() / (g.norm() * r.norm() + 1e-30)).item()
            if cos < worst[0]:
                worst = (cos, k)
    rel = math.sqrt(num / den)
    print(f"{name}: group sizes {s2}; grad rel L2 vs oracle {rel:.3e}, worst cosine {worst}")
    assert rel < 5e-2
    assert worst[0] > 0.99, worst


def test_per_bucket_backward_equals_single_graph_with_grouping(golden):
    """The overlapped (per-bucket captured) train step equals the single-graph step bit for bit with grouped weight
    gradients on: the queue is flushed at every backward segment, so the groups -- and with them every job's
    splits -- do not depend on how the segments are dealt to backward() calls, and each bucket's gradients are
    final when its all-reduce starts."""
    from fmdiff.pipelines.train.fused import FusedTrainStep
    from oracle import spec as S
    from oracle import unet as U
    O = ops()
    assert O.WGRAD_GROUP
    T, M = golden
    name = "ldct_fm_test"
    meta = M[name]
    tr_ = meta["training"]
    sd = U.seeded_state_dict(S.derive_spec(meta["unet"], tr_["conditioning"], tr_["channels"] or 1), meta["seed"])
    x, cond = T[f"{name}/x"].to(DEV), T[f"{name}/cond"].to(DEV)
    res = []
    for split, overlap in ((False, False), (True, True)):
        model = _build(meta).to(DEV)
        model.load_state_dict(sd)
        tr = FusedTrainStep(model, lr=1e-3, warmup=1, overlap_allreduce=overlap)
        torch.manual_seed(11)
        tr.capture(x.clamp(0, 1), cond, warmup_iters=1, split_collectives=split)
        loss = float(tr.replay().item())
        torch.cuda.synchronize()
        res.append((loss, {k: p.detach().clone() for k, p in model.named_parameters()}))
    assert res[0][0] == res[1][0] and math.isfinite(res[0][0])
    for k in res[0][1]:
        assert torch.equal(res[0][1][k], res[1][1][k]), k
