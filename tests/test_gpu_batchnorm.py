"""csrc/batchnorm.hip on the device against the per-output bounds of tests/bn_bounds.py (derivation there): fold,
forward, backward and the image staging.  Every output buffer is NaN in every byte beforehand, so an element that
is not written fails its bound; every launch sequence runs twice and must give equal bits."""
import functools

import pytest
import torch

import bn_bounds as B

pytestmark = pytest.mark.gpu
DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SHAPES = [(105, 8), (105, 24), (105, 64), (2112, 8), (2112, 24), (2112, 64), (2112, 512)]   # (M = N H W, C)
GEOM = {105: (3, 5, 7), 2112: (3, 22, 32)}


def ops():
    from fmdiff.runtime import ops as O
    return O


def nan_like(shape, dtype):
    """Every byte 0xFF: NaN in bf16 and fp32, -1 in int64."""
    n = 1
    for s in shape:
        n *= s
    return torch.full((n * torch.empty((), dtype=dtype).element_size(),), 255, dtype=torch.uint8,
                      device=DEV).view(dtype).view(shape)


@functools.lru_cache(maxsize=None)
def problem(M, C):
    return B.make_inputs(M, C, seed=M + C)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF16 else torch.int32)


def _fold(O, slab_st, M, T, training, rm, rv, nbt):
    return O.bn_fold(slab_st, M, T["gamma"].to(DEV), T["beta"].to(DEV), rm, rv, nbt, training=training)


# 64-pixel slab rows and a conv's own statistics exist for images of whole 64-pixel rows only (H*W = 704 here); 5x7
# images take one slab row per image
FOLD_CASES = [(M, C, src) for M, C in SHAPES
              for src in (("channel_stats_per_image", "channel_stats_64", "conv_epilogue") if M == 2112
                          else ("channel_stats_per_image",))]


@pytest.mark.parametrize("M,C,source", FOLD_CASES)
def test_bn_fold(M, C, source):
    O = ops()
    T = problem(M, C)
    N, H, W = GEOM[M]
    x = T["x"].to(DEV).view(N, H, W, C)
    if source == "channel_stats_per_image":
        st = O.channel_stats(x, rows=H * W)
        assert st.slab.shape[0] == N
    elif source == "channel_stats_64":
        st = O.channel_stats(x, rows=64)
    else:
        # the statistics a conv emits: a 3x3 conv whose centre tap is the identity reproduces x.  M = 2112 is no
        # multiple of a pixel tile, so the unsplit epilogue emits none; the split-K combine does (16-pixel rows)
        wm = torch.zeros(C, C, 3, 3, device=DEV)
        wm[:, :, 1, 1] = torch.eye(C, device=DEV)
        plans = []
        y, st = O.conv(x, C, O.prep_weights(wm, 0), want_stats="free", splits=3, force_generic=True, plan_out=plans)
        assert st is not None and plans[0].stats_rows == st.rows > 0, "this plan emits no statistics"
        assert torch.equal(_bits(y), _bits(x))
    slab = st.slab.cpu()
    for training in (True, False):
        runs = []
        for _ in range(2):
            rm, rv = T["rm"].to(DEV), T["rv"].to(DEV)
            nbt = torch.tensor(41, dtype=torch.int64, device=DEV)
            a, b, mr = _fold(O, st, M, T, training, rm, rv, nbt)
            runs.append([t.cpu() for t in (a, b, mr, rm, rv, nbt)])
        assert all(torch.equal(_bits(p) if p.dtype != torch.int64 else p, _bits(q) if q.dtype != torch.int64 else q)
                   for p, q in zip(*runs)), "two runs differ"
        a, b, mr, rm, rv, nbt = runs[0]
        R = B.fold_ref(slab, M, T["gamma"], T["beta"], T["rm"], T["rv"], training=training)
        Bd, b_ref = B.fold_bounds(R, M, T["gamma"], T["beta"], T["rm"], T["rv"], a, training=training)
        got = dict(mean=mr[:, 0], rstd=mr[:, 1], a=a, rm=rm, rv=rv)
        res = {k: B.ratio(got[k], R[k], Bd[k]) for k in (("mean", "rstd", "a", "rm", "rv") if training
                                                         else ("mean", "rstd", "a"))}
        res["b"] = B.ratio(b, b_ref, Bd["b"])
        print(f"bn_fold M={M} C={C} {source} training={training}: " + " ".join(f"{k}={v:.3f}" for k, v in res.items()))
        assert all(v <= 1.0 for v in res.values()), res
        if training:
            assert nbt.dtype == torch.int64 and int(nbt) == 42
        else:
            assert int(nbt) == 41 and torch.equal(rm, T["rm"]) and torch.equal(rv, T["rv"])
    # the slab itself: within the fp32 chain of fmd_channel_stats of the fp64 sums of x (gn_bounds' row)
    xd = T["x"].double()
    k = -(-st.rows // 32) + min(st.rows, 32)
    tot = slab.double().sum(0)
    assert ((tot[:, 0] - xd.sum(0)).abs() <= (k + N) * B.U * xd.abs().sum(0)).all()
    assert ((tot[:, 1] - (xd * xd).sum(0)).abs() <= (k + N + 1) * B.U * (xd * xd).sum(0)).all()


def _affine(O, T, M, C, training):
    """(a, b, mean_rstd) on the device from the kernel itself, then the kink planted in channel 0."""
    N, H, W = GEOM[M]
    x = T["x"].to(DEV).view(N, H, W, C)
    st = O.channel_stats(x, rows=H * W)
    a, b, mr = _fold(O, st, M, T, training, T["rm"].to(DEV), T["rv"].to(DEV), None)
    a, b = a.cpu(), b.cpu()
    xk = B.plant_kink(T["x"].clone(), a, b)
    return xk, a, b, mr.cpu()


@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("M,C", SHAPES)
def test_bn_act_fwd(M, C, norm):
    O = ops()
    T = problem(M, C)
    x, a, b, _ = _affine(O, T, M, C, True)
    if not norm:
        a = b = None
        x[0:3, 0] = 0.0
    else:
        zero, pos, neg = B.kink_census(x, a, b)
        assert zero >= 3 and pos > 0 and neg > 0
    xs = x.to(DEV)
    outs = []
    for _ in range(2):
        y = nan_like((M, C), BF16)
        O.bn_act_fwd(xs, None if a is None else a.to(DEV), None if b is None else b.to(DEV), out=y)
        outs.append(y.cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    v, b32 = B.act_fwd_ref(x, a, b)
    r = B.ratio(outs[0], v, B.bf16_store(v, b32))
    print(f"bn_act_fwd M={M} C={C} norm={norm}: {r:.3f}")
    assert r <= 1.0
    if norm:   # the bits of the emulation, too: one fma, one rounding
        assert torch.equal(_bits(outs[0]), _bits(B.emulate_fwd(x, a, b)))


@pytest.mark.parametrize("mode", ["train", "eval", "plain"])
@pytest.mark.parametrize("M,C", SHAPES)
def test_bn_act_bwd(M, C, mode):
    O = ops()
    T = problem(M, C)
    training = mode == "train"
    x, a, b, mr = _affine(O, T, M, C, training)
    dy = T["dy"]
    if mode == "plain":
        x[0:3, 0] = 0.0
        outs = []
        for _ in range(2):
            dx = nan_like((M, C), BF16)
            O.bn_act_bwd(dy.to(DEV), x.to(DEV), out=dx)
            outs.append(dx.cpu())
        assert torch.equal(_bits(outs[0]), _bits(outs[1]))
        R = B.act_bwd_ref(dy, x, None, None, None, None, M)
        assert B.ratio(outs[0], R["dx"], B.act_bwd_bounds(R, x, None, None, None, M)["dx"]) <= 1.0
        assert torch.equal(outs[0][0:3, 0], (dy[0:3, 0].float() * torch.tensor(0.2)).to(BF16))   # slope at exactly 0
        return
    zero, pos, neg = B.kink_census(x, a, b)
    assert zero >= 3 and pos > 0 and neg > 0
    mean, rstd = mr[:, 0], mr[:, 1]
    dev = [t.to(DEV) for t in (dy, x, a, b, mr)]
    for acc in (True, False):
        outs = []
        for _ in range(2):
            dx = nan_like((M, C), BF16)
            dg = T["old_dgamma"].to(DEV) if acc else nan_like((C,), F32)
            db = T["old_dbeta"].to(DEV) if acc else nan_like((C,), F32)
            O.bn_act_bwd(*dev, training=training, dgamma=dg, dbeta=db, accumulate=acc, out=dx)
            outs.append((dx.cpu(), dg.cpu(), db.cpu()))
        assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(*outs)), "two runs differ"
        og, ob = (T["old_dgamma"], T["old_dbeta"]) if acc else (None, None)
        R = B.act_bwd_ref(dy, x, a, b, mean, rstd, M, training=training, old_dgamma=og, old_dbeta=ob)
        Bd = B.act_bwd_bounds(R, x, a, mean, rstd, M, training=training, old_dgamma=og, old_dbeta=ob)
        res = {k: B.ratio(g, R[k], Bd[k]) for k, g in zip(("dx", "dgamma", "dbeta"), outs[0])}
        print(f"bn_act_bwd M={M} C={C} {mode} acc={acc}: " + " ".join(f"{k}={v:.3f}" for k, v in res.items()))
        assert all(v <= 1.0 for v in res.values()), res
    # the flag: dx keeps its bits, gamma / beta gradients are left alone
    dx = nan_like((M, C), BF16)
    dg, db = T["old_dgamma"].to(DEV), T["old_dbeta"].to(DEV)
    O.bn_act_bwd(*dev, training=training, dgamma=dg, dbeta=db, skip_param_grads=True, out=dx)
    assert torch.equal(_bits(dx.cpu()), _bits(outs[0][0]))
    assert torch.equal(dg.cpu(), T["old_dgamma"]) and torch.equal(db.cpu(), T["old_dbeta"])


TWO_TERM = [(105, 24), (2112, 8), (2112, 64), (2112, 512)]


def _x32(T, M, C):
    """fp32 activations with a full mantissa around the bf16 inputs."""
    g = torch.Generator().manual_seed(M * 7 + C)
    return T["x"].float() * (1 + 1e-3 * torch.randn(M, C, generator=g))


@pytest.mark.parametrize("M,C", TWO_TERM)
def test_two_term_forward_statistics_and_backward(M, C):
    """The walker's forms: statistics of an fp32 tensor, the fold on them, the forward's two-term store and the
    backward on fp32 x, each against its bound, NaN beforehand, two runs bit-equal."""
    O = ops()
    T = problem(M, C)
    x32 = _x32(T, M, C)
    xs = x32.to(DEV)
    st = O.bn_stats_f32(xs)
    ref, bound = B.stats_f32_ref(x32)
    assert st.rows == B.BN_ROWS and B.ratio(st.slab.cpu(), ref, bound) <= 1.0
    assert torch.equal(st.slab, O.bn_stats_f32(xs).slab)
    rm, rv = T["rm"].to(DEV), T["rv"].to(DEV)
    a, b, mr = _fold(O, st, M, T, True, rm, rv, None)
    R = B.fold_ref(st.slab.cpu(), M, T["gamma"], T["beta"], T["rm"], T["rv"])
    Bd, b_ref = B.fold_bounds(R, M, T["gamma"], T["beta"], T["rm"], T["rv"], a.cpu())
    assert B.ratio(a.cpu(), R["a"], Bd["a"]) <= 1.0 and B.ratio(b.cpu(), b_ref, Bd["b"]) <= 1.0
    a, b, mr = a.cpu(), b.cpu(), mr.cpu()
    B.plant_kink(x32, a, b)
    zero, pos, neg = B.kink_census(x32, a, b)
    assert zero >= 3 and pos > 0 and neg > 0
    xs = x32.to(DEV)
    outs = []
    for _ in range(2):
        y = nan_like((M, 2 * C), BF16)
        O.bn_act_fwd(xs, a.to(DEV), b.to(DEV), out=y, split=True)
        outs.append(y.cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    hi, lo = outs[0][:, :C], outs[0][:, C:]
    v, b32 = B.act_fwd_ref(x32, a, b)
    r = B.ratio(hi.double() + lo.double(), v, B.split_store(v, b32))
    print(f"two-term forward M={M} C={C}: {r:.3f}")
    assert r <= 1.0 and B.ratio(hi, v, B.bf16_store(v, b32)) <= 1.0
    eh, el = B.emulate_fwd(x32, a, b, split=True)
    assert torch.equal(_bits(hi.contiguous()), _bits(eh)) and torch.equal(_bits(lo.contiguous()), _bits(el))
    dy = T["dy"]
    for training in (True, False):
        outs = []
        for _ in range(2):
            dx, dg, db = nan_like((M, C), BF16), nan_like((C,), F32), nan_like((C,), F32)
            O.bn_act_bwd(dy.to(DEV), xs, a.to(DEV), b.to(DEV), mr.to(DEV), training=training, dgamma=dg, dbeta=db,
                         accumulate=False, out=dx)
            outs.append((dx.cpu(), dg.cpu(), db.cpu()))
        assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(*outs))
        Rb = B.act_bwd_ref(dy, x32, a, b, mr[:, 0], mr[:, 1], M, training=training)
        Bb = B.act_bwd_bounds(Rb, x32, a, mr[:, 0], mr[:, 1], M, training=training)
        res = {k: B.ratio(g, Rb[k], Bb[k]) for k, g in zip(("dx", "dgamma", "dbeta"), outs[0])}
        print(f"backward on fp32 x M={M} C={C} training={training}: " + " ".join(f"{k}={v:.3f}" for k, v in res.items()))
        assert all(v <= 1.0 for v in res.values()), res


def test_refusals_launch_nothing():
    from fmdiff import _lib
    L = _lib.lib()
    O = ops()
    s = O.stream()
    C = 8
    f = lambda *sh: torch.zeros(*sh, device=DEV, dtype=F32)   # noqa: E731
    h = lambda *sh: nan_like(sh, BF16)                          # noqa: E731
    slab, g, bt, rm, rv, a, b, mr = f(2, C, 2), f(C), f(C), f(C), f(C), nan_like((C,), F32), f(C), f(C, 2)
    nbt = torch.zeros((), dtype=torch.int64, device=DEV)
    p = lambda t: t.data_ptr()   # noqa: E731
    fold = lambda slab_p, Cc, M, a_p: L.fmd_bn_fold(slab_p, 2, Cc, M, p(g), p(bt), 1e-5, 0.1, 1, p(rm), p(rv), p(nbt),  # noqa: E731
                                                    a_p, p(b), p(mr), s)
    assert fold(p(slab), C, 1, p(a)) < 0            # one value per channel in training mode
    assert fold(p(slab), 12, 100, p(a)) < 0         # C not a multiple of 8
    assert fold(p(slab) + 4, C, 100, p(a)) < 0      # misaligned slab
    assert fold(p(slab), C, 100, p(a) + 2) < 0      # misaligned output
    x, y = h(16, C), h(16, C)
    assert L.fmd_bn_act_fwd(p(x), 16, 12, None, None, 0.2, p(y), s) < 0
    assert L.fmd_bn_act_fwd(p(x) + 2, 15, C, None, None, 0.2, p(y), s) < 0
    assert L.fmd_bn_act_fwd(p(x), 16, C, p(b), None, 0.2, p(y), s) < 0      # a without b
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    bwd = lambda x_p, Cc, M, tr: L.fmd_bn_act_bwd(p(x), x_p, M, Cc, p(b), p(b), p(mr), 0.2, tr, p(y), p(g), p(bt), 1, 0,  # noqa: E731
                                                   p(ws), s)
    assert bwd(p(x), 12, 16, 1) < 0 and bwd(p(x) + 2, C, 15, 1) < 0 and bwd(p(x), C, 1, 1) < 0
    assert L.fmd_image_stage(p(f(1, 1, 16)), 1, 1, 16, 12, 0, p(y), s) < 0
    assert L.fmd_image_stage(p(f(1, 1, 16)), 1, 1, 16, 8, 0, p(y) + 2, s) < 0
    torch.cuda.synchronize()
    assert int(nbt) == 0 and torch.isnan(a).all() and torch.isnan(y.float()).all()   # nothing ran
    with pytest.raises(RuntimeError):
        O.bn_fold(O.Stats(slab, 64), 1, g, bt, rm, rv, nbt)


@pytest.mark.parametrize("mode", ["identity", "clamp", "sigmoid"])
@pytest.mark.parametrize("N,C,H,W", [(3, 1, 5, 7), (2, 3, 16, 24), (2, 10, 9, 11)])
def test_image_stage(mode, N, C, H, W):
    O = ops()
    g = torch.Generator().manual_seed(N * 100 + C)
    x = torch.randn(N, C, H, W, generator=g) * 1.5
    x.view(-1)[:6] = torch.tensor([1.0, -1.0, 1.0000001, -1.0000001, 3.0, -3.0])
    m = O.IMAGE_MODES[mode]
    Cp = max(8, -(-C // 8) * 8)
    outs = []
    for _ in range(2):
        y = nan_like((N, H, W, Cp), BF16)
        O.image_stage(x.to(DEV), mode, out=y)
        outs.append(y.cpu())
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))
    y = outs[0]
    assert (_bits(y[..., C:]) == 0).all(), "padding channels must be exactly zero"
    v, b32 = B.image_ref(x, m)
    r = B.ratio(y[..., :C].permute(0, 3, 1, 2), v, B.bf16_store(v, b32) if m else 2.0 ** -9 * B.pow2_above(v.abs()))
    assert r <= 1.0, r
    # the two-term form: the hi half is the one-term output, hi + lo is within 2^-17 P(|v|), both paddings zero
    y2 = nan_like((N, H, W, 2 * Cp), BF16)
    O.image_stage(x.to(DEV), mode, out=y2, split=True)
    y2 = y2.cpu()
    assert torch.equal(_bits(y2[..., :Cp].contiguous()), _bits(y))
    assert (_bits(y2[..., C:Cp].contiguous()) == 0).all() and (_bits(y2[..., Cp + C:].contiguous()) == 0).all()
    two = (y2[..., :C].double() + y2[..., Cp:Cp + C].double()).permute(0, 3, 1, 2)
    assert B.ratio(two, v, B.split_store(v, b32)) <= 1.0
    # backward against torch's own autograd of the map
    gy = (torch.randn(N, H, W, Cp, generator=g)).to(BF16)
    dx = O.image_stage_bwd(gy.to(DEV), x.to(DEV), mode).cpu()
    xr = x.double().clone().requires_grad_()
    img = xr if m == 0 else (xr.clamp(-1.0, 1.0) + 1.0) * 0.5 if m == 1 else torch.sigmoid(xr)
    img.backward(gy[..., :C].permute(0, 3, 1, 2).double())
    vb, bb = B.image_bwd_ref(gy[..., :C].permute(0, 3, 1, 2), x, m)
    assert (vb - xr.grad).abs().max().item() < 1e-14
    assert B.ratio(dx, vb, bb) <= 1.0
    if m == 1:   # torch.clamp passes the gradient at the boundary: x = +-1 exactly
        flat, gflat = dx.view(-1), gy[..., :C].permute(0, 3, 1, 2).reshape(-1).float()
        assert flat[0] == gflat[0] * 0.5 and flat[1] == gflat[1] * 0.5 and (flat[2:6] == 0).all()
