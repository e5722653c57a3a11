"""The folded GroupNorm (csrc/groupnorm.hip) run through fmdiff.runtime.ops as the engine calls it -- channel_stats
-> gn_prep -> gn_apply_fwd (and gn_fused_apply where eligible), channel_stats(dz, y) -> gn_bwd_prep -> gn_bwd_apply
-- against an fp64 autograd reference with per-output, per-element error bounds (gn_bounds.py; test_gn_bounds.py
shows on the CPU that the bounds hold for the documented arithmetic and reject wrong kernels): every embedding
mode, two sources with groups that straddle the boundary, accumulating destinations and gradients, strided emb /
demb slots, the four-in-flight slab loops, folded slabs, NDHWC, 1x1 images and 256-channel groups, on white-noise,
correlated and large-offset inputs.  Also: the deferred gamma / beta fold on the straddling cases, and the two
forward-only folds inside a conv (halo prologue, fmd_conv_small) on a 256|128 concat."""
import functools

import pytest
import torch

import gn_bounds as gb

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = 24576.0          # bf16- and fp32-exact sentinel no output comes near
PAD = 64                # sentinel elements before and after each dx destination
FWD = ("a", "b", "mean", "rstd", "t")


def ops():
    from fmdiff.runtime import ops as O
    return O


@functools.lru_cache(maxsize=None)
def _case(case, dist):
    """Inputs, the fp64 reference (autograd; P, Q, R from the closed form) and the bounds: computed once."""
    inp = gb.make_inputs(case, dist)
    cf = gb.closed_form(inp)
    ref = gb.reference(inp)
    ref.update(P=cf["P"], Q=cf["Q"], R=cf["R"])
    return inp, ref, gb.bounds(inp, cf), gb.bounds(inp, cf, fused=True)


def _slab_check(st, terms, N, HW, tag):
    """Every slab entry against the fp64 sum of its own bf16 operands, within 1e-5 of the sum of their moduli."""
    C = terms[0].shape[-1]
    got = st.slab.double().cpu().reshape(N, HW // st.rows, C, 2)
    for k, t in enumerate(terms):
        t = t.reshape(N, HW // st.rows, st.rows, C)
        err = (got[..., k] - t.sum(2)).abs()
        assert bool((err <= 1e-5 * t.abs().sum(2) + gb.TINY).all()), (tag, k, float(err.max()))


def _slot(N, W, width, values=None):
    """A [N][W] fp32 buffer of sentinels and the view that starts at its slot (row stride W): what emb / demb are
    inside the engine's grouped-linear buffers."""
    off = 0 if W == width else 64
    buf = torch.full((N, W), SENT, device=DEV)
    if values is not None:
        buf[:, off:off + width] = values.to(DEV)
    return buf, buf[:, off:], off


def _dest(old, acc):
    """A bf16 destination between two sentinel pads: holding `old` where the kernel accumulates, sentinels else."""
    n = old.numel()
    buf = torch.full((n + 2 * PAD,), SENT, device=DEV, dtype=torch.bfloat16)
    view = buf[PAD:PAD + n].view(old.shape)
    if acc:
        view.copy_(old.to(DEV))
    return buf, view


def _pipeline(O, inp, defer=False):
    """The forward and backward as engine.py issues them; returns every output on the CPU."""
    c = inp["case"]
    N, HW, C, C0, C1, G, mode, W = c["N"], c["HW"], c["C"], c["C0"], c["C1"], c["G"], c["mode"], c["W"]
    sp = c["sp"]
    x = inp["x"].to(DEV)
    x0 = x[..., :C0].reshape(N, *sp, C0).contiguous()
    x1 = x[..., C0:].reshape(N, *sp, C1).contiguous() if C1 else None
    dz = inp["dz"].to(DEV).reshape(N, *sp, C).contiguous()
    gamma, beta = inp["gamma"].to(DEV), inp["beta"].to(DEV)
    st0 = O.channel_stats(x0, rows=c["rows0"])       # the default (64-pixel rows, or one row per image) unless
    st1 = O.channel_stats(x1, rows=c["rows1"]) if C1 else None   # the case sets its own, as conv epilogues do
    emb_buf, emb, emb_off = _slot(N, W, 2 * C, inp["emb"]) if mode == 1 else (None, None, 0)
    kw = dict(emb=emb, emb_stride=W, emb_mode=1) if mode == 1 else {}
    a, b, mr = O.gn_prep(st0, st1, N, HW, C0, C1, G, gb.EPS, gamma, beta, **kw)
    t = O.gn_apply_fwd(x0, x1, a, b)
    got = dict(a=a, b=b, mean=mr[..., 0], rstd=mr[..., 1], t=t.reshape(N, HW, C))
    fused = None
    if O.gn_fused_eligible(HW, C, C0, G):
        fa, fb, fmr, ft = O.gn_fused_apply(x0, x1, G, gb.EPS, gamma, beta, **kw)
        fused = dict(a=fa, b=fb, mean=fmr[..., 0], rstd=fmr[..., 1], t=ft.reshape(N, HW, C))
    # backward
    s12 = O.channel_stats(dz, y=(x0, x1, C0))
    assert s12.rows == c["rows"]
    dg, db = inp["dg0"].to(DEV), inp["db0"].to(DEV)
    demb_buf = demb = None
    width = {0: 0, 1: 2 * C, 2: C}[mode]
    if mode:
        demb_buf, demb, demb_off = _slot(N, W, width)
    bkw = dict(kw)
    if mode:
        bkw.update(emb_mode=mode, demb=demb, demb_stride=W)
    if mode == 2:
        bkw.update(fwd=st0)
    if defer:
        O.gb_defer()
    try:
        P, Q, R = O.gn_bwd_prep(s12, N, HW, C, G, mr, gamma, beta, dg, db, **bkw)
    finally:
        if defer:
            O.gb_flush()
    extra = inp["extra"].to(DEV).reshape(N, *sp, C).contiguous() if inp["extra"] is not None else None
    buf0, dx0 = _dest(inp["old0"].reshape(N, *sp, C0), c["acc0"])
    buf1, dx1 = _dest(inp["old1"].reshape(N, *sp, C1), c["acc1"]) if C1 else (None, None)
    O.gn_bwd_apply(dz, x0, x1, P, Q, R, extra, dx0, c["acc0"], dx1, c["acc1"])
    torch.cuda.synchronize()
    # nothing outside the written regions was touched
    for buf in (buf0, buf1):
        if buf is not None:
            assert bool((buf[:PAD] == SENT).all()) and bool((buf[-PAD:] == SENT).all())
    if mode:
        keep = torch.ones(W, dtype=torch.bool, device=DEV)
        keep[demb_off:demb_off + width] = False
        assert bool((demb_buf[:, keep] == SENT).all())
        assert not bool((demb_buf[:, ~keep] == SENT).any())
    if mode == 1:
        assert torch.equal(emb_buf[:, emb_off:emb_off + 2 * C], inp["emb"].to(DEV))
    got.update(P=P, Q=Q, R=R, dx0=dx0.reshape(N, HW, C0), dx1=dx1.reshape(N, HW, C1) if C1 else torch.empty(0),
               dgamma=dg, dbeta=db, demb=demb[:, :width] if mode else None)
    cpu = {k: (v.cpu() if v is not None else None) for k, v in got.items()}
    slabs = dict(st0=st0, st1=st1, s12=s12)
    return cpu, ({k: v.cpu() for k, v in fused.items()} if fused else None), slabs


@pytest.mark.parametrize("dist", gb.DISTRIBUTIONS)
@pytest.mark.parametrize("case", list(gb.CASES))
def test_groupnorm_bounds(case, dist, monkeypatch):
    O = ops()
    inp, ref, bnd, bnd_fused = _case(case, dist)
    c = inp["case"]
    N, HW, C0 = c["N"], c["HW"], c["C0"]
    if c["fold"] > 1:    # fmd_stats_fold forced on this slab (a fold that divides its 1100 rows)
        monkeypatch.setattr(O, "STATS_FOLD_MIN", 2)
        monkeypatch.setattr(O, "STATS_FOLD", c["fold"])
    got, fused, slabs = _pipeline(O, inp)
    E = HW // c["rows"]                     # fold_stats' own condition, on the host: only `folded` is folded
    assert (c["fold"] > 1) == bool(O.STATS_FOLD_MIN and E >= O.STATS_FOLD_MIN and E % O.STATS_FOLD == 0)
    assert c["fold"] == 1 or O.STATS_FOLD == c["fold"]
    assert bool(inp["dg0"].abs().min() > 0) and bool(inp["db0"].abs().min() > 0)
    x, dz = inp["x"].double(), inp["dz"].double()
    _slab_check(slabs["st0"], (x[..., :C0], x[..., :C0] ** 2), N, HW, "st0")
    if slabs["st1"] is not None:
        _slab_check(slabs["st1"], (x[..., C0:], x[..., C0:] ** 2), N, HW, "st1")
    _slab_check(slabs["s12"], (dz, dz * x), N, HW, "s12")
    ratios = gb.check_all(got, ref, bnd, f"{case} {dist}")
    print(f"GN_RATIO {case} {dist} " + " ".join(f"{n}={v:.3f}" for n, v in ratios.items()))
    if fused is not None:
        fr = gb.check_all(fused, ref, bnd_fused, f"{case} {dist} fused", names=FWD)
        print(f"GN_RATIO_FUSED {case} {dist} " + " ".join(f"{n}={v:.3f}" for n, v in fr.items()))


def test_fused_apply_is_reached():
    """The cases in which gn_fused_apply must meet the bounds too (source of truth: fmd_gn_fused_apply)."""
    O = ops()
    elig = [n for n in gb.CASES if O.gn_fused_eligible(*(gb.geometry(n)[k] for k in ("HW", "C", "C0", "G")))]
    assert elig == ["emb_add_slot", "ss_slot", "hw1", "cg256"], elig


def test_groups_wider_than_256_channels_are_refused():
    """fmd_gn_bwd_prep holds one group's channels in a 256-thread block: C / G > 256 is an error, not a wrong sum."""
    O = ops()
    N, HW, C = 2, 16, 512
    st = O.Stats(torch.zeros(N, C, 2, device=DEV), HW)
    mr = torch.ones(N, 1, 2, device=DEV)
    gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
    with pytest.raises(RuntimeError, match="fmd_gn_bwd_prep"):
        O.gn_bwd_prep(st, N, HW, C, 1, mr, gamma, beta, None, None)
    O.gn_bwd_prep(st, N, HW, C, 2, mr.expand(N, 2, 2).contiguous(), gamma, beta, None, None)   # C / G = 256: taken
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", ["straddle_cg24", "cfgB_256_128", "cfgB_512_256"])
def test_deferred_gamma_beta_on_straddling_groups(case):
    """gb_defer / gb_flush on real slabs of the straddling cases: dgamma / dbeta bit-equal to the direct call."""
    O = ops()
    inp = _case(case, "corr")[0]
    direct, _, _ = _pipeline(O, inp)
    deferred, _, _ = _pipeline(O, inp, defer=True)
    assert O._gb_pending is None
    assert torch.equal(direct["dgamma"], deferred["dgamma"]) and torch.equal(direct["dbeta"], deferred["dbeta"])
    assert not torch.equal(deferred["dgamma"], inp["dg0"])


# ---------------------------------------------------------------- the other forward folds on a straddling concat
def _fold_problem(N, H, K, dist):
    case = dict(N=N, sp=(H, H), C0=256, C1=128, G=32, mode=0)
    inp = gb.make_inputs(case, dist)
    # the second source on another scale and level, so that a straddling group fed from the wrong rows or the
    # wrong source is wrong by its whole size and not by the sampling noise of one common distribution
    inp["x"][..., 256:] = (0.5 * inp["x"][..., 256:].float() - 1.0).to(torch.bfloat16)
    cf = gb.closed_form(inp)
    c = inp["case"]
    assert [g for g in range(32) if gb.straddles(c, g)] == [21]
    x = inp["x"].to(DEV)
    x0, x1 = x[..., :256].reshape(N, H, H, 256).contiguous(), x[..., 256:].reshape(N, H, H, 128).contiguous()
    g = torch.Generator().manual_seed(K + H)
    w = (torch.randn(K, 384, 3, 3, generator=g) / (3 * 384 ** 0.5)).to(DEV)
    a, b = cf["a"].float().to(DEV), cf["b"].float().to(DEV)      # the fp64 fold, rounded to fp32
    return inp, x0, x1, w, a, b


def _routes_agree(got, ref, tag):
    """test_gpu_halo_fold.py's bound between two routes to the same conv: 8e-3 x scale, one bf16 step."""
    err, scale = (got.float() - ref.float()).abs().max().item(), ref.float().abs().max().item()
    print(f"GN_FOLD {tag} err/scale={err / scale:.2e}")
    assert err <= 8e-3 * scale, (tag, err, scale)


@pytest.mark.parametrize("dist", gb.DISTRIBUTIONS)
def test_halo_prologue_fold_on_a_straddling_concat(dist, monkeypatch):
    """conv(pro_fold=) on the halo path, 256|128 at 16x16 (group 21 = channels 252-263), against the same conv fed
    pro=(a, b, True) from the fp64 fold.  The kernel's fp32 rsqrtf against the fp64 1 / sqrt is part of that step."""
    O = ops()
    monkeypatch.setattr(O, "HALO_FOLD", True)
    N, H, K = 8, 16, 128
    inp, x0, x1, w, a, b = _fold_problem(N, H, K, dist)
    assert O.halo_eligible(N, H, H, H, K, Cin=384, pro=True)

    def no_separate_fold(*args, **kw):
        raise AssertionError("the halo path declined the fold: gn_prep ran as its own launch")

    wk = O.prep_weights(w, 0)
    f = dict(st0=O.channel_stats(x0), st1=O.channel_stats(x1), groups=32, eps=gb.EPS,
             gamma=inp["gamma"].to(DEV), beta=inp["beta"].to(DEV), emb=None, emb_stride=0)
    ref, _ = O.conv(x0, K, wk, src1=x1, pro=(a, b, True))
    monkeypatch.setattr(O, "_fold_now", no_separate_fold)
    got, _ = O.conv(x0, K, wk, src1=x1, pro_fold=f)
    torch.cuda.synchronize()
    _routes_agree(got, ref, f"halo {dist}")


@pytest.mark.parametrize("dist", gb.DISTRIBUTIONS)
def test_conv_small_fold_on_a_straddling_concat(dist):
    """fmd_conv_small's GroupNorm fold on the smallest 256|128, G = 32 shape it takes (2x2 images), against the
    implicit-GEMM conv fed pro=(a, b, True) from the fp64 fold."""
    O = ops()
    N, H, K = 2, 2, 128
    inp, x0, x1, w, a, b = _fold_problem(N, H, K, dist)
    wk = O.prep_weights(w, 0)
    gn = dict(st0=O.channel_stats(x0), st1=O.channel_stats(x1), groups=32, eps=gb.EPS,
              gamma=inp["gamma"].to(DEV), beta=inp["beta"].to(DEV))
    assert O.conv_small_ok(tuple(x0.shape), K, C1=128, mode="s1", gn=gn)
    got, _ = O.conv_small(x0, K, wk, src1=x1, mode="s1", gn=gn)
    ref, _ = O.conv(x0, K, wk, src1=x1, pro=(a, b, True))
    torch.cuda.synchronize()
    _routes_agree(got, ref, f"conv_small {dist}")
