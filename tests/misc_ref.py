"""fp64 restatements, exact lattices, error bounds, an fp32 emulation with mutants and the shared checks of the
glue kernels of csrc/misc.hip (time path, train / sampler steps, layout and resampling).  TEST INFRASTRUCTURE ONLY.

Layout.  Every family has
  * ``*_ref``: the documented operation (include/fmdiff.h, the reference Python the kernel comments name) in fp64;
    with ``dt=torch.float32`` the same statement runs in fp32, which is what ``Emu`` is built from;
  * ``check_*(O, dev, ...)``: the whole test of one case against an ``ops``-like namespace ``O``.  The GPU modules
    pass ``fmdiff.runtime.ops`` and "cuda"; test_misc_ref.py passes ``Emu()`` and "cpu", so the bounds, the
    lattices and the guards are proved on the CPU first, and ``Emu(mutant=...)`` shows that the very same check at
    the very same shapes rejects a kernel that is wrong in a known way;
  * ``Emu``: an fp32 CPU emulation of the documented arithmetic behind the wrappers' signatures.  Its reductions are
    explicit fp32 loops (one rounded product, one rounded add per term); ``Emu(perm=True)`` walks them in a
    permuted order, which must not change a single bit of a lattice case.

Technique 1, exact lattice.  Inputs are small dyadic rationals, so every fp32 product and partial sum the kernel can
form is exact in any order, with or without FMA contraction; the only rounding is the final store.  The fp64 value
cast to fp32 (then, for bf16 outputs, ``.to(torch.bfloat16)``, round to nearest even) must be ``torch.equal`` to the
kernel's output.  Lattices:
  linear family   x = k/8 |k| <= 32, w = k/16 |k| <= 16, bias = dy = k/8 |k| <= 16, old values k/4 |k| <= 64
                  (forward, dW, db, dx and their accumulation exact up to I = 1024, B = 32)
  bf16 pools      inputs k/4 |k| <= 31, old values k/4 |k| <= 100, scale 1, 1/4 or 1/8, at most 8 terms
  mse             pred - target on k/4 |k| <= 8 (sum of squares exact up to 2^14 elements)
  noise_prepare   x0, noise = k/8 |k| <= 32, ca, cb = k/8 |k| <= 8, cond = k/256 |k| <= 4096 (a real bf16 rounding)
  sched_step      x, eps = k/8 |k| <= 8; the chain coefficients c0, c3, c7, c8 in {0, +-1/2, +-1}, the others on
                  k/4 |k| <= 4 (all on the k/8 lattice); x is reloaded from the lattice before every step (ring and
                  last carry over), which keeps 6 steps within 24 bits
  lincomb         inputs k/8 |k| <= 32, coefficients k/8 |k| <= 16

Technique 2, fp64 bound (u = 2^-24, U = 2^-8, first order, asserted with attn_bounds.check at MARGIN):
  timestep_embedding  e = fl(fl(nlp f) / den) (two roundings), arg = fl(t_eff fl(expf(e))), out = sinf / cosf(arg):
                      |d arg| <= (2 |e| + 5) u |arg|, |d out| <= |d arg| + 2 u.  t t_scale is exact for every
                      t used here, so the truncation of t_eff is exact too.
  SiLU                t = z sigma(z) with the hardware exp and reciprocal: e_t = 8 u (1 + |z|) |t| (gn_bounds.py).
  silu_grad           g = s (1 + z (1 - s)) with the same s, relative error e_s = 8 u (1 + |z|):
                      d(1 - s) <= s e_s + u (1 - s);  in = 1 + z (1 - s): d in <= |z| (s e_s + 2 u (1 - s)) + u |in|;
                      e_g = s e_s (|in| + |z| s) + s (2 u |z| (1 - s) + u |in|) + u |g|.
  sums                |got - v| <= u |v| + n u sum|terms| + sum|term errors|, n the longest fp32 chain:
                      linear: n = ceil(I / 64) + 8 (lane chain, 6 shuffles, bias, product); grouped linear:
                      n = I / 4 + 5; dW: n = B + 2; dx with in_silu: the sum over O is exact on the lattice, so
                      e_dx = |sum| e_g + 2 u |sum g| + u |dx|.
  mse (3*3*35)        the sum of squares is exact on the lattice; inv = fl(1 / numel), the product in fp64 and one
                      store: |loss - v| <= 3 u |v|; dpred = bf16(fl(2 gs dlt inv)): U |v| + 3 u |v|.  Margin 1.
  adamw               one step from the kernel's own fp32 state, hyper-parameters at their fp32 ABI values:
                      e_m = u |gs| (1-b1) + 2 u |(gs - m)(1 - b1)| + u |m'|
                      e_v = u |v b2| + 5 u (1 - b2) gs^2 + u |v'|
                      e_den = (e_v / (2 sqrt v') + 4 u sqrt v') / sqrt(bc2) + u den
                      e_q = e_m / den + |m'| e_den / den^2 + u |q|;  e_s = (lr / bc1) e_q + 4 u |s|
                      e_p = 3 u |p| + e_s + u |p'|
                      (fmd_adamw takes bc1, bc2 from the host in fp64 -> fp32; fmd_adamw_sched forms them from its
                      fp32 betas in fp64, and lambda by get_cosine_schedule_with_warmup's formula in fp64.)
Bit equality without a lattice: flow_euler and ddpm_step promise the eager fp32 torch expression (no contraction,
correctly rounded division), so random fp32 inputs must give ``torch.equal``; sched_step promises the fmd_lincomb
chain, so a carried six-step run of random inputs must equal the same rows pushed through ``lincomb``.

Buffers.  Every output the test allocates lives inside a larger tensor with GUARD sentinel elements before and after
it (``guarded``); every padding a kernel must not read holds NaN; every padding it must write as zero is prefilled.

Largest err / bound seen on an MI355X (check()'s return value; bit-equal families have none):
  timestep_embedding 0.518 (dim 320, shift 1, t = 999)
  linear(in_silu) 0.022;  linear_bwd(in_silu) dw 0.247, dx 0.970 (the fp32 rounding of old + dx: met, not padded)
  GroupedLinear(in_silu) y 0.020, dw 0.247, dx 0.932;  silu_bwd 0.334
  mse (3*3*35, margin 1) loss 0.418, dpred 0.875 (one bf16 rounding)
  adamw p 0.302, m 0.839, v 0.929;  adamw_sched p 0.348, m 0.849, v 0.490
The fp32 emulation on the CPU gives the same figures to two digits except linear(in_silu) 0.072, GroupedLinear y
0.057, adamw p 0.502, adamw_sched p 0.581 and v 0.889, timestep_embedding 0.522.
"""
from __future__ import annotations

import math

import torch

from attn_bounds import MARGIN, TINY, U, check  # noqa: F401  (re-exported)
from gn_bounds import U32

BF16 = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
GUARD = 64            # sentinel elements on each side of a guarded buffer (keeps 16-byte alignment)
SENT = -768.0         # exact in bf16 and fp32, outside every lattice
RATIOS: dict = {}     # family -> largest err / bound seen by the checks of this process


def note(family: str, r: float) -> float:
    RATIOS[family] = max(RATIOS.get(family, 0.0), float(r))
    return r


def rng(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


def lat(shape, g, kmax: int, den: int, dtype=F32) -> torch.Tensor:
    """k / den with integer |k| <= kmax."""
    return (torch.randint(-kmax, kmax + 1, tuple(shape), generator=g).double() / den).to(dtype)


def f32(x: float) -> float:
    """x rounded to fp32 (what a ``float`` ABI argument carries)."""
    return float(torch.tensor(float(x), dtype=F32))


def guarded(shape, dtype, dev, fill=None):
    """(buffer, view): ``view`` of ``shape`` inside ``buffer`` with GUARD sentinels on each side."""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), SENT, dtype=dtype, device=dev)
    view = buf[GUARD:GUARD + n].view(tuple(shape))
    if fill is not None:
        view.copy_(fill) if torch.is_tensor(fill) else view.fill_(fill)
    return buf, view


def assert_guards(buf, name: str):
    b = buf.detach().cpu().float()
    n = b.numel() - 2 * GUARD
    assert bool((b[:GUARD] == SENT).all()) and bool((b[GUARD + n:] == SENT).all()), f"{name}: guard overwritten"


def assert_equal(got, want64, name: str, bf16=False):
    """Bit equality with the fp64 value rounded once (a NaN anywhere fails)."""
    want = want64.to(F32)
    if bf16:
        want = want.to(BF16)
    got = got.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{name}: {got.dtype} {tuple(got.shape)}"
    if not torch.equal(got, want):
        bad = ~(got.float() == want.float())
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ; first at {idx}: "
                             f"got {float(got[idx]):.9g} want {float(want[idx]):.9g}")


def _flat(t, shape, stride):
    """A strided window over ``t``'s storage starting at ``t``'s first element (what a raw pointer + stride sees)."""
    return torch.as_strided(t, tuple(shape), tuple(stride), t.storage_offset())


def silu64(z):
    return z * torch.sigmoid(z)


def silu_grad64(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def e_silu(z):
    """Evaluation error of SiLU with the hardware exp / reciprocal (gn_bounds.py's term)."""
    z = z.double()
    return 8 * U32 * (1 + z.abs()) * silu64(z).abs()


def e_silu_grad(z):
    z = z.double()
    s = torch.sigmoid(z)
    es = 8 * U32 * (1 + z.abs())
    inner = 1 + z * (1 - s)
    g = s * inner
    return s * es * (inner.abs() + z.abs() * s) + s * (2 * U32 * z.abs() * (1 - s) + U32 * inner.abs()) + U32 * g.abs()


# =============================================================================================== time path
TEMB_T = (0.0, 1.0, 17.0, 979.6122436523438, 999.0, 1000.0)
TEMB_DIMS = (2, 33, 128, 320)


def temb_trunc_t(half_step: bool) -> torch.Tensor:
    """t = j / 8 (t 999 is exact, an integer only for j % 8 == 0) or j / 8 + 1 / 16 (never an integer)."""
    t = torch.arange(0, 17, dtype=F32) / 8
    return t + 1.0 / 16 if half_step else t


def temb_ref(t, dim, flip, shift=0, max_period=10000.0, t_scale=1.0, t_trunc=False, dt=F64, mutant=None):
    """timestep_embedding of the reference (time_embedding.py) on t_eff = t t_scale, truncated toward zero when
    t_trunc ((t (N - 1)).long()).  Returns (embedding [N, dim], bound [N, dim])."""
    half = dim // 2
    tv = t.to(dt) * torch.tensor(t_scale, dtype=dt)
    if t_trunc:
        tv = tv.round() if mutant == "trunc_rounds" else tv.trunc()
    den = max(half if mutant == "half_no_shift" else half - shift, 1)
    e = (-math.log(max_period) * torch.arange(half, dtype=dt)) / den
    arg = tv[:, None] * torch.exp(e)[None, :]
    parts = [torch.sin(arg), torch.cos(arg)]
    if bool(flip) != (mutant == "flip_inverted"):
        parts = parts[::-1]
    earg = ((2 * e.abs() + 5) * U32)[None, :].double() * arg.abs().double() + 2 * U32
    cols, bnd = parts, [earg, earg]
    if dim % 2:
        z = torch.zeros_like(arg[:, :1])
        cols, bnd = cols + [z], bnd + [z.double()]
    return torch.cat(cols, -1), torch.cat(bnd, -1)


def check_temb(O, dev, dim, flip, shift, trunc=None):
    """trunc: None (t_scale 1), False (t = j/8, t_scale 999, t_trunc) or True (t = j/8 + 1/16)."""
    if trunc is None:
        t, kw = torch.tensor(TEMB_T, dtype=F32), {}
    else:
        t, kw = temb_trunc_t(trunc), dict(t_scale=999.0, t_trunc=True)
    got = O.timestep_embedding(t.to(dev), dim, bool(flip), shift, **kw).cpu()
    ref, bnd = temb_ref(t, dim, flip, shift, **kw)
    assert got.shape == ref.shape and got.dtype == F32
    if dim % 2:
        assert bool((got[:, -1] == 0).all()), "odd dim: the last column is exactly 0"
    return note("timestep_embedding", check(got, ref, bnd, f"temb dim={dim} flip={flip} shift={shift} trunc={trunc}"))


LINEAR_CASES = ((1, 128, 300), (8, 64, 5), (9, 200, 77), (32, 1024, 130))
LINEAR_BWD_CASES = tuple((B, I, Oo) for B in (1, 8, 9, 32) for I in (64, 200, 512) for Oo in (5, 300, 512))
COL0 = 3              # first column of a strided slice inside its wider row
EXTRA = 7             # columns a strided row has beyond the slice


def linear_inputs(B, I, Oo, seed):
    g = rng(seed)
    return dict(x=lat((B, I), g, 32, 8), w=lat((Oo, I), g, 16, 16), b=lat((Oo,), g, 16, 8), dy=lat((B, Oo), g, 16, 8),
                dw0=lat((Oo, I), g, 64, 4), db0=lat((Oo,), g, 64, 4), dx0=lat((B, I), g, 64, 4))


def linear_ref(x, w, b, in_silu=False):
    xin = silu64(x.double()) if in_silu else x.double()
    y = xin @ w.double().t()
    return y if b is None else y + b.double()


def linear_bound(x, w, b, v, n):
    """in_silu forward: SiLU evaluation of every term + a chain of n fp32 operations."""
    s = silu64(x.double()).abs()
    aw = w.double().abs().t()
    ab = 0.0 if b is None else b.double().abs()
    return e_silu(x) @ aw + (n + 1) * U32 * (s @ aw + ab) + U32 * v.abs()


def linear_bwd_ref(x, w, dy, dw0, db0, dx0, in_silu=False):
    """(dw, db, dx) with dw0 / db0 / dx0 the values accumulated into (dx0 None: dx is overwritten)."""
    x, w, dy = x.double(), w.double(), dy.double()
    xin = silu64(x) if in_silu else x
    dw = dw0.double() + dy.t() @ xin
    db = None if db0 is None else db0.double() + dy.sum(0)
    sv = dy @ w
    dx = sv * silu_grad64(x) if in_silu else sv
    if dx0 is not None:
        dx = dx + dx0.double()
    return dw, db, dx


def linear_bwd_bounds(x, w, dy, dw0, dw, dx):
    """in_silu backward bounds of (dw, dx); db has no SiLU in it and stays exact."""
    B = x.shape[0]
    ady = dy.double().abs()
    s = silu64(x.double()).abs()
    e_dw = ady.t() @ e_silu(x) + (B + 2) * U32 * (ady.t() @ s + dw0.double().abs()) + U32 * dw.abs()
    sv = dy.double() @ w.double()
    e_dx = sv.abs() * e_silu_grad(x) + 2 * U32 * (sv * silu_grad64(x.double())).abs() + U32 * dx.abs()
    return e_dw, e_dx


def _strided(dev, B, Oo, strided, fill):
    """A [B, Oo] window (optionally a column slice of wider rows) inside a guarded buffer filled with ``fill``."""
    ld = Oo + EXTRA if strided else Oo
    buf, full = guarded((B, ld), F32, dev, fill)
    return buf, full, (full[:, COL0:COL0 + Oo] if strided else full), ld


def _nan_rows(t, dev, extra=2):
    """``t`` followed by ``extra`` rows of NaN the kernel must never read (rows >= B)."""
    full = torch.full((t.shape[0] + extra, *t.shape[1:]), float("nan"), dtype=t.dtype)
    full[:t.shape[0]] = t
    return full.to(dev)[:t.shape[0]]


def check_linear(O, dev, B, I, Oo, bias=True, strided=False, in_silu=False, seed=11):
    d = linear_inputs(B, I, Oo, seed)
    x, w, b = _nan_rows(d["x"], dev), d["w"].to(dev), (d["b"].to(dev) if bias else None)
    buf, full, out, ld = _strided(dev, B, Oo, strided, SENT)
    O.linear(x, w, b, in_silu=in_silu, out=out, out_stride=ld if strided else None)
    name = f"linear B={B} I={I} O={Oo} bias={bias} strided={strided} silu={in_silu}"
    assert_guards(buf, name)
    got = full.cpu()
    if strided:
        assert bool((got[:, :COL0] == SENT).all()) and bool((got[:, COL0 + Oo:] == SENT).all()), \
            f"{name}: columns next to the slice overwritten"
        got = got[:, COL0:COL0 + Oo]
    ref = linear_ref(d["x"], d["w"], d["b"] if bias else None, in_silu)
    if not in_silu:
        assert_equal(got, ref, name)
        return None
    bnd = linear_bound(d["x"], d["w"], d["b"] if bias else None, ref, (I + 63) // 64 + 8)
    return note("linear(in_silu)", check(got, ref, bnd, name))


def check_linear_bwd(O, dev, B, I, Oo, dx_acc=False, strided=False, in_silu=False, want_dx=True, want_dw=True,
                     seed=13):
    d = linear_inputs(B, I, Oo, seed)
    name = f"linear_bwd B={B} I={I} O={Oo} acc={dx_acc} strided={strided} silu={in_silu} dx={want_dx} dw={want_dw}"
    x, w = _nan_rows(d["x"], dev), d["w"].to(dev)
    bdy, fdy, dy, ld = _strided(dev, B, Oo, strided, float("nan"))
    dy.copy_(d["dy"])
    runs = []
    for _ in range(2):                                  # two runs from equal state: the order is fixed
        bw, dw = guarded((Oo, I), F32, dev, d["dw0"])
        bb, db = guarded((Oo,), F32, dev, d["db0"])
        bx, dx = guarded((B, I), F32, dev, d["dx0"] if dx_acc else SENT + 1)
        O.linear_bwd(x, w, dy, dw if want_dw else None, db if want_dw else None, dx=dx if want_dx else None,
                     dx_acc=dx_acc, in_silu=in_silu, dy_stride=ld if strided else None)
        for bf, n in ((bw, "dw"), (bb, "db"), (bx, "dx")):
            assert_guards(bf, f"{name} {n}")
        runs.append((dw.cpu(), db.cpu(), dx.cpu()))
    for a, b_, n in zip(runs[0], runs[1], ("dw", "db", "dx")):
        assert torch.equal(a, b_), f"{name}: {n} differs between two runs"
    rdw, rdb, rdx = linear_bwd_ref(d["x"], d["w"], d["dy"], d["dw0"], d["db0"], d["dx0"] if dx_acc else None, in_silu)
    gdw, gdb, gdx = runs[0]
    if not want_dw:                                     # untouched
        rdw, rdb = d["dw0"].double(), d["db0"].double()
    if not want_dx:
        rdx = torch.full_like(rdx, SENT + 1)
    assert_equal(gdb, rdb, f"{name} db")
    if not in_silu:
        assert_equal(gdw, rdw, f"{name} dw")
        assert_equal(gdx, rdx, f"{name} dx")
        return None
    e_dw, e_dx = linear_bwd_bounds(d["x"], d["w"], d["dy"], d["dw0"], rdw, rdx)
    r = 0.0
    if want_dw:
        r = max(r, note("linear_bwd(in_silu) dw", check(gdw, rdw, e_dw, f"{name} dw")))
    else:
        assert_equal(gdw, rdw, f"{name} dw")
    if want_dx:
        r = max(r, note("linear_bwd(in_silu) dx", check(gdx, rdx, e_dx, f"{name} dx")))
    else:
        assert_equal(gdx, rdx, f"{name} dx")
    return r


GL_GROUPS = (64, 100, 1, 256)     # a ragged last block (100 = 64 + 36) and a single-row group
GL_NOBIAS = 1                     # the group built with bias=None
# (B, I) the host takes both ways: B I 4 <= 64 KiB forward, (B I + 64 BM) 4 <= 64 KiB backward (BM = 8 or 32)
GL_CASES = tuple((B, I) for I in (128, 256, 512, 1024) for B in (1, 8, 9, 32) if B * I + 64 * 32 <= 16384)


def gl_inputs(B, I, seed):
    g = rng(seed)
    tot = sum(GL_GROUPS)
    return dict(x=lat((B, I), g, 32, 8), dy=lat((B, tot), g, 16, 8), dx0=lat((B, I), g, 64, 4),
                w=[lat((n, I), g, 16, 16) for n in GL_GROUPS], b=[lat((n,), g, 16, 8) for n in GL_GROUPS],
                dw0=[lat((n, I), g, 64, 4) for n in GL_GROUPS], db0=[lat((n,), g, 64, 4) for n in GL_GROUPS])


def _gl_modules(d, I, dev):
    """torch.nn.Linear modules holding the lattice weights; their .grad are guarded views with the old values."""
    lins, bufs = [], []
    for k, n in enumerate(GL_GROUPS):
        lin = torch.nn.Linear(I, n, bias=k != GL_NOBIAS).to(dev)
        with torch.no_grad():
            lin.weight.copy_(d["w"][k])
            if lin.bias is not None:
                lin.bias.copy_(d["b"][k])
        bw, gw = guarded((n, I), F32, dev, d["dw0"][k])
        lin.weight.grad = gw
        bufs.append(bw)
        if lin.bias is not None:
            bb, gb = guarded((n,), F32, dev, d["db0"][k])
            lin.bias.grad = gb
            bufs.append(bb)
        lins.append(lin)
    return lins, bufs


def check_grouped_linear(O, dev, B, I, dx_acc=False, in_silu=False, seed=17):
    d = gl_inputs(B, I, seed)
    name = f"grouped_linear B={B} I={I} acc={dx_acc} silu={in_silu}"
    x, dy = d["x"].to(dev), d["dy"].to(dev)
    bias = [None if k == GL_NOBIAS else d["b"][k] for k in range(len(GL_GROUPS))]
    yref = torch.cat([linear_ref(d["x"], d["w"][k], bias[k], in_silu) for k in range(len(GL_GROUPS))], 1)
    off = [sum(GL_GROUPS[:k]) for k in range(len(GL_GROUPS))]
    refs = [linear_bwd_ref(d["x"], d["w"][k], d["dy"][:, off[k]:off[k] + n], d["dw0"][k],
                           None if k == GL_NOBIAS else d["db0"][k], None, in_silu) for k, n in enumerate(GL_GROUPS)]
    sv = sum(d["dy"][:, off[k]:off[k] + n].double() @ d["w"][k].double() for k, n in enumerate(GL_GROUPS))
    rdx = sv * silu_grad64(d["x"].double()) if in_silu else sv
    if dx_acc:
        rdx = rdx + d["dx0"].double()
    runs = []
    for _ in range(2):
        lins, bufs = _gl_modules(d, I, dev)
        gl = O.GroupedLinear(lins, in_silu)
        y = gl.forward(x)
        bx, dx = guarded((B, I), F32, dev, d["dx0"] if dx_acc else SENT + 1)
        gl.backward(x, dy, dx=dx, dx_acc=dx_acc)
        for bf in bufs + [bx]:
            assert_guards(bf, name)
        runs.append([y.cpu(), dx.cpu()] + [l.weight.grad.cpu() for l in lins]
                    + [l.bias.grad.cpu() for l in lins if l.bias is not None])
    for a, b_ in zip(*runs):
        assert torch.equal(a, b_), f"{name}: two runs differ"
    gy, gdx = runs[0][0], runs[0][1]
    gdw = runs[0][2:2 + len(GL_GROUPS)]
    gdb = iter(runs[0][2 + len(GL_GROUPS):])
    r = 0.0
    for k, n in enumerate(GL_GROUPS):
        if k != GL_NOBIAS:
            assert_equal(next(gdb), refs[k][1], f"{name} db[{k}]")
    if not in_silu:
        assert_equal(gy, yref, f"{name} y")
        assert_equal(gdx, rdx, f"{name} dx")
        for k in range(len(GL_GROUPS)):
            assert_equal(gdw[k], refs[k][0], f"{name} dw[{k}]")
        return None
    for k, n in enumerate(GL_GROUPS):
        sl = slice(off[k], off[k] + n)
        bnd = linear_bound(d["x"], d["w"][k], bias[k], yref[:, sl], I // 4 + 5)
        r = max(r, note("GroupedLinear(in_silu) y", check(gy[:, sl], yref[:, sl], bnd, f"{name} y[{k}]")))
        e_dw, _ = linear_bwd_bounds(d["x"], d["w"][k], d["dy"][:, sl], d["dw0"][k], refs[k][0], refs[k][2])
        r = max(r, note("GroupedLinear(in_silu) dw", check(gdw[k], refs[k][0], e_dw, f"{name} dw[{k}]")))
    e_dx = sv.abs() * e_silu_grad(d["x"]) + 2 * U32 * (sv * silu_grad64(d["x"].double())).abs() + U32 * rdx.abs()
    return max(r, note("GroupedLinear(in_silu) dx", check(gdx, rdx, e_dx, f"{name} dx")))


# grid_for(n) caps the grid at 16384 blocks of 256 threads: only n above 16384 * 256 makes a thread stride
# (70001 elements are 274 blocks, one pass), so the smallest striding length is in the list too.
SILU_BWD_N = (1, 255, 257, 70001, 16384 * 256 + 1)
SILU_SPECIAL = (0.0, 88.0, -88.0, 1e-40, -1e-40, 30.0, -30.0)


def silu_bwd_inputs(n, seed=19):
    g = rng(seed)
    z = (torch.rand(n, generator=g) * 60 - 30).to(F32)
    k = min(n, len(SILU_SPECIAL))
    z[:k] = torch.tensor(SILU_SPECIAL[(n % len(SILU_SPECIAL)):] + SILU_SPECIAL[:(n % len(SILU_SPECIAL))])[:k]
    return z, torch.randn(n, generator=g)


def check_silu_bwd(O, dev, n):
    z, dy = silu_bwd_inputs(n)
    got = O.silu_bwd(z.to(dev), dy.to(dev)).cpu()
    ref = dy.double() * silu_grad64(z.double())
    bnd = dy.double().abs() * e_silu_grad(z) + U32 * ref.abs()
    return note("silu_bwd", check(got, ref, bnd, f"silu_bwd n={n}"))


# =============================================================================================== train / sampler steps
STEP_N, STEP_SP = 3, (5, 7)       # HW = 35: a multiple of nothing


def _bc(c, like):
    return c.view(-1, *[1] * (like.dim() - 1))


def _to_nhwc_pad(v, Cpad):
    """[N, C, *S] -> [N, *S, Cpad] with zero pad channels."""
    v = v.movedim(1, -1)
    return torch.cat([v, v.new_zeros(*v.shape[:-1], Cpad - v.shape[-1])], -1)


def _nhwc_nan(v, Kpad, dev):
    """[N, C, *S] fp32 -> device [N, *S, Kpad] with NaN in channels >= C (a UNet output's unread padding)."""
    v = v.movedim(1, -1)
    return torch.cat([v, torch.full((*v.shape[:-1], Kpad - v.shape[-1]), float("nan"))], -1).contiguous().to(dev)


def noise_prepare_ref(x0, noise, ca, cb, cond, Cpad, dt=F64):
    """ca and cb: ca[n] x0 + cb[n] noise (DDPM add_noise); ca only: (1 - ca[n]) x0 + ca[n] noise (FM, ca = t);
    neither: noise.  Then the cond channels, then zeros: [N, *S, Cpad]."""
    nz = noise.to(dt)
    if ca is not None and cb is not None:
        v = _bc(ca.to(dt), nz) * x0.to(dt) + _bc(cb.to(dt), nz) * nz
    elif ca is not None:
        v = (1 - _bc(ca.to(dt), nz)) * x0.to(dt) + _bc(ca.to(dt), nz) * nz
    else:
        v = nz
    if cond is not None:
        v = torch.cat([v, cond.to(dt)], 1)
    return _to_nhwc_pad(v, Cpad)


def noise_prepare_inputs(mode, Cx, Cc, seed=23):
    g = rng(seed)
    sh = (STEP_N, Cx, *STEP_SP)
    d = dict(x0=lat(sh, g, 32, 8), noise=lat(sh, g, 32, 8), ca=lat((STEP_N,), g, 8, 8), cb=lat((STEP_N,), g, 8, 8),
             cond=lat((STEP_N, Cc, *STEP_SP), g, 4096, 256) if Cc else None)
    if mode != "ddpm":
        d["cb"] = None
    if mode == "copy":
        d["x0"] = d["ca"] = None
    return d


def check_noise_prepare(O, dev, mode, Cx, Cc, Cpad, reuse_out=False):
    d = noise_prepare_inputs(mode, Cx, Cc)
    name = f"noise_prepare {mode} Cx={Cx} Cc={Cc} Cpad={Cpad} out={reuse_out}"
    a = {k: (None if v is None else v.to(dev)) for k, v in d.items()}
    if reuse_out:
        buf, out = guarded((STEP_N, *STEP_SP, Cpad), BF16, dev, 3.0)     # pad channels must be WRITTEN as zero
        got = O.noise_prepare(a["x0"], a["noise"], a["ca"], a["cb"], a["cond"], Cpad, out=out)
        assert got.data_ptr() == out.data_ptr(), f"{name}: out= not reused"
        assert_guards(buf, name)
    else:
        got = O.noise_prepare(a["x0"], a["noise"], a["ca"], a["cb"], a["cond"], Cpad)
    assert_equal(got, noise_prepare_ref(d["x0"], d["noise"], d["ca"], d["cb"], d["cond"], Cpad), name, bf16=True)


def mse_ref(pred, ta, tb, tb_sign, grad_scale, dt=F64, mutant=None):
    """pred [N, *S, Kpad] (channels >= Cx unread), ta / tb [N, Cx, *S]: loss = mean((pred - (ta + sign tb))^2)
    and dpred = grad_scale 2 (pred - target) / numel on the Cx channels, exactly 0 on the rest."""
    Cx, Kpad = ta.shape[1], pred.shape[-1]
    target = ta.to(dt)
    if tb is not None:
        target = target + (1.0 if mutant == "tb_sign_dropped" else tb_sign) * tb.to(dt)
    dlt = pred[..., :Cx].to(dt) - target.movedim(1, -1)
    numel = dlt.numel() * (Kpad if mutant == "inv_numel_kpad" else Cx) // Cx
    inv = (torch.ones((), dtype=dt) / numel)
    loss = (dlt * dlt).sum() * inv
    g = (grad_scale * 2.0) * dlt * inv
    return loss, torch.cat([g, g.new_zeros(*g.shape[:-1], Kpad - Cx)], -1), dlt, inv


def mse_inputs(kind, Cx, Kpad, seed=29):
    """kind "pow2": N Cx HW = 4 x 1 x 32 (loss and dpred exact); "odd": 3 x Cx x 35."""
    g = rng(seed)
    N, sp = (4, (4, 8)) if kind == "pow2" else (STEP_N, STEP_SP)
    sh = (N, Cx, *sp)
    return dict(pred=lat(sh, g, 3, 4), ta=lat(sh, g, 3, 4), tb=lat(sh, g, 2, 4), Kpad=Kpad)


def check_mse(O, dev, kind, Cx, Kpad, tb_sign=None, grad_scale=1.0, with_dpred=True, npartial=64):
    d = mse_inputs(kind, Cx, Kpad)
    name = f"mse {kind} Cx={Cx} Kpad={Kpad} tb={tb_sign} gs={grad_scale} dpred={with_dpred} partial={npartial}"
    pred = _nhwc_nan(d["pred"], Kpad, dev)
    ta = d["ta"].to(dev)
    tb = None if tb_sign is None else d["tb"].to(dev)
    bl, loss = guarded((1,), F32, dev)
    bp, partial = guarded((npartial,), F32, dev)
    bd, dpred = guarded(tuple(pred.shape), BF16, dev, 3.0)
    O.mse(pred, ta, tb, tb_sign if tb_sign is not None else 1.0, grad_scale, loss, partial,
          dpred if with_dpred else None)
    for bf in (bl, bp, bd):
        assert_guards(bf, name)
    blocks = min(npartial, (pred.numel() + 255) // 256)
    assert bool((partial.cpu()[blocks:] == SENT).all()), f"{name}: partial written past the grid"
    rl, rg, _, _ = mse_ref(pred.cpu(), d["ta"], None if tb_sign is None else d["tb"], tb_sign or 1.0, grad_scale)
    gl, gd = loss.cpu()[0], dpred.cpu()
    if not with_dpred:
        assert bool((gd == 3.0).all()), f"{name}: dpred written although None was passed"
    else:
        assert bool((gd[..., Cx:] == 0).all()), f"{name}: dpred pad channels are not exactly 0"
    if kind == "pow2":
        assert_equal(gl, rl, f"{name} loss")
        if with_dpred:
            assert_equal(gd, rg, f"{name} dpred", bf16=True)
        return None
    r = note("mse loss", check(gl, rl, 3 * U32 * rl.abs(), f"{name} loss", margin=1.0))
    if with_dpred:
        r = max(r, note("mse dpred", check(gd, rg, (U + 3 * U32) * rg.abs(), f"{name} dpred", margin=1.0)))
    return r


# ----------------------------------------------------------------------------------------------- AdamW
ADAMW_N = (1, 3, 4, 5, 1027)
ADAMW_HP = dict(lr=1e-3, b1=0.9, b2=0.999, eps=1e-8)
ADAMW_SPECIAL = (0.0, 1e4, 1e-12)
SCHED_WARMUP, SCHED_TOTAL = 2, 6
SCHED_STEPS = (0, 1, 2, 3, 5, 6, 7, 8)      # scheduler steps s; the jump 3 -> 5 is a counter_add of 2


def cosine_lambda(s: int, warmup: int, total: int) -> float:
    """get_cosine_schedule_with_warmup's lr_lambda (num_cycles = 0.5), written out."""
    if s < warmup:
        return float(s) / float(max(1, warmup))
    progress = float(s - warmup) / float(max(1, total - warmup))
    return max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * progress)))


def adamw_ref(p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2, grad_scale=1.0):
    """One torch.optim.AdamW step in fp64 from the given state.  Returns ((p, m, v), (e_p, e_m, e_v))."""
    u = U32
    p, g, m, v = (t.double() for t in (p, g, m, v))
    gs = g * grad_scale
    p1 = p * (1 - lr * wd)
    m1 = m + (gs - m) * (1 - b1)
    v1 = v * b2 + (1 - b2) * gs * gs
    rt = v1.sqrt()
    den = rt / math.sqrt(bc2) + eps
    q = m1 / den
    s = (lr / bc1) * q
    p2 = p1 - s
    e_m = u * gs.abs() * (1 - b1) + 2 * u * ((gs - m) * (1 - b1)).abs() + u * m1.abs()
    e_v = u * (v * b2).abs() + 5 * u * (1 - b2) * gs * gs + u * v1
    half = torch.where(rt > 0, e_v / (2 * rt.clamp(min=TINY)), torch.zeros_like(rt))
    e_den = (half + 4 * u * rt) / math.sqrt(bc2) + u * den
    e_q = e_m / den + m1.abs() * e_den / (den * den) + u * q.abs()
    e_s = (lr / bc1) * e_q + 4 * u * s.abs()
    e_p = 3 * u * p.abs() + e_s + u * p2.abs()
    return (p2, m1, v1), (e_p, e_m, e_v)


def adamw_grad(n, step, seed=31):
    g = torch.randn(n, generator=rng(seed + step))
    for j in range(min(n, 3)):
        g[j] = ADAMW_SPECIAL[(j + step) % 3]
    return g


def _offset_view(t, off, dev):
    """``t`` at an element offset inside a guarded buffer: (buffer, view); view[:0] .. the offset hold SENT."""
    buf, full = guarded((off + t.numel(),), F32, dev)
    full[off:].copy_(t)
    return buf, full[off:]


def check_adamw(O, dev, n, off, wd, sched, grad_scale=1.0, steps=None):
    """Six fmd_adamw steps (sched False) or the schedule's eight fmd_adamw_sched steps, each compared with one fp64
    step from the kernel's own previous fp32 state; the step is also repeated from a copy of that state."""
    hp = {k: f32(v) for k, v in ADAMW_HP.items()}
    wd32 = f32(wd)
    name = f"adamw{'_sched' if sched else ''} n={n} off={off} wd={wd} gs={grad_scale}"
    g0 = rng(37 + n)
    bufs = [_offset_view(t, off, dev) for t in (torch.randn(n, generator=g0), torch.zeros(n), torch.zeros(n))]
    (bp, p), (bm, m), (bv, v) = bufs
    ctr = torch.zeros(1, dtype=torch.int32, device=dev)
    seq = list(SCHED_STEPS if sched else range(6)) if steps is None else list(steps)
    r = 0.0
    for k, s in enumerate(seq):
        if sched:
            cur = int(ctr.cpu()[0])
            if s != cur:
                O.counter_add(ctr, s - cur)
                assert int(ctr.cpu()[0]) == s, f"{name}: counter_add({s - cur})"
        step = s + 1
        bg, g = _offset_view(adamw_grad(n, step), off, dev)
        prev = [t.cpu().clone() for t in (p, m, v)]
        twin = [_offset_view(t, off, dev) for t in prev]

        def run(pp, mm, vv):
            if sched:
                O.adamw_sched(pp, g, mm, vv, ctr, ADAMW_HP["lr"], SCHED_WARMUP, SCHED_TOTAL, ADAMW_HP["b1"],
                              ADAMW_HP["b2"], ADAMW_HP["eps"], wd, grad_scale)
            else:
                O.adamw(pp, g, mm, vv, ADAMW_HP["lr"], ADAMW_HP["b1"], ADAMW_HP["b2"], ADAMW_HP["eps"], wd, step)
        run(p, m, v)
        run(*[t[1] for t in twin])
        for (bf, _), what in zip(bufs + twin + [(bg, g)], "p m v p2 m2 v2 g".split()):
            assert_guards(bf, f"{name} step {step} {what}")
            assert bool((bf.cpu()[GUARD:GUARD + off] == SENT).all()), f"{name}: {what} written below its offset"
        got = [t.cpu() for t in (p, m, v)]
        for a, (_, b_), what in zip(got, twin, "pmv"):
            assert torch.equal(a, b_.cpu()), f"{name} step {step}: {what} differs between two runs"
        if sched:
            lr = hp["lr"] * cosine_lambda(s, SCHED_WARMUP, SCHED_TOTAL)
            bc1, bc2 = 1.0 - hp["b1"] ** step, 1.0 - hp["b2"] ** step
        else:                                           # the wrapper's host arithmetic, then the fp32 ABI
            lr = hp["lr"]
            bc1, bc2 = f32(1.0 - ADAMW_HP["b1"] ** step), f32(1.0 - ADAMW_HP["b2"] ** step)
        ref, bnd = adamw_ref(*prev[:1], g.cpu(), *prev[1:], lr, hp["b1"], hp["b2"], hp["eps"], wd32, bc1, bc2,
                             grad_scale if sched else 1.0)
        fam = "adamw_sched" if sched else "adamw"
        for a, rf, bd, what in zip(got, ref, bnd, "pmv"):
            r = max(r, note(f"{fam} {what}", check(a, rf, bd, f"{name} step {step} {what}")))
    return r


# ----------------------------------------------------------------------------------------------- sampler steps
def next_ref(x_new, cond, Cpad):
    """The next model input: bf16 RNE of x, then the cond channels, then zeros ([N, *S, Cpad])."""
    v = x_new.float() if cond is None else torch.cat([x_new.float(), cond.float()], 1)
    return _to_nhwc_pad(v, Cpad).to(BF16)


def flow_euler_eager(x, v, sigmas, idx):
    """The eager fp32 expression FlowMatchEulerDiscreteScheduler.step evaluates."""
    return x + (sigmas[idx + 1] - sigmas[idx]) * v


def ddpm_eager(x, e, row, z):
    """The eager fp32 expression of the DDPM / DDIM step: row = [sqrt_b, sqrt_a, c_x0, c_xt, std, clip, c_eps]."""
    sqrt_b, sqrt_a, cx0, cxt, sd, clip, ceps = (row[k] for k in range(7))
    x0 = (x - sqrt_b * e) / sqrt_a
    if float(clip) > 0:
        x0 = x0.clamp(-clip, clip)
    pv = cx0 * x0 + cxt * x if float(cxt) != 0 else cx0 * x0
    if float(ceps) != 0:
        pv = pv + ceps * e
    if z is not None and float(sd) > 0:
        pv = pv + sd * z
    return pv


def _table(row, idx, nrows, dev):
    """``row`` at index ``idx`` of a table whose other rows are NaN (any other read must show)."""
    t = torch.full((nrows, *row.shape), float("nan"), dtype=row.dtype)
    t[idx] = row
    return t.to(dev)


STEP_IDX = 3


def _step_setup(dev, Cx, Cc, with_next, seed):
    g = rng(seed)
    sh = (STEP_N, Cx, *STEP_SP)
    x = 2 * torch.randn(sh, generator=g)
    mo = torch.randn(sh, generator=g)
    cond = torch.randn((STEP_N, Cc, *STEP_SP), generator=g) if Cc else None
    bx, xd = guarded(sh, F32, dev, x)
    bn, nx = guarded((STEP_N, *STEP_SP, 8), BF16, dev, 3.0) if with_next else (None, None)
    idx = torch.tensor([STEP_IDX], dtype=torch.int32, device=dev)
    return g, x, mo, cond, bx, xd, bn, nx, idx


def _step_verify(name, want, cond, bx, xd, bn, nx):
    assert_guards(bx, name)
    got = xd.cpu()
    assert torch.equal(got, want), f"{name}: x is not bit-equal to the eager fp32 expression " \
        f"({int((got != want).sum())} of {want.numel()} differ)"
    if nx is not None:
        assert_guards(bn, name)
        assert torch.equal(nx.cpu(), next_ref(want, cond, 8)), f"{name}: next"


def check_flow_euler(O, dev, Cx, Cc, with_next=True):
    name = f"flow_euler Cx={Cx} Cc={Cc} next={with_next}"
    g, x, v, cond, bx, xd, bn, nx, idx = _step_setup(dev, Cx, Cc, with_next, 41)
    sig = torch.full((6,), float("nan"))
    sig[STEP_IDX], sig[STEP_IDX + 1] = 0.7331, 0.4127
    O.flow_euler(xd, _nhwc_nan(v, 8, dev), sig.to(dev), idx, None if cond is None else cond.to(dev), nx)
    _step_verify(name, flow_euler_eager(x, v, sig, STEP_IDX), cond, bx, xd, bn, nx)


# name: (sqrt_b, sqrt_a, c_x0, c_xt, std, clip, c_eps), noise ("buf" / "table0" / "table2" / None)
DDPM_ROWS = {
    "ddpm_clip":      ((0.6, 0.8, 0.31, 0.67, 0.21, 1.0, 0.0), "buf"),
    "ddpm_noclip":    ((0.6, 0.8, 0.31, 0.67, 0.21, 0.0, 0.0), "buf"),
    "cxt0":           ((0.6, 0.8, 0.93, 0.0, 0.0, 1.0, 0.0), None),
    "ddim":           ((0.43, 0.9, 0.77, 0.0, 0.0, 1.0, 0.59), None),
    "table_base0":    ((0.6, 0.8, 0.31, 0.67, 0.21, 1.0, 0.0), "table0"),
    "table_base2":    ((0.6, 0.8, 0.31, 0.67, 0.21, 1.0, 0.0), "table2"),
    "sd_no_noise":    ((0.6, 0.8, 0.31, 0.67, 0.21, 1.0, 0.0), None),
}


def check_ddpm_step(O, dev, rowname, Cx, Cc=3, with_next=True):
    name = f"ddpm_step {rowname} Cx={Cx} Cc={Cc} next={with_next}"
    row, nz = DDPM_ROWS[rowname]
    row = torch.tensor(row, dtype=F32)
    g, x, e, cond, bx, xd, bn, nx, idx = _step_setup(dev, Cx, Cc, with_next, 43)
    z = torch.randn(x.shape, generator=g)
    noise, base = None, -1
    if nz == "buf":
        noise = z.to(dev)
    elif nz is not None:
        base = int(nz[-1])
        noise = _table(z, STEP_IDX - base, 5, dev)
    O.ddpm_step(xd, _nhwc_nan(e, 8, dev), _table(row, STEP_IDX, 5, dev), idx, noise,
                None if cond is None else cond.to(dev), nx, noise_base=base)
    want = ddpm_eager(x, e, row, z if nz is not None else None)
    if float(row[5]) > 0:                               # the row's clip is exercised on both sides
        x0 = (x - row[0] * e) / row[1]
        assert bool((x0 > row[5]).any()) and bool((x0 < -row[5]).any())
    _step_verify(name, want, cond, bx, xd, bn, nx)


# ----------------------------------------------------------------------------------------------- multistep solvers
NCOEF = 12
SS_N, SS_CX, SS_CC, SS_KPAD, SS_CPAD = 2, 2, 1, 8, 8


def sched_rows(kind, seed=47):
    """Six coefficient rows on the k/8 lattice.  "dpm": c[2] = 0 everywhere (last = None); "unipc": row 0 has no
    corrector, rows 1 .. 5 have c[2] = 1."""
    g = rng(seed)
    chain = torch.tensor([-1.0, -0.5, 0.5, 1.0])
    rows = lat((6, NCOEF), g, 4, 4)
    for k in (0, 3, 7, 8):
        rows[:, k] = chain[torch.randint(0, 4, (6,), generator=g)]
    rows[:, 2] = 0.0
    if kind == "dpm":
        rows[:, 3:8] = 0.0
    else:
        rows[1:, 2] = 1.0
        rows[0, 3:8] = 0.0
    for k in (1, 9, 10, 11):                            # no accidental zero where a term must show
        rows[:, k] = torch.where(rows[:, k] == 0, torch.full_like(rows[:, k], 0.75), rows[:, k])
    return rows


def sched_step_ref(x, eps, ring, last, c, i, dt=F64, order=None, mutant=None):
    """One step of the header's formula on [N, Cx, *S] tensors; ``ring`` (list of 4) and ``last`` are replaced
    functionally.  Returns (x_new, ring, last).  ``order`` permutes the terms of every sum (fp32 emulation)."""
    c = [float(v) for v in c]

    def comb(terms):
        terms = [terms[j] for j in order if j < len(terms)] if order is not None else terms
        acc = torch.zeros_like(x.to(dt))
        for cf, t in terms:
            acc = acc + torch.tensor(cf, dtype=dt) * t.to(dt)
        return acc
    r = lambda j: ring[(i - j) & 3]                      # noqa: E731
    m = comb([(c[0], x), (c[1], eps)])
    xc = x.to(dt)
    if c[2] != 0:
        xc = comb([(c[3], last), (c[4], r(1)), (c[5], r(2)), (c[6], r(3)), (c[7], m)])
    xn = comb([(c[8], xc), (c[9], m), (c[10], r(1)), (c[11], r(2))])
    ring = list(ring)
    ring[((i + 1) if mutant == "ring_plus_one" else i) & 3] = m
    if last is not None and mutant != "last_not_updated":
        last = xc
    return xn, ring, last


def _order_for(perm):
    return [int(j) for j in torch.randperm(5, generator=rng(53))] if perm else None


def check_sched_step(O, dev, kind):
    """Steps i = 0 .. 5 from a zeroed ring / last on the lattice (x reloaded every step): x, the four ring buffers,
    last and next after every step against the header's formula in fp64."""
    name = f"sched_step {kind}"
    g = rng(59)
    sh = (SS_N, SS_CX, *STEP_SP)
    rows = sched_rows(kind)
    coef = rows.to(dev)
    cond = lat((SS_N, SS_CC, *STEP_SP), g, 4096, 256)
    bx, x = guarded(sh, F32, dev, 0.0)
    rb = [guarded(sh, F32, dev, 0.0) for _ in range(4)]
    bl, last = guarded(sh, F32, dev, 0.0) if kind == "unipc" else (None, None)
    bn, nx = guarded((SS_N, *STEP_SP, SS_CPAD), BF16, dev, 3.0)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    ring64 = [torch.zeros(sh, dtype=F64) for _ in range(4)]
    last64 = torch.zeros(sh, dtype=F64) if kind == "unipc" else None
    for i in range(6):
        x0, eps = lat(sh, g, 8, 8), lat(sh, g, 8, 8)
        x.copy_(x0)
        idx.fill_(i)
        O.sched_step(x, _nhwc_nan(eps, SS_KPAD, dev), [v for _, v in rb], last, coef, idx, cond.to(dev), nx)
        xn, ring64, last64 = sched_step_ref(x0, eps, ring64, last64, rows[i], i)
        for bf in [bx, bn] + [b for b, _ in rb] + ([bl] if bl is not None else []):
            assert_guards(bf, f"{name} step {i}")
        assert_equal(x, xn, f"{name} step {i} x")
        for k in range(4):
            assert_equal(rb[k][1], ring64[k], f"{name} step {i} ring[{k}]")
        if last is not None:
            assert_equal(last, last64, f"{name} step {i} last")
        assert torch.equal(nx.cpu(), next_ref(xn, cond, SS_CPAD)), f"{name} step {i} next"


def check_sched_step_vs_lincomb(O, dev, kind):
    """A carried six-step run of random fp32 inputs: fmd_sched_step against the eager scheduler's route, the same
    coefficients through fmd_lincomb.  The header states they are equal."""
    name = f"sched_step == lincomb {kind}"
    g = rng(61)
    sh = (SS_N, SS_CX, *STEP_SP)
    rows = sched_rows(kind)
    coef = rows.to(dev)
    x0 = torch.randn(sh, generator=g)
    xa, xb = x0.to(dev).clone(), x0.to(dev).clone()
    ra = [torch.zeros(sh, device=dev) for _ in range(4)]
    rb = [torch.zeros(sh, device=dev) for _ in range(4)]
    la = torch.zeros(sh, device=dev) if kind == "unipc" else None
    lb = torch.zeros(sh, device=dev) if kind == "unipc" else None
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    new = lambda: torch.empty(sh, device=dev)           # noqa: E731
    for i in range(6):
        eps = torch.randn(sh, generator=g)
        idx.fill_(i)
        O.sched_step(xa, _nhwc_nan(eps, SS_KPAD, dev), ra, la, coef, idx, None, None)
        c = [float(v) for v in rows[i]]
        r = lambda j: rb[(i - j) & 3]                    # noqa: E731
        m = O.lincomb(new(), [xb, eps.to(dev)], c[0:2])
        xc = xb
        if c[2] != 0:
            xc = O.lincomb(new(), [lb, r(1), r(2), r(3), m], c[3:8])
        xb = O.lincomb(new(), [xc, m, r(1), r(2)], c[8:12])
        rb[i & 3] = m
        if lb is not None:
            lb = xc
        assert torch.equal(xa.cpu(), xb.cpu()), f"{name} step {i}: x"
        for k in range(4):
            assert torch.equal(ra[k].cpu(), rb[k].cpu()), f"{name} step {i}: ring[{k}]"
        if la is not None:
            assert torch.equal(la.cpu(), lb.cpu()), f"{name} step {i}: last"
    assert bool(torch.isfinite(xa).all())


LINCOMB_N = (1, 3, 4, 1027, 1028)


def lincomb_ref(inputs, coefs, dt=F64, order=None):
    ks = list(range(len(inputs))) if order is None else [k for k in order if k < len(inputs)]
    acc = torch.zeros_like(inputs[0].to(dt))
    for k in ks:
        acc = acc + torch.tensor(float(coefs[k]), dtype=dt) * inputs[k].to(dt)
    return acc


def check_lincomb(O, dev, nin, n, alias=False):
    name = f"lincomb nin={nin} n={n} alias={alias}"
    g = rng(67)
    ins = [lat((n,), g, 32, 8) for _ in range(nin)]
    cs = [float(v) for v in lat((nin,), g, 16, 8)]
    bufs = [guarded((n,), F32, dev, t) for t in ins]
    bo, out = bufs[0] if alias else guarded((n,), F32, dev)
    got = O.lincomb(out, [v for _, v in bufs], cs)
    assert got.data_ptr() == out.data_ptr()
    for bf, _ in bufs + [(bo, out)]:
        assert_guards(bf, name)
    assert_equal(out, lincomb_ref(ins, cs), name)
    for k in range(0 if not alias else 1, nin):
        assert torch.equal(bufs[k][1].cpu(), ins[k]), f"{name}: input {k} modified"


def check_gather_row(O, dev, n, rows=5, row=3):
    name = f"gather_row n={n}"
    want = torch.randn(n, generator=rng(71))
    bo, out = guarded((n,), F32, dev)
    O.gather_row(_table(want, row, rows, dev), torch.tensor([row], dtype=torch.int32, device=dev), out)
    assert_guards(bo, name)
    assert torch.equal(out.cpu(), want), name


def check_fill_from_table(O, dev, N, rows=5, row=3):
    name = f"fill_from_table N={N}"
    want = torch.randn((), generator=rng(73))
    bo, out = guarded((N,), F32, dev)
    O.fill_from_table(_table(want, row, rows, dev), torch.tensor([row], dtype=torch.int32, device=dev), out)
    assert_guards(bo, name)
    assert torch.equal(out.cpu(), want.expand(N)), name


# =============================================================================================== layout / resampling
LAYOUT_SP = ((35,), (5, 7), (1, 5, 7))       # HW = 35 as a 1-D, 2-D and 3-D extent


def check_nchw_to_nhwc(O, dev, C, Cpad, sp):
    x = torch.randn((2, C, *sp), generator=rng(79))              # not bf16-exact: the move rounds once
    got = O.nchw_to_nhwc(x.to(dev), Cpad)
    want = _to_nhwc_pad(x, Cpad or C).to(BF16)
    assert got.dtype == BF16 and torch.equal(got.cpu(), want), f"nchw_to_nhwc C={C} Cpad={Cpad} sp={sp}"


def check_nhwc_to_nchw(O, dev, C, Cs, sp, src_f32):
    y = torch.randn((2, *sp, Cs), generator=rng(83))
    y = y if src_f32 else y.to(BF16)
    y[..., C:] = float("nan")
    got = O.nhwc_to_nchw(y.to(dev), C)
    want = y[..., :C].movedim(-1, 1).float().contiguous()
    assert got.dtype == F32 and torch.equal(got.cpu(), want), f"nhwc_to_nchw C={C} Cs={Cs} sp={sp} f32={src_f32}"


def check_affine_channels(O, dev, C, scale, shift, Cpad=8):
    name = f"affine_channels C={C} {scale} x + {shift}"
    g = rng(89)
    x = lat((2, 5, 7, Cpad), g, 31, 4, BF16)
    bits = x.view(torch.int16).clone()
    pad = torch.randint(-32768, 32767, (2, 5, 7, Cpad - C), generator=g).to(torch.int16)
    if C < Cpad:
        pad[0, 0, 0, 0], pad[0, 0, 1, 0] = 0x7FC1, -0x005B        # NaN payloads 0x7fc1, 0xffa5
        bits[..., C:] = pad
    x = bits.view(BF16)
    got = O.affine_channels(x.to(dev), C, scale, shift).cpu()
    assert_equal(got[..., :C], scale * x[..., :C].double() + shift, name, bf16=True)
    assert torch.equal(got.view(torch.int16)[..., C:], bits[..., C:]), f"{name}: pad channels not copied bit for bit"


def _blocks(factors, order=None):
    import itertools
    offs = list(itertools.product(*[range(f) for f in factors]))
    return offs if order is None else [offs[j] for j in order if j < len(offs)]


def resample_down_ref(src, low, factors, scale, old=None, dt=F64, order=None, mutant=None):
    """dst[low] = scale * sum of src's block (+ old); src [N, *high, C].  A high extent of 2 low + 1 drops its last
    index."""
    v = src.to(dt)
    if mutant == "odd_row_included":                    # the last block swallows the odd index too
        v = v.clone()
        for dim, (f, l) in enumerate(zip(factors, low)):
            if f == 2 and v.shape[1 + dim] == 2 * l + 1:
                v.narrow(1 + dim, 2 * l - 1, 1).add_(v.narrow(1 + dim, 2 * l, 1))
    acc = torch.zeros((v.shape[0], *low, v.shape[-1]), dtype=dt)
    for off in _blocks(factors, order):
        sl = tuple(slice(o, o + f * l, f) for o, f, l in zip(off, factors, low))
        acc = acc + v[(slice(None), *sl, slice(None))]
    out = acc * torch.tensor(scale, dtype=dt)
    return out if old is None else out + old.to(dt)


def resample_up_ref(src, high, factors, scale, old=None, dt=F64):
    """dst[high] = scale * src[high >> 1 along the factor-2 dims] (+ old), 0 past the low extent; src [N, *low, C]."""
    v = src.to(dt) * torch.tensor(scale, dtype=dt)
    low = v.shape[1:-1]
    out = torch.zeros((v.shape[0], *high, v.shape[-1]), dtype=dt)
    for off in _blocks(factors):
        sl = tuple(slice(o, o + f * l, f) for o, f, l in zip(off, factors, low))
        out[(slice(None), *sl, slice(None))] = v
    return out if old is None else out + old.to(dt)


# name: (factors, low extents); "1d" is a 1-D signal as an (L, 1) image
RESAMPLE_SETS = {"1d": ((2, 1), (3, 1)), "2d": ((2, 2), (2, 3)), "3d_hw": ((1, 2, 2), (2, 2, 3)),
                 "3d": ((2, 2, 2), (1, 2, 3))}
RESAMPLE_SCALES = (1.0, 0.125, 0.25)


def check_resample2(O, dev, kind, odd, up, acc, scale, C=5):
    """odd: None (high = 2 low) or the index of the factor-2 dim whose high extent is 2 low + 1."""
    factors, low = RESAMPLE_SETS[kind]
    assert odd is None or factors[odd] == 2
    high = tuple(f * l + (1 if j == odd else 0) for j, (f, l) in enumerate(zip(factors, low)))
    name = f"resample2 {kind} odd={odd} up={up} acc={acc} scale={scale} C={C}"
    g = rng(97)
    N = 2
    src = lat((N, *(low if up else high), C), g, 31, 4, BF16)
    old = lat((N, *(high if up else low), C), g, 100, 4, BF16)
    bd, dst = guarded(tuple(old.shape), BF16, dev, old if acc else 3.0)
    O.resample2(src.to(dev), dst, bool(up), scale, acc=bool(acc), factors=factors)
    assert_guards(bd, name)
    ref = (resample_up_ref(src, high, factors, scale, old if acc else None) if up
           else resample_down_ref(src, low, factors, scale, old if acc else None))
    assert_equal(dst, ref, name, bf16=True)


POOL_HW = ((1, 1), (3, 5))
POOL_DHW = ((1, 1, 1), (3, 5, 2))
POOL_C = (1, 5, 8)


def check_sum_pool(O, dev, low, C, acc):
    """sum_pool2 (2-D extents) / sum_pool2_3d (3-D extents)."""
    name = f"sum_pool2{'_3d' if len(low) == 3 else ''} low={low} C={C} acc={acc}"
    g = rng(101)
    src = lat((2, *[2 * v for v in low], C), g, 31, 4, BF16)
    old = lat((2, *low, C), g, 100, 4, BF16)
    bd, dst = guarded(tuple(old.shape), BF16, dev, old if acc else 3.0)
    (O.sum_pool2 if len(low) == 2 else O.sum_pool2_3d)(src.to(dev), dst, bool(acc))
    assert_guards(bd, name)
    assert_equal(dst, resample_down_ref(src, low, (2,) * len(low), 1.0, old if acc else None), name, bf16=True)


def check_add(O, dev, C, sp=(3, 5)):
    name = f"add_ C={C}"
    g = rng(103)
    a = lat((2, *sp, C), g, 31, 4, BF16)
    old = lat((2, *sp, C), g, 100, 4, BF16)
    bd, dst = guarded(tuple(old.shape), BF16, dev, old)
    O.add_(dst, a.to(dev))
    assert_guards(bd, name)
    assert_equal(dst, old.double() + a.double(), name, bf16=True)


def check_host_rejections(O, dev):
    """Arguments the host functions return an error for BEFORE any launch (read from their code): lincomb with 0
    or 7 inputs (the wrapper), fill_from_table with N = 257, resample2 with a factor of 3, a high extent of
    f low + 2, and unequal extents on a factor-1 dim."""
    import pytest
    t = torch.zeros(8, device=dev)
    for k in (0, 7):
        with pytest.raises(ValueError):
            O.lincomb(t, [t] * k, [1.0] * k)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(RuntimeError):
        O.fill_from_table(torch.zeros(4, device=dev), idx, torch.zeros(257, device=dev))
    z = lambda *s: torch.zeros(s, dtype=BF16, device=dev)     # noqa: E731
    for src, dst, fac in ((z(1, 9, 9, 4), z(1, 3, 3, 4), (3, 3)),          # a factor of 3
                          (z(1, 8, 6, 4), z(1, 3, 3, 4), (2, 2)),          # Hh = 2 Hl + 2
                          (z(1, 4, 6, 6, 4), z(1, 2, 3, 3, 4), (1, 2, 2)),  # Dh = fz Dl + 2 on a factor-1 dim
                          (z(1, 3, 6, 6, 4), z(1, 2, 3, 3, 4), (1, 2, 2))):  # Dh = Dl + 1 on a factor-1 dim
        for up in (False, True):
            with pytest.raises(RuntimeError):
                O.resample2(dst if up else src, src if up else dst, up, 1.0, factors=fac)


# =============================================================================================== fp32 emulation
def _silu32(z):
    return z * torch.sigmoid(z)


def _silu_grad32(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def _t(a):
    return torch.tensor(float(a), dtype=F32)


class _EmuGroupedLinear:
    def __init__(self, emu, linears, in_silu):
        self.emu, self.linears, self.in_silu = emu, list(linears), bool(in_silu)
        self.O = [int(l.weight.shape[0]) for l in self.linears]
        self.off = [sum(self.O[:k]) for k in range(len(self.O))]
        self.total = sum(self.O)

    def forward(self, x):
        y = torch.empty((x.shape[0], self.total), dtype=F32)
        for l, o, n in zip(self.linears, self.off, self.O):
            self.emu.linear(x, l.weight.data, None if l.bias is None else l.bias.data, self.in_silu,
                            out=y[:, o:o + n], out_stride=self.total)
        return y

    def backward(self, x, dy, dx=None, dx_acc=False):
        e = self.emu
        sv = torch.zeros_like(x)
        for l, o, n in zip(self.linears, self.off, self.O):
            e.linear_bwd(x, l.weight.data, dy[:, o:o + n], l.weight.grad, None if l.bias is None else l.bias.grad,
                         in_silu=self.in_silu, dy_stride=self.total)
            for r in e._order(n):
                sv = sv + dy[:, o + r:o + r + 1] * l.weight.data[r][None]
        if dx is not None:
            if self.in_silu:
                sv = sv * _silu_grad32(x)
            dx.copy_(dx + sv if dx_acc else sv)


class Emu:
    """The documented operations behind the ``ops`` wrappers in fp32 on the CPU, with the wrappers' signatures.
    ``perm``: every reduction walks its terms in a permuted order.  ``mutant``: one known bug (see MUTANTS)."""

    def __init__(self, mutant=None, perm=False):
        self.mutant, self.perm = mutant, perm

    def _order(self, n):
        return [int(j) for j in torch.randperm(n, generator=rng(107))] if self.perm else list(range(n))

    # ---- time path
    def timestep_embedding(self, t, dim, flip, shift=0, max_period=10000.0, t_scale=1.0, t_trunc=False):
        return temb_ref(t.float(), dim, flip, shift, max_period, t_scale, t_trunc, dt=F32, mutant=self.mutant)[0]

    def linear(self, x, w, b, in_silu=False, out=None, out_stride=None):
        B, I = x.shape
        Oo = w.shape[0]
        xin = _silu32(x) if in_silu else x
        acc = torch.zeros((B, Oo), dtype=F32)
        for i in self._order(I):
            acc = acc + xin[:, i:i + 1] * w[:, i][None]
        if b is not None:
            acc = acc + b
            if self.mutant == "bias_twice":
                acc = acc + b
        if out is None:
            out = torch.empty((B, Oo), dtype=F32)
        ld = out_stride or Oo
        _flat(out, (B, Oo), (ld, 1)).copy_(acc)
        if self.mutant == "pad_rows_stored":            # rows b >= B stored with row B - 1's value
            room = out.untyped_storage().nbytes() // 4 - (out.storage_offset() + B * ld)
            k = max(0, min(Oo, room))
            torch.as_strided(out, (k,), (1,), out.storage_offset() + B * ld).copy_(acc[B - 1, :k])
        return out

    def linear_bwd(self, x, w, dy, dw, db, dx=None, dx_acc=False, in_silu=False, dy_stride=None):
        B, I = x.shape
        Oo = w.shape[0]
        ld = Oo if self.mutant == "dy_stride_ignored" else (dy_stride or dy.shape[-1])
        d = _flat(dy, (B, Oo), (ld, 1))
        if dw is not None:
            xin = _silu32(x) if in_silu else x
            s, t = torch.zeros_like(dw), torch.zeros((Oo,), dtype=F32)
            for b in self._order(B):
                s = s + d[b][:, None] * xin[b][None]
                t = t + d[b]
            dw.copy_(dw + s)
            if db is not None:
                db.copy_(t if self.mutant == "db_not_accumulated" else db + t)
        if dx is not None:
            sv = torch.zeros_like(x)
            for o in self._order(Oo):
                sv = sv + d[:, o:o + 1] * w[o][None]
            if in_silu:
                sv = sv * _silu_grad32(x)
            dx.copy_(dx + sv if dx_acc else sv)

    def GroupedLinear(self, linears, in_silu):
        return _EmuGroupedLinear(self, linears, in_silu)

    def silu_bwd(self, x, dy):
        return dy * _silu_grad32(x)

    # ---- train step
    def noise_prepare(self, x0, noise, ca, cb, cond, Cpad, out=None):
        v = noise_prepare_ref(x0, noise, ca, cb, cond, Cpad, dt=F32)
        Cx, Cc = noise.shape[1], (cond.shape[1] if cond is not None else 0)
        if self.mutant == "cond_offset" and Cc:
            v[..., Cx:Cx + Cc] = v[..., Cx:Cx + Cc].roll(1, -1)
        if self.mutant == "pad_not_zeroed":
            v[..., Cx + Cc:] = out[..., Cx + Cc:].float() if out is not None else 1.0
        if out is None:
            return v.to(BF16)
        out.copy_(v.to(BF16))
        return out

    def mse(self, pred, ta, tb, tb_sign, grad_scale, loss, partial, dpred=None):
        Cx = ta.shape[1]
        _, g, dlt, inv = mse_ref(pred, ta, tb, float(tb_sign), float(grad_scale), dt=F32, mutant=self.mutant)
        blocks = min(partial.numel(), (pred.numel() + 255) // 256)
        sq = torch.zeros(pred.shape, dtype=F32)
        sq[..., :Cx] = dlt * dlt
        blk = (torch.arange(pred.numel()) // 256) % blocks
        o = torch.tensor(self._order(pred.numel()))
        part = torch.zeros(blocks, dtype=F32).index_add_(0, blk[o], sq.flatten()[o])
        partial[:blocks] = part
        loss[0] = (part.double().sum() * inv.double()).float()
        if dpred is not None:
            dpred.copy_(g.to(BF16))

    def _adam(self, p, g, m, v, lr, b1, b2, eps, wd, bc1, bc2s, gs):
        gv = g * _t(gs)
        gq = g if self.mutant == "v_unscaled_g" else gv
        p.copy_(p * (1 - _t(lr) * _t(wd)))
        m.copy_(m + (gv - m) * (1 - _t(b1)))
        v.copy_(v * _t(b2) + (1 - _t(b2)) * gq * gq)
        den = v.sqrt() / bc2s + _t(eps)
        p.copy_(p - (_t(lr) / _t(bc1)) * (m / den))

    def _bc2s(self, bc2):
        return _t(bc2) if self.mutant == "bc2_no_sqrt" else _t(bc2).sqrt()

    def adamw(self, p, g, m, v, lr, beta1, beta2, eps, wd, step):
        self._adam(p, g, m, v, lr, beta1, beta2, eps, wd, 1.0 - beta1 ** step, self._bc2s(1.0 - beta2 ** step), 1.0)

    def adamw_sched(self, p, g, m, v, step_ctr, base_lr, warmup, total, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0,
                    grad_scale=1.0):
        step = int(step_ctr[0]) + 1
        s = step - 1 + (1 if self.mutant == "lambda_off_by_one" else 0)
        lr = f32(base_lr) * cosine_lambda(s, warmup, total)
        b1, b2 = f32(beta1), f32(beta2)
        self._adam(p, g, m, v, lr, b1, b2, eps, wd, 1.0 - b1 ** step, self._bc2s(1.0 - b2 ** step), grad_scale)

    def counter_add(self, ctr, v=1):
        ctr[0] += int(v)

    # ---- sampler steps
    @staticmethod
    def _nchw(t_nhwc, Cx):
        return t_nhwc[..., :Cx].movedim(-1, 1)

    def flow_euler(self, x, v_nhwc, sigmas, index, cond, next_inp):
        idx = 0 if self.mutant == "index_zero" else int(index[0])
        x.copy_(flow_euler_eager(x, self._nchw(v_nhwc, x.shape[1]), sigmas, idx))
        if next_inp is not None:
            next_inp.copy_(next_ref(x, cond, next_inp.shape[-1]))

    def ddpm_step(self, x, eps_nhwc, coef, index, noise, cond, next_inp, noise_base=-1):
        idx = int(index[0])
        z = noise
        if noise is not None and noise_base >= 0:
            z = noise[idx if self.mutant == "noise_base_ignored" else idx - noise_base]
        x.copy_(ddpm_eager(x, self._nchw(eps_nhwc, x.shape[1]), coef[idx], z))
        if next_inp is not None:
            next_inp.copy_(next_ref(x, cond, next_inp.shape[-1]))

    def sched_step(self, x, eps_nhwc, ring, last, coef, index, cond, next_inp):
        i = int(index[0])
        xn, rg, ls = sched_step_ref(x, self._nchw(eps_nhwc, x.shape[1]), [r.clone() for r in ring],
                                    None if last is None else last.clone(), coef[i], i, dt=F32,
                                    order=_order_for(self.perm), mutant=self.mutant)
        for dst, src in zip(ring, rg):
            dst.copy_(src)
        if last is not None:
            last.copy_(ls)
        x.copy_(xn)
        if next_inp is not None:
            next_inp.copy_(next_ref(xn, cond, next_inp.shape[-1]))

    def lincomb(self, out, inputs, coefs):
        if not 1 <= len(inputs) <= 6 or len(inputs) != len(coefs):
            raise ValueError("lincomb: 1..6 inputs, one coefficient each")
        out.copy_(lincomb_ref(inputs, coefs, dt=F32, order=self._order(len(inputs)) if self.perm else None))
        return out

    def gather_row(self, table, index, out):
        n, r = out.numel(), (0 if self.mutant == "row_zero" else int(index[0]))
        out.copy_(table.reshape(-1)[r * n:(r + 1) * n].view_as(out))

    def fill_from_table(self, table, index, out):
        if out.numel() > 256:
            raise RuntimeError("fmd_fill_from_table failed with code -1")
        out.fill_(float(table[0 if self.mutant == "row_zero" else int(index[0])]))

    # ---- layout / resampling
    def nchw_to_nhwc(self, x, Cpad=None):
        return _to_nhwc_pad(x.float(), Cpad or x.shape[1]).to(BF16)

    def nhwc_to_nchw(self, y, Cc):
        return y[..., :Cc].movedim(-1, 1).float().contiguous()

    def affine_channels(self, x, C, scale, shift):
        y = x.clone()
        y[..., :C] = (_t(scale) * x[..., :C].float() + _t(shift)).to(BF16)
        return y

    def resample2(self, src, dst, up, scale, acc=False, factors=None):
        nd = src.dim() - 2
        f = tuple(factors) if factors is not None else (2,) * nd
        lo, hi = (src.shape[1:-1], dst.shape[1:-1]) if up else (dst.shape[1:-1], src.shape[1:-1])
        for fk, l, h in zip(f, lo, hi):
            if fk not in (1, 2) or h < fk * l or h > fk * l + (1 if fk == 2 else 0):
                raise RuntimeError("fmd_resample2 failed with code -1")
        old = dst.clone() if acc else None
        if up:
            v = resample_up_ref(src, tuple(hi), f, scale, old, dt=F32)
        else:
            v = resample_down_ref(src, tuple(lo), f, scale, old, dt=F32,
                                  order=self._order(2 ** nd) if self.perm else None, mutant=self.mutant)
        dst.copy_(v.to(BF16))

    def sum_pool2(self, src, dst, acc):
        self.resample2(src, dst, False, 1.0, acc=acc)

    def sum_pool2_3d(self, src, dst, acc=False):
        self.resample2(src, dst, False, 1.0, acc=acc)

    def add_(self, dst, a):
        dst.copy_((dst.float() + a.float()).to(BF16))


# mutant -> the worry of the issue it stands for
MUTANTS = {
    "half_no_shift": "timestep_embedding divides by half instead of half - shift",
    "flip_inverted": "timestep_embedding: flip_sin_to_cos inverted",
    "trunc_rounds": "t_trunc rounds to nearest instead of truncating",
    "pad_rows_stored": "linear stores row B - 1 for a batch row b >= B",
    "bias_twice": "linear adds the bias twice",
    "dy_stride_ignored": "linear_bwd reads dy with stride O",
    "db_not_accumulated": "linear_bwd overwrites db",
    "cond_offset": "noise_prepare: cond channels off by one",
    "pad_not_zeroed": "noise_prepare leaves the pad channels",
    "tb_sign_dropped": "mse ignores tb_sign",
    "inv_numel_kpad": "mse divides by N Kpad HW",
    "v_unscaled_g": "adamw_sched updates v with the unscaled gradient",
    "bc2_no_sqrt": "adamw divides by bc2 instead of sqrt(bc2)",
    "lambda_off_by_one": "adamw_sched's lambda one scheduler step ahead",
    "index_zero": "flow_euler reads sigma row 0",
    "noise_base_ignored": "ddpm_step indexes the noise table by the step",
    "ring_plus_one": "sched_step writes ring slot (i + 1) & 3",
    "last_not_updated": "sched_step never stores last",
    "row_zero": "gather_row / fill_from_table read row 0",
    "odd_row_included": "resample2 pools the odd last index of a 2 low + 1 extent",
}


# =============================================================================================== the cases
# family -> {case id: fn(O, dev)}; the GPU modules and test_misc_ref.py run the same ones.
CASES: dict = {}


def _add(family, cid, fn, *a, **kw):
    CASES.setdefault(family, {})[cid] = lambda O, dev: fn(O, dev, *a, **kw)


def _build_cases():
    for dim in TEMB_DIMS:
        for flip in (0, 1):
            for shift in (0, 1):
                _add("timestep_embedding", f"dim{dim}-flip{flip}-shift{shift}", check_temb, dim, flip, shift)
    for dim in (33, 128):
        for half_step in (False, True):
            _add("timestep_embedding", f"dim{dim}-trunc-{'sixteenth' if half_step else 'eighth'}", check_temb, dim, 1,
                 0, trunc=half_step)
    for B, I, Oo in LINEAR_CASES:
        for bias in (True, False):
            for strided in (False, True):
                _add("linear", f"B{B}-I{I}-O{Oo}-bias{int(bias)}-strided{int(strided)}", check_linear, B, I, Oo,
                     bias=bias, strided=strided)
        _add("linear", f"B{B}-I{I}-O{Oo}-silu", check_linear, B, I, Oo, bias=True, strided=True, in_silu=True)
    def linear_bwd_exact(O, dev, B, I, Oo):
        for acc in (False, True):
            for strided in (False, True):
                check_linear_bwd(O, dev, B, I, Oo, dx_acc=acc, strided=strided)
    for B, I, Oo in LINEAR_BWD_CASES:
        _add("linear_bwd", f"B{B}-I{I}-O{Oo}-exact", linear_bwd_exact, B, I, Oo)
        _add("linear_bwd", f"B{B}-I{I}-O{Oo}-silu", check_linear_bwd, B, I, Oo, dx_acc=True, strided=True,
             in_silu=True)
    for B, I, Oo in ((8, 200, 300), (9, 512, 512)):
        _add("linear_bwd", f"B{B}-I{I}-O{Oo}-nodx", check_linear_bwd, B, I, Oo, strided=True, want_dx=False)
        _add("linear_bwd", f"B{B}-I{I}-O{Oo}-nodw", check_linear_bwd, B, I, Oo, strided=True, want_dw=False)
    for B, I in GL_CASES:
        for acc in (False, True):
            _add("grouped_linear", f"B{B}-I{I}-acc{int(acc)}", check_grouped_linear, B, I, dx_acc=acc)
        _add("grouped_linear", f"B{B}-I{I}-silu", check_grouped_linear, B, I, dx_acc=True, in_silu=True)
    for n in SILU_BWD_N:
        _add("silu_bwd", f"n{n}", check_silu_bwd, n)

    for mode in ("ddpm", "fm", "copy"):
        for Cc in (0, 3):
            for Cx in (1, 2):
                for Cpad in (8, 16):
                    _add("noise_prepare", f"{mode}-Cx{Cx}-Cc{Cc}-Cpad{Cpad}", check_noise_prepare, mode, Cx, Cc, Cpad)
        _add("noise_prepare", f"{mode}-Cx2-Cc3-Cpad8-out", check_noise_prepare, mode, 2, 3, 8, reuse_out=True)
    for kind, cxs in (("pow2", (1,)), ("odd", (1, 3))):
        for Cx in cxs:
            for Kpad in (8, 16):
                for tb in (None, 1.0, -1.0):
                    for gs in (1.0, 0.25):
                        _add("mse", f"{kind}-Cx{Cx}-Kpad{Kpad}-tb{tb}-gs{gs}", check_mse, kind, Cx, Kpad, tb, gs)
                for npart in (1, 4):
                    _add("mse", f"{kind}-Cx{Cx}-Kpad{Kpad}-partial{npart}", check_mse, kind, Cx, Kpad, -1.0, 0.25,
                         npartial=npart)
            _add("mse", f"{kind}-Cx{Cx}-Kpad8-nodpred", check_mse, kind, Cx, 8, -1.0, 1.0, with_dpred=False)

    def adam_all_offsets(O, dev, n, wd, sched, gs=1.0):
        return max(check_adamw(O, dev, n, off, wd, sched, gs) for off in range(4))
    for n in ADAMW_N:
        for wd in (0.0, 0.01):
            _add("adamw", f"n{n}-wd{wd}", adam_all_offsets, n, wd, False)
            for gs in (1.0, 0.5):
                _add("adamw_sched", f"n{n}-wd{wd}-gs{gs}", adam_all_offsets, n, wd, True, gs)
    for Cx in (1, 2):
        for Cc in (0, 3):
            _add("flow_euler", f"Cx{Cx}-Cc{Cc}", check_flow_euler, Cx, Cc)
        _add("flow_euler", f"Cx{Cx}-nonext", check_flow_euler, Cx, 3, with_next=False)
        for row in DDPM_ROWS:
            _add("ddpm_step", f"{row}-Cx{Cx}", check_ddpm_step, row, Cx)
    _add("ddpm_step", "ddpm_clip-Cx2-Cc0", check_ddpm_step, "ddpm_clip", 2, Cc=0)
    _add("ddpm_step", "table_base2-Cx2-nonext", check_ddpm_step, "table_base2", 2, with_next=False)
    for kind in ("dpm", "unipc"):
        _add("sched_step", f"{kind}-lattice", check_sched_step, kind)
        _add("sched_step", f"{kind}-lincomb", check_sched_step_vs_lincomb, kind)
    for nin in (1, 6):
        for n in LINCOMB_N:
            for alias in (False, True):
                _add("lincomb", f"nin{nin}-n{n}-alias{int(alias)}", check_lincomb, nin, n, alias)
    for n in (1, 1027):
        _add("gather_row", f"n{n}", check_gather_row, n)
    for N in (1, 256):
        _add("fill_from_table", f"N{N}", check_fill_from_table, N)
    _add("host_rejections", "all", check_host_rejections)

    for C in (1, 3, 8):
        for Cpad in (None, 8, 16):
            for sp in LAYOUT_SP:
                _add("nchw_to_nhwc", f"C{C}-Cpad{Cpad}-{len(sp)}d", check_nchw_to_nhwc, C, Cpad, sp)
        for f32src in (False, True):
            for sp in LAYOUT_SP:
                _add("nhwc_to_nchw", f"C{C}-f32{int(f32src)}-{len(sp)}d", check_nhwc_to_nchw, C, 16 if C == 8 else 8,
                     sp, f32src)
    for C in (0, 1, 3, 8):
        for sc, sh in ((2.0, -1.0), (-0.5, 0.25)):
            _add("affine_channels", f"C{C}-{sc}x{sh:+}", check_affine_channels, C, sc, sh)
    for C in POOL_C:
        _add("add_", f"C{C}", check_add, C)
        for acc in (False, True):
            for low in POOL_HW + POOL_DHW:
                _add("sum_pool", f"{'x'.join(map(str, low))}-C{C}-acc{int(acc)}", check_sum_pool, low, C, acc)

    def resample_all(O, dev, kind, odd, up):
        for acc in (False, True):
            for scale in RESAMPLE_SCALES:
                check_resample2(O, dev, kind, odd, up, acc, scale)
    for kind, (factors, _) in RESAMPLE_SETS.items():
        for odd in [None] + [j for j, f in enumerate(factors) if f == 2]:
            for up in (False, True):
                _add("resample2", f"{kind}-odd{odd}-up{int(up)}", resample_all, kind, odd, up)


_build_cases()

TIMEPATH = ("timestep_embedding", "linear", "linear_bwd", "grouped_linear", "silu_bwd")
STEPS = ("noise_prepare", "mse", "adamw", "adamw_sched", "flow_euler", "ddpm_step", "sched_step", "lincomb",
         "gather_row", "fill_from_table", "host_rejections")
RESAMPLE = ("nchw_to_nhwc", "nhwc_to_nchw", "affine_channels", "add_", "sum_pool", "resample2")


def case_ids(families):
    return [(f, c) for f in families for c in CASES[f]]


# mutant -> (family, the cases of that family in which it must be rejected)
MUTANT_CASES = {
    "half_no_shift": ("timestep_embedding", lambda c: "shift1" in c and "dim2-" not in c),
    "flip_inverted": ("timestep_embedding", lambda c: True),
    "trunc_rounds": ("timestep_embedding", lambda c: "trunc" in c),
    "pad_rows_stored": ("linear", lambda c: True),
    "bias_twice": ("linear", lambda c: "bias0" not in c),
    "dy_stride_ignored": ("linear_bwd", lambda c: not c.startswith("B1-")),          # one row has no stride
    "db_not_accumulated": ("linear_bwd", lambda c: "nodw" not in c),
    "cond_offset": ("noise_prepare", lambda c: "Cc3" in c),
    "pad_not_zeroed": ("noise_prepare", lambda c: True),
    "tb_sign_dropped": ("mse", lambda c: "tb-1.0" in c or "partial" in c or "nodpred" in c),
    "inv_numel_kpad": ("mse", lambda c: True),
    "v_unscaled_g": ("adamw_sched", lambda c: "gs0.5" in c),
    "bc2_no_sqrt": ("adamw", lambda c: True),
    "lambda_off_by_one": ("adamw_sched", lambda c: True),
    "index_zero": ("flow_euler", lambda c: True),
    "noise_base_ignored": ("ddpm_step", lambda c: "table_base2" in c),
    "ring_plus_one": ("sched_step", lambda c: "lattice" in c),
    "last_not_updated": ("sched_step", lambda c: c == "unipc-lattice"),
    "row_zero": ("gather_row", lambda c: True),
    "odd_row_included": ("resample2", lambda c: "oddNone" not in c and "up0" in c),
}
