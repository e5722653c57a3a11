"""fp64 reference, first-order error bounds and a CPU emulation of the folded GroupNorm (csrc/groupnorm.hip),
shared by test_gn_bounds.py (CPU) and test_gpu_groupnorm.py (GPU).

Everything works on flattened NHWC tensors: x, dz, extra [N][HW][C] with C = C0 + C1 the channel concat of the
two sources, per-(n, c) planes [N][C], per-(n, group) planes [N][G].

The operation.  mode 0: z = GN(x); mode 1: z = GN(x) (1 + scale) + shift with emb[n] = (scale | shift);
mode 2: z = GN(x) where x already carries an additive embedding e[n][c], whose gradient is sum_hw dx.
Forward outputs: mean, rstd per (n, g); a, b with z = a x + b; t = SiLU(z).  Backward, from dz = dL/dz:
dx = P dz + Q x + R (+ extra, + the old destination where acc), dgamma, dbeta (+= into existing gradients), demb.
With s = 1 + scale (1 in modes 0, 2), gp = gamma s, r = rstd, m = mean, cnt = Cg HW and per (n, c)
S1 = sum_hw dz, S2 = sum_hw dz x, Sx = sum_hw x, D = S2 - m S1:
  A1 = sum_group gp S1 / cnt          A2 = sum_group gp r D / cnt
  P = r gp     Q = -r^2 A2     R = r^2 A2 m - r A1        (so Q x + R = Q (x - m) - r A1)
  dgamma = sum_n s r D     dbeta = sum_n s S1
  demb (mode 1) = (gamma r D + beta S1 | S1)       demb (mode 2) = P S1 + Q Sx + R HW
reference() does not use these: it differentiates F.group_norm in double.  closed_form() does, for the bounds
and the mutants, and test_gn_bounds.py asserts the two equal at 1e-9.

The kernel arithmetic the bounds are derived from (see the kernel source):
  * fmd_channel_stats: a slab row is `rows` pixels of one image; 32 pixel lanes each add their pixels (stride 32)
    in fp32, then the lanes are added in order in fp32: a chain of k = ceil(rows / 32) + min(rows, 32) fp32
    additions (+ 1 rounding of the product x x or dz x).  fmd_stats_fold adds `fold` rows in fp32: k += fold.
  * fmd_gn_prep: a group inside one source with an even Cg -- per thread an fp32 chain over its
    ceil(E / 256) slab rows x Cg channels (k += Cg + ceil(E / 256) + 2), fp64 across threads; otherwise (odd Cg,
    or a group that straddles C0) fp64 throughout.  mean = G1 / cnt, var = G2 / cnt - mean^2, rstd =
    1 / sqrt(var + eps) in fp64; mean and rstd are SAVED IN fp32, and a, b are computed from those in fp32.
  * fmd_gn_fused_apply: per thread an fp32 chain of at most 16 four-channel units (k = 18), fp64 across threads.
  * fmd_gn_bwd_prep: fp64 over the slab rows and channels, with the saved fp32 mean / rstd; P, Q, R, the per-n
    gamma / beta terms and demb are rounded to fp32 once.  dgamma / dbeta: fp32 sum over n, fp32 += .
  * fmd_gn_apply_fwd / fmd_gn_bwd_apply: fp32 a x + b, SiLU with the hardware exp and reciprocal;
    fp32 P dz + Q x + R (+ extra) (+ old); one pack2 rounding to bf16 (round to nearest).
With u = 2^-24 (fp32) and U = 2^-8 (bf16) unit roundoffs, |.| elementwise, worst case and first order:
  e_F1 = k u sum|x|        e_F2 = (k + 1) u sum x^2        (per channel; summed over the group: e_G1, e_G2)
  e_S1 = k u sum|dz|       e_S2 = (k + 1) u sum|dz x|
  e_m  = e_G1 / cnt + u |m|
  e_r  = r^3 / 2 (e_G2 / cnt + 2 |m| e_G1 / cnt) + u r        amplifies by (3 m^2 + var) / var
  e_a  = |a| (e_r / r + 3 u)
  e_b  = |gp| (|m| e_r + r e_m) + 4 u (|beta s| + |m a| + |shift|)
  e_z  = |a| (e_r / r) |x - m| + |a| e_m + u (5 |a x| + |b| + 4 (|beta s| + |m a| + |shift|))
  e_t  = U |t| + |silu'(z)| e_z + 8 u (1 + |z|) |t|
  e_D  = e_S2 + |m| e_S1 + e_m |S1|
  e_A1 = sum_group |gp| e_S1 / cnt        e_A2 = sum_group |gp| (r e_D + e_r |D|) / cnt
  e_P  = |gp| e_r + u |P|
  e_Q  = 2 r e_r |A2| + r^2 e_A2 + u |Q|
  e_rA = e_r |A1| + r e_A1
  e_R  = e_Q |m| + |Q| e_m + e_rA + u |R|
  e_dx = U |dx| + 6 u (|P dz| + |Q x| + |R| + |extra| + |old|) + e_P |dz| + e_Q |x - m| + |Q| e_m + e_rA
  e_dgamma = sum_n (|s| (r e_D + e_r |D|) + u |s r D|) + (N + 1) u (sum_n |s r D| + |old|)
  e_dbeta  = sum_n (|s| e_S1 + u |s S1|) + (N + 1) u (sum_n |s S1| + |old|)
  e_demb1  = (|gamma| (r e_D + e_r |D|) + |beta| e_S1 + u |.|  |  e_S1 + u |S1|)
  e_demb2  = e_P |S1| + |P| e_S1 + e_Q |Sx - m HW| + |Q| (e_Sx + HW e_m) + HW e_rA + u |.|
The dx bound follows the kernel's own cancellation: R is built from the same fp32 mean and the same Q that
multiply x, so their errors enter through x - m, not through x; what is left at |Q x| + |R| is fp32 rounding
alone.  Second-order terms (e_var against var, products of errors, fused multiply-adds) are left to the margin
of check().
"""
import math
import zlib

import torch
import torch.nn.functional as F

from attn_bounds import MARGIN, TINY, U, check  # noqa: F401  (re-exported)

U32 = 2.0 ** -24       # fp32 unit roundoff
EPS = 1e-5
DISTRIBUTIONS = ("noise", "corr", "offset")
NAMES = ("a", "b", "mean", "rstd", "t", "P", "Q", "R", "dx0", "dx1", "dgamma", "dbeta", "demb")

# name: N, spatial, C0, C1, G, mode, + acc0, acc1, extra, rows0/rows1 (forward slab rows, None: 64 if HW % 64 == 0
# else HW), fold (slab rows folded before the reductions), W (row stride of the emb / demb buffers)
CASES = {
    "cg2_hw16":      dict(N=3, sp=(4, 4), C0=64, C1=0, G=32, mode=0, acc0=1, extra=True),
    "cg3_odd_ss":    dict(N=2, sp=(16, 16), C0=96, C1=0, G=32, mode=1),
    "straddle_cg24": dict(N=3, sp=(8, 8), C0=64, C1=32, G=4, mode=0, acc0=1, acc1=0, extra=True),
    "cfgB_256_128":  dict(N=2, sp=(16, 16), C0=256, C1=128, G=32, mode=0, acc0=0, acc1=1, extra=True,
                          rows0=64, rows1=256),
    "cfgB_512_256":  dict(N=2, sp=(8, 8), C0=512, C1=256, G=32, mode=0, acc0=1, acc1=1),
    "emb_add_slot":  dict(N=3, sp=(16, 16), C0=128, C1=0, G=32, mode=2, W=448, rows0=16),   # fwd slab: 16 rows, s12: 4
    "ss_slot":       dict(N=3, sp=(8, 8), C0=128, C1=0, G=32, mode=1, W=640),
    "tall_slab":     dict(N=1, sp=(275, 256), C0=16, C1=0, G=2, mode=1),
    "folded":        dict(N=1, sp=(275, 256), C0=16, C1=0, G=2, mode=0, fold=4),
    "vol3d":         dict(N=2, sp=(4, 4, 4), C0=64, C1=0, G=32, mode=1),
    "hw1":           dict(N=3, sp=(1, 1), C0=512, C1=0, G=32, mode=1),
    "cg256":         dict(N=2, sp=(4, 4), C0=256, C1=0, G=1, mode=0, extra=True),
}


def geometry(case):
    """The case with its defaults filled in and the derived sizes (HW, C, Cg, slab rows, fp32 chain lengths)."""
    c = dict(acc0=0, acc1=0, extra=False, rows0=None, rows1=None, fold=1, W=None)
    c.update(CASES[case] if isinstance(case, str) else case)
    HW = math.prod(c["sp"])
    C = c["C0"] + c["C1"]
    dflt = 64 if HW % 64 == 0 else HW
    c.update(HW=HW, C=C, Cg=C // c["G"], rows0=c["rows0"] or dflt, rows1=c["rows1"] or dflt, rows=dflt)
    if c["W"] is None:
        c["W"] = 2 * C
    return c


def straddles(c, g):
    return g * c["Cg"] < c["C0"] < (g + 1) * c["Cg"]


def vector_branch(c, g):
    """gn_prep_kernel reads group g as 16-byte vectors with fp32 partial sums (else: scalar, fp64)."""
    return c["Cg"] % 2 == 0 and not straddles(c, g)


def _chain(rows, fold):
    return -(-rows // 32) + min(rows, 32) + (fold if fold > 1 else 0)


# ------------------------------------------------------------------ inputs
def make_inputs(case, dist):
    """bf16 x, dz, extra, old0, old1 and fp32 gamma, beta, emb, dg0, db0 from a generator seeded by (case, dist).
    noise: x = 2 randn + 0.5, white dz.  corr: the same x, dz = 0.3 randn + a per-channel offset ~ N(0.5, 1) +
    0.25 x (the offset's mean keeps A1, and so R, away from zero in groups of any size: with a centred offset the
    two 8-channel groups of tall_slab drew R at 8 % of P dz).  offset: x = randn + 16, dz = 0.3 randn + the offset +
    0.5 (x - 16): the correlated part is taken from the centred x and doubled, because with 0.25 x the constant 4
    it adds to dz makes P dz sixteen times Q (x - mean) and the case would stop exercising Q
    (test_gn_bounds.py::test_inputs_exercise_the_mean_terms).
    gamma in [0.5, 1.5); beta 0.1 randn, emb 0.3 randn; extra and the old destinations bf16 randn; the existing
    gradients dg0, db0 = sqrt(N HW) randn, the size of a sum of N HW terms of order one."""
    c = geometry(case)
    name = case if isinstance(case, str) else repr(sorted(case.items()))
    g = torch.Generator().manual_seed(zlib.crc32(f"{name}/{dist}".encode()))
    N, HW, C, C0 = c["N"], c["HW"], c["C"], c["C0"]

    def rnd(*s):
        return torch.randn(*s, generator=g)

    if dist in ("noise", "corr"):
        x = (2.0 * rnd(N, HW, C) + 0.5).to(torch.bfloat16)
    elif dist == "offset":
        x = (rnd(N, HW, C) + 16.0).to(torch.bfloat16)
    else:
        raise ValueError(dist)
    white, off = rnd(N, HW, C), rnd(1, 1, C) + 0.5
    if dist == "noise":
        dz = white
    elif dist == "corr":
        dz = 0.3 * white + off + 0.25 * x.float()
    else:
        dz = 0.3 * white + off + 0.5 * (x.float() - 16.0)
    inp = dict(case=c, x=x, dz=dz.to(torch.bfloat16),
               gamma=torch.rand(C, generator=g) + 0.5, beta=0.1 * rnd(C),
               emb=0.3 * rnd(N, 2 * C) if c["mode"] == 1 else None,
               extra=rnd(N, HW, C).to(torch.bfloat16) if c["extra"] else None,
               old0=rnd(N, HW, C0).to(torch.bfloat16), old1=rnd(N, HW, C - C0).to(torch.bfloat16),
               dg0=math.sqrt(N * HW) * rnd(C), db0=math.sqrt(N * HW) * rnd(C))
    return inp


def _old(inp):
    """The old destinations where acc is set (zero elsewhere), as one [N][HW][C] fp64 tensor."""
    c = inp["case"]
    o0 = inp["old0"].double() * (1.0 if c["acc0"] else 0.0)
    o1 = inp["old1"].double() * (1.0 if c["acc1"] else 0.0)
    return torch.cat([o0, o1], -1)


def _per_group(v, G):
    """[N][C] -> [N][G] sums."""
    return v.reshape(v.shape[0], G, -1).sum(-1)


def _expand(v, Cg):
    """[N][G] -> [N][C]."""
    return v.repeat_interleave(Cg, dim=1)


# ------------------------------------------------------------------ reference (fp64 autograd of F.group_norm)
def reference(inp):
    c = inp["case"]
    N, HW, C, C0, G, mode = c["N"], c["HW"], c["C"], c["C0"], c["G"], c["mode"]
    x = inp["x"].double().transpose(1, 2).contiguous().requires_grad_()      # [N][C][HW]
    dz = inp["dz"].double().transpose(1, 2)
    gamma = inp["gamma"].double().requires_grad_()
    beta = inp["beta"].double().requires_grad_()
    leaves = [x, gamma, beta]
    if mode == 1:
        emb = inp["emb"].double().requires_grad_()
        leaves.append(emb)
        z = F.group_norm(x, G, gamma, beta, EPS) * (1 + emb[:, :C, None]) + emb[:, C:, None]
    elif mode == 2:
        e = torch.zeros(N, C, 1, dtype=torch.float64, requires_grad=True)
        leaves.append(e)
        z = F.group_norm(x + e, G, gamma, beta, EPS)
    else:
        z = F.group_norm(x, G, gamma, beta, EPS)
    grads = torch.autograd.grad(z, leaves, dz)
    dx = grads[0].transpose(1, 2)
    if inp["extra"] is not None:
        dx = dx + inp["extra"].double()
    dx = dx + _old(inp)
    xg = inp["x"].double().reshape(N, HW, G, C // G)
    mean = xg.mean((1, 3))
    rstd = 1.0 / torch.sqrt(xg.var((1, 3), unbiased=False) + EPS)
    out = dict(mean=mean, rstd=rstd, t=F.silu(z.detach()).transpose(1, 2), dx0=dx[..., :C0], dx1=dx[..., C0:],
               dgamma=inp["dg0"].double() + grads[1], dbeta=inp["db0"].double() + grads[2],
               demb=grads[3].reshape(N, -1) if mode else None)
    # a, b: the affine the GroupNorm is folded into, written out from the two-pass mean / rstd above and tied to
    # autograd by the assertion that a x + b reproduces its z
    with torch.no_grad():
        z = z.detach()
        m_, r_ = _expand(mean, C // G), _expand(rstd, C // G)
        s = 1 + inp["emb"].double()[:, :C] if mode == 1 else torch.ones(N, C, dtype=torch.float64)
        sh = inp["emb"].double()[:, C:] if mode == 1 else torch.zeros(N, C, dtype=torch.float64)
        out["a"] = r_ * inp["gamma"].double() * s
        out["b"] = (inp["beta"].double() - m_ * r_ * inp["gamma"].double()) * s + sh
        assert torch.allclose(out["a"][:, None] * inp["x"].double() + out["b"][:, None], z.transpose(1, 2),
                              rtol=0, atol=1e-9 * float(1 + z.abs().max()))
    return out


# ------------------------------------------------------------------ closed form (fp64) and bounds
def closed_form(inp):
    """The kernels' algebra in exact (fp64) arithmetic: everything reference() returns plus P, Q, R and the
    intermediate sums the bounds need."""
    c = inp["case"]
    N, HW, C, C0, G, Cg, mode = c["N"], c["HW"], c["C"], c["C0"], c["G"], c["Cg"], c["mode"]
    x, dz = inp["x"].double(), inp["dz"].double()
    gamma, beta = inp["gamma"].double(), inp["beta"].double()
    cnt = Cg * HW
    Sx, Sxx = x.sum(1), (x * x).sum(1)
    m = _per_group(Sx, G) / cnt
    var = (_per_group(Sxx, G) / cnt - m * m).clamp(min=0)
    r = 1.0 / torch.sqrt(var + EPS)
    mc, rc = _expand(m, Cg), _expand(r, Cg)
    if mode == 1:
        s, sh = 1 + inp["emb"].double()[:, :C], inp["emb"].double()[:, C:]
    else:
        s, sh = torch.ones(N, C, dtype=torch.float64), torch.zeros(N, C, dtype=torch.float64)
    gp = gamma * s
    a = rc * gp
    b = (beta - mc * rc * gamma) * s + sh
    z = a[:, None] * x + b[:, None]
    S1, S2 = dz.sum(1), (dz * x).sum(1)
    D = S2 - mc * S1
    A1 = _expand(_per_group(gp * S1, G) / cnt, Cg)
    A2 = _expand(_per_group(gp * rc * D, G) / cnt, Cg)
    P, Q = rc * gp, -rc * rc * A2
    R = rc * rc * A2 * mc - rc * A1
    core = P[:, None] * dz + Q[:, None] * x + R[:, None]
    ex = inp["extra"].double() if inp["extra"] is not None else torch.zeros_like(core)
    dx = core + ex + _old(inp)
    if mode == 1:
        demb = torch.cat([gamma * rc * D + beta * S1, S1], 1)
    elif mode == 2:
        demb = P * S1 + Q * Sx + R * HW
    else:
        demb = None
    return dict(mean=m, rstd=r, a=a, b=b, t=F.silu(z), P=P, Q=Q, R=R, dx0=dx[..., :C0], dx1=dx[..., C0:],
                dgamma=inp["dg0"].double() + (s * rc * D).sum(0), dbeta=inp["db0"].double() + (s * S1).sum(0),
                demb=demb,
                _z=z, _s=s, _sh=sh, _gp=gp, _S1=S1, _S2=S2, _Sx=Sx, _D=D, _A1=A1, _A2=A2, _mc=mc, _rc=rc, _ex=ex)


def bounds(inp, cf, fused=False):
    """Elementwise first-order worst-case error bounds of every output (module docstring), from closed_form().
    fused: the forward outputs of fmd_gn_fused_apply (statistics straight from the activation)."""
    c = inp["case"]
    N, HW, C, C0, G, Cg, mode = c["N"], c["HW"], c["C"], c["C0"], c["G"], c["Cg"], c["mode"]
    u = U32
    x, dz = inp["x"].double(), inp["dz"].double()
    gamma, beta = inp["gamma"].double().abs(), inp["beta"].double().abs()
    cnt = Cg * HW
    # fp32 chain lengths per channel (forward slabs, + gn_prep's vector branch) and of the backward slab
    kf = torch.empty(C, dtype=torch.float64)
    kf[:C0] = _chain(c["rows0"], c["fold"])
    kf[C0:] = _chain(c["rows1"], c["fold"])
    for g in range(G):
        if vector_branch(c, g):
            rows = c["rows0"] if (g + 1) * Cg <= C0 else c["rows1"]
            kf[g * Cg:(g + 1) * Cg] += Cg + -(-(HW // (rows * c["fold"])) // 256) + 2
    kfx = kf.clone()                      # the forward slab as fmd_gn_bwd_prep reads it (mode 2): fp64 from the rows
    kfx[:] = _chain(c["rows0"], c["fold"])
    if fused:
        kf[:] = 18
    kb = _chain(c["rows"], c["fold"])
    ax, adz = x.abs().sum(1), dz.abs().sum(1)
    e_F1, e_F2 = kf * u * ax, (kf + 1) * u * (x * x).sum(1)
    e_S1, e_S2 = kb * u * adz, (kb + 1) * u * (dz * x).abs().sum(1)
    m, r = cf["mean"], cf["rstd"]
    e_G1, e_G2 = _per_group(e_F1, G), _per_group(e_F2, G)
    e_m = e_G1 / cnt + u * m.abs()
    e_r = 0.5 * r ** 3 * (e_G2 / cnt + 2 * m.abs() * e_G1 / cnt) + u * r
    mc, rc, e_mc, e_rc = cf["_mc"], cf["_rc"], _expand(e_m, Cg), _expand(e_r, Cg)
    a, b, s, sh, gp = cf["a"], cf["b"], cf["_s"].abs(), cf["_sh"].abs(), cf["_gp"].abs()
    rnd_b = 4 * u * (beta * s + (mc * a).abs() + sh)
    e_a = a.abs() * (e_rc / rc + 3 * u)
    e_b = gp * (mc.abs() * e_rc + rc * e_mc) + rnd_b
    z = cf["_z"]
    xc = (x - mc[:, None]).abs()
    e_z = (a.abs() * e_rc / rc)[:, None] * xc + (a.abs() * e_mc)[:, None] \
        + u * (5 * (a[:, None] * x).abs() + (b.abs() + rnd_b / u)[:, None])
    sg = torch.sigmoid(z)
    t = cf["t"]
    e_t = U * t.abs() + (sg * (1 + z * (1 - sg))).abs() * e_z + 8 * u * (1 + z.abs()) * t.abs()
    out = dict(mean=e_m, rstd=e_r, a=e_a, b=e_b, t=e_t)
    if fused:
        return out
    S1, D, A1, A2 = cf["_S1"], cf["_D"], cf["_A1"], cf["_A2"]
    e_D = e_S2 + mc.abs() * e_S1 + e_mc * S1.abs()
    e_rD = rc * e_D + e_rc * D.abs()
    e_A1 = _expand(_per_group(gp * e_S1, G) / cnt, Cg)
    e_A2 = _expand(_per_group(gp * e_rD, G) / cnt, Cg)
    P, Q, R = cf["P"], cf["Q"], cf["R"]
    e_P = gp * e_rc + u * P.abs()
    e_Q = 2 * rc * e_rc * A2.abs() + rc * rc * e_A2 + u * Q.abs()
    e_rA = e_rc * A1.abs() + rc * e_A1
    e_R = e_Q * mc.abs() + Q.abs() * e_mc + e_rA + u * R.abs()
    dx = torch.cat([cf["dx0"], cf["dx1"]], -1)
    mag = (P[:, None] * dz).abs() + (Q[:, None] * x).abs() + R.abs()[:, None] + cf["_ex"].abs() + _old(inp).abs()
    e_dx = U * dx.abs() + 6 * u * mag + e_P[:, None] * dz.abs() + e_Q[:, None] * xc \
        + (Q.abs() * e_mc + e_rA)[:, None]
    tg, tb = s * rc * D.abs(), s * S1.abs()
    e_dg = (s * e_rD + u * tg).sum(0) + (N + 1) * u * (tg.sum(0) + inp["dg0"].double().abs())
    e_db = (s * e_S1 + u * tb).sum(0) + (N + 1) * u * (tb.sum(0) + inp["db0"].double().abs())
    out.update(P=e_P, Q=e_Q, R=e_R, dx0=e_dx[..., :C0], dx1=e_dx[..., C0:], dgamma=e_dg, dbeta=e_db, demb=None)
    if mode == 1:
        out["demb"] = torch.cat([gamma * e_rD + beta * e_S1 + u * cf["demb"][:, :C].abs(),
                                 e_S1 + u * S1.abs()], 1)
    elif mode == 2:
        Sx = cf["_Sx"]
        e_Sx = kfx * u * ax
        out["demb"] = e_P * S1.abs() + P.abs() * e_S1 + e_Q * (Sx - mc * HW).abs() \
            + Q.abs() * (e_Sx + HW * e_mc) + HW * e_rA + u * cf["demb"].abs()
    return out


def check_all(got, ref, bnd, tag, margin=MARGIN, names=NAMES):
    """check() of every output separately; returns {name: max err / bound}."""
    return {n: check(got[n], ref[n], bnd[n], f"{tag} {n}", margin)
            for n in names if ref.get(n) is not None and ref[n].numel()}


# ------------------------------------------------------------------ emulation of the kernel arithmetic
MUTANTS = ("no_mean_terms", "no_R", "uncentred_Q", "rstd_1pct", "gp_without_scale", "dbeta_without_scale",
           "demb_swapped", "demb2_no_R", "straddle_src0_only", "acc_ignored", "extra_dropped",
           "last_slab_row_dropped", "dgamma_overwrites")


def applies(mutant, case):
    """Does this mutant change anything in this case?"""
    c = geometry(case)
    if mutant in ("gp_without_scale", "dbeta_without_scale", "demb_swapped"):
        return c["mode"] == 1
    if mutant == "demb2_no_R":
        return c["mode"] == 2
    if mutant == "straddle_src0_only":
        return any(straddles(c, g) for g in range(c["G"]))
    if mutant == "acc_ignored":
        return bool(c["acc1"])
    if mutant == "extra_dropped":
        return bool(c["extra"])
    if mutant == "last_slab_row_dropped":
        return c["HW"] // (c["rows"] * c["fold"]) >= 2
    return True


def _bf(x):
    return x.to(torch.bfloat16)


def slab_rows(v, rows):
    """fmd_channel_stats: [N][HW][C] fp32 -> [N][HW / rows][C], 32 pixel lanes (stride 32) then the lanes in order."""
    N, HW, C = v.shape
    E = HW // rows
    J = -(-rows // 32)
    v = v.reshape(N, E, rows, C)
    if J * 32 != rows:
        v = torch.cat([v, torch.zeros(N, E, J * 32 - rows, C)], 2)
    v = v.reshape(N, E, J, 32, C)
    lanes = torch.zeros(N, E, 32, C)
    for j in range(J):
        lanes = lanes + v[:, :, j]
    out = torch.zeros(N, E, C)
    for i in range(32):
        out = out + lanes[:, :, i]
    return out


def fold_rows(slab, fold):
    """fmd_stats_fold for fold <= its row lanes: `fold` consecutive slab rows added in order in fp32."""
    if fold == 1:
        return slab
    N, E, C = slab.shape
    s = slab.reshape(N, E // fold, fold, C)
    out = torch.zeros(N, E // fold, C)
    for k in range(fold):
        out = out + s[:, :, k]
    return out


def _prep_vector(p):
    """gn_prep_kernel's vector branch: p [B][E][Cg / 2] fp32 (channel pairs already added) -> [B] fp64.  Thread t
    owns rows t, t + 256, ...: four independent chains while four rows remain, the rest into chain 0."""
    B, E, Q = p.shape
    J = -(-E // 256)
    if J * 256 != E:
        p = torch.cat([p, torch.zeros(B, J * 256 - E, Q)], 1)
    p = p.reshape(B, J, 256, Q)
    full = E - (J - 1) * 256
    out = torch.zeros(B, 256)
    for lo, hi, n in ((0, full, J), (full, 256, J - 1)):
        if lo == hi or n == 0:
            continue
        f = [torch.zeros(B, hi - lo) for _ in range(4)]
        j = 0
        while j + 3 < n:
            for k in range(4):
                for q in range(Q):
                    f[k] = f[k] + p[:, j + k, lo:hi, q]
            j += 4
        while j < n:
            for q in range(Q):
                f[0] = f[0] + p[:, j, lo:hi, q]
            j += 1
        out[:, lo:hi] = (f[0] + f[1]) + (f[2] + f[3])
    return out.double().sum(-1)


def emulate(inp, mutant=None):
    """CPU emulation of channel_stats -> (stats_fold) -> gn_prep -> gn_apply_fwd and channel_stats(dz, y) ->
    gn_bwd_prep -> gn_bwd_apply: fp32 slab rows, fp64 across rows and channels (fp32 per thread in gn_prep's
    vector branch), fp32 mean / rstd / a / b / P / Q / R, fp32 apply, bf16 round to nearest.
    `mutant` plants one of MUTANTS (a kernel that is wrong in that way)."""
    assert mutant is None or mutant in MUTANTS
    c = inp["case"]
    N, HW, C, C0, G, Cg, mode = c["N"], c["HW"], c["C"], c["C0"], c["G"], c["Cg"], c["mode"]
    f32 = torch.float32
    x, dz = inp["x"].float(), inp["dz"].float()
    gamma, beta = inp["gamma"], inp["beta"]
    cnt = float(Cg * HW)
    # ---- forward statistics, one slab per source
    srcs = [(x[..., :C0], c["rows0"])] + ([(x[..., C0:], c["rows1"])] if C > C0 else [])
    st = [(fold_rows(slab_rows(v, rw), c["fold"]), fold_rows(slab_rows(v * v, rw), c["fold"])) for v, rw in srcs]
    g1 = torch.zeros(N, G, dtype=torch.float64)
    g2 = torch.zeros(N, G, dtype=torch.float64)
    for g in range(G):
        lo, hi = g * Cg, (g + 1) * Cg
        if vector_branch(c, g):
            k, off = (0, 0) if hi <= C0 else (1, C0)
            for which, dst in ((0, g1), (1, g2)):
                s = st[k][which][:, :, lo - off:hi - off]
                dst[:, g] = _prep_vector(s[..., 0::2] + s[..., 1::2])
        else:
            for k, off, width in ((0, 0, C0), (1, C0, C - C0)):
                a_, b_ = max(lo - off, 0), min(hi - off, width)
                if a_ >= b_ or (k == 1 and mutant == "straddle_src0_only"):
                    continue
                g1[:, g] += st[k][0][:, :, a_:b_].double().sum((1, 2))
                g2[:, g] += st[k][1][:, :, a_:b_].double().sum((1, 2))
    mean = g1 / cnt
    var = (g2 / cnt - mean * mean).clamp(min=0)
    rstd = 1.0 / torch.sqrt(var + float(torch.tensor(EPS, dtype=f32)))
    if mutant == "rstd_1pct":
        rstd = rstd * 1.01
    meanf, rstdf = mean.to(f32), rstd.to(f32)
    mcf, rcf = _expand(meanf, Cg), _expand(rstdf, Cg)
    av = rcf * gamma
    bv = beta - mcf * av
    if mode == 1:
        es, esh = 1.0 + inp["emb"][:, :C], inp["emb"][:, C:]
        av = av * es
        bv = bv * es + esh
    zf = x * av[:, None] + bv[:, None]
    t = _bf(zf * torch.sigmoid(zf))
    # ---- backward statistics (one slab over the concat) and fmd_gn_bwd_prep in fp64
    rb = c["rows"]
    s1 = fold_rows(slab_rows(dz, rb), c["fold"]).double()
    s2 = fold_rows(slab_rows(dz * x, rb), c["fold"]).double()
    if mutant == "last_slab_row_dropped":
        s1, s2 = s1[:, :-1], s2[:, :-1]
    S1, S2 = s1.sum(1), s2.sum(1)
    m, r = mcf.double(), rcf.double()
    s = 1.0 + inp["emb"][:, :C].double() if mode == 1 else torch.ones(N, C, dtype=torch.float64)
    gm, bt = gamma.double(), beta.double()
    gp = gm * s
    gpA = gm if mutant == "gp_without_scale" else gp
    A1 = _expand(_per_group(gpA * S1, G) / cnt, Cg)
    A2 = _expand(_per_group(gpA * r * (S2 - m * S1), G) / cnt, Cg)
    dzxh = r * (S2 - m * S1)
    Pv, Qv = r * gpA, -r * r * A2
    Rv = -r * A1 if mutant == "uncentred_Q" else r * r * A2 * m - r * A1
    P, Q, R = Pv.to(f32), Qv.to(f32), Rv.to(f32)
    gb_g = (s * dzxh).to(f32)
    gb_b = (S1 if mutant == "dbeta_without_scale" else s * S1).to(f32)
    dg = torch.zeros(C) if mutant == "dgamma_overwrites" else inp["dg0"].clone()
    db = inp["db0"].clone()
    acc_g, acc_b = torch.zeros(C), torch.zeros(C)
    for n in range(N):
        acc_g, acc_b = acc_g + gb_g[n], acc_b + gb_b[n]
    dg, db = dg + acc_g, db + acc_b
    demb = None
    if mode == 1:
        halves = [(gm * dzxh + bt * S1).to(f32), S1.to(f32)]
        demb = torch.cat(halves[::-1] if mutant == "demb_swapped" else halves, 1)
    elif mode == 2:
        Sx = fold_rows(slab_rows(x, c["rows0"]), c["fold"]).double().sum(1)
        demb = (Pv * S1 + Qv * Sx + (0.0 if mutant == "demb2_no_R" else Rv * HW)).to(f32)
    # ---- fmd_gn_bwd_apply
    Qa = torch.zeros_like(Q) if mutant == "no_mean_terms" else Q
    Ra = torch.zeros_like(R) if mutant in ("no_mean_terms", "no_R") else R
    dx = P[:, None] * dz + Qa[:, None] * x + Ra[:, None]
    if inp["extra"] is not None and mutant != "extra_dropped":
        dx = dx + inp["extra"].float()
    dx0, dx1 = dx[..., :C0], dx[..., C0:]
    if c["acc0"]:
        dx0 = dx0 + inp["old0"].float()
    if c["acc1"] and mutant != "acc_ignored":
        dx1 = dx1 + inp["old1"].float()
    return dict(mean=meanf, rstd=rstdf, a=av, b=bv, t=t, P=P, Q=Q, R=R, dx0=_bf(dx0), dx1=_bf(dx1), dgamma=dg,
                dbeta=db, demb=demb)
