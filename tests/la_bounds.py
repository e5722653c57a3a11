"""fp64 reference, first-order error bounds and an fp32 emulation of the linear attention kernels
(csrc/attention.hip: la_kstats, la_ctx_part, la_ctx_reduce, la_out, la_bwd_q, la_bwd_reduce, la_bwd_kv), shared by
test_la_bounds.py (CPU) and test_gpu_linear_attention.py (GPU).

Everything works on the canonical planes the kernels see, q, dO [BH][Tq][dh] and k, v [BH][Tk][dh]; the head-split
maps of attn_bounds.py carry them to and from the token layouts.

The operation (LinearQKVAttention), per plane, n a token, d and e head dims:
  ks = softmax over tokens of k:  x_nd = k_nd - M_d, M_d = max_n k_nd, Z_d = sum_n exp(x_nd), ks = exp(x) / Z
  qs = softmax over d of q:       y_nd = q_nd - max_d q_nd, qs = exp(y) / sum_d exp(y)
  A_de = sum_n ks_nd v_ne,  s_d = sum_n ks_nd,  ctx = A / (s + eps),  O = qs ctx
and the closed-form backward the kernels use (G = dctx):
  dqs = dO ctx^T,  dot_n = sum_d qs dqs,  dQ = qs (dqs - dot)
  G_de = sum_n qs_nd dO_ne,  dA = G / (s + eps),  P_d = sum_e G ctx,  ds = -P / (s + eps),  cc = P + ds s
  dV = ks dA,  dks0 = v dA^T,  dK = ks (dks0 + ds - cc)          (cc = sum_n ks dks: the column-softmax Jacobian)

The kernel arithmetic the bounds are derived from (see the kernel source): inputs are exact bf16, everything is
fp32, and O, dQ, dK, dV are rounded once to bf16 (round to nearest); the state (ctx | M | Z | s) stays fp32.
With u = 2^-8, w = 2^-24 the unit roundoffs, |.| elementwise and rho a relative, E an absolute error:

  exp.   The argument x = k - M (or q - max q) is a difference of two bf16 values, rounded to fp32: w |x|.
         __expf(x) = exp2(x log2 e): the constant's and the product's roundings each move the argument of exp2
         by w |x| log2 e, i.e. the result by w |x| relative; exp2 itself is good to one ulp (2 w).  Together
         rho_exp(x) = (3 |x| + 2) w: the term that grows with |k - M| and |q - max q|.
  Z.     la_kstats keeps a running (m, z) per column in four interleaved row groups, z = z exp(m - mn) + exp(x - mn),
         then combines groups, then la_combine_stats combines chunks, always z exp(m_part - m_whole).  The maxima
         only rise along that path, so the exponent arguments a term exp(k_nd - .) meets add up to exactly |x_nd|,
         through at most L + 2 non-trivial exps (exp(0) = 1 is exact), L = ceil(per_k / 4) the steps of a group,
         and 2 L + 4 + nch_k multiplications and additions.  All terms are positive, so
           rho_Z[d] = w (3 sum_n ks_nd |x_nd|  +  4 L + nch_k + 8),     E_Z = Z rho_Z.
         M is a maximum of bf16 values and must be exact.
  ks.    exp(x) * (1 / Z): rho_ks[n,d] = (3 |x_nd| + 5) w + rho_Z[d]   (exp, reciprocal 2 w, product w).
  qs.    rho_qs[n,d] = (3 |y_nd| + 5) w + rho_z[n],  rho_z[n] = w (sum_d qs_nd (3 |y_nd| + 2) + dh).
  sums over tokens run sequentially over the rows of a chunk (la_ctx_part, la_bwd_q; zero padding adds exactly),
         then over the chunks' partial slabs in order: c_k = (per_k + nch_k + 1) w, c_q = (per_q + nch_q + 1) w
         (one for the products); sums over a head dim: c_d = (dh + 1) w.
  E_s   = sum_n ks rho_ks + c_k s
  E_A   = sum_n ks rho_ks |v| + c_k sum_n ks |v|
  rho_i = E_s / (s + eps) + 4 w                      1 / (s + eps): the sum, the reciprocal, the product with it
  E_ctx = E_A / (s + eps) + |ctx| rho_i
  E_O   = (qs rho_qs) |ctx| + qs E_ctx + c_d qs |ctx| + u |O|
  E_dqs = |dO| E_ctx^T + c_d |dO| |ctx|^T
  E_dot = sum_d qs (rho_qs |dqs| + E_dqs) + c_d sum_d qs |dqs|
  E_dQ  = qs (E_dqs + E_dot + 2 w (|dqs| + |dot|)) + (rho_qs + u) |dQ|
  E_G   = sum_n qs rho_qs |dO| + c_q sum_n qs |dO|
  E_dA  = E_G / (s + eps) + |dA| rho_i
  E_P   = sum_e (E_G |ctx| + |G| E_ctx) + (dh + 3) w sum_e |G| |ctx|
  E_ds  = E_P / (s + eps) + |ds| rho_i
  E_cc  = E_P + E_ds s + |ds| E_s + 2 w (|P| + |ds| s)
  E_dV  = (ks rho_ks) |dA| + ks E_dA + c_d ks |dA| + u |dV|
  E_dk0 = |v| E_dA^T + c_d |v| |dA|^T
  E_dK  = ks (E_dk0 + E_ds + E_cc + 2 w (|dks0| + |ds| + |cc|)) + (rho_ks + w + u) |dK|
Every c counts the longest sequential fp32 sum of the kernel (rows per chunk, plus chunks, plus dh); none is
fitted to a measurement.  Second-order terms are left to the margin of check().
"""
import math
import zlib

import torch

from attn_bounds import (MARGIN, TINY, U, _bf, _bf_trunc, check, check_unbiased,  # noqa: F401 (re-exported)
                         join_heads, split_heads)

W32 = 2.0 ** -24       # fp32 unit roundoff
LA_D, LA_MAXCH, LA_SB = 64, 64, 64
DISTRIBUTIONS = ("flat", "peaked", "offset")
OUTPUTS = ("O", "dQ", "dK", "dV")
STATE = ("ctx", "Z", "s")


# ------------------------------------------------------------------ chunking (restatement of la_args)
def la_chunks(T):
    nch = min(LA_MAXCH, max(1, -(-T // 1024)))
    return nch, -(-T // nch)


def la_instance(Tq, Tk):
    """(nchq, perq, nchk, perk, (rows in the last 64-row LDS sub-block of a full query chunk, of a full key chunk)).
    The source of truth is la_args() in csrc/attention.hip."""
    (nchq, perq), (nchk, perk) = la_chunks(Tq), la_chunks(Tk)
    return nchq, perq, nchk, perk, ((min(Tq, perq) - 1) % LA_SB + 1, (min(Tk, perk) - 1) % LA_SB + 1)


# ------------------------------------------------------------------ reference and bounds (fp64)
def reference(q, k, v, do, eps):
    """LinearQKVAttention forward and closed-form backward in fp64 (module docstring)."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    M = k.max(1).values
    xk = k - M[:, None]
    ek = xk.exp()
    Z = ek.sum(1)
    ks = ek / Z[:, None]
    xq = q - q.max(-1, keepdim=True).values
    eq = xq.exp()
    qs = eq / eq.sum(-1, keepdim=True)
    s = ks.sum(1)
    inv = 1.0 / (s + eps)
    A = ks.transpose(1, 2) @ v
    ctx = A * inv[..., None]
    O = qs @ ctx
    dqs = do @ ctx.transpose(1, 2)
    dot = (qs * dqs).sum(-1, keepdim=True)
    G = qs.transpose(1, 2) @ do
    dA = G * inv[..., None]
    P = (G * ctx).sum(-1)
    ds = -P * inv
    cc = P + ds * s
    dks0 = v @ dA.transpose(1, 2)
    return dict(O=O, dQ=qs * (dqs - dot), dK=ks * (dks0 + (ds - cc)[:, None]), dV=ks @ dA, ctx=ctx, M=M, Z=Z, s=s,
                ks=ks, qs=qs, xk=xk, xq=xq, A=A, dqs=dqs, dot=dot, G=G, dA=dA, P=P, ds=ds, cc=cc, dks0=dks0)


def bounds(ref, q, k, v, do, eps):
    """Elementwise first-order worst-case error bounds of O, dQ, dK, dV, ctx, Z, s (module docstring)."""
    va, doa = v.double().abs(), do.double().abs()
    Tq, dh = q.shape[1], q.shape[2]
    nchq, perq, nchk, perk, _ = la_instance(Tq, k.shape[1])
    w = W32
    ks, qs, s, ctx = ref["ks"], ref["qs"], ref["s"], ref["ctx"]
    xk, xq = ref["xk"].abs(), ref["xq"].abs()
    t = lambda m: m.transpose(1, 2)
    L = -(-perk // 4)
    rZ = w * (3 * (ks * xk).sum(1) + 4 * L + nchk + 8)
    rks = (3 * xk + 5) * w + rZ[:, None]
    rqs = (3 * xq + 5) * w + w * ((qs * (3 * xq + 2)).sum(-1, keepdim=True) + dh)
    ck, cq, cd = (perk + nchk + 1) * w, (perq + nchq + 1) * w, (dh + 1) * w
    inv = 1.0 / (s + eps)
    ksr, qsr = ks * rks, qs * rqs
    E_s = ksr.sum(1) + ck * s
    E_A = t(ksr) @ va + ck * (t(ks) @ va)
    rinv = E_s * inv + 4 * w
    actx = ctx.abs()
    E_ctx = E_A * inv[..., None] + actx * rinv[..., None]
    E_O = qsr @ actx + qs @ E_ctx + cd * (qs @ actx) + U * ref["O"].abs()
    dqs, dot = ref["dqs"].abs(), ref["dot"].abs()
    E_dqs = doa @ t(E_ctx) + cd * (doa @ t(actx))
    E_dot = (qsr * dqs + qs * E_dqs).sum(-1, keepdim=True) + cd * (qs * dqs).sum(-1, keepdim=True)
    E_dQ = qs * (E_dqs + E_dot + 2 * w * (dqs + dot)) + (rqs + U) * ref["dQ"].abs()
    G, dA, ds = ref["G"].abs(), ref["dA"].abs(), ref["ds"].abs()
    E_G = t(qsr) @ doa + cq * (t(qs) @ doa)
    E_dA = E_G * inv[..., None] + dA * rinv[..., None]
    E_P = (E_G * actx + G * E_ctx).sum(-1) + (dh + 3) * w * (G * actx).sum(-1)
    E_ds = E_P * inv + ds * rinv
    E_cc = E_P + E_ds * s + ds * E_s + 2 * w * (ref["P"].abs() + ds * s)
    E_dV = ksr @ dA + ks @ E_dA + cd * (ks @ dA) + U * ref["dV"].abs()
    E_dk0 = va @ t(E_dA) + cd * (va @ t(dA))
    E_t = E_dk0 + (E_ds + E_cc)[:, None] + 2 * w * (ref["dks0"].abs() + (ds + ref["cc"].abs())[:, None])
    E_dK = ks * E_t + (rks + w + U) * ref["dK"].abs()
    return dict(O=E_O, dQ=E_dQ, dK=E_dK, dV=E_dV, ctx=E_ctx, Z=ref["Z"] * rZ, s=E_s)


def check_all(got, ref, bnd, tag, margin=MARGIN, names=OUTPUTS + STATE):
    """check() of each tensor separately, M exact; returns {name: max ratio}."""
    if "M" in got:
        assert torch.equal(got["M"].double(), ref["M"]), f"{tag} M: the column maximum of bf16 values is not exact"
    return {n: check(got[n], ref[n], bnd[n], f"{tag} {n}", margin) for n in names if n in got}


# ------------------------------------------------------------------ emulation of the kernel arithmetic
MUTANTS = ("drop_last_key", "per_floor", "stats_no_rescale", "max_first_chunk_only", "eps_dropped", "no_cc", "no_ds",
           "dq_no_dot", "q_pad_in_softmax", "swap_dk_dv", "bwd_uses_nchk_for_dctx", "out_trunc")


def _chunked(x, nch, per, T, fill, drop_last=False):
    """[BH][T][dh] -> [BH][nch][PP][dh], PP = per rounded up to whole 64-row sub-blocks, and the mask [nch][PP] of
    the rows la_range() gives chunk c: n = c per + j, j < per, n < T (drop_last: the last row of a chunk is lost)."""
    PP = -(-per // LA_SB) * LA_SB
    j = torch.arange(PP)[None, :]
    n = torch.arange(nch)[:, None] * per + j
    n1 = (torch.arange(nch)[:, None] * per + per).clamp(max=T)
    valid = (j < per) & (n < (n1 - 1 if drop_last else n1))
    xc = x[:, n.clamp(max=T - 1).reshape(-1)].reshape(x.shape[0], nch, PP, x.shape[-1])
    return torch.where(valid[None, :, :, None], xc, torch.full_like(xc, fill)), valid


def _token_outer(a, b, per):
    """Per chunk, acc[d][e] += a[j][d] b[j][e] row after row (la_ctx_part / la_bwd_q), and the column sums of a."""
    BH, nch, _, dh = a.shape
    acc, ssum = torch.zeros(BH, nch, dh, dh), torch.zeros(BH, nch, dh)
    for j in range(min(per, a.shape[2])):
        acc = acc + a[:, :, j, :, None] * b[:, :, j, None, :]
        ssum = ssum + a[:, :, j]
    return acc, ssum


def _slab_sum(part, n):
    out = torch.zeros_like(part[:, 0])
    for c in range(n):
        out = out + part[:, c]
    return out


def emulate(q, k, v, do, eps, mutant=None):
    """fp32 emulation of la_fwd / la_bwd in the kernels' structure: la_args chunking, 64-row sub-blocks, the four
    interleaved row groups of la_kstats, the per-chunk M / Z combine, partial A / s / dctx slabs summed in chunk
    order, bf16 stores.  `mutant` plants one of MUTANTS (a kernel that is wrong in that way).  Rows a mutant never
    writes read as zero."""
    assert mutant is None or mutant in MUTANTS
    qf, kf, vf, dof = (t.float() for t in (q, k, v, do))
    BH, Tq, dh = qf.shape
    Tk = kf.shape[1]
    (nchq, perq), (nchk, perk) = la_chunks(Tq), la_chunks(Tk)
    if mutant == "per_floor":
        perq, perk = max(1, Tq // nchq), max(1, Tk // nchk)
    eps = torch.tensor(0.0 if mutant == "eps_dropped" else eps, dtype=torch.float32)
    store = _bf_trunc if mutant == "out_trunc" else _bf
    ninf = -math.inf

    # la_kstats: running (m, z) per column in four row groups, then the group combine
    kc, kvalid = _chunked(kf, nchk, perk, Tk, ninf)
    m, z = torch.full((BH, nchk, 4, dh), ninf), torch.zeros(BH, nchk, 4, dh)
    for i in range(0, -(-min(perk, Tk) // 4) * 4, 4):
        x, ok = kc[:, :, i:i + 4], kvalid[None, :, i:i + 4, None]
        mn = torch.maximum(m, x)
        zn = z * torch.exp(m - mn) + torch.exp(x - mn)
        m, z = torch.where(ok, mn, m), torch.where(ok, zn, z)
    Mc = m.max(2).values
    Zc = torch.zeros(BH, nchk, dh)
    for i in range(4):
        Zc = Zc + torch.where(m[:, :, i] > ninf, z[:, :, i] * torch.exp(m[:, :, i] - Mc), torch.zeros(()))
    # la_combine_stats
    M = Mc[:, 0] if mutant == "max_first_chunk_only" else Mc.max(1).values
    Z = torch.zeros(BH, dh)
    for c in range(nchk):
        scale = torch.ones(()) if mutant == "stats_no_rescale" else torch.exp(Mc[:, c] - M)
        Z = Z + torch.where(Mc[:, c] > ninf, Zc[:, c] * scale, torch.zeros(()))
    Zi = torch.where(Z > 0, 1.0 / Z, torch.zeros(()))

    def stage_kv(drop_last=False):   # la_stage_kv: zero padded ks, v rows
        kcc, ok = _chunked(kf, nchk, perk, Tk, 0.0, drop_last)
        ksc = torch.where(ok[None, :, :, None], torch.exp(kcc - M[:, None, None]) * Zi[:, None, None], torch.zeros(()))
        return ksc, _chunked(vf, nchk, perk, Tk, 0.0, drop_last)[0], ok

    # la_ctx_part, la_ctx_reduce
    ksc, vc, _ = stage_kv(mutant == "drop_last_key")
    partA, parts = _token_outer(ksc, vc, perk)
    s = _slab_sum(parts, nchk)
    inv = 1.0 / (s + eps)
    ctx = _slab_sum(partA, nchk) * inv[..., None]

    # la_q_softmax
    if mutant == "q_pad_in_softmax":
        qs = torch.softmax(torch.cat([qf, torch.zeros(BH, Tq, LA_D - dh)], -1), -1)[..., :dh]
    else:
        e = torch.exp(qf - qf.max(-1, keepdim=True).values)
        zq = torch.zeros(BH, Tq)
        for d in range(dh):
            zq = zq + e[..., d]
        qs = e * (1.0 / zq)[..., None]
    # la_out
    O = torch.zeros(BH, Tq, dh)
    for d in range(dh):
        O = O + qs[..., d, None] * ctx[:, None, d, :]

    # la_bwd_q: dq, partial dctx per query chunk
    dqs = dof @ ctx.transpose(1, 2)
    dot = (qs * dqs).sum(-1, keepdim=True)
    dQ = qs * dqs if mutant == "dq_no_dot" else qs * (dqs - dot)
    qrows = _chunked(qf, nchq, perq, Tq, 0.0)[1]
    covered = torch.zeros(Tq, dtype=torch.bool)
    covered[(torch.arange(nchq)[:, None] * perq + torch.arange(qrows.shape[1])[None, :])[qrows]] = True
    dQ = torch.where(covered[None, :, None], dQ, torch.zeros(()))
    partG, _ = _token_outer(_chunked(qs, nchq, perq, Tq, 0.0)[0], _chunked(dof, nchq, perq, Tq, 0.0)[0], perq)
    # la_bwd_reduce
    if mutant == "bwd_uses_nchk_for_dctx":   # the slabs past nchq still hold the forward's partial A
        G = _slab_sum(torch.cat([partG, partA[:, nchq:]], 1), nchk)
    else:
        G = _slab_sum(partG, nchq)
    dA = G * inv[..., None]
    P = (G * ctx).sum(-1)
    ds = -P * inv
    cc = torch.zeros_like(P) if mutant == "no_cc" else P + ds * s
    if mutant == "no_ds":
        ds = torch.zeros_like(ds)
    # la_bwd_kv
    ksc, vc, ok = stage_kv()
    dVc = ksc @ dA[:, None]
    dKc = ksc * (vc @ dA.transpose(1, 2)[:, None] + ds[:, None, None] - cc[:, None, None])
    dK, dV = torch.zeros(BH, Tk, dh), torch.zeros(BH, Tk, dh)
    rows = (torch.arange(nchk)[:, None] * perk + torch.arange(ok.shape[1])[None, :])[ok]
    dK[:, rows], dV[:, rows] = dKc[:, ok], dVc[:, ok]
    if mutant == "swap_dk_dv":
        dK, dV = dV, dK
    return dict(O=store(O), dQ=store(dQ), dK=store(dK), dV=store(dV), ctx=ctx, M=M, Z=Z, s=s)


# ------------------------------------------------------------------ inputs
def make_inputs(key, dist, BH, Tq, Tk, dh, positive=False):
    """Canonical bf16 q, do [BH][Tq][dh] and k, v [BH][Tk][dh] from a generator seeded by (key, dist).
    flat: q, k, v = randn * 0.7 (what the max-norm tests use); peaked: k * 2 with one token per (plane, column) set
    to 12 (the column softmax is near one-hot and the chunk maxima differ widely), q * 6 (|q - max q| up to 40);
    offset: k + 40, q - 30, v + 3 (a common shift of k or q cancels exactly; at 40 the bf16 spacing is 0.25).
    dO is randn; positive: v, dO > 0 (for check_unbiased only)."""
    g = torch.Generator().manual_seed(zlib.crc32(f"{key}/{dist}".encode()))

    def rnd(*s):
        return torch.randn(*s, generator=g)

    q, k, v, do = rnd(BH, Tq, dh) * 0.7, rnd(BH, Tk, dh) * 0.7, rnd(BH, Tk, dh) * 0.7, rnd(BH, Tq, dh)
    if dist == "peaked":
        q, k = q * 6.0, k * 2.0
        tok = torch.randint(0, Tk, (BH, 1, dh), generator=g)
        k.scatter_(1, tok, 12.0)
    elif dist == "offset":
        q, k, v = q - 30.0, k + 40.0, v + 3.0
    elif dist != "flat":
        raise ValueError(dist)
    if positive:
        v, do = v.abs(), do.abs()
    return tuple(t.to(torch.bfloat16) for t in (q, k, v, do))


# ------------------------------------------------------------------ the case rows of test_gpu_linear_attention.py
# self (B, T, heads, dh, raw), cross (B, Tq, Tk, heads, dh, raw) -> la_instance(Tq, Tk) the row must reach
SELF_CASES = [
    ((2, 1, 2, 12, 0), (1, 1, 1, 1, (1, 1))), ((2, 1, 2, 64, 1), (1, 1, 1, 1, (1, 1))),   # one token
]
for _dh in (12, 24, 40, 64):                         # one partial sub-block; both head splits at every dh
    for _raw in (0, 1):
        SELF_CASES.append(((2, 17, 2, _dh, _raw), (1, 17, 1, 17, (17, 17))))
SELF_CASES += [
    ((1, 17, 3, 1, 0), (1, 17, 1, 17, (17, 17))),                   # dh = 1: qs = 1, dQ = 0 exactly
    ((2, 64, 3, 24, 1), (1, 64, 1, 64, (64, 64))),                  # one full sub-block
    ((2, 65, 3, 24, 0), (1, 65, 1, 65, (1, 1))),                    # ... and one row
    ((3, 100, 3, 24, 1), (1, 100, 1, 100, (36, 36))),
    ((1, 1024, 2, 32, 0), (1, 1024, 1, 1024, (64, 64))),            # the last T with one chunk
    ((1, 1025, 2, 32, 1), (2, 513, 2, 513, (1, 1))),                # two chunks, a one-row sub-block
    ((1, 2100, 1, 16, 0), (3, 700, 3, 700, (60, 60))),
    ((1, 65537, 1, 8, 0), (64, 1025, 64, 1025, (1, 1))),            # the LA_MAXCH cap: nch no longer follows T
    ((1, 65537, 1, 8, 1), (64, 1025, 64, 1025, (1, 1))),
]
CROSS_CASES = []
for _raw in (0, 1):
    CROSS_CASES += [((2, 70, 2100, 2, 16, _raw), (1, 70, 3, 700, (6, 60))),     # nchq < nchk
                    ((2, 2100, 5, 2, 48, _raw), (3, 700, 1, 5, (60, 5)))]       # nchq > nchk, Tk < 64
CROSS_CASES += [((2, 1, 300, 2, 16, 1), (1, 1, 1, 300, (1, 44))),
                ((1, 1025, 64, 1, 64, 0), (2, 513, 1, 64, (1, 64)))]
# ("self" | "cross", case): the rows repeated at eps = 0.25, where Z, s, ds, cc and eps are live arithmetic
EPS_CASES = [("self", (2, 65, 3, 24, 0)), ("self", (1, 1025, 2, 32, 1)), ("cross", (2, 70, 2100, 2, 16, 1))]
EPS_DEFAULT, EPS_LIVE = 1e-6, 0.25


def canonical(kind, case):
    """(BH, Tq, Tk, dh) of a case row."""
    if kind == "self":
        B, T, heads, dh, _ = case
        return B * heads, T, T, dh
    B, Tq, Tk, heads, dh, _ = case
    return B * heads, Tq, Tk, dh


def all_rows():
    """Every (kind, case, eps) row the GPU tests run."""
    return ([("self", c, EPS_DEFAULT) for c, _ in SELF_CASES] + [("cross", c, EPS_DEFAULT) for c, _ in CROSS_CASES]
            + [(kind, c, EPS_LIVE) for kind, c in EPS_CASES])


def row_key(kind, case, eps):
    return f"{kind} {case}" + ("" if eps == EPS_DEFAULT else f" eps={eps}")
