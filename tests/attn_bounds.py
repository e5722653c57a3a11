"""fp64 reference, first-order error bounds and a bf16 emulation of the MFMA softmax attention
(csrc/attention_mfma.hip), shared by test_attention_bounds.py (CPU) and test_gpu_attention.py (GPU).

Everything works on the canonical planes [B*heads][T][dh] the kernels see; the head-split maps at the end
carry them to and from the reference's token layouts (raw reshape or view/transpose, self or cross).

The kernel arithmetic the bounds are derived from (see the kernel source):
  * S = K Q^T and every other product are MFMA tiles of bf16 operands with fp32 accumulation;
  * the online softmax runs in fp32 in log2 units; l sums the UNROUNDED p;
  * P is rounded to bf16 (round to nearest) before P V and before dO^T P, dS before dS K and dS^T Q;
  * in the backward p = exp2(s - lse) from the saved lse, delta = rowsum(dO * O) from the kernel's own bf16 O;
  * every output is rounded once, with pack2 (round to nearest).
With u = 2^-8 the bf16 unit roundoff (round to nearest: |fl(x) - x| <= u |x|) and |.| elementwise:
  E_O   = 2u P|V|                        one u for P's rounding, one for the output's (|O| <= P|V|)
  E_dV  = u P^T|dO| + u |dV|
  A_i   = sum_d |dO_id| (P|V|)_id        |delta_i - delta_ref_i| <= sum_d |dO_id| E_O_id = 2u A_i
  E_dS  = 2u A_i P_ij + u |dS_ij|        delta's error times P, plus dS's own rounding
  E_dQ  = scale E_dS|K| + u |dQ|
  E_dK  = scale E_dS^T|Q| + u |dK|
  E_lse = dh 2^-24 max_j scale sum_d |q_id k_jd| + 2^-20 max(1, |lse_i|)
fp32 effects (accumulation order, exp2 / log2 of the hardware, the lse's own fp32 rounding inside p) are second
order against u and are left to the margin of check().
"""
import math
import zlib

import torch

U = 2.0 ** -8          # bf16 unit roundoff (8 significand bits, round to nearest)
TINY = 1e-30
MARGIN = 1.5           # second-order terms, fp32 accumulation order, hardware exp2 / log2
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
DISTRIBUTIONS = ("flat", "peaked", "offset")


# ------------------------------------------------------------------ reference and bounds (fp64)
def reference(q, k, v, do, scale):
    """Attention forward and backward in fp64 with an explicit softmax; q, do [BH][Tq][dh], k, v [BH][Tk][dh]."""
    q, k, v, do = (t.double() for t in (q, k, v, do))
    S = scale * (q @ k.transpose(1, 2))
    m = S.max(-1, keepdim=True).values
    lse = (m + (S - m).exp().sum(-1, keepdim=True).log()).squeeze(-1)
    P = (S - lse[..., None]).exp()
    O = P @ v
    delta = (do * O).sum(-1)
    dS = P * (do @ v.transpose(1, 2) - delta[..., None])
    return dict(O=O, lse=lse, dQ=scale * (dS @ k), dK=scale * (dS.transpose(1, 2) @ q), dV=P.transpose(1, 2) @ do,
                P=P, dS=dS, delta=delta)


def bounds(ref, q, k, v, do, scale):
    """Elementwise first-order worst-case error bounds of O, lse, dQ, dK, dV (module docstring)."""
    q, k, v, do = (t.double().abs() for t in (q, k, v, do))
    P, dS = ref["P"], ref["dS"]
    dh = q.shape[-1]
    PV = P @ v
    A = (do * PV).sum(-1)
    E_dS = 2 * U * A[..., None] * P + U * dS.abs()
    lse = ref["lse"]
    return dict(
        O=2 * U * PV,
        dV=U * (P.transpose(1, 2) @ do) + U * ref["dV"].abs(),
        dQ=scale * (E_dS @ k) + U * ref["dQ"].abs(),
        dK=scale * (E_dS.transpose(1, 2) @ q) + U * ref["dK"].abs(),
        lse=dh * 2.0 ** -24 * scale * (q @ k.transpose(1, 2)).max(-1).values
        + 2.0 ** -20 * lse.abs().clamp(min=1.0))


def check(got, ref, bound, name, margin=MARGIN):
    """Assert |got - ref| <= margin * bound + TINY elementwise (a NaN fails); returns max err / bound."""
    err = (got.double() - ref).abs()
    ratio = torch.nan_to_num(err / (bound + TINY), nan=math.inf)
    bad = ~(err <= margin * bound + TINY)
    if bool(bad.any()):
        flat = int(torch.where(bad, ratio, torch.zeros_like(ratio)).argmax())
        idx = tuple(int(i) for i in torch.unravel_index(torch.tensor(flat), ratio.shape))
        raise AssertionError(
            f"{name}: {int(bad.sum())} of {bad.numel()} elements outside {margin} x bound; worst at {idx}: "
            f"got {float(got[idx]):.9g} ref {float(ref[idx]):.9g} err {float(err[idx]):.3e} "
            f"bound {float(bound[idx]):.3e} ratio {float(ratio[idx]):.3f}")
    return float(ratio.max())


def check_all(got, ref, bnd, tag, margin=MARGIN):
    """check() of the five tensors separately; returns {name: max ratio}."""
    return {n: check(got[n], ref[n], bnd[n], f"{tag} {n}", margin) for n in ("O", "lse", "dQ", "dK", "dV")}


def check_unbiased(got, ref, bound, name, margin=MARGIN, sigmas=6.0):
    """Assert that the errors of O (or dV) carry no systematic sign: what check() cannot see.

    A P that is truncated instead of rounded errs by at most u P|V| + 2u |O| <= 1.5 E_O, so no worst-case bound
    at margin 1.5 rejects it; but its errors all point one way, and with v, dO > 0 (make_inputs(positive=True))
    they add up.  Row r (a query of O, a key of dV) owns its P entries and its output roundings, so the row sums
    X_r = sum_d (got - ref)_rd are independent, have zero mean under round to nearest, and |X_r| <= W_r =
    margin * sum_d bound_rd once check() has passed.  Hoeffding: |sum_r X_r| > sigmas * sqrt(sum_r W_r^2) has
    probability <= 2 exp(-sigmas^2 / 2) = 3e-8 at 6.  Returns sum X / limit (the emulation: |.| < 0.05; P
    truncated at 2048 rows: -1.8)."""
    X = (got.double() - ref).sum(-1)
    W = margin * bound.sum(-1)
    assert bool((X.abs() <= W + TINY).all()), f"{name}: run check() first"
    ratio = float(X.sum() / (sigmas * (W ** 2).sum().sqrt()))
    assert abs(ratio) <= 1.0, (f"{name}: signed error sum {float(X.sum()):.4e} over {X.numel()} rows is {ratio:.2f} x "
                               f"the {sigmas}-sigma limit of zero-mean rounding: a biased conversion (truncation?)")
    return ratio


# ------------------------------------------------------------------ emulation of the kernel arithmetic
MUTANTS = ("drop_last_key", "scale_1pct", "no_rescale", "lse_log2", "swap_dk_dv", "no_delta", "p_trunc",
           "extra_query_row")


def _bf(x):
    return x.to(torch.bfloat16).float()


def _bf_trunc(x):
    """fp32 -> bf16 by dropping the low 16 bits (what a shift instead of a rounding conversion does)."""
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32)


def emulate(q, k, v, do, scale, block=32, mutant=None):
    """fp32 / bf16 emulation of attn_mfma_fwd / _bwd_q / _bwd_kv: online softmax over `block`-key blocks in log2
    units, bf16 P into P V, fp32 l from the unrounded p, bf16 O, p = exp2(s - lse) in the backward, delta from the
    bf16 O, bf16 dS, bf16 outputs.  `mutant` plants one of MUTANTS (a kernel that is wrong in that way)."""
    assert mutant is None or mutant in MUTANTS
    qf, kf, vf, dof = (t.float() for t in (q, k, v, do))
    BH, Tq, dh = qf.shape
    Tk = kf.shape[1]
    Tk_eff = Tk - 1 if mutant == "drop_last_key" else Tk
    kf, vf = kf[:, :Tk_eff], vf[:, :Tk_eff]
    sl2 = torch.tensor((1.01 if mutant == "scale_1pct" else 1.0) * scale * LOG2E, dtype=torch.float32)
    rp = _bf_trunc if mutant == "p_trunc" else _bf
    m = torch.full((BH, Tq), -math.inf)
    l = torch.zeros(BH, Tq)
    acc = torch.zeros(BH, Tq, dh)
    for j0 in range(0, Tk_eff, block):
        s = (qf @ kf[:, j0:j0 + block].transpose(1, 2)) * sl2
        mn = torch.maximum(m, s.max(-1).values)
        corr = torch.exp2(m - mn)
        p = torch.exp2(s - mn[..., None])
        l = l * corr + p.sum(-1)
        if not (mutant == "no_rescale" and j0 > 0):
            acc = acc * corr[..., None]
        acc = acc + rp(p) @ vf[:, j0:j0 + block]
        m = mn
    O = (acc * (1.0 / l)[..., None]).to(torch.bfloat16)
    L2 = m + torch.log2(l)
    lse = L2 if mutant == "lse_log2" else L2 * LN2
    # backward (a kernel that stores log2 units reads them back consistently: only the stored lse is wrong)
    L2b = lse if mutant == "lse_log2" else lse * LOG2E
    if mutant == "extra_query_row":   # bwd_kv does not mask the first row past Tq: it re-reads the last staged one
        qk, dok = torch.cat([qf, qf[:, -1:]], 1), torch.cat([dof, dof[:, -1:]], 1)
    else:
        qk, dok = qf, dof
    delta = (dof * O.float()).sum(-1)
    p = torch.exp2((qf @ kf.transpose(1, 2)) * sl2 - L2b[..., None])
    dp = dof @ vf.transpose(1, 2)
    ds = p * dp if mutant == "no_delta" else p * (dp - delta[..., None])
    dQ = (_bf(ds) @ kf) * scale
    if mutant == "extra_query_row":
        p = torch.cat([p, p[:, -1:]], 1)
        ds = torch.cat([ds, ds[:, -1:]], 1)
    dK = (_bf(ds).transpose(1, 2) @ qk) * scale
    dV = rp(p).transpose(1, 2) @ dok
    if mutant == "drop_last_key":
        dK, dV = (torch.cat([t, torch.zeros(BH, 1, dh)], 1) for t in (dK, dV))
    if mutant == "swap_dk_dv":
        dK, dV = dV, dK
    return dict(O=O, lse=lse, dQ=dQ.to(torch.bfloat16), dK=dK.to(torch.bfloat16), dV=dV.to(torch.bfloat16))


# ------------------------------------------------------------------ inputs
def make_inputs(key, dist, BH, Tq, Tk, dh, positive=False):
    """Canonical bf16 q, do [BH][Tq][dh] and k, v [BH][Tk][dh] from a generator seeded by (key, dist).
    flat: q, k = randn * 0.5 (logits of order 1); peaked: randn * 3 (logit std ~ 9, P near one-hot, |lse| 30-50);
    offset: randn + 3.5 (at dh = 64 the mean logit ~ 98 > ln(FLT_MAX): no max subtraction -> overflow).
    v and dO are always randn (positive: |randn|, for check_unbiased only)."""
    g = torch.Generator().manual_seed(zlib.crc32(f"{key}/{dist}".encode()))

    def rnd(*s):
        return torch.randn(*s, generator=g)

    if dist == "flat":
        q, k = rnd(BH, Tq, dh) * 0.5, rnd(BH, Tk, dh) * 0.5
    elif dist == "peaked":
        q, k = rnd(BH, Tq, dh) * 3.0, rnd(BH, Tk, dh) * 3.0
    elif dist == "offset":
        q, k = rnd(BH, Tq, dh) + 3.5, rnd(BH, Tk, dh) + 3.5
    else:
        raise ValueError(dist)
    v, do = rnd(BH, Tk, dh), rnd(BH, Tq, dh)
    if positive:
        v, do = v.abs(), do.abs()
    return tuple(t.to(torch.bfloat16) for t in (q, k, v, do))


# ------------------------------------------------------------------ which kernel instance a shape reaches
# Mirror of dhp_of(), ks_q() and the split choices of fmd_attn_mfma_fwd / fmd_attn_mfma_bwd.  The source of
# truth is csrc/attention_mfma.hip: when a threshold moves there, move it here and re-derive the GPU cases so
# that every instance is still reached.
def dhp_of(dh):
    return 16 if dh <= 16 else (32 if dh <= 32 else 64)


def ks_q(Tq, Tk, BH):
    nwg = ((Tq + 127) // 128) * BH
    if Tk > 128 and nwg < 512:
        return 4
    return 2 if Tk > 32 else 1


def instance(BH, Tq, Tk, dh):
    """(DHP, key splits of the forward, of dQ, query splits of dK/dV, staged key blocks of the forward)."""
    D, ks = dhp_of(dh), ks_q(Tq, Tk, BH)
    return dict(dhp=D, ks_fwd=ks, ks_dq=min(2, ks) if D == 64 else ks, ks_kv=2 if Tq > 32 else 1,
                key_blocks=-(-Tk // (32 * ks)))


# ------------------------------------------------------------------ head-split maps (torch index maps)
# Reference layouts: self attention reads one fused [B][T][3*inner] projection, cross attention q [B][Tq][inner]
# and kv [B][Tk][2*inner]; o, dO are [B][Tq][inner].  raw: SpatialSelfAttention / SpatialCrossAttention reshape
# the channel-major (B, P*inner, T) buffer to (B, heads, T, P*dh) without a transpose and chunk the last dim;
# view: DiffusersAttentionND's .view(B, T, heads, dh).transpose(1, 2) of each inner-wide slice.
def split_heads(x, heads, dh, raw, parts):
    """[B][T][parts*inner] -> `parts` canonical tensors [B*heads][T][dh]."""
    B, T, _ = x.shape
    inner = heads * dh
    if raw:
        out = x.transpose(1, 2).reshape(B, heads, T, parts * dh).chunk(parts, dim=-1)
    else:
        out = [x[..., i * inner:(i + 1) * inner].reshape(B, T, heads, dh).transpose(1, 2) for i in range(parts)]
    return [t.reshape(B * heads, T, dh).contiguous() for t in out]


def join_heads(planes, B, heads, dh, raw):
    """Inverse of split_heads: canonical tensors [B*heads][T][dh] -> [B][T][len(planes)*inner]."""
    T = planes[0].shape[1]
    parts, inner = len(planes), heads * dh
    pl = [t.reshape(B, heads, T, dh) for t in planes]
    if raw:
        return torch.cat(pl, -1).reshape(B, parts * inner, T).transpose(1, 2).contiguous()
    return torch.cat([t.transpose(1, 2).reshape(B, T, inner) for t in pl], -1).contiguous()
