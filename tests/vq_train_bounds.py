"""fp64 restatement, per-element error bounds and a torch fp32 emulation of the quantizer's training kernels
(csrc/vq_train.hip), shared by test_vq_train_bounds.py (CPU) and test_gpu_vq_train.py (GPU).  Every function
runs on the device of its inputs.  DESIGN.md section 4 ("Quantizer training") carries the same derivation.

Given the codes, with n_k the count and S_kd the sum over the rows of code k (first D channels only),
g = decay, u = 2^-24, K codes, M rows:

    cs'_k = g cs_k + (1 - g) n_k                 w'_kd = g w_kd + (1 - g) S_kd
    n     = sum_k cs'_k                          cl_k  = (cs'_k + eps) / (n + K eps) * n
    e'_kd = w'_kd / cl_k                         dz_md = g_zq_md + g_loss c 2/(MD) (z_md - q_md)

Every bound is c u (sum of the magnitudes of the terms), c = the fp32 roundings on the path as the kernel is
written, plus one:

  cs'   roundings: g -> fp32, (1 - g) -> fp32, the product g cs, the fma.  c = 5:
            B_cs = 5 u (g |cs| + (1 - g) n_k)
  w'    the same four and the rounding of the fp64 segment sum to fp32 (the fp64 additions themselves err by
        2^-53 per row, far below first order in u).  c = 6:
            B_w = 6 u (g |w| + (1 - g) sum_{m in k} |z_md|)
  n     an fp64 sum of the fp32 cs' (exact to first order in u), rounded to fp32 once:
            B_n = sum_k B_cs + u n
  e'    through the quotient.  The same fp32 n enters numerator and denominator of cl, so its error moves cl
        by (K eps / (n + K eps)) B_n / n only; the other roundings are eps -> fp32 and the sum cs' + eps, K eps ->
        fp32 and the sum n + K eps, the division, the product and the final division:
            R_cl = (B_cs + u eps + u (cs' + eps)) / (cs' + eps) + (K eps / (n + K eps)) B_n / n
                   + u (K eps + n + K eps) / (n + K eps) + 2 u
            B_e  = B_w / cl + |e'| (R_cl + u)
  dz    roundings: c -> fp32, 2/(MD) -> fp32, g_loss c, that times 2/(MD), z - q, the fma.  c = 7:
            B_dz = 7 u (|g_zq| + |coef| (|z| + |q|)),   coef = g_loss c 2/(MD)
  dE    (opt-in codebook gradient coef2 (n_k e - S), coef2 = g_loss 2/(MD)): 2/(MD) -> fp32, g_loss times it, the
        segment sum, the fma, the product.  c = 6:
            B_dE = 6 u |coef2| (n_k |e| + sum_{m in k} |z_md|)

Against the reference's recorded fp32 results the reference's own error is added, in the same form
(``reference=True``): five roundings on cs' and w' (g and 1 - g to fp32, two products, one sum), its segment sum
an fp32 matmul over M terms of which n_k are not zero, (n_k + 2) u sum |z|, its n an fp32 sum of K terms,
K u n, and the same quotient; its autograd dz sums the commitment and codebook terms separately, so
|coef| is g_loss (1 + beta) 2/(MD) for the classic quantizer, again with c = 7.
"""
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
U = 2.0 ** -24
C_CS, C_W, C_DZ, C_DE = 5, 6, 7, 6
MUTANTS = ("unused_not_decayed", "zq_from_updated", "loss_from_updated", "classic_beta", "no_eps", "n_before",
           "drop_row", "pad_read")


# ------------------------------------------------------------------ fp64 restatement
def segment_sums64(z, codes, K):
    """(n_k [K], S [K, D], A = sum |z| [K, D]) in fp64 for z [M, D] and codes [M]."""
    z64, codes = z.double(), codes.reshape(-1)
    S = torch.zeros(K, z.shape[1], dtype=torch.float64, device=z.device).index_add_(0, codes, z64)
    A = torch.zeros_like(S).index_add_(0, codes, z64.abs())
    return torch.bincount(codes, minlength=K).double(), S, A


def update64(z, codes, cs, w, decay, eps):
    """The EMA update in fp64: dict(cs, w, n, cl, e) after the step and (n_k, S, A) of the segments."""
    K = w.shape[0]
    n_k, S, A = segment_sums64(z, codes, K)
    cs2 = decay * cs.double() + (1.0 - decay) * n_k
    w2 = decay * w.double() + (1.0 - decay) * S
    n = cs2.sum()
    cl = (cs2 + eps) / (n + K * eps) * n
    return dict(cs=cs2, w=w2, n=n, cl=cl, e=w2 / cl[:, None], n_k=n_k, S=S, A=A)


def update_bounds(r, cs, w, decay, eps, reference=False):
    """Per-element bounds dict(cs, w, n, e) of the kernel against ``r = update64(...)`` (module docstring);
    ``reference``: the bounds of the reference's own fp32 evaluation instead."""
    K = w.shape[0]
    mag_cs = decay * cs.double().abs() + (1.0 - decay) * r["n_k"]
    mag_w = decay * w.double().abs() + (1.0 - decay) * r["A"]
    if reference:
        b_cs = 5 * U * mag_cs
        b_w = 5 * U * mag_w + (1.0 - decay) * (r["n_k"][:, None] + 2.0) * U * r["A"]
        b_n = b_cs.sum() + K * U * r["n"]
    else:
        b_cs = C_CS * U * mag_cs
        b_w = C_W * U * mag_w
        b_n = b_cs.sum() + U * r["n"]
    n, keps, cse = r["n"], K * eps, r["cs"] + eps
    r_cl = (b_cs + U * eps + U * cse) / cse + (keps / (n + keps)) * b_n / n + U * (keps + n + keps) / (n + keps) + 2 * U
    b_e = b_w / r["cl"][:, None] + r["e"].abs() * (r_cl[:, None] + U)
    return dict(cs=b_cs, w=b_w, n=b_n, e=b_e)


def dz64(z, q, g_zq, g_loss, c):
    """g_zq + g_loss c 2/(MD) (z - q) in fp64 for [M, D] operands (g_zq None: zero)."""
    M, D = z.shape
    out = float(g_loss) * c * 2.0 / (M * D) * (z.double() - q.double())
    return out if g_zq is None else out + g_zq.double()


def dz_bound(z, q, g_zq, coef_mag, cc=C_DZ):
    g = 0.0 if g_zq is None else g_zq.double().abs()
    return cc * U * (g + coef_mag * (z.double().abs() + q.double().abs()))


def codebook_grad64(z, codes, e, g_loss):
    """(dE, bound): the codebook term g_loss 2/(MD) (n_k e_k - S_k) and B_dE."""
    M, D = z.shape
    n_k, S, A = segment_sums64(z, codes, e.shape[0])
    coef = float(g_loss) * 2.0 / (M * D)
    return coef * (n_k[:, None] * e.double() - S), C_DE * U * abs(coef) * (n_k[:, None] * e.double().abs() + A)


def check(name, got, want, bound, what):
    """Asserts |got - want| <= bound on every element (NaN fails); returns the largest error / bound."""
    err = (got.double() - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64, device=err.device)
    ok = err <= bound
    if not bool(ok.all()):
        worst = float(torch.nan_to_num(err / bound.clamp_min(1e-300), nan=float("inf"))[~ok].max())
        raise AssertionError(f"{name}: {what}: {int((~ok).sum())} of {ok.numel()} elements outside the bound "
                             f"(largest error / bound {worst:.3g})")
    return float((err / bound.clamp_min(1e-300)).max())


def check_update(name, got, r, b):
    """``got``: dict(cs, w, e, n) of fp32 results (n fp64 or fp32).  Returns the ratios per output."""
    return {k: check(name, got[k].reshape(r[k].shape), r[k], b[k], k) for k in ("cs", "w", "n", "e")}


# ------------------------------------------------------------------ emulation of the kernels' arithmetic
def _f32(v, dev):
    return torch.tensor(float(v), dtype=torch.float32, device=dev)


def _fma(a, b, c):
    return (a.double() * b.double() + c.double()).float()


def emulate(z_pad, D, codes, emb, cs, w, decay, eps, beta, classic, g_zq, g_loss, mutant=None):
    """One training step as csrc/vq.hip + csrc/vq_train.hip compute it, in torch fp32 on rows ``z_pad`` [M, ldz]
    whose padding channels may hold NaN: dict(zq, vq_loss, cs, w, n, e, dz).  ``mutant``: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS, mutant
    dev = z_pad.device
    M, K = z_pad.shape[0], emb.shape[0]
    z = z_pad[:, :D]
    gam, omg = _f32(decay, dev), _f32(1 - decay, dev)
    rows = torch.arange(M, device=dev)
    if mutant == "drop_row":
        rows = rows[1:]
    zs = z[rows].double()
    if mutant == "pad_read":
        zs = zs.clone()
        zs[:, D - 1] += z_pad[rows, D].double()
    S = torch.zeros(K, D, dtype=torch.float64, device=dev).index_add_(0, codes[rows], zs).float()
    n_k = torch.bincount(codes, minlength=K).float()
    cs2 = _fma(omg, n_k, gam * cs)
    w2 = _fma(omg, S, gam * w)
    if mutant == "unused_not_decayed":
        cs2 = torch.where(n_k > 0, cs2, cs)
        w2 = torch.where(n_k[:, None] > 0, w2, w)
    n = (cs if mutant == "n_before" else cs2).double().sum()
    nf = n.float()
    cl = ((cs2 + _f32(eps, dev)) / (nf + _f32(K * eps, dev))) * nf
    if mutant == "no_eps":
        cl = cs2
    e2 = w2 / cl[:, None]
    q = emb[codes]
    qz = e2[codes] if mutant == "zq_from_updated" else q
    ql = e2[codes] if mutant == "loss_from_updated" else q
    zq = z + (qz - z)
    mse = ((ql.double() - z.double()) ** 2).mean()
    vq_loss = ((1.0 + beta if classic else beta) * mse).float()
    c = beta if mutant == "classic_beta" or not classic else beta - 1.0
    coef = (_f32(g_loss, dev) * _f32(c, dev)) * _f32(2.0 / (M * D), dev)
    dz = _fma(coef, z - q, torch.zeros_like(z) if g_zq is None else g_zq)
    return dict(zq=zq, vq_loss=vq_loss, cs=cs2, w=w2, n=n, e=e2, dz=dz)


def check_step(name, got, z, codes, emb, cs, w, decay, eps, beta, classic, g_zq, g_loss):
    """Every assertion on one step's results ``got`` (keys of ``emulate``) against fp64; returns the ratios."""
    r = update64(z, codes, cs, w, decay, eps)
    ratios = check_update(name, got, r, update_bounds(r, cs, w, decay, eps))
    q = emb[codes]
    # z + (q - z): two roundings
    ratios["zq"] = check(name, got["zq"], z.double() + (q.double() - z.double()), 3 * U * (z.double().abs() + q.double().abs()),
                         "zq")
    mse = ((q.double() - z.double()) ** 2).mean()
    loss64 = (1.0 + beta if classic else beta) * mse
    ratios["vq_loss"] = check(name, got["vq_loss"], loss64, 1e-5 * loss64.abs(), "vq_loss")
    c = beta - 1.0 if classic else beta
    coef = abs(float(g_loss) * c * 2.0 / z.numel())
    ratios["dz"] = check(name, got["dz"], dz64(z, q, g_zq, g_loss, c), dz_bound(z, q, g_zq, coef), "dz")
    return ratios


# ------------------------------------------------------------------ inputs
def make_state(K, D, tag, sizes="rand"):
    """(embedding, ema_cluster_size, ema_w) fp32 on the CPU: a seeded normal codebook, sizes ``ones`` / ``rand``
    (0.05 + 4 rand) / ``dead`` (rand with a third of the entries exactly 0), ema_w = embedding * size as a run of
    updates leaves it (so the next embedding keeps its scale), except on dead entries, where it is the embedding."""
    import vq_bounds as vb
    g = vb.gen(f"vq_train_state/{K}x{D}/{tag}/{sizes}")
    emb = torch.randn(K, D, generator=g)
    if sizes == "ones":
        cs = torch.ones(K)
    else:
        cs = 0.05 + 4.0 * torch.rand(K, generator=g)
        if sizes == "dead":
            cs[torch.rand(K, generator=g) < 1.0 / 3.0] = 0.0
    w = torch.where(cs[:, None] > 0, emb * cs[:, None], emb)
    return emb.contiguous(), cs.contiguous(), w.contiguous()


def load_fixture():
    """The tensors of tests/golden/vq_train_golden.pt and vq_train_golden_b.pt, and dict(beta, decay, eps, g_loss)."""
    G = {}
    for name in ("vq_train_golden.pt", "vq_train_golden_b.pt"):
        G.update(torch.load(os.path.join(HERE, "golden", name), weights_only=True))
    for tag in ("a", "b"):
        G[f"{tag}.state0.ema_w"] = G[f"{tag}.state0.embedding"]
    beta, decay, eps, g_loss = G["hyper"].tolist()
    return G, dict(beta=beta, decay=decay, eps=eps, g_loss=g_loss)


FIXTURE_SHAPES = {"a": (3, (5, 7), 100, 8), "b": (2, (8, 8), 512, 64)}
FIXTURE_STEPS = 4


def fixture_state(G, tag, s):
    return tuple(G[f"{tag}.state{s}.{k}"] for k in ("embedding", "ema_cluster_size", "ema_w"))


def flat(z):
    """[N, D, *spatial] -> [M, D] rows in the quantizer's order."""
    zl = z.movedim(1, -1)
    return zl.reshape(-1, zl.shape[-1])
