"""fp64 reference, per-row error bound and a torch emulation of the nearest-code search (csrc/vq.hip), shared by
test_vq_bounds.py (CPU) and test_gpu_vq.py (GPU).  Every function runs on the device of its inputs.

The kernel arithmetic the bound is derived from (see the kernel source).  For a latent vector z and a code e,
both fp32 with D elements, the kernel compares scores

    s(k) = fl32( z_h.e_h + z_h.e_l + z_l.e_h ) - hn[k],        hn[k] = fl32( 0.5 sum_d e_kd^2 ),

where x_h = bf16(x), x_l = bf16(x - x_h) (round to nearest, u = 2^-9 relative: x - x_h is exact in fp32), the
three products of every 16-element step are added to one fp32 MFMA accumulator, and hn is an fmaf chain over
d = 0 .. D-1.  The exact score is s*(k) = z.e_k - 0.5 |e_k|^2 and the squared distance is |z|^2 - 2 s*(k).
With A_k = sum_d |z_d| |e_kd|, per (row, code), in score units:

  split     x = x_h + x_l + r_x with |r_x| <= 2^-18 |x| and |x_l| <= 2^-9 (1 + 2^-9) |x|.  The products the kernel
            leaves out are z_l e_l + r_z e + (z - r_z) r_e, each at most 2^-18 (1 + 2^-8) |z| |e| per element:
                E_split = 3 * 2^-18 * (1 + 2^-8) * A_k
            (the dropped z_l.e_l product is one of the three).
  chain     bf16 x bf16 products are exact in fp32; every addition to the accumulator rounds once, by at most
            2^-24 of a partial sum that never exceeds (1 + 2^-8) A_k.  There are at most 3 D such roundings
            (padding adds exact zeros), so the worst case is 3 D * 2^-24 * (1 + 2^-8) * A_k.
            THIS TERM IS STATISTICAL, NOT A WORST CASE, for D > 12: the worst case at D = 256 (768 roundings all
            of one sign and full size) would make the whole bound 2.5 x B_loose below, which the issue forbids,
            and is not attainable in practice.  Instead the roundings are modelled as independent and zero-mean,
            for which Hoeffding gives |sum| <= 6 sqrt(3 D) single roundings with probability 1 - 3e-8 per score:
                E_chain = min(3 D, 6 sqrt(3 D)) * 2^-24 * (1 + 2^-8) * A_k
            The other three terms are worst-case bounds.
  hn        D fmaf roundings, each at most 2^-24 |e_k|^2, then the halving (exact):
                E_hn = 0.5 * D * 2^-24 * |e_k|^2
  subtract  one rounding of the difference: E_sub = 2^-24 * (A_k + 0.5 |e_k|^2)

The kernel picks c with s(c) >= s(b) for the true best b, so s*(b) - s*(c) <= E(c) + E(b) and, in distance
units, d(c) - d(b) <= 2 (E(c) + E(b)) <= 4 max_k E(k).  row_bound() evaluates that with A = max_k A_k of the
row and E2 = max_k |e_k|^2:

    bound = 4 * ( E_split + E_chain + E_hn + E_sub )(A, E2).

It is never looser than the bound the case inputs were chosen against,
    B_loose = 2 * ( 2^-15 A + 2^-24 (D + 4) (A + E2) )
(loose_bound(); test_vq_bounds.py asserts bound <= B_loose on every row of every case).  In units of 2^-24:
bound = (775 + 4.02 n) A + (2 D + 2) E2 with n = min(3 D, 6 sqrt(3 D)), B_loose = (1032 + 2 D) A + (2 D + 8) E2,
and n <= (257 + 2 D) / 4.02 for every 1 <= D <= 256.

A row is "undecided" when the fp64 gap between its best and second-best distance is <= 2 * bound; on every
other row  excess <= 1.5 * bound  forces the fp64 argmin.
"""
import json
import math
import os
import sys
import warnings
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))

MARGIN = 1.5
UNDECIDED_MAX = 0.03     # share of a case's rows whose best/second-best gap is within 2 x bound
DISTRIBUTIONS = ("randn", "offset1", "scaled", "clustered")
MUTANTS = ("single_plane", "no_hn", "hn_not_halved", "tie_highest", "drop_last_split", "pad_hn_zero",
           "skip_last_row_block")

# mirrors of csrc/vq.hip's tiling constants (plan() below is checked against fmd_vq_plan)
BM, TILE, CHUNK, KC, TARGET_WG, MAX_SPLITS, FROWS = 64, 32, 128, 64, 512, 64, 32


def plan(M, K, D):
    """Python mirror of fmd_vq_plan: dict(splits, codes_per_split, Kpad, Dpad, block_rows)."""
    nch, rb = -(-K // CHUNK), -(-M // BM)
    want = max(1, min(-(-TARGET_WG // rb), MAX_SPLITS, nch))
    cps = -(-nch // want)
    return dict(splits=-(-nch // cps), codes_per_split=cps * CHUNK, Kpad=nch * CHUNK, Dpad=-(-D // KC) * KC,
                block_rows=BM, tile_codes=TILE, finalize_rows=FROWS)


def gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()) & 0x7FFFFFFF)


def make_inputs(M, K, D, dist, tag="s6"):
    """(z [M, D], e [K, D], j or None) fp32 on the CPU, seeded by the case name; ``clustered``: z = e_j + 0.05 n,
    whose nearest code must be j.  The default seed suffix was picked among seven so that the single-plane
    mutant of the emulation is rejected on the 105 x 100 x 8 case too (105 rows hold few near ties): a choice
    made on the mutant, never on the kernel."""
    g = gen(f"vq/{M}x{K}x{D}/{dist}/{tag}")
    z = torch.randn(M, D, generator=g)
    e = torch.randn(K, D, generator=g)
    j = None
    if dist == "offset1":
        z, e = z + 1.0, e + 1.0
    elif dist == "scaled":
        z, e = 1e-2 * z, 1e-2 * e
    elif dist == "clustered":
        j = torch.randint(0, K, (M,), generator=g)
        z = e[j] + 0.05 * z
    elif dist != "randn":
        raise ValueError(dist)
    return z.contiguous(), e.contiguous(), j


# ------------------------------------------------------------------ reference and bound (fp64)
def reference(z, e, rows=512):
    """fp64 distances reduced per row: dict(dmin, idx, gap, A = max_k sum_d |z||e|, E2 = max_k |e|^2) and a
    function dist(codes) -> d64(z_i, e_codes[i])."""
    z64, e64 = z.double(), e.double()
    esq = (e64 * e64).sum(1)
    dmin, idx, gap, A = [], [], [], []
    for r0 in range(0, z64.shape[0], rows):
        zz = z64[r0:r0 + rows]
        d = (zz * zz).sum(1, keepdim=True) + esq - 2.0 * (zz @ e64.t())
        if d.shape[1] > 1:
            top = torch.topk(d, 2, dim=1, largest=False)
            gap.append(top.values[:, 1] - top.values[:, 0])
        else:
            gap.append(torch.full((d.shape[0],), math.inf, dtype=torch.float64, device=d.device))
        m = d.min(1)
        dmin.append(m.values)
        idx.append(m.indices)
        A.append((zz.abs() @ e64.abs().t()).max(1).values)

    def dist(codes):
        q = e64[codes.reshape(-1).to(e64.device)]
        return ((z64 - q) ** 2).sum(1)

    ref = dict(dmin=torch.cat(dmin), idx=torch.cat(idx), gap=torch.cat(gap), A=torch.cat(A), E2=esq.max(),
               D=z.shape[1], dist=dist)
    # the expanded form above cancels |z|^2 + |e|^2 against 2 z.e; take the minimum itself from the direct form
    ref["dmin"] = dist(ref["idx"])
    return ref


def row_bound(ref):
    """Per-row bound on d64(chosen) - min d64, distance units (module docstring)."""
    D, A, E2 = ref["D"], ref["A"], ref["E2"]
    n = min(3.0 * D, 6.0 * math.sqrt(3.0 * D))
    split = 3.0 * 2.0 ** -18 * (1 + 2.0 ** -8) * A
    chain = n * 2.0 ** -24 * (1 + 2.0 ** -8) * A
    hn = 0.5 * D * 2.0 ** -24 * E2
    sub = 2.0 ** -24 * (A + 0.5 * E2)
    return 4.0 * (split + chain + hn + sub)


def loose_bound(ref):
    D, A, E2 = ref["D"], ref["A"], ref["E2"]
    return 2.0 * (2.0 ** -15 * A + 2.0 ** -24 * (D + 4) * (A + E2))


def check(codes, ref, name, margin=MARGIN):
    """The near-minimiser assertion: codes in range, undecided rows <= 3 %, excess <= margin * bound on every
    row.  Returns dict(ratio = max excess / bound, undecided = share, agree = share equal to the fp64 argmin)."""
    codes = codes.reshape(-1)
    bound = row_bound(ref)
    assert codes.dtype == torch.int64 and codes.numel() == bound.numel(), f"{name}: codes {codes.dtype} {codes.shape}"
    und = float((ref["gap"] <= 2.0 * bound).double().mean())
    assert und <= UNDECIDED_MAX, f"{name}: {und:.4f} of the rows are undecided (gap <= 2 x bound): a vacuous case"
    excess = ref["dist"](codes) - ref["dmin"]
    ratio = excess / bound
    bad = ~(excess <= margin * bound)
    if bool(bad.any()):
        i = int(torch.where(bad, ratio, torch.zeros_like(ratio)).argmax())
        raise AssertionError(f"{name}: {int(bad.sum())} of {bad.numel()} rows further than {margin} x bound from the "
                             f"nearest code; worst row {i}: chose {int(codes[i])} (excess {float(excess[i]):.3e}), "
                             f"fp64 argmin {int(ref['idx'][i])}, bound {float(bound[i]):.3e}, "
                             f"ratio {float(ratio[i]):.2f}")
    return dict(ratio=float(ratio.max()), undecided=und,
                agree=float((codes.to(ref["idx"].device) == ref["idx"]).double().mean()))


# ------------------------------------------------------------------ emulation of the kernel arithmetic
def _bf(x):
    return x.to(torch.bfloat16).to(torch.float32)


def emulate(z, e, splits=None, codes_per_split=None, mutant=None):
    """Codes [M] int64 as csrc/vq.hip computes them, in torch fp32: two bf16 planes per operand, three products,
    fp32 hn with +inf on the padded codes, per-split first maximum, splits merged in ascending order with a
    strict >, out-of-range winners clamped as fmd_vq_finalize does.  ``mutant``: one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS, mutant
    M, D = z.shape
    K = e.shape[0]
    p = plan(M, K, D)
    S = p["splits"] if splits is None else splits
    cps = p["codes_per_split"] if codes_per_split is None else codes_per_split
    Kpad = -(-K // CHUNK) * CHUNK
    z, e = z.float(), e.float()
    ep = torch.zeros(Kpad, D, dtype=torch.float32, device=e.device)
    ep[:K] = e
    zh, eh = _bf(z), _bf(ep)
    zl, el = _bf(z - zh), _bf(ep - eh)
    hn = torch.full((Kpad,), math.inf, dtype=torch.float32, device=e.device)
    hn[:K] = 0.5 * (e * e).sum(1)
    if mutant == "hn_not_halved":
        hn[:K] = (e * e).sum(1)
    if mutant == "no_hn":
        hn[:K] = 0.0
    if mutant == "pad_hn_zero":
        hn[K:] = 0.0
    dot = zh @ eh.t()
    if mutant != "single_plane":
        dot = (zl @ eh.t() + zh @ el.t()) + dot
    score = dot - hn
    best = torch.full((M,), -math.inf, dtype=torch.float32, device=z.device)
    idx = torch.zeros(M, dtype=torch.int64, device=z.device)
    nsplit = S - 1 if mutant == "drop_last_split" else S
    for s in range(nsplit):
        blk = score[:, s * cps:min((s + 1) * cps, Kpad)]
        if blk.shape[1] == 0:
            continue
        if mutant == "tie_highest":
            v = blk.max(1).values
            i = blk.shape[1] - 1 - (blk.flip(1) == v[:, None]).double().argmax(1)
            take = v >= best
        else:
            v, i = blk.max(1)          # the first maximum: the lowest index
            take = v > best
        best = torch.where(take, v, best)
        idx = torch.where(take, i + s * cps, idx)
    idx = idx.clamp(0, K - 1)
    if mutant == "skip_last_row_block":
        idx[(M - 1) // BM * BM:] = 0   # whatever the buffer held: the tests' sentinel reads as code 0
    return idx


def quantizer_restatement(z, embedding, beta, classic, eps=1e-5):
    """The reference quantizer's forward restated in plain torch fp32 (its distance formula, first argmin,
    gather, straight-through output, mse-based loss and perplexity), for channels-first z of any spatial rank.
    Returns (z_q, vq_loss, perplexity, codes [N, *spatial])."""
    zl = z.movedim(1, -1).contiguous()
    flat = zl.reshape(-1, zl.shape[-1])
    dist = (flat ** 2).sum(1, keepdim=True) + (embedding ** 2).sum(1) - 2.0 * flat @ embedding.t()
    idx = dist.argmin(1)
    q = embedding[idx].reshape(zl.shape).movedim(-1, 1).contiguous()
    z_q = z + (q - z)
    mse = ((z_q - z) ** 2).mean()
    vq_loss = mse + beta * mse if classic else beta * mse
    p = torch.bincount(idx, minlength=embedding.shape[0]).to(z.dtype) / idx.numel()
    perplexity = torch.exp(-(p * torch.log(p + eps)).sum())
    return z_q, vq_loss, perplexity, idx.reshape(zl.shape[:-1])


def stats64(z, embedding, codes, beta, classic, eps=1e-5):
    """(vq_loss, perplexity) in fp64 for given codes [N, *spatial] and channels-last-flattened z [M, D]."""
    q = embedding.double()[codes.reshape(-1)]
    mse = ((q - z.double()) ** 2).mean()
    p = torch.bincount(codes.reshape(-1), minlength=embedding.shape[0]).double() / codes.numel()
    return float((1.0 + beta if classic else beta) * mse), float(torch.exp(-(p * torch.log(p + eps)).sum()))


# ------------------------------------------------------------------ ties
TIE_SHAPE = (96, 16384, 64)   # 64 splits of two 128-code chunks each
# (lower, higher) index of a duplicated code row: the same lane (registers 1 and 5), the two lane halves of one
# tile, two waves of one chunk, two chunks of one split, two splits, and the first against the last code
TIE_PAIRS = ((1, 9), (3, 5), (40, 100), (10, 138), (20, 5000), (0, 16383))
TIE_ROWS = 8                  # latent vectors per pair


def make_tie_inputs():
    """(z, e, expect): rows r*TIE_ROWS .. of z sit next to pair r's duplicated code, whose two copies score
    bit-identically, so the lower index must come back; row len(TIE_PAIRS)*TIE_ROWS is all zero, whose nearest
    code is the one of smallest norm; expect is -1 on the remaining (random) rows."""
    M, K, D = TIE_SHAPE
    g = gen("vq/ties")
    e = torch.randn(K, D, generator=g)
    z = torch.randn(M, D, generator=g)
    expect = torch.full((M,), -1, dtype=torch.int64)
    for r, (a, b) in enumerate(TIE_PAIRS):
        e[b] = e[a]
        rows = slice(r * TIE_ROWS, (r + 1) * TIE_ROWS)
        z[rows] = e[a] + 0.01 * z[rows]
        expect[rows] = a
    zero = len(TIE_PAIRS) * TIE_ROWS
    e[777] = 0.05 * e[777]    # the smallest norm by far
    z[zero] = 0.0
    expect[zero] = 777
    return z.contiguous(), e.contiguous(), expect


# ------------------------------------------------------------------ fixture and config-shaped settings
def load_fixture():
    """(tensors of tests/golden/vq_golden.pt, the constructor arguments)."""
    G = torch.load(os.path.join(HERE, "golden", "vq_golden.pt"), weights_only=True)
    return G, json.loads(bytes(G["cfg_json"].tolist()).decode())


def build_fixture_model(G, cfg, qt):
    """The project's VQVAE with the fixture's weights: the trunk from the name-seeded rule the generator used,
    the codebook entries from the file."""
    if os.path.join(HERE, "golden") not in sys.path:
        sys.path.insert(0, os.path.join(HERE, "golden"))
    import seeded_params as SP
    from fmdiff.models.vae import VQVAE
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = VQVAE(quantizer_type=qt, **cfg)
    state = SP.seeded_params(((k, tuple(p.shape)) for k, p in m.named_parameters() if not k.startswith("codebook.")),
                             int(G["seed"]))
    state.update({k[len(qt) + 1:]: v for k, v in G.items() if k.startswith(f"{qt}.codebook.")})
    m.load_state_dict(state, strict=True)
    return m.eval(), state


# the model blocks of configs/LDCT/LDCT_vqvae.json and configs/MNIST/mnist_vqvae_original.json (settings only)
LDCT_VQ = {"in_channels": 1, "out_channels": 1, "resolution": 256, "base_ch": 32, "down_channels": [32, 64, 128, 256],
           "num_res_blocks": 2, "attn_resolutions": [], "z_channels": 256, "embed_dim": 256, "dropout": 0.0,
           "use_attention": False, "spatial_dims": 2, "emb_channels": None, "use_scale_shift_norm": False,
           "attn_heads": 1, "attn_dim_head": 64, "latent_type": "vq", "codebook_size": 16384, "vq_beta": 0.25,
           "vq_ema_decay": 0.99, "vq_ema_eps": 1e-05, "norm_type": "gn", "act": "silu", "ckpt_path": None,
           "model_type": "vae", "quantizer_type": "ema", "discriminator_type": "patchgan"}
MNIST_VQ = {"in_channels": 1, "out_channels": 1, "resolution": 32, "base_ch": 64, "down_channels": [64, 128, 256],
            "num_res_blocks": 2, "attn_resolutions": [], "z_channels": 64, "embed_dim": 64, "dropout": 0.0,
            "use_attention": False, "spatial_dims": 2, "emb_channels": "None", "use_scale_shift_norm": False,
            "attn_heads": 4, "attn_dim_head": 64, "latent_type": "vq", "codebook_size": 512, "vq_beta": 0.25,
            "norm_type": "gn", "act": "silu", "ckpt_path": "None", "model_type": "vae", "quantizer_type": "classic",
            "discriminator_type": "patchgan"}
