"""Tensor-level launchers over the C ABI (device memory from PyTorch's allocator).

Every function launches on the current HIP stream and returns new device
tensors; none of them synchronises, so the whole train / sample step can be
captured into a hipGraph.  Activations are NHWC bf16 ``[N, H, W, C]``.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from .. import _lib
from . import tuning, wgrad_plan
from .._lib import ConvDesc, GnApplyDesc, GnOutDesc, SkipBwdDesc, SkipBwdPlan, WgradDesc

BF16 = torch.bfloat16
F32 = torch.float32
NUM_CU = 256


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _need_cuda(t: torch.Tensor, what: str):
    if t.device.type != "cuda":
        raise RuntimeError(f"{what}: fmdiff HIP kernels need ROCm device tensors (got {t.device}); "
                           "there is no CPU path")


@dataclass
class Stats:
    """Per-channel partial sums of an activation: slab [N*HW/rows][C][2] (sum, sum of squares)."""
    slab: torch.Tensor
    rows: int


def channel_stats(x: torch.Tensor, rows: Optional[int] = None, y: Tuple = None) -> Stats:
    """(sum x, sum x^2) per (n, channel, row-block), or (sum x, sum x*y) when ``y=(y0, y1, C0)`` is given."""
    N, Cc = x.shape[0], x.shape[-1]
    HW = x[0, ..., 0].numel()   # pixels per image (H*W, or D*H*W for NDHWC)
    if rows is None:
        # 64-pixel slab rows (like the conv epilogues): enough blocks to cover the chip even at 32x32
        rows = 64 if HW % 64 == 0 else HW
    slab = torch.empty((N * HW // rows, Cc, 2), device=x.device, dtype=F32)
    y0, y1, C0 = (None, None, Cc) if y is None else y
    _lib.call("fmd_channel_stats", _p(x), _p(y0), _p(y1), C0, N, HW, Cc, rows, _p(slab), stream())
    return Stats(slab, rows)


# slabs with at least STATS_FOLD_MIN rows per image are folded STATS_FOLD rows at a time before the GroupNorm
# (n, group) reductions (fmd_stats_fold): config E's 128^3 levels (32768 rows of 64 pixels)
STATS_FOLD_MIN = tuning.get("STATS_FOLD_MIN")
STATS_FOLD = 128


def fold_stats(st: Optional[Stats], HW: int) -> Optional[Stats]:
    """``st`` with STATS_FOLD consecutive slab rows summed (same per-image sums), or ``st`` itself when small."""
    if st is None or not STATS_FOLD_MIN:
        return st
    E = HW // st.rows
    C = st.slab.shape[1]
    if E < STATS_FOLD_MIN or E % STATS_FOLD or C % 2 or not st.slab.is_contiguous():
        return st
    rows_total = st.slab.shape[0]
    out = torch.empty((rows_total // STATS_FOLD, C, 2), device=st.slab.device, dtype=F32)
    _lib.call("fmd_stats_fold", _p(st.slab), rows_total, C, STATS_FOLD, _p(out), stream())
    return Stats(out, st.rows * STATS_FOLD)


def gn_prep(st0: Stats, st1: Optional[Stats], N: int, HW: int, C0: int, C1: int, groups: int, eps: float,
            gamma, beta, emb=None, emb_stride=0, emb_mode=0):
    """Fold GroupNorm (+ scale/shift) into a[n][c], b[n][c]; returns (a, b, mean_rstd)."""
    st0, st1 = fold_stats(st0, HW), fold_stats(st1, HW)
    dev = st0.slab.device
    Ct = C0 + C1
    a = torch.empty((N, Ct), device=dev, dtype=F32)
    b = torch.empty((N, Ct), device=dev, dtype=F32)
    mr = torch.empty((N, groups, 2), device=dev, dtype=F32)
    _lib.call("fmd_gn_prep", _p(st0.slab), st0.rows, _p(st1.slab) if st1 else None, st1.rows if st1 else 1,
              N, HW, C0, C1, groups, float(eps), _p(gamma), _p(beta), _p(emb), emb_stride, emb_mode,
              _p(a), _p(b), _p(mr), stream())
    return a, b, mr


# deferred gamma/beta gradient folds (gb_defer / gb_flush): (ws, N, C, dgamma, dbeta) per GroupNorm backward
_gb_pending: Optional[list] = None


def gb_defer():
    """Start collecting gn_bwd_prep's gamma/beta folds; gb_flush() applies them in batched launches."""
    global _gb_pending
    _gb_pending = []


def gb_flush():
    """Fold every deferred (dgamma, dbeta) contribution (fmd_gn_gb_fold, <= GB_MAX jobs per launch) and stop
    deferring.  Same sums in the same order as the per-call fold."""
    global _gb_pending
    jobs, _gb_pending = _gb_pending or [], None
    for i in range(0, len(jobs), _lib.GB_MAX):
        part = jobs[i:i + _lib.GB_MAX]
        arr = (_lib.GbJob * len(part))()
        for k, (ws, N, Cc, dg, dbt) in enumerate(part):
            arr[k].ws, arr[k].dgamma, arr[k].dbeta, arr[k].N, arr[k].C = _p(ws), _p(dg), _p(dbt), N, Cc
        _lib.call("fmd_gn_gb_fold", arr, len(part), stream())


def gn_bwd_prep(s12: Stats, N: int, HW: int, Ct: int, groups: int, mr, gamma, beta, dgamma, dbeta,
                emb=None, emb_stride=0, emb_mode=0, demb=None, demb_stride=0, fwd: Optional[Stats] = None):
    s12, fwd = fold_stats(s12, HW), fold_stats(fwd, HW)
    dev = s12.slab.device
    P = torch.empty((N, Ct), device=dev, dtype=F32)
    Q = torch.empty((N, Ct), device=dev, dtype=F32)
    R = torch.empty((N, Ct), device=dev, dtype=F32)
    ws = torch.empty((N, Ct, 2), device=dev, dtype=F32)
    if _gb_pending is not None and (dgamma is not None or dbeta is not None):
        _gb_pending.append((ws, N, Ct, dgamma, dbeta))   # ws stays referenced until the fold is issued
        dgamma = dbeta = None
    _lib.call("fmd_gn_bwd_prep", _p(s12.slab), s12.rows, N, HW, Ct, groups, _p(mr), _p(gamma), _p(beta), _p(emb),
              emb_stride, emb_mode, _p(P), _p(Q), _p(R), _p(dgamma), _p(dbeta), _p(demb), demb_stride,
              _p(fwd.slab) if fwd else None, fwd.rows if fwd else 1, _p(ws), stream())
    return P, Q, R


def gn_apply_fwd(x0, x1, a, b, silu=True):
    """t = SiLU(a*x + b) over the channel concat of x0|x1 (NHWC bf16): the materialised GN prologue."""
    N, C0 = x0.shape[0], x0.shape[-1]
    HW = x0[0, ..., 0].numel()                    # any spatial rank (N, *sp, C)
    C1 = x1.shape[-1] if x1 is not None else 0
    t = torch.empty((*x0.shape[:-1], C0 + C1), device=x0.device, dtype=BF16)
    _lib.call("fmd_gn_apply_fwd", _p(x0), _p(x1), C0, C1, N * HW, HW, _p(a), _p(b), int(silu), _p(t), stream())
    return t


GN_FUSED_MAX = 16384   # elements per (n, group) that fmd_gn_fused_apply holds in one workgroup's registers
GN_FUSED = bool(tuning.get("GN_FUSED"))   # A/B switch (0: slab statistics + gn_prep + apply)


def gn_fused_eligible(HW: int, C: int, C0: int, groups: int) -> bool:
    """Mirror of fmd_gn_fused_apply's applicability test (csrc/groupnorm.hip)."""
    Cg = C // groups if C % groups == 0 else 0
    return GN_FUSED and Cg > 0 and Cg % 4 == 0 and C0 % 4 == 0 and 256 % (Cg // 4) == 0 and HW * Cg <= GN_FUSED_MAX


# the GroupNorm forward of a split-K conv's output inside its combine (fmd_conv_gn); CONV_GN=0 (runtime/tuning.py): the separate
# fmd_gn_fused_apply launch (A/B runs)
CONV_GN = bool(tuning.get("CONV_GN"))
# fewest combine blocks (images x channel blocks) for which the fused form beats the two launches it replaces
# (latent step profile: 64 blocks 13.1 us vs 5-7 + 5.2 us; 128 blocks 8.0 us, 256 blocks 7.2 us)
CONV_GN_MIN_BLOCKS = tuning.get("CONV_GN_MIN_BLOCKS")
CONV_GN_CB = tuning.get("CONV_GN_CB")   # fewest channels per combine block (fmd_conv_gn; _lib sets the library's)
if CONV_GN_CB not in (4, 8, 16, 32, 64):
    raise ValueError(f"CONV_GN_CB must be 4, 8, 16, 32 or 64, not {CONV_GN_CB}")


def conv_gn_eligible(K: int, groups: int, N: int = 1 << 30) -> bool:
    """Mirror of fmd_conv_gn's channel test (whole groups per block of max(CONV_GN_CB, K/groups) <= 64 channels,
    CONV_GN_CB from runtime/tuning.py, default 4) plus the block-count floor."""
    if K % 64 or K % groups or 64 % (K // groups):
        return False
    return N * (K // max(CONV_GN_CB, K // groups)) >= CONV_GN_MIN_BLOCKS


def gn_fused_apply(x0, x1, groups: int, eps: float, gamma, beta, emb=None, emb_stride=0, emb_mode=0, silu=True):
    """GroupNorm of x0|x1 from the activations themselves (no statistics slab): returns (a, b, mean_rstd, t)
    with t = SiLU(a*x + b) materialised -- channel_stats + gn_prep + gn_apply_fwd in one launch."""
    N, C0 = x0.shape[0], x0.shape[-1]
    HW = x0[0, ..., 0].numel()
    C1 = x1.shape[-1] if x1 is not None else 0
    Ct = C0 + C1
    dev = x0.device
    a = torch.empty((N, Ct), device=dev, dtype=F32)
    b = torch.empty((N, Ct), device=dev, dtype=F32)
    mr = torch.empty((N, groups, 2), device=dev, dtype=F32)
    t = torch.empty((*x0.shape[:-1], Ct), device=dev, dtype=BF16)
    _lib.call("fmd_gn_fused_apply", _p(x0), _p(x1), C0, C1, N, HW, groups, float(eps), _p(gamma), _p(beta), _p(emb),
              emb_stride, emb_mode, int(silu), _p(a), _p(b), _p(mr), _p(t), stream())
    return a, b, mr, t


def dropout_apply(x, p: float, seed: torch.Tensor, salt: int, ep=None, out=None):
    """y = x * keep / (1 - p) over NHWC bf16 ``x``, keep regenerated from (seed[0], salt, element index)
    (fmd_dropout_apply); ``ep=(h, a, b)``: the backward through the dropout and the GN+SiLU prologue,
    y = x * keep / (1 - p) * silu'(a * h + b).  ``out`` may be ``x`` (in place)."""
    _need_cuda(x, "dropout")
    N, Cc = x.shape[0], x.shape[-1]
    HW = x[0, ..., 0].numel()
    y = torch.empty_like(x) if out is None else out
    h, a, b = ep if ep is not None else (None, None, None)
    _lib.call("fmd_dropout_apply", _p(x), Cc, N * HW, HW, float(p), _p(seed), int(salt) & 0xffffffff, _p(h), _p(a),
              _p(b), _p(y), stream())
    return y


def gn_bwd_apply(dz, x0, x1, P, Q, R, extra, dx0, acc0, dx1=None, acc1=0):
    N = dz.shape[0]
    HW = dz[0, ..., 0].numel()                    # any spatial rank (N, *sp, C)
    C0 = x0.shape[-1]
    C1 = x1.shape[-1] if x1 is not None else 0
    _lib.call("fmd_gn_bwd_apply", _p(dz), _p(x0), _p(x1), C0, C1, N * HW, HW, _p(P), _p(Q), _p(R),
              _p(extra), _p(dx0), int(acc0), _p(dx1), int(acc1), stream())


def conv1x1_gn_apply(dy, wgt_t, dz, x0, x1, P, Q, R, dx0, acc0, dx1=None, acc1=0):
    """dx = dy @ W^T (1x1 data gradient, ``wgt_t`` = mode-1 weights [C][1][K]) + P*dz + Q*x + R (+ dx):
    the ResBlock skip-conv data gradient fused into the block input's GroupNorm backward
    (fmd_conv_gn_apply; == conv(..., transposed=True) followed by gn_bwd_apply(extra=...))."""
    _need_cuda(dy, "conv1x1_gn_apply")
    N, Kd = dy.shape[0], dy.shape[-1]
    W = dy.shape[-2]
    H = dy[0, ..., 0, 0].numel()                  # pointwise: a (D, H, W) volume runs as a (D*H, W) plane
    Ct = dz.shape[-1]
    d = ConvDesc()
    d.N, d.Hs, d.Ws, d.C0, d.C1, d.Ho, d.Wo, d.K = N, H, W, Kd, 0, H, W, Ct
    d.ks, d.stride, d.pad, d.upsample, d.transposed = 1, 1, 0, 0, 1
    d.src0, d.wgt, d.splits = _p(dy), _p(wgt_t), 1
    g = GnApplyDesc()
    g.dz, g.x0, g.x1, g.C0 = _p(dz), _p(x0), _p(x1), x0.shape[-1]
    g.P, g.Q, g.R = _p(P), _p(Q), _p(R)
    g.dx0, g.acc0, g.dx1, g.acc1 = _p(dx0), int(acc0), _p(dx1), int(acc1)
    _lib.call("fmd_conv_gn_apply", C.byref(d), C.byref(g), stream())


def out_hw(Hs, ks, stride, pad, upsample):
    Hin = Hs * (2 if upsample else 1)
    return (Hin + 2 * pad - ks) // stride + 1


# split-K of the generic implicit GEMM on small grids: >= SPLIT_MIN_STEPS k-steps per split, about
# SPLIT_CU_MULT workgroups per CU, at most SPLIT_CAP splits (env overrides for A/B measurements)
SPLIT_MIN_STEPS = tuning.get("SPLIT_MIN_STEPS")
SPLIT_CU_MULT = tuning.get("SPLIT_CU_MULT")
SPLIT_CAP = tuning.get("SPLIT_CAP")
# outputs of at most BPX64_M pixels (K > 64, split-K) run on 64-pixel tiles (csrc/conv.hip small_m)
# (train step 24.94 / 25.03 -> 24.83 / 24.87 ms, config D batch 8 77 -> 82.6 images/s); at most BPX32_M: 32-pixel
# tiles (the latent UNet's 4x4 .. 1x1 levels: 82.3 -> 83.1 images/s)
BPX64_M = 2048
BPX32_M = 128


def igemm_split_tile(K, M):
    """(bco, bpx): output channels x pixels of the implicit-GEMM tile a problem runs on IF it runs split-K (the 64- /
    32-pixel tiles exist only for splits > 1) -- what :func:`_choose_splits` counts workgroups with, before the
    split count the plan needs is known.  tests/test_conv_plan.py holds it to fmd_conv_plan's answer."""
    if K <= 16:
        return 16, 256
    if K <= 64:
        return 64, 128
    return 128, (128 if M > BPX64_M else 32 if M <= BPX32_M else 64)


def _choose_splits(M, K, nk, bpx=128, bco=128):
    tiles = -(-M // bpx) * -(-K // bco)
    if tiles >= NUM_CU or nk < 8:
        return 1
    return max(1, min(nk // SPLIT_MIN_STEPS, -(-SPLIT_CU_MULT * NUM_CU // tiles), SPLIT_CAP))


HALO_CMAX = 512   # widest GN-prologue input of the halo kernel's affine table (csrc/conv_halo.hip CMAX)
HALO_BK = 32      # input channels per halo chunk (FMD_HALO_BK)
SPLIT_STATS_ROWS = 16   # pixels per statistics row of a split-K conv (FMD_SPLIT_STATS_ROWS)


# halo split-K on the small levels: ~HALO_SPLIT_WG workgroups, >= HALO_MIN_CHUNKS 32-channel chunks per split,
# <= HALO_SPLIT_CAP splits (env overrides for A/B runs)
HALO_SPLIT_WG = tuning.get("HALO_SPLIT_WG")
# forward-only GroupNorm folded in the halo conv's prologue from the statistics slabs (fmd_conv_desc.fold_*) where
# the slab has at most HALO_FOLD_MAX_ROWS rows per image (runtime/tuning.py)
HALO_FOLD = bool(tuning.get("HALO_FOLD"))
HALO_FOLD_MAX_ROWS = tuning.get("HALO_FOLD_MAX_ROWS")
# split-K halo convs (2-D) combine their parts inside the launch (fmd_conv_desc.tickets; statistics from the conv
# epilogue with 64-pixel rows) instead of the splitk_reduce_rows launch
HALO_TICKET = bool(tuning.get("HALO_TICKET"))
SPLIT_TICKET = bool(tuning.get("SPLIT_TICKET"))   # the implicit GEMM's split-K likewise (whole tiles)
HALO_MIN_CHUNKS = tuning.get("HALO_MIN_CHUNKS")
HALO_SPLIT_CAP = tuning.get("HALO_SPLIT_CAP")
# fewest halo workgroups (tiles x splits); mirrors fmd_halo_set_min_workgroups (tuning HALO_MIN_WG, applied at _lib load)
HALO_MIN_WG = tuning.get("HALO_MIN_WG")


def halo_splits(N, Ho, Wo, K, Cin, ztaps=1) -> int:
    """Split-K factor the halo kernel uses: 1 when the 16x16 tiles x cout tiles already give >= 128
    workgroups, else enough chunk-range splits (>= 2 chunks each) to reach ~256; 0 = not eligible
    (fewer than HALO_MIN_WG workgroups)."""
    nwg = N * (Ho // 16) * (Wo // 16) * -(-K // 128)
    if nwg >= max(128, HALO_MIN_WG):   # the kernel's own threshold (fmd_halo_set_min_workgroups) may be higher
        return 1
    nch = -(-max(Cin, 1) // HALO_BK) * ztaps
    sp = min(-(-HALO_SPLIT_WG // max(nwg, 1)), nch // HALO_MIN_CHUNKS, HALO_SPLIT_CAP)
    if sp < 2 and nwg >= HALO_MIN_WG:
        return 1
    if sp < 2 or nwg * sp < HALO_MIN_WG:
        return 0
    cps = -(-nch // sp)
    while sp > 1 and (sp - 1) * cps >= nch:   # every split owns at least one chunk (mirrors the kernel)
        sp -= 1
    return sp if nwg * sp >= HALO_MIN_WG else 0


def halo_eligible(N, Hs, Ho, Wo, K, ks=3, stride=1, pad=1, upsample=False, transposed=False, Cin=0,
                  pro=False, ztaps=1) -> bool:
    """Mirror of fmd_conv_halo's applicability test (csrc/conv_halo.hip): 3x3 s1 p1 forward gather,
    16x16 output tiles, K > 16, at least HALO_MIN_WG (default 32) workgroups (with split-K over channel chunks
    when the level is small), GN-prologue inputs of at most HALO_CMAX channels."""
    Ws = Wo // 2 if upsample else Wo
    return (K > 16 and ks == 3 and stride == 1 and pad == 1 and not transposed and not (pro and Cin > HALO_CMAX)
            and Ho % 16 == 0 and Wo % 16 == 0 and (Ho == 2 * Hs if upsample else Ho == Hs)
            and N * Hs * Ws * max(Cin, 1) < (1 << 31)   # the kernel's 32-bit element offsets (conv_halo.hip)
            and halo_splits(N, Ho, Wo, K, Cin, ztaps) > 0)


def s2d_eligible(N, Hs, Ws, Ho, Wo, K, C, ks, Ds=0, Do=0) -> bool:
    """Mirror of fmd_conv_s2d's applicability test (csrc/conv_halo9.hip): a stride-2 pad-1 3x3 / 4x4 forward
    gather onto 16x16 output tiles, C % 32 == 0, K % 128 == 0, >= 128 workgroups.  3-D: ``Ds`` = 2 ``Do`` input /
    output depths (stride 2 in depth too; the depth taps run as chunks)."""
    d3 = Ds > 0 or Do > 0
    if d3 and Ds != 2 * Do:
        return False
    Ni, No = N * (Ds if d3 else 1), N * (Do if d3 else 1)
    return (ks in (3, 4) and Hs == 2 * Ho and Ws == 2 * Wo and Ho % 16 == 0 and Wo % 16 == 0 and C % 32 == 0
            and K % 128 == 0 and No * (Ho // 16) * (Wo // 16) * (K // 128) >= 128
            and Ni * Hs * Ws * C < (1 << 31) and No * Ho * Wo * K < (1 << 31))


def d2s_eligible(N, Hs, Ws, Ho, Wo, K, C, Ds=0, Do=0) -> bool:
    """Mirror of fmd_conv_d2s's applicability test: the transposed gather of a stride-2 pad-1 3x3 conv from an
    Hs x Ws gradient (multiples of 16) onto Ho = 2 Hs, Wo = 2 Ws, C % 32 == 0, K % 128 == 0, >= 128 workgroups.
    3-D: ``Do`` = 2 ``Ds`` (8 output classes per tile)."""
    d3 = Ds > 0 or Do > 0
    if d3 and Do != 2 * Ds:
        return False
    Ni, No = N * (Ds if d3 else 1), N * (Do if d3 else 1)
    return (Ho == 2 * Hs and Wo == 2 * Ws and Hs % 16 == 0 and Ws % 16 == 0 and C % 32 == 0 and K % 128 == 0
            and Ni * (Hs // 16) * (Ws // 16) * (8 if d3 else 4) * (K // 128) >= 128
            and Ni * Hs * Ws * C < (1 << 31) and No * Ho * Wo * K < (1 << 31))


def s2d_tile_weights(w: torch.Tensor, mode: int, out=None) -> torch.Tensor:
    """fp32 [K][C][ks][ks] (3-D: [K][C][3][3][3]) -> fmd_conv_s2d / fmd_conv_d2s tiles (mode 0 stride-2 forward,
    1 data gradient of a 3x3 conv on a nearest-x2 input, 2 stride-2 3x3 data gradient)."""
    K, Cc, ks = w.shape[0], w.shape[1], w.shape[2]
    dims = w.dim() - 2
    n = int(_lib.lib().fmd_s2d_tiled_size_nd(K, Cc, mode, ks, dims))
    if out is None:
        out = torch.empty((n,), device=w.device, dtype=BF16)
    _lib.call("fmd_s2d_tile_weights_nd", _p(w.contiguous()), K, Cc, ks, mode, dims, _p(out), stream())
    return out


def conv(src0, K, wgt, *, src1=None, ks=3, stride=1, pad=1, upsample=False, transposed=False, out_hw_=None,
         pro=None, src2=None, src3=None, wgt2=None, bias=None, bias2=None, bias_nc=None, resid=None, out=None,
         out_f32=False,
         accumulate=False, want_stats=False, ep=None, splits=None, force_generic=False, wgt_tiled=None,
         wgt2_tiled=None, gout=None, s2d_tiled=None, gn=None,
         pro_fold=None, plan_out=None) -> Tuple[torch.Tensor, Optional[Stats]]:
    """Implicit-GEMM conv (see csrc/conv.hip, csrc/conv_halo.hip).  ``pro=(a, b, silu)``, ``ep=(x0, x1, a, b)``.
    ``want_stats``: True = per-channel statistics of the output (a separate fmd_channel_stats pass when the
    kernel cannot emit them); "free" = only when the kernel emits them (else None: Act statistics are then
    derived on demand, and a small-level consumer that computes its own GroupNorm never pays for them).
    ``gout``: bf16 tensor shaped like the (concatenated) input; the halo path writes the prologue's output
    G = SiLU(a*x+b) into it (the weight gradient's operand).  Requires ``pro``, (C0+C1) % 32 == 0 and a
    halo-eligible problem (:func:`halo_eligible`); raises otherwise.
    ``pro_fold``: dict(st0=Stats, st1=Stats or None, groups, eps, gamma, beta[, emb, emb_stride], silu) -- a
    forward-only GroupNorm prologue in place of ``pro``: on the halo path each workgroup folds its sample's affine
    from the statistics slabs (fmd_conv_desc.fold_*, no gn_prep launch); elsewhere it is folded by :func:`gn_prep`
    first and passed as ``pro``.
    ``gn``: dict(groups, eps, gamma, beta[, emb, emb_stride, emb_mode]) -- when the conv runs split-K and
    :func:`conv_gn_eligible` holds, its combine also computes the GroupNorm + SiLU of the output (fmd_conv_gn)
    and stores ``gn["res"] = (a, b, mean_rstd, t)`` as :func:`gn_fused_apply` returns them; otherwise ``gn`` is
    left without "res" and the caller runs the GroupNorm itself.
    ``s2d_tiled``: :func:`s2d_tile_weights` of the stride-2 conv's weight -- the problem runs on the space-to-depth
    halo kernel (fmd_conv_s2d; the caller checks :func:`s2d_eligible`), ``wgt`` unused.
    ``plan_out``: a list; the ``ConvPlan`` the library answered for this call (what fmd_conv then launches) and the
    descriptor's split count are appended to it -- for tests that assert the kernel instance they mean to reach."""
    _need_cuda(src0, "conv")
    # 3-D (spatial_dims = 3): NDHWC tensors, cubic kernels; ``out_hw_`` is then (Do, Ho, Wo)
    d3 = src0.dim() == 5
    if d3:
        N, Ds, Hs, Ws, C0 = src0.shape
    else:
        N, Hs, Ws, C0 = src0.shape
        Ds = 0
    C1 = src1.shape[-1] if src1 is not None else 0
    if out_hw_ is not None:
        Do, Ho, Wo = out_hw_ if d3 else (0, *out_hw_)
    else:
        Ho, Wo = out_hw(Hs, ks, stride, pad, upsample), out_hw(Ws, ks, stride, pad, upsample)
        Do = out_hw(Ds, ks, stride, pad, upsample) if d3 else 0
    M = N * max(Do, 1) * Ho * Wo
    dev = src0.device
    if out is None:
        shape = (N, Do, Ho, Wo, K) if d3 else (N, Ho, Wo, K)
        out = torch.empty(shape, device=dev, dtype=F32 if out_f32 else BF16)
    d = ConvDesc()
    d.N, d.Hs, d.Ws, d.C0, d.C1, d.Ho, d.Wo, d.K = N, Hs, Ws, C0, C1, Ho, Wo, K
    d.Ds, d.Do = Ds, Do
    d.ks, d.stride, d.pad, d.upsample, d.transposed = ks, stride, pad, int(upsample), int(transposed)
    d.src0, d.src1 = _p(src0), _p(src1)
    if pro is not None:
        d.pro_a, d.pro_b, d.pro_silu = _p(pro[0]), _p(pro[1]), int(pro[2])
    d.wgt = _p(wgt)
    if src2 is not None:
        d.src2, d.src3, d.C2, d.C3, d.wgt2 = _p(src2), _p(src3), src2.shape[-1], (src3.shape[-1] if src3 is not None else 0), _p(wgt2)
    d.bias, d.bias2, d.bias_nc, d.resid, d.out = _p(bias), _p(bias2), _p(bias_nc), _p(resid), _p(out)
    d.out_f32, d.accumulate = int(out_f32), int(accumulate)
    if ep is not None:
        x0, x1, ea, eb = ep
        d.ep_x0, d.ep_x1, d.ep_C0, d.ep_a, d.ep_b = _p(x0), _p(x1), x0.shape[-1], _p(ea), _p(eb)
        if x1 is None and x0.shape[-1] != K:
            raise ValueError("epilogue tensor channels must match the conv output channels")
    T = ks * ks * (ks if d3 else 1)
    # host-side operand checks: the kernels index weights as [>=K rows][T][exactly C0+C1] (main) and
    # [>=K][1][C2+C3] (1x1 segment); halo tiles as [K/128][C/32][9][32][128] blocks
    if wgt is not None and (wgt.dim() != 3 or wgt.shape[0] < K or wgt.shape[1] != T or wgt.shape[2] != C0 + C1):
        raise ValueError(f"conv weights {tuple(wgt.shape)} do not match K={K}, taps={T}, C={C0 + C1}")
    if src2 is not None and wgt2 is not None and (wgt2.shape[0] < K or wgt2.shape[-1] != d.C2 + d.C3):
        raise ValueError(f"1x1 segment weights {tuple(wgt2.shape)} do not match K={K}, C={d.C2 + d.C3}")
    for tw, cc, taps in ((wgt_tiled, C0 + C1, 27 if d3 else 9), (wgt2_tiled if src2 is not None else None,
                                                               d.C2 + d.C3, 1)):
        if tw is not None and tw.numel() < -(-K // 128) * 128 * -(-cc // HALO_BK) * HALO_BK * taps:
            raise ValueError(f"halo-tiled weights ({tw.numel()} elements) too small for K={K}, C={cc}")
    nk = -(-(C0 + C1) // 64) * T + (-(-(d.C2 + d.C3) // 64) if src2 is not None else 0)
    if d3:   # depth-tap chunks on the halo kernel: pre-tiled (kz, channel block) weights are required
        halo = (not force_generic and wgt_tiled is not None and Do == (2 * Ds if upsample else Ds) and
                halo_eligible(N * Do, Hs, Ho, Wo, K, ks, stride, pad, upsample, transposed, C0 + C1,
                              pro is not None, ztaps=3))
    else:
        halo = not force_generic and halo_eligible(N, Hs, Ho, Wo, K, ks, stride, pad, upsample, transposed,
                                                   C0 + C1, pro is not None or pro_fold is not None)
    d.force_generic = int(force_generic)
    fold = None
    if pro_fold is not None:
        if pro is not None:
            raise ValueError("conv: pro and pro_fold are exclusive")
        rows_ok = all(st is None or (Hs * Ws) % st.rows == 0 and (Hs * Ws) // st.rows <= HALO_FOLD_MAX_ROWS
                      for st in (pro_fold["st0"], pro_fold.get("st1")))
        if halo and not d3 and gout is None and s2d_tiled is None and HALO_FOLD and rows_ok:
            fold = pro_fold
            _set_fold(d, fold)
        else:
            pro = _fold_now(pro_fold, N, Hs * Ws, C0, C1)
            d.pro_a, d.pro_b, d.pro_silu = _p(pro[0]), _p(pro[1]), int(pro[2])
    if s2d_tiled is not None:   # stride-2 on the halo kernel: one launch, statistics in its epilogue
        ok = (s2d_eligible(N, Hs, Ws, Ho, Wo, K, C0 + C1, ks, Ds, Do) if not transposed else
              (ks == 3 and pro is None and d2s_eligible(N, Hs, Ws, Ho, Wo, K, C0 + C1, Ds, Do)))
        if not ok or stride != 2 or pad != 1 or upsample or src2 is not None or out_f32 or gout is not None:
            raise ValueError("conv: s2d_tiled given for a problem fmd_conv_s2d / fmd_conv_d2s does not take")
        d.wgt_tiled, d.splits = _p(s2d_tiled), 1
        st = None
        if want_stats and (max(Do, 1) * Ho * Wo) % 64 == 0:
            slab = torch.empty((M // 64, K, 2), device=dev, dtype=F32)
            d.stats = _p(slab)
            st = Stats(slab, 64)
        _lib.call("fmd_conv_d2s" if transposed else "fmd_conv_s2d", C.byref(d), stream())
        if want_stats is True and st is None:
            st = channel_stats(out)
        return out, st
    if gout is not None:
        want = (N, Ds, Hs, Ws, C0 + C1) if d3 else (N, Hs, Ws, C0 + C1)
        if pro is None or not halo or (C0 + C1) % HALO_BK or tuple(gout.shape) != want or gout.dtype != BF16:
            raise ValueError(f"gout {tuple(gout.shape)} needs a GN prologue, the halo path and shape {want} bf16")
        d.gout = _p(gout)
    if halo:
        splits = halo_splits(N * max(Do, 1), Ho, Wo, K, C0 + C1, 3 if d3 else 1)
        if wgt_tiled is None:
            wgt_tiled = tile_weights(wgt)
        if src2 is not None and wgt2_tiled is None:
            wgt2_tiled = tile_weights(wgt2)
        d.wgt_tiled, d.wgt2_tiled = _p(wgt_tiled), _p(wgt2_tiled)
    if splits is None:
        bco, bpx = igemm_split_tile(K, M)
        splits = _choose_splits(M, K, nk, bpx, bco)
    ws = None
    if splits > 1:
        ws = torch.empty((splits, M, K), device=dev, dtype=F32)
        d.ws, d.splits = _p(ws), splits
    else:
        d.splits = 1
    with_gn = (gn is not None and CONV_GN and splits > 1 and not want_stats and not out_f32 and not accumulate
               and ep is None and conv_gn_eligible(K, gn["groups"], N))
    # the offers (the fold is in d): statistics from the launch where the images are whole 64-pixel rows, and the
    # split combined inside the launch; the plan says which of them the kernel that runs takes
    allow = _lib.CONV_WANT_STATS if want_stats and (max(Do, 1) * Ho * Wo) % 64 == 0 else 0
    if splits > 1 and not with_gn:
        allow |= (_lib.CONV_TICKET_HALO if HALO_TICKET else 0) | (_lib.CONV_TICKET_IGEMM if SPLIT_TICKET else 0)
        d.n_tickets = SMALL_TICKETS
    L, plan = _lib.lib(), _lib.ConvPlan()
    _lib.check(L.fmd_conv_plan(C.byref(d), allow, C.byref(plan)), "fmd_conv_plan")
    if plan_out is not None:
        plan_out.extend((plan, int(d.splits)))
    if fold is not None and not plan.fold:   # the fold as its own launch
        pro = _fold_now(fold, N, Hs * Ws, C0, C1)
        _clear_fold(d)
        d.pro_a, d.pro_b, d.pro_silu = _p(pro[0]), _p(pro[1]), int(pro[2])
    if with_gn:
        a = torch.empty((N, K), device=dev, dtype=F32)
        b = torch.empty((N, K), device=dev, dtype=F32)
        mr = torch.empty((N, gn["groups"], 2), device=dev, dtype=F32)
        t = torch.empty_like(out)
        g = GnOutDesc()
        g.G, g.eps, g.gamma, g.beta = gn["groups"], float(gn["eps"]), _p(gn["gamma"]), _p(gn["beta"])
        emb = gn.get("emb")
        g.emb, g.emb_stride, g.emb_mode = _p(emb), gn.get("emb_stride", 0), gn.get("emb_mode", 0) if emb is not None else 0
        g.silu, g.a, g.b, g.mean_rstd, g.t = int(gn.get("silu", True)), _p(a), _p(b), _p(mr), _p(t)
        _lib.call("fmd_conv_gn", C.byref(d), C.byref(g), stream())
        gn["res"] = (a, b, mr, t)
        return out, None
    st = None
    if plan.stats_rows:
        slab = torch.empty((M // plan.stats_rows, K, 2), device=dev, dtype=F32)
        d.stats = _p(slab)
        st = Stats(slab, plan.stats_rows)
    if plan.tickets:
        d.tickets, d.tickets_rows = _p(combine_workspace(dev)[1]), plan.stats_rows
    _lib.check(L.fmd_conv(C.byref(d), stream()), "fmd_conv")
    if want_stats is True and st is None:   # "free": only statistics the kernel emits; the consumer derives others
        if ep is not None:
            st = channel_stats(out, y=(ep[0], ep[1], ep[0].shape[-1]))
        else:
            st = channel_stats(out)
    return out, st


def _set_fold(d, f):
    d.fold_st0, d.fold_rows0 = _p(f["st0"].slab), f["st0"].rows
    if f.get("st1") is not None:
        d.fold_st1, d.fold_rows1 = _p(f["st1"].slab), f["st1"].rows
    d.fold_G, d.fold_eps = f["groups"], float(f["eps"])
    d.fold_gamma, d.fold_beta = _p(f.get("gamma")), _p(f.get("beta"))
    emb = f.get("emb")
    d.fold_emb = _p(emb)
    d.fold_emb_stride = (f.get("emb_stride") or emb.shape[-1]) if emb is not None else 0
    d.pro_silu = int(f.get("silu", True))


def _clear_fold(d):
    d.fold_st0 = d.fold_st1 = d.fold_gamma = d.fold_beta = d.fold_emb = None
    d.fold_rows0 = d.fold_rows1 = d.fold_G = d.fold_emb_stride = 0


def _fold_now(f, N, HW, C0, C1):
    """(a, b, silu) of a pro_fold dict by fmd_gn_prep (the fold as its own launch)."""
    emb = f.get("emb")
    a, b, _ = gn_prep(f["st0"], f.get("st1"), N, HW, C0, C1, f["groups"], f["eps"], f.get("gamma"), f.get("beta"),
                      emb=emb, emb_stride=(f.get("emb_stride") or emb.shape[-1]) if emb is not None else 0,
                      emb_mode=1 if emb is not None else 0)
    return a, b, bool(f.get("silu", True))


CONV_SMALL_MODES = {"s1": 0, "s2": 1, "up": 2, "point": 3}
# forward-only small levels in one launch per conv (fmd_conv_small, runtime/tuning.py SMALL_CONV / SMALL_CONV_MAX_HW)
SMALL_CONV = bool(tuning.get("SMALL_CONV"))
SMALL_CONV_MAX_HW = tuning.get("SMALL_CONV_MAX_HW")
SMALL_CONV_MAX_WORK = tuning.get("SMALL_CONV_MAX_WORK")
SMALL_CONV_SPLIT = tuning.get("SMALL_CONV_SPLIT")
# The in-launch combine of a split reduction (csrc/splitk_combine.h): fp32 partial tiles + arrival tickets.
SMALL_PART_BYTES = 8 << 20
SMALL_TICKETS = 4096
_combine_ws = {}   # (device index, stream handle) -> (part buffer, tickets); owner: combine_workspace / release_...


def combine_workspace(dev):
    """(part buffer, tickets) of the in-launch combine for the current stream of ``dev``: SMALL_PART_BYTES of fp32
    parts (fmd_conv_small; fmd_conv's ticketed kernels keep their parts in the conv's own workspace) and
    SMALL_TICKETS int32 arrival counters, both created together on that stream at first use.  Launches on one stream
    serialise, so they share one set; the tickets are zero at creation and every completed launch leaves them zero,
    so nothing fills them again.  (A first use inside a graph capture would record that zero-fill into the graph:
    ``capture_stream`` creates its entry beforehand.)

    The entry lives until ``release_combine_workspace``.  torch hands out stream handles from a fixed pool per
    device (32 per priority, plus the default stream), so the dictionary is bounded by that pool, not by the number
    of ``torch.cuda.Stream`` objects created -- but every pool stream that ever ran a ticketed conv or a split
    ``conv_small`` keeps its 8 MiB + 16 KiB until released."""
    key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
    ws = _combine_ws.get(key)
    if ws is None:
        ws = (torch.empty(SMALL_PART_BYTES // 4, device=dev, dtype=F32),
              torch.zeros(SMALL_TICKETS, device=dev, dtype=torch.int32))
        _combine_ws[key] = ws
    return ws


def release_combine_workspace(stream):
    """Drop the combine workspace of ``stream`` (a ``torch.cuda.Stream`` the caller is done with, joined by a
    ``wait_stream`` or synchronised; the memory goes back to the allocator under that stream, so work still queued
    on it stays ordered before any reuse).  The capture stream's entry is kept: captured graphs have its pointers
    baked in, and its handle can come round again in a later ``torch.cuda.Stream()`` (the pool is round-robin).
    For the same reason the handle of an abandoned stream can be that of another live ``torch.cuda.Stream`` object
    (a FusedTrainStep's work stream, say) once 32 streams have been created; releasing then drops the live stream's
    entry too.  That is harmless: launches on the shared handle stay ordered, and the entry is created again, zero
    tickets included, at that stream's next eager use."""
    cap = _cap_streams.get(stream.device.index)
    if cap is None or cap.cuda_stream != stream.cuda_stream:
        _combine_ws.pop((stream.device.index, stream.cuda_stream), None)


# the accessor's name while it was private: the earlier revisions of tests/test_gpu_halo_ticket.py and
# tests/test_gpu_halo_fold.py read the tickets through it, and they must keep passing on this library
_small_workspace = combine_workspace


def combine_workspace_streams(dev):
    """The stream handles that hold a combine workspace on ``dev`` (introspection, for tests: nothing in the library
    calls it)."""
    return [h for (i, h) in _combine_ws if i == dev.index]


_cap_streams = {}
CAPTURE_STREAM = bool(tuning.get("CAPTURE_STREAM"))


def capture_stream():
    """The stream graph captures run on: a side stream whose in-launch-combine workspace (tickets zeroed) is created
    before the first capture, so a capture records no fill of it (a fresh per-stream workspace allocated inside the
    capture would replay its zero-fill every step).

    Sharing rule: every graph captured on this stream has the same ticket array and part buffer baked in -- a
    FusedTrainStep's main and bucket graphs, and any sampler captured in the same process, share one workspace.
    Such graphs must be replayed one after another (on one stream, or ordered by stream waits), never concurrently
    on two streams: interleaved ticket adds of two launches would leave tiles without a reducer.  FusedTrainStep.replay
    (its bucket graphs included) and the samplers replay on the caller's current stream, which keeps the rule;
    nothing checks it."""
    if not CAPTURE_STREAM:
        return None   # torch's own capture stream
    idx = torch.cuda.current_device()
    s = _cap_streams.get(idx)
    if s is None:
        s = torch.cuda.Stream(idx)
        with torch.cuda.stream(s):
            combine_workspace(torch.device("cuda", idx))
        _cap_streams[idx] = s
    return s


def _conv_small_desc(shape0, C1, K, mode, gn, skip, ptrs, split=None):
    """fmd_conv_small_desc for input shape ``shape0`` = (N, Hs, Ws, C0) (+ C1 concat channels).  ``ptrs``: dict of
    device pointers (a host-only plan query passes placeholders)."""
    from .._lib import ConvSmallDesc
    N, Hs, Ws, C0 = shape0
    m = CONV_SMALL_MODES[mode]
    Ho, Wo = (Hs // 2, Ws // 2) if m == 1 else (2 * Hs, 2 * Ws) if m == 2 else (Hs, Ws)
    d = ConvSmallDesc()
    d.N, d.Hs, d.Ws, d.C0, d.C1, d.Ho, d.Wo, d.K, d.mode = N, Hs, Ws, C0, C1, Ho, Wo, K, m
    d.src0, d.src1, d.wgt, d.out = ptrs["src0"], ptrs.get("src1"), ptrs["wgt"], ptrs["out"]
    if gn is not None:
        d.st0, d.rows0 = ptrs["st0"], gn["st0"].rows
        if gn.get("st1") is not None:
            d.st1, d.rows1 = ptrs["st1"], gn["st1"].rows
        d.G, d.eps = gn["groups"], float(gn["eps"])
        d.gamma, d.beta, d.emb = ptrs.get("gamma"), ptrs.get("beta"), ptrs.get("emb")
        emb = gn.get("emb")
        d.emb_stride = (gn.get("emb_stride") or emb.shape[-1]) if emb is not None else 0
        d.silu = int(gn.get("silu", True))
    if skip:   # (C2, C3): channels of the raw 1x1-segment sources at the output pixels
        d.C2, d.C3 = skip
        d.src2, d.src3, d.wgt2 = ptrs["src2"], ptrs.get("src3"), ptrs["wgt2"]
    d.split = SMALL_CONV_SPLIT if split is None else split
    if d.split != 1:
        d.part, d.part_bytes, d.tickets, d.n_tickets = ptrs["part"], SMALL_PART_BYTES, ptrs["tickets"], SMALL_TICKETS
    return d, (N, Ho, Wo)


def _conv_small_query(fn, shape0, K, C1, mode, gn, skip, split):
    fake = dict(src0=16, src1=16 if C1 else None, wgt=16, out=16, st0=16, st1=16, wgt2=16, src2=16,
                src3=16 if skip and skip[1] else None, part=16, tickets=16)
    d, _ = _conv_small_desc(tuple(shape0), C1, K, mode, gn, skip, fake, split)
    return int(getattr(_lib.lib(), fn)(C.byref(d)))


def conv_small_ok(shape0, K, *, C1=0, mode="s1", gn=None, skip=None, split=None) -> bool:
    """Whether fmd_conv_small takes the problem on input shape ``shape0`` = (N, Hs, Ws, C0) (fmd_conv_small_plan:
    geometry, channel counts, one CU's LDS; a host-side query, nothing is launched), within the SMALL_CONV switches.
    ``skip``: (C2, C3) channels of a 1x1 segment's sources, or None.  ``split``: parts of the reduction (None:
    SMALL_CONV_SPLIT; 0 the plan's choice, 1 none)."""
    if not SMALL_CONV or len(shape0) != 4 or K % 16:
        return False
    m = CONV_SMALL_MODES[mode]
    HWo = shape0[1] * shape0[2] * (4 if m == 2 else 1) // (4 if m == 1 else 1)
    if HWo > SMALL_CONV_MAX_HW or HWo * (shape0[3] + C1) > SMALL_CONV_MAX_WORK:
        return False
    return _conv_small_query("fmd_conv_small_plan", shape0, K, C1, mode, gn, skip, split) > 0


def conv_small_split(shape0, K, *, C1=0, mode="s1", gn=None, skip=None, split=None) -> int:
    """The parts fmd_conv_small splits the reduction of this problem into (fmd_conv_small_split; host-side)."""
    return _conv_small_query("fmd_conv_small_split", shape0, K, C1, mode, gn, skip, split)


def conv_small(src0, K, wgt, *, src1=None, mode="s1", gn=None, src2=None, src3=None, skip_wgt=None, bias=None,
               bias2=None, bias_nc=None, resid=None, out=None, want_stats=True,
               split=None) -> Tuple[torch.Tensor, Optional[Stats]]:
    """One-launch small-level conv (fmd_conv_small, csrc/conv_small.hip; forward only).

    ``mode``: "s1" 3x3 stride 1, "s2" 3x3 stride 2 (DownsampleND), "up" nearest-x2 + 3x3 (UpsampleND), "point" 1x1
    (the centre tap of a 3x3 on 1x1 images).  ``wgt``: fmd_prep_weights mode-0 layout [K][T][C0 + C1].
    ``gn``: GroupNorm(+scale/shift)+SiLU prologue folded from the inputs' statistics:
    dict(st0=Stats, st1=Stats or None, groups, eps, gamma, beta[, emb, emb_stride, silu]).  ``src2`` | ``src3``,
    ``skip_wgt`` (bf16 [K][1][C2 + C3]): a 1x1 conv over raw tensors at the output resolution (the ResBlock skip
    connection over the block input).  ``bias_nc``: [N][>=K] per-sample bias
    (row stride taken from the tensor).  Returns (out, Stats of the bf16 output: 64-pixel rows, or one row per
    image when Ho*Wo < 64).  ``split``: parts of the reduction, combined inside the launch (None: SMALL_CONV_SPLIT;
    0 the plan's choice -- enough workgroups for the chip --, 1 none, 2..16 forced)."""
    _need_cuda(src0, "conv_small")
    C1 = src1.shape[-1] if src1 is not None else 0
    ptrs = dict(src0=_p(src0), src1=_p(src1), wgt=_p(wgt), out=_p(out), wgt2=_p(skip_wgt), src2=_p(src2),
                src3=_p(src3))
    if gn is not None:
        ptrs.update(st0=_p(gn["st0"].slab), st1=_p(gn["st1"].slab) if gn.get("st1") is not None else None,
                    gamma=_p(gn.get("gamma")), beta=_p(gn.get("beta")), emb=_p(gn.get("emb")))
    skip = (src2.shape[-1], src3.shape[-1] if src3 is not None else 0) if skip_wgt is not None else None
    part, tickets = combine_workspace(src0.device)
    ptrs.update(part=_p(part), tickets=_p(tickets))
    d, (N, Ho, Wo) = _conv_small_desc(tuple(src0.shape), C1, K, mode, gn, skip, ptrs, split)
    d.bias, d.bias2, d.resid = _p(bias), _p(bias2), _p(resid)
    if bias_nc is not None:
        d.bias_nc, d.bias_nc_stride = _p(bias_nc), bias_nc.stride(0)
    if out is None:
        out = torch.empty((N, Ho, Wo, K), device=src0.device, dtype=BF16)
        d.out = _p(out)
    st = None
    if want_stats:
        rows = 64 if (Ho * Wo) % 64 == 0 else Ho * Wo
        slab = torch.empty((N * Ho * Wo // rows, K, 2), device=src0.device, dtype=F32)
        d.stats = _p(slab)
        st = Stats(slab, rows)
    _lib.call("fmd_conv_small", C.byref(d), stream())
    return out, st


def conv_combine(ws, K, out_shape, *, bias=None, bias2=None, bias_nc=None, resid=None, ep=None, out=None,
                 accumulate=False, want_stats=False):
    """out (bf16, N-D ``out_shape`` = (N, *sp)) = sum of the fp32 slabs ws [S][M][K] + conv epilogue
    (fmd_conv_combine); returns (out, Stats)."""
    N, sp = out_shape[0], tuple(out_shape[1:])
    Do, Ho, Wo = (0, *sp) if len(sp) == 2 else sp
    if out is None:
        out = torch.empty((N, *sp, K), device=ws.device, dtype=BF16)
    d = ConvDesc()
    d.N, d.Ho, d.Wo, d.Do, d.Hs, d.Ws, d.Ds, d.K = N, Ho, Wo, Do, Ho, Wo, Do, K
    d.ks, d.stride, d.pad = 3, 1, 1
    d.ws, d.splits = _p(ws), ws.shape[0]
    d.bias, d.bias2, d.bias_nc, d.resid, d.out = _p(bias), _p(bias2), _p(bias_nc), _p(resid), _p(out)
    d.accumulate = int(accumulate)
    if ep is not None:
        x0, x1, ea, eb = ep
        d.ep_x0, d.ep_x1, d.ep_C0, d.ep_a, d.ep_b = _p(x0), _p(x1), x0.shape[-1], _p(ea), _p(eb)
    HWo = max(Do, 1) * Ho * Wo
    M = N * HWo
    st = None
    fused = want_stats and not accumulate and K % 4 == 0 and HWo % SPLIT_STATS_ROWS == 0
    if fused:
        slab = torch.empty((M // SPLIT_STATS_ROWS, K, 2), device=ws.device, dtype=F32)
        d.stats = _p(slab)
        st = Stats(slab, SPLIT_STATS_ROWS)
    _lib.call("fmd_conv_combine", C.byref(d), stream())
    if want_stats and not fused:
        st = channel_stats(out, y=(ep[0], ep[1], ep[0].shape[-1])) if ep is not None else channel_stats(out)
    return out, st


def head_eligible(H, W, C, K, D=0) -> bool:
    """Mirror of the head kernels' shape test (csrc/head.hip); D > 0: 3-D data of depth D."""
    return H % 16 == 0 and W % 16 == 0 and C % 32 == 0 and 1 <= K <= (2 if D else 8)


def _head_dims(h):
    """(N, D, H, W, C) of a 2-D NHWC (D = 0) or 3-D NDHWC head input."""
    if h.dim() == 4:
        N, H, W, Cc = h.shape
        return N, 0, H, W, Cc
    return tuple(h.shape)


def head_fwd(h, pro, w, bias, K, Kp=8, out=None):
    """out fp32 channels-last [..., Kp] = conv3x3(x3)(SiLU(a*h+b)) for the first K channels (csrc/head.hip);
    ``out``: the buffer to write instead of a new one."""
    _need_cuda(h, "head_fwd")
    N, D, H, W, Cc = _head_dims(h)
    if out is None:
        out = torch.empty((*h.shape[:-1], Kp), device=h.device, dtype=F32)
    _lib.call("fmd_head_fwd", _p(h), N, D, H, W, Cc, _p(pro[0]), _p(pro[1]), _p(w.contiguous()), _p(bias), K,
              _p(out), stream())
    return out


def head_dgrad(dpred, w, K, h, pro, out=None):
    """(dz bf16 channels-last, Stats(sum dz, sum dz*h)) of the head conv (csrc/head.hip); ``out``: the (dz, slab)
    buffers to write instead of new ones."""
    N, D, H, W, Cc = _head_dims(h)
    if out is None:
        out = (torch.empty_like(h), torch.empty((h.numel() // Cc // 64, Cc, 2), device=h.device, dtype=F32))
    dz, slab = out
    _lib.call("fmd_head_dgrad", _p(dpred), _p(w.contiguous()), K, _p(h), _p(pro[0]), _p(pro[1]), N, D, H, W, Cc,
              _p(dz), _p(slab), stream())
    return dz, Stats(slab, 64)


def head_wgrad(dpred, K, h, pro, dw, db):
    N, D, H, W, Cc = _head_dims(h)
    n = int(_lib.lib().fmd_head_wgrad_workspace(N, D, H, W, Cc, K))
    ws = torch.empty((n,), device=h.device, dtype=F32)
    _lib.call("fmd_head_wgrad", _p(dpred), K, _p(h), _p(pro[0]), _p(pro[1]), N, D, H, W, Cc, _p(dw), _p(db), _p(ws),
              stream())


# generic weight-gradient split-K: >= WGRAD_MIN_STEPS 32-pixel steps per split, ~WGRAD_CU_MULT workgroups per CU
WGRAD_MIN_STEPS = tuning.get("WGRAD_MIN_STEPS")
WGRAD_CU_MULT = tuning.get("WGRAD_CU_MULT")
# workgroups the halo weight gradient aims for (one per CU); fewer means fewer pixel splits, i.e. smaller
# split-K slabs (their write + reduce read) at the small levels (tuning WGRAD_HALO_WG: A/B override)
WGRAD_HALO_WG = tuning.get("WGRAD_HALO_WG") or NUM_CU
# split-K slab caps (MB): the partial slabs' write + reduce read bound the small levels (A/B: tuning WGRAD_SLAB_MB,
# WGRAD_GEN_SLAB_MB)
WGRAD_SLAB_MB = tuning.get("WGRAD_SLAB_MB")
WGRAD_GEN_SLAB_MB = tuning.get("WGRAD_GEN_SLAB_MB")
WGRAD_S2D = bool(tuning.get("WGRAD_S2D"))
# grouped weight gradients (fmd_wgrad_group): the deferred jobs of a level in one launch with the group's splits
WGRAD_GROUP = bool(tuning.get("WGRAD_GROUP"))
WGRAD_GROUP_MAX_PIX = tuning.get("WGRAD_GROUP_MAX_PIX")
WGRAD_GROUP_SPLITS = tuning.get("WGRAD_GROUP_SPLITS")


def wgrad_halo_eligible(Hs, Ws, Ho, Wo, K, C, C0, ks=3, stride=1, pad=1, upsample=False, ldy=None) -> bool:
    """Mirror of fmd_wgrad_halo's applicability test (csrc/wgrad_halo.hip): 3x3 pad 1, stride 1 (optionally on a
    nearest-x2 input) or 2-D stride 2 (the space-to-depth planes as chunks; 3-D stride 2 stays generic)."""
    if stride == 2:
        geo = WGRAD_S2D and not upsample and Hs == 2 * Ho and Ws == 2 * Wo
    else:
        geo = stride == 1 and (Ho == 2 * Hs and Wo == 2 * Ws if upsample else Ho == Hs and Wo == Ws)
    return (ks == 3 and pad == 1 and geo and Ho % 8 == 0
            and Wo % 16 == 0 and K % 128 == 0 and C % 64 == 0 and C0 % 8 == 0 and (ldy or K) % 8 == 0)


def _plan_kw() -> dict:
    return dict(num_cu=NUM_CU, halo_wg=WGRAD_HALO_WG, slab_mb=WGRAD_SLAB_MB, gen_slab_mb=WGRAD_GEN_SLAB_MB,
                min_steps=WGRAD_MIN_STEPS, cu_mult=WGRAD_CU_MULT)


class WgradJob:
    """One weight gradient ready to launch but for its splits and workspace: the descriptor, its shape record
    for the planner and the tensors the descriptor points into (kept alive until the launch is issued)."""
    __slots__ = ("d", "shape", "keep", "device")

    def __init__(self, d, shape, keep, device):
        self.d, self.shape, self.keep, self.device = d, shape, keep, device

    def single_splits(self) -> int:
        return wgrad_plan.single_splits(self.shape, **_plan_kw())


def wgrad_job(src0, dy, dw, *, src1=None, ks=3, stride=1, pad=1, upsample=False, pro=None, db=None, accumulate=True,
              dy_offset=0, force_generic=False) -> WgradJob:
    """Descriptor of one weight gradient (arguments as for ``wgrad``); nothing is launched."""
    d3 = src0.dim() == 5
    if d3:
        N, Ds, Hs, Ws, C0 = src0.shape
        _, Do, Ho, Wo, ldy = dy.shape
    else:
        N, Hs, Ws, C0 = src0.shape
        _, Ho, Wo, ldy = dy.shape
        Ds = Do = 0
    C1 = src1.shape[-1] if src1 is not None else 0
    K = dw.shape[0]
    M = N * max(Do, 1) * Ho * Wo
    Ct = C0 + C1
    d = WgradDesc()
    d.N, d.Hs, d.Ws, d.C0, d.C1, d.Ho, d.Wo, d.K = N, Hs, Ws, C0, C1, Ho, Wo, K
    d.Ds, d.Do = Ds, Do
    d.ks, d.stride, d.pad, d.upsample = ks, stride, pad, int(upsample)
    d.src0, d.src1 = _p(src0), _p(src1)
    if pro is not None:
        d.pro_a, d.pro_b, d.pro_silu = _p(pro[0]), _p(pro[1]), int(pro[2])
    d.dy, d.ldy, d.dw, d.db, d.accumulate = dy.data_ptr() + 2 * dy_offset, ldy, _p(dw), _p(db), int(accumulate)
    d.force_generic = int(force_generic)
    # the kernel the library will choose (mirror of fmd_wgrad's dispatch) and the shape the split rules work on:
    # halo kernel -- workgroups over (cout tile, 64-cin chunk [x depth tap | x stride-2 plane], pixel-tile split);
    # generic kernel -- narrow inputs (Ct < 128, T > 1) tile the flattened (tap, cin) pairs (csrc/wgrad.hip
    # make_args ``merged``).  The rules themselves are in wgrad_plan.
    halo = (not force_generic and (not d3 or (stride == 1 and Do == (2 * Ds if upsample else Ds))) and
            wgrad_halo_eligible(Hs, Ws, Ho, Wo, K, Ct, C0, ks, stride, pad, upsample, ldy))
    shape = wgrad_plan.Shape(N=N, Ho=Ho, Wo=Wo, K=K, C=Ct, ks=ks, stride=stride, halo=bool(halo),
                             pro=0 if pro is None else 2 if pro[2] else 1, Do=Do)
    keep = (src0, src1, dy, dw, db) + (tuple(pro[:2]) if pro is not None else ())
    return WgradJob(d, shape, keep, dy.device)


def _wgrad_workspace(jobs) -> torch.Tensor:
    """One allocation for the jobs' partial slabs (each desc's ``splits`` set): d.ws of every job points into it."""
    sizes = [-(-int(_lib.lib().fmd_wgrad_workspace(C.byref(j.d))) // 64) * 64 for j in jobs]
    ws = torch.empty((sum(sizes),), device=jobs[0].device, dtype=F32)
    off = 0
    for j, n in zip(jobs, sizes):
        j.d.ws = ws.data_ptr() + 4 * off
        off += n
    return ws


def wgrad_group(jobs, splits) -> None:
    """Launch the jobs (one kernel instance: equal ``shape.key``) with the given splits (an int for all, or one
    per job) through fmd_wgrad_group: one MFMA launch and one combine launch per FMD_WGRAD_GROUP_MAX jobs.  Each
    job's result is bit-identical to ``wgrad`` with the same splits."""
    splits = [splits] * len(jobs) if isinstance(splits, int) else list(splits)
    for lo in range(0, len(jobs), wgrad_plan.GROUP_MAX):
        part = jobs[lo:lo + wgrad_plan.GROUP_MAX]
        for j, s in zip(part, splits[lo:]):
            j.d.splits = s
        ws = _wgrad_workspace(part)   # noqa: F841 -- stream-ordered allocation: alive until the launches are issued
        arr = (WgradDesc * len(part))(*[j.d for j in part])
        _lib.call("fmd_wgrad_group", arr, len(part), stream())


class WgradQueue:
    """Deferred weight gradients of one backward pass, one list per kernel instance.  Nothing reads a weight
    gradient before the engine's ``_join``, so the jobs of a level wait here and go out as grouped launches with
    the group plan's (fewer) splits: when the output grid changes, when a list reaches the group cap, and at
    ``flush``.  A job that would write a dW / db already queued flushes first (program order per destination)."""

    def __init__(self):
        self.lists = {}
        self.grid = None
        self.dests = set()

    def __len__(self):
        return sum(len(v) for v in self.lists.values())

    def push(self, job: WgradJob) -> None:
        dst = {int(job.d.dw or 0), int(job.d.db or 0)} - {0}
        if (self.grid is not None and job.shape.grid != self.grid) or (dst & self.dests):
            self.flush()
        self.grid = job.shape.grid
        self.dests |= dst
        lst = self.lists.setdefault(job.shape.key, [])
        lst.append(job)
        if len(lst) >= wgrad_plan.GROUP_MAX:
            self._launch(self.lists.pop(job.shape.key))

    def _launch(self, jobs) -> None:
        if WGRAD_GROUP_SPLITS:   # each job's ungrouped splits: bit-identical to the immediate path
            wgrad_group(jobs, [j.single_splits() for j in jobs])
            return
        for idx, splits in wgrad_plan.plan_groups([j.shape for j in jobs], **_plan_kw()):
            wgrad_group([jobs[i] for i in idx], splits)

    def flush(self) -> None:
        lists, self.lists, self.grid, self.dests = self.lists, {}, None, set()
        for jobs in lists.values():
            self._launch(jobs)

    def clear(self) -> None:
        self.lists, self.grid, self.dests = {}, None, set()


_wgrad_queue: Optional[WgradQueue] = None


class wgrad_defer:
    """Within the block, ``wgrad`` calls that may wait are queued on ``queue`` instead of launched."""

    def __init__(self, queue: Optional[WgradQueue]):
        self.queue = queue

    def __enter__(self):
        global _wgrad_queue
        self.prev, _wgrad_queue = _wgrad_queue, self.queue

    def __exit__(self, *exc):
        global _wgrad_queue
        _wgrad_queue = self.prev


def wgrad(src0, dy, dw, *, src1=None, ks=3, stride=1, pad=1, upsample=False, pro=None, db=None, accumulate=True,
          splits=None, dy_offset=0, force_generic=False, immediate=False):
    """dW (+)= conv weight gradient in the reference [K][C][kh][kw] fp32 layout (and db).

    ``dy_offset``: use channels [dy_offset, dy_offset + dw.shape[0]) of a wider dY (fused q/k/v).
    A 1-D k-tap weight ([K][C][k], k > 1) on (L, 1)-image activations: the k x k gradient of its embedding
    is computed and its centre column (the only one that meets data) is added in.
    Under ``wgrad_defer`` the job is queued for a grouped launch unless ``immediate`` (the caller post-processes
    dw right away), ``splits`` is given, it is 3-D, or its output grid exceeds WGRAD_GROUP_MAX_PIX pixels; a job
    launched at once flushes the queue first, so launches that write gradients keep their program order."""
    q = _wgrad_queue
    if dw.dim() == 3 and dw.shape[2] > 1 and src0.dim() == 4:
        full = torch.zeros((*dw.shape[:2], ks, ks), device=dw.device, dtype=F32)
        wgrad(src0, dy, full, src1=src1, ks=ks, stride=stride, pad=pad, upsample=upsample, pro=pro, db=db,
              accumulate=accumulate, splits=splits, dy_offset=dy_offset, force_generic=force_generic, immediate=True)
        col = full[..., (ks - 1) // 2]
        if accumulate:
            dw.add_(col)
        else:
            dw.copy_(col)
        return
    job = wgrad_job(src0, dy, dw, src1=src1, ks=ks, stride=stride, pad=pad, upsample=upsample, pro=pro, db=db,
                    accumulate=accumulate, dy_offset=dy_offset, force_generic=force_generic)
    if q is not None:
        if (not immediate and splits is None and src0.dim() == 4
                and job.shape.pixels <= WGRAD_GROUP_MAX_PIX):
            q.push(job)
            return
        q.flush()
    job.d.splits = job.single_splits() if splits is None else splits
    ws = _wgrad_workspace([job])   # noqa: F841
    _lib.call("fmd_wgrad", C.byref(job.d), stream())


# the skip conv's weight / bias gradient inside the GroupNorm-1 backward apply pass (fmd_skip_bwd); SKIP_BWD=0
# (runtime/tuning.py): fmd_conv_gn_apply + the ks=1 weight gradient (A/B runs, bisection)
SKIP_BWD = bool(tuning.get("SKIP_BWD"))
SKIP_BWD_MIN_TILES = tuning.get("SKIP_BWD_MIN_TILES")   # fewest pixel tiles per group the plan takes (measured floor)


class _SkipWs:
    """What ``_wgrad_workspace`` sizes: the fused launch's slabs are those of a 1x1 weight gradient with
    ``slabs`` splits."""
    __slots__ = ("d", "device")

    def __init__(self, Kd, C0, C1, slabs, device):
        self.d = WgradDesc()
        self.d.K, self.d.C0, self.d.C1, self.d.ks, self.d.splits = Kd, C0, C1, 1, slabs
        self.device = device


def _skip_bwd_desc(N, HW, C0, C1, Kd, groups=0, min_tiles=None) -> SkipBwdDesc:
    d = SkipBwdDesc()
    d.N, d.HW, d.C0, d.C1, d.Kd, d.groups, d.num_cu = N, HW, C0, C1, Kd, groups, NUM_CU
    d.min_tiles = SKIP_BWD_MIN_TILES if min_tiles is None else min_tiles
    return d


def skip_bwd_plan(N, HW, C0, C1, Kd, groups=0, min_tiles=None) -> Optional[SkipBwdPlan]:
    """fmd_skip_bwd_plan's answer for a skip conv of Kd output channels over N x HW pixels of a C0|C1 input
    (host arithmetic only): the plan, or None where the fused pass is not taken (or SKIP_BWD=0).  ``min_tiles``: the
    floor on pixel tiles per group (default SKIP_BWD_MIN_TILES; tests pass 0 to run small shapes)."""
    if not SKIP_BWD:
        return None
    p = SkipBwdPlan()
    rc = _lib.lib().fmd_skip_bwd_plan(C.byref(_skip_bwd_desc(N, HW, C0, C1, Kd, groups, min_tiles)), C.byref(p))
    return p if rc == 0 and p.taken else None


def skip_bwd(dy, wgt_t, dz, x0, x1, P, Q, R, dx0, acc0, dx1, acc1, dw, db, accumulate=True, groups=0,
             min_tiles=None) -> bool:
    """The skip conv's whole backward in one pass (fmd_skip_bwd): dx as ``conv1x1_gn_apply`` (same arguments,
    bit-identical) and dw / db (+)= the ks=1 weight gradient of ``wgrad(x0, dy, dw, src1=x1, ks=1, pad=0, db=db)``.
    ``groups``: forced pixel groups, ``min_tiles``: the plan's floor (tests).  Returns False, with nothing launched,
    where the plan refuses."""
    _need_cuda(dy, "skip_bwd")
    N, Kd = dy.shape[0], dy.shape[-1]
    HW = dy[0, ..., 0].numel()
    C0 = x0.shape[-1]
    C1 = x1.shape[-1] if x1 is not None else 0
    plan = skip_bwd_plan(N, HW, C0, C1, Kd, groups, min_tiles)
    if plan is None:
        return False
    d = _skip_bwd_desc(N, HW, C0, C1, Kd, groups, min_tiles)
    d.dy, d.wgt_t = _p(dy), _p(wgt_t)
    d.g.dz, d.g.x0, d.g.x1, d.g.C0 = _p(dz), _p(x0), _p(x1), C0
    d.g.P, d.g.Q, d.g.R = _p(P), _p(Q), _p(R)
    d.g.dx0, d.g.acc0, d.g.dx1, d.g.acc1 = _p(dx0), int(acc0), _p(dx1), int(acc1)
    d.dw, d.db, d.accumulate = _p(dw), _p(db), int(accumulate)
    job = _SkipWs(Kd, C0, C1, plan.slabs, dy.device)
    ws = _wgrad_workspace([job])   # noqa: F841 -- stream-ordered allocation
    if ws.numel() < plan.ws_floats:
        raise RuntimeError("skip_bwd: workspace smaller than the plan's")
    d.ws = job.d.ws
    _lib.call("fmd_skip_bwd", C.byref(d), stream())
    return True


def prep_weights(w: torch.Tensor, mode: int, Kpad: Optional[int] = None, Cpad: Optional[int] = None, out=None):
    """fp32 [K][C][kh][kw] -> bf16 kernel layout (mode 0 fwd [Kpad][T][Cpad]; 1 dgrad [Cpad][T][Kpad]; 2 up-dgrad)."""
    K, Cc = w.shape[0], w.shape[1]
    ks = w.shape[2] if w.dim() >= 4 else 1
    Kpad = Kpad or K
    Cpad = Cpad or Cc
    if w.dim() == 5:   # 3-D: ks^3 taps (modes 0, 1, 3)
        T = ks ** 3
        shape = (Kpad, T, Cpad) if mode == 0 else (Cpad, T, Kpad)
        if out is None:
            out = torch.empty(shape, device=w.device, dtype=BF16)
        _lib.call("fmd_prep_weights_t", _p(w.contiguous()), K, Cc, T, mode, Kpad, Cpad, _p(out), stream())
        return out
    T = 16 if mode == 2 else ks * ks
    shape = (Kpad, T, Cpad) if mode == 0 else (Cpad, T, Kpad)
    if out is None:
        out = torch.empty(shape, device=w.device, dtype=BF16)
    _lib.call("fmd_prep_weights", _p(w.contiguous()), K, Cc, ks, mode, Kpad, Cpad, _p(out), stream())
    return out


def tile_weights(wk: torch.Tensor, out=None):
    """bf16 kernel-layout weights [rows][T][cols] -> halo-kernel tiles (csrc/conv_halo.hip)."""
    R, T, Cc = wk.shape
    n = int(_lib.lib().fmd_halo_tiled_size(R, T, Cc))
    if out is None:
        out = torch.empty((n,), device=wk.device, dtype=BF16)
    _lib.call("fmd_tile_weights_halo", _p(wk), R, T, Cc, _p(out), stream())
    return out


def nchw_to_nhwc(x: torch.Tensor, Cpad: Optional[int] = None) -> torch.Tensor:
    _need_cuda(x, "nchw_to_nhwc")
    x = x.contiguous().float()
    N, Cc = x.shape[:2]
    HW = x[0, 0].numel()
    Cpad = Cpad or Cc
    y = torch.empty((N, *x.shape[2:], Cpad), device=x.device, dtype=BF16)
    _lib.call("fmd_nchw_to_nhwc", _p(x), N, Cc, HW, Cpad, _p(y), stream())
    return y


def nhwc_to_nchw(y: torch.Tensor, Cc: int) -> torch.Tensor:
    N = y.shape[0]
    sp = y.shape[1:-1]
    Cs = y.shape[-1]
    x = torch.empty((N, Cc, *sp), device=y.device, dtype=F32)
    _lib.call("fmd_nhwc_to_nchw", _p(y), int(y.dtype == F32), N, Cc, x[0, 0].numel(), Cs, _p(x), stream())
    return x


def timestep_embedding(t: torch.Tensor, dim: int, flip: bool, shift: int = 0, max_period: float = 10000.0,
                       t_scale: float = 1.0, t_trunc: bool = False):
    if t.dtype != F32:
        t = t.float()
    t = t.contiguous()
    out = torch.empty((t.shape[0], dim), device=t.device, dtype=F32)
    _lib.call("fmd_timestep_embedding", _p(t), t.shape[0], dim, int(flip), shift, float(max_period), float(t_scale),
              int(t_trunc), _p(out), stream())
    return out


def linear(x, w, b, in_silu=False, out=None, out_stride=None):
    B, I = x.shape
    O = w.shape[0]
    if out is None:
        out = torch.empty((B, O), device=x.device, dtype=F32)
    _lib.call("fmd_linear", _p(x), B, I, _p(w), _p(b), O, int(in_silu), _p(out), out_stride or O, stream())
    return out


def linear_bwd(x, w, dy, dw, db, dx=None, dx_acc=False, in_silu=False, dy_stride=None):
    B, I = x.shape
    O = w.shape[0]
    _lib.call("fmd_linear_bwd", _p(x), B, I, _p(w), O, int(in_silu), _p(dy), dy_stride or dy.shape[-1], _p(dx),
              int(dx_acc), _p(dw), _p(db), stream())


class GroupedLinear:
    """Every ResBlock ``emb_layers`` projection (residual.py:63-68) of a UNet as one launch each way
    (csrc/misc.hip glinear_*): outputs are concatenated [B][sum O]; group g owns columns
    [off_g, off_g + O_g).  The device descriptor table is rebuilt only when a parameter or gradient
    storage moves (never during hipGraph capture once warmed up)."""

    ROWS = 64

    def __init__(self, linears, in_silu: bool):
        self.linears = list(linears)
        self.in_silu = bool(in_silu)
        self.O = [int(l.weight.shape[0]) for l in self.linears]
        self.I = int(self.linears[0].weight.shape[1])
        self.off = []
        o = 0
        for n in self.O:
            self.off.append(o)
            o += n
        self.total = o
        self.blocks_host = [(g, r0) for g, n in enumerate(self.O) for r0 in range(0, n, self.ROWS)]
        self._key = None
        self._groups = None
        self._blocks = None

    def _table(self, dev):
        key = tuple((l.weight.data_ptr(), l.bias.data_ptr() if l.bias is not None else 0,
                     l.weight.grad.data_ptr() if l.weight.grad is not None else 0,
                     l.bias.grad.data_ptr() if (l.bias is not None and l.bias.grad is not None) else 0)
                    for l in self.linears)
        if key != self._key:
            rows = [[w, b, gw, gb, n, off] for (w, b, gw, gb), n, off in zip(key, self.O, self.off)]
            self._groups = torch.tensor(rows, dtype=torch.int64).to(dev)
            self._blocks = torch.tensor(self.blocks_host, dtype=torch.int32).to(dev)
            self._key = key
        return self._groups, self._blocks

    def forward(self, x):
        _need_cuda(x, "GroupedLinear")
        B = x.shape[0]
        x = x.contiguous()
        g, blk = self._table(x.device)
        y = torch.empty((B, self.total), device=x.device, dtype=F32)
        _lib.call("fmd_grouped_linear", _p(x), B, self.I, _p(g), _p(blk), blk.shape[0], int(self.in_silu), _p(y),
                  self.total, stream())
        return y

    def backward(self, x, dy, dx=None, dx_acc=False):
        for l in self.linears:
            if l.weight.grad is None:
                l.weight.grad = torch.zeros_like(l.weight)
            if l.bias is not None and l.bias.grad is None:
                l.bias.grad = torch.zeros_like(l.bias)
        B = x.shape[0]
        g, blk = self._table(x.device)
        nws = int(_lib.lib().fmd_grouped_linear_bwd_workspace(B, self.I, blk.shape[0]))
        ws = torch.empty((nws,), device=x.device, dtype=F32)
        _lib.call("fmd_grouped_linear_bwd", _p(x.contiguous()), B, self.I, _p(g), _p(blk), blk.shape[0],
                  int(self.in_silu), _p(dy), self.total, _p(dx), int(dx_acc), _p(ws), stream())


def silu_bwd(x, dy):
    dx = torch.empty_like(x)
    _lib.call("fmd_silu_bwd_f32", _p(x), _p(dy), _p(dx), x.numel(), stream())
    return dx


# softmax attention: MFMA kernels over canonical [B*heads][rows][head_pad] planes (csrc/attention_mfma.hip)


def _attn_planes(B, heads, rows, dh, dev):
    D = int(_lib.lib().fmd_attn_head_pad(dh))
    if D < 0:
        raise ValueError(f"attention head dim {dh} > 64 is not supported")
    return torch.empty((B * heads, rows, D), device=dev, dtype=BF16)


def _attn_pack(src_q, src_kv, B, Tq, Tk, heads, dh, raw, cross, which0, which1, cq, ck=None, cv=None):
    _lib.call("fmd_attn_pack", _p(src_q), _p(src_kv), B, Tq, Tk, heads, dh, int(raw), int(cross), which0, which1,
              _p(cq), _p(ck), _p(cv), stream())


class AttnSaved:
    """What the MFMA softmax attention forward keeps for its backward: lse [B][heads][Tq] and the canonical
    q, k, v, o planes (so the backward packs only dout)."""
    __slots__ = ("lse", "cq", "ck", "cv", "co")

    def __init__(self, lse, cq, ck, cv, co):
        self.lse, self.cq, self.ck, self.cv, self.co = lse, cq, ck, cv, co


def _attn_softmax_fwd(src_q, src_kv, B, Tq, Tk, heads, dh, raw, cross):
    dev = src_q.device
    cq, ck, cv = _attn_planes(B, heads, Tq, dh, dev), _attn_planes(B, heads, Tk, dh, dev), _attn_planes(B, heads, Tk, dh, dev)
    _attn_pack(src_q, src_kv, B, Tq, Tk, heads, dh, raw, cross, 0, 2, cq, ck, cv)
    co = torch.empty_like(cq)
    lse = torch.empty((B, heads, Tq), device=dev, dtype=F32)
    _lib.call("fmd_attn_mfma_fwd", _p(cq), _p(ck), _p(cv), B * heads, Tq, Tk, dh, _p(co), _p(lse), stream())
    o = torch.empty((B, Tq, heads * dh), device=dev, dtype=BF16)
    _lib.call("fmd_attn_unpack", _p(co), None, None, B, Tq, Tk, heads, dh, int(raw), int(cross), 3, 3, _p(o), None,
              stream())
    return o, AttnSaved(lse, cq, ck, cv, co)


def _attn_softmax_bwd(src_q, src_kv, o, dout, saved, B, Tq, Tk, heads, dh, raw, cross, dst_q, dst_kv):
    """``saved``: the forward's AttnSaved, or a bare lse tensor (q, k, v, o are then packed again)."""
    dev = src_q.device
    if isinstance(saved, AttnSaved):
        lse, cq, ck, cv, co = saved.lse, saved.cq, saved.ck, saved.cv, saved.co
    else:
        lse = saved
        cq, ck = _attn_planes(B, heads, Tq, dh, dev), _attn_planes(B, heads, Tk, dh, dev)
        cv = _attn_planes(B, heads, Tk, dh, dev)
        _attn_pack(src_q, src_kv, B, Tq, Tk, heads, dh, raw, cross, 0, 2, cq, ck, cv)
        co = torch.empty_like(cq)
        _attn_pack(o, o, B, Tq, Tk, heads, dh, raw, cross, 3, 3, co)
    cdo = torch.empty_like(cq)
    _attn_pack(dout.contiguous(), dout, B, Tq, Tk, heads, dh, raw, cross, 3, 3, cdo)
    cdq, cdk, cdv = torch.empty_like(cq), torch.empty_like(ck), torch.empty_like(cv)
    delta = torch.empty_like(lse)
    _lib.call("fmd_attn_mfma_bwd", _p(cq), _p(ck), _p(cv), _p(co), _p(cdo), _p(lse), _p(delta), B * heads, Tq, Tk,
              dh, _p(cdq), _p(cdk), _p(cdv), stream())
    _lib.call("fmd_attn_unpack", _p(cdq), _p(cdk), _p(cdv), B, Tq, Tk, heads, dh, int(raw), int(cross), 0, 2,
              _p(dst_q), _p(dst_kv), stream())


def attention_fwd(qkv, T, heads, dh, raw):
    """Softmax self-attention over the fused qkv projection [B][T][3*inner] -> (o [B][T][inner], lse)."""
    return _attn_softmax_fwd(qkv, qkv, qkv.shape[0], T, T, heads, dh, raw, 0)


def _la_workspace(B, heads, dev):
    return torch.empty((int(_lib.lib().fmd_linear_attention_workspace(B, heads)),), device=dev, dtype=F32)


def linear_attention_fwd(qkv, T, heads, dh, raw, eps=1e-6):
    """LinearQKVAttention over the fused qkv projection (csrc/attention.hip); returns (o, state)."""
    B = qkv.shape[0]
    o = torch.empty((B, T, heads * dh), device=qkv.device, dtype=BF16)
    state = torch.empty((int(_lib.lib().fmd_linear_attention_state(B, heads)),), device=qkv.device, dtype=F32)
    _lib.call("fmd_linear_attention_fwd", _p(qkv), B, T, heads, dh, int(raw), float(eps), _p(o), _p(state),
              _p(_la_workspace(B, heads, qkv.device)), stream())
    return o, state


def linear_attention_bwd(qkv, dout, state, T, heads, dh, raw, eps=1e-6):
    B = qkv.shape[0]
    dqkv = torch.empty_like(qkv)
    _lib.call("fmd_linear_attention_bwd", _p(qkv), _p(dout), _p(state), _p(_la_workspace(B, heads, qkv.device)), B, T,
              heads, dh, int(raw), float(eps), _p(dqkv), stream())
    return dqkv


def cross_attention_fwd(q, kv, Tq, Tk, heads, dh, linear_eps=None, raw=1):
    """SpatialCrossAttention core (csrc/attention.hip): q [B][Tq][inner], kv [B][Tk][2*inner] -> (o, saved),
    softmax (saved = lse) or LinearQKVAttention when ``linear_eps`` is given (saved = state)."""
    B = q.shape[0]
    if linear_eps is None:
        return _attn_softmax_fwd(q, kv, B, Tq, Tk, heads, dh, raw, 1)
    o = torch.empty((B, Tq, heads * dh), device=q.device, dtype=BF16)
    saved = torch.empty((int(_lib.lib().fmd_linear_attention_state(B, heads)),), device=q.device, dtype=F32)
    ws = _la_workspace(B, heads, q.device)
    _lib.call("fmd_cross_attention_fwd", _p(q), _p(kv), B, Tq, Tk, heads, dh, int(raw), 1, float(linear_eps),
              _p(o), _p(saved), _p(ws), stream())
    return o, saved


def cross_attention_bwd(q, kv, o, dout, saved, Tq, Tk, heads, dh, linear_eps=None, raw=1):
    B = q.shape[0]
    dq, dkv = torch.empty_like(q), torch.empty_like(kv)
    if linear_eps is None:
        _attn_softmax_bwd(q, kv, o, dout, saved, B, Tq, Tk, heads, dh, raw, 1, dq, dkv)
        return dq, dkv
    _lib.call("fmd_cross_attention_bwd", _p(q), _p(kv), _p(o), _p(dout), _p(saved), _p(_la_workspace(B, heads, q.device)),
              B, Tq, Tk, heads, dh, int(raw), 1, float(linear_eps), _p(dq), _p(dkv), stream())
    return dq, dkv


def context_norm_fwd(ctx, tok_major, groups, eps, gamma, beta, Cpad):
    """GroupNorm of a cross-attention context (fp32 [N][C][T] or token-major [N][T][C]) -> bf16 [N][T][1][Cpad]
    (a 1-wide NHWC plane for the kv 1x1 conv) and the (mean, rstd) table."""
    _need_cuda(ctx, "context_norm_fwd")
    N = ctx.shape[0]
    C, T = (ctx.shape[2], ctx.shape[1]) if tok_major else (ctx.shape[1], ctx.shape[2])
    out = torch.empty((N, T, 1, Cpad), device=ctx.device, dtype=BF16)
    mr = torch.empty((N, groups, 2), device=ctx.device, dtype=F32)
    _lib.call("fmd_context_norm_fwd", _p(ctx), N, C, T, int(tok_major), groups, float(eps), _p(gamma), _p(beta), Cpad,
              _p(out), _p(mr), stream())
    return out, mr


def context_norm_bwd(ctx, tok_major, groups, mr, dout, dgamma, dbeta):
    N = ctx.shape[0]
    C, T = (ctx.shape[2], ctx.shape[1]) if tok_major else (ctx.shape[1], ctx.shape[2])
    _lib.call("fmd_context_norm_bwd", _p(ctx), N, C, T, int(tok_major), groups, _p(mr), _p(dout), dout.shape[-1],
              _p(dgamma), _p(dbeta), stream())


def attention_bwd(qkv, o, dout, lse, T, heads, dh, raw):
    dqkv = torch.empty_like(qkv)
    _attn_softmax_bwd(qkv, qkv, o, dout, lse, qkv.shape[0], T, T, heads, dh, raw, 0, dqkv, dqkv)
    return dqkv


def _dhw(t):
    """(N, D, H, W, C) view extents of an N(D)(H)WC tensor (missing leading spatial dims = 1)."""
    N, C = t.shape[0], t.shape[-1]
    sp = list(t.shape[1:-1])
    sp = [1] * (3 - len(sp)) + sp
    return N, sp, C


def resample2(src, dst, up: bool, scale: float, acc: bool = False, factors=None):
    """dst (+)= avg/sum-pool-by-2 (up=False) or nearest-x2 (up=True) of src; ``factors`` (per spatial dim, 1 or
    2; default every dim 2) -- a 1-D signal as an (L, 1) image resamples its first dim only."""
    _need_cuda(src, "resample2")
    N, s_sp, C = _dhw(src)
    _, d_sp, _ = _dhw(dst)
    lo, hi = (s_sp, d_sp) if up else (d_sp, s_sp)
    nd = src.dim() - 2
    f = [1] * (3 - nd) + (list(factors) if factors is not None else [2] * nd)
    _lib.call("fmd_resample2", _p(src), N, lo[0], lo[1], lo[2], hi[0], hi[1], hi[2], C, f[0], f[1], f[2], int(up),
              float(scale), _p(dst), int(acc), stream())


def sum_pool2(src, dst, acc):
    N, H, W, Cc = dst.shape
    _lib.call("fmd_sum_pool2", _p(src), N, H, W, Cc, _p(dst), int(acc), stream())


def sum_pool2_3d(src, dst, acc=False):
    """dst (+)= 2x2x2 block sums of src (bf16 NDHWC): the data gradient of a nearest-x2 3-D upsample."""
    N, D, H, W, Cc = dst.shape
    _lib.call("fmd_sum_pool2_3d", _p(src), N, D, H, W, Cc, _p(dst), int(acc), stream())


def add_(dst, a):
    _lib.call("fmd_add_bf16", _p(a), _p(dst), dst.numel(), stream())


def noise_prepare(x0, noise, ca, cb, cond, Cpad, out=None):
    N, Cx = noise.shape[:2]
    HW = noise[0, 0].numel()
    Cc = cond.shape[1] if cond is not None else 0
    if out is None:
        out = torch.empty((N, *noise.shape[2:], Cpad), device=noise.device, dtype=BF16)
    _lib.call("fmd_noise_prepare", _p(x0), _p(noise), _p(ca), _p(cb), _p(cond), N, HW, Cx, Cc, Cpad, _p(out),
              stream())
    return out


def mse(pred_nhwc, ta, tb, tb_sign, grad_scale, loss, partial, dpred=None):
    N = pred_nhwc.shape[0]
    Kpad = pred_nhwc.shape[-1]
    Cx = ta.shape[1]
    HW = ta[0, 0].numel()
    _lib.call("fmd_mse", _p(pred_nhwc), Kpad, _p(ta), _p(tb), float(tb_sign), N, Cx, HW, float(grad_scale),
              _p(partial), partial.numel(), _p(loss), _p(dpred), stream())


def adamw_sched(p, g, m, v, step_ctr, base_lr, warmup, total, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0,
                grad_scale=1.0, ema=None, ema_decay=0.0, ema_warmup=True):
    """``ema``: a flat fp32 buffer like ``p``; then the same launch also moves it towards the new parameters
    (fmd_adamw_sched_ema, decay ``ema_decay`` in [0, 1), warmed up as min(decay, (1 + s) / (10 + s)) if
    ``ema_warmup``)."""
    if ema is None:
        _lib.call("fmd_adamw_sched", _p(p), _p(g), _p(m), _p(v), p.numel(), _p(step_ctr), float(base_lr), int(warmup),
                  int(total), float(beta1), float(beta2), float(eps), float(wd), float(grad_scale), stream())
        return
    if ema.dtype != F32 or not ema.is_contiguous() or ema.numel() != p.numel() or ema.device != p.device:
        raise ValueError("adamw_sched: ema must be a contiguous fp32 buffer of p's size on p's device")
    _lib.call("fmd_adamw_sched_ema", _p(p), _p(g), _p(m), _p(v), _p(ema), p.numel(), _p(step_ctr), float(base_lr),
              int(warmup), int(total), float(beta1), float(beta2), float(eps), float(wd), float(grad_scale),
              float(ema_decay), int(bool(ema_warmup)), stream())


def counter_add(ctr, v=1):
    _lib.call("fmd_counter_add", _p(ctr), int(v), stream())


def fill_from_table(table, index, out):
    _lib.call("fmd_fill_from_table", _p(table), _p(index), _p(out), out.numel(), stream())


def lincomb(out, inputs, coefs):
    """out = sum_k coefs[k] * inputs[k] (fp32 device tensors of out's size; out may be one of the inputs)."""
    _need_cuda(out, "lincomb")
    if not 1 <= len(inputs) <= _lib.LINCOMB_MAX or len(inputs) != len(coefs):
        raise ValueError("lincomb: 1..6 inputs, one coefficient each")
    d = _lib.LincombDesc()
    d.out, d.nin, d.n = _p(out), len(inputs), out.numel()
    for k, (t, c) in enumerate(zip(inputs, coefs)):
        if t.dtype != F32 or not t.is_contiguous() or t.numel() != out.numel():
            raise ValueError("lincomb: contiguous fp32 inputs of the output's size")
        d.in_[k] = _p(t)
        d.c[k] = float(c)
    _lib.call("fmd_lincomb", C.byref(d), stream())
    return out


def gather_row(table, index, out):
    """out = table[index[0]] (row of ``out.numel()`` fp32 elements; ``index`` is a device int32 counter)."""
    _lib.call("fmd_gather_row", _p(table), _p(index), out.numel(), _p(out), stream())


def flow_euler(x, v_nhwc, sigmas, index, cond, next_inp):
    N, Cx = x.shape[:2]
    HW = x[0, 0].numel()
    Cc = cond.shape[1] if cond is not None else 0
    _lib.call("fmd_flow_euler", _p(x), _p(v_nhwc), v_nhwc.shape[-1], _p(sigmas), _p(index), N, Cx, HW, _p(cond), Cc,
              next_inp.shape[-1] if next_inp is not None else 0, _p(next_inp), stream())


def affine_channels(x, C: int, scale: float, shift: float):
    """y = x (channels-last bf16) with channels [0, C) mapped to scale * x + shift (fmd_affine_channels)."""
    _need_cuda(x, "affine_channels")
    y = torch.empty_like(x)
    _lib.call("fmd_affine_channels", _p(x), int(C), x.shape[-1], x.numel() // x.shape[-1], float(scale), float(shift),
              _p(y), stream())
    return y


def ddpm_step(x, eps_nhwc, coef, index, noise, cond, next_inp, noise_base=-1):
    """``noise``: one [N,Cx,*S] buffer (``noise_base`` < 0) or a per-step table [rows][N,Cx,*S] whose row 0 is step
    ``noise_base`` (fmd_ddpm_step)."""
    N, Cx = x.shape[:2]
    HW = x[0, 0].numel()
    Cc = cond.shape[1] if cond is not None else 0
    _lib.call("fmd_ddpm_step", _p(x), _p(eps_nhwc), eps_nhwc.shape[-1], _p(coef), _p(index), _p(noise),
              int(noise_base), N, Cx, HW,
              _p(cond), Cc, next_inp.shape[-1] if next_inp is not None else 0, _p(next_inp), stream())


def sched_step(x, eps_nhwc, ring, last, coef, index, cond, next_inp):
    """One table-driven DPM-Solver / UniPC step (fmd_sched_step): x [N,Cx,*S] fp32 updated in place, ring = 4
    fp32 history buffers of x's shape, last (UniPC corrector state) or None, coef [steps][12] fp32."""
    N, Cx = x.shape[:2]
    d = _lib.SchedStepDesc()
    d.x, d.eps, d.last, d.coef, d.index = _p(x), _p(eps_nhwc), _p(last), _p(coef), _p(index)
    for k in range(4):
        d.ring[k] = _p(ring[k])
    d.N, d.Cx, d.HW, d.Kpad = N, Cx, x[0, 0].numel(), eps_nhwc.shape[-1]
    d.cond, d.Cc = _p(cond), cond.shape[1] if cond is not None else 0
    d.Cpad, d.next = (next_inp.shape[-1], _p(next_inp)) if next_inp is not None else (0, None)
    _lib.call("fmd_sched_step", C.byref(d), stream())


def adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step):
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    _lib.call("fmd_adamw", _p(p), _p(g), _p(m), _p(v), p.numel(), float(lr), float(beta1), float(beta2), float(eps),
              float(wd), float(bc1), float(bc2), stream())


# ------------------------------------------------------------------ vector quantizer (csrc/vq.hip)
@dataclass
class VQOut:
    """Outputs of ``vq_quantize``; ``vq_loss`` / ``perplexity`` / ``mse`` are 0-dim views of one device tensor."""
    zq: torch.Tensor        # fp32 channels-first [N, D, *spatial] = z + (q - z)
    zq_nhwc: torch.Tensor   # bf16 [N, *spatial, Cpad], channels >= D zero: the decoder's operand
    vq_loss: torch.Tensor
    perplexity: torch.Tensor
    codes: torch.Tensor     # int64 [N, *spatial]
    hist: torch.Tensor      # int32 [K]
    mse: torch.Tensor


_vq_planes: list = []   # (weakref(codebook), _version, data_ptr, (Eh, El, hn)), most recent last
_VQ_PLANES_MAX = 8


def vq_plan(M: int, K: int, D: int) -> _lib.VqPlan:
    plan = _lib.VqPlan()
    if _lib.lib().fmd_vq_plan(M, K, D, C.byref(plan)) != 0:
        raise NotImplementedError(f"vq_quantize: M={M}, K={K}, D={D} is not supported (1 <= D <= 256)")
    return plan


def vq_codebook_planes(codebook: torch.Tensor):
    """bf16 planes E_h, E_l [Kpad][Dpad] and hn = |e|^2 / 2 [Kpad] of an fp32 codebook [K][D], cached per tensor
    object and keyed on its ``(_version, data_ptr)`` like the VAE engine's folded output conv.

    The key sees torch's own in-place writes only.  A codebook rewritten through a raw pointer (as the fused
    optimizer kernels write parameters) keeps its ``_version``, and the planes are built on the stream current at
    the first call.  ``vq_ema_update`` is the one kernel path that writes a codebook: it rewrites these planes in
    the same launch, bumps ``embedding._version`` and moves this entry's key along with it."""
    import weakref
    ver, ptr = codebook._version, codebook.data_ptr()
    _vq_planes[:] = [e for e in _vq_planes if e[0]() is not None]
    for e in _vq_planes:
        if e[0]() is codebook and e[1] == ver and e[2] == ptr:
            return e[3]
    K, D = codebook.shape
    plan = vq_plan(1, K, D)
    dev = codebook.device
    Eh = torch.empty((plan.Kpad, plan.Dpad), device=dev, dtype=BF16)
    El = torch.empty((plan.Kpad, plan.Dpad), device=dev, dtype=BF16)
    hn = torch.empty((plan.Kpad,), device=dev, dtype=F32)
    _lib.call("fmd_vq_prep", _p(codebook), K, D, _p(Eh), _p(El), _p(hn), stream())
    _vq_planes[:] = [e for e in _vq_planes if e[0]() is not codebook][-(_VQ_PLANES_MAX - 1):]
    _vq_planes.append((weakref.ref(codebook), ver, ptr, (Eh, El, hn)))
    return Eh, El, hn


def vq_quantize(z_flat, D: int, codebook, beta: float, classic: bool, plan_out=None, *, eps: float = 1e-5,
                Cpad: Optional[int] = None, out: Optional[dict] = None) -> VQOut:
    """Nearest-code quantisation of ``z_flat`` (fp32 channels-last ``[N, *spatial, ldz]``, the first ``D``
    channels of every vector) against the fp32 ``codebook`` [K][D]; see ``VQOut``.  ``plan_out``: a list that
    receives the launch plan (``_lib.VqPlan``).  ``out``: optional preallocated ``zq`` / ``zq_nhwc`` / ``codes`` /
    ``hist`` (zeroed) / ``stats`` tensors.  Nothing synchronises with the host."""
    _need_cuda(z_flat, "vq_quantize")
    _need_cuda(codebook, "vq_quantize")
    if z_flat.dtype != F32 or codebook.dtype != F32 or not z_flat.is_contiguous() or not codebook.is_contiguous():
        raise RuntimeError("vq_quantize: contiguous fp32 tensors")
    if z_flat.dim() < 2 or codebook.dim() != 2 or codebook.shape[1] != D or z_flat.shape[-1] < D:
        raise RuntimeError(f"vq_quantize: z [..., >= {D}] against a codebook [K, {D}], got {tuple(z_flat.shape)} "
                           f"and {tuple(codebook.shape)}")
    N, sp, ldz = z_flat.shape[0], tuple(z_flat.shape[1:-1]), z_flat.shape[-1]
    HW = 1
    for v in sp:
        HW *= v
    M, K = N * HW, codebook.shape[0]
    plan = vq_plan(M, K, D)
    if plan_out is not None:
        plan_out.append(plan)
    dev = z_flat.device
    Eh, El, hn = vq_codebook_planes(codebook)
    Cpad = Cpad or max(8, -(-D // 8) * 8)
    out = out or {}
    nslab = -(-M // plan.finalize_rows)
    ws = torch.empty((int(_lib.lib().fmd_vq_workspace(M, K, D)),), device=dev, dtype=torch.uint8)
    codes = out["codes"] if "codes" in out else torch.empty((N, *sp), device=dev, dtype=torch.int64)
    zq = out["zq"] if "zq" in out else torch.empty((N, D, *sp), device=dev, dtype=F32)
    zq_nhwc = out["zq_nhwc"] if "zq_nhwc" in out else torch.empty((N, *sp, Cpad), device=dev, dtype=BF16)
    hist = out["hist"] if "hist" in out else torch.zeros((K,), device=dev, dtype=torch.int32)
    stats = out["stats"] if "stats" in out else torch.empty((3,), device=dev, dtype=F32)
    if (tuple(codes.shape) != (N, *sp) or tuple(zq.shape) != (N, D, *sp) or tuple(zq_nhwc.shape) != (N, *sp, Cpad)
            or hist.numel() != K or stats.numel() != 3
            or not all(t.is_contiguous() for t in (codes, zq, zq_nhwc, hist, stats))):
        raise RuntimeError("vq_quantize: preallocated outputs of the wrong shape")
    slab = torch.empty((nslab,), device=dev, dtype=F32)
    s = stream()
    _lib.call("fmd_vq_argmin", _p(z_flat), ldz, M, K, D, _p(Eh), _p(El), _p(hn), _p(ws), s)
    _lib.call("fmd_vq_finalize", _p(z_flat), ldz, M, HW, K, D, _p(codebook), _p(ws), _p(codes), _p(zq), _p(zq_nhwc),
              Cpad, _p(slab), _p(hist), s)
    _lib.call("fmd_vq_stats", _p(slab), nslab, _p(hist), K, M, D, float(beta), int(bool(classic)), float(eps),
              _p(stats), s)
    return VQOut(zq, zq_nhwc, stats[0], stats[1], codes, hist, stats[2])


# ------------------------------------------------------------------ quantizer training (csrc/vq_train.hip)
def _vq_rows(z_flat, D: int, what: str):
    _need_cuda(z_flat, what)
    if z_flat.dtype != F32 or not z_flat.is_contiguous() or z_flat.dim() < 2 or z_flat.shape[-1] < D:
        raise RuntimeError(f"{what}: contiguous fp32 rows [..., >= {D}], got {tuple(z_flat.shape)} {z_flat.dtype}")
    return z_flat.numel() // z_flat.shape[-1], z_flat.shape[-1]


def _vq_state(t, shape, what: str, dtype=F32):
    _need_cuda(t, what)
    if t.dtype != dtype or not t.is_contiguous() or tuple(t.shape) != tuple(shape):
        raise RuntimeError(f"{what}: expected a contiguous {dtype} tensor {tuple(shape)}, got {tuple(t.shape)} {t.dtype}")


def vq_train_plan(M: int, K: int, D: int):
    """(codes per workgroup, grid) of the segmented-sum launch."""
    cpw, grid = C.c_int32(), C.c_int32()
    if _lib.lib().fmd_vq_train_plan(M, K, D, C.byref(cpw), C.byref(grid)) != 0:
        raise NotImplementedError(f"vq training kernels: M={M}, K={K}, D={D} is not supported (1 <= D <= 256)")
    return cpw.value, grid.value


def vq_ema_update(z_flat, D: int, codes, hist, embedding, ema_cluster_size, ema_w, decay: float, eps: float,
                  nsum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The EMA codebook update of ``VectorQuantizerEMA`` (reference ``codebook.py:120-129``), in place on
    ``ema_cluster_size`` [K], ``ema_w`` [K, D] and ``embedding`` [K, D], from the latent rows ``z_flat`` (fp32
    channels-last, the first ``D`` channels), the ``codes`` and the histogram ``hist`` of the ``vq_quantize`` call
    that used ``embedding``.  Deterministic (fp64 segment sums in row order, no atomics), nothing synchronises.

    The planes ``vq_codebook_planes(embedding)`` caches are rewritten in the same launch and their cache key
    follows ``embedding._version``, which is bumped: the next ``vq_quantize`` reads the new codebook, also after
    a graph replay of this call (the replay rewrites the cached buffers; the key it was captured with holds).
    Returns ``nsum``: the fp64 sum of the new cluster sizes, a one-element device tensor."""
    M, ldz = _vq_rows(z_flat, D, "vq_ema_update")
    K = embedding.shape[0]
    _vq_state(embedding, (K, D), "vq_ema_update")
    _vq_state(ema_w, (K, D), "vq_ema_update")
    _vq_state(ema_cluster_size, (K,), "vq_ema_update")
    _vq_state(hist, (K,), "vq_ema_update", torch.int32)
    _need_cuda(codes, "vq_ema_update")
    if codes.dtype != torch.int64 or not codes.is_contiguous() or codes.numel() != M:
        raise RuntimeError(f"vq_ema_update: codes must be contiguous int64 with {M} elements")
    vq_train_plan(M, K, D)
    if nsum is None:
        nsum = torch.empty((1,), device=z_flat.device, dtype=torch.float64)
    Eh, El, hn = vq_codebook_planes(embedding)
    omd = 1 - decay   # in double, as the reference's Python does; rounded to fp32 at the call
    _lib.call("fmd_vq_ema_update", _p(z_flat), ldz, M, K, D, _p(codes), _p(hist), float(decay), float(omd), float(eps),
              float(K * eps), _p(ema_cluster_size), _p(ema_w), _p(embedding), _p(Eh), _p(El), _p(hn), _p(nsum),
              stream())
    for t in (embedding, ema_w, ema_cluster_size):
        torch.autograd.graph.increment_version(t)
    for i, e in enumerate(_vq_planes):
        if e[0]() is embedding:
            _vq_planes[i] = (e[0], embedding._version, embedding.data_ptr(), e[3])
    return nsum


_vq_consts: dict = {}


def _vq_const(dev, v: float) -> torch.Tensor:
    key = (str(dev), v)
    if key not in _vq_consts:
        _vq_consts[key] = torch.full((1,), v, device=dev, dtype=F32)
    return _vq_consts[key]


def vq_backward(z_flat, D: int, codes, codebook, g_zq, g_loss, c: float, *, out=None) -> torch.Tensor:
    """Gradient of the quantizer to its input: ``dz = g_zq + g_loss * c * (2 / (M D)) * (z - q)`` on the first
    ``D`` channels, zero on the padding; ``c`` is beta for the EMA quantizer and beta - 1 for the classic one.
    ``z_flat`` / ``g_zq`` (or None for zero) / the result are fp32 channels-last with their own row strides;
    ``g_loss`` is a one-element device tensor or None (zero); ``codebook`` None: ``z_flat`` already holds z - q."""
    M, ldz = _vq_rows(z_flat, D, "vq_backward")
    dev = z_flat.device
    K, ldg = 1, 0
    if codebook is not None:
        K = codebook.shape[0]
        _vq_state(codebook, (K, D), "vq_backward")
        _need_cuda(codes, "vq_backward")
        if codes.dtype != torch.int64 or not codes.is_contiguous() or codes.numel() != M:
            raise RuntimeError(f"vq_backward: codes must be contiguous int64 with {M} elements")
    if g_zq is not None:
        Mg, ldg = _vq_rows(g_zq, D, "vq_backward")
        if Mg != M:
            raise RuntimeError(f"vq_backward: g_zq has {Mg} rows, z has {M}")
    if g_loss is None:
        g_loss = _vq_const(dev, 0.0)
    _need_cuda(g_loss, "vq_backward")
    if g_loss.dtype != F32 or g_loss.numel() != 1:
        raise RuntimeError("vq_backward: g_loss must be one fp32 element")
    dz = torch.empty_like(z_flat) if out is None else out
    Mo, lddz = _vq_rows(dz, D, "vq_backward")
    if Mo != M:
        raise RuntimeError("vq_backward: preallocated output of the wrong shape")
    _lib.call("fmd_vq_backward", _p(z_flat), ldz, M, K, D, _p(codes) if codebook is not None else None, _p(codebook),
              _p(g_zq), ldg, _p(g_loss), float(c), float(2.0 / (M * D)), _p(dz), lddz, stream())
    return dz


def vq_join_bwd(g_zq, D: int, z_flat, codes, codebook, g_loss, c: float, *, ld_out: Optional[int] = None,
                out=None) -> torch.Tensor:
    """The latent join of the VQVAE backward in one launch: ``vq_backward``'s value
    ``g_zq + g_loss * c * (2 / (M D)) * (z - q)``, element for element, rounded once (to nearest even) to the bf16
    channels-last operand ``[N, *spatial, ld_out]`` of the encoder head's backward; channels ``D .. ld_out - 1`` are
    exact zeros (default ``ld_out``: D rounded up to 8).

    ``g_zq``: the 1x1 data gradient as the conv left it, bf16 or fp32 channels-last ``[N, *spatial, >= D]`` with a
    row stride that is a multiple of 8, or None (zero).  ``z_flat`` / ``codes`` / ``codebook`` as for
    ``vq_backward`` (``codebook`` None: ``z_flat`` holds the saved residual z - q).  ``g_loss``: a one-element fp32
    device tensor or None (zero).  Padding channels of the inputs are never read.  Nothing synchronises."""
    what = "vq_join_bwd"
    M, ldz = _vq_rows(z_flat, D, what)
    dev = z_flat.device
    if not 1 <= D <= 256:
        raise ValueError(f"{what}: 1 <= D <= 256, got {D}")
    K = 1
    if codebook is not None:
        K = codebook.shape[0]
        _vq_state(codebook, (K, D), what)
        _need_cuda(codes, what)
        if codes.dtype != torch.int64 or not codes.is_contiguous() or codes.numel() != M:
            raise RuntimeError(f"{what}: codes must be contiguous int64 with {M} elements")
    ldg, g_f32 = 0, 0
    if g_zq is not None:
        _need_cuda(g_zq, what)
        if g_zq.dtype not in (BF16, F32) or not g_zq.is_contiguous() or g_zq.dim() < 2:
            raise RuntimeError(f"{what}: g_zq must be contiguous bf16 or fp32 rows, got {g_zq.dtype} "
                               f"{tuple(g_zq.shape)}")
        ldg, g_f32 = int(g_zq.shape[-1]), int(g_zq.dtype == F32)
        if ldg < D or ldg % 8 or g_zq.numel() // ldg != M or g_zq.data_ptr() % 16:
            raise ValueError(f"{what}: g_zq needs {M} 16-byte aligned rows with a stride >= {D} that is a multiple "
                             f"of 8, got {tuple(g_zq.shape)}")
    if g_loss is not None:
        _need_cuda(g_loss, what)
        if g_loss.dtype != F32 or g_loss.numel() != 1:
            raise RuntimeError(f"{what}: g_loss must be one fp32 element")
    if out is None:
        ld_out = int(ld_out or max(8, -(-D // 8) * 8))
        if ld_out < D or ld_out % 8:
            raise ValueError(f"{what}: ld_out {ld_out} must be a multiple of 8 and >= {D}")
        out = torch.empty((*z_flat.shape[:-1], ld_out), device=dev, dtype=BF16)
    else:
        _need_cuda(out, what)
        ld_out = int(out.shape[-1])
        if (out.dtype != BF16 or not out.is_contiguous() or ld_out < D or ld_out % 8 or out.numel() // ld_out != M
                or out.data_ptr() % 16):
            raise ValueError(f"{what}: out must be contiguous bf16 with {M} rows and a stride >= {D} that is a "
                             f"multiple of 8, got {out.dtype} {tuple(out.shape)}")
    _lib.call("fmd_vq_join_bwd", _p(z_flat), ldz, M, K, D, _p(codes) if codebook is not None else None, _p(codebook),
              _p(g_zq), g_f32, ldg, _p(g_loss), float(c), float(2.0 / (M * D)), _p(out), ld_out, stream())
    return out


def vq_residual(z_flat, D: int, codes, codebook) -> torch.Tensor:
    """``z - codebook[codes]`` rounded once (padding channels zero): what ``vq_backward`` needs of a codebook that
    is about to be overwritten by ``vq_ema_update``.  ``fma(1, z - q, 0)`` is exact, so a later
    ``vq_backward(residual, ..., codebook=None, ...)`` gives the bits of the direct call."""
    M, _ = _vq_rows(z_flat, D, "vq_residual")
    r = torch.empty_like(z_flat)
    _lib.call("fmd_vq_backward", _p(z_flat), z_flat.shape[-1], M, codebook.shape[0], D, _p(codes), _p(codebook), None,
              0, _p(_vq_const(z_flat.device, 1.0)), 1.0, 1.0, _p(r), r.shape[-1], stream())
    return r


def vq_codebook_grad(z_flat, D: int, codes, hist, codebook, g_loss) -> torch.Tensor:
    """``g_loss * (2 / (M D)) * (n_k e_k - S_k)`` [K, D]: the codebook term of the VQ-VAE loss, from the same
    segmented sums as the EMA update (an opt-in deviation: the reference sends the codebook no gradient)."""
    M, ldz = _vq_rows(z_flat, D, "vq_codebook_grad")
    K = codebook.shape[0]
    _vq_state(codebook, (K, D), "vq_codebook_grad")
    _vq_state(hist, (K,), "vq_codebook_grad", torch.int32)
    _need_cuda(codes, "vq_codebook_grad")
    if codes.dtype != torch.int64 or not codes.is_contiguous() or codes.numel() != M:
        raise RuntimeError(f"vq_codebook_grad: codes must be contiguous int64 with {M} elements")
    vq_train_plan(M, K, D)
    if g_loss is None:
        g_loss = _vq_const(z_flat.device, 0.0)
    dE = torch.empty_like(codebook)
    _lib.call("fmd_vq_codebook_grad", _p(z_flat), ldz, M, K, D, _p(codes), _p(hist), _p(codebook), _p(g_loss),
              float(2.0 / (M * D)), _p(dE), stream())
    return dE


# ------------------------------------------------------------------ image metrics (csrc/metrics.hip)
@dataclass
class ImageMetrics:
    """Per-image outputs of ``image_metrics``: fp64 ``[N]`` views of one ``[3, N]`` device tensor (``stacked``)."""
    mse: torch.Tensor
    psnr: torch.Tensor
    ssim: torch.Tensor
    stacked: torch.Tensor


def image_metrics(gen: torch.Tensor, tgt: torch.Tensor, clamp: bool = True, *, out: Optional[torch.Tensor] = None,
                  ws: Optional[torch.Tensor] = None) -> ImageMetrics:
    """MSE, PSNR and SSIM (skimage's defaults: 7-wide uniform window, sample covariance, data_range 1) of every
    image of two fp32 channels-first batches ``[N, C, H, W]`` or ``[N, C, D, H, W]``, all in fp64 on the device.
    ``clamp`` clamps both to [0, 1] first (the diffusion evaluate); the autoencoder evaluate passes False.
    ``[N, C, L]`` signals get ``mse`` and ``psnr`` and NaN in ``ssim`` (the reference skips channels with fewer
    than two dimensions).  ``out``: optional fp64 ``[3, N]``; ``ws``: optional uint8 workspace of at least
    ``fmd_image_metrics_workspace`` bytes.  Nothing synchronises with the host."""
    if tuple(gen.shape) != tuple(tgt.shape):
        raise ValueError(f"image_metrics: shape mismatch, {tuple(gen.shape)} against {tuple(tgt.shape)}")
    if gen.dim() >= 6:
        raise NotImplementedError(f"image_metrics: {gen.dim() - 2} spatial axes (1 to 3 are built)")
    if gen.dim() < 3:
        raise ValueError(f"image_metrics: channels-first batches [N, C, *spatial], got {tuple(gen.shape)}")
    N, Cc = int(gen.shape[0]), int(gen.shape[1])
    sp = tuple(int(v) for v in gen.shape[2:])
    if len(sp) >= 2 and min(sp) < 7:
        raise ValueError("win_size exceeds image extent. Either ensure that your images are at least 7x7; or pass "
                         f"win_size explicitly (image_metrics has the 7-wide window only); got {sp}")
    if N < 1 or Cc < 1 or min(sp) < 1:
        raise ValueError(f"image_metrics: empty batch {tuple(gen.shape)}")
    _need_cuda(gen, "image_metrics")
    _need_cuda(tgt, "image_metrics")
    if gen.dtype != F32 or tgt.dtype != F32 or not gen.is_contiguous() or not tgt.is_contiguous():
        raise RuntimeError("image_metrics: contiguous fp32 tensors")
    D, H, W = (0,) * (3 - len(sp)) + sp   # an absent axis is 0
    need = int(_lib.lib().fmd_image_metrics_workspace(N, Cc, D, H, W))
    if need < 0:
        raise NotImplementedError(f"image_metrics: shape {tuple(gen.shape)} is beyond the kernel's grid")
    dev = gen.device
    if ws is None:
        ws = torch.empty((need,), device=dev, dtype=torch.uint8)
    elif ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_contiguous() or ws.data_ptr() % 8:
        raise RuntimeError(f"image_metrics: workspace of at least {need} bytes, 8-byte aligned")
    if out is None:
        out = torch.empty((3, N), device=dev, dtype=torch.float64)
    elif out.dtype != torch.float64 or tuple(out.shape) != (3, N) or not out.is_contiguous():
        raise RuntimeError(f"image_metrics: out must be contiguous fp64 [3, {N}]")
    _lib.call("fmd_image_metrics", _p(gen), _p(tgt), N, Cc, D, H, W, int(bool(clamp)), _p(ws), _p(out[0]),
              _p(out[1]), _p(out[2]), stream())
    return ImageMetrics(out[0], out[1], out[2], out)


# ------------------------------------------------------------------ VAE criterion (csrc/vae_loss.hip)
LOSS_TERMS = {"l1": 0, "mse": 1, "bce": 2, "focal": 3, "bce_focal": 4, "hinge_real": 5, "hinge_fake": 6, "neg": 7,
              "square": 8}
LOSS_REDUCTIONS = {"none": 0, "sum": 1, "mean": 2}
VAE_LOSS_CHUNK, VAE_LOSS_ROWS, GAUSS_ROWS = 2048, 512, 256   # FMD_VAE_LOSS_CHUNK / _ROWS, FMD_GAUSS_ROWS


@dataclass
class LossOut:
    """What one ``elementwise_loss`` launch wrote (None: not asked for)."""
    loss: Optional[torch.Tensor]      # fp32 scalar
    elem: Optional[torch.Tensor]      # fp32, the target's shape (the shape of x when flat)
    dx: Optional[torch.Tensor]        # fp32, x's layout
    dx_bf16: Optional[torch.Tensor]   # bf16 [N, *spatial, ldb]


def _f32c(t, what: str, name: str):
    _need_cuda(t, what)
    if t.dtype != F32 or not t.is_contiguous():
        raise RuntimeError(f"{what}: {name} must be a contiguous fp32 tensor, got {t.dtype}"
                           f"{'' if t.is_contiguous() else ' (not contiguous)'}")


def _ws(ws, need: int, dev, what: str):
    if ws is None:
        return torch.empty((max(need, 8),), device=dev, dtype=torch.uint8)
    if ws.dtype != torch.uint8 or ws.numel() < need or not ws.is_contiguous() or ws.data_ptr() % 8:
        raise RuntimeError(f"{what}: workspace of at least {need} bytes, 8-byte aligned")
    return ws


def elementwise_loss(term: str, x, target=None, *, reduction: str = "mean", alpha: float = 0.25,
                     channels: Optional[int] = None, g=None, scale: float = 1.0, loss: bool = True,
                     grad: bool = False, grad_bf16: bool = False, ldb: Optional[int] = None,
                     out: Optional[dict] = None, ws=None) -> LossOut:
    """One launch of the element-wise loss family (``include/fmdiff.h``, "VAE training criterion") over ``x``.

    Flat (``channels=None``): ``x`` and ``target`` are contiguous fp32 of one shape.  Head layout
    (``channels=C``): ``x`` is channels-last ``[N, *spatial, ld]`` with ``ld >= C`` (channels past ``C`` are never
    read) and ``target`` channels-first ``[N, C, *spatial]``.  ``loss`` asks for the reduced value (``sum`` /
    ``mean``) or, with ``reduction="none"``, the per-element term; ``grad`` / ``grad_bf16`` ask for
    ``g * scale * d term / dx`` in x's layout (fp32) and its bf16 copy ``[N, *spatial, ldb]`` (head layout only),
    where ``g`` is a device tensor: one element, or for ``reduction="none"`` one per element of the term.
    ``out``: optional preallocated ``loss`` / ``elem`` / ``dx`` / ``dx_bf16``; ``ws``: optional uint8 workspace.
    Nothing synchronises with the host."""
    what = "elementwise_loss"
    if term not in LOSS_TERMS:
        raise ValueError(f"{what}: unknown term '{term}'")
    if reduction not in LOSS_REDUCTIONS:
        raise ValueError(f"{what}: unknown reduction '{reduction}'")
    tid, rid = LOSS_TERMS[term], LOSS_REDUCTIONS[reduction]
    has_t = tid <= 4
    if has_t and target is None:
        raise ValueError(f"{what}: term '{term}' needs a target")
    if not has_t and (target is not None or channels is not None):
        raise ValueError(f"{what}: term '{term}' takes no target and flat addressing")
    _f32c(x, what, "x")
    if has_t:
        _f32c(target, what, "target")
    if channels is None:
        if has_t and tuple(target.shape) != tuple(x.shape):
            raise ValueError(f"{what}: shape mismatch, x {tuple(x.shape)} against target {tuple(target.shape)}")
        N, Cc, P, ld = 1, 1, x.numel(), 0
        tshape = tuple(x.shape)
        if grad_bf16:
            raise ValueError(f"{what}: the bf16 gradient copy is written in the head layout only")
    else:
        Cc = int(channels)
        if (x.dim() < 3 or target.dim() != x.dim() or target.shape[1] != Cc or x.shape[-1] < Cc
                or x.shape[0] != target.shape[0] or tuple(x.shape[1:-1]) != tuple(target.shape[2:])):
            raise ValueError(f"{what}: head layout wants x [N, *spatial, >= {Cc}] and target [N, {Cc}, *spatial], "
                             f"got {tuple(x.shape)} and {tuple(target.shape)}")
        N, ld = int(x.shape[0]), int(x.shape[-1])
        P = x.numel() // max(1, N * ld)
        tshape = tuple(target.shape)
    need = int(_lib.lib().fmd_vae_loss_workspace(tid, N, Cc, P, ld))
    if need < 0:
        raise ValueError(f"{what}: empty tensor or a shape beyond the kernel's grid, {tuple(x.shape)}")
    dev, out = x.device, out or {}
    want_g = grad or grad_bf16
    g_elem = 0
    if want_g:
        if g is None:
            raise ValueError(f"{what}: a gradient needs the upstream gradient g (a device tensor)")
        _f32c(g, what, "g")
        if g.numel() != 1:
            if rid != 0 or tuple(g.shape) != tshape:
                raise ValueError(f"{what}: g must have one element, or the term's shape {tshape} with "
                                 f"reduction='none'; got {tuple(g.shape)}")
            g_elem = 1

    def buf(key, shape, dtype):
        t = out.get(key)
        if t is None:
            return torch.empty(shape, device=dev, dtype=dtype)
        _need_cuda(t, what)
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise RuntimeError(f"{what}: out['{key}'] must be contiguous {dtype} {tuple(shape)}")
        return t

    o_loss = buf("loss", (), F32) if loss and rid != 0 else None
    o_elem = buf("elem", tshape, F32) if loss and rid == 0 else None
    o_dx = buf("dx", tuple(x.shape), F32) if grad else None
    o_b = None
    if grad_bf16:
        ldb = int(ldb or max(8, -(-Cc // 8) * 8))
        if ldb < Cc:
            raise ValueError(f"{what}: ldb {ldb} below the channel count {Cc}")
        o_b = buf("dx_bf16", (*x.shape[:-1], ldb), BF16)
    if o_loss is None and o_elem is None and not want_g:
        raise ValueError(f"{what}: nothing asked for")
    if o_loss is not None:
        ws = _ws(ws, need, dev, what)
    _lib.call("fmd_vae_loss", tid, rid, _p(x), _p(target), N, Cc, P, ld, float(alpha), _p(g) if want_g else None,
              g_elem, float(scale), _p(ws) if o_loss is not None else None, _p(o_loss), _p(o_elem), _p(o_dx),
              _p(o_b), int(ldb or 0), stream())
    return LossOut(o_loss, o_elem, o_dx, o_b)


def _gauss_dims(moments, E: int, what: str):
    _f32c(moments, what, "moments")
    if moments.dim() < 3 or moments.shape[-1] < 2 * E or E < 1:
        raise ValueError(f"{what}: moments are channels-last [N, *spatial, >= {2 * E}], got {tuple(moments.shape)}")
    N, ldm = int(moments.shape[0]), int(moments.shape[-1])
    sp = tuple(int(v) for v in moments.shape[1:-1])
    P = 1
    for v in sp:
        P *= v
    return N, sp, P, ldm


def _gauss_cf(t, shape, what: str, name: str):
    if t is None:
        return
    _f32c(t, what, name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: {name} must be {tuple(shape)}, got {tuple(t.shape)}")


def gauss_sample_kl(moments, E: int, eps=None, *, Cp: Optional[int] = None, out: Optional[dict] = None, ws=None):
    """Posterior of ``DiagonalGaussian`` in one pass over the channels-last fp32 ``moments`` ``[N, *spatial, >= 2E]``
    (mu then logvar): ``z = mu + exp(0.5 clamp(logvar, -30, 20)) eps`` channels-first ``[N, E, *spatial]`` (``eps``
    channels-first of that shape; None: the mode, ``z = mu``), ``kl [N]``, and with ``Cp`` the decoder's staged
    operand, bf16 ``[N, *spatial, Cp]``.  Returns ``(z, kl, z_staged or None)``.  Nothing synchronises."""
    what = "gauss_sample_kl"
    N, sp, P, ldm = _gauss_dims(moments, E, what)
    _gauss_cf(eps, (N, E, *sp), what, "eps")
    need = int(_lib.lib().fmd_gauss_workspace(N, E, P))
    if need < 0:
        raise ValueError(f"{what}: empty tensor or a shape beyond the kernel's grid, {tuple(moments.shape)}")
    dev, out = moments.device, out or {}

    def buf(key, shape, dtype):
        t = out.get(key)
        if t is None:
            return torch.empty(shape, device=dev, dtype=dtype)
        _need_cuda(t, what)
        if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
            raise RuntimeError(f"{what}: out['{key}'] must be contiguous {dtype} {tuple(shape)}")
        return t

    z = buf("z", (N, E, *sp), F32)
    kl = buf("kl", (N,), F32)
    zs = None
    if Cp is not None:
        if Cp < E:
            raise ValueError(f"{what}: Cp {Cp} below the latent channels {E}")
        zs = buf("z_staged", (N, *sp, int(Cp)), BF16)
    ws = _ws(ws, need, dev, what)
    _lib.call("fmd_gauss_sample_kl", _p(moments), ldm, N, E, P, _p(eps), _p(z), _p(zs), int(Cp or 0), _p(ws), _p(kl),
              stream())
    return z, kl, zs


def gauss_backward(moments, E: int, eps, g_z, g_kl, *, ldd: Optional[int] = None, ldb: Optional[int] = None,
                   out: Optional[dict] = None):
    """Gradient of ``gauss_sample_kl`` to the moments, recomputed from them: fp32 channels-last
    ``[N, *spatial, ldd]`` (default: the stride of ``moments``) and, with ``ldb``, its bf16 copy; padding channels
    zero.  ``g_z`` (channels-first like ``z``), ``g_kl`` (``[N]``) and ``eps`` may each be None (zero).  Returns
    ``(d_moments, d_moments_bf16 or None)``."""
    what = "gauss_backward"
    N, sp, P, ldm = _gauss_dims(moments, E, what)
    _gauss_cf(eps, (N, E, *sp), what, "eps")
    _gauss_cf(g_z, (N, E, *sp), what, "g_z")
    _gauss_cf(g_kl, (N,), what, "g_kl")
    ldd = int(ldd or ldm)
    if ldd < 2 * E or (ldb is not None and ldb < 2 * E):
        raise ValueError(f"{what}: output strides below {2 * E} channels")
    dev, out = moments.device, out or {}
    dm = out.get("d_moments")
    if dm is None:
        dm = torch.empty((N, *sp, ldd), device=dev, dtype=F32)
    else:
        _f32c(dm, what, "out['d_moments']")
        if tuple(dm.shape) != (N, *sp, ldd):
            raise RuntimeError(f"{what}: out['d_moments'] must be {(N, *sp, ldd)}")
    db = None
    if ldb is not None:
        db = out.get("d_moments_bf16")
        if db is None:
            db = torch.empty((N, *sp, int(ldb)), device=dev, dtype=BF16)
        elif db.dtype != BF16 or tuple(db.shape) != (N, *sp, int(ldb)) or not db.is_contiguous() or not db.is_cuda:
            raise RuntimeError(f"{what}: out['d_moments_bf16'] must be contiguous bf16 {(N, *sp, int(ldb))}")
    if int(_lib.lib().fmd_gauss_workspace(N, E, P)) < 0:
        raise ValueError(f"{what}: empty tensor or a shape beyond the kernel's grid, {tuple(moments.shape)}")
    _lib.call("fmd_gauss_backward", _p(moments), ldm, N, E, P, _p(eps), _p(g_z), _p(g_kl), _p(dm), ldd, _p(db),
              int(ldb or 0), stream())
    return dm, db


# ------------------------------------------------------------------ latent 1x1 conv backward (csrc/pointwise_bwd.hip)
POINTWISE_ROWS, POINTWISE_MAXC = 512, 8   # FMD_POINTWISE_ROWS / _MAXC


def pointwise_bwd(dy, x, W, *, channels_last: bool = False, ldg: Optional[int] = None, want_g: bool = True,
                  dW=None, db=None, accumulate: bool = False, out=None, ws=None):
    """Backward of the latent 1x1 conv ``y = W x + b`` (AutoencoderKL's ``post_quant_conv``) in one launch plus the
    finishing launch of the sums.  ``dy`` bf16 channels-last ``[N, *spatial, >= Z]`` and ``x`` bf16 channels-last
    ``[N, *spatial, >= E]`` (the staged latent of ``gauss_sample_kl``); channels past Z / E never enter a result.
    ``W`` fp32 ``[Z, E]`` (or ``[Z, E, 1, 1]``), Z and E at most ``POINTWISE_MAXC``.

    Returns ``(g, dW, db)``: ``g`` fp32, channels-first ``[N, E, *spatial]`` (the ``g_z`` of ``gauss_backward``) or
    with ``channels_last`` ``[N, *spatial, ldg]`` (padding channels zero; default ``ldg``: E rounded up to 8), into
    ``out`` when given, None without ``want_g``; ``dW`` ``[Z, E]`` / ``db`` ``[Z]``: the fp32 tensors passed in
    (``x`` may be None without them), written, or with ``accumulate`` added to.  Nothing synchronises."""
    what = "pointwise_bwd"
    _need_cuda(dy, what)
    if W.dim() not in (2, 4) or (W.dim() == 4 and tuple(W.shape[2:]) != (1, 1)):
        raise ValueError(f"{what}: W is [Z, E] or [Z, E, 1, 1], got {tuple(W.shape)}")
    Z, E = int(W.shape[0]), int(W.shape[1])
    _f32c(W, what, "W")
    sums = dW is not None or db is not None
    for t, name, cmin in ((dy, "dy", Z), (x, "x", E)):
        if t is None and name == "x" and not sums:
            continue
        if t is None:
            raise ValueError(f"{what}: dW / db need x")
        _need_cuda(t, what)
        if t.dtype != BF16 or not t.is_contiguous() or t.dim() < 3 or t.shape[-1] < cmin:
            raise RuntimeError(f"{what}: {name} must be contiguous bf16 [N, *spatial, >= {cmin}], got {t.dtype} "
                               f"{tuple(t.shape)}")
    if x is not None and tuple(x.shape[:-1]) != tuple(dy.shape[:-1]):
        raise ValueError(f"{what}: dy {tuple(dy.shape)} and x {tuple(x.shape)} differ in their rows")
    N, sp = int(dy.shape[0]), tuple(int(v) for v in dy.shape[1:-1])
    P = 1
    for v in sp:
        P *= v
    need = int(_lib.lib().fmd_pointwise_bwd_workspace(N * P, Z, E))
    if need < 0:
        raise ValueError(f"{what}: Z = {Z}, E = {E} beyond the kernel's limit of {POINTWISE_MAXC} channels, an "
                         f"empty tensor or a shape beyond its grid, {tuple(dy.shape)}")
    for t, name, shape in ((dW, "dW", (Z, E)), (db, "db", (Z,))):
        if t is not None:
            _f32c(t, what, name)
            if t.numel() != Z * (E if name == "dW" else 1) or tuple(t.shape[:len(shape)]) != shape:
                raise ValueError(f"{what}: {name} must be {shape}, got {tuple(t.shape)}")
    g = None
    if want_g:
        if channels_last:
            ldg = int(ldg or max(8, -(-E // 8) * 8))
            if ldg < E:
                raise ValueError(f"{what}: ldg {ldg} below the channel count {E}")
            shape = (N, *sp, ldg)
        else:
            shape = (N, E, *sp)
        g = out
        if g is None:
            g = torch.empty(shape, device=dy.device, dtype=F32)
        else:
            _f32c(g, what, "out")
            if tuple(g.shape) != shape:
                raise RuntimeError(f"{what}: out must be {shape}, got {tuple(g.shape)}")
    elif not sums:
        raise ValueError(f"{what}: nothing asked for")
    if sums:
        ws = _ws(ws, need, dy.device, what)
    _lib.call("fmd_pointwise_bwd", _p(dy), int(dy.shape[-1]), _p(x) if sums else None,
              int(x.shape[-1]) if sums else 0, _p(W), N, P, Z, E, _p(g), int(bool(channels_last)), int(ldg or 0),
              _p(dW), _p(db), int(bool(accumulate)), _p(ws) if sums else None, stream())
    return g, dW, db


# ------------------------------------------------------------------ BatchNorm + LeakyReLU, image staging (csrc/batchnorm.hip)
BN_ROWS = 64   # FMD_BN_ROWS
IMAGE_MODES = {"identity": 0, "clamp": 1, "sigmoid": 2}


def _rows_c(x, what: str):
    """(M, C) of a contiguous bf16 channels-last activation."""
    _need_cuda(x, what)
    if x.dtype != BF16 or not x.is_contiguous() or x.dim() < 2:
        raise RuntimeError(f"{what}: contiguous bf16 channels-last activations, got {x.dtype} {tuple(x.shape)}")
    Cc = int(x.shape[-1])
    return x.numel() // Cc, Cc


def bn_fold(st: Optional[Stats], M: int, gamma, beta, running_mean, running_var, num_batches_tracked=None, *,
            eps: float = 1e-5, momentum: float = 0.1, training: bool = True):
    """nn.BatchNorm2d's statistics step on the device.  ``st``: the statistics slab of the normalised activation
    (a conv epilogue's or ``channel_stats``'; unused in eval mode).  Training: batch mean / biased variance over the
    M elements of a channel, the running statistics and ``num_batches_tracked`` (int64) updated in place; eval: the
    running statistics.  Returns ``(a, b, mean_rstd)`` with ``a = gamma rstd``, ``b = beta - mean a``."""
    _need_cuda(gamma, "bn_fold")
    Cc = int(gamma.numel())
    dev = gamma.device
    a = torch.empty((Cc,), device=dev, dtype=F32)
    b = torch.empty((Cc,), device=dev, dtype=F32)
    mr = torch.empty((Cc, 2), device=dev, dtype=F32)
    slab = st.slab if training else None
    if slab is not None and (slab.dim() != 3 or slab.shape[1] != Cc or slab.shape[2] != 2 or not slab.is_contiguous()
                             or slab.dtype != F32):
        raise ValueError(f"bn_fold: slab {tuple(slab.shape)} is not [rows][{Cc}][2] fp32")
    if num_batches_tracked is not None and num_batches_tracked.dtype != torch.int64:
        raise ValueError("bn_fold: num_batches_tracked must be int64")
    _lib.call("fmd_bn_fold", _p(slab), int(slab.shape[0]) if slab is not None else 0, Cc, int(M), _p(gamma), _p(beta),
              float(eps), float(momentum), int(bool(training)), _p(running_mean), _p(running_var),
              _p(num_batches_tracked), _p(a), _p(b), _p(mr), stream())
    return a, b, mr


def _rows_c32(x, what: str):
    """(M, C) of a contiguous fp32 channels-last tensor (a conv's ``out_f32`` output)."""
    _f32c(x, what, "x")
    Cc = int(x.shape[-1])
    return x.numel() // Cc, Cc


def bn_stats_f32(x) -> Stats:
    """(sum x, sum x^2) per channel and BN_ROWS-row block of an fp32 channels-last tensor: the slab ``bn_fold``
    reads when the conv wrote fp32 (which emits no statistics of its own)."""
    M, Cc = _rows_c32(x, "bn_stats_f32")
    slab = torch.empty((-(-M // BN_ROWS), Cc, 2), device=x.device, dtype=F32)
    _lib.call("fmd_bn_stats_f32", _p(x), M, Cc, _p(slab), stream())
    return Stats(slab, BN_ROWS)


def bn_act_fwd(x, a=None, b=None, slope: float = 0.2, out=None, split: bool = False):
    """``lrelu(a[c] x + b[c], slope)`` as bf16 (one fma, one rounding); ``a`` None: the plain activation.
    ``split``: ``x`` is fp32 and the result is written as two bf16 terms, ``[..., 2 C]`` with the hi terms in channels
    [0, C) and the lo terms bf16(v - hi) in [C, 2 C) (about 16 significant bits; the walker's activation form)."""
    if split:
        M, Cc = _rows_c32(x, "bn_act_fwd")
        y = torch.empty((*x.shape[:-1], 2 * Cc), device=x.device, dtype=BF16) if out is None else out
        _lib.call("fmd_bn_act_fwd_split", _p(x), M, Cc, _p(a), _p(b), float(slope), _p(y), stream())
        return y
    M, Cc = _rows_c(x, "bn_act_fwd")
    y = torch.empty_like(x) if out is None else out
    _lib.call("fmd_bn_act_fwd", _p(x), M, Cc, _p(a), _p(b), float(slope), _p(y), stream())
    return y


def bn_act_bwd(dy, x, a=None, b=None, mean_rstd=None, *, slope: float = 0.2, training: bool = True, dgamma=None,
               dbeta=None, accumulate: bool = True, skip_param_grads: bool = False, out=None, ws=None):
    """Backward of ``bn_act_fwd`` behind a BatchNorm: returns ``dx`` (bf16, the operand of the conv's data and weight
    gradients); ``dgamma`` / ``dbeta`` are written, or with ``accumulate`` added to, unless ``skip_param_grads``.
    ``x``: the normalised activation, bf16 or (the walker's) fp32; ``dy`` and ``dx`` are bf16 either way."""
    f32 = x.dtype == F32
    M, Cc = _rows_c32(x, "bn_act_bwd") if f32 else _rows_c(x, "bn_act_bwd")
    if _rows_c(dy, "bn_act_bwd") != (M, Cc):
        raise ValueError(f"bn_act_bwd: dy {tuple(dy.shape)} and x {tuple(x.shape)} differ")
    dx = torch.empty_like(dy) if out is None else out
    if a is not None and (training or not skip_param_grads):
        need = int(_lib.lib().fmd_bn_act_bwd_workspace(M, Cc))
        if need < 0:
            raise ValueError(f"bn_act_bwd: C = {Cc} must be a positive multiple of 8, M = {M}")
        ws = _ws(ws, need, x.device, "bn_act_bwd")
    else:
        ws = None
    _lib.call("fmd_bn_act_bwd_f32" if f32 else "fmd_bn_act_bwd", _p(dy), _p(x), M, Cc, _p(a), _p(b), _p(mean_rstd),
              float(slope), int(bool(training)), _p(dx), _p(dgamma), _p(dbeta), int(bool(accumulate)),
              int(bool(skip_param_grads)), _p(ws), stream())
    return dx


def image_stage(x, mode="identity", Cp: Optional[int] = None, out=None, split: bool = False):
    """fp32 NCHW image batch -> bf16 NHWC with the channels padded to ``Cp`` (a multiple of 8; padding zero) and the
    reference's ``raw_output_to_image`` fused: "identity", "clamp" ``(clamp(x, -1, 1) + 1) / 2``, "sigmoid".
    ``split``: two bf16 terms per value, ``[..., 2 Cp]`` (hi | lo, as ``bn_act_fwd``)."""
    _need_cuda(x, "image_stage")
    _f32c(x, "image_stage", "x")
    N, Cc = int(x.shape[0]), int(x.shape[1])
    sp = tuple(int(v) for v in x.shape[2:])
    Cp = int(Cp or max(8, -(-Cc // 8) * 8))
    y = torch.empty((N, *sp, 2 * Cp if split else Cp), device=x.device, dtype=BF16) if out is None else out
    _lib.call("fmd_image_stage_split" if split else "fmd_image_stage", _p(x), N, Cc, x[0, 0].numel(), Cp,
              IMAGE_MODES[mode], _p(y), stream())
    return y


def image_stage_bwd(g, x, mode="identity"):
    """Gradient of ``image_stage`` to the raw fp32 NCHW ``x`` from the bf16 NHWC gradient ``g`` of its output."""
    _need_cuda(x, "image_stage_bwd")
    _f32c(x, "image_stage_bwd", "x")
    _, Cp = _rows_c(g, "image_stage_bwd")
    dx = torch.empty_like(x)
    _lib.call("fmd_image_stage_bwd", _p(g), _p(x), int(x.shape[0]), int(x.shape[1]), x[0, 0].numel(), Cp,
              IMAGE_MODES[mode], _p(dx), stream())
    return dx


# ------------------------------------------------------------------ VGG perceptual loss (csrc/perceptual.hip)
def _perc_hw(size, what: str):
    if size is None:
        return None
    hw = (int(size), int(size)) if isinstance(size, int) else tuple(int(v) for v in size)
    if len(hw) != 2 or hw[0] < 1 or hw[1] < 1:
        raise ValueError(f"{what}: size must be a positive int or (h, w), got {size!r}")
    return hw


def _perc_images(recon, target, what: str):
    _f32c(recon, what, "recon")
    if target is not None:
        _f32c(target, what, "target")
        if target.shape != recon.shape:
            raise ValueError(f"{what}: recon {tuple(recon.shape)} and target {tuple(target.shape)} differ")
    if recon.dim() != 4 or recon.shape[1] not in (1, 3) or recon.numel() == 0:
        raise ValueError(f"{what}: images [N, 1 or 3, H, W], got {tuple(recon.shape)}")
    return tuple(int(v) for v in recon.shape)


def perc_stage(recon, target, mode="identity", size=None):
    """The perceptual loss's input: fp32 NCHW ``recon`` and ``target`` (1 or 3 channels) -> one two-term bf16 batch
    ``[2 N, Ho, Wo, 16]`` (recon first; 8 hi | 8 lo channels, one channel repeated to three).  ``mode``: the image map
    (``IMAGE_MODES``) of the recon half, the target is used as given; ``size``: bilinear resize to ``(Ho, Wo)`` with
    torch's ``align_corners=False`` rule."""
    N, Cc, Hs, Ws = _perc_images(recon, target, "perc_stage")
    Ho, Wo = _perc_hw(size, "perc_stage") or (Hs, Ws)
    out = torch.empty((2 * N, Ho, Wo, 16), device=recon.device, dtype=BF16)
    _lib.call("fmd_perc_stage", _p(recon), _p(target), N, Cc, Hs, Ws, Ho, Wo, IMAGE_MODES[mode], _p(out), stream())
    return out


def perc_stage_bwd(g, recon, mode="identity"):
    """Gradient of ``perc_stage`` to the raw fp32 NCHW ``recon`` from the bf16 ``[N, Ho, Wo, Cp]`` gradient ``g`` of
    the recon half of its output (the first conv's data gradient)."""
    N, Cc, Hs, Ws = _perc_images(recon, None, "perc_stage_bwd")
    _, Cp = _rows_c(g, "perc_stage_bwd")
    if g.dim() != 4 or g.shape[0] != N:
        raise ValueError(f"perc_stage_bwd: g [{N}, Ho, Wo, Cp], got {tuple(g.shape)}")
    dx = torch.empty_like(recon)
    _lib.call("fmd_perc_stage_bwd", _p(g), _p(recon), N, Cc, Hs, Ws, int(g.shape[1]), int(g.shape[2]), Cp,
              IMAGE_MODES[mode], _p(dx), stream())
    return dx


def perc_tap_fwd(y, C: int, *, pool: bool = False, want_out: bool = True, save: bool = True, weight: float = 1.0,
                 value=None, loss=None, first: bool = True, ws=None, out=None, sgn=None):
    """The feature tap on a conv's fp32 output ``y [2 N, H, W, Cp]`` (recon rows first): ``value`` (a device fp32
    scalar, made if None) receives ``mean |relu(y_rec) - relu(y_tgt)|`` over the ``C`` real channels, ``loss`` (if
    given) ``weight * value`` (``first``) or that added to it.  Returns ``(out, sgn, value)``: ``out`` the next conv's
    two-term operand ``relu(y)`` for all 2 N images, behind a 2x2 stride-2 max pool with ``pool`` (None without
    ``want_out``); ``sgn`` the int8 sign of the difference ``[N, H, W, Cp]`` that ``perc_tap_bwd`` reads (None without
    ``save``)."""
    _f32c(y, "perc_tap_fwd", "y")
    if y.dim() != 4 or y.shape[0] % 2 or y.shape[0] < 2:
        raise ValueError(f"perc_tap_fwd: y [2 N, H, W, Cp], got {tuple(y.shape)}")
    N, H, W, Cp = int(y.shape[0]) // 2, int(y.shape[1]), int(y.shape[2]), int(y.shape[3])
    need = int(_lib.lib().fmd_perc_tap_workspace(N, H, W, Cp))
    if need < 0 or not 1 <= int(C) <= Cp:
        raise ValueError(f"perc_tap_fwd: Cp = {Cp} must be a positive multiple of 8 and 1 <= C = {C} <= Cp")
    if want_out and pool and (H < 2 or W < 2):
        raise ValueError(f"perc_tap_fwd: a {H}x{W} map is too small for the 2x2 pool")
    dev = y.device
    ws = _ws(ws, need, dev, "perc_tap_fwd")
    oshape = (2 * N, H // 2, W // 2, 2 * Cp) if pool else (2 * N, H, W, 2 * Cp)
    if not want_out:
        out = None
    elif out is None:
        out = torch.empty(oshape, device=dev, dtype=BF16)
    elif tuple(out.shape) != oshape or out.dtype != BF16 or not out.is_contiguous():
        raise ValueError(f"perc_tap_fwd: out must be bf16 {oshape}")
    if not save:
        sgn = None
    elif sgn is None:
        sgn = torch.empty((N, H, W, Cp), device=dev, dtype=torch.int8)
    elif tuple(sgn.shape) != (N, H, W, Cp) or sgn.dtype != torch.int8 or not sgn.is_contiguous():
        raise ValueError(f"perc_tap_fwd: sgn must be int8 {(N, H, W, Cp)}")
    if value is None:
        value = torch.empty((), device=dev, dtype=F32)
    _lib.call("fmd_perc_tap_fwd", _p(y), N, H, W, Cp, int(C), int(bool(pool)), _p(out), _p(sgn), _p(ws),
              float(weight), int(bool(first)), _p(value), _p(loss), stream())
    return out, sgn, value


def perc_tap_bwd(y_rec, sgn, C: int, g_loss, *, weight: float = 1.0, g_below=None, pool: bool = False, out=None):
    """Backward of the tap, recon half: bf16 ``dy [N, H, W, Cp]`` of the tapped conv's output from the saved recon
    rows ``y_rec`` (fp32), ``sgn``, the device scalar ``g_loss`` and the gradient ``g_below`` of the tap's output
    (``[N, H/2, W/2, Cp]`` with ``pool``: routed to the first maximum of each window; None: the last tap)."""
    _f32c(y_rec, "perc_tap_bwd", "y_rec")
    _f32c(g_loss, "perc_tap_bwd", "g_loss")
    _need_cuda(sgn, "perc_tap_bwd")
    if y_rec.dim() != 4 or sgn.dtype != torch.int8 or sgn.shape != y_rec.shape or not sgn.is_contiguous():
        raise ValueError(f"perc_tap_bwd: y_rec [N, H, W, Cp] fp32 and sgn int8 of that shape, got "
                         f"{tuple(y_rec.shape)} and {sgn.dtype} {tuple(sgn.shape)}")
    N, H, W, Cp = (int(v) for v in y_rec.shape)
    if Cp % 8 or not 1 <= int(C) <= Cp or g_loss.numel() != 1:
        raise ValueError(f"perc_tap_bwd: Cp = {Cp} a multiple of 8, 1 <= C = {C} <= Cp, g_loss one element")
    if g_below is not None:
        want = (N, H // 2, W // 2, Cp) if pool else (N, H, W, Cp)
        _rows_c(g_below, "perc_tap_bwd")
        if tuple(g_below.shape) != want or 0 in want:
            raise ValueError(f"perc_tap_bwd: g_below {tuple(g_below.shape)}, expected {want}")
    dy = torch.empty((N, H, W, Cp), device=y_rec.device, dtype=BF16) if out is None else out
    _lib.call("fmd_perc_tap_bwd", _p(y_rec), _p(sgn), N, H, W, Cp, int(C), int(bool(pool)), _p(g_below), _p(g_loss),
              float(weight), _p(dy), stream())
    return dy
