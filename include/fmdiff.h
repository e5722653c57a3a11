/*
 * fmdiff: MI355X-native (gfx950 / CDNA4) kernels for the flow-matching /
 * diffusion UNet train + sample hot path.  C ABI, plain pointers and sizes.
 *
 * Ownership: every buffer (activations, weights, workspaces) is allocated by
 * the caller (PyTorch's caching allocator) and passed in; the library
 * allocates nothing.  Errors: every entry point returns 0 on success, a
 * positive hipError_t, or a negative argument-validation code; no exception
 * crosses the ABI.  Threading: kernels are stateless and launch on the
 * caller's hipStream_t.
 *
 * Layouts: activations NHWC bf16 ("pixels x channels"); conv weights bf16
 * [K][ks*ks][C] (forward) -- the fp32 master copy stays in the reference's
 * [K][C][kh][kw] layout so state_dicts are drop-in.
 *
 * The reference has no native plugin API: its boundary is the Python module
 * surface.  Each entry point names the reference op(s) it replaces.
 */
#ifndef FMDIFF_H
#define FMDIFF_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* fmd_stream_t; /* hipStream_t */

/* ------------------------------------------------------------------ conv
 * Implicit-GEMM convolution on MFMA, replacing ConvND -> nn.Conv{2}d
 * (src/nn/ops/convolution.py:8-54), the GroupNorm+SiLU(+scale/shift) that
 * feeds it (src/nn/blocks/residual.py:95-117), nearest-x2 UpsampleND
 * (src/nn/ops/upsampling.py:27), DownsampleND stride 2 (upsampling.py:49-56),
 * the decoder torch.cat (src/models/unet/unet.py:322), the 1x1 skip conv and
 * residual add (residual.py:120).  The same kernel computes data gradients
 * (transposed gather) for the backward pass.
 */
typedef struct fmd_conv_desc {
  int32_t N, Hs, Ws;        /* stored input dims */
  int32_t C0, C1;           /* channels of src0 / src1 (virtual concat, C = C0 + C1) */
  int32_t Ho, Wo, K;        /* output dims / output channels */
  int32_t ks, stride, pad;  /* square kernel, stride, zero padding */
  int32_t upsample;         /* 1: logical input = nearest-x2 of the stored input */
  int32_t transposed;       /* 1: gather (o + pad - k) / stride  (data-gradient mode) */
  const void* src0;         /* bf16 NHWC [N][Hs][Ws][C0] */
  const void* src1;         /* bf16 NHWC [N][Hs][Ws][C1] or NULL */
  const float* pro_a;       /* [N][C] prologue affine x*a+b (GroupNorm fused), or NULL */
  const float* pro_b;
  int32_t pro_silu;         /* apply SiLU after the affine */
  const void* wgt;          /* bf16 [K][ks*ks][C] */
  const void* src2;         /* optional 1x1 second GEMM over the concat (src2 | src3): */
  const void* src3;         /*   bf16 [N][Ho][Wo][C2] and [N][Ho][Wo][C3] (ResBlock skip conv) */
  int32_t C2, C3;
  const void* wgt2;         /* bf16 [K][C2+C3] */
  const float* bias;        /* [K] or NULL */
  const float* bias2;       /* [K] or NULL (skip-conv bias, added too) */
  const float* bias_nc;     /* [N][K] per-sample bias (time-embedding add) or NULL */
  const void* resid;        /* bf16 [N][Ho][Wo][K] residual or NULL */
  void* out;                /* bf16 (or fp32 if out_f32) [N][Ho][Wo][K] */
  int32_t out_f32;
  int32_t accumulate;       /* out += result */
  float* stats;             /* slab [M/64][K][2] of per-64-pixel partial sums, or NULL; with splits > 1
                               [M/FMD_SPLIT_STATS_ROWS][K][2] (written by the split-K combine), or
                               [M/tickets_rows][K][2] when the split is combined inside the launch (tickets) */
  const void* ep_x0;        /* data-gradient epilogue: x = forward GN input at (p, c); if ep_a: */
                            /*   out *= silu'(ep_a*x+ep_b); stats become (sum out, sum out*x) */
  const void* ep_x1;
  int32_t ep_C0;
  const float* ep_a;
  const float* ep_b;
  float* ws;                /* split-K workspace fp32 [splits][M][K] */
  int32_t splits;
  int32_t force_generic;    /* 1: never take the halo-tiled 3x3 path (testing) */
  const void* wgt_tiled;    /* wgt re-tiled by fmd_tile_weights_halo (enables the halo path) */
  const void* wgt2_tiled;   /* wgt2 re-tiled likewise (T = 1) */
  int32_t Ds, Do;           /* 3-D problems (spatial_dims = 3, NDHWC): stored / output depth; 0 = 2-D.
                               Cubic kernel (ks^3 taps, wgt [K][ks^3][C]); implicit-GEMM path only */
  void* gout;               /* optional bf16 [N][Hs][Ws][C0+C1] (3-D: [N][Ds][Hs][Ws][C]): the prologue's output
                               G = SiLU(pro_a*x+pro_b) (or the affine alone), written once per element by the
                               halo path -- the weight gradient's operand, so the backward does not recompute
                               the GroupNorm+SiLU.  Requires pro_a, (C0+C1) % 32 == 0 and the halo path (fmd_conv
                               returns -9 otherwise); NULL = off */
  const float* fold_st0;    /* forward-only GroupNorm prologue folded in the halo kernel (2-D, csrc/conv_halo9.hip),
                               in place of pro_a / pro_b: each workgroup computes its sample's affine from the
                               producers' statistics slab of src0 [N*Hs*Ws/fold_rows0][C0][2] (and of src1), the
                               groups, eps, gamma, beta and the scale-shift rows -- gn_prep's fold, without its
                               launch.  An offer: fmd_conv_plan says whether the kernel that runs takes it
                               (plan.fold); where it does not the caller folds with fmd_gn_prep and passes pro_a /
                               pro_b instead (an unplanned fmd_conv returns -13).  NULL = off */
  int32_t fold_rows0;
  const float* fold_st1;
  int32_t fold_rows1;
  int32_t fold_G;
  float fold_eps;
  const float* fold_gamma;  /* [C0 + C1] or NULL */
  const float* fold_beta;
  const float* fold_emb;    /* scale-shift norm: [N][fold_emb_stride] scale | shift, or NULL */
  int32_t fold_emb_stride;
  int32_t* tickets;         /* split-K (splits > 1) combined inside the conv launch (2-D: the v9b halo kernel or the
                               implicit GEMM on whole tiles): [n_tickets] arrival counters, zero on entry and left
                               zero; d->ws holds the parts' fp32 tiles (same [splits][M][K] size) and the statistics
                               come from the conv epilogue, one row per tickets_rows pixels (64 on the halo kernel,
                               the wave's pixel range on the implicit GEMM).  An offer: fmd_conv_plan says whether
                               the kernel that runs takes it (plan.tickets) and the rows it writes (plan.stats_rows);
                               where it does not the caller clears it (an unplanned fmd_conv returns -14 when the
                               ticket is not taken or tickets_rows is not the rows written).  NULL = the separate
                               combine launch */
  int32_t n_tickets;
  int32_t tickets_rows;     /* pixels per statistics row the caller allocated for a ticketed conv with stats */
} fmd_conv_desc;

/* What fmd_conv will launch for a descriptor: a host-side query, nothing is launched.  fmd_conv runs the same
 * decision, so the plan and the launch agree. */
#define FMD_CONV_IGEMM 1          /* plan.kernel: implicit GEMM (csrc/conv.hip), tile bco x bpx */
#define FMD_CONV_HALO8 2          /* halo-tiled 3x3, round-3 kernel (csrc/conv_halo.hip) */
#define FMD_CONV_HALO9 3          /* halo-tiled 3x3, v9b (csrc/conv_halo9.hip), tile_rows x 16 pixel tiles */
#define FMD_CONV_TICKET_HALO 1    /* allow: the in-launch combine is offered to the halo kernel */
#define FMD_CONV_TICKET_IGEMM 2   /* allow: ... to the implicit GEMM */
#define FMD_CONV_WANT_STATS 4     /* allow: statistics are wanted (d->stats set counts too) */
typedef struct fmd_conv_plan_t {
  int32_t kernel;           /* FMD_CONV_IGEMM / FMD_CONV_HALO8 / FMD_CONV_HALO9 */
  int32_t tile_rows;        /* halo v9b: 16, 8 or 4 output rows per tile; else 0 */
  int32_t bco, bpx;         /* implicit GEMM: output channels x pixels per tile; else 0 */
  int32_t tickets;          /* 1: d->tickets is taken, the split is combined inside the launch */
  int32_t combine_launch;   /* 1: a splitk_reduce* launch follows the conv launch */
  int32_t stats_rows;       /* pixels per row the launch writes into d->stats; 0: no kernel emits them for this
                               problem (the caller leaves d->stats NULL and runs fmd_channel_stats) */
  int32_t fold;             /* 1: d->fold_* is consumed in the prologue; 0: the caller must supply pro_a / pro_b */
} fmd_conv_plan_t;
/* Plans d with the caller's offers: the in-launch combine of a split (allow: to which kernel families; d->n_tickets
 * counters; d->tickets itself may still be NULL), the statistics (allow) and the fold (d->fold_*).  A declined offer is
 * dropped, the ticket before the fold, until the plan is a form that runs.  The caller then sets d->tickets and
 * tickets_rows = stats_rows if plan.tickets (else leaves them NULL / 0), replaces fold_* by pro_a / pro_b unless
 * plan.fold, sets d->stats to a slab of stats_rows-pixel rows (or leaves it NULL), and calls fmd_conv once.  Returns
 * 0, or the negative code of a descriptor no kernel runs. */
int fmd_conv_plan(const fmd_conv_desc* d, int32_t allow, fmd_conv_plan_t* out);
/* Dispatches 3x3 stride-1 forward-gather problems with enough 16x16 output tiles to the halo-tiled kernels
 * (csrc/conv_halo.hip, csrc/conv_halo9.hip), everything else to the implicit GEMM (csrc/conv.hip): fmd_conv_plan's
 * decision with both families allowed the ticket, then the launch.  Every offer in d must be taken as made: -13 (fold
 * declined), -14 (ticket declined, or tickets_rows is not the rows written), -5 / -11 (d->stats cannot be written). */
int fmd_conv(const fmd_conv_desc* d, fmd_stream_t s);
/* Halo-tiled 3x3 stride-1 conv; returns 1 (nothing launched) when the problem does not qualify. */
int fmd_conv_halo(const fmd_conv_desc* d, fmd_stream_t s);
/* Split-K combine alone: d->out = sum of the d->splits fp32 slabs [splits][M][K] in d->ws + the conv epilogue
 * (bias, bias2, bias_nc, resid, ep_*, stats with FMD_SPLIT_STATS_ROWS-pixel rows).  Replaces nothing on its
 * own: it closes convolutions issued as several partial launches (3-D 3x3x3 convs as three depth-tap planes
 * of the 2-D halo kernel, ConvND 3-D path, src/nn/ops/convolution.py:36). */
int fmd_conv_combine(const fmd_conv_desc* d, fmd_stream_t s);
/* GroupNorm-backward apply fused as a conv epilogue (fmd_conv_gn_apply):
 * dx = conv(d) + P*dz + Q*x + R (+ dx if acc), x/dx split over two concat sources at C0. */
typedef struct fmd_gn_apply_desc {
  const void* dz;           /* bf16 [M][C] (C = the conv's K) */
  const void* x0;           /* bf16 [M][C0] forward GroupNorm input */
  const void* x1;           /* bf16 [M][C - C0] or NULL */
  int32_t C0;
  const float* P;           /* [N][C] */
  const float* Q;
  const float* R;
  void* dx0;                /* bf16 [M][C0] */
  int32_t acc0;
  void* dx1;                /* bf16 [M][C - C0] or NULL */
  int32_t acc1;
} fmd_gn_apply_desc;
/* The ResBlock skip-conv data gradient fused into the GroupNorm backward of the block input
 * (replaces conv(dy, W_skip^T) + fmd_gn_bwd_apply(extra = that)). */
int fmd_conv_gn_apply(const fmd_conv_desc* d, const fmd_gn_apply_desc* g, fmd_stream_t s);

/* GroupNorm forward of a split-K conv's output, fused into its split-K combine (fmd_conv_gn).  For each (n, c):
 * out = conv result (bf16, as fmd_conv writes it); then per (n, group) mean / rstd of out, a = rstd*gamma,
 * b = beta - mean*a (emb_mode 1: a *= 1 + emb[n][c], b = b*(1 + emb[n][c]) + emb[n][K + c]) and the materialised
 * t = SiLU(a*out + b) (silu = 0: the affine alone) -- the outputs of fmd_gn_fused_apply on out. */
typedef struct fmd_gn_out_desc {
  int32_t G;                /* groups */
  float eps;
  const float* gamma;       /* [K] or NULL */
  const float* beta;        /* [K] or NULL */
  const float* emb;         /* [N][emb_stride] scale | shift (emb_mode 1) or NULL */
  int32_t emb_stride, emb_mode, silu;
  float* a;                 /* [N][K] */
  float* b;                 /* [N][K] */
  float* mean_rstd;         /* [N][G][2] */
  void* t;                  /* bf16 [N][Ho][Wo][K] */
} fmd_gn_out_desc;
/* fmd_conv with d->splits > 1 whose combine also produces the GroupNorm of the output (one workgroup per
 * (image, whole groups of max(CB = 4 or fmd_conv_gn_set_block_channels, C/G) channels): the group statistics close inside it).  Requires K % 64 == 0, 64 % (K/G) == 0, no
 * d->stats / out_f32 / accumulate / ep_*.  Replaces fmd_conv + fmd_gn_fused_apply on the small levels
 * (src/nn/blocks/residual.py:71-76 conv1 -> out_layers GroupNorm + SiLU). */
int fmd_conv_gn(const fmd_conv_desc* d, const fmd_gn_out_desc* g, fmd_stream_t s);

/* Input channels per halo-kernel chunk (csrc/conv_halo.hip). */
#define FMD_SPLIT_STATS_ROWS 16   /* pixels per statistics row of a split-K conv */
/* Fewest workgroups (16x16 tiles x cout tiles x split-K chunks) a 2-D problem needs to take the halo conv
 * (default 32; fewer go to the implicit GEMM).  The Python side applies its tuning table's HALO_MIN_WG through it
 * (fmdiff/runtime/tuning.py); the host's halo_splits mirror reads the same table entry. */
int fmd_halo_set_min_workgroups(int32_t n);
/* Halo-conv grids with fewer workgroups than n (16-row tiles x cout tiles x splits; default 1024) run 8-row tiles
 * instead (twice the workgroups: the 128^2 / 64^2 levels would otherwise be one lock-step round); 0 = never.  A
 * tuning hook (tuning table HALO_TH8_MAX_WG). */
int fmd_halo_set_th8_max_workgroups(int32_t n);
/* 8-row grids (tiles x splits) with fewer workgroups than n (default 512) run 4-row tiles instead (plain 2-D 3x3:
 * the latent UNet's 32^2 convs would otherwise fill half the CUs); 0 = never.  Tuning table HALO_TH4_MAX_WG. */
int fmd_halo_set_th4_max_workgroups(int32_t n);
/* Fewest channels per combine block of fmd_conv_gn (4, 8, 16, 32 or 64; default 4):
 * a block owns max(cb, K / G) channels = whole groups.  Returns -1 for any other value.  A tuning hook; the host's
 * conv_gn_eligible mirror reads ops.CONV_GN_CB. */
int fmd_conv_gn_set_block_channels(int32_t cb);
#define FMD_HALO_BK 32
/* [K][T][C] bf16 kernel weights -> the halo kernel's per-(cout tile, FMD_HALO_BK-channel chunk, tap) 8 KiB tiles. */
int64_t fmd_halo_tiled_size(int32_t K, int32_t T, int32_t C);
int fmd_tile_weights_halo(const void* w, int32_t K, int32_t T, int32_t C, void* out, fmd_stream_t s);
/* Stride-2 pad-1 convs (3x3, or the 4x4 data gradient of conv3x3(nearest_x2(x))) as a 2x2 conv over the
 * space-to-depth view of the input (plane (a, b) = pixels (2y + a, 2x + b), staged from the full-resolution NHWC
 * tensor) on the halo kernel (csrc/conv_halo9.hip).  Replaces the implicit GEMM of DownsampleND's conv
 * (src/nn/ops/upsampling.py:49-56) and the data gradient of UpsampleND's conv (upsampling.py:27-29).  Needs
 * d->wgt_tiled from fmd_s2d_tile_weights, Hs = 2 Ho, Ws = 2 Wo, Ho and Wo multiples of 16, (C0 + C1) % 32 == 0,
 * K % 128 == 0, >= 128 output tiles; d->accumulate adds into d->out.  3-D (d->Ds = 2 d->Do, stride 2 in depth too;
 * weights from fmd_s2d_tile_weights_nd with dims 3): the depth taps run as chunks over full-resolution slices
 * 2z + kz - 1 (Conv3d of DownsampleND; the 4x4x4 data gradient of UpsampleND's Conv3d).  Returns 1 when the problem
 * does not qualify. */
int fmd_conv_s2d(const fmd_conv_desc* d, fmd_stream_t s);
/* The data gradient of a stride-2 pad-1 3x3 conv (the transposed gather of DownsampleND's conv,
 * src/nn/ops/upsampling.py:49-56) as a stride-1 2x2 conv from the low-resolution gradient onto the depth-to-space
 * view of the output (4 pixel classes x K channels, one class per 128-channel tile) on the halo kernel.  d as for
 * fmd_conv with transposed = 1: Ho = 2 Hs, Wo = 2 Ws, Hs and Ws multiples of 16, (C0 + C1) % 32 == 0, K % 128 == 0,
 * no prologue; d->wgt_tiled from fmd_s2d_tile_weights mode 2; d->accumulate adds into d->out.  3-D (d->Do = 2 d->Ds,
 * weights from fmd_s2d_tile_weights_nd with dims 3): 8 output classes (depth parity, a, b), the gradient slices z and
 * z + 1 as chunks.  Returns 1 when the problem does not qualify. */
int fmd_conv_d2s(const fmd_conv_desc* d, fmd_stream_t s);
/* fp32 reference-layout conv weight [K][C][ks][ks] -> the halo tiles of fmd_conv_s2d / fmd_conv_d2s.  mode 0: the
 * stride-2 forward (rows K, ks 3 or 4); mode 1: the 4x4 data gradient of a 3x3 conv on a nearest-x2 input
 * (rows C, inner channels K, ks 3); mode 2: the stride-2 3x3 data gradient (rows 4C class-major, C % 128 == 0,
 * inner K).  The inner channel count must be a multiple of 32. */
int64_t fmd_s2d_tiled_size(int32_t K, int32_t C, int32_t mode);
int fmd_s2d_tile_weights(const float* w, int32_t K, int32_t C, int32_t ks, int32_t mode, void* out, fmd_stream_t s);
/* The same for 2-D (dims 2, as above) or 3-D (dims 3) masters: [K][C][3][3][3] fp32 -> the 3-D tiles of
 * fmd_conv_s2d / fmd_conv_d2s (mode 0: 3 depth taps x the 2-D chunks; mode 1: the 4 folded depth taps; mode 2: rows
 * 8C class-major, 2 depth offsets). */
int64_t fmd_s2d_tiled_size_nd(int32_t K, int32_t C, int32_t mode, int32_t ks, int32_t dims);
int fmd_s2d_tile_weights_nd(const float* w, int32_t K, int32_t C, int32_t ks, int32_t mode, int32_t dims, void* out,
                            fmd_stream_t s);

/* Small-level conv in ONE launch (csrc/conv_small.hip): the sampler's low-resolution levels, where the split-K
 * implicit GEMM needed a combine launch and a GroupNorm launch beside every conv.  A workgroup owns up to 64 output
 * pixels (64-pixel blocks of one image, or whole images when Ho*Wo < 64) x 16 output channels and the FULL reduction:
 * the input rows its taps read (all C = C0 + C1 channels) are staged once in LDS with the GroupNorm affine
 * (+ scale/shift) + SiLU applied -- the affine folded in-kernel from the producers' statistics slabs -- and eight
 * waves split the 32-channel chunks, combining in LDS in a fixed order.  Replaces, per conv, ResBlockND's
 * GroupNorm(+scale/shift)+SiLU -> ConvND 3x3 (src/nn/blocks/residual.py:84-120, normalization.py:11-19,
 * convolution.py:8-54) with the time-embedding add, the 1x1 skip conv + residual add (residual.py:77-82, 120),
 * DownsampleND's stride-2 conv and UpsampleND's nearest-x2 + conv (upsampling.py:8-62), and emits the per-channel
 * statistics the next GroupNorm folds.  Forward only (no saved affine for a backward). */
typedef struct fmd_conv_small_desc {
  int32_t N, Hs, Ws, C0, C1; /* input bf16 NHWC [N][Hs][Ws][C0] (+ [N][Hs][Ws][C1], virtual concat) */
  int32_t Ho, Wo, K;         /* output bf16 NHWC [N][Ho][Wo][K] */
  int32_t mode;              /* 0: 3x3 stride 1 pad 1; 1: 3x3 stride 2 pad 1; 2: nearest-x2 gather, 3x3 s1 p1;
                                3: 1x1 (the centre tap of a 3x3 on 1x1 images) */
  const void* src0;
  const void* src1;
  const void* wgt;           /* bf16 [K][T][C0 + C1], T = 9 (modes 0-2) or 1: fmd_prep_weights mode 0 */
  const float* st0;          /* GroupNorm prologue when non-NULL: statistics slab of src0 [N*Hs*Ws/rows0][C0][2] */
  int32_t rows0;             /*   (sum, sum of squares per rows0-pixel block of one image) */
  const float* st1;          /* ... of src1 (C1 > 0) */
  int32_t rows1;
  int32_t G;                 /* groups */
  float eps;
  const float* gamma;        /* [C0 + C1] or NULL */
  const float* beta;
  const float* emb;          /* scale-shift norm: [N][emb_stride] scale | shift, or NULL */
  int32_t emb_stride;
  int32_t silu;              /* SiLU after the affine */
  const void* src2;          /* 1x1 segment (ResBlock skip conv) over raw (src2 | src3) at the OUTPUT pixels, */
  const void* src3;          /*   bf16 [N][Ho][Wo][C2] (+ [N][Ho][Wo][C3]); C2 = 0: none (modes 0 and 3 only) */
  int32_t C2, C3;
  const void* wgt2;          /* bf16 [K][C2 + C3] */
  const float* bias;         /* [K] or NULL */
  const float* bias2;        /* [K] or NULL (skip-conv bias) */
  const float* bias_nc;      /* per-sample bias [N][bias_nc_stride] (time-embedding add) or NULL */
  int32_t bias_nc_stride;    /* 0: K */
  const void* resid;         /* bf16 [N][Ho][Wo][K] or NULL */
  void* out;
  float* stats;              /* NULL or [N*Ho*Wo/srows][K][2] of the bf16 outputs, srows = 64 if Ho*Wo % 64 == 0
                                else Ho*Wo (one row per image) */
  float* part;               /* split of the reduction over input channels (grids smaller than the chip): fp32
                                partial tiles, part_bytes bytes; NULL: no split */
  int64_t part_bytes;
  uint32_t* tickets;         /* [n_tickets] arrival counters of the in-launch combine: zero before first use, left
                                zero by every completed launch; one set per stream (launches on it serialise) */
  int32_t n_tickets;
  int32_t split;             /* parts: 0 chosen by the plan (enough workgroups for the chip), 1 none, 2..16 forced */
} fmd_conv_small_desc;
/* LDS bytes the launch needs (> 0), or a negative code when the problem does not qualify (geometry, channel
 * counts, or more than one CU's LDS). */
int fmd_conv_small_plan(const fmd_conv_small_desc* d);
/* The number of parts the plan splits the reduction into (>= 1), or the plan's negative code. */
int fmd_conv_small_split(const fmd_conv_small_desc* d);
int fmd_conv_small(const fmd_conv_small_desc* d, fmd_stream_t s);

/* UNet output head: out = conv3x3(SiLU(a*h + b)) to K <= 8 channels, fp32 NHWC [N][H][W][8]
 * (channels >= K zero), replacing the final GroupNorm -> SiLU -> ConvND of
 * src/models/unet/unet.py:286-293 (unet_diffusers_nd.py conv_norm_out/conv_act/conv_out).
 * D == 0: 2-D, h bf16 NHWC [N][H][W][C], w fp32 [K][C][3][3] (reference layout).
 * D >= 1: 3-D (ConvND with dims=3), h [N][D][H][W][C], w [K][C][3][3][3], out [N][D][H][W][8], zero depth
 * padding; K <= 2.  pro_a/pro_b: [N][C] GroupNorm affine; H, W multiples of 16, C a multiple of 32. */
int fmd_head_fwd(const void* h, int32_t N, int32_t D, int32_t H, int32_t W, int32_t C, const float* pro_a,
                 const float* pro_b, const float* w, const float* bias, int32_t K, float* out, fmd_stream_t s);
/* Data gradient of the head: dz = silu'(a*h + b) * conv^T(dpred) (bf16, h's layout) and the
 * GroupNorm-backward sums (sum dz, sum dz*h) per 64-pixel slab row: stats [N*D*H*W/64][C][2].
 * dpred: bf16 [..][8] in h's layout; D as in fmd_head_fwd. */
int fmd_head_dgrad(const void* dpred, const float* w, int32_t K, const void* h, const float* pro_a, const float* pro_b,
                   int32_t N, int32_t D, int32_t H, int32_t W, int32_t C, void* dz, float* stats, fmd_stream_t s);
/* Weight gradient of the head: dw[K][C][taps] += sum_p dpred (x) SiLU(a*h + b), db[K] += sum_p dpred. */
int64_t fmd_head_wgrad_workspace(int32_t N, int32_t D, int32_t H, int32_t W, int32_t C, int32_t K);
int fmd_head_wgrad(const void* dpred, int32_t K, const void* h, const float* pro_a, const float* pro_b, int32_t N,
                   int32_t D, int32_t H, int32_t W, int32_t C, float* dw, float* db, float* ws, fmd_stream_t s);

/* Weight-gradient GEMM: dW[K][C][kh][kw] (+)= sum_p dY[p][K] x gather(src)[p][tap][C]
 * with the same gather/prologue as the forward; db[K] (+)= sum_p dY[p][K].
 * Replaces autograd of nn.Conv2d weight/bias (convolution.py:53). */
typedef struct fmd_wgrad_desc {
  int32_t N, Hs, Ws, C0, C1, Ho, Wo, K, ks, stride, pad, upsample;
  const void* src0; const void* src1;
  const float* pro_a; const float* pro_b; int32_t pro_silu;
  const void* dy;           /* bf16 [N][Ho][Wo][ldy], first K channels used */
  int32_t ldy;              /* dy row stride in elements (0 -> K) */
  float* dw;                /* fp32 [K][C][ks][ks] (reference layout) */
  float* db;                /* fp32 [K] or NULL */
  int32_t accumulate;
  float* ws;                /* fp32 workspace, size fmd_wgrad_workspace() floats */
  int32_t splits;           /* split-K over pixels (halo path: over 8x16-pixel tiles) */
  int32_t force_generic;    /* 1: never use the halo-tiled kernel (tests) */
  int32_t Ds, Do;           /* 3-D: stored / output depth (0 = 2-D); dw [K][C][ks][ks][ks] */
} fmd_wgrad_desc;

/* Dispatches 3x3 stride-1 problems (K % 128 == 0, C % 64 == 0, Ho % 8 == 0, Wo % 16 == 0) to the
 * halo-tiled kernel (csrc/wgrad_halo.hip), everything else to the per-tap kernel (csrc/wgrad.hip). */
int fmd_wgrad(const fmd_wgrad_desc* d, fmd_stream_t s);
/* Halo-tiled 3x3 weight gradient (partial slabs only, no reduce); returns 1 when not applicable. */
int fmd_wgrad_halo(const fmd_wgrad_desc* d, fmd_stream_t s);
int64_t fmd_wgrad_workspace(const fmd_wgrad_desc* d);

/* Grouped weight gradients: the n <= FMD_WGRAD_GROUP_MAX problems run as ONE MFMA launch and ONE combine
 * launch.  Each desc keeps its own ws / splits / dw / db / accumulate exactly as for fmd_wgrad, and each job's
 * arithmetic and summation order are those of fmd_wgrad with the same splits (bit-identical results).  All
 * jobs must use the same kernel instance -- the halo kernel with the same prologue form and stride, or all
 * the generic kernel -- otherwise a negative code is returned and nothing is launched.  The job table
 * travels by value in the kernel arguments, so the call is safe under stream capture. */
#define FMD_WGRAD_GROUP_MAX 16
int fmd_wgrad_group(const fmd_wgrad_desc* descs, int32_t n, fmd_stream_t s);
/* The halo launch of a group alone (partial slabs only, no reduce); 1 when no job qualifies. */
int fmd_wgrad_halo_group(const fmd_wgrad_desc* descs, int32_t n, fmd_stream_t s);
/* The combine of fmd_wgrad alone: dw / db (+)= the sum of the d->splits partial slabs in d->ws (layout of
 * fmd_wgrad_workspace), for producers that write the slabs themselves (fmd_skip_bwd). */
int fmd_wgrad_combine(const fmd_wgrad_desc* d, fmd_stream_t s);

/* The whole backward of the ResBlock's 1x1 skip conv in one pass over dy and the block input (csrc/skip_bwd.hip):
 * dx = round_bf16(dy . W_s^T) + P*dz + Q*x + R (+ dx) exactly as fmd_conv_gn_apply (bit-identical), and
 * dW_s[Kd][C] (+)= dy^T . x, db_s[Kd] (+)= sum_p dy from the same staged tiles (persistent workgroups, fp32 partial
 * slabs, one fmd_wgrad_combine).  Replaces fmd_conv_gn_apply + the ks = 1 fmd_wgrad of the same block
 * (autograd of the skip nn.Conv2d, src/nn/blocks/residual.py:77-82,120). */
typedef struct fmd_skip_bwd_desc {
  int32_t N, HW;            /* images, pixels per image (any spatial rank): M = N * HW */
  int32_t C0, C1, Kd;       /* concat sources of the block input; skip-conv output channels */
  const void* dy;           /* bf16 [M][Kd] */
  const void* wgt_t;        /* bf16 [C0 + C1][Kd]: mode-1 (data-gradient) weights */
  fmd_gn_apply_desc g;      /* as for fmd_conv_gn_apply; g.C0 == C0 */
  float* dw;                /* fp32 [Kd][C0 + C1] (reference layout, 1x1) */
  float* db;                /* fp32 [Kd] or NULL */
  int32_t accumulate;
  float* ws;                /* fp32 workspace, plan.ws_floats */
  int32_t groups;           /* 0: the plan's pixel groups; > 0: forced (tests) */
  int32_t num_cu;           /* compute units of the device (0: 256) */
  int32_t min_tiles;        /* the plan's own groups: taken only with at least this many 64-pixel tiles per group */
} fmd_skip_bwd_desc;
typedef struct fmd_skip_bwd_plan_t {
  int32_t taken;            /* 0: not taken -- run fmd_conv_gn_apply + fmd_wgrad */
  int32_t c_tile;           /* input channels per workgroup */
  int32_t workgroups;       /* pixel groups x c-tiles launched */
  int32_t slabs;            /* partial slabs written: min(pixel groups, pixel tiles) */
  int64_t ws_floats;        /* slabs * (Kd * C + Kd): exactly what the launch writes */
} fmd_skip_bwd_plan_t;
/* Host arithmetic only (reads the descriptor's scalars).  Returns 0 (taken) or 1 (not taken). */
int fmd_skip_bwd_plan(const fmd_skip_bwd_desc* d, fmd_skip_bwd_plan_t* out);
/* -1: the plan refuses the descriptor (nothing launched). */
int fmd_skip_bwd(const fmd_skip_bwd_desc* d, fmd_stream_t s);

/* ------------------------------------------------------------- groupnorm
 * nn.GroupNorm (src/nn/ops/normalization.py:11-19, attention.py:97) is never
 * materialised: producers emit per-channel sums, fmd_gn_prep folds mean/rstd,
 * gamma/beta and the ResBlock scale/shift into a per-(n,c) affine consumed by
 * the conv prologue. */
int fmd_channel_stats(const void* x, const void* y0, const void* y1, int32_t C0, int32_t N, int32_t HW, int32_t C,
                      int32_t rows, float* out /* [N*HW/rows][C][2] */, fmd_stream_t s);
/* Slab fold: out[j] = sum of slab rows [j*fold, (j+1)*fold) of a [rows_total][C][2] statistics slab (fold must not
 * straddle images: (HW/rows) % fold == 0).  Used before fmd_gn_prep / fmd_gn_bwd_prep on slabs with thousands of
 * rows per image (config E's 128^3 levels). */
int fmd_stats_fold(const float* slab, int64_t rows_total, int32_t C, int32_t fold, float* out, fmd_stream_t s);
int fmd_gn_prep(const float* st0, int32_t rows0, const float* st1, int32_t rows1, int32_t N, int32_t HW,
                int32_t C0, int32_t C1, int32_t G, float eps, const float* gamma, const float* beta,
                const float* emb, int32_t emb_stride, int32_t emb_mode /*0 none,1 scale-shift*/,
                float* a, float* b, float* mean_rstd, fmd_stream_t s);
/* emb_mode 0: plain GN; 1: scale/shift (demb = [dscale | dshift]); 2: embedding added to the GN
 * input (demb[n][c] = sum_hw dx, from the forward channel sums fwd_st of x). */
int fmd_gn_bwd_prep(const float* s12, int32_t rows, int32_t N, int32_t HW, int32_t C, int32_t G,
                    const float* mean_rstd, const float* gamma, const float* beta, const float* emb,
                    int32_t emb_stride, int32_t emb_mode, float* P, float* Q, float* R,
                    float* dgamma, float* dbeta, float* demb, int32_t demb_stride, const float* fwd_st,
                    int32_t fwd_rows, float* ws /* [N][C][2] scratch */, fmd_stream_t s);
/* Deferred gamma/beta gradients: fmd_gn_bwd_prep called with dgamma = dbeta = NULL leaves the per-(n,c)
 * partials in its ws; one fmd_gn_gb_fold launch (<= FMD_GB_MAX jobs) then adds sum_n of every job's
 * partials to its dgamma/dbeta -- one launch per backward pass instead of one per GroupNorm. */
#define FMD_GB_MAX 64
typedef struct {
  const float* ws;   /* [N][C][2] (dgamma, dbeta) partials */
  float* dgamma;     /* [C] += , may be NULL */
  float* dbeta;      /* [C] += , may be NULL */
  int32_t N, C;
} fmd_gb_job;
int fmd_gn_gb_fold(const fmd_gb_job* jobs, int32_t njobs, fmd_stream_t s);
/* t = SiLU(a*x + b) (silu != 0) or a*x + b over the concat x0|x1 (bf16 [M][C0+C1]): the GroupNorm
 * prologue materialised once for its consumers. */
/* Whole GroupNorm forward of a small level (HW * C/G <= 16384) in one launch, straight from x0|x1: per
 * (n, group) statistics, a/b (+ emb scale/shift, emb_mode 1), mean/rstd, and t = [SiLU](a*x + b) over the
 * channel concat (= fmd_channel_stats + fmd_gn_prep + fmd_gn_apply_fwd).  C/G % 4 == 0, C0 % 4 == 0. */
int fmd_gn_fused_apply(const void* x0, const void* x1, int32_t C0, int32_t C1, int32_t N, int32_t HW, int32_t G,
                       float eps, const float* gamma, const float* beta, const float* emb, int32_t emb_stride,
                       int32_t emb_mode, int32_t silu, float* a, float* b, float* mean_rstd, void* t,
                       fmd_stream_t s);
int fmd_gn_apply_fwd(const void* x0, const void* x1, int32_t C0, int32_t C1, int64_t M, int32_t HW,
                     const float* a, const float* b, int32_t silu, void* t, fmd_stream_t s);

/* ResBlockND dropout (replaces nn.Dropout in out_layers, src/nn/blocks/residual.py:117): y = x * keep / (1-p)
 * over NHWC bf16 [M pixels][C], keep = hash(seed[0], salt, element index) >= p * 2^32 (regenerated, not
 * stored).  With ep_x (bf16 [M][C]) and ep_a/ep_b ([N][C] fp32, N = M / HW) it is the backward through the
 * dropout and the GN+SiLU prologue: y = x * keep / (1-p) * silu'(ep_a * ep_x + ep_b).  x == y is allowed. */
int fmd_dropout_apply(const void* x, int32_t C, int64_t M, int32_t HW, float p, const int32_t* seed, uint32_t salt,
                      const void* ep_x, const float* ep_a, const float* ep_b, void* y, fmd_stream_t s);
int fmd_gn_bwd_apply(const void* dz, const void* x0, const void* x1, int32_t C0, int32_t C1, int64_t M,
                     int32_t HW, const float* P, const float* Q, const float* R, const void* extra,
                     void* dx0, int32_t acc0, void* dx1, int32_t acc1, fmd_stream_t s);

/* -------------------------------------------------- weights and layouts
 * fp32 reference-layout conv weight -> bf16 kernel layout.  mode 0: [Kpad][T][Cpad]
 * forward; mode 1: [Cpad][T][Kpad] data gradient (transposed gather); mode 2:
 * [Cpad][16][Kpad] data gradient of nearest-x2 upsample + 3x3 conv (4x4 taps). */
int fmd_prep_weights(const float* w, int32_t K, int32_t C, int32_t ks, int32_t mode, int32_t Kpad, int32_t Cpad,
                     void* out, fmd_stream_t s);
/* Same for any tap count T (w [K][C][T], e.g. T = 27 for a 3x3x3 kernel); modes 0, 1 and 3 (3 = mode 1
 * with the taps reversed: the stride-1 data gradient as a forward gather). */
int fmd_prep_weights_t(const float* w, int32_t K, int32_t C, int32_t T, int32_t mode, int32_t Kpad, int32_t Cpad,
                       void* out, fmd_stream_t s);
/* All bf16 weight layouts of a model in one launch (after each optimizer step).  jobs: device int64
 * [njobs][16], one per fp32 master w[K][C][ks*ks] = {w, K | C<<32, ks | nout<<32, first block | ktiles<<32,
 * then nout (<= 6) pairs {out, mode | kind<<8 | R<<16 | Cc<<40}}; kind 0 = the fmd_prep_weights layout
 * (R rows x T x Cc), kind 1 = its halo tiles.  A block covers a 32x32 (k, c) tile of one master; jobs
 * sorted by first block; nblocks = total. */
int fmd_prep_weights_batch(const void* jobs, int32_t njobs, int32_t nblocks, fmd_stream_t s);
/* The same for cubic 3x3x3 masters w[K][C][27] (job ks = 3): blocks cover 16 (k) x 32 (c) tiles (ktiles counts
 * 16-row k tiles); kinds 0 / 1 as above with T = 27, and kind 2 = the depth-tap halo kernel's tiles of the
 * [R][3*Cr][3][3] view (channel block kz*Cr + c = depth tap kz of channel c; Cr = Cc rounded up to 32):
 * [ceil(R/128)][3*Cr/32][9][4][128][8] (modes 0 and 3). */
int fmd_prep_weights_batch_cubic(const void* jobs, int32_t njobs, int32_t nblocks, fmd_stream_t s);
int fmd_nchw_to_nhwc(const float* x, int32_t N, int32_t C, int32_t HW, int32_t Cpad, void* y, fmd_stream_t s);
int fmd_nhwc_to_nchw(const void* y, int32_t src_f32, int32_t N, int32_t C, int32_t HW, int32_t Cs, float* x,
                     fmd_stream_t s);
/* Parameter-free resampling by 2 along the dims whose factor (fz, fy, fx) is 2, NDHWC bf16 (2-D: D = 1; 1-D:
 * D = H = 1).  up = 0: dst[low] (+)= scale * sum of src's 2^d block -- AvgPoolND(kernel=stride=2)
 * (src/nn/ops/pooling.py:33-53, scale 1/2^d; DownsampleND(use_conv=False), upsampling.py:52-58) and the
 * nearest-x2 data gradient (scale 1).  up = 1: dst[high] (+)= scale * src[high >> 1] -- UpsampleND(use_conv=
 * False)'s F.interpolate(scale_factor=2, mode="nearest") (upsampling.py:24-29, scale 1) and the avg-pool data
 * gradient (scale 1/2^d).  High extents are 2*low or 2*low + 1 (floor pooling of an odd extent) along a
 * factor-2 dim and equal to the low extent along a factor-1 dim; anything else returns -1. */
int fmd_resample2(const void* src, int32_t N, int32_t Dl, int32_t Hl, int32_t Wl, int32_t Dh, int32_t Hh, int32_t Wh,
                  int32_t C, int32_t fz, int32_t fy, int32_t fx, int32_t up, float scale, void* dst, int32_t acc,
                  fmd_stream_t s);
int fmd_sum_pool2(const void* src, int32_t N, int32_t H, int32_t W, int32_t C, void* dst, int32_t acc, fmd_stream_t s);
/* dst[n][z][y][x][c] (+)= sum of the 2x2x2 block of src (bf16 NDHWC, src 2D x 2H x 2W): the data gradient
 * of a nearest-x2 3-D upsample. */
int fmd_sum_pool2_3d(const void* src, int32_t N, int32_t D, int32_t H, int32_t W, int32_t C, void* dst,
                     int32_t acc, fmd_stream_t s);
int fmd_add_bf16(const void* a, void* dst, int64_t n, fmd_stream_t s);

/* ------------------------------------------------------ time embedding
 * timestep_embedding (src/nn/ops/time_embedding.py:4-32), the time MLP
 * (src/models/unet/unet.py:117-121, src/models/unet/utils.py:9-24) and the
 * ResBlock emb_layers (src/nn/blocks/residual.py:63-68,102-104). */
/* t_eff = t*t_scale, truncated to an integer when t_trunc (the FM trainer's (t*(N-1)).long()) */
int fmd_timestep_embedding(const float* t, int32_t N, int32_t dim, int32_t flip, int32_t shift, float max_period,
                           float t_scale, int32_t t_trunc, float* out, fmd_stream_t s);
int fmd_linear(const float* x, int32_t B, int32_t I, const float* w, const float* b, int32_t O, int32_t in_silu,
               float* y, int32_t y_stride, fmd_stream_t s);
int fmd_linear_bwd(const float* x, int32_t B, int32_t I, const float* w, int32_t O, int32_t in_silu,
                   const float* dy, int32_t dy_stride, float* dx, int32_t dx_acc, float* dw, float* db,
                   fmd_stream_t s);
/* Grouped linears: every ResBlock emb_layers projection of the UNet in one launch.  groups: device
 * array of {const float* w; const float* b; float* dw; float* db; int64 O; int64 off} (row offset of the
 * group in y / dy); blocks: device int2 array {group, first row} of 64-row blocks.  The backward
 * accumulates dW/db (+=) and writes / accumulates dx (with SiLU' when in_silu). */
int fmd_grouped_linear(const float* x, int32_t B, int32_t I, const void* groups, const void* blocks, int32_t nblk,
                       int32_t in_silu, float* y, int32_t y_stride, fmd_stream_t s);
int64_t fmd_grouped_linear_bwd_workspace(int32_t B, int32_t I, int32_t nblk);
int fmd_grouped_linear_bwd(const float* x, int32_t B, int32_t I, const void* groups, const void* blocks,
                           int32_t nblk, int32_t in_silu, const float* dy, int32_t dy_stride, float* dx,
                           int32_t dx_acc, float* ws, fmd_stream_t s);
int fmd_silu_bwd_f32(const float* x, const float* dy, float* dx, int64_t n, fmd_stream_t s);

/* ----------------------------------------------------------- attention
 * Softmax attention (F.scaled_dot_product_attention inside SpatialSelfAttention / DiffusersAttentionND /
 * SpatialCrossAttention) runs on the MFMA kernels declared further down (fmd_attn_pack / fmd_attn_mfma_fwd /
 * fmd_attn_mfma_bwd / fmd_attn_unpack). */
/* LinearQKVAttention (src/nn/blocks/attention.py:53-70) inside SpatialSelfAttention(use_linear=True)
 * (attention.py:104-117; same raw head split): out = softmax_d(q) (softmax_tokens(k)^T v / (sum ks + eps)).
 * ``state`` (fmd_linear_attention_state floats) is written by the forward and read by the backward;
 * ``ws`` holds fmd_linear_attention_workspace floats. dh <= 64. */
/* SpatialCrossAttention (attention.py:120-189): q [B][Tq][inner] (q_proj output), kv [B][Tk][2*inner]
 * (kv_proj output), raw head split q.reshape(b, heads, Tq, dh), kv.reshape(b, heads, Tk, 2dh).chunk(2).
 * linear must be 1: LinearQKVAttention (lse_or_state = fmd_linear_attention_state floats, ws = workspace);
 * linear = 0 returns -2 (softmax cross-attention is fmd_attn_mfma_fwd / fmd_attn_mfma_bwd). */
int fmd_cross_attention_fwd(const void* q, const void* kv, int32_t B, int32_t Tq, int32_t Tk, int32_t heads,
                            int32_t dh, int32_t raw, int32_t linear, float eps, void* o, float* lse_or_state,
                            float* ws, fmd_stream_t s);
int fmd_cross_attention_bwd(const void* q, const void* kv, const void* o, const void* dout, const float* lse_or_state,
                            float* ws_or_delta, int32_t B, int32_t Tq, int32_t Tk, int32_t heads, int32_t dh,
                            int32_t raw, int32_t linear, float eps, void* dq, void* dkv, fmd_stream_t s);
/* Softmax attention on MFMA (csrc/attention_mfma.hip), the path behind every softmax attention block
 * (attention.py:42-44, 115, 185, 269).  The reference's head split (raw reshape or view/transpose; self:
 * src_q = src_kv = qkv [B][T][3*inner]; cross: src_q = q [B][Tq][inner], src_kv = kv [B][Tk][2*inner];
 * which 3 = the attention output o [B][Tq][inner]) is undone into canonical bf16 planes
 * [B*heads][rows][fmd_attn_head_pad(dh)] (q/o/dq plane cq, k plane ck, v plane cv; pad zero-filled).
 * fmd_attn_pack gathers planes which0..which1 (0 q, 1 k, 2 v, 3 o/dout into cq); fmd_attn_unpack scatters
 * them back (0..2 into dst_q for self attention = dqkv, into dst_q / dst_kv for cross; 3 into dst_q).
 * fmd_attn_mfma_fwd: co = softmax(cq ck^T / sqrt(dh)) cv, lse [B*heads][Tq] (natural log).
 * fmd_attn_mfma_bwd: delta [B*heads][Tq] scratch, writes cdq, cdk, cdv.  dh <= 64. */
int32_t fmd_attn_head_pad(int32_t dh);
int fmd_attn_pack(const void* src_q, const void* src_kv, int32_t B, int32_t Tq, int32_t Tk, int32_t heads,
                  int32_t dh, int32_t raw, int32_t cross, int32_t which0, int32_t which1, void* cq, void* ck,
                  void* cv, fmd_stream_t s);
int fmd_attn_unpack(const void* cq, const void* ck, const void* cv, int32_t B, int32_t Tq, int32_t Tk,
                    int32_t heads, int32_t dh, int32_t raw, int32_t cross, int32_t which0, int32_t which1,
                    void* dst_q, void* dst_kv, fmd_stream_t s);
int fmd_attn_mfma_fwd(const void* cq, const void* ck, const void* cv, int32_t BH, int32_t Tq, int32_t Tk,
                      int32_t dh, void* co, float* lse, fmd_stream_t s);
int fmd_attn_mfma_bwd(const void* cq, const void* ck, const void* cv, const void* co, const void* cdo,
                      const float* lse, float* delta, int32_t BH, int32_t Tq, int32_t Tk, int32_t dh, void* cdq,
                      void* cdk, void* cdv, fmd_stream_t s);
/* context_norm of SpatialCrossAttention: GroupNorm over the fp32 context ((N, C, T) or token-major (N, T, C))
 * -> bf16 [N][T][Cpad] (zero pad channels); mr [N][groups][2] = mean, rstd.  The backward accumulates
 * dgamma / dbeta only (the context is conditioning data). */
int fmd_context_norm_fwd(const float* ctx, int32_t N, int32_t C, int32_t T, int32_t tok_major, int32_t groups,
                         float eps, const float* gamma, const float* beta, int32_t Cpad, void* out, float* mr,
                         fmd_stream_t s);
int fmd_context_norm_bwd(const float* ctx, int32_t N, int32_t C, int32_t T, int32_t tok_major, int32_t groups,
                         const float* mr, const void* dout, int32_t Cpad, float* dgamma, float* dbeta,
                         fmd_stream_t s);
size_t fmd_linear_attention_workspace(int32_t B, int32_t heads);
size_t fmd_linear_attention_state(int32_t B, int32_t heads);
int fmd_linear_attention_fwd(const void* qkv, int32_t B, int32_t T, int32_t heads, int32_t dh, int32_t raw,
                             float eps, void* o, float* state, float* ws, fmd_stream_t s);
int fmd_linear_attention_bwd(const void* qkv, const void* dout, const float* state, float* ws, int32_t B, int32_t T,
                             int32_t heads, int32_t dh, int32_t raw, float eps, void* dqkv, fmd_stream_t s);

/* ------------------------------------------ train step / sampler / optim
 * FM input x_t = (1-t)x0 + t*eps and DDPM add_noise (flow_matching_lib.py:151-158,
 * diffusion_lib.py:154-160) -> NHWC model input with the concatenated
 * conditioning; MSE loss + gradient (flow_matching_lib.py:166-167); the
 * FlowMatchEuler / DDPM step (diffusers, called at src/pipelines/utils.py:218);
 * torch.optim.AdamW (flow_matching_lib.py:73,177). */
/* x channels: ca&&cb: ca[n]*x0 + cb[n]*noise (DDPM add_noise); ca only: (1-ca[n])*x0 + ca[n]*noise
 * (FM, ca = t); neither: noise (sampler input). */
int fmd_noise_prepare(const float* x0, const float* noise, const float* ca, const float* cb, const float* cond,
                      int32_t N, int32_t HW, int32_t Cx, int32_t Cc, int32_t Cpad, void* inp, fmd_stream_t s);
/* diffusers DDPMScheduler.add_noise (diffusion_lib.py:158, diffusion_utils.py:162/222) in fp32:
 * out[n] = sqrt_acp[t[n]] * x0[n] + sqrt_1m_acp[t[n]] * noise[n] over per_sample elements per sample,
 * torch's operation order (two rounded products, one rounded add): bit-exact with the eager op.
 * sqrt_acp / sqrt_1m_acp: [num_train_timesteps] fp32 tables; timesteps: int64 [N] on the device. */
int fmd_add_noise(const float* x0, const float* noise, const float* sqrt_acp, const float* sqrt_1m_acp,
                  const int64_t* timesteps, int32_t N, int64_t per_sample, float* out, fmd_stream_t s);
int fmd_mse(const float* pred, int32_t Kpad, const float* ta, const float* tb, float tb_sign, int32_t N, int32_t Cx,
            int32_t HW, float grad_scale, float* partial, int32_t max_blocks, float* loss, void* dpred,
            fmd_stream_t s);
int fmd_adamw(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
              float wd, float bc1, float bc2, fmd_stream_t s);
/* AdamW with the step count on device and get_cosine_schedule_with_warmup's LR computed in-kernel
 * (graph-replayable train step); g is scaled by grad_scale first. */
int fmd_adamw_sched(float* p, const float* g, float* m, float* v, int64_t n, const int32_t* step_ctr, float base_lr,
                    int32_t warmup, int32_t total, float beta1, float beta2, float eps, float wd, float grad_scale,
                    fmd_stream_t s);
/* fmd_adamw_sched plus, in the same pass, an exponential moving average of the parameters (ema: a fifth flat fp32
 * buffer of n elements).  With s = step_ctr[0] (0-based, the s of the LR schedule):
 *   d   = ema_warmup ? min(ema_decay, (1 + s) / (10 + s)) : ema_decay
 *   ema = ema + (1 - d) * (p_new - ema)
 * p_new is the parameter this launch has just computed.  Every operation is one rounded fp32 operation (division,
 * subtraction, multiply, add; none contracted), so separate fp32 ops on the host reproduce the bits.  p, m, v are
 * written exactly as by fmd_adamw_sched.  Returns -1 for a NULL ema or ema_decay outside [0, 1). */
int fmd_adamw_sched_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const int32_t* step_ctr,
                        float base_lr, int32_t warmup, int32_t total, float beta1, float beta2, float eps, float wd,
                        float grad_scale, float ema_decay, int32_t ema_warmup, fmd_stream_t s);
int fmd_flow_euler(float* x, const float* v, int32_t Kpad, const float* sigmas, const int32_t* index, int32_t N,
                   int32_t Cx, int32_t HW, const float* cond, int32_t Cc, int32_t Cpad, void* next, fmd_stream_t s);
/* noise: DDPM variance noise, a per-step table whose row 0 belongs to step noise_base (row = index - noise_base),
 * or, with noise_base < 0, one [N][Cx][HW] buffer refilled before every step; NULL for DDIM / the last step. */
int fmd_ddpm_step(float* x, const float* eps, int32_t Kpad, const float* coef, const int32_t* index,
                  const float* noise, int32_t noise_base, int32_t N, int32_t Cx, int32_t HW, const float* cond,
                  int32_t Cc, int32_t Cpad, void* next, fmd_stream_t s);
int fmd_fill_from_table(const float* table, const int32_t* index, float* out, int32_t N, fmd_stream_t s);
/* out = sum_k c[k] * in[k] over n fp32 elements: the multistep scheduler updates (DPM-Solver / UniPC,
 * replaces diffusers' DPMSolverMultistepScheduler.step / UniPCMultistepScheduler.step tensor arithmetic,
 * called at src/pipelines/utils.py:218).  out may alias an input.  n % 4 == 0 needs 16-byte alignment. */
#define FMD_LINCOMB_MAX 6
typedef struct {
  float* out;
  const float* in[FMD_LINCOMB_MAX];
  float c[FMD_LINCOMB_MAX];
  int32_t nin;
  int64_t n;
} fmd_lincomb_desc;
int fmd_lincomb(const fmd_lincomb_desc* d, fmd_stream_t s);
/* One multistep-solver step with every scalar taken from row index[0] of a per-step coefficient table, so a
 * whole DPM-Solver / UniPC sampling loop replays from one captured step (the graph-replayed form of the
 * DPMSolverMultistepScheduler.step / UniPCMultistepScheduler.step arithmetic, reference call site
 * src/pipelines/utils.py:218).  Per element of the sample (step i = index[0], r(j) = ring[j & 3]):
 *   m      = c[0]*x + c[1]*eps                                   (data prediction; dpmsolver: eps itself)
 *   r(i)   = m
 *   xc     = c[2] != 0 ? c[3]*last + c[4]*r(i-1) + c[5]*r(i-2) + c[6]*r(i-3) + c[7]*m : x   (UniPC corrector)
 *   last   = xc                                                  (if last != NULL)
 *   x      = c[8]*xc + c[9]*r(i) + c[10]*r(i-1) + c[11]*r(i-2)   (predictor / solver update)
 * each sum accumulated left to right from 0 with fused multiply-adds, as fmd_lincomb does, so the step equals
 * the eager scheduler's fmd_lincomb calls on the same coefficients.  x: [N][Cx][HW] fp32; eps: the UNet
 * output [N*HW][Kpad] fp32; ring / last: [N][Cx][HW] fp32; next (optional): the next model input
 * (NHWC bf16 [N*HW][Cpad], x then cond channels, zero padded) as fmd_flow_euler writes it. */
#define FMD_SCHED_NCOEF 12
typedef struct {
  float* x;
  const float* eps;
  float* ring[4];
  float* last;
  const float* coef;        /* [steps][FMD_SCHED_NCOEF] */
  const int32_t* index;
  int32_t N, Cx, HW, Kpad;
  const float* cond;
  int32_t Cc, Cpad;
  void* next;
} fmd_sched_step_desc;
int fmd_sched_step(const fmd_sched_step_desc* d, fmd_stream_t s);
/* out[0:n] = table[index[0]*n : (index[0]+1)*n] -- a per-step row (e.g. precomputed time embeddings of a
 * sampling schedule) selected by a device-side step counter, so the step stays graph-replayable. */
int fmd_gather_row(const float* table, const int32_t* index, int64_t n, float* out, fmd_stream_t s);
int fmd_counter_add(int32_t* c, int32_t v, fmd_stream_t s);
/* y = x (NHWC bf16, Cpad channels per pixel) with channels [0, C) mapped to scale * x + shift: the model
 * input centring of UNetDiffusersND(center_input_sample=True), `x = 2 * x - 1.0`
 * (src/models/unet/unet_diffusers_nd.py:156-157), applied to the packed input (one extra bf16 rounding). */
int fmd_affine_channels(const void* x, int32_t C, int32_t Cpad, int64_t npix, float scale, float shift, void* y,
                        fmd_stream_t s);

/* ------------------------------------------------------------- vector quantizer
 * Forward of VectorQuantizer / VectorQuantizerEMA (src/nn/modules/vae/codebook.py:67-84, :109-137) without
 * the M x K distance and one-hot matrices (csrc/vq.hip).  z: M latent vectors of D <= 256 fp32 values with
 * row stride ldz (an NHWC tensor with padded channels); E: the fp32 codebook [K][D].  The nearest code
 * maximises z.e_k - 0.5 |e_k|^2, computed from two bf16 planes per operand (three MFMA products, fp32
 * accumulation) with 0.5 |e_k|^2 in fp32; the lowest index wins equal scores.  Unsupported shapes (D > 256,
 * M or K < 1 or > 2^30) return -1.
 *
 * Call order: fmd_vq_prep once per codebook value, then fmd_vq_argmin -> fmd_vq_finalize -> fmd_vq_stats.
 * Nothing synchronises with the host. */
typedef struct fmd_vq_plan_t {
  int32_t splits;          /* S: code ranges searched by separate workgroups (grid = row blocks x S) */
  int32_t block_rows;      /* latent vectors per argmin workgroup */
  int32_t tile_codes;      /* codes per wave tile */
  int32_t codes_per_split; /* codes of one split (the last may hold fewer) */
  int32_t Kpad, Dpad;      /* plane dims: Eh / El are bf16 [Kpad][Dpad], hn is fp32 [Kpad] */
  int32_t finalize_rows;   /* latent vectors per finalize workgroup: slab holds ceil(M / finalize_rows) floats */
} fmd_vq_plan_t;
/* What fmd_vq_argmin / fmd_vq_finalize will launch for this shape; Kpad and Dpad do not depend on M. */
int fmd_vq_plan(int32_t M, int32_t K, int32_t D, fmd_vq_plan_t* out);
/* Bytes of the argmin workspace: best score fp32 [S][M], then index int32 [S][M].  Negative: unsupported. */
int64_t fmd_vq_workspace(int32_t M, int32_t K, int32_t D);
/* Codebook planes: E = Eh + El (bf16, zero padded to [Kpad][Dpad]); hn[k] = 0.5 |e_k|^2 summed over
 * d = 0 .. D-1 in order, +inf for k >= K. */
int fmd_vq_prep(const float* E, int32_t K, int32_t D, void* Eh, void* El, float* hn, fmd_stream_t s);
int fmd_vq_argmin(const float* z, int32_t ldz, int32_t M, int32_t K, int32_t D, const void* Eh, const void* El,
                  const float* hn, void* ws, fmd_stream_t s);
/* Merges the splits; codes int64 [M]; zq fp32 channels-first [M / HW][D][HW] = z + (q - z), every operation
 * rounded on its own (codebook.py:41); zq_nhwc (optional) bf16 [M][Cpad], channels >= D zero; slab: one
 * partial sum of (q - z)^2 per finalize workgroup; hist int32 [K], zeroed by the caller, += code counts. */
int fmd_vq_finalize(const float* z, int32_t ldz, int32_t M, int32_t HW, int32_t K, int32_t D, const float* E,
                    const void* ws, int64_t* codes, float* zq, void* zq_nhwc, int32_t Cpad, float* slab,
                    int32_t* hist, fmd_stream_t s);
/* out[0] = vq_loss = (classic ? 1 + beta : beta) * mse (forward value of codebook.py:79-81 / :133-134),
 * out[1] = perplexity = exp(-sum p log(p + eps)), p = hist / M (codebook.py:52-53), out[2] = mse. */
int fmd_vq_stats(const float* slab, int32_t nslab, const int32_t* hist, int32_t K, int32_t M, int32_t D, float beta,
                 int32_t classic, float eps, float* out, fmd_stream_t s);

/* Training half (csrc/vq_train.hip), given the codes and the histogram of fmd_vq_finalize.  S_k = the sum of
 * the latent rows with code k is a segmented sum: a workgroup owns a range of codes, scans the M codes in
 * ascending row order and adds its rows to fp64 accumulators in that order, so every S_kd is one fp32 rounding
 * of the exact sum and the same bits on every run.  No atomics, no M x K or K x D temporary, no host
 * synchronisation.  Only the first D channels of a row are read. */
/* Host-side query: codes per workgroup and grid of the segmented-sum launch.  Negative: unsupported shape. */
int fmd_vq_train_plan(int32_t M, int32_t K, int32_t D, int32_t* codes_per_wg, int32_t* grid);
/* The EMA update of codebook.py:120-129, in place on the three fp32 buffers, every one of the K codes:
 *   ema_cluster_size_k <- fma(one_minus_decay, n_k, decay * ema_cluster_size_k),   n_k = hist[k];
 *   n = sum_k ema_cluster_size_k in fp64 (fixed order), rounded to fp32; written to nsum[0] (8 bytes, fp64);
 *   ema_w_kd <- fma(one_minus_decay, S_kd, decay * ema_w_kd);
 *   embedding_kd <- ema_w_kd / (((ema_cluster_size_k + eps) / (n + k_eps)) * n),   k_eps = K * eps.
 * Two launches (cluster sizes and n, then everything else).  Eh / El / hn: the planes of fmd_vq_prep for this
 * codebook, rewritten for the new embedding with the same arithmetic (all three or none). */
int fmd_vq_ema_update(const float* z, int32_t ldz, int32_t M, int32_t K, int32_t D, const int64_t* codes,
                      const int32_t* hist, float decay, float one_minus_decay, float eps, float k_eps,
                      float* ema_cluster_size, float* ema_w, float* embedding, void* Eh, void* El, float* hn,
                      double* nsum, fmd_stream_t s);
/* d_embedding[k][d] = (g_loss[0] * scale) * fma(n_k, embedding_kd, -S_kd): the codebook term of the VQ-VAE
 * loss (the reference sends no gradient to the codebook; an opt-in deviation).  Written, not accumulated. */
int fmd_vq_codebook_grad(const float* z, int32_t ldz, int32_t M, int32_t K, int32_t D, const int64_t* codes,
                         const int32_t* hist, const float* embedding, const float* g_loss, float scale,
                         float* d_embedding, fmd_stream_t s);
/* dz[m][d] = fma((g_loss[0] * c) * scale, z_md - embedding[codes_m][d], g_zq[m][d]) for d < D and 0 for
 * D <= d < lddz; g_zq null: zero.  embedding null: the rows of z already hold z - q (codes is not read).
 * c = beta (EMA quantizer) or beta - 1 (classic), scale = 2 / (M D); g_loss is a device scalar. */
int fmd_vq_backward(const float* z, int32_t ldz, int32_t M, int32_t K, int32_t D, const int64_t* codes,
                    const float* embedding, const float* g_zq, int32_t ldg, const float* g_loss, float c,
                    float scale, float* dz, int32_t lddz, fmd_stream_t s);
/* The latent join of the VQVAE backward: fmd_vq_backward's value, element for element and in its operation order,
 * with g_zq read as the 1x1 data gradient left it (channels-last, g_f32 = 0: bf16, 1: fp32; null: zero) and dz
 * stored as bf16 (one rounding, to nearest even): the channels-last operand of the encoder head's backward, with
 * channels D .. lddz-1 exact zeros.  g_loss null: zero.  Channels >= D of z, g_zq and embedding rows are never
 * read.  1 <= D <= 256; ldg and lddz multiples of 8 and >= D, g_zq and dz 16-byte aligned; ldz >= D.  Returns -1
 * on anything else; one launch, no workspace. */
int fmd_vq_join_bwd(const float* z, int32_t ldz, int32_t M, int32_t K, int32_t D, const int64_t* codes,
                    const float* embedding, const void* g_zq, int32_t g_f32, int32_t ldg, const float* g_loss,
                    float c, float scale, void* dz, int32_t lddz, fmd_stream_t s);

/* ------------------------------------------------------------- image metrics
 * Per-image MSE, PSNR and SSIM of the evaluate modes (src/pipelines/samplers/diffusion_like.py:251-263,
 * src/utils/evaluation_utils.py:64-91) in one pass over both tensors (csrc/metrics.hip).  gen / tgt: fp32
 * contiguous channels-first [N][C][H][W] (D == 0), [N][C][D][H][W], or signals [N][C][W] (D == 0 and H == 0:
 * no SSIM, ssim[n] = NaN).  clamp != 0 clamps both to [0, 1] first, as torch.clamp does (NaN stays NaN).
 *   mse[n]  = mean over the image of (g - t)^2
 *   psnr[n] = 10 log10(1 / max(mse, 1e-12)); 120 for an exact match
 *   ssim[n] = mean over channels and window positions of skimage's structural_similarity defaults: uniform
 *             7-wide window over every spatial axis, sample covariance, C1 = 1e-4, C2 = 9e-4, the positions
 *             whose whole window lies inside the image (3 cropped from every side)
 * All arithmetic is fp64 and every sum has a fixed order (no atomics): an image's numbers do not depend on N
 * or on its place in the batch, and a NaN reaches its own image only.  ws: fmd_image_metrics_workspace bytes
 * of partials.  A spatial side below 7, C < 1, N < 1 or a grid beyond 2^31 - 1 workgroups: -1 from both.
 * Nothing synchronises with the host. */
int64_t fmd_image_metrics_workspace(int32_t N, int32_t C, int32_t D, int32_t H, int32_t W);
int fmd_image_metrics(const float* gen, const float* tgt, int32_t N, int32_t C, int32_t D, int32_t H, int32_t W,
                      int32_t clamp, void* ws, double* mse, double* psnr, double* ssim, fmd_stream_t s);

/* ------------------------------------------------------------- VAE training criterion
 * The losses of VAE training (src/nn/losses/vae.py:104-151, src/pipelines/train/vae_lib.py:226-275, with
 * raw_output_to_image of src/models/autoencoder/base.py:21-28 fused in) and the posterior of
 * src/nn/modules/vae/reparameterizer.py:19-47 (csrc/vae_loss.hip).  Inputs are fp32; img = (clamp(x,-1,1) + 1)
 * * 0.5 is torch's three fp32 operations; everything after it is fp64 (exp / log1p / expm1 included) and every
 * value written is one rounding of its fp64 value.  Every sum is fp64 in a fixed order (per-workgroup partials
 * in ws, then a finishing launch): no atomics, the grid is a function of the shape, the same bits on every run.
 * Nothing synchronises with the host; upstream gradients are device memory.
 *
 * term (p = sigma(x), t the target):
 *   0 l1          |img - t|                          d/dx: sign(img - t) * 0.5 * [-1 <= x <= 1], sign(0) = 0
 *   1 mse         (img - t)^2                        d/dx: (img - t) * [-1 <= x <= 1]
 *   2 bce         max(x,0) - x t + log1p(exp(-|x|))  d/dx: p - t
 *   3 focal       a_t (1 - p_t)^2 ce, 1 - p_t = t sigma(-x) + (1 - t) sigma(x), a_t = alpha t + (1-alpha)(1-t)
 *                                                    d/dx: a_t [(1-p_t)^2 (p - t) - 2 (1-p_t) p (1-p) (2t-1) ce]
 *   4 bce_focal   bce + focal
 *   5 hinge_real  relu(1 - x)  (d/dx = 0 at x = 1)   6 hinge_fake  relu(1 + x)  (d/dx = 0 at x = -1)
 *   7 neg         -x                                 8 square      x^2
 * Terms 5 to 8 take no target.  reduction: 0 none, 1 sum, 2 mean.
 *
 * Addressing.  ld > 0, head layout (terms 0 to 4): x channels-last [N][P][ld], channels >= C never read (the
 * decoder head's fp32 output in place); target, g (g_elem != 0) and elem channels-first [N][C][P]; dx
 * [N][P][ld] and dx_bf16 [N][P][ldb] (the operand of fmd_head_dgrad), channels >= C written as 0.
 * FMD_VAE_LOSS_ROWS pixels per workgroup.  ld == 0, flat: N = C = 1 and x, target, g, elem, dx are P contiguous
 * elements; FMD_VAE_LOSS_CHUNK elements per workgroup; no dx_bf16.
 *
 * Outputs, each optional (null: not wanted; at least one): loss[0] = fp32 of the fp64 sum (/ N C P for the
 * mean), which needs ws and reduction != 0; elem = the per-element term; dx = (g * scale [/ N C P for the mean])
 * * d term / dx with g = g[0], or g[i] per element of the term when g_elem != 0; dx_bf16 = bf16 of dx.
 * fmd_vae_loss_workspace: bytes of ws (8 per workgroup).  Empty shapes, C > ld, an unknown term, a grid beyond
 * 2^31 - 1: -1 from both. */
#define FMD_VAE_LOSS_CHUNK 2048
#define FMD_VAE_LOSS_ROWS 512
int64_t fmd_vae_loss_workspace(int32_t term, int32_t N, int32_t C, int64_t P, int32_t ld);
int fmd_vae_loss(int32_t term, int32_t reduction, const float* x, const float* target, int32_t N, int32_t C,
                 int64_t P, int32_t ld, float alpha, const float* g, int32_t g_elem, float scale, void* ws,
                 float* loss, float* elem, float* dx, void* dx_bf16, int32_t ldb, fmd_stream_t s);
/* Posterior in one pass.  moments fp32 channels-last [N][P][ldm], channels 0 .. E-1 mu and E .. 2E-1 logvar
 * (the encoder head's output in place); eps fp32 channels-first [N][E][P], null: the mode (z = mu).
 *   lv = clamp(logvar, -30, 20);  z = mu + exp(0.5 lv) eps  -> z fp32 channels-first [N][E][P];
 *   z_staged (optional) bf16 channels-last [N][P][Cp], bf16 of z, channels >= E zero (the decoder's operand);
 *   kl[n] = 0.5 sum_{c,p} (mu^2 + expm1(lv) - lv): FMD_GAUSS_ROWS pixels per workgroup, the partials of sample n
 *   summed on their own, so kl[n] does not depend on N or on n.  ws: fmd_gauss_workspace bytes. */
#define FMD_GAUSS_ROWS 256
int64_t fmd_gauss_workspace(int32_t N, int32_t E, int64_t P);
int fmd_gauss_sample_kl(const float* moments, int32_t ldm, int32_t N, int32_t E, int64_t P, const float* eps,
                        float* z, void* z_staged, int32_t Cp, void* ws, float* kl, fmd_stream_t s);
/* d_mu = g_z + g_kl[n] mu;  d_logvar = [-30 <= logvar <= 20] (g_z eps 0.5 exp(0.5 lv) + g_kl[n] 0.5 expm1(lv)).
 * g_z fp32 [N][E][P] or null (zero), g_kl fp32 [N] or null (zero), eps null: zero.  d_moments fp32 [N][P][ldd]
 * and / or d_moments_bf16 [N][P][ldb], channels >= 2E zero. */
int fmd_gauss_backward(const float* moments, int32_t ldm, int32_t N, int32_t E, int64_t P, const float* eps,
                       const float* g_z, const float* g_kl, float* d_moments, int32_t ldd, void* d_moments_bf16,
                       int32_t ldb, fmd_stream_t s);

/* ---- Backward of the latent 1x1 conv (csrc/pointwise_bwd.hip): AutoencoderKL's post_quant_conv,
 * y[m][z] = b[z] + sum_e W[z][e] x[m][e], 1 <= Z, E <= FMD_POINTWISE_MAXC, M = N * P rows.
 *   dy bf16 [M][ldy] (channels >= Z never enter a result), x bf16 [M][ldx] (the staged latent that
 *   fmd_gauss_sample_kl wrote; channels >= E likewise), W fp32 [Z][E], the master weight.
 *   g (optional) fp32: g[m][e] = sum_z dy[m][z] W[z][e], added in fp64 in ascending z and rounded once;
 *     g_channels_last == 0: channels-first [N][E][P], the g_z of fmd_gauss_backward;
 *     else [M][ldg] with the channels >= E written as 0.
 *   dW[z][e] = sum_m dy[m][z] x[m][e] and db[z] = sum_m dy[m][z] (each optional; x and ws needed by either): fp64
 *     sums in a fixed order, rounded once to fp32, then stored (accumulate == 0) or added in fp32 to the value there.
 * The same bits on every run: no atomics, FMD_POINTWISE_ROWS rows per workgroup, one fp64 partial per workgroup
 * and sum in ws, a finishing launch.  fmd_pointwise_bwd_workspace: bytes of ws.  Z or E beyond the limit, empty
 * shapes, strides below the channel counts, nothing asked for: -1 from both. */
#define FMD_POINTWISE_ROWS 512
#define FMD_POINTWISE_MAXC 8
int64_t fmd_pointwise_bwd_workspace(int64_t M, int32_t Z, int32_t E);
int fmd_pointwise_bwd(const void* dy, int32_t ldy, const void* x, int32_t ldx, const float* W, int32_t N, int64_t P,
                      int32_t Z, int32_t E, float* g, int32_t g_channels_last, int32_t ldg, float* dW, float* db,
                      int32_t accumulate, void* ws, fmd_stream_t s);

/* ---- BatchNorm2d + LeakyReLU of the GAN discriminators (csrc/batchnorm.hip; reference
 * src/nn/modules/vae/discriminators.py, src/nn/losses/vae.py PatchDiscriminator).  Activations bf16 channels-last
 * [M][C], M = N*H*W, C % 8 == 0, 16-byte aligned; parameters and statistics fp32.  Deterministic: fp32 per lane over a
 * fixed row range, lanes and blocks combined in a fixed order, the per-channel fold in fp64, no atomics.  Bad shapes
 * or null operands: -1, misaligned pointers: -2, too many workgroups: -3; nothing is launched then.
 *
 * fmd_bn_fold: slab [rows_total][C][2] of (sum x, sum x^2) over all M elements of a channel (a conv epilogue's or
 *   fmd_channel_stats').  training != 0: mean, biased variance; a = gamma rstd, b = beta - mean a, mean_rstd [C][2];
 *   running_mean / running_var (unbiased, M / (M - 1)) updated with ``momentum`` and *num_batches_tracked (int64, may
 *   be NULL) incremented on the device, as nn.BatchNorm2d does; M == 1 is an error.  training == 0: a, b and
 *   mean_rstd from the running statistics, nothing updated, slab unused. */
int fmd_bn_fold(const float* slab, int64_t rows_total, int32_t C, int64_t M, const float* gamma, const float* beta,
                float eps, float momentum, int32_t training, float* running_mean, float* running_var,
                int64_t* num_batches_tracked, float* a, float* b, float* mean_rstd, fmd_stream_t s);
/* y = lrelu(fmaf(a[c], x, b[c]), slope), rounded once to bf16; a == b == NULL: y = lrelu(x) (a layer without norm). */
int fmd_bn_act_fwd(const void* x, int64_t M, int32_t C, const float* a, const float* b, float slope, void* y,
                   fmd_stream_t s);
/* g = dy * lrelu'(fmaf(a, x, b)) (the derivative at 0 is ``slope``, as torch); S1 = sum g, S2 = sum g xhat per
 * channel with xhat = (x - mean) rstd from mean_rstd.  training: dx = a (g - S1/M - xhat S2/M); else dx = a g;
 * a == NULL: dx = g.  dx bf16.  dgamma (+)= S2, dbeta (+)= S1 (``accumulate`` as fmd_wgrad) unless
 * skip_param_grads.  Launches: partial sums per FMD_BN_ROWS rows, their fp64 fold, the apply pass; ws of
 * fmd_bn_act_bwd_workspace(M, C) bytes (needed whenever sums are: a != NULL and (training or parameter gradients)). */
#define FMD_BN_ROWS 64
int64_t fmd_bn_act_bwd_workspace(int64_t M, int32_t C);
int fmd_bn_act_bwd(const void* dy, const void* x, int64_t M, int32_t C, const float* a, const float* b,
                   const float* mean_rstd, float slope, int32_t training, void* dx, float* dgamma, float* dbeta,
                   int32_t accumulate, int32_t skip_param_grads, void* ws, fmd_stream_t s);
/* The discriminator's input: fp32 NCHW [N][C][HW] -> bf16 NHWC [N*HW][Cp] (Cp % 8 == 0, channels >= C zero) with
 * raw_output_to_image fused: mode 0 identity, 1 (clamp(x, -1, 1) + 1) / 2, 2 sigmoid(x).  The backward reads the
 * first conv's bf16 data gradient g [N*HW][Cp] and the raw x and writes fp32 NCHW: g, g 0.5 [-1 <= x <= 1], or
 * g s (1 - s). */
int fmd_image_stage(const float* x, int32_t N, int32_t C, int64_t HW, int32_t Cp, int32_t mode, void* out,
                    fmd_stream_t s);
int fmd_image_stage_bwd(const void* g, const float* x, int32_t N, int32_t C, int64_t HW, int32_t Cp, int32_t mode,
                        float* dx, fmd_stream_t s);
/* The two-term forms the discriminator walker runs on.  A bf16 operand moves a pre-activation by 2^-9 of its size,
 * which flips LeakyReLU branches next to the kink and with them the gradient ("Discriminators");
 * so an activation is carried as hi = bf16(v), lo = bf16(v - hi) in one bf16 tensor [M][2 C] (channels [0, C) hi,
 * [C, 2 C) lo: about 16 significant bits), the conv reads both terms (and both terms of its weights) and writes fp32.
 *   fmd_image_stage_split: fmd_image_stage with out [N*HW][2 Cp].
 *   fmd_bn_stats_f32: slab [ceil(M / FMD_BN_ROWS)][C][2] of (sum x, sum x^2) of an fp32 [M][C] tensor, the operand
 *     of fmd_bn_fold (an fp32 conv output carries no statistics of its own).
 *   fmd_bn_act_fwd_split: fmd_bn_act_fwd with x fp32 [M][C] and y bf16 [M][2 C].
 *   fmd_bn_act_bwd_f32: fmd_bn_act_bwd with x fp32 [M][C] (dy and dx stay bf16 [M][C]); same workspace. */
int fmd_image_stage_split(const float* x, int32_t N, int32_t C, int64_t HW, int32_t Cp, int32_t mode, void* out,
                          fmd_stream_t s);
int fmd_bn_stats_f32(const float* x, int64_t M, int32_t C, float* slab, fmd_stream_t s);
int fmd_bn_act_fwd_split(const float* x, int64_t M, int32_t C, const float* a, const float* b, float slope, void* y,
                         fmd_stream_t s);
int fmd_bn_act_bwd_f32(const void* dy, const float* x, int64_t M, int32_t C, const float* a, const float* b,
                       const float* mean_rstd, float slope, int32_t training, void* dx, float* dgamma, float* dbeta,
                       int32_t accumulate, int32_t skip_param_grads, void* ws, fmd_stream_t s);

/* ---- VGG perceptual loss of VAE training (csrc/perceptual.hip; reference src/nn/losses/vae.py:22-72): staging, the
 * feature tap and the 2x2 max pool around a conv stack that runs on the two-term route above (the untapped ReLUs are
 * fmd_bn_act_fwd_split / fmd_bn_act_bwd_f32 with slope 0).  Recon and target travel as ONE batch of 2 N images, recon
 * first.  Deterministic: fixed-order sums (fp64 for the loss), no atomics.  Bad shapes or null operands: -1,
 * misaligned pointers: -2, too many workgroups: -3; nothing is launched then.
 *
 * fmd_perc_stage: recon, target fp32 NCHW [N][C][Hs][Ws], C 1 or 3 -> out bf16 [2 N][Ho][Wo][16], 8 hi | 8 lo channels
 *   (hi = bf16(v), lo = bf16(v - hi)); one channel is repeated to three, channels 3..7 are zero.  The image map
 *   ``mode`` (fmd_image_stage) applies to the recon half only.  (Ho, Wo) != (Hs, Ws): bilinear resize, torch's
 *   align_corners=False rule: source coordinate max((o + 1/2) in / out - 1/2, 0), upper neighbour clamped to the edge.
 * fmd_perc_stage_bwd: g bf16 [N][Ho][Wo][Cp] (gradient of the first conv's input, recon half; channels 0..2 read) ->
 *   dx fp32 [N][C][Hs][Ws] of the raw recon: each source pixel adds the destination pixels that read it (rows, then
 *   columns ascending; the range comes from the inverted coordinate map), the repeated channels are added as
 *   (g0 + g1) + g2, then the map's derivative as fmd_image_stage_bwd. */
int fmd_perc_stage(const float* recon, const float* target, int32_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t Ho,
                   int32_t Wo, int32_t mode, void* out, fmd_stream_t s);
int fmd_perc_stage_bwd(const void* g, const float* recon, int32_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t Ho,
                       int32_t Wo, int32_t Cp, int32_t mode, float* dx, fmd_stream_t s);
/* fmd_perc_tap_fwd: y fp32 [2 N][H][W][Cp], a tapped conv's output with its bias.  Over the C real channels:
 *   *value = (float)(sum |relu(y_rec) - relu(y_tgt)| / (N C H W)) (the difference one fp32 rounding, the sum fp64), and
 *   *loss = weight *value (first != 0) or *loss + weight *value (loss may be NULL).  sgn (int8 [N][H][W][Cp], may be
 *   NULL) receives sign(relu(y_rec) - relu(y_tgt)), 0 in padding channels.  out (may be NULL) is the next conv's
 *   two-term operand for all 2 N images: [2 N][H][W][2 Cp] with relu(y), or with pool != 0 [2 N][H/2][W/2][2 Cp] with
 *   relu of the 2x2 stride-2 maximum of y (odd sizes floor, as nn.MaxPool2d(2, 2)).  ws: fmd_perc_tap_workspace bytes.
 * fmd_perc_tap_bwd: recon half only.  dy bf16 [N][H][W][Cp] =
 *   [y_rec > 0] (g_loss[0] weight / (N C H W) sgn + below), with below = 0 (g_below NULL), g_below [N][H][W][Cp]
 *   (pool == 0), or g_below [N][H/2][W/2][Cp] routed to the first maximum of y_rec in its window in row-major order
 *   (pool != 0; pixels the floor leaves outside every window get none). */
int64_t fmd_perc_tap_workspace(int32_t N, int32_t H, int32_t W, int32_t Cp);
int fmd_perc_tap_fwd(const float* y, int32_t N, int32_t H, int32_t W, int32_t Cp, int32_t C, int32_t pool, void* out,
                     void* sgn, void* ws, float weight, int32_t first, float* value, float* loss, fmd_stream_t s);
int fmd_perc_tap_bwd(const float* y_rec, const void* sgn, int32_t N, int32_t H, int32_t W, int32_t Cp, int32_t C,
                     int32_t pool, const void* g_below, const float* g_loss, float weight, void* dy, fmd_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
