// BatchNorm2d with batch statistics + LeakyReLU for the GAN discriminators (reference
// src/nn/modules/vae/discriminators.py, src/nn/losses/vae.py PatchDiscriminator: conv -> nn.BatchNorm2d ->
// nn.LeakyReLU(0.2)), forward and backward, and the discriminator's input staging.
//
// Activations are the engine's: bf16 channels-last [M][C], M = N*H*W, C % 8 == 0; a lane owns 8 fixed channels of
// a row (one 16-byte access).  Parameters, statistics and the folded affine are fp32.
//
//   fmd_bn_fold        slab [rows][C][2] of (sum x, sum x^2) -> a = gamma*rstd, b = beta - mean*a, (mean, rstd), and
//                      the running statistics / num_batches_tracked of nn.BatchNorm2d (training); eval: a, b from
//                      the running statistics.
//   fmd_bn_act_fwd     y = lrelu(fmaf(a, x, b)), one bf16 rounding.
//   fmd_bn_act_bwd     g = dy * lrelu'(fmaf(a, x, b)); training: dx = a (g - S1/M - xhat S2/M) with S1 = sum g,
//                      S2 = sum g xhat; dgamma (+)= S2, dbeta (+)= S1.  Two passes over (dy, x) as two launches
//                      with a C/8-workgroup fold of the partial slab between them.
//   fmd_image_stage(_bwd)  fp32 NCHW -> bf16 NHWC padded to 8 channels with the image map fused, and its gradient.
//   two-term forms     fmd_image_stage_split, fmd_bn_stats_f32, fmd_bn_act_fwd_split, fmd_bn_act_bwd_f32: what the
//                      discriminator walker runs.  A value is stored as hi = bf16(v) | lo = bf16(v - hi) in one bf16
//                      tensor [M][2 C]; the conv reads both terms and writes fp32, which BatchNorm reads.  bf16 forward
//                      operands would flip LeakyReLU branches next to the kink (include/fmdiff.h).
//
// Every reduction: fp32 per lane over a fixed row range (a lane's rows of one BN_ROWS-row block, ascending), the 32
// row lanes of a block added in ascending order, the blocks added per channel in fp64 (a lane's blocks ascending,
// then the 32 lanes ascending).  No atomics; the grids depend on the shapes only, so two runs give equal bits.
#include "common.h"
#include "fmdiff.h"

namespace {

constexpr int BN_ROWS = FMD_BN_ROWS;   // rows of one partial-sum block of the backward (as fmd_channel_stats: 64)
static_assert(BN_ROWS % 32 == 0, "32 row lanes per block");

// The 8 channels of group ``idx8`` of x: bf16 (one 16-byte load) or fp32 (two).
template <bool XF32>
FMD_DEV void load8(const void* x, size_t idx8, float (&v)[8]) {
  if (XF32) {
    const f32x4* p = (const f32x4*)((const float*)x + idx8 * 8);
    const f32x4 q0 = p[0], q1 = p[1];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = q0[j], v[4 + j] = q1[j];
  } else {
    unpack8(*(const u32x4*)((const bf16r*)x + idx8 * 8), v);
  }
}

// Sum over the rows of a [rows][C][2] fp32 slab for the 8 channels c0 .. c0+7 of this workgroup, in fp64: thread
// (cl = t & 7, rl = t >> 3) adds rows rl, rl + 32, ... in ascending order, then the 32 row lanes are added in
// ascending order.  Returns with red[0][cl][0..1] final (valid for every thread after the barrier).
FMD_DEV void fold_column(const float* __restrict__ slab, long long rows, int C, int c0, double (&red)[32][8][2]) {
  const int t = threadIdx.x, cl = t & 7, rl = t >> 3;
  double s0 = 0.0, s1 = 0.0;
  for (long long j = rl; j < rows; j += 32) {
    const float2 v = *(const float2*)(slab + ((size_t)j * C + c0 + cl) * 2);
    s0 += (double)v.x;
    s1 += (double)v.y;
  }
  red[rl][cl][0] = s0;
  red[rl][cl][1] = s1;
  __syncthreads();
  if (t < 16) {
    const int c = t >> 1, w = t & 1;
    double s = red[0][c][w];
    for (int r = 1; r < 32; ++r) s += red[r][c][w];
    red[0][c][w] = s;
  }
  __syncthreads();
}

struct FoldArgs {
  const float* slab;
  long long rows, M;
  int C, training;
  const float *gamma, *beta;
  float eps, momentum;
  float *running_mean, *running_var;
  long long* nbt;
  float *a, *b, *mean_rstd;
};

__global__ __launch_bounds__(256) void bn_fold_kernel(FoldArgs p) {
  __shared__ double red[32][8][2];
  const int t = threadIdx.x, c0 = blockIdx.x * 8;
  if (p.training) fold_column(p.slab, p.rows, p.C, c0, red);
  if (t >= 8) return;
  const int c = c0 + t;
  double mean, rstd;
  if (p.training) {
    const double M = (double)p.M;
    mean = red[0][t][0] / M;
    double var = red[0][t][1] / M - mean * mean;   // biased; the cancellation is carried in fp64
    if (var < 0.0) var = 0.0;
    rstd = 1.0 / sqrt(var + (double)p.eps);
    const double mom = (double)p.momentum;
    p.running_mean[c] = (float)((1.0 - mom) * (double)p.running_mean[c] + mom * mean);
    p.running_var[c] = (float)((1.0 - mom) * (double)p.running_var[c] + mom * (var * (M / (M - 1.0))));
    if (blockIdx.x == 0 && t == 0 && p.nbt) *p.nbt += 1;
  } else {
    mean = (double)p.running_mean[c];
    rstd = 1.0 / sqrt((double)p.running_var[c] + (double)p.eps);
  }
  const float a = (float)((double)p.gamma[c] * rstd);
  p.a[c] = a;
  p.b[c] = (float)((double)p.beta[c] - mean * (double)a);   // consistent with the rounded a the kernels multiply by
  p.mean_rstd[2 * c] = (float)mean;
  p.mean_rstd[2 * c + 1] = (float)rstd;
}

// ---------------------------------------------------------------------------------------------- forward apply
// SPLIT: x is fp32 and y is [M][2 C]: channels [0, C) the hi terms, [C, 2 C) the lo terms (split8)
template <bool SPLIT>
__global__ __launch_bounds__(256) void bn_act_fwd_kernel(const void* __restrict__ x, long long M, int CG,
                                                         const float* __restrict__ a, const float* __restrict__ b,
                                                         float slope, bf16r* __restrict__ y) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * CG) return;
  const int cg = (int)(i % CG);
  float v[8];
  load8<SPLIT>(x, (size_t)i, v);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float u = a ? fmaf(a[cg * 8 + j], v[j], b[cg * 8 + j]) : v[j];
    v[j] = u > 0.f ? u : u * slope;
  }
  if (SPLIT) {
    u32x4 hi, lo;
    split8(v, hi, lo);
    bf16r* row = y + ((size_t)(i / CG) * 2 * CG + cg) * 8;
    *(u32x4*)row = hi;
    *(u32x4*)(row + (size_t)CG * 8) = lo;
  } else {
    *(u32x4*)(y + (size_t)i * 8) = pack8(v);
  }
}

// (sum x, sum x^2) of one BN_ROWS-row block of an fp32 [M][C] tensor (a conv's fp32 output, which carries no
// statistics of its own): the reduce kernel's thread layout and order.  slab [blocks][C][2].
__global__ __launch_bounds__(256) void bn_stats_f32_kernel(const float* __restrict__ x, long long M, int C,
                                                           float* __restrict__ slab) {
  __shared__ float red[32][8][16];
  const int t = threadIdx.x, cgl = t & 7, pl = t >> 3;
  const int c = (blockIdx.y * 8 + cgl) * 8;
  float s[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) s[k] = 0.f;
  if (c < C) {
    const long long r0 = (long long)blockIdx.x * BN_ROWS;
    const long long r1 = r0 + BN_ROWS < M ? r0 + BN_ROWS : M;
    for (long long r = r0 + pl; r < r1; r += 32) {
      float xv[8];
      load8<true>(x, ((size_t)r * C + c) / 8, xv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s[2 * j] += xv[j];
        s[2 * j + 1] = fmaf(xv[j], xv[j], s[2 * j + 1]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) red[pl][cgl][k] = s[k];
  __syncthreads();
  if (t < 128) {
    const int g8 = t >> 4, k = t & 15;
    const int cc = (blockIdx.y * 8 + g8) * 8;
    if (cc < C) {
      float v = red[0][g8][k];
      for (int r = 1; r < 32; ++r) v += red[r][g8][k];
      slab[((size_t)blockIdx.x * C + cc) * 2 + k] = v;
    }
  }
}

// --------------------------------------------------------------------------------------------------- backward
// Pass 1: partial (sum g, sum g xhat) of one BN_ROWS-row block for 64 channels: 256 threads = 8 channel groups x
// 32 row lanes.  part [blocks][C][2].
template <bool XF32>
__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const bf16r* __restrict__ dy, const void* __restrict__ x,
                                                            long long M, int C, const float* __restrict__ a,
                                                            const float* __restrict__ b,
                                                            const float* __restrict__ mr, float slope,
                                                            float* __restrict__ part) {
  __shared__ float red[32][8][16];
  const int t = threadIdx.x, cgl = t & 7, pl = t >> 3;
  const int c = (blockIdx.y * 8 + cgl) * 8;
  const bool on = c < C;
  float s[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) s[k] = 0.f;
  if (on) {
    float av[8], bv[8], mean[8], rstd[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      av[j] = a[c + j], bv[j] = b[c + j];
      mean[j] = mr[2 * (c + j)], rstd[j] = mr[2 * (c + j) + 1];
    }
    const long long r0 = (long long)blockIdx.x * BN_ROWS;
    const long long r1 = r0 + BN_ROWS < M ? r0 + BN_ROWS : M;
    for (long long r = r0 + pl; r < r1; r += 32) {
      float dv[8], xv[8];
      unpack8(*(const u32x4*)(dy + (size_t)r * C + c), dv);
      load8<XF32>(x, ((size_t)r * C + c) / 8, xv);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float u = fmaf(av[j], xv[j], bv[j]);
        const float g = u > 0.f ? dv[j] : dv[j] * slope;
        const float xh = (xv[j] - mean[j]) * rstd[j];
        s[2 * j] += g;
        s[2 * j + 1] = fmaf(g, xh, s[2 * j + 1]);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) red[pl][cgl][k] = s[k];
  __syncthreads();
  if (t < 128) {
    const int g8 = t >> 4, k = t & 15;
    const int cc = (blockIdx.y * 8 + g8) * 8;
    if (cc < C) {
      float v = red[0][g8][k];
      for (int r = 1; r < 32; ++r) v += red[r][g8][k];
      part[((size_t)blockIdx.x * C + cc) * 2 + k] = v;
    }
  }
}

// The fold between the passes: S1, S2 per channel in fp64; dbeta (+)= S1, dgamma (+)= S2; coef[c] = (S1/M, S2/M)
// for the apply pass (zeros in eval mode, where the statistics are constants).
__global__ __launch_bounds__(256) void bn_bwd_fold_kernel(const float* __restrict__ part, long long rows, long long M,
                                                          int C, int training, float* __restrict__ dgamma,
                                                          float* __restrict__ dbeta, int accumulate,
                                                          float* __restrict__ coef) {
  __shared__ double red[32][8][2];
  const int t = threadIdx.x, c0 = blockIdx.x * 8;
  fold_column(part, rows, C, c0, red);
  if (t >= 8) return;
  const int c = c0 + t;
  const double s1 = red[0][t][0], s2 = red[0][t][1];
  if (dbeta) dbeta[c] = accumulate ? dbeta[c] + (float)s1 : (float)s1;
  if (dgamma) dgamma[c] = accumulate ? dgamma[c] + (float)s2 : (float)s2;
  coef[2 * c] = training ? (float)(s1 / (double)M) : 0.f;
  coef[2 * c + 1] = training ? (float)(s2 / (double)M) : 0.f;
}

// Pass 2: dx.  a == null: dx = g (no norm); coef == null: dx = a g (eval mode without parameter gradients).
template <bool XF32>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const bf16r* __restrict__ dy, const void* __restrict__ x,
                                                           long long M, int CG, const float* __restrict__ a,
                                                           const float* __restrict__ b, const float* __restrict__ mr,
                                                           const float* __restrict__ coef, float slope,
                                                           bf16r* __restrict__ dx) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * CG) return;
  const int c = (int)(i % CG) * 8;
  float dv[8], xv[8];
  unpack8(*(const u32x4*)(dy + (size_t)i * 8), dv);
  load8<XF32>(x, (size_t)i, xv);
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    if (!a) {
      dv[j] = xv[j] > 0.f ? dv[j] : dv[j] * slope;
      continue;
    }
    const float aj = a[c + j];
    const float u = fmaf(aj, xv[j], b[c + j]);
    const float g = u > 0.f ? dv[j] : dv[j] * slope;
    if (coef) {
      const float xh = (xv[j] - mr[2 * (c + j)]) * mr[2 * (c + j) + 1];
      dv[j] = aj * fmaf(-xh, coef[2 * (c + j) + 1], g - coef[2 * (c + j)]);
    } else {
      dv[j] = aj * g;
    }
  }
  *(u32x4*)(dx + (size_t)i * 8) = pack8(dv);
}

// ------------------------------------------------------------------------------------------------ image stage
FMD_DEV float sigmoid_exact(float v) { return 1.0f / (1.0f + expf(-v)); }

// item i = cg * M + m (pixels fastest: coalesced NCHW reads); out [M][Cp], or with SPLIT [M][2 Cp] (hi | lo, split8)
template <bool SPLIT>
__global__ __launch_bounds__(256) void image_stage_kernel(const float* __restrict__ x, int C, long long HW, long long M,
                                                          int Cp, int mode, bf16r* __restrict__ out) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= M * (Cp / 8)) return;
  const int cg = (int)(i / M);
  const long long m = i - (long long)cg * M;
  const long long n = m / HW, hw = m - n * HW;
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = cg * 8 + j;
    float r = 0.f;
    if (c < C) {
      r = x[((size_t)n * C + c) * (size_t)HW + (size_t)hw];
      if (mode == 1) r = (fminf(fmaxf(r, -1.f), 1.f) + 1.f) * 0.5f;
      else if (mode == 2) r = sigmoid_exact(r);
    }
    v[j] = r;
  }
  if (SPLIT) {
    u32x4 hi, lo;
    split8(v, hi, lo);
    *(u32x4*)(out + (size_t)m * 2 * Cp + cg * 8) = hi;
    *(u32x4*)(out + (size_t)m * 2 * Cp + Cp + cg * 8) = lo;
  } else {
    *(u32x4*)(out + (size_t)m * Cp + cg * 8) = pack8(v);
  }
}

// item i in NCHW order of dx [N][C][HW]; g bf16 [M][Cp]
__global__ __launch_bounds__(256) void image_stage_bwd_kernel(const bf16r* __restrict__ g, const float* __restrict__ x,
                                                              int C, long long HW, long long total, int Cp, int mode,
                                                              float* __restrict__ dx) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const long long hw = i % HW, nc = i / HW;
  const long long n = nc / C;
  const int c = (int)(nc - n * C);
  float gv = bf2f(g[((size_t)n * HW + hw) * Cp + c]);
  if (mode == 1) {
    const float r = x[i];
    gv = (r >= -1.f && r <= 1.f) ? gv * 0.5f : 0.f;   // torch.clamp passes the gradient at the boundary
  } else if (mode == 2) {
    // s (1 - s) = e / (1 + e)^2 with e = exp(-|x|): no 1 - s cancellation at large |x|
    const float e = expf(-fabsf(x[i])), d = 1.f + e;
    gv = gv * (e / (d * d));
  }
  dx[i] = gv;
}

constexpr long long LIM = (1ll << 31) - 1;
bool al(const void* p, unsigned n) { return ((unsigned long long)p & (n - 1)) == 0; }

}  // namespace

extern "C" int fmd_bn_fold(const float* slab, int64_t rows_total, int32_t C, int64_t M, const float* gamma,
                           const float* beta, float eps, float momentum, int32_t training, float* running_mean,
                           float* running_var, int64_t* num_batches_tracked, float* a, float* b, float* mean_rstd,
                           fmd_stream_t s) {
  if (C < 8 || C % 8 || M < 1 || !gamma || !beta || !running_mean || !running_var || !a || !b || !mean_rstd) return -1;
  if (training && (M < 2 || !slab || rows_total < 1)) return -1;   // one value per channel: torch raises too
  if (!al(slab, 8) || !al(gamma, 4) || !al(beta, 4) || !al(running_mean, 4) || !al(running_var, 4) ||
      !al(num_batches_tracked, 8) || !al(a, 4) || !al(b, 4) || !al(mean_rstd, 4))
    return -2;
  FoldArgs p;
  p.slab = slab, p.rows = rows_total, p.M = M, p.C = C, p.training = training != 0;
  p.gamma = gamma, p.beta = beta, p.eps = eps, p.momentum = momentum;
  p.running_mean = running_mean, p.running_var = running_var, p.nbt = (long long*)num_batches_tracked;
  p.a = a, p.b = b, p.mean_rstd = mean_rstd;
  hipLaunchKernelGGL(bn_fold_kernel, dim3(C / 8), dim3(256), 0, (hipStream_t)s, p);
  return (int)hipGetLastError();
}

namespace {
int act_fwd(const void* x, int64_t M, int32_t C, const float* a, const float* b, float slope, void* y, bool split,
            fmd_stream_t s) {
  if (C < 8 || C % 8 || M < 1 || !x || !y || (a != nullptr) != (b != nullptr)) return -1;
  if (!al(x, 16) || !al(y, 16) || !al(a, 4) || !al(b, 4)) return -2;
  const long long blocks = (M * (C / 8) + 255) / 256;
  if (blocks > LIM) return -3;
  if (split)
    hipLaunchKernelGGL(bn_act_fwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, x, (long long)M,
                       C / 8, a, b, slope, (bf16r*)y);
  else
    hipLaunchKernelGGL(bn_act_fwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, x, (long long)M,
                       C / 8, a, b, slope, (bf16r*)y);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int fmd_bn_act_fwd(const void* x, int64_t M, int32_t C, const float* a, const float* b, float slope,
                              void* y, fmd_stream_t s) {
  return act_fwd(x, M, C, a, b, slope, y, false, s);
}

extern "C" int fmd_bn_act_fwd_split(const float* x, int64_t M, int32_t C, const float* a, const float* b, float slope,
                                    void* y, fmd_stream_t s) {
  return act_fwd(x, M, C, a, b, slope, y, true, s);
}

extern "C" int fmd_bn_stats_f32(const float* x, int64_t M, int32_t C, float* slab, fmd_stream_t s) {
  if (C < 8 || C % 8 || M < 1 || !x || !slab) return -1;
  if (!al(x, 16) || !al(slab, 8)) return -2;
  const long long rblocks = (M + BN_ROWS - 1) / BN_ROWS;
  if (rblocks > LIM) return -3;
  hipLaunchKernelGGL(bn_stats_f32_kernel, dim3((unsigned)rblocks, (C + 63) / 64), dim3(256), 0, (hipStream_t)s, x,
                     (long long)M, C, slab);
  return (int)hipGetLastError();
}

extern "C" int64_t fmd_bn_act_bwd_workspace(int64_t M, int32_t C) {
  if (C < 8 || C % 8 || M < 1) return -1;
  const long long blocks = (M + BN_ROWS - 1) / BN_ROWS;
  if (blocks > LIM) return -1;
  return (blocks * C * 2 + (long long)C * 2) * 4;
}

namespace {
template <bool XF32>
int act_bwd(const void* dy, const void* x, int64_t M, int32_t C, const float* a, const float* b,
            const float* mean_rstd, float slope, int32_t training, void* dx, float* dgamma, float* dbeta,
            int32_t accumulate, int32_t skip_param_grads, void* ws, fmd_stream_t s) {
  if (C < 8 || C % 8 || M < 1 || !dy || !x || !dx) return -1;
  if ((a != nullptr) != (b != nullptr) || (a && !mean_rstd)) return -1;
  if (!al(dy, 16) || !al(x, 16) || !al(dx, 16) || !al(a, 4) || !al(b, 4) || !al(mean_rstd, 4) || !al(dgamma, 4) ||
      !al(dbeta, 4) || !al(ws, 8))
    return -2;
  const bool params = a && !skip_param_grads && (dgamma || dbeta);
  const bool sums = a && (training || params);
  if (a && !skip_param_grads && !dgamma && !dbeta) return -1;   // gradients asked for, nowhere to put them
  if (a && training && M < 2) return -1;
  if (sums && !ws) return -1;
  const long long rblocks = (M + BN_ROWS - 1) / BN_ROWS;
  const long long blocks = (M * (C / 8) + 255) / 256;
  if (blocks > LIM || rblocks > LIM) return -3;
  hipStream_t st = (hipStream_t)s;
  float* part = (float*)ws;
  float* coef = sums ? part + (size_t)rblocks * C * 2 : nullptr;
  if (sums) {
    hipLaunchKernelGGL(bn_bwd_reduce_kernel<XF32>, dim3((unsigned)rblocks, (C + 63) / 64), dim3(256), 0, st,
                       (const bf16r*)dy, x, (long long)M, C, a, b, mean_rstd, slope, part);
    hipLaunchKernelGGL(bn_bwd_fold_kernel, dim3(C / 8), dim3(256), 0, st, (const float*)part, rblocks, (long long)M,
                       C, training != 0, params ? dgamma : nullptr, params ? dbeta : nullptr, accumulate, coef);
  }
  hipLaunchKernelGGL(bn_bwd_apply_kernel<XF32>, dim3((unsigned)blocks), dim3(256), 0, st, (const bf16r*)dy, x,
                     (long long)M, C / 8, a, b, mean_rstd, (a && training) ? coef : nullptr, slope, (bf16r*)dx);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int fmd_bn_act_bwd(const void* dy, const void* x, int64_t M, int32_t C, const float* a, const float* b,
                              const float* mean_rstd, float slope, int32_t training, void* dx, float* dgamma,
                              float* dbeta, int32_t accumulate, int32_t skip_param_grads, void* ws, fmd_stream_t s) {
  return act_bwd<false>(dy, x, M, C, a, b, mean_rstd, slope, training, dx, dgamma, dbeta, accumulate,
                        skip_param_grads, ws, s);
}

extern "C" int fmd_bn_act_bwd_f32(const void* dy, const float* x, int64_t M, int32_t C, const float* a,
                                  const float* b, const float* mean_rstd, float slope, int32_t training, void* dx,
                                  float* dgamma, float* dbeta, int32_t accumulate, int32_t skip_param_grads, void* ws,
                                  fmd_stream_t s) {
  return act_bwd<true>(dy, x, M, C, a, b, mean_rstd, slope, training, dx, dgamma, dbeta, accumulate,
                       skip_param_grads, ws, s);
}

namespace {
int image_stage(const float* x, int32_t N, int32_t C, int64_t HW, int32_t Cp, int32_t mode, void* out, bool split,
                fmd_stream_t s) {
  if (N < 1 || C < 1 || HW < 1 || Cp < C || Cp % 8 || mode < 0 || mode > 2 || !x || !out) return -1;
  if (!al(x, 4) || !al(out, 16)) return -2;
  const long long M = (long long)N * HW;
  const long long blocks = (M * (Cp / 8) + 255) / 256;
  if (blocks > LIM) return -3;
  if (split)
    hipLaunchKernelGGL(image_stage_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, x, C,
                       (long long)HW, M, Cp, mode, (bf16r*)out);
  else
    hipLaunchKernelGGL(image_stage_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, x, C,
                       (long long)HW, M, Cp, mode, (bf16r*)out);
  return (int)hipGetLastError();
}
}  // namespace

extern "C" int fmd_image_stage(const float* x, int32_t N, int32_t C, int64_t HW, int32_t Cp, int32_t mode, void* out,
                               fmd_stream_t s) {
  return image_stage(x, N, C, HW, Cp, mode, out, false, s);
}

extern "C" int fmd_image_stage_split(const float* x, int32_t N, int32_t C, int64_t HW, int32_t Cp, int32_t mode,
                                     void* out, fmd_stream_t s) {
  return image_stage(x, N, C, HW, Cp, mode, out, true, s);
}

extern "C" int fmd_image_stage_bwd(const void* g, const float* x, int32_t N, int32_t C, int64_t HW, int32_t Cp,
                                   int32_t mode, float* dx, fmd_stream_t s) {
  if (N < 1 || C < 1 || HW < 1 || Cp < C || Cp % 8 || mode < 0 || mode > 2 || !g || !dx || (mode && !x)) return -1;
  if (!al(g, 16) || !al(x, 4) || !al(dx, 4)) return -2;
  const long long total = (long long)N * C * HW;
  const long long blocks = (total + 255) / 256;
  if (blocks > LIM) return -3;
  hipLaunchKernelGGL(image_stage_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, (const bf16r*)g, x,
                     C, (long long)HW, total, Cp, mode, dx);
  return (int)hipGetLastError();
}
