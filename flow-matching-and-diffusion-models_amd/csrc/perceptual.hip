// The VGG perceptual loss of VAE training (reference src/nn/losses/vae.py:22-72): what the conv stack itself does not
// do.  The convs run on the two-term 3x3 route of the discriminators (csrc/batchnorm.hip header); the untapped ReLUs
// are fmd_bn_act_fwd_split / fmd_bn_act_bwd_f32 with slope 0.
//
//   fmd_perc_stage      recon and target, fp32 NCHW [N][C][Hs][Ws] with C 1 or 3 -> ONE batch of 2 N images (recon
//                       first) in the two-term form [2 N][Ho][Wo][16] (8 hi | 8 lo channels, 3 of them used), with
//                       the image map on the recon half, the repeat of one channel to three and the bilinear resize
//                       of F.interpolate(align_corners=False) fused.
//   fmd_perc_stage_bwd  bf16 [N][Ho][Wo][Cp] gradient of the first conv's input (recon half) -> fp32 NCHW gradient of
//                       the raw recon: the resize inverted as a gather (every source pixel adds the destination pixels
//                       that read it, rows then columns ascending), the three repeated channels added, the map's
//                       derivative.
//   fmd_perc_tap_fwd    a tapped conv output y fp32 [2 N][H][W][Cp]: mean |relu(y_rec) - relu(y_tgt)| over the C real
//                       channels (fp64, fixed order), the sign of the difference for the backward, and the next conv's
//                       two-term operand for all 2 N images, through a 2x2 stride-2 max pool where one follows.
//   fmd_perc_tap_bwd    dy = [y_rec > 0] (g w / count sign + the gradient from below, routed by the pool to the first
//                       maximum of its window), bf16, recon half only.
//
// A lane owns 8 channels of a pixel (16-byte accesses); the tap kernels walk 2x2 windows so that the pool needs no
// second pass.  Sums: a thread adds its elements in a fixed order in fp64, a fixed butterfly adds the 64 lanes, the
// four wave totals are added in order into one partial per workgroup, and a finishing launch adds the partials
// thread-strided and then by a fixed tree (the shape of csrc/vae_loss.hip).  No atomics; the grids depend on the
// shapes only, so two runs give equal bits.
#include "common.h"
#include "fmdiff.h"

#include <math.h>

namespace {

FMD_DEV void load8f(const float* p, float (&v)[8]) {
  const f32x4 q0 = ((const f32x4*)p)[0], q1 = ((const f32x4*)p)[1];
#pragma unroll
  for (int j = 0; j < 4; ++j) v[j] = q0[j], v[4 + j] = q1[j];
}

FMD_DEV float relu(float v) { return v < 0.f ? 0.f : v; }   // a NaN stays a NaN

// ------------------------------------------------------------------------------------------------ bilinear map
// Destination index o of an axis resized from ``in`` source pixels with scale = in / out (fp32): the two source
// pixels it reads and their weights, torch's align_corners=False rule.  Each operation is one fp32 rounding
// (no contraction), which tests/perc_bounds.py restates.
struct Axis {
  int i0, i1;
  float l0, l1;
};

FMD_DEV Axis src_axis(int o, float scale, int in) {
  float s = __fsub_rn(__fmul_rn((float)o + 0.5f, scale), 0.5f);
  s = s < 0.f ? 0.f : s;
  Axis a;
  a.i0 = (int)s;
  if (a.i0 > in - 1) a.i0 = in - 1;
  a.i1 = a.i0 < in - 1 ? a.i0 + 1 : a.i0;   // the upper neighbour is clamped to the edge
  a.l1 = __fsub_rn(s, (float)a.i0);
  a.l0 = __fsub_rn(1.0f, a.l1);
  return a;
}

FMD_DEV float image_map(float r, int mode) {
  if (mode == 1) return (fminf(fmaxf(r, -1.f), 1.f) + 1.f) * 0.5f;
  if (mode == 2) return 1.0f / (1.0f + expf(-r));
  return r;
}

// item m: one output pixel of the 2 N images
template <bool RESIZE>
__global__ __launch_bounds__(256) void perc_stage_kernel(const float* __restrict__ recon,
                                                         const float* __restrict__ target, int N, int C, int Hs,
                                                         int Ws, int Ho, int Wo, float sh, float sw, int mode,
                                                         bf16r* __restrict__ out) {
  const long long m = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long HWo = (long long)Ho * Wo;
  if (m >= 2ll * N * HWo) return;
  const int n2 = (int)(m / HWo);
  const long long p = m - (long long)n2 * HWo;
  const int oy = (int)(p / Wo), ox = (int)(p - (long long)oy * Wo);
  const bool tgt = n2 >= N;
  const float* img = (tgt ? target : recon) + (size_t)(tgt ? n2 - N : n2) * C * ((size_t)Hs * Ws);
  const int md = tgt ? 0 : mode;   // the target is used as given
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = 0.f;
  Axis ay, ax;
  if (RESIZE) {
    ay = src_axis(oy, sh, Hs);
    ax = src_axis(ox, sw, Ws);
  }
  for (int c = 0; c < C; ++c) {
    const float* pl = img + (size_t)c * ((size_t)Hs * Ws);
    float r;
    if (RESIZE) {
      const float a = image_map(pl[(size_t)ay.i0 * Ws + ax.i0], md), b = image_map(pl[(size_t)ay.i0 * Ws + ax.i1], md);
      const float e = image_map(pl[(size_t)ay.i1 * Ws + ax.i0], md), f = image_map(pl[(size_t)ay.i1 * Ws + ax.i1], md);
      const float top = __fadd_rn(__fmul_rn(ax.l0, a), __fmul_rn(ax.l1, b));
      const float bot = __fadd_rn(__fmul_rn(ax.l0, e), __fmul_rn(ax.l1, f));
      r = __fadd_rn(__fmul_rn(ay.l0, top), __fmul_rn(ay.l1, bot));
    } else {
      r = image_map(pl[(size_t)oy * Ws + ox], md);
    }
    v[c] = r;
  }
  if (C == 1) v[1] = v[2] = v[0];
  u32x4 hi, lo;
  split8(v, hi, lo);
  *(u32x4*)(out + (size_t)m * 16) = hi;
  *(u32x4*)(out + (size_t)m * 16 + 8) = lo;
}

// First and last destination index that can read source pixel y: src(o) in [y - 1, y + 1) inverted, one index of
// slack on both sides for the fp32 roundings (the loop keeps only the indices whose src_axis really names y).
FMD_DEV void reader_range(int y, float inv_scale, int out, int& lo, int& hi) {
  const float a = floorf(((float)y - 0.5f) * inv_scale - 0.5f) - 1.0f;
  const float b = ceilf(((float)y + 1.5f) * inv_scale - 0.5f) + 1.0f;
  lo = a < 0.f ? 0 : (a > (float)(out - 1) ? out - 1 : (int)a);
  hi = b > (float)(out - 1) ? out - 1 : (b < 0.f ? 0 : (int)b);
}

// item i in NCHW order of dx [N][C][Hs][Ws]; g bf16 [N][Ho][Wo][Cp]
template <bool RESIZE>
__global__ __launch_bounds__(256) void perc_stage_bwd_kernel(const bf16r* __restrict__ g,
                                                             const float* __restrict__ recon, int N, int C, int Hs,
                                                             int Ws, int Ho, int Wo, int Cp, float sh, float sw,
                                                             float ih, float iw, int mode, float* __restrict__ dx) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long HWs = (long long)Hs * Ws;
  if (i >= (long long)N * C * HWs) return;
  const long long nc = i / HWs, hw = i - nc * HWs;
  const int n = (int)(nc / C), c = (int)(nc - (long long)n * C);
  const int y = (int)(hw / Ws), x = (int)(hw - (long long)y * Ws);
  const bf16r* gn = g + (size_t)n * Ho * Wo * Cp;
  float acc = 0.f;
  if (RESIZE) {
    int ylo, yhi, xlo, xhi;
    reader_range(y, ih, Ho, ylo, yhi);
    reader_range(x, iw, Wo, xlo, xhi);
    for (int oy = ylo; oy <= yhi; ++oy) {
      const Axis ay = src_axis(oy, sh, Hs);
      if (ay.i0 != y && ay.i1 != y) continue;
      const float wy = ay.i0 == y ? (ay.i1 == y ? __fadd_rn(ay.l0, ay.l1) : ay.l0) : ay.l1;
      for (int ox = xlo; ox <= xhi; ++ox) {
        const Axis ax = src_axis(ox, sw, Ws);
        if (ax.i0 != x && ax.i1 != x) continue;
        const float wx = ax.i0 == x ? (ax.i1 == x ? __fadd_rn(ax.l0, ax.l1) : ax.l0) : ax.l1;
        const bf16r* q = gn + ((size_t)oy * Wo + ox) * Cp;
        const float gs = C == 1 ? __fadd_rn(__fadd_rn(bf2f(q[0]), bf2f(q[1])), bf2f(q[2])) : bf2f(q[c]);
        acc = __fadd_rn(acc, __fmul_rn(__fmul_rn(wy, wx), gs));
      }
    }
  } else {
    const bf16r* q = gn + ((size_t)y * Wo + x) * Cp;
    acc = C == 1 ? __fadd_rn(__fadd_rn(bf2f(q[0]), bf2f(q[1])), bf2f(q[2])) : bf2f(q[c]);
  }
  if (mode == 1) {
    const float r = recon[i];
    acc = (r >= -1.f && r <= 1.f) ? acc * 0.5f : 0.f;   // torch.clamp passes the gradient at the boundary
  } else if (mode == 2) {
    // s (1 - s) = e / (1 + e)^2 with e = exp(-|x|): no 1 - s cancellation at large |x|
    const float e = expf(-fabsf(recon[i])), d = 1.f + e;
    acc = acc * (e / (d * d));
  }
  dx[i] = acc;
}

// ------------------------------------------------------------------------------------------------------- tap
struct TapArgs {
  const float* y;      // fwd: [2 N][H][W][Cp]; bwd: the recon rows [N][H][W][Cp]
  int N, H, W, Cp, C, pool;
  bf16r* out;          // fwd: two-term operand of the next conv, or null
  signed char* sgn;    // fwd: written (or null); bwd: read.  [N][H][W][Cp]
  double* part;        // fwd: one partial per workgroup
  const bf16r* gbelow; // bwd: [N][H/2][W/2][Cp] (pool) or [N][H][W][Cp], or null
  const float* gloss;
  float weight;
  double count;
  bf16r* dy;           // bwd: [N][H][W][Cp]
};

// item: (n, window row, window column, channel group), channel group fastest; a window is 2x2 pixels, cut at
// odd edges.  Returns false past the end.
FMD_DEV bool tap_item(const TapArgs& a, int& n, int& wy, int& wx, int& cg) {
  const int CG = a.Cp / 8, Hw = (a.H + 1) / 2, Ww = (a.W + 1) / 2;
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)a.N * Hw * Ww * CG) return false;
  cg = (int)(i % CG);
  long long r = i / CG;
  wx = (int)(r % Ww);
  r /= Ww;
  wy = (int)(r % Hw);
  n = (int)(r / Hw);
  return true;
}

__global__ __launch_bounds__(256) void perc_tap_fwd_kernel(TapArgs a) {
  __shared__ double red[4];
  int n, wy, wx, cg;
  double acc = 0.0;
  if (tap_item(a, n, wy, wx, cg)) {
    const int H = a.H, W = a.W, Cp = a.Cp, c0 = cg * 8;
    const bool whole = 2 * wy + 1 < H && 2 * wx + 1 < W;
    const int Ho = H / 2, Wo = W / 2;
    float mr[8], mt[8];
#pragma unroll
    for (int k = 0; k < 4; ++k) {   // row-major: (0,0), (0,1), (1,0), (1,1)
      const int yy = 2 * wy + (k >> 1), xx = 2 * wx + (k & 1);
      if (yy >= H || xx >= W) continue;
      const size_t pr = (((size_t)n * H + yy) * W + xx) * Cp + c0;
      const size_t pt = (((size_t)(n + a.N) * H + yy) * W + xx) * Cp + c0;
      float yr[8], yt[8];
      load8f(a.y + pr, yr);
      load8f(a.y + pt, yt);
      unsigned int sb[2] = {0u, 0u};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool real = c0 + j < a.C;
        if (!real) yr[j] = yt[j] = 0.f;
        const float d = __fsub_rn(relu(yr[j]), relu(yt[j]));
        if (real) acc += (double)fabsf(d);
        const unsigned int s = d > 0.f ? 0x01u : (d < 0.f ? 0xffu : 0u);
        sb[j >> 2] |= s << (8 * (j & 3));
        mr[j] = (k == 0 || yr[j] > mr[j]) ? yr[j] : mr[j];
        mt[j] = (k == 0 || yt[j] > mt[j]) ? yt[j] : mt[j];
      }
      if (a.sgn) *(u32x2*)(a.sgn + pr) = u32x2{sb[0], sb[1]};
      if (a.out && !a.pool) {
        float vr[8], vt[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) vr[j] = relu(yr[j]), vt[j] = relu(yt[j]);
        u32x4 hi, lo;
        split8(vr, hi, lo);
        bf16r* o = a.out + (((size_t)n * H + yy) * W + xx) * 2 * Cp + c0;
        *(u32x4*)o = hi;
        *(u32x4*)(o + Cp) = lo;
        split8(vt, hi, lo);
        o = a.out + (((size_t)(n + a.N) * H + yy) * W + xx) * 2 * Cp + c0;
        *(u32x4*)o = hi;
        *(u32x4*)(o + Cp) = lo;
      }
    }
    if (a.out && a.pool && whole) {   // pool and ReLU commute: the maximum of y, one ReLU
#pragma unroll
      for (int j = 0; j < 8; ++j) mr[j] = relu(mr[j]), mt[j] = relu(mt[j]);
      u32x4 hi, lo;
      split8(mr, hi, lo);
      bf16r* o = a.out + (((size_t)n * Ho + wy) * Wo + wx) * 2 * Cp + c0;
      *(u32x4*)o = hi;
      *(u32x4*)(o + Cp) = lo;
      split8(mt, hi, lo);
      o = a.out + (((size_t)(n + a.N) * Ho + wy) * Wo + wx) * 2 * Cp + c0;
      *(u32x4*)o = hi;
      *(u32x4*)(o + Cp) = lo;
    }
  }
  const double s = block_sum(acc, red);
  if (threadIdx.x == 0) a.part[blockIdx.x] = s;
}

// value = (float)(sum of the partials / count); loss = weight value (first) or loss + weight value, fp32
__global__ __launch_bounds__(256) void perc_tap_final_kernel(const double* __restrict__ part, long long P, double count,
                                                             float weight, int first, float* __restrict__ value,
                                                             float* __restrict__ loss) {
  __shared__ double r[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (long long i = tid; i < P; i += 256) s += part[i];
  r[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) r[tid] += r[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    const float v = (float)(r[0] / count);
    *value = v;
    if (loss) {
      const float t = __fmul_rn(weight, v);
      *loss = first ? t : __fadd_rn(*loss, t);
    }
  }
}

__global__ __launch_bounds__(256) void perc_tap_bwd_kernel(TapArgs a) {
  int n, wy, wx, cg;
  if (!tap_item(a, n, wy, wx, cg)) return;
  const int H = a.H, W = a.W, Cp = a.Cp, c0 = cg * 8;
  const bool routed = a.gbelow && a.pool && 2 * wy + 1 < H && 2 * wx + 1 < W;
  const float coef = (float)((double)a.gloss[0] * (double)a.weight / a.count);
  float yv[4][8];
  int arg[8];
  float best[8];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = 2 * wy + (k >> 1), xx = 2 * wx + (k & 1);
    if (yy >= H || xx >= W) continue;
    load8f(a.y + (((size_t)n * H + yy) * W + xx) * Cp + c0, yv[k]);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (k == 0 || yv[k][j] > best[j]) best[j] = yv[k][j], arg[j] = k;   // strict: the first maximum keeps it
  }
  float gp[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) gp[j] = 0.f;
  if (routed)
    unpack8(*(const u32x4*)(a.gbelow + (((size_t)n * (H / 2) + wy) * (W / 2) + wx) * Cp + c0), gp);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int yy = 2 * wy + (k >> 1), xx = 2 * wx + (k & 1);
    if (yy >= H || xx >= W) continue;
    const size_t p = (((size_t)n * H + yy) * W + xx) * Cp + c0;
    const u32x2 sb = *(const u32x2*)(a.sgn + p);
    float gb[8];
    if (a.gbelow && !a.pool) unpack8(*(const u32x4*)(a.gbelow + p), gb);
    float dv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int s = (int)(signed char)((sb[j >> 2] >> (8 * (j & 3))) & 0xffu);
      const float l1 = s > 0 ? coef : (s < 0 ? -coef : 0.f);
      float below = 0.f;
      if (a.gbelow) below = a.pool ? ((routed && arg[j] == k) ? gp[j] : 0.f) : gb[j];
      dv[j] = yv[k][j] > 0.f ? __fadd_rn(l1, below) : 0.f;   // the ReLU derivative at 0 is 0
    }
    *(u32x4*)(a.dy + p) = pack8(dv);
  }
}

constexpr long long LIM = (1ll << 31) - 1;
bool al(const void* p, unsigned n) { return ((unsigned long long)p & (n - 1)) == 0; }

// workgroups of a tap launch, or -1
long long tap_blocks(long long N, long long H, long long W, long long Cp, long long C) {
  if (N < 1 || H < 1 || W < 1 || Cp < 8 || Cp % 8 || C < 1 || C > Cp) return -1;
  if (N > (1 << 20) || H > (1 << 15) || W > (1 << 15) || Cp > (1 << 16)) return -1;
  const long long items = N * ((H + 1) / 2) * ((W + 1) / 2) * (Cp / 8);
  const long long b = (items + 255) / 256;
  return b > LIM ? -1 : b;
}

bool stage_ok(long long N, long long C, long long Hs, long long Ws, long long Ho, long long Wo, int mode) {
  if (N < 1 || (C != 1 && C != 3) || Hs < 1 || Ws < 1 || Ho < 1 || Wo < 1 || mode < 0 || mode > 2) return false;
  return N <= (1 << 20) && Hs <= (1 << 15) && Ws <= (1 << 15) && Ho <= (1 << 15) && Wo <= (1 << 15);
}

}  // namespace

extern "C" int fmd_perc_stage(const float* recon, const float* target, int32_t N, int32_t C, int32_t Hs, int32_t Ws,
                              int32_t Ho, int32_t Wo, int32_t mode, void* out, fmd_stream_t s) {
  if (!stage_ok(N, C, Hs, Ws, Ho, Wo, mode) || !recon || !target || !out) return -1;
  if (!al(recon, 4) || !al(target, 4) || !al(out, 16)) return -2;
  const long long blocks = (2ll * N * Ho * Wo + 255) / 256;
  if (blocks > LIM) return -3;
  const float sh = (float)Hs / (float)Ho, sw = (float)Ws / (float)Wo;
  if (Hs != Ho || Ws != Wo)
    hipLaunchKernelGGL(perc_stage_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, recon, target, N,
                       C, Hs, Ws, Ho, Wo, sh, sw, mode, (bf16r*)out);
  else
    hipLaunchKernelGGL(perc_stage_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, recon, target,
                       N, C, Hs, Ws, Ho, Wo, sh, sw, mode, (bf16r*)out);
  return (int)hipGetLastError();
}

extern "C" int fmd_perc_stage_bwd(const void* g, const float* recon, int32_t N, int32_t C, int32_t Hs, int32_t Ws,
                                  int32_t Ho, int32_t Wo, int32_t Cp, int32_t mode, float* dx, fmd_stream_t s) {
  if (!stage_ok(N, C, Hs, Ws, Ho, Wo, mode) || Cp < 8 || Cp % 8 || !g || !dx || (mode && !recon)) return -1;
  if (!al(g, 16) || !al(recon, 4) || !al(dx, 4)) return -2;
  const long long blocks = ((long long)N * C * Hs * Ws + 255) / 256;
  if (blocks > LIM) return -3;
  const float sh = (float)Hs / (float)Ho, sw = (float)Ws / (float)Wo;
  const float ih = (float)Ho / (float)Hs, iw = (float)Wo / (float)Ws;
  if (Hs != Ho || Ws != Wo)
    hipLaunchKernelGGL(perc_stage_bwd_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s,
                       (const bf16r*)g, recon, N, C, Hs, Ws, Ho, Wo, Cp, sh, sw, ih, iw, mode, dx);
  else
    hipLaunchKernelGGL(perc_stage_bwd_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s,
                       (const bf16r*)g, recon, N, C, Hs, Ws, Ho, Wo, Cp, sh, sw, ih, iw, mode, dx);
  return (int)hipGetLastError();
}

extern "C" int64_t fmd_perc_tap_workspace(int32_t N, int32_t H, int32_t W, int32_t Cp) {
  const long long b = tap_blocks(N, H, W, Cp, Cp);
  return b < 0 ? -1 : b * 8;
}

extern "C" int fmd_perc_tap_fwd(const float* y, int32_t N, int32_t H, int32_t W, int32_t Cp, int32_t C, int32_t pool,
                                void* out, void* sgn, void* ws, float weight, int32_t first, float* value,
                                float* loss, fmd_stream_t s) {
  const long long blocks = tap_blocks(N, H, W, Cp, C);
  if (blocks < 0 || !y || !ws || !value) return -1;
  if (out && pool && (H < 2 || W < 2)) return -1;   // the pooled map would be empty
  if (!al(y, 16) || !al(out, 16) || !al(sgn, 8) || !al(ws, 8) || !al(value, 4) || !al(loss, 4)) return -2;
  TapArgs a = {};
  a.y = y, a.N = N, a.H = H, a.W = W, a.Cp = Cp, a.C = C, a.pool = pool != 0;
  a.out = (bf16r*)out, a.sgn = (signed char*)sgn, a.part = (double*)ws;
  hipLaunchKernelGGL(perc_tap_fwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, a);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(perc_tap_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, (const double*)ws, blocks,
                     (double)N * (double)C * (double)H * (double)W, weight, first != 0, value, loss);
  return (int)hipGetLastError();
}

extern "C" int fmd_perc_tap_bwd(const float* y_rec, const void* sgn, int32_t N, int32_t H, int32_t W, int32_t Cp,
                                int32_t C, int32_t pool, const void* g_below, const float* g_loss, float weight,
                                void* dy, fmd_stream_t s) {
  const long long blocks = tap_blocks(N, H, W, Cp, C);
  if (blocks < 0 || !y_rec || !sgn || !g_loss || !dy) return -1;
  if (g_below && pool && (H < 2 || W < 2)) return -1;
  if (!al(y_rec, 16) || !al(sgn, 8) || !al(g_below, 16) || !al(g_loss, 4) || !al(dy, 16)) return -2;
  TapArgs a = {};
  a.y = y_rec, a.N = N, a.H = H, a.W = W, a.Cp = Cp, a.C = C, a.pool = pool != 0;
  a.sgn = (signed char*)sgn, a.gbelow = (const bf16r*)g_below, a.gloss = g_loss, a.weight = weight;
  a.count = (double)N * (double)C * (double)H * (double)W;
  a.dy = (bf16r*)dy;
  hipLaunchKernelGGL(perc_tap_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, a);
  return (int)hipGetLastError();
}
