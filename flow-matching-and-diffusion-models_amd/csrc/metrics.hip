// Per-image MSE, PSNR and SSIM of the evaluate modes (reference src/pipelines/samplers/diffusion_like.py:251-263
// and src/utils/evaluation_utils.py:64-91, which calls skimage's structural_similarity with its defaults:
// uniform 7-wide window over every spatial axis, sample covariance, C1 = 1e-4, C2 = 9e-4, 3 positions cropped
// from every side).  One read of both tensors gives the three numbers per image, on the device.
//
// Every operation from the window moments through S is fp64 ("Image metrics: fp64 bound":
// fp32 window sums cost up to 4.7e-4 of the image mean because vx sits next to C2).  The window moments are
// DIRECT sums, 49 or 343 terms in a fixed order, no sliding add/subtract: that is what the bound is derived for.
//
// Tiling: one workgroup per (image, channel, tile of window positions).  The haloed tile of both images is
// staged once in LDS as fp32 (after the clamp).  A thread owns one column of the tile and RUN consecutive
// positions along the march axis (y in 2-D, z in 3-D): it sums the five moments x, y, x^2, y^2, xy over the
// window's cross-section (7 taps in 2-D, 7 x 7 in 3-D) at RUN + 6 march positions, and adds each cross-section
// to the (at most seven) windows that contain it, so every window is its seven cross-sections added in march
// order.  The squared error of the elements a tile owns is summed while the tile is staged.  Each workgroup
// writes one (squared error, sum of S) partial; a second launch sums an image's partials in a fixed order.  No
// atomics: an image's numbers depend on its own C and spatial shape only.
#include "common.h"
#include "fmdiff.h"

#include <math.h>

namespace {

constexpr int MT_WIN = 7;
constexpr int MT_HALO = MT_WIN - 1;
constexpr int MT_CHUNK = 4096;     // elements per workgroup of the 1-D (no SSIM) kernel
constexpr double MT_C1 = 1e-4, MT_C2 = 9e-4;

// window positions per workgroup [x, y, z] and per thread along the march axis (RUN): a thread computes
// RUN + 6 cross-sections for RUN windows; THREADS = TX * TY * TZ / RUN
template <int ND>
struct Tile;
template <>
struct Tile<2> {
  static constexpr int TX = 32, TY = 32, TZ = 1, LZ = 1, RUN = 4, THREADS = 256, MIN_WG = 2;
};
template <>
struct Tile<3> {   // 34.5 KB of LDS and 128 threads: four workgroups per CU
  static constexpr int TX = 8, TY = 8, TZ = 16, LZ = TZ + MT_HALO, RUN = 8, THREADS = 128, MIN_WG = 4;
};

struct Mom {
  double x, y, xx, yy, xy;
};

// torch.clamp(v, 0, 1): both comparisons are false for a NaN, which therefore passes through
FMD_DEV float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

FMD_DEV void mom_add(Mom& m, float a, float b) {
  const double x = (double)a, y = (double)b;
  m.x += x;
  m.y += y;
  m.xx += x * x;   // the product of two fp32 values is exact in fp64
  m.yy += y * y;
  m.xy += x * y;
}

// S of one window from its moment sums.  Contraction is off and the numerator and denominator are built from the
// same roundings, so identical images give num == den bit for bit and S == 1.0 exactly.
FMD_DEV double ssim_point(const Mom& s, double inv_np, double cov) {
#pragma clang fp contract(off)
  const double ux = s.x * inv_np, uy = s.y * inv_np;
  const double uxx = ux * ux, uyy = uy * uy, uxy = ux * uy;
  const double vx = cov * (s.xx * inv_np - uxx);
  const double vy = cov * (s.yy * inv_np - uyy);
  const double vxy = cov * (s.xy * inv_np - uxy);
  const double a1 = 2.0 * uxy + MT_C1, a2 = 2.0 * vxy + MT_C2;
  const double b1 = (uxx + uyy) + MT_C1, b2 = (vx + vy) + MT_C2;
  return (a1 * a2) / (b1 * b2);
}

// NW waves: fixed butterfly within a wave, then the wave totals in order.  Thread 0 holds the result.
template <int NW>
FMD_DEV void block_sum2(double& a, double& b, double* red) {
  a = wave_sum_f64(a);
  b = wave_sum_f64(b);
  const int tid = threadIdx.x;
  if ((tid & 63) == 0) {
    red[2 * (tid >> 6)] = a;
    red[2 * (tid >> 6) + 1] = b;
  }
  __syncthreads();
  if (tid == 0) {
    a = red[0];
    b = red[1];
#pragma unroll
    for (int w = 1; w < NW; ++w) {
      a += red[2 * w];
      b += red[2 * w + 1];
    }
  }
}

// part[((nc * ntz + tz) * nty + ty) * ntx + tx] = {squared error of the owned elements, sum of S}
template <int ND>
__global__ __launch_bounds__(Tile<ND>::THREADS, Tile<ND>::MIN_WG) void metrics_tile_kernel(const float* __restrict__ gen,
                                                           const float* __restrict__ tgt, int D, int H, int W,
                                                           int ntx, int nty, int ntz, int clamp,
                                                           double* __restrict__ part) {
  using T = Tile<ND>;
  constexpr int TX = T::TX, TY = T::TY, TZ = T::TZ, RUN = T::RUN, NT = T::THREADS;
  static_assert(TX * TY * TZ == RUN * NT, "one thread per column and run");
  constexpr int LX = TX + MT_HALO, LY = TY + MT_HALO, LZ = T::LZ;
  constexpr int NL = LZ * LY * LX;
  __shared__ float sg[NL], st[NL];
  __shared__ double red[8];
  const int tid = threadIdx.x;
  long long b = blockIdx.x;
  const int tx = (int)(b % ntx);
  b /= ntx;
  const int ty = (int)(b % nty);
  b /= nty;
  const int tz = (int)(b % ntz);
  const long long nc = b / ntz;
  const int x0 = tx * TX, y0 = ty * TY, z0 = tz * TZ;
  const int Dd = ND == 3 ? D : 1;
  const size_t base = (size_t)nc * Dd * H * W;
  // every element belongs to exactly one tile: the tile's own TX x TY x TZ block, and the last tile of an axis
  // also takes the halo behind it (it reaches the image's edge: ntx * TX >= W - 6)
  const int ownx = tx == ntx - 1 ? LX : TX, owny = ty == nty - 1 ? LY : TY;
  const int ownz = ND == 3 ? (tz == ntz - 1 ? LZ : TZ) : 1;

  double se = 0.0;
  for (int e = tid; e < NL; e += NT) {
    const int lx = e % LX, ly = (e / LX) % LY, lz = e / (LX * LY);
    const int gx = x0 + lx, gy = y0 + ly, gz = z0 + lz;
    float a = 0.f, c = 0.f;   // outside the image: read by masked positions only
    if (gx < W && gy < H && gz < Dd) {
      const size_t i = base + ((size_t)gz * H + gy) * W + gx;
      a = gen[i];
      c = tgt[i];
      if (clamp) {
        a = clamp01(a);
        c = clamp01(c);
      }
      if (lx < ownx && ly < owny && lz < ownz) {
        const double d = (double)a - (double)c;
        se += d * d;
      }
    }
    sg[e] = a;
    st[e] = c;
  }
  __syncthreads();

  // thread -> column and march start
  int cx, cy, m0;
  if (ND == 2) {
    cx = tid & (TX - 1);
    cy = 0;
    m0 = (tid / TX) * RUN;
  } else {
    cx = tid & (TX - 1);
    cy = (tid / TX) & (TY - 1);
    m0 = (tid / (TX * TY)) * RUN;
  }
  const int Wo = W - MT_HALO, Ho = H - MT_HALO, Do = ND == 3 ? D - MT_HALO : 1;
  // positions of this thread's run inside the image (march axis: y in 2-D, z in 3-D)
  const int Mo = ND == 2 ? Ho : Do, mg = (ND == 2 ? y0 : z0) + m0;
  int nrun = Mo - mg;
  nrun = nrun > RUN ? RUN : nrun;
  if (x0 + cx >= Wo || (ND == 3 && y0 + cy >= Ho)) nrun = 0;

  double ss = 0.0;
  if (nrun > 0) {
    const double np = ND == 2 ? 49.0 : 343.0;
    const double inv_np = 1.0 / np, cov = np / (np - 1.0);
    Mom win[RUN];
#pragma unroll
    for (int r = 0; r < RUN; ++r) win[r] = {0.0, 0.0, 0.0, 0.0, 0.0};
    // the march loop stays rolled: unrolled, hipcc hoists every LDS read of the run and spills in 3-D
#pragma unroll 1
    for (int m = 0; m < RUN + MT_HALO; ++m) {
      Mom s = {0.0, 0.0, 0.0, 0.0, 0.0};
      if (ND == 2) {
        const int o = (m0 + m) * LX + cx;
#pragma unroll
        for (int dx = 0; dx < MT_WIN; ++dx) mom_add(s, sg[o + dx], st[o + dx]);
      } else {
#pragma unroll 1
        for (int dy = 0; dy < MT_WIN; ++dy) {
          const int o = ((m0 + m) * LY + cy + dy) * LX + cx;
#pragma unroll
          for (int dx = 0; dx < MT_WIN; ++dx) mom_add(s, sg[o + dx], st[o + dx]);
        }
      }
      // cross-section m belongs to the windows r = m - 6 .. m (adding 0.0 elsewhere is exact), so a window is
      // s_r + s_r+1 + ... + s_r+6 in this order
#pragma unroll
      for (int r = 0; r < RUN; ++r) {
        const bool in = r <= m && m <= r + MT_HALO;
        win[r].x += in ? s.x : 0.0;
        win[r].y += in ? s.y : 0.0;
        win[r].xx += in ? s.xx : 0.0;
        win[r].yy += in ? s.yy : 0.0;
        win[r].xy += in ? s.xy : 0.0;
      }
    }
#pragma unroll
    for (int r = 0; r < RUN; ++r)
      if (r < nrun) ss += ssim_point(win[r], inv_np, cov);
  }
  block_sum2<NT / 64>(se, ss, red);
  if (tid == 0) {
    part[2 * (size_t)blockIdx.x] = se;
    part[2 * (size_t)blockIdx.x + 1] = ss;
  }
}

// [N, C, L] signals: squared error only.  part[(n * chunks + chunk)] = {squared error, 0}
__global__ __launch_bounds__(256) void metrics_signal_kernel(const float* __restrict__ gen,
                                                             const float* __restrict__ tgt, long long per_image,
                                                             int chunks, int clamp, double* __restrict__ part) {
  __shared__ double red[8];
  const long long n = blockIdx.x / chunks, ch = blockIdx.x % chunks;
  const long long e0 = ch * MT_CHUNK;
  const long long e1 = e0 + MT_CHUNK < per_image ? e0 + MT_CHUNK : per_image;
  double se = 0.0, zero = 0.0;
  for (long long e = e0 + threadIdx.x; e < e1; e += 256) {
    float a = gen[(size_t)(n * per_image + e)], c = tgt[(size_t)(n * per_image + e)];
    if (clamp) {
      a = clamp01(a);
      c = clamp01(c);
    }
    const double d = (double)a - (double)c;
    se += d * d;
  }
  block_sum2<4>(se, zero, red);
  if (threadIdx.x == 0) {
    part[2 * (size_t)blockIdx.x] = se;
    part[2 * (size_t)blockIdx.x + 1] = 0.0;
  }
}

// One workgroup per image: its P partials summed thread-strided, then a fixed tree.  npos == 0: no SSIM (NaN).
__global__ __launch_bounds__(256) void metrics_final_kernel(const double* __restrict__ part, long long P,
                                                            double count, double npos, double* __restrict__ mse,
                                                            double* __restrict__ psnr, double* __restrict__ ssim) {
  __shared__ double r1[256], r2[256];
  const int tid = threadIdx.x;
  const double* p = part + 2 * (size_t)blockIdx.x * (size_t)P;
  double se = 0.0, ss = 0.0;
  for (long long i = tid; i < P; i += 256) {
    se += p[2 * i];
    ss += p[2 * i + 1];
  }
  r1[tid] = se;
  r2[tid] = ss;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      r1[tid] += r1[tid + o];
      r2[tid] += r2[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double m = r1[0] / count;
    mse[blockIdx.x] = m;
    // 10 log10(1 / max(m, 1e-12)); a NaN fails the comparison and reaches log10
    psnr[blockIdx.x] = m <= 1e-12 ? 120.0 : 10.0 * log10(1.0 / m);
    ssim[blockIdx.x] = npos > 0.0 ? r2[0] / npos : (double)NAN;
  }
}

struct Plan {
  int nd;                 // 1, 2 or 3 spatial axes
  int ntx, nty, ntz;      // tiles per axis (nd >= 2)
  long long per_image;    // partials per image
  double count, npos;     // elements per image; window positions x channels (0: none)
};

int plan_of(long long N, long long C, long long D, long long H, long long W, Plan* p) {
  const long long lim = 1ll << 31;
  if (N < 1 || C < 1 || N >= lim || C >= lim || W >= lim || H >= lim || D >= lim) return -1;
  if (D == 0 && H == 0) {   // [N, C, L]
    if (W < 1 || C * W >= (1ll << 40)) return -1;
    const long long chunks = (C * W + MT_CHUNK - 1) / MT_CHUNK;
    if (N * chunks >= lim) return -1;
    *p = {1, 0, 0, 0, chunks, (double)(C * W), 0.0};
    return 0;
  }
  const int nd = D == 0 ? 2 : 3;
  if (W < MT_WIN || H < MT_WIN || (nd == 3 && D < MT_WIN)) return -1;
  const long long Wo = W - MT_HALO, Ho = H - MT_HALO, Do = nd == 3 ? D - MT_HALO : 1;
  long long ntx, nty, ntz;
  if (nd == 2) {
    ntx = (Wo + Tile<2>::TX - 1) / Tile<2>::TX;
    nty = (Ho + Tile<2>::TY - 1) / Tile<2>::TY;
    ntz = 1;
  } else {
    ntx = (Wo + Tile<3>::TX - 1) / Tile<3>::TX;
    nty = (Ho + Tile<3>::TY - 1) / Tile<3>::TY;
    ntz = (Do + Tile<3>::TZ - 1) / Tile<3>::TZ;
  }
  if (ntx * nty >= lim) return -1;   // every factor is below 2^31: each product is checked before the next
  const long long tiles = ntx * nty * ntz;
  if (tiles >= lim || C * tiles >= lim || N * C * tiles >= lim) return -1;
  *p = {nd, (int)ntx, (int)nty, (int)ntz, C * tiles, (double)C * (double)(nd == 3 ? D : 1) * (double)H * (double)W,
        (double)C * (double)Wo * (double)Ho * (double)Do};
  return 0;
}

}  // namespace

extern "C" int64_t fmd_image_metrics_workspace(int32_t N, int32_t C, int32_t D, int32_t H, int32_t W) {
  Plan p;
  if (plan_of(N, C, D, H, W, &p)) return -1;
  return (int64_t)N * p.per_image * 16;
}

extern "C" int fmd_image_metrics(const float* gen, const float* tgt, int32_t N, int32_t C, int32_t D, int32_t H,
                                 int32_t W, int32_t clamp, void* ws, double* mse, double* psnr, double* ssim,
                                 fmd_stream_t s) {
  Plan p;
  if (!gen || !tgt || !ws || !mse || !psnr || !ssim || plan_of(N, C, D, H, W, &p)) return -1;
  const unsigned grid = (unsigned)((long long)N * p.per_image);
  double* part = (double*)ws;
  if (p.nd == 1)
    hipLaunchKernelGGL(metrics_signal_kernel, dim3(grid), dim3(256), 0, (hipStream_t)s, gen, tgt,
                       (long long)C * W, (int)p.per_image, clamp, part);
  else if (p.nd == 2)
    hipLaunchKernelGGL(metrics_tile_kernel<2>, dim3(grid), dim3(Tile<2>::THREADS), 0, (hipStream_t)s, gen, tgt, 1, H, W, p.ntx,
                       p.nty, p.ntz, clamp, part);
  else
    hipLaunchKernelGGL(metrics_tile_kernel<3>, dim3(grid), dim3(Tile<3>::THREADS), 0, (hipStream_t)s, gen, tgt, D, H, W, p.ntx,
                       p.nty, p.ntz, clamp, part);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(metrics_final_kernel, dim3(N), dim3(256), 0, (hipStream_t)s, part, p.per_image, p.count,
                     p.npos, mse, psnr, ssim);
  return (int)hipGetLastError();
}
