// The VAE training criterion (reference src/nn/losses/vae.py:104-151, src/models/autoencoder/base.py:21-28,
// src/pipelines/train/vae_lib.py:226-275 and src/nn/modules/vae/reparameterizer.py:19-47): one element-wise
// loss-and-reduce kernel templated over the term, and the posterior kernel (clamp, reparameterise, KL) with its
// backward.
//
// Arithmetic, which tests/vae_loss_bounds.py restates: inputs are fp32.  img = (clamp(x, -1, 1) + 1) * 0.5 is
// the three fp32 operations of torch, so img, the clamp mask and sign(img - t) are the bits torch sees.
// Everything after that is fp64, transcendentals included (exp, log1p, expm1 of the device's fp64 library), and
// every value written is ONE rounding of its fp64 value to fp32 (the bf16 copies: f2bf of that fp32).  Sums are
// fp64 in a fixed order: a thread adds its elements in ascending order, a fixed butterfly adds the 64 lanes, the
// four wave totals are added in order into one partial per workgroup, and a finishing launch adds the partials
// thread-strided and then by a fixed tree.  No atomics; the grid depends on the problem size only.
//
// This is memory- and launch-bound work: 256 threads, 16-byte accesses where the layout allows them, no LDS
// beyond the block reduction.
#include "common.h"
#include "fmdiff.h"

#include <math.h>

namespace {

constexpr int VL_CHUNK = FMD_VAE_LOSS_CHUNK;   // flat elements per workgroup: 256 threads x 2 trips x 4
constexpr int VL_ROWS = FMD_VAE_LOSS_ROWS;     // head-layout pixels per workgroup: 256 threads x 2 trips
constexpr int GS_ROWS = FMD_GAUSS_ROWS;        // posterior pixels per workgroup: one per thread
static_assert(VL_CHUNK % 1024 == 0 && VL_ROWS % 256 == 0 && GS_ROWS == 256, "trip counts");

enum { T_L1, T_MSE, T_BCE, T_FOCAL, T_BCE_FOCAL, T_HINGE_REAL, T_HINGE_FAKE, T_NEG, T_SQUARE, T_COUNT };

// v: the term, u: d term / d x, both fp64.  Comparisons with a NaN are false: a NaN x gives a NaN term.
template <int T>
FMD_DEV void term_of(float xf, float tf, double alpha, double& v, double& u) {
  if (T == T_L1 || T == T_MSE) {
    const float cl = xf < -1.f ? -1.f : (xf > 1.f ? 1.f : xf);
    const float img = (cl + 1.0f) * 0.5f;
    const double d = (double)img - (double)tf;
    const double m = (xf >= -1.f && xf <= 1.f) ? 1.0 : 0.0;   // inclusive, as torch.clamp's backward
    if (T == T_L1) {
      v = fabs(d);
      u = (d > 0.0 ? 0.5 : (d < 0.0 ? -0.5 : 0.0)) * m;
    } else {
      v = d * d;
      u = d * m;   // 2 (img - t) * 0.5
    }
  } else if (T == T_BCE || T == T_FOCAL || T == T_BCE_FOCAL) {
    const double x = (double)xf, t = (double)tf;
    const double e = exp(-fabs(x));
    const double r = 1.0 / (1.0 + e);
    const double sp = x >= 0.0 ? r : e * r;   // sigma(x)
    const double sn = x >= 0.0 ? e * r : r;   // sigma(-x)
    // max(x, 0) - x t, without the cancellation
    const double ce = (x > 0.0 ? x * (1.0 - t) : -x * t) + log1p(e);
    v = 0.0;
    u = 0.0;
    if (T != T_FOCAL) {
      v = ce;
      u = sp - t;
    }
    if (T != T_BCE) {
      const double q = t * sn + (1.0 - t) * sp;   // 1 - p_t
      const double at = alpha * t + (1.0 - alpha) * (1.0 - t);
      v += at * (q * q) * ce;
      u += at * ((q * q) * (sp - t) - 2.0 * q * sp * sn * (2.0 * t - 1.0) * ce);
    }
  } else if (T == T_HINGE_REAL) {
    v = xf < 1.f ? 1.0 - (double)xf : (xf == xf ? 0.0 : (double)xf);
    u = xf < 1.f ? -1.0 : 0.0;
  } else if (T == T_HINGE_FAKE) {
    v = xf > -1.f ? 1.0 + (double)xf : (xf == xf ? 0.0 : (double)xf);
    u = xf > -1.f ? 1.0 : 0.0;
  } else if (T == T_NEG) {
    v = -(double)xf;
    u = -1.0;
  } else {
    v = (double)xf * (double)xf;
    u = 2.0 * (double)xf;
  }
}

struct LossArgs {
  const float* x;
  const float* t;
  long long N, C, P;   // flat: N = C = 1, P = the element count
  int ld;              // head layout: row stride of x and dx; flat: 0
  double alpha;
  const float* g;      // upstream gradient: one element, or one per element of the term (g_elem)
  int g_elem;
  double gscale;       // scale (x 1 / count for the mean)
  double* part;        // one partial per workgroup, or null
  float* elem;         // per-element term, or null
  float* dx;           // gradient in x's layout, or null
  bf16r* dxb;          // bf16 copy [N * P][ldb] (head layout), or null
  int ldb;
  int vec;             // bit 0: x / t / g / elem / dx (flat) or dx rows (head) take 16-byte accesses; bit 1: dxb rows
};

template <int T, bool TGT>
__global__ __launch_bounds__(256) void vae_loss_flat_kernel(LossArgs a) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const long long n = a.P, base = (long long)blockIdx.x * VL_CHUNK;
  const bool want_g = a.dx != nullptr;
  const double g0 = want_g && !a.g_elem ? (double)a.g[0] * a.gscale : 0.0;
  double acc = 0.0;
#pragma unroll
  for (int trip = 0; trip < VL_CHUNK / 1024; ++trip) {
    const long long e0 = base + trip * 1024 + tid * 4;
    if (e0 >= n) break;
    const bool full = (a.vec & 1) && e0 + 4 <= n;
    alignas(16) float xv[4], tv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f}, ev[4], dv[4];
    if (full) {
      *(f32x4*)xv = *(const f32x4*)(a.x + e0);
      if (TGT) *(f32x4*)tv = *(const f32x4*)(a.t + e0);
      if (want_g && a.g_elem) *(f32x4*)gv = *(const f32x4*)(a.g + e0);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = e0 + j < n;
        xv[j] = in ? a.x[e0 + j] : 0.f;
        if (TGT) tv[j] = in ? a.t[e0 + j] : 0.f;
        if (want_g && a.g_elem) gv[j] = in ? a.g[e0 + j] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      double v, u;
      term_of<T>(xv[j], tv[j], a.alpha, v, u);
      if (e0 + j < n) acc += v;
      ev[j] = (float)v;
      dv[j] = (float)((a.g_elem ? (double)gv[j] * a.gscale : g0) * u);
    }
    if (full) {
      if (a.elem) *(f32x4*)(a.elem + e0) = *(f32x4*)ev;
      if (want_g) *(f32x4*)(a.dx + e0) = *(f32x4*)dv;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + j < n) {
          if (a.elem) a.elem[e0 + j] = ev[j];
          if (want_g) a.dx[e0 + j] = dv[j];
        }
    }
  }
  if (a.part) {
    const double s = block_sum(acc, red);
    if (tid == 0) a.part[blockIdx.x] = s;
  }
}

// x channels-last [N][P][ld] (channels >= C are never read), target / g / elem channels-first [N][C][P]
template <int T>
__global__ __launch_bounds__(256) void vae_loss_head_kernel(LossArgs a) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const long long rows = a.N * a.P;
  const int C = (int)a.C;
  const bool want_g = a.dx != nullptr || a.dxb != nullptr;
  const double g0 = want_g && !a.g_elem ? (double)a.g[0] * a.gscale : 0.0;
  const int lmax = a.dx && a.dxb ? (a.ld > a.ldb ? a.ld : a.ldb) : (a.dx ? a.ld : (a.dxb ? a.ldb : 0));
  double acc = 0.0;
#pragma unroll 1
  for (int trip = 0; trip < VL_ROWS / 256; ++trip) {
    const long long r = (long long)blockIdx.x * VL_ROWS + trip * 256 + tid;
    if (r >= rows) break;
    const long long n = r / a.P, p = r - n * a.P;
    const float* row = a.x + (size_t)r * a.ld;
    const int cend = want_g ? (lmax > C ? lmax : C) : C;
    for (int c0 = 0; c0 < cend; c0 += 8) {
      float dv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        dv[j] = 0.f;
        if (c < C) {
          const size_t ti = ((size_t)n * C + c) * (size_t)a.P + (size_t)p;
          double v, u;
          term_of<T>(row[c], a.t[ti], a.alpha, v, u);
          acc += v;
          if (a.elem) a.elem[ti] = (float)v;
          if (want_g) dv[j] = (float)((a.g_elem ? (double)a.g[ti] * a.gscale : g0) * u);
        }
      }
      if (a.dx) {
        float* d = a.dx + (size_t)r * a.ld + c0;
        if ((a.vec & 1) && c0 + 8 <= a.ld) {
          *(f32x4*)d = f32x4{dv[0], dv[1], dv[2], dv[3]};
          *(f32x4*)(d + 4) = f32x4{dv[4], dv[5], dv[6], dv[7]};
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (c0 + j < a.ld) d[j] = dv[j];
        }
      }
      if (a.dxb) {
        bf16r* d = a.dxb + (size_t)r * a.ldb + c0;
        if ((a.vec & 2) && c0 + 8 <= a.ldb) {
          *(u32x4*)d = u32x4{pack2(dv[0], dv[1]), pack2(dv[2], dv[3]), pack2(dv[4], dv[5]), pack2(dv[6], dv[7])};
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (c0 + j < a.ldb) d[j] = (bf16r)f2bf(dv[j]);
        }
      }
    }
  }
  if (a.part) {
    const double s = block_sum(acc, red);
    if (tid == 0) a.part[blockIdx.x] = s;
  }
}

// out[b] = (float)(sum of part[b * P .. b * P + P - 1] / div): thread-strided in ascending order, then a fixed tree
__global__ __launch_bounds__(256) void vae_sum_final_kernel(const double* __restrict__ part, long long P, double div,
                                                            float* __restrict__ out) {
  __shared__ double r[256];
  const int tid = threadIdx.x;
  const double* p = part + (size_t)blockIdx.x * (size_t)P;
  double s = 0.0;
  for (long long i = tid; i < P; i += 256) s += p[i];
  r[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) r[tid] += r[tid + o];
    __syncthreads();
  }
  if (tid == 0) out[blockIdx.x] = (float)(r[0] / div);
}

FMD_DEV float clamp_lv(float lv) { return lv < -30.f ? -30.f : (lv > 20.f ? 20.f : lv); }

// Workgroup (n, b): pixels b * 256 .. of sample n.  part[n * bps + b] = sum over its pixels and channels of
// mu^2 + expm1(lv) - lv.
__global__ __launch_bounds__(256) void gauss_fwd_kernel(const float* __restrict__ mom, int ldm, int E, long long P,
                                                        int bps, const float* __restrict__ eps,
                                                        float* __restrict__ z, bf16r* __restrict__ zs, int Cp,
                                                        int vec, double* __restrict__ part) {
  __shared__ double red[4];
  const int tid = threadIdx.x;
  const long long n = blockIdx.x / bps;
  const long long p = (long long)(blockIdx.x % bps) * GS_ROWS + tid;
  double acc = 0.0;
  if (p < P) {
    const size_t r = (size_t)n * (size_t)P + (size_t)p;
    const float* row = mom + r * ldm;
    const int cend = zs ? Cp : E;
    for (int c0 = 0; c0 < cend; c0 += 8) {
      float zv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + j;
        zv[j] = 0.f;
        if (c < E) {
          const float mu = row[c], lv = clamp_lv(row[E + c]);
          const size_t zi = ((size_t)n * E + c) * (size_t)P + (size_t)p;
          float zf = mu;
          if (eps) zf = (float)((double)mu + exp(0.5 * (double)lv) * (double)eps[zi]);
          z[zi] = zf;
          zv[j] = zf;
          acc += (double)mu * (double)mu + (expm1((double)lv) - (double)lv);
        }
      }
      if (zs) {
        bf16r* d = zs + r * Cp + c0;
        if (vec && c0 + 8 <= Cp) {
          *(u32x4*)d = u32x4{pack2(zv[0], zv[1]), pack2(zv[2], zv[3]), pack2(zv[4], zv[5]), pack2(zv[6], zv[7])};
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            if (c0 + j < Cp) d[j] = (bf16r)f2bf(zv[j]);
        }
      }
    }
  }
  const double s = block_sum(acc, red);
  if (tid == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void gauss_bwd_kernel(const float* __restrict__ mom, int ldm, long long N, int E,
                                                        long long P, const float* __restrict__ eps,
                                                        const float* __restrict__ gz, const float* __restrict__ gkl,
                                                        float* __restrict__ dm, int ldd, bf16r* __restrict__ dmb,
                                                        int ldb, int vec) {
  const long long r = (long long)blockIdx.x * GS_ROWS + threadIdx.x;
  if (r >= N * P) return;
  const long long n = r / P, p = r - n * P;
  const float* row = mom + (size_t)r * ldm;
  const double gk = gkl ? (double)gkl[n] : 0.0;
  const int cend = dm && dmb ? (ldd > ldb ? ldd : ldb) : (dm ? ldd : ldb);
  for (int c0 = 0; c0 < cend; c0 += 8) {
    float dv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + j;
      dv[j] = 0.f;
      if (c < 2 * E) {
        const int ch = c < E ? c : c - E;
        const size_t zi = ((size_t)n * E + ch) * (size_t)P + (size_t)p;
        const double g = gz ? (double)gz[zi] : 0.0;
        if (c < E) {
          dv[j] = (float)(g + gk * (double)row[c]);
        } else {
          const float raw = row[c];
          const double lv = (double)clamp_lv(raw);
          const double m = (raw >= -30.f && raw <= 20.f) ? 0.5 : 0.0;   // inclusive, as torch.clamp's backward
          const double e = eps ? (double)eps[zi] : 0.0;
          dv[j] = (float)(m * (g * e * exp(0.5 * lv) + gk * expm1(lv)));
        }
      }
    }
    if (dm) {
      float* d = dm + (size_t)r * ldd + c0;
      if ((vec & 1) && c0 + 8 <= ldd) {
        *(f32x4*)d = f32x4{dv[0], dv[1], dv[2], dv[3]};
        *(f32x4*)(d + 4) = f32x4{dv[4], dv[5], dv[6], dv[7]};
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (c0 + j < ldd) d[j] = dv[j];
      }
    }
    if (dmb) {
      bf16r* d = dmb + (size_t)r * ldb + c0;
      if ((vec & 2) && c0 + 8 <= ldb) {
        *(u32x4*)d = u32x4{pack2(dv[0], dv[1]), pack2(dv[2], dv[3]), pack2(dv[4], dv[5]), pack2(dv[6], dv[7])};
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (c0 + j < ldb) d[j] = (bf16r)f2bf(dv[j]);
      }
    }
  }
}

constexpr long long LIM = (1ll << 31) - 1;

bool aligned16(const void* p) { return ((unsigned long long)p & 15) == 0; }

bool has_target(int term) { return term <= T_BCE_FOCAL; }

// workgroups of the loss launch, or -1
long long loss_blocks(int term, long long N, long long C, long long P, int ld) {
  if (term < 0 || term >= T_COUNT || N < 1 || C < 1 || P < 1 || N > LIM || C > LIM || P > (1ll << 44)) return -1;
  long long b;
  if (ld > 0) {
    if (!has_target(term) || C > ld || P > (1ll << 40) || N * P > (1ll << 40)) return -1;
    b = (N * P + VL_ROWS - 1) / VL_ROWS;
  } else {
    if (ld < 0 || N != 1 || C != 1) return -1;
    b = (P + VL_CHUNK - 1) / VL_CHUNK;
  }
  return b > LIM ? -1 : b;
}

long long gauss_bps(long long N, long long E, long long P) {
  if (N < 1 || E < 1 || P < 1 || N > LIM || E > (1 << 20) || P > LIM) return -1;
  const long long bps = (P + GS_ROWS - 1) / GS_ROWS;
  return N * bps > LIM ? -1 : bps;
}

template <int T>
void launch_loss(const LossArgs& a, long long blocks, hipStream_t s) {
  if (a.ld > 0)
    hipLaunchKernelGGL(vae_loss_head_kernel<T>, dim3((unsigned)blocks), dim3(256), 0, s, a);
  else
    hipLaunchKernelGGL((vae_loss_flat_kernel<T, (T <= T_BCE_FOCAL)>), dim3((unsigned)blocks), dim3(256), 0, s, a);
}

}  // namespace

extern "C" int64_t fmd_vae_loss_workspace(int32_t term, int32_t N, int32_t C, int64_t P, int32_t ld) {
  const long long b = loss_blocks(term, N, C, P, ld);
  return b < 0 ? -1 : b * 8;
}

extern "C" int fmd_vae_loss(int32_t term, int32_t reduction, const float* x, const float* target, int32_t N,
                            int32_t C, int64_t P, int32_t ld, float alpha, const float* g, int32_t g_elem,
                            float scale, void* ws, float* loss, float* elem, float* dx, void* dx_bf16, int32_t ldb,
                            fmd_stream_t s) {
  const long long blocks = loss_blocks(term, N, C, P, ld);
  const bool want_g = dx || dx_bf16;
  if (blocks < 0 || !x || reduction < 0 || reduction > 2 || (has_target(term) && !target) || (want_g && !g) ||
      (loss && (!ws || reduction == 0)) || (dx_bf16 && (ld <= 0 || ldb < C)) || (!loss && !elem && !want_g))
    return -1;
  const double count = (double)N * (double)C * (double)P;
  LossArgs a;
  a.x = x;
  a.t = has_target(term) ? target : nullptr;
  a.N = N, a.C = C, a.P = P, a.ld = ld;
  a.alpha = (double)alpha;
  a.g = g, a.g_elem = g_elem != 0;
  a.gscale = reduction == 2 ? (double)scale / count : (double)scale;
  a.part = loss ? (double*)ws : nullptr;
  a.elem = elem, a.dx = dx, a.dxb = (bf16r*)dx_bf16, a.ldb = ldb;
  if (ld > 0)
    a.vec = ((ld % 8 == 0 && aligned16(dx)) ? 1 : 0) | ((ldb % 8 == 0 && aligned16(dx_bf16)) ? 2 : 0);
  else
    a.vec = aligned16(x) && aligned16(a.t) && aligned16(elem) && aligned16(dx) && (!a.g_elem || aligned16(g));
  hipStream_t st = (hipStream_t)s;
  switch (term) {
    case T_L1: launch_loss<T_L1>(a, blocks, st); break;
    case T_MSE: launch_loss<T_MSE>(a, blocks, st); break;
    case T_BCE: launch_loss<T_BCE>(a, blocks, st); break;
    case T_FOCAL: launch_loss<T_FOCAL>(a, blocks, st); break;
    case T_BCE_FOCAL: launch_loss<T_BCE_FOCAL>(a, blocks, st); break;
    case T_HINGE_REAL: launch_loss<T_HINGE_REAL>(a, blocks, st); break;
    case T_HINGE_FAKE: launch_loss<T_HINGE_FAKE>(a, blocks, st); break;
    case T_NEG: launch_loss<T_NEG>(a, blocks, st); break;
    default: launch_loss<T_SQUARE>(a, blocks, st); break;
  }
  int rc = (int)hipGetLastError();
  if (rc || !loss) return rc;
  hipLaunchKernelGGL(vae_sum_final_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, blocks,
                     reduction == 2 ? count : 1.0, loss);
  return (int)hipGetLastError();
}

extern "C" int64_t fmd_gauss_workspace(int32_t N, int32_t E, int64_t P) {
  const long long bps = gauss_bps(N, E, P);
  return bps < 0 ? -1 : (int64_t)N * bps * 8;
}

extern "C" int fmd_gauss_sample_kl(const float* moments, int32_t ldm, int32_t N, int32_t E, int64_t P,
                                   const float* eps, float* z, void* z_staged, int32_t Cp, void* ws, float* kl,
                                   fmd_stream_t s) {
  const long long bps = gauss_bps(N, E, P);
  if (bps < 0 || !moments || !z || !ws || !kl || ldm < 2 * E || (z_staged && Cp < E)) return -1;
  const int vec = z_staged && Cp % 8 == 0 && aligned16(z_staged);
  hipLaunchKernelGGL(gauss_fwd_kernel, dim3((unsigned)(N * bps)), dim3(256), 0, (hipStream_t)s, moments, ldm, E,
                     (long long)P, (int)bps, eps, z, (bf16r*)z_staged, Cp, vec, (double*)ws);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(vae_sum_final_kernel, dim3(N), dim3(256), 0, (hipStream_t)s, (const double*)ws, bps, 2.0, kl);
  return (int)hipGetLastError();
}

extern "C" int fmd_gauss_backward(const float* moments, int32_t ldm, int32_t N, int32_t E, int64_t P,
                                  const float* eps, const float* g_z, const float* g_kl, float* d_moments,
                                  int32_t ldd, void* d_moments_bf16, int32_t ldb, fmd_stream_t s) {
  const long long bps = gauss_bps(N, E, P);
  if (bps < 0 || !moments || ldm < 2 * E || (!d_moments && !d_moments_bf16) || (d_moments && ldd < 2 * E) ||
      (d_moments_bf16 && ldb < 2 * E))
    return -1;
  const long long blocks = ((long long)N * P + GS_ROWS - 1) / GS_ROWS;
  if (blocks > LIM) return -1;
  const int vec = ((d_moments && ldd % 8 == 0 && aligned16(d_moments)) ? 1 : 0) |
                  ((d_moments_bf16 && ldb % 8 == 0 && aligned16(d_moments_bf16)) ? 2 : 0);
  hipLaunchKernelGGL(gauss_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)s, moments, ldm,
                     (long long)N, E, (long long)P, eps, g_z, g_kl, d_moments, ldd, (bf16r*)d_moments_bf16, ldb, vec);
  return (int)hipGetLastError();
}
