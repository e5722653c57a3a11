// Training half of the vector quantizer (reference src/nn/modules/vae/codebook.py:120-129 and the autograd of
// :41, :79-81, :133-134): the EMA codebook update, the gradient to the latent and the opt-in codebook gradient,
// given the codes and the histogram that fmd_vq_finalize wrote.
//
// The reference forms S_k = sum of the latent rows that chose code k as a [K, M] @ [M, D] product with a one-hot
// matrix.  Here it is a per-code segmented sum without a sort: a workgroup owns a contiguous range of codes,
// scans the M codes in ascending row order 1024 at a time, compacts the rows of its range in that order into
// LDS and adds them, channel by channel, to fp64 accumulators.  Every S_kd is therefore summed in ascending row
// order by one thread, whatever the launch timing: the result is the same bits on every run, and rounding it
// to fp32 once leaves an error of one fp32 rounding.  No atomics, no M x K object, no K x D temporary.
//
// Work split: 256 threads are `groups` rows of 2^dt_shift >= D threads (thread = one channel); group g owns
// codes g * cpg .. g * cpg + cpg - 1 of the workgroup's range (cpg = 2^cpg_shift <= 16), one accumulator slot
// per code in LDS at [slot][thread].  A thread only ever touches its own column of the accumulators.
#include "common.h"
#include "fmdiff.h"

#include <math.h>

namespace {

constexpr int VT_CHUNK = 1024;       // rows scanned per round: 4 consecutive rows per thread
constexpr int VT_CPG_MAX_SHIFT = 4;  // at most 16 codes per thread group
constexpr int VT_TARGET_WG = 1024;   // four workgroups per CU
constexpr int VT_DMAX = 256;
constexpr int VT_FLIGHT = 32;       // row loads a thread keeps outstanding while it adds a segment

struct seg_plan {
  int dt_shift, cpg_shift, cpw, grid;
};

int seg_plan_of(long long M, long long K, long long D, seg_plan* p) {
  if (M < 1 || K < 1 || D < 1 || D > VT_DMAX || M > (1ll << 30) || K > (1ll << 30)) return -1;
  int dts = 3;
  while ((1 << dts) < D) ++dts;
  const int groups = 256 >> dts;
  int cs = 0;
  while (cs < VT_CPG_MAX_SHIFT && (K + ((long long)groups << cs) - 1) / ((long long)groups << cs) > VT_TARGET_WG) ++cs;
  p->dt_shift = dts;
  p->cpg_shift = cs;
  p->cpw = groups << cs;
  p->grid = (int)((K + p->cpw - 1) / p->cpw);
  return 0;
}

// ema_cluster_size <- gamma * ema_cluster_size + (1 - gamma) * n_k for every code, and n = their sum in fp64:
// thread t adds codes t, t + 256, ... in ascending order, then a fixed tree over the 256 partial sums.
__global__ __launch_bounds__(256) void vq_ema_sizes_kernel(const int* __restrict__ hist, int K, float gam, float omg,
                                                           float* __restrict__ cs, double* __restrict__ nsum) {
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0;
  for (int k = tid; k < K; k += 256) {
    const float v = fmaf(omg, (float)hist[k], gam * cs[k]);
    cs[k] = v;
    s += (double)v;
  }
  red[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) nsum[0] = red[0];
}

// Adds entries e .. e + B - 1 of the compacted list to the accumulators of this thread (acc: its column), in order.
// B loads are in flight: a long segment is one thread group streaming its rows, so its speed is the number of
// loads it keeps outstanding, and no load sits under a branch (a load under a condition is waited for before
// the next one is issued): entries past the end or of another thread group read a row of the list all the same
// and drop it.  The sum of the code of the previous row stays in a register (cur, ca): a run of rows of one
// code is a chain of fp64 register additions, not of LDS round trips; the additions and their order are the
// same either way.
template <int B>
FMD_DEV void seg_add(const float* __restrict__ z, int ldz, int d, const int* lrow, const unsigned short* lcode,
                     int e, int n, int g, int cpg_shift, double* acc, int& cur, double& ca) {
  float v[B];
  int sl[B];
#pragma unroll
  for (int u = 0; u < B; ++u) {
    const int idx = e + u < n ? e + u : n - 1;
    const int c = lcode[idx];
    sl[u] = (e + u < n && (c >> cpg_shift) == g) ? (c & ((1 << cpg_shift) - 1)) : -1;
    v[u] = z[(size_t)lrow[idx] * ldz + d];
  }
#pragma unroll
  for (int u = 0; u < B; ++u)
    if (sl[u] >= 0) {
      if (sl[u] != cur) {
        if (cur >= 0) acc[cur * 256] = ca;
        cur = sl[u];
        ca = acc[cur * 256];
      }
      ca += (double)v[u];
    }
}

// MODE 0: the EMA update of ema_w and embedding (+ the bf16 planes and hn of the new embedding, as
// vq_prep_planes / vq_prep_hn of csrc/vq.hip compute them).  MODE 1: dE = coef (n_k e_k - S_k), the codebook
// term of the VQ-VAE loss, coef = g_loss * scale.
template <int MODE>
__global__ __launch_bounds__(256) void vq_segsum_kernel(const float* __restrict__ z, int ldz, int M, int K, int D,
                                                        const long long* __restrict__ codes,
                                                        const int* __restrict__ hist, int dt_shift, int cpg_shift,
                                                        int cpw, float gam, float omg, float eps, float keps,
                                                        const float* __restrict__ cs,
                                                        const double* __restrict__ nsum, float* __restrict__ W,
                                                        float* __restrict__ E, bf16r* __restrict__ Eh,
                                                        bf16r* __restrict__ El, float* __restrict__ hn, int Dpad,
                                                        const float* __restrict__ gl, float scale,
                                                        float* __restrict__ dE) {
  __shared__ double acc[(1 << VT_CPG_MAX_SHIFT) * 256];   // [slot][thread]
  __shared__ int lrow[VT_CHUNK];
  __shared__ unsigned short lcode[VT_CHUNK];              // code - k0 < cpw <= 512
  __shared__ int wtot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cpg = 1 << cpg_shift;
  const int g = tid >> dt_shift, d = tid & ((1 << dt_shift) - 1);
  const long long k0 = (long long)blockIdx.x * cpw;
  for (int s = 0; s < cpg; ++s) acc[s * 256 + tid] = 0.0;

  for (long long r0 = 0; r0 < M; r0 += VT_CHUNK) {
    // ordered compaction of the rows of this round whose code is in [k0, k0 + cpw)
    int loc[4], cnt = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const long long m = r0 + 4 * tid + i;
      int c = -1;
      if (m < M) {
        const long long k = codes[m] - k0;
        if (k >= 0 && k < cpw && k + k0 < K) c = (int)k;
      }
      loc[i] = c;
      cnt += c >= 0;
    }
    int inc = cnt;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    int pos = inc - cnt;
    for (int w = 0; w < wave; ++w) pos += wtot[w];
    const int n = wtot[0] + wtot[1] + wtot[2] + wtot[3];   // <= VT_CHUNK
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (loc[i] >= 0) {
        lrow[pos] = (int)(r0 + 4 * tid + i);
        lcode[pos] = (unsigned short)loc[i];
        ++pos;
      }
    __syncthreads();
    // ascending row order per (code, channel): whole batches of VT_FLIGHT entries, then the rest four at a time
    if (d < D) {
      int cur = -1, e = 0;
      double ca = 0.0;
      for (; e + VT_FLIGHT <= n; e += VT_FLIGHT)
        seg_add<VT_FLIGHT>(z, ldz, d, lrow, lcode, e, n, g, cpg_shift, acc + tid, cur, ca);
      for (; e < n; e += 4) seg_add<4>(z, ldz, d, lrow, lcode, e, n, g, cpg_shift, acc + tid, cur, ca);
      if (cur >= 0) acc[cur * 256 + tid] = ca;
    }
    __syncthreads();   // lrow / lcode / wtot are rewritten by the next round
  }

  if (MODE == 1) {
    const float coef = gl[0] * scale;
    for (int s = 0; s < cpg; ++s) {
      const long long k = k0 + g * cpg + s;
      if (k < K && d < D) {
        const size_t o = (size_t)k * D + d;
        dE[o] = coef * fmaf((float)hist[k], E[o], -(float)acc[s * 256 + tid]);
      }
    }
    return;
  }

  const float nf = (float)nsum[0];
  const float denom = nf + keps;
  for (int s = 0; s < cpg; ++s) {
    const long long k = k0 + g * cpg + s;
    float e = 0.f;
    if (k < K && d < D) {
      const size_t o = (size_t)k * D + d;
      const float S = (float)acc[s * 256 + tid];
      const float w = fmaf(omg, S, gam * W[o]);
      const float cl = ((cs[k] + eps) / denom) * nf;
      e = w / cl;
      W[o] = w;
      E[o] = e;
      if (Eh) {
        const unsigned h = f2bf(e);
        Eh[(size_t)k * Dpad + d] = (bf16r)h;
        El[(size_t)k * Dpad + d] = (bf16r)f2bf(e - bf2f(h));
      }
    }
    acc[s * 256 + tid] = (double)e;   // own slot: the new row, for hn below
  }
  if (!hn) return;
  __syncthreads();
  // hn[k] = 0.5 |e_k|^2, the fmaf chain of vq_prep_hn over d = 0 .. D-1
  for (int t = tid; t < cpw; t += 256) {
    const long long k = k0 + t;
    if (k >= K) break;
    const int col = (t >> cpg_shift) << dt_shift, s = t & (cpg - 1);
    float sum = 0.f;
    for (int dd = 0; dd < D; ++dd) {
      const float e = (float)acc[s * 256 + col + dd];
      sum = fmaf(e, e, sum);
    }
    hn[k] = 0.5f * sum;
  }
}

// The code of row m, clamped into the codebook (a code is never out of range after fmd_vq_finalize; the clamp keeps
// a corrupted one from reading outside the codebook).  Shared by the two latent-gradient kernels below.
FMD_DEV long long vq_code_row(const long long* __restrict__ codes, long long m, int K) {
  const long long k = codes[m];
  return k < 0 ? 0 : (k >= K ? K - 1 : k);
}

// dz = g_zq + coef (z - q) on the first D channels, zero on the rest; coef = (g_loss * c) * scale.  E null: the
// rows of z already hold z - q.
__global__ __launch_bounds__(256) void vq_backward_kernel(const float* __restrict__ z, int ldz, int M, int K, int D,
                                                          const long long* __restrict__ codes,
                                                          const float* __restrict__ E, const float* __restrict__ g,
                                                          int ldg, const float* __restrict__ gl, float c, float scale,
                                                          float* __restrict__ dz, int lddz) {
  const float coef = (gl[0] * c) * scale;
  const long long total = (long long)M * lddz;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long m = i / lddz;
    const int d = (int)(i - m * lddz);
    float o = 0.f;
    if (d < D) {
      float diff = z[(size_t)m * ldz + d];
      if (E) diff = diff - E[(size_t)vq_code_row(codes, m, K) * D + d];
      o = fmaf(coef, diff, g ? g[(size_t)m * ldg + d] : 0.f);
    }
    dz[i] = o;
  }
}

// n <= 8 consecutive floats of a row into v (the rest zero).  vec: the row is 16-byte aligned, so a whole group
// of 8 is two 16-byte loads; a partial group reads its valid channels only, one by one.
FMD_DEV void vq_load8(const float* __restrict__ p, int n, bool vec, float* v) {
  if (vec && n == 8) {
    const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  } else {
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = u < n ? p[u] : 0.f;
  }
}

// The latent join of the VQVAE backward: the arithmetic of vq_backward_kernel, element for element, with g read as
// the 1x1 data gradient left it (bf16 or fp32, channels-last, own row stride) and dz stored as the bf16 operand the
// encoder head's backward reads: rounded once, to nearest even, channels D .. lddz-1 exact zeros.
// A thread owns 8 consecutive channels of a row (one 16-byte store; 16- or 2 x 16-byte loads when the group is
// whole), consecutive lanes consecutive groups, rows grid-strided.  Channels >= D of g, z and E are never read.
template <bool GF32>
__global__ __launch_bounds__(256) void vq_join_bwd_kernel(const float* __restrict__ z, int ldz, int zvec, int M,
                                                          int K, int D, const long long* __restrict__ codes,
                                                          const float* __restrict__ E, int evec,
                                                          const void* __restrict__ g, int ldg,
                                                          const float* __restrict__ gl, float c, float scale,
                                                          bf16r* __restrict__ dz, int lddz) {
  const float coef = ((gl ? gl[0] : 0.f) * c) * scale;
  const int G = lddz >> 3;
  const long long total = (long long)M * G;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long m = i / G;
    const int d0 = (int)(i - m * G) << 3;
    const int n = D - d0 < 8 ? D - d0 : 8;   // <= 0: a group of padding channels only
    u32x4 o = {0u, 0u, 0u, 0u};
    if (n > 0) {
      float diff[8], gv[8];
      vq_load8(z + (size_t)m * ldz + d0, n, zvec, diff);
      if (E) {
        float e[8];
        vq_load8(E + (size_t)vq_code_row(codes, m, K) * D + d0, n, evec, e);
#pragma unroll
        for (int u = 0; u < 8; ++u) diff[u] = diff[u] - e[u];
      }
      if (!g) {
#pragma unroll
        for (int u = 0; u < 8; ++u) gv[u] = 0.f;
      } else if (GF32) {
        vq_load8((const float*)g + (size_t)m * ldg + d0, n, true, gv);
      } else {
        const bf16r* gp = (const bf16r*)g + (size_t)m * ldg + d0;
        if (n == 8) {
          const u32x4 w = *(const u32x4*)gp;
          gv[0] = bf_lo(w.x); gv[1] = bf_hi(w.x); gv[2] = bf_lo(w.y); gv[3] = bf_hi(w.y);
          gv[4] = bf_lo(w.z); gv[5] = bf_hi(w.z); gv[6] = bf_lo(w.w); gv[7] = bf_hi(w.w);
        } else {
#pragma unroll
          for (int u = 0; u < 8; ++u) gv[u] = u < n ? bf2f(gp[u]) : 0.f;
        }
      }
      float r[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) r[u] = u < n ? fmaf(coef, diff[u], gv[u]) : 0.f;
      o.x = pack2(r[0], r[1]);
      o.y = pack2(r[2], r[3]);
      o.z = pack2(r[4], r[5]);
      o.w = pack2(r[6], r[7]);
    }
    *(u32x4*)(dz + (size_t)m * lddz + d0) = o;
  }
}

}  // namespace

extern "C" int fmd_vq_train_plan(int32_t M, int32_t K, int32_t D, int32_t* codes_per_wg, int32_t* grid) {
  seg_plan p;
  if (seg_plan_of(M, K, D, &p)) return -1;
  if (codes_per_wg) *codes_per_wg = p.cpw;
  if (grid) *grid = p.grid;
  return 0;
}

extern "C" int fmd_vq_ema_update(const float* z, int32_t ldz, int32_t M, int32_t K, int32_t D, const int64_t* codes,
                                 const int32_t* hist, float decay, float one_minus_decay, float eps, float k_eps,
                                 float* ema_cluster_size, float* ema_w, float* embedding, void* Eh, void* El,
                                 float* hn, double* nsum, fmd_stream_t s) {
  seg_plan p;
  fmd_vq_plan_t q;
  if (!z || !codes || !hist || !ema_cluster_size || !ema_w || !embedding || !nsum || seg_plan_of(M, K, D, &p) ||
      fmd_vq_plan(M, K, D, &q) || ldz < D || (!Eh != !El) || (!Eh != !hn))
    return -1;
  hipLaunchKernelGGL(vq_ema_sizes_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, hist, K, decay, one_minus_decay,
                     ema_cluster_size, nsum);
  hipLaunchKernelGGL(vq_segsum_kernel<0>, dim3(p.grid), dim3(256), 0, (hipStream_t)s, z, ldz, M, K, D,
                     (const long long*)codes, hist, p.dt_shift, p.cpg_shift, p.cpw, decay, one_minus_decay, eps,
                     k_eps, (const float*)ema_cluster_size, (const double*)nsum, ema_w, embedding, (bf16r*)Eh,
                     (bf16r*)El, hn, q.Dpad, (const float*)nullptr, 0.f, (float*)nullptr);
  return (int)hipGetLastError();
}

extern "C" int fmd_vq_codebook_grad(const float* z, int32_t ldz, int32_t M, int32_t K, int32_t D,
                                    const int64_t* codes, const int32_t* hist, const float* embedding,
                                    const float* g_loss, float scale, float* d_embedding, fmd_stream_t s) {
  seg_plan p;
  if (!z || !codes || !hist || !embedding || !g_loss || !d_embedding || seg_plan_of(M, K, D, &p) || ldz < D) return -1;
  hipLaunchKernelGGL(vq_segsum_kernel<1>, dim3(p.grid), dim3(256), 0, (hipStream_t)s, z, ldz, M, K, D,
                     (const long long*)codes, hist, p.dt_shift, p.cpg_shift, p.cpw, 0.f, 0.f, 0.f, 0.f,
                     (const float*)nullptr, (const double*)nullptr, (float*)nullptr, (float*)embedding,
                     (bf16r*)nullptr, (bf16r*)nullptr, (float*)nullptr, 0, g_loss, scale, d_embedding);
  return (int)hipGetLastError();
}

extern "C" int fmd_vq_backward(const float* z, int32_t ldz, int32_t M, int32_t K, int32_t D, const int64_t* codes,
                               const float* embedding, const float* g_zq, int32_t ldg, const float* g_loss, float c,
                               float scale, float* dz, int32_t lddz, fmd_stream_t s) {
  if (!z || !g_loss || !dz || M < 1 || K < 1 || D < 1 || M > (1 << 30) || ldz < D || lddz < D || (g_zq && ldg < D) ||
      (embedding && !codes))
    return -1;
  const long long total = (long long)M * lddz;
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(vq_backward_kernel, dim3(grid), dim3(256), 0, (hipStream_t)s, z, ldz, M, K, D,
                     (const long long*)codes, embedding, g_zq, ldg, g_loss, c, scale, dz, lddz);
  return (int)hipGetLastError();
}

extern "C" int fmd_vq_join_bwd(const float* z, int32_t ldz, int32_t M, int32_t K, int32_t D, const int64_t* codes,
                               const float* embedding, const void* g_zq, int32_t g_f32, int32_t ldg,
                               const float* g_loss, float c, float scale, void* dz, int32_t lddz, fmd_stream_t s) {
  if (!z || !dz || M < 1 || K < 1 || D < 1 || D > VT_DMAX || M > (1 << 30) || ldz < D || lddz < D || (lddz & 7) ||
      ((uintptr_t)dz & 15) || (g_zq && (ldg < D || (ldg & 7) || ((uintptr_t)g_zq & 15))) || (g_f32 & ~1) ||
      (embedding && !codes))
    return -1;
  const int zvec = !(ldz & 3) && !((uintptr_t)z & 15);
  const int evec = embedding && !(D & 3) && !((uintptr_t)embedding & 15);
  const long long total = (long long)M * (lddz >> 3);
  const int grid = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
  if (g_f32)
    hipLaunchKernelGGL(vq_join_bwd_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)s, z, ldz, zvec, M, K, D,
                       (const long long*)codes, embedding, evec, g_zq, ldg, g_loss, c, scale, (bf16r*)dz, lddz);
  else
    hipLaunchKernelGGL(vq_join_bwd_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)s, z, ldz, zvec, M, K, D,
                       (const long long*)codes, embedding, evec, g_zq, ldg, g_loss, c, scale, (bf16r*)dz, lddz);
  return (int)hipGetLastError();
}
