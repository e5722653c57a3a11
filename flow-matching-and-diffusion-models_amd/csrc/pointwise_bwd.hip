// Backward of the latent 1x1 conv of AutoencoderKL (post_quant_conv, reference src/models/vae/kl.py:124-128):
// y[m][z] = b[z] + sum_e W[z][e] x[m][e] with E = embed_dim inputs and Z = z_channels outputs, both at most 8.
// One VALU launch (plus the finishing launch of the sums) instead of a padded MFMA data gradient, a padded weight
// gradient and a layout pass, and the latent gradient keeps fp32: it is the g_z of fmd_gauss_backward, where the
// small KL term is added to it.
//
// Arithmetic, which tests/pointwise_bounds.py restates: dy and x are bf16, W is fp32; every product is formed in
// fp64 (a product of two bf16 values is exact there) and every value written is ONE rounding of its fp64 value to
// fp32.  g[m][e] adds its Z terms in ascending z.  dW and db are fp64 sums in a fixed order: a thread adds its
// rows in ascending order, a fixed butterfly adds the 64 lanes, the four wave totals are added in order into one
// partial per workgroup, and the finishing launch adds the partials thread-strided and then by a fixed tree.  No
// atomics; the grid depends on the problem size only.
//
// A thread holds Z * E + Z fp64 sums in registers, which is what limits Z and E to 8 (16 would need more than
// 500 VGPRs).  Memory- and launch-bound work: 256 threads, one row per thread and trip, 16-byte row loads.
#include "common.h"
#include "fmdiff.h"

namespace {

constexpr int PW_ROWS = FMD_POINTWISE_ROWS;   // rows per workgroup: 256 threads x 2 trips
constexpr int PW_MAXC = FMD_POINTWISE_MAXC;
static_assert(PW_ROWS % 256 == 0 && PW_MAXC == 8, "trip count; a row of 8 bf16 is one 16-byte load");

struct PwArgs {
  const bf16r* dy;   // [M][ldy]
  const bf16r* x;    // [M][ldx]
  const float* W;    // [Z][E]
  long long M, P;    // rows, and rows per sample (the channels-first g)
  int ldy, ldx;
  float* g;          // null: not wanted
  int g_cl, ldg;     // g channels-last [M][ldg] (padding zero), else channels-first [M / P][E][P]
  double* part;      // [workgroups][Z * E + Z], null: no dW / db
  int vec;           // bit 0: dy rows, bit 1: x rows, bit 2: channels-last g rows take 16-byte accesses
};

// channels 0 .. C-1 of one bf16 row as fp32; with ``vec`` one 16-byte load (the row has at least 8 channels; those
// past C stay unused), else C two-byte loads
template <int C>
FMD_DEV void load_row(const bf16r* row, bool vec, float (&v)[C]) {
  if (vec) {
    const u32x4 q = *(const u32x4*)row;
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = (c & 1) ? bf_hi(q[c >> 1]) : bf_lo(q[c >> 1]);
  } else {
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = bf2f(row[c]);
  }
}

template <int Z, int E>
__global__ __launch_bounds__(256) void pointwise_bwd_kernel(PwArgs a) {
  constexpr int NS = Z * E + Z;
  __shared__ double red[4][NS];
  const int tid = threadIdx.x;
  double w[Z][E];
#pragma unroll
  for (int z = 0; z < Z; ++z)
#pragma unroll
    for (int e = 0; e < E; ++e) w[z][e] = (double)a.W[z * E + e];
  double sw[Z][E], sb[Z];
#pragma unroll
  for (int z = 0; z < Z; ++z) {
    sb[z] = 0.0;
#pragma unroll
    for (int e = 0; e < E; ++e) sw[z][e] = 0.0;
  }
#pragma unroll 1
  for (int trip = 0; trip < PW_ROWS / 256; ++trip) {
    const long long m = (long long)blockIdx.x * PW_ROWS + trip * 256 + tid;
    if (m >= a.M) break;
    float dv[Z];
    load_row<Z>(a.dy + (size_t)m * a.ldy, a.vec & 1, dv);
    if (a.part) {
      float xv[E];
      load_row<E>(a.x + (size_t)m * a.ldx, a.vec & 2, xv);
#pragma unroll
      for (int z = 0; z < Z; ++z) {
        sb[z] += (double)dv[z];
#pragma unroll
        for (int e = 0; e < E; ++e) sw[z][e] += (double)dv[z] * (double)xv[e];
      }
    }
    if (a.g) {
      float gv[PW_MAXC];
#pragma unroll
      for (int e = 0; e < PW_MAXC; ++e) {
        double s = 0.0;
        if (e < E) {
#pragma unroll
          for (int z = 0; z < Z; ++z) s += (double)dv[z] * w[z][e < E ? e : 0];
        }
        gv[e] = (float)s;
      }
      if (a.g_cl) {
        float* d = a.g + (size_t)m * a.ldg;
        for (int c0 = 0; c0 < a.ldg; c0 += 8) {
          if ((a.vec & 4) && c0 + 8 <= a.ldg) {
            *(f32x4*)(d + c0) = c0 ? f32x4{0.f, 0.f, 0.f, 0.f} : f32x4{gv[0], gv[1], gv[2], gv[3]};
            *(f32x4*)(d + c0 + 4) = c0 ? f32x4{0.f, 0.f, 0.f, 0.f} : f32x4{gv[4], gv[5], gv[6], gv[7]};
          } else {
#pragma unroll
            for (int j = 0; j < 8; ++j)
              if (c0 + j < a.ldg) d[c0 + j] = c0 ? 0.f : gv[j];
          }
        }
      } else {
        const long long n = m / a.P, p = m - n * a.P;
#pragma unroll
        for (int e = 0; e < E; ++e) a.g[((size_t)n * E + e) * (size_t)a.P + (size_t)p] = gv[e];
      }
    }
  }
  if (!a.part) return;
#pragma unroll
  for (int z = 0; z < Z; ++z) {
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const double s = wave_sum_f64(sw[z][e]);
      if ((tid & 63) == 0) red[tid >> 6][z * E + e] = s;
    }
    const double s = wave_sum_f64(sb[z]);
    if ((tid & 63) == 0) red[tid >> 6][Z * E + z] = s;
  }
  __syncthreads();
  if (tid < NS) a.part[(size_t)blockIdx.x * NS + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// Workgroup j: the sum of part[b * NS + j] over the B workgroups of the first launch, thread-strided in ascending
// order, then a fixed tree.  j < ZE goes to dW[j], the rest to db[j - ZE]; stored, or added to the fp32 value there.
__global__ __launch_bounds__(256) void pointwise_final_kernel(const double* __restrict__ part, long long B, int NS,
                                                              int ZE, float* __restrict__ dW, float* __restrict__ db,
                                                              int accumulate) {
  __shared__ double r[256];
  const int tid = threadIdx.x, j = blockIdx.x;
  double s = 0.0;
  for (long long b = tid; b < B; b += 256) s += part[(size_t)b * NS + j];
  r[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) r[tid] += r[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    float* dst = j < ZE ? (dW ? dW + j : nullptr) : (db ? db + (j - ZE) : nullptr);
    if (dst) *dst = accumulate ? *dst + (float)r[0] : (float)r[0];
  }
}

constexpr long long LIM = (1ll << 31) - 1;

bool aligned16(const void* p) { return ((unsigned long long)p & 15) == 0; }

// workgroups of the first launch, or -1
long long pw_blocks(long long M, int Z, int E) {
  if (M < 1 || M > (1ll << 40) || Z < 1 || E < 1 || Z > PW_MAXC || E > PW_MAXC) return -1;
  const long long b = (M + PW_ROWS - 1) / PW_ROWS;
  return b > LIM ? -1 : b;
}

template <int Z, int E>
void launch_ze(const PwArgs& a, long long blocks, hipStream_t s) {
  hipLaunchKernelGGL((pointwise_bwd_kernel<Z, E>), dim3((unsigned)blocks), dim3(256), 0, s, a);
}

template <int Z>
void launch_z(int E, const PwArgs& a, long long blocks, hipStream_t s) {
  switch (E) {
    case 1: launch_ze<Z, 1>(a, blocks, s); break;
    case 2: launch_ze<Z, 2>(a, blocks, s); break;
    case 3: launch_ze<Z, 3>(a, blocks, s); break;
    case 4: launch_ze<Z, 4>(a, blocks, s); break;
    case 5: launch_ze<Z, 5>(a, blocks, s); break;
    case 6: launch_ze<Z, 6>(a, blocks, s); break;
    case 7: launch_ze<Z, 7>(a, blocks, s); break;
    default: launch_ze<Z, 8>(a, blocks, s); break;
  }
}

}  // namespace

extern "C" int64_t fmd_pointwise_bwd_workspace(int64_t M, int32_t Z, int32_t E) {
  const long long b = pw_blocks(M, Z, E);
  return b < 0 ? -1 : b * (long long)(Z * E + Z) * 8;
}

extern "C" int fmd_pointwise_bwd(const void* dy, int32_t ldy, const void* x, int32_t ldx, const float* W, int32_t N,
                                 int64_t P, int32_t Z, int32_t E, float* g, int32_t g_channels_last, int32_t ldg,
                                 float* dW, float* db, int32_t accumulate, void* ws, fmd_stream_t s) {
  if (N < 1 || P < 1 || P > (1ll << 40)) return -1;
  const long long M = (long long)N * P;
  const long long blocks = pw_blocks(M, Z, E);
  const bool sums = dW || db;
  if (blocks < 0 || !dy || ldy < Z || !W || (!g && !sums) || (sums && (!x || ldx < E || !ws)) ||
      (g && g_channels_last && ldg < E))
    return -1;
  PwArgs a;
  a.dy = (const bf16r*)dy, a.x = (const bf16r*)x, a.W = W;
  a.M = M, a.P = P, a.ldy = ldy, a.ldx = ldx;
  a.g = g, a.g_cl = g_channels_last != 0, a.ldg = ldg;
  a.part = sums ? (double*)ws : nullptr;
  a.vec = ((ldy % 8 == 0 && aligned16(dy)) ? 1 : 0) | ((sums && ldx % 8 == 0 && aligned16(x)) ? 2 : 0) |
          ((g && a.g_cl && ldg % 8 == 0 && aligned16(g)) ? 4 : 0);
  hipStream_t st = (hipStream_t)s;
  switch (Z) {
    case 1: launch_z<1>(E, a, blocks, st); break;
    case 2: launch_z<2>(E, a, blocks, st); break;
    case 3: launch_z<3>(E, a, blocks, st); break;
    case 4: launch_z<4>(E, a, blocks, st); break;
    case 5: launch_z<5>(E, a, blocks, st); break;
    case 6: launch_z<6>(E, a, blocks, st); break;
    case 7: launch_z<7>(E, a, blocks, st); break;
    default: launch_z<8>(E, a, blocks, st); break;
  }
  int rc = (int)hipGetLastError();
  if (rc || !sums) return rc;
  hipLaunchKernelGGL(pointwise_final_kernel, dim3(Z * E + Z), dim3(256), 0, st, (const double*)ws, blocks,
                     Z * E + Z, Z * E, dW, db, accumulate);
  return (int)hipGetLastError();
}
