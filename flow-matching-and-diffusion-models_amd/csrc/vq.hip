// Vector-quantizer forward for the VQ-VAE codebooks (reference src/nn/modules/vae/codebook.py:67-84, :109-137):
// nearest code per latent vector on MFMA without the M x K distance matrix, then gather, straight-through
// output, commitment loss, code histogram and perplexity.
//
// The nearest code of z maximises s(k) = z.e_k - 0.5 |e_k|^2 (the |z|^2 term of codebook.py:70-72 is constant
// per row).  One bf16 plane per operand picks a wrong code on about 1 % of rows, so both operands are split
// into two bf16 planes, x = x_h + x_l, and the product is z_h.e_h + z_h.e_l + z_l.e_h accumulated in fp32 on
// v_mfma_f32_32x32x16_bf16 (z_l.e_l, about 2^-16 of the product, is dropped); 0.5 |e_k|^2 is fp32 from the
// fp32 master.  DESIGN.md section 4 derives the error bound the tests hold the result to.
//
// Orientation as in attn_mfma_fwd (S^T = K Q^T): codes are the MFMA's A rows and latent vectors its B
// columns, so the accumulator column (lane & 31) is one latent vector and a lane's 16 registers are 16 codes
// in ascending order: the running (best score, index) is per lane, no cross-lane traffic inside the loop.
#include "common.h"
#include "fmdiff.h"

#include <math.h>

namespace {

constexpr int VQ_BM = 64;          // latent vectors per workgroup: two 32-column MFMA tiles
constexpr int VQ_TILE = 32;        // codes per wave tile (one 32x32 accumulator per column tile)
constexpr int VQ_CHUNK = 128;      // codes per workgroup round: 4 waves x VQ_TILE
constexpr int VQ_KC = 64;          // reduction elements per super-step: 4 MFMA k-steps, one 128-B line per code
constexpr int VQ_DMAX = 256;
constexpr int VQ_TARGET_WG = 512;  // two workgroups per CU
constexpr int VQ_MAX_SPLITS = 64;
constexpr int VQ_FROWS = 32;       // latent vectors per finalize workgroup

FMD_DEV bf16x8 ld8(const bf16r* p) { return __builtin_bit_cast(bf16x8, *(const u32x4*)p); }

// (score, index) merge: the greater score wins, the lower index on equal scores (torch.argmin's first minimum)
FMD_DEV void merge_best(float& s, int& i, float os, int oi) {
  if (os > s || (os == s && oi < i)) {
    s = os;
    i = oi;
  }
}

int plan_of(long long M, long long K, long long D, fmd_vq_plan_t* p) {
  if (M < 1 || K < 1 || D < 1 || D > VQ_DMAX || M > (1ll << 30) || K > (1ll << 30)) return -1;
  const int nch = (int)((K + VQ_CHUNK - 1) / VQ_CHUNK);
  const int rb = (int)((M + VQ_BM - 1) / VQ_BM);
  int want = (VQ_TARGET_WG + rb - 1) / rb;
  if (want > VQ_MAX_SPLITS) want = VQ_MAX_SPLITS;
  if (want > nch) want = nch;
  const int cps = (nch + want - 1) / want;   // chunks per split; no split is empty
  p->splits = (nch + cps - 1) / cps;
  p->block_rows = VQ_BM;
  p->tile_codes = VQ_TILE;
  p->codes_per_split = cps * VQ_CHUNK;
  p->Kpad = nch * VQ_CHUNK;
  p->Dpad = (int)((D + VQ_KC - 1) / VQ_KC) * VQ_KC;
  p->finalize_rows = VQ_FROWS;
  return 0;
}

// fp32 codebook [K][D] -> bf16 planes [Kpad][Dpad] (zero padded): e = e_h + e_l up to 2^-17 |e|
__global__ __launch_bounds__(256) void vq_prep_planes(const float* __restrict__ E, int K, int D, int Kpad, int Dpad,
                                                      bf16r* __restrict__ Eh, bf16r* __restrict__ El) {
  const long long total = (long long)Kpad * Dpad;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int k = (int)(i / Dpad), d = (int)(i % Dpad);
    const float v = (k < K && d < D) ? E[(size_t)k * D + d] : 0.f;
    const unsigned h = f2bf(v);
    Eh[i] = (bf16r)h;
    El[i] = (bf16r)f2bf(v - bf2f(h));
  }
}

// hn[k] = 0.5 |e_k|^2, summed d = 0 .. D-1 by one thread; padded codes +inf (their score is -inf: never chosen)
__global__ __launch_bounds__(256) void vq_prep_hn(const float* __restrict__ E, int K, int D, int Kpad,
                                                  float* __restrict__ hn) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= Kpad) return;
  if (k >= K) {
    hn[k] = INFINITY;
    return;
  }
  float s = 0.f;
  for (int d = 0; d < D; ++d) {
    const float e = E[(size_t)k * D + d];
    s = fmaf(e, e, s);
  }
  hn[k] = 0.5f * s;
}

// One workgroup: VQ_BM latent vectors against the codes of one split.  z rows are staged once (both planes) in
// LDS; every wave streams its own 32-code tiles straight from global memory (a code tile is used by one wave
// only, so LDS staging would add a round trip and share nothing).  Within a 64-element super-step lane
// (r, h) = (lane & 31, lane >> 5) owns elements 64 s + 32 h + 8 j + (0..7) in MFMA k-step j of BOTH operands:
// the MFMA sums over its k slots whatever element they hold, so this permutation of the reduction index is
// free, and each code row is read as one whole 128-byte line per super-step.
template <int NKS>
__global__ __launch_bounds__(256, 2) void vq_argmin_kernel(const float* __restrict__ z, int ldz, int M, int D,
                                                           const bf16r* __restrict__ Eh,
                                                           const bf16r* __restrict__ El,
                                                           const float* __restrict__ hn, int S, int cps, int nch,
                                                           float* __restrict__ best, int* __restrict__ bidx) {
  constexpr int DP = NKS * VQ_KC;
  constexpr int LDS_LD = DP + 8;   // 16 bytes of row padding: consecutive rows start one 16-B slot apart
  __shared__ __attribute__((aligned(16))) bf16r zs[2 * VQ_BM * LDS_LD];   // [plane][row][LDS_LD]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int split = blockIdx.x % S, rb = blockIdx.x / S;
  const long long row0 = (long long)rb * VQ_BM;

  for (int e = tid; e < VQ_BM * DP; e += 256) {
    const int r = e / DP, d = e % DP;
    const long long m = row0 + r;
    const float v = (m < M && d < D) ? z[(size_t)m * ldz + d] : 0.f;
    const unsigned h = f2bf(v);
    zs[r * LDS_LD + d] = (bf16r)h;
    zs[VQ_BM * LDS_LD + r * LDS_LD + d] = (bf16r)f2bf(v - bf2f(h));
  }
  __syncthreads();

  const int c = lane & 31, hh = lane >> 5;
  float bs0 = -INFINITY, bs1 = -INFINITY;
  int bi0 = 0, bi1 = 0;
  const int ch0 = split * cps;
  const int ch1 = ch0 + cps < nch ? ch0 + cps : nch;
  const bf16r* zrow = zs + c * LDS_LD + 32 * hh;
  // code fragments of the next super-step are loaded before the MFMAs of this one (one step of lookahead)
  bf16x8 ah[4], al[4], nh[4], nl[4];
  const size_t lane_off = (size_t)c * DP + 32 * hh;
  if (ch0 < ch1) {
    const size_t o = (size_t)(ch0 * VQ_CHUNK + wave * VQ_TILE) * DP + lane_off;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ah[j] = ld8(Eh + o + 8 * j);
      al[j] = ld8(El + o + 8 * j);
    }
  }
  for (int ch = ch0; ch < ch1; ++ch) {
    const int code0 = ch * VQ_CHUNK + wave * VQ_TILE;   // < Kpad = nch * VQ_CHUNK
    f32x16 acc0 = {0.f}, acc1 = {0.f};
#pragma unroll 1
    for (int s = 0; s < NKS; ++s) {
      const int ns = s + 1 < NKS ? s + 1 : 0, nc = s + 1 < NKS ? ch : ch + 1;
      if (nc < ch1) {
        const size_t o = (size_t)(nc * VQ_CHUNK + wave * VQ_TILE) * DP + lane_off + VQ_KC * ns;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          nh[j] = ld8(Eh + o + 8 * j);
          nl[j] = ld8(El + o + 8 * j);
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = VQ_KC * s + 8 * j;
        const bf16x8 zh0 = ld8(zrow + k), zl0 = ld8(zrow + VQ_BM * LDS_LD + k);
        const bf16x8 zh1 = ld8(zrow + 32 * LDS_LD + k), zl1 = ld8(zrow + (VQ_BM + 32) * LDS_LD + k);
        acc0 = mfma32(al[j], zh0, acc0);
        acc1 = mfma32(al[j], zh1, acc1);
        acc0 = mfma32(ah[j], zl0, acc0);
        acc1 = mfma32(ah[j], zl1, acc1);
        acc0 = mfma32(ah[j], zh0, acc0);
        acc1 = mfma32(ah[j], zh1, acc1);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        ah[j] = nh[j];
        al[j] = nl[j];
      }
    }
    // accumulator register 4 g + q of lane half hh is code 8 g + 4 hh + q of the tile: ascending in the register
    // index, and a strict > keeps the lowest index among equal scores
    const float* hp = hn + code0 + 4 * hh;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const f32x4 h4 = *(const f32x4*)(hp + 8 * g);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int code = code0 + 8 * g + 4 * hh + q;
        const float s0 = acc0[4 * g + q] - h4[q], s1 = acc1[4 * g + q] - h4[q];
        if (s0 > bs0) {
          bs0 = s0;
          bi0 = code;
        }
        if (s1 > bs1) {
          bs1 = s1;
          bi1 = code;
        }
      }
    }
  }
  // the two lane halves hold disjoint codes of the same latent vectors
  merge_best(bs0, bi0, __shfl_xor(bs0, 32, 64), __shfl_xor(bi0, 32, 64));
  merge_best(bs1, bi1, __shfl_xor(bs1, 32, 64), __shfl_xor(bi1, 32, 64));
  __syncthreads();   // every wave is done reading zs: reuse it for the cross-wave merge
  float* rs = (float*)zs;          // [wave][VQ_BM]
  int* ri = (int*)zs + 4 * VQ_BM;  // [wave][VQ_BM]
  if (hh == 0) {
    rs[wave * VQ_BM + c] = bs0;
    ri[wave * VQ_BM + c] = bi0;
    rs[wave * VQ_BM + 32 + c] = bs1;
    ri[wave * VQ_BM + 32 + c] = bi1;
  }
  __syncthreads();
  if (tid < VQ_BM && row0 + tid < M) {
    float s = rs[tid];
    int i = ri[tid];
#pragma unroll
    for (int w = 1; w < 4; ++w) merge_best(s, i, rs[w * VQ_BM + tid], ri[w * VQ_BM + tid]);
    best[(size_t)split * M + row0 + tid] = s;
    bidx[(size_t)split * M + row0 + tid] = i;
  }
}

// Per latent vector: merge the splits (ascending, strict >: the lowest index wins), write the code, count it,
// gather q from the fp32 master and write z_q = z + (q - z) with every operation rounded on its own, which is
// the reference's straight-through expression (codebook.py:41) bit for bit.
__global__ __launch_bounds__(256) void vq_finalize_kernel(const float* __restrict__ z, int ldz, int M, int HW, int K,
                                                          int D, const float* __restrict__ E,
                                                          const float* __restrict__ best,
                                                          const int* __restrict__ bidx, int S,
                                                          long long* __restrict__ codes, float* __restrict__ zq,
                                                          bf16r* __restrict__ zq_nhwc, int Cpad,
                                                          float* __restrict__ slab, int* __restrict__ hist) {
  __shared__ int sidx[VQ_FROWS];
  __shared__ float red[4];
  const int tid = threadIdx.x;
  const long long row0 = (long long)blockIdx.x * VQ_FROWS;
  if (tid < VQ_FROWS) {
    const long long m = row0 + tid;
    int i = 0;
    if (m < M) {
      float b = best[m];
      i = bidx[m];
      for (int s = 1; s < S; ++s) {
        const float o = best[(size_t)s * M + m];
        if (o > b) {
          b = o;
          i = bidx[(size_t)s * M + m];
        }
      }
      i = i < 0 ? 0 : (i >= K ? K - 1 : i);
      codes[m] = i;
      atomicAdd(&hist[i], 1);
    }
    sidx[tid] = i;
  }
  __syncthreads();
  float sum = 0.f;
  if (zq_nhwc) {
    for (int e = tid; e < VQ_FROWS * Cpad; e += 256) {
      const int r = e / Cpad, d = e % Cpad;
      const long long m = row0 + r;
      if (m >= M) break;
      float o = 0.f;
      if (d < D) {
#pragma clang fp contract(off)
        const float zv = z[(size_t)m * ldz + d];
        const float dq = E[(size_t)sidx[r] * D + d] - zv;
        o = zv + dq;
      }
      zq_nhwc[(size_t)m * Cpad + d] = (bf16r)f2bf(o);
    }
  }
  // channels-first store: consecutive threads take consecutive latent vectors of one channel
  for (int e = tid; e < VQ_FROWS * D; e += 256) {
#pragma clang fp contract(off)
    const int d = e / VQ_FROWS, r = e % VQ_FROWS;
    const long long m = row0 + r;
    if (m >= M) continue;
    const float zv = z[(size_t)m * ldz + d];
    const float dq = E[(size_t)sidx[r] * D + d] - zv;
    const float sq = dq * dq;
    sum = sum + sq;
    zq[((size_t)(m / HW) * D + d) * HW + m % HW] = zv + dq;
  }
  sum = wave_sum(sum);
  if ((tid & 63) == 0) red[tid >> 6] = sum;
  __syncthreads();
  if (tid == 0) slab[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// out[0] = vq_loss, out[1] = perplexity, out[2] = mse.  One workgroup, fp64 sums in a fixed order.
__global__ __launch_bounds__(256) void vq_stats_kernel(const float* __restrict__ slab, int nslab,
                                                       const int* __restrict__ hist, int K, int M, int D, float beta,
                                                       int classic, float eps, float* __restrict__ out) {
  __shared__ double r1[256], r2[256];
  const int tid = threadIdx.x;
  double s = 0.0, h = 0.0;
  for (int i = tid; i < nslab; i += 256) s += (double)slab[i];
  for (int k = tid; k < K; k += 256) {
    const double p = (double)hist[k] / (double)M;
    h += p * log(p + (double)eps);
  }
  r1[tid] = s;
  r2[tid] = h;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      r1[tid] += r1[tid + o];
      r2[tid] += r2[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double mse = r1[0] / ((double)M * (double)D);
    out[0] = (float)((classic ? 1.0 + (double)beta : (double)beta) * mse);
    out[1] = (float)exp(-r2[0]);
    out[2] = (float)mse;
  }
}

template <int NKS>
int launch_argmin(const fmd_vq_plan_t& p, const float* z, int ldz, int M, int K, int D, const void* Eh,
                  const void* El, const float* hn, void* ws, hipStream_t s) {
  const int nch = p.Kpad / VQ_CHUNK, cps = p.codes_per_split / VQ_CHUNK;
  const int rb = (M + VQ_BM - 1) / VQ_BM;
  float* best = (float*)ws;
  int* bidx = (int*)ws + (size_t)p.splits * M;
  hipLaunchKernelGGL((vq_argmin_kernel<NKS>), dim3(rb * p.splits), dim3(256), 0, s, z, ldz, M, D,
                     (const bf16r*)Eh, (const bf16r*)El, hn, p.splits, cps, nch, best, bidx);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int fmd_vq_plan(int32_t M, int32_t K, int32_t D, fmd_vq_plan_t* out) {
  if (!out) return -1;
  return plan_of(M, K, D, out);
}

extern "C" int64_t fmd_vq_workspace(int32_t M, int32_t K, int32_t D) {
  fmd_vq_plan_t p;
  if (plan_of(M, K, D, &p)) return -1;
  return (int64_t)p.splits * M * 8;   // best fp32 [S][M], then index int32 [S][M]
}

extern "C" int fmd_vq_prep(const float* E, int32_t K, int32_t D, void* Eh, void* El, float* hn, fmd_stream_t s) {
  fmd_vq_plan_t p;
  if (!E || !Eh || !El || !hn || plan_of(1, K, D, &p)) return -1;
  const long long total = (long long)p.Kpad * p.Dpad;
  const int grid = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  hipLaunchKernelGGL(vq_prep_planes, dim3(grid), dim3(256), 0, (hipStream_t)s, E, K, D, p.Kpad, p.Dpad, (bf16r*)Eh,
                     (bf16r*)El);
  hipLaunchKernelGGL(vq_prep_hn, dim3((p.Kpad + 255) / 256), dim3(256), 0, (hipStream_t)s, E, K, D, p.Kpad, hn);
  return (int)hipGetLastError();
}

extern "C" int fmd_vq_argmin(const float* z, int32_t ldz, int32_t M, int32_t K, int32_t D, const void* Eh,
                             const void* El, const float* hn, void* ws, fmd_stream_t s) {
  fmd_vq_plan_t p;
  if (!z || !Eh || !El || !hn || !ws || plan_of(M, K, D, &p) || ldz < D) return -1;
  switch (p.Dpad / VQ_KC) {
    case 1: return launch_argmin<1>(p, z, ldz, M, K, D, Eh, El, hn, ws, (hipStream_t)s);
    case 2: return launch_argmin<2>(p, z, ldz, M, K, D, Eh, El, hn, ws, (hipStream_t)s);
    case 3: return launch_argmin<3>(p, z, ldz, M, K, D, Eh, El, hn, ws, (hipStream_t)s);
    case 4: return launch_argmin<4>(p, z, ldz, M, K, D, Eh, El, hn, ws, (hipStream_t)s);
  }
  return -1;
}

extern "C" int fmd_vq_finalize(const float* z, int32_t ldz, int32_t M, int32_t HW, int32_t K, int32_t D,
                               const float* E, const void* ws, int64_t* codes, float* zq, void* zq_nhwc,
                               int32_t Cpad, float* slab, int32_t* hist, fmd_stream_t s) {
  fmd_vq_plan_t p;
  if (!z || !E || !ws || !codes || !zq || !slab || !hist || plan_of(M, K, D, &p) || ldz < D || HW < 1 || M % HW ||
      (zq_nhwc && Cpad < D))
    return -1;
  const float* best = (const float*)ws;
  const int* bidx = (const int*)ws + (size_t)p.splits * M;
  hipLaunchKernelGGL(vq_finalize_kernel, dim3((M + VQ_FROWS - 1) / VQ_FROWS), dim3(256), 0, (hipStream_t)s, z, ldz, M,
                     HW, K, D, E, best, bidx, p.splits, (long long*)codes, zq, (bf16r*)zq_nhwc, Cpad, slab, hist);
  return (int)hipGetLastError();
}

extern "C" int fmd_vq_stats(const float* slab, int32_t nslab, const int32_t* hist, int32_t K, int32_t M, int32_t D,
                            float beta, int32_t classic, float eps, float* out, fmd_stream_t s) {
  if (!slab || !hist || !out || nslab < 1 || K < 1 || M < 1 || D < 1) return -1;
  hipLaunchKernelGGL(vq_stats_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, slab, nslab, hist, K, M, D, beta,
                     classic, eps, out);
  return (int)hipGetLastError();
}
