// Whole backward of the ResBlock's 1x1 skip convolution in one pass over dy and the block input (gfx950).
//
// A persistent workgroup owns CT = 128 input channels (its c-tile) and strides over the 64-pixel tiles of
// M = N*(D*)H*W in a fixed order.  Per tile it
//   1. computes dx = round_bf16(dy . W_s^T) + P*dz + Q*x + R (+ dx), split over the concat sources at C0 -- the
//      arithmetic of fmd_conv_gn_apply (conv_igemm<128, 128, 2, 2, 32, true>, csrc/conv.hip) with the same MFMA,
//      the same k order over Kd and the same rounding, so dx is bit-identical to that launch;
//   2. accumulates dW_s[Kd][c-tile] += dy_tile^T . x_tile in registers: both operands are pixel-major, so the
//      fragments come from the SAME LDS images as (1) through ds_read_b64_tr_b16 (csrc/wgrad.hip's layout, tile128_off:
//      its 8-byte swizzle keeps 16-byte chunks whole, so the row reads of (1) work on it too);
//   3. (c-tile 0 only) accumulates db_s[k] += sum_p dy[p][k].
// At the end each workgroup writes its fp32 partial slab; fmd_wgrad_combine (wgrad_reduce2, T = 1) sums the slabs
// in slab order into weight.grad / bias.grad.  Deterministic: fixed tile-to-workgroup map, no atomics.
//
// The pass is HBM-bound (64 MFMAs per wave against 64-80 KB of traffic per tile): the next tile's dy / x are
// loaded under this tile's MFMAs and stores, the next tile's dz / old dx under the next tile's MFMAs.  W_s^T of
// the c-tile is staged in LDS once per workgroup.
//
// Replaces: autograd of the skip nn.Conv2d (src/nn/blocks/residual.py:77-82,120): weight, bias and data gradient.
#include "common.h"
#include "../../include/fmdiff.h"

namespace {

constexpr int KD = 128, CT = 128, BPX = 64, NT = 256;

struct SArgs {
  fmd_skip_bwd_desc d;
  int M, C, HW;
  int ntp, ntc;   // pixel tiles, c-tiles
  int G;          // pixel groups launched (workgroups per c-tile)
  int nsl;        // slabs: min(G, ntp) -- a group without tiles writes none
  int xcd;        // G % 8 == 0: the c-tiles of a pixel group run on one XCD (dy shared through its L2)
};

__global__ __launch_bounds__(NT, 2) void skip_bwd_kernel(const SArgs A) {
  __shared__ __attribute__((aligned(16))) bf16r ldsW[CT * KD];    // W_s^T[c][k], 16-byte chunk ^ (c & 15)
  __shared__ __attribute__((aligned(16))) bf16r ldsY[BPX * KD];   // dy tile; then the rounded conv term [p][c]
  __shared__ __attribute__((aligned(16))) bf16r ldsX[BPX * CT];   // x tile
  const fmd_skip_bwd_desc& d = A.d;
  const fmd_gn_apply_desc& g = d.g;
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int l16 = lane & 15, lq = lane >> 4;

  const int b = blockIdx.x;
  int ct, grp;
  if (A.xcd) {
    const int k = b >> 3;
    ct = k % A.ntc;
    grp = (k / A.ntc) * 8 + (b & 7);
  } else {
    ct = b % A.ntc;
    grp = b / A.ntc;
  }
  if (grp >= A.ntp) return;   // no tiles: no slab

  const int C = A.C, C0 = g.C0, C1 = C - g.C0;
  const int chunk = tid & 15, rb = tid >> 4;
  const int co = ct * CT + chunk * 8;
  const bool c_ok = co < C;
  const bool first = co < C0;   // C0 % 8 == 0: the 8 channels are in one source
  const int accf = first ? g.acc0 : g.acc1;
  const bool do_bias = d.db && ct == 0;
  const bf16r* __restrict__ dy = (const bf16r*)d.dy;
  const bf16r* __restrict__ xs = first ? (const bf16r*)g.x0 + co : (const bf16r*)g.x1 + (co - C0);
  bf16r* __restrict__ dxs = first ? (bf16r*)g.dx0 + co : (bf16r*)g.dx1 + (co - C0);
  const int ldx = first ? C0 : C1;
  const bf16r* __restrict__ dzs = (const bf16r*)g.dz + co;

  // W_s^T rows of the c-tile, once
  {
    const bf16r* w = (const bf16r*)d.wgt_t;
#pragma unroll
    for (int j = 0; j < CT / 16; ++j) {
      const int r = rb + 16 * j;
      u32x4 v = {0u, 0u, 0u, 0u};
      if (ct * CT + r < C) v = *(const u32x4*)(w + (size_t)(ct * CT + r) * KD + chunk * 8);
      *(u32x4*)(ldsW + r * KD + 8 * (chunk ^ (r & 15))) = v;
    }
  }

  u32x4 ry[4], rx[4], vz[4], old[4];
  const u32x4 zero4 = {0u, 0u, 0u, 0u};
  auto load_yx = [&](int t) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = t * BPX + rb + 16 * j;
      const bool ok = p < A.M;
      ry[j] = ok ? *(const u32x4*)(dy + (size_t)p * KD + chunk * 8) : zero4;
      rx[j] = ok && c_ok ? *(const u32x4*)(xs + (size_t)p * ldx) : zero4;
    }
  };
  auto load_zo = [&](int t) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = t * BPX + rb + 16 * j;
      const bool ok = p < A.M && c_ok;
      vz[j] = ok ? *(const u32x4*)(dzs + (size_t)p * C) : zero4;
      old[j] = ok && accf ? *(const u32x4*)(dxs + (size_t)p * ldx) : zero4;
    }
  };

  f32x4 accw[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) accw[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bacc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) bacc[e] = 0.f;

  // transposed fragment of a [pixel][128] tile: pixels 32 st + 8 lg + {q, 4 + q}, columns col0 + 4 pp
  const int lg = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
  auto frag = [&](const bf16r* t, int st, int col0) -> bf16x8 {
    const s16x4 lo = ds_read_tr16(t + tile128_off(32 * st + 8 * lg + q, col0 / 4 + pp));
    const s16x4 hi = ds_read_tr16(t + tile128_off(32 * st + 8 * lg + 4 + q, col0 / 4 + pp));
    typedef __attribute__((ext_vector_type(8))) short s16x8;
    s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(bf16x8, v);
  };

  load_yx(grp);
  load_zo(grp);
#pragma unroll 1
  for (int t = grp; t < A.ntp; t += A.G) {
    const bool nxt = t + A.G < A.ntp;
    // stage this tile
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = rb + 16 * j;
      *(u32x4*)(ldsY + tile128_off(r, 2 * chunk)) = ry[j];
      *(u32x4*)(ldsX + tile128_off(r, 2 * chunk)) = rx[j];
    }
    if (do_bias) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          bacc[2 * e] += bf_lo(ry[j][e]);
          bacc[2 * e + 1] += bf_hi(ry[j][e]);
        }
    }
    __syncthreads();
    if (nxt) load_yx(t + A.G);

    // (1) conv term: D[c][p] = sum_k W^T[c][k] dy[p][k], k in four 32-wide steps (conv_igemm's K-iterations)
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kk = 0; kk < KD / 32; ++kk) {
      const int kc = 4 * kk + lq;
      bf16x8 af[4], bfr[2];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int r = wm * 64 + 16 * i + l16;
        af[i] = *(const bf16x8*)(ldsW + r * KD + 8 * (kc ^ (r & 15)));
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int r = wn * 32 + 16 * j + l16;
        bfr[j] = *(const bf16x8*)(ldsY + tile128_off(r, 2 * kc));
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = mfma16(af[i], bfr[j], acc[i][j]);
    }

    // (2) dW[k][c] += sum_p dy[p][k] x[p][c]: two 32-pixel steps
#pragma unroll
    for (int st = 0; st < BPX / 32; ++st) {
      bf16x8 af[4], bfr[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = frag(ldsY, st, wm * 64 + 16 * i);
#pragma unroll
      for (int j = 0; j < 4; ++j) bfr[j] = frag(ldsX, st, wn * 64 + 16 * j);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) accw[i][j] = mfma16(af[i], bfr[j], accw[i][j]);
    }
    __syncthreads();   // every wave is done with the dy image

    // the conv term, rounded to bf16, over the dy image: [p][c], 16-byte chunk ^ (p & 15)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int cl = wm * 64 + 16 * i + 4 * lq;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int pi = wn * 32 + 16 * j + l16;
        u32x2 o;
        o[0] = pack2(acc[i][j][0], acc[i][j][1]);
        o[1] = pack2(acc[i][j][2], acc[i][j][3]);
        *(u32x2*)(ldsY + pi * CT + (((cl >> 3) ^ (pi & 15)) * 8) + (cl & 7)) = o;
      }
    }
    __syncthreads();

    // dx = conv + P*dz + Q*x + R (+ dx): the expression of conv_igemm's GNA epilogue, 8 channels of one pixel
    if (c_ok) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int pi = rb + 16 * k;
        const int p = t * BPX + pi;
        if (p >= A.M) continue;
        const int n = p / A.HW;
        const u32x4 ve = *(const u32x4*)(ldsY + pi * CT + ((chunk ^ (pi & 15)) * 8));
        const u32x4 vx = *(const u32x4*)(ldsX + tile128_off(pi, 2 * chunk));
        const float* pq = g.P + (size_t)n * C + co;
        const float* qq = g.Q + (size_t)n * C + co;
        const float* rr = g.R + (size_t)n * C + co;
        const f32x4 P0 = *(const f32x4*)pq, P1 = *(const f32x4*)(pq + 4);
        const f32x4 Q0 = *(const f32x4*)qq, Q1 = *(const f32x4*)(qq + 4);
        const f32x4 R0 = *(const f32x4*)rr, R1 = *(const f32x4*)(rr + 4);
        const float Pv[8] = {P0[0], P0[1], P0[2], P0[3], P1[0], P1[1], P1[2], P1[3]};
        const float Qv[8] = {Q0[0], Q0[1], Q0[2], Q0[3], Q1[0], Q1[1], Q1[2], Q1[3]};
        const float Rv[8] = {R0[0], R0[1], R0[2], R0[3], R1[0], R1[1], R1[2], R1[3]};
        u32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          // conv_igemm's P*dz + Q*x + R + conv compiles to fma(P, dz, Q*x) + R + conv; written out, because here
          // the contraction would pick fma(Q, x, P*dz), one bf16 ulp away on a few elements in 10^5
          float lo = __builtin_fmaf(Pv[2 * e], bf_lo(vz[k][e]), Qv[2 * e] * bf_lo(vx[e])) + Rv[2 * e] + bf_lo(ve[e]);
          float hi = __builtin_fmaf(Pv[2 * e + 1], bf_hi(vz[k][e]), Qv[2 * e + 1] * bf_hi(vx[e])) + Rv[2 * e + 1] +
                     bf_hi(ve[e]);
          if (accf) { lo += bf_lo(old[k][e]); hi += bf_hi(old[k][e]); }
          o[e] = pack2(lo, hi);
        }
        *(u32x4*)(dxs + (size_t)p * ldx) = o;
      }
    }
    if (nxt) load_zo(t + A.G);
    __syncthreads();   // the images are free for the next tile
  }

  // partial slab grp: ws[grp][k][c]; bias rows after the nsl weight slabs
  const size_t per = (size_t)KD * C;
  float* ws = d.ws + (size_t)grp * per;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int ci = ct * CT + wn * 64 + 16 * j + l16;
      if (ci >= C) continue;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = wm * 64 + 16 * i + 4 * lq + r;
        ws[(size_t)k * C + ci] = accw[i][j][r];
      }
    }
  }
  if (do_bias) {
    float* bsum = (float*)ldsY;   // [4 waves][KD], free after the loop's last barrier
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float v = bacc[e];
      v += __shfl_xor(v, 16, 64);
      v += __shfl_xor(v, 32, 64);
      bacc[e] = v;
    }
    if (lane < 16) {
#pragma unroll
      for (int e = 0; e < 8; ++e) bsum[wid * KD + chunk * 8 + e] = bacc[e];
    }
    __syncthreads();
    if (tid < KD) {
      float* wb = d.ws + (size_t)A.nsl * per + (size_t)grp * KD;
      wb[tid] = bsum[tid] + bsum[KD + tid] + bsum[2 * KD + tid] + bsum[3 * KD + tid];
    }
  }
}

// Host arithmetic only.  0 = taken (args filled), 1 = not taken.
int decide(const fmd_skip_bwd_desc* d, SArgs* A, fmd_skip_bwd_plan_t* p) {
  *p = fmd_skip_bwd_plan_t{};
  const int64_t M64 = (int64_t)d->N * d->HW;
  const int C = d->C0 + d->C1;
  // The dW accumulators are Kd x c_tile fp32 per workgroup: Kd = 128 with 128 channels is the instance built
  if (d->Kd != KD || d->N < 1 || d->HW < 1 || (d->C0 % 8) || (d->C1 % 8) || d->C0 < 8) return 1;
  // up to 64 input channels fmd_conv_gn_apply runs its 64-channel instance: dx is held to the 128-channel one's bits
  if (C <= 64) return 1;
  if (M64 > (int64_t)1 << 30) return 1;
  const int M = (int)M64;
  const int ntp = (M + BPX - 1) / BPX, ntc = (C + CT - 1) / CT;
  const int ncu = d->num_cu > 0 ? d->num_cu : 256;
  int G;
  if (d->groups > 0) {
    G = d->groups;
  } else {
    // two resident workgroups per CU; whole multiples of 8 so a pixel group's c-tiles share an XCD
    G = 2 * ncu / ntc;
    if (G < 1) G = 1;
    if (G > ntp) G = ntp;
    if (G >= 8) G -= G % 8;
    // Measured faster than the launches it replaces with 8 to 32 pixel tiles per group (config B's 128^2 and 256^2
    // levels at batch 8).  Below that a workgroup's slab and the combine launch of its own are
    // not paid for by measurement: those blocks keep fmd_conv_gn_apply + the grouped ks = 1 weight gradient
    if ((int64_t)ntp < (int64_t)d->min_tiles * G) return 1;
  }
  if ((int64_t)G * ntc > 65535) return 1;
  const int nsl = G < ntp ? G : ntp;
  p->taken = 1;
  p->c_tile = CT;
  p->workgroups = G * ntc;
  p->slabs = nsl;
  p->ws_floats = (int64_t)nsl * ((int64_t)KD * C + KD);
  if (A) {
    A->d = *d;
    A->M = M;
    A->C = C;
    A->HW = d->HW;
    A->ntp = ntp;
    A->ntc = ntc;
    A->G = G;
    A->nsl = nsl;
    A->xcd = G % 8 == 0;
  }
  return 0;
}

}  // namespace

extern "C" int fmd_skip_bwd_plan(const fmd_skip_bwd_desc* d, fmd_skip_bwd_plan_t* out) {
  return decide(d, nullptr, out);
}

extern "C" int fmd_skip_bwd(const fmd_skip_bwd_desc* d, fmd_stream_t stream) {
  SArgs A;
  fmd_skip_bwd_plan_t p;
  if (decide(d, &A, &p)) return -1;   // the plan refuses: the caller runs fmd_conv_gn_apply + fmd_wgrad
  const fmd_gn_apply_desc& g = d->g;
  if (!d->dy || !d->wgt_t || !d->dw || !d->ws) return -2;
  if (!g.dz || !g.x0 || !g.P || !g.Q || !g.R || !g.dx0 || g.C0 != d->C0) return -7;
  if (d->C1 && (!g.x1 || !g.dx1)) return -7;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(skip_bwd_kernel, dim3(p.workgroups), dim3(NT), 0, s, A);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  // the slabs are those of a 1x1 weight gradient with p.slabs splits: its combine writes dW[k][c] and db[k]
  fmd_wgrad_desc w = {};
  w.N = d->N; w.Hs = w.Ho = d->HW; w.Ws = w.Wo = 1;
  w.C0 = d->C0 + d->C1; w.K = KD;   // the combine sees the concatenated input only as its channel count
  w.ks = 1; w.stride = 1;
  w.dw = d->dw; w.db = d->db; w.accumulate = d->accumulate;
  w.ws = d->ws; w.splits = p.slabs;
  return fmd_wgrad_combine(&w, stream);
}
