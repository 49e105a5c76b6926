// Row-tile SeqLSTMCore forward and BPTT for several networks in one launch
// (gfx950, H = 64, fp32): the recurrent launches of the two fused SAC steps
// under "rows_kernel": "tile". seq_lstm_fwd_tile_multi and
// seq_lstm_bwd_tile_multi take exactly the device pointer tables of the row
// multi kernels (seq_lstm.hip), so a step builds one set of tables for both:
//   forward   core_tab [C][10] body_w, body_b, w_ih, w_hh, b_g, heads_w,
//                              heads_b, body2_w, body2_b, x2
//             out_tab  [C][4]  outs, hS, cS, stash
//   backward  in_tab   [C][7]  gouts, stash, w_ih, w_hh, heads_w, body_w,
//                              body2_w
//             out_tab  [C][3]  dgates, dxb, dx2
// Grid: blockIdx.x = tile of 16 batch rows, blockIdx.y = network. x, h0 and
// c0 are kernel arguments shared by all networks; every table entry is cast
// to the global address space where it is read, so no access goes through a
// flat instruction. The tensors and the stash field order are those of
// core_rows.h: the loss kernels, both multi weight-gradient kernels and the
// optimizers run on the results unchanged.
//
// The recurrence is the design of seq_lstm_tile.hip (read its header for the
// fragment layout, the K permutation and the bank argument): a wave owns 16
// hidden units of all four gates, 128 resident weight fragments per lane, one
// ds_read_b128 per four K-steps, row stride 132 (backward: 260) floats, the A
// tile double buffered by step parity with one barrier per step, c / dh / dc
// in registers, nothing in LDS sized by S, ragged tiles clamped, zero-filled
// and storing nothing. This file keeps its own copy of those step bodies:
// seq_lstm_tile.hip is not touched, so its two kernels keep their compiler
// figures (profiles/sac_tile.md).
//
// New here:
//
// Dual body in the forward (kDual; the continuous critics). Columns
//   [0, half) of xb are relu(x · body_w + body_b), columns [half, H) are
//   relu(x2 · body2_w + body2_b) with x2 per network (table slot 9). Both
//   weight blocks and the joined bias [body_b | body2_b] sit in LDS, and x2
//   has its own two-step ring next to x's, refilled by the same rule (global
//   load issued before the MFMA block, parked behind it). The thread that
//   owns column bk picks ring, weight column, weight stride and input count
//   once, before the loop; its sum is then the row kernel's chain (bias
//   first, inputs ascending), so xb and with it every ReLU mask of the
//   backward is bit-identical to the row path. A table row whose x2 is 0 is a
//   single-body core, as in the row kernel. The single-body instantiation
//   holds neither the second ring nor the selects.
//
// dx2 in the backward (kDx2): dx2[row][t][f] = Σ_j dxb[row][t][half + j] ·
//   body2_w[f][j] on the ReLU-masked dxb, the action gradient of a
//   continuous critic. Those columns leave the MFMA spread over waves (wave w
//   owns columns 16w .. 16w+15). The waves at or above half park their masked
//   values in a small LDS buffer [2][16][H − half + 4], double buffered by
//   step parity, and step t's dx2 is reduced ONE STEP LATE, behind the
//   barrier that step t − 1 takes anyway: four lanes per output, a quarter of
//   the columns each, two lane exchanges (the pattern of the forward's
//   heads). The step keeps its single barrier; the last step is flushed
//   behind one more barrier after the loop. With accum_dx2 the result is
//   atomicAdd-ed into a buffer the caller zeroed (the twin critics sum into
//   dact), otherwise stored. Each network's value is a fixed-order sum, and
//   fp32 addition commutes, so the accumulated result is bit-reproducible
//   for TWO accumulating networks (0 + a + b = 0 + b + a) and NOT for more
//   (three terms associate in arrival order). dx2 == 0 in the table skips all
//   of it. dx, dh0 and dc0 stay skipped, as in seq_lstm_bwd_multi_kernel: the
//   inputs of these networks are leaves.
#include "common.h"
#include "core_rows.h"
#include "wgrad_body.h"

#include <algorithm>

// One scalar fmaf chain per sum, in a stated order (see wgrad_split.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

// Outputs reached through a device pointer table: global stores.
using gst_f32 = __attribute__((address_space(1))) float*;

constexpr int kTmRows = 16;           // batch rows per workgroup
constexpr int kTmH = 64;              // hidden size
constexpr int kTmG = 4 * kTmH;        // gate columns
constexpr int kTmThreads = 256;       // 4 waves
constexpr int kTmFwdLd = 2 * kTmH + 4;  // LDS row stride of [xb | h], floats
constexpr int kTmBwdLd = kTmG + 4;      // LDS row stride of dgates, floats
constexpr long kTmMaxLds = 64 * 1024;   // dynamic LDS of one launch
constexpr int kFwdTabCols = 10, kFwdOutCols = 4;
constexpr int kBwdTabCols = 7, kBwdOutCols = 3;

// Single body: F2 = 0 and half = H.
__host__ __device__ constexpr long fwd_tile_multi_lds_floats(int F, int D,
                                                             int F2, int half) {
  return 2L * kTmRows * kTmFwdLd + (long)F * half +
         (long)F2 * (kTmH - half) + kTmH + (long)kTmH * D + D +
         2L * kTmRows * F + 2L * kTmRows * F2;
}
// F2 = 0: no dx2, no parking buffer.
__host__ __device__ constexpr long bwd_tile_multi_lds_floats(int D, int F2,
                                                             int half) {
  return 2L * kTmRows * kTmBwdLd + (long)kTmH * D + 2L * kTmRows * D +
         (F2 > 0 ? 2L * kTmRows * (kTmH - half + 4) + (long)F2 * (kTmH - half)
                 : 0L);
}

// Element e of step t's (16, W) slice of a (B, S, W) tensor; zero past B.
template <class P>
__device__ __forceinline__ float tm_slice_load(P src, int e, int t, int row0,
                                               int B, int S, int W) {
  const int row = row0 + e / W;
  const long rowc = min(row, B - 1);
  const float v = src[(rowc * S + t) * W + e % W];
  return row < B ? v : 0.0f;
}

template <bool kDual>
__global__ __launch_bounds__(kTmThreads) void seq_lstm_fwd_tile_multi_kernel(
    const float* __restrict__ x,        // (B,S,F), all networks
    const float* __restrict__ h0,       // (B,H) rows, stride h0s
    const float* __restrict__ c0,       // (B,H) rows, stride h0s
    const long* __restrict__ core_tab,  // [C][10]
    const long* __restrict__ out_tab,   // [C][4]
    int B, int S, int F, int D, long h0s, int F2_arg, int half_arg) {
  constexpr int H = kTmH, G = kTmG, LD = kTmFwdLd;
  const long* ct = core_tab + (long)blockIdx.y * kFwdTabCols;
  const long* ot = out_tab + (long)blockIdx.y * kFwdOutCols;
  const gptr_f32 body_w = (gptr_f32)ct[0];   // (F,half)
  const gptr_f32 body_b = (gptr_f32)ct[1];   // (half)
  const gptr_f32 w_ih = (gptr_f32)ct[2];     // (H,4H)
  const gptr_f32 w_hh = (gptr_f32)ct[3];     // (H,4H)
  const gptr_f32 b_g = (gptr_f32)ct[4];      // (4H)
  const gptr_f32 heads_w = (gptr_f32)ct[5];  // (H,D)
  const gptr_f32 heads_b = (gptr_f32)ct[6];  // (D)
  const gptr_f32 body2_w = (gptr_f32)ct[7];  // (F2,H-half)
  const gptr_f32 body2_b = (gptr_f32)ct[8];  // (H-half)
  const gptr_f32 x2 = (gptr_f32)ct[9];       // (B,S,F2), this network's
  const gst_f32 outs = (gst_f32)ot[0];       // (B,S,D)
  const gst_f32 hS = (gst_f32)ot[1];         // (B,H)
  const gst_f32 cS = (gst_f32)ot[2];         // (B,H)
  const gst_f32 stash = (gst_f32)ot[3];      // (B,S,7H)
  // a row without x2 is a single-body core (the row kernel's rule)
  const bool dual = kDual && ct[9] != 0;
  const int half = dual ? half_arg : H;
  const int F2 = dual ? F2_arg : 0;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* a_s = reinterpret_cast<float*>(smem_raw);  // [2][16][LD] xb | h
  float* bw_s = a_s + 2 * kTmRows * LD;             // (F,half)
  float* b2w_s = bw_s + F * half;                   // (F2,H-half)
  float* bb_s = b2w_s + F2 * (H - half);            // (H) body_b | body2_b
  float* hw_s = bb_s + H;                           // (H,D)
  float* hb_s = hw_s + H * D;                       // (D)
  float* x_s = hb_s + D;                            // [2][16][F] ring
  float* x2_s = x_s + 2 * kTmRows * F;              // [2][16][F2] ring

  const int tid = threadIdx.x;
  const int w = tid / kWave, lane = tid % kWave;
  const int i = lane & 15, kq = lane >> 4;
  const int u = 16 * w + i;  // this lane's hidden unit (accumulator column)
  const int row0 = blockIdx.x * kTmRows;
  const int nx = kTmRows * F, nx2 = kTmRows * F2;

  // B fragments: bf[g][4q+m] = [w_ih ; w_hh][16q + 4kq + m][g·H + u].
  float bf[4][32];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const gptr_f32 src = (q < 4) ? w_ih : w_hh;  // K = 64 .. 127 is w_hh
#pragma unroll
      for (int m = 0; m < 4; ++m)
        bf[g][4 * q + m] = src[(16 * (q & 3) + 4 * kq + m) * G + g * H + u];
    }
  }
  float bias[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) bias[g] = b_g[g * H + u];

  // The small weights, the inputs of the first two steps, h0 into buffer 0.
  for (int e = tid; e < F * half; e += kTmThreads) bw_s[e] = body_w[e];
  for (int e = tid; e < H * D; e += kTmThreads) hw_s[e] = heads_w[e];
  for (int e = tid; e < D; e += kTmThreads) hb_s[e] = heads_b[e];
  for (int e = tid; e < nx; e += kTmThreads) {
    x_s[e] = tm_slice_load(x, e, 0, row0, B, S, F);
    if (S > 1) x_s[nx + e] = tm_slice_load(x, e, 1, row0, B, S, F);
  }
  if constexpr (kDual) {
    for (int e = tid; e < F2 * (H - half); e += kTmThreads)
      b2w_s[e] = body2_w[e];
    if (tid < H) bb_s[tid] = tid < half ? body_b[tid] : body2_b[tid - half];
    for (int e = tid; e < nx2; e += kTmThreads) {
      x2_s[e] = tm_slice_load(x2, e, 0, row0, B, S, F2);
      if (S > 1) x2_s[nx2 + e] = tm_slice_load(x2, e, 1, row0, B, S, F2);
    }
  } else {
    if (tid < H) bb_s[tid] = body_b[tid];
  }
  // thread (wave w, column tid % 64) covers rows 4w .. 4w+3 of a 16×64 block
  const int bk = tid % H, br0 = (tid / H) * 4;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int row = row0 + br0 + rr;
    const float v = h0[(long)min(row, B - 1) * h0s + bk];
    a_s[(br0 + rr) * LD + H + bk] = row < B ? v : 0.0f;
  }
  float c[4], h_last[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * kq + r;
    const float v = c0[(long)min(row, B - 1) * h0s + u];
    c[r] = row < B ? v : 0.0f;
  }
#pragma unroll
  for (int g = 0; g < 4; ++g) PDRL_PIN_REGS(bf[g], 32);
  __syncthreads();

  // Which encoder feeds column bk: ring, slot size, weight column and stride,
  // input count. Fixed for the whole sequence.
  const bool lo = !kDual || bk < half;
  const float* ring = lo ? x_s : x2_s;
  const int nslot = lo ? nx : nx2;
  const int nf = lo ? F : F2;
  const float* wcol = lo ? bw_s + bk : b2w_s + (bk - half);
  const int wst = lo ? half : H - half;

  // Body of step t into the xb half of `dst`, from ring slot t & 1. Same
  // fmaf order as the row kernel: bias first, then f ascending.
  auto body = [&](int t, float* dst) {
    const float* xs = ring + (t & 1) * nslot;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int r = br0 + rr;
      float acc = bb_s[bk];
      for (int f = 0; f < nf; ++f) acc = fmaf(xs[r * nf + f], wcol[f * wst], acc);
      acc = fmaxf(acc, 0.0f);
      dst[r * LD + bk] = acc;
      const int row = row0 + r;
      if (row < B) stash[((long)row * S + t) * kStashFields * H + bk] = acc;
    }
  };
  // Heads of step t on the h half of `src`: four lanes share one output,
  // 16 terms each, summed by two lane exchanges.
  auto heads = [&](int t, const float* src) {
    const int part = tid & 3;
    for (int o0 = 0; o0 < kTmRows * D; o0 += kTmThreads / 4) {
      const int o = o0 + tid / 4;
      const int oc = min(o, kTmRows * D - 1);
      const int r = oc / D, d = oc % D;
      const f32x4* hp =
          reinterpret_cast<const f32x4*>(src + r * LD + H + 16 * part);
      const float* wp = hw_s + 16 * part * D + d;
      float s = 0.0f;
#pragma unroll
      for (int k4 = 0; k4 < 4; ++k4) {
        const f32x4 hv = hp[k4];
#pragma unroll
        for (int m = 0; m < 4; ++m) s = fmaf(hv[m], wp[(4 * k4 + m) * D], s);
      }
      s += __shfl_xor(s, 1, kWave);
      s += __shfl_xor(s, 2, kWave);
      const int row = row0 + r;
      if (part == 0 && o < kTmRows * D && row < B)
        outs[((long)row * S + t) * D + d] = s + hb_s[d];
    }
  };

  body(0, a_s);
  __syncthreads();

  for (int t = 0; t < S; ++t) {
    const float* a_cur = a_s + (t & 1) * kTmRows * LD;
    float* a_nxt = a_s + ((t + 1) & 1) * kTmRows * LD;

    // inputs of step t+2, requested now, parked in the rings behind the MFMAs
    float x_pre = 0.0f, x2_pre = 0.0f;
    const bool pre = t + 2 < S;
    if (pre && tid < nx) x_pre = tm_slice_load(x, tid, t + 2, row0, B, S, F);
    if constexpr (kDual) {
      if (pre && tid < nx2)
        x2_pre = tm_slice_load(x2, tid, t + 2, row0, B, S, F2);
    }

    if (t > 0) heads(t - 1, a_cur);

    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
      acc[g] = f32x4{bias[g], bias[g], bias[g], bias[g]};
    const f32x4* ap = reinterpret_cast<const f32x4*>(a_cur + i * LD + 4 * kq);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const f32x4 av = ap[4 * q];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
#pragma unroll
        for (int g = 0; g < 4; ++g)
          acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bf[g][4 * q + m],
                                                        acc[g], 0, 0, 0);
      }
    }

#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float ig = sigmoidf_dev(acc[0][r]);
      const float fg = sigmoidf_dev(acc[1][r]);
      const float gg = tanhf(acc[2][r]);
      const float og = sigmoidf_dev(acc[3][r]);
      const float c_new = fg * c[r] + ig * gg;
      const float h_new = og * tanhf(c_new);
      c[r] = c_new;
      h_last[r] = h_new;
      a_nxt[(4 * kq + r) * LD + H + u] = h_new;
      const int row = row0 + 4 * kq + r;
      if (row < B) {
        const gst_f32 sp = stash + ((long)row * S + t) * kStashFields * H + u;
        sp[H] = ig;
        sp[2 * H] = fg;
        sp[3 * H] = gg;
        sp[4 * H] = og;
        sp[5 * H] = c_new;
        sp[6 * H] = h_new;
      }
    }

    if (t + 1 < S) body(t + 1, a_nxt);
    if (pre) {
      float* xs = x_s + (t & 1) * nx;
      if (tid < nx) xs[tid] = x_pre;
      for (int e = tid + kTmThreads; e < nx; e += kTmThreads)
        xs[e] = tm_slice_load(x, e, t + 2, row0, B, S, F);
      if constexpr (kDual) {
        float* xs2 = x2_s + (t & 1) * nx2;
        if (tid < nx2) xs2[tid] = x2_pre;
        for (int e = tid + kTmThreads; e < nx2; e += kTmThreads)
          xs2[e] = tm_slice_load(x2, e, t + 2, row0, B, S, F2);
      }
    }
    __syncthreads();
  }

  heads(S - 1, a_s + (S & 1) * kTmRows * LD);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * kq + r;
    if (row < B) {
      hS[(long)row * H + u] = h_last[r];
      cS[(long)row * H + u] = c[r];
    }
  }
}

template <bool kDx2>
__global__ __launch_bounds__(kTmThreads) void seq_lstm_bwd_tile_multi_kernel(
    const float* __restrict__ c0,      // (B,H) rows, stride h0s
    const long* __restrict__ in_tab,   // [C][7]
    const long* __restrict__ out_tab,  // [C][3]
    int B, int S, int D, long h0s, int F2, int half, int accum_dx2) {
  constexpr int H = kTmH, G = kTmG, LD = kTmBwdLd;
  const long* it = in_tab + (long)blockIdx.y * kBwdTabCols;
  const long* ot = out_tab + (long)blockIdx.y * kBwdOutCols;
  const gptr_f32 gouts = (gptr_f32)it[0];    // (B,S,D) head-output grads
  const gptr_f32 stash = (gptr_f32)it[1];    // (B,S,7H)
  const gptr_f32 w_ih = (gptr_f32)it[2];     // (H,4H)
  const gptr_f32 w_hh = (gptr_f32)it[3];     // (H,4H)
  const gptr_f32 heads_w = (gptr_f32)it[4];  // (H,D)
  const gptr_f32 body2_w = (gptr_f32)it[6];  // (F2,H-half)
  const gst_f32 dgates = (gst_f32)ot[0];     // (B,S,4H) pre-activation, or 0
  const gst_f32 dxb = (gst_f32)ot[1];        // (B,S,H) pre-ReLU
  const gst_f32 dx2 = (gst_f32)ot[2];        // (B,S,F2), or 0
  const bool want_dg = ot[0] != 0;
  const bool do_dx2 = kDx2 && ot[2] != 0 && it[6] != 0;
  const int W2 = H - half;   // parked columns (kDx2 only)
  const int PL = W2 + 4;     // their LDS row stride

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* dg_s = reinterpret_cast<float*>(smem_raw);  // [2][16][LD]
  float* hw_s = dg_s + 2 * kTmRows * LD;             // (H,D)
  float* g_s = hw_s + H * D;                         // [2][16][D] ring
  float* p_s = g_s + 2 * kTmRows * D;                // [2][16][PL] masked dxb
  float* w2_s = p_s + 2 * kTmRows * PL;              // (F2,W2)

  const int tid = threadIdx.x;
  const int w = tid / kWave, lane = tid % kWave;
  const int i = lane & 15, kq = lane >> 4;
  const int u = 16 * w + i;
  const int row0 = blockIdx.x * kTmRows;
  const int ng = kTmRows * D;

  // B fragments: bf[0][4q+m] = w_hh[u][16q + 4kq + m] (dh), bf[1] the same
  // of w_ih (dxb): runs of four floats of weight row u (dword loads: the
  // parameters are views of a flat buffer and promise no 16-byte alignment).
  float bf[2][64];
#pragma unroll
  for (int q = 0; q < 16; ++q) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      bf[0][4 * q + m] = w_hh[u * G + 16 * q + 4 * kq + m];
      bf[1][4 * q + m] = w_ih[u * G + 16 * q + 4 * kq + m];
    }
  }

  for (int e = tid; e < H * D; e += kTmThreads) hw_s[e] = heads_w[e];
  for (int e = tid; e < ng; e += kTmThreads) {
    g_s[((S - 1) & 1) * ng + e] =
        tm_slice_load(gouts, e, S - 1, row0, B, S, D);
    if (S > 1)
      g_s[(S & 1) * ng + e] = tm_slice_load(gouts, e, S - 2, row0, B, S, D);
  }
  if constexpr (kDx2) {
    if (do_dx2)
      for (int e = tid; e < F2 * W2; e += kTmThreads) w2_s[e] = body2_w[e];
  }

  // Stash fields of one step for this lane's four (row, unit) pairs.
  float s_i[4], s_f[4], s_g[4], s_o[4], s_c[4], s_cp[4], s_xb[4];
  auto fetch = [&](int t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * kq + r;
      const long rowc = min(row, B - 1);
      const bool live = row < B;
      const gptr_f32 sp = stash + (rowc * S + t) * kStashFields * H + u;
      const float cp = (t > 0) ? sp[5 * H - kStashFields * H]
                               : c0[rowc * h0s + u];
      const float xb = sp[0], ig = sp[H], fg = sp[2 * H], gg = sp[3 * H],
                  og = sp[4 * H], cc = sp[5 * H];
      s_xb[r] = live ? xb : 0.0f;
      s_i[r] = live ? ig : 0.0f;
      s_f[r] = live ? fg : 0.0f;
      s_g[r] = live ? gg : 0.0f;
      s_o[r] = live ? og : 0.0f;
      s_c[r] = live ? cc : 0.0f;
      s_cp[r] = live ? cp : 0.0f;
    }
  };
  fetch(S - 1);
#pragma unroll
  for (int n = 0; n < 2; ++n) PDRL_PIN_REGS(bf[n], 64);
  __syncthreads();

  // dx2 of step t from the parked buffer t & 1: four lanes share one output,
  // W2 / 4 columns each, summed by two lane exchanges.
  auto dx2_reduce = [&](int t) {
    const int part = tid & 3, q4 = W2 / 16;  // float4s per lane
    const float* ps = p_s + (t & 1) * kTmRows * PL;
    for (int o0 = 0; o0 < kTmRows * F2; o0 += kTmThreads / 4) {
      const int o = o0 + tid / 4;
      const int oc = min(o, kTmRows * F2 - 1);
      const int r = oc / F2, f = oc % F2;
      const f32x4* pp =
          reinterpret_cast<const f32x4*>(ps + r * PL + 4 * q4 * part);
      const float* wp = w2_s + f * W2 + 4 * q4 * part;
      float s = 0.0f;
      for (int k4 = 0; k4 < q4; ++k4) {
        const f32x4 pv = pp[k4];
#pragma unroll
        for (int m = 0; m < 4; ++m) s = fmaf(pv[m], wp[4 * k4 + m], s);
      }
      s += __shfl_xor(s, 1, kWave);
      s += __shfl_xor(s, 2, kWave);
      const int row = row0 + r;
      if (part == 0 && o < kTmRows * F2 && row < B) {
        const gst_f32 out = dx2 + ((long)row * S + t) * F2 + f;
        if (accum_dx2) {
          __hip_atomic_fetch_add(out, s, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT);
        } else {
          *out = s;
        }
      }
    }
  };

  float dh_rec[4] = {0.f, 0.f, 0.f, 0.f}, dc_rec[4] = {0.f, 0.f, 0.f, 0.f};

  for (int t = S - 1; t >= 0; --t) {
    float* dg = dg_s + (t & 1) * kTmRows * LD;
    const float* gs = g_s + (t & 1) * ng;

    bool relu_on[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int rt = 4 * kq + r;
      // head back-projection: dh_heads = Σ_d gouts[t][d] · heads_w[u][d]
      float dh = 0.0f;
      for (int d = 0; d < D; ++d) dh = fmaf(gs[rt * D + d], hw_s[u * D + d], dh);
      dh += dh_rec[r];
      const float i_ = s_i[r], f_ = s_f[r], g_ = s_g[r], o_ = s_o[r];
      const float tc = tanhf(s_c[r]);
      const float dc = dc_rec[r] + dh * o_ * (1.0f - tc * tc);
      const float d_i = dc * g_ * i_ * (1.0f - i_);
      const float d_f = dc * s_cp[r] * f_ * (1.0f - f_);
      const float d_g = dc * i_ * (1.0f - g_ * g_);
      const float d_o = dh * tc * o_ * (1.0f - o_);
      dc_rec[r] = dc * f_;
      relu_on[r] = s_xb[r] > 0.0f;
      float* lp = dg + rt * LD + u;
      lp[0] = d_i;
      lp[H] = d_f;
      lp[2 * H] = d_g;
      lp[3 * H] = d_o;
      const int row = row0 + rt;
      if (want_dg && row < B) {
        const gst_f32 gp = dgates + ((long)row * S + t) * G + u;
        gp[0] = d_i;
        gp[H] = d_f;
        gp[2 * H] = d_g;
        gp[3 * H] = d_o;
      }
    }

    // requests of the steps to come, landing behind the MFMA block
    if (t > 0) fetch(t - 1);
    float g_pre = 0.0f;
    const bool pre = t >= 2;
    if (pre && tid < ng)
      g_pre = tm_slice_load(gouts, tid, t - 2, row0, B, S, D);
    __syncthreads();

    // step t+1 parked its upper half before this barrier
    if constexpr (kDx2) {
      if (do_dx2 && t + 1 < S) dx2_reduce(t + 1);
    }

    f32x4 acc_h = {0.f, 0.f, 0.f, 0.f}, acc_x = {0.f, 0.f, 0.f, 0.f};
    const f32x4* ap = reinterpret_cast<const f32x4*>(dg + i * LD + 4 * kq);
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const f32x4 av = ap[4 * q];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        acc_h = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bf[0][4 * q + m],
                                                     acc_h, 0, 0, 0);
        acc_x = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bf[1][4 * q + m],
                                                     acc_x, 0, 0, 0);
      }
    }

#pragma unroll
    for (int r = 0; r < 4; ++r) {
      dh_rec[r] = acc_h[r];
      const float v = relu_on[r] ? acc_x[r] : 0.0f;
      const int row = row0 + 4 * kq + r;
      if (row < B) dxb[((long)row * S + t) * H + u] = v;
      if constexpr (kDx2) {
        // wave-uniform: half is a multiple of 16
        if (do_dx2 && u >= half)
          p_s[((t & 1) * kTmRows + 4 * kq + r) * PL + (u - half)] = v;
      }
    }
    // ring slot t & 1 was read before this step's barrier; step t-2 reads
    // it behind the next one
    if (pre) {
      float* gn = g_s + (t & 1) * ng;
      if (tid < ng) gn[tid] = g_pre;
      for (int e = tid + kTmThreads; e < ng; e += kTmThreads)
        gn[e] = tm_slice_load(gouts, e, t - 2, row0, B, S, D);
    }
  }

  if constexpr (kDx2) {
    if (do_dx2) {  // uniform over the workgroup
      __syncthreads();
      dx2_reduce(0);
    }
  }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

namespace {

bool tab_ok(const at::Tensor& t, int cols, long C) {
  return t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kLong &&
         t.dim() == 2 && t.size(1) == cols && t.size(0) >= C;
}

// half of a dual-body launch; F2 = 0 (single body) has none.
void check_half(const char* who, long F2, long half) {
  TORCH_CHECK(F2 >= 0, who, ": F2 must be >= 0");
  if (F2 > 0)
    TORCH_CHECK(half > 0 && half < kTmH && half % 16 == 0, who,
                ": half must be a multiple of 16 inside (0, 64), got ", half);
}

}  // namespace

// F2 > 0: dual-body launch, x2 / body2_w / body2_b from the table (a row
// whose x2 is 0 runs single-body). The outputs behind out_tab are the
// caller's: (B,S,D), (B,H), (B,H), (B,S,7H) per network.
void seq_lstm_fwd_tile_multi_hip(const at::Tensor& x, const at::Tensor& h0,
                                 const at::Tensor& c0,
                                 const at::Tensor& core_tab,
                                 const at::Tensor& out_tab, long C, long D,
                                 long F2, long half) {
  const char* who = "fwd_tile_multi";
  CHECK_IN(x);
  TORCH_CHECK(x.dim() == 3, who, ": x must be (B,S,F)");
  TORCH_CHECK(h0.dim() == 2 && c0.dim() == 2, who, ": h0/c0 must be (B,H)");
  const int B = x.size(0), S = x.size(1), F = x.size(2);
  const int H = h0.size(1);
  TORCH_CHECK(H == kTmH, who, " specialized for H=64");
  TORCH_CHECK(B >= 1 && S >= 1 && F >= 1 && D >= 1 && C >= 1 && C <= 65535,
              who, ": empty batch, sequence, input, head or network list");
  CHECK_GPU(h0); CHECK_F32(h0); CHECK_GPU(c0); CHECK_F32(c0);
  TORCH_CHECK(h0.size(0) == B && c0.size(0) == B && c0.size(1) == H &&
                  h0.stride(1) == 1 && c0.stride(1) == 1 &&
                  h0.stride(0) == c0.stride(0),
              who, ": h0/c0 must be (B,H) row views with one shared row "
              "stride");
  TORCH_CHECK(tab_ok(core_tab, kFwdTabCols, C) &&
                  tab_ok(out_tab, kFwdOutCols, C),
              who, ": tables are int64 on the GPU, one 10-wide / 4-wide row "
              "per network");
  check_half(who, F2, half);
  if (F2 == 0) half = H;
  // a table row without x2 lays its LDS out as a single-body core
  const long lds =
      std::max(fwd_tile_multi_lds_floats(F, (int)D, (int)F2, (int)half),
               fwd_tile_multi_lds_floats(F, (int)D, 0, H)) *
      sizeof(float);
  TORCH_CHECK(lds <= kTmMaxLds, who, " needs ", lds,
              " bytes of LDS for (F, D, F2) = (", F, ", ", D, ", ", F2, ")");
  const dim3 grid((B + kTmRows - 1) / kTmRows, (unsigned)C);
#define PDRL_LAUNCH_FTM(DUAL)                                               \
  hipLaunchKernelGGL((seq_lstm_fwd_tile_multi_kernel<DUAL>), grid,          \
                     dim3(kTmThreads), lds, current_stream(),               \
                     x.data_ptr<float>(), h0.data_ptr<float>(),             \
                     c0.data_ptr<float>(), core_tab.data_ptr<long>(),       \
                     out_tab.data_ptr<long>(), B, S, F, (int)D,             \
                     (long)h0.stride(0), (int)F2, (int)half)
  if (F2 > 0) {
    PDRL_LAUNCH_FTM(true);
  } else {
    PDRL_LAUNCH_FTM(false);
  }
#undef PDRL_LAUNCH_FTM
  HIP_CHECK_LAST();
}

// x gives (B, S) only: the inputs are leaves. F2 > 0: networks whose dx2
// slot is set get dx2 (B,S,F2), stored or, with accum_dx2, added.
void seq_lstm_bwd_tile_multi_hip(const at::Tensor& x, const at::Tensor& c0,
                                 const at::Tensor& in_tab,
                                 const at::Tensor& out_tab, long C, long D,
                                 long F2, long half, bool accum_dx2) {
  const char* who = "bwd_tile_multi";
  CHECK_IN(x);
  TORCH_CHECK(x.dim() == 3, who, ": x must be (B,S,F)");
  TORCH_CHECK(c0.dim() == 2, who, ": c0 must be (B,H)");
  const int B = x.size(0), S = x.size(1);
  const int H = c0.size(1);
  TORCH_CHECK(H == kTmH, who, " specialized for H=64");
  TORCH_CHECK(B >= 1 && S >= 1 && D >= 1 && C >= 1 && C <= 65535, who,
              ": empty batch, sequence, head or network list");
  CHECK_GPU(c0); CHECK_F32(c0);
  TORCH_CHECK(c0.size(0) == B && c0.stride(1) == 1, who,
              ": c0 must be a (B,H) row view with inner stride 1");
  TORCH_CHECK(tab_ok(in_tab, kBwdTabCols, C) &&
                  tab_ok(out_tab, kBwdOutCols, C),
              who, ": tables are int64 on the GPU, one 7-wide / 3-wide row "
              "per network");
  check_half(who, F2, half);
  if (F2 == 0) half = H;
  const long lds =
      bwd_tile_multi_lds_floats((int)D, (int)F2, (int)half) * sizeof(float);
  TORCH_CHECK(lds <= kTmMaxLds, who, " needs ", lds,
              " bytes of LDS for (D, F2) = (", D, ", ", F2, ")");
  const dim3 grid((B + kTmRows - 1) / kTmRows, (unsigned)C);
#define PDRL_LAUNCH_BTM(DX2)                                                \
  hipLaunchKernelGGL((seq_lstm_bwd_tile_multi_kernel<DX2>), grid,           \
                     dim3(kTmThreads), lds, current_stream(),               \
                     c0.data_ptr<float>(), in_tab.data_ptr<long>(),         \
                     out_tab.data_ptr<long>(), B, S, (int)D,                \
                     (long)c0.stride(0), (int)F2, (int)half,                \
                     accum_dx2 ? 1 : 0)
  if (F2 > 0) {
    PDRL_LAUNCH_BTM(true);
  } else {
    PDRL_LAUNCH_BTM(false);
  }
#undef PDRL_LAUNCH_BTM
  HIP_CHECK_LAST();
}
