// Row-tile SeqLSTMCore forward and BPTT for several networks in one launch at
// hidden size 128 (gfx950, fp32): the recurrent launches of the two fused SAC
// steps under "rows_kernel": "tile" when the model is 128 wide.
// seq_lstm_fwd_tile128_multi and seq_lstm_bwd_tile128_multi take exactly the
// device pointer tables of the row multi kernels (seq_lstm.hip) and of the
// H = 64 multi tile (seq_lstm_tile_multi.hip):
//   forward   core_tab [C][10] body_w, body_b, w_ih, w_hh, b_g, heads_w,
//                              heads_b, body2_w, body2_b, x2
//             out_tab  [C][4]  outs, hS, cS, stash
//             xw_tab   [C]     (B,S,4H) scratch per network (new here)
//   backward  in_tab   [C][7]  gouts, stash, w_ih, w_hh, heads_w, body_w,
//                              body2_w
//             out_tab  [C][3]  dgates, dxb, dx2
// Grid: blockIdx.x = tile of 16 batch rows, blockIdx.y = network; 512 threads
// (8 waves, two per SIMD, 256 registers per lane). x, h0 and c0 are kernel
// arguments shared by all networks; every table entry is cast to the global
// address space where it is read, so no access goes through a flat
// instruction. Tensors and stash field order are those of core_rows.h.
//
// The two-phase split is the design of seq_lstm_tile128.hip (read its header
// for why one of w_ih / w_hh is resident at a time, and seq_lstm_tile.hip's
// for the fragment layout, the K permutation and the bank argument); the
// tables, the dual-body encoder and dx2 are those of seq_lstm_tile_multi.hip,
// re-placed for two phases. This file keeps its own copy of the step bodies:
// neither sibling is touched, so their kernels keep their compiler figures.
//
// Forward. A wave owns 16 hidden units of all four gates (128 fragments per
// lane).
//   Phase 1, every t independent, w_ih resident: the VALU body writes xb_t
//   into the A tile (double buffered by step parity) and the stash, the MFMAs
//   compute xw_t = xb_t · w_ih + b_g and each lane parks its 16 values in its
//   network's scratch. The dual body (kDual, the continuous critics) lives
//   entirely here: both encoder weight blocks and the joined bias
//   [body_b | body2_b] sit in LDS, x2 has its own two-step ring next to x's,
//   and the thread that owns column bk picks ring, weight column, weight
//   stride and input count once, before the loop. Its sum is the row kernel's
//   chain (bias first, inputs ascending), so xb and every ReLU mask of the
//   backward are bit-identical to the row path. A table row whose x2 is 0 is
//   a single-body core. The single-body instantiation holds neither the
//   second ring nor the selects. Phase 2 never sees any of it.
//   Phase 2, the recurrence, w_hh resident: a lane reads back, one step
//   ahead, exactly the scratch addresses it wrote itself (no barrier or fence
//   is needed for a thread's own stores) as the accumulators' initial value.
//   The h tile is double buffered by step parity, one barrier per step; the
//   heads of step t − 1 read the buffer step t multiplies.
//
// Backward. Wave w owns columns [16w, 16w + 16) of dh = dgates · w_hhᵀ.
//   Phase 1, the reverse time loop, w_hh resident: gate gradients
//   elementwise, stored to dgates and to the double-buffered LDS tile, then
//   the dh MFMAs on 128 resident fragments; dh / dc stay in registers.
//   Phase 2, every t independent, w_ih resident: the workgroup stages the
//   dgates rows it has just written back through the LDS tile, one step
//   ahead in registers, and dxb_t = relu'(xb_t) ⊙ (dgates_t · w_ihᵀ) comes
//   off the MFMAs. Phase 2 reads dgates back from global memory, so the
//   dgates slot of out_tab must be set for every network (the H = 64 kernel
//   lets it be 0; the SAC steps always set it).
//
// dx2 (kDx2) belongs to phase 2: dx2[row][t][f] = Σ_j dxb[row][t][half + j] ·
//   body2_w[f][j] on the ReLU-masked dxb. The waves at or above half park
//   their masked values in an LDS buffer [2][16][H − half + 4] chosen by step
//   PARITY, and step t's sum is taken at the top of iteration t + 1, behind
//   the barrier that closes iteration t anyway (the last step's behind the
//   loop's last barrier: no flush barrier at all). Nothing in this phase is
//   serial, so the late sum delays nothing; reducing in the same iteration
//   would put a second barrier between the parking stores and the reads.
//   Iteration t + 2 overwrites buffer t & 1 only behind the barrier of
//   iteration t + 1, after its readers. Sum order: four lanes per output, a
//   quarter of the columns each, two lane exchanges, as in the H = 64 kernel.
//   With accum_dx2 the result is atomicAdd-ed into a buffer the caller
//   zeroed, otherwise stored. Each network's value is a fixed-order sum and
//   fp32 addition commutes, so the accumulated result is bit-reproducible for
//   TWO accumulating networks (0 + a + b = 0 + b + a) and NOT for more.
//   dx2 == 0 in the table skips all of it. dx, dh0 and dc0 stay skipped: the
//   inputs of these networks are leaves.
//
// Ragged tiles: rows ≥ B are clamped to row B − 1 before any pointer
// arithmetic, their loaded values are replaced by zeros and they store
// nothing, the scratch included. Nothing in LDS is sized by S.
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

// Memory reached through a device pointer table and written: global stores.
using gst_f32 = __attribute__((address_space(1))) float*;

constexpr int kM8Rows = 16;          // batch rows per workgroup
constexpr int kM8H = 128;            // hidden size
constexpr int kM8G = 4 * kM8H;       // gate columns
constexpr int kM8Threads = 512;      // 8 waves
constexpr int kM8FwdLd = kM8H + 4;   // LDS row stride of xb / h, floats
constexpr int kM8BwdLd = kM8G + 4;   // LDS row stride of dgates, floats
constexpr long kM8FwdMaxLds = 64 * 1024;
constexpr long kM8BwdMaxLds = 160 * 1024;  // a gfx950 workgroup's LDS
constexpr int kFwdTabCols = 10, kFwdOutCols = 4;
constexpr int kBwdTabCols = 7, kBwdOutCols = 3;

// Single body: F2 = 0 and half = H.
__host__ __device__ constexpr long fwd_tile128_multi_lds_floats(int F, int D,
                                                                int F2,
                                                                int half) {
  return 2L * kM8Rows * kM8FwdLd + (long)F * half +
         (long)F2 * (kM8H - half) + kM8H + (long)kM8H * D + D +
         2L * kM8Rows * F + 2L * kM8Rows * F2;
}
// F2 = 0: no dx2, no parking buffer.
__host__ __device__ constexpr long bwd_tile128_multi_lds_floats(int D, int F2,
                                                                int half) {
  return 2L * kM8Rows * kM8BwdLd + (long)kM8H * D + 2L * kM8Rows * D +
         (F2 > 0 ? 2L * kM8Rows * (kM8H - half + 4) + (long)F2 * (kM8H - half)
                 : 0L);
}

// Element e of step t's (16, W) slice of a (B, S, W) tensor; zero past B.
template <class P>
__device__ __forceinline__ float m8_slice_load(P src, int e, int t, int row0,
                                               int B, int S, int W) {
  const int row = row0 + e / W;
  const long rowc = min(row, B - 1);
  const float v = src[(rowc * S + t) * W + e % W];
  return row < B ? v : 0.0f;
}

// acc[g] += A(16×128, LDS rows of stride kM8FwdLd) · B fragments of gate g.
__device__ __forceinline__ void m8_gates_mma(const float* a_tile, int i,
                                             int kq, const float (&bf)[4][32],
                                             f32x4 (&acc)[4]) {
  const f32x4* ap =
      reinterpret_cast<const f32x4*>(a_tile + i * kM8FwdLd + 4 * kq);
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
}

// acc += A(16×512, LDS rows of stride kM8BwdLd) · B fragments (K = 512).
__device__ __forceinline__ void m8_dgates_mma(const float* a_tile, int i,
                                              int kq, const float (&bf)[128],
                                              f32x4& acc) {
  const f32x4* ap =
      reinterpret_cast<const f32x4*>(a_tile + i * kM8BwdLd + 4 * kq);
#pragma unroll
  for (int q = 0; q < 32; ++q) {
    const f32x4 av = ap[4 * q];
#pragma unroll
    for (int m = 0; m < 4; ++m)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bf[4 * q + m], acc, 0,
                                                 0, 0);
  }
}

template <bool kDual>
__global__ __launch_bounds__(kM8Threads) void seq_lstm_fwd_tile128_multi_kernel(
    const float* __restrict__ x,        // (B,S,F), all networks
    const float* __restrict__ h0,       // (B,H) rows, stride h0s
    const float* __restrict__ c0,       // (B,H) rows, stride h0s
    const long* __restrict__ core_tab,  // [C][10]
    const long* __restrict__ out_tab,   // [C][4]
    const long* __restrict__ xw_tab,    // [C]
    int B, int S, int F, int D, long h0s, int F2_arg, int half_arg) {
  constexpr int H = kM8H, G = kM8G, LD = kM8FwdLd;
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
  const gst_f32 xw = (gst_f32)xw_tab[blockIdx.y];  // (B,S,4H) scratch
  // a row without x2 is a single-body core (the row kernel's rule)
  const bool dual = kDual && ct[9] != 0;
  const int half = dual ? half_arg : H;
  const int F2 = dual ? F2_arg : 0;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* a_s = reinterpret_cast<float*>(smem_raw);  // [2][16][LD] xb, then h
  float* bw_s = a_s + 2 * kM8Rows * LD;             // (F,half)
  float* b2w_s = bw_s + F * half;                   // (F2,H-half)
  float* bb_s = b2w_s + F2 * (H - half);            // (H) body_b | body2_b
  float* hw_s = bb_s + H;                           // (H,D)
  float* hb_s = hw_s + H * D;                       // (D)
  float* x_s = hb_s + D;                            // [2][16][F] ring
  float* x2_s = x_s + 2 * kM8Rows * F;              // [2][16][F2] ring

  const int tid = threadIdx.x;
  const int w = tid / kWave, lane = tid % kWave;
  const int i = lane & 15, kq = lane >> 4;
  const int u = 16 * w + i;  // this lane's hidden unit (accumulator column)
  const int row0 = blockIdx.x * kM8Rows;
  const int nx = kM8Rows * F, nx2 = kM8Rows * F2;

  // B fragments: bf[g][4q+m] = src[16q + 4kq + m][g·H + u].
  float bf[4][32];
  auto load_b = [&](gptr_f32 src) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
#pragma unroll
        for (int m = 0; m < 4; ++m)
          bf[g][4 * q + m] = src[(16 * q + 4 * kq + m) * G + g * H + u];
      }
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) PDRL_PIN_REGS(bf[g], 32);
  };
  load_b(w_ih);
  float bias[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) bias[g] = b_g[g * H + u];

  // The small weights and the inputs of the first two steps.
  for (int e = tid; e < F * half; e += kM8Threads) bw_s[e] = body_w[e];
  for (int e = tid; e < H * D; e += kM8Threads) hw_s[e] = heads_w[e];
  for (int e = tid; e < D; e += kM8Threads) hb_s[e] = heads_b[e];
  for (int e = tid; e < nx; e += kM8Threads) {
    x_s[e] = m8_slice_load(x, e, 0, row0, B, S, F);
    if (S > 1) x_s[nx + e] = m8_slice_load(x, e, 1, row0, B, S, F);
  }
  if constexpr (kDual) {
    for (int e = tid; e < F2 * (H - half); e += kM8Threads)
      b2w_s[e] = body2_w[e];
    if (tid < H) bb_s[tid] = tid < half ? body_b[tid] : body2_b[tid - half];
    for (int e = tid; e < nx2; e += kM8Threads) {
      x2_s[e] = m8_slice_load(x2, e, 0, row0, B, S, F2);
      if (S > 1) x2_s[nx2 + e] = m8_slice_load(x2, e, 1, row0, B, S, F2);
    }
  } else {
    if (tid < H) bb_s[tid] = body_b[tid];
  }
  __syncthreads();

  // thread (column tid % 128) covers rows 4·(tid / 128) .. + 3 of a 16×128
  // block
  const int bk = tid % H, br0 = (tid / H) * 4;
  // Which encoder feeds column bk: ring, slot size, weight column and stride,
  // input count. Fixed for the whole sequence.
  const bool lo = !kDual || bk < half;
  const float* ring = lo ? x_s : x2_s;
  const int nslot = lo ? nx : nx2;
  const int nf = lo ? F : F2;
  const float* wcol = lo ? bw_s + bk : b2w_s + (bk - half);
  const int wst = lo ? half : H - half;

  // Body of step t into `dst`, from ring slot t & 1. Same fmaf order as the
  // row kernel: bias first, then f ascending.
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

  // ---- phase 1: xw_t = xb_t · w_ih + b_g for every t ----
  body(0, a_s);
  __syncthreads();
  for (int t = 0; t < S; ++t) {
    const float* a_cur = a_s + (t & 1) * kM8Rows * LD;
    float* a_nxt = a_s + ((t + 1) & 1) * kM8Rows * LD;

    // inputs of step t+2, requested now, parked in the rings behind the MFMAs
    float x_pre = 0.0f, x2_pre = 0.0f;
    const bool pre = t + 2 < S;
    if (pre && tid < nx) x_pre = m8_slice_load(x, tid, t + 2, row0, B, S, F);
    if constexpr (kDual) {
      if (pre && tid < nx2)
        x2_pre = m8_slice_load(x2, tid, t + 2, row0, B, S, F2);
    }

    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
      acc[g] = f32x4{bias[g], bias[g], bias[g], bias[g]};
    m8_gates_mma(a_cur, i, kq, bf, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * kq + r;
      if (row < B) {
        const gst_f32 xp = xw + ((long)row * S + t) * G + u;
#pragma unroll
        for (int g = 0; g < 4; ++g) xp[g * H] = acc[g][r];
      }
    }

    if (t + 1 < S) body(t + 1, a_nxt);
    if (pre) {
      float* xs = x_s + (t & 1) * nx;
      if (tid < nx) xs[tid] = x_pre;
      for (int e = tid + kM8Threads; e < nx; e += kM8Threads)
        xs[e] = m8_slice_load(x, e, t + 2, row0, B, S, F);
      if constexpr (kDual) {
        float* xs2 = x2_s + (t & 1) * nx2;
        if (tid < nx2) xs2[tid] = x2_pre;
        for (int e = tid + kM8Threads; e < nx2; e += kM8Threads)
          xs2[e] = m8_slice_load(x2, e, t + 2, row0, B, S, F2);
      }
    }
    __syncthreads();
  }

  // ---- phase 2: the recurrence, w_hh resident ----
  load_b(w_hh);
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int row = row0 + br0 + rr;
    const float v = h0[(long)min(row, B - 1) * h0s + bk];
    a_s[(br0 + rr) * LD + bk] = row < B ? v : 0.0f;
  }
  float c[4], h_last[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * kq + r;
    const float v = c0[(long)min(row, B - 1) * h0s + u];
    c[r] = row < B ? v : 0.0f;
  }
  // This lane's parked values of step t: the addresses it stored in phase 1.
  f32x4 xw_pre[4];
  auto fetch_xw = [&](int t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * kq + r;
      const gst_f32 xp = xw + ((long)min(row, B - 1) * S + t) * G + u;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float v = xp[g * H];
        xw_pre[g][r] = row < B ? v : 0.0f;
      }
    }
  };
  fetch_xw(0);
  __syncthreads();

  // Heads of step t on the h tile `src`: four lanes share one output, 32
  // terms each, summed by two lane exchanges.
  auto heads = [&](int t, const float* src) {
    const int part = tid & 3;
    for (int o0 = 0; o0 < kM8Rows * D; o0 += kM8Threads / 4) {
      const int o = o0 + tid / 4;
      const int oc = min(o, kM8Rows * D - 1);
      const int r = oc / D, d = oc % D;
      const f32x4* hp = reinterpret_cast<const f32x4*>(src + r * LD + 32 * part);
      const float* wp = hw_s + 32 * part * D + d;
      float s = 0.0f;
#pragma unroll
      for (int k4 = 0; k4 < 8; ++k4) {
        const f32x4 hv = hp[k4];
#pragma unroll
        for (int m = 0; m < 4; ++m) s = fmaf(hv[m], wp[(4 * k4 + m) * D], s);
      }
      s += __shfl_xor(s, 1, kWave);
      s += __shfl_xor(s, 2, kWave);
      const int row = row0 + r;
      if (part == 0 && o < kM8Rows * D && row < B)
        outs[((long)row * S + t) * D + d] = s + hb_s[d];
    }
  };

  for (int t = 0; t < S; ++t) {
    const float* a_cur = a_s + (t & 1) * kM8Rows * LD;
    float* a_nxt = a_s + ((t + 1) & 1) * kM8Rows * LD;

    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = xw_pre[g];
    if (t + 1 < S) fetch_xw(t + 1);  // lands behind the MFMA block

    if (t > 0) heads(t - 1, a_cur);
    m8_gates_mma(a_cur, i, kq, bf, acc);

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
      a_nxt[(4 * kq + r) * LD + u] = h_new;
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
    __syncthreads();
  }

  heads(S - 1, a_s + (S & 1) * kM8Rows * LD);
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
__global__ __launch_bounds__(kM8Threads) void seq_lstm_bwd_tile128_multi_kernel(
    const float* __restrict__ c0,      // (B,H) rows, stride h0s
    const long* __restrict__ in_tab,   // [C][7]
    const long* __restrict__ out_tab,  // [C][3]
    int B, int S, int D, long h0s, int F2, int half, int accum_dx2) {
  constexpr int H = kM8H, G = kM8G, LD = kM8BwdLd;
  const long* it = in_tab + (long)blockIdx.y * kBwdTabCols;
  const long* ot = out_tab + (long)blockIdx.y * kBwdOutCols;
  const gptr_f32 gouts = (gptr_f32)it[0];    // (B,S,D) head-output grads
  const gptr_f32 stash = (gptr_f32)it[1];    // (B,S,7H)
  const gptr_f32 w_ih = (gptr_f32)it[2];     // (H,4H)
  const gptr_f32 w_hh = (gptr_f32)it[3];     // (H,4H)
  const gptr_f32 heads_w = (gptr_f32)it[4];  // (H,D)
  const gptr_f32 body2_w = (gptr_f32)it[6];  // (F2,H-half)
  const gst_f32 dgates = (gst_f32)ot[0];     // (B,S,4H) pre-activation
  const gst_f32 dxb = (gst_f32)ot[1];        // (B,S,H) pre-ReLU
  const gst_f32 dx2 = (gst_f32)ot[2];        // (B,S,F2), or 0
  const bool do_dx2 = kDx2 && ot[2] != 0 && it[6] != 0;
  const int W2 = H - half;   // parked columns (kDx2 only)
  const int PL = W2 + 4;     // their LDS row stride

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* dg_s = reinterpret_cast<float*>(smem_raw);  // [2][16][LD]
  float* hw_s = dg_s + 2 * kM8Rows * LD;             // (H,D)
  float* g_s = hw_s + H * D;                         // [2][16][D] ring
  float* p_s = g_s + 2 * kM8Rows * D;                // [2][16][PL] masked dxb
  float* w2_s = p_s + 2 * kM8Rows * PL;              // (F2,W2)

  const int tid = threadIdx.x;
  const int w = tid / kWave, lane = tid % kWave;
  const int i = lane & 15, kq = lane >> 4;
  const int u = 16 * w + i;
  const int row0 = blockIdx.x * kM8Rows;
  const int ng = kM8Rows * D;

  // B fragments: bf[4q+m] = src[u][16q + 4kq + m], runs of four floats of
  // weight row u (dword loads: the parameters are views of a flat buffer and
  // promise no 16-byte alignment).
  float bf[128];
  auto load_b = [&](gptr_f32 src) {
#pragma unroll
    for (int q = 0; q < 32; ++q) {
#pragma unroll
      for (int m = 0; m < 4; ++m)
        bf[4 * q + m] = src[u * G + 16 * q + 4 * kq + m];
    }
    PDRL_PIN_REGS(bf, 128);
  };
  load_b(w_hh);

  for (int e = tid; e < H * D; e += kM8Threads) hw_s[e] = heads_w[e];
  for (int e = tid; e < ng; e += kM8Threads) {
    g_s[((S - 1) & 1) * ng + e] =
        m8_slice_load(gouts, e, S - 1, row0, B, S, D);
    if (S > 1)
      g_s[(S & 1) * ng + e] = m8_slice_load(gouts, e, S - 2, row0, B, S, D);
  }
  if constexpr (kDx2) {
    if (do_dx2)
      for (int e = tid; e < F2 * W2; e += kM8Threads) w2_s[e] = body2_w[e];
  }

  // Stash fields of one step for this lane's four (row, unit) pairs.
  float s_i[4], s_f[4], s_g[4], s_o[4], s_c[4], s_cp[4];
  auto fetch = [&](int t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * kq + r;
      const long rowc = min(row, B - 1);
      const bool live = row < B;
      const gptr_f32 sp = stash + (rowc * S + t) * kStashFields * H + u;
      const float cp = (t > 0) ? sp[5 * H - kStashFields * H]
                               : c0[rowc * h0s + u];
      const float ig = sp[H], fg = sp[2 * H], gg = sp[3 * H], og = sp[4 * H],
                  cc = sp[5 * H];
      s_i[r] = live ? ig : 0.0f;
      s_f[r] = live ? fg : 0.0f;
      s_g[r] = live ? gg : 0.0f;
      s_o[r] = live ? og : 0.0f;
      s_c[r] = live ? cc : 0.0f;
      s_cp[r] = live ? cp : 0.0f;
    }
  };
  fetch(S - 1);
  __syncthreads();

  // ---- phase 1: the reverse time loop, w_hh resident ----
  float dh_rec[4] = {0.f, 0.f, 0.f, 0.f}, dc_rec[4] = {0.f, 0.f, 0.f, 0.f};
  for (int t = S - 1; t >= 0; --t) {
    float* dg = dg_s + (t & 1) * kM8Rows * LD;
    const float* gs = g_s + (t & 1) * ng;

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
      float* lp = dg + rt * LD + u;
      lp[0] = d_i;
      lp[H] = d_f;
      lp[2 * H] = d_g;
      lp[3 * H] = d_o;
      const int row = row0 + rt;
      if (row < B) {
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
      g_pre = m8_slice_load(gouts, tid, t - 2, row0, B, S, D);
    __syncthreads();

    f32x4 acc_h = {0.f, 0.f, 0.f, 0.f};
    m8_dgates_mma(dg, i, kq, bf, acc_h);
#pragma unroll
    for (int r = 0; r < 4; ++r) dh_rec[r] = acc_h[r];
    // ring slot t & 1 was read before this step's barrier; step t-2 reads
    // it behind the next one
    if (pre) {
      float* gn = g_s + (t & 1) * ng;
      if (tid < ng) gn[tid] = g_pre;
      for (int e = tid + kM8Threads; e < ng; e += kM8Threads)
        gn[e] = m8_slice_load(gouts, e, t - 2, row0, B, S, D);
    }
  }

  // ---- phase 2: dxb_t = relu'(xb_t) ⊙ (dgates_t · w_ihᵀ), every t ----
  // Behind this barrier the tile's dgates rows are visible to the whole
  // workgroup and both LDS buffers are free.
  __syncthreads();
  load_b(w_ih);
  // Thread tid stages column tid of the 16 rows of a step's dgates tile.
  float dg_pre[kM8Rows];
  auto stage_load = [&](int t) {
#pragma unroll
    for (int j = 0; j < kM8Rows; ++j) {
      const int row = row0 + j;
      const float v = dgates[((long)min(row, B - 1) * S + t) * G + tid];
      dg_pre[j] = row < B ? v : 0.0f;
    }
  };
  auto stage_store = [&](float* dst) {
#pragma unroll
    for (int j = 0; j < kM8Rows; ++j) dst[j * LD + tid] = dg_pre[j];
  };
  stage_load(0);
  stage_store(dg_s);

  // dx2 of step t from the parked buffer t & 1: four lanes share one output,
  // W2 / 4 columns each, summed by two lane exchanges.
  auto dx2_reduce = [&](int t) {
    const int part = tid & 3, q4 = W2 / 16;  // float4s per lane
    const float* ps = p_s + (t & 1) * kM8Rows * PL;
    for (int o0 = 0; o0 < kM8Rows * F2; o0 += kM8Threads / 4) {
      const int o = o0 + tid / 4;
      const int oc = min(o, kM8Rows * F2 - 1);
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
      if (part == 0 && o < kM8Rows * F2 && row < B) {
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
  __syncthreads();

  for (int t = 0; t < S; ++t) {
    const float* dg = dg_s + (t & 1) * kM8Rows * LD;
    if (t + 1 < S) stage_load(t + 1);
    float xb[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long rowc = min(row0 + 4 * kq + r, B - 1);
      xb[r] = stash[(rowc * S + t) * kStashFields * H + u];
    }
    // step t-1 parked its upper half before the barrier that closed it
    if constexpr (kDx2) {
      if (do_dx2 && t > 0) dx2_reduce(t - 1);
    }

    f32x4 acc_x = {0.f, 0.f, 0.f, 0.f};
    m8_dgates_mma(dg, i, kq, bf, acc_x);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float v = xb[r] > 0.0f ? acc_x[r] : 0.0f;
      const int row = row0 + 4 * kq + r;
      if (row < B) dxb[((long)row * S + t) * H + u] = v;
      if constexpr (kDx2) {
        // wave-uniform: half is a multiple of 16
        if (do_dx2 && u >= half)
          p_s[((t & 1) * kM8Rows + 4 * kq + r) * PL + (u - half)] = v;
      }
    }
    // the other buffer was last read before the previous step's barrier
    if (t + 1 < S) stage_store(dg_s + ((t + 1) & 1) * kM8Rows * LD);
    __syncthreads();
  }
  if constexpr (kDx2) {
    if (do_dx2) dx2_reduce(S - 1);  // behind the loop's last barrier
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
    TORCH_CHECK(half > 0 && half < kM8H && half % 16 == 0, who,
                ": half must be a multiple of 16 inside (0, 128), got ", half);
}

}  // namespace

// F2 > 0: dual-body launch, x2 / body2_w / body2_b from the table (a row
// whose x2 is 0 runs single-body). The outputs behind out_tab and the
// scratch tensors behind xw_tab are the caller's: (B,S,D), (B,H), (B,H),
// (B,S,7H) and (B,S,4H) per network.
void seq_lstm_fwd_tile128_multi_hip(const at::Tensor& x, const at::Tensor& h0,
                                    const at::Tensor& c0,
                                    const at::Tensor& core_tab,
                                    const at::Tensor& out_tab,
                                    const at::Tensor& xw_tab, long C, long D,
                                    long F2, long half) {
  const char* who = "fwd_tile128_multi";
  CHECK_IN(x);
  TORCH_CHECK(x.dim() == 3, who, ": x must be (B,S,F)");
  TORCH_CHECK(h0.dim() == 2 && c0.dim() == 2, who, ": h0/c0 must be (B,H)");
  const int B = x.size(0), S = x.size(1), F = x.size(2);
  const int H = h0.size(1);
  TORCH_CHECK(H == kM8H, who, " specialized for H=128");
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
  TORCH_CHECK(xw_tab.is_cuda() && xw_tab.is_contiguous() &&
                  xw_tab.scalar_type() == at::kLong && xw_tab.dim() == 1 &&
                  xw_tab.size(0) >= C,
              who, ": xw_tab is int64 on the GPU, one (B,S,4H) scratch "
              "pointer per network");
  check_half(who, F2, half);
  if (F2 == 0) half = H;
  // a table row without x2 lays its LDS out as a single-body core
  const long lds =
      std::max(fwd_tile128_multi_lds_floats(F, (int)D, (int)F2, (int)half),
               fwd_tile128_multi_lds_floats(F, (int)D, 0, H)) *
      sizeof(float);
  TORCH_CHECK(lds <= kM8FwdMaxLds, who, " needs ", lds,
              " bytes of LDS for (F, D, F2) = (", F, ", ", D, ", ", F2, ")");
  const dim3 grid((B + kM8Rows - 1) / kM8Rows, (unsigned)C);
#define PDRL_LAUNCH_FM8(DUAL)                                               \
  hipLaunchKernelGGL((seq_lstm_fwd_tile128_multi_kernel<DUAL>), grid,       \
                     dim3(kM8Threads), lds, current_stream(),               \
                     x.data_ptr<float>(), h0.data_ptr<float>(),             \
                     c0.data_ptr<float>(), core_tab.data_ptr<long>(),       \
                     out_tab.data_ptr<long>(), xw_tab.data_ptr<long>(), B,  \
                     S, F, (int)D, (long)h0.stride(0), (int)F2, (int)half)
  if (F2 > 0) {
    PDRL_LAUNCH_FM8(true);
  } else {
    PDRL_LAUNCH_FM8(false);
  }
#undef PDRL_LAUNCH_FM8
  HIP_CHECK_LAST();
}

// x gives (B, S) only: the inputs are leaves. Every network's dgates slot
// must be set (phase 2 reads it back). F2 > 0: networks whose dx2 slot is set
// get dx2 (B,S,F2), stored or, with accum_dx2, added.
void seq_lstm_bwd_tile128_multi_hip(const at::Tensor& x, const at::Tensor& c0,
                                    const at::Tensor& in_tab,
                                    const at::Tensor& out_tab, long C, long D,
                                    long F2, long half, bool accum_dx2) {
  const char* who = "bwd_tile128_multi";
  CHECK_IN(x);
  TORCH_CHECK(x.dim() == 3, who, ": x must be (B,S,F)");
  TORCH_CHECK(c0.dim() == 2, who, ": c0 must be (B,H)");
  const int B = x.size(0), S = x.size(1);
  const int H = c0.size(1);
  TORCH_CHECK(H == kM8H, who, " specialized for H=128");
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
      bwd_tile128_multi_lds_floats((int)D, (int)F2, (int)half) * sizeof(float);
  TORCH_CHECK(lds <= kM8BwdMaxLds, who, " needs ", lds,
              " bytes of LDS for (D, F2) = (", D, ", ", F2, ")");
  const dim3 grid((B + kM8Rows - 1) / kM8Rows, (unsigned)C);
#define PDRL_LAUNCH_BM8(DX2)                                                \
  hipLaunchKernelGGL((seq_lstm_bwd_tile128_multi_kernel<DX2>), grid,        \
                     dim3(kM8Threads), lds, current_stream(),               \
                     c0.data_ptr<float>(), in_tab.data_ptr<long>(),         \
                     out_tab.data_ptr<long>(), B, S, (int)D,                \
                     (long)c0.stride(0), (int)F2, (int)half,                \
                     accum_dx2 ? 1 : 0)
  if (F2 > 0) {
    PDRL_LAUNCH_BM8(true);
  } else {
    PDRL_LAUNCH_BM8(false);
  }
#undef PDRL_LAUNCH_BM8
  HIP_CHECK_LAST();
}
