// Row-tile SeqLSTMCore forward and BPTT for hidden size 128 (gfx950, fp32),
// selected by "rows_kernel": "tile128" in the fused on-policy step.
//
// seq_lstm_tile.hip keeps all of [w_ih ; w_hh] in registers, 128 fragments
// per lane at H = 64. At H = 128 the two matrices are 512 KiB, the whole
// register file of a CU, so these kernels keep ONE of them resident at a time
// and take the other matrix's GEMM, which is not recurrent, off the time loop
// into a phase of its own inside the same launch.
//
// Shared shape: 16 batch rows per workgroup, 8 waves (two per SIMD, 256
// registers per lane), v_mfma_f32_16x16x4_f32. Fragment layout, K permutation
// (MFMA number 4q + m takes from lane (i, kq) the K index 16q + 4kq + m, so
// one ds_read_b128 feeds four K-steps) and LDS row strides ≡ 4 (mod 64) are
// those of seq_lstm_tile.hip; its header gives the bank arithmetic.
//
// Forward. Wave w owns hidden units u = 16w + i of all four gates (four
// 16×16 output tiles, 32 K-steps each = 128 fragments), so i, f, g, o of a
// (row, unit) pair meet in one lane and c never leaves its registers.
//   Phase 1, every t independent: the fragments hold w_ih. The VALU body
//   writes xb_t into the A tile (and the stash), the MFMAs compute
//   xw_t = xb_t · w_ih + b_g, and each lane parks its 16 values in the
//   caller's (B, S, 4H) scratch tensor. The A tile is double buffered by step
//   parity (one barrier per t) and x runs through a two-step LDS ring.
//   Phase 2, the recurrence: the same registers now hold w_hh. A lane reads
//   back, one step ahead, exactly the scratch addresses it wrote itself and
//   uses them as the accumulators' initial value, so the serial chain of a
//   step is 128 MFMAs over h_{t-1} and the activations. The h tile is double
//   buffered by step parity: one barrier per step. The heads of step t − 1
//   read h_{t-1} from the buffer step t multiplies.
//
// Backward. Wave w owns columns [16w, 16w + 16) of dh = dgates · w_hhᵀ
// (K = 512 = 128 fragments); dh and dc of a (row, unit) pair stay in the lane
// that builds the gate gradients, as in the H = 64 tile.
//   Phase 1, the reverse time loop: gate gradients elementwise, stored to
//   dgates and to the LDS A tile, then the dh MFMAs.
//   Phase 2, every t independent: the registers take w_ih, the workgroup
//   stages the dgates rows it has just written (global memory, behind a
//   barrier) back through the LDS tile, one step ahead in registers, and
//   dxb_t = relu'(xb_t) ⊙ (dgates_t · w_ihᵀ) comes off the MFMAs.
//   The dgates tile is DOUBLE buffered in both phases (2·16·516 floats =
//   66 048 B, one barrier per step). The register budget already pins one
//   workgroup to a CU, so the second buffer costs no occupancy, and gfx950
//   gives a workgroup 160 KiB; single buffering would put a second barrier
//   between the MFMA block and the elementwise work of every serial step.
//
// Ragged tiles: rows ≥ B are clamped to row B − 1 before any pointer
// arithmetic, their loaded values are replaced by zeros and they store
// nothing. Nothing in LDS is sized by S.
#include "common.h"
#include "core_rows.h"
#include "wgrad_body.h"

// One scalar fmaf chain per sum, in a stated order (see wgrad_split.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int kT8Rows = 16;          // batch rows per workgroup
constexpr int kT8H = 128;            // hidden size
constexpr int kT8G = 4 * kT8H;       // gate columns
constexpr int kT8Threads = 512;      // 8 waves
constexpr int kT8FwdLd = kT8H + 4;   // LDS row stride of xb / h, floats
constexpr int kT8BwdLd = kT8G + 4;   // LDS row stride of dgates, floats
constexpr long kT8FwdMaxLds = 64 * 1024;
constexpr long kT8BwdMaxLds = 160 * 1024;  // a gfx950 workgroup's LDS

__host__ __device__ constexpr long fwd_tile128_lds_floats(int F, int D) {
  return 2L * kT8Rows * kT8FwdLd + (long)F * kT8H + kT8H + (long)kT8H * D + D +
         2L * kT8Rows * F;
}
__host__ __device__ constexpr long bwd_tile128_lds_floats(int D) {
  return 2L * kT8Rows * kT8BwdLd + (long)kT8H * D + 2L * kT8Rows * D;
}

// Element e of step t's (16, W) slice of a (B, S, W) tensor; zero past B.
__device__ __forceinline__ float tile128_slice_load(
    const float* __restrict__ src, int e, int t, int row0, int B, int S,
    int W) {
  const int row = row0 + e / W;
  const long rowc = min(row, B - 1);
  const float v = src[(rowc * S + t) * W + e % W];
  return row < B ? v : 0.0f;
}

// acc[g] += A(16×128, LDS rows of stride kT8FwdLd) · B fragments of gate g.
__device__ __forceinline__ void tile128_gates_mma(const float* a_tile, int i,
                                                  int kq,
                                                  const float (&bf)[4][32],
                                                  f32x4 (&acc)[4]) {
  const f32x4* ap =
      reinterpret_cast<const f32x4*>(a_tile + i * kT8FwdLd + 4 * kq);
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

// acc += A(16×512, LDS rows of stride kT8BwdLd) · B fragments (K = 512).
__device__ __forceinline__ void tile128_dgates_mma(const float* a_tile, int i,
                                                   int kq,
                                                   const float (&bf)[128],
                                                   f32x4& acc) {
  const f32x4* ap =
      reinterpret_cast<const f32x4*>(a_tile + i * kT8BwdLd + 4 * kq);
#pragma unroll
  for (int q = 0; q < 32; ++q) {
    const f32x4 av = ap[4 * q];
#pragma unroll
    for (int m = 0; m < 4; ++m)
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[m], bf[4 * q + m], acc, 0,
                                                 0, 0);
  }
}

__global__ __launch_bounds__(kT8Threads) void seq_lstm_fwd_tile128_kernel(
    const float* __restrict__ x,        // (B,S,F)
    const float* __restrict__ h0,       // (B,H) rows, stride h0s
    const float* __restrict__ c0,       // (B,H) rows, stride h0s
    const float* __restrict__ body_w,   // (F,H)
    const float* __restrict__ body_b,   // (H)
    const float* __restrict__ w_ih,     // (H,4H)
    const float* __restrict__ w_hh,     // (H,4H)
    const float* __restrict__ b_g,      // (4H)
    const float* __restrict__ heads_w,  // (H,D)
    const float* __restrict__ heads_b,  // (D)
    float* __restrict__ outs,           // (B,S,D)
    float* __restrict__ hS,             // (B,H)
    float* __restrict__ cS,             // (B,H)
    float* __restrict__ stash,          // (B,S,7H)
    float* __restrict__ xw,             // (B,S,4H) scratch: xb·w_ih + b_g
    int B, int S, int F, int D, long h0s) {
  constexpr int H = kT8H, G = kT8G, LD = kT8FwdLd;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* a_s = reinterpret_cast<float*>(smem_raw);  // [2][16][LD] xb, then h
  float* bw_s = a_s + 2 * kT8Rows * LD;             // (F,H)
  float* bb_s = bw_s + F * H;                       // (H)
  float* hw_s = bb_s + H;                           // (H,D)
  float* hb_s = hw_s + H * D;                       // (D)
  float* x_s = hb_s + D;                            // [2][16][F] ring

  const int tid = threadIdx.x;
  const int w = tid / kWave, lane = tid % kWave;
  const int i = lane & 15, kq = lane >> 4;
  const int u = 16 * w + i;  // this lane's hidden unit (accumulator column)
  const int row0 = blockIdx.x * kT8Rows;
  const int nx = kT8Rows * F;

  // B fragments: bf[g][4q+m] = src[16q + 4kq + m][g·H + u].
  float bf[4][32];
  auto load_b = [&](const float* __restrict__ src) {
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

  // The small weights and x of the first two steps.
  for (int e = tid; e < F * H; e += kT8Threads) bw_s[e] = body_w[e];
  for (int e = tid; e < H * D; e += kT8Threads) hw_s[e] = heads_w[e];
  if (tid < H) bb_s[tid] = body_b[tid];
  for (int e = tid; e < D; e += kT8Threads) hb_s[e] = heads_b[e];
  for (int e = tid; e < nx; e += kT8Threads) {
    x_s[e] = tile128_slice_load(x, e, 0, row0, B, S, F);
    if (S > 1) x_s[nx + e] = tile128_slice_load(x, e, 1, row0, B, S, F);
  }
  __syncthreads();

  // thread (column tid % 128) covers rows 4·(tid / 128) .. + 3 of a 16×128
  // block
  const int bk = tid % H, br0 = (tid / H) * 4;
  // Body of step t into `dst`, from ring slot t & 1. Same fmaf order as the
  // row kernel: bias first, then f ascending.
  auto body = [&](int t, float* dst) {
    const float* xs = x_s + (t & 1) * nx;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int r = br0 + rr;
      float acc = bb_s[bk];
      for (int f = 0; f < F; ++f) acc = fmaf(xs[r * F + f], bw_s[f * H + bk], acc);
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
    const float* a_cur = a_s + (t & 1) * kT8Rows * LD;
    float* a_nxt = a_s + ((t + 1) & 1) * kT8Rows * LD;

    // x of step t+2, requested now, parked in the ring behind the MFMAs
    float x_pre = 0.0f;
    const bool pre = t + 2 < S;
    if (pre && tid < nx) x_pre = tile128_slice_load(x, tid, t + 2, row0, B, S, F);

    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g)
      acc[g] = f32x4{bias[g], bias[g], bias[g], bias[g]};
    tile128_gates_mma(a_cur, i, kq, bf, acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * kq + r;
      if (row < B) {
        float* xp = xw + ((long)row * S + t) * G + u;
#pragma unroll
        for (int g = 0; g < 4; ++g) xp[g * H] = acc[g][r];
      }
    }

    if (t + 1 < S) body(t + 1, a_nxt);
    if (pre) {
      float* xs = x_s + (t & 1) * nx;
      if (tid < nx) xs[tid] = x_pre;
      for (int e = tid + kT8Threads; e < nx; e += kT8Threads)
        xs[e] = tile128_slice_load(x, e, t + 2, row0, B, S, F);
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
      const float* xp = xw + ((long)min(row, B - 1) * S + t) * G + u;
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
    for (int o0 = 0; o0 < kT8Rows * D; o0 += kT8Threads / 4) {
      const int o = o0 + tid / 4;
      const int oc = min(o, kT8Rows * D - 1);
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
      if (part == 0 && o < kT8Rows * D && row < B)
        outs[((long)row * S + t) * D + d] = s + hb_s[d];
    }
  };

  for (int t = 0; t < S; ++t) {
    const float* a_cur = a_s + (t & 1) * kT8Rows * LD;
    float* a_nxt = a_s + ((t + 1) & 1) * kT8Rows * LD;

    f32x4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = xw_pre[g];
    if (t + 1 < S) fetch_xw(t + 1);  // lands behind the MFMA block

    if (t > 0) heads(t - 1, a_cur);
    tile128_gates_mma(a_cur, i, kq, bf, acc);

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
        float* sp = stash + ((long)row * S + t) * kStashFields * H + u;
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

  heads(S - 1, a_s + (S & 1) * kT8Rows * LD);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * kq + r;
    if (row < B) {
      hS[(long)row * H + u] = h_last[r];
      cS[(long)row * H + u] = c[r];
    }
  }
}

__global__ __launch_bounds__(kT8Threads) void seq_lstm_bwd_tile128_kernel(
    const float* __restrict__ gouts,    // (B,S,D) head-output grads
    const float* __restrict__ stash,    // (B,S,7H)
    const float* __restrict__ c0,       // (B,H) rows, stride h0s
    const float* __restrict__ w_ih,     // (H,4H)
    const float* __restrict__ w_hh,     // (H,4H)
    const float* __restrict__ heads_w,  // (H,D)
    float* __restrict__ dgates,         // (B,S,4H) pre-activation
    float* __restrict__ dxb,            // (B,S,H) pre-ReLU
    int B, int S, int D, long h0s) {
  constexpr int H = kT8H, G = kT8G, LD = kT8BwdLd;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* dg_s = reinterpret_cast<float*>(smem_raw);  // [2][16][LD]
  float* hw_s = dg_s + 2 * kT8Rows * LD;             // (H,D)
  float* g_s = hw_s + H * D;                         // [2][16][D] ring

  const int tid = threadIdx.x;
  const int w = tid / kWave, lane = tid % kWave;
  const int i = lane & 15, kq = lane >> 4;
  const int u = 16 * w + i;
  const int row0 = blockIdx.x * kT8Rows;
  const int ng = kT8Rows * D;

  // B fragments: bf[4q+m] = src[u][16q + 4kq + m], runs of four floats of
  // weight row u (dword loads: the parameters are views of a flat buffer and
  // promise no 16-byte alignment).
  float bf[128];
  auto load_b = [&](const float* __restrict__ src) {
#pragma unroll
    for (int q = 0; q < 32; ++q) {
#pragma unroll
      for (int m = 0; m < 4; ++m)
        bf[4 * q + m] = src[u * G + 16 * q + 4 * kq + m];
    }
    PDRL_PIN_REGS(bf, 128);
  };
  load_b(w_hh);

  for (int e = tid; e < H * D; e += kT8Threads) hw_s[e] = heads_w[e];
  for (int e = tid; e < ng; e += kT8Threads) {
    g_s[((S - 1) & 1) * ng + e] =
        tile128_slice_load(gouts, e, S - 1, row0, B, S, D);
    if (S > 1)
      g_s[(S & 1) * ng + e] =
          tile128_slice_load(gouts, e, S - 2, row0, B, S, D);
  }

  // Stash fields of one step for this lane's four (row, unit) pairs.
  float s_i[4], s_f[4], s_g[4], s_o[4], s_c[4], s_cp[4];
  auto fetch = [&](int t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * kq + r;
      const long rowc = min(row, B - 1);
      const bool live = row < B;
      const float* sp = stash + (rowc * S + t) * kStashFields * H + u;
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
    float* dg = dg_s + (t & 1) * kT8Rows * LD;
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
        float* gp = dgates + ((long)row * S + t) * G + u;
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
      g_pre = tile128_slice_load(gouts, tid, t - 2, row0, B, S, D);
    __syncthreads();

    f32x4 acc_h = {0.f, 0.f, 0.f, 0.f};
    tile128_dgates_mma(dg, i, kq, bf, acc_h);
#pragma unroll
    for (int r = 0; r < 4; ++r) dh_rec[r] = acc_h[r];
    // ring slot t & 1 was read before this step's barrier; step t-2 reads
    // it behind the next one
    if (pre) {
      float* gn = g_s + (t & 1) * ng;
      if (tid < ng) gn[tid] = g_pre;
      for (int e = tid + kT8Threads; e < ng; e += kT8Threads)
        gn[e] = tile128_slice_load(gouts, e, t - 2, row0, B, S, D);
    }
  }

  // ---- phase 2: dxb_t = relu'(xb_t) ⊙ (dgates_t · w_ihᵀ), every t ----
  // Behind this barrier the tile's dgates rows are visible to the whole
  // workgroup and both LDS buffers are free.
  __syncthreads();
  load_b(w_ih);
  // Thread tid stages column tid of the 16 rows of a step's dgates tile.
  float dg_pre[kT8Rows];
  auto stage_load = [&](int t) {
#pragma unroll
    for (int j = 0; j < kT8Rows; ++j) {
      const int row = row0 + j;
      const float v = dgates[((long)min(row, B - 1) * S + t) * G + tid];
      dg_pre[j] = row < B ? v : 0.0f;
    }
  };
  auto stage_store = [&](float* dst) {
#pragma unroll
    for (int j = 0; j < kT8Rows; ++j) dst[j * LD + tid] = dg_pre[j];
  };
  stage_load(0);
  stage_store(dg_s);
  __syncthreads();

  for (int t = 0; t < S; ++t) {
    const float* dg = dg_s + (t & 1) * kT8Rows * LD;
    if (t + 1 < S) stage_load(t + 1);
    float xb[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const long rowc = min(row0 + 4 * kq + r, B - 1);
      xb[r] = stash[(rowc * S + t) * kStashFields * H + u];
    }

    f32x4 acc_x = {0.f, 0.f, 0.f, 0.f};
    tile128_dgates_mma(dg, i, kq, bf, acc_x);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * kq + r;
      if (row < B)
        dxb[((long)row * S + t) * H + u] = xb[r] > 0.0f ? acc_x[r] : 0.0f;
    }
    // the other buffer was last read before the previous step's barrier
    if (t + 1 < S) stage_store(dg_s + ((t + 1) & 1) * kT8Rows * LD);
    __syncthreads();
  }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

void seq_lstm_fwd_tile128_hip(
    const at::Tensor& x, const at::Tensor& h0, const at::Tensor& c0,
    const at::Tensor& body_w, const at::Tensor& body_b,
    const at::Tensor& w_ih, const at::Tensor& w_hh, const at::Tensor& b_g,
    const at::Tensor& heads_w, const at::Tensor& heads_b, at::Tensor& outs,
    at::Tensor& hS, at::Tensor& cS, at::Tensor& stash,
    at::Tensor& xw_scratch) {
  CHECK_IN(x); CHECK_IN(outs); CHECK_IN(hS); CHECK_IN(cS); CHECK_IN(stash);
  CHECK_IN(xw_scratch);
  TORCH_CHECK(x.dim() == 3, "x must be (B,S,F)");
  TORCH_CHECK(h0.dim() == 2 && c0.dim() == 2 && heads_w.dim() == 2,
              "h0/c0 must be (B,H) and heads_w (H,D)");
  const int B = x.size(0), S = x.size(1), F = x.size(2);
  const int H = h0.size(1), D = heads_w.size(1);
  TORCH_CHECK(H == kT8H, "fwd_tile128 specialized for H=128");
  TORCH_CHECK(B >= 1 && S >= 1 && F >= 1 && D >= 1,
              "fwd_tile128: empty batch, sequence, input or head");
  CHECK_GPU(h0); CHECK_F32(h0); CHECK_GPU(c0); CHECK_F32(c0);
  TORCH_CHECK(h0.size(0) == B && c0.size(0) == B && c0.size(1) == H &&
                  h0.stride(1) == 1 && c0.stride(1) == 1 &&
                  h0.stride(0) == c0.stride(0),
              "h0/c0 must be (B,H) row views with one shared row stride");
  CHECK_IN(body_w); CHECK_IN(body_b); CHECK_IN(w_ih); CHECK_IN(w_hh);
  CHECK_IN(b_g); CHECK_IN(heads_w); CHECK_IN(heads_b);
  TORCH_CHECK(body_w.numel() == (long)F * H && body_b.numel() == H &&
                  w_ih.numel() == (long)H * 4 * H &&
                  w_hh.numel() == (long)H * 4 * H && b_g.numel() == 4 * H &&
                  heads_w.size(0) == H && heads_b.numel() == D,
              "fwd_tile128: weight shapes do not match (F, H, D)");
  const long N = (long)B * S;
  TORCH_CHECK(outs.numel() == N * D && hS.numel() == (long)B * H &&
                  cS.numel() == (long)B * H &&
                  stash.numel() == N * kStashFields * H,
              "fwd_tile128: output shapes do not match x");
  TORCH_CHECK(xw_scratch.numel() == N * 4 * H,
              "fwd_tile128: xw_scratch must be (B,S,4H)");
  const long lds = fwd_tile128_lds_floats(F, D) * sizeof(float);
  TORCH_CHECK(lds <= kT8FwdMaxLds, "fwd_tile128 needs ", lds,
              " bytes of LDS for (F, D) = (", F, ", ", D, ")");
  hipLaunchKernelGGL(
      seq_lstm_fwd_tile128_kernel, dim3((B + kT8Rows - 1) / kT8Rows),
      dim3(kT8Threads), lds, current_stream(), x.data_ptr<float>(),
      h0.data_ptr<float>(), c0.data_ptr<float>(), body_w.data_ptr<float>(),
      body_b.data_ptr<float>(), w_ih.data_ptr<float>(),
      w_hh.data_ptr<float>(), b_g.data_ptr<float>(),
      heads_w.data_ptr<float>(), heads_b.data_ptr<float>(),
      outs.data_ptr<float>(), hS.data_ptr<float>(), cS.data_ptr<float>(),
      stash.data_ptr<float>(), xw_scratch.data_ptr<float>(), B, S, F, D,
      (long)h0.stride(0));
  HIP_CHECK_LAST();
}

void seq_lstm_bwd_tile128_hip(const at::Tensor& gouts, const at::Tensor& stash,
                              const at::Tensor& c0, const at::Tensor& w_ih,
                              const at::Tensor& w_hh,
                              const at::Tensor& heads_w, at::Tensor& dgates,
                              at::Tensor& dxb) {
  CHECK_IN(gouts); CHECK_IN(stash); CHECK_IN(dgates); CHECK_IN(dxb);
  CHECK_IN(w_ih); CHECK_IN(w_hh); CHECK_IN(heads_w);
  TORCH_CHECK(gouts.dim() == 3, "gouts must be (B,S,D)");
  TORCH_CHECK(c0.dim() == 2 && heads_w.dim() == 2,
              "c0 must be (B,H) and heads_w (H,D)");
  const int B = gouts.size(0), S = gouts.size(1), D = gouts.size(2);
  const int H = c0.size(1);
  TORCH_CHECK(H == kT8H, "bwd_tile128 specialized for H=128");
  TORCH_CHECK(B >= 1 && S >= 1 && D >= 1,
              "bwd_tile128: empty batch, sequence or head");
  CHECK_GPU(c0); CHECK_F32(c0);
  TORCH_CHECK(c0.size(0) == B && c0.stride(1) == 1,
              "c0 must be a (B,H) row view with inner stride 1");
  TORCH_CHECK(w_ih.numel() == (long)H * 4 * H &&
                  w_hh.numel() == (long)H * 4 * H && heads_w.size(0) == H &&
                  heads_w.size(1) == D,
              "bwd_tile128: weight shapes do not match (H, D)");
  const long N = (long)B * S;
  TORCH_CHECK(stash.numel() == N * kStashFields * H &&
                  dgates.numel() == N * 4 * H && dxb.numel() == N * H,
              "bwd_tile128: operand shapes do not match gouts");
  const long lds = bwd_tile128_lds_floats(D) * sizeof(float);
  TORCH_CHECK(lds <= kT8BwdMaxLds, "bwd_tile128 needs ", lds,
              " bytes of LDS for D = ", D);
  hipLaunchKernelGGL(
      seq_lstm_bwd_tile128_kernel, dim3((B + kT8Rows - 1) / kT8Rows),
      dim3(kT8Threads), lds, current_stream(), gouts.data_ptr<float>(),
      stash.data_ptr<float>(), c0.data_ptr<float>(), w_ih.data_ptr<float>(),
      w_hh.data_ptr<float>(), heads_w.data_ptr<float>(),
      dgates.data_ptr<float>(), dxb.data_ptr<float>(), B, S, D,
      (long)c0.stride(0));
  HIP_CHECK_LAST();
}
