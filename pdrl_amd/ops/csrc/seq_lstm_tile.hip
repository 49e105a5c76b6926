// Row-tile SeqLSTMCore forward and BPTT for many-row batches (gfx950, H = 64,
// fp32), selected by "rows_kernel": "tile".
//
// The row kernels (seq_lstm.hip, fwd_loss.hip) give one workgroup to one
// batch row: every workgroup pulls all of w_ih and w_hh (128 KiB) out of L2
// for S steps of ONE row, on the VALU. That is the right shape while B is
// below the CU count. Here one workgroup of 4 waves owns a tile of 16 batch
// rows and runs the recurrent GEMMs on v_mfma_f32_16x16x4_f32, so the weights
// are fetched once per 16 rows and ceil(B/16) workgroups fill the chip from
// B = 16 · CUs on. Nothing in LDS is sized by S: the kernels run at any S ≥ 1.
// They read and write exactly the tensors of the row kernels (stash field
// order of core_rows.h), so the loss launches, both weight-gradient kernels
// and the optimizer are shared.
//
// Fragment layout of the 16x16x4 MFMA (as used in wgrad_body.h): with
// i = lane & 15 and kq = lane >> 4, a lane supplies A[row i][k = kq] and
// B[k = kq][col i]; C/D register r of a lane is C[row 4·kq + r][col i].
//
// Forward, per step: gates(16×256) = [xb_t | h_{t-1}](16×128) · [w_ih ; w_hh]
//   Wave w owns hidden units u = 16w + i of all FOUR gates: four 16×16 output
//   tiles, 32 MFMAs each over K = 128. A lane therefore holds i, f, g, o of
//   the same four (row, unit) pairs, and the activations, the cell update and
//   c over the whole sequence stay in its registers; no gate goes through
//   LDS. The wave's B fragments (4 tiles × 32 K-steps = 128 VGPRs) are loaded
//   once and stay resident for all S steps.
//   The A tile lives in LDS, both halves double buffered by step parity:
//   step t multiplies buffer t & 1 and writes h_t (from the accumulator
//   layout) and xb_{t+1} (VALU body) into the other one, so a step costs ONE
//   barrier. The heads of step t − 1 read h_{t-1} from the buffer step t
//   multiplies. x is staged two steps ahead through a small LDS ring: its
//   global load is issued before the MFMA block and lands behind it.
//
// K permutation and row stride. MFMA number 4q + m of a step takes from lane
// (i, kq) the K index 16q + 4kq + m, in the A and the B fragment alike (a
// sum over K does not care about the order). A lane's four A values of one q
// are then contiguous: one ds_read_b128 feeds 4 K-steps × 4 gate tiles =
// 16 MFMAs. The row stride is 128 + 4 = 132 floats (260 in the backward):
// stride ≡ 4 (mod 64) puts the 16 rows that the lanes of one kq read at the
// same column on 16 disjoint 4-bank groups, the conflict-free pattern of a
// b128 read; and the h_new / dgates stores from the accumulator layout
// (address 132·(4kq + r) + u) hit bank 16kq + 4r + u mod 64: all 64 lanes of
// a wave on different banks.
//
// Backward, per step (reverse): the pre-activation gate gradients are built
// elementwise with the formulas of seq_lstm_bwd_row_on, stored to dgates and
// placed in LDS (double buffered, one barrier per step) as the A operand of
//   [dh_{t-1} | dxb_pre](16×128) = dgates(16×256) · [w_hh ; w_ih]ᵀ.
//   Wave w owns columns [16w, 16w+16) of BOTH halves: two tiles × 64 K-steps,
//   again 128 resident weight fragments, each a contiguous float4 of a
//   weight row thanks to the K permutation. (Columns [32w, 32w+32) would be
//   the same register budget, but would leave dh with two waves only and
//   cost a second barrier and an LDS round trip to hand it to the threads
//   that hold dc.) With this split a lane's dh_{t-1} comes out of the MFMA in
//   the layout of the forward's accumulators: dh and dc of a (row, unit)
//   pair never leave the lane, every wave does a quarter of the elementwise
//   work, and the stash is read back with the pattern it was written in.
//   The stash fields of step t − 1 are requested before the MFMA block of
//   step t; gouts goes through a two-step LDS ring like x in the forward,
//   and the head back-projection gouts_t · heads_wᵀ runs inside the loop.
//
// Global stores from the accumulator layout cover, per instruction, four
// contiguous 64-byte runs (16 lanes × 4 B in each of 4 rows).
//
// Ragged tiles: rows ≥ B are clamped to row B − 1 before any pointer
// arithmetic, their loaded values are replaced by zeros and they store
// nothing.
#include "common.h"
#include "core_rows.h"
#include "wgrad_body.h"

// One scalar fmaf chain per sum, in a stated order (see wgrad_split.hip).
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int kTlRows = 16;           // batch rows per workgroup
constexpr int kTlH = 64;              // hidden size
constexpr int kTlG = 4 * kTlH;        // gate columns
constexpr int kTlThreads = 256;       // 4 waves
constexpr int kTlFwdLd = 2 * kTlH + 4;  // LDS row stride of [xb | h], floats
constexpr int kTlBwdLd = kTlG + 4;      // LDS row stride of dgates, floats
constexpr long kTlMaxLds = 64 * 1024;   // dynamic LDS of one launch

__host__ __device__ constexpr long fwd_tile_lds_floats(int F, int D) {
  return 2L * kTlRows * kTlFwdLd + (long)F * kTlH + kTlH + (long)kTlH * D + D +
         2L * kTlRows * F;
}
__host__ __device__ constexpr long bwd_tile_lds_floats(int D) {
  return 2L * kTlRows * kTlBwdLd + (long)kTlH * D + 2L * kTlRows * D;
}

// Element e of step t's (16, W) slice of a (B, S, W) tensor; zero past B.
__device__ __forceinline__ float tile_slice_load(const float* __restrict__ src,
                                                 int e, int t, int row0, int B,
                                                 int S, int W) {
  const int row = row0 + e / W;
  const long rowc = min(row, B - 1);
  const float v = src[(rowc * S + t) * W + e % W];
  return row < B ? v : 0.0f;
}

__global__ __launch_bounds__(kTlThreads) void seq_lstm_fwd_tile_kernel(
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
    int B, int S, int F, int D, long h0s) {
  constexpr int H = kTlH, G = kTlG, LD = kTlFwdLd;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* a_s = reinterpret_cast<float*>(smem_raw);  // [2][16][LD] xb | h
  float* bw_s = a_s + 2 * kTlRows * LD;             // (F,H)
  float* bb_s = bw_s + F * H;                       // (H)
  float* hw_s = bb_s + H;                           // (H,D)
  float* hb_s = hw_s + H * D;                       // (D)
  float* x_s = hb_s + D;                            // [2][16][F] ring

  const int tid = threadIdx.x;
  const int w = tid / kWave, lane = tid % kWave;
  const int i = lane & 15, kq = lane >> 4;
  const int u = 16 * w + i;  // this lane's hidden unit (accumulator column)
  const int row0 = blockIdx.x * kTlRows;
  const int nx = kTlRows * F;

  // B fragments: bf[g][4q+m] = [w_ih ; w_hh][16q + 4kq + m][g·H + u].
  float bf[4][32];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float* src = (q < 4) ? w_ih : w_hh;  // K = 64 .. 127 is w_hh
#pragma unroll
      for (int m = 0; m < 4; ++m)
        bf[g][4 * q + m] = src[(16 * (q & 3) + 4 * kq + m) * G + g * H + u];
    }
  }
  float bias[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) bias[g] = b_g[g * H + u];

  // The small weights, x of the first two steps, h0 into buffer 0.
  for (int e = tid; e < F * H; e += kTlThreads) bw_s[e] = body_w[e];
  for (int e = tid; e < H * D; e += kTlThreads) hw_s[e] = heads_w[e];
  if (tid < H) bb_s[tid] = body_b[tid];
  for (int e = tid; e < D; e += kTlThreads) hb_s[e] = heads_b[e];
  for (int e = tid; e < nx; e += kTlThreads) {
    x_s[e] = tile_slice_load(x, e, 0, row0, B, S, F);
    if (S > 1) x_s[nx + e] = tile_slice_load(x, e, 1, row0, B, S, F);
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

  // Body of step t into the xb half of `dst`, from ring slot t & 1. Same
  // fmaf order as the row kernel: bias first, then f ascending.
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
  // Heads of step t on the h half of `src`: four lanes share one output,
  // 16 terms each, summed by two lane exchanges.
  auto heads = [&](int t, const float* src) {
    const int part = tid & 3;
    for (int o0 = 0; o0 < kTlRows * D; o0 += kTlThreads / 4) {
      const int o = o0 + tid / 4;
      const int oc = min(o, kTlRows * D - 1);
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
      if (part == 0 && o < kTlRows * D && row < B)
        outs[((long)row * S + t) * D + d] = s + hb_s[d];
    }
  };

  body(0, a_s);
  __syncthreads();

  for (int t = 0; t < S; ++t) {
    const float* a_cur = a_s + (t & 1) * kTlRows * LD;
    float* a_nxt = a_s + ((t + 1) & 1) * kTlRows * LD;

    // x of step t+2, requested now, parked in the ring behind the MFMAs
    float x_pre = 0.0f;
    const bool pre = t + 2 < S;
    if (pre && tid < nx) x_pre = tile_slice_load(x, tid, t + 2, row0, B, S, F);

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
        float* sp = stash + ((long)row * S + t) * kStashFields * H + u;
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
      for (int e = tid + kTlThreads; e < nx; e += kTlThreads)
        xs[e] = tile_slice_load(x, e, t + 2, row0, B, S, F);
    }
    __syncthreads();
  }

  heads(S - 1, a_s + (S & 1) * kTlRows * LD);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = row0 + 4 * kq + r;
    if (row < B) {
      hS[(long)row * H + u] = h_last[r];
      cS[(long)row * H + u] = c[r];
    }
  }
}

__global__ __launch_bounds__(kTlThreads) void seq_lstm_bwd_tile_kernel(
    const float* __restrict__ gouts,    // (B,S,D) head-output grads
    const float* __restrict__ stash,    // (B,S,7H)
    const float* __restrict__ c0,       // (B,H) rows, stride h0s
    const float* __restrict__ w_ih,     // (H,4H)
    const float* __restrict__ w_hh,     // (H,4H)
    const float* __restrict__ heads_w,  // (H,D)
    float* __restrict__ dgates,         // (B,S,4H) pre-activation
    float* __restrict__ dxb,            // (B,S,H) pre-ReLU
    int B, int S, int D, long h0s) {
  constexpr int H = kTlH, G = kTlG, LD = kTlBwdLd;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* dg_s = reinterpret_cast<float*>(smem_raw);  // [2][16][LD]
  float* hw_s = dg_s + 2 * kTlRows * LD;             // (H,D)
  float* g_s = hw_s + H * D;                         // [2][16][D] ring

  const int tid = threadIdx.x;
  const int w = tid / kWave, lane = tid % kWave;
  const int i = lane & 15, kq = lane >> 4;
  const int u = 16 * w + i;
  const int row0 = blockIdx.x * kTlRows;
  const int ng = kTlRows * D;

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

  for (int e = tid; e < H * D; e += kTlThreads) hw_s[e] = heads_w[e];
  for (int e = tid; e < ng; e += kTlThreads) {
    g_s[((S - 1) & 1) * ng + e] =
        tile_slice_load(gouts, e, S - 1, row0, B, S, D);
    if (S > 1)
      g_s[(S & 1) * ng + e] = tile_slice_load(gouts, e, S - 2, row0, B, S, D);
  }

  // Stash fields of one step for this lane's four (row, unit) pairs.
  float s_i[4], s_f[4], s_g[4], s_o[4], s_c[4], s_cp[4], s_xb[4];
  auto fetch = [&](int t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = row0 + 4 * kq + r;
      const long rowc = min(row, B - 1);
      const bool live = row < B;
      const float* sp = stash + (rowc * S + t) * kStashFields * H + u;
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

  float dh_rec[4] = {0.f, 0.f, 0.f, 0.f}, dc_rec[4] = {0.f, 0.f, 0.f, 0.f};

  for (int t = S - 1; t >= 0; --t) {
    float* dg = dg_s + (t & 1) * kTlRows * LD;
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
      g_pre = tile_slice_load(gouts, tid, t - 2, row0, B, S, D);
    __syncthreads();

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
      const int row = row0 + 4 * kq + r;
      if (row < B)
        dxb[((long)row * S + t) * H + u] = relu_on[r] ? acc_x[r] : 0.0f;
    }
    // ring slot t & 1 was read before this step's barrier; step t-2 reads
    // it behind the next one
    if (pre) {
      float* gn = g_s + (t & 1) * ng;
      if (tid < ng) gn[tid] = g_pre;
      for (int e = tid + kTlThreads; e < ng; e += kTlThreads)
        gn[e] = tile_slice_load(gouts, e, t - 2, row0, B, S, D);
    }
  }
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

void seq_lstm_fwd_tile_hip(
    const at::Tensor& x, const at::Tensor& h0, const at::Tensor& c0,
    const at::Tensor& body_w, const at::Tensor& body_b,
    const at::Tensor& w_ih, const at::Tensor& w_hh, const at::Tensor& b_g,
    const at::Tensor& heads_w, const at::Tensor& heads_b, at::Tensor& outs,
    at::Tensor& hS, at::Tensor& cS, at::Tensor& stash) {
  CHECK_IN(x); CHECK_IN(outs); CHECK_IN(hS); CHECK_IN(cS); CHECK_IN(stash);
  TORCH_CHECK(x.dim() == 3, "x must be (B,S,F)");
  TORCH_CHECK(h0.dim() == 2 && c0.dim() == 2 && heads_w.dim() == 2,
              "h0/c0 must be (B,H) and heads_w (H,D)");
  const int B = x.size(0), S = x.size(1), F = x.size(2);
  const int H = h0.size(1), D = heads_w.size(1);
  TORCH_CHECK(H == 64, "fwd_tile specialized for H=64");
  TORCH_CHECK(B >= 1 && S >= 1 && F >= 1 && D >= 1,
              "fwd_tile: empty batch, sequence, input or head");
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
              "fwd_tile: weight shapes do not match (F, H, D)");
  const long N = (long)B * S;
  TORCH_CHECK(outs.numel() == N * D && hS.numel() == (long)B * H &&
                  cS.numel() == (long)B * H &&
                  stash.numel() == N * kStashFields * H,
              "fwd_tile: output shapes do not match x");
  const long lds = fwd_tile_lds_floats(F, D) * sizeof(float);
  TORCH_CHECK(lds <= kTlMaxLds, "fwd_tile needs ", lds,
              " bytes of LDS for (F, D) = (", F, ", ", D, ")");
  hipLaunchKernelGGL(
      seq_lstm_fwd_tile_kernel, dim3((B + kTlRows - 1) / kTlRows),
      dim3(kTlThreads), lds, current_stream(), x.data_ptr<float>(),
      h0.data_ptr<float>(), c0.data_ptr<float>(), body_w.data_ptr<float>(),
      body_b.data_ptr<float>(), w_ih.data_ptr<float>(),
      w_hh.data_ptr<float>(), b_g.data_ptr<float>(),
      heads_w.data_ptr<float>(), heads_b.data_ptr<float>(),
      outs.data_ptr<float>(), hS.data_ptr<float>(), cS.data_ptr<float>(),
      stash.data_ptr<float>(), B, S, F, D, (long)h0.stride(0));
  HIP_CHECK_LAST();
}

void seq_lstm_bwd_tile_hip(const at::Tensor& gouts, const at::Tensor& stash,
                           const at::Tensor& c0, const at::Tensor& w_ih,
                           const at::Tensor& w_hh, const at::Tensor& heads_w,
                           at::Tensor& dgates, at::Tensor& dxb) {
  CHECK_IN(gouts); CHECK_IN(stash); CHECK_IN(dgates); CHECK_IN(dxb);
  CHECK_IN(w_ih); CHECK_IN(w_hh); CHECK_IN(heads_w);
  TORCH_CHECK(gouts.dim() == 3, "gouts must be (B,S,D)");
  TORCH_CHECK(c0.dim() == 2 && heads_w.dim() == 2,
              "c0 must be (B,H) and heads_w (H,D)");
  const int B = gouts.size(0), S = gouts.size(1), D = gouts.size(2);
  const int H = c0.size(1);
  TORCH_CHECK(H == 64, "bwd_tile specialized for H=64");
  TORCH_CHECK(B >= 1 && S >= 1 && D >= 1,
              "bwd_tile: empty batch, sequence or head");
  CHECK_GPU(c0); CHECK_F32(c0);
  TORCH_CHECK(c0.size(0) == B && c0.stride(1) == 1,
              "c0 must be a (B,H) row view with inner stride 1");
  TORCH_CHECK(w_ih.numel() == (long)H * 4 * H &&
                  w_hh.numel() == (long)H * 4 * H && heads_w.size(0) == H &&
                  heads_w.size(1) == D,
              "bwd_tile: weight shapes do not match (H, D)");
  const long N = (long)B * S;
  TORCH_CHECK(stash.numel() == N * kStashFields * H &&
                  dgates.numel() == N * 4 * H && dxb.numel() == N * H,
              "bwd_tile: operand shapes do not match gouts");
  const long lds = bwd_tile_lds_floats(D) * sizeof(float);
  TORCH_CHECK(lds <= kTlMaxLds, "bwd_tile needs ", lds,
              " bytes of LDS for D = ", D);
  hipLaunchKernelGGL(
      seq_lstm_bwd_tile_kernel, dim3((B + kTlRows - 1) / kTlRows),
      dim3(kTlThreads), lds, current_stream(), gouts.data_ptr<float>(),
      stash.data_ptr<float>(), c0.data_ptr<float>(), w_ih.data_ptr<float>(),
      w_hh.data_ptr<float>(), heads_w.data_ptr<float>(),
      dgates.data_ptr<float>(), dxb.data_ptr<float>(), B, S, D,
      (long)c0.stride(0));
  HIP_CHECK_LAST();
}
