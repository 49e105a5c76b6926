// Shared weight-gradient device bodies (MFMA gate GEMMs + wave-per-element
// small grads) for wgrad.hip and sac_loss.hip. Template definitions only.
#pragma once

#include "common.h"
#include "core_rows.h"


using f32x4 = __attribute__((ext_vector_type(4))) float;

// A pointer read back from the LDS row table has lost its address space, and
// a load through it is a flat load: those return out of order, so the
// compiler waits for ALL outstanding memory operations (vmcnt(0)) at the
// first use and no prefetch survives. The rows are always global memory
// (stash or h0); saying so turns the loads into global loads with counted
// in-order waits.
using gptr_f32 = const __attribute__((address_space(1))) float*;

// A-operand row n of the gate GEMMs: xb (sel 0) or hprev (sel 1).
template <int H>
__device__ __forceinline__ const float* gate_a_row(const float* stash,
                                                   const float* h0, int n,
                                                   int S, int sel, long h0s) {
  if (sel == 0) {
    return stash + (long)n * kStashFields * H;  // xb field
  }
  const int t = n % S;
  if (t == 0) {
    return h0 + (long)(n / S) * h0s;
  }
  return stash + (long)(n - 1) * kStashFields * H + 6 * H;  // h field
}

// Flat 1-D block index → the (bx, by) pair the tile mapping below is written
// in: [0, 2·gemm_blocks) are the GEMM tiles of sel 0 then sel 1, everything
// after that is a small-grad block (by == 0). No block is dispatched idle.
template <int H>
__device__ __forceinline__ void wgrad_flat_block(int bid, int& bx, int& by) {
  constexpr int gemm_blocks = (H / 16) * (4 * H / kWave);
  if (bid < 2 * gemm_blocks) {
    by = bid / gemm_blocks;
    bx = bid % gemm_blocks;
  } else {
    by = 0;
    bx = bid - gemm_blocks;
  }
}

// Host side of the same mapping: blocks in the flat wgrad grid.
template <int H>
inline int wgrad_flat_grid(int total_small_waves) {
  constexpr int gemm_blocks = (H / 16) * (4 * H / kWave);
  return 2 * gemm_blocks + (total_small_waves * kWave + 255) / 256;
}

template <int H>
__device__ void wgrad_small_body(const float*, const float*, const float*,
                                 const float*, const float*, float*, float*,
                                 float*, float*, float*, float*, int, int,
                                 int, int, const float*, int, float*, float*,
                                 int);

// K sweep of one wave's 16x16 tile over the nchunks full chunks of 4·U rows:
// acc += A[n][m0+i] · B[n][g0+i] for n = 0 .. nchunks·4U-1, in that order on
// ONE accumulator chain (the sum is bit-identical to a plain n loop).
//
// A ring of P chunks keeps P-1 chunks of loads in flight: chunk c's MFMA
// chain runs behind the loads of chunk c+P-1. For that the waits must be
// COUNTED (vmcnt(N) for the oldest chunk only), which needs three things:
//  - global loads (gptr_f32 above): one flat load anywhere in the ring
//    makes every wait a vmcnt(0) and the pipeline collapses to load→wait;
//  - static slots: the loop is unrolled over P (runtime-indexed register
//    arrays would go to scratch);
//  - a steady-state loop with no branch around a load and a single exit, so
//    the counts the compiler derives at its head are the steady-state ones.
//    Chunks whose prefetch would run past K are peeled into a straight-line
//    drain after the loop instead.
// The row-pointer table is read one chunk ahead of its loads, so the LDS
// round trip sits under the previous chunk's MFMAs as well.
//
// Depth: a wave's vmcnt counter is 6 bits (63 operations outstanding at
// most) and a chunk is 2·U = 16 of them, so P <= 4. Measured at B·S = 640,
// once the waits are counted one chunk of look-ahead covers most of the
// latency: P = 3 beats P = 2 by 0.3 µs per step and P = 4 is slower again
// (profiles/wgrad_latency.md).
constexpr int kWgU = 8;  // MFMAs per chunk, 32 n-rows
constexpr int kWgP = 3;  // ring depth in chunks (2·U·P = 48 operand VGPRs)
static_assert(kWgP >= 2 && (kWgP - 1) * 2 * kWgU <= 63,
              "the awaited chunk must be reachable by a counted vmcnt wait");

template <int G>
__device__ __forceinline__ f32x4 wgrad_sweep(const float* const* tab,
                                             const float* __restrict__ dgates,
                                             int nchunks, int acol, int bcol,
                                             int k) {
  constexpr int U = kWgU, P = kWgP, step = 4 * U;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  if (nchunks <= 0) return acc;
  const int last = nchunks - 1;
  float a[P][U], b[P][U];
  gptr_f32 ap[U];  // A-row pointers of the NEXT chunk to load

  // `chunk` is clamped to the last one wherever it can run past the end:
  // the ring fill of a short sweep and the pointer read-ahead (a cache hit,
  // never consumed).
#define PDRL_WG_PTRS(chunk)                                                \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                          \
    ap[u] = (gptr_f32)tab[min((chunk), last) * step + 4 * u + k];          \
  }
#define PDRL_WG_LOAD(slot, chunk)                                          \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                          \
    const int n = min((chunk), last) * step + 4 * u + k;                   \
    a[slot][u] = ap[u][acol];                                              \
    b[slot][u] = dgates[(long)n * G + bcol];                               \
  }
#define PDRL_WG_MFMA(slot)                                                 \
  __builtin_amdgcn_sched_barrier(0); /* keep loads issued ahead */         \
  _Pragma("unroll") for (int u = 0; u < U; ++u) {                          \
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[slot][u], b[slot][u],     \
                                               acc, 0, 0, 0);              \
  }                                                                        \
  __builtin_amdgcn_sched_barrier(0);

  PDRL_WG_PTRS(0);
#pragma unroll
  for (int p = 0; p < P - 1; ++p) {  // fill the ring: chunks 0 .. P-2
    PDRL_WG_LOAD(p, p);
    PDRL_WG_PTRS(p + 1);
  }
  // Whole turns whose prefetches all lie inside K. Chunk c0+p sits in slot
  // p; its turn issues chunk c0+p+P-1 into the slot chunk c0+p-1 just left.
  int c0 = 0;
  for (; c0 + 2 * P - 1 <= nchunks; c0 += P) {
#pragma unroll
    for (int p = 0; p < P; ++p) {
      PDRL_WG_LOAD((p + P - 1) % P, c0 + p + P - 1);
      PDRL_WG_PTRS(c0 + p + P);
      PDRL_WG_MFMA(p);
    }
  }
  // Drain: at most 2P-2 chunks left, straight-line on the same static
  // slots; a chunk prefetches only while that stays inside K.
#pragma unroll
  for (int p = 0; p < 2 * P - 2; ++p) {
    if (c0 + p >= nchunks) break;
    if (c0 + p + P - 1 < nchunks) {
      PDRL_WG_LOAD((p + P - 1) % P, c0 + p + P - 1);
      PDRL_WG_PTRS(c0 + p + P);
    }
    PDRL_WG_MFMA(p % P);
  }
  return acc;
#undef PDRL_WG_MFMA
#undef PDRL_WG_PTRS
#undef PDRL_WG_LOAD
}

// One wave computes one 16x16 tile of C = A^T · B.
// bx → (m0, g_base); 4 waves fan out over g; by → which GEMM.
//
// One launch covers BOTH gate-GEMMs (MFMA tiles) and the small grads: the
// flat block index (wgrad_flat_block) puts the 2·gemm_blocks GEMM blocks
// first and the wave-per-element small-grad blocks after them.
template <int H>
__device__ __forceinline__ void wgrad_gates_body(
    const float* __restrict__ stash,   // (B,S,7H)
    const float* __restrict__ h0,      // (B,H)
    const float* __restrict__ dgates,  // (N,4H)
    float* __restrict__ dw_ih,         // (H,4H)
    float* __restrict__ dw_hh,         // (H,4H)
    float* __restrict__ norm_sq,       // optional ||grad||² accumulator
    const float* __restrict__ x,       // (N,F) small-grad inputs …
    const float* __restrict__ dxb,     // (N,H)
    const float* __restrict__ gouts,   // (N,D)
    float* __restrict__ dbody_w, float* __restrict__ dbody_b,
    float* __restrict__ db_g, float* __restrict__ dheads_w,
    float* __restrict__ dheads_b, int F, int D,
    int N, int S, long h0s, char* smem_raw, int bid,
    const float* __restrict__ x2 = nullptr,  // (N,F2) dual-body second input
    int F2 = 0, float* __restrict__ dbody2_w = nullptr,
    float* __restrict__ dbody2_b = nullptr, int half = H) {
  constexpr int G = 4 * H;
  const int g_blocks = G / kWave;  // 64-wide g blocks
  const int gemm_blocks = (H / 16) * g_blocks;
  int bx, by;
  wgrad_flat_block<H>(bid, bx, by);
  if (bx >= gemm_blocks) {
    wgrad_small_body<H>(x, dxb, stash, dgates, gouts, dbody_w, dbody_b, db_g,
                        dheads_w, dheads_b, norm_sq, N, F, D,
                        (bx - gemm_blocks) * (256 / kWave),
                        x2, F2, dbody2_w, dbody2_b, half);
    return;
  }
  const int wave = threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  const int m0 = (bx / g_blocks) * 16;
  const int g0 = (bx % g_blocks) * kWave + wave * 16;
  const int sel = by;
  float* out = (sel == 0) ? dw_ih : dw_hh;

  const int i = lane & 15;   // row within A frag / col within B frag
  const int k = lane >> 4;   // inner (n) offset 0..3

  // A-row pointer table, built ONCE per block: the per-row n%S / n/S integer
  // divisions in the load loop (640 of them per lane) serialized the K sweep
  // — with the table each load is ptr[n] (LDS broadcast) + one global load.
  const float** tab = reinterpret_cast<const float**>(smem_raw);
  for (int n = threadIdx.x; n < N; n += 256) {
    tab[n] = gate_a_row<H>(stash, h0, n, S, sel, h0s);
  }
  __syncthreads();

  const int step = 4 * kWgU;
  f32x4 acc = wgrad_sweep<G>(tab, dgates, N / step, m0 + i, g0 + i, k);
  for (int n0 = N - (N % step); n0 < N; n0 += 4) {  // ragged tail, zero-padded
    const bool live = (n0 + k) < N;
    const float a = live ? ((gptr_f32)tab[n0 + k])[m0 + i] : 0.f;
    const float b = live ? dgates[(long)(n0 + k) * G + g0 + i] : 0.f;
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
  }

  // C map: col = lane&15, row = (lane>>4)*4 + reg
  const int c_col = g0 + (lane & 15);
  const int c_row0 = m0 + (lane >> 4) * 4;
  float nrm = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    out[(long)(c_row0 + r) * G + c_col] = acc[r];
    nrm = fmaf(acc[r], acc[r], nrm);
  }
  if (norm_sq != nullptr) {  // block-reduce ||grad||² → one atomic per block
    __shared__ float red[4];
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
      nrm += __shfl_down(nrm, off, kWave);
    if (lane == 0) red[wave] = nrm;
    __syncthreads();
    if (threadIdx.x == 0)
      atomicAdd(norm_sq, red[0] + red[1] + red[2] + red[3]);
  }
}


constexpr int kWgSmallUnroll = 4;  // rows in flight per lane, small grads

// One wave per output element; lanes stride the K=N reduction.
// Segments: dbody_w (F*half) | dbody_b (half) | dbody2_w (F2*half2) |
//           dbody2_b (half2) | db_g (4H) | dheads_w (H*D) | dheads_b (D)
// (single body: half == H, F2 == 0 → the dual segments vanish)
template <int H>
__device__ void wgrad_small_body(
    const float* __restrict__ x,       // (N,F)
    const float* __restrict__ dxb,     // (N,H)
    const float* __restrict__ stash,   // (N,7H)
    const float* __restrict__ dgates,  // (N,4H)
    const float* __restrict__ gouts,   // (N,D)
    float* __restrict__ dbody_w, float* __restrict__ dbody_b,
    float* __restrict__ db_g, float* __restrict__ dheads_w,
    float* __restrict__ dheads_b, float* __restrict__ norm_sq,
    int N, int F, int D, int wave_base,
    const float* __restrict__ x2, int F2, float* __restrict__ dbody2_w,
    float* __restrict__ dbody2_b, int half) {
  constexpr int G = 4 * H;
  const int wave_id = wave_base + (int)threadIdx.x / kWave;
  const int lane = threadIdx.x % kWave;
  const int half2 = (x2 != nullptr) ? H - half : 0;
  const int n_fw = F * half, n_fw2 = F2 * half2, n_hw = H * D;
  const int total = n_fw + half + n_fw2 + half2 + G + n_hw + D;
  const bool live_wave = wave_id < total;

  // resolve segment
  const float *pa = nullptr, *pb = nullptr;
  long stride_a = 0, stride_b = 0;
  float* out = nullptr;
  int oi = 0;
  int e = live_wave ? wave_id : 0;
  if (!live_wave) {
    pb = dgates; stride_b = G; out = nullptr;
  } else if (e < n_fw) {  // dbody_w[f][j] = sum x[n][f]*dxb[n][j]
    const int f = e / half, j = e % half;
    pa = x + f; stride_a = F;
    pb = dxb + j; stride_b = H;
    out = dbody_w; oi = e;
  } else if ((e -= n_fw) < half) {  // dbody_b[j] = sum dxb[n][j]
    pb = dxb + e; stride_b = H;
    out = dbody_b; oi = e;
  } else if ((e -= half) < n_fw2) {  // dbody2_w[f][j] = sum x2[n][f]*dxb[n][half+j]
    const int f = e / half2, j = e % half2;
    pa = x2 + f; stride_a = F2;
    pb = dxb + half + j; stride_b = H;
    out = dbody2_w; oi = e;
  } else if ((e -= n_fw2) < half2) {  // dbody2_b[j] = sum dxb[n][half+j]
    pb = dxb + half + e; stride_b = H;
    out = dbody2_b; oi = e;
  } else if ((e -= half2) < G) {  // db_g[g] = sum dgates[n][g]
    pb = dgates + e; stride_b = G;
    out = db_g; oi = e;
  } else if ((e -= G) < n_hw) {  // dheads_w[k][d] = sum h[n][k]*gouts[n][d]
    const int k = e / D, d = e % D;
    pa = stash + 6 * H + k; stride_a = kStashFields * H;
    pb = gouts + d; stride_b = D;
    out = dheads_w; oi = e;
  } else {  // dheads_b[d] = sum gouts[n][d]
    e -= n_hw;
    pb = gouts + e; stride_b = D;
    out = dheads_b; oi = e;
  }

  float acc = 0.f;
  if (live_wave) {
    // R rounds of loads issue before the first dependent fmaf (one exposed
    // round trip per R rows instead of one per row); the lane's accumulation
    // order n = lane, lane+64, ... is unchanged.
    constexpr int R = kWgSmallUnroll;
    int n = lane;
    for (; n + (R - 1) * kWave < N; n += R * kWave) {
      float av[R], bv[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const long nr = n + r * kWave;
        bv[r] = pb[nr * stride_b];
        av[r] = (pa != nullptr) ? pa[nr * stride_a] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < R; ++r)
        acc = (pa != nullptr) ? fmaf(av[r], bv[r], acc) : acc + bv[r];
    }
    for (; n < N; n += kWave) {
      const float bv = pb[(long)n * stride_b];
      acc = (pa != nullptr) ? fmaf(pa[(long)n * stride_a], bv, acc) : acc + bv;
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
      acc += __shfl_down(acc, off, kWave);
    if (lane == 0) out[oi] = acc;
  }
  if (norm_sq != nullptr) {  // one atomic per block
    __shared__ float red_s[4];
    if (lane == 0) red_s[threadIdx.x / kWave] = live_wave ? acc * acc : 0.f;
    __syncthreads();
    if (threadIdx.x == 0)
      atomicAdd(norm_sq, red_s[0] + red_s[1] + red_s[2] + red_s[3]);
  }
}

