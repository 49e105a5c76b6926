// Split-K weight-gradient device bodies of wgrad_split_multi.hip: the work
// split and the ordered reduce of wgrad_split.hip (described at its head),
// generalised to dual-body cores. Template definitions only.
//
// wgrad_split.hip keeps its own single-body copy: built from these bodies
// its kernel came out one VGPR larger (117 + 12 AGPRs, 3 waves per SIMD
// instead of 4; profiles/sac_split.md), so it was left as it is.
//
// kDual: the core has two encoders. dxb columns [0, half) belong to body_w
// (x, F wide) and columns [half, H) to body2_w (x2, F2 wide), so the small
// units of one slab are
//   dbody_w   tiles  ceil(F/16)  × half/16        (+ dbody_b lane sums)
//   dbody2_w  tiles  ceil(F2/16) × (H-half)/16    (+ dbody2_b lane sums)
//   dheads_wᵀ tiles  ceil(D/16)  × H/16           (+ dheads_b lane sums)
// With kDual false the second list is empty and half is H.
#pragma once

#include "common.h"
#include "wgrad_body.h"

#include <algorithm>
#include <tuple>

// Built without the packed fp32 VALU forms (v_pk_add/mul/fma_f32): every sum
// here is meant to be one scalar chain in a stated order.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

using gptr_f32x4 = const __attribute__((address_space(1))) f32x4*;
// Gradient views reached through a device pointer table have lost their
// address space as well; stores through them are global stores.
using gout_f32 = __attribute__((address_space(1))) float*;

constexpr int kSpRows = 32;        // C rows per GEMM group: 2 m-tiles per wave
constexpr int kSpCols = 64;        // C columns per GEMM group: 16 per wave
constexpr int kSpChunk = 64;       // rows of one staged chunk
constexpr int kSpU = kSpChunk / 4;  // MFMA steps per chunk
constexpr int kSpLd = kSpRows + 16;  // LDS row stride in floats
constexpr int kSpGroupFloats = (kSpRows + 1) * kSpCols;  // + the db_g row
constexpr int kSpSmallFloats = 16 * 16 + 16;             // + the bias sums
constexpr int kSpSmallU = 8;       // steps in flight per wave, small units
constexpr int kSpMaxSlabs = 16;    // bounds the finisher's serial reduce
constexpr int kSpMinSlabRows = 64;  // no slab shorter than one chunk
static_assert(kSpChunk * 8 == 2 * 256, "two float4 per thread stage a chunk");

struct SplitArgs {
  const float *x, *h0, *stash, *dgates, *dxb, *gouts;
  float *dw_ih, *dw_hh, *dbody_w, *dbody_b, *db_g, *dheads_w, *dheads_b;
  float* norm_sq;  // optional
  float* ws;       // (nslabs, per_slab) partial cells; unused with one slab
  int* tickets;    // one counter per output group, 0 between launches
  int N, S, F, D, slab_rows, nslabs;
  long h0s;
  // dual-body cores only
  const float* x2;
  float *dbody2_w, *dbody2_b;
  int F2, half;
};

// Output groups of one slab: GEMM groups first, then the small units.
template <int H>
struct SplitShape {
  static constexpr int G = 4 * H;
  static constexpr int g_groups = G / kSpCols;
  static constexpr int n_gemm = (2 * H / kSpRows) * g_groups;
  static constexpr int jt = H / 16;  // tiles along the wide (H) operand
  __host__ __device__ static int n_small(int F, int D) {
    return ((F + 15) / 16 + (D + 15) / 16) * jt;
  }
  __host__ __device__ static int n_small_dual(int F, int D, int F2, int half) {
    return ((F + 15) / 16) * (half / 16) +
           ((F2 + 15) / 16) * ((H - half) / 16) + ((D + 15) / 16) * jt;
  }
  __host__ __device__ static long per_slab(int n_small_units) {
    return (long)n_gemm * kSpGroupFloats +
           (long)n_small_units * kSpSmallFloats;
  }
};

template <int H, bool kDual>
__device__ __forceinline__ int split_n_small(const SplitArgs& a) {
  if constexpr (kDual) {
    return SplitShape<H>::n_small_dual(a.F, a.D, a.F2, a.half);
  } else {
    return SplitShape<H>::n_small(a.F, a.D);
  }
}

// Small unit u: which gradient (0 dbody_w, 1 dbody2_w, 2 dheads_wᵀ) and the
// tile's origin along the narrow (q0) and the wide (j0) operand.
struct SplitUnit {
  int kind, q0, j0;
};

template <int H, bool kDual>
__device__ __forceinline__ SplitUnit split_unit(const SplitArgs& a, int u) {
  using Sh = SplitShape<H>;
  if constexpr (kDual) {
    const int jb = a.half / 16, jb2 = Sh::jt - jb;
    const int tiles1 = ((a.F + 15) / 16) * jb;
    const int tiles2 = ((a.F2 + 15) / 16) * jb2;
    if (u < tiles1) return {0, (u / jb) * 16, (u % jb) * 16};
    u -= tiles1;
    if (u < tiles2) return {1, (u / jb2) * 16, (u % jb2) * 16};
    u -= tiles2;
    return {2, (u / Sh::jt) * 16, (u % Sh::jt) * 16};
  } else {
    const int tiles1 = ((a.F + 15) / 16) * Sh::jt;
    const bool body = u < tiles1;  // dbody_w tile, else dheads_wᵀ tile
    const int v = body ? u : u - tiles1;
    return {body ? 0 : 2, (v / Sh::jt) * 16, (v % Sh::jt) * 16};
  }
}

// Where value e of output group grp lives in the gradient views; nullptr for
// padding (rows of a small tile past F, F2 or D, bias sums a unit does not
// own).
template <int H, bool kDual>
__device__ __forceinline__ gout_f32 split_dest(const SplitArgs& a, int grp,
                                               int e) {
  using Sh = SplitShape<H>;
  constexpr int G = Sh::G;
  if (grp < Sh::n_gemm) {
    const int mg = grp / Sh::g_groups, gg = grp % Sh::g_groups;
    const int row = e / kSpCols, g = gg * kSpCols + e % kSpCols;
    if (row == kSpRows) return mg == 0 ? (gout_f32)a.db_g + g : nullptr;
    const int m = mg * kSpRows + row;
    return (gout_f32)(m < H ? a.dw_ih + (long)m * G
                            : a.dw_hh + (long)(m - H) * G) + g;
  }
  const SplitUnit un = split_unit<H, kDual>(a, grp - Sh::n_gemm);
  const int q0 = un.q0, j0 = un.j0;
  const int hb = kDual ? a.half : H;  // row length of dbody_w
  if (e < 256) {
    const int q = q0 + e / 16, j = j0 + e % 16;
    if (un.kind == 0)
      return q < a.F ? (gout_f32)a.dbody_w + (long)q * hb + j : nullptr;
    if (kDual && un.kind == 1)
      return q < a.F2 ? (gout_f32)a.dbody2_w + (long)q * (H - hb) + j
                      : nullptr;
    return q < a.D ? (gout_f32)a.dheads_w + (long)j * a.D + q : nullptr;
  }
  const int i = e - 256;
  if (un.kind == 0) return q0 == 0 ? (gout_f32)a.dbody_b + j0 + i : nullptr;
  if (kDual && un.kind == 1)
    return q0 == 0 ? (gout_f32)a.dbody2_b + j0 + i : nullptr;
  return (j0 == 0 && q0 + i < a.D) ? (gout_f32)a.dheads_b + q0 + i : nullptr;
}

// One value of this workgroup's output: straight to the gradient (one slab)
// or into the workgroup's workspace cell.
template <int H, bool kDual>
__device__ __forceinline__ void split_put(const SplitArgs& a, int grp,
                                          float* cell, int e, float v,
                                          float& nrm) {
  if (a.nslabs == 1) {
    gout_f32 d = split_dest<H, kDual>(a, grp, e);
    if (d != nullptr) {
      *d = v;
      nrm = fmaf(v, v, nrm);
    }
  } else {
    cell[e] = v;
  }
}

template <int H, bool kDual>
__device__ __forceinline__ void split_gemm_block(const SplitArgs& a, int slab,
                                                 int grp, float* cell,
                                                 float* lds, float& nrm) {
  using Sh = SplitShape<H>;
  constexpr int G = Sh::G;
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
  const int i = lane & 15, k = lane >> 4;
  const int mg = grp / Sh::g_groups, gg = grp % Sh::g_groups;
  const int sel = (mg * kSpRows) / H, col0 = (mg * kSpRows) % H;
  const int n_lo = slab * a.slab_rows;
  const int n_hi = min(a.N, n_lo + a.slab_rows);
  const int nch = (n_hi - n_lo + kSpChunk - 1) / kSpChunk;
  const int srow = tid >> 3, sc4 = (tid & 7) * 4;  // staging row, float4 col
  const gptr_f32 bcol =
      (gptr_f32)a.dgates + gg * kSpCols + wave * 16 + i;

  // A row n (a live row of this slab), at this thread's staging column
  auto a_row = [&](int n) -> gptr_f32x4 {
    const float* p;
    if (sel == 0) {
      p = a.stash + (long)n * kStashFields * H;  // xb field
    } else {
      const int b = n / a.S;
      p = (n - b * a.S == 0)
              ? a.h0 + (long)b * a.h0s
              : a.stash + (long)(n - 1) * kStashFields * H + 6 * H;
    }
    return (gptr_f32x4)(p + col0 + sc4);
  };

  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  f32x4 st[2];
  float bf[2][kSpU];

  // Loads of chunk c: the two staged A float4s first, then the wave's 16
  // dgates fragments. Rows past the slab are clamped here, zeroed at use.
#define PDRL_SP_LOAD(slot, c)                                              \
  _Pragma("unroll") for (int r = 0; r < 2; ++r) {                          \
    const int n = n_lo + (c) * kSpChunk + srow + 32 * r;                   \
    st[r] = *a_row(min(n, n_hi - 1));                                      \
  }                                                                        \
  _Pragma("unroll") for (int u = 0; u < kSpU; ++u) {                       \
    const int n = n_lo + (c) * kSpChunk + 4 * u + k;                       \
    bf[slot][u] = bcol[(long)min(n, n_hi - 1) * G];                        \
  }
#define PDRL_SP_STORE(slot, c)                                             \
  _Pragma("unroll") for (int r = 0; r < 2; ++r) {                          \
    const int n = n_lo + (c) * kSpChunk + srow + 32 * r;                   \
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};                                  \
    *reinterpret_cast<f32x4*>(lds + (slot) * kSpChunk * kSpLd +            \
                              (srow + 32 * r) * kSpLd + sc4) =             \
        n < n_hi ? st[r] : z;                                              \
  }                                                                        \
  __syncthreads();
#define PDRL_SP_MFMA(slot, c)                                              \
  __builtin_amdgcn_sched_barrier(0); /* keep loads issued ahead */         \
  _Pragma("unroll") for (int u = 0; u < kSpU; ++u) {                       \
    const int n = n_lo + (c) * kSpChunk + 4 * u + k;                       \
    const float bv = n < n_hi ? bf[slot][u] : 0.f;                         \
    const float* ar = lds + (slot) * kSpChunk * kSpLd + (4 * u + k) * kSpLd; \
    bsum += bv;                                                            \
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[i], bv, acc0, 0, 0, 0); \
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ar[16 + i], bv, acc1, 0,   \
                                                0, 0);                     \
  }                                                                        \
  __builtin_amdgcn_sched_barrier(0);

  PDRL_SP_LOAD(0, 0);
  PDRL_SP_STORE(0, 0);
  // Slot 0 holds chunk c at the head of every turn. A slot's LDS buffer is
  // rewritten one barrier after its last reader: the store of chunk c+2
  // follows the barrier that ends chunk c+1's turn half.
  int c = 0;
  for (; c + 2 <= nch; c += 2) {
    PDRL_SP_LOAD(1, c + 1);
    PDRL_SP_MFMA(0, c);
    PDRL_SP_STORE(1, c + 1);
    PDRL_SP_LOAD(0, c + 2);  // past the slab: clamped, never consumed
    PDRL_SP_MFMA(1, c + 1);
    PDRL_SP_STORE(0, c + 2);
  }
  if (c < nch) {  // odd chunk count: the last one is already in slot 0
    PDRL_SP_MFMA(0, c);
  }
#undef PDRL_SP_LOAD
#undef PDRL_SP_STORE
#undef PDRL_SP_MFMA

  // C map: col = lane&15, row = (lane>>4)*4 + reg
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int e = (k * 4 + r) * kSpCols + wave * 16 + i;
    split_put<H, kDual>(a, grp, cell, e, acc0[r], nrm);
    split_put<H, kDual>(a, grp, cell, e + 16 * kSpCols, acc1[r], nrm);
  }
  // db_g: fold the four k-groups of the fragment sums, k = 0 keeps the total
  bsum += __shfl_down(bsum, 32, kWave);
  bsum += __shfl_down(bsum, 16, kWave);
  if (mg == 0 && k == 0) {
    split_put<H, kDual>(a, grp, cell, kSpRows * kSpCols + wave * 16 + i, bsum,
                        nrm);
  }
}

template <int H, bool kDual>
__device__ __forceinline__ void split_small_block(const SplitArgs& a, int slab,
                                                  int grp, float* cell,
                                                  float* lds, float& nrm) {
  using Sh = SplitShape<H>;
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
  const int i = lane & 15, k = lane >> 4;
  const SplitUnit un = split_unit<H, kDual>(a, grp - Sh::n_gemm);
  const int q0 = un.q0, j0 = un.j0;
  const bool heads = un.kind == 2;
  // narrow operand (zero-padded to 16 columns) and wide operand (H columns);
  // every candidate is read before one is chosen, so the argument block is
  // never indexed by the unit kind
  int Q = heads ? a.D : a.F;
  const float* nar = heads ? a.gouts : a.x;
  const float* wide = heads ? a.stash + 6 * H : a.dxb;
  if constexpr (kDual) {
    const int F2 = a.F2, half = a.half;
    const float* x2 = a.x2;
    if (un.kind == 1) {
      Q = F2;
      nar = x2;
      wide += half;
    }
  }
  const long sn = Q, sw = heads ? kStashFields * H : H;
  const bool qlive = q0 + i < Q;
  const gptr_f32 pn = (gptr_f32)nar + min(q0 + i, Q - 1);
  const gptr_f32 pw = (gptr_f32)wide + j0 + i;
  const int n_lo = slab * a.slab_rows;
  const int n_hi = min(a.N, n_lo + a.slab_rows);
  const int nsteps = (n_hi - n_lo + 3) / 4;

  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float asum = 0.f, bsum = 0.f;
  // wave w takes steps w, w+4, …, kSpSmallU of them in flight
  for (int s0 = wave; s0 < nsteps; s0 += 4 * kSpSmallU) {
    float av[kSpSmallU], bv[kSpSmallU];
#pragma unroll
    for (int r = 0; r < kSpSmallU; ++r) {
      const long nc = min(n_lo + 4 * (s0 + 4 * r) + k, n_hi - 1);
      av[r] = pn[nc * sn];
      bv[r] = pw[nc * sw];
    }
#pragma unroll
    for (int r = 0; r < kSpSmallU; ++r) {
      const bool live = n_lo + 4 * (s0 + 4 * r) + k < n_hi;
      const float af = (live && qlive) ? av[r] : 0.f;
      const float bf = live ? bv[r] : 0.f;
      asum += af;
      bsum += bf;
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf, acc, 0, 0, 0);
    }
  }
  // the four waves' tiles and bias sums, added in wave order
  float* mine = lds + wave * kSpSmallFloats;
#pragma unroll
  for (int r = 0; r < 4; ++r) mine[(k * 4 + r) * 16 + i] = acc[r];
  float bias = heads ? asum : bsum;
  bias += __shfl_down(bias, 32, kWave);
  bias += __shfl_down(bias, 16, kWave);
  if (k == 0) mine[256 + i] = bias;
  __syncthreads();
  for (int e = tid; e < kSpSmallFloats; e += 256) {
    const float s = ((lds[e] + lds[kSpSmallFloats + e]) +
                     lds[2 * kSpSmallFloats + e]) +
                    lds[3 * kSpSmallFloats + e];
    split_put<H, kDual>(a, grp, cell, e, s, nrm);
  }
}

// Everything workgroup (slab, grp) of one network does: its partial values,
// then — more than one slab — the ticket and, for the last arrival, the
// slab-ordered reduce of the group into the gradient views.
template <int H, bool kDual>
__device__ __forceinline__ void split_workgroup(const SplitArgs& a, int slab,
                                                int grp) {
  using Sh = SplitShape<H>;
  __shared__ __attribute__((aligned(16))) float lds[2 * kSpChunk * kSpLd];
  __shared__ float red[4];
  __shared__ int s_last;
  const long per_slab = Sh::per_slab(split_n_small<H, kDual>(a));
  const long grp_off =
      grp < Sh::n_gemm
          ? (long)grp * kSpGroupFloats
          : (long)Sh::n_gemm * kSpGroupFloats +
                (long)(grp - Sh::n_gemm) * kSpSmallFloats;
  // values the finisher sums: only m-group 0 carries the db_g row
  const int count = grp >= Sh::n_gemm        ? kSpSmallFloats
                    : grp < Sh::g_groups     ? kSpGroupFloats
                                             : kSpRows * kSpCols;
  float* cell = a.ws + slab * per_slab + grp_off;
  float nrm = 0.f;
  if (grp < Sh::n_gemm) {
    split_gemm_block<H, kDual>(a, slab, grp, cell, lds, nrm);
  } else {
    split_small_block<H, kDual>(a, slab, grp, cell, lds, nrm);
  }

  if (a.nslabs > 1) {
    // One thread fences for the workgroup, on both sides. The barrier orders
    // every thread's cell stores before thread 0's release fence and its
    // acquire fence before every thread's cell loads; fences are cumulative,
    // and a device-scope fence writes back or invalidates L2 for the whole
    // wave, so one per workgroup costs a quarter of one per wave
    // (profiles/wgrad_split.md).
    __syncthreads();
    if (threadIdx.x == 0) {
      __threadfence();  // the workgroup's cell values, visible device-wide
      s_last = atomicAdd(a.tickets + grp, 1) == a.nslabs - 1;
      if (s_last) __threadfence();  // the other slabs' cells, before reading
    }
    __syncthreads();
    if (!s_last) return;
    // Four values per thread and kSpMaxSlabs cells in flight: the loads of a
    // batch are independent, only the adds run in slab order (a sum over
    // sl = 0, 1, 2, … one cell at a time would be nslabs dependent round
    // trips). Cells past the last slab are clamped when loaded and skipped
    // when added.
    const f32x4* cells = reinterpret_cast<const f32x4*>(a.ws + grp_off);
    const long stride4 = per_slab / 4;
    for (int e4 = threadIdx.x; e4 < count / 4; e4 += 256) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
      for (int sl0 = 0; sl0 < a.nslabs; sl0 += kSpMaxSlabs) {
        f32x4 v[kSpMaxSlabs];
#pragma unroll
        for (int j = 0; j < kSpMaxSlabs; ++j)
          v[j] = cells[min(sl0 + j, a.nslabs - 1) * stride4 + e4];
#pragma unroll
        for (int j = 0; j < kSpMaxSlabs; ++j)
          if (sl0 + j < a.nslabs) s += v[j];
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        gout_f32 d = split_dest<H, kDual>(a, grp, 4 * e4 + r);
        if (d != nullptr) {
          *d = s[r];
          nrm = fmaf(s[r], s[r], nrm);
        }
      }
    }
    if (threadIdx.x == 0) a.tickets[grp] = 0;  // ready for the next launch
  }

  if (a.norm_sq != nullptr) {  // one atomic per finishing workgroup
    const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
      nrm += __shfl_down(nrm, off, kWave);
    if (lane == 0) red[wave] = nrm;
    __syncthreads();
    if (threadIdx.x == 0)
      atomicAdd(a.norm_sq, red[0] + red[1] + red[2] + red[3]);
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// Slab length for N rows of `nets` networks in one launch: about one GEMM
// workgroup per CU over all of them, at most kSpMaxSlabs slabs, none shorter
// than kSpMinSlabRows, a multiple of 4 rows.
inline int split_slab_rows(int N, int n_gemm, long forced, int nets = 1) {
  if (forced > 0) return (int)std::min<long>(forced, N);
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  int slabs = std::max(1, std::min(kSpMaxSlabs, cus / (n_gemm * nets)));
  slabs = std::max(1, std::min(slabs, N / kSpMinSlabRows));
  return ((N + slabs - 1) / slabs + 3) / 4 * 4;
}
