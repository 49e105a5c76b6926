// Split-K weight gradients for the fused SeqLSTMCore backward (gfx950).
//
// The sweep kernel (wgrad.hip) gives every wave one 16x16 tile and all
// K = B·S rows: its grid is fixed by H and its run time grows with the
// batch. Here K is cut into slabs and the grid is (slab × output group), so
// a large batch spreads over the whole chip, and nothing in LDS is sized by
// K: there is no row cap.
//
// Work split (the same for H = 32 / 64 / 128)
//   The two gate GEMMs are one: C = [xb | hprev]ᵀ · dgates, (2H × 4H).
//   GEMM group = 32 rows × 64 columns of C (8 KiB), one workgroup of 4 waves
//   per (slab, group). Wave w owns the 16 columns g0 + 16w and BOTH 16-row
//   m-tiles: 2 tiles per wave, each dgates fragment feeds 2 MFMAs
//   (v_mfma_f32_16x16x4_f32, exact fp32). The 32 A columns of a slab are
//   staged through LDS in chunks of 64 rows, double buffered, one float4 pair
//   per thread per chunk; the staging thread resolves the hprev address
//   (h0 at t = 0, else the previous row's h field) and does the n / S
//   division, so neither sits on the MFMA chain. Each wave streams its own
//   dgates fragments from global memory, one chunk (16 loads) ahead of the
//   chunk it multiplies: global-address-space loads into two static register
//   slots, a steady-state loop with a single exit and an odd-chunk drain, so
//   every wait is a counted vmcnt. Rows past the slab's end are clamped to
//   its last row when loaded and zeroed when consumed: a slab may start and
//   end anywhere in a sequence, and has no separate tail path.
//   db_g is the column sum of dgates: the waves of m-group 0 add up the
//   fragments they load anyway (row 32 of their group).
//   Small unit = one 16x16 MFMA tile of dbody_w = xᵀ·dxb or of
//   dheads_wᵀ = goutsᵀ·h (the narrow operand, F or D wide, zero-padded to
//   16). The 4 waves of its workgroup take every fourth 4-row step of the
//   slab and are summed through LDS in wave order; dbody_b and dheads_b are
//   the lane sums of the fragments (16 more values per unit).
//
// Traffic per launch at H = 64: dgates is read 2H/32 = 4 times by the GEMM
// groups (the sweep: 8) and the A rows 4H/64 = 4 times (the sweep: 16), all
// of it through L2. A taller group would read dgates less often, but the
// finisher below reads nslabs × group bytes on ONE CU; 8 KiB groups and at
// most 16 slabs keep that at 128 KiB and still fill 256 CUs at H = 64
// (16 groups × 16 slabs). Both numbers are tuning constants
// (profiles/wgrad_split.md).
//
// One launch, ordered reduce, nobody waits
//   With one slab every workgroup writes its values straight into the
//   gradient views. With more, it writes them to its (slab, group) cell of
//   the workspace, fences at device scope and takes a ticket (one atomicAdd
//   on the group's counter). The workgroup that draws the last ticket fences,
//   sums the group's cells in slab order 0, 1, 2, …, writes the gradients,
//   adds the group's Σx² to norm_sq (one atomic per finishing workgroup) and
//   sets the counter back to 0 for the next launch or graph replay. The
//   result depends on the inputs and the slab length only.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):
//   2 tiles per wave, 24 KiB of static LDS (2 × 64 rows × 48 floats; rows
//   padded from 32 to 48 floats so the four k-groups of an A-fragment read
//   hit different banks) + 20 B of flags (+ 224 B in the instantiation that
//   carries the stats-reduce block); H = 32 / 64 / 128 alike: 116 VGPRs +
//   12 AGPRs, 4 waves per SIMD, no scratch, no flat loads, every vmcnt wait
//   in the chunk loop counted.
#include "common.h"
#include "loss_row.h"
#include "wgrad_body.h"

#include <tuple>
#include <type_traits>

// The kernels of this file are built without the packed fp32 VALU forms
// (v_pk_add/mul/fma_f32): every sum here is meant to be one scalar chain in
// a stated order.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

using gptr_f32x4 = const __attribute__((address_space(1))) f32x4*;

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
  __host__ __device__ static long per_slab(int F, int D) {
    return (long)n_gemm * kSpGroupFloats +
           (long)n_small(F, D) * kSpSmallFloats;
  }
};

// Where value e of output group grp lives in the gradient views; nullptr for
// padding (rows of a small tile past F or D, bias sums a unit does not own).
template <int H>
__device__ __forceinline__ float* split_dest(const SplitArgs& a, int grp,
                                             int e) {
  using Sh = SplitShape<H>;
  constexpr int G = Sh::G;
  if (grp < Sh::n_gemm) {
    const int mg = grp / Sh::g_groups, gg = grp % Sh::g_groups;
    const int row = e / kSpCols, g = gg * kSpCols + e % kSpCols;
    if (row == kSpRows) return mg == 0 ? a.db_g + g : nullptr;
    const int m = mg * kSpRows + row;
    return (m < H ? a.dw_ih + (long)m * G : a.dw_hh + (long)(m - H) * G) + g;
  }
  const int u = grp - Sh::n_gemm;
  const int tiles1 = ((a.F + 15) / 16) * Sh::jt;
  const bool body = u < tiles1;  // dbody_w tile, else dheads_wᵀ tile
  const int v = body ? u : u - tiles1;
  const int q0 = (v / Sh::jt) * 16, j0 = (v % Sh::jt) * 16;
  if (e < 256) {
    const int q = q0 + e / 16, j = j0 + e % 16;
    if (body) return q < a.F ? a.dbody_w + (long)q * H + j : nullptr;
    return q < a.D ? a.dheads_w + (long)j * a.D + q : nullptr;
  }
  const int i = e - 256;
  if (body) return q0 == 0 ? a.dbody_b + j0 + i : nullptr;
  return (j0 == 0 && q0 + i < a.D) ? a.dheads_b + q0 + i : nullptr;
}

// One value of this workgroup's output: straight to the gradient (one slab)
// or into the workgroup's workspace cell.
template <int H>
__device__ __forceinline__ void split_put(const SplitArgs& a, int grp,
                                          float* cell, int e, float v,
                                          float& nrm) {
  if (a.nslabs == 1) {
    float* d = split_dest<H>(a, grp, e);
    if (d != nullptr) {
      *d = v;
      nrm = fmaf(v, v, nrm);
    }
  } else {
    cell[e] = v;
  }
}

template <int H>
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
    split_put<H>(a, grp, cell, e, acc0[r], nrm);
    split_put<H>(a, grp, cell, e + 16 * kSpCols, acc1[r], nrm);
  }
  // db_g: fold the four k-groups of the fragment sums, k = 0 keeps the total
  bsum += __shfl_down(bsum, 32, kWave);
  bsum += __shfl_down(bsum, 16, kWave);
  if (mg == 0 && k == 0) {
    split_put<H>(a, grp, cell, kSpRows * kSpCols + wave * 16 + i, bsum, nrm);
  }
}

template <int H>
__device__ __forceinline__ void split_small_block(const SplitArgs& a, int slab,
                                                  int grp, float* cell,
                                                  float* lds, float& nrm) {
  using Sh = SplitShape<H>;
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
  const int i = lane & 15, k = lane >> 4;
  const int u = grp - Sh::n_gemm;
  const int tiles1 = ((a.F + 15) / 16) * Sh::jt;
  const bool body = u < tiles1;
  const int v = body ? u : u - tiles1;
  const int q0 = (v / Sh::jt) * 16, j0 = (v % Sh::jt) * 16;
  // narrow operand (zero-padded to 16 columns) and wide operand (H columns)
  const int Q = body ? a.F : a.D;
  const long sn = Q, sw = body ? H : kStashFields * H;
  const bool qlive = q0 + i < Q;
  const gptr_f32 pn = (gptr_f32)(body ? a.x : a.gouts) + min(q0 + i, Q - 1);
  const gptr_f32 pw =
      (gptr_f32)(body ? a.dxb : a.stash + 6 * H) + j0 + i;
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
  float bias = body ? bsum : asum;
  bias += __shfl_down(bias, 32, kWave);
  bias += __shfl_down(bias, 16, kWave);
  if (k == 0) mine[256 + i] = bias;
  __syncthreads();
  for (int e = tid; e < kSpSmallFloats; e += 256) {
    const float s = ((lds[e] + lds[kSpSmallFloats + e]) +
                     lds[2 * kSpSmallFloats + e]) +
                    lds[3 * kSpSmallFloats + e];
    split_put<H>(a, grp, cell, e, s, nrm);
  }
}

template <int H, bool kReduce>
__global__ __launch_bounds__(256) void wgrad_split_kernel(
    SplitArgs a, int reduce_block, const float* __restrict__ stats_part,
    float* __restrict__ stats, int algo, int B, float cp, float cv, float ce,
    float creg) {
  if constexpr (kReduce) {  // the row step's stats-reduce block, as in wgrad.hip
    if ((int)blockIdx.x == reduce_block) {
      onpolicy_stats_reduce(stats_part, stats, algo, B, a.S, a.D, cp, cv, ce,
                            creg);
      return;
    }
  }
  using Sh = SplitShape<H>;
  __shared__ __attribute__((aligned(16))) float lds[2 * kSpChunk * kSpLd];
  __shared__ float red[4];
  __shared__ int s_last;
  const int n_groups = Sh::n_gemm + Sh::n_small(a.F, a.D);
  const int slab = (int)blockIdx.x / n_groups;
  const int grp = (int)blockIdx.x % n_groups;
  const long per_slab = Sh::per_slab(a.F, a.D);
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
    split_gemm_block<H>(a, slab, grp, cell, lds, nrm);
  } else {
    split_small_block<H>(a, slab, grp, cell, lds, nrm);
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
        float* d = split_dest<H>(a, grp, 4 * e4 + r);
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

// Slab length for N rows: about one GEMM workgroup per CU, at most
// kSpMaxSlabs slabs, none shorter than kSpMinSlabRows, a multiple of 4 rows.
int split_slab_rows(int N, int n_gemm, long forced) {
  if (forced > 0) return (int)std::min<long>(forced, N);
  const int cus = at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  int slabs = std::max(1, std::min(kSpMaxSlabs, cus / n_gemm));
  slabs = std::max(1, std::min(slabs, N / kSpMinSlabRows));
  return ((N + slabs - 1) / slabs + 3) / 4 * 4;
}

template <int H>
std::tuple<long, long, long, long> split_plan(int N, int F, int D,
                                              long slab_rows) {
  using Sh = SplitShape<H>;
  const int rows = split_slab_rows(N, Sh::n_gemm, slab_rows);
  const int nslabs = (N + rows - 1) / rows;
  const long floats = nslabs > 1 ? nslabs * Sh::per_slab(F, D) : 0;
  return {floats, Sh::n_gemm + Sh::n_small(F, D), rows, nslabs};
}

std::tuple<long, long, long, long> split_plan_h(int H, int N, int F, int D,
                                                long slab_rows) {
  TORCH_CHECK(N >= 1 && F >= 1 && D >= 1 && slab_rows >= 0,
              "wgrad_split: bad shape");
  switch (H) {
    case 32: return split_plan<32>(N, F, D, slab_rows);
    case 64: return split_plan<64>(N, F, D, slab_rows);
    case 128: return split_plan<128>(N, F, D, slab_rows);
    default: TORCH_CHECK(false, "hidden size ", H, " unsupported");
  }
}

template <int H>
void launch_wgrad_split(const SplitArgs& a, long n_groups,
                        const float* stats_part, float* stats, int algo,
                        int B, float cp, float cv, float ce, float creg) {
  const int work_blocks = a.nslabs * (int)n_groups;
  const int reduce_block = stats_part != nullptr ? work_blocks : -1;
  dim3 grid(work_blocks + (stats_part != nullptr ? 1 : 0));
  auto launch = [&](auto reduce) {
    hipLaunchKernelGGL((wgrad_split_kernel<H, decltype(reduce)::value>), grid,
                       dim3(256), 0, current_stream(), a, reduce_block,
                       stats_part, stats, algo, B, cp, cv, ce, creg);
  };
  if (stats_part != nullptr) {
    launch(std::true_type{});
  } else {
    launch(std::false_type{});
  }
  HIP_CHECK_LAST();
}

}  // namespace

// (workspace floats, ticket counters, slab rows, slabs) for one shape;
// slab_rows = 0 asks the heuristic.
std::tuple<long, long, long, long> seq_lstm_wgrad_split_plan(
    long N, long H, long F, long D, long slab_rows) {
  return split_plan_h((int)H, (int)N, (int)F, (int)D, slab_rows);
}

void seq_lstm_wgrad_split_out_hip(
    const at::Tensor& x, const at::Tensor& h0, const at::Tensor& stash,
    const at::Tensor& dgates, const at::Tensor& dxb, const at::Tensor& gouts,
    at::Tensor& dw_ih, at::Tensor& dw_hh, at::Tensor& dbody_w,
    at::Tensor& dbody_b, at::Tensor& db_g, at::Tensor& dheads_w,
    at::Tensor& dheads_b, const c10::optional<at::Tensor>& norm_sq,
    at::Tensor& workspace, at::Tensor& tickets, long slab_rows,
    const c10::optional<at::Tensor>& stats_part,
    const c10::optional<at::Tensor>& stats, long algo, long B_stats, double cp,
    double cv, double ce, double creg, const c10::optional<at::Tensor>& x2) {
  TORCH_CHECK(!x2.has_value(),
              "wgrad_split covers single-body cores only (x2 given): the "
              "dual-body critics use seq_lstm_wgrad_multi");
  CHECK_IN(x); CHECK_IN(stash); CHECK_IN(dgates);
  CHECK_IN(dxb); CHECK_IN(gouts);
  CHECK_GPU(h0); CHECK_F32(h0);
  TORCH_CHECK(x.dim() == 3 && h0.dim() == 2 && gouts.dim() == 3,
              "wgrad_split: x (B,S,F), h0 (B,H), gouts (B,S,D)");
  const int B = x.size(0), S = x.size(1), F = x.size(2);
  const int H = h0.size(1), D = gouts.size(2);
  const long N = (long)B * S;
  TORCH_CHECK(N >= 1 && N < (1L << 31) / (kStashFields * 128),
              "wgrad_split: B*S out of range");
  // the staged A rows are read as float4
  TORCH_CHECK(h0.size(0) == B && h0.stride(1) == 1 && h0.stride(0) % 4 == 0 &&
                  reinterpret_cast<uintptr_t>(h0.data_ptr<float>()) % 16 == 0,
              "wgrad_split: h0 must be (B,H), inner stride 1, rows 16-byte "
              "aligned");
  TORCH_CHECK(stash.numel() == N * kStashFields * H &&
                  dgates.numel() == N * 4 * H && dxb.numel() == N * H &&
                  gouts.numel() == N * D,
              "wgrad_split: stash/dgates/dxb/gouts do not match (B,S,H,D)");
  auto out_ok = [](const at::Tensor& t, long n) {
    return t.is_cuda() && t.is_contiguous() &&
           t.scalar_type() == at::kFloat && t.numel() == n;
  };
  TORCH_CHECK(out_ok(dw_ih, 4L * H * H) && out_ok(dw_hh, 4L * H * H) &&
                  out_ok(dbody_w, (long)F * H) && out_ok(dbody_b, H) &&
                  out_ok(db_g, 4L * H) && out_ok(dheads_w, (long)H * D) &&
                  out_ok(dheads_b, D),
              "wgrad_split: gradient views do not match (F,H,D)");
  const auto [floats, n_tickets, rows, nslabs] =
      split_plan_h(H, (int)N, F, D, slab_rows);
  TORCH_CHECK(workspace.is_cuda() && workspace.is_contiguous() &&
                  workspace.scalar_type() == at::kFloat &&
                  workspace.numel() >= floats &&
                  reinterpret_cast<uintptr_t>(workspace.data_ptr<float>()) %
                          16 == 0,
              "wgrad_split: workspace needs ", floats, " floats, 16-byte "
              "aligned (seq_lstm_wgrad_split_workspace)");
  TORCH_CHECK(tickets.is_cuda() && tickets.is_contiguous() &&
                  tickets.scalar_type() == at::kInt &&
                  tickets.numel() >= n_tickets,
              "wgrad_split: tickets needs ", n_tickets, " int32 counters");
  const float* sp = nullptr;
  float* st = nullptr;
  if (stats_part.has_value()) {
    TORCH_CHECK(stats.has_value(), "stats_part needs the stats vector");
    CHECK_IN((*stats_part)); CHECK_IN((*stats));
    TORCH_CHECK(algo >= kAlgoImpala && algo <= kAlgoPpoC,
                "the stats reduce covers IMPALA / PPO / PPO-C");
    TORCH_CHECK(B_stats == B && S >= 2 && D >= 2 &&
                    stats_part->numel() >= (long)B * 8 &&
                    stats->numel() >= 7,
                "wgrad_split: stats operands do not match (B, S, D)");
    sp = stats_part->data_ptr<float>();
    st = stats->data_ptr<float>();
  }
  if (norm_sq.has_value()) {
    CHECK_GPU((*norm_sq)); CHECK_F32((*norm_sq));
  }
  SplitArgs a;
  a.x = x.data_ptr<float>();
  a.h0 = h0.data_ptr<float>();
  a.stash = stash.data_ptr<float>();
  a.dgates = dgates.data_ptr<float>();
  a.dxb = dxb.data_ptr<float>();
  a.gouts = gouts.data_ptr<float>();
  a.dw_ih = dw_ih.data_ptr<float>();
  a.dw_hh = dw_hh.data_ptr<float>();
  a.dbody_w = dbody_w.data_ptr<float>();
  a.dbody_b = dbody_b.data_ptr<float>();
  a.db_g = db_g.data_ptr<float>();
  a.dheads_w = dheads_w.data_ptr<float>();
  a.dheads_b = dheads_b.data_ptr<float>();
  a.norm_sq = norm_sq.has_value() ? norm_sq->data_ptr<float>() : nullptr;
  a.ws = workspace.data_ptr<float>();
  a.tickets = tickets.data_ptr<int>();
  a.N = (int)N; a.S = S; a.F = F; a.D = D;
  a.slab_rows = (int)rows; a.nslabs = (int)nslabs;
  a.h0s = h0.stride(0);
  switch (H) {
    case 32:
      launch_wgrad_split<32>(a, n_tickets, sp, st, (int)algo, B, (float)cp,
                             (float)cv, (float)ce, (float)creg);
      break;
    case 64:
      launch_wgrad_split<64>(a, n_tickets, sp, st, (int)algo, B, (float)cp,
                             (float)cv, (float)ce, (float)creg);
      break;
    case 128:
      launch_wgrad_split<128>(a, n_tickets, sp, st, (int)algo, B, (float)cp,
                              (float)cv, (float)ce, (float)creg);
      break;
    default: TORCH_CHECK(false, "hidden size ", H, " unsupported");
  }
}
