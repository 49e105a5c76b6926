// V-MPO cross-row middle phase over several workgroups (gfx950): a drop-in
// for vmpo_mid_kernel (vmpo_loss.hip) with nothing in LDS sized by
// BT = B·(S−1), selected by "vmpo_mid_kernel": "wide".
//
// Work split
//   The grid is G workgroups of 1024 threads (16 waves, 4 per SIMD, at most
//   one workgroup per CU: G ≤ 64 on a 256-CU part). Workgroup g owns the
//   slab of transitions [g·L, min(BT, (g+1)·L)); a slab may start and end
//   anywhere in a row.
//   1. Selection, redundantly in every workgroup. The exact K-th largest
//      advantage (K = max(1, BT/2)) needs one global decision per radix
//      digit, so splitting it would need one rendezvous per digit; reading
//      adv_g (4·BT bytes, L2-resident) G times needs none. Keys are the
//      block kernel's f2u mapping. Three passes over 11 + 11 + 10 bit digits
//      (the block kernel: four of 8 bits) into integer histograms: 2048 bins,
//      4 copies, wave w adds into copy w & 3 (advantages cluster into a few
//      bins, and same-address LDS atomics serialise). A thread loads adv_g
//      as float4, four of them in flight; up to BT = 16384 (16 keys per
//      thread) the keys stay in registers between the passes, past that each
//      pass re-reads them from L2. Thread t owns bins 2t and 2t+1 of the
//      suffix scan (shuffles inside a wave, one LDS stage across the 16).
//      Every workgroup ends with the same thresh_u, n_gt, n_eq and global
//      maximum m; K ≥ 1 puts the maximum into the top half, so m is the
//      block kernel's "max over selected".
//   2. Ties as in the block kernel: keys equal to thresh_u are taken in
//      ascending flat index until K is reached. Only when not all of them are
//      taken (n_eq > K − n_gt) does a workgroup need a rank: it counts the
//      equal keys below its slab in one more pass over [0, g·L), waiting for
//      nobody, and ranks its own by ballot + one LDS stage per 1024 elements.
//   3. Slab work, 1024 consecutive transitions at a time: the unnormalised
//      e_i = exp((adv_i − m)/eta) (0 when not selected) goes to psi_g, and
//      Z, Σ e·adv, Σ e·logp, the Huber, KL and logit-square sums are reduced
//      by wave shuffles and one LDS stage, in wave order, into six floats.
//   4. One launch, nobody waits. With G = 1 the workgroup finalises what it
//      holds. Otherwise it stores its six floats in workspace slot g, every
//      wave fences at device scope (psi_g is every thread's store), and
//      thread 0 takes a ticket with one atomicAdd. The workgroup that draws
//      the last ticket sums the slots in slab order 0, 1, 2, …, advances the
//      LCG, writes stats / g_eta / g_alpha / scalars_g[7] by the block
//      kernel's formulas, adds to norm_sq, rescales psi_g by 1/Z in one
//      float4 streaming pass and leaves the counter at 0 for the next launch
//      or graph replay. The result depends on the inputs and L only.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): 70 VGPRs
// with the keys cached, 68 without, no AGPRs, no scratch; 33264 B of static
// LDS whatever BT is: 32 KiB of histograms (reused to stage the slots for the
// ordered sum) + the reduce stages. The registers would allow 7 waves per
// SIMD; a workgroup is 16 waves, so 4 per SIMD and one workgroup per CU run.
// Measurements: profiles/vmpo_wide.md.
#include "common.h"

#include <utility>

// One scalar chain per sum, in a stated order: no packed fp32 VALU forms.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int kWThreads = 1024;
constexpr int kWWaves = kWThreads / kWave;
constexpr int kWBins = 2048;    // 11-bit digits; the last pass uses 1024
constexpr int kWCopies = 4;     // histogram copies, wave w uses w & 3
constexpr int kWRegQuads = 4;   // float4 loads in flight / cached per thread
constexpr int kWCachedMax = kWThreads * kWRegQuads * 4;  // BT kept in VGPRs
constexpr int kWMaxSlabs = 64;  // bounds the finisher's ordered sum
constexpr int kWMinSlab = 1024;  // heuristic: one element per thread
constexpr int kWSlot = 8;       // floats per workspace slot (6 used)
static_assert(kWMaxSlabs * kWSlot <= kWCopies * kWBins, "slots staged in hist");

using f32x4 = __attribute__((ext_vector_type(4))) float;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

// The functions of this file carry a target attribute (above), and a callee
// without it is not inlined into them: the HIP header wrappers (threadIdx,
// __syncthreads, __shfl_down, atomicAdd, __expf, …) would each stay a call.
// So the kernel goes to the builtins those wrappers are made of.
__device__ __forceinline__ void w_barrier() {  // __syncthreads()
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ __forceinline__ void w_fence_device() {  // __threadfence()
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "agent");
}
__device__ __forceinline__ int w_lane() {
  return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
}
// value of lane + off; the own value where that is past the wave
__device__ __forceinline__ int w_shfl_down(int v, int off) {
  const int self = w_lane();
  const int src = self + off < kWave ? self + off : self;
  return __builtin_amdgcn_ds_bpermute(src << 2, v);
}
__device__ __forceinline__ float w_shfl_down(float v, int off) {
  return __builtin_bit_cast(
      float, w_shfl_down(__builtin_bit_cast(int, v), off));
}
__device__ __forceinline__ float w_exp(float x) {  // __expf
  return __builtin_amdgcn_exp2f(0x1.715476p+0f * x);
}
__device__ __forceinline__ float w_log(float x) {  // __logf
  return __builtin_logf(x);
}

__device__ __forceinline__ float huber_w(float d) {
  const float a = __builtin_fabsf(d);
  return (a < 1.0f) ? 0.5f * d * d : a - 0.5f;
}
// the block kernel's order-preserving float -> uint mapping, and its inverse
__device__ __forceinline__ unsigned f2u_w(float f) {
  const unsigned u = __builtin_bit_cast(unsigned, f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float u2f_w(unsigned u) {
  return __builtin_bit_cast(float,
                            (u & 0x80000000u) ? (u ^ 0x80000000u) : ~u);
}

__device__ __forceinline__ float wsum_f(float v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += w_shfl_down(v, off);
  return v;
}
__device__ __forceinline__ int wsum_i(int v) {
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) v += w_shfl_down(v, off);
  return v;
}

// Keys of float4 group j of adv_g; elements past BT get key 0, which no
// finite value maps to and which every pass skips.
__device__ __forceinline__ u32x4 load_keys(const float* __restrict__ adv_g,
                                           int j, int BT) {
  u32x4 k = {0u, 0u, 0u, 0u};
  const int i0 = 4 * j;
  if (i0 + 3 < BT) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(adv_g + i0);
#pragma unroll
    for (int c = 0; c < 4; ++c) k[c] = f2u_w(v[c]);
  } else {
#pragma unroll
    for (int c = 0; c < 4; ++c)
      if (i0 + c < BT) k[c] = f2u_w(adv_g[i0 + c]);
  }
  return k;
}

// Block-wide integer sum, the same value in every thread. The second barrier
// frees stage for whoever writes it next.
__device__ __forceinline__ int block_sum_i(int v, int* stage, int tid) {
  v = wsum_i(v);
  if ((tid & (kWave - 1)) == 0) stage[tid >> 6] = v;
  w_barrier();
  int r = 0;
#pragma unroll
  for (int w = 0; w < kWWaves; ++w) r += stage[w];
  w_barrier();
  return r;
}

struct WideArgs {
  const float *mo, *behav, *logp, *lse, *adv, *td, *log_eta, *log_alpha;
  float *psi, *scalars, *g_eta, *g_alpha, *stats, *norm_sq;
  unsigned* rng_state;
  float* ws;     // (G, kWSlot) slab partials; unused with one slab
  int* tickets;  // one counter, 0 between launches
  int B, S, A, slab, nslabs;
  float cp, cv, creg, eps_eta, alpha_below, alpha_upper;
};

template <bool kCached>
__global__ __launch_bounds__(kWThreads) void vmpo_mid_wide_kernel(WideArgs a) {
  const int S = a.S, A = a.A, D = A + 1, T = S - 1;
  const int BT = a.B * T;
  const int tid = (int)__builtin_amdgcn_workitem_id_x();
  const int bid = (int)__builtin_amdgcn_workgroup_id_x();
  const int wave = tid >> 6, lane = tid & (kWave - 1);
  const int nq = (BT + 3) >> 2;  // float4 groups, the ragged last included
  const int K = BT / 2 > 0 ? BT / 2 : 1;
  const int lo = bid * a.slab;
  const int hi = lo + a.slab < BT ? lo + a.slab : BT;

  __shared__ __attribute__((aligned(16))) unsigned s_hist[kWCopies][kWBins];
  __shared__ int s_stage[kWWaves];
  __shared__ unsigned s_sel[3];
  __shared__ unsigned s_maxkey;
  __shared__ float s_red[6][kWWaves];
  __shared__ float s_tot[6];
  __shared__ float s_inv_z;
  __shared__ int s_last;

  // ---- 1. selection: thresh_u, n_gt, n_eq and the maximum, in every
  // workgroup ------------------------------------------------------------
  u32x4 keys[kWRegQuads];
  auto load_tile = [&](int j0) {
#pragma unroll
    for (int r = 0; r < kWRegQuads; ++r)
      keys[r] = load_keys(a.adv, j0 + r * kWThreads, BT);  // past nq: zeros
  };
  // f(key, flat index) over all of adv_g: from registers, or from L2 in
  // tiles of kWRegQuads float4 per thread
  auto for_keys = [&](auto&& f) {
    for (int j0 = tid; j0 < nq; j0 += kWRegQuads * kWThreads) {
      if (!kCached) load_tile(j0);
#pragma unroll
      for (int r = 0; r < kWRegQuads; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c)
          f(keys[r][c], 4 * (j0 + r * kWThreads) + c);
    }
  };
  if (kCached) load_tile(tid);  // BT ≤ kWCachedMax: the one tile there is
  if (tid == 0) s_maxkey = 0u;

  unsigned prefix = 0u;
  int above = 0, n_eq = 0;
  unsigned* hist_mine = s_hist[wave & (kWCopies - 1)];
#pragma unroll 1
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0;
    const unsigned dmask = pass == 2 ? 1023u : 2047u;
    const unsigned pmask =
        pass == 0 ? 0u : pass == 1 ? 0xFFE00000u : 0xFFFFFC00u;
    for (int e = tid; e < kWCopies * kWBins; e += kWThreads)
      (&s_hist[0][0])[e] = 0u;
    if (tid == 0) {  // kept when no bin holds the K-th key (non-finite input)
      s_sel[0] = prefix; s_sel[1] = (unsigned)above; s_sel[2] = 0u;
    }
    w_barrier();
    unsigned mx = 0u;
    for_keys([&](unsigned u, int) {
      mx = u > mx ? u : mx;
      if ((u & pmask) == prefix && u != 0u)
        __hip_atomic_fetch_add(&hist_mine[(u >> shift) & dmask], 1u,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    });
    if (pass == 0) {
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1) {
        const unsigned o = (unsigned)w_shfl_down((int)mx, off);
        mx = o > mx ? o : mx;
      }
      if (lane == 0)
        __hip_atomic_fetch_max(&s_maxkey, mx, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    w_barrier();
    // thread t owns bins 2t, 2t+1: counts with digit ≥ 2t, by suffix scan
    int c0 = 0, c1 = 0;
#pragma unroll
    for (int w = 0; w < kWCopies; ++w) {
      c0 += (int)s_hist[w][2 * tid];
      c1 += (int)s_hist[w][2 * tid + 1];
    }
    int suf = c0 + c1;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const int up = w_shfl_down(suf, off);
      if (lane + off < kWave) suf += up;
    }
    if (lane == 0) s_stage[wave] = suf;
    w_barrier();
    int ge0 = suf;
#pragma unroll
    for (int w = 0; w < kWWaves; ++w)
      if (w > wave) ge0 += s_stage[w];
    const int ge1 = ge0 - c0;  // digit ≥ 2t+1, which is also digit > 2t
    const int gt1 = ge1 - c1;
    if (above + gt1 < K && K <= above + ge1) {
      s_sel[0] = prefix | ((unsigned)(2 * tid + 1) << shift);
      s_sel[1] = (unsigned)(above + gt1);
      s_sel[2] = (unsigned)c1;
    } else if (above + ge1 < K && K <= above + ge0) {
      s_sel[0] = prefix | ((unsigned)(2 * tid) << shift);
      s_sel[1] = (unsigned)(above + ge1);
      s_sel[2] = (unsigned)c0;
    }
    w_barrier();
    prefix = s_sel[0];
    above = (int)s_sel[1];
    n_eq = (int)s_sel[2];
    w_barrier();
  }
  const unsigned thresh_u = prefix;
  const int need_eq = K - above;       // ≥ 1 for finite input
  const bool ranked = n_eq > need_eq;  // else every equal key is selected
  const float m = u2f_w(s_maxkey);
  const float eta = w_exp(*a.log_eta);

  // ---- 2. equal keys below the slab, where a rank decides ---------------
  int rank0 = 0;
  if (ranked && lo > 0) {
    int cnt = 0;
    if (kCached) {
      for_keys([&](unsigned u, int i) { cnt += (u == thresh_u && i < lo); });
    } else {  // only [0, lo) is read
      const int nql = (lo + 3) >> 2;
      for (int j0 = tid; j0 < nql; j0 += kWRegQuads * kWThreads) {
        load_tile(j0);
#pragma unroll
        for (int r = 0; r < kWRegQuads; ++r)
#pragma unroll
          for (int c = 0; c < 4; ++c)
            cnt += (keys[r][c] == thresh_u &&
                    4 * (j0 + r * kWThreads) + c < lo);
      }
    }
    rank0 = block_sum_i(cnt, s_stage, tid);
  }

  // ---- 3. the slab ------------------------------------------------------
  float z = 0.f, wa = 0.f, pl = 0.f, vl = 0.f, kl = 0.f, rg = 0.f;
  for (int c0 = lo; c0 < hi; c0 += kWThreads) {  // uniform trip count
    const int i = c0 + tid;
    const bool live = i < hi;
    const float adv = live ? a.adv[i] : 0.f;
    const unsigned u = live ? f2u_w(adv) : 0u;
    bool sel = u > thresh_u;
    if (u == thresh_u && live) sel = !ranked;
    if (ranked && rank0 < need_eq) {  // uniform: some equal key may be taken
      const unsigned long long eq =
          __builtin_amdgcn_ballot_w64(live && u == thresh_u);
      if (lane == 0) s_stage[wave] = __builtin_popcountll(eq);
      w_barrier();
      int before = rank0, all = 0;
#pragma unroll
      for (int w = 0; w < kWWaves; ++w) {
        const int n = s_stage[w];
        if (w < wave) before += n;
        all += n;
      }
      before += __builtin_popcountll(eq & ((1ull << lane) - 1ull));
      if (live && u == thresh_u) sel = before < need_eq;
      rank0 += all;
      w_barrier();
    }
    if (live) {
      const int b = i / T, t = i - b * T;
      const long si = (long)b * S + t;
      const float e = sel ? w_exp((adv - m) / eta) : 0.f;
      a.psi[i] = e;
      z += e;
      wa = __builtin_fmaf(e, adv, wa);
      pl = __builtin_fmaf(e, a.logp[si], pl);
      vl += huber_w(a.mo[si * D + A] - a.td[i]);
      const float* zb = a.behav + si * A;
      const float* zq = a.mo + si * D;
      const float lq = a.lse[si];
      float mb = zb[0];
      for (int j = 1; j < A; ++j) mb = __builtin_fmaxf(mb, zb[j]);
      float sb = 0.f;
      for (int j = 0; j < A; ++j) sb += w_exp(zb[j] - mb);
      const float lb = mb + w_log(sb);
      for (int j = 0; j < A; ++j) {
        const float lpb = zb[j] - lb;
        const float lpq = zq[j] - lq;
        kl += w_exp(lpb) * (lpb - lpq);
        rg = __builtin_fmaf(zq[j], zq[j], rg);
      }
    }
  }
  z = wsum_f(z); wa = wsum_f(wa); pl = wsum_f(pl);
  vl = wsum_f(vl); kl = wsum_f(kl); rg = wsum_f(rg);
  if (lane == 0) {
    s_red[0][wave] = z; s_red[1][wave] = wa; s_red[2][wave] = pl;
    s_red[3][wave] = vl; s_red[4][wave] = kl; s_red[5][wave] = rg;
  }
  w_barrier();
  if (tid < 6) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < kWWaves; ++w) s += s_red[tid][w];
    s_tot[tid] = s;
    if (a.nslabs > 1) a.ws[bid * kWSlot + tid] = s;
  }

  // ---- 4. ticket; the last workgroup finalises ---------------------------
  if (a.nslabs > 1) {
    // psi_g and the slot are stores of many waves: each fences its own, the
    // barrier puts them all before thread 0's ticket
    w_fence_device();
    w_barrier();
    if (tid == 0)
      s_last = __hip_atomic_fetch_add(a.tickets, 1, __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT) ==
               a.nslabs - 1;
    w_barrier();
    if (!s_last) return;
    w_fence_device();  // the other slabs' slots and psi values, before reading
    float* stage = reinterpret_cast<float*>(&s_hist[0][0]);
    for (int e = tid; e < a.nslabs * kWSlot; e += kWThreads)
      stage[e] = a.ws[e];
    w_barrier();
    if (tid < 6) {
      float s = 0.f;
      for (int g = 0; g < a.nslabs; ++g) s += stage[g * kWSlot + tid];
      s_tot[tid] = s;
    }
    if (tid == 0) *a.tickets = 0;  // ready for the next launch
  }
  w_barrier();
  if (tid == 0) {
    const unsigned st = *a.rng_state * 1664525u + 1013904223u;
    *a.rng_state = st;
    const float uni = (st >> 8) * (1.0f / 16777216.0f);
    const float eps_alpha =
        a.alpha_below + (a.alpha_upper - a.alpha_below) * uni;
    const float alpha_v = w_exp(*a.log_alpha);
    const float Z = s_tot[0], WA = s_tot[1];
    const float pl_v = -s_tot[2] / Z;
    const float vl_v = s_tot[3] / BT;
    const float kl_mean = s_tot[4] / BT;
    const float reg_v = a.creg * s_tot[5] / (BT * A);
    const float lse_sel = m / eta + w_log(Z);
    const float eta_loss =
        eta * a.eps_eta + eta * (lse_sel - w_log((float)K));
    a.stats[0] = a.cp * pl_v + a.cv * vl_v + eta_loss +
                 (alpha_v * eps_alpha) + reg_v;
    a.stats[1] = pl_v;
    a.stats[2] = vl_v;
    a.stats[3] = eta;
    a.stats[4] = alpha_v;
    a.stats[5] = kl_mean;
    const float deta =
        a.eps_eta + (lse_sel - w_log((float)K)) - (WA / Z) / eta;
    const float ge = deta * eta;
    const float ga = alpha_v * (eps_alpha - kl_mean);
    a.g_eta[0] = ge;
    a.g_alpha[0] = ga;
    a.scalars[7] = alpha_v;
    if (a.norm_sq != nullptr)
      __hip_atomic_fetch_add(a.norm_sq, ge * ge + ga * ga, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    s_inv_z = 1.0f / Z;
  }
  w_barrier();
  const float inv_z = s_inv_z;
  f32x4* psi4 = reinterpret_cast<f32x4*>(a.psi);
  for (int j = tid; j < (BT >> 2); j += kWThreads) {
    f32x4 p = psi4[j];
#pragma unroll
    for (int c = 0; c < 4; ++c) p[c] *= inv_z;
    psi4[j] = p;
  }
  for (int i = (BT & ~3) + tid; i < BT; i += kWThreads) a.psi[i] *= inv_z;
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// Slab length for BT transitions. Every workgroup repeats the selection, so
// workgroups are added only while each still has a full pass of slab work:
// no slab shorter than kWMinSlab (one transition per thread), at most
// kWMaxSlabs of them (the finisher adds the slots one after another), and at
// most one workgroup per four CUs (64 of 256 on an MI355X): the launch
// shares the chip with nothing else, but the redundant adv_g reads grow
// with G. A forced length (tests) may give any number up to kWMaxSlabs.
std::pair<int, int> wide_plan(long BT, long forced) {
  TORCH_CHECK(BT >= 1 && BT < (1L << 30) && forced >= 0,
              "vmpo_mid_wide: B*(S-1) must be in [1, 2^30)");
  long slab;
  if (forced > 0) {
    slab = std::min(forced, BT);
  } else {
    const long cus =
        at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
    long slabs = std::max(1L, std::min<long>(kWMaxSlabs, cus / 4));
    slabs = std::max(1L, std::min(slabs, BT / kWMinSlab));
    slab = (BT + slabs - 1) / slabs;
  }
  const long nslabs = (BT + slab - 1) / slab;
  TORCH_CHECK(nslabs <= kWMaxSlabs, "vmpo_mid_wide: slab ", slab, " cuts ",
              BT, " transitions into more than ", kWMaxSlabs, " slabs");
  return {(int)slab, (int)nslabs};
}

}  // namespace

// (workspace floats, int32 tickets) for one shape; slab = 0 asks the
// heuristic.
std::pair<long, long> vmpo_mid_wide_workspace(long BT, long slab) {
  const int nslabs = wide_plan(BT, slab).second;
  return {nslabs > 1 ? (long)nslabs * kWSlot : 0L, 1L};
}

void vmpo_mid_wide_hip(const at::Tensor& mo, const at::Tensor& behav,
                       const at::Tensor& logp_g, const at::Tensor& lse_g,
                       const at::Tensor& adv_g, const at::Tensor& td_g,
                       const at::Tensor& log_eta, const at::Tensor& log_alpha,
                       at::Tensor& psi_g, at::Tensor& scalars_g,
                       at::Tensor& g_eta, at::Tensor& g_alpha,
                       at::Tensor& stats,
                       const c10::optional<at::Tensor>& norm_sq,
                       at::Tensor& rng_state, long A, double cp, double cv,
                       double creg, double eps_eta, double alpha_below,
                       double alpha_upper, at::Tensor& ws, at::Tensor& tickets,
                       long slab) {
  CHECK_IN(mo); CHECK_IN(behav); CHECK_IN(logp_g); CHECK_IN(lse_g);
  CHECK_IN(adv_g); CHECK_IN(td_g); CHECK_IN(psi_g); CHECK_IN(scalars_g);
  CHECK_IN(stats); CHECK_IN(ws);
  CHECK_GPU(log_eta); CHECK_F32(log_eta); CHECK_GPU(log_alpha);
  CHECK_F32(log_alpha); CHECK_GPU(g_eta); CHECK_F32(g_eta);
  CHECK_GPU(g_alpha); CHECK_F32(g_alpha);
  TORCH_CHECK(mo.dim() == 3 && A >= 1 && mo.size(2) == A + 1 &&
                  mo.size(1) >= 2 && mo.size(0) >= 1,
              "vmpo_mid_wide: mo must be (B, S >= 2, A + 1)");
  const long B = mo.size(0), S = mo.size(1);
  const long N = B * S, BT = B * (S - 1);
  // counts and flat indices are int32 in the kernel
  TORCH_CHECK(N < (1L << 30), "vmpo_mid_wide: B*S must be below 2^30");
  const auto [slab_len, nslabs] = wide_plan(BT, slab);
  TORCH_CHECK(behav.numel() == N * A && logp_g.numel() >= N &&
                  lse_g.numel() >= N && adv_g.numel() >= BT &&
                  td_g.numel() >= BT && psi_g.numel() >= BT &&
                  scalars_g.numel() >= 8 && stats.numel() >= 6 &&
                  log_eta.numel() == 1 && log_alpha.numel() == 1 &&
                  g_eta.numel() == 1 && g_alpha.numel() == 1,
              "vmpo_mid_wide: operands do not match (B, S, A)");
  // adv_g and psi_g are read and written as float4
  TORCH_CHECK(reinterpret_cast<uintptr_t>(adv_g.data_ptr<float>()) % 16 == 0 &&
                  reinterpret_cast<uintptr_t>(psi_g.data_ptr<float>()) % 16 ==
                      0,
              "vmpo_mid_wide: adv_g and psi_g must be 16-byte aligned");
  TORCH_CHECK(nslabs == 1 || ws.numel() >= (long)nslabs * kWSlot,
              "vmpo_mid_wide: workspace needs ", nslabs * kWSlot,
              " floats (vmpo_mid_wide_workspace)");
  TORCH_CHECK(tickets.is_cuda() && tickets.is_contiguous() &&
                  tickets.scalar_type() == at::kInt && tickets.numel() >= 1,
              "vmpo_mid_wide: tickets needs one int32 counter");
  TORCH_CHECK(rng_state.is_cuda() && rng_state.scalar_type() == at::kInt &&
                  rng_state.numel() >= 1,
              "vmpo_mid_wide: rng_state must be one int32 on the GPU");
  if (norm_sq.has_value()) {
    CHECK_GPU((*norm_sq)); CHECK_F32((*norm_sq));
  }
  WideArgs a;
  a.mo = mo.data_ptr<float>();
  a.behav = behav.data_ptr<float>();
  a.logp = logp_g.data_ptr<float>();
  a.lse = lse_g.data_ptr<float>();
  a.adv = adv_g.data_ptr<float>();
  a.td = td_g.data_ptr<float>();
  a.log_eta = log_eta.data_ptr<float>();
  a.log_alpha = log_alpha.data_ptr<float>();
  a.psi = psi_g.data_ptr<float>();
  a.scalars = scalars_g.data_ptr<float>();
  a.g_eta = g_eta.data_ptr<float>();
  a.g_alpha = g_alpha.data_ptr<float>();
  a.stats = stats.data_ptr<float>();
  a.norm_sq = norm_sq.has_value() ? norm_sq->data_ptr<float>() : nullptr;
  a.rng_state = (unsigned*)rng_state.data_ptr<int>();
  a.ws = ws.data_ptr<float>();
  a.tickets = tickets.data_ptr<int>();
  a.B = (int)B; a.S = (int)S; a.A = (int)A;
  a.slab = slab_len; a.nslabs = nslabs;
  a.cp = (float)cp; a.cv = (float)cv; a.creg = (float)creg;
  a.eps_eta = (float)eps_eta;
  a.alpha_below = (float)alpha_below; a.alpha_upper = (float)alpha_upper;
  if (BT <= kWCachedMax) {
    hipLaunchKernelGGL(vmpo_mid_wide_kernel<true>, dim3(nslabs),
                       dim3(kWThreads), 0, current_stream(), a);
  } else {
    hipLaunchKernelGGL(vmpo_mid_wide_kernel<false>, dim3(nslabs),
                       dim3(kWThreads), 0, current_stream(), a);
  }
  HIP_CHECK_LAST();
}
