// Split-K weight gradients for several networks in one launch (gfx950): the
// twin critics of the two SAC steps, dual-body cores included, and the SAC
// actor with its loss tail. The sweep kernels these replace
// (wgrad_gates_mfma_multi_kernel, sac_actor_wgrad_kernel) stage a B·S-entry
// row table in LDS and so cap the batch at 8192 rows; nothing here is sized
// by B·S.
//
// Grid: blockIdx.x = slab × output group (+ one tail block, SAC actor only),
// blockIdx.y = network. The work of a workgroup is wgrad_split.hip's, from
// the shared bodies in wgrad_split_body.h:
//   - 32×64 GEMM groups of [xb | hprev]ᵀ·dgates, two m-tiles per wave
//     (v_mfma_f32_16x16x4_f32), the A rows staged through LDS in 64-row
//     chunks, double buffered, each wave streaming its own dgates fragments
//     one chunk ahead on counted waits; db_g is the column sum of the
//     fragments already loaded;
//   - small gradients as 16×16 MFMA tiles, the four waves of a unit summed
//     in wave order. A dual-body core (kDual) has two encoder lists: dbody_w
//     over dxb columns [0, half) and dbody2_w = x2ᵀ·dxb[:, half:] over
//     columns [half, H), each with its bias as the lane sums.
//
// Operands: x, h0 and x2 are shared by all networks and arrive as kernel
// arguments. Everything per network comes from a device table with one
// 14-wide row per network, the row seq_lstm_wgrad_multi reads:
//   stash, dgates, dxb, gouts, dw_ih, dw_hh, dbody_w, dbody_b, db_g,
//   dheads_w, dheads_b, norm_sq (0: none), dbody2_w, dbody2_b.
// Network c owns workspace cells [c·nslabs·per_slab, …) and ticket counters
// [c·n_groups, …): per network and output group one counter, the reduce of
// wgrad_split.hip (last ticket sums the group's cells in slab order, writes
// the views, adds the group's Σg² to the network's norm_sq with one atomic,
// sets the counter back to 0; one slab: direct write, no ticket; nobody
// waits; one fence per workgroup on each side of the ticket). Two networks
// may name the same norm_sq, as the twin critics do.
//
// kTail (the SAC actor, one network, arguments instead of a table): one
// extra block runs sac_actor_tail, the block sac_actor_wgrad_kernel carries.
// The instantiations without it hold none of its code or LDS.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950) are listed
// in profiles/sac_split.md: no scratch, 4 waves per SIMD.
#include "common.h"
#include "sac_tail.h"
#include "wgrad_split_body.h"

#include <tuple>
#include <type_traits>

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int kTabCols = 14;

struct SacTailArgs {
  const float *stats_part, *log_alpha;
  float *g_alpha, *stats4, *alpha_norm, *clock;
  int B;
  float target_entropy, beta1, beta2;
};

template <int H, bool kDual, bool kTail>
__global__ __launch_bounds__(256, 4) void wgrad_split_multi_kernel(
    SplitArgs a, const long* __restrict__ tab, int n_groups, long net_floats,
    SacTailArgs t) {
  if constexpr (kTail) {
    if ((int)blockIdx.x == a.nslabs * n_groups) {
      sac_actor_tail(t.stats_part, t.log_alpha, t.g_alpha, t.stats4,
                     t.alpha_norm, t.clock, t.B, a.N, t.target_entropy,
                     t.beta1, t.beta2);
      return;
    }
  } else {
    const int net = blockIdx.y;
    const long* ct = tab + (long)net * kTabCols;
    a.stash = reinterpret_cast<const float*>(ct[0]);
    a.dgates = reinterpret_cast<const float*>(ct[1]);
    a.dxb = reinterpret_cast<const float*>(ct[2]);
    a.gouts = reinterpret_cast<const float*>(ct[3]);
    a.dw_ih = reinterpret_cast<float*>(ct[4]);
    a.dw_hh = reinterpret_cast<float*>(ct[5]);
    a.dbody_w = reinterpret_cast<float*>(ct[6]);
    a.dbody_b = reinterpret_cast<float*>(ct[7]);
    a.db_g = reinterpret_cast<float*>(ct[8]);
    a.dheads_w = reinterpret_cast<float*>(ct[9]);
    a.dheads_b = reinterpret_cast<float*>(ct[10]);
    a.norm_sq = reinterpret_cast<float*>(ct[11]);
    if constexpr (kDual) {
      a.dbody2_w = reinterpret_cast<float*>(ct[12]);
      a.dbody2_b = reinterpret_cast<float*>(ct[13]);
    }
    a.ws += net * net_floats;
    a.tickets += net * n_groups;
  }
  split_workgroup<H, kDual>(a, (int)blockIdx.x / n_groups,
                            (int)blockIdx.x % n_groups);
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

struct MultiPlan {
  long floats;    // workspace floats over all networks
  long tickets;   // counters over all networks
  int n_groups;   // output groups of one network
  long net_floats;  // workspace floats of one network
  int rows, nslabs;
};

// half = 0: single body. Otherwise the exact small-unit count of that half.
template <int H>
MultiPlan multi_plan(int N, int F, int F2, int D, int half, int nets,
                     long slab_rows) {
  using Sh = SplitShape<H>;
  const int n_small = half > 0 ? Sh::n_small_dual(F, D, F2, half)
                               : Sh::n_small(F, D);
  MultiPlan p;
  p.rows = split_slab_rows(N, Sh::n_gemm, slab_rows, nets);
  p.nslabs = (N + p.rows - 1) / p.rows;
  p.n_groups = Sh::n_gemm + n_small;
  p.net_floats = p.nslabs > 1 ? p.nslabs * Sh::per_slab(n_small) : 0;
  p.floats = nets * p.net_floats;
  p.tickets = (long)nets * p.n_groups;
  return p;
}

MultiPlan multi_plan_h(int H, long N, int F, int F2, int D, int half,
                       int nets, long slab_rows) {
  TORCH_CHECK(N >= 1 && N < (1L << 31) / (kStashFields * 128),
              "wgrad_split_multi: B*S out of range");
  TORCH_CHECK(F >= 1 && F2 >= 0 && D >= 1 && nets >= 1 && nets <= 65535 &&
                  slab_rows >= 0,
              "wgrad_split_multi: bad shape");
  switch (H) {
    case 32: return multi_plan<32>((int)N, F, F2, D, half, nets, slab_rows);
    case 64: return multi_plan<64>((int)N, F, F2, D, half, nets, slab_rows);
    case 128: return multi_plan<128>((int)N, F, F2, D, half, nets, slab_rows);
    default: TORCH_CHECK(false, "hidden size ", H, " unsupported");
  }
}

bool f32_dev(const at::Tensor& t) {
  return t.is_cuda() && t.is_contiguous() && t.scalar_type() == at::kFloat;
}

bool aligned16(const at::Tensor& t) {
  return reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0;
}

// Checks shared by both entry points: the shared operands, the workspace
// and the tickets. Fills the shape and workspace fields of `a`.
MultiPlan check_shared(const char* who, SplitArgs& a, const at::Tensor& x,
                       const at::Tensor& h0, long D, int nets,
                       at::Tensor& workspace, at::Tensor& tickets,
                       long slab_rows, const c10::optional<at::Tensor>& x2,
                       long F2, long half) {
  TORCH_CHECK(f32_dev(x) && x.dim() == 3, who, ": x must be (B,S,F) float32, "
              "contiguous, on the GPU");
  TORCH_CHECK(h0.is_cuda() && h0.scalar_type() == at::kFloat && h0.dim() == 2,
              who, ": h0 must be (B,H) float32 on the GPU");
  const int B = x.size(0), S = x.size(1), F = x.size(2);
  const int H = h0.size(1);
  const long N = (long)B * S;
  // the staged A rows are read as float4
  TORCH_CHECK(h0.size(0) == B && h0.stride(1) == 1 && h0.stride(0) % 4 == 0 &&
                  aligned16(h0),
              who, ": h0 must be (B,H), inner stride 1, rows 16-byte aligned");
  const bool dual = x2.has_value();
  if (dual) {
    TORCH_CHECK(f32_dev(*x2) && x2->numel() == N * F2 && F2 >= 1, who,
                ": x2 must be (B,S,F2) float32, contiguous, on the GPU");
    TORCH_CHECK(half > 0 && half < H && half % 16 == 0, who,
                ": half must be a multiple of 16 inside (0, H), got ", half);
  }
  const MultiPlan p = multi_plan_h(H, N, F, dual ? (int)F2 : 0, (int)D,
                                   dual ? (int)half : 0, nets, slab_rows);
  TORCH_CHECK(f32_dev(workspace) && workspace.numel() >= p.floats &&
                  aligned16(workspace),
              who, ": workspace needs ", p.floats,
              " floats, 16-byte aligned (seq_lstm_wgrad_split_multi_workspace)");
  TORCH_CHECK(tickets.is_cuda() && tickets.is_contiguous() &&
                  tickets.scalar_type() == at::kInt &&
                  tickets.numel() >= p.tickets,
              who, ": tickets needs ", p.tickets, " int32 counters");
  a.x = x.data_ptr<float>();
  a.h0 = h0.data_ptr<float>();
  a.h0s = h0.stride(0);
  a.x2 = dual ? x2->data_ptr<float>() : nullptr;
  a.F2 = dual ? (int)F2 : 0;
  a.half = dual ? (int)half : H;
  a.ws = workspace.data_ptr<float>();
  a.tickets = tickets.data_ptr<int>();
  a.N = (int)N; a.S = S; a.F = F; a.D = (int)D;
  a.slab_rows = p.rows; a.nslabs = p.nslabs;
  return p;
}

template <int H, bool kDual, bool kTail>
void launch_multi(const SplitArgs& a, const long* tab, const MultiPlan& p,
                  int nets, const SacTailArgs& t) {
  dim3 grid(p.nslabs * p.n_groups + (kTail ? 1 : 0), nets);
  hipLaunchKernelGGL((wgrad_split_multi_kernel<H, kDual, kTail>), grid,
                     dim3(256), 0, current_stream(), a, tab, p.n_groups,
                     p.net_floats, t);
  HIP_CHECK_LAST();
}

}  // namespace

// (workspace floats, int32 tickets) for `nets` networks. F2 = 0: single-body
// cores. The dual-body figure holds for every split of H into two halves
// (it counts max(⌈F/16⌉, ⌈F2/16⌉) encoder tiles per 16 dxb columns).
std::tuple<long, long> seq_lstm_wgrad_split_multi_workspace(
    long N, long H, long F, long F2, long D, long nets, long slab_rows) {
  const MultiPlan p = multi_plan_h((int)H, N, (int)std::max(F, F2), 0, (int)D,
                                   0, (int)nets, slab_rows);
  return {p.floats, p.tickets};
}

void seq_lstm_wgrad_split_multi_hip(
    const at::Tensor& x, const at::Tensor& h0, const at::Tensor& tab,
    long nets, long D, at::Tensor& workspace, at::Tensor& tickets,
    long slab_rows, const c10::optional<at::Tensor>& x2, long F2, long half) {
  TORCH_CHECK(tab.is_cuda() && tab.is_contiguous() &&
                  tab.scalar_type() == at::kLong && tab.dim() == 2 &&
                  tab.size(1) == kTabCols && tab.size(0) >= nets,
              "wgrad_split_multi: the table holds one 14-wide int64 row per "
              "network, on the GPU");
  SplitArgs a{};
  const MultiPlan p =
      check_shared("wgrad_split_multi", a, x, h0, D, (int)nets, workspace,
                   tickets, slab_rows, x2, F2, half);
  const long* tp = tab.data_ptr<long>();
  const int H = h0.size(1);
  const SacTailArgs none{};
#define PDRL_LAUNCH_SPM(HH)                                              \
  if (x2.has_value())                                                    \
    launch_multi<HH, true, false>(a, tp, p, (int)nets, none);            \
  else                                                                   \
    launch_multi<HH, false, false>(a, tp, p, (int)nets, none)
  switch (H) {
    case 32: PDRL_LAUNCH_SPM(32); break;
    case 64: PDRL_LAUNCH_SPM(64); break;
    case 128: PDRL_LAUNCH_SPM(128); break;
    default: TORCH_CHECK(false, "hidden size ", H, " unsupported");
  }
#undef PDRL_LAUNCH_SPM
}

void sac_actor_wgrad_split_hip(
    const at::Tensor& x, const at::Tensor& h0, const at::Tensor& stash,
    const at::Tensor& dgates, const at::Tensor& dxb, const at::Tensor& gouts,
    at::Tensor& dw_ih, at::Tensor& dw_hh, at::Tensor& dbody_w,
    at::Tensor& dbody_b, at::Tensor& db_g, at::Tensor& dheads_w,
    at::Tensor& dheads_b, const c10::optional<at::Tensor>& norm_sq,
    const at::Tensor& stats_part, const at::Tensor& log_alpha,
    at::Tensor& g_alpha, at::Tensor& stats4,
    const c10::optional<at::Tensor>& alpha_norm,
    const c10::optional<at::Tensor>& clock, double target_entropy,
    double beta1, double beta2, at::Tensor& workspace, at::Tensor& tickets,
    long slab_rows) {
  const char* who = "sac_actor_wgrad_split";
  TORCH_CHECK(gouts.dim() == 3, who, ": gouts must be (B,S,D)");
  const long D = gouts.size(2);
  SplitArgs a{};
  const MultiPlan p = check_shared(who, a, x, h0, D, 1, workspace, tickets,
                                   slab_rows, c10::nullopt, 0, 0);
  const int B = x.size(0), F = x.size(2), H = h0.size(1);
  const long N = a.N;
  TORCH_CHECK(H == 64, who, " specialized for H=64");
  TORCH_CHECK(f32_dev(stash) && f32_dev(dgates) && f32_dev(dxb) &&
                  f32_dev(gouts) && stash.numel() == N * kStashFields * H &&
                  dgates.numel() == N * 4 * H && dxb.numel() == N * H &&
                  gouts.numel() == N * D && aligned16(stash),
              who, ": stash/dgates/dxb/gouts do not match (B,S,H,D)");
  auto out_ok = [](const at::Tensor& t, long n) {
    return f32_dev(t) && t.numel() == n;
  };
  TORCH_CHECK(out_ok(dw_ih, 4L * H * H) && out_ok(dw_hh, 4L * H * H) &&
                  out_ok(dbody_w, (long)F * H) && out_ok(dbody_b, H) &&
                  out_ok(db_g, 4L * H) && out_ok(dheads_w, (long)H * D) &&
                  out_ok(dheads_b, D),
              who, ": gradient views do not match (F,H,D)");
  TORCH_CHECK(f32_dev(stats_part) && stats_part.numel() >= 2L * B &&
                  f32_dev(log_alpha) && log_alpha.numel() >= 1 &&
                  f32_dev(g_alpha) && g_alpha.numel() >= 1 &&
                  f32_dev(stats4) && stats4.numel() >= 4,
              who, ": tail operands: stats_part (B,2), log_alpha (1), "
              "g_alpha (1), stats4 (4)");
  if (norm_sq.has_value()) TORCH_CHECK(f32_dev(*norm_sq), who, ": norm_sq");
  if (alpha_norm.has_value())
    TORCH_CHECK(f32_dev(*alpha_norm), who, ": alpha_norm");
  if (clock.has_value())
    TORCH_CHECK(f32_dev(*clock) && clock->numel() >= 3, who, ": clock (3)");
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
  SacTailArgs t;
  t.stats_part = stats_part.data_ptr<float>();
  t.log_alpha = log_alpha.data_ptr<float>();
  t.g_alpha = g_alpha.data_ptr<float>();
  t.stats4 = stats4.data_ptr<float>();
  t.alpha_norm = alpha_norm.has_value() ? alpha_norm->data_ptr<float>()
                                        : nullptr;
  t.clock = clock.has_value() ? clock->data_ptr<float>() : nullptr;
  t.B = B;
  t.target_entropy = (float)target_entropy;
  t.beta1 = (float)beta1;
  t.beta2 = (float)beta2;
  launch_multi<64, false, true>(a, nullptr, p, 1, t);
}
