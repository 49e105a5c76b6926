// Launches of the row-local on-policy losses (loss_row.h) for IMPALA / PPO /
// PPO-Continuous / V-MPO.
//
// The on-policy losses are ROW-LOCAL: once a block has its row's forward
// outputs it can compute that row's policy stats, V-trace/GAE scan and
// analytic head grads with no grid barrier. The only cross-row products
// are the monitoring sums: each row stores its partials, and ONE block of
// a later launch reduces them (stream order guarantees every row's stores
// landed).
//
// Three sets of launches run the same device functions:
//   row step (H=64, IMPALA / PPO / PPO-C): seq_lstm_row_step = forward +
//                  loss phase + BPTT per row in ONE launch. BPTT for a row
//                  needs nothing from another row either, so no launch
//                  boundary is needed; the stats reduce rides one extra
//                  block of the weight-gradient launch (wgrad.hip).
//   fused pair (H=64): seq_lstm_fwd_loss = forward + loss phase per row;
//                  seq_lstm_bwd_fin  = stats reduce in block 0 (V-MPO: the
//                  row's grad emission) + BPTT per row. V-MPO runs it,
//                  because vmpo_mid between the two is cross-row; for the
//                  other algorithms it is the reference of the row step.
//   stand-alone (any H): onpolicy_loss_rows after seq_lstm_forward, then
//                  onpolicy_stats_fin (V-MPO: vmpo_mid + vmpo_grad_rows),
//                  then the ordinary seq_lstm_backward_core.
//
// Stats protocol (race-free by stream ordering, no barriers, no atomics):
//   loss phase:    block 0 zeroes norm_sq (its next writer, the wgrad
//                  kernel, runs in a LATER launch); each row block
//                  PLAIN-stores its loss partials into its own stats_part
//                  row.
//   stats reduce:  one block OF A LATER LAUNCH reduces the (B, 8) partials
//                  in parallel and writes the final stats vector — nothing
//                  to re-zero (rows are fully overwritten every step).
#include "common.h"
#include "core_rows.h"
#include "loss_row.h"

#include <vector>

namespace {

template <int H>
__global__ __launch_bounds__(4 * H) void seq_lstm_fwd_loss_kernel(
    const float* __restrict__ x, const float* __restrict__ h0,
    const float* __restrict__ c0, const float* __restrict__ body_w,
    const float* __restrict__ body_b, const float* __restrict__ w_ih,
    const float* __restrict__ w_hh, const float* __restrict__ b_g,
    const float* __restrict__ heads_w, const float* __restrict__ heads_b,
    float* __restrict__ outs, float* __restrict__ hS, float* __restrict__ cS,
    float* __restrict__ stash,
    const float* __restrict__ act, const float* __restrict__ behav,
    const float* __restrict__ rew, const float* __restrict__ fir,
    float* __restrict__ gouts, float* __restrict__ stats_part,
    float* __restrict__ norm_sq,
    float* __restrict__ vm_lse, float* __restrict__ vm_logp,
    float* __restrict__ vm_adv, float* __restrict__ vm_td,
    int algo, int B, int S, int F, int D, long h0s, float gamma, float lmbda,
    float rho_bar, float rho_min, float c_bar, float rew_scale, float cp,
    float cv, float ce, float eps_clip, float creg) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int b = blockIdx.x;
  seq_lstm_fwd_row<H>(x, h0, c0, body_w, body_b, w_ih, w_hh, b_g, heads_w,
                      heads_b, outs, hS, cS, stash, b, S, F, D, h0s,
                      smem_raw);
  __syncthreads();  // smem_raw reused by the loss phase
  onpolicy_loss_phase(algo, outs, act, behav, rew, fir, gouts, stats_part,
                      norm_sq, vm_lse, vm_logp, vm_adv, vm_td, b, B, S, D,
                      gamma, lmbda, rho_bar, rho_min, c_bar, rew_scale, cp,
                      cv, ce, eps_clip, creg, smem_raw);
}

// Stand-alone loss phase over the outputs of an ordinary seq_lstm_forward:
// one block per batch row.
__global__ __launch_bounds__(kLossThreads) void onpolicy_loss_rows_kernel(
    const float* __restrict__ outs, const float* __restrict__ act,
    const float* __restrict__ behav, const float* __restrict__ rew,
    const float* __restrict__ fir, float* __restrict__ gouts,
    float* __restrict__ stats_part, float* __restrict__ norm_sq,
    float* __restrict__ vm_lse, float* __restrict__ vm_logp,
    float* __restrict__ vm_adv, float* __restrict__ vm_td, int algo, int B,
    int S, int D, float gamma, float lmbda, float rho_bar, float rho_min,
    float c_bar, float rew_scale, float cp, float cv, float ce,
    float eps_clip, float creg) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  onpolicy_loss_phase(algo, outs, act, behav, rew, fir, gouts, stats_part,
                      norm_sq, vm_lse, vm_logp, vm_adv, vm_td, blockIdx.x, B,
                      S, D, gamma, lmbda, rho_bar, rho_min, c_bar, rew_scale,
                      cp, cv, ce, eps_clip, creg, smem_raw);
}

// Stand-alone stats reduce (IMPALA / PPO / PPO-C): ONE block.
__global__ __launch_bounds__(kLossThreads) void onpolicy_stats_fin_kernel(
    const float* __restrict__ stats_part, float* __restrict__ stats,
    int algo, int B, int S, int D, float cp, float cv, float ce,
    float creg) {
  onpolicy_stats_reduce(stats_part, stats, algo, B, S, D, cp, cv, ce, creg);
}

// Stand-alone V-MPO grad emission after vmpo_mid: one block per batch row.
__global__ __launch_bounds__(kLossThreads) void vmpo_grad_rows_kernel(
    const float* __restrict__ outs, const float* __restrict__ act,
    const float* __restrict__ behav, const float* __restrict__ vm_lse,
    const float* __restrict__ vm_psi, const float* __restrict__ vm_td,
    const float* __restrict__ vm_scalars, float* __restrict__ gouts, int B,
    int S, int D, float cp, float cv, float creg) {
  vmpo_grad_row(outs, act, behav, vm_lse, vm_psi, vm_td, vm_scalars, gouts,
                blockIdx.x, B, S, D - 1, cp, cv, creg);
}

template <int H>
__global__ __launch_bounds__(4 * H) void seq_lstm_bwd_fin_kernel(
    const float* __restrict__ gouts, const float* __restrict__ stash,
    const float* __restrict__ x, const float* __restrict__ c0,
    const float* __restrict__ body_w, const float* __restrict__ w_ih,
    const float* __restrict__ w_hh, const float* __restrict__ heads_w,
    float* __restrict__ dgates, float* __restrict__ dxb,
    float* __restrict__ stats, float* __restrict__ stats_part,
    const float* __restrict__ act, const float* __restrict__ behav,
    const float* __restrict__ vm_lse, const float* __restrict__ vm_psi,
    const float* __restrict__ vm_td, const float* __restrict__ vm_scalars,
    int algo, int B, int S, int F, int D, long h0s,
    float cp, float cv, float ce, float creg,
    const float* __restrict__ vm_outs) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  if (algo == kAlgoVmpo) {
    // V-MPO: emit this row's packed head grads from the middle kernel's
    // psi/scalars (stats already finalized there), then backward
    vmpo_grad_row(vm_outs, act, behav, vm_lse, vm_psi, vm_td, vm_scalars,
                  // gouts is written then consumed by bwd_row below
                  const_cast<float*>(gouts), blockIdx.x, B, S, D - 1, cp,
                  cv, creg);
    __syncthreads();
  } else if (blockIdx.x == 0) {
    onpolicy_stats_reduce(stats_part, stats, algo, B, S, D, cp, cv, ce,
                          creg);
    __syncthreads();  // s74 done before smem_raw phases start
  }
  seq_lstm_bwd_row<H>(gouts, nullptr, nullptr, stash, x, c0, body_w, w_ih,
                      w_hh, heads_w, nullptr, nullptr, nullptr, dgates, dxb,
                      blockIdx.x, S, F, D, h0s, smem_raw);
}

// Floats of LDS the forward phase of a row uses: xb, hs (S,H) | gates (4H) |
// hbuf, cbuf (H). The row step keeps its loss inputs behind them.
constexpr long kRowStepMaxLds = 64 * 1024;  // dynamic LDS of a launch
__host__ __device__ constexpr int fwd_row_lds_floats(int S, int H) {
  return 2 * S * H + 4 * H + 2 * H;
}
// The same with what seq_lstm_fwd_row_on<H, true> keeps behind them: the
// hoisted input projections px (S,4H) and the head weights (H,D), (D).
__host__ __device__ constexpr int fwd_row_split_lds_floats(int S, int H,
                                                           int D) {
  return fwd_row_lds_floats(S, H) + 4 * S * H + H * D + D;
}

// The whole row-local step of IMPALA / PPO / PPO-C in ONE launch: block b
// forwards its row, runs the row's loss phase and back-propagates through
// time. gouts and stash are written and read back by the same block (never
// const here); the block barriers between the phases order those accesses,
// and the same barriers free smem_raw for the next phase. The stats reduce,
// the only reader of other rows' stats_part, rides the weight-gradient launch.
//
// The loss phase runs on LDS copies of its inputs, so neither lane 0's
// serial scan nor the gradient loop waits for global memory: the row's act /
// behav / rew / fir are loaded into registers beside the weight loads at the
// top (their latency sits under the forward) and parked in LDS behind the
// forward's buffers, where the heads also leave a copy of the outs they
// store. BPTT's LDS overlays all of it once the loss phase is done.
//
// kSplit runs the forward with the input projection x·w_ih of all steps
// computed ahead of its time loop and the head weights kept in LDS
// (seq_lstm_fwd_row_on<H, true>). Same bits, more LDS; the launcher takes
// kSplit where that LDS fits a launch.
template <int H, bool kSplit>
__global__ __launch_bounds__(4 * H) void seq_lstm_row_step_kernel(
    const float* __restrict__ x, const float* __restrict__ h0,
    const float* __restrict__ c0, const float* __restrict__ body_w,
    const float* __restrict__ body_b, const float* __restrict__ w_ih,
    const float* __restrict__ w_hh, const float* __restrict__ b_g,
    const float* __restrict__ heads_w, const float* __restrict__ heads_b,
    float* __restrict__ outs, float* __restrict__ hS, float* __restrict__ cS,
    float* __restrict__ stash,
    const float* __restrict__ act, const float* __restrict__ behav,
    const float* __restrict__ rew, const float* __restrict__ fir,
    float* __restrict__ gouts, float* __restrict__ stats_part,
    float* __restrict__ norm_sq, float* __restrict__ dgates,
    float* __restrict__ dxb,
    int algo, int B, int S, int F, int D, long h0s, float gamma, float lmbda,
    float rho_bar, float rho_min, float c_bar, float rew_scale, float cp,
    float cv, float ce, float eps_clip, float creg) {
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const long sb = (long)b * S;
  const int act_per = (algo == kAlgoPpoC) ? (D - 1) / 2 : 1;
  float* s_outs =
      reinterpret_cast<float*>(smem_raw) +
      (kSplit ? fwd_row_split_lds_floats(S, H, D)
              : fwd_row_lds_floats(S, H));                      // (S,D)
  float* s_act = s_outs + S * D;                                // (S,act_per)
  float* s_behav = s_act + S * act_per;                         // (S)
  float* s_rew = s_behav + S;                                   // (S)
  float* s_fir = s_rew + S;                                     // (S)

  // one step per thread: S <= kLossThreads is checked on the host and the
  // block has 4H threads; PPO-C's S*A actions are staged by a loop below
  static_assert(4 * H >= kLossThreads, "a thread for each of a row's steps");
  float r_act = 0.f, r_behav = 0.f, r_rew = 0.f, r_fir = 0.f;
  if (tid < S) {
    if (algo != kAlgoPpoC) r_act = act[sb + tid];
    r_behav = behav[sb + tid];
    r_rew = rew[sb + tid];
    r_fir = fir[sb + tid];
  }
  seq_lstm_fwd_row_on<H, kSplit>(x, h0, c0, body_w, body_b, w_ih, w_hh, b_g,
                                 heads_w, heads_b, outs, hS, cS, stash, b, S,
                                 F, D, h0s, smem_raw, nullptr, nullptr,
                                 nullptr, 0, H, s_outs);
  if (tid < S) {
    if (algo != kAlgoPpoC) s_act[tid] = r_act;
    s_behav[tid] = r_behav;
    s_rew[tid] = r_rew;
    s_fir[tid] = r_fir;
  }
  if (algo == kAlgoPpoC) {
    for (int i = tid; i < S * act_per; i += 4 * H)
      s_act[i] = act[sb * act_per + i];
  }
  // BPTT's weight rows: their 128 registers are dead until BPTT starts and
  // the forward's 128 column registers are dead from here on, so the loads
  // go out now and their latency sits under the loss phase, which issues no
  // global load of its own to queue behind them
  float wih_row[H], whh_row[H];
  seq_lstm_bwd_load_rows<H>(w_ih, w_hh, wih_row, whh_row);
  __syncthreads();  // loss inputs parked; smem_raw's front free for the loss
  onpolicy_loss_phase</*kRowView=*/true>(
      algo, s_outs, s_act, s_behav, s_rew, s_fir, gouts, stats_part, norm_sq,
      nullptr, nullptr, nullptr, nullptr, b, B, S, D, gamma, lmbda, rho_bar,
      rho_min, c_bar, rew_scale, cp, cv, ce, eps_clip, creg, smem_raw);
  __syncthreads();  // gouts stored; smem_raw reused by BPTT
  seq_lstm_bwd_row_on<H, true>(wih_row, whh_row, gouts, nullptr, nullptr,
                               stash, x, c0, body_w, w_ih, w_hh, heads_w,
                               nullptr, nullptr, nullptr, dgates, dxb, b, S,
                               F, D, h0s, smem_raw);
}

inline float* opt_ptr(const c10::optional<at::Tensor>& t) {
  return t.has_value() ? t->data_ptr<float>() : nullptr;
}

}  // namespace

// Dynamic LDS of one row-step block: the forward's buffers with the parked
// loss inputs (outs, act, behav, rew, fir) behind them; the loss scratch
// (6*S floats) and BPTT's buffers overlay them. The parked inputs can push
// this past what the two-launch pair needs, so callers ask before they
// launch (FusedOnPolicyStep falls back to the pair).
long seq_lstm_row_step_lds_bytes(long S, long D, long algo) {
  constexpr long H = 64, G = 4 * H;
  const long act_per = (algo == kAlgoPpoC) ? (D - 1) / 2 : 1;
  const long lds_fwd =
      fwd_row_lds_floats((int)S, (int)H) + S * D + S * act_per + 3 * S;
  const long lds_loss = 6 * S;
  const long lds_bwd = S * H + G + S * H + 2 * G;
  return std::max(std::max(lds_fwd, lds_loss), lds_bwd) * (long)sizeof(float);
}

// The same for the split instantiation, whose forward keeps px (S,4H) and
// the head weights as well; the loss phase and BPTT are the same.
long seq_lstm_row_step_split_lds_bytes(long S, long D, long algo) {
  constexpr long H = 64, G = 4 * H;
  const long act_per = (algo == kAlgoPpoC) ? (D - 1) / 2 : 1;
  const long lds_fwd = fwd_row_split_lds_floats((int)S, (int)H, (int)D) +
                       S * D + S * act_per + 3 * S;
  const long lds_loss = 6 * S;
  const long lds_bwd = S * H + G + S * H + 2 * G;
  return std::max(std::max(lds_fwd, lds_loss), lds_bwd) * (long)sizeof(float);
}

// Whether seq_lstm_row_step launches the split instantiation for this shape:
// wherever its LDS fits a launch. The other instantiation's need is never
// larger, so no shape loses the row step to this.
bool seq_lstm_row_step_uses_split(long S, long D, long algo) {
  return seq_lstm_row_step_split_lds_bytes(S, D, algo) <= kRowStepMaxLds;
}

// Forward + loss + BPTT per row for IMPALA / PPO / PPO-C (V-MPO's middle
// kernel is cross-row: it keeps seq_lstm_fwd_loss → vmpo_mid →
// seq_lstm_bwd_fin). The per-row stat partials are left for the reduce block
// of seq_lstm_wgrad_out.
void seq_lstm_row_step_hip(
    const at::Tensor& x, const at::Tensor& h0, const at::Tensor& c0,
    const at::Tensor& body_w, const at::Tensor& body_b,
    const at::Tensor& w_ih, const at::Tensor& w_hh, const at::Tensor& b_g,
    const at::Tensor& heads_w, const at::Tensor& heads_b, at::Tensor& outs,
    at::Tensor& hS, at::Tensor& cS, at::Tensor& stash, const at::Tensor& act,
    const at::Tensor& behav, const at::Tensor& rew, const at::Tensor& fir,
    at::Tensor& gouts, at::Tensor& stats_part,
    const c10::optional<at::Tensor>& norm_sq, at::Tensor& dgates,
    at::Tensor& dxb, long algo, double gamma, double lmbda, double rho_bar,
    double rho_min, double c_bar, double rew_scale, double cp, double cv,
    double ce, double eps_clip, double creg) {
  CHECK_IN(x); CHECK_IN(outs); CHECK_IN(hS); CHECK_IN(cS); CHECK_IN(stash);
  CHECK_IN(act); CHECK_IN(behav); CHECK_IN(rew); CHECK_IN(fir);
  CHECK_IN(gouts); CHECK_IN(stats_part); CHECK_IN(dgates); CHECK_IN(dxb);
  TORCH_CHECK(x.dim() == 3, "x must be (B,S,F)");
  const int B = x.size(0), S = x.size(1), F = x.size(2);
  const int H = h0.size(1), D = heads_w.size(1);
  TORCH_CHECK(H == 64, "row_step specialized for H=64");
  TORCH_CHECK(algo >= kAlgoImpala && algo <= kAlgoPpoC,
              "row_step covers IMPALA / PPO / PPO-C; V-MPO's middle kernel "
              "is cross-row");
  TORCH_CHECK(S >= 2 && S <= kLossThreads,
              "row-local loss gives one thread to each step: 2 <= S <= ",
              kLossThreads);
  TORCH_CHECK(D >= (algo == kAlgoPpoC ? 3 : 2) &&
                  (algo != kAlgoPpoC || D % 2 == 1),
              "packed head width does not match the algorithm");
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
                  heads_w.numel() == (long)H * D && heads_b.numel() == D,
              "row_step: weight shapes do not match (F, H, D)");
  const long N = (long)B * S;
  const long act_per = (algo == kAlgoPpoC) ? (D - 1) / 2 : 1;
  TORCH_CHECK(outs.numel() == N * D && gouts.numel() == N * D &&
                  hS.numel() == (long)B * H && cS.numel() == (long)B * H &&
                  stash.numel() == N * kStashFields * H &&
                  dgates.numel() == N * 4 * H && dxb.numel() == N * H &&
                  act.numel() == N * act_per && behav.numel() == N &&
                  rew.numel() == N && fir.numel() == N &&
                  stats_part.numel() >= (long)B * 8,
              "row_step: operand shapes do not match x");
  constexpr int G = 4 * 64;
  const bool split = seq_lstm_row_step_uses_split(S, D, algo);
  const long lds = split ? seq_lstm_row_step_split_lds_bytes(S, D, algo)
                         : seq_lstm_row_step_lds_bytes(S, D, algo);
  TORCH_CHECK(lds <= kRowStepMaxLds, "row_step needs ", lds,
              " bytes of LDS for (S, D) = (", S, ", ", D,
              "); run seq_lstm_fwd_loss + seq_lstm_bwd_fin instead");
  const auto kernel = split ? seq_lstm_row_step_kernel<64, true>
                            : seq_lstm_row_step_kernel<64, false>;
  hipLaunchKernelGGL(
      kernel, dim3(B), dim3(G), lds, current_stream(), x.data_ptr<float>(),
      h0.data_ptr<float>(),
      c0.data_ptr<float>(), body_w.data_ptr<float>(),
      body_b.data_ptr<float>(), w_ih.data_ptr<float>(),
      w_hh.data_ptr<float>(), b_g.data_ptr<float>(),
      heads_w.data_ptr<float>(), heads_b.data_ptr<float>(),
      outs.data_ptr<float>(), hS.data_ptr<float>(), cS.data_ptr<float>(),
      stash.data_ptr<float>(), act.data_ptr<float>(),
      behav.data_ptr<float>(), rew.data_ptr<float>(), fir.data_ptr<float>(),
      gouts.data_ptr<float>(), stats_part.data_ptr<float>(),
      opt_ptr(norm_sq), dgates.data_ptr<float>(), dxb.data_ptr<float>(),
      (int)algo, B, S, F, D, (long)h0.stride(0), (float)gamma, (float)lmbda,
      (float)rho_bar, (float)rho_min, (float)c_bar, (float)rew_scale,
      (float)cp, (float)cv, (float)ce, (float)eps_clip, (float)creg);
  HIP_CHECK_LAST();
}

void seq_lstm_fwd_loss_hip(
    const at::Tensor& x, const at::Tensor& h0, const at::Tensor& c0,
    const at::Tensor& body_w, const at::Tensor& body_b,
    const at::Tensor& w_ih, const at::Tensor& w_hh, const at::Tensor& b_g,
    const at::Tensor& heads_w, const at::Tensor& heads_b, at::Tensor& outs,
    at::Tensor& hS, at::Tensor& cS, at::Tensor& stash, const at::Tensor& act,
    const at::Tensor& behav, const at::Tensor& rew, const at::Tensor& fir,
    at::Tensor& gouts, at::Tensor& stats_part,
    const c10::optional<at::Tensor>& norm_sq, long algo, double gamma,
    double lmbda, double rho_bar, double rho_min, double c_bar,
    double rew_scale, double cp, double cv, double ce, double eps_clip,
    double creg, const c10::optional<at::Tensor>& vm_lse,
    const c10::optional<at::Tensor>& vm_logp,
    const c10::optional<at::Tensor>& vm_adv,
    const c10::optional<at::Tensor>& vm_td) {
  CHECK_IN(x);
  const int B = x.size(0), S = x.size(1), F = x.size(2);
  const int H = h0.size(1), D = heads_w.size(1);
  TORCH_CHECK(H == 64, "fwd_loss specialized for H=64");
  const int lds_fwd = (2 * S * H + 4 * H + 2 * H) * (int)sizeof(float);
  const int lds = std::max(lds_fwd, 6 * S * (int)sizeof(float));
  hipLaunchKernelGGL(
      (seq_lstm_fwd_loss_kernel<64>), dim3(B), dim3(4 * 64), lds,
      current_stream(), x.data_ptr<float>(), h0.data_ptr<float>(),
      c0.data_ptr<float>(), body_w.data_ptr<float>(),
      body_b.data_ptr<float>(), w_ih.data_ptr<float>(),
      w_hh.data_ptr<float>(), b_g.data_ptr<float>(),
      heads_w.data_ptr<float>(), heads_b.data_ptr<float>(),
      outs.data_ptr<float>(), hS.data_ptr<float>(), cS.data_ptr<float>(),
      stash.data_ptr<float>(), act.data_ptr<float>(),
      behav.data_ptr<float>(), rew.data_ptr<float>(), fir.data_ptr<float>(),
      gouts.data_ptr<float>(), stats_part.data_ptr<float>(),
      opt_ptr(norm_sq), opt_ptr(vm_lse), opt_ptr(vm_logp), opt_ptr(vm_adv),
      opt_ptr(vm_td), (int)algo,
      B, S, F, D, (long)h0.stride(0), (float)gamma, (float)lmbda,
      (float)rho_bar, (float)rho_min, (float)c_bar, (float)rew_scale,
      (float)cp, (float)cv, (float)ce, (float)eps_clip, (float)creg);
  HIP_CHECK_LAST();
}

void seq_lstm_bwd_fin_hip(
    const at::Tensor& gouts, const at::Tensor& stash, const at::Tensor& x,
    const at::Tensor& c0, const at::Tensor& body_w, const at::Tensor& w_ih,
    const at::Tensor& w_hh, const at::Tensor& heads_w, at::Tensor& dgates,
    at::Tensor& dxb, at::Tensor& stats, at::Tensor& stats_part,
    long algo, double cp, double cv, double ce,
    double creg, const c10::optional<at::Tensor>& act,
    const c10::optional<at::Tensor>& behav,
    const c10::optional<at::Tensor>& vm_lse,
    const c10::optional<at::Tensor>& vm_psi,
    const c10::optional<at::Tensor>& vm_td,
    const c10::optional<at::Tensor>& vm_scalars,
    const c10::optional<at::Tensor>& vm_outs) {
  CHECK_IN(x);
  const int B = x.size(0), S = x.size(1), F = x.size(2);
  const int H = c0.size(1), D = heads_w.size(1);
  TORCH_CHECK(H == 64, "bwd_fin specialized for H=64");
  constexpr int G = 4 * 64;
  const int lds = (S * 64 + G + S * 64 + 2 * G) * (int)sizeof(float);
  hipLaunchKernelGGL(
      (seq_lstm_bwd_fin_kernel<64>), dim3(B), dim3(G), lds, current_stream(),
      gouts.data_ptr<float>(), stash.data_ptr<float>(), x.data_ptr<float>(),
      c0.data_ptr<float>(), body_w.data_ptr<float>(),
      w_ih.data_ptr<float>(), w_hh.data_ptr<float>(),
      heads_w.data_ptr<float>(), dgates.data_ptr<float>(),
      dxb.data_ptr<float>(), stats.data_ptr<float>(),
      stats_part.data_ptr<float>(), opt_ptr(act), opt_ptr(behav),
      opt_ptr(vm_lse), opt_ptr(vm_psi), opt_ptr(vm_td), opt_ptr(vm_scalars),
      (int)algo, B, S, F, D,
      (long)c0.stride(0), (float)cp, (float)cv, (float)ce, (float)creg,
      opt_ptr(vm_outs));
  HIP_CHECK_LAST();
}

// outs (B,S,D) from seq_lstm_forward → gouts + per-row stats partials
// (V-MPO: the vm_* scratch consumed by vmpo_mid / vmpo_grad_rows).
void onpolicy_loss_rows_hip(
    const at::Tensor& outs, const at::Tensor& act, const at::Tensor& behav,
    const at::Tensor& rew, const at::Tensor& fir, at::Tensor& gouts,
    at::Tensor& stats_part, const c10::optional<at::Tensor>& norm_sq,
    long algo, double gamma, double lmbda, double rho_bar, double rho_min,
    double c_bar, double rew_scale, double cp, double cv, double ce,
    double eps_clip, double creg, const c10::optional<at::Tensor>& vm_lse,
    const c10::optional<at::Tensor>& vm_logp,
    const c10::optional<at::Tensor>& vm_adv,
    const c10::optional<at::Tensor>& vm_td) {
  CHECK_IN(outs); CHECK_IN(act); CHECK_IN(behav); CHECK_IN(rew);
  CHECK_IN(fir); CHECK_IN(gouts); CHECK_IN(stats_part);
  TORCH_CHECK(outs.dim() == 3, "outs must be (B,S,D)");
  const int B = outs.size(0), S = outs.size(1), D = outs.size(2);
  const long N = (long)B * S;
  TORCH_CHECK(S >= 2 && S <= kLossThreads,
              "row-local loss gives one thread to each step: 2 <= S <= ",
              kLossThreads);
  TORCH_CHECK(algo >= kAlgoImpala && algo <= kAlgoVmpo, "unknown algo");
  TORCH_CHECK(D >= (algo == kAlgoPpoC ? 3 : 2) &&
                  (algo != kAlgoPpoC || D % 2 == 1),
              "packed head width does not match the algorithm");
  const long act_per = (algo == kAlgoPpoC) ? (D - 1) / 2 : 1;
  TORCH_CHECK(act.numel() == N * act_per && behav.numel() == N &&
                  rew.numel() == N && fir.numel() == N &&
                  gouts.numel() == outs.numel() &&
                  stats_part.numel() >= (long)B * 8,
              "onpolicy_loss_rows: operand shapes do not match outs");
  if (algo == kAlgoVmpo) {
    TORCH_CHECK(vm_lse.has_value() && vm_logp.has_value() &&
                    vm_adv.has_value() && vm_td.has_value(),
                "V-MPO needs the vm_* scratch");
    TORCH_CHECK(vm_lse->numel() >= N && vm_logp->numel() >= N &&
                    vm_adv->numel() >= (long)B * (S - 1) &&
                    vm_td->numel() >= (long)B * (S - 1),
                "vm_* scratch too small");
  }
  hipLaunchKernelGGL(
      onpolicy_loss_rows_kernel, dim3(B), dim3(kLossThreads),
      6 * S * sizeof(float), current_stream(), outs.data_ptr<float>(),
      act.data_ptr<float>(), behav.data_ptr<float>(), rew.data_ptr<float>(),
      fir.data_ptr<float>(), gouts.data_ptr<float>(),
      stats_part.data_ptr<float>(), opt_ptr(norm_sq), opt_ptr(vm_lse),
      opt_ptr(vm_logp), opt_ptr(vm_adv), opt_ptr(vm_td), (int)algo, B, S, D,
      (float)gamma, (float)lmbda, (float)rho_bar, (float)rho_min,
      (float)c_bar, (float)rew_scale, (float)cp, (float)cv, (float)ce,
      (float)eps_clip, (float)creg);
  HIP_CHECK_LAST();
}

// (B,8) per-row partials → final stats vector (IMPALA / PPO / PPO-C).
void onpolicy_stats_fin_hip(const at::Tensor& stats_part, at::Tensor& stats,
                            long algo, long B, long S, long D, double cp,
                            double cv, double ce, double creg) {
  CHECK_IN(stats_part); CHECK_IN(stats);
  TORCH_CHECK(B >= 1 && S >= 2 && D >= 2 && stats_part.numel() >= B * 8 &&
                  stats.numel() >= 7,
              "onpolicy_stats_fin: bad shapes");
  hipLaunchKernelGGL(onpolicy_stats_fin_kernel, dim3(1), dim3(kLossThreads),
                     0, current_stream(), stats_part.data_ptr<float>(),
                     stats.data_ptr<float>(), (int)algo, (int)B, (int)S,
                     (int)D, (float)cp, (float)cv, (float)ce, (float)creg);
  HIP_CHECK_LAST();
}

// V-MPO packed head grads from vmpo_mid's psi weights and scalars.
void vmpo_grad_rows_hip(const at::Tensor& outs, const at::Tensor& act,
                        const at::Tensor& behav, const at::Tensor& vm_lse,
                        const at::Tensor& vm_psi, const at::Tensor& vm_td,
                        const at::Tensor& vm_scalars, at::Tensor& gouts,
                        double cp, double cv, double creg) {
  CHECK_IN(outs); CHECK_IN(act); CHECK_IN(behav); CHECK_IN(vm_lse);
  CHECK_IN(vm_psi); CHECK_IN(vm_td); CHECK_IN(vm_scalars); CHECK_IN(gouts);
  TORCH_CHECK(outs.dim() == 3, "outs must be (B,S,D)");
  const int B = outs.size(0), S = outs.size(1), D = outs.size(2);
  const long N = (long)B * S, BT = (long)B * (S - 1);
  TORCH_CHECK(S >= 2 && D >= 2 && act.numel() == N &&
                  behav.numel() == N * (D - 1) && vm_lse.numel() >= N &&
                  vm_psi.numel() >= BT && vm_td.numel() >= BT &&
                  vm_scalars.numel() >= 8 && gouts.numel() == outs.numel(),
              "vmpo_grad_rows: operand shapes do not match outs");
  hipLaunchKernelGGL(vmpo_grad_rows_kernel, dim3(B), dim3(kLossThreads), 0,
                     current_stream(), outs.data_ptr<float>(),
                     act.data_ptr<float>(), behav.data_ptr<float>(),
                     vm_lse.data_ptr<float>(), vm_psi.data_ptr<float>(),
                     vm_td.data_ptr<float>(), vm_scalars.data_ptr<float>(),
                     gouts.data_ptr<float>(), B, S, D, (float)cp, (float)cv,
                     (float)creg);
  HIP_CHECK_LAST();
}
