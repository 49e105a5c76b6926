// Device actor: fused policy-act + env-step rollout for CDNA4 (gfx950).
//
// One launch advances N native environments by S steps and writes the
// (N, S, ·) batch in the learner's own field layout (buffers.rollout_fields)
// straight into persistent device tensors: policy forward, categorical
// sample, log-prob, env dynamics, termination and auto-reset never leave the
// GPU. The single-call CPU counterpart is cpu_actor.cpp::act_batch_discrete;
// the eager oracle is pdrl_amd/ops/rollout.py. rollout_gaussian (below) is the
// continuous-control sibling: same geometry and recurrent part, a Gaussian
// policy (PPO-C / SAC-C sampling schemes of cpu_actor.cpp::act_batch_gaussian)
// and a float action. rollout_eval_discrete / rollout_eval_gaussian (further
// below) are the greedy evaluation kernels: whole episodes, no batch.
//
// Geometry: as seq_lstm_fwd_row (core_rows.h) — one 4H-thread workgroup per
// environment, thread = gate column with its w_ih / w_hh column resident in
// 2×H VGPRs, loaded once per launch and amortised over the S steps. The
// environments are independent, so there is no inter-workgroup traffic and
// no atomics: episode returns are written per (env, step) and reduced
// lazily by the host. obs, xb, h, c, gates and the logits head columns live
// in LDS (a few KB). The logits are a wave-0 butterfly reduction; thread 0
// then samples while wave 1 steps the dynamics for every action (lane =
// action) and draws the reset uniforms, so the two scalar chains overlap.
// Five barriers a step.
//
// Random numbers come from the stateless counter hash in rollout_rng.h,
// keyed by (seed, env, tick, lane): per-env tick counters live on device and
// are advanced by the kernel, so replays and re-launches never repeat draws.

#include "common.h"
#include "rollout_rng.h"

#include <algorithm>
#include <cstdint>

namespace {

// "No episode ended at this step" marker in ep_ret (any real return is far
// above it, negative-reward envs included).
constexpr float kNoEpisode = -1.0e30f;

// ---- native env dynamics -------------------------------------------------
// An env is a traits struct: kObsDim, kActions, reset(state, u[4]) and
// step(state, action, reward, terminated). A second env is one more struct
// and one more case in rollout_discrete_hip.

// CartPole-v1: constants and Euler update of pdrl_amd/envs/cartpole.py, fp32.
struct CartPoleDyn {
  static constexpr int kObsDim = 4;
  static constexpr int kActions = 2;

  __device__ static void reset(float* s, const float* u) {
    // explicit mul-then-add (no fma contraction): bit-exact vs the oracle
#pragma unroll
    for (int i = 0; i < kObsDim; ++i)
      s[i] = __fadd_rn(-0.05f, __fmul_rn(0.1f, u[i]));
  }

  __device__ static void step(float* s, int a, float& reward,
                              bool& terminated) {
    constexpr float kGravity = 9.8f, kMassPole = 0.1f, kTotalMass = 1.1f;
    constexpr float kLength = 0.5f, kPoleMassLength = 0.05f;
    constexpr float kForceMag = 10.0f, kTau = 0.02f;
    constexpr float kThetaThreshold = 0.20943951023931953f;  // 12 degrees
    constexpr float kXThreshold = 2.4f;
    float x = s[0], x_dot = s[1], theta = s[2], theta_dot = s[3];
    const float force = (a == 1) ? kForceMag : -kForceMag;
    const float cos_t = cosf(theta), sin_t = sinf(theta);
    const float temp =
        (force + kPoleMassLength * theta_dot * theta_dot * sin_t) / kTotalMass;
    const float theta_acc =
        (kGravity * sin_t - cos_t * temp) /
        (kLength * (4.0f / 3.0f - kMassPole * cos_t * cos_t / kTotalMass));
    const float x_acc = temp - kPoleMassLength * theta_acc * cos_t / kTotalMass;
    x = x + kTau * x_dot;
    x_dot = x_dot + kTau * x_acc;
    theta = theta + kTau * theta_dot;
    theta_dot = theta_dot + kTau * theta_acc;
    s[0] = x; s[1] = x_dot; s[2] = theta; s[3] = theta_dot;
    terminated = x < -kXThreshold || x > kXThreshold ||
                 theta < -kThetaThreshold || theta > kThetaThreshold;
    reward = 1.0f;
  }
};

// Continuous-action envs have their own traits interface: kObsDim, kActDim,
// kResetDraws (hash lanes 1..kResetDraws feed reset), drift(state) — the part
// of the update that does not depend on the action, so another wave can
// evaluate it while the policy heads are still being reduced — and
// step(state, action, drift, reward, terminated) with a float action. Only
// the sampled action is stepped (there is no "every action" to enumerate).

// MountainCarContinuous-v0: constants and update of
// pdrl_amd/envs/mountain_car.py, fp32, in the op order of the oracle
// (MountainCarContDyn in pdrl_amd/ops/rollout.py); explicit mul / add / sub so
// no fma contraction moves a trajectory across the wall or goal tests.
struct MountainCarContDyn {
  static constexpr int kObsDim = 2;
  static constexpr int kActDim = 1;
  static constexpr int kResetDraws = 1;

  __device__ static void reset(float* s, const float* u) {
    s[0] = __fadd_rn(-0.6f, __fmul_rn(0.2f, u[0]));
    s[1] = 0.0f;
  }

  __device__ static float drift(const float* s) {
    return __fmul_rn(0.0025f, cosf(__fmul_rn(3.0f, s[0])));
  }

  __device__ static void step(float* s, float a, float drift, float& reward,
                              bool& terminated) {
    const float force = fminf(fmaxf(a, -1.0f), 1.0f);
    float vel =
        __fadd_rn(s[1], __fsub_rn(__fmul_rn(force, 0.0015f), drift));
    vel = fminf(fmaxf(vel, -0.07f), 0.07f);
    const float raw = __fadd_rn(s[0], vel);
    const float pos = fminf(fmaxf(raw, -1.2f), 0.6f);
    if (pos <= -1.2f && vel < 0.0f) vel = 0.0f;
    terminated = pos >= 0.45f && vel >= 0.0f;
    reward = __fadd_rn(__fmul_rn(__fmul_rn(-0.1f, force), force),
                       terminated ? 100.0f : 0.0f);
    s[0] = pos;
    s[1] = vel;
  }
};

// Live policy weights (transposed layout, read by pointer every launch):
// what the training rollouts and the evaluation kernels have in common.
struct PolicyWeights {
  const float* body_w;   // (F, H)
  const float* body_b;   // (H)
  const float* w_ih;     // (H, 4H)
  const float* w_hh;     // (H, 4H)
  const float* b_g;      // (4H)
  const float* heads_w;  // (H, D) — columns [0, A) are the logits head
  const float* heads_b;  // (D)
};

struct RolloutArgs : PolicyWeights {
  // persistent per-env state (read and written)
  float* env_state;      // (N, F)
  float* h;              // (N, H)
  float* c;              // (N, H)
  float* is_fir;         // (N)
  int* ep_steps;         // (N)
  float* ep_run;         // (N) running episode return
  unsigned* tick;        // (N) steps taken since construction
  // outputs, (N, S, ·)
  float* obs;
  float* act;
  float* rew;
  float* logits;
  float* log_prob;
  float* is_fir_out;
  float* hx;
  float* cx;
  float* ep_ret;         // (N, S)
  int N, S, D;
  unsigned seed;
  int time_horizon, max_episode_steps;
};

// ---- recurrent part, shared by rollout_discrete and rollout_gaussian ------
// Thread tid of the 4H-thread workgroup owns gate column tid (and, for
// tid < H, body column tid). load() runs once per launch, step() once per env
// step; everything is force-inlined so the weight columns stay in the calling
// kernel's VGPRs.
template <int H, int F>
struct RecurrentCore {
  static constexpr int G = 4 * H;
  // Register-resident gate weight columns (thread = gate column tid). A
  // 4H-thread workgroup has a 256-VGPR budget per thread, which holds both
  // columns (2H values) only up to H = 64; at H = 128 the w_hh column stays
  // in registers and the w_ih column is streamed per step (coalesced,
  // L2-resident, S·H loads per thread) — no scratch in either case.
  static constexpr bool kWihRegs = H <= 64;
  static constexpr int HW = kWihRegs ? H : 4;
  float wih[HW], whh[H];
  float bias;
  float bw[F];  // body column of thread j < H (F is a handful of values)
  float bb;

  // Weight columns into registers; env n's carried h / c into LDS.
  __device__ __forceinline__ void load(const RolloutArgs& p, int tid, int n,
                                       float* s_h, float* s_c) {
    load_weights(p, tid);
    if (tid < H) {
      s_h[tid] = p.h[(long)n * H + tid];
      s_c[tid] = p.c[(long)n * H + tid];
    }
  }

  // Weight columns into registers.
  __device__ __forceinline__ void load_weights(const PolicyWeights& p,
                                               int tid) {
    if constexpr (kWihRegs) {
#pragma unroll
      for (int k = 0; k < H; ++k) wih[k] = p.w_ih[k * G + tid];
      PDRL_PIN_REGS(wih, H);
    }
#pragma unroll
    for (int k = 0; k < H; ++k) whh[k] = p.w_hh[k * G + tid];
    PDRL_PIN_REGS(whh, H);
    bias = p.b_g[tid];
    bb = 0.0f;
    if (tid < H) {
#pragma unroll
      for (int k = 0; k < F; ++k) bw[k] = p.body_w[k * H + tid];
      bb = p.body_b[tid];
    } else {
#pragma unroll
      for (int k = 0; k < F; ++k) bw[k] = 0.0f;
    }
  }

  // Record the pre-step obs / hx / cx / is_fir into output row ``row``, then
  // body GEMV + ReLU, gates, cell update. Three barriers, the last one after
  // the cell update: on return s_h / s_c hold the new recurrent state.
  __device__ __forceinline__ void step(const RolloutArgs& p, int tid, long row,
                                       const float* s_obs, const float* s_fir,
                                       float* s_xb, float* s_h, float* s_c,
                                       float* s_gates) {
    step_impl<true>(p, tid, row, s_obs, s_fir, s_xb, s_h, s_c, s_gates);
  }

  // The advance part of step() alone — nothing is recorded (evaluation).
  __device__ __forceinline__ void advance(const PolicyWeights& p, int tid,
                                          const float* s_obs, float* s_xb,
                                          float* s_h, float* s_c,
                                          float* s_gates) {
    step_impl<false>(p, tid, 0, s_obs, nullptr, s_xb, s_h, s_c, s_gates);
  }

  template <bool kRecord, typename Args>
  __device__ __forceinline__ void step_impl(const Args& p, int tid, long row,
                                            const float* s_obs,
                                            const float* s_fir, float* s_xb,
                                            float* s_h, float* s_c,
                                            float* s_gates) {
    if constexpr (kRecord) {
      if (tid < F) p.obs[row * F + tid] = s_obs[tid];
      if (tid == 0) p.is_fir_out[row] = *s_fir;
    }
    if (tid < H) {
      if constexpr (kRecord) {
        p.hx[row * H + tid] = s_h[tid];
        p.cx[row * H + tid] = s_c[tid];
      }
      float acc = bb;
#pragma unroll
      for (int k = 0; k < F; ++k) acc = fmaf(s_obs[k], bw[k], acc);
      s_xb[tid] = fmaxf(acc, 0.0f);
    }
    __syncthreads();

    // gates (b128 LDS broadcast reads against register weight columns)
    {
      const float4* xb4 = reinterpret_cast<const float4*>(s_xb);
      const float4* h4 = reinterpret_cast<const float4*>(s_h);
      float acc = bias;
      // streamed mode: re-derive the column pointer opaquely every step, or
      // the loop-invariant loads get hoisted out of the t loop into (spilt)
      // registers — the same compiler habit PDRL_PIN_REGS counters
      const float* wcol = p.w_ih + tid;
      if constexpr (!kWihRegs) asm volatile("" : "+v"(wcol));
#pragma unroll
      for (int k = 0; k < H / 4; ++k) {
        const float4 xv = xb4[k];
        if constexpr (!kWihRegs) {
#pragma unroll
          for (int j = 0; j < 4; ++j) wih[j] = wcol[(4 * k + j) * G];
        }
        const int w = kWihRegs ? 4 * k : 0;
        acc = fmaf(xv.x, wih[w], acc);
        acc = fmaf(xv.y, wih[w + 1], acc);
        acc = fmaf(xv.z, wih[w + 2], acc);
        acc = fmaf(xv.w, wih[w + 3], acc);
      }
#pragma unroll
      for (int k = 0; k < H / 4; ++k) {
        const float4 hv = h4[k];
        acc = fmaf(hv.x, whh[4 * k], acc);
        acc = fmaf(hv.y, whh[4 * k + 1], acc);
        acc = fmaf(hv.z, whh[4 * k + 2], acc);
        acc = fmaf(hv.w, whh[4 * k + 3], acc);
      }
      const int sel = tid / H;  // 0:i 1:f 2:g 3:o
      const float g = (sel == 2) ? tanhf(acc) : sigmoidf_dev(acc);
      s_gates[tid] = g;
    }
    __syncthreads();

    // cell update
    if (tid < H) {
      const float c_new =
          s_gates[H + tid] * s_c[tid] + s_gates[tid] * s_gates[2 * H + tid];
      s_c[tid] = c_new;
      s_h[tid] = s_gates[3 * H + tid] * tanhf(c_new);
    }
    __syncthreads();
  }
};

template <int H, typename Env>
__global__ __launch_bounds__(4 * H) void rollout_discrete(RolloutArgs p) {
  constexpr int G = 4 * H;
  constexpr int F = Env::kObsDim;
  constexpr int A = Env::kActions;
  const int tid = threadIdx.x;
  const int n = blockIdx.x;
  if (n >= p.N) return;  // uniform per workgroup

  __shared__ __attribute__((aligned(16))) float s_xb[H];
  __shared__ __attribute__((aligned(16))) float s_h[H];
  __shared__ __attribute__((aligned(16))) float s_c[H];
  __shared__ __attribute__((aligned(16))) float s_gates[G];
  __shared__ float s_hw[A * H];  // logits head columns, [a][k]
  __shared__ float s_obs[F];
  __shared__ float s_cand[A * F];  // next state for every action
  __shared__ float s_crew[A];
  __shared__ int s_cterm[A];
  __shared__ float s_ur[4];  // reset uniforms of this tick
  __shared__ float s_fir;
  __shared__ int s_reset;

  RecurrentCore<H, F> core;
  core.load(p, tid, n, s_h, s_c);
  float hb[A];
#pragma unroll
  for (int a = 0; a < A; ++a) hb[a] = p.heads_b[a];

  for (int idx = tid; idx < A * H; idx += G) {
    const int a = idx / H, k = idx % H;
    s_hw[idx] = p.heads_w[k * p.D + a];
  }
  if (tid < F) s_obs[tid] = p.env_state[(long)n * F + tid];

  // episode bookkeeping lives in thread 0's registers across the S steps
  int steps = 0;
  float run = 0.0f;
  unsigned tick = p.tick[n];  // every thread tracks it (hash counter)
  if (tid == 0) {
    s_fir = p.is_fir[n];
    steps = p.ep_steps[n];
    run = p.ep_run[n];
  }
  __syncthreads();

  for (int t = 0; t < p.S; ++t) {
    const long row = (long)n * p.S + t;
    tick += 1u;
    // record the pre-step obs / hx / cx / is_fir; body, gates, cell update
    core.step(p, tid, row, s_obs, &s_fir, s_xb, s_h, s_c, s_gates);

    // logits = head columns [0, A): wave 0 splits the H-long dot products
    // over its lanes and butterfly-reduces them (a serial loop in one lane
    // is ~H dependent LDS round trips — it dominated the step)
    float lg[A];
    if (tid < kWave) {
#pragma unroll
      for (int a = 0; a < A; ++a) {
        float part = 0.0f;
        for (int k = tid; k < H; k += kWave)
          part = fmaf(s_h[k], s_hw[a * H + k], part);
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1)
          part += __shfl_xor(part, off, kWave);
        lg[a] = part + hb[a];
      }
    } else if (tid < kWave + A) {
      // meanwhile wave 1 steps the dynamics for EVERY action (lane = action)
      // and draws the reset uniforms: the two single-lane scalar chains
      // (softmax/sample/log-prob vs sin/cos/divides) run side by side
      const int a = tid - kWave;
      float st[F];
#pragma unroll
      for (int k = 0; k < F; ++k) st[k] = s_obs[k];
      float reward;
      bool terminated;
      Env::step(st, a, reward, terminated);
#pragma unroll
      for (int k = 0; k < F; ++k) s_cand[a * F + k] = st[k];
      s_crew[a] = reward;
      s_cterm[a] = terminated ? 1 : 0;
    } else if (tid < kWave + A + 4) {
      const unsigned k = (unsigned)(tid - kWave - A);
      s_ur[k] = pdrl_rng::uniform(p.seed, (unsigned)n, tick, k + 1u);
    }

    // softmax, sample, log-prob (thread 0, no barrier needed: it already
    // holds the reduced logits)
    int chosen = A - 1;
    if (tid == 0) {
      float mx = lg[0];
#pragma unroll
      for (int a = 0; a < A; ++a) {
        p.logits[row * A + a] = lg[a];
        mx = fmaxf(mx, lg[a]);
      }
      float prob[A];
      float Z = 0.0f;
#pragma unroll
      for (int a = 0; a < A; ++a) {
        prob[a] = expf(lg[a] - mx);
        Z += prob[a];
      }
      // inverse CDF against one uniform (rule of cpu_actor.cpp)
      const float u = pdrl_rng::uniform(p.seed, (unsigned)n, tick, 0u);
      float cdf = 0.0f;
      bool found = false;
      float lg_chosen = lg[A - 1];
#pragma unroll
      for (int a = 0; a < A; ++a) {  // static indices: lg/prob stay in VGPRs
        cdf += prob[a] / Z;
        if (!found && u < cdf) {
          chosen = a;
          lg_chosen = lg[a];
          found = true;
        }
      }
      p.act[row] = (float)chosen;
      p.log_prob[row] = lg_chosen - mx - logf(Z);
    }
    __syncthreads();

    // pick the sampled action's outcome; termination, auto-reset (thread 0)
    if (tid == 0) {
      float st[F];
#pragma unroll
      for (int k = 0; k < F; ++k) st[k] = s_cand[chosen * F + k];
      const float reward = s_crew[chosen];
      const bool terminated = s_cterm[chosen] != 0;
      steps += 1;
      run += reward;
      p.rew[row] = reward;
      const bool done = terminated || steps >= p.max_episode_steps;
      const bool reset = done || steps >= p.time_horizon;
      p.ep_ret[row] = reset ? run : kNoEpisode;
      if (reset) {
        Env::reset(st, s_ur);
        steps = 0;
        run = 0.0f;
      }
#pragma unroll
      for (int k = 0; k < F; ++k) s_obs[k] = st[k];
      s_fir = reset ? 1.0f : 0.0f;
      s_reset = reset ? 1 : 0;
    }
    __syncthreads();
    // thread j is the only reader of s_h[j] / s_c[j] before the next barrier
    if (s_reset != 0 && tid < H) {
      s_h[tid] = 0.0f;
      s_c[tid] = 0.0f;
    }
  }

  // persist the per-env state for the next launch
  if (tid < H) {
    p.h[(long)n * H + tid] = s_h[tid];
    p.c[(long)n * H + tid] = s_c[tid];
  }
  if (tid < F) p.env_state[(long)n * F + tid] = s_obs[tid];
  if (tid == 0) {
    p.is_fir[n] = s_fir;
    p.ep_steps[n] = steps;
    p.ep_run[n] = run;
    p.tick[n] = tick;
  }
}

// ---- Gaussian policy (continuous control) ---------------------------------
struct GaussianArgs : RolloutArgs {
  float* ou_state;        // (N) persistent OU exploration state (Mode 1)
  int ou_envs;            // envs [0, ou_envs) explore with OU noise forever
  unsigned warmup_steps;  // every env explores while tick <= warmup_steps
  float ou_theta, ou_sigma;
};

// Heads: column 0 = mu, column 1 = std (Mode 0, PPO-C) or log_std (Mode 1,
// SAC-C); the ``logits`` field is [mu_raw | second_raw], ``act`` has width 1.
// Per step, after the shared recurrent part: wave 0 butterfly-reduces the two
// head columns while, in wave 1, one lane turns hash lanes 5 / 6 into the
// step's standard normal (log / sqrt / cos), one evaluates the env's
// action-independent drift and kResetDraws lanes draw the reset uniforms.
// Thread 0 does the part of the scheme's transform that needs the heads only
// before the barrier too, and after it the sample, the log-prob, the env
// step, the bookkeeping and the reset. Five barriers a step, as in
// rollout_discrete. The sampling chain uses the precise libm forms: parity
// of the sample against the oracle is what the tests measure.
template <int H, typename Env, int Mode>
__global__ __launch_bounds__(4 * H) void rollout_gaussian(GaussianArgs p) {
  // One tick has eight hash lanes: 1..4 reset, 5 / 6 the normal. A second
  // action dimension needs a wider counter (rollout_rng.h).
  static_assert(Env::kActDim == 1,
                "eight hash lanes per tick allow exactly one action dimension");
  static_assert(Env::kResetDraws >= 1 && Env::kResetDraws <= 4,
                "reset draws use hash lanes 1..4");
  static_assert(Mode == 0 || Mode == 1, "Mode: 0 = PPO-C, 1 = SAC-C");
  constexpr int G = 4 * H;
  constexpr int F = Env::kObsDim;
  constexpr int R = Env::kResetDraws;
  constexpr float kHalfLog2Pi = 0.9189385f;
  const int tid = threadIdx.x;
  const int n = blockIdx.x;
  if (n >= p.N) return;  // uniform per workgroup

  __shared__ __attribute__((aligned(16))) float s_xb[H];
  __shared__ __attribute__((aligned(16))) float s_h[H];
  __shared__ __attribute__((aligned(16))) float s_c[H];
  __shared__ __attribute__((aligned(16))) float s_gates[G];
  __shared__ float s_hw[2 * H];  // mu and std / log_std head columns, [a][k]
  __shared__ float s_obs[F];
  __shared__ float s_ur[R];  // reset uniforms of this tick
  __shared__ float s_normal;
  __shared__ float s_drift;
  __shared__ float s_fir;
  __shared__ int s_reset;

  RecurrentCore<H, F> core;
  core.load(p, tid, n, s_h, s_c);
  float hb[2];
#pragma unroll
  for (int a = 0; a < 2; ++a) hb[a] = p.heads_b[a];

  for (int idx = tid; idx < 2 * H; idx += G) {
    const int a = idx / H, k = idx % H;
    s_hw[idx] = p.heads_w[k * p.D + a];
  }
  if (tid < F) s_obs[tid] = p.env_state[(long)n * F + tid];

  // episode bookkeeping and the OU state live in thread 0's registers
  int steps = 0;
  float run = 0.0f, ou = 0.0f;
  unsigned tick = p.tick[n];  // every thread tracks it (hash counter)
  if (tid == 0) {
    s_fir = p.is_fir[n];
    steps = p.ep_steps[n];
    run = p.ep_run[n];
    if constexpr (Mode == 1) ou = p.ou_state[n];
  }
  __syncthreads();

  for (int t = 0; t < p.S; ++t) {
    const long row = (long)n * p.S + t;
    tick += 1u;
    core.step(p, tid, row, s_obs, &s_fir, s_xb, s_h, s_c, s_gates);

    float lg[2];
    if (tid < kWave) {
      // the two head columns: wave 0 splits the H-long dot products over its
      // lanes and butterfly-reduces them
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        float part = 0.0f;
        for (int k = tid; k < H; k += kWave)
          part = fmaf(s_h[k], s_hw[a * H + k], part);
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1)
          part += __shfl_xor(part, off, kWave);
        lg[a] = part + hb[a];
      }
    } else if (tid == kWave) {
      // meanwhile, Box-Muller on hash lanes 5 (radius) and 6 (angle);
      // 1 - u5 is exact in fp32 and never 0
      const float u5 = pdrl_rng::uniform(p.seed, (unsigned)n, tick, 5u);
      const float u6 = pdrl_rng::uniform(p.seed, (unsigned)n, tick, 6u);
      s_normal = __fmul_rn(sqrtf(__fmul_rn(-2.0f, logf(1.0f - u5))),
                           cosf(__fmul_rn(6.2831855f, u6)));
    } else if (tid == kWave + 1) {
      float st[F];
#pragma unroll
      for (int k = 0; k < F; ++k) st[k] = s_obs[k];
      s_drift = Env::drift(st);
    } else if (tid < kWave + 2 + R) {
      const unsigned k = (unsigned)(tid - kWave - 2);
      s_ur[k] = pdrl_rng::uniform(p.seed, (unsigned)n, tick, k + 1u);
    }
    // The part of the transform that needs the heads only (thread 0, which
    // holds them) goes before the barrier, under wave 1's chains. Mode 0,
    // PPO-C: Normal(tanh(mu), softplus(std) + 1e-4), loc = mean and ls =
    // log(sd); mode 1, SAC-C: tanh-squashed Normal(mu, exp(clamp(log_std))),
    // loc = mu and ls the clamped log_std.
    float loc = 0.0f, sd = 0.0f, ls = 0.0f;
    if (tid == 0) {
      p.logits[row * 2] = lg[0];
      p.logits[row * 2 + 1] = lg[1];
      if constexpr (Mode == 0) {
        loc = tanhf(lg[0]);
        sd = (lg[1] > 20.0f ? lg[1] : log1pf(expf(lg[1]))) + 1e-4f;
        ls = logf(sd);
      } else {
        loc = lg[0];
        ls = fminf(fmaxf(lg[1], -20.0f), 2.0f);
        sd = expf(ls);
      }
    }
    __syncthreads();

    // sample, log-prob, env step, termination, auto-reset (thread 0)
    if (tid == 0) {
      const float nrm = s_normal;
      float act, lp;
      if constexpr (Mode == 0) {
        // the action is stored unclipped, as the workers do
        act = __fadd_rn(loc, __fmul_rn(sd, nrm));
        lp = -0.5f * nrm * nrm - ls - kHalfLog2Pi;
      } else {
        const float mu = loc;
        float z, quad;
        if (n < p.ou_envs || tick <= p.warmup_steps) {
          // OU exploration: correlated noise replaces the policy sample; the
          // log-prob is the policy's density at that action
          ou = __fadd_rn(__fsub_rn(ou, __fmul_rn(p.ou_theta, ou)),
                         __fmul_rn(p.ou_sigma, nrm));
          z = ou;
          const float q = (z - mu) / sd;
          quad = -0.5f * (q * q);
        } else {
          z = __fadd_rn(mu, __fmul_rn(sd, nrm));
          quad = -0.5f * nrm * nrm;
        }
        act = tanhf(z);
        // 1 - a*a + 1e-7 without fma contraction: with the same action it
        // equals the oracle's value to the last bit, so the logf that
        // amplifies it (by up to 2 / (1 - a*a)) sees no extra difference
        const float om =
            __fadd_rn(__fsub_rn(1.0f, __fmul_rn(act, act)), 1e-7f);
        lp = quad - ls - kHalfLog2Pi - logf(om);
      }
      p.act[row] = act;
      p.log_prob[row] = lp;

      float st[F];
#pragma unroll
      for (int k = 0; k < F; ++k) st[k] = s_obs[k];
      float reward;
      bool terminated;
      Env::step(st, act, s_drift, reward, terminated);
      steps += 1;
      run += reward;
      p.rew[row] = reward;
      const bool done = terminated || steps >= p.max_episode_steps;
      const bool reset = done || steps >= p.time_horizon;
      p.ep_ret[row] = reset ? run : kNoEpisode;
      if (reset) {
        Env::reset(st, s_ur);
        steps = 0;
        run = 0.0f;
        ou = 0.0f;
      }
#pragma unroll
      for (int k = 0; k < F; ++k) s_obs[k] = st[k];
      s_fir = reset ? 1.0f : 0.0f;
      s_reset = reset ? 1 : 0;
    }
    __syncthreads();
    // thread j is the only reader of s_h[j] / s_c[j] before the next barrier
    if (s_reset != 0 && tid < H) {
      s_h[tid] = 0.0f;
      s_c[tid] = 0.0f;
    }
  }

  // persist the per-env state for the next launch
  if (tid < H) {
    p.h[(long)n * H + tid] = s_h[tid];
    p.c[(long)n * H + tid] = s_c[tid];
  }
  if (tid < F) p.env_state[(long)n * F + tid] = s_obs[tid];
  if (tid == 0) {
    p.is_fir[n] = s_fir;
    p.ep_steps[n] = steps;
    p.ep_run[n] = run;
    p.tick[n] = tick;
    if constexpr (Mode == 1) p.ou_state[n] = ou;
  }
}

// ---- greedy evaluation: whole episodes in one launch ----------------------
// rollout_eval_discrete / rollout_eval_gaussian run E episodes per env back
// to back under the deterministic action (arg-max logit; tanh(mu)) and write
// one return and one length per (env, episode). Geometry, weight residency
// and the wave 0 / wave 1 overlap are those of the training kernels; what is
// gone is everything a batch needs: no (N, S, ·) record, no softmax, no
// log-prob, no sampling draw, no OU state — and nothing persistent is read or
// written, so a launch cannot disturb the training envs. Episode e of env n
// starts from Env::reset of hash tick e (lanes 1..draws) with h = c = 0, a
// pure function of (seed, n, e); ``start_state`` may replace the start of
// episode 0. An episode ends on ``terminated`` or at max_episode_steps.
//
// The step loop is bounded by E * max_episode_steps (every episode takes at
// most max_episode_steps steps, so that many iterations finish all of them);
// the workgroup-uniform control word in LDS only leaves it early.
struct EvalArgs : PolicyWeights {
  const float* start_state;  // (N, F) start of episode 0, or nullptr
  float* ep_ret;             // (N, E)
  int* ep_len;               // (N, E)
  int N, E, D;
  unsigned seed;
  int max_episode_steps;
};

// control word written by thread 0 at the end of a step
constexpr int kEvalGoOn = 0, kEvalNextEpisode = 1, kEvalAllDone = 2;

template <int H, typename Env>
__global__ __launch_bounds__(4 * H) void rollout_eval_discrete(EvalArgs p) {
  constexpr int G = 4 * H;
  constexpr int F = Env::kObsDim;
  constexpr int A = Env::kActions;
  static_assert(F <= 4, "reset draws use hash lanes 1..4");
  const int tid = threadIdx.x;
  const int n = blockIdx.x;
  if (n >= p.N) return;  // uniform per workgroup

  __shared__ __attribute__((aligned(16))) float s_xb[H];
  __shared__ __attribute__((aligned(16))) float s_h[H];
  __shared__ __attribute__((aligned(16))) float s_c[H];
  __shared__ __attribute__((aligned(16))) float s_gates[G];
  __shared__ float s_hw[A * H];  // logits head columns, [a][k]
  __shared__ float s_obs[F];
  __shared__ float s_cand[A * F];  // next state for every action
  __shared__ float s_crew[A];
  __shared__ int s_cterm[A];
  __shared__ float s_ur[F];  // start state uniforms of the next episode
  __shared__ int s_ctl;

  RecurrentCore<H, F> core;
  core.load_weights(p, tid);
  float hb[A];
#pragma unroll
  for (int a = 0; a < A; ++a) hb[a] = p.heads_b[a];
  for (int idx = tid; idx < A * H; idx += G) {
    const int a = idx / H, k = idx % H;
    s_hw[idx] = p.heads_w[k * p.D + a];
  }
  if (tid < H) {
    s_h[tid] = 0.0f;
    s_c[tid] = 0.0f;
  }
  if (tid == 0) {
    float st[F];
    if (p.start_state != nullptr) {
#pragma unroll
      for (int k = 0; k < F; ++k) st[k] = p.start_state[(long)n * F + k];
    } else {
      float u[F];
#pragma unroll
      for (int k = 0; k < F; ++k)
        u[k] = pdrl_rng::uniform(p.seed, (unsigned)n, 0u, (unsigned)k + 1u);
      Env::reset(st, u);
    }
#pragma unroll
    for (int k = 0; k < F; ++k) s_obs[k] = st[k];
  }
  __syncthreads();

  // every thread tracks the episode index (hash counter of the next start
  // state); the step count and the running return live in thread 0
  int episode = 0, steps = 0;
  float run = 0.0f;
  const int max_iters = p.E * p.max_episode_steps;  // <= 2^22 (binding)
  for (int it = 0; it < max_iters; ++it) {
    core.advance(p, tid, s_obs, s_xb, s_h, s_c, s_gates);

    float lg[A];
    if (tid < kWave) {
      // logits: wave 0 splits the H-long dot products over its lanes and
      // butterfly-reduces them, exactly as rollout_discrete does
#pragma unroll
      for (int a = 0; a < A; ++a) {
        float part = 0.0f;
        for (int k = tid; k < H; k += kWave)
          part = fmaf(s_h[k], s_hw[a * H + k], part);
#pragma unroll
        for (int off = kWave / 2; off > 0; off >>= 1)
          part += __shfl_xor(part, off, kWave);
        lg[a] = part + hb[a];
      }
    } else if (tid < kWave + A) {
      // meanwhile wave 1 steps the dynamics for every action (lane = action)
      const int a = tid - kWave;
      float st[F];
#pragma unroll
      for (int k = 0; k < F; ++k) st[k] = s_obs[k];
      float reward;
      bool terminated;
      Env::step(st, a, reward, terminated);
#pragma unroll
      for (int k = 0; k < F; ++k) s_cand[a * F + k] = st[k];
      s_crew[a] = reward;
      s_cterm[a] = terminated ? 1 : 0;
    } else if (tid < kWave + A + F) {
      // ... and draws the start state of the episode that would follow
      const unsigned k = (unsigned)(tid - kWave - A);
      s_ur[k] = pdrl_rng::uniform(p.seed, (unsigned)n,
                                  (unsigned)episode + 1u, k + 1u);
    }

    // greedy action (thread 0 holds the reduced logits): strict > scan from
    // action 0, so ties go to the lowest index
    int chosen = 0;
    if (tid == 0) {
      float best = lg[0];
#pragma unroll
      for (int a = 1; a < A; ++a) {
        if (lg[a] > best) {
          best = lg[a];
          chosen = a;
        }
      }
    }
    __syncthreads();

    // the chosen action's outcome; episode end and fresh start (thread 0)
    if (tid == 0) {
      float st[F];
#pragma unroll
      for (int k = 0; k < F; ++k) st[k] = s_cand[chosen * F + k];
      steps += 1;
      run += s_crew[chosen];
      const bool done = s_cterm[chosen] != 0 || steps >= p.max_episode_steps;
      int ctl = kEvalGoOn;
      if (done) {
        p.ep_ret[(long)n * p.E + episode] = run;
        p.ep_len[(long)n * p.E + episode] = steps;
        Env::reset(st, s_ur);
        steps = 0;
        run = 0.0f;
        ctl = (episode + 1 >= p.E) ? kEvalAllDone : kEvalNextEpisode;
      }
#pragma unroll
      for (int k = 0; k < F; ++k) s_obs[k] = st[k];
      s_ctl = ctl;
    }
    __syncthreads();
    const int ctl = s_ctl;  // the same value in every thread of the workgroup
    if (ctl == kEvalAllDone) break;
    if (ctl == kEvalNextEpisode) {
      episode += 1;
      // thread j is the only reader of s_h[j] / s_c[j] before the next barrier
      if (tid < H) {
        s_h[tid] = 0.0f;
        s_c[tid] = 0.0f;
      }
    }
  }
}

template <int H, typename Env>
__global__ __launch_bounds__(4 * H) void rollout_eval_gaussian(EvalArgs p) {
  static_assert(Env::kActDim == 1, "one action dimension (head column 0)");
  static_assert(Env::kResetDraws >= 1 && Env::kResetDraws <= 4,
                "reset draws use hash lanes 1..4");
  constexpr int F = Env::kObsDim;
  constexpr int R = Env::kResetDraws;
  constexpr int G = 4 * H;
  const int tid = threadIdx.x;
  const int n = blockIdx.x;
  if (n >= p.N) return;  // uniform per workgroup

  __shared__ __attribute__((aligned(16))) float s_xb[H];
  __shared__ __attribute__((aligned(16))) float s_h[H];
  __shared__ __attribute__((aligned(16))) float s_c[H];
  __shared__ __attribute__((aligned(16))) float s_gates[G];
  __shared__ float s_hw[H];  // mu head column
  __shared__ float s_obs[F];
  __shared__ float s_ur[R];  // start state uniforms of the next episode
  __shared__ float s_drift;
  __shared__ int s_ctl;

  RecurrentCore<H, F> core;
  core.load_weights(p, tid);
  const float hb = p.heads_b[0];
  if (tid < H) {
    s_hw[tid] = p.heads_w[tid * p.D];
    s_h[tid] = 0.0f;
    s_c[tid] = 0.0f;
  }
  if (tid == 0) {
    float st[F];
    if (p.start_state != nullptr) {
#pragma unroll
      for (int k = 0; k < F; ++k) st[k] = p.start_state[(long)n * F + k];
    } else {
      float u[R];
#pragma unroll
      for (int k = 0; k < R; ++k)
        u[k] = pdrl_rng::uniform(p.seed, (unsigned)n, 0u, (unsigned)k + 1u);
      Env::reset(st, u);
    }
#pragma unroll
    for (int k = 0; k < F; ++k) s_obs[k] = st[k];
  }
  __syncthreads();

  int episode = 0, steps = 0;
  float run = 0.0f;
  const int max_iters = p.E * p.max_episode_steps;  // <= 2^22 (binding)
  for (int it = 0; it < max_iters; ++it) {
    core.advance(p, tid, s_obs, s_xb, s_h, s_c, s_gates);

    float mu = 0.0f;
    if (tid < kWave) {
      // the mu head column only: wave 0 butterfly-reduces the dot product
      float part = 0.0f;
      for (int k = tid; k < H; k += kWave)
        part = fmaf(s_h[k], s_hw[k], part);
#pragma unroll
      for (int off = kWave / 2; off > 0; off >>= 1)
        part += __shfl_xor(part, off, kWave);
      mu = part + hb;
    } else if (tid == kWave) {
      // meanwhile wave 1 evaluates the action-independent drift
      float st[F];
#pragma unroll
      for (int k = 0; k < F; ++k) st[k] = s_obs[k];
      s_drift = Env::drift(st);
    } else if (tid < kWave + 1 + R) {
      // ... and draws the start state of the episode that would follow
      const unsigned k = (unsigned)(tid - kWave - 1);
      s_ur[k] = pdrl_rng::uniform(p.seed, (unsigned)n,
                                  (unsigned)episode + 1u, k + 1u);
    }
    // deterministic action of both head schemes: the mean of PPO-C's
    // Normal(tanh(mu), ·) and of SAC-C's squashed Gaussian at zero noise
    float act = 0.0f;
    if (tid == 0) act = tanhf(mu);
    __syncthreads();

    // env step, episode end and fresh start (thread 0)
    if (tid == 0) {
      float st[F];
#pragma unroll
      for (int k = 0; k < F; ++k) st[k] = s_obs[k];
      float reward;
      bool terminated;
      Env::step(st, act, s_drift, reward, terminated);
      steps += 1;
      run += reward;
      const bool done = terminated || steps >= p.max_episode_steps;
      int ctl = kEvalGoOn;
      if (done) {
        p.ep_ret[(long)n * p.E + episode] = run;
        p.ep_len[(long)n * p.E + episode] = steps;
        Env::reset(st, s_ur);
        steps = 0;
        run = 0.0f;
        ctl = (episode + 1 >= p.E) ? kEvalAllDone : kEvalNextEpisode;
      }
#pragma unroll
      for (int k = 0; k < F; ++k) s_obs[k] = st[k];
      s_ctl = ctl;
    }
    __syncthreads();
    const int ctl = s_ctl;  // the same value in every thread of the workgroup
    if (ctl == kEvalAllDone) break;
    if (ctl == kEvalNextEpisode) {
      episode += 1;
      // thread j is the only reader of s_h[j] / s_c[j] before the next barrier
      if (tid < H) {
        s_h[tid] = 0.0f;
        s_c[tid] = 0.0f;
      }
    }
  }
}

template <typename Env>
void launch_eval_discrete(const EvalArgs& a, int H) {
  const dim3 grid(a.N);
  switch (H) {
    case 32:
      hipLaunchKernelGGL((rollout_eval_discrete<32, Env>), grid, dim3(128), 0,
                         current_stream(), a);
      break;
    case 64:
      hipLaunchKernelGGL((rollout_eval_discrete<64, Env>), grid, dim3(256), 0,
                         current_stream(), a);
      break;
    case 128:
      hipLaunchKernelGGL((rollout_eval_discrete<128, Env>), grid, dim3(512), 0,
                         current_stream(), a);
      break;
    default:
      TORCH_CHECK(false, "hidden size ", H, " unsupported (32/64/128)");
  }
  HIP_CHECK_LAST();
}

template <typename Env>
void launch_eval_gaussian(const EvalArgs& a, int H) {
  const dim3 grid(a.N);
  switch (H) {
    case 32:
      hipLaunchKernelGGL((rollout_eval_gaussian<32, Env>), grid, dim3(128), 0,
                         current_stream(), a);
      break;
    case 64:
      hipLaunchKernelGGL((rollout_eval_gaussian<64, Env>), grid, dim3(256), 0,
                         current_stream(), a);
      break;
    case 128:
      hipLaunchKernelGGL((rollout_eval_gaussian<128, Env>), grid, dim3(512), 0,
                         current_stream(), a);
      break;
    default:
      TORCH_CHECK(false, "hidden size ", H, " unsupported (32/64/128)");
  }
  HIP_CHECK_LAST();
}

template <int H, typename Env>
void launch_gaussian_mode(const GaussianArgs& a, int mode) {
  const dim3 grid(a.N), block(4 * H);
  if (mode == 0)
    hipLaunchKernelGGL((rollout_gaussian<H, Env, 0>), grid, block, 0,
                       current_stream(), a);
  else
    hipLaunchKernelGGL((rollout_gaussian<H, Env, 1>), grid, block, 0,
                       current_stream(), a);
}

template <typename Env>
void launch_gaussian(const GaussianArgs& a, int H, int mode) {
  switch (H) {
    case 32: launch_gaussian_mode<32, Env>(a, mode); break;
    case 64: launch_gaussian_mode<64, Env>(a, mode); break;
    case 128: launch_gaussian_mode<128, Env>(a, mode); break;
    default:
      TORCH_CHECK(false, "hidden size ", H, " unsupported (32/64/128)");
  }
  HIP_CHECK_LAST();
}

template <typename Env>
void launch_env(const RolloutArgs& a, int H) {
  const dim3 grid(a.N);
  switch (H) {
    case 32:
      hipLaunchKernelGGL((rollout_discrete<32, Env>), grid, dim3(128), 0,
                         current_stream(), a);
      break;
    case 64:
      hipLaunchKernelGGL((rollout_discrete<64, Env>), grid, dim3(256), 0,
                         current_stream(), a);
      break;
    case 128:
      hipLaunchKernelGGL((rollout_discrete<128, Env>), grid, dim3(512), 0,
                         current_stream(), a);
      break;
    default:
      TORCH_CHECK(false, "hidden size ", H, " unsupported (32/64/128)");
  }
  HIP_CHECK_LAST();
}

void check_i32(const at::Tensor& t, long n, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.scalar_type() == at::kInt && t.numel() == n,
              name, " must be a contiguous int32 GPU tensor of ", n,
              " elements");
}

void check_f32(const at::Tensor& t, long n, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous() &&
                  t.scalar_type() == at::kFloat && t.numel() == n,
              name, " must be a contiguous float32 GPU tensor of ", n,
              " elements");
}

// Checks and pointer packing of the live policy weights, shared by every
// entry point. The env fixes obs_dim (F_env, else env_msg is raised) and A,
// the number of leading head columns the kernel reads.
PolicyWeights pack_policy_weights(
    const at::Tensor& body_w, const at::Tensor& body_b, const at::Tensor& w_ih,
    const at::Tensor& w_hh, const at::Tensor& b_g, const at::Tensor& heads_w,
    const at::Tensor& heads_b, long F_env, const char* env_msg, long A) {
  CHECK_IN(body_w); CHECK_IN(body_b); CHECK_IN(w_ih); CHECK_IN(w_hh);
  CHECK_IN(b_g); CHECK_IN(heads_w); CHECK_IN(heads_b);
  TORCH_CHECK(body_w.dim() == 2 && w_ih.dim() == 2 && heads_w.dim() == 2,
              "rollout: bad tensor ranks");
  const long F = body_w.size(0), H = body_w.size(1), D = heads_w.size(1);
  TORCH_CHECK(F == F_env, env_msg);
  TORCH_CHECK(D >= A && heads_w.size(0) == H, "heads_w shape");
  check_f32(body_b, H, "body_b");
  check_f32(w_ih, H * 4 * H, "w_ih");
  check_f32(w_hh, H * 4 * H, "w_hh");
  check_f32(b_g, 4 * H, "b_g");
  check_f32(heads_b, D, "heads_b");
  const auto dev = body_w.device();
  for (const at::Tensor* t : std::initializer_list<const at::Tensor*>{
        &body_b, &w_ih, &w_hh, &b_g, &heads_w, &heads_b})
    TORCH_CHECK(t->device() == dev, "rollout: tensors on different devices");
  PolicyWeights w;
  w.body_w = body_w.data_ptr<float>();
  w.body_b = body_b.data_ptr<float>();
  w.w_ih = w_ih.data_ptr<float>();
  w.w_hh = w_hh.data_ptr<float>();
  w.b_g = b_g.data_ptr<float>();
  w.heads_w = heads_w.data_ptr<float>();
  w.heads_b = heads_b.data_ptr<float>();
  return w;
}

// Argument checks and pointer packing shared by both training entry points;
// A is also the width of the ``logits`` field.
RolloutArgs pack_rollout_args(
    const at::Tensor& body_w, const at::Tensor& body_b, const at::Tensor& w_ih,
    const at::Tensor& w_hh, const at::Tensor& b_g, const at::Tensor& heads_w,
    const at::Tensor& heads_b, at::Tensor& env_state, at::Tensor& h,
    at::Tensor& c, at::Tensor& is_fir, at::Tensor& ep_steps,
    at::Tensor& ep_run, at::Tensor& tick, at::Tensor& obs, at::Tensor& act,
    at::Tensor& rew, at::Tensor& logits, at::Tensor& log_prob,
    at::Tensor& is_fir_out, at::Tensor& hx, at::Tensor& cx,
    at::Tensor& ep_ret, long F_env, const char* env_msg, long A, long seed,
    long time_horizon, long max_episode_steps) {
  RolloutArgs a;
  static_cast<PolicyWeights&>(a) = pack_policy_weights(
      body_w, body_b, w_ih, w_hh, b_g, heads_w, heads_b, F_env, env_msg, A);
  TORCH_CHECK(env_state.dim() == 2 && obs.dim() == 3,
              "rollout: bad tensor ranks");
  const long F = body_w.size(0), H = body_w.size(1), D = heads_w.size(1);
  const long N = env_state.size(0), S = obs.size(1);
  TORCH_CHECK(N >= 1 && S >= 1, "rollout: empty batch");
  check_f32(env_state, N * F, "env_state");
  check_f32(h, N * H, "h");
  check_f32(c, N * H, "c");
  check_f32(is_fir, N, "is_fir state");
  check_i32(ep_steps, N, "ep_steps");
  check_f32(ep_run, N, "ep_run");
  check_i32(tick, N, "tick");
  check_f32(obs, N * S * F, "obs");
  check_f32(act, N * S, "act");
  check_f32(rew, N * S, "rew");
  check_f32(logits, N * S * A, "logits");
  check_f32(log_prob, N * S, "log_prob");
  check_f32(is_fir_out, N * S, "is_fir");
  check_f32(hx, N * S * H, "hx");
  check_f32(cx, N * S * H, "cx");
  check_f32(ep_ret, N * S, "ep_ret");
  const auto dev = body_w.device();
  for (const at::Tensor* t : std::initializer_list<const at::Tensor*>{
        &env_state, &h, &c, &is_fir, &ep_steps, &ep_run, &tick, &obs, &act,
        &rew, &logits, &log_prob, &is_fir_out, &hx, &cx, &ep_ret})
    TORCH_CHECK(t->device() == dev, "rollout: tensors on different devices");
  TORCH_CHECK(time_horizon >= 1 && max_episode_steps >= 1,
              "rollout: horizons must be positive");

  a.env_state = env_state.data_ptr<float>();
  a.h = h.data_ptr<float>();
  a.c = c.data_ptr<float>();
  a.is_fir = is_fir.data_ptr<float>();
  a.ep_steps = ep_steps.data_ptr<int>();
  a.ep_run = ep_run.data_ptr<float>();
  a.tick = reinterpret_cast<unsigned*>(tick.data_ptr<int>());
  a.obs = obs.data_ptr<float>();
  a.act = act.data_ptr<float>();
  a.rew = rew.data_ptr<float>();
  a.logits = logits.data_ptr<float>();
  a.log_prob = log_prob.data_ptr<float>();
  a.is_fir_out = is_fir_out.data_ptr<float>();
  a.hx = hx.data_ptr<float>();
  a.cx = cx.data_ptr<float>();
  a.ep_ret = ep_ret.data_ptr<float>();
  a.N = (int)N;
  a.S = (int)S;
  a.D = (int)D;
  a.seed = (unsigned)seed;
  a.time_horizon = (int)std::min<long>(time_horizon, INT32_MAX);
  a.max_episode_steps = (int)std::min<long>(max_episode_steps, INT32_MAX);
  return a;
}

// Upper bound of the evaluation kernels' step loop, E * max_episode_steps.
constexpr long kEvalMaxIters = 1L << 22;

// Argument checks and pointer packing of the evaluation entry points.
// ep_ret (N, E) fixes the number of envs and of episodes per env.
EvalArgs pack_eval_args(
    const at::Tensor& body_w, const at::Tensor& body_b, const at::Tensor& w_ih,
    const at::Tensor& w_hh, const at::Tensor& b_g, const at::Tensor& heads_w,
    const at::Tensor& heads_b, at::Tensor& ep_ret, at::Tensor& ep_len,
    const c10::optional<at::Tensor>& start_state, long F_env,
    const char* env_msg, long A, long seed, long max_episode_steps) {
  EvalArgs a;
  static_cast<PolicyWeights&>(a) = pack_policy_weights(
      body_w, body_b, w_ih, w_hh, b_g, heads_w, heads_b, F_env, env_msg, A);
  TORCH_CHECK(ep_ret.dim() == 2, "rollout_eval: ep_ret must be (N, E)");
  const long N = ep_ret.size(0), E = ep_ret.size(1);
  TORCH_CHECK(N >= 1 && N <= INT32_MAX, "rollout_eval: bad number of envs");
  TORCH_CHECK(E >= 1, "rollout_eval: episodes must be positive");
  TORCH_CHECK(max_episode_steps >= 1,
              "rollout_eval: max_episode_steps must be positive");
  TORCH_CHECK(E <= kEvalMaxIters && max_episode_steps <= kEvalMaxIters &&
                  E * max_episode_steps <= kEvalMaxIters,
              "rollout_eval: episodes * max_episode_steps = ", E, " * ",
              max_episode_steps, " exceeds the step loop bound ",
              kEvalMaxIters);
  check_f32(ep_ret, N * E, "ep_ret");
  check_i32(ep_len, N * E, "ep_len");
  const auto dev = body_w.device();
  TORCH_CHECK(ep_ret.device() == dev && ep_len.device() == dev,
              "rollout: tensors on different devices");
  a.start_state = nullptr;
  if (start_state.has_value()) {
    check_f32(*start_state, N * F_env, "start_state");
    TORCH_CHECK(start_state->device() == dev,
                "rollout: tensors on different devices");
    a.start_state = start_state->data_ptr<float>();
  }
  a.ep_ret = ep_ret.data_ptr<float>();
  a.ep_len = ep_len.data_ptr<int>();
  a.N = (int)N;
  a.E = (int)E;
  a.D = (int)heads_w.size(1);
  a.seed = (unsigned)seed;
  a.max_episode_steps = (int)max_episode_steps;
  return a;
}

}  // namespace

// env_id: 0 = CartPole-v1 (ids are assigned in pdrl_amd/ops/rollout.py).
void rollout_discrete_hip(
    const at::Tensor& body_w, const at::Tensor& body_b, const at::Tensor& w_ih,
    const at::Tensor& w_hh, const at::Tensor& b_g, const at::Tensor& heads_w,
    const at::Tensor& heads_b, at::Tensor& env_state, at::Tensor& h,
    at::Tensor& c, at::Tensor& is_fir, at::Tensor& ep_steps,
    at::Tensor& ep_run, at::Tensor& tick, at::Tensor& obs, at::Tensor& act,
    at::Tensor& rew, at::Tensor& logits, at::Tensor& log_prob,
    at::Tensor& is_fir_out, at::Tensor& hx, at::Tensor& cx,
    at::Tensor& ep_ret, long env_id, long seed, long time_horizon,
    long max_episode_steps) {
  long F_env = 0, A = 0;
  const char* env_msg = "";
  switch (env_id) {
    case 0:
      F_env = CartPoleDyn::kObsDim;
      A = CartPoleDyn::kActions;
      env_msg = "CartPole needs obs_dim 4";
      break;
    default:
      TORCH_CHECK(false, "rollout: unknown device env id ", env_id);
  }
  const RolloutArgs a = pack_rollout_args(
      body_w, body_b, w_ih, w_hh, b_g, heads_w, heads_b, env_state, h, c,
      is_fir, ep_steps, ep_run, tick, obs, act, rew, logits, log_prob,
      is_fir_out, hx, cx, ep_ret, F_env, env_msg, A, seed, time_horizon,
      max_episode_steps);
  switch (env_id) {
    case 0: launch_env<CartPoleDyn>(a, (int)body_w.size(1)); break;
  }
}

// Gaussian-policy sibling. env_id: 1 = MountainCarContinuous-v0. mode: 0 =
// heads (mu, std), PPO-C sampling; 1 = heads (mu, log_std), SAC-C sampling
// with optional OU exploration (ou_envs, warmup_steps; see GaussianArgs).
void rollout_gaussian_hip(
    const at::Tensor& body_w, const at::Tensor& body_b, const at::Tensor& w_ih,
    const at::Tensor& w_hh, const at::Tensor& b_g, const at::Tensor& heads_w,
    const at::Tensor& heads_b, at::Tensor& env_state, at::Tensor& h,
    at::Tensor& c, at::Tensor& is_fir, at::Tensor& ep_steps,
    at::Tensor& ep_run, at::Tensor& tick, at::Tensor& ou_state,
    at::Tensor& obs, at::Tensor& act, at::Tensor& rew, at::Tensor& logits,
    at::Tensor& log_prob, at::Tensor& is_fir_out, at::Tensor& hx,
    at::Tensor& cx, at::Tensor& ep_ret, long env_id, long mode, long seed,
    long time_horizon, long max_episode_steps, long ou_envs,
    long warmup_steps, double ou_theta, double ou_sigma) {
  long F_env = 0;
  const char* env_msg = "";
  switch (env_id) {
    case 1:
      F_env = MountainCarContDyn::kObsDim;
      env_msg = "MountainCarContinuous needs obs_dim 2";
      break;
    default:
      TORCH_CHECK(false, "rollout: unknown continuous device env id ", env_id);
  }
  TORCH_CHECK(mode == 0 || mode == 1, "rollout: mode must be 0 or 1");
  TORCH_CHECK(ou_envs >= 0 && warmup_steps >= 0,
              "rollout: ou_envs and warmup_steps must not be negative");
  TORCH_CHECK(mode == 1 || (ou_envs == 0 && warmup_steps == 0),
              "rollout: OU exploration needs mode 1 (mu, log_std)");
  // logits field = [mu | std or log_std]: two head columns
  GaussianArgs a;
  static_cast<RolloutArgs&>(a) = pack_rollout_args(
      body_w, body_b, w_ih, w_hh, b_g, heads_w, heads_b, env_state, h, c,
      is_fir, ep_steps, ep_run, tick, obs, act, rew, logits, log_prob,
      is_fir_out, hx, cx, ep_ret, F_env, env_msg, 2, seed, time_horizon,
      max_episode_steps);
  TORCH_CHECK(a.D >= 2, "heads_w shape");
  check_f32(ou_state, a.N, "ou_state");
  TORCH_CHECK(ou_state.device() == body_w.device(),
              "rollout: tensors on different devices");
  a.ou_state = ou_state.data_ptr<float>();
  a.ou_envs = (int)std::min<long>(ou_envs, INT32_MAX);
  a.warmup_steps = (unsigned)std::min<long>(warmup_steps, UINT32_MAX);
  a.ou_theta = (float)ou_theta;
  a.ou_sigma = (float)ou_sigma;
  switch (env_id) {
    case 1:
      launch_gaussian<MountainCarContDyn>(a, (int)body_w.size(1), (int)mode);
      break;
  }
}

// Greedy evaluation, discrete policy: E = ep_ret.size(1) whole episodes per
// env in one launch. env_id as in rollout_discrete_hip.
void rollout_eval_discrete_hip(
    const at::Tensor& body_w, const at::Tensor& body_b, const at::Tensor& w_ih,
    const at::Tensor& w_hh, const at::Tensor& b_g, const at::Tensor& heads_w,
    const at::Tensor& heads_b, at::Tensor& ep_ret, at::Tensor& ep_len,
    const c10::optional<at::Tensor>& start_state, long env_id, long seed,
    long max_episode_steps) {
  switch (env_id) {
    case 0: {
      const EvalArgs a = pack_eval_args(
          body_w, body_b, w_ih, w_hh, b_g, heads_w, heads_b, ep_ret, ep_len,
          start_state, CartPoleDyn::kObsDim, "CartPole needs obs_dim 4",
          CartPoleDyn::kActions, seed, max_episode_steps);
      launch_eval_discrete<CartPoleDyn>(a, (int)body_w.size(1));
      break;
    }
    default:
      TORCH_CHECK(false, "rollout: unknown device env id ", env_id);
  }
}

// Greedy evaluation, Gaussian policy: the action is tanh(mu) for both head
// schemes, so only head column 0 is read. env_id as in rollout_gaussian_hip.
void rollout_eval_gaussian_hip(
    const at::Tensor& body_w, const at::Tensor& body_b, const at::Tensor& w_ih,
    const at::Tensor& w_hh, const at::Tensor& b_g, const at::Tensor& heads_w,
    const at::Tensor& heads_b, at::Tensor& ep_ret, at::Tensor& ep_len,
    const c10::optional<at::Tensor>& start_state, long env_id, long seed,
    long max_episode_steps) {
  switch (env_id) {
    case 1: {
      const EvalArgs a = pack_eval_args(
          body_w, body_b, w_ih, w_hh, b_g, heads_w, heads_b, ep_ret, ep_len,
          start_state, MountainCarContDyn::kObsDim,
          "MountainCarContinuous needs obs_dim 2", 1, seed, max_episode_steps);
      launch_eval_gaussian<MountainCarContDyn>(a, (int)body_w.size(1));
      break;
    }
    default:
      TORCH_CHECK(false, "rollout: unknown continuous device env id ", env_id);
  }
}

// Host evaluation of the rollout's uniform (same header as the kernel).
double rollout_uniform_host(long seed, long env, long tick, long k) {
  return (double)pdrl_rng::uniform((uint32_t)seed, (uint32_t)env,
                                   (uint32_t)tick, (uint32_t)k);
}
