// Device actor: fused policy-act + env-step kernels for CDNA4 (gfx950).
//
// Two kernels, each composed from a policy scheme and shared helpers:
//
//   rollout_train<H, Policy>  one launch advances N native environments by S
//     steps and writes the (N, S, ·) batch in the learner's own field layout
//     (buffers.rollout_fields) straight into persistent device tensors:
//     policy forward, sample, log-prob, env dynamics, termination and
//     auto-reset never leave the GPU. Per-env state is carried from launch to
//     launch. Bindings rollout_discrete and rollout_gaussian.
//   rollout_eval<H, Policy>   greedy evaluation: E whole episodes per env
//     under the deterministic action, one return and one length per (env,
//     episode), no batch, nothing persistent. Bindings rollout_eval_discrete
//     and rollout_eval_gaussian.
//
// The eager oracles are pdrl_amd/ops/rollout.py and pdrl_amd/ops/evaluate.py,
// the single-call CPU counterparts cpu_actor.cpp::act_batch_discrete /
// act_batch_gaussian.
//
// Geometry: as seq_lstm_fwd_row (core_rows.h) — one 4H-thread workgroup per
// environment, thread = gate column with its w_ih / w_hh column resident in
// 2×H VGPRs (RecurrentCore), loaded once per launch and amortised over the
// steps. The environments are independent, so there is no inter-workgroup
// traffic and no atomics: episode returns are written per (env, step) and
// reduced lazily by the host. obs, xb, h, c, gates and the head columns live
// in LDS (a few KB). A step is five barriers: three in RecurrentCore, then
// wave 0 butterfly-reduces the head columns (reduce_heads) while wave 1 does
// the scheme's side work (env dynamics that need no action, random draws),
// thread 0 does the part of the scheme that needs the heads only, barrier,
// thread 0 finishes the step (action → next state, reward, terminated) and
// the kernel's episode bookkeeping, barrier.
//
// Where things go (two places each, no kernel is touched):
//   a new env     its traits struct, and its line in the env table of its
//                 family right below it ("native env dynamics"); an env whose
//                 observation is not its state adds kStateDim and observe();
//   a new policy  one scheme struct in "policy schemes" (sampling schemes
//                 feed rollout_train, greedy ones rollout_eval), and the
//                 entry point that launches it.
//
// Random numbers come from the stateless counter hash in rollout_rng.h,
// keyed by (seed, env, tick, lane): per-env tick counters live on device and
// are advanced by the kernel, so replays and re-launches never repeat draws.

#include "common.h"
#include "rollout_rng.h"

#include <algorithm>
#include <cstdint>
#include <type_traits>

namespace {

// "No episode ended at this step" marker in ep_ret (any real return is far
// above it, negative-reward envs included).
constexpr float kNoEpisode = -1.0e30f;

// ---- native env dynamics -------------------------------------------------
// An env is a traits struct. Common to both families: kObsDim, kResetDraws
// (hash lanes 1..kResetDraws feed reset) and reset(state, u[kResetDraws]).
// The step differs by action type, and the two forms are not put behind one
// shape: a discrete env has kActions and step(state, action, reward,
// terminated), cheap enough that wave 1 steps EVERY action while the logits
// are reduced; a continuous env (further below) cannot enumerate its actions
// and splits the update at the action instead. A second env is one more
// struct and one more line in its family's table (with_discrete_env /
// with_continuous_env).
//
// An env whose observation is not its state vector (hidden state, angles seen
// as cos / sin) also defines kStateDim and observe(state, obs): the kernels
// carry kStateDim values per env (env_state, start_state) and feed the policy
// and the ``obs`` record the kObsDim values of observe. An env that defines
// neither is an identity env: kStateDim == kObsDim, and the observation array
// IS the state array (chosen at compile time: no extra LDS, copy or barrier).

template <typename Env, typename = void>
struct EnvObs {  // identity env
  static constexpr bool kIdentity = true;
  static constexpr int kStateDim = Env::kObsDim;
};
template <typename Env>
struct EnvObs<Env, std::void_t<decltype(&Env::observe)>> {
  static constexpr bool kIdentity = false;
  static constexpr int kStateDim = Env::kStateDim;
};

// x modulo 2π into [-π, π), as x - 2π·floor((x + π) / 2π) in explicit
// roundings on both sides (wrap_angle in pdrl_amd/ops/rollout.py): the floor
// decides a jump of 2π, and no library remainder is called.
__device__ __forceinline__ float wrap_angle(float x) {
  constexpr float kPi = 3.1415927f, kTwoPi = 6.2831855f;
  return __fsub_rn(
      x, __fmul_rn(kTwoPi, floorf(__fdiv_rn(__fadd_rn(x, kPi), kTwoPi))));
}

// CartPole-v1: constants and Euler update of pdrl_amd/envs/cartpole.py, fp32.
struct CartPoleDyn {
  static constexpr int kObsDim = 4;
  static constexpr int kActions = 2;
  static constexpr int kResetDraws = 4;

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

// Acrobot-v1: "book" equations of motion and RK4 step of
// pdrl_amd/envs/acrobot.py, fp32, in the op order of the oracle (AcrobotDyn in
// pdrl_amd/ops/rollout.py) with the unit masses and lengths folded in. State
// (θ1, θ2, θ̇1, θ̇2), observed as (cos θ1, sin θ1, cos θ2, sin θ2, θ̇1, θ̇2).
struct AcrobotDyn {
  static constexpr int kObsDim = 6;
  static constexpr int kStateDim = 4;
  static constexpr int kActions = 3;
  static constexpr int kResetDraws = 4;

  __device__ static void observe(const float* s, float* o) {
    sincosf(s[0], &o[1], &o[0]);
    sincosf(s[1], &o[3], &o[2]);
    o[4] = s[2]; o[5] = s[3];
  }

  __device__ static void reset(float* s, const float* u) {
#pragma unroll
    for (int i = 0; i < kStateDim; ++i)
      s[i] = __fadd_rn(-0.1f, __fmul_rn(0.2f, u[i]));
  }

  // (θ̈1, θ̈2): d1 = 3.5 + cos θ2, d2 = 1.25 + 0.5 cos θ2, cos(x - π/2) = sin x
  __device__ __forceinline__ static void derivs(float t1, float t2, float v1,
                                                float v2, float torque,
                                                float& a1, float& a2) {
    float c2, s2;
    sincosf(t2, &s2, &c2);
    const float d1 = 3.5f + c2;
    const float d2 = 1.25f + 0.5f * c2;
    const float phi2 = 4.9f * sinf(t1 + t2);
    const float phi1 =
        -0.5f * v2 * v2 * s2 - v2 * v1 * s2 + 14.7f * sinf(t1) + phi2;
    a2 = (torque + d2 / d1 * phi1 - 0.5f * v1 * v1 * s2 - phi2) /
         (1.25f - d2 * d2 / d1);
    a1 = -(d2 * a2 + phi1) / d1;
  }

  __device__ static void step(float* s, int a, float& reward,
                              bool& terminated) {
    constexpr float kDt = 0.2f, kHalf = 0.1f, kSixth = 0.2 / 6.0;
    constexpr float kMaxVel1 = 4.0 * 3.141592653589793;
    constexpr float kMaxVel2 = 9.0 * 3.141592653589793;
    float t1 = s[0], t2 = s[1], v1 = s[2], v2 = s[3];
    const float torque = (float)a - 1.0f;
    float k1a, k1b, k2a, k2b, k3a, k3b, k4a, k4b;
    derivs(t1, t2, v1, v2, torque, k1a, k1b);
    const float x1 = v1 + kHalf * k1a, x2 = v2 + kHalf * k1b;
    derivs(t1 + kHalf * v1, t2 + kHalf * v2, x1, x2, torque, k2a, k2b);
    const float y1 = v1 + kHalf * k2a, y2 = v2 + kHalf * k2b;
    derivs(t1 + kHalf * x1, t2 + kHalf * x2, y1, y2, torque, k3a, k3b);
    const float z1 = v1 + kDt * k3a, z2 = v2 + kDt * k3b;
    derivs(t1 + kDt * y1, t2 + kDt * y2, z1, z2, torque, k4a, k4b);
    t1 = wrap_angle(t1 + kSixth * (v1 + 2.0f * x1 + 2.0f * y1 + z1));
    t2 = wrap_angle(t2 + kSixth * (v2 + 2.0f * x2 + 2.0f * y2 + z2));
    v1 = v1 + kSixth * (k1a + 2.0f * k2a + 2.0f * k3a + k4a);
    v2 = v2 + kSixth * (k1b + 2.0f * k2b + 2.0f * k3b + k4b);
    v1 = fminf(fmaxf(v1, -kMaxVel1), kMaxVel1);
    v2 = fminf(fmaxf(v2, -kMaxVel2), kMaxVel2);
    s[0] = t1; s[1] = t2; s[2] = v1; s[3] = v2;
    // the tip height decides the episode: explicit roundings
    terminated = __fsub_rn(-cosf(t1), cosf(__fadd_rn(t1, t2))) > 1.0f;
    reward = terminated ? 0.0f : -1.0f;
  }
};

// Continuous-action envs: kActDim, drift(state) — the part of the update
// that does not depend on the action, so another wave can evaluate it while
// the policy heads are still being reduced — and step(state, action, drift,
// reward, terminated) with a float action. Only the chosen action is stepped.

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

// Pendulum-v1 with the normalised action of pdrl_amd/envs/pendulum.py (torque
// 2·clip(a, -1, 1)), fp32, in the op order of the oracle (PendulumDyn in
// pdrl_amd/ops/rollout.py); g = 10, m = l = 1, dt = 0.05 folded in. State
// (θ, θ̇) with θ never wrapped, observed as (cos θ, sin θ, θ̇). Nothing here
// is discontinuous (the clips and wrap(θ)² are continuous), so apart from the
// wrap and reset no rounding is pinned.
struct PendulumDyn {
  static constexpr int kObsDim = 3;
  static constexpr int kStateDim = 2;
  static constexpr int kActDim = 1;
  static constexpr int kResetDraws = 2;

  __device__ static void observe(const float* s, float* o) {
    sincosf(s[0], &o[1], &o[0]);
    o[2] = s[1];
  }

  __device__ static void reset(float* s, const float* u) {
    s[0] = __fadd_rn(-3.1415927f, __fmul_rn(6.2831855f, u[0]));
    s[1] = __fadd_rn(-1.0f, __fmul_rn(2.0f, u[1]));
  }

  // 15·sin θ·dt
  __device__ static float drift(const float* s) { return 0.75f * sinf(s[0]); }

  __device__ static void step(float* s, float a, float drift, float& reward,
                              bool& terminated) {
    const float u = 2.0f * fminf(fmaxf(a, -1.0f), 1.0f);
    float th = s[0], thd = s[1];
    const float w = wrap_angle(th);
    reward = -(w * w + 0.1f * thd * thd + 0.001f * u * u);  // pre-step state
    thd = fminf(fmaxf(thd + (drift + 0.15f * u), -8.0f), 8.0f);
    th = th + 0.05f * thd;
    s[0] = th;
    s[1] = thd;
    terminated = false;
  }
};

// Env tables (ids are assigned in pdrl_amd/ops/rollout.py): f(traits, message
// raised when the core's obs_dim does not match).
template <typename Fn>
void with_discrete_env(long env_id, Fn&& f) {
  switch (env_id) {
    case 0: f(CartPoleDyn{}, "CartPole needs obs_dim 4"); break;
    case 2: f(AcrobotDyn{}, "Acrobot needs obs_dim 6"); break;
    default: TORCH_CHECK(false, "rollout: unknown device env id ", env_id);
  }
}

template <typename Fn>
void with_continuous_env(long env_id, Fn&& f) {
  switch (env_id) {
    case 1:
      f(MountainCarContDyn{}, "MountainCarContinuous needs obs_dim 2");
      break;
    case 3: f(PendulumDyn{}, "Pendulum needs obs_dim 3"); break;
    default:
      TORCH_CHECK(false, "rollout: unknown continuous device env id ", env_id);
  }
}

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
  float* env_state;      // (N, kStateDim)
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

// ---- recurrent part, shared by rollout_train and rollout_eval -------------
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

// Arguments of the sampling Gaussian schemes.
struct GaussianArgs : RolloutArgs {
  float* ou_state;        // (N) persistent OU exploration state (Mode 1)
  int ou_envs;            // envs [0, ou_envs) explore with OU noise forever
  unsigned warmup_steps;  // every env explores while tick <= warmup_steps
  float ou_theta, ou_sigma;
};

// Arguments of rollout_eval (see there).
struct EvalArgs : PolicyWeights {
  const float* start_state;  // (N, kStateDim) start of episode 0, or nullptr
  float* ep_ret;             // (N, E)
  int* ep_len;               // (N, E)
  int N, E, D;
  unsigned seed;
  int max_episode_steps;
};

// control word written by thread 0 at the end of a step
constexpr int kEvalGoOn = 0, kEvalNextEpisode = 1, kEvalAllDone = 2;

// ---- LDS and step parts shared by both kernels -----------------------------
// The LDS block of a kernel: the recurrent part (b128 broadcast reads, hence
// the alignment), the K leading head columns ([a][k]), the env's observation
// (FE = kObsDim values; an env with its own observe() keeps its kStateDim
// state values behind them, FE = kObsDim + kStateDim: env_state_lds) and the
// reset uniforms of the step. Separate arrays on purpose: as members of one
// struct they cost the Gaussian rollout about 1 % (the compiler lays out and
// addresses separate arrays better; profiles/device_rollout.md).
#define PDRL_ROLLOUT_LDS(H, FE, K, R)                             \
  __shared__ __attribute__((aligned(16))) float s_xb[H];         \
  __shared__ __attribute__((aligned(16))) float s_h[H];          \
  __shared__ __attribute__((aligned(16))) float s_c[H];          \
  __shared__ __attribute__((aligned(16))) float s_gates[4 * H];  \
  __shared__ float s_hw[K * H];                                  \
  __shared__ float s_obs[FE];                                    \
  __shared__ float s_ur[R]

template <typename Env>
constexpr int kEnvLdsFloats =
    Env::kObsDim + (EnvObs<Env>::kIdentity ? 0 : EnvObs<Env>::kStateDim);

// Where the env's state lives: in the observation array itself (identity
// env) or right behind it.
template <typename Env>
__device__ __forceinline__ float* env_state_lds(float* s_obs) {
  if constexpr (EnvObs<Env>::kIdentity)
    return s_obs;
  else
    return s_obs + Env::kObsDim;
}

// Thread 0, start of a launch: the first state into LDS and, where the env
// has its own observe(), its observation.
template <typename Env>
__device__ __forceinline__ void publish_state(const float* st, float* s_obs,
                                              float* s_state) {
  constexpr int SD = EnvObs<Env>::kStateDim;
#pragma unroll
  for (int k = 0; k < SD; ++k) s_state[k] = st[k];
  if constexpr (!EnvObs<Env>::kIdentity) {
    float ob[Env::kObsDim];
    Env::observe(st, ob);
#pragma unroll
    for (int k = 0; k < Env::kObsDim; ++k) s_obs[k] = ob[k];
  }
}

// Envs with their own observe() fill the scalar register file: the trig
// expansions come on top of the 23 argument pointers of a training launch,
// and the addresses the epilogue writes through, live over the whole step
// loop, are then spilt to VGPR lanes. Such an instance keeps the address of
// a persistent scalar in two VGPRs instead (kHold; otherwise nothing
// happens and the instance is what it was).
template <bool kHold, typename T>
__device__ __forceinline__ void hold_in_vgprs(T*& ptr) {
  if constexpr (kHold) asm volatile("" : "+v"(ptr));
}

// Head biases into registers (every thread), head columns into LDS.
template <int H, int K>
__device__ __forceinline__ void stage_heads(const PolicyWeights& p, int D,
                                            int tid, float* s_hw,
                                            float (&hb)[K]) {
#pragma unroll
  for (int a = 0; a < K; ++a) hb[a] = p.heads_b[a];
  for (int idx = tid; idx < K * H; idx += 4 * H) {
    const int a = idx / H, k = idx % H;
    s_hw[idx] = p.heads_w[k * D + a];
  }
}

// Wave 0: the K head outputs. The H-long dot products are split over the
// lanes and butterfly-reduced (a serial loop in one lane is ~H dependent LDS
// round trips — it dominated the step). Static indices: lg stays in VGPRs.
template <int H, int K>
__device__ __forceinline__ void reduce_heads(const float* s_h,
                                             const float* s_hw,
                                             const float (&hb)[K], int lane,
                                             float (&lg)[K]) {
#pragma unroll
  for (int a = 0; a < K; ++a) {
    float part = 0.0f;
    for (int k = lane; k < H; k += kWave)
      part = fmaf(s_h[k], s_hw[a * H + k], part);
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1)
      part += __shfl_xor(part, off, kWave);
    lg[a] = part + hb[a];
  }
}

// Fresh recurrent state. Thread j is the only reader of s_h[j] / s_c[j]
// before the next barrier.
template <int H>
__device__ __forceinline__ void zero_recurrent(int tid, float* s_h,
                                               float* s_c) {
  if (tid < H) {
    s_h[tid] = 0.0f;
    s_c[tid] = 0.0f;
  }
}

// Side lane k of [0, R): uniform k of a reset keyed by counter ``ctr``.
template <int R>
__device__ __forceinline__ void draw_reset_uniform(int k, float* s_ur,
                                                   unsigned seed, int n,
                                                   unsigned ctr) {
  if (k < R)
    s_ur[k] = pdrl_rng::uniform(seed, (unsigned)n, ctr, (unsigned)k + 1u);
}

// ---- policy schemes ---------------------------------------------------------
// A scheme is what differs between the kernels' instances. Every scheme has
//   Env, kHeads   the env traits; the number of leading head columns read
//   Lds           its private LDS, written by side(), read by post()
//   Choice        what thread 0 carries over the fourth barrier
//   side(lane, s_state, lds, s_ur, seed, n, ctr)
//                 wave 1 (lane = tid - kWave) while wave 0 reduces the heads:
//                 dynamics that need no action yet, random draws, and the
//                 uniforms of a reset caused by this step (hash counter ctr)
//   next_obs(ch, lds, fresh, st, ob)
//                 thread 0, envs with their own observe() only: the
//                 observation of the step's final state (``fresh``: a reset
//                 has replaced what post() yielded)
// A sampling scheme (rollout_train) also has Args, Regs (thread-0 registers
// carried over the steps and, through load / store, over the launches) and
//   pre(p, row, n, tick, lg, ch)      thread 0, before the barrier: what
//                 needs the heads only; records ``logits``
//   post(p, row, n, tick, ch, regs, lds, s_state, st, reward, terminated)
//                 thread 0, after it: records ``act`` and ``log_prob`` (or
//                 pre did), yields the step's outcome
// and a greedy scheme (rollout_eval), which records nothing,
//   pre(lg, ch) and post(ch, lds, s_state, st, reward, terminated).
// The precise libm forms throughout: parity of the sample against the oracle
// is what the tests measure.

struct NoRegs {
  template <typename Args>
  __device__ __forceinline__ void load(const Args&, int) {}
  template <typename Args>
  __device__ __forceinline__ void store(const Args&, int) const {}
  __device__ __forceinline__ void reset() {}
};

// Categorical policy over a discrete env. Wave 1 steps the dynamics for
// EVERY action (lane = action) and draws the reset uniforms, so thread 0's
// scalar chain (softmax / sample / log-prob, or the arg-max) and the env's
// (sin / cos / divides) run side by side; post only picks a candidate.
// Its LDS: the candidates of one step. An env with its own observe() also
// keeps every candidate's observation, so that picking stays a copy.
template <int A, int SD, int F, bool kIdentity>
struct CandidateLds {
  alignas(16) float cand[A * SD];  // next state for every action
  float crew[A];
  int cterm[A];
};
template <int A, int SD, int F>
struct CandidateLds<A, SD, F, false> {
  alignas(16) float cand[A * SD];
  float cobs[A * F];  // its observation
  float crew[A];
  int cterm[A];
};

template <typename EnvT>
struct CategoricalBase {
  using Env = EnvT;
  static constexpr int F = Env::kObsDim;
  static constexpr int SD = EnvObs<Env>::kStateDim;
  static constexpr bool kIdentity = EnvObs<Env>::kIdentity;
  static constexpr int A = Env::kActions;
  static constexpr int kHeads = A;

  using Lds = CandidateLds<A, SD, F, kIdentity>;
  struct Choice {
    int chosen = 0;
  };

  __device__ __forceinline__ static void side(int lane, const float* s_state,
                                              Lds& s, float* s_ur,
                                              unsigned seed, int n,
                                              unsigned ctr) {
    if (lane < A) {
      float st[SD];
#pragma unroll
      for (int k = 0; k < SD; ++k) st[k] = s_state[k];
      float reward;
      bool terminated;
      Env::step(st, lane, reward, terminated);
#pragma unroll
      for (int k = 0; k < SD; ++k) s.cand[lane * SD + k] = st[k];
      if constexpr (!kIdentity) {
        float ob[F];
        Env::observe(st, ob);
#pragma unroll
        for (int k = 0; k < F; ++k) s.cobs[lane * F + k] = ob[k];
      }
      s.crew[lane] = reward;
      s.cterm[lane] = terminated ? 1 : 0;
    } else {
      draw_reset_uniform<Env::kResetDraws>(lane - A, s_ur, seed, n, ctr);
    }
  }

  // greedy form of post(); the sampling scheme forwards to it
  __device__ __forceinline__ static void post(const Choice& ch, const Lds& s,
                                              const float*, float* st,
                                              float& reward,
                                              bool& terminated) {
#pragma unroll
    for (int k = 0; k < SD; ++k) st[k] = s.cand[ch.chosen * SD + k];
    reward = s.crew[ch.chosen];
    terminated = s.cterm[ch.chosen] != 0;
  }

  // Observation of the step's final state ``st`` (envs with their own
  // observe()): the chosen candidate's, unless a reset replaced the state
  // (rare), which is observed here.
  __device__ __forceinline__ static void next_obs(const Choice& ch,
                                                  const Lds& s, bool fresh,
                                                  const float* st, float* ob) {
    if constexpr (!kIdentity) {
      if (fresh) {
        Env::observe(st, ob);
      } else {
#pragma unroll
        for (int k = 0; k < F; ++k) ob[k] = s.cobs[ch.chosen * F + k];
      }
    }
  }
};

// Softmax, inverse-CDF sample against hash lane 0, log-prob.
template <typename EnvT>
struct CategoricalSample : CategoricalBase<EnvT> {
  using Base = CategoricalBase<EnvT>;
  using Args = RolloutArgs;
  using Regs = NoRegs;
  using typename Base::Choice;
  using typename Base::Lds;
  static constexpr int A = Base::A;

  __device__ __forceinline__ static void pre(const Args& p, long row, int n,
                                             unsigned tick,
                                             const float (&lg)[A],
                                             Choice& ch) {
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
    int chosen = A - 1;
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
    ch.chosen = chosen;
    p.act[row] = (float)chosen;
    p.log_prob[row] = lg_chosen - mx - logf(Z);
  }

  __device__ __forceinline__ static void post(const Args&, long, int, unsigned,
                                              const Choice& ch, Regs&,
                                              const Lds& s, const float*,
                                              float* st, float& reward,
                                              bool& terminated) {
    Base::post(ch, s, nullptr, st, reward, terminated);
  }
};

// Arg-max logit: strict > scan from action 0, so ties go to the lowest index.
template <typename EnvT>
struct CategoricalGreedy : CategoricalBase<EnvT> {
  using Base = CategoricalBase<EnvT>;
  using typename Base::Choice;
  using typename Base::Lds;
  static constexpr int A = Base::A;

  __device__ __forceinline__ static void pre(const float (&lg)[A],
                                             Choice& ch) {
    float best = lg[0];
#pragma unroll
    for (int a = 1; a < A; ++a) {
      if (lg[a] > best) {
        best = lg[a];
        ch.chosen = a;
      }
    }
  }
};

// Gaussian policy over a continuous env, action of width 1: head column 0 is
// mu. One side lane evaluates the env's action-independent drift, kResetDraws
// lanes draw the reset uniforms; thread 0 steps the one chosen action.
template <typename EnvT>
struct GaussianBase {
  using Env = EnvT;
  static constexpr int SD = EnvObs<Env>::kStateDim;
  // One tick has eight hash lanes: 1..4 reset, 5 / 6 the normal. A second
  // action dimension needs a wider counter (rollout_rng.h).
  static_assert(Env::kActDim == 1,
                "eight hash lanes per tick allow exactly one action dimension");

  __device__ __forceinline__ static void env_side(int lane,
                                                  const float* s_state,
                                                  float& s_drift, float* s_ur,
                                                  unsigned seed, int n,
                                                  unsigned ctr) {
    if (lane == 0) {
      float st[SD];
#pragma unroll
      for (int k = 0; k < SD; ++k) st[k] = s_state[k];
      s_drift = Env::drift(st);
    } else {
      draw_reset_uniform<Env::kResetDraws>(lane - 1, s_ur, seed, n, ctr);
    }
  }

  __device__ __forceinline__ static void env_step(const float* s_state,
                                                  float act, float drift,
                                                  float* st, float& reward,
                                                  bool& terminated) {
#pragma unroll
    for (int k = 0; k < SD; ++k) st[k] = s_state[k];
    Env::step(st, act, drift, reward, terminated);
  }

  // Thread 0 stepped the one chosen action, so it observes the outcome too
  // (envs with their own observe()). Observing in the body threads at the
  // top of the next step instead measured 29-32 % slower
  // (profiles/device_rollout.md).
  template <typename Choice, typename Lds>
  __device__ __forceinline__ static void next_obs(const Choice&, const Lds&,
                                                  bool, const float* st,
                                                  float* ob) {
    if constexpr (!EnvObs<Env>::kIdentity) Env::observe(st, ob);
  }
};

// Sampling schemes of cpu_actor.cpp::act_batch_gaussian. Heads: column 0 =
// mu, column 1 = std (Mode 0, PPO-C) or log_std (Mode 1, SAC-C); the
// ``logits`` field is [mu_raw | second_raw], ``act`` has width 1. Side lane 0
// turns hash lanes 5 / 6 into the step's standard normal (log / sqrt / cos).
template <typename EnvT, int Mode>
struct GaussianSample : GaussianBase<EnvT> {
  static_assert(Mode == 0 || Mode == 1, "Mode: 0 = PPO-C, 1 = SAC-C");
  using Base = GaussianBase<EnvT>;
  using Args = GaussianArgs;
  static constexpr int kHeads = 2;
  static constexpr float kHalfLog2Pi = 0.9189385f;

  struct Lds {
    float normal;
    float drift;
  };
  struct Choice {
    float loc = 0.0f, sd = 0.0f, ls = 0.0f;
  };
  struct Regs {  // the OU exploration state (Mode 1)
    static constexpr bool kHold = !EnvObs<EnvT>::kIdentity;
    float ou = 0.0f;
    float* ou_ptr = nullptr;  // kHold only: see hold_in_vgprs
    __device__ __forceinline__ void load(const Args& p, int n) {
      if constexpr (Mode == 1 && kHold) {
        ou_ptr = p.ou_state + n;
        hold_in_vgprs<true>(ou_ptr);
        ou = *ou_ptr;
      } else if constexpr (Mode == 1) {
        ou = p.ou_state[n];
      }
    }
    __device__ __forceinline__ void store(const Args& p, int n) const {
      if constexpr (Mode == 1 && kHold)
        *ou_ptr = ou;
      else if constexpr (Mode == 1)
        p.ou_state[n] = ou;
    }
    __device__ __forceinline__ void reset() { ou = 0.0f; }
  };

  __device__ __forceinline__ static void side(int lane, const float* s_state,
                                              Lds& s, float* s_ur,
                                              unsigned seed, int n,
                                              unsigned ctr) {
    if (lane == 0) {
      // Box-Muller on hash lanes 5 (radius) and 6 (angle); 1 - u5 is exact
      // in fp32 and never 0
      const float u5 = pdrl_rng::uniform(seed, (unsigned)n, ctr, 5u);
      const float u6 = pdrl_rng::uniform(seed, (unsigned)n, ctr, 6u);
      s.normal = __fmul_rn(sqrtf(__fmul_rn(-2.0f, logf(1.0f - u5))),
                           cosf(__fmul_rn(6.2831855f, u6)));
    } else {
      Base::env_side(lane - 1, s_state, s.drift, s_ur, seed, n, ctr);
    }
  }

  // Mode 0, PPO-C: Normal(tanh(mu), softplus(std) + 1e-4), loc = mean and
  // ls = log(sd); mode 1, SAC-C: tanh-squashed Normal(mu, exp(clamp(log_std))),
  // loc = mu and ls the clamped log_std. Runs under wave 1's chains.
  __device__ __forceinline__ static void pre(const Args& p, long row, int,
                                             unsigned, const float (&lg)[2],
                                             Choice& ch) {
    p.logits[row * 2] = lg[0];
    p.logits[row * 2 + 1] = lg[1];
    if constexpr (Mode == 0) {
      ch.loc = tanhf(lg[0]);
      ch.sd = (lg[1] > 20.0f ? lg[1] : log1pf(expf(lg[1]))) + 1e-4f;
      ch.ls = logf(ch.sd);
    } else {
      ch.loc = lg[0];
      ch.ls = fminf(fmaxf(lg[1], -20.0f), 2.0f);
      ch.sd = expf(ch.ls);
    }
  }

  // sample, log-prob, env step
  __device__ __forceinline__ static void post(const Args& p, long row, int n,
                                              unsigned tick, const Choice& ch,
                                              Regs& regs, const Lds& s,
                                              const float* s_state, float* st,
                                              float& reward,
                                              bool& terminated) {
    const float nrm = s.normal;
    float act, lp;
    if constexpr (Mode == 0) {
      // the action is stored unclipped, as the workers do
      act = __fadd_rn(ch.loc, __fmul_rn(ch.sd, nrm));
      lp = -0.5f * nrm * nrm - ch.ls - kHalfLog2Pi;
    } else {
      const float mu = ch.loc;
      float z, quad;
      if (n < p.ou_envs || tick <= p.warmup_steps) {
        // OU exploration: correlated noise replaces the policy sample; the
        // log-prob is the policy's density at that action
        regs.ou = __fadd_rn(__fsub_rn(regs.ou, __fmul_rn(p.ou_theta, regs.ou)),
                            __fmul_rn(p.ou_sigma, nrm));
        z = regs.ou;
        const float q = (z - mu) / ch.sd;
        quad = -0.5f * (q * q);
      } else {
        z = __fadd_rn(mu, __fmul_rn(ch.sd, nrm));
        quad = -0.5f * nrm * nrm;
      }
      act = tanhf(z);
      // 1 - a*a + 1e-7 without fma contraction: with the same action it
      // equals the oracle's value to the last bit, so the logf that
      // amplifies it (by up to 2 / (1 - a*a)) sees no extra difference
      const float om =
          __fadd_rn(__fsub_rn(1.0f, __fmul_rn(act, act)), 1e-7f);
      lp = quad - ch.ls - kHalfLog2Pi - logf(om);
    }
    p.act[row] = act;
    p.log_prob[row] = lp;
    Base::env_step(s_state, act, s.drift, st, reward, terminated);
  }
};

// tanh(mu): the mean of PPO-C's Normal(tanh(mu), ·) and of SAC-C's squashed
// Gaussian at zero noise, so only head column 0 is read.
template <typename EnvT>
struct GaussianGreedy : GaussianBase<EnvT> {
  using Base = GaussianBase<EnvT>;
  static constexpr int kHeads = 1;

  struct Lds {
    float drift;
  };
  struct Choice {
    float act = 0.0f;
  };

  __device__ __forceinline__ static void side(int lane, const float* s_state,
                                              Lds& s, float* s_ur,
                                              unsigned seed, int n,
                                              unsigned ctr) {
    Base::env_side(lane, s_state, s.drift, s_ur, seed, n, ctr);
  }

  __device__ __forceinline__ static void pre(const float (&lg)[1],
                                             Choice& ch) {
    ch.act = tanhf(lg[0]);
  }

  __device__ __forceinline__ static void post(const Choice& ch, const Lds& s,
                                              const float* s_state, float* st,
                                              float& reward,
                                              bool& terminated) {
    Base::env_step(s_state, ch.act, s.drift, st, reward, terminated);
  }
};

// ---- training rollout: S steps of every env, (N, S, ·) batch ---------------
template <int H, typename Policy>
__global__ __launch_bounds__(4 * H) void rollout_train(
    typename Policy::Args p) {
  using Env = typename Policy::Env;
  constexpr int F = Env::kObsDim;
  constexpr int SD = EnvObs<Env>::kStateDim;
  constexpr bool kIdentity = EnvObs<Env>::kIdentity;
  static_assert(!kIdentity || SD == F, "identity env: the obs is the state");
  constexpr int K = Policy::kHeads;
  constexpr int R = Env::kResetDraws;
  static_assert(R >= 1 && R <= 4, "reset draws use hash lanes 1..4");
  const int tid = threadIdx.x;
  const int n = blockIdx.x;
  if (n >= p.N) return;  // uniform per workgroup

  PDRL_ROLLOUT_LDS(H, kEnvLdsFloats<Env>, K, R);
  float* const s_state = env_state_lds<Env>(s_obs);
  __shared__ typename Policy::Lds sp;
  __shared__ float s_fir;
  __shared__ int s_reset;

  RecurrentCore<H, F> core;
  core.load(p, tid, n, s_h, s_c);
  float hb[K];
  stage_heads<H, K>(p, p.D, tid, s_hw, hb);
  if constexpr (kIdentity) {
    if (tid < F) s_obs[tid] = p.env_state[(long)n * F + tid];
  } else if (tid == 0) {
    float st[SD];
#pragma unroll
    for (int k = 0; k < SD; ++k) st[k] = p.env_state[(long)n * SD + k];
    publish_state<Env>(st, s_obs, s_state);
  }

  // episode bookkeeping and the scheme's registers live in thread 0 across
  // the S steps
  int steps = 0;
  float run = 0.0f;
  typename Policy::Regs regs;
  // every thread tracks the tick (hash counter)
  unsigned* tick_ptr = p.tick + n;
  hold_in_vgprs<!kIdentity>(tick_ptr);
  unsigned tick = *tick_ptr;
  if (tid == 0) {
    s_fir = p.is_fir[n];
    steps = p.ep_steps[n];
    run = p.ep_run[n];
    regs.load(p, n);
  }
  __syncthreads();

  for (int t = 0; t < p.S; ++t) {
    const long row = (long)n * p.S + t;
    tick += 1u;
    // record the pre-step obs / hx / cx / is_fir; body, gates, cell update
    core.step(p, tid, row, s_obs, &s_fir, s_xb, s_h, s_c, s_gates);

    float lg[K];
    if (tid < kWave)
      reduce_heads<H, K>(s_h, s_hw, hb, tid, lg);
    else
      Policy::side(tid - kWave, s_state, sp, s_ur, p.seed, n, tick);
    // thread 0 already holds the reduced heads: no barrier needed
    typename Policy::Choice ch;
    if (tid == 0) Policy::pre(p, row, n, tick, lg, ch);
    __syncthreads();

    // the step's outcome; termination, auto-reset (thread 0)
    if (tid == 0) {
      float st[SD];
      float reward;
      bool terminated;
      Policy::post(p, row, n, tick, ch, regs, sp, s_state, st, reward,
                   terminated);
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
        regs.reset();
      }
#pragma unroll
      for (int k = 0; k < SD; ++k) s_state[k] = st[k];
      if constexpr (!kIdentity) {
        float ob[F];
        Policy::next_obs(ch, sp, reset, st, ob);
#pragma unroll
        for (int k = 0; k < F; ++k) s_obs[k] = ob[k];
      }
      s_fir = reset ? 1.0f : 0.0f;
      s_reset = reset ? 1 : 0;
    }
    __syncthreads();
    if (s_reset != 0) zero_recurrent<H>(tid, s_h, s_c);
  }

  // persist the per-env state for the next launch
  if (tid < H) {
    p.h[(long)n * H + tid] = s_h[tid];
    p.c[(long)n * H + tid] = s_c[tid];
  }
  if (tid < SD) p.env_state[(long)n * SD + tid] = s_state[tid];
  if (tid == 0) {
    p.is_fir[n] = s_fir;
    p.ep_steps[n] = steps;
    p.ep_run[n] = run;
    *tick_ptr = tick;
    regs.store(p, n);
  }
}

// ---- greedy evaluation: whole episodes in one launch ------------------------
// E episodes per env back to back under the scheme's deterministic action;
// one return and one length per (env, episode). Geometry, weight residency
// and the wave 0 / wave 1 overlap are those of rollout_train; what is gone is
// everything a batch needs: no (N, S, ·) record, no softmax, no log-prob, no
// sampling draw, no OU state — and nothing persistent is read or written, so
// a launch cannot disturb the training envs. Episode e of env n starts from
// Env::reset of hash tick e (lanes 1..draws) with h = c = 0, a pure function
// of (seed, n, e); ``start_state`` may replace the start of episode 0. An
// episode ends on ``terminated`` or at max_episode_steps.
//
// The step loop is bounded by E * max_episode_steps (every episode takes at
// most max_episode_steps steps, so that many iterations finish all of them);
// the workgroup-uniform control word in LDS only leaves it early.
template <int H, typename Policy>
__global__ __launch_bounds__(4 * H) void rollout_eval(EvalArgs p) {
  using Env = typename Policy::Env;
  constexpr int F = Env::kObsDim;
  constexpr int SD = EnvObs<Env>::kStateDim;
  constexpr bool kIdentity = EnvObs<Env>::kIdentity;
  static_assert(!kIdentity || SD == F, "identity env: the obs is the state");
  constexpr int K = Policy::kHeads;
  constexpr int R = Env::kResetDraws;
  static_assert(R >= 1 && R <= 4, "reset draws use hash lanes 1..4");
  const int tid = threadIdx.x;
  const int n = blockIdx.x;
  if (n >= p.N) return;  // uniform per workgroup

  // s_ur: start state of the next episode
  PDRL_ROLLOUT_LDS(H, kEnvLdsFloats<Env>, K, R);
  float* const s_state = env_state_lds<Env>(s_obs);
  __shared__ typename Policy::Lds sp;
  __shared__ int s_ctl;

  RecurrentCore<H, F> core;
  core.load_weights(p, tid);
  float hb[K];
  stage_heads<H, K>(p, p.D, tid, s_hw, hb);
  zero_recurrent<H>(tid, s_h, s_c);
  if (tid == 0) {
    float st[SD];
    if (p.start_state != nullptr) {
#pragma unroll
      for (int k = 0; k < SD; ++k) st[k] = p.start_state[(long)n * SD + k];
    } else {
      float u[R];
#pragma unroll
      for (int k = 0; k < R; ++k)
        u[k] = pdrl_rng::uniform(p.seed, (unsigned)n, 0u, (unsigned)k + 1u);
      Env::reset(st, u);
    }
    publish_state<Env>(st, s_obs, s_state);
  }
  __syncthreads();

  // every thread tracks the episode index (hash counter of the next start
  // state); the step count and the running return live in thread 0
  int episode = 0, steps = 0;
  float run = 0.0f;
  const int max_iters = p.E * p.max_episode_steps;  // <= 2^22 (binding)
  for (int it = 0; it < max_iters; ++it) {
    core.advance(p, tid, s_obs, s_xb, s_h, s_c, s_gates);

    float lg[K];
    if (tid < kWave)
      reduce_heads<H, K>(s_h, s_hw, hb, tid, lg);
    else
      Policy::side(tid - kWave, s_state, sp, s_ur, p.seed, n,
                   (unsigned)episode + 1u);
    typename Policy::Choice ch;
    if (tid == 0) Policy::pre(lg, ch);
    __syncthreads();

    // the step's outcome; episode end and fresh start (thread 0)
    if (tid == 0) {
      float st[SD];
      float reward;
      bool terminated;
      Policy::post(ch, sp, s_state, st, reward, terminated);
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
      for (int k = 0; k < SD; ++k) s_state[k] = st[k];
      if constexpr (!kIdentity) {
        float ob[F];
        Policy::next_obs(ch, sp, done, st, ob);
#pragma unroll
        for (int k = 0; k < F; ++k) s_obs[k] = ob[k];
      }
      s_ctl = ctl;
    }
    __syncthreads();
    const int ctl = s_ctl;  // the same value in every thread of the workgroup
    if (ctl == kEvalAllDone) break;
    if (ctl == kEvalNextEpisode) {
      episode += 1;
      zero_recurrent<H>(tid, s_h, s_c);
    }
  }
}

// ---- host side --------------------------------------------------------------
// f(std::integral_constant<int, H>) launches one kernel for the hidden size.
template <typename Fn>
void dispatch_hidden(int H, Fn&& f) {
  switch (H) {
    case 32: f(std::integral_constant<int, 32>{}); break;
    case 64: f(std::integral_constant<int, 64>{}); break;
    case 128: f(std::integral_constant<int, 128>{}); break;
    default:
      TORCH_CHECK(false, "hidden size ", H, " unsupported (32/64/128)");
  }
  HIP_CHECK_LAST();
}

template <typename Policy>
void launch_train(const typename Policy::Args& a, int H) {
  dispatch_hidden(H, [&](auto h) {
    constexpr int kH = decltype(h)::value;
    hipLaunchKernelGGL((rollout_train<kH, Policy>), dim3(a.N), dim3(4 * kH),
                       0, current_stream(), a);
  });
}

template <typename Policy>
void launch_eval(const EvalArgs& a, int H) {
  dispatch_hidden(H, [&](auto h) {
    constexpr int kH = decltype(h)::value;
    hipLaunchKernelGGL((rollout_eval<kH, Policy>), dim3(a.N), dim3(4 * kH), 0,
                       current_stream(), a);
  });
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
// A is also the width of the ``logits`` field. The env fixes the core's
// obs_dim (F_env) and, on its own, the width of env_state (SD_env).
RolloutArgs pack_rollout_args(
    const at::Tensor& body_w, const at::Tensor& body_b, const at::Tensor& w_ih,
    const at::Tensor& w_hh, const at::Tensor& b_g, const at::Tensor& heads_w,
    const at::Tensor& heads_b, at::Tensor& env_state, at::Tensor& h,
    at::Tensor& c, at::Tensor& is_fir, at::Tensor& ep_steps,
    at::Tensor& ep_run, at::Tensor& tick, at::Tensor& obs, at::Tensor& act,
    at::Tensor& rew, at::Tensor& logits, at::Tensor& log_prob,
    at::Tensor& is_fir_out, at::Tensor& hx, at::Tensor& cx,
    at::Tensor& ep_ret, long F_env, const char* env_msg, long SD_env, long A,
    long seed, long time_horizon, long max_episode_steps) {
  RolloutArgs a;
  static_cast<PolicyWeights&>(a) = pack_policy_weights(
      body_w, body_b, w_ih, w_hh, b_g, heads_w, heads_b, F_env, env_msg, A);
  TORCH_CHECK(obs.dim() == 3, "rollout: bad tensor ranks");
  TORCH_CHECK(env_state.dim() == 2 && env_state.size(1) == SD_env,
              "rollout: env_state must be (N, ", SD_env,
              "), the env's state vector, got ", env_state.sizes());
  const long F = body_w.size(0), H = body_w.size(1), D = heads_w.size(1);
  const long N = env_state.size(0), S = obs.size(1);
  TORCH_CHECK(N >= 1 && S >= 1, "rollout: empty batch");
  check_f32(env_state, N * SD_env, "env_state");
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
    const char* env_msg, long SD_env, long A, long seed,
    long max_episode_steps) {
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
    TORCH_CHECK(start_state->dim() == 2 && start_state->size(1) == SD_env,
                "rollout_eval: start_state must be (N, ", SD_env,
                "), the env's state vector");
    check_f32(*start_state, N * SD_env, "start_state");
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

// Categorical policy. env_id: see with_discrete_env.
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
  with_discrete_env(env_id, [&](auto env, const char* env_msg) {
    using Policy = CategoricalSample<decltype(env)>;
    const RolloutArgs a = pack_rollout_args(
        body_w, body_b, w_ih, w_hh, b_g, heads_w, heads_b, env_state, h, c,
        is_fir, ep_steps, ep_run, tick, obs, act, rew, logits, log_prob,
        is_fir_out, hx, cx, ep_ret, Policy::Env::kObsDim, env_msg,
        EnvObs<typename Policy::Env>::kStateDim, Policy::kHeads, seed,
        time_horizon, max_episode_steps);
    launch_train<Policy>(a, (int)body_w.size(1));
  });
}

// Gaussian-policy sibling. env_id: see with_continuous_env. mode: 0 = heads
// (mu, std), PPO-C sampling; 1 = heads (mu, log_std), SAC-C sampling with
// optional OU exploration (ou_envs, warmup_steps; see GaussianArgs).
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
  with_continuous_env(env_id, [&](auto env, const char* env_msg) {
    using Env = decltype(env);
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
        is_fir_out, hx, cx, ep_ret, Env::kObsDim, env_msg,
        EnvObs<Env>::kStateDim, 2, seed, time_horizon, max_episode_steps);
    TORCH_CHECK(a.D >= 2, "heads_w shape");
    check_f32(ou_state, a.N, "ou_state");
    TORCH_CHECK(ou_state.device() == body_w.device(),
                "rollout: tensors on different devices");
    a.ou_state = ou_state.data_ptr<float>();
    a.ou_envs = (int)std::min<long>(ou_envs, INT32_MAX);
    a.warmup_steps = (unsigned)std::min<long>(warmup_steps, UINT32_MAX);
    a.ou_theta = (float)ou_theta;
    a.ou_sigma = (float)ou_sigma;
    if (mode == 0)
      launch_train<GaussianSample<Env, 0>>(a, (int)body_w.size(1));
    else
      launch_train<GaussianSample<Env, 1>>(a, (int)body_w.size(1));
  });
}

// Greedy evaluation: E = ep_ret.size(1) whole episodes per env in one launch.
template <typename Policy>
static void rollout_eval_hip(
    const at::Tensor& body_w, const at::Tensor& body_b, const at::Tensor& w_ih,
    const at::Tensor& w_hh, const at::Tensor& b_g, const at::Tensor& heads_w,
    const at::Tensor& heads_b, at::Tensor& ep_ret, at::Tensor& ep_len,
    const c10::optional<at::Tensor>& start_state, const char* env_msg,
    long seed, long max_episode_steps) {
  const EvalArgs a = pack_eval_args(
      body_w, body_b, w_ih, w_hh, b_g, heads_w, heads_b, ep_ret, ep_len,
      start_state, Policy::Env::kObsDim, env_msg,
      EnvObs<typename Policy::Env>::kStateDim, Policy::kHeads, seed,
      max_episode_steps);
  launch_eval<Policy>(a, (int)body_w.size(1));
}

// Discrete policy, arg-max action. env_id as in rollout_discrete_hip.
void rollout_eval_discrete_hip(
    const at::Tensor& body_w, const at::Tensor& body_b, const at::Tensor& w_ih,
    const at::Tensor& w_hh, const at::Tensor& b_g, const at::Tensor& heads_w,
    const at::Tensor& heads_b, at::Tensor& ep_ret, at::Tensor& ep_len,
    const c10::optional<at::Tensor>& start_state, long env_id, long seed,
    long max_episode_steps) {
  with_discrete_env(env_id, [&](auto env, const char* env_msg) {
    rollout_eval_hip<CategoricalGreedy<decltype(env)>>(
        body_w, body_b, w_ih, w_hh, b_g, heads_w, heads_b, ep_ret, ep_len,
        start_state, env_msg, seed, max_episode_steps);
  });
}

// Gaussian policy, tanh(mu) for both head schemes. env_id as in
// rollout_gaussian_hip.
void rollout_eval_gaussian_hip(
    const at::Tensor& body_w, const at::Tensor& body_b, const at::Tensor& w_ih,
    const at::Tensor& w_hh, const at::Tensor& b_g, const at::Tensor& heads_w,
    const at::Tensor& heads_b, at::Tensor& ep_ret, at::Tensor& ep_len,
    const c10::optional<at::Tensor>& start_state, long env_id, long seed,
    long max_episode_steps) {
  with_continuous_env(env_id, [&](auto env, const char* env_msg) {
    rollout_eval_hip<GaussianGreedy<decltype(env)>>(
        body_w, body_b, w_ih, w_hh, b_g, heads_w, heads_b, ep_ret, ep_len,
        start_state, env_msg, seed, max_episode_steps);
  });
}

// Host evaluation of the rollout's uniform (same header as the kernel).
double rollout_uniform_host(long seed, long env, long tick, long k) {
  return (double)pdrl_rng::uniform((uint32_t)seed, (uint32_t)env,
                                   (uint32_t)tick, (uint32_t)k);
}
