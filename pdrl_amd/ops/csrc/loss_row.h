// Row-local on-policy losses (IMPALA / PPO / PPO-Continuous / V-MPO) for ONE
// batch row: policy stats, V-trace/GAE scan, analytic packed head grads,
// per-row loss-stat partials. These are the ONLY implementation of the
// on-policy loss math; fwd_loss.hip runs them either fused into the
// forward/backward launches (H=64) or as stand-alone row-parallel launches
// (any H). The losses have NO cross-row coupling except the monitoring
// means (and V-MPO's top-half selection, vmpo_loss.hip).
#pragma once

#include "common.h"

constexpr int kAlgoImpala = 0;
constexpr int kAlgoPpo = 1;
constexpr int kAlgoPpoC = 2;
constexpr int kAlgoVmpo = 3;
// block size of the stand-alone launches; the row functions give one thread
// to each of a row's S steps, so S <= kLossThreads (checked on the host)
constexpr int kLossThreads = 256;

__device__ __forceinline__ float ms_huber(float d) {
  const float a = fabsf(d);
  return (a < 1.0f) ? 0.5f * d * d : a - 0.5f;
}
__device__ __forceinline__ float ms_huber_grad(float d) {
  return fminf(fmaxf(d, -1.0f), 1.0f);
}


// Row-local IMPALA/PPO loss for batch row b: categorical stats, V-trace or
// TD+GAE scan, analytic packed head grads, per-row loss-stat partials.
// The INPUTS (outs, act, behav, rew, fir) are read at row offset si, the
// outputs (gouts, stats_part) are written at row b. By default the inputs
// are the global (B, S, ...) arrays and si = b*S; with kRowView they are a
// view of row b alone (si = 0): the row step (fwd_loss.hip) passes LDS copies
// of the row's inputs, so neither lane 0's scan nor the gradient loop issues
// a global load there.
// stats_part: (B, 8) per-row loss partials [pl, vl, es, ravg/rsum, rg,
// rmin, rmax] written with PLAIN stores — a per-launch accumulator would
// funnel 5-7 atomics per block onto one cache line, which measured ~10 µs
// at B=128 (the whole benefit of fusing the loss into the forward). The
// consumer (onpolicy_stats_reduce below) reduces the B rows in parallel.
template <bool kRowView = false>
__device__ void onpolicy_loss_row(
    int algo, const float* __restrict__ outs, const float* __restrict__ act,
    const float* __restrict__ behav, const float* __restrict__ rew,
    const float* __restrict__ fir, float* __restrict__ gouts,
    float* __restrict__ stats_part, int b, int B, int S,
    int A, float gamma, float lmbda, float rho_bar, float rho_min,
    float c_bar, float rew_scale, float cp, float cv, float ce,
    float eps_clip, float creg, char* smem) {
  const int D = A + 1;
  const int T = S - 1;
  const int BT = B * T;
  const int tid = threadIdx.x;
  float* s_logp = reinterpret_cast<float*>(smem);  // (S)
  float* s_lse = s_logp + S;                       // (S)
  float* s_ent = s_lse + S;                        // (S)
  float* s_w = s_ent + S;                          // (T) rho (IMPALA)
  float* s_adv = s_w + S;                          // (T)
  float* s_ret = s_adv + S;                        // (T) vs (IMPALA) | td (PPO)
  const long sb = (long)b * S;
  const long si = kRowView ? 0 : sb;  // row offset of the inputs

  if (tid < S) {
    const float* z = outs + (si + tid) * D;
    float m = z[0];
    for (int j = 1; j < A; ++j) m = fmaxf(m, z[j]);
    float s = 0.f;
    for (int j = 0; j < A; ++j) s += __expf(z[j] - m);
    const float l = m + __logf(s);
    float h = 0.f;
    for (int j = 0; j < A; ++j) {
      const float lp = z[j] - l;
      h -= __expf(lp) * lp;
    }
    s_logp[tid] = z[(int)act[si + tid]] - l;
    s_lse[tid] = l;
    s_ent[tid] = h;
  }
  __syncthreads();

  if (tid == 0) {
    // scans + this row's loss partials (T is tiny: serial on one lane)
    float pl = 0.f, vl = 0.f, es = 0.f, rs = 0.f, rg = 0.f;
    if (algo == kAlgoImpala) {
      float acc = 0.f;
      for (int t = T - 1; t >= 0; --t) {
        const float ratio = __expf(s_logp[t] - behav[si + t]);
        const float rho = fminf(fmaxf(ratio, rho_min), rho_bar);
        const float c = fminf(ratio, c_bar);
        const float mask = 1.f - fir[si + t + 1];
        const float vt = outs[(si + t) * D + A];
        const float vn = outs[(si + t + 1) * D + A];
        const float delta =
            rho * (rew[si + t] * rew_scale + gamma * mask * vn - vt);
        acc = fmaf(gamma * mask * c, acc, delta);
        s_w[t] = rho;
        s_ret[t] = vt + acc;
      }
      for (int t = 0; t < T; ++t) {
        const float mask = 1.f - fir[si + t + 1];
        const float vnext = (t + 1 < T) ? s_ret[t + 1] : outs[(si + T) * D + A];
        s_adv[t] = s_w[t] * (rew[si + t] * rew_scale + gamma * mask * vnext -
                             outs[(si + t) * D + A]);
      }
      for (int t = 0; t < T; ++t) {
        pl -= s_logp[t] * s_adv[t];
        vl += ms_huber(outs[(si + t) * D + A] - s_ret[t]);
        es += s_ent[t];
        rs += s_w[t];
        for (int j = 0; j < A; ++j) {
          const float z = outs[(si + t) * D + j];
          rg = fmaf(z, z, rg);
        }
      }
    } else {  // PPO: TD target + GAE, clipped surrogate
      float run = 0.f;
      for (int t = T - 1; t >= 0; --t) {
        const float mask = 1.f - fir[si + t + 1];
        const float tdv = rew[si + t] * rew_scale +
                          gamma * mask * outs[(si + t + 1) * D + A];
        const float delta = tdv - outs[(si + t) * D + A];
        run = fmaf(gamma * lmbda * mask, run, delta);
        s_ret[t] = tdv;
        s_adv[t] = run;
      }
      float rmin = 1e30f, rmax = -1e30f;
      for (int t = 0; t < T; ++t) {
        const float r = __expf(s_logp[t] - behav[si + t]);
        const float a = s_adv[t];
        const float s1 = r * a;
        const float s2 =
            fminf(fmaxf(r, 1.f - eps_clip), 1.f + eps_clip) * a;
        pl -= fminf(s1, s2);
        vl += ms_huber(outs[(si + t) * D + A] - s_ret[t]);
        es += s_ent[t];
        rs += r;
        rmin = fminf(rmin, r);
        rmax = fmaxf(rmax, r);
        for (int j = 0; j < A; ++j) {
          const float z = outs[(si + t) * D + j];
          rg = fmaf(z, z, rg);
        }
      }
      stats_part[(long)b * 8 + 5] = rmin;
      stats_part[(long)b * 8 + 6] = rmax;
    }
    float* sp = stats_part + (long)b * 8;
    sp[0] = pl;
    sp[1] = vl;
    sp[2] = es;
    sp[3] = rs;
    sp[4] = rg;
  }
  __syncthreads();

  // analytic packed head grads, elementwise over this row
  const float invN = 1.0f / BT;
  const float dreg = 2.0f * creg * invN / A;
  for (int idx = tid; idx < S * D; idx += (int)blockDim.x) {
    const int t = idx / D, j = idx % D;
    float* g = gouts + (sb + t) * D;
    if (t >= T) {
      g[j] = 0.f;
      continue;
    }
    const float* z = outs + (si + t) * D;
    if (j == A) {
      g[A] = cv * ms_huber_grad(z[A] - s_ret[t]) * invN;
      continue;
    }
    float dlogp;
    if (algo == kAlgoImpala) {
      dlogp = -cp * s_adv[t] * invN;
    } else {
      const float r = __expf(s_logp[t] - behav[si + t]);
      const float a_v = s_adv[t];
      const bool inside = (r > 1.f - eps_clip) && (r < 1.f + eps_clip);
      const float s1 = r * a_v;
      const float s2 = fminf(fmaxf(r, 1.f - eps_clip), 1.f + eps_clip) * a_v;
      const float gr = (inside || s1 < s2) ? a_v * r : 0.f;
      dlogp = -cp * gr * invN;
    }
    const float dH = -ce * invN;
    const float H = s_ent[t];
    const float lp = z[j] - s_lse[t];
    const float pj = __expf(lp);
    const int a = (int)act[si + t];
    g[j] = dlogp * ((j == a ? 1.f : 0.f) - pj) + dH * (-pj * (lp + H)) +
           dreg * z[j];
  }
}


// Row-local PPO-Continuous loss (Gaussian tanh-mean policy; reference math:
// networks/models.py:103-118 + ppo/learning.py). Packed heads
// [mu | std | value], D = 2A+1.
// Same kRowView input views and per-row stats_part protocol as
// onpolicy_loss_row.
template <bool kRowView = false>
__device__ inline void ppoc_loss_row(
    const float* __restrict__ outs, const float* __restrict__ act,
    const float* __restrict__ behav, const float* __restrict__ rew,
    const float* __restrict__ fir, float* __restrict__ gouts,
    float* __restrict__ stats_part, int b, int B, int S, int A, float gamma,
    float lmbda, float rew_scale, float cp, float cv, float ce,
    float eps_clip, float creg, char* smem) {
  constexpr float kRowLogSqrt2Pi = 0.9189385332046727f;
  constexpr float kRowEntConst = 1.4189385332046727f;  // 0.5*(1+log(2*pi))
  const int D = 2 * A + 1;
  const int T = S - 1;
  const int BT = B * T;
  const int tid = threadIdx.x;
  float* s_logp = reinterpret_cast<float*>(smem);  // (S)
  float* s_ent = s_logp + S;                       // (S)
  float* s_adv = s_ent + S;                        // (T)
  float* s_ret = s_adv + S;                        // (T)
  const long sb = (long)b * S;
  const long si = kRowView ? 0 : sb;  // row offset of the inputs

  if (tid < S) {
    const float* z = outs + (si + tid) * D;
    float lp = 0.f, h = 0.f;
    for (int j = 0; j < A; ++j) {
      const float mut = tanhf(z[j]);
      const float sig = ((z[A + j] > 20.f) ? z[A + j]
                                           : log1pf(__expf(z[A + j]))) + 1e-4f;
      const float x = act[(si + tid) * A + j];
      const float d = (x - mut) / sig;
      lp += -0.5f * d * d - __logf(sig) - kRowLogSqrt2Pi;
      h += __logf(sig) + kRowEntConst;
    }
    s_logp[tid] = lp;
    s_ent[tid] = h;
  }
  __syncthreads();

  if (tid == 0) {
    float run = 0.f;
    for (int t = T - 1; t >= 0; --t) {
      const float mask = 1.f - fir[si + t + 1];
      const float tdv = rew[si + t] * rew_scale +
                        gamma * mask * outs[(si + t + 1) * D + 2 * A];
      const float delta = tdv - outs[(si + t) * D + 2 * A];
      run = fmaf(gamma * lmbda * mask, run, delta);
      s_ret[t] = tdv;
      s_adv[t] = run;
    }
    float pl = 0.f, vl = 0.f, es = 0.f, rs = 0.f, rg = 0.f;
    float rmin = 1e30f, rmax = -1e30f;
    for (int t = 0; t < T; ++t) {
      const float r = __expf(s_logp[t] - behav[si + t]);
      const float a = s_adv[t];
      const float s1 = r * a;
      const float s2 = fminf(fmaxf(r, 1.f - eps_clip), 1.f + eps_clip) * a;
      pl -= fminf(s1, s2);
      vl += ms_huber(outs[(si + t) * D + 2 * A] - s_ret[t]);
      es += s_ent[t];
      rs += r;
      rmin = fminf(rmin, r);
      rmax = fmaxf(rmax, r);
      for (int j = 0; j < 2 * A; ++j) {
        const float z = outs[(si + t) * D + j];
        rg = fmaf(z, z, rg);
      }
    }
    float* sp = stats_part + (long)b * 8;
    sp[0] = pl;
    sp[1] = vl;
    sp[2] = es;
    sp[3] = rs;
    sp[4] = rg;
    sp[5] = rmin;
    sp[6] = rmax;
  }
  __syncthreads();

  const float invN = 1.0f / BT;
  const float dreg = 2.0f * creg * invN / (2 * A);
  for (int idx = tid; idx < S * D; idx += (int)blockDim.x) {
    const int t = idx / D, j = idx % D;
    float* g = gouts + (sb + t) * D;
    if (t >= T) {
      g[j] = 0.f;
      continue;
    }
    const float a_v = s_adv[t];
    const float r = __expf(s_logp[t] - behav[si + t]);
    const bool inside = (r > 1.f - eps_clip) && (r < 1.f + eps_clip);
    const float s1 = r * a_v;
    const float s2 = fminf(fmaxf(r, 1.f - eps_clip), 1.f + eps_clip) * a_v;
    const float gr = (inside || s1 < s2) ? a_v * r : 0.f;
    const float dlogp = -cp * gr * invN;
    const float dH = -ce * invN;
    const float* z = outs + (si + t) * D;
    if (j == 2 * A) {
      g[j] = cv * ms_huber_grad(z[2 * A] - s_ret[t]) * invN;
    } else if (j < A) {
      const float mut = tanhf(z[j]);
      const float sig = ((z[A + j] > 20.f) ? z[A + j]
                                           : log1pf(__expf(z[A + j]))) + 1e-4f;
      const float x = act[(si + t) * A + j];
      const float diff = x - mut;
      const float dl_dmut = diff / (sig * sig);
      g[j] = dlogp * dl_dmut * (1.f - mut * mut) + dreg * z[j];
    } else {
      const int jj = j - A;
      const float mut = tanhf(z[jj]);
      const float sig = ((z[j] > 20.f) ? z[j] : log1pf(__expf(z[j]))) + 1e-4f;
      const float x = act[(si + t) * A + jj];
      const float diff = x - mut;
      const float dl_dsig = diff * diff / (sig * sig * sig) - 1.0f / sig;
      const float dH_dsig = 1.0f / sig;
      const float sgm = 1.0f / (1.0f + __expf(-z[j]));
      g[j] = (dlogp * dl_dsig + dH * dH_dsig) * sgm + dreg * z[j];
    }
  }
}

// ---- V-MPO row-local phases (reference math: v_mpo/learning.py:49-124).
// The cross-row phases — top-half selection, psi softmax, dual losses,
// stats — run between them in vmpo_loss.hip's single-block vmpo_mid_kernel.

// phases A+B for one row: log-softmax stats and the GAE scan, written to
// GLOBAL scratch consumed by the single-block middle kernel.
__device__ inline void vmpo_pre_row(
    const float* __restrict__ outs, const float* __restrict__ act,
    const float* __restrict__ rew, const float* __restrict__ fir,
    float* __restrict__ lse_g, float* __restrict__ logp_g,
    float* __restrict__ adv_g, float* __restrict__ td_g, int b, int S,
    int A, float gamma, float lmbda, float rew_scale) {
  const int D = A + 1;
  const int T = S - 1;
  const int tid = threadIdx.x;
  const long sb = (long)b * S, tb = (long)b * T;

  if (tid < S) {
    const float* z = outs + (sb + tid) * D;
    float mx = z[0];
    for (int j = 1; j < A; ++j) mx = fmaxf(mx, z[j]);
    float sum = 0.f;
    for (int j = 0; j < A; ++j) sum += __expf(z[j] - mx);
    const float l = mx + __logf(sum);
    lse_g[sb + tid] = l;
    logp_g[sb + tid] = z[(int)act[sb + tid]] - l;
  }
  __syncthreads();
  if (tid == 0) {
    float run = 0.f;
    for (int t = T - 1; t >= 0; --t) {
      const float mask = 1.f - fir[sb + t + 1];
      const float tdv = rew[sb + t] * rew_scale +
                        gamma * mask * outs[(sb + t + 1) * D + A];
      const float delta = tdv - outs[(sb + t) * D + A];
      run = fmaf(gamma * lmbda * mask, run, delta);
      td_g[tb + t] = tdv;
      adv_g[tb + t] = run;
    }
  }
}

// phase E for one row: analytic packed head grads from the middle kernel's
// psi weights and scalars ([7] = alpha).
__device__ inline void vmpo_grad_row(
    const float* __restrict__ outs, const float* __restrict__ act,
    const float* __restrict__ behav,  // (N,A) behaviour LOGITS
    const float* __restrict__ lse_g, const float* __restrict__ psi_g,
    const float* __restrict__ td_g, const float* __restrict__ scalars_g,
    float* __restrict__ gouts, int b, int B, int S, int A, float cp,
    float cv, float creg) {
  const int D = A + 1;
  const int T = S - 1;
  const int BT = B * T;
  const int tid = threadIdx.x;
  const long sb = (long)b * S, tb = (long)b * T;
  const float alpha_v = scalars_g[7];
  const float invBT = 1.0f / BT;
  const float dreg = 2.0f * creg * invBT / A;

  for (int idx = tid; idx < S * D; idx += (int)blockDim.x) {
    const int t = idx / D, j = idx % D;
    float* g = gouts + (sb + t) * D;
    if (t >= T) {
      g[j] = 0.f;
      continue;
    }
    const float* zq = outs + (sb + t) * D;
    if (j == A) {
      const float dv = fminf(fmaxf(zq[A] - td_g[tb + t], -1.0f), 1.0f);
      g[A] = cv * dv * invBT;
      continue;
    }
    const float dlogp = -cp * psi_g[tb + t];  // zero for unselected
    const float* zb = behav + (sb + t) * A;
    float mb = zb[0];
    for (int k = 1; k < A; ++k) mb = fmaxf(mb, zb[k]);
    float sb_ = 0.f;
    for (int k = 0; k < A; ++k) sb_ += __expf(zb[k] - mb);
    const float lb = mb + __logf(sb_);
    const int a = (int)act[sb + t];
    const float q = __expf(zq[j] - lse_g[sb + t]);
    const float pb = __expf(zb[j] - lb);
    g[j] = dlogp * ((j == a ? 1.f : 0.f) - q) + alpha_v * (q - pb) * invBT +
           dreg * zq[j];
  }
}

// ---- what a row's block runs once the row's forward outputs exist:
// block 0 zeroes norm_sq (its next writer, the wgrad kernel, runs in a
// LATER launch), then the algorithm's row-local loss phase. kRowView: the
// inputs are views of row b alone (V-MPO's pre-phase has no such form). D is
// the packed head width (A+1, or 2A+1 for PPO-C); smem holds 6*S floats.
template <bool kRowView = false>
__device__ __forceinline__ void onpolicy_loss_phase(
    int algo, const float* __restrict__ outs, const float* __restrict__ act,
    const float* __restrict__ behav, const float* __restrict__ rew,
    const float* __restrict__ fir, float* __restrict__ gouts,
    float* __restrict__ stats_part, float* __restrict__ norm_sq,
    float* __restrict__ vm_lse, float* __restrict__ vm_logp,
    float* __restrict__ vm_adv, float* __restrict__ vm_td, int b, int B,
    int S, int D, float gamma, float lmbda, float rho_bar, float rho_min,
    float c_bar, float rew_scale, float cp, float cv, float ce,
    float eps_clip, float creg, char* smem) {
  if (b == 0 && threadIdx.x == 0 && norm_sq != nullptr) *norm_sq = 0.f;
  if (algo == kAlgoVmpo) {  // log-softmax + GAE to global scratch
    if constexpr (!kRowView) {
      vmpo_pre_row(outs, act, rew, fir, vm_lse, vm_logp, vm_adv, vm_td, b, S,
                   D - 1, gamma, lmbda, rew_scale);
    }
  } else if (algo == kAlgoPpoC) {  // Gaussian tanh-mean policy
    ppoc_loss_row<kRowView>(outs, act, behav, rew, fir, gouts, stats_part, b,
                            B, S, (D - 1) / 2, gamma, lmbda, rew_scale, cp,
                            cv, ce, eps_clip, creg, smem);
  } else {
    onpolicy_loss_row<kRowView>(algo, outs, act, behav, rew, fir, gouts,
                                stats_part, b, B, S, D - 1, gamma, lmbda,
                                rho_bar, rho_min, c_bar, rew_scale, cp, cv,
                                ce, eps_clip, creg, smem);
  }
}

// ONE block: parallel reduce of the (B, 8) per-row loss partials (all
// written by an EARLIER launch — stream order) into the final stats vector
// of IMPALA / PPO / PPO-C. Nothing to re-zero: rows are fully overwritten
// every step. Ends with its scratch still live — barrier before reusing LDS.
__device__ __forceinline__ void onpolicy_stats_reduce(
    const float* stats_part, float* stats,
    int algo, int B, int S, int D, float cp, float cv, float ce,
    float creg) {
  const int tid = threadIdx.x;
  float pl = 0.f, vl = 0.f, es = 0.f, rs = 0.f, rg = 0.f;
  float rmn = 1e30f, rmx = -1e30f;
  for (int b = tid; b < B; b += (int)blockDim.x) {
    const float* sp = stats_part + (long)b * 8;
    pl += sp[0];
    vl += sp[1];
    es += sp[2];
    rs += sp[3];
    rg += sp[4];
    if (algo != kAlgoImpala) {  // PPO and PPO-C track ratio min/max
      rmn = fminf(rmn, sp[5]);
      rmx = fmaxf(rmx, sp[6]);
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    pl += __shfl_down(pl, off, kWave);
    vl += __shfl_down(vl, off, kWave);
    es += __shfl_down(es, off, kWave);
    rs += __shfl_down(rs, off, kWave);
    rg += __shfl_down(rg, off, kWave);
    rmn = fminf(rmn, __shfl_down(rmn, off, kWave));
    rmx = fmaxf(rmx, __shfl_down(rmx, off, kWave));
  }
  __shared__ float s74[7][8];
  const int lane = tid & (kWave - 1), wave = tid >> 6;
  if (lane == 0) {
    s74[0][wave] = pl; s74[1][wave] = vl; s74[2][wave] = es;
    s74[3][wave] = rs; s74[4][wave] = rg; s74[5][wave] = rmn;
    s74[6][wave] = rmx;
  }
  __syncthreads();
  if (tid == 0) {
    const int nw = (int)blockDim.x / kWave;
    float P = 0, V = 0, E = 0, R = 0, G2 = 0, MN = 1e30f, MX = -1e30f;
    for (int w = 0; w < nw; ++w) {
      P += s74[0][w]; V += s74[1][w]; E += s74[2][w];
      R += s74[3][w]; G2 += s74[4][w];
      MN = fminf(MN, s74[5][w]); MX = fmaxf(MX, s74[6][w]);
    }
    const int nlog = D - 1;  // regularized heads: A, or 2A for PPO-C
    const float inv = 1.0f / (B * (S - 1));
    stats[0] = cp * P * inv + cv * V * inv - ce * E * inv +
               creg * G2 * inv / nlog;
    stats[1] = P * inv;
    stats[2] = V * inv;
    stats[3] = E * inv;
    stats[4] = R * inv;
    if (algo != kAlgoImpala) {
      stats[5] = MN;
      stats[6] = MX;
    }
  }
}
