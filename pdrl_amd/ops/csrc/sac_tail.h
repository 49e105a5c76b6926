// The actor-loss tail both SAC actor weight-gradient kernels carry on one
// extra block (sac_actor_wgrad in sac_loss.hip, sac_actor_wgrad_split in
// wgrad_split_multi.hip): the same code, so the two give the same bits.
#pragma once

#include "common.h"

// ONE block of 256 threads: sums the (B,2) per-row {loss, entropy} partials
// an earlier launch stored into {g_alpha, stats4[0..3], alpha_norm} and
// advances the shared Adam clock (t, 1-β1ᵗ, 1-β2ᵗ).
__device__ __forceinline__ void sac_actor_tail(
    const float* __restrict__ stats_part, const float* __restrict__ log_alpha,
    float* __restrict__ g_alpha, float* __restrict__ stats4,
    float* __restrict__ alpha_norm, float* __restrict__ clock, int B, int N,
    float target_entropy, float beta1, float beta2) {
  const int tid = threadIdx.x;
  __shared__ float r0[256], r1[256];
  float l = 0.f, en = 0.f;
  for (int b = tid; b < B; b += 256) {
    l += stats_part[2 * b];
    en += stats_part[2 * b + 1];
  }
  r0[tid] = l;
  r1[tid] = en;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off) { r0[tid] += r0[tid + off]; r1[tid] += r1[tid + off]; }
    __syncthreads();
  }
  if (tid == 0) {
    const float inv = 1.0f / N;
    const float alpha = __expf(*log_alpha);
    const float ent_mean = r1[0] * inv;
    const float da = ent_mean - target_entropy;  // dlog_alpha
    g_alpha[0] = da;
    stats4[0] = r0[0] * inv;            // loss-actor
    stats4[1] = __logf(alpha) * da;     // loss-alpha (value)
    stats4[2] = alpha;
    stats4[3] = ent_mean;
    if (alpha_norm != nullptr) *alpha_norm = da * da;
  }
  if (tid == 1 && clock != nullptr) {
    const float t = clock[0] + 1.0f;
    clock[0] = t;
    clock[1] = 1.0f - __powf(beta1, t);
    clock[2] = 1.0f - __powf(beta2, t);
  }
}
