// Counter-based random stream of the device rollout (rollout.hip), shared
// by the kernel and host code so a test can reproduce it bit for bit.
// Stateless: a uniform is a pure function of (seed, env, tick, lane), which
// is what makes the stream graph-safe and independent of launch geometry.
// All arithmetic is uint32 (wrap-around); the torch mirror of this file is
// pdrl_amd/ops/rollout.py::uniform.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#define PDRL_HD __host__ __device__ __forceinline__
#else
#define PDRL_HD inline
#endif

namespace pdrl_rng {

PDRL_HD uint32_t wang(uint32_t s) {
  s = (s ^ 61u) ^ (s >> 16);
  s *= 9u;
  s ^= s >> 4;
  s *= 0x27d4eb2du;
  s ^= s >> 15;
  return s;
}

// Lane k of env's draw at ``tick`` (eight lanes per tick): k = 0 is the
// categorical action uniform (unused by Gaussian policies), k = 1..4 the
// reset state of a reset caused by the step at ``tick`` (tick 0: the initial
// state at construction), k = 5 / 6 the radius / angle uniform of a Gaussian
// policy's one standard normal per tick, k = 7 is free. One normal per tick
// is one action dimension: more need a wider counter than tick * 8 + k.
// The raw 32 bits of that lane. The counter tick * 8 + k is uint32: it wraps
// after 2^29 ticks.
PDRL_HD uint32_t bits(uint32_t seed, uint32_t env, uint32_t tick, uint32_t k) {
  const uint32_t h0 = wang(seed ^ (env * 0x9E3779B1u));
  return wang(h0 ^ wang(tick * 8u + k + 0x85ebca6bu));
}

// Result in [0, 1), a multiple of 2^-24.
PDRL_HD float uniform(uint32_t seed, uint32_t env, uint32_t tick, uint32_t k) {
  return static_cast<float>(bits(seed, env, tick, k) >> 8) * (1.0f / 16777216.0f);
}

// Device replay (replay.hip) draws its sampled slots from the free lane 7:
// env = output row b, tick = the replay's 1-based sampling-call count, seed
// xor-ed with kReplaySalt so a replay seeded like the rollout does not share
// its stream. slot = (bits * filled) >> 32 lies in [0, filled); the torch
// mirror is pdrl_amd/buffers/device_replay.py::replay_slots.
constexpr uint32_t kReplaySalt = 0x5BD1E995u;
constexpr uint32_t kReplayLane = 7u;

PDRL_HD uint32_t replay_slot(uint32_t seed, uint32_t row, uint32_t draw,
                             uint32_t filled) {
  const uint32_t h = bits(seed ^ kReplaySalt, row, draw, kReplayLane);
  return static_cast<uint32_t>((static_cast<uint64_t>(h) * filled) >> 32);
}

}  // namespace pdrl_rng
