// Device replay: append new trajectories to the per-field rings and gather a
// uniformly sampled batch, in ONE launch (buffers/device_replay.py::
// FusedDeviceReplay; the eager path there is this kernel's oracle).
//
// Grid = n_push + n_sample workgroups, one trajectory row each:
//   * workgroup i < n_push copies source row i of every field into ring
//     slot (head + i) % capacity;
//   * workgroup n_push + b draws slot_b from the counter hash
//     (rollout_rng.h::replay_slot) and copies that trajectory of every field
//     into row b of the output tensors.
// Workgroups of one launch are not ordered, so a sample row whose slot is
// written by this launch reads the SOURCE batch, never the ring: that is
// the case when off = (slot - head % capacity + capacity) % capacity <
// n_push, and the row is source row off. With n_push <= capacity every slot
// has at most one writer, so the result is exactly "push, then sample" with
// no grid barrier, atomics, fences or spinning.
//
// The cursor (head), fill level and draw count are host integers passed as
// launch arguments; the field table is a by-value kernel argument (no H2D
// copy, no device pointer table). Ring offsets are 64-bit: capacity * S * dim
// passes 2^32 floats at HBM-sized replays. A field whose row length is a
// multiple of 4 floats (and whose bases are 16-byte aligned) moves as
// dwordx4, any other as dwords — row starts of e.g. a 5-float row are only
// 4-byte aligned.
#include "common.h"
#include "rollout_rng.h"

#include <cstdint>
#include <vector>

namespace {

constexpr int kMaxFields = 12;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kUnroll = 4;  // loads in flight per lane before the stores

struct ReplayField {
  const float* src;  // (n_push, S, dim) or null when n_push == 0
  float* ring;       // (capacity, S, dim)
  float* out;        // (>= n_sample, S, dim) or null when n_sample == 0
  int row_floats;    // S * dim
  int vec4;          // 1: row_floats % 4 == 0 and all bases 16-byte aligned
};

struct ReplayTable {
  ReplayField f[kMaxFields];
  int n_fields;
};

template <typename T>
__device__ __forceinline__ void copy_units(const T* __restrict__ s,
                                           T* __restrict__ d, int units,
                                           int lane) {
  for (int base = lane; base < units; base += kWave * kUnroll) {
    // unconditional loads at an index clamped into the row keep v[] in
    // registers (a predicated fill gets the array demoted to LDS)
    T v[kUnroll];
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      v[j] = s[min(base + j * kWave, units - 1)];
    }
#pragma unroll
    for (int j = 0; j < kUnroll; ++j) {
      const int i = base + j * kWave;
      if (i < units) d[i] = v[j];
    }
  }
}

__global__ __launch_bounds__(kThreads) void replay_push_sample_kernel(
    const ReplayTable tab, const int n_push, const int64_t head_slot,
    const int64_t capacity, const uint32_t filled, const uint32_t draw,
    const uint32_t seed) {
  const int wg = blockIdx.x;
  const int lane = threadIdx.x % kWave;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);

  // row-level decision, identical in every lane of the workgroup
  bool read_src, write_out;
  int64_t src_row, dst_row;
  if (wg < n_push) {
    int64_t slot = head_slot + wg;
    if (slot >= capacity) slot -= capacity;
    read_src = true, write_out = false;
    src_row = wg, dst_row = slot;
  } else {
    const uint32_t b = static_cast<uint32_t>(wg - n_push);
    const int64_t slot = pdrl_rng::replay_slot(seed, b, draw, filled);
    int64_t off = slot - head_slot;
    if (off < 0) off += capacity;
    read_src = off < n_push;  // written by this launch: take it at the source
    write_out = true;
    src_row = read_src ? off : slot;
    dst_row = b;
  }

  // one wave per field, wave-uniform table index
  for (int fi = wave; fi < tab.n_fields; fi += kWaves) {
    const ReplayField f = tab.f[fi];
    const int64_t rf = f.row_floats;
    const float* s = (read_src ? f.src : f.ring) + src_row * rf;
    float* d = (write_out ? f.out : f.ring) + dst_row * rf;
    if (f.vec4) {
      copy_units(reinterpret_cast<const float4*>(s),
                 reinterpret_cast<float4*>(d), f.row_floats / 4, lane);
    } else {
      copy_units(s, d, f.row_floats, lane);
    }
  }
}

struct ByteRange {
  uintptr_t lo, hi;
};

ByteRange range_of(const at::Tensor& t) {
  const uintptr_t lo = reinterpret_cast<uintptr_t>(t.data_ptr());
  return {lo, lo + static_cast<uintptr_t>(t.numel()) * t.element_size()};
}

bool overlaps(const ByteRange& a, const ByteRange& b) {
  return a.lo < b.hi && b.lo < a.hi;
}

bool aligned16(const void* p) {
  return reinterpret_cast<uintptr_t>(p) % 16 == 0;
}

}  // namespace

// src / out may be empty lists when n_push / n_sample is 0. head is the
// number of trajectories ever written BEFORE this call, filled the fill level
// AFTER its push, draw the 1-based sampling-call count.
void replay_push_sample_hip(const std::vector<at::Tensor>& src,
                            const std::vector<at::Tensor>& ring,
                            const std::vector<at::Tensor>& out, long n_push,
                            long n_sample, long head, long capacity,
                            long filled, long draw, long seed) {
  const size_t nf = ring.size();
  TORCH_CHECK(nf >= 1 && nf <= static_cast<size_t>(kMaxFields),
              "replay_push_sample: 1..", kMaxFields, " fields, got ", nf);
  TORCH_CHECK(n_push >= 0 && n_sample >= 0, "negative row count");
  TORCH_CHECK(capacity >= 1 && capacity < (1L << 31),
              "capacity must be in [1, 2^31)");
  TORCH_CHECK(n_push <= capacity, "n_push ", n_push, " > capacity ", capacity);
  TORCH_CHECK(head >= 0, "head must not be negative");
  TORCH_CHECK(filled >= 0 && filled <= capacity, "filled out of range");
  TORCH_CHECK(n_sample == 0 || filled >= 1, "sampling from an empty replay");
  TORCH_CHECK(n_push + n_sample < (1L << 31), "too many rows for one launch");
  TORCH_CHECK(n_push == 0 || src.size() == nf, "src needs one tensor per field");
  TORCH_CHECK(n_sample == 0 || out.size() == nf, "out needs one tensor per field");
  if (n_push + n_sample == 0) return;

  ReplayTable tab{};
  tab.n_fields = static_cast<int>(nf);
  const auto device = ring[0].device();
  for (size_t i = 0; i < nf; ++i) {
    const at::Tensor& r = ring[i];
    CHECK_IN(r);
    TORCH_CHECK(r.device() == device, "ring fields on different devices");
    TORCH_CHECK(r.dim() == 3 && r.size(0) == capacity,
                "ring field must be (capacity, S, dim)");
    const int64_t rf = r.size(1) * r.size(2);
    TORCH_CHECK(rf >= 1 && rf < (1L << 31), "row length out of range");
    ReplayField& f = tab.f[i];
    f.ring = r.data_ptr<float>();
    f.row_floats = static_cast<int>(rf);
    bool vec = rf % 4 == 0 && aligned16(f.ring);
    const ByteRange rr = range_of(r);
    if (n_push > 0) {
      const at::Tensor& s = src[i];
      CHECK_IN(s);
      TORCH_CHECK(s.device() == device, "src on a different device");
      TORCH_CHECK(s.dim() == 3 && s.size(0) == n_push &&
                      s.size(1) == r.size(1) && s.size(2) == r.size(2),
                  "src field must be (n_push, S, dim)");
      f.src = s.data_ptr<float>();
      vec = vec && aligned16(f.src);
    }
    if (n_sample > 0) {
      const at::Tensor& o = out[i];
      CHECK_IN(o);
      TORCH_CHECK(o.device() == device, "out on a different device");
      TORCH_CHECK(o.dim() == 3 && o.size(0) >= n_sample &&
                      o.size(1) == r.size(1) && o.size(2) == r.size(2),
                  "out field must be (>= n_sample, S, dim)");
      f.out = o.data_ptr<float>();
      vec = vec && aligned16(f.out);
    }
    f.vec4 = vec ? 1 : 0;
    // no src / out memory may overlap ANY ring (or each other)
    for (size_t j = 0; j < nf; ++j) {
      const ByteRange rj = range_of(ring[j]);
      TORCH_CHECK(j == i || !overlaps(rr, rj), "ring fields overlap");
      if (n_push > 0)
        TORCH_CHECK(!overlaps(range_of(src[i]), rj), "src overlaps a ring");
      if (n_sample > 0)
        TORCH_CHECK(!overlaps(range_of(out[i]), rj), "out overlaps a ring");
      if (n_push > 0 && n_sample > 0)
        TORCH_CHECK(!overlaps(range_of(src[i]), range_of(out[j])),
                    "src overlaps out");
    }
  }

  const dim3 grid(static_cast<unsigned>(n_push + n_sample));
  hipLaunchKernelGGL(replay_push_sample_kernel, grid, dim3(kThreads), 0,
                     current_stream(), tab, static_cast<int>(n_push),
                     static_cast<int64_t>(head % capacity),
                     static_cast<int64_t>(capacity),
                     static_cast<uint32_t>(filled),
                     static_cast<uint32_t>(draw & 0xFFFFFFFFL),
                     static_cast<uint32_t>(seed & 0xFFFFFFFFL));
  HIP_CHECK_LAST();
}
