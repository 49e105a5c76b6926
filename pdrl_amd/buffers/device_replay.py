"""Device-resident replay buffer for off-policy learners (SAC).

BASELINE.json configs[5]: "SAC-Continuous ... replay buffer resident in
288 GB HBM on 1×MI355X". The reference keeps its replay in 43 MB of host
shared memory and re-copies every sampled batch host→device
(reference: shared_batch.py:71-72, learner.py:179-233). Here the replay
lives ON the GPU:

* ingest: new trajectories drained from the host ring are appended to
  device-side per-field rings with ONE packed H2D copy per drain;
* sampling: indices are drawn on device (CUDA RNG) and gathered with
  index_select — the sampled batch never touches the host;
* capacity: sized by ``buffer_size``; at the default record width
  (CartPole shapes ≈ 2.8 KB/trajectory) 288 GB of HBM3E fits ~100M
  trajectories — the host-shm 10240-slot limit of the reference is gone.

``DeviceReplay`` does this with eager torch ops: 8-16 slice copies per append
and a ``randint`` + 8 ``index_select`` per sample. ``FusedDeviceReplay``
(``"replay_kernel": "fused"``) keeps the same rings and does append + sample
in ONE launch of csrc/replay.hip, with the sampled slots drawn from the
rollout's stateless counter hash instead of a ``torch.Generator``:

    h      = hash_bits(seed ^ 0x5BD1E995, row b, draw t, lane 7)   # uint32
    slot_b = (uint64(h) * filled) >> 32                            # [0, filled)

``t`` is the 1-based count of sampling calls on the replay object (a host
integer, like the ring cursor) and ``filled = min(head after the push,
capacity)``; a sampled batch is therefore a pure function of ``(seed, t,
filled)`` and the ring contents. ``capacity < 2^31`` keeps the product in
int64 in the torch mirror; the hash counter ``t * 8 + 7`` is uint32, so the
stream repeats after 2^29 sampling calls.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from pdrl_amd.ops.rollout import hash_bits

_M32 = 0xFFFFFFFF
REPLAY_SALT = 0x5BD1E995  # csrc/rollout_rng.h::kReplaySalt
REPLAY_LANE = 7           # the hash lane the rollout leaves free
MAX_FIELDS = 12           # size of the kernel's by-value field table


class DeviceReplay:
    def __init__(self, field_dims: dict[str, int], seq_len: int, capacity: int,
                 device, seed: int = 0):
        self.field_dims = dict(field_dims)
        self.seq_len = seq_len
        self.capacity = capacity
        self.device = torch.device(device)
        self._store = {
            name: torch.empty(capacity, seq_len, dim, dtype=torch.float32,
                              device=self.device)
            for name, dim in field_dims.items()
        }
        self._head = 0  # total trajectories ever written
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(seed)

    @property
    def size(self) -> int:
        return min(self._head, self.capacity)

    def nbytes(self) -> int:
        return sum(t.numel() * 4 for t in self._store.values())

    def append_batch(self, traj_batch: dict[str, np.ndarray | torch.Tensor]):
        """Append N trajectories {field: (N, seq, dim)} (one H2D per field,
        wrap-around handled)."""
        any_field = next(iter(traj_batch.values()))
        n = int(any_field.shape[0])
        if n == 0:
            return
        assert n <= self.capacity
        start = self._head % self.capacity
        first = min(n, self.capacity - start)
        for name, dim in self.field_dims.items():
            src = traj_batch[name]
            if isinstance(src, np.ndarray):
                src = torch.from_numpy(src)
            src = src.to(self.device, non_blocking=True).view(n, self.seq_len, dim)
            self._store[name][start : start + first] = src[:first]
            if first < n:
                self._store[name][: n - first] = src[first:]
        self._head += n

    def sample(self, batch: int) -> dict[str, torch.Tensor] | None:
        """Uniform sample of ``batch`` stored trajectories; indices drawn and
        gathered entirely on device."""
        filled = self.size
        if filled < batch:
            return None
        idx = torch.randint(0, filled, (batch,), device=self.device,
                            generator=self._gen)
        return {name: t.index_select(0, idx) for name, t in self._store.items()}


def replay_slots(seed: int, n: int, draw: int, filled: int,
                 device="cpu") -> torch.Tensor:
    """Ring slots (int64, in [0, filled)) of output rows 0..n-1 at sampling
    call ``draw``: the torch mirror of csrc/rollout_rng.h::replay_slot."""
    rows = torch.arange(n, dtype=torch.int64, device=device)
    h = hash_bits((int(seed) ^ REPLAY_SALT) & _M32, rows, int(draw), REPLAY_LANE)
    return (h * int(filled)) >> 32


class FusedDeviceReplay:
    """``DeviceReplay``'s rings (same ``_store`` layout, cursor and wrap
    rule) with append and sample fused into one launch of csrc/replay.hip.

    ``push_sample(batch, n)`` appends ``batch`` and returns ``n`` uniformly
    sampled trajectories; the result is exactly "push, then sample" (a
    sampled slot written by the same launch is read from ``batch``).
    ``append_batch`` / ``sample`` are the push-only / sample-only forms of
    the same launch.

    The sampled batch lives in persistent output tensors: the SAME dict of
    the SAME tensors is returned by every call with the same ``n`` and is
    overwritten by the next such call (the contract of
    ``DeviceRollout.batch``) — consume or clone it before sampling again.

    On a CPU device, or with ``PDRL_REPLAY_EAGER=1``, the class runs the
    pure-torch implementation of the same rules, which is both the fallback
    and the kernel's oracle; on ``cuda`` otherwise a missing kernel is an
    error, not a fallback.
    """

    def __init__(self, field_dims: dict[str, int], seq_len: int, capacity: int,
                 device, seed: int = 0):
        if not 1 <= capacity < 2 ** 31:
            raise ValueError(f"capacity must be in [1, 2^31), got {capacity}")
        if not 1 <= len(field_dims) <= MAX_FIELDS:
            raise ValueError(
                f"1..{MAX_FIELDS} fields supported, got {len(field_dims)}")
        self.field_dims = dict(field_dims)
        self.seq_len = int(seq_len)
        self.capacity = int(capacity)
        self.device = torch.device(device)
        self.seed = int(seed) & _M32
        self.eager = (self.device.type != "cuda"
                      or os.environ.get("PDRL_REPLAY_EAGER") == "1")
        if not self.eager:
            from pdrl_amd import ops

            self._ext = ops.ext()  # a missing kernel is an error, not a fallback
        self._store = {
            name: torch.empty(self.capacity, self.seq_len, dim,
                              dtype=torch.float32, device=self.device)
            for name, dim in self.field_dims.items()
        }
        self._rings = list(self._store.values())
        self._head = 0   # total trajectories ever written
        self._draws = 0  # sampling calls that produced a batch
        self._out: dict[int, dict[str, torch.Tensor]] = {}

    @property
    def size(self) -> int:
        return min(self._head, self.capacity)

    def nbytes(self) -> int:
        return sum(t.numel() * 4 for t in self._store.values())

    # ------------------------------------------------------------------ #
    def _outputs(self, n: int) -> dict[str, torch.Tensor]:
        out = self._out.get(n)
        if out is None:
            out = self._out[n] = {
                name: torch.zeros(n, self.seq_len, dim, dtype=torch.float32,
                                  device=self.device)
                for name, dim in self.field_dims.items()
            }
        return out

    def _sources(self, batch) -> tuple[int, list[torch.Tensor]]:
        """Device fp32 contiguous (n, S, dim) views of ``batch``, in field
        order; numpy / host tensors are moved to the device first."""
        if not batch:
            return 0, []
        n = int(next(iter(batch.values())).shape[0])
        if n > self.capacity:
            raise ValueError(
                f"push of {n} trajectories exceeds capacity {self.capacity}")
        if n == 0:
            return 0, []
        srcs = []
        for name, dim in self.field_dims.items():
            src = batch[name]
            if isinstance(src, np.ndarray):
                src = torch.from_numpy(src)
            src = src.to(device=self.device, dtype=torch.float32,
                         non_blocking=True)
            srcs.append(src.reshape(n, self.seq_len, dim).contiguous())
        return n, srcs

    def push_sample(self, batch, n_sample: int) -> dict[str, torch.Tensor] | None:
        """Append ``batch`` ({field: (N, S, dim)}, or None), then sample
        ``n_sample`` trajectories. Returns None — after pushing — while fewer
        than ``n_sample`` trajectories are stored (or when ``n_sample`` is
        0); the draw counter advances only when a batch is returned."""
        n_sample = int(n_sample)
        if n_sample < 0:
            raise ValueError("n_sample must not be negative")
        n_push, srcs = self._sources(batch)
        filled = min(self._head + n_push, self.capacity)
        do_sample = 0 < n_sample <= filled
        if n_push == 0 and not do_sample:
            return None
        out = self._outputs(n_sample) if do_sample else None
        draw = self._draws + 1
        self._launch(srcs, n_push, out, filled, draw)
        self._head += n_push
        if do_sample:
            self._draws = draw
        return out

    def _launch(self, srcs, n_push, out, filled, draw):
        """One launch: push ``srcs`` (n_push rows per field) at the cursor
        and, when ``out`` is given, fill its rows with draw ``draw`` over
        ``filled`` slots. Does not move the cursor or the draw counter."""
        if self.eager:
            self._push_sample_eager(srcs, n_push, out, filled, draw)
            return
        outs = list(out.values()) if out is not None else []
        self._ext.replay_push_sample(
            srcs, self._rings, outs, n_push,
            int(outs[0].shape[0]) if outs else 0, self._head, self.capacity,
            filled, draw, self.seed)

    def append_batch(self, traj_batch: dict[str, np.ndarray | torch.Tensor]):
        """Append N trajectories {field: (N, seq, dim)} (push only)."""
        self.push_sample(traj_batch, 0)

    def sample(self, batch: int) -> dict[str, torch.Tensor] | None:
        """Uniform sample of ``batch`` stored trajectories (sample only)."""
        return self.push_sample(None, batch)

    @torch.no_grad()
    def _push_sample_eager(self, srcs, n_push, out, filled, draw):
        """Torch reference of csrc/replay.hip: slice-copy the push (the wrap
        rule of ``DeviceReplay.append_batch``), then gather the hash-drawn
        slots into the persistent outputs."""
        if n_push:
            start = self._head % self.capacity
            first = min(n_push, self.capacity - start)
            for ring, src in zip(self._rings, srcs):
                ring[start : start + first] = src[:first]
                if first < n_push:
                    ring[: n_push - first] = src[first:]
        if out is not None:
            n_sample = int(next(iter(out.values())).shape[0])
            idx = replay_slots(self.seed, n_sample, draw, filled, self.device)
            for ring, dst in zip(self._rings, out.values()):
                torch.index_select(ring, 0, idx, out=dst)
