"""csrc/replay.hip against its oracle: a FusedDeviceReplay on the GPU and one
on the CPU (the pure-torch path) are fed the same data; outputs and rings
must be equal bit for bit — the kernel only copies and does integer
arithmetic, so every comparison is ``torch.equal``."""
import math

import pytest
import torch

from pdrl_amd.buffers.device_replay import FusedDeviceReplay

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# row lengths at S=5: 20, 5, 5, 10, 5, 5, 160, 160 floats — both load widths,
# and rows of the narrow fields start 4-byte aligned only
FIELDS = {"obs": 4, "act": 1, "rew": 1, "logits": 2, "log_prob": 1,
          "is_fir": 1, "hx": 32, "cx": 32}


class Source:
    """Batches from a running arange: every element ever produced is unique
    (and exact in fp32 below 2^24)."""

    def __init__(self, fields, seq_len):
        self.fields, self.S, self.next = fields, seq_len, 1.0

    def batch(self, n):
        out = {}
        for name, dim in self.fields.items():
            count = n * self.S * dim
            out[name] = torch.arange(
                self.next, self.next + count, dtype=torch.float32).view(n, self.S, dim)
            self.next += count
        assert self.next < 2 ** 24
        return out


def on_gpu(batch):
    return {k: v.to(DEV) for k, v in batch.items()}


def pair(fields, seq_len, capacity, seed=1234, fill=0.0):
    gpu = FusedDeviceReplay(fields, seq_len, capacity, DEV, seed=seed)
    ora = FusedDeviceReplay(fields, seq_len, capacity, "cpu", seed=seed)
    assert not gpu.eager and ora.eager
    for rep in (gpu, ora):
        for t in rep._store.values():
            t.fill_(fill)
    return gpu, ora


def assert_same(gpu, ora, out_gpu, out_ora, what):
    assert (out_gpu is None) == (out_ora is None), what
    if out_ora is not None:
        for name, t in out_ora.items():
            assert torch.equal(out_gpu[name].cpu(), t), (what, name)
    for name, t in ora._store.items():
        assert torch.equal(gpu._store[name].cpu(), t), (what, "ring", name)
    assert (gpu.size, gpu._head, gpu._draws) == (ora.size, ora._head, ora._draws)


def launch_unruled(rep, batch, n_sample):
    """push_sample without DeviceReplay's "fewer stored than asked → None"
    rule: the same one launch, with more output rows than stored
    trajectories. Only a test wants that: it guarantees repeated slots."""
    n_push, srcs = rep._sources(batch)
    filled = min(rep._head + n_push, rep.capacity)
    out = rep._outputs(n_sample)
    rep._launch(srcs, n_push, out, filled, rep._draws + 1)
    rep._head += n_push
    rep._draws += 1
    return out


def test_call_sequence_matches_oracle():
    S, cap = 5, 11
    gpu, ora = pair(FIELDS, S, cap)
    src = Source(FIELDS, S)
    calls = [("append", 4, 0), ("push_sample", 4, 6), ("push_sample", 5, 7),
             ("append", 11, 0), ("sample", 0, 9), ("push_sample", 3, 16),
             # 16 > capacity: the public call pushes and returns no batch,
             # so the 16-row launch is also driven below that rule, and once
             # more through the public call with a batch
             ("unruled", 3, 16), ("push_sample", 3, 11)]
    produced = 0
    for i, (kind, n_push, n_sample) in enumerate(calls):
        what = f"call {i + 1}: {kind}({n_push}, {n_sample})"
        batch = src.batch(n_push) if n_push else None
        if kind == "append":
            out_g = gpu.append_batch(on_gpu(batch))
            out_o = ora.append_batch(batch)
        elif kind == "unruled":
            out_g = launch_unruled(gpu, on_gpu(batch), n_sample)
            out_o = launch_unruled(ora, batch, n_sample)
        elif kind == "sample":
            out_g, out_o = gpu.sample(n_sample), ora.sample(n_sample)
        else:
            out_g = gpu.push_sample(on_gpu(batch), n_sample)
            out_o = ora.push_sample(batch, n_sample)
        assert_same(gpu, ora, out_g, out_o, what)
        produced += out_o is not None
    assert produced == 5 and ora._draws == 5 and ora._head == 33


@pytest.mark.parametrize("head0", [0, 23])
def test_same_launch_hazard(head0):
    """Every slot of the ring is rewritten by the launch that samples it, so
    a sample row that read the ring instead of the source batch would return
    the stale -1 (or a torn row)."""
    fields, S, cap, n_sample = {"obs": 4, "hx": 128, "cx": 128}, 8, 64, 1024
    gpu, ora = pair(fields, S, cap, fill=-1.0)
    if head0:  # move the cursor off slot 0; the ring still holds only -1
        stale = {k: torch.full((head0, S, d), -1.0) for k, d in fields.items()}
        gpu.append_batch(on_gpu(stale))
        ora.append_batch(stale)
    batch = Source(fields, S).batch(cap)
    # through the public call 1024 > capacity yields no batch (the rule of
    # DeviceReplay.sample), so drive the same one launch below it
    for rep in (gpu, ora):
        for t in rep._outputs(n_sample).values():
            t.fill_(-1.0)
    outs = [launch_unruled(gpu, on_gpu(batch), n_sample),
            launch_unruled(ora, batch, n_sample)]
    assert_same(gpu, ora, outs[0], outs[1], "hazard launch")
    for name, t in outs[0].items():
        assert bool((t > 0).all()), name  # no -1 anywhere
    # and the public call as such: pushes, returns None on both
    more = Source(fields, S).batch(cap)
    assert_same(gpu, ora, gpu.push_sample(on_gpu(more), n_sample),
                ora.push_sample(more, n_sample), "push_sample(64, 1024)")
    assert not bool((gpu._store["hx"] < 0).any())


def test_partly_filled_ring():
    S, cap = 5, 1024
    gpu, ora = pair(FIELDS, S, cap, fill=float("nan"))
    batch = Source(FIELDS, S).batch(100)
    gpu.append_batch(on_gpu(batch))
    ora.append_batch(batch)
    out_g, out_o = gpu.sample(256), ora.sample(256)
    assert out_g is None and out_o is None  # 100 < 256: DeviceReplay's rule
    out_g, out_o = gpu.sample(100), ora.sample(100)
    for name, t in out_o.items():
        got = out_g[name].cpu()
        assert not bool(torch.isnan(got).any()), name
        assert torch.equal(got, t), name
    # 256 rows over the 100 filled slots, in the launch below the rule
    outs = [launch_unruled(gpu, None, 256), launch_unruled(ora, None, 256)]
    for name, t in outs[1].items():
        got = outs[0][name].cpu()
        assert not bool(torch.isnan(got).any()), name
        assert torch.equal(got, t), name
    for name, t in ora._store.items():
        assert torch.equal(gpu._store[name][:100].cpu(), t[:100]), name
        assert bool(torch.isnan(gpu._store[name][100:]).all()), name


def test_numpy_ingest():
    S, cap = 5, 16
    gpu, ora = pair(FIELDS, S, cap)
    src = Source(FIELDS, S)
    for n in (6, 13):  # the second wraps
        batch = src.batch(n)
        gpu.append_batch({k: v.numpy() for k, v in batch.items()})
        ora.append_batch(batch)
    assert_same(gpu, ora, None, None, "numpy append")


def test_persistent_outputs_and_launch_checks():
    S, cap = 5, 16
    gpu, _ = pair(FIELDS, S, cap)
    src = Source(FIELDS, S)
    a = gpu.push_sample(on_gpu(src.batch(8)), 4)
    ptrs = {k: v.data_ptr() for k, v in a.items()}
    b = gpu.push_sample(on_gpu(src.batch(8)), 4)
    assert b is a and ptrs == {k: v.data_ptr() for k, v in b.items()}
    ext, rings = gpu._ext, gpu._rings
    outs = list(a.values())
    with pytest.raises(RuntimeError, match="overlaps a ring"):
        ext.replay_push_sample([r[:2] for r in rings], rings, [], 2, 0, 0,
                               cap, 2, 1, 0)
    with pytest.raises(RuntimeError, match="empty replay"):
        ext.replay_push_sample([], rings, outs, 0, 4, 0, cap, 0, 1, 0)
    with pytest.raises(RuntimeError, match="n_push"):
        big = [torch.zeros(cap + 1, S, d, device=DEV) for d in FIELDS.values()]
        ext.replay_push_sample(big, rings, [], cap + 1, 0, 0, cap, cap, 1, 0)
    with pytest.raises(RuntimeError, match="float32"):
        ext.replay_push_sample([], rings, [o.double() for o in outs], 0, 4, 0,
                               cap, 16, 1, 0)
    with pytest.raises(RuntimeError, match="n_sample"):
        ext.replay_push_sample([], rings, outs, 0, 5, 0, cap, 16, 1, 0)


@pytest.mark.parametrize("algo", ["SAC", "SAC-Continuous"])
def test_learner_device_mode_fused_end_to_end(params, algo):
    from pdrl_amd.agents import Learner

    p = params
    p.algo = algo
    if algo == "SAC":
        p.env, p.obs_dim, p.n_actions, p.continuous = "CartPole-v1", 4, 2, False
    else:
        p.env = "MountainCarContinuous-v0"
        p.obs_dim, p.n_actions, p.continuous = 2, 1, True
    p.batch_size, p.seq_len = 32, 5
    p.model_save_interval = 10_000
    p.actor_mode = "device"
    p.replay_kernel = "fused"
    lrn = Learner(None, "127.0.0.1", 0, p, device=DEV)
    seen, sizes = [], []
    try:
        rep = lrn.device_replay
        assert isinstance(rep, FusedDeviceReplay) and not rep.eager
        assert not lrn.device_rollout.eager
        step = lrn.updater.step

        def spy(batch):
            sizes.append(rep.size)
            for name, dim in rep.field_dims.items():
                assert batch[name].shape == (32, 5, dim) and batch[name].is_cuda
            seen.append(step(batch))
            return seen[-1]

        lrn.updater.step = spy
        lrn.run(max_updates=3)
        torch.cuda.synchronize()
        assert lrn.updater.update_count == 3 and len(seen) == 3
        for stats in seen:
            assert all(math.isfinite(float(v)) for v in stats.values()), stats
        n = lrn.device_rollout.N
        assert sizes == [n, 2 * n, 3 * n]  # one rollout pushed per update
        assert rep._draws == 3
    finally:
        lrn.close()
