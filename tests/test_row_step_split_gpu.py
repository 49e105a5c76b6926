"""The split instantiation of seq_lstm_row_step (input projections computed
ahead of the forward's time loop, head weights read from LDS) against the
two-launch pair seq_lstm_fwd_loss + seq_lstm_bwd_fin, which runs the
projection inside its loop and loads the head weights behind it. Every
accumulator sees the same fmaf sequence on both sides, so every array must
be equal BIT FOR BIT.
Each case asserts which instantiation the launcher takes, so that the test
cannot pass without running the one it is about. All tests here require an
MI355X."""
import functools

import pytest
import torch

from tests.test_row_step_gpu import (ALGO_ID, _assert_same, _ext, _pair,
                                     _row_step)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H = 64
MAX_LDS = 64 * 1024

# (B, S, A) for IMPALA and PPO
DISCRETE_SHAPES = [
    (1, 2, 2),   # T = 1, and the only block is block 0
    (3, 3, 2),   # small plain case
    (2, 7, 5),   # H·D = 384 > 256 threads: the head weights' second fetch
    (7, 8, 5),   # S·H = 512 > 256 threads: every strided loop runs twice
    (16, 5, 2),  # the flagship row shape
]
CASES = ([(algo, *shape) for algo in ("IMPALA", "PPO")
          for shape in DISCRETE_SHAPES] +
         [("PPO-C", 3, 3, 1), ("PPO-C", 7, 8, 3)])


def _dims(algo, A):
    """Packed head width and actions per step."""
    return (2 * A + 1, A) if algo == "PPO-C" else (A + 1, 1)


def _split_bytes(algo, S, A):
    """The split layout, in floats: the forward keeps xb, hs (S,H), gates
    (4H), hbuf, cbuf (H), px (S,4H), the head weights (H,D), (D) and behind
    them the parked loss inputs; BPTT keeps dhh, dxb_s (S,H), dg4, part_h,
    part_x (4H); the loss phase's 6·S overlays the front."""
    D, act_per = _dims(algo, A)
    fwd = (2 * S * H + 6 * H + 4 * S * H + H * D + D +
           S * (D + act_per + 3))
    bwd = 2 * S * H + 12 * H
    return 4 * max(fwd, bwd, 6 * S)


def _check(algo, B, S, A):
    ref_ws, ref_grads = _pair(algo, B, S, A)
    norm = torch.full((1,), 3.5, device=DEV)
    ws, grads = _row_step(algo, B, S, A, norm)
    _assert_same(ws, grads, ref_ws, ref_grads, 5 if algo == "IMPALA" else 7)
    assert norm.item() == 0.0, "block 0 must zero norm_sq"


@pytest.mark.parametrize("algo,B,S,A", CASES)
def test_split_row_step_equals_two_launch_pair(algo, B, S, A):
    e = _ext()
    D, _ = _dims(algo, A)
    assert e.seq_lstm_row_step_split_lds_bytes(S, D, ALGO_ID[algo]) == \
        _split_bytes(algo, S, A)
    assert e.seq_lstm_row_step_uses_split(S, D, ALGO_ID[algo])
    _check(algo, B, S, A)


@functools.lru_cache(maxsize=None)
def _longest_split(algo, A):
    """The largest S the launcher still gives the split instantiation."""
    e = _ext()
    D, _ = _dims(algo, A)
    S = 2
    while e.seq_lstm_row_step_uses_split(S + 1, D, ALGO_ID[algo]):
        S += 1
        assert S < 256
    return S


def test_split_lds_formula_and_threshold():
    e = _ext()
    # flagship: the forward with px and the parked inputs is the largest phase
    assert e.seq_lstm_row_step_split_lds_bytes(5, 3, 0) == \
        (6 * 5 * 64 + 6 * 64 + 65 * 3 + 5 * (3 + 1 + 3)) * 4
    for algo, A in (("IMPALA", 2), ("PPO", 5), ("PPO-C", 3)):
        D, _ = _dims(algo, A)
        for S in (2, 3, 8, 39, 40, 41, 60, 100):
            need = e.seq_lstm_row_step_split_lds_bytes(S, D, ALGO_ID[algo])
            assert need == _split_bytes(algo, S, A)
            assert e.seq_lstm_row_step_uses_split(S, D, ALGO_ID[algo]) == \
                (need <= MAX_LDS)
            # no shape loses the row step: the split need is never the smaller
            assert need >= e.seq_lstm_row_step_lds_bytes(S, D, ALGO_ID[algo])
    S = _longest_split("IMPALA", 2)
    assert _split_bytes("IMPALA", S, 2) <= MAX_LDS < \
        _split_bytes("IMPALA", S + 1, 2)


def test_longest_split_sequence():
    """The last S whose split layout fits a launch."""
    S = _longest_split("IMPALA", 2)
    _check("IMPALA", 2, S, 2)


def test_first_sequence_past_the_split():
    """One step more: the launcher takes the other instantiation."""
    e = _ext()
    S = _longest_split("IMPALA", 2) + 1
    assert not e.seq_lstm_row_step_uses_split(S, 3, 0)
    assert e.seq_lstm_row_step_lds_bytes(S, 3, 0) <= MAX_LDS
    _check("IMPALA", 2, S, 2)


def test_long_sequence_runs_without_the_split():
    """S = 60: the split layout needs about 94 KiB, the other about 34 KiB."""
    e = _ext()
    assert e.seq_lstm_row_step_split_lds_bytes(60, 3, 0) > MAX_LDS
    assert not e.seq_lstm_row_step_uses_split(60, 3, 0)
    assert e.seq_lstm_row_step_lds_bytes(60, 3, 0) <= MAX_LDS
    _check("IMPALA", 2, 60, 2)
