"""The "wgrad_kernel" key on the two SAC updaters: validated at construction,
before the GPU / extension check, so it behaves the same on a CPU-only box."""
import pytest

from pdrl_amd.agents.learner_module import switch_module
from pdrl_amd.utils import load_params


def _build(algo, wgrad_kernel):
    p = load_params()
    p.algo, p.wgrad_kernel = algo, wgrad_kernel
    p.batch_size, p.seq_len = 4, 5
    p.obs_dim, p.n_actions = (3, 1) if algo.endswith("Continuous") else (4, 2)
    upd_cls, model_cls = switch_module(algo)
    model = model_cls(p.obs_dim, p.n_actions, p.seq_len, p.hidden_size)
    return upd_cls(model, p, "cpu")


@pytest.mark.parametrize("algo", ["SAC", "SAC-Continuous"])
def test_bad_wgrad_kernel_raises(algo):
    with pytest.raises(ValueError, match="wgrad_kernel must be 'sweep' or "
                                         "'split', got 'bogus'"):
        _build(algo, "bogus")


@pytest.mark.parametrize("algo", ["SAC", "SAC-Continuous"])
def test_split_builds_on_cpu(algo):
    assert _build(algo, "split").fused_step is None
