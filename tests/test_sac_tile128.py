"""rows_kernel="tile" in the SAC updaters: accepted at hidden size 64 and
128, rejected at any other width (no GPU needed)."""
import pytest


def _updater(algo, hidden_size):
    from pdrl_amd.agents.learner_module import switch_module
    from pdrl_amd.utils import load_params

    p = load_params()
    continuous = algo.endswith("Continuous")
    p.algo, p.rows_kernel, p.hidden_size = algo, "tile", hidden_size
    p.obs_dim, p.n_actions = (3, 1) if continuous else (4, 2)
    upd_cls, model_cls = switch_module(algo)
    model = model_cls(p.obs_dim, p.n_actions, p.seq_len, p.hidden_size)
    return upd_cls(model, p, "cpu")


@pytest.mark.parametrize("algo", ["SAC", "SAC-Continuous"])
def test_sac_tile_accepted_at_hidden_128(algo):
    assert _updater(algo, 128).params.rows_kernel == "tile"


@pytest.mark.parametrize("algo", ["SAC", "SAC-Continuous"])
def test_sac_tile_rejected_at_hidden_96(algo):
    with pytest.raises(ValueError, match="rows_kernel"):
        _updater(algo, 96)
