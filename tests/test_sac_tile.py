"""The rows_kernel key of the two SAC updaters: validated before the
extension is looked at, so a bad value fails on a CPU box too."""
import pytest


@pytest.mark.parametrize("algo", ["SAC", "SAC-Continuous"])
@pytest.mark.parametrize("rows_kernel,hidden", [("tiles", 64), ("tile", 32)])
def test_sac_updater_rejects_bad_rows_kernel(algo, rows_kernel, hidden):
    from pdrl_amd.agents.learner_module import switch_module
    from pdrl_amd.utils import load_params

    continuous = algo.endswith("Continuous")
    p = load_params()
    p.algo, p.rows_kernel, p.hidden_size = algo, rows_kernel, hidden
    p.obs_dim, p.n_actions = (3, 1) if continuous else (4, 2)
    upd_cls, model_cls = switch_module(algo)
    model = model_cls(p.obs_dim, p.n_actions, p.seq_len, p.hidden_size)
    with pytest.raises(ValueError, match="rows_kernel"):
        upd_cls(model, p, "cpu")
