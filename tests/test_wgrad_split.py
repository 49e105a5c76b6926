"""The wgrad_kernel key: its default and its validation (no GPU needed)."""
import pytest


def test_wgrad_kernel_defaults_to_sweep():
    from pdrl_amd.utils import load_params

    assert load_params().wgrad_kernel == "sweep"


def test_updater_rejects_bad_wgrad_kernel():
    from pdrl_amd.agents.learner_module import ImpalaUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params

    p = load_params()
    p.algo, p.obs_dim, p.n_actions = "IMPALA", 4, 2
    p.wgrad_kernel = "bogus"
    model = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)
    with pytest.raises(ValueError, match="wgrad_kernel"):
        ImpalaUpdater(model, p, "cpu")
