"""The vmpo_mid_kernel key: its default and its validation (no GPU needed)."""
import pytest


def test_vmpo_mid_kernel_defaults_to_block():
    from pdrl_amd.utils import load_params

    assert load_params().vmpo_mid_kernel == "block"


def test_updater_rejects_bad_vmpo_mid_kernel():
    from pdrl_amd.agents.learner_module import VMPOUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params

    p = load_params()
    p.algo, p.obs_dim, p.n_actions = "V-MPO", 4, 2
    p.vmpo_mid_kernel = "bogus"
    model = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)
    with pytest.raises(ValueError, match="vmpo_mid_kernel"):
        VMPOUpdater(model, p, "cpu")
