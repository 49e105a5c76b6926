"""The rollout_kernel key and DeviceRollout's ``kernel`` keyword: default,
way in from parameters.json and validation (no GPU needed)."""
import json

import pytest

from pdrl_amd.networks import MlpLSTMSingle
from pdrl_amd.ops.rollout import DeviceRollout
from pdrl_amd.utils import load_params


def test_rollout_kernel_defaults_to_row():
    assert load_params().rollout_kernel == "row"


def test_rollout_kernel_loads_from_parameters_json(tmp_path):
    cfg = vars(load_params())
    cfg["rollout_kernel"] = "tile"
    path = tmp_path / "parameters.json"
    path.write_text(json.dumps(cfg))
    assert load_params(path).rollout_kernel == "tile"


@pytest.mark.parametrize("kernel,hidden", [("bogus", 64), ("tile", 128)])
def test_device_rollout_rejects_bad_kernel(kernel, hidden):
    core = MlpLSTMSingle(4, 2, 5, hidden).actor.core
    with pytest.raises(ValueError, match="rollout kernel"):
        DeviceRollout(core, "CartPole-v1", 4, 5, "cpu", 1, time_horizon=500,
                      kernel=kernel)


def test_eager_path_ignores_the_kernel():
    core = MlpLSTMSingle(4, 2, 5, 64).actor.core
    ro = DeviceRollout(core, "CartPole-v1", 4, 5, "cpu", 1, time_horizon=500,
                       kernel="tile")
    assert ro.eager and ro.kernel == "tile"
    assert ro.rollout()["obs"].shape == (4, 5, 4)
