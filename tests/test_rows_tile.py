"""The rows_kernel key: its default, its validation and its way in from
parameters.json (no GPU needed)."""
import json

import pytest


def _updater(**keys):
    from pdrl_amd.agents.learner_module import ImpalaUpdater
    from pdrl_amd.networks import MlpLSTMSingle
    from pdrl_amd.utils import load_params

    p = load_params()
    p.algo, p.obs_dim, p.n_actions = "IMPALA", 4, 2
    for k, v in keys.items():
        setattr(p, k, v)
    model = MlpLSTMSingle(4, 2, p.seq_len, p.hidden_size)
    return ImpalaUpdater(model, p, "cpu")


def test_rows_kernel_defaults_to_row():
    from pdrl_amd.utils import load_params

    assert load_params().rows_kernel == "row"


def test_rows_kernel_loads_from_parameters_json(tmp_path):
    from pdrl_amd.utils import load_params

    cfg = vars(load_params())
    cfg["rows_kernel"] = "tile"
    path = tmp_path / "parameters.json"
    path.write_text(json.dumps(cfg))
    assert load_params(path).rows_kernel == "tile"
    _updater(rows_kernel="tile")  # accepted at hidden_size 64


@pytest.mark.parametrize("keys", [
    dict(rows_kernel="bogus"),
    dict(rows_kernel="tile", hidden_size=128),
])
def test_updater_rejects_bad_rows_kernel(keys):
    with pytest.raises(ValueError, match="rows_kernel"):
        _updater(**keys)
