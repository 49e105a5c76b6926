"""The rows_kernel value "tile128": where it is accepted, where it is not,
and its way in from parameters.json (no GPU needed)."""
import json

import pytest


def _updater(algo="IMPALA", **keys):
    from pdrl_amd.agents.learner_module import switch_module
    from pdrl_amd.utils import load_params

    p = load_params()
    continuous = algo.endswith("Continuous")
    p.algo = algo
    p.obs_dim, p.n_actions = (3, 1) if continuous else (4, 2)
    for k, v in keys.items():
        setattr(p, k, v)
    upd_cls, model_cls = switch_module(algo)
    model = model_cls(p.obs_dim, p.n_actions, p.seq_len, p.hidden_size)
    return upd_cls(model, p, "cpu")


def test_tile128_loads_from_parameters_json_at_hidden_128(tmp_path):
    from pdrl_amd.utils import load_params

    cfg = vars(load_params())
    cfg["rows_kernel"], cfg["hidden_size"] = "tile128", 128
    path = tmp_path / "parameters.json"
    path.write_text(json.dumps(cfg))
    p = load_params(path)
    assert (p.rows_kernel, p.hidden_size) == ("tile128", 128)
    _updater(rows_kernel=p.rows_kernel, hidden_size=p.hidden_size)


@pytest.mark.parametrize("algo,hidden_size", [
    ("IMPALA", 64),            # the H = 128 tile at another width
    ("SAC", 128),              # the SAC steps take "row" and "tile" only
    ("SAC-Continuous", 128),
])
def test_tile128_rejected(algo, hidden_size):
    with pytest.raises(ValueError, match="rows_kernel"):
        _updater(algo, rows_kernel="tile128", hidden_size=hidden_size)
