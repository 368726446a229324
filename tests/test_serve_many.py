"""The daemon's /score_many endpoint: several days in one request, with
the predictive mean and risk on demand (CPU eager path here)."""

import numpy as np
import pytest
import torch

fastapi = pytest.importorskip("fastapi")
from fastapi.testclient import TestClient

from factorvae_amd.serve import ScoringEngine, build_app


@pytest.fixture(scope="module")
def served():
    torch.manual_seed(0)
    eng = ScoringEngine(None, num_latent=12, hidden_size=8, num_portfolio=4,
                        num_factor=3, seq_length=5, device="cpu")
    return eng, TestClient(build_app(eng))


def test_score_many_matches_prediction_dist(served):
    eng, client = served
    rng = np.random.default_rng(2)
    days = [rng.standard_normal((n, 5, 12)).astype("float32")
            for n in (3, 9, 1)]
    r = client.post("/score_many", json={"days": [d.tolist() for d in days],
                                         "dist": True})
    assert r.status_code == 200
    out = r.json()["days"]
    assert [len(o["scores"]) for o in out] == [3, 9, 1]
    for d, o in zip(days, out):
        mu, sigma = eng.model.prediction_dist(torch.from_numpy(d))
        assert np.allclose(o["mu"], mu.reshape(-1).numpy(), atol=1e-6)
        assert np.allclose(o["sigma"], sigma.reshape(-1).numpy(), atol=1e-6)
        assert np.isfinite(o["scores"]).all()

    r = client.post("/score_many", json={"days": [d.tolist() for d in days]})
    assert r.status_code == 200
    assert all(set(o) == {"scores"} for o in r.json()["days"])


def test_score_many_rejects_a_wrong_shape(served):
    _, client = served
    bad = np.zeros((4, 6, 12)).tolist()
    r = client.post("/score_many", json={"days": [bad]})
    assert r.status_code == 422
