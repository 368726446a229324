"""Serving layer: a FastAPI scoring daemon over the fused HIP predict
path.

The reference has no serving story (scores are produced offline by a
notebook); this daemon keeps a checkpoint resident on the GPU and scores
cross-sections on demand: 612 req/s / 184k stock-scores/s at p50
1.6 ms over loopback HTTP on CSI300-shaped days via /score_raw
(measured on 1×MI355X, profiles/r2_serving.md; eager CPU fallback when
no GPU is present).

Run:  python -m factorvae_amd.serve --checkpoint best_models/x.pt \
          [--num_factor 96 --hidden_size 64 ...] [--port 8321]

Endpoints:
  GET  /health                -> {"status": "ok", "device": ..., "engine": ...}
  GET  /model                 -> model hyperparameters
  POST /score                 -> body {"x": [[..T*C floats..] per stock]}
                                 (shape (N, T, C)) -> {"scores": [N floats]}
  POST /score_batch           -> body {"days": [ (N_i, T, C) nested lists ]}
                                 -> {"scores": [ [N_i floats] ... ]}
  POST /score_many            -> body {"days": [...], "dist": false}: every
                                 day scored in ONE batched GPU call ->
                                 {"days": [{"scores": [...]} ...]} (plus
                                 "mu" / "sigma" per day with dist)
"""

from __future__ import annotations

import argparse
from typing import List, Optional

import torch

from .models.modules import build_factorvae
from .utils import load_model, test_args


class ScoringEngine:
    """Checkpoint-resident scorer; fused HIP path on GPU, eager on CPU."""

    def __init__(self, checkpoint: Optional[str], num_latent: int,
                 hidden_size: int, num_portfolio: int, num_factor: int,
                 seq_length: int, device: Optional[str] = None):
        self.seq_length = seq_length
        self.num_latent = num_latent
        self.hp = dict(num_latent=num_latent, hidden_size=hidden_size,
                       num_portfolio=num_portfolio, num_factor=num_factor,
                       seq_length=seq_length)
        self.device = torch.device(
            device or ("cuda" if torch.cuda.is_available() else "cpu"))
        args = test_args(run_name="serve", num_factor=num_factor,
                         hidden_size=hidden_size, num_latent=num_latent,
                         num_portfolio=num_portfolio, seq_length=seq_length)
        self.model = load_model(args)
        if checkpoint:
            state = torch.load(checkpoint, map_location="cpu",
                               weights_only=True)
            self.model.load_state_dict(state)
        self.model.to(self.device).eval()

        self.trainer = None
        self.engine = "eager"
        if self.device.type == "cuda":
            try:
                from .engine.fused import FusedTrainer

                self.trainer = FusedTrainer(self.model, lr=0.0, t_max=1,
                                            device=self.device, train=False)
                self.engine = "fused"
            except Exception:
                self.trainer = None

    @torch.no_grad()
    def score(self, x: torch.Tensor) -> torch.Tensor:
        """(N, T, C) fp32 -> (N,) prediction scores."""
        if x.ndim != 3 or x.shape[1] != self.seq_length \
                or x.shape[2] != self.num_latent:
            raise ValueError(
                f"expected (N, {self.seq_length}, {self.num_latent}), "
                f"got {tuple(x.shape)}")
        x = x.to(self.device, dtype=torch.float32)
        if self.trainer is not None:
            out = self.trainer.predict(x)
        else:
            out = self.model.prediction(x)
        return out.reshape(-1).cpu()

    @torch.no_grad()
    def score_many(self, xs, dist: bool = False):
        """List of (N_i, T, C) days -> one dict per day with "scores"
        (and "mu" / "sigma" with dist), all days in one batched call
        (FusedTrainer.predict_many) on the fused engine."""
        days = []
        for x in xs:
            if x.ndim != 3 or x.shape[1] != self.seq_length \
                    or x.shape[2] != self.num_latent:
                raise ValueError(
                    f"expected (N, {self.seq_length}, {self.num_latent}), "
                    f"got {tuple(x.shape)}")
            days.append(x.to(dtype=torch.float32))
        if self.trainer is not None:
            outs = self.trainer.predict_many(days, return_dist=dist)
        else:
            outs = []
            for x in days:
                x = x.to(self.device)
                if dist:
                    mu, sigma = self.model.prediction_dist(x)
                    outs.append((mu + torch.randn_like(sigma) * sigma, mu,
                                 sigma))
                else:
                    outs.append(self.model.prediction(x))
        res = []
        for o in outs:
            if dist:
                res.append({"scores": o[0].reshape(-1).tolist(),
                            "mu": o[1].reshape(-1).tolist(),
                            "sigma": o[2].reshape(-1).tolist()})
            else:
                res.append({"scores": o.reshape(-1).tolist()})
        return res


try:  # module-level request models (FastAPI resolves annotations here)
    from fastapi import Request, Response
    from pydantic import BaseModel

    class ScoreRequest(BaseModel):
        x: List[List[List[float]]]  # (N, T, C)

    class BatchRequest(BaseModel):
        days: List[List[List[List[float]]]]

    class ManyRequest(BaseModel):
        days: List[List[List[List[float]]]]
        dist: bool = False
except ImportError:  # serving extras absent: ScoringEngine still usable
    ScoreRequest = BatchRequest = ManyRequest = Request = Response = None


def build_app(engine: ScoringEngine):
    from fastapi import FastAPI, HTTPException

    app = FastAPI(title="FactorVAE MI355X scoring daemon")

    @app.get("/health")
    def health():
        return {"status": "ok", "device": str(engine.device),
                "engine": engine.engine}

    @app.get("/model")
    def model_info():
        return engine.hp

    @app.post("/score")
    def score(req: ScoreRequest):
        try:
            x = torch.tensor(req.x, dtype=torch.float32)
            out = engine.score(x)
        except ValueError as e:
            raise HTTPException(status_code=422, detail=str(e))
        return {"scores": out.tolist()}

    @app.post("/score_batch")
    def score_batch(req: BatchRequest):
        try:
            outs = [engine.score(torch.tensor(d, dtype=torch.float32)).tolist()
                    for d in req.days]
        except ValueError as e:
            raise HTTPException(status_code=422, detail=str(e))
        return {"scores": outs}

    @app.post("/score_many")
    def score_many(req: ManyRequest):
        """All days of the request in one batched GPU call; with dist the
        predictive mean and risk come back next to the scores."""
        try:
            days = [torch.tensor(d, dtype=torch.float32) for d in req.days]
            return {"days": engine.score_many(days, dist=req.dist)}
        except ValueError as e:
            raise HTTPException(status_code=422, detail=str(e))

    @app.post("/score_raw")
    async def score_raw(request: Request):
        """Binary fast path for production clients: the body is the
        (N, T, C) cross-section as little-endian float32 bytes (N
        derived from the length); the response body is the N scores as
        float32 bytes. Avoids the JSON float parse/serialize that
        dominates /score (28 MB of text per CSI300 request)."""
        import numpy as np

        body = await request.body()
        per_row = engine.seq_length * engine.num_latent * 4
        if len(body) == 0 or len(body) % per_row != 0:
            raise HTTPException(
                status_code=422,
                detail=f"body must be N*{per_row} bytes of float32")
        n = len(body) // per_row
        try:
            x = torch.from_numpy(
                np.frombuffer(body, dtype="<f4").copy().reshape(
                    n, engine.seq_length, engine.num_latent))
            out = engine.score(x)
        except ValueError as e:
            raise HTTPException(status_code=422, detail=str(e))
        return Response(content=out.numpy().astype("<f4").tobytes(),
                        media_type="application/octet-stream")

    return app


def main(argv=None):
    p = argparse.ArgumentParser(description="FactorVAE scoring daemon")
    p.add_argument("--checkpoint", type=str, default=None)
    p.add_argument("--num_latent", type=int, default=158)
    p.add_argument("--hidden_size", type=int, default=64)
    p.add_argument("--num_portfolio", type=int, default=128)
    p.add_argument("--num_factor", type=int, default=96)
    p.add_argument("--seq_length", type=int, default=20)
    p.add_argument("--host", type=str, default="127.0.0.1")
    p.add_argument("--port", type=int, default=8321)
    p.add_argument("--device", type=str, default=None,
                   help="cuda / cpu (default: cuda if available)")
    args = p.parse_args(argv)

    engine = ScoringEngine(args.checkpoint, args.num_latent,
                           args.hidden_size, args.num_portfolio,
                           args.num_factor, args.seq_length,
                           device=args.device)
    app = build_app(engine)
    import uvicorn

    uvicorn.run(app, host=args.host, port=args.port)


if __name__ == "__main__":
    main()
