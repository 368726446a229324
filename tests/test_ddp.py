"""Distributed data-parallel tests (gloo backend, world_size=2, CPU).

Validates the DP design the HIP/RCCL path relies on: flat-bucket
gradient all-reduce, round-robin day sharding, and 2-rank equivalence
with a single-rank run over the same two days.
"""

import multiprocessing as mp
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

from factorvae_amd.models.modules import build_factorvae
from factorvae_amd.parallel.ddp import FlatGradBucket
from factorvae_amd.utils import set_seed

C, H, M, K, N, T = 10, 8, 12, 4, 16, 5


def _make_day(seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, T, C, generator=g)
    y = torch.randn(N, 1, generator=g)
    return x, y


def _worker(rank, world_size, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        set_seed(0)
        model = build_factorvae(num_latent=C, hidden_size=H, num_portfolio=M, num_factor=K)
        model.eval()  # dropout off for determinism; decoder eps seeded below
        bucket = FlatGradBucket(model.parameters())

        x, y = _make_day(100 + rank)  # each rank its own day
        torch.manual_seed(1234)  # identical eps draw on both ranks
        loss, *_ = model(x, y)
        bucket.zero_()
        loss.backward()
        bucket.flat.div_(world_size)
        dist.all_reduce(bucket.flat, op=dist.ReduceOp.SUM)
        q.put((rank, float(loss.item()), bucket.flat.clone().numpy()))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_two_rank_flat_allreduce_matches_grad_average():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29511
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        rank, loss, flat = q.get(timeout=110)
        results[rank] = (loss, flat)
    for p in procs:
        p.join(timeout=30)

    # reference: serial grad average of the two days on one model
    set_seed(0)
    model = build_factorvae(num_latent=C, hidden_size=H, num_portfolio=M, num_factor=K)
    model.eval()
    bucket = FlatGradBucket(model.parameters())
    accum = torch.zeros_like(bucket.flat)
    for r in range(2):
        x, y = _make_day(100 + r)
        torch.manual_seed(1234)
        loss, *_ = model(x, y)
        bucket.zero_()
        loss.backward()
        accum += bucket.flat / 2

    np.testing.assert_allclose(results[0][1], accum.numpy(), atol=1e-5)
    np.testing.assert_allclose(results[0][1], results[1][1], atol=1e-6)


def test_flat_bucket_is_view_of_grads():
    set_seed(3)
    model = build_factorvae(num_latent=C, hidden_size=H, num_portfolio=M, num_factor=K)
    bucket = FlatGradBucket(model.parameters())
    total = sum(p.numel() for p in model.parameters())
    assert bucket.flat.numel() == total
    x, y = _make_day(7)
    model.eval()
    loss, *_ = model(x, y)
    loss.backward()
    # grads landed in the arena (views share storage)
    assert bucket.flat.abs().sum() > 0
    for p in model.parameters():
        assert p.grad is not None
        assert p.grad.data_ptr() >= bucket.flat.data_ptr()
        assert p.grad.data_ptr() < bucket.flat.data_ptr() + bucket.flat.numel() * 4


def _train_main_worker(rank, world_size, port, tmpdir, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ["WORLD_SIZE"] = str(world_size)
    os.environ["RANK"] = str(rank)
    os.environ["LOCAL_RANK"] = str(rank)
    try:
        from types import SimpleNamespace

        from factorvae_amd.data.synthetic import make_synthetic_frame
        from factorvae_amd.engine.trainer import train_main
        from factorvae_amd.utils import DataArgument, checkpoint_path

        df = make_synthetic_frame(n_days=24, n_stocks=20, seed=5)
        args = SimpleNamespace(
            num_epochs=2, lr=1e-3, num_latent=158, num_portfolio=8,
            seq_len=6, num_factor=4, hidden_size=16, seed=0,
            run_name="ddp_e2e", save_dir=tmpdir, dataset=None,
            engine="eager", wandb=False, resume=False,
        )
        data_args = DataArgument(
            start_time="2015-01-01", end_time="2015-12-31",
            fit_end_time="2015-01-28", val_start_time="2015-01-29",
            val_end_time="2015-02-04", seq_len=6,
        )
        best = train_main(args, data_args, df=df)
        ckpt = checkpoint_path(tmpdir, "ddp_e2e", 4, 16, 8, 0)
        q.put((rank, best, os.path.exists(ckpt), os.path.exists(ckpt + ".opt")))
    except Exception as e:  # surface failures to the parent
        import traceback
        q.put((rank, f"ERROR: {e}\n{traceback.format_exc()}", False, False))
    finally:
        if dist.is_initialized():
            dist.destroy_process_group()


@pytest.mark.timeout(240)
def test_train_main_two_rank_end_to_end(tmp_path, monkeypatch):
    """Full experiment driver on 2 gloo ranks: day sharding, loss
    all-reduce, rank-0 best-val checkpoint + optimizer side-car."""
    # CPU/gloo ranks: the spawned workers must not see a GPU (rank r
    # would select GPU r, which a 1-GPU machine does not have); an
    # out-of-range index leaves no device visible to them
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "-1")
    monkeypatch.setenv("CUDA_VISIBLE_DEVICES", "-1")
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_train_main_worker,
                         args=(r, 2, 29533, str(tmp_path), q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    try:
        for _ in range(2):
            rank, best, has_ckpt, has_side = q.get(timeout=200)
            assert not isinstance(best, str), best
            results[rank] = (best, has_ckpt, has_side)
        for p in procs:
            p.join(timeout=60)
    finally:
        # a failed rank must not leave its peer waiting in a collective
        for p in procs:
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    # identical best-val on both ranks (all-reduced), rank 0 wrote files
    assert results[0][0] == pytest.approx(results[1][0], rel=1e-5)
    assert results[0][1] and results[0][2]


# ---------------------------------------------------------------- odd days
class _FakeLoader:
    """Minimal stand-in yielding (N,T,C+1) day blocks for DeviceEpochCache."""

    def __init__(self, n_days, n=4, t=3, c=5):
        self.blocks = [(torch.randn(n, t, c + 1), None) for _ in range(n_days)]

    def __iter__(self):
        return iter(self.blocks)


def test_device_cache_padded_sharding_equal_counts():
    """n_days % world_size != 0: every rank still gets the same step count
    (padded wrap-around), so per-step collectives stay in lockstep and
    t_max = num_batches * epochs agrees across ranks."""
    from factorvae_amd.data.device_cache import DeviceEpochCache

    for n_days, ws in [(5, 2), (3, 2), (7, 4), (2, 4), (6, 3)]:
        cache = DeviceEpochCache(_FakeLoader(n_days), torch.device("cpu"))
        counts = []
        seen = set()
        for r in range(ws):
            days = list(cache.order(epoch=1, shuffle=True, rank=r, world_size=ws))
            counts.append(len(days))
            assert len(days) == cache.num_batches(r, ws)
            for x, _ in days:
                seen.add(x.data_ptr())
        assert len(set(counts)) == 1, (n_days, ws, counts)
        assert counts[0] == (n_days + ws - 1) // ws
        # union of shards covers every day exactly (padding repeats some)
        assert len(seen) == n_days


def test_batch_sampler_padded_sharding_equal_counts():
    from factorvae_amd.data.sampler import init_data_loader
    from factorvae_amd.data.synthetic import make_synthetic_frame

    df = make_synthetic_frame(n_days=15, n_stocks=6, seed=11)
    lens = []
    for r in range(2):
        dl = init_data_loader(df, step_len=4, shuffle=True, start=None,
                              end=None, rank=r, world_size=2, seed=3)
        batches = list(dl.batch_sampler)
        lens.append(len(batches))
        assert len(batches) == len(dl.batch_sampler)
    assert lens[0] == lens[1]


def _odd_day_worker(rank, world_size, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        from factorvae_amd.data.device_cache import DeviceEpochCache
        
        set_seed(0)
        model = build_factorvae(num_latent=C, hidden_size=H,
                                num_portfolio=M, num_factor=K)
        bucket = FlatGradBucket(model.parameters())
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        cache = DeviceEpochCache(_FakeLoader(3, n=N, t=T, c=C),
                                 torch.device("cpu"))
        # 3 days, 2 ranks: without padding rank 1 would run 1 step while
        # rank 0 runs 2 -> mismatched all_reduce count -> hang here
        steps = 0
        for inputs, labels in cache.order(0, shuffle=True, rank=rank,
                                          world_size=world_size):
            bucket.zero_()
            loss, *_ = model(inputs, labels)
            loss.backward()
            bucket.all_reduce_()
            opt.step()
            steps += 1
        q.put((rank, steps))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_odd_day_count_two_ranks_no_hang():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_odd_day_worker, args=(r, 2, 29534, q))
             for r in range(2)]
    for p in procs:
        p.start()
    results = {}
    for _ in range(2):
        rank, steps = q.get(timeout=100)
        results[rank] = steps
    for p in procs:
        p.join(timeout=30)
    assert results[0] == results[1] == 2
