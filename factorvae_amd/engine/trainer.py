"""Training / validation loops and the experiment driver.

Functional equivalents of /root/reference/train_model.py:11-82 and
/root/reference/main.py:19-87, re-designed for MI355X:

- epoch-loss readback is a single D2H sync per epoch (the reference
  calls loss.item() every step, train_model.py:28);
- gradients live in one flat bucket all-reduced over RCCL when
  distributed (parallel.ddp);
- optional device-resident epoch cache removes all per-epoch host
  traffic;
- best-val checkpointing uses the reference's state_dict contract and
  file-name schema (main.py:73-80).
"""

from __future__ import annotations

import os
from typing import Optional

import torch
import torch.optim as optim

from ..models.modules import build_factorvae
from ..parallel.ddp import (
    FlatGradBucket,
    all_reduce_scalar,
    get_rank,
    get_world_size,
    init_distributed,
    is_distributed,
)
from ..utils import checkpoint_path, set_seed


def resolve_engine(engine: str, hidden_size: int, device_type: str,
                   warn: bool = True) -> str:
    """Pick the execution engine. "auto" = fused on GPU, eager on CPU;
    shapes outside the fused kernels' envelope (hidden_size > 64) fall
    back to eager with a warning instead of failing (the public CLI
    accepts any --hidden_size)."""
    engine = engine or "auto"
    if engine == "auto":
        engine = "fused" if device_type == "cuda" else "eager"
    if engine == "fused" and device_type != "cuda":
        if warn:
            import warnings
            warnings.warn(
                "--engine fused requires a GPU (HIP streams/graphs); "
                "falling back to the eager engine on this CPU-only "
                "machine", RuntimeWarning, stacklevel=2)
        engine = "eager"
    if engine == "fused" and hidden_size > 64:
        if warn:
            import warnings
            warnings.warn(
                f"hidden_size={hidden_size} exceeds the fused engine's "
                f"H<=64 kernel envelope; falling back to the eager engine",
                RuntimeWarning, stacklevel=2)
        engine = "eager"
    return engine


def _split_batch(char_with_label: torch.Tensor, device: torch.device):
    """Slice the (N,T,C+1) block into features (N,T,C) and the last-step
    label (N,1) (/root/reference/train_model.py:18-24)."""
    char = char_with_label[:, :, :-1]
    returns = char_with_label[:, :, -1]
    inputs = char.to(device).float()
    labels = returns[:, -1].reshape(-1, 1).to(device).float()
    return inputs, labels


def train(factor_model, dataloader, optimizer, scheduler, args=None,
          grad_bucket: Optional[FlatGradBucket] = None,
          device: Optional[torch.device] = None) -> float:
    """One epoch over day-batches; returns mean loss over days
    (/root/reference/train_model.py:11-37)."""
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    factor_model.to(device)
    factor_model.train()

    total_loss = torch.zeros((), device=device)
    n_batches = 0
    for char_with_label, _ in dataloader:
        inputs, labels = _split_batch(char_with_label, device)

        if grad_bucket is not None:
            grad_bucket.zero_()
        else:
            optimizer.zero_grad(set_to_none=True)

        loss, *_ = factor_model(inputs, labels)
        total_loss += loss.detach()
        loss.backward()
        if grad_bucket is not None:
            grad_bucket.all_reduce_()
        optimizer.step()
        if scheduler is not None:
            scheduler.step()
        n_batches += 1

    return (total_loss / max(n_batches, 1)).item()


@torch.no_grad()
def validate(factor_model, dataloader, args=None,
             device: Optional[torch.device] = None) -> float:
    """Eval epoch: mean full VAE loss (decoder still samples, dropout off)
    (/root/reference/train_model.py:40-60)."""
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    factor_model.to(device)
    factor_model.eval()

    total_loss = torch.zeros((), device=device)
    n_batches = 0
    for char_with_label, _ in dataloader:
        inputs, labels = _split_batch(char_with_label, device)
        loss, *_ = factor_model(inputs, labels)
        total_loss += loss.detach()
        n_batches += 1
    return (total_loss / max(n_batches, 1)).item()


@torch.no_grad()
def test(factor_model, dataloader, args=None,
         device: Optional[torch.device] = None) -> float:
    """Size-weighted eval epoch (/root/reference/train_model.py:62-82;
    kept for API parity — its averaging convention is the reference's)."""
    if device is None:
        device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    factor_model.to(device)
    factor_model.eval()

    total_loss = torch.zeros((), device=device)
    n_batches = 0
    for char_with_label, _ in dataloader:
        inputs, labels = _split_batch(char_with_label, device)
        loss, *_ = factor_model(inputs, labels)
        total_loss += loss.detach() * inputs.size(0)
        n_batches += 1
    return (total_loss / max(n_batches, 1)).item()


def train_main(args, data_args, df=None) -> float:
    """Experiment driver (/root/reference/main.py:19-87): build model and
    loaders, Adam + CosineAnnealingLR(T_max=days*epochs), epoch loop with
    best-val state_dict checkpointing. Distributed-aware: day-sharded
    loaders, flat-bucket gradient all-reduce, val-loss all-reduce,
    rank-0-only checkpointing. Returns best validation loss.

    Opt-in ranking metrics: args.val_metrics computes the validation
    range's daily IC / RankIC summary on the predictive mean after every
    epoch (on the device with the fused engine, metrics.py's oracle with
    the eager one) and logs it; args.select_by = "rankic" (implies
    val_metrics) keeps the checkpoint of the best validation RankIC
    instead of the lowest validation loss. args.val_batched (fused engine;
    the eager one ignores it) takes the validation loss from the batched
    posterior pass, FusedTrainer.validate_epoch(batched=True); together
    with val_metrics one validate_metrics(with_loss=True) pass over the
    validation range yields the loss and the ranking metrics.
    args.val_panel (implies val_batched) holds the validation range as a
    data.panel.PanelDays, each (stock, date) row once, and sends those
    passes through the panel route; every rank then validates the whole
    range. Logged keys and checkpoint selection are the same either way.

    Engines (args.engine, default "auto" = fused on GPU, eager on CPU):
    - "fused": the MI355X production path — device-resident epoch cache
      (one H2D per day ever), hipGraph-captured HIP-kernel step, fused
      Adam, one-bucket RCCL all-reduce.
    - "eager": the PyTorch-ROCm oracle path (same math via modules.py).
    New-engine additions over the reference: JSONL/wandb metrics, a
    cross-sections/sec step timer, and a true-resume side-car (optimizer
    + epoch state next to the weights-only reference checkpoint).
    """
    import pandas as pd

    from ..data.sampler import init_data_loader
    from ..observability import MetricsLogger, StepTimer

    rank = init_distributed()
    world_size = get_world_size()
    set_seed(args.seed)

    if rank == 0 and not os.path.exists(args.save_dir):
        os.makedirs(args.save_dir, exist_ok=True)

    factorVAE = build_factorvae(
        num_latent=args.num_latent,
        hidden_size=args.hidden_size,
        num_portfolio=args.num_portfolio,
        num_factor=args.num_factor,
    )

    if df is None:
        df = pd.read_pickle(args.dataset).iloc[:, :159]
        df = df.rename(columns={df.columns[-1]: "LABEL0"})

    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    engine = resolve_engine(getattr(args, "engine", "auto"),
                            args.hidden_size, device.type)
    if engine != "fused" and getattr(args, "dtype", "fp32") != "fp32":
        import warnings
        warnings.warn(
            f"--dtype {args.dtype} only applies to the fused engine; the "
            "eager path runs fp32", RuntimeWarning, stacklevel=2)

    logger = MetricsLogger(args.run_name, out_dir=args.save_dir,
                           use_wandb=getattr(args, "wandb", False),
                           config={k: v for k, v in vars(args).items()
                                   if isinstance(v, (int, float, str, bool))},
                           rank=rank)
    timer = StepTimer(device)
    save_root = checkpoint_path(args.save_dir, args.run_name,
                                args.num_factor, args.hidden_size,
                                args.num_portfolio, args.seed)
    sidecar = save_root + ".opt"
    resume = bool(getattr(args, "resume", False))
    select_by = getattr(args, "select_by", None)
    if (select_by is None and resume and os.path.exists(save_root)
            and os.path.exists(sidecar)):
        # a resumed run goes on selecting the way the side-car's run did
        select_by = torch.load(sidecar, map_location="cpu",
                               weights_only=True).get("select_by")
    select_by = select_by or "loss"
    if select_by not in ("loss", "rankic"):
        raise ValueError(f"select_by must be loss or rankic, got {select_by}")
    val_metrics = (bool(getattr(args, "val_metrics", False))
                   or select_by == "rankic")
    val_topk = int(getattr(args, "val_topk", 0) or 0)
    val_batched = bool(getattr(args, "val_batched", False))
    # the validation range as a PanelDays (implies val_batched); the fp8
    # engine has no batched validation to send it through
    val_panel = (bool(getattr(args, "val_panel", False))
                 and engine == "fused"
                 and getattr(args, "dtype", "fp32") != "fp8")
    val_batched = val_batched or val_panel

    if engine == "fused":
        from ..data.device_cache import DeviceEpochCache
        from ..data.panel import PanelDays
        from .fused import FusedTrainer

        # unsharded loaders -> every rank caches all days once (288 GB
        # HBM3E), then each epoch does the sampler-equivalent global
        # shuffle + round-robin shard on device-resident tensors
        nw = int(getattr(args, "num_workers", 0) or 0)
        train_cache = DeviceEpochCache(init_data_loader(
            df, shuffle=False, step_len=data_args.seq_len,
            start=data_args.start_time, end=data_args.fit_end_time,
            select_feature=data_args.select_feature, num_workers=nw),
            device, seed=args.seed)
        valid_loader = init_data_loader(
            df, shuffle=False, step_len=data_args.seq_len,
            start=data_args.val_start_time, end=data_args.val_end_time,
            select_feature=data_args.select_feature, num_workers=nw)
        if val_panel:
            # every rank holds the whole range once per (stock, date) row
            # and validates all of it
            valid_days = PanelDays.from_loader(valid_loader).to(device)
        else:
            valid_cache = DeviceEpochCache(valid_loader, device,
                                           seed=args.seed)
            valid_days = valid_cache.days

        steps_per_epoch = train_cache.num_batches(rank, world_size)
        trainer = FusedTrainer(factorVAE, lr=args.lr,
                               t_max=steps_per_epoch * args.num_epochs,
                               device=device,
                               dtype=getattr(args, "dtype", "fp32"))
        optimizer = scheduler = grad_bucket = None
    else:
        train_dataloader = init_data_loader(
            df, shuffle=True, step_len=data_args.seq_len,
            start=data_args.start_time, end=data_args.fit_end_time,
            select_feature=data_args.select_feature,
            rank=rank, world_size=world_size, seed=args.seed,
            num_workers=int(getattr(args, "num_workers", 0) or 0),
        )
        valid_dataloader = init_data_loader(
            df, shuffle=False, step_len=data_args.seq_len,
            start=data_args.val_start_time, end=data_args.val_end_time,
            select_feature=data_args.select_feature,
            rank=rank, world_size=world_size, seed=args.seed,
        )
        if val_metrics:
            # the full validation range on every rank: no communication,
            # no wrap-pad duplicates
            metric_days = [_split_batch(cwl, device) for cwl, _ in
                           init_data_loader(
                               df, shuffle=False, step_len=data_args.seq_len,
                               start=data_args.val_start_time,
                               end=data_args.val_end_time,
                               select_feature=data_args.select_feature)]
        T_max = len(train_dataloader) * args.num_epochs
        factorVAE.to(device)
        grad_bucket = (FlatGradBucket(factorVAE.parameters())
                       if is_distributed() else None)
        optimizer = optim.Adam(factorVAE.parameters(), lr=args.lr)
        scheduler = optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=T_max)
        trainer = None

    start_epoch = 0
    best_val_loss = float("inf")
    best_val_rankic = float("-inf")
    if resume and os.path.exists(save_root) and os.path.exists(sidecar):
        state = torch.load(save_root, map_location=device, weights_only=True)
        factorVAE.load_state_dict(state)
        side = torch.load(sidecar, map_location="cpu", weights_only=True)
        start_epoch = int(side.get("epoch", 0))
        best_val_loss = float(side.get("best_val_loss", float("inf")))
        best_val_rankic = float(side.get("best_val_rankic", float("-inf")))
        if trainer is not None and "fused_opt" in side:
            trainer.load_opt_state_dict(side["fused_opt"])
        elif optimizer is not None and "optimizer" in side:
            optimizer.load_state_dict(side["optimizer"])
            scheduler.load_state_dict(side["scheduler"])
        if rank == 0:
            print(f"Resumed from {save_root} at epoch {start_epoch}")

    for epoch in range(start_epoch, args.num_epochs):
        timer.start()
        if engine == "fused":
            days = list(train_cache.order(epoch, shuffle=True, rank=rank,
                                          world_size=world_size))
            train_loss = trainer.train_epoch(days)
            timer.tick(len(days))
            rate = timer.rate()
            vm = None
            if val_batched and val_metrics:
                # one batched pass over the full validation range gives
                # the loss and the ranking metrics
                vm = trainer.validate_metrics(valid_days, topk=val_topk,
                                              with_loss=True)
                val_loss = vm["loss"]
            elif val_panel:
                val_loss = trainer.validate_epoch(valid_days, batched=True)
            else:
                val_days = list(valid_cache.order(0, shuffle=False, rank=rank,
                                                  world_size=world_size))
                val_loss = trainer.validate_epoch(val_days,
                                                  batched=val_batched)
        else:
            if hasattr(train_dataloader.batch_sampler, "set_epoch"):
                train_dataloader.batch_sampler.set_epoch(epoch)
            train_loss = train(factorVAE, train_dataloader, optimizer,
                               scheduler, args, grad_bucket=grad_bucket,
                               device=device)
            timer.tick(len(train_dataloader))
            rate = timer.rate()
            val_loss = validate(factorVAE, valid_dataloader, args,
                                device=device)
        val_loss = all_reduce_scalar(val_loss, device=device)
        train_loss = all_reduce_scalar(train_loss, device=device)
        rate_total = all_reduce_scalar(rate, device=device, average=False)

        if rank == 0:
            print(f"Epoch {epoch + 1}: Train Loss: {train_loss:.4f}, "
                  f"Validation Loss: {val_loss:.4f}, "
                  f"{rate_total:.1f} cross-sections/s")
        record = {"Train Loss": train_loss, "Validation Loss": val_loss,
                  "cross_sections_per_sec": rate_total}
        rankic = float("nan")
        if val_metrics:
            if engine == "fused":
                if vm is None:
                    vm = trainer.validate_metrics(valid_days, topk=val_topk)
            else:
                from ..metrics import evaluate_days_eager, summarize_ic
                vm = summarize_ic(evaluate_days_eager(
                    factorVAE, metric_days, on=("mu",), topk=val_topk))
            rankic = vm["RankIC"]
            if rank == 0:
                print(f"Epoch {epoch + 1}: Validation IC: {vm['IC']:.4f}, "
                      f"Validation RankIC: {rankic:.4f}, "
                      f"Validation RankIC_IR: {vm['RankIC_IR']:.4f}")
            record.update({"Validation IC": vm["IC"],
                           "Validation RankIC": rankic,
                           "Validation RankIC_IR": vm["RankIC_IR"]})
            if val_topk > 0:
                record["Validation long_short"] = vm["long_short"]
        logger.log(record, step=epoch)
        if select_by == "rankic":
            improved = rankic > best_val_rankic  # False for NaN
            best_val_loss = min(best_val_loss, val_loss)
            if improved:
                best_val_rankic = rankic
        else:
            improved = val_loss < best_val_loss
            if improved:
                best_val_loss = val_loss
            if val_metrics and rankic > best_val_rankic:
                best_val_rankic = rankic
        if improved:
            if rank == 0:
                torch.save(factorVAE.state_dict(), save_root)
                side = {"epoch": epoch + 1, "best_val_loss": best_val_loss}
                if select_by == "rankic":
                    side["select_by"] = select_by
                    side["best_val_rankic"] = best_val_rankic
                if trainer is not None:
                    side["fused_opt"] = trainer.opt_state_dict()
                else:
                    side["optimizer"] = optimizer.state_dict()
                    side["scheduler"] = scheduler.state_dict()
                torch.save(side, sidecar)
                print(f"Model saved at {save_root}")

    summary = {"Best Validation Loss": best_val_loss}
    if val_metrics:
        summary["Best Validation RankIC"] = (
            best_val_rankic if best_val_rankic > float("-inf")
            else float("nan"))
    logger.finish(summary)
    return best_val_loss
