"""Fused MI355X training engine.

Runs the whole FactorVAE training step — forward, hand-written backward,
flat-bucket gradient all-reduce, fused Adam + device-side cosine LR —
through the hand-written HIP kernels in factorvae_amd/ops/hip/, with the
kernel sequence captured into a hipGraph (one replay per trading-day
step; the reference pays ~100 eager ATen/cuDNN launches plus a D2H sync
per step, /root/reference/train_model.py:26-32).

Design:
- every parameter lives in ONE flat fp32 arena ordered so that the K
  attention heads' {query, key W, key b, value W, value b} are contiguous
  stacked (K,H,H)/(K,H) views (zero-copy kernel inputs; the module's
  Parameters are rebound to arena views so state_dict()/load_state_dict
  keep the reference checkpoint contract);
- gradients live in a mirror arena: backward kernels write/accumulate
  into views, the DP all-reduce is one RCCL call on the flat buffer, and
  Adam is one kernel over the arena;
- eps / dropout-mask RNG uses torch's generator OUTSIDE the graph (two
  tiny kernels per step), keeping set_seed reproducibility;
- four HIP streams per step: the main activation chain, two side
  streams for the weight-gradient reductions, and (in DP runs) a comm
  stream whose early all-reduce of the non-extractor gradient slice
  overlaps the extractor backward;
- loss stays on device; reading it is the caller's (async) choice.
"""

from __future__ import annotations

import math
import os
import warnings
from typing import Dict, Optional

import torch

from ..data.panel import PanelDays
from ..models.modules import FactorVAE
from ..ops import get_extension
from ..parallel.ddp import get_world_size, is_distributed


class UnsupportedShapeError(ValueError):
    """Model shape outside the fused kernels' tiling envelope; callers
    fall back to the eager (PyTorch-ROCm) engine."""


class _Arena:
    """Flat fp32 buffer + named views with a custom packing order."""

    def __init__(self, device, specs):
        # specs: list of (name, shape)
        self.offsets = {}
        total = 0
        for name, shape in specs:
            n = 1
            for s in shape:
                n *= s
            self.offsets[name] = (total, shape)
            total += n
        self.flat = torch.zeros(total, device=device, dtype=torch.float32)

    def view(self, name):
        off, shape = self.offsets[name]
        n = 1
        for s in shape:
            n *= s
        return self.flat[off:off + n].view(*shape)


class FusedTrainer:
    """Fused training engine for one FactorVAE model on one GPU rank."""

    DROPOUT_P = 0.1

    def __init__(self, model: FactorVAE, lr: float, t_max: int,
                 device: Optional[torch.device] = None, eta_min: float = 0.0,
                 use_graph: bool = True, max_stocks: Optional[int] = None,
                 train: bool = True, dtype: str = "fp32"):
        assert dtype in ("fp32", "bf16", "fp8")
        self.ext = get_extension()
        # bf16 mode (BASELINE.json configs 2-4): the FLOP-bound extractor
        # GEMM family (R = N*T rows) runs on bf16 MFMA (~2.5 PF/s dense on
        # gfx950 vs 157 TF/s f32) with fp32 accumulate; fp32 master
        # weights + fp32 Adam + fp32 grad all-reduce; the latency-bound
        # N-row kernels (encoder/attention/decoder/GRU recurrence) stay
        # fp32 — their cost is dispatch+LDS, not FLOPs.
        # fp8 mode (config 5): forward extractor GEMMs on fp8 e4m3 MFMA
        # (weights+activations; per-tensor weight scales, LN-normalized
        # activations at unit scale); backward reuses the bf16 path.
        self.bf16 = dtype in ("bf16", "fp8")
        self.fp8 = dtype == "fp8"
        self.dtype = dtype
        self.model = model
        self.device = device or torch.device("cuda")
        model.to(self.device)
        self.lr = lr
        self.eta_min = eta_min
        self.t_max = t_max
        self.training = train
        # FV_GRAPH=0: eager-launch every kernel (no hipGraph capture at
        # all) — the last-resort guard rail for capture-hostile boxes
        self.use_graph = use_graph and os.environ.get("FV_GRAPH",
                                                       "1") != "0"

        fe = model.feature_extractor
        self.C = fe.num_latent
        self.H = fe.hidden_size
        enc = model.factor_encoder
        self.M = enc.linear.out_features
        self.K = model.factor_predictor.num_factor
        if self.H > 64:
            # the GRU/attention kernel register/LDS tilings are sized for
            # H <= 64 (all reference checkpoints: H in {20, 32, 64});
            # callers catch this and fall back to the eager engine
            raise UnsupportedShapeError(
                f"fused engine supports hidden_size <= 64, got {self.H}; "
                f"use engine='eager'")

        self._build_param_arena()
        # bf16/fp8 @ H=64: Whh wgrad computed inside the GRU backward
        # kernel (FV_WHH_FUSED=0 restores the standalone TN call)
        self._whh_fused = (self.bf16 and self.H == 64
                           and os.environ.get("FV_WHH_FUSED", "1") != "0")
        # fp32: shortened backward tail. 1 (default) = paired Whh/Wih
        # wgrad + LeakyReLU backward in the Wih dgrad's epilogue, results
        # bit-identical to the old sequence; 2 = also the LayerNorm/W1x
        # gradients without the dxln GEMM (differs by fp32 rounding);
        # FV_F32_TAIL=0 restores the old kernel sequence
        self._f32_tail = 0
        if not self.bf16:
            self._f32_tail = {"0": 0, "2": 2}.get(
                os.environ.get("FV_F32_TAIL", "1"), 1)
        # fp32: LayerNorm + W1x projection + GRU input projection as one
        # kernel (bit-identical); FV_F32_HEAD=0 restores the three launches
        self._f32_head = (not self.bf16
                          and os.environ.get("FV_F32_HEAD", "1") != "0")
        # every dtype: the fp32 gemm_nn / gemm_tn kernels with the waits taken
        # out of their loops (variant=1 of the bindings) and, in the default
        # fp32 tail, the LayerNorm parameter gradients out of the dxln GEMM's
        # epilogue plus one reduce for the three weight gradients
        # (bit-identical); FV_F32_GEMM=0 restores the original kernels and
        # launch sequence
        self._gv = 0 if os.environ.get("FV_F32_GEMM", "1") == "0" else 1
        # every dtype: the latency-oriented attn_fused_fwd / attn_fused_bwd /
        # enc_fused_fwd kernels (bit-identical); FV_MID=0 restores the
        # original kernels
        self._mid = 0 if os.environ.get("FV_MID", "1") == "0" else 1
        # fp32, H = 64, N <= ext.gru_wave_max_n(): the GRU recurrence with
        # one wave per stock (variant=1 of gru_fwd / gru_fwd_infer / gru_bwd,
        # bit-identical); FV_F32_GRU=0 restores the f32 MFMA kernels
        self._gru_v = 0 if os.environ.get("FV_F32_GRU", "1") == "0" else 1
        # every dtype, N <= 384: the training step's middle chain
        # (docs/KERNELS.md): dec_fwd_bwd -> enc_bwd_mid on main with the loss
        # gradients formed at their consumers, instead of dec_fwd ->
        # loss_fused -> dec_bwd -> dec_bwd_reduce -> enc_bwd_fused
        # (bit-identical); FV_MID_CHAIN=0 restores that sequence. Needs the
        # latency-oriented attention backward, so FV_MID=0 turns it off too.
        self._mid_chain = (self._mid == 1 and self.device.type == "cuda"
                           and self.H <= 64 and self.K <= 128
                           and os.environ.get("FV_MID_CHAIN", "1") != "0")
        self._chain_pending = False
        # where the middle chain applies: the fused middle (docs/KERNELS.md).
        # Main runs gru_fwd -> mid_fwd -> mid_bwd -> enc_bwd_mid -> gru_bwd
        # with nothing to join: the attention and encoder forwards are one
        # launch, the attention backward and dec_fwd_bwd are one launch, and
        # in fp32 dh_combine is gru_bwd's prologue (bit-identical);
        # FV_MID_FUSE=0 restores the two-stream middle chain.
        self._mid_fuse = (self._mid_chain
                          and os.environ.get("FV_MID_FUSE", "1") != "0")
        self._fuse_pending = False
        # with the fused middle, in a captured step: the eps / dropout-mask
        # fills run on side stream 0 in front of attn_qk_fwd instead of at
        # the head of main. mid_fwd already waits for that stream, so no
        # edge is added, and the generator calls keep their order (same
        # draws). FV_RNG_SIDE=0 keeps them on main.
        self._rng_side = (self._mid_fuse
                          and os.environ.get("FV_RNG_SIDE", "1") != "0")
        self._rng_pending = False
        # whether the last fp32 backward ran dh_combine as gru_bwd's prologue
        self._combine_ran = False
        if self.bf16:
            C3 = 3 * self.H
            # padded (+ transposed-padded) weight shadows for the
            # register-stationary NT kernel: k dim zero-padded to a
            # multiple of 32 so the MFMA k-tail is exact (pads are
            # zeroed here once and never written by the refresh kernel)
            KPc = (self.C + 31) & ~31
            KP3 = (C3 + 31) & ~31
            zb = lambda *s: torch.zeros(*s, dtype=torch.bfloat16,
                                        device=self.device)
            self.w1x_p = zb(self.C, KPc)    # W1x (C,C) k-padded
            self.w1xT_p = zb(self.C, KPc)   # W1x^T
            self.wih_p = zb(C3, KPc)        # Wih (3H,C) k-padded
            self.wihT_p = zb(self.C, KP3)   # Wih^T (C,3H) k-padded
            self.whh_bf = torch.empty(C3, self.H, dtype=torch.bfloat16,
                                      device=self.device)
            if self.fp8:
                # row stride padded to 128 for the MX-scaled K=128 MFMA
                # path (the only fp8 form at the ~5 PF/s rate); pads are
                # zeroed here and never written (casts write Ci cols)
                ldp = ((self.C + 127) & ~127)
                self._fp8_rs = ldp <= 256
                if not self._fp8_rs:  # fallback: K=32 fp8 MFMA path
                    ldp = (self.C + 3) & ~3
                f8 = torch.float8_e4m3fn
                self.w1x_f8 = torch.zeros(self.C, ldp, dtype=f8,
                                          device=self.device)
                self.wih_f8 = torch.zeros(C3, ldp, dtype=f8,
                                          device=self.device)
                self.s_w1x = torch.ones(1, device=self.device)
                self.is_w1x = torch.ones(1, device=self.device)
                self.s_wih = torch.ones(1, device=self.device)
                self.is_wih = torch.ones(1, device=self.device)
                if self._fp8_rs:
                    # fp8 dgrad path: transposed padded weight shadows +
                    # delayed-scaling state for the two dgrad operands
                    # (amax collected this step -> scale next step)
                    KPt3 = (C3 + 127) & ~127
                    KPtC = (self.C + 127) & ~127
                    self.wihT_f8 = torch.zeros(self.C, KPt3, dtype=f8,
                                               device=self.device)
                    self.w1xT_f8 = torch.zeros(self.C, KPtC, dtype=f8,
                                               device=self.device)
                    one = lambda v: torch.full((1,), float(v),
                                               device=self.device)
                    self.amax_dgi = one(1.0)
                    self.s_dgi = one(448.0)
                    self.is_dgi = one(1.0 / 448.0)
                    self.amax_dzx = one(1.0)
                    self.s_dzx = one(448.0)
                    self.is_dzx = one(1.0 / 448.0)
            self._refresh_bf16_shadows()
        self.grads = torch.zeros_like(self.params.flat)
        self.adam_m = torch.zeros_like(self.params.flat)
        self.adam_v = torch.zeros_like(self.params.flat)
        self.step_t = torch.zeros(1, device=self.device, dtype=torch.int32)

        self._ws_n = 0
        self._ws_cache: Dict = {}
        self._graphs: Dict = {}
        self._g_inputs = None
        # side stream: weight-gradient GEMMs/colsums run here, overlapped
        # with the activation-gradient critical path (fork/join via events;
        # the dependencies are recorded into the captured hipGraph)
        self.s_side = (torch.cuda.Stream(device=self.device)
                       if self.device.type == "cuda" else None)
        # second side stream: the three big extractor wgrad reductions
        # run here so they overlap BOTH the main path and the other
        # (attention/encoder) wgrads — at A-share shapes the side work
        # exceeds the main path, so one side stream becomes the bottleneck
        self.s_side2 = (torch.cuda.Stream(device=self.device)
                        if self.device.type == "cuda" else None)
        # FV_MAIN_PRIO=1 (opt-in, default OFF): run the critical path on
        # a HIGH-priority stream. Measured MUCH slower on gfx950
        # (CSI300 2804 -> 1338 cs/s; A-share 591 -> 531): replaying the
        # graph from a priority queue appears to serialize the captured
        # side branches. Kept as a documented negative-result knob.
        self.s_main = None
        if (self.device.type == "cuda"
                and os.environ.get("FV_MAIN_PRIO", "0") == "1"):
            self.s_main = torch.cuda.Stream(device=self.device, priority=-1)
        # comm stream: in DP runs the attention/encoder/decoder slice of
        # the gradient arena (everything packed after the extractor) is
        # all-reduced here as soon as its last producer finishes,
        # overlapped with the extractor backward; the extractor slice
        # follows after the join (xGMI ring latency hides under ~40% of
        # the backward)
        self.s_comm = (torch.cuda.Stream(device=self.device)
                       if self.device.type == "cuda" else None)

    # ---------------------------------------------------------------- params
    def _param_specs(self):
        m = self.model
        C, H, M, K = self.C, self.H, self.M, self.K
        specs = []

        def add(name, param):
            specs.append((name, param, tuple(param.shape)))

        fe = m.feature_extractor
        add("ln_g", fe.normalize.weight)
        add("ln_b", fe.normalize.bias)
        add("W1x", fe.linear.weight)
        add("b1x", fe.linear.bias)
        add("Wih", fe.gru.weight_ih_l0)
        add("Whh", fe.gru.weight_hh_l0)
        add("bih", fe.gru.bias_ih_l0)
        add("bhh", fe.gru.bias_hh_l0)

        enc = m.factor_encoder
        add("Wenc", enc.linear.weight)
        add("benc", enc.linear.bias)
        add("Wmu_e", enc.linear_mu.weight)
        add("bmu_e", enc.linear_mu.bias)
        add("Wsig_e", enc.linear_sigma.weight)
        add("bsig_e", enc.linear_sigma.bias)

        dec = m.factor_decoder
        add("W1d", dec.alpha_layer.linear1.weight)
        add("b1d", dec.alpha_layer.linear1.bias)
        add("wmu_d", dec.alpha_layer.mu_layer.weight)
        add("bmu_d", dec.alpha_layer.mu_layer.bias)
        add("wsig_d", dec.alpha_layer.sigma_layer.weight)
        add("bsig_d", dec.alpha_layer.sigma_layer.bias)
        add("Wb", dec.beta_layer.linear1.weight)
        add("bb", dec.beta_layer.linear1.bias)

        pred = m.factor_predictor
        # stacked attention groups: heads consecutive -> contiguous (K,..)
        for i, layer in enumerate(pred.attention_layers):
            add(f"q_att.{i}", layer.query)
        for i, layer in enumerate(pred.attention_layers):
            add(f"Wk.{i}", layer.key_layer.weight)
        for i, layer in enumerate(pred.attention_layers):
            add(f"bk.{i}", layer.key_layer.bias)
        for i, layer in enumerate(pred.attention_layers):
            add(f"Wv.{i}", layer.value_layer.weight)
        for i, layer in enumerate(pred.attention_layers):
            add(f"bv.{i}", layer.value_layer.bias)

        add("Wl", pred.linear.weight)
        add("bl", pred.linear.bias)
        add("wmu_p", pred.mu_layer.weight)
        add("bmu_p", pred.mu_layer.bias)
        add("wsig_p", pred.sigma_layer.weight)
        add("bsig_p", pred.sigma_layer.bias)
        return specs

    def _build_param_arena(self):
        specs = self._param_specs()
        self.params = _Arena(self.device, [(n, s) for n, _, s in specs])
        for name, param, _ in specs:
            v = self.params.view(name)
            v.copy_(param.data)
            param.data = v
        # stacked cross-head views
        K, H = self.K, self.H
        off0, _ = self.params.offsets["q_att.0"]
        self.p_q = self.params.flat[off0:off0 + K * H].view(K, H)
        offW, _ = self.params.offsets["Wk.0"]
        self.p_Wk = self.params.flat[offW:offW + K * H * H].view(K, H, H)
        offb, _ = self.params.offsets["bk.0"]
        self.p_bk = self.params.flat[offb:offb + K * H].view(K, H)
        offV, _ = self.params.offsets["Wv.0"]
        self.p_Wv = self.params.flat[offV:offV + K * H * H].view(K, H, H)
        offvb, _ = self.params.offsets["bv.0"]
        self.p_bv = self.params.flat[offvb:offvb + K * H].view(K, H)

    def p(self, name):
        return self.params.view(name)

    def g(self, name):
        off, shape = self.params.offsets[name]
        n = 1
        for s in shape:
            n *= s
        return self.grads[off:off + n].view(*shape)

    def _gstack(self, base, shape):
        off, _ = self.params.offsets[base]
        n = 1
        for s in shape:
            n *= s
        return self.grads[off:off + n].view(*shape)

    # ------------------------------------------------------------ workspaces
    def _alloc_ws(self, N: int, T: int):
        d = self.device
        C, H, M, K = self.C, self.H, self.M, self.K
        R = N * T
        f = lambda *shape: torch.zeros(*shape, device=d, dtype=torch.float32)
        w = {}
        w["x"] = f(N, T, C)
        w["y"] = f(N, 1)
        w["xln"] = f(R, C)
        w["mean"] = f(R)
        w["rstd"] = f(R)
        w["xp"] = f(R, C)
        w["gi"] = f(R, 3 * H)
        w["h"] = f(N, H)
        w["h_prev"] = f(N, T, H)
        w["gates4"] = f(N, T, 4 * H)
        w["scores_enc"] = f(N, M)
        w["a_enc"] = f(N, M)
        w["yp"] = f(M)
        w["fmu"] = f(K)
        w["fsig_pre"] = f(K)
        w["fsig"] = f(K)
        w["fsig_c"] = f(K)
        w["qk"] = f(K, H)
        w["cb"] = f(K)
        w["s_att"] = f(N, K)
        w["mask"] = f(N, K)
        w["a_att"] = f(N, K)
        w["sd"] = f(N, K)
        w["guard"] = torch.zeros(K, device=d, dtype=torch.int32)
        w["enc_done"] = torch.zeros(1, device=d, dtype=torch.int32)
        w["u"] = f(K, H)
        w["ctx"] = f(K, H)
        w["hm2"] = f(K, H)
        w["pmu"] = f(K)
        w["psig_pre"] = f(K)
        w["psig"] = f(K)
        w["psig_c"] = f(K)
        w["a1"] = f(N, H)
        w["beta"] = f(N, K)
        w["asig_pre"] = f(N)
        w["sigma"] = f(N)
        w["eps"] = f(N)
        w["recon"] = f(N)
        w["loss"] = f(1)
        w["mse"] = f(1)
        w["kl"] = f(1)
        # backward
        w["drecon"] = f(N)
        w["dfmu"] = f(K)
        w["dfsig_c"] = f(K)
        w["dpmu"] = f(K)
        w["dpsig_c"] = f(K)
        w["dh"] = f(N, H)
        w["dz1"] = f(N, H)
        w["dbeta"] = f(N, K)
        w["dz2"] = f(K, H)
        w["dctx"] = f(K, H)
        w["du"] = f(K, H)
        w["da"] = f(N, K)
        w["ds"] = f(N, K)
        w["dc"] = f(K)
        w["dqk"] = f(K, H)
        w["dscores"] = f(N, M)
        w["dgi"] = f(R, 3 * H)
        w["dgh"] = f(R, 3 * H)
        if not self.bf16 and not self._f32_tail:
            w["dxp"] = f(R, C)
        max_mn = max(3 * H * max(H, C), C * C, M * H, K * max(H, M))
        w["tn_part"] = f(128 * max_mn)
        w["tn_part2"] = f(128 * max_mn)
        w["tn_part3"] = f(128 * max_mn)
        max_m = max(3 * H, C, M, K)
        w["tn_partb"] = f(128 * max_m)
        w["tn_partb2"] = f(128 * max_m)
        w["tn_partb3"] = f(128 * max_m)
        # N-row reductions (attention/encoder/decoder wgrads + fwd u):
        # chunked over z so a 3500-stock day doesn't serialize 6 blocks
        small_mn = 32 * max(M, K, H) * H
        w["tn_part_u"] = f(small_mn)
        w["tn_part_s"] = f(small_mn)
        w["tn_partb_s"] = f(32 * max_m)
        # attention-branch partials: that branch runs on its own stream
        # concurrently with the dec/enc wgrads that use tn_part_s
        w["tn_part_a"] = f(small_mn)
        # deterministic shared-grad partials (no float atomics anywhere)
        # (one block of slack beyond the decoder's own block count)
        w["dec_part"] = f((self.ext.dec_nblk(N) + 1) * (2 * K + 2 * H + 2))
        w["hpart"] = f(K * (2 * H + 2))
        w["dzx"] = f(R, C)
        if self._f32_tail != 2:
            # FV_F32_TAIL=2 never forms dxln (its LayerNorm gradients
            # come out of ln_w1x_finish)
            w["ln_part"] = f((self.ext.ln_bwd_yblocks(R, C) + 1) * 2 * C)
            w["dxln"] = f(R, C)
        if self.bf16:
            fb = lambda *shape: torch.zeros(*shape, device=d,
                                            dtype=torch.bfloat16)
            # A-side operands of the register-stationary NT kernel get
            # 8 elements of tail slack (its k-tail b128 fragment may
            # read up to 4 bytes past the last row; the zero-padded
            # weight makes the contribution exact)
            fbs = lambda r, c: torch.zeros(r * c + 8, device=d,
                                           dtype=torch.bfloat16
                                           )[:r * c].view(r, c)
            w["xln_bf"] = fbs(R, C)
            w["xp_bf"] = fbs(R, C)
            w["dgi_bf"] = fbs(R, 3 * H)
            w["dzx_bf"] = fbs(R, C)
            if self._whh_fused:
                # the in-GRU Whh wgrad replaces the dgh_bf operand image
                # + h_prev cast with per-block partials
                nblk = self.ext.gru_wgrad_blocks(N)
                w["whh_part"] = f(nblk * 3 * H * H)
                w["bhh_part"] = f(nblk * 3 * H)
            else:
                w["h_prev_bf"] = fb(R, H)
                w["dgh_bf"] = fb(R, 3 * H)
            if self.fp8:
                ldp = self.w1x_f8.size(1)
                f8t = lambda *shape: torch.zeros(
                    *shape, device=d, dtype=torch.float8_e4m3fn)
                w["xln_f8"] = f8t(R, ldp)
                w["xp_f8"] = f8t(R, ldp)
                if self._fp8_rs:
                    w["dgi_f8"] = f8t(R, self.wihT_f8.size(1))
                    w["dzx_f8"] = f8t(R, self.w1xT_f8.size(1))
        self._ws_cache[(N, T)] = w
        self.ws = w
        self._ws_n = N
        self._ws_t = T

    def _main_ctx(self):
        """Context manager entering the high-priority main stream (or a
        no-op when unavailable/disabled)."""
        if self.s_main is not None:
            return torch.cuda.stream(self.s_main)
        import contextlib
        return contextlib.nullcontext()

    def _main_entry(self):
        """Order s_main after work the caller enqueued on its stream
        (input tensors)."""
        if self.s_main is not None:
            self.s_main.wait_stream(torch.cuda.current_stream(self.device))

    def _main_exit(self):
        """Order the caller's stream after the step's s_main work (the
        caller reads the device loss/scores)."""
        if self.s_main is not None:
            torch.cuda.current_stream(self.device).wait_stream(self.s_main)

    # ------------------------------------------------------ stream helpers
    def _streams(self):
        return (self.s_side, self.s_side2)

    def _fork(self, si: int = 0):
        """Make side stream si wait for everything issued on main."""
        sides = self._streams()
        if sides[si] is None:
            return
        e = torch.cuda.Event()
        e.record(torch.cuda.current_stream(self.device))
        sides[si].wait_event(e)

    def _join(self, si: int = 0):
        """Make main wait for everything issued on side stream si."""
        sides = self._streams()
        if sides[si] is None:
            return
        e = torch.cuda.Event()
        e.record(sides[si])
        torch.cuda.current_stream(self.device).wait_event(e)

    class _OnSide:
        """Context manager: run enqueues on a side stream (no-op when the
        stream is unavailable, e.g. CPU)."""

        def __init__(self, trainer, si: int = 0):
            self.stream = trainer._streams()[si]

        def __enter__(self):
            if self.stream is not None:
                self.ctx = torch.cuda.stream(self.stream)
                self.ctx.__enter__()
            return self

        def __exit__(self, *a):
            if self.stream is not None:
                self.ctx.__exit__(*a)
            return False

    # ------------------------------------------------------------ the step
    def _launch_forward(self, N: int, T: int, with_loss: bool = True,
                        x=None, y=None, train: bool = False):
        """Forward pass. train=True promises that _launch_backward follows:
        where the middle chain applies, the forward then ends behind
        enc_fused_fwd, and the decoder forward and the loss are launched
        by _launch_backward as part of that chain."""
        ext, w, p = self.ext, self.ws, self.p
        C, H, M, K = self.C, self.H, self.M, self.K
        R = N * T
        x2d = (w["x"] if x is None else x).view(R, C)
        yv = w["y"] if y is None else y
        alpha = 1.0 / math.sqrt(float(H) + 1e-6)

        # the K-head query/key projection depends only on parameters:
        # issue it on the side stream overlapped with the extractor
        self._fork(0)
        fuse = (train and with_loss and self._mid_fuse and N <= 384)
        e_qk = None
        with self._OnSide(self, 0):
            if self._rng_pending:
                # FV_RNG_SIDE: main waits for e_qk below before anything
                # reads eps or mask
                self._rng_pending = False
                self._fill_rng(N)
            ext.attn_qk_fwd(self.p_q, self.p_Wk, self.p_bk, w["qk"], w["cb"])
            if fuse:
                e_qk = torch.cuda.Event()
                e_qk.record(torch.cuda.current_stream(self.device))

        if self.fp8:
            # fwd in e4m3 (weights+activations); also emits the bf16
            # activation copies the bf16 backward consumes
            ext.ln_fwd(x2d, p("ln_g"), p("ln_b"), None, w["mean"],
                       w["rstd"], 1e-5, w["xln_bf"], w["xln_f8"])
            if self._fp8_rs:
                # MX-scaled K=128 MFMA (double the K=32 form's rate)
                ext.gemm_nt_fp8_rs(w["xln_f8"], self.w1x_f8, p("b1x"),
                                   self.is_w1x, None, w["xp_bf"],
                                   w["xp_f8"], R, self.C, self.C, 1.0, True)
                ext.gemm_nt_fp8_rs(w["xp_f8"], self.wih_f8, p("bih"),
                                   self.is_wih, w["gi"].view(R, 3 * H),
                                   None, None, R, self.C, 3 * H, 1.0, False)
            else:
                ext.gemm_nt_fp8(w["xln_f8"], self.w1x_f8, p("b1x"),
                                self.is_w1x, None, w["xp_bf"], w["xp_f8"],
                                R, self.C, self.C, 1.0, True)
                ext.gemm_nt_fp8(w["xp_f8"], self.wih_f8, p("bih"),
                                self.is_wih, w["gi"].view(R, 3 * H), None,
                                None, R, self.C, 3 * H, 1.0, False)
        elif self.bf16:
            ext.ln_fwd(x2d, p("ln_g"), p("ln_b"), None, w["mean"],
                       w["rstd"], 1e-5, w["xln_bf"])
            ext.gemm_nt_bf16_rs(w["xln_bf"], self.w1x_p, p("b1x"), None,
                                w["xp_bf"], None, 1.0, True)
            ext.gemm_nt_bf16_rs(w["xp_bf"], self.wih_p, p("bih"), w["gi"],
                                None, None, 1.0, False)
        else:
            # one launch for LayerNorm + both projections; FV_F32_TAIL=2
            # never reads xln (its tail uses x, mean, rstd), so that R x C
            # store is skipped. An unsupported shape launches nothing and
            # returns False: the three kernels below run instead.
            if not (self._f32_head and ext.extractor_head_fwd(
                    x2d, p("ln_g"), p("ln_b"), p("W1x"), p("b1x"), p("Wih"),
                    p("bih"), None if self._f32_tail == 2 else w["xln"],
                    w["mean"], w["rstd"], w["xp"], w["gi"], 1e-5)):
                ext.ln_fwd(x2d, p("ln_g"), p("ln_b"), w["xln"],
                           w["mean"], w["rstd"], 1e-5)
                ext.gemm_nt(w["xln"], p("W1x"), p("b1x"), w["xp"], 1.0, False,
                            True)
                ext.gemm_nt(w["xp"], p("Wih"), p("bih"), w["gi"], 1.0, False,
                            False)
        if self.bf16 and H == 64:
            # h_seq is a dead output in the engine (backward consumes
            # h_prev + gates4); skip its (N,T,H) write entirely
            ext.gru_fwd_mfma(w["gi"], self.whh_bf, p("bhh"), w["h"],
                             None, w["h_prev"], w["gates4"], N, T, H)
        else:
            ext.gru_fwd(w["gi"], p("Whh"), p("bhh"), w["h"], None,
                        w["h_prev"], w["gates4"], N, T, H,
                        variant=self._gru_v)
        if self.bf16 and not self._whh_fused:
            # h_prev bf16 image (Whh TN wgrad operand) on side stream 2
            if self.s_side2 is not None:
                e_ = torch.cuda.Event()
                e_.record(torch.cuda.current_stream(self.device))
                self.s_side2.wait_event(e_)
                with torch.cuda.stream(self.s_side2):
                    ext.cast_f32_bf16(w["h_prev"].view(-1),
                                      w["h_prev_bf"].view(-1))
            else:
                ext.cast_f32_bf16(w["h_prev"].view(-1),
                                  w["h_prev_bf"].view(-1))
        # h is ready: the K-head attention branch (prior path) runs on the
        # side stream, overlapped with the encoder + decoder branches on
        # main — they are independent until the loss joins pmu/psig with
        # the posterior-decoded recon
        mask = w["mask"] if self.training else None
        keep_inv = 1.0 / (1.0 - self.DROPOUT_P)
        if fuse:
            # the fused middle: both forwards in ONE launch on main, as
            # gru_fwd's first successor; qk / cb come from side stream 0.
            # An unsupported shape launches nothing and returns False: the
            # two kernels below run instead.
            torch.cuda.current_stream(self.device).wait_event(e_qk)
            if ext.mid_fwd(w["h"], w["qk"], w["cb"], mask, self.p_Wv,
                           self.p_bv, p("Wl"), p("bl"), p("wmu_p"),
                           p("bmu_p"), p("wsig_p"), p("bsig_p"), w["a_att"],
                           w["sd"], w["guard"], w["u"], w["ctx"], w["hm2"],
                           w["pmu"], w["psig_pre"], w["psig"], w["psig_c"],
                           p("Wenc"), p("benc"), yv, w["scores_enc"],
                           w["a_enc"], w["yp"], p("Wmu_e"), p("bmu_e"),
                           p("Wsig_e"), p("bsig_e"), w["fmu"], w["fsig_pre"],
                           w["fsig"], w["fsig_c"], w["enc_done"], alpha,
                           keep_inv):
                self._chain_pending = True
                self._fuse_pending = True
                return
        self._fork(0)
        with self._OnSide(self, 0):
            if N <= 448:
                # whole per-head chain in ONE kernel (h staged in LDS)
                ext.attn_fused_fwd(w["h"], w["qk"], w["cb"], mask, self.p_Wv,
                                   self.p_bv, p("Wl"), p("bl"), p("wmu_p"),
                                   p("bmu_p"), p("wsig_p"), p("bsig_p"),
                                   w["a_att"], w["sd"], w["guard"], w["u"],
                                   w["ctx"], w["hm2"], w["pmu"],
                                   w["psig_pre"], w["psig"], w["psig_c"],
                                   alpha, keep_inv, self._mid)
            else:
                ext.gemm_nt(w["h"], w["qk"], w["cb"], w["s_att"], alpha,
                            False, False)
                ext.attn_softmax_fwd(w["s_att"], mask, w["a_att"], w["sd"],
                                     w["guard"], keep_inv)
                ext.gemm_tn(w["a_att"], w["h"], w["u"], w["tn_part_u"], 2,
                            False, variant=self._gv)
                ext.attn_ctx_fwd(w["u"], self.p_Wv, self.p_bv, w["guard"],
                                 w["ctx"])
                ext.pred_mlp_fwd(w["ctx"], p("Wl"), p("bl"), p("wmu_p"),
                                 p("bmu_p"), p("wsig_p"), p("bsig_p"),
                                 w["hm2"], w["pmu"], w["psig_pre"], w["psig"],
                                 w["psig_c"])
        if N <= 448:
            # the mu/sigma heads ride the portfolio kernel (its last
            # workgroup computes them after an agent-scope yp handoff)
            ext.enc_fused_fwd(w["h"], p("Wenc"), p("benc"), yv,
                              w["scores_enc"], w["a_enc"], w["yp"],
                              p("Wmu_e"), p("bmu_e"), p("Wsig_e"),
                              p("bsig_e"), w["fmu"], w["fsig_pre"],
                              w["fsig"], w["fsig_c"], w["enc_done"],
                              self._mid)
            if train and with_loss and self._mid_chain and N <= 384:
                self._chain_pending = True
                return
        else:
            ext.gemm_nt(w["h"], p("Wenc"), p("benc"), w["scores_enc"], 1.0,
                        False, False)
            ext.enc_softmax_fwd(w["scores_enc"], yv, w["a_enc"], w["yp"])
            ext.enc_heads_fwd(w["yp"], p("Wmu_e"), p("bmu_e"), p("Wsig_e"),
                              p("bsig_e"), w["fmu"], w["fsig_pre"],
                              w["fsig"], w["fsig_c"])
        ext.dec_fwd(w["h"], p("W1d"), p("b1d"), p("wmu_d"), p("bmu_d"),
                    p("wsig_d"), p("bsig_d"), p("Wb"), p("bb"), w["fmu"],
                    w["fsig_c"], w["eps"], w["recon"], w["a1"], w["beta"],
                    w["asig_pre"], w["sigma"])
        self._join(0)
        if self.bf16:
            # the h_prev bf16 cast was forked onto side stream 2: it must
            # join before a forward-only hipGraph capture ends (an
            # unjoined captured branch invalidates the capture; in the
            # training step the backward's joins covered it)
            self._join(1)
        if with_loss:
            # one kernel: loss scalars AND the five loss input-gradients
            # (the gradient writes cost nothing extra; validation simply
            # ignores them)
            ext.loss_fused(w["recon"], yv, w["fmu"], w["fsig_c"], w["pmu"],
                           w["psig_c"], w["loss"], w["mse"], w["kl"],
                           w["drecon"], w["dfmu"], w["dfsig_c"], w["dpmu"],
                           w["dpsig_c"], 1.0)

    def _launch_backward(self, N: int, T: int, x=None, y=None,
                         comm_overlap: bool = False):
        """Backward pass. Three independent gradient branches run
        concurrently: the decoder+encoder chain on the main stream, the
        K-head attention backward on side stream 2, and every
        weight-gradient GEMM / colsum forked onto side stream 1 as soon
        as its producer is done (fork/join events become hipGraph edges
        under capture). The loss input-gradients were already produced
        by forward's loss_fused kernel; the three dh contributions are
        assembled by ONE dh_combine kernel at the join."""
        ext, w, p, g = self.ext, self.ws, self.p, self.g
        C, H, M, K = self.C, self.H, self.M, self.K
        R = N * T
        x2d = (w["x"] if x is None else x).view(R, C)
        yv = w["y"] if y is None else y
        alpha = 1.0 / math.sqrt(float(H) + 1e-6)
        keep_inv = 1.0 / (1.0 - self.DROPOUT_P)
        chunks = (int(os.environ.get("FV_TN_CHUNKS", "0"))
                  or max(1, min(32, R // 1024)))

        main = torch.cuda.current_stream(self.device) if self.s_side else None
        fork, _on_side = self._fork, self._OnSide
        sides = self._streams()

        # ---- attention backward branch (side stream 2): independent of
        # the decoder/encoder chain given the loss grads from forward
        mask = w["mask"] if self.training else None
        gWv = self._gstack("Wv.0", (K, H, H))
        gbv = self._gstack("bv.0", (K, H))
        gq = self._gstack("q_att.0", (K, H))
        gWk = self._gstack("Wk.0", (K, H, H))
        gbk = self._gstack("bk.0", (K, H))
        chain, self._chain_pending = self._chain_pending, False
        fused, self._fuse_pending = self._fuse_pending, False
        if fused and self._launch_mid_fused(
                N, yv, mask, alpha, keep_inv, (gWv, gbv, gq, gWk, gbk)):
            # everything dh needs is on main. In fp32 the three dh terms
            # are added by gru_bwd itself (its binding says whether that
            # route exists for this shape); bf16 / fp8 keep dh_combine.
            combine = not self.bf16
            if not combine:
                self._dh_combine()
            e_encb = torch.cuda.Event()
            e_encb.record(main)

            def wenc_wgrad():
                # needed by Adam only; waits for enc_bwd_mid's dscores
                s0 = sides[0]
                s0.wait_event(e_encb)
                with torch.cuda.stream(s0):
                    ext.gemm_tn(w["dscores"], w["h"], g("Wenc"),
                                w["tn_part_s"], 2, False, g("benc"),
                                w["tn_partb_s"], variant=self._gv)

            if comm_overlap:
                # the reduce below takes Wenc's gradient too
                wenc_wgrad()
                wenc_wgrad = None
            self._comm_overlap_point(main, sides, comm_overlap)
            # otherwise gru_bwd is enqueued first, as enc_bwd_mid's first
            # successor, and the Wenc weight gradient behind it
            self._launch_extractor_bwd(N, T, x2d, chunks, main, sides,
                                       comm_overlap, combine=combine,
                                       after_gru=wenc_wgrad,
                                       ts=1 if self.bf16 else 0)
            return
        if chain:
            # dh_combine waits for the attention kernel only; the final
            # join before Adam covers what follows it on that stream
            main.wait_event(self._launch_mid_chain(
                N, yv, mask, alpha, keep_inv, (gWv, gbv, gq, gWk, gbk)))
        else:
            self._launch_mid_old(N, yv, mask, alpha, keep_inv,
                                 (gWv, gbv, gq, gWk, gbk))
            self._join(1)
        # ---- attention branch joined; assemble all three dh contributions
        # (attention ds@qk + a@du, encoder dscores@Wenc) in ONE kernel
        self._dh_combine()
        self._comm_overlap_point(main, sides, comm_overlap)
        self._launch_extractor_bwd(N, T, x2d, chunks, main, sides,
                                   comm_overlap)

    def _dh_combine(self):
        ext, w = self.ext, self.ws
        ext.dh_combine(w["dh"], w["ds"], w["qk"], w["a_att"], w["du"],
                       w["dscores"], self.p("Wenc"))

    def _comm_overlap_point(self, main, sides, comm_overlap):
        if comm_overlap:
            # every non-extractor gradient (arena tail from Wenc on) is
            # final: reduce it now, overlapped with the extractor bwd
            e1 = torch.cuda.Event()
            e1.record(main)
            self.s_comm.wait_event(e1)
            for sstream in sides:
                # the wgrads of the middle run on side 0, and with the
                # middle chain the attention branch does too
                if sstream is not None:
                    e2 = torch.cuda.Event()
                    e2.record(sstream)
                    self.s_comm.wait_event(e2)
            with torch.cuda.stream(self.s_comm):
                tail = self.grads[self.params.offsets["Wenc"][0]:]
                tail.div_(get_world_size())
                torch.distributed.all_reduce(tail)

    def _launch_mid_fused(self, N, yv, mask, alpha, keep_inv, gatt):
        """The fused middle (docs/KERNELS.md): _launch_forward ended behind
        mid_fwd on main. mid_bwd (attention backward + dec_fwd_bwd, one
        launch) and enc_bwd_mid follow there, each its predecessor's
        first-enqueued successor. What only Adam or the caller needs is
        forked behind mid_bwd onto side stream 0 and enqueued after
        enc_bwd_mid: two concurrent branches, and nothing main waits for.
        Returns False, having launched nothing, if mid_bwd refuses the
        shape; _launch_mid_chain then runs behind mid_fwd."""
        ext, w, p, g = self.ext, self.ws, self.p, self.g
        gWv, gbv, gq, gWk, gbk = gatt
        main = torch.cuda.current_stream(self.device)
        s0 = self._streams()[0]
        if not ext.mid_bwd(
                w["psig"], w["psig_pre"], w["hm2"], p("wmu_p"), p("wsig_p"),
                p("Wl"), w["h"], w["a_att"], w["sd"], mask, w["guard"],
                w["u"], self.p_Wv, self.p_q, self.p_Wk, self.p_bk, w["dz2"],
                w["du"], w["ds"], w["dc"], gWv, gbv, gq, gWk, gbk,
                w["hpart"], w["fmu"], w["fsig_c"], w["pmu"], w["psig_c"],
                w["dpmu"], w["dpsig_c"], p("W1d"), p("b1d"), p("wmu_d"),
                p("bmu_d"), p("wsig_d"), p("bsig_d"), p("Wb"), p("bb"),
                w["eps"], yv, w["recon"], w["a1"], w["beta"],
                w["asig_pre"], w["sigma"], w["drecon"], w["dh"], w["dz1"],
                w["dbeta"], w["dec_part"], alpha, keep_inv, 1.0):
            return False
        e_mb = torch.cuda.Event()
        e_mb.record(main)
        ext.enc_bwd_mid(w["dec_part"], ext.dec_nblk(N), w["fmu"],
                        w["fsig_c"], w["pmu"],
                        w["psig_c"], w["fsig"], w["fsig_pre"], w["yp"],
                        p("Wmu_e"), p("Wsig_e"), w["a_enc"], yv,
                        w["dscores"], g("Wmu_e"), g("bmu_e"), g("Wsig_e"),
                        g("bsig_e"), w["dfmu"], w["dfsig_c"], 1.0)
        s0.wait_event(e_mb)
        with torch.cuda.stream(s0):
            ext.pred_head_reduce(w["hpart"], g("wmu_p"), g("bmu_p"),
                                 g("wsig_p"), g("bsig_p"), self.K, self.H)
            ext.gemm_tn(w["dz2"], w["ctx"], g("Wl"), None, 1, False, g("bl"),
                        variant=self._gv)
            ext.dec_bwd_reduce_heads(w["dec_part"], g("wmu_d"), g("bmu_d"),
                                     g("wsig_d"), g("bsig_d"), N, self.K)
            ext.gemm_tn(w["dz1"], w["h"], g("W1d"), w["tn_part_s"], 2, False,
                        g("b1d"), w["tn_partb_s"], variant=self._gv)
            ext.gemm_tn(w["dbeta"], w["h"], g("Wb"), w["tn_part_s"], 2, False,
                        g("bb"), w["tn_partb_s"], variant=self._gv)
            ext.loss_scalars(w["recon"], yv, w["fmu"], w["fsig_c"], w["pmu"],
                             w["psig_c"], w["loss"], w["mse"], w["kl"])
        return True

    def _launch_mid_chain(self, N, yv, mask, alpha, keep_inv, gatt):
        """The middle of the training step as two critical-path nodes,
        dec_fwd_bwd -> enc_bwd_mid (docs/KERNELS.md). _launch_forward
        ended behind enc_fused_fwd. The loss gradients are formed where
        they are used. The attention backward runs behind its forward on
        side stream 0, followed there by what only Adam or the caller
        needs: the decoder head-gradient reduce, the weight gradients and
        the loss scalars. Returns the event dh_combine has to wait for."""
        ext, w, p, g = self.ext, self.ws, self.p, self.g
        gWv, gbv, gq, gWk, gbk = gatt
        main = torch.cuda.current_stream(self.device)
        s_att = self._streams()[0]
        # fmu / fsig_c are ready (enc_fused_fwd) ...
        e_enc = torch.cuda.Event()
        e_enc.record(main)
        # ... and pmu / psig_c behind attn_fused_fwd
        e_att = torch.cuda.Event()
        e_att.record(s_att)
        # the critical-path successor of enc_fused_fwd is enqueued first:
        # it keeps the hardware queue (profiles/f32_tail.md)
        ext.dec_fwd_bwd(w["h"], p("W1d"), p("b1d"), p("wmu_d"), p("bmu_d"),
                        p("wsig_d"), p("bsig_d"), p("Wb"), p("bb"), w["fmu"],
                        w["fsig_c"], w["eps"], yv, w["recon"], w["a1"],
                        w["beta"], w["asig_pre"], w["sigma"], w["drecon"],
                        w["dh"], w["dz1"], w["dbeta"], w["dec_part"], 1.0)
        # attention backward: its forward's same-stream successor; head k
        # forms dpmu / dpsig_c itself
        s_att.wait_event(e_enc)
        with torch.cuda.stream(s_att):
            ext.attn_fused_bwd(w["dpmu"], w["dpsig_c"], w["psig"],
                               w["psig_pre"], w["hm2"], p("wmu_p"),
                               p("wsig_p"), p("Wl"), w["h"], w["a_att"],
                               w["sd"], mask, w["guard"], w["u"],
                               self.p_Wv, self.p_q, self.p_Wk, self.p_bk,
                               w["dz2"], w["du"], w["ds"], w["dc"], gWv,
                               gbv, gq, gWk, gbk, w["hpart"], g("wmu_p"),
                               g("bmu_p"), g("wsig_p"), g("bsig_p"),
                               alpha, keep_inv, self._mid, w["fmu"],
                               w["fsig_c"], w["pmu"], w["psig_c"], 1.0)
            e_join = torch.cuda.Event()
            e_join.record(s_att)
            ext.gemm_tn(w["dz2"], w["ctx"], g("Wl"), None, 1, False, g("bl"),
                        variant=self._gv)
        # encoder backward, again enqueued before the side work: every
        # workgroup sums the decoder's factor partials and adds the KL
        # gradients itself
        main.wait_event(e_att)
        ext.enc_bwd_mid(w["dec_part"], ext.dec_nblk(N), w["fmu"],
                        w["fsig_c"], w["pmu"],
                        w["psig_c"], w["fsig"], w["fsig_pre"], w["yp"],
                        p("Wmu_e"), p("Wsig_e"), w["a_enc"], yv,
                        w["dscores"], g("Wmu_e"), g("bmu_e"), g("Wsig_e"),
                        g("bsig_e"), w["dfmu"], w["dfsig_c"], 1.0)
        e_encb = torch.cuda.Event()
        e_encb.record(main)
        # off the critical path, needed by Adam / the caller only: behind
        # the attention branch on its stream, so the middle of the step
        # stays at two concurrent branches. As a third branch this work
        # shared a hardware queue with attn_fused_bwd and ran in front of
        # it (profiles/mid_chain.md).
        s_att.wait_event(e_encb)
        with torch.cuda.stream(s_att):
            ext.dec_bwd_reduce_heads(w["dec_part"], g("wmu_d"), g("bmu_d"),
                                     g("wsig_d"), g("bsig_d"), N, self.K)
            ext.gemm_tn(w["dz1"], w["h"], g("W1d"), w["tn_part_s"], 2, False,
                        g("b1d"), w["tn_partb_s"], variant=self._gv)
            ext.gemm_tn(w["dbeta"], w["h"], g("Wb"), w["tn_part_s"], 2, False,
                        g("bb"), w["tn_partb_s"], variant=self._gv)
            ext.loss_scalars(w["recon"], yv, w["fmu"], w["fsig_c"], w["pmu"],
                             w["psig_c"], w["loss"], w["mse"], w["kl"])
            ext.gemm_tn(w["dscores"], w["h"], g("Wenc"), w["tn_part_s"], 2,
                        False, g("benc"), w["tn_partb_s"], variant=self._gv)
        return e_join

    def _launch_mid_old(self, N, yv, mask, alpha, keep_inv, gatt):
        """The middle of the backward as separate kernels (FV_MID_CHAIN=0,
        N > 384, or a forward that already ran dec_fwd and loss_fused)."""
        ext, w, p, g = self.ext, self.ws, self.p, self.g
        gWv, gbv, gq, gWk, gbk = gatt
        fork, _on_side = self._fork, self._OnSide
        fork(1)
        with _on_side(self, 1):
            if N <= 384:
                # whole per-head backward chain in ONE kernel (incl. the
                # query/key/value wgrads)
                ext.attn_fused_bwd(w["dpmu"], w["dpsig_c"], w["psig"],
                                   w["psig_pre"], w["hm2"], p("wmu_p"),
                                   p("wsig_p"), p("Wl"), w["h"], w["a_att"],
                                   w["sd"], mask, w["guard"], w["u"],
                                   self.p_Wv, self.p_q, self.p_Wk, self.p_bk,
                                   w["dz2"], w["du"], w["ds"], w["dc"], gWv,
                                   gbv, gq, gWk, gbk, w["hpart"], g("wmu_p"),
                                   g("bmu_p"), g("wsig_p"), g("bsig_p"),
                                   alpha, keep_inv, self._mid)
            else:
                ext.pred_mlp_bwd(w["dpmu"], w["dpsig_c"], w["psig"],
                                 w["psig_pre"], w["hm2"], p("wmu_p"),
                                 p("wsig_p"), w["dz2"], w["hpart"],
                                 g("wmu_p"), g("bmu_p"), g("wsig_p"),
                                 g("bsig_p"))
                ext.gemm_nn(w["dz2"], p("Wl"), None, w["dctx"], 1.0, False,
                            False, variant=self._gv)
                ext.attn_head_bwd(w["dctx"], w["u"], self.p_Wv, w["guard"],
                                  w["du"], gWv, gbv)
                ext.gemm_nt(w["h"], w["du"], None, w["da"], 1.0, False,
                            False)
                ext.attn_softmax_bwd(w["da"], w["a_att"], w["sd"], mask,
                                     w["guard"], w["ds"], w["dc"], keep_inv,
                                     alpha)
                ext.gemm_tn(w["ds"], w["h"], w["dqk"], w["tn_part_a"], 2,
                            False, variant=self._gv)
                ext.attn_qk_bwd(w["dqk"], w["dc"], self.p_q, self.p_Wk,
                                self.p_bk, gq, gWk, gbk)
            # cross-head Wl wgrad (dz2 is final in both branches)
            ext.gemm_tn(w["dz2"], w["ctx"], g("Wl"), None, 1, False, g("bl"),
                        variant=self._gv)

        # ---- decoder backward (main)
        ext.dec_bwd(w["drecon"], w["h"], w["a1"], w["beta"], w["asig_pre"],
                    w["sigma"], w["eps"], w["fmu"], w["fsig_c"], p("W1d"),
                    p("wmu_d"), p("wsig_d"), p("Wb"), w["dh"], w["dz1"],
                    w["dbeta"], w["dec_part"], w["dfmu"], w["dfsig_c"],
                    g("wmu_d"), g("bmu_d"), g("wsig_d"), g("bsig_d"))
        fork()
        with _on_side(self):
            ext.gemm_tn(w["dz1"], w["h"], g("W1d"), w["tn_part_s"], 2, False,
                        g("b1d"), w["tn_partb_s"], variant=self._gv)
            ext.gemm_tn(w["dbeta"], w["h"], g("Wb"), w["tn_part_s"], 2, False,
                        g("bb"), w["tn_partb_s"], variant=self._gv)

        # ---- encoder backward (heads + stock-axis softmax bwd, main)
        ext.enc_bwd_fused(w["dfmu"], w["dfsig_c"], w["fsig"], w["fsig_pre"],
                          w["yp"], p("Wmu_e"), p("Wsig_e"), w["a_enc"], yv,
                          w["dscores"], g("Wmu_e"), g("bmu_e"), g("Wsig_e"),
                          g("bsig_e"))
        fork()
        with _on_side(self):
            ext.gemm_tn(w["dscores"], w["h"], g("Wenc"), w["tn_part_s"], 2,
                        False, g("benc"), w["tn_partb_s"], variant=self._gv)

    def _launch_extractor_bwd(self, N, T, x2d, chunks, main, sides,
                              comm_overlap, combine=False, after_gru=None,
                              ts=1):
        """GRU + projections + LayerNorm backward, and the final join.
        combine (fp32): w["dh"] is the decoder's, and gru_bwd is asked to
        add dh_combine's three terms itself. after_gru: enqueues side work
        that must not be gru_bwd's predecessor's first successor. ts: the
        side stream of the weight gradients. In fp32 the fused middle
        passes 0, the stream its own Adam-only work is on: as a branch of
        its own next to side stream 1 that work shared a hardware queue
        with the tail's weight gradients and ran behind them, in front of
        Adam, and the step was 9 % slower than the parent. In bf16 the same
        move measured slower, so bf16 / fp8 keep 1 (profiles/mid_fuse.md)."""
        ext, w, p, g = self.ext, self.ws, self.p, self.g
        H, R = self.H, N * T
        fork, _on_side = self._fork, self._OnSide
        fp8_rs = self.fp8 and getattr(self, "_fp8_rs", False)
        fp8_gru_fused = fp8_rs and H == 64
        if fp8_rs:
            # turn last step's collected amaxes into this step's operand
            # scales (and reset); must precede the producers below
            ext.scale_from_amax2(self.amax_dgi, self.s_dgi, self.is_dgi,
                                 self.amax_dzx, self.s_dzx, self.is_dzx)
        if self.bf16 and H == 64:
            # fp32 dgi/dgh images are dead in bf16 mode (the wgrads use
            # the bf16 copies); in fp8 mode the kernel also emits the
            # scaled e4m3 dgrad operand directly from registers; with
            # _whh_fused the Whh/bhh wgrad partials come out of the same
            # kernel (no dgh_bf image, no standalone TN call)
            ext.gru_bwd_mfma(w["dh"], w["h_prev"], w["gates4"], self.whh_bf,
                             None, None, N, T, H,
                             w["dgi_bf"].view(N, T, 3 * H),
                             (None if self._whh_fused
                              else w["dgh_bf"].view(N, T, 3 * H)),
                             dgi_f8=w["dgi_f8"] if fp8_gru_fused else None,
                             s_dgi=self.s_dgi if fp8_gru_fused else None,
                             amax_dgi=(self.amax_dgi if fp8_gru_fused
                                       else None),
                             whh_part=(w["whh_part"] if self._whh_fused
                                       else None),
                             bhh_part=(w["bhh_part"] if self._whh_fused
                                       else None))
        elif self.bf16:
            ext.gru_bwd(w["dh"], w["h_prev"], w["gates4"], p("Whh"),
                        w["dgi"], w["dgh"], N, T, H,
                        w["dgi_bf"].view(N, T, 3 * H),
                        w["dgh_bf"].view(N, T, 3 * H))
        else:
            # with the operands gru_bwd either runs dh_combine as its
            # prologue or launches nothing and returns False
            self._combine_ran = bool(combine and ext.gru_bwd(
                w["dh"], w["h_prev"], w["gates4"], p("Whh"), w["dgi"],
                w["dgh"], N, T, H, variant=self._gru_v, ds=w["ds"],
                qk=w["qk"], a=w["a_att"], du=w["du"],
                dscores=w["dscores"], Wenc=p("Wenc")))
            if not self._combine_ran:
                if combine:
                    self._dh_combine()
                ext.gru_bwd(w["dh"], w["h_prev"], w["gates4"], p("Whh"),
                            w["dgi"], w["dgh"], N, T, H,
                            variant=self._gru_v)
        if after_gru is not None:
            after_gru()
        if self.bf16:
            # bf16 / fp8 always pass ts = 1: without the fused Whh weight
            # gradient, _launch_forward cast h_prev to h_prev_bf on that
            # stream, and the stream's order is what puts the cast in front
            # of its consumer below
            assert ts == 1
            fork(ts)
            with _on_side(self, ts):
                if self._whh_fused:
                    ext.wgrad_reduce(w["whh_part"], g("Whh"),
                                     w["bhh_part"], g("bhh"),
                                     ext.gru_wgrad_blocks(N), False)
                else:
                    ext.gemm_tn_bf16(w["dgh_bf"].view(R, 3 * H),
                                     w["h_prev_bf"], g("Whh"), w["tn_part"],
                                     chunks, False, g("bhh"),
                                     w["tn_partb"])
                ext.gemm_tn_bf16(w["dgi_bf"].view(R, 3 * H), w["xp_bf"],
                                 g("Wih"), w["tn_part2"], chunks, False,
                                 g("bih"), w["tn_partb2"])
            if fp8_rs:
                # fp8 dgrads on the MX K=128 path (delayed per-tensor
                # scaling; the bf16 dzx copy still feeds the W1x wgrad)
                if not fp8_gru_fused:
                    ext.cast_f32_fp8_damax(w["dgi"].view(R, 3 * H),
                                           w["dgi_f8"], self.s_dgi,
                                           self.amax_dgi)
                ext.gemm_nt_fp8_rs(w["dgi_f8"], self.wihT_f8, None,
                                   self.is_wih, None, w["dzx_bf"],
                                   w["dzx_f8"], R, 3 * H, self.C, 1.0,
                                   False, inv_sa=self.is_dgi,
                                   lrelu_bwd_of=w["xp_bf"],
                                   s_out=self.s_dzx,
                                   amax_out=self.amax_dzx)
            else:
                ext.gemm_nt_bf16_rs(w["dgi_bf"].view(R, 3 * H), self.wihT_p,
                                    None, None, w["dzx_bf"], w["xp_bf"],
                                    1.0, False)
            fork(ts)
            with _on_side(self, ts):
                ext.gemm_tn_bf16(w["dzx_bf"], w["xln_bf"], g("W1x"),
                                 w["tn_part3"], chunks, False, g("b1x"),
                                 w["tn_partb3"])
            if fp8_rs:
                ext.gemm_nt_fp8_rs(w["dzx_f8"], self.w1xT_f8, None,
                                   self.is_w1x, w["dxln"], None, None, R,
                                   self.C, self.C, 1.0, False,
                                   inv_sa=self.is_dzx)
            else:
                ext.gemm_nt_bf16_rs(w["dzx_bf"], self.w1xT_p, None,
                                    w["dxln"], None, None, 1.0, False)
        elif self._f32_tail:
            # shortened fp32 tail (docs/KERNELS.md): side 1 holds ONE
            # paired Whh/Wih wgrad launch + one reduce; main runs the
            # Wih dgrad with the LeakyReLU backward in its epilogue.
            # Main is the longer chain: its gemm_nn is enqueued BEFORE
            # the side-stream pair so that, as gru_bwd's first successor
            # in the captured graph, it stays on gru_bwd's hardware queue
            # (the successor that changes queue starts ~10 us late;
            # profiles/f32_tail.md)
            # FV_F32_GEMM (level 1 only): the pair and the W1x wgrad leave
            # their slices to ONE reduce at the end of side 1, and the dxln
            # GEMM forms ln_bwd_params' partials in its epilogue
            one_reduce = bool(self._gv) and self._f32_tail != 2
            fork(ts)
            ext.gemm_nn(w["dgi"].view(R, 3 * H), p("Wih"), None, w["dzx"],
                        1.0, False, False, lrelu_bwd_of=w["xp"],
                        variant=self._gv)
            with _on_side(self, ts):
                ext.gemm_tn_pair(w["dgh"].view(R, 3 * H),
                                 w["h_prev"].view(R, H), g("Whh"),
                                 w["dgi"].view(R, 3 * H), w["xp"], g("Wih"),
                                 w["tn_part"], w["tn_part2"], chunks, False,
                                 g("bhh"), g("bih"), w["tn_partb"],
                                 w["tn_partb2"],
                                 variant=self._gv, reduce=not one_reduce)
            if self._f32_tail == 2:
                # opt-in: W1x/LayerNorm gradients straight from
                # dzx^T @ xhat (no dxln GEMM, no ln_bwd_params pass);
                # equal to the default only up to fp32 rounding
                nz = ext.gemm_tn_xhat(w["dzx"], x2d, w["mean"], w["rstd"],
                                      w["tn_part3"], w["tn_partb3"],
                                      variant=self._gv)
                ext.ln_w1x_finish(w["tn_part3"], w["tn_partb3"], nz,
                                  p("W1x"), p("ln_g"), p("ln_b"), g("W1x"),
                                  g("b1x"), g("ln_g"), g("ln_b"))
            else:
                # bit-identical gradients: the W1x wgrad follows the pair
                # on side 1 (a third concurrent branch got serialized
                # BEHIND it on the same hardware queue: pair last, step
                # 4 % slower), the dxln GEMM and the LayerNorm parameter
                # gradients stay on main's queue
                fork(ts)
                ln_fused = bool(self._gv) and ext.gemm_nn_ln(
                    w["dzx"], p("W1x"), x2d, w["mean"], w["rstd"],
                    w["ln_part"])
                if not ln_fused:
                    # FV_F32_GEMM=0, or ln_bwd_params' row chunks are not
                    # the GEMM's 64-row tiles at this R
                    ext.gemm_nn(w["dzx"], p("W1x"), None, w["dxln"], 1.0,
                                False, False, variant=self._gv)
                with _on_side(self, ts):
                    ext.gemm_tn(w["dzx"], w["xln"], g("W1x"), w["tn_part3"],
                                chunks, False, g("b1x"), w["tn_partb3"],
                                variant=self._gv, reduce=not one_reduce)
                    if one_reduce:
                        ext.tn_reduce_list(
                            [g("Whh"), g("Wih"), g("W1x")],
                            [w["tn_part"], w["tn_part2"], w["tn_part3"]],
                            [g("bhh"), g("bih"), g("b1x")],
                            [w["tn_partb"], w["tn_partb2"], w["tn_partb3"]],
                            R, chunks, False)
                if ln_fused:
                    ext.ln_bwd_reduce(w["ln_part"], g("ln_g"), g("ln_b"), R,
                                      self.C)
                else:
                    ext.ln_bwd_params(x2d, w["dxln"], w["mean"], w["rstd"],
                                      w["ln_part"], g("ln_g"), g("ln_b"),
                                      chunks)
        else:
            fork(ts)
            with _on_side(self, ts):
                ext.gemm_tn(w["dgh"].view(R, 3 * H), w["h_prev"].view(R, H),
                            g("Whh"), w["tn_part"], chunks, False,
                            g("bhh"), w["tn_partb"], variant=self._gv)
                ext.gemm_tn(w["dgi"].view(R, 3 * H), w["xp"], g("Wih"),
                            w["tn_part2"], chunks, False, g("bih"),
                            w["tn_partb2"], variant=self._gv)
            ext.gemm_nn(w["dgi"].view(R, 3 * H), p("Wih"), None, w["dxp"], 1.0,
                        False, False, variant=self._gv)
            ext.lrelu_bwd(w["dxp"], w["xp"], w["dzx"])
            fork(ts)
            with _on_side(self, ts):
                ext.gemm_tn(w["dzx"], w["xln"], g("W1x"), w["tn_part3"], chunks,
                            False, g("b1x"), w["tn_partb3"], variant=self._gv)
            ext.gemm_nn(w["dzx"], p("W1x"), None, w["dxln"], 1.0, False, False,
                        variant=self._gv)
        if not self._f32_tail:
            fork()
            with _on_side(self):
                ext.ln_bwd_params(x2d, w["dxln"], w["mean"], w["rstd"],
                                  w["ln_part"], g("ln_g"), g("ln_b"), chunks)
        # join: main waits for all side-stream wgrad work (+ the early
        # comm slice, so the final slice reduce and adam are ordered)
        join_streams = list(sides)
        if comm_overlap:
            join_streams.append(self.s_comm)
        for sstream in join_streams:
            if sstream is not None:
                e = torch.cuda.Event()
                e.record(sstream)
                main.wait_event(e)

    def _refresh_bf16_shadows(self):
        self.ext.cast_shadows(self.p("W1x"), self.w1x_p, self.w1xT_p,
                              self.p("Wih"), self.wih_p, self.wihT_p,
                              self.p("Whh"), self.whh_bf)
        if self.fp8:
            self.ext.absmax_scale(self.p("W1x"), self.s_w1x, self.is_w1x)
            self.ext.cast_f32_fp8_scaled(self.p("W1x"), self.w1x_f8,
                                         self.s_w1x)
            self.ext.absmax_scale(self.p("Wih"), self.s_wih, self.is_wih)
            self.ext.cast_f32_fp8_scaled(self.p("Wih"), self.wih_f8,
                                         self.s_wih)
            if self._fp8_rs:
                self.ext.cast_f32_fp8_scaled_t(self.p("Wih"), self.wihT_f8,
                                               self.s_wih)
                self.ext.cast_f32_fp8_scaled_t(self.p("W1x"), self.w1xT_f8,
                                               self.s_w1x)

    def _launch_optimizer(self, inc: bool = True):
        if inc:
            self.ext.step_inc(self.step_t)
        self.ext.adam(self.params.flat, self.grads, self.adam_m, self.adam_v,
                      self.step_t, self.lr, self.eta_min, float(self.t_max),
                      0.9, 0.999, 1e-8)
        if self.bf16:
            self._refresh_bf16_shadows()

    def _fill_rng(self, N: int):
        self.ws["eps"].normal_()
        if self.training:
            self.ws["mask"].bernoulli_(1.0 - self.DROPOUT_P)

    # max distinct (N, T) shapes whose workspaces + captured graphs stay
    # resident; beyond this the least-recently-used shape is dropped
    # (long multi-year runs see hundreds of distinct daily stock counts)
    WS_CACHE_MAX = 256

    def _ensure_ws(self, N: int, T: int):
        """Workspaces (and captured graphs) are cached per (N, T): real
        universes have a different stock count N every day, and 288 GB
        HBM3E makes keeping one ~60 MB workspace per distinct shape far
        cheaper than re-capturing the step graph each day (256 shapes
        ≈ a few tens of GB, sized for MI355X HBM).

        Overflow policy is a synchronized FULL reset — drop every
        workspace and every captured graph at once, never individual
        shapes. Destroying single hipGraphExec objects while dozens of
        sibling graphs stay live was observed to corrupt later replays
        of the SURVIVORS on ROCm 7.2 (host segfault inside
        hipGraphLaunch) once the churn got big enough: a 96-shape
        ragged-universe run crashed in epoch 2 with per-shape LRU
        eviction (profiles/r2_final_validation.md), while an
        all-at-once rebuild from an empty runtime state is the pattern
        the small-cap eviction test and every fixed-shape run already
        exercise safely. The reset costs one recapture pass (~30 ms per
        shape) and fires only when a run exceeds WS_CACHE_MAX
        (`FV_WS_CACHE` overrides) distinct day shapes."""
        if self._ws_n == N and getattr(self, "_ws_t", None) == T:
            return
        lru = self.__dict__.setdefault("_ws_lru", [])
        if (N, T) in lru:
            lru.remove((N, T))
        lru.append((N, T))
        w = self._ws_cache.get((N, T))
        if w is not None:
            self.ws = w
            self._ws_n = N
            self._ws_t = T
        else:
            cap = int(os.environ.get("FV_WS_CACHE", "0")) or self.WS_CACHE_MAX
            if len(lru) > cap:
                if self.device.type == "cuda":
                    torch.cuda.synchronize(self.device)
                self._graphs.clear()
                self._ws_cache.clear()
                lru.clear()
                lru.append((N, T))
                if not getattr(self, "_ws_reset_warned", False):
                    self._ws_reset_warned = True
                    warnings.warn(
                        f"shape-cache overflow (> {cap} distinct (N, T) "
                        "day shapes): all workspaces/graphs reset and "
                        "rebuilt; raise FV_WS_CACHE to avoid recaptures")
            self._alloc_ws(N, T)

    # -------------------------------------------------- graph capability probe
    _caps = None

    class _abort_watchdog:
        """Fail-fast guard around hipGraph captures that include RCCL
        collectives at world_size > 1: a capture hang cannot be
        interrupted in-process, so if it exceeds FV_CAPTURE_WATCHDOG_S
        (default 180 s) the rank hard-exits — torchrun then fails the
        whole job quickly instead of a multi-GPU scaling run hanging
        until the outer driver's budget is gone. No-op at ws <= 1
        (ws=1 hardware smoke: comm capture verified OK on MI355X,
        profiles/r2_rccl_ws1.md)."""

        def __init__(self, tag: str):
            self.tag = tag

        def __enter__(self):
            import threading

            self.evt = threading.Event()
            self.armed = is_distributed() and get_world_size() > 1
            if not self.armed:
                return self
            limit = float(os.environ.get("FV_CAPTURE_WATCHDOG_S", "180"))

            def _wd():
                if not self.evt.wait(limit):
                    import sys as _sys
                    print(f"[fused] {self.tag} exceeded {limit:.0f}s — "
                          f"aborting rank (set FV_COMM_GRAPH=0 to force "
                          f"the split no-comm-capture plan)",
                          file=_sys.stderr, flush=True)
                    _os._exit(17)

            self.thr = threading.Thread(target=_wd, daemon=True)
            self.thr.start()
            return self

        def __exit__(self, *a):
            if self.armed:
                self.evt.set()
            return False

    def _probe_caps(self):
        """Can torch RNG ops / RCCL collectives be captured in a hipGraph?
        Probed once; capture plans adapt (fallbacks keep correctness).

        Env guard rails (hardware de-risk for multi-GPU runs):
        - FV_COMM_GRAPH=0 forces the split plan (never attempts to
          capture an RCCL collective into a hipGraph — the safe path if
          a ROCm build hangs at comm capture);
        - FV_RNG_GRAPH=0 keeps RNG fills outside the graph.
        """
        if self._caps is not None:
            return self._caps
        allow_comm = os.environ.get("FV_COMM_GRAPH", "1") != "0"
        allow_rng = os.environ.get("FV_RNG_GRAPH", "1") != "0"
        rng_ok = allow_rng
        if rng_ok:
            try:
                t_ = torch.zeros(8, device=self.device)
                torch.cuda.synchronize()
                gp = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gp):
                    t_.normal_()
                gp.replay()
                torch.cuda.synchronize()
            except Exception:
                rng_ok = False
                torch.cuda.synchronize()
        comm_ok = False
        if is_distributed() and allow_comm:
            try:
                with self._abort_watchdog("RCCL comm-capture probe"):
                    t_ = torch.ones(8, device=self.device)
                    torch.distributed.all_reduce(t_)  # eager warmup of the PG
                    torch.cuda.synchronize()
                    gp = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gp):
                        torch.distributed.all_reduce(t_)
                    gp.replay()
                    torch.cuda.synchronize()
                comm_ok = True
            except Exception:
                comm_ok = False
                torch.cuda.synchronize()
        self._caps = (rng_ok, comm_ok)
        return self._caps

    def _graph_step_body(self, x, y, N, T, rng_in_graph: bool,
                         comm_in_graph: bool, with_opt: bool = True):
        """The full training step as a capturable kernel sequence.
        No grads.zero_(): every gradient-arena slot has exactly one
        plain-writing producer kernel per step."""
        inc_early = False
        if with_opt and self.s_side is not None:
            # LR-step counter increment runs on the side stream, overlapped
            # with forward (it must still follow the previous step's adam,
            # hence the fork event)
            e = torch.cuda.Event()
            e.record(torch.cuda.current_stream(self.device))
            self.s_side.wait_event(e)
            with torch.cuda.stream(self.s_side):
                self.ext.step_inc(self.step_t)
            inc_early = True
        if rng_in_graph:
            if self._rng_side and N <= 384:
                # _launch_forward takes its fused path and issues the fills
                # on side stream 0
                self._rng_pending = True
            else:
                self._fill_rng(N)
        self._launch_forward(N, T, x=x, y=y, train=True)
        assert not self._rng_pending
        self._launch_backward(N, T, x=x, y=y, comm_overlap=comm_in_graph)
        if comm_in_graph:
            # the non-extractor slice was reduced inside backward,
            # overlapped; only the extractor slice remains
            head = self.grads[:self.params.offsets["Wenc"][0]]
            head.div_(get_world_size())
            torch.distributed.all_reduce(head)
        if with_opt:
            self._launch_optimizer(inc=not inc_early)

    def step(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """One training step on a day cross-section; returns device loss."""
        N, T, C = x.shape
        assert C == self.C
        self._ensure_ws(N, T)
        w = self.ws
        self._main_entry()
        with self._main_ctx():
            w["x"].copy_(x)
            w["y"].copy_(y.view(N, 1))

        if not self.use_graph:
            from ..observability import roctx_range

            with self._main_ctx():
                self._fill_rng(N)
                with roctx_range("fv_forward"):
                    self._launch_forward(N, T, train=True)
                with roctx_range("fv_backward"):
                    self._launch_backward(N, T)
                if is_distributed():
                    with roctx_range("fv_allreduce"):
                        self.grads.div_(get_world_size())
                        torch.distributed.all_reduce(self.grads)
                with roctx_range("fv_adam"):
                    self._launch_optimizer()
            self._main_exit()
            return w["loss"]

        rng_ok, comm_ok = self._probe_caps()
        key = ("train", N, T)
        if key not in self._graphs:
            try:
                self._capture(key, N, T, rng_ok, comm_ok)
            except Exception:
                # capture unavailable (driver box quirk): permanent
                # fallback to the eager-launch path — same kernels, same
                # numerics, just per-launch dispatch cost
                torch.cuda.synchronize(self.device)
                self.use_graph = False
                return self.step(x, y)
        plan = self._graphs[key]
        if not rng_ok:
            with self._main_ctx():
                self._fill_rng(N)
        with self._main_ctx():
            if plan["split"]:
                plan["g_fb"].replay()
                self.grads.div_(get_world_size())
                torch.distributed.all_reduce(self.grads)
                plan["g_opt"].replay()
            else:
                plan["g"].replay()
        self._main_exit()
        return w["loss"]

    def _capture(self, key, N: int, T: int, rng_ok: bool, comm_ok: bool):
        # warmup fwd+bwd (settles lazy state; params/step counter untouched)
        torch.cuda.synchronize()
        with self._main_ctx():
            if not rng_ok:
                self._fill_rng(N)
            self.grads.zero_()
            self._launch_forward(N, T, train=True)
            self._launch_backward(N, T)
        torch.cuda.synchronize()

        split = is_distributed() and not comm_ok
        if split:
            g1 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g1, stream=self.s_main):
                self._graph_step_body(None, None, N, T, rng_ok, False,
                                      with_opt=False)
            g2 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g2, stream=self.s_main):
                self._launch_optimizer()
            self._graphs[key] = {"split": True, "g_fb": g1, "g_opt": g2}
        else:
            with self._abort_watchdog("train-step graph capture"):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=self.s_main):
                    self._graph_step_body(None, None, N, T, rng_ok,
                                          is_distributed() and comm_ok)
            self._graphs[key] = {"split": False, "g": g}

    # -------------------------------------------------------- bench fast path
    def make_bench_runner(self, days):
        """Capture len(days) full training steps into ONE graph that reads
        the resident day tensors directly (no copies, no per-step host
        work). Returns (replay_fn, steps_per_replay). Falls back to the
        per-step path when collectives cannot be captured."""
        G = len(days)
        N, T, C = days[0][0].shape
        self._ensure_ws(N, T)
        rng_ok, comm_ok = self._probe_caps()
        days = [(x, y.view(-1, 1)) for x, y in days]

        if is_distributed() and not comm_ok:
            def run_fallback():
                for x, y in days:
                    self.step(x, y)
            return run_fallback, G

        # warmup
        torch.cuda.synchronize()
        with self._main_ctx():
            if not rng_ok:
                self._fill_rng(N)
            self.grads.zero_()
            self._launch_forward(N, T, x=days[0][0], y=days[0][1],
                                 train=True)
            self._launch_backward(N, T, x=days[0][0], y=days[0][1])
        torch.cuda.synchronize()

        # per-day RNG buffers when RNG can't live in the graph
        rng_bufs = None
        if not rng_ok:
            rng_bufs = [(torch.empty(N, device=self.device),
                         torch.empty(N, self.K, device=self.device))
                        for _ in range(G)]

        try:
            with self._abort_watchdog("bench multi-step graph capture"):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=self.s_main):
                    for i, (x, y) in enumerate(days):
                        if rng_bufs is not None:
                            self.ws["eps"].copy_(rng_bufs[i][0])
                            if self.training:
                                self.ws["mask"].copy_(rng_bufs[i][1])
                        self._graph_step_body(x, y, N, T, rng_ok,
                                              is_distributed() and comm_ok)
        except Exception:
            torch.cuda.synchronize()

            def run_nograph():
                for x, y in days:
                    self.step(x, y)
            return run_nograph, G

        def run():
            if rng_bufs is not None:
                for e, m in rng_bufs:
                    e.normal_()
                    if self.training:
                        m.bernoulli_(1.0 - self.DROPOUT_P)
            self._main_entry()  # order replay after the RNG fills
            with self._main_ctx():
                g.replay()
            self._main_exit()   # next call's fills wait for this replay

        return run, G

    def forward_only(self, x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
        """Fused validation forward (no grad); returns device loss.
        hipGraph-captured per (N, T, dropout-mode) like the train step —
        the per-epoch validation pass otherwise pays full launch
        latency for every kernel."""
        N, T, C = x.shape
        self._ensure_ws(N, T)
        w = self.ws
        self._main_entry()
        with self._main_ctx():
            w["x"].copy_(x)
            w["y"].copy_(y.view(N, 1))
            self._fill_rng(N)
        if not self.use_graph:
            with self._main_ctx():
                self._launch_forward(N, T)
            self._main_exit()
            return w["loss"]
        key = ("val", N, T, self.training)
        if key not in self._graphs:
            try:
                torch.cuda.synchronize(self.device)
                with self._main_ctx():
                    self._launch_forward(N, T)  # warmup
                torch.cuda.synchronize(self.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=self.s_main):
                    self._launch_forward(N, T)
                self._graphs[key] = {"g": g}
            except Exception:
                torch.cuda.synchronize(self.device)
                self._graphs[key] = {"g": None}
        g = self._graphs[key]["g"]
        with self._main_ctx():
            if g is None:
                self._launch_forward(N, T)
            else:
                g.replay()
        self._main_exit()
        return w["loss"]

    def _launch_predict(self, N: int, T: int):
        """Prediction kernel sequence: extractor -> predictor (prior) ->
        decoder with PRIOR mu/sigma (module.py:273-278)."""
        ext, p, w = self.ext, self.p, self.ws
        self._launch_forward(N, T, with_loss=False)
        ext.dec_fwd(w["h"], p("W1d"), p("b1d"), p("wmu_d"), p("bmu_d"),
                    p("wsig_d"), p("bsig_d"), p("Wb"), p("bb"), w["pmu"],
                    w["psig_c"], w["eps"], w["recon"], w["a1"], w["beta"],
                    w["asig_pre"], w["sigma"])

    def predict(self, x: torch.Tensor) -> torch.Tensor:
        """model.prediction through the fused kernels; the sequence is
        hipGraph-captured per (N, T) shape (eps refilled outside)."""
        N, T, C = x.shape
        self._ensure_ws(N, T)
        w = self.ws
        self._main_entry()
        with self._main_ctx():
            w["x"].copy_(x)
        was_training = self.training
        self.training = False  # prediction: dropout off
        try:
            with self._main_ctx():
                self._fill_rng(N)
            if not self.use_graph:
                with self._main_ctx():
                    w["y"].zero_()
                    self._launch_predict(N, T)
                self._main_exit()
                return w["recon"].view(N, 1).clone()
            key = ("predict", N, T)
            if key not in self._graphs:
                try:
                    w["y"].zero_()
                    torch.cuda.synchronize(self.device)
                    with self._main_ctx():
                        self._launch_predict(N, T)  # warmup
                    torch.cuda.synchronize(self.device)
                    gp = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gp, stream=self.s_main):
                        self._launch_predict(N, T)
                    self._graphs[key] = {"g": gp}
                except Exception:
                    torch.cuda.synchronize(self.device)
                    self._graphs[key] = {"g": None}
            gp = self._graphs[key]["g"]
            with self._main_ctx():
                if gp is None:
                    self._launch_predict(N, T)
                else:
                    gp.replay()
            self._main_exit()
            return w["recon"].view(N, 1).clone()
        finally:
            self.training = was_training

    # ------------------------------------------------ batched scoring
    # default row budget (sum of N_d * T) of one predict_many chunk:
    # ~2 KB of workspace per row at C=158/H=64, i.e. about 1 GB
    PREDICT_ROWS = 1 << 19

    def _alloc_infer_ws(self, R: int, Nn: int, D: int, with_beta: bool,
                        with_svar: bool = False):
        """Grow-only inference workspace of predict_many; separate from
        self.ws / the (N, T) shape cache so scoring never disturbs
        training buffers or captured graphs."""
        iw = self.__dict__.setdefault("_iws", {"R": 0, "N": 0, "D": 0})
        d, C, H, K = self.device, self.C, self.H, self.K
        f = lambda *shape: torch.empty(*shape, device=d, dtype=torch.float32)
        if "qk" not in iw:
            iw["qk"] = f(K, H)
            iw["cb"] = f(K)
        if R > iw["R"]:
            iw["x"] = f(R, C)
            iw["mean"] = f(R)
            iw["rstd"] = f(R)
            iw["gi"] = f(R, 3 * H)
            iw.pop("xln", None)
            if self.bf16:
                # zeroed tail slack: the register-stationary NT kernel
                # reads every row as KP = ceil32(C) elements against
                # zero-padded weights, so the last row's k-tail fragment
                # reads KP - C elements past it (2 at C = 158, where
                # _alloc_ws's 8 suffice; 22 at C = 10), and 0 * garbage
                # is only 0 for finite garbage
                slack = self.w1x_p.shape[1] - C + 8
                fbs = lambda r, c: torch.zeros(
                    r * c + slack, device=d,
                    dtype=torch.bfloat16)[:r * c].view(r, c)
                iw["xln_bf"] = fbs(R, C)
                iw["xp_bf"] = fbs(R, C)
            else:
                iw["xp"] = f(R, C)
            iw["R"] = R
        if Nn > iw["N"]:
            iw["h"] = f(Nn, H)
            iw["eps"] = f(Nn)
            iw["out"] = f(3, Nn)  # rows: sample, mu, sigma
            iw.pop("beta", None)
            iw.pop("svar", None)
            iw.pop("label", None)
            iw["N"] = Nn
        if with_beta and "beta" not in iw:
            iw["beta"] = f(iw["N"], K)
        if with_svar and "svar" not in iw:
            iw["svar"] = f(iw["N"])
        if D > iw["D"]:
            iw["seg_off"] = torch.empty(D + 1, device=d, dtype=torch.int32)
            iw["pmu"] = f(D, K)
            iw["psig_c"] = f(D, K)
            iw["guard"] = torch.empty(D, K, device=d, dtype=torch.int32)
            iw["D"] = D
        return iw

    def _launch_infer_head(self, iw, x2d, gi):
        """Extractor head of the engine's dtype over the rows of x2d
        (R, C) into gi (R, 3H), through the inference workspace. Row-local:
        a row's gi does not depend on where in x2d it stands."""
        ext, p = self.ext, self.p
        R = x2d.shape[0]
        mean, rstd = iw["mean"][:R], iw["rstd"][:R]
        if self.bf16:
            xln_bf = iw["xln_bf"][:R]
            xp_bf = iw["xp_bf"][:R]
            ext.ln_fwd(x2d, p("ln_g"), p("ln_b"), None, mean, rstd, 1e-5,
                       xln_bf)
            ext.gemm_nt_bf16_rs(xln_bf, self.w1x_p, p("b1x"), None, xp_bf,
                                None, 1.0, True)
            ext.gemm_nt_bf16_rs(xp_bf, self.wih_p, p("bih"), gi, None, None,
                                1.0, False)
        else:
            xp = iw["xp"][:R]
            if not (self._f32_head and ext.extractor_head_fwd(
                    x2d, p("ln_g"), p("ln_b"), p("W1x"), p("b1x"), p("Wih"),
                    p("bih"), None, mean, rstd, xp, gi, 1e-5)):
                if "xln" not in iw:
                    iw["xln"] = torch.empty(iw["R"], self.C,
                                            device=self.device)
                xln = iw["xln"][:R]
                ext.ln_fwd(x2d, p("ln_g"), p("ln_b"), xln, mean, rstd, 1e-5)
                ext.gemm_nt(xln, p("W1x"), p("b1x"), xp, 1.0, False, True)
                ext.gemm_nt(xp, p("Wih"), p("bih"), gi, 1.0, False, False)

    def _launch_predict_many(self, iw, R: int, Nn: int, D: int, T: int,
                             max_n: int, with_beta: bool,
                             prior_dec: bool = True,
                             with_svar: bool = False):
        """Kernel sequence of one packed chunk: extractor head of the
        engine's dtype over all rows -> GRU without backward state ->
        _launch_pm_tail."""
        ext, p, H = self.ext, self.p, self.H
        gi = iw["gi"][:R]
        h = iw["h"][:Nn]
        self._launch_infer_head(iw, iw["x"][:R], gi)
        if self.bf16 and H == 64:
            ext.gru_fwd_mfma_infer(gi, self.whh_bf, p("bhh"), h, Nn, T, H)
        else:
            ext.gru_fwd_infer(gi, p("Whh"), p("bhh"), h, Nn, T, H,
                              variant=self._gru_v)
        self._launch_pm_tail(iw, Nn, D, max_n, with_beta, prior_dec,
                             with_svar)

    def _launch_pm_tail(self, iw, Nn: int, D: int, max_n: int,
                        with_beta: bool, prior_dec: bool = True,
                        with_svar: bool = False):
        """Behind the GRU of one packed chunk: segmented prior attention ->
        segmented decoder (prior_dec=False stops behind the attention:
        loss_many decodes the posterior only). with_svar: the decoder also
        writes the rows' idiosyncratic variance into iw["svar"]."""
        ext, p, H = self.ext, self.p, self.H
        h = iw["h"][:Nn]
        seg = iw["seg_off"][:D + 1]
        alpha = 1.0 / math.sqrt(float(H) + 1e-6)
        ext.attn_seg_fwd(h, seg, max_n, iw["qk"], iw["cb"], self.p_Wv,
                         self.p_bv, p("Wl"), p("bl"), p("wmu_p"), p("bmu_p"),
                         p("wsig_p"), p("bsig_p"), iw["pmu"], iw["psig_c"],
                         iw["guard"], alpha)
        if not prior_dec:
            return
        out = iw["out"]
        ext.dec_seg_fwd(h, seg, p("W1d"), p("b1d"), p("wmu_d"), p("bmu_d"),
                        p("wsig_d"), p("bsig_d"), p("Wb"), p("bb"), iw["pmu"],
                        iw["psig_c"], iw["eps"][:Nn], out[1, :Nn],
                        out[2, :Nn], out[0, :Nn],
                        iw["beta"][:Nn] if with_beta else None,
                        iw["svar"][:Nn] if with_svar else None)

    def _launch_posterior(self, iw, Nn: int, D: int, max_n: int,
                          with_factors: bool):
        """Posterior steps of one packed chunk, behind
        _launch_predict_many's attention: segmented encoder -> posterior
        heads -> segmented decoder fed the posterior rows and the chunk's
        eps -> segmented loss. Returns the chunk's result as one flat
        device vector: loss[D] mse[D] kl[D], and with_factors also
        post_mu, post_sigma, prior_mu, prior_sigma, D*K each."""
        ext, p = self.ext, self.p
        M, K = self.M, self.K
        f = lambda *shape: torch.empty(*shape, device=self.device,
                                       dtype=torch.float32)
        # grow-only, sized with the buffers _alloc_infer_ws keeps
        if iw.get("post_N", 0) < iw["N"]:
            iw["post_out"] = f(3, iw["N"])  # rows: recon, mu, sigma
            iw["post_N"] = iw["N"]
        if iw.get("post_D", 0) < iw["D"]:
            iw["yp"] = f(iw["D"], M)
            iw["post"] = f(iw["D"] * (3 + 4 * K))
            iw["post_D"] = iw["D"]
        DK = D * K
        flat = iw["post"]
        loss, mse, kl = flat[:D], flat[D:2 * D], flat[2 * D:3 * D]
        fmu = flat[3 * D:3 * D + DK].view(D, K)
        fsig_c = flat[3 * D + DK:3 * D + 2 * DK].view(D, K)
        h, seg = iw["h"][:Nn], iw["seg_off"][:D + 1]
        y, yp, po = iw["label"][:Nn], iw["yp"][:D], iw["post_out"]
        pmu, psig_c = iw["pmu"][:D], iw["psig_c"][:D]
        ext.enc_seg_fwd(h, seg, max_n, p("Wenc"), p("benc"), y, yp)
        ext.enc_seg_heads(yp, p("Wmu_e"), p("bmu_e"), p("Wsig_e"),
                          p("bsig_e"), fmu, fsig_c)
        ext.dec_seg_fwd(h, seg, p("W1d"), p("b1d"), p("wmu_d"), p("bmu_d"),
                        p("wsig_d"), p("bsig_d"), p("Wb"), p("bb"), fmu,
                        fsig_c, iw["eps"][:Nn], po[1, :Nn], po[2, :Nn],
                        po[0, :Nn], None)
        ext.loss_seg(po[0, :Nn], y, seg, fmu, fsig_c, pmu, psig_c, loss, mse,
                     kl)
        if not with_factors:
            return flat[:3 * D]
        flat[3 * D + 2 * DK:3 * D + 3 * DK].copy_(pmu.reshape(-1))
        flat[3 * D + 3 * DK:3 * D + 4 * DK].copy_(psig_c.reshape(-1))
        return flat[:3 * D + 4 * DK]

    @torch.no_grad()
    def loss_many(self, days, eps=None, sample: bool = True,
                  return_factors: bool = False,
                  max_rows: Optional[int] = None):
        """Per-day validation loss, and optionally the factors, of many
        trading days in a few launches: the posterior half of the model
        (encoder q(z | x, y), decoder driven by the posterior factors,
        MSE + KL against the prior) over the packing of predict_many.

        days: list of (x_d (N_d, T, C), y_d (N_d, 1) or (N_d,)), host or
        device, or a PanelDays with labels (the same bits as the list of
        its windows()). eps: optional list of (N_d,) reparameterisation
        draws;
        when None they are drawn per chunk with torch's generator, as
        predict_many does, unless sample=False, which zero-fills them (the
        reconstruction is then the posterior mean) and leaves torch's
        generators alone. A given eps is used whatever `sample` says.

        Returns host tensors in input-day order: {"loss", "mse", "kl":
        (D,) float32, "n": (D,) int32 rows per day}, and with
        return_factors also "post_mu", "post_sigma", "prior_mu",
        "prior_sigma": (D, K) — the sigmas as the KL sees them, after the
        zero clamp. A day without rows has n = 0 and NaN everywhere else.

        Days are chunked exactly as in predict_many (one kernel sequence
        and one device-to-host copy per chunk) and a day's result does not
        depend on what it is batched with. Dropout is off, as in
        validate_epoch. Like predict_many it touches no training buffer,
        captured graph or in-graph RNG state."""
        xs, ys, lens_all = self._pm_split_days("loss_many", days)
        if eps is not None:
            eps = list(eps)
        D_all, K = len(lens_all), self.K
        nan = float("nan")
        res = {k: torch.full((D_all,), nan) for k in ("loss", "mse", "kl")}
        res["n"] = torch.tensor(lens_all, dtype=torch.int32)
        names = ("post_mu", "post_sigma", "prior_mu", "prior_sigma")
        if return_factors:
            for name in names:
                res[name] = torch.full((D_all, K), nan)
        for idxs, lens, offs, iw in self._pm_chunks(
                "loss_many", xs, eps, max_rows, False, ys=ys,
                draw_eps=sample, prior_dec=False):
            if iw is None:
                continue  # days without rows: n = 0, NaN
            D = len(idxs)
            host = self._launch_posterior(iw, offs[-1], D, max(lens),
                                          return_factors).cpu()
            ii = torch.tensor(idxs)
            for j, k in enumerate(("loss", "mse", "kl")):
                res[k][ii] = host[j * D:(j + 1) * D]
            if return_factors:
                for j, name in enumerate(names):
                    o = 3 * D + j * D * K
                    res[name][ii] = host[o:o + D * K].view(D, K)
        if return_factors:
            # an empty day inside a chunk: its factor rows were never
            # written on the device
            empty = res["n"] == 0
            for name in names:
                res[name][empty] = nan
        return res

    @torch.no_grad()
    def predict_many(self, xs, eps=None, return_dist: bool = False,
                     return_beta: bool = False,
                     max_rows: Optional[int] = None):
        """Score many trading days in a few launches.

        xs: list of (N_d, T, C) tensors (N_d may differ; T and C fixed;
        host or device), or a PanelDays, which gives the same bits as the
        list of its windows() (the extractor head then runs once per
        referenced row, see _pm_chunks_panel). eps: optional list of (N_d,) standard-normal
        draws; when None they are drawn per chunk with torch's generator.

        Returns one entry per day, on the host:
          score                          (default)
          (score, mu, sigma)             return_dist
          (score, beta)                  return_beta
          (score, mu, sigma, beta)       both
        score / mu / sigma are (N_d, 1), beta is (N_d, K); score is the
        reference's stochastic sample mu + eps * sigma, mu and sigma the
        decoder's predictive mean and risk under the prior.

        Days are packed greedily into chunks whose sum of N_d * T stays
        within max_rows (default FV_PREDICT_ROWS); a day larger than the
        budget is its own chunk. Each chunk is one host-to-device copy
        (host inputs), one kernel sequence over the packed rows and one
        device-to-host copy. A day's result does not depend on what it is
        batched with. Uses a dedicated inference workspace: training
        buffers, the shape/graph cache and the in-graph RNG state are not
        touched (with eps=None the generator advances, as in predict)."""
        if not isinstance(xs, PanelDays):
            xs = list(xs)
        if eps is not None:
            eps = list(eps)
        results = [None] * len(xs)
        for idxs, lens, offs, iw in self._pm_chunks(
                "predict_many", xs, eps, max_rows, return_beta):
            if iw is None:
                for i in idxs:
                    results[i] = self._pm_entry(
                        torch.empty(3, 0), torch.empty(0, self.K), 0, 0,
                        return_dist, return_beta)
                continue
            Nn = offs[-1]
            out = iw["out"][:, :Nn].cpu()  # the chunk's one D2H copy
            beta = iw["beta"][:Nn].cpu() if return_beta else None
            for i, o, n in zip(idxs, offs, lens):
                results[i] = self._pm_entry(out, beta, o, n, return_dist,
                                            return_beta)
        return results

    @torch.no_grad()
    def risk_many(self, xs, weights=None, solve=(),
                  return_components: bool = False,
                  max_rows: Optional[int] = None):
        """The factor risk model of many trading days on the device: per
        day the covariance the prior decoder implies,
        Sigma = beta diag(factor_sigma^2) beta^T + diag(specific_var)
        (factorvae_amd.risk), evaluated for one portfolio and optionally
        solved for minimum-variance / mean-variance weights, without beta
        or Sigma leaving the device.

        xs: list of (N_d, T, C) or a PanelDays, as for predict_many.
        weights: None (equal weight 1/N_d) or one (N_d,) tensor per day,
        host or device, used as given (no normalisation). solve: a subset
        of ("minvar", "mv"): Sigma^-1 1 / (1^T Sigma^-1 1) and
        Sigma^-1 mu / |Sigma^-1 mu|_1 (all-zero when that norm is 0).

        Returns host tensors in input-day order: "n" (D,) int32; "mean",
        "mean_factor", "var_factor", "var_specific", "vol" (D,) float32;
        "exposure", "factor_var" (D, K); "mcr" a list of (N_d,) marginal
        contributions to risk (sum_i w_i mcr_i = vol); with solve the
        lists "minvar" / "mv" of (N_d,) weights and "solve_info" (D,)
        int32 (0 solved, 1 a failed Cholesky pivot: that day's weights are
        NaN); with return_components the lists "mu", "specific_var"
        (N_d,), "beta" (N_d, K) and "factor_mu", "factor_sigma" (D, K). A
        day without rows has n = 0, NaN per-day values and empty per-stock
        tensors.

        Days are chunked exactly as in predict_many (one kernel sequence
        and one device-to-host copy of a flat result buffer per chunk) and
        a day's result does not depend on what it is batched with. The
        decoder's eps is zero-filled: torch's generators are left alone.
        Like predict_many it touches no training buffer or captured
        graph."""
        from ..risk import STAT_KEYS, check_solve, check_weights, empty_result

        solve = check_solve(solve)
        panel = isinstance(xs, PanelDays)
        if not panel:
            xs = list(xs)
        lens_all = xs.lens() if panel else [int(x.shape[0]) for x in xs]
        weights = check_weights(weights, lens_all)
        K, R, dev = self.K, len(solve), self.device
        res = empty_result(lens_all, K, solve, return_components)
        for idxs, lens, offs, iw in self._pm_chunks(
                "risk_many", xs, None, max_rows, True, draw_eps=False,
                with_svar=True):
            if iw is None:
                continue  # days without rows: n = 0, NaN
            D, Nn = len(idxs), offs[-1]
            # flat result: stats D*5 | exposure D*K | factor_var D*K |
            # mcr Nn | weights Nn*R | info D (int32 bits) | components
            size = D * (5 + 2 * K) + Nn + Nn * R + (D if R else 0)
            if return_components:
                size += Nn * (2 + K) + 2 * D * K
            if iw.get("risk_cap", 0) < size:
                iw["risk"] = torch.empty(size, device=dev)
                iw["risk_cap"] = size
            if iw.get("risk_w_cap", 0) < iw["N"]:
                iw["risk_w"] = torch.empty(iw["N"], device=dev)
                iw["risk_b"] = torch.empty(iw["N"] * 4, device=dev)
                iw["risk_x"] = torch.empty(iw["N"] * 4, device=dev)
                iw["risk_w_cap"] = iw["N"]
            flat, o = iw["risk"], 0

            def take(n, *shape):
                nonlocal o
                v = flat[o:o + n]
                o += n
                return v.view(*shape) if shape else v

            stats = take(D * 5, D, 5)
            expo, fvar = take(D * K, D, K), take(D * K, D, K)
            mcr = take(Nn)
            wout = take(Nn * R, R, Nn) if R else None
            info = take(D).view(torch.int32) if R else None

            wd = iw["risk_w"]
            if weights is None:
                wd[:Nn].copy_(torch.cat([
                    torch.full((n,), 1.0 / n if n else 0.0) for n in lens]))
            else:
                self._pm_pack_rows(wd, [weights[i] for i in idxs], offs,
                                   lens)
            seg = iw["seg_off"][:D + 1]
            beta, svar = iw["beta"][:Nn], iw["svar"][:Nn]
            mu = iw["out"][1, :Nn]
            pmu, psig_c = iw["pmu"][:D], iw["psig_c"][:D]
            self.ext.risk_seg(beta, svar, mu, wd[:Nn], seg, pmu, psig_c,
                              stats, expo, fvar, mcr)
            if R:
                b = iw["risk_b"][:Nn * R].view(Nn, R)
                x = iw["risk_x"][:Nn * R].view(Nn, R)
                for c, s in enumerate(solve):
                    if s == "minvar":
                        b[:, c].fill_(1.0)
                    else:
                        b[:, c].copy_(mu)
                norms = torch.empty(D, 2, R, device=dev)
                self.ext.risk_solve_seg(beta, svar, seg, psig_c, b, x, info,
                                        norms)
                # the day's normaliser spread over its rows; the segment
                # sums come from the kernel, ordered within the day
                rows = torch.repeat_interleave(
                    norms, torch.tensor(lens, device=dev), dim=0,
                    output_size=Nn)
                for c, s in enumerate(solve):
                    if s == "minvar":
                        torch.div(x[:, c], rows[:, 0, c], out=wout[c])
                    else:
                        den = rows[:, 1, c]
                        wout[c].copy_(torch.where(
                            den == 0, torch.zeros_like(den), x[:, c] / den))
            if return_components:
                take(Nn).copy_(mu)
                take(Nn).copy_(svar)
                take(Nn * K).copy_(beta.reshape(-1))
                take(D * K).copy_(pmu.reshape(-1))
                take(D * K).copy_(psig_c.reshape(-1))
            host = flat[:o].cpu()  # the chunk's one D2H copy
            o = 0

            def give(n, *shape):
                nonlocal o
                v = host[o:o + n]
                o += n
                return v.view(*shape) if shape else v

            ii = torch.tensor(idxs)
            st_h = give(D * 5, D, 5)
            for j, k in enumerate(STAT_KEYS):
                res[k][ii] = st_h[:, j]
            res["exposure"][ii] = give(D * K, D, K)
            res["factor_var"][ii] = give(D * K, D, K)
            per_stock = {"mcr": give(Nn)}
            if R:
                w_h = give(Nn * R, R, Nn)
                for c, s in enumerate(solve):
                    per_stock[s] = w_h[c]
                res["solve_info"][ii] = give(D).view(torch.int32)
            if return_components:
                per_stock["mu"] = give(Nn)
                per_stock["specific_var"] = give(Nn)
                per_stock["beta"] = give(Nn * K, Nn, K)
                res["factor_mu"][ii] = give(D * K, D, K)
                res["factor_sigma"][ii] = give(D * K, D, K)
            for k, v in per_stock.items():
                for i, a, n in zip(idxs, offs, lens):
                    res[k][i] = v[a:a + n]
        if return_components:
            # an empty day inside a chunk: its prior rows were never
            # written on the device
            empty = res["n"] == 0
            res["factor_mu"][empty] = float("nan")
            res["factor_sigma"][empty] = float("nan")
        return res

    def _pm_chunks(self, what: str, xs, eps, max_rows, with_beta: bool,
                   ys=None, draw_eps: bool = True, prior_dec: bool = True,
                   with_svar: bool = False):
        """The chunk/pack loop shared by predict_many and evaluate_many:
        checks the days, packs them greedily into chunks within max_rows,
        and for each chunk copies the inputs into the inference workspace,
        runs the kernel sequence and yields (idxs, lens, offs, iw) with
        the results still on the device. A chunk without any row yields
        iw = None and launches nothing. ys: optional per-day labels, packed
        into iw["label"]. draw_eps=False zero-fills a missing eps instead
        of drawing it, leaving torch's generator alone. prior_dec=False
        leaves out the prior decoder (_launch_predict_many); with_svar
        adds its idiosyncratic variance output iw["svar"]. xs may be a
        PanelDays (_pm_chunks_panel): the same chunks, the same yields."""
        if self.fp8:
            raise ValueError(f"{what} supports the fp32 and bf16 "
                             "engines; fp8 scoring is not implemented")
        if self.K > 128:
            raise UnsupportedShapeError(
                f"{what} supports num_factor <= 128, got {self.K}")
        if eps is not None:
            if len(eps) != len(xs):
                raise ValueError("eps must hold one (N_d,) tensor per day")
        if not len(xs):
            return
        if isinstance(xs, PanelDays):
            yield from self._pm_chunks_panel(what, xs, eps, max_rows,
                                             with_beta, ys, draw_eps,
                                             prior_dec, with_svar)
            return
        T = xs[0].shape[1]
        for i, x in enumerate(xs):
            if x.ndim != 3 or x.shape[1] != T or x.shape[2] != self.C:
                raise ValueError(
                    f"day {i}: expected (N, {T}, {self.C}), got "
                    f"{tuple(x.shape)}")
            if eps is not None and eps[i].numel() != x.shape[0]:
                raise ValueError(f"day {i}: eps must have {x.shape[0]} "
                                 f"entries, got {eps[i].numel()}")
            if ys is not None and ys[i].numel() != x.shape[0]:
                raise ValueError(f"day {i}: labels must have {x.shape[0]} "
                                 f"entries, got {ys[i].numel()}")
        if max_rows is None:
            max_rows = (int(os.environ.get("FV_PREDICT_ROWS", "0"))
                        or self.PREDICT_ROWS)
        chunks = self._pm_greedy([x.shape[0] for x in xs], T, max_rows)

        ext, C = self.ext, self.C
        # everything below runs on the caller's stream: order it after any
        # training step still in flight on the priority stream
        self._main_exit()
        qk_done = False
        for idxs in chunks:
            lens = [xs[i].shape[0] for i in idxs]
            Nn, D = sum(lens), len(idxs)
            R = Nn * T
            offs = [0]
            for n in lens:
                offs.append(offs[-1] + n)
            if Nn == 0:
                yield idxs, lens, offs, None
                continue
            iw = self._alloc_infer_ws(R, Nn, D, with_beta, with_svar)
            if not qk_done:
                ext.attn_qk_fwd(self.p_q, self.p_Wk, self.p_bk, iw["qk"],
                                iw["cb"])
                qk_done = True
            iw["seg_off"][:D + 1].copy_(
                torch.tensor(offs, dtype=torch.int32), non_blocking=False)
            xd = iw["x"][:R]
            flat = [xs[i].reshape(-1, C) for i in idxs]
            if all(t.device.type == "cpu" for t in flat):
                host = torch.cat([t.float() for t in flat], dim=0)
                xd.copy_(host)
            elif all(t.device == xd.device and t.dtype == xd.dtype
                     for t in flat):
                torch.cat(flat, dim=0, out=xd)  # one packing kernel
            else:
                for t, o, n in zip(flat, offs, lens):
                    xd[o * T:(o + n) * T].copy_(t)
            self._pm_pack_eps_labels(iw, idxs, lens, offs, eps, ys, draw_eps)
            self._launch_predict_many(iw, R, Nn, D, T, max(lens), with_beta,
                                      prior_dec, with_svar)
            yield idxs, lens, offs, iw

    @staticmethod
    def _pm_split_days(what: str, days):
        """(xs, ys, rows per day) of a list of (x_d, y_d) or a PanelDays."""
        if isinstance(days, PanelDays):
            if days.labels is None:
                raise ValueError(f"{what} needs a panel with labels")
            return days, days.labels, days.lens()
        days = list(days)
        return ([x for x, _ in days], [y for _, y in days],
                [int(x.shape[0]) for x, _ in days])

    @staticmethod
    def _pm_greedy(lens, T: int, max_rows: int):
        """Day numbers packed greedily into chunks whose sum of N_d * T
        stays within max_rows; a larger day is its own chunk."""
        chunks, cur, rows = [], [], 0
        for i, n in enumerate(lens):
            r = n * T
            if cur and rows + r > max_rows:
                chunks.append(cur)
                cur, rows = [], 0
            cur.append(i)
            rows += r
        chunks.append(cur)
        return chunks

    def _pm_pack_eps_labels(self, iw, idxs, lens, offs, eps, ys,
                            draw_eps: bool):
        """A chunk's eps (given, drawn over its Nn rows at once, or zero)
        and labels into the inference workspace."""
        Nn = offs[-1]
        if eps is None:
            if draw_eps:
                iw["eps"][:Nn].normal_()
            else:
                iw["eps"][:Nn].zero_()
        else:
            self._pm_pack_rows(iw["eps"], [eps[i] for i in idxs], offs, lens)
        if ys is not None:
            if "label" not in iw:
                iw["label"] = torch.empty(iw["N"], device=self.device)
            self._pm_pack_rows(iw["label"], [ys[i] for i in idxs], offs,
                               lens)

    # default row budget of one day block of the panel route: gi_rows is
    # 768 B per row at H = 64, i.e. 1.5 GiB
    PANEL_ROWS = 1 << 21

    def _pm_chunks_panel(self, what: str, panel, eps, max_rows,
                         with_beta: bool, ys, draw_eps: bool,
                         prior_dec: bool, with_svar: bool = False):
        """_pm_chunks for a PanelDays: the same greedy day chunks (so a
        seed draws the same eps) and the same yields, but the extractor
        head runs once per referenced row and the GRU gathers.

        Consecutive chunks form a day block while the row range
        [lo, hi] they reference holds at most FV_PANEL_ROWS rows. Per
        block the head runs over rows[lo:hi+1] in slices of at most
        max_rows rows into the grow-only gi_rows buffer; per chunk the
        ids, rebased by -lo with negative entries kept, go to the
        workspace and the gather GRU and _launch_pm_tail run."""
        T, C, H = panel.T, self.C, self.H
        lens = panel.lens()
        if panel.C != C:
            raise ValueError(f"{what}: the panel's rows have {panel.C} "
                             f"features, the model {C}")
        for i, n in enumerate(lens):
            if eps is not None and eps[i].numel() != n:
                raise ValueError(f"day {i}: eps must have {n} entries, got "
                                 f"{eps[i].numel()}")
        if max_rows is None:
            max_rows = (int(os.environ.get("FV_PREDICT_ROWS", "0"))
                        or self.PREDICT_ROWS)
        budget = (int(os.environ.get("FV_PANEL_ROWS", "0"))
                  or self.PANEL_ROWS)
        # day blocks of whole chunks: [lo, hi, chunks]; lo None = no row
        blocks = []
        for idxs in self._pm_greedy(lens, T, max_rows):
            spans = [panel.span[i] for i in idxs if panel.span[i]]
            lo = min((s[0] for s in spans), default=None)
            hi = max((s[1] for s in spans), default=None)
            if spans and hi - lo + 1 > budget:
                raise ValueError(
                    f"{what}: days {idxs[0]}..{idxs[-1]} reference a range "
                    f"of {hi - lo + 1} rows, more than FV_PANEL_ROWS = "
                    f"{budget}; lower max_rows or raise FV_PANEL_ROWS")
            b = blocks[-1] if blocks else None
            if b and not spans:
                b[2].append(idxs)
            elif b and b[0] is None:
                b[0], b[1] = lo, hi
                b[2].append(idxs)
            elif b and max(hi, b[1]) - min(lo, b[0]) + 1 <= budget:
                b[0], b[1] = min(lo, b[0]), max(hi, b[1])
                b[2].append(idxs)
            else:
                blocks.append([lo, hi, [idxs]])

        ext, p, dev = self.ext, self.p, self.device
        self._main_exit()
        step = max(int(max_rows), 1)
        qk_done = False
        for lo, hi, chunks in blocks:
            U = 0 if lo is None else hi - lo + 1
            lo = lo or 0
            Nn_max = max(sum(lens[i] for i in idxs) for idxs in chunks)
            if Nn_max == 0:
                for idxs in chunks:
                    yield idxs, [0] * len(idxs), [0] * (len(idxs) + 1), None
                continue
            iw = self._alloc_infer_ws(min(step, max(U, 1)), Nn_max,
                                      max(len(idxs) for idxs in chunks),
                                      with_beta, with_svar)
            if iw.get("gi_rows_cap", 0) < max(U, 1):
                iw["gi_rows"] = torch.empty(max(U, 1), 3 * H, device=dev)
                iw["gi_rows_cap"] = max(U, 1)
            if iw.get("pidx_cap", 0) < Nn_max * T:
                iw["pidx"] = torch.empty(Nn_max * T, device=dev,
                                         dtype=torch.int32)
                iw["pidx_cap"] = Nn_max * T
            gi_rows = iw["gi_rows"]
            for o in range(0, U, step):
                r = min(step, U - o)
                src = panel.rows[lo + o:lo + o + r]
                if src.device != gi_rows.device:   # host rows: slice by slice
                    iw["x"][:r].copy_(src)
                    src = iw["x"][:r]
                self._launch_infer_head(iw, src, gi_rows[o:o + r])
            if not qk_done:
                ext.attn_qk_fwd(self.p_q, self.p_Wk, self.p_bk, iw["qk"],
                                iw["cb"])
                qk_done = True
            for idxs in chunks:
                cl = [lens[i] for i in idxs]
                Nn, D = sum(cl), len(idxs)
                offs = [0]
                for n in cl:
                    offs.append(offs[-1] + n)
                if Nn == 0:
                    yield idxs, cl, offs, None
                    continue
                iw["seg_off"][:D + 1].copy_(
                    torch.tensor(offs, dtype=torch.int32), non_blocking=False)
                ids = torch.cat([panel.ids[i] for i in idxs], dim=0)
                pidx = iw["pidx"][:Nn * T].view(Nn, T)
                pidx.copy_(torch.where(ids >= 0, ids - lo, ids))
                self._pm_pack_eps_labels(iw, idxs, cl, offs, eps, ys,
                                         draw_eps)
                h = iw["h"][:Nn]
                if self.bf16 and H == 64:
                    ext.gru_fwd_mfma_infer_gather(gi_rows, U, pidx,
                                                  self.whh_bf, p("bhh"), h,
                                                  Nn, T, H)
                else:
                    ext.gru_fwd_infer_gather(gi_rows, U, pidx, p("Whh"),
                                             p("bhh"), h, Nn, T, H,
                                             variant=self._gru_v)
                self._launch_pm_tail(iw, Nn, D, max(cl), with_beta,
                                     prior_dec, with_svar)
                yield idxs, cl, offs, iw

    @staticmethod
    def _pm_pack_rows(dst, vals, offs, lens):
        """Pack per-day (N_d,) vectors back to back into dst[:sum N_d]."""
        Nn = offs[-1]
        v = [t.reshape(-1).float() for t in vals]
        if all(t.device.type == "cpu" for t in v):
            dst[:Nn].copy_(torch.cat(v))
        elif all(t.device == dst.device for t in v):
            torch.cat(v, out=dst[:Nn])
        else:
            for t, o, n in zip(v, offs, lens):
                dst[o:o + n].copy_(t)

    @staticmethod
    def _pm_entry(out, beta, o: int, n: int, return_dist: bool,
                  return_beta: bool):
        score = out[0, o:o + n].reshape(n, 1)
        if not (return_dist or return_beta):
            return score
        entry = [score]
        if return_dist:
            entry += [out[1, o:o + n].reshape(n, 1),
                      out[2, o:o + n].reshape(n, 1)]
        if return_beta:
            entry.append(beta[o:o + n])
        return tuple(entry)

    # ------------------------------------------------- on-device metrics
    # longest day daily_ic_seg's LDS plan holds; longer days come back
    # with count = -1
    EVAL_MAX_N = 8192

    @torch.no_grad()
    def evaluate_many(self, days, on=("mu",), topk: int = 0, eps=None,
                      max_rows: Optional[int] = None,
                      with_loss: bool = False):
        """Per-day IC, RankIC and top-k long/short returns of many trading
        days, computed on the device from the batched scoring workspace.

        days: list of (x_d (N_d, T, C), y_d (N_d, 1) or (N_d,)), host or
        device, or a PanelDays with labels (the same bits as the list of
        its windows()). on: the prediction columns to rank on, a subset of
        ("score", "mu") — the stochastic sample and the predictive mean.
        eps as in predict_many; when None, "score" draws it and a
        mu-only evaluation leaves torch's generator alone.

        Days are packed and chunked exactly as in predict_many; after a
        chunk's kernel sequence daily_ic_seg reads the requested rows of
        the packed scores and only D*P*4 doubles + D*P ints come back to
        the host. Returns {"columns": on, "ic", "rank_ic", "long",
        "short": (D, P) float64, "count": (D, P) int32} as host tensors in
        input-day order; definitions in factorvae_amd.metrics. Rows whose
        prediction or label is not finite are left out and `count` is the
        number of rows used; a day longer than 8192 stocks is reported as
        count = -1 with NaN values. Like predict_many it touches no
        training buffer, captured graph or in-graph RNG state.

        with_loss=True also runs loss_many's posterior steps on each chunk,
        behind the prior decoder, so the extractor, the GRU and the prior
        attention run once for both; the result gains "loss", "mse", "kl":
        (D,) float32 as loss_many returns them. The posterior
        reconstruction uses the same per-stock eps as the "score" column;
        when eps is None it is then drawn even for a mu-only evaluation."""
        from ..metrics import check_columns

        on = check_columns(on)
        topk = int(topk)
        if topk < 0:
            raise ValueError(f"topk must be >= 0, got {topk}")
        xs, ys, lens_all = self._pm_split_days("evaluate_many", days)
        if eps is not None:
            eps = list(eps)
        D_all, P = len(lens_all), len(on)
        stats = torch.full((D_all, P, 4), float("nan"), dtype=torch.float64)
        count = torch.zeros(D_all, P, dtype=torch.int32)
        # rows of iw["out"]: sample, mu, sigma
        row = {"score": 0, "mu": 1}
        r_lo = min(row[c] for c in on)
        r_hi = max(row[c] for c in on) + 1
        col = [row[c] - r_lo for c in on]
        Pk = r_hi - r_lo
        lmk = torch.full((3, D_all), float("nan")) if with_loss else None
        for idxs, lens, offs, iw in self._pm_chunks(
                "evaluate_many", xs, eps, max_rows, False, ys=ys,
                draw_eps="score" in on or with_loss):
            if iw is None:
                continue  # days without rows: count 0, NaN
            D, Nn = len(idxs), offs[-1]
            if iw.get("ic_cap", 0) < D * Pk:
                iw["ic_stats"] = torch.empty(D * Pk * 4, device=self.device,
                                             dtype=torch.float64)
                iw["ic_count"] = torch.empty(D * Pk, device=self.device,
                                             dtype=torch.int32)
                iw["ic_cap"] = D * Pk
            st, cn = iw["ic_stats"][:D * Pk * 4], iw["ic_count"][:D * Pk]
            self.ext.daily_ic_seg(iw["out"][r_lo:r_hi, :Nn],
                                  iw["label"][:Nn], iw["seg_off"][:D + 1],
                                  min(max(lens), self.EVAL_MAX_N), topk, st,
                                  cn)
            if with_loss:
                # launched ahead of the copies below, which wait
                post = self._launch_posterior(iw, Nn, D, max(lens), False)
            st_h = st.cpu().view(D, Pk, 4)[:, col]
            cn_h = cn.cpu().view(D, Pk)[:, col]
            ii = torch.tensor(idxs)
            stats[ii] = st_h
            count[ii] = cn_h
            if with_loss:
                lmk[:, ii] = post.cpu().view(3, D)
        res = {"columns": on, "ic": stats[:, :, 0].clone(),
               "rank_ic": stats[:, :, 1].clone(),
               "long": stats[:, :, 2].clone(),
               "short": stats[:, :, 3].clone(), "count": count}
        if with_loss:
            res["loss"], res["mse"], res["kl"] = (lmk[0].clone(),
                                                  lmk[1].clone(),
                                                  lmk[2].clone())
        return res

    @torch.no_grad()
    def validate_metrics(self, days, topk: int = 0, with_loss: bool = False):
        """Summary of evaluate_many on the predictive mean, dropout off:
        {"IC", "ICIR", "RankIC", "RankIC_IR", "long_short", "n_days"}
        (metrics.summarize_ic: means over the days with a finite value,
        IR = mean / std with ddof=0). with_loss=True adds "loss": the
        float64 mean of the finite per-day validation losses of the same
        pass (evaluate_many(with_loss=True); 0.0 without any)."""
        from ..metrics import summarize_ic

        was = self.training
        self.training = False
        try:
            per_day = self.evaluate_many(days, on=("mu",), topk=topk,
                                         with_loss=with_loss)
        finally:
            self.training = was
        out = summarize_ic({k: per_day[k].numpy()
                            for k in ("ic", "rank_ic", "long", "short")})
        if with_loss:
            loss = per_day["loss"].double()
            loss = loss[torch.isfinite(loss)]
            out["loss"] = float(loss.mean()) if loss.numel() else 0.0
        return out

    # ------------------------------------------------------------- epochs
    # steps per multi-step training graph (real-epoch batching)
    TRAIN_GRAPH_STEPS = 8

    def _get_multi_graph(self, N: int, T: int, g_len: int):
        """A captured graph of g_len full training steps reading from
        per-slot input buffers, with in-graph per-step loss
        accumulation into `lsum` — one replay per g_len days removes
        the per-day replay/launch host overhead from real epochs."""
        key = ("trainG", N, T, g_len)
        plan = self._graphs.get(key)
        if plan is not None:
            return plan
        w = self.ws
        xb = [torch.empty_like(w["x"]) for _ in range(g_len)]
        yb = [torch.empty_like(w["y"]) for _ in range(g_len)]
        lsum = torch.zeros(1, device=self.device)
        # warmup (params/step counter untouched)
        torch.cuda.synchronize(self.device)
        with self._main_ctx():
            self._fill_rng(N)
            self._launch_forward(N, T, x=xb[0], y=yb[0], train=True)
            self._launch_backward(N, T, x=xb[0], y=yb[0])
        torch.cuda.synchronize(self.device)
        try:
            with self._abort_watchdog("train multi-step graph capture"):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=self.s_main):
                    for i in range(g_len):
                        self._graph_step_body(xb[i], yb[i], N, T, True,
                                              is_distributed())
                        lsum += w["loss"]
        except Exception:
            torch.cuda.synchronize(self.device)
            plan = {"g": None}
            self._graphs[key] = plan
            return plan
        plan = {"g": g, "xb": xb, "yb": yb, "lsum": lsum}
        self._graphs[key] = plan
        return plan

    def train_epoch(self, days, shuffle_order=None) -> float:
        """One epoch over device-resident day tensors. Runs of
        TRAIN_GRAPH_STEPS consecutive same-shape days execute as ONE
        multi-step graph replay (in-graph RNG + loss accumulation);
        ragged leftovers fall back to the per-day step graph."""
        total = torch.zeros((), device=self.device)
        n = 0
        days = list(days)
        G = self.TRAIN_GRAPH_STEPS
        rng_ok, comm_ok = (self._probe_caps()
                           if (self.use_graph and self.device.type == "cuda")
                           else (False, False))
        use_multi = (self.use_graph and rng_ok and G > 1
                     and not (is_distributed() and not comm_ok)
                     and len(days) > 0
                     and days[0][0].numel() * 4 <= 16 << 20)
        # (size gate: the per-slot D2D input copies must stay well under
        # the ~20 us/step host replay overhead the batching removes —
        # big A-share days fall back to per-day replays)
        i = 0
        while i < len(days):
            x, y = days[i]
            run = 1
            if use_multi:
                while (run < G and i + run < len(days)
                       and days[i + run][0].shape == x.shape):
                    run += 1
            if use_multi and run == G:
                N, T, C = x.shape
                self._ensure_ws(N, T)
                plan = self._get_multi_graph(N, T, G)
                if plan["g"] is not None:
                    self._main_entry()
                    with self._main_ctx():
                        for j in range(G):
                            plan["xb"][j].copy_(days[i + j][0])
                            plan["yb"][j].copy_(days[i + j][1].view(-1, 1))
                        plan["lsum"].zero_()
                        plan["g"].replay()
                        total += plan["lsum"][0]
                    self._main_exit()
                    n += G
                    i += G
                    continue
            loss = self.step(x, y)
            total += loss[0]
            n += 1
            i += 1
        return (total / max(n, 1)).item()

    # ------------------------------------------------- optimizer side-car
    def opt_state_dict(self) -> Dict:
        """Optimizer/scheduler state for true resume (the reference saves
        only model weights, /root/reference/main.py:79 — SURVEY.md §5.4
        calls out the side-car as a new-engine addition)."""
        return {
            "adam_m": self.adam_m.detach().cpu(),
            "adam_v": self.adam_v.detach().cpu(),
            "step_t": self.step_t.detach().cpu(),
            "lr": self.lr,
            "eta_min": self.eta_min,
            "t_max": self.t_max,
        }

    def load_opt_state_dict(self, sd: Dict) -> None:
        self.adam_m.copy_(sd["adam_m"].to(self.device))
        self.adam_v.copy_(sd["adam_v"].to(self.device))
        self.step_t.copy_(sd["step_t"].to(self.device))
        self.lr = float(sd.get("lr", self.lr))
        self.eta_min = float(sd.get("eta_min", self.eta_min))
        self.t_max = int(sd.get("t_max", self.t_max))
        # lr/t_max are baked into captured graphs as kernel args
        self._graphs.clear()
        if self.bf16:  # weights typically re-loaded alongside opt state
            self._refresh_bf16_shadows()

    @torch.no_grad()
    def validate_epoch(self, days, batched: bool = False) -> float:
        """Mean validation loss over the days, dropout off. The default
        route replays the training-shaped forward once per day.
        batched=True goes through loss_many instead and returns the
        float64 host mean of its per-day losses over the days with rows
        (the fp8 engine, which loss_many refuses, keeps the per-day loop).
        The two routes draw their decoder noise from different streams
        (the per-day workspace's in-graph RNG fill against one normal_()
        per packed chunk): they agree in distribution, not in value."""
        if batched and not self.fp8:
            r = self.loss_many(days)
            loss = r["loss"][r["n"] > 0].double()
            return float(loss.mean()) if loss.numel() else 0.0
        was = self.training
        self.training = False
        total = torch.zeros((), device=self.device)
        n = 0
        try:
            for x, y in days:
                loss = self.forward_only(x, y)
                total += loss[0]
                n += 1
        finally:
            self.training = was
        return (total / max(n, 1)).item()
