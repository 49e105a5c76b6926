"""FusedOnPolicyStep: the entire IMPALA/PPO/PPO-C/V-MPO training iteration
as a fixed HIP kernel DAG, bypassing autograd, with optional hipGraph
capture.

The loss math has ONE implementation — the row-local device functions of
csrc/loss_row.h (plus V-MPO's cross-row vmpo_mid) — reached by three launch
sequences:

Row step (H=64, IMPALA / PPO / PPO-C, at most one batch row per CU; the
default; profiles/row_step.md):
  1. seq_lstm_row_step  — per batch row, in ONE launch: forward, the row's
                          loss phase (V-trace/GAE scans, analytic head
                          grads, per-row stat partials) and BPTT. Nothing
                          in it crosses rows, so no launch boundary
  2. seq_lstm_wgrad_out — MFMA weight-grad GEMMs written DIRECTLY into the
                          flat grad buffer's parameter views; one extra
                          block reduces the stat partials
  3. rmsprop/adam       — fused clip + update
     [world > 1: RCCL all-reduce of the flat bucket before the update]

Fused pair (H=64: V-MPO, whose middle kernel IS cross-row; the others with
more rows than CUs, where the row step measured slower):
  1. seq_lstm_fwd_loss  — forward + the log-softmax + GAE pre-phase
  2. vmpo_mid           — single-block cross-row kernel (radix-256 top-half
                          selection, psi softmax, eta/alpha duals, stats)
  3. seq_lstm_bwd_fin   — the analytic grad emission + BPTT per row (for
                          the other algorithms: stat-partial reduce in
                          block 0 + BPTT; kept as the row step's reference)
  4-5. seq_lstm_wgrad_out and the optimizer, as above

Separate launches (H=32/128, or PDRL_FWDLOSS=0 at H=64): the same device
functions behind their own thin launches —
  seq_lstm_forward → onpolicy_loss_rows → onpolicy_stats_fin
  (V-MPO: vmpo_mid → vmpo_grad_rows) → seq_lstm_backward_core
— then the weight-grad and optimizer launches as above.

No host syncs anywhere; stats are read back only at the log interval.
With hipGraph capture (`use_graph`), the whole step replays as one graph
launch — single-rank; multi-rank splits into two graphs around the
stream-ordered collective (see run()). The launch-overhead answer to the
reference's ~hundreds of eager dispatches per iteration.
"""
from __future__ import annotations

import os
import warnings

import torch

from . import ext

_IMPALA_STATS = ["loss-total", "loss-policy", "loss-value", "entropy", "rho-avg"]
_PPO_STATS = [
    "loss-total", "loss-policy", "loss-value", "entropy",
    "ratio-avg", "ratio-min", "ratio-max",
]
_VMPO_STATS = ["loss-total", "loss-policy", "loss-value", "eta", "alpha", "kl"]

BATCH_FIELDS = ["obs", "act", "rew", "logits", "log_prob", "is_fir", "hx", "cx"]

_ALGO_ID = {"IMPALA": 0, "PPO": 1, "PPO-C": 2, "V-MPO": 3}  # csrc/loss_row.h
_WGRAD_MAX_ROWS = 8192          # row-pointer table of the wgrad kernels (LDS)
_ROW_STEP_MAX_LDS_BYTES = 64 * 1024  # dynamic LDS of one launch
_VMPO_MID_LDS_BYTES = 56 * 1024  # vmpo_mid keeps s_adv + s_psi (BT each) in LDS


class GraphableStep:
    """Capture/replay scaffolding shared by the fused step DAGs: first run
    captures the kernel sequence on the caller's tensors; later runs replay
    (copying only fields whose storage moved)."""

    use_graph: bool = True
    _graph = None
    _static = None
    _graph_failed = False
    stat_names: list = []
    stats_buf = None
    params = None

    def _full(self, batch):  # implemented by subclasses
        raise NotImplementedError

    def _pin_and_warm(self, batch):
        """Pin the caller's tensors as the graph inputs and run the step a
        few times on a side stream (allocator + RCCL channel warmup)."""
        self._static = {k: batch[k] for k in BATCH_FIELDS}
        self._static_ptrs = {k: batch[k].data_ptr() for k in BATCH_FIELDS}
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(3):
                self._full(self._static)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()

    def _restage(self, batch):
        """Refresh the pinned graph inputs whose storage moved."""
        for k in BATCH_FIELDS:
            if batch[k].data_ptr() != self._static_ptrs[k]:
                self._static[k].copy_(batch[k], non_blocking=True)

    def _stats(self) -> dict:
        return {name: self.stats_buf[i] for i, name in enumerate(self.stat_names)}

    def _try_capture(self, batch):
        try:
            self._pin_and_warm(batch)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._full(self._static)
            self._graph = g
        except Exception as exc:  # capture unsupported → stream-ordered path
            warnings.warn(f"hipGraph capture failed ({exc}); running the fused "
                          "step stream-ordered instead")
            self._graph_failed = True
            self._static = None

    def run(self, batch) -> dict:
        if self.use_graph and self._graph is None and not self._graph_failed:
            self._try_capture(batch)
        if self._graph is not None:
            self._restage(batch)
            self._graph.replay()
        else:
            self._full(batch)
        return self._stats()


class FusedOnPolicyStep(GraphableStep):
    _ws_shape = None
    _n_cus = None
    _split_graphs = None
    _split_failed = False

    def __init__(self, algo: str, core, params, optimizer, grad_reducer=None,
                 use_graph: bool = True, duals=None):
        assert algo in _ALGO_ID
        self.algo = algo
        self.core = core
        self.params = params
        self.optimizer = optimizer
        self.grad_reducer = grad_reducer
        self.A = int(params.n_actions)
        dev = core.body_w.device
        self.stats_buf = torch.zeros(8, dtype=torch.float32, device=dev)
        self.stat_names = {"IMPALA": _IMPALA_STATS, "PPO": _PPO_STATS,
                           "V-MPO": _VMPO_STATS, "PPO-C": _PPO_STATS}[algo]
        self.duals = duals  # (log_eta, log_alpha) params for V-MPO
        if algo == "V-MPO":
            assert duals is not None
            self.rng_state = torch.randint(
                1, 2**31 - 1, (1,), dtype=torch.int32, device=dev)
        # fwd_loss / bwd_fin are specialized for the H=64 model family;
        # PDRL_FWDLOSS=0 selects the separate launches there too
        self.fused_rows = core.w_ih.size(0) == 64 and bool(
            int(os.environ.get("PDRL_FWDLOSS", "1")))
        # forward + loss + BPTT in one launch wherever nothing crosses rows
        self.row_step = self.fused_rows and algo != "V-MPO"
        self.use_graph = use_graph
        self._graph = None
        self._static: dict[str, torch.Tensor] | None = None
        self._graph_failed = False

    # ------------------------------------------------------------------ #
    def _norm_buf(self):
        """The optimizer's device-resident ||grad||² scalar (zeroed by the
        loss phase, accumulated by the wgrad kernels in single-rank mode)."""
        if self.grad_reducer is not None:
            return None  # post-allreduce norm is computed by optimizer.step()
        return self.optimizer.norm_sq

    def _grad_views(self):
        c = self.core
        ps = [c.body_w, c.body_b, c.w_ih, c.w_hh, c.b_g, c.heads_w, c.heads_b]
        gs = [p.grad for p in ps]
        assert all(g is not None for g in gs), "flat grad views missing"
        # wgrad_out writes (dw_ih, dw_hh, dbody_w, dbody_b, db_g, dheads_w, dheads_b)
        return [gs[2], gs[3], gs[0], gs[1], gs[4], gs[5], gs[6]]

    def fits(self, batch) -> bool:
        """Whether the fused step covers this shape; updaters fall back to
        eager autograd when it does not. The row-local losses have no shape
        cap of their own."""
        B, S, _ = batch["obs"].shape
        if B * S > _WGRAD_MAX_ROWS:
            return False
        if self.algo == "V-MPO":
            return 2 * B * (S - 1) * 4 <= _VMPO_MID_LDS_BYTES
        return True

    def compute_grads_only(self, batch):
        """Everything but the optimizer (for gradient parity tests): fills
        the flat grad buffer and the stats vector."""
        self._body(batch, update=False)

    # ------------------------------------------------------------------ #
    def _workspace(self, B, S):
        """Persistent device scratch for one (B, S): head grads, per-row
        loss partials, V-MPO's inter-phase buffers and — fused rows only,
        the separate launches allocate their own — the activations."""
        if self._ws_shape == (B, S):
            return self._ws
        c = self.core
        dev = c.body_w.device
        H = c.w_ih.size(0)
        D = c.heads_w.size(1)

        def mk(*shape):
            return torch.empty(*shape, device=dev)

        ws = {"gouts": mk(B, S, D),
              "stats_part": mk(B, 8)}  # per-row loss partials (plain stores)
        if self.algo == "V-MPO":
            BT = B * (S - 1)
            ws.update({
                "vm_lse": mk(B * S), "vm_logp": mk(B * S),
                "vm_adv": mk(BT), "vm_td": mk(BT), "vm_psi": mk(BT),
                "vm_scalars": mk(8),
            })
        if self.fused_rows:
            ws.update({
                "outs": mk(B, S, D), "hS": mk(B, H), "cS": mk(B, H),
                "stash": mk(B, S, 7 * H),
                "dgates": mk(B, S, 4 * H), "dxb": mk(B, S, H),
            })
        self._ws, self._ws_shape = ws, (B, S)
        return ws

    def _runs_row_step(self, e, B, S, D) -> bool:
        """Whether this shape takes the one-launch row step; otherwise the
        two-launch pair runs (same results, bit for bit).
        - One block per CU at the most. The row step takes memory round
          trips off a block's critical path, which pays while every block
          has a CU to itself; it needs 175-207 VGPRs (2 blocks/CU, the pair's
          kernels fit 3), and with several blocks per CU it measured slower
          than the pair: +8.2 us at B=640, +5.6 us at B=1536. Measured on
          256 CUs: B=128 gains 4.3 us and B=256, the edge of this gate,
          3.5 us; no B between 256 and 640 was measured, so the true
          crossover is unknown (profiles/row_step.md).
        - It parks its loss inputs in LDS behind the forward's buffers;
          where that does not fit a launch, the pair still may."""
        if not self.row_step:
            return False
        if self._n_cus is None:
            self._n_cus = torch.cuda.get_device_properties(
                self.core.body_w.device).multi_processor_count
        return (B <= self._n_cus and e.seq_lstm_row_step_lds_bytes(
            S, D, _ALGO_ID[self.algo]) <= _ROW_STEP_MAX_LDS_BYTES)

    def _loss(self, e, batch, ws):
        """Forward, loss and BPTT for every row: fills ws["gouts"] and —
        except on the row step, which leaves the reduce to the wgrad launch
        — the stats vector. Returns (hx0, stash, dgates, dxb, stats_kw):
        the wgrad kernel's inputs and its stats-reduce arguments."""
        c, p = self.core, self.params
        x = batch["obs"]
        B, S, _ = x.shape
        D = c.heads_w.size(1)
        # strided row views (stride S*H) — the kernels take h0/c0 strides,
        # so no .contiguous() copies here
        hx0 = batch["hx"][:, 0]
        cx0 = batch["cx"][:, 0]
        act = batch["act"].reshape(-1)
        rew = batch["rew"].reshape(B, S)
        behav = batch["log_prob"].reshape(B, S)
        fir = batch["is_fir"].reshape(B, S)
        vmpo = self.algo == "V-MPO"
        algo_i = _ALGO_ID[self.algo]
        norm = self._norm_buf()
        gouts, part = ws["gouts"], ws["stats_part"]
        coefs = (p.policy_loss_coef, p.value_loss_coef, p.entropy_coef,
                 float(getattr(p, "logit_reg", 0.0)))  # cp, cv, ce, creg
        weights = (c.body_w, c.body_b, c.w_ih, c.w_hh, c.b_g, c.heads_w,
                   c.heads_b)
        bwd_weights = (c.body_w, c.w_ih, c.w_hh, c.heads_w)
        loss_args = (act, behav, rew, fir, gouts, part, norm, algo_i,
                     p.gamma, p.lmbda, 0.8, 0.1, 1.0, p.reward_scale,
                     *coefs[:3], p.eps_clip, coefs[3])
        pre = ({k: ws[k] for k in ("vm_lse", "vm_logp", "vm_adv", "vm_td")}
               if vmpo else {})

        if self._runs_row_step(e, B, S, D):
            e.seq_lstm_row_step(x, hx0, cx0, *weights, ws["outs"], ws["hS"],
                                ws["cS"], ws["stash"], act, behav, rew, fir,
                                gouts, part, norm, ws["dgates"], ws["dxb"],
                                *loss_args[7:])
            stats_kw = dict(stats_part=part, stats=self.stats_buf,
                            algo=algo_i, B=B, cp=coefs[0], cv=coefs[1],
                            ce=coefs[2], creg=coefs[3])
            return hx0, ws["stash"], ws["dgates"], ws["dxb"], stats_kw

        if self.fused_rows:
            outs, stash = ws["outs"], ws["stash"]
            e.seq_lstm_fwd_loss(x, hx0, cx0, *weights, outs, ws["hS"],
                                ws["cS"], stash, *loss_args, **pre)
        else:
            outs, _, _, stash = e.seq_lstm_forward(x, hx0, cx0, *weights)
            e.onpolicy_loss_rows(outs, *loss_args, **pre)

        grad = {}
        if vmpo:
            behav_logits = batch["logits"].reshape(B * S, self.A)
            log_eta, log_alpha = self.duals
            if not e.vmpo_mid(
                outs, behav_logits, ws["vm_logp"], ws["vm_lse"],
                ws["vm_adv"], ws["vm_td"], log_eta.data.view(1),
                log_alpha.data.view(1), ws["vm_psi"], ws["vm_scalars"],
                log_eta.grad.view(1), log_alpha.grad.view(1), self.stats_buf,
                norm, self.rng_state, self.A, coefs[0], coefs[1], coefs[3],
                p.coef_eta, p.coef_alpha_below, p.coef_alpha_upper,
            ):
                raise RuntimeError(
                    f"V-MPO batch ({B}, {S}) exceeds vmpo_mid's LDS; gate "
                    "on fits() and fall back to the eager step")
            grad = dict(act=act, behav=behav_logits, vm_lse=ws["vm_lse"],
                        vm_psi=ws["vm_psi"], vm_td=ws["vm_td"],
                        vm_scalars=ws["vm_scalars"])

        if self.fused_rows:
            dgates, dxb = ws["dgates"], ws["dxb"]
            if vmpo:
                grad["vm_outs"] = outs
            e.seq_lstm_bwd_fin(gouts, stash, x, cx0, *bwd_weights, dgates,
                               dxb, self.stats_buf, part, algo_i, *coefs,
                               **grad)
        else:
            if vmpo:  # stats were finalized by vmpo_mid
                e.vmpo_grad_rows(outs, gouts=gouts, cp=coefs[0], cv=coefs[1],
                                 creg=coefs[3], **grad)
            else:
                e.onpolicy_stats_fin(part, self.stats_buf, algo_i, B, S, D,
                                     *coefs)
            _, _, _, dgates, dxb = e.seq_lstm_backward_core(
                gouts, None, None, stash, x, cx0, *bwd_weights)
        return hx0, stash, dgates, dxb, {}

    def _body(self, batch, update: bool = True):
        e = ext()
        x = batch["obs"]
        ws = self._workspace(x.size(0), x.size(1))
        hx0, stash, dgates, dxb, stats_kw = self._loss(e, batch, ws)
        e.seq_lstm_wgrad_out(x, hx0, stash, dgates, dxb, ws["gouts"],
                             *self._grad_views(), self._norm_buf(),
                             **stats_kw)
        if not update:
            return
        if self.grad_reducer is not None:
            # multi-rank: norm must be of the AVERAGED grads → recompute
            self.grad_reducer.all_reduce([self.optimizer.flat_grad])
            self.optimizer.step()
        else:
            # single rank: ||grad||² was zeroed by the loss phase and
            # accumulated by the wgrad kernels — skip fill + l2norm launches
            self.optimizer._update()

    def _full(self, batch):
        for _ in range(self.params.K_epoch):
            self._body(batch)

    # -- multi-rank split-graph: capture [fwd..wgrad] and [optimizer] as
    # two graphs with the RCCL all-reduce stream-ordered between them.
    # Full capture WITH the collective (PDRL_GRAPH_RCCL=1) is faster but
    # cannot be validated on a single-GPU box; a bad replay would hang the
    # driver's one multi-GPU run, so the split is the default.
    def _try_capture_split(self, batch):
        self._split_failed = True
        if self.params.K_epoch != 1:
            return
        try:
            self._pin_and_warm(batch)
            g_pre = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_pre):
                self._body(self._static, update=False)
            g_post = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g_post):
                self.optimizer.step()
            self._split_graphs = (g_pre, g_post)
            self._split_failed = False
        except Exception as exc:
            warnings.warn(
                f"split-graph capture failed ({exc}); running the fused "
                "multi-rank step stream-ordered instead")
            self._static = None

    def run(self, batch) -> dict:
        if self.grad_reducer is None or not self.use_graph or bool(
                int(os.environ.get("PDRL_GRAPH_RCCL", "0"))):
            return super().run(batch)
        if self._split_graphs is None and not self._split_failed:
            self._try_capture_split(batch)
        if self._split_graphs is None:
            self._full(batch)
        else:
            self._restage(batch)
            g_pre, g_post = self._split_graphs
            g_pre.replay()
            self.grad_reducer.all_reduce([self.optimizer.flat_grad])
            g_post.replay()
        return self._stats()
