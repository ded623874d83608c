"""AdamW for the MolKGNN training step, one HIP launch for the whole model (``mkgnn_adamw_step``).

The reference builds ``torch.optim.AdamW`` over two parameter groups (``model.py:368-385``).  This class keeps that
interface -- ``param_groups`` with ``lr`` / ``betas`` / ``eps`` / ``weight_decay`` / ``maximize``, per-parameter state
``step`` / ``exp_avg`` / ``exp_avg_sq``, ``state_dict`` round trips, parameters without a gradient skipped -- and the
same update formula; the ~80 small tensors of the model are updated by one kernel instead of PyTorch's five
(``csrc/kgnn_optim.hip``).  The step counters live on the device, so a step can be captured in a hipGraph; a
learning-rate schedule reaches a captured step through ``lr`` given as a 0-dim CUDA tensor that the scheduler fills.
fp32 CUDA parameters only; no CPU path (``MolKGNNLibraryError`` otherwise).

``max_grad_norm`` / ``skip_nonfinite`` (both off by default: the step above, the same launch and the same bits) clip the
gradients by their global norm and skip a step whose norm is not finite, inside the step and on the device
(``mkgnn_adamw_step_clipped``): one more launch, nothing read back, capturable.

``average='ema' | 'mean'`` (off by default: the steps above, the same launches, bits and state size) keeps an average of the
weights inside the same launch (``mkgnn_adamw_step_averaged``): ``state[p]['param_avg']`` / ``['n_averaged']``,
``averaged_parameters()``, ``swap_averaged()`` and the context manager ``averaged_weights()``.
"""
from __future__ import annotations

import contextlib
import math
from typing import List

import torch

from . import _lib


class FusedAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, maximize: bool = False,
                 grad_scale: float = 1.0, max_grad_norm=None, skip_nonfinite: bool = False, average=None,
                 average_decay: float = 0.999, average_warmup: bool = True, average_start: int = 0):
        """``max_grad_norm``: the gradients of one step are scaled by ``min(1, max_grad_norm / (norm + 1e-6))``, ``norm`` the
        2-norm of ALL gradients the step reads, across the parameter groups, each after its group's ``maximize`` and
        ``grad_scale`` -- ``torch.nn.utils.clip_grad_norm_``'s coefficient.  Unlike ``clip_grad_norm_`` the clip lives in the
        step: ``.grad`` is NOT written back, a gradient read after ``step()`` is the unclipped one.  ``skip_nonfinite``: a step
        whose norm is ``inf`` or NaN does not happen -- no parameter, moment or step count changes by a bit, and
        ``skipped_steps`` goes up by one; decided on the device, so it works in a captured step.  Without it a non-finite norm
        does what torch does (an infinite norm zeroes the finite gradients and turns the infinite ones into NaN; a NaN norm turns
        all of them into NaN).  ``max_grad_norm=None`` with the guard on: the norm and the guard, no clipping.  ``grad_norm``
        (the norm before clipping), ``clip_coef`` and ``skipped_steps`` are 0-dim CUDA tensors filled by the step; reading them
        does not synchronise until their value is asked for.  Both settings are attributes of the optimiser, not keys of
        ``param_groups`` (the norm spans the groups): ``state_dict()`` does not carry them.

        ``average``: ``'ema'`` or ``'mean'`` keeps, per parameter, an average of the iterates in ``state[p]['param_avg']`` with the
        number of iterates in it in ``state[p]['n_averaged']`` -- ``torch.optim.swa_utils.AveragedModel``'s update, made inside the
        step's launch.  A parameter's step that does not happen (no gradient, an active flag of 0, a step ``skip_nonfinite``
        skipped) is not averaged.  Until a parameter's step count exceeds ``average_start`` its average tracks it.  ``'ema'``:
        ``avg += (1 - d) (p - avg)`` with ``d = average_decay`` or, with ``average_warmup``, ``min(average_decay, (1 + n) /
        (10 + n))``; ``'mean'``: ``avg += (p - avg) / (n + 1)``.  Only parameters are averaged: buffers (the batch-norm
        running statistics) are the live model's.  Settings of the optimiser, not of its groups; the two state entries travel in
        ``state_dict()``."""
        if not isinstance(lr, torch.Tensor) and lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid betas: {betas}")
        if eps < 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        # grad_scale: every gradient is multiplied by it first -- 1 / world after a summing all-reduce, so that the
        # averaging costs no kernel of its own (default 1: torch.optim.AdamW's update)
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, maximize=maximize,
                                      grad_scale=grad_scale))
        if len(self.param_groups) > 4:
            raise ValueError("FusedAdamW takes at most 4 parameter groups")
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0.0:                      # (a NaN is refused here as well)
                raise ValueError(f"Invalid max_grad_norm: {max_grad_norm} (> 0, or None)")
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = bool(skip_nonfinite)
        if average not in (None, "ema", "mean"):
            raise ValueError(f"Invalid average: {average!r} (None, 'ema' or 'mean')")
        average_decay = float(average_decay)
        if not 0.0 <= average_decay < 1.0:                   # (a NaN is refused here as well)
            raise ValueError(f"Invalid average_decay: {average_decay} (0 <= decay < 1)")
        if int(average_start) != average_start or average_start < 0:
            raise ValueError(f"Invalid average_start: {average_start} (an integer >= 0)")
        self.average = average
        self.average_decay, self.average_warmup, self.average_start = average_decay, bool(average_warmup), int(average_start)
        self._in_averaged = False                            # inside averaged_weights(): the parameters hold the averages
        self._swap_key = None
        self._swap_table = None
        self._clip_stats = None                              # [norm, coef, skipped steps, reserved] on the device
        self._clip_ws = None                                 # one double per 1024-element block of the table, and one more
        self._clip_need = 0
        self._table_key = None
        self._table = None
        self._active: dict = {}
        # per-parameter constants of step() -- group, packed-state pointer, element count, active-flag pointer -- looked up once
        # and kept while nothing that determines them changes (an eager step of this model is host-bound: ~80 tensors)
        self._fast: list = []
        self._fast_sig = None
        self._ver = 0

    def set_grad_active(self, flags: dict) -> None:
        """``{parameter: one-element float32 CUDA tensor}``: a parameter whose flag reads 0 when the step runs is
        skipped (as if its gradient were ``None``) -- decided on the device, so a captured data-parallel step skips the
        banks of a degree that no rank's batch contained (``dp.FlatGradAllReduce.active_flags``)."""
        for p, f in flags.items():
            if not (isinstance(f, torch.Tensor) and f.is_cuda and f.dtype == torch.float32 and f.numel() == 1):
                raise ValueError("an active flag must be one float32 element on the GPU")
        self._active = dict(flags)
        self._table_key = None
        self._ver += 1
        self.prepare_state(list(flags))                      # flagged parameters are stepped on the device's say-so: state must exist

    # -- clipping: workspace and stats of mkgnn_adamw_step_clipped --
    @property
    def clipping(self) -> bool:
        return self.max_grad_norm is not None or self.skip_nonfinite

    def _clip_buffers(self, dev, need: int):
        """(workspace, stats) on ``dev``, the workspace of at least ``need`` bytes; allocated outside any capture."""
        if self._clip_stats is None or self._clip_stats.device != dev or self._clip_ws.numel() * 8 < need:
            if torch.cuda.is_current_stream_capturing():
                # (a zero fill of the stats recorded into a graph would reset skipped_steps at every replay)
                raise _lib.MolKGNNLibraryError(
                    "FusedAdamW: the clipping workspace would be allocated inside a hipGraph capture -- call prepare_state() (or "
                    "run one eager step in which every parameter has a gradient) before capturing")
            if self._clip_stats is None or self._clip_stats.device != dev:
                self._clip_stats = torch.zeros(4, dtype=torch.float32, device=dev)
            self._clip_ws = torch.empty(max(need, 8) // 8, dtype=torch.float64, device=dev)
        return self._clip_ws, self._clip_stats

    def _stat(self, i: int) -> torch.Tensor:
        if not self.clipping:
            raise RuntimeError("FusedAdamW: grad_norm / clip_coef / skipped_steps exist with max_grad_norm or skip_nonfinite set")
        if self._clip_stats is None:
            ps = [p for g in self.param_groups for p in g["params"] if p.numel()]
            if not ps:
                raise RuntimeError("FusedAdamW: no parameters")
            _lib.require_gpu_tensor(ps[0], "parameter")
            self._clip_buffers(ps[0].device, 8 * (sum((p.numel() + 1023) // 1024 for p in ps) + 1))
        return self._clip_stats[i]

    @property
    def grad_norm(self) -> torch.Tensor:
        """The global gradient norm of the last step before clipping (what ``clip_grad_norm_`` returns), a 0-dim CUDA tensor."""
        return self._stat(0)

    @property
    def clip_coef(self) -> torch.Tensor:
        """The coefficient the last step multiplied its gradients by, a 0-dim CUDA tensor."""
        return self._stat(1)

    @property
    def skipped_steps(self) -> torch.Tensor:
        """How many steps ``skip_nonfinite`` has skipped so far, a 0-dim CUDA tensor (float32)."""
        return self._stat(2)

    # -- state: one buffer per parameter, [exp_avg | exp_avg_sq | step | 2 reserved | a step count per 1024 elements]
    # (mkgnn_adamw_state_floats); the three state entries are views of it.  With averaging [param_avg | n_averaged | an
    # n_averaged per 1024 elements] (mkgnn_adamw_average_floats) follows in the same buffer, two more views --
    @staticmethod
    def _state_floats(n: int) -> int:
        return 2 * n + 3 + (n + 1023) // 1024

    @staticmethod
    def _average_floats(n: int) -> int:
        return n + 1 + (n + 1023) // 1024

    def _packed_floats(self, n: int) -> int:
        return self._state_floats(n) + (self._average_floats(n) if self.average is not None else 0)

    def _packed_state(self, p: torch.Tensor) -> torch.Tensor:
        st = self.state[p]
        n = p.numel()
        buf = st.get("_packed")
        if buf is not None and st["exp_avg"].data_ptr() == buf.data_ptr() and st["step"].data_ptr() == buf[2 * n:].data_ptr() and buf.numel() == self._packed_floats(n):
            if self.average is None or ("param_avg" in st and st["param_avg"].data_ptr() == buf[self._state_floats(n):].data_ptr()):
                return buf
        if p.is_cuda and torch.cuda.is_current_stream_capturing():
            # a zero fill recorded into a graph would reset exp_avg / exp_avg_sq / step at EVERY replay (and, data-parallel,
            # on this rank only: the replicas would drift apart silently)
            raise _lib.MolKGNNLibraryError(
                "FusedAdamW: optimiser state would be allocated inside a hipGraph capture -- call prepare_state() (or run "
                "one eager step in which every parameter has a gradient) before capturing")
        new = torch.zeros(self._packed_floats(n), dtype=torch.float32, device=p.device)
        if "exp_avg" in st:                                  # e.g. loaded from a state_dict (ours or torch.optim.AdamW's)
            new[:n] = st["exp_avg"].reshape(-1).to(new)
            new[n:2 * n] = st["exp_avg_sq"].reshape(-1).to(new)
            new[2 * n] = float(st["step"])
            new[2 * n + 3:self._state_floats(n)] = float(st["step"])     # (the update's per-block copies of the step count)
        st["_packed"] = new
        st["exp_avg"] = new[:n].view_as(p)
        st["exp_avg_sq"] = new[n:2 * n].view_as(p)
        st["step"] = new[2 * n:2 * n + 1].view(())
        if self.average is not None:
            off = self._state_floats(n)
            if "param_avg" in st and "n_averaged" in st:     # loaded, or carried over from a buffer that is being replaced
                new[off:off + n] = st["param_avg"].reshape(-1).to(new)
                new[off + n:] = float(st["n_averaged"])      # (the canonical count and the update's per-block copies)
            else:                                            # a fresh average: the parameter itself, nothing averaged yet
                new[off:off + n] = p.detach().reshape(-1)
            st["param_avg"] = new[off:off + n].view_as(p)
            st["n_averaged"] = new[off + n:off + n + 1].view(())
        else:                                                # (a state saved by an averaging optimiser, loaded into one that is not)
            st.pop("param_avg", None)
            st.pop("n_averaged", None)
        self._table_key = None
        self._ver += 1
        return new

    @torch.no_grad()
    def prepare_state(self, params=None) -> None:
        """Materialise the packed state of ``params`` (default: every parameter of every group) now, outside any capture:
        a parameter whose gradient is absent in the eager warm-up steps -- a degree bank that this rank's warm-up batches do
        not contain -- must not get its zero-filled state as a node of a captured graph (``_packed_state`` refuses)."""
        for p in (params if params is not None else [q for g in self.param_groups for q in g["params"]]):
            if p.numel():
                _lib.require_gpu_tensor(p, "parameter")
                self._packed_state(p)
        if self.clipping:                                    # the workspace of a step in which every parameter has a gradient
            self._stat(0)

    def state_dict(self):
        sd = super().state_dict()                            # the packed buffer is an implementation detail: its three views are saved
        sd["state"] = {k: {kk: vv for kk, vv in v.items() if kk != "_packed"} for k, v in sd["state"].items()}
        return sd

    @torch.no_grad()
    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._ver += 1
        for p in list(self.state):                           # pack now: torch may hand over the caller's tensors uncopied
            if isinstance(p, torch.Tensor) and "exp_avg" in self.state[p]:
                self.state[p].pop("_packed", None)
                self._packed_state(p)

    # -- the average of the weights --
    def _require_average(self, who: str) -> None:
        if self.average is None:
            raise RuntimeError(f"FusedAdamW.{who}: the optimiser was built without average='ema' | 'mean'")

    def averaged_parameters(self) -> dict:
        """``{parameter: its average}`` for every parameter that has state, each a view of the optimiser's state shaped like the
        parameter (``prepare_state()`` gives every parameter state)."""
        self._require_average("averaged_parameters")
        return {p: st["param_avg"] for p, st in self.state.items() if "_packed" in st and "param_avg" in st}

    @torch.no_grad()
    def swap_averaged(self) -> None:
        """Exchange every parameter that has state with its average, in place, in one launch (``mkgnn_flat_swap``): the model then
        computes with the averaged weights, and a second call restores it bit for bit.  Capturable.  The parameters' storage does
        not move, so a captured training step stays valid; stepping while swapped would train the average -- use
        ``averaged_weights()``, which refuses that."""
        self._require_average("swap_averaged")
        pairs = [(p, a) for p, a in self.averaged_parameters().items() if p.numel()]
        if not pairs:
            return
        key = tuple((p.data_ptr(), a.data_ptr(), p.numel()) for p, a in pairs)
        if key != self._swap_key:
            dev = pairs[0][0].device
            for p, _ in pairs:
                _lib.require_gpu_tensor(p, "parameter")
                if p.dtype != torch.float32 or not p.is_contiguous() or p.device != dev:
                    raise _lib.MolKGNNLibraryError("FusedAdamW needs contiguous float32 parameters on one device")
            table = (_lib.SwapItem * len(key))()
            for e, (a, b, n) in zip(table, key):
                e.a, e.b, e.numel = a, b, n
            self._swap_table, self._swap_key = table, key
        dev = pairs[0][0].device
        lib = _lib.load()
        with torch.cuda.device(dev):
            _lib.check(lib.mkgnn_flat_swap(self._swap_table, len(key), _lib.stream_ptr(dev)), "mkgnn_flat_swap")

    @contextlib.contextmanager
    def averaged_weights(self):
        """``with opt.averaged_weights(): ...`` -- the parameters hold their averages inside the block (``swap_averaged()`` on
        entry) and their live values again after it, also when the block raises.  ``step()`` inside the block raises."""
        self._require_average("averaged_weights")
        if self._in_averaged:
            raise RuntimeError("FusedAdamW.averaged_weights: already inside averaged_weights()")
        self.swap_averaged()
        self._in_averaged = True
        try:
            yield self
        finally:
            self._in_averaged = False
            self.swap_averaged()

    @torch.no_grad()
    def step(self, closure=None):
        if self._in_averaged:
            raise RuntimeError("FusedAdamW.step inside averaged_weights(): the parameters hold the averages, a step would train them")
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        lib = _lib.load()
        rows: List[tuple] = []
        keep = []                                            # tensors the enqueued kernel reads: referenced until the call returns
        dev = None
        sig = (self._ver, tuple(len(g["params"]) for g in self.param_groups), self.average)
        if sig != self._fast_sig:                            # (param_groups, state or flags changed: look everything up again)
            self._fast = [[p, gi, None, p.numel(), None] for gi, group in enumerate(self.param_groups) for p in group["params"] if p.numel()]
            self._fast_sig = sig
        for ent in self._fast:
            p = ent[0]
            g = p.grad
            if g is None:
                continue
            if ent[2] is None or ent[2][1] != p.data_ptr():  # first step with a gradient (or the parameter's storage moved)
                _lib.require_gpu_tensor(p, "parameter")
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise _lib.MolKGNNLibraryError("FusedAdamW needs contiguous float32 parameters")
                ver = self._ver
                st_ptr = self._packed_state(p).data_ptr()    # (may allocate: bumps _ver, the list is rebuilt next step)
                act = self._active.get(p)
                ent[2], ent[4] = (st_ptr, p.data_ptr()), (None if act is None else act.data_ptr())
                if ver != self._ver:
                    self._fast_sig = None
            else:
                # a state entry replaced -- or the whole state cleared -- from outside (not through load_state_dict)
                ea = self.state[p].get("exp_avg")
                if ea is None or ea.data_ptr() != ent[2][0]:
                    ent[2] = (self._packed_state(p).data_ptr(), p.data_ptr())
            if g.is_sparse:
                raise RuntimeError("FusedAdamW does not support sparse gradients")
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = g.float().contiguous()
                keep.append(g)
            if dev is None:
                dev = p.device
            elif p.device != dev:
                raise _lib.MolKGNNLibraryError("FusedAdamW: parameters on more than one device")
            rows.append((ent[2][1], g.data_ptr(), ent[2][0], ent[3], ent[1], ent[4]))
        if not rows:
            return loss
        key = tuple(rows)
        if key != self._table_key:                           # pointers are stable from step to step: build the table once
            table = (_lib.AdamWTensor * len(rows))()
            for e, r in zip(table, rows):
                e.param, e.grad, e.state, e.numel, e.group, e.active = r
            self._table, self._table_key = table, key
            self._clip_need = int(lib.mkgnn_adamw_clip_workspace_bytes(table, len(rows))) if self.clipping else 0
        groups = (_lib.AdamWGroup * len(self.param_groups))()
        for e, group in zip(groups, self.param_groups):
            lr = group["lr"]
            if isinstance(lr, torch.Tensor):
                if lr.is_cuda:
                    if lr.dtype != torch.float32 or lr.numel() != 1:
                        raise ValueError("a tensor lr must be one float32 element")
                    e.lr_device, e.lr = lr.data_ptr(), 0.0
                else:
                    e.lr_device, e.lr = None, float(lr)
            else:
                e.lr_device, e.lr = None, float(lr)
            e.beta1, e.beta2 = float(group["betas"][0]), float(group["betas"][1])
            e.eps, e.weight_decay, e.maximize = float(group["eps"]), float(group["weight_decay"]), int(bool(group["maximize"]))
            e.grad_scale = float(group.get("grad_scale", 1.0))
        avg = None
        if self.average is not None:
            avg = _lib.AdamWAverage(_lib.ADAMW_AVERAGE_EMA if self.average == "ema" else _lib.ADAMW_AVERAGE_MEAN, self.average_decay,
                                    int(self.average_warmup), self.average_start)
        with torch.cuda.device(dev):
            if not self.clipping:
                if avg is None:
                    _lib.check(lib.mkgnn_adamw_step(self._table, len(rows), groups, len(groups), _lib.stream_ptr(dev)),
                               "mkgnn_adamw_step")
                else:                                        # (+inf, no guard, no stats: the unclipped step, one launch)
                    _lib.check(lib.mkgnn_adamw_step_averaged(self._table, len(rows), groups, len(groups), avg, math.inf, 0, None, 0,
                                                             None, _lib.stream_ptr(dev)), "mkgnn_adamw_step_averaged")
            else:
                if not self._clip_need:                      # (the settings were switched on after the table was built)
                    self._clip_need = int(lib.mkgnn_adamw_clip_workspace_bytes(self._table, len(rows)))
                ws, stats = self._clip_buffers(dev, self._clip_need)
                max_norm = math.inf if self.max_grad_norm is None else float(self.max_grad_norm)
                if avg is not None:
                    _lib.check(lib.mkgnn_adamw_step_averaged(self._table, len(rows), groups, len(groups), avg, max_norm,
                                                             int(self.skip_nonfinite), ws.data_ptr(), ws.numel() * 8,
                                                             stats.data_ptr(), _lib.stream_ptr(dev)), "mkgnn_adamw_step_averaged")
                else:
                    _lib.check(lib.mkgnn_adamw_step_clipped(self._table, len(rows), groups, len(groups), max_norm,
                                                            int(self.skip_nonfinite), ws.data_ptr(), ws.numel() * 8, stats.data_ptr(),
                                                            _lib.stream_ptr(dev)), "mkgnn_adamw_step_clipped")
        del keep
        return loss
