"""Optimiser / LR schedule with the reference's rules (``lib/solver/build.py:6-58``,
``lib/solver/lr_scheduler.py``): one param group per tensor, bias lr x
BIAS_LR_FACTOR and bias weight decay WEIGHT_DECAY_BIAS, Adam / AdamW / SGD, warm-up +
step / exp / poly / cosine / linear decay per epoch.

``FusedAdam`` and ``FusedSGD`` keep ``torch.optim.Adam``'s / ``torch.optim.SGD``'s
state layout and per-group hyper-parameters (so LR schedulers and checkpoints
work) but execute the whole step as ONE multi-tensor HIP kernel over a device
pointer table instead of one launch set per parameter group (the reference
builds 183 groups).
"""

from bisect import bisect_right
from math import cos, pi

import numpy as np
import torch

from . import ops

ADAM_CHUNK = 65536
# the SGD kernel moves 20 B per element against Adam's 28 with a fraction of the arithmetic: half the chunk gives the 45.1 M
# parameters ~1 500 blocks (six per CU) of 32 16-byte accesses per thread and array
SGD_CHUNK = 32768


class _FusedMultiTensor(torch.optim.Optimizer):
    """What the fused optimisers share: the device pointer tables and chunk map of ONE multi-tensor launch, the double-buffered
    pinned staging row of the per-step tables, and the table set / pinned ring of a recorded step.

    A per-step row is 3n + 1 eight-byte slots for n tensors: [n gradient pointers | 4 rows of n fp32] (lr, weight decay and
    two rows the subclass defines).  Subclasses set NAME, CHUNK, name their per-parameter state tensors (`_state_keys`) and
    the per-replay rows (`_replay_rows`)."""

    NAME = "fused optimizer"
    CHUNK = ADAM_CHUNK

    def __init__(self, params, defaults):
        super().__init__(params, defaults)
        self._plan = None  # device pointer tables; rebuilt whenever a parameter, gradient or state tensor moves

    def load_state_dict(self, state_dict):
        """The loaded state tensors replace the ones the cached pointer tables refer to."""
        super().load_state_dict(state_dict)
        self._plan = None

    def __setstate__(self, state):
        super().__setstate__(state)
        self._plan = None

    def _state_keys(self):
        raise NotImplementedError

    def _build(self, items):
        """Static part of the plan: parameter / state pointer tables and the chunk map (re-made only when a parameter
        or state tensor moves).  Gradient tensors are fresh allocations every step: their table goes up per step
        through pinned staging buffers with an asynchronous copy - a pageable host-to-device copy would wait for the
        whole backward pass and stop the host from running ahead of the GPU."""
        dev = items[0][0].device
        for p, g, st in items:
            if not (p.is_contiguous() or p.is_contiguous(memory_format=torch.channels_last)):
                raise RuntimeError("%s needs dense parameters" % self.NAME)
        ct, co = [], []
        for i, (p, _, _) in enumerate(items):
            for off in range(0, p.numel(), self.CHUNK):
                ct.append(i)
                co.append(off)
        n = len(items)

        def up(values, dtype):
            return torch.from_numpy(np.asarray(values, dtype=dtype)).to(dev)

        self._plan = {
            "key": self._key(items),
            "p": up(np.array([p.data_ptr() for p, _, _ in items], dtype=np.uint64).view(np.int64), np.int64),
            "state": [up(np.array([s[k].data_ptr() for _, _, s in items], dtype=np.uint64).view(np.int64), np.int64)
                      for k in self._state_keys()],
            "sizes": up([p.numel() for p, _, _ in items], np.int64),
            "ct": up(ct, np.int32),
            "co": up(co, np.int64),
            "n": len(ct),
            # per-step tables in one row of 8-byte slots: [n gradient pointers | 4 x n fp32], double-buffered
            "dyn": [torch.empty(3 * n + 1, dtype=torch.int64, device=dev) for _ in range(2)],
            "stage": [torch.empty(3 * n + 1, dtype=torch.int64).pin_memory() if dev.type == "cuda" else torch.empty(3 * n + 1, dtype=torch.int64)
                      for _ in range(2)],
            "done": [None, None],
            "turn": 0,
        }

    def _key(self, items):
        keys = self._state_keys()
        return tuple((p.data_ptr(),) + tuple(st[k].data_ptr() for k in keys) for p, _, st in items)

    def _upload(self, items, r0, r1, r2, r3):
        """This step's gradient pointers and four per-tensor fp32 rows -> device, without a host sync."""
        pl = self._plan
        n = len(items)
        k = pl["turn"]
        pl["turn"] = k ^ 1
        if pl["done"][k] is not None:
            pl["done"][k].synchronize()  # the copy issued two steps ago read this staging buffer (long finished)
        host = pl["stage"][k].numpy()
        host[:n] = np.array([g.data_ptr() for _, g, _ in items], dtype=np.uint64).view(np.int64)
        f = host[n:].view(np.float32)
        f[:n] = np.asarray(r0, dtype=np.float32)
        f[n : 2 * n] = np.asarray(r1, dtype=np.float32)
        f[2 * n : 3 * n] = np.asarray(r2, dtype=np.float32)
        f[3 * n : 4 * n] = np.asarray(r3, dtype=np.float32)
        dyn = pl["dyn"][k]
        dyn.copy_(pl["stage"][k], non_blocking=True)
        if dyn.is_cuda:
            ev = torch.cuda.Event()
            ev.record()
            pl["done"][k] = ev
        return dyn

    # ---- hipGraph capture (engine/graph.py): the step's kernel launch is recorded once and replayed.  Gradient tensors of
    # a captured backward live at fixed addresses, so their pointer table is written by ONE captured copy from a pinned
    # buffer that never changes afterwards; what changes from replay to replay - lr / weight decay of every group (LR
    # schedulers), Adam's per-parameter bias corrections, SGD's first-step encoding - lives in the tail of the same device
    # table and is refreshed by `advance_for_replay()` with a stream-ordered copy from a small ring of pinned buffers right
    # before each replay (no host sync, no captured host memory that changes).
    def prepare_capture(self, defer_table_copy=False):
        """OUTSIDE capture (pinned allocations are not capturable), after at least one eager step built the static
        pointer tables: the device / pinned tables of the captured step.
        defer_table_copy: the copy of the captured gradients' addresses to the device is NOT recorded; the caller runs it once,
        right after the recording ended, with finish_capture() (the addresses never change afterwards; a recorded host-to-device
        copy is the one node of the step that csrc/step_replay.hip cannot read back from the graph)."""
        if self._plan is None:
            raise RuntimeError("%s.prepare_capture(): run one eager step first (static pointer tables)" % self.NAME)
        pl = self._plan
        n = len(pl["sizes"])
        # one table set PER RECORDING (a run may hold several - engine.graph.BucketedTrainStep records the step once per caption
        # bucket -, each with its own captured gradient tensors): the recording made next uses `cap`, returned to the caller, who
        # passes it back to finish_capture() / advance_for_replay()
        cap = {
            "graph_n": n,
            "graph_dyn": torch.empty(3 * n + 1, dtype=torch.int64, device=pl["sizes"].device),
            "graph_gptr_host": torch.empty(n, dtype=torch.int64).pin_memory(),
            "graph_ring": [torch.empty(2 * n + 1, dtype=torch.int64).pin_memory() for _ in range(4)],
            "graph_ring_ev": [None] * 4,
            "graph_turn": 0,
            "graph_defer": bool(defer_table_copy),
            "graph_pending": False,
        }
        pl["cap"] = cap
        return cap

    def finish_capture(self, cap=None):
        """After the recording ended (prepare_capture(defer_table_copy=True)): the gradient address table -> device, once."""
        pl = cap if cap is not None else (self._plan or {}).get("cap")
        if pl is not None and pl.get("graph_pending"):
            n = pl["graph_n"]
            pl["graph_dyn"][:n].copy_(pl["graph_gptr_host"], non_blocking=True)
            pl["graph_pending"] = False

    def _capture_tables(self, items):
        """INSIDE the capture: the captured gradients' addresses -> the static table (a captured copy node)."""
        pl = self._plan.get("cap") or {}
        n = len(items)
        if pl.get("graph_n") != n:
            raise RuntimeError("%s.step() inside a stream capture needs prepare_capture() first (engine.graph.CapturedTrainStep "
                               "does it) and the same set of parameters with gradients as the eager steps" % self.NAME)
        pl["graph_gptr_host"].numpy()[:] = np.array([g.data_ptr() for _, g, _ in items], dtype=np.uint64).view(np.int64)
        if pl.get("graph_defer"):
            pl["graph_pending"] = True  # (finish_capture() copies it once the recording has ended)
        else:
            pl["graph_dyn"][:n].copy_(pl["graph_gptr_host"], non_blocking=True)
        return pl["graph_dyn"]

    def _replay_rows(self):
        """The four per-tensor fp32 rows of the step about to be replayed (the host-side state advances with them)."""
        raise NotImplementedError

    def advance_for_replay(self, cap=None):
        """Host side of one replayed step: the four per-tensor rows (the groups' CURRENT lr / weight decay and what the
        subclass keeps per parameter) -> the device table of the recording about to be replayed (`cap`: what its
        prepare_capture() returned; None: the latest), stream-ordered."""
        pl = cap if cap is not None else self._plan["cap"]
        n = pl["graph_n"]
        r0, r1, r2, r3 = self._replay_rows()
        k = pl["graph_turn"]
        pl["graph_turn"] = (k + 1) % len(pl["graph_ring"])
        if pl["graph_ring_ev"][k] is not None:
            pl["graph_ring_ev"][k].synchronize()  # the copy issued four steps ago (long finished)
        f = pl["graph_ring"][k].numpy().view(np.float32)
        f[:n] = np.asarray(r0, dtype=np.float32)
        f[n : 2 * n] = np.asarray(r1, dtype=np.float32)
        f[2 * n : 3 * n] = np.asarray(r2, dtype=np.float32)
        f[3 * n : 4 * n] = np.asarray(r3, dtype=np.float32)
        pl["graph_dyn"][n:].copy_(pl["graph_ring"][k], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        pl["graph_ring_ev"][k] = ev
        ops.note_parameter_write()

    def _tables(self, items):
        """The plan for `items` = [(parameter, gradient, state)], rebuilt when a tensor moved; whether a capture is on."""
        capturing = items[0][0].is_cuda and torch.cuda.is_current_stream_capturing()
        key = self._key(items)
        if self._plan is None or self._plan["key"] != key:
            if capturing:
                raise RuntimeError("%s: parameter / state tensors moved since the eager warm-up steps; cannot build tables inside a capture" % self.NAME)
            self._build(items)
        return self._plan, capturing

    @staticmethod
    def _dense_grad(p):
        g = p.grad
        if g.stride() != p.stride():  # gradient arrived in another dense layout: re-layout once
            g = torch.empty_like(p, memory_format=torch.preserve_format).copy_(g)
            p.grad = g
        return g


class FusedAdam(_FusedMultiTensor):
    NAME = "FusedAdam"
    CHUNK = ADAM_CHUNK

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.decoupled = decoupled

    def load_state_dict(self, state_dict):
        """torch.optim.Adam-compatible state (resume: Checkpointer.load -> optimizer.load_state_dict).  The loaded
        moment tensors replace the ones the cached pointer tables refer to, and the bias-correction step count
        lives in the per-parameter ``state[p]["step"]`` entries, which are restored here - nothing else to keep."""
        super().load_state_dict(state_dict)
        for st in self.state.values():  # torch saves the step as a tensor: one conversion here, no host sync per step later
            if "step" in st and not isinstance(st["step"], int):
                st["step"] = int(st["step"])

    def _state_keys(self):
        return ("exp_avg", "exp_avg_sq")

    def _replay_rows(self):
        """Per-parameter step counts, bias corrections, the groups' current lr / weight decay."""
        lrs, wds, bc1, bc2 = [], [], [], []
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                t = int(st["step"]) + 1
                st["step"] = t
                lrs.append(group["lr"])
                wds.append(group["weight_decay"])
                bc1.append(1.0 - b1 ** t)
                bc2.append((1.0 - b2 ** t) ** 0.5)
        return lrs, wds, bc1, bc2

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        items, lrs, wds = [], [], []
        b1 = b2 = eps = None
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                items.append((p, self._dense_grad(p), st))
                lrs.append(group["lr"])
                wds.append(group["weight_decay"])
                gb1, gb2 = group["betas"]
                if b1 is None:
                    b1, b2, eps = gb1, gb2, group["eps"]
                elif (b1, b2, eps) != (gb1, gb2, group["eps"]):
                    raise RuntimeError("FusedAdam: betas/eps must be shared by all groups")
        if not items:
            return loss
        pl, capturing = self._tables(items)
        n = len(items)
        if capturing:
            # nothing executes during a capture: step counts and hyper-parameters are advanced per REPLAY (advance_for_replay)
            dyn = self._capture_tables(items)
        else:
            # one step count PER PARAMETER, as torch.optim.Adam keeps it (a parameter that starts receiving gradients
            # later, or a resumed state with unequal counts, gets its own bias correction)
            bc1, bc2 = [], []
            for _, _, st in items:
                t = int(st["step"]) + 1
                st["step"] = t
                bc1.append(1.0 - b1 ** t)
                bc2.append((1.0 - b2 ** t) ** 0.5)
            dyn = self._upload(items, lrs, wds, bc1, bc2)
        m, v = pl["state"]
        ops.call("trid_adam_multi_f32", ops._p(pl["p"]), ops._p(dyn), ops._p(m), ops._p(v),
                 ops._p(pl["sizes"]), ops._p(dyn) + 8 * n, ops._p(dyn) + 12 * n, ops._p(pl["ct"]), ops._p(pl["co"]), pl["n"],
                 ADAM_CHUNK, float(b1), float(b2), float(eps), ops._p(dyn) + 16 * n, ops._p(dyn) + 20 * n,
                 1 if self.decoupled else 0, ops.stream())
        ops.note_parameter_write()  # raw-pointer write: torch's tensor._version does not move
        return loss


class FusedSGD(_FusedMultiTensor):
    """``torch.optim.SGD`` (maximize=False) as ONE multi-tensor launch: same constructor, same ``momentum_buffer`` state
    layout (checkpoints of either class load into the other), lr / weight decay per group and re-read every step.

    torch's first update of a parameter is ``buf = d`` without dampening.  The kernel computes ``buf = mom_i * buf +
    gscale_i * d`` with per-tensor DEVICE coefficients: (0, 1) over a zero-filled buffer for that first update, (momentum,
    1 - dampening) afterwards - no branch in the kernel, no special case in a recorded step.  ``self._fresh`` holds the
    parameters whose buffer was allocated and not yet written (torch's "the buffer does not exist yet"; here it exists
    from the moment its parameter first has a gradient, so that the pointer tables can be built).

    ``_fresh`` is host state outside ``state_dict()``.  That is sound because a buffer is allocated and first written in
    the SAME ``step()`` call, and a capture refuses to allocate: between steps ``_fresh`` is empty, so a saved or loaded
    buffer has always been written.  Allocating buffers anywhere else (``__init__``, ``prepare_capture``) would break it."""

    NAME = "FusedSGD"
    CHUNK = SGD_CHUNK

    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False):
        if lr < 0.0:
            raise ValueError("Invalid learning rate: {}".format(lr))
        if momentum < 0.0:
            raise ValueError("Invalid momentum value: {}".format(momentum))
        if weight_decay < 0.0:
            raise ValueError("Invalid weight_decay value: {}".format(weight_decay))
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        defaults = dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay, nesterov=nesterov)
        super().__init__(params, defaults)
        self._fresh = set()

    def __setstate__(self, state):
        super().__setstate__(state)
        self._fresh = set()

    def load_state_dict(self, state_dict):
        """torch.optim.SGD-compatible state.  torch writes ``momentum_buffer: None`` for a parameter that has a state entry
        but has not been updated yet: dropped here, so that its first-update rule still applies."""
        super().load_state_dict(state_dict)
        for st in self.state.values():
            if "momentum_buffer" in st and st["momentum_buffer"] is None:
                del st["momentum_buffer"]
        self._fresh = set()  # every loaded buffer has been written

    def _shared(self):
        """momentum / dampening / nesterov: one launch has one of each."""
        g0 = self.param_groups[0]
        for key in ("momentum", "dampening", "nesterov"):
            for group in self.param_groups:
                if group[key] != g0[key]:
                    raise RuntimeError("FusedSGD: %s must be shared by all groups (got %r and %r)" % (key, g0[key], group[key]))
        return g0["momentum"], g0["dampening"], bool(g0["nesterov"])

    def _state_keys(self):
        # group 0 speaks for all groups: every caller (step, _replay_rows, and _tables / the plan key below them) runs
        # behind _shared(), which has refused groups that disagree
        return ("momentum_buffer",) if self.param_groups[0]["momentum"] != 0 else ()

    def _rows(self, momentum, dampening):
        """lr, weight decay, buffer coefficient and gradient scale of every parameter with a gradient; marks their first
        update as done."""
        lrs, wds, moms, gs = [], [], [], []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                lrs.append(group["lr"])
                wds.append(group["weight_decay"])
                if momentum != 0:
                    first = p in self._fresh
                    self._fresh.discard(p)
                    moms.append(0.0 if first else momentum)
                    gs.append(1.0 if first else 1.0 - dampening)
                else:
                    moms.append(0.0)
                    gs.append(1.0)
        return lrs, wds, moms, gs

    def _replay_rows(self):
        momentum, dampening, _ = self._shared()
        return self._rows(momentum, dampening)

    @torch.no_grad()
    def step(self, closure=None):
        loss = closure() if closure is not None else None
        momentum, dampening, nesterov = self._shared()
        items = []
        for group in self.param_groups:
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p] if momentum != 0 else None
                if st is not None and "momentum_buffer" not in st:
                    st["momentum_buffer"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    self._fresh.add(p)
                items.append((p, self._dense_grad(p), st))
        if not items:
            return loss
        pl, capturing = self._tables(items)
        n = len(items)
        if capturing:
            # nothing executes during a capture: the hyper-parameter rows are written per REPLAY (advance_for_replay)
            dyn = self._capture_tables(items)
        else:
            dyn = self._upload(items, *self._rows(momentum, dampening))
        buf = ops._p(pl["state"][0]) if momentum != 0 else None
        ops.call("trid_sgd_multi_f32", ops._p(pl["p"]), ops._p(dyn), buf, ops._p(pl["sizes"]), ops._p(dyn) + 8 * n,
                 ops._p(dyn) + 12 * n, ops._p(dyn) + 16 * n, ops._p(dyn) + 20 * n, ops._p(pl["ct"]), ops._p(pl["co"]), pl["n"],
                 SGD_CHUNK, float(momentum), 1 if nesterov else 0, ops.stream())
        ops.note_parameter_write()  # raw-pointer write: torch's tensor._version does not move
        return loss


def make_optimizer(cfg, model, fused=True):
    """fused=False: the torch optimiser of the same rule (a reference to compare with; it does not run on the library)."""
    params = []
    for key, value in model.named_parameters():
        if not value.requires_grad:
            continue
        lr = cfg.SOLVER.BASE_LR
        weight_decay = cfg.SOLVER.WEIGHT_DECAY
        if "bias" in key:
            lr = cfg.SOLVER.BASE_LR * cfg.SOLVER.BIAS_LR_FACTOR
            weight_decay = cfg.SOLVER.WEIGHT_DECAY_BIAS
        params.append({"params": [value], "lr": lr, "weight_decay": weight_decay})
    betas = (cfg.SOLVER.ADAM_ALPHA, cfg.SOLVER.ADAM_BETA)
    name = cfg.SOLVER.OPTIMIZER
    if name == "SGD":
        cls = FusedSGD if fused else torch.optim.SGD
        return cls(params, lr=cfg.SOLVER.BASE_LR, momentum=cfg.SOLVER.SGD_MOMENTUM)
    if name in ("Adam", "AdamW"):
        if fused:
            return FusedAdam(params, lr=cfg.SOLVER.BASE_LR, betas=betas, eps=1e-8, decoupled=(name == "AdamW"))
        cls = torch.optim.Adam if name == "Adam" else torch.optim.AdamW
        return cls(params, lr=cfg.SOLVER.BASE_LR, betas=betas, eps=1e-8)
    raise NotImplementedError(name)


class LRSchedulerWithWarmup(torch.optim.lr_scheduler._LRScheduler):
    def __init__(self, optimizer, milestones, gamma=0.1, mode="step", warmup_factor=1.0 / 3, warmup_epochs=10,
                 warmup_method="linear", total_epochs=100, target_lr=0, power=0.9, last_epoch=-1):
        if list(milestones) != sorted(milestones):
            raise ValueError("SOLVER.STEPS must be sorted in increasing order, got %r" % (milestones,))
        if mode not in ("step", "exp", "poly", "cosine", "linear"):
            raise ValueError("unknown lr scheduler mode {}".format(mode))
        if warmup_method not in ("constant", "linear"):
            raise ValueError("unknown warmup_method {}".format(warmup_method))
        self.milestones, self.mode, self.gamma = milestones, mode, gamma
        self.warmup_factor, self.warmup_epochs, self.warmup_method = warmup_factor, warmup_epochs, warmup_method
        self.total_epochs, self.target_lr, self.power = total_epochs, target_lr, power
        super().__init__(optimizer, last_epoch)

    def _factor(self):
        e = self.last_epoch
        if e < self.warmup_epochs:
            if self.warmup_method == "constant":
                return ("mul", self.warmup_factor)
            a = e / self.warmup_epochs
            return ("mul", self.warmup_factor * (1 - a) + a)
        if self.mode == "step":
            return ("mul", self.gamma ** bisect_right(self.milestones, e))
        r = (e - self.warmup_epochs) / (self.total_epochs - self.warmup_epochs)
        if self.mode == "exp":
            return ("mul", self.power ** r)
        if self.mode == "linear":
            return ("mul", 1 - r)
        if self.mode == "poly":
            return ("to", self.power ** (1 - r))
        return ("to", 0.5 * (1 + cos(pi * r)))

    def get_lr(self):
        kind, f = self._factor()
        if kind == "mul":
            return [b * f for b in self.base_lrs]
        return [self.target_lr + (b - self.target_lr) * f for b in self.base_lrs]


def make_lr_scheduler(cfg, optimizer):
    s = cfg.SOLVER
    return LRSchedulerWithWarmup(optimizer, milestones=s.STEPS, gamma=s.GAMMA, warmup_factor=s.WARMUP_FACTOR,
                                 warmup_epochs=s.WARMUP_EPOCHS, warmup_method=s.WARMUP_METHOD, total_epochs=s.NUM_EPOCHS,
                                 mode=s.LRSCHEDULER, target_lr=s.TARGET_LR, power=s.POWER)
