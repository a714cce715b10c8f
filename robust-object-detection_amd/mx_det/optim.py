"""SGD on libmx_det's multi-tensor kernel (mx_sgd_step): torch.optim.SGD's API and update rule.

The reference trains with torch.optim.SGD(params, lr=0.005, momentum=0.9, weight_decay=5e-4) and
StepLR(8, 0.1) (scripts/train_frcnn_baseline.py:149-153, step at :176). This class is a drop-in
(same constructor, param_groups, state_dict with per-parameter 'momentum_buffer', works with
torch.optim.lr_scheduler) whose step() is ONE launch per 64 parameters for f32 CUDA parameters
instead of torch's foreach path (three multi_tensor_apply launches plus host-side grouping).
Parameters that are not f32 CUDA tensors (e.g. a CPU model) take torch's own implementation.

AdamW (below) is the same for the restoration U-Net's loop: torch.optim.AdamW's API, state layout and
update rule on mx_adamw_step / mx_adamw_pack_step.
"""
import ctypes
import os

import torch
from torch.autograd.graph import increment_version
from torch.optim.adam import adam as _torch_adam
from torch.optim.optimizer import _get_scalar_dtype, _use_grad_for_differentiable

from . import _lib
from . import conv as mc


# MX_SGD_PACK=0: keep the update and the conv operand repack as two launches (sgd_kernel, then
# WeightPacker.refresh's pack_batched_kernel before the next forward)
_SGD_PACK = int(os.environ.get("MX_SGD_PACK", "1"))


# MX_ADAMW_PACK=0: the same for AdamW (adamw_kernel, then the repack)
_ADAMW_PACK = int(os.environ.get("MX_ADAMW_PACK", "1"))


def _f32_dense(t):
    return t.is_cuda and t.dtype == torch.float32 and not t.is_sparse and t.is_contiguous()


def _fused_plan(prefix, prm, entries, pk, device):
    """The device plan of a fused launch, built by the entries `prefix`_plan_bytes / `prefix`_build
    ("mx_sgd_pack", "mx_adamw_pack") from the filled parameter table prm, whose pack indices count the
    entries that are not None in order. Returns plan, blocks, lds (the step entry's arguments)."""
    packs = [e for e in entries if e is not None]
    descs = (mc.PackDesc * len(packs))(*[pk.desc(e) for e in packs])
    n = len(prm)
    nb = getattr(_lib.load(), prefix + "_plan_bytes")(n)
    host = torch.empty(nb, dtype=torch.uint8, pin_memory=True)
    blocks, lds = ctypes.c_int64(0), ctypes.c_size_t(0)
    _lib.call(prefix + "_build", prm, n, descs, host.data_ptr(), nb, ctypes.byref(blocks), ctypes.byref(lds))
    return host.to(device, non_blocking=True), blocks.value, lds.value


def _grad_table(c, grads, device):
    """c["gdev"], the device table of the gradients' pointers: uploaded again when they differ from
    c["gkey"]. False when a gradient is not f32 / dense / contiguous / CUDA."""
    gptr = [g.data_ptr() for g in grads]
    if gptr != c["gkey"]:
        if not all(_f32_dense(g) for g in grads):
            return False
        c["gdev"] = torch.tensor(gptr, dtype=torch.int64).pin_memory().to(device, non_blocking=True)
        c["gkey"] = gptr
    return True


class _SgdParam(ctypes.Structure):  # mx_sgd_param
    _fields_ = [("p", ctypes.c_void_p), ("buf", ctypes.c_void_p), ("n", ctypes.c_int64), ("first", ctypes.c_int32),
                ("pack", ctypes.c_int32)]


class SGD(torch.optim.SGD):
    def __init__(self, params, lr=1e-3, momentum=0, dampening=0, weight_decay=0, nesterov=False, **kw):
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                         nesterov=nesterov, **kw)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        fast = self.__dict__.setdefault("_fast", {})
        for group in self.param_groups:
            if self._pack_step(group):
                continue
            if self._fast_step(group, fast):
                continue
            ps = [p for p in group["params"] if p.grad is not None]
            if not ps:
                continue
            if (group.get("maximize") or group["momentum"] == 0 or
                    any(not _f32_dense(p) or p.grad.is_sparse or not p.grad.is_contiguous() for p in ps)):
                self._torch_step(group, ps)
                continue
            n = len(ps)
            bufs, first = [], (ctypes.c_uint8 * n)()
            for i, p in enumerate(ps):
                st = self.state[p]
                b = st.get("momentum_buffer")
                if b is None:
                    b = st["momentum_buffer"] = torch.empty_like(p, memory_format=torch.contiguous_format)
                    first[i] = 1
                bufs.append(b)
            P = (ctypes.c_void_p * n)(*[p.data_ptr() for p in ps])
            G = (ctypes.c_void_p * n)(*[p.grad.data_ptr() for p in ps])
            B = (ctypes.c_void_p * n)(*[b.data_ptr() for b in bufs])
            N = (ctypes.c_int64 * n)(*[p.numel() for p in ps])
            _lib.call("mx_sgd_step", P, G, B, N, first, n, float(group["lr"]), float(group["momentum"]),
                      float(group["dampening"]), float(group["weight_decay"]), int(group["nesterov"]),
                      _lib.stream())
            # the kernel wrote through raw pointers: bump the version counters as an in-place torch op
            # would (autograd checks, and the conv WeightPacker repacks by version)
            increment_version(ps)
            increment_version(bufs)
            if len(ps) == len(group["params"]):  # all present: cache the static arrays for _fast_step
                fast[id(group)] = {"ps": group["params"], "n": n, "P": P, "B": B, "N": N,
                                   "first": (ctypes.c_uint8 * n)(), "bufs": bufs,
                                   "pptr": [p.data_ptr() for p in ps], "bptr": [b.data_ptr() for b in bufs]}
        return loss

    def _pack_step(self, group):
        """Conv weights registered with the current WeightPacker (mx_det.conv.get_packer) get their
        bf16 operands written by the update itself (mx_sgd_pack_step: one launch for the whole group,
        no separate repack of the new weights before the next forward). Returns False to take the
        other paths (no packer, nothing to fold, or a case the multi-tensor kernel does not cover).
        Steady state (same parameters, buffers and packer): only the gradients' pointers are gathered
        on the host; the device plan is rebuilt when anything else changes."""
        pk = mc.get_packer()
        if pk is None or _SGD_PACK == 0:
            return False
        ps = group["params"]
        cache = self.__dict__.setdefault("_pk", {})
        c = cache.get(id(group))
        if c is not None and c["ps"] is ps and c["packer"] is pk and c["ready"]:
            grads = [p.grad for p in ps]
            if any(g is None for g in grads):
                return False
            st = self.state
            if ([p.data_ptr() for p in ps] != c["pptr"] or
                    any(st[p].get("momentum_buffer") is not b for p, b in zip(ps, c["bufs"]))):
                c = None
        if c is None or c["ps"] is not ps or c["packer"] is not pk or not c["ready"]:
            if (not ps or group.get("maximize") or group["momentum"] == 0 or
                    any(p.grad is None or not _f32_dense(p) or p.grad.is_sparse for p in ps)):
                return False
            c = self._pack_plan(group, pk)
            if c is None:
                return False
            cache[id(group)] = c
            grads = [p.grad for p in ps]
        if not _grad_table(c, grads, ps[0].device):
            return False
        _lib.call("mx_sgd_pack_step", c["plan"].data_ptr(), c["gdev"].data_ptr(), len(ps), c["blocks"], c["lds"],
                  float(group["lr"]), float(group["momentum"]), float(group["dampening"]),
                  float(group["weight_decay"]), int(group["nesterov"]), _lib.stream())
        increment_version(ps)
        increment_version(c["bufs"])
        pk.mark_packed(c["entries"])
        if not c["ready"]:  # first momentum step done: the next plan has every first flag clear
            c["ready"] = all(not f for f in c["first"])
            if not c["ready"]:
                cache.pop(id(group), None)
        return True

    def _pack_plan(self, group, pk):
        ps = group["params"]
        entries = pk.fusable(ps)
        if not any(e is not None for e in entries):
            return None
        n = len(ps)
        # new momentum buffers stay local until the plan is built: a failed build must not leave
        # uninitialised buffers in self.state (a retried step / state_dict would read them as momentum)
        first, bufs, fresh = [], [], {}
        for p in ps:
            b = self.state[p].get("momentum_buffer") if p in self.state else None
            if b is None:
                b = fresh[p] = torch.empty_like(p, memory_format=torch.contiguous_format)
                first.append(1)
            else:
                first.append(0)
            bufs.append(b)
        prm = (_SgdParam * n)()
        j = 0
        for i, (p, b, e) in enumerate(zip(ps, bufs, entries)):
            prm[i] = _SgdParam(p.data_ptr(), b.data_ptr(), p.numel(), first[i], j if e is not None else -1)
            j += e is not None
        plan, blocks, lds = _fused_plan("mx_sgd_pack", prm, entries, pk, ps[0].device)
        for p, b in fresh.items():
            self.state[p]["momentum_buffer"] = b
        return {"ps": ps, "packer": pk, "pptr": [p.data_ptr() for p in ps], "entries": entries, "bufs": bufs,
                "first": first, "ready": not any(first), "plan": plan, "blocks": blocks, "lds": lds, "gkey": None}

    def _fast_step(self, group, fast):
        """Steady state: every parameter of the group has a grad and a momentum buffer, and the
        parameter list is unchanged -> reuse the cached pointer arrays; only the grads' pointers
        (new tensors each step) are gathered. Returns False to take the general path."""
        ps = group["params"]
        c = fast.get(id(group))
        if c is None or c["ps"] is not ps or c["n"] != len(ps):
            fast.pop(id(group), None)
            return False
        # parameters and momentum buffers still the cached storage (p.data =, load_state_dict, ...)
        st = self.state
        bufs = [st[p].get("momentum_buffer") if p in st else None for p in ps]
        if (any(b is None for b in bufs) or [p.data_ptr() for p in ps] != c["pptr"]
                or [b.data_ptr() for b in bufs] != c["bptr"]):
            fast.pop(id(group), None)
            return False
        grads = [p.grad for p in ps]
        if any(g is None or not g.is_contiguous() for g in grads):
            return False
        n = len(ps)
        G = (ctypes.c_void_p * n)(*[g.data_ptr() for g in grads])
        _lib.call("mx_sgd_step", c["P"], G, c["B"], c["N"], c["first"], n, float(group["lr"]),
                  float(group["momentum"]), float(group["dampening"]), float(group["weight_decay"]),
                  int(group["nesterov"]), _lib.stream())
        increment_version(ps)
        increment_version(c["bufs"])
        return True

    def _torch_step(self, group, ps):
        for p in ps:
            d = p.grad
            if group["weight_decay"]:
                d = d.add(p, alpha=group["weight_decay"])
            if group["momentum"]:
                st = self.state[p]
                b = st.get("momentum_buffer")
                if b is None:
                    b = st["momentum_buffer"] = d.clone().detach()
                else:
                    b.mul_(group["momentum"]).add_(d, alpha=1 - group["dampening"])
                d = d.add(b, alpha=group["momentum"]) if group["nesterov"] else b
            p.add_(d, alpha=-group["lr"] if not group.get("maximize") else group["lr"])


class _AdamwParam(ctypes.Structure):  # mx_adamw_param
    _fields_ = [("p", ctypes.c_void_p), ("exp_avg", ctypes.c_void_p), ("exp_avg_sq", ctypes.c_void_p),
                ("n", ctypes.c_int64), ("pack", ctypes.c_int32), ("reserved", ctypes.c_int32)]


class AdamW(torch.optim.AdamW):
    """torch.optim.AdamW on libmx_det's kernels: the restoration U-Net's optimizer (the reference builds
    AdamW(lr=1e-3, weight_decay=1e-4) and a cosine schedule, train_restoration.py:246-272). A drop-in:
    same constructor, param_groups and LR-scheduler behaviour, and the state is torch's own layout (per
    parameter 'step' as a CPU f32 scalar tensor, 'exp_avg', 'exp_avg_sq'), so a state_dict() loads
    into torch.optim.AdamW and the other way round. Per group, step() takes one of three paths:

    * fused (mx_adamw_pack_step, ONE launch for the group): a WeightPacker is current
      (mx_det.conv.get_packer()), every parameter has an f32 contiguous CUDA grad, and all share one
      step number. Conv weights registered with the packer get their bf16 operands written by the
      update itself, so the next forward's refresh() has nothing to repack.
    * plain (mx_adamw_step, one launch per 64 tensors): no packer, MX_ADAMW_PACK=0, differing step
      numbers, or a parameter without a grad this step (skipped; it keeps its step, as in torch).
    * torch's own implementation, with torch's bits: amsgrad, maximize, capturable, differentiable,
      fused, a tensor lr or beta, non-f32 / CPU / sparse / non-contiguous parameters or grads.

    The step is not meant for graph capture: its launch arguments change every step."""

    @_use_grad_for_differentiable
    def step(self, closure=None):
        self._cuda_graph_capture_health_check()
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        for group in self.param_groups:
            if not self._flags_covered(group):
                self.__dict__.get("_pk", {}).pop(id(group), None)
                self._torch_step(group)
            elif self._pack_step(group):
                continue
            else:
                # another path moves the step numbers: the fused plan's cached one is stale from here
                self.__dict__.get("_pk", {}).pop(id(group), None)
                ps = [p for p in group["params"] if p.grad is not None]
                if not ps:
                    continue
                if self._tensors_covered(ps):
                    self._plain_step(group, ps)
                else:
                    self._torch_step(group)
        return loss

    @staticmethod
    def _flags_covered(group):
        b1, b2 = group["betas"]
        return not (group["amsgrad"] or group["maximize"] or group["capturable"] or group["differentiable"]
                    or group["fused"] or torch.is_tensor(group["lr"]) or torch.is_tensor(b1) or torch.is_tensor(b2)
                    or not group.get("decoupled_weight_decay", True))

    def _tensors_covered(self, ps):
        for p in ps:
            if not (_f32_dense(p) and _f32_dense(p.grad)):
                return False
            st = self.state.get(p)
            if st and not (st["step"].is_cpu and _f32_dense(st["exp_avg"]) and _f32_dense(st["exp_avg_sq"])):
                return False
        return True

    @staticmethod
    def _new_state(p):
        # zero-initialised, as torch's _init_group creates it
        return {"step": torch.tensor(0.0, dtype=_get_scalar_dtype()),
                "exp_avg": torch.zeros_like(p, memory_format=torch.preserve_format),
                "exp_avg_sq": torch.zeros_like(p, memory_format=torch.preserve_format)}

    def _torch_step(self, group):
        """torch.optim.Adam.step's body for one group."""
        ps, grads, ms, vs, mx, steps = [], [], [], [], [], []
        b1, b2 = group["betas"]
        has_complex = self._init_group(group, ps, grads, ms, vs, mx, steps)
        _torch_adam(ps, grads, ms, vs, mx, steps, amsgrad=group["amsgrad"], has_complex=has_complex, beta1=b1,
                    beta2=b2, lr=group["lr"], weight_decay=group["weight_decay"], eps=group["eps"],
                    maximize=group["maximize"], foreach=group["foreach"], capturable=group["capturable"],
                    differentiable=group["differentiable"], fused=group["fused"],
                    grad_scale=getattr(self, "grad_scale", None), found_inf=getattr(self, "found_inf", None),
                    decoupled_weight_decay=group["decoupled_weight_decay"])

    def _plain_step(self, group, ps):
        n = len(ps)
        sts = []
        for p in ps:
            st = self.state[p]
            if len(st) == 0:
                st.update(self._new_state(p))
            sts.append(st)
        ms, vs, steps = [s["exp_avg"] for s in sts], [s["exp_avg_sq"] for s in sts], [s["step"] for s in sts]
        P = (ctypes.c_void_p * n)(*[p.data_ptr() for p in ps])
        G = (ctypes.c_void_p * n)(*[p.grad.data_ptr() for p in ps])
        M = (ctypes.c_void_p * n)(*[m.data_ptr() for m in ms])
        V = (ctypes.c_void_p * n)(*[v.data_ptr() for v in vs])
        N = (ctypes.c_int64 * n)(*[p.numel() for p in ps])
        S = (ctypes.c_int64 * n)(*[int(t) + 1 for t in steps])
        b1, b2 = group["betas"]
        _lib.call("mx_adamw_step", P, G, M, V, N, S, n, float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                  float(group["weight_decay"]), _lib.stream())
        torch._foreach_add_(steps, 1)
        # the kernel wrote through raw pointers: bump the version counters as an in-place torch op
        # would (autograd checks, and the conv WeightPacker repacks by version)
        increment_version(ps)
        increment_version(ms)
        increment_version(vs)

    def _pack_step(self, group):
        """The fused path (see the class docstring); False to take the others. Steady state (same
        parameters, state tensors and packer): only the gradients' pointers are gathered on the host;
        the device plan is rebuilt when anything else changes (load_state_dict, p.data = ...). The
        hyper-parameters are launch arguments, so an LR schedule rebuilds nothing."""
        pk = mc.get_packer()
        if pk is None or _ADAMW_PACK == 0:
            return False
        ps = group["params"]
        cache = self.__dict__.setdefault("_pk", {})
        c = cache.get(id(group))
        if c is not None and (c["ps"] is not ps or c["n"] != len(ps) or c["packer"] is not pk):
            c = None
        if c is not None:
            grads = [p.grad for p in ps]
            if any(g is None for g in grads):
                return False
            st = self.state
            if [p.data_ptr() for p in ps] != c["pptr"] or int(c["steps"][0]) != c["step"]:
                c = None
            else:
                for p, m, v, t in zip(ps, c["ms"], c["vs"], c["steps"]):
                    s = st[p]
                    if s.get("exp_avg") is not m or s.get("exp_avg_sq") is not v or s.get("step") is not t:
                        c = None
                        break
        if c is None:
            cache.pop(id(group), None)
            if not ps or any(p.grad is None or not _f32_dense(p) or p.grad.is_sparse for p in ps):
                return False
            c = self._pack_plan(group, pk)
            if c is None:
                return False
            cache[id(group)] = c
            grads = [p.grad for p in ps]
        if not _grad_table(c, grads, ps[0].device):
            return False
        b1, b2 = group["betas"]
        _lib.call("mx_adamw_pack_step", c["plan"].data_ptr(), c["gdev"].data_ptr(), len(ps), c["blocks"], c["lds"],
                  c["step"] + 1, float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                  float(group["weight_decay"]), _lib.stream())
        for p, s in c.pop("fresh", {}).items():  # state created for this plan: now it has been used
            self.state[p].update(s)
        torch._foreach_add_(c["steps"], 1)
        c["step"] += 1
        increment_version(ps)
        increment_version(c["ms"])
        increment_version(c["vs"])
        pk.mark_packed(c["entries"])
        return True

    def _pack_plan(self, group, pk):
        ps = group["params"]
        entries = pk.fusable(ps)
        if not any(e is not None for e in entries):
            return None
        n = len(ps)
        # new state stays local until the plan is built and its first step has run: a failed build must
        # not leave state behind that no step has touched (see SGD._pack_plan)
        sts, fresh = [], {}
        for p in ps:
            s = self.state.get(p)
            if not s:
                s = fresh[p] = self._new_state(p)
            elif not (s["step"].is_cpu and _f32_dense(s["exp_avg"]) and _f32_dense(s["exp_avg_sq"])):
                return None
            sts.append(s)
        steps = [s["step"] for s in sts]
        nums = {int(t) for t in steps}
        if len(nums) != 1:  # one launch carries one step number
            return None
        ms, vs = [s["exp_avg"] for s in sts], [s["exp_avg_sq"] for s in sts]
        prm = (_AdamwParam * n)()
        j = 0
        for i, (p, m, v, e) in enumerate(zip(ps, ms, vs, entries)):
            prm[i] = _AdamwParam(p.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel(), j if e is not None else -1, 0)
            j += e is not None
        plan, blocks, lds = _fused_plan("mx_adamw_pack", prm, entries, pk, ps[0].device)
        return {"ps": ps, "n": n, "packer": pk, "pptr": [p.data_ptr() for p in ps], "entries": entries, "ms": ms,
                "vs": vs, "steps": steps, "step": nums.pop(), "fresh": fresh, "plan": plan, "blocks": blocks,
                "lds": lds, "gkey": None}
