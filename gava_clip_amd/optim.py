"""FusedAdamW: torch.optim.AdamW's step as one HIP kernel over all parameters (gava_adamw_step, csrc/optimizer.hip).

The kernel updates p, exp_avg and exp_avg_sq of every parameter with a gradient in one launch and the step counts in a second,
reads GradScaler's scale and found_inf from device memory (a step with a non-finite gradient is skipped on the device, nothing
visits the host) and, when the optimizer was built from a VitaCLIP, writes the packed 16-bit copies of the summary-attention
projections (VitaCLIP._packed, the vision backward pack) from the updated values it holds in registers, so that neither
VitaCLIP._refresh_summary_weights nor training.refresh_vision_backward has anything left to do.

    opt = FusedAdamW(model, lr=8e-4, weight_decay=0.01)           # or a parameter list / param groups: no copies then
    sched = torch.optim.lr_scheduler.CosineAnnealingLR(opt, T_max=steps)
    scaler.scale(loss).backward(); scaler.step(opt); scaler.update(); sched.step()

State keys and param_groups are torch.optim.AdamW's: a state_dict of either loads into the other.  The gradient is read only:
with a GradScaler, p.grad still holds the scaled gradient after the step.

Clipping by global norm is part of the step (gava_grad_norm, gava_adamw_step_clipped): torch's unscale_ + clip_grad_norm_ + step
in four launches (two each), without writing a gradient and without a host wait.

    opt = FusedAdamW(model, lr=4e-4, weight_decay=0.2, max_grad_norm=1.0)     # float("inf"): measure, do not clip
    scaler.scale(loss).backward(); scaler.step(opt); scaler.update()
    opt.last["grad_norm"], opt.last["clip_coef"], opt.last["nonfinite"]       # 0-dim device views; opt.grad_norms(): per parameter

The norm is that of the unscaled gradients over all param groups.  A non-finite norm skips the step on the device (torch's
clip_grad_norm_ would scale by NaN and poison every parameter).  max_grad_norm is an attribute, settable between steps; it is
no param_groups key and no part of state_dict().
"""
import ctypes as C
import math

import torch

from . import hip
from .hip import GavaError

_TORCH_GROUP_DEFAULTS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None,
                             decoupled_weight_decay=True)
_REFUSED_FLAGS = ("amsgrad", "maximize", "capturable", "differentiable")


def check_param(p):
    """The parameters the kernel takes: dense fp32 on the device, contiguous."""
    if not isinstance(p, torch.Tensor):
        raise GavaError(f"FusedAdamW: parameters must be tensors, got {type(p).__name__}")
    if p.dtype != torch.float32:
        raise GavaError(f"FusedAdamW updates fp32 parameters only, got {p.dtype}")
    if not p.is_cuda:
        raise GavaError(f"FusedAdamW updates device parameters only, got a parameter on {p.device}")
    if p.is_sparse or not p.is_contiguous():
        raise GavaError("FusedAdamW updates dense contiguous parameters only")


def check_grad(p, g):
    if g.is_sparse:
        raise GavaError("FusedAdamW does not take sparse gradients")
    if g.dtype != torch.float32 or g.device != p.device or g.shape != p.shape or not g.is_contiguous():
        raise GavaError(f"FusedAdamW: the gradient of a parameter must be a contiguous fp32 tensor of its shape on its device "
                        f"(got {g.dtype} {tuple(g.shape)} on {g.device} for {tuple(p.shape)} on {p.device})")


def check_max_grad_norm(v):
    """None (no clipping stage), or a positive float: finite clips, inf measures only."""
    if v is None:
        return None
    if isinstance(v, bool) or not isinstance(v, (int, float)) or math.isnan(v) or not v > 0:
        raise GavaError(f"FusedAdamW: max_grad_norm must be None or a positive number (float('inf') measures without clipping), got {v!r}")
    return float(v)


def _check_flags(flags):
    for k in _REFUSED_FLAGS:
        if flags.get(k):
            raise GavaError(f"FusedAdamW does not support {k}=True")


class FusedAdamW(torch.optim.Optimizer):
    _step_supports_amp_scaling = True      # GradScaler.step sets self.grad_scale / self.found_inf and calls step() directly

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, *, amsgrad=False, maximize=False,
                 capturable=False, differentiable=False, max_grad_norm=None):
        self.max_grad_norm = max_grad_norm
        self.last = {}           # after a step with max_grad_norm: grad_norm, clip_coef, nonfinite (views of the device stats, valid until the next step)
        _check_flags(dict(amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable))
        self._model = None
        if isinstance(params, torch.nn.Module):
            module = params
            if isinstance(module, (torch.nn.parallel.DistributedDataParallel, torch.nn.DataParallel)):
                module = module.module
            if hasattr(module, "_summary_weight_versions") and hasattr(module, "visual"):
                self._model = module
            params = list(module.parameters())      # frozen ones included, as torch.optim.AdamW(model.parameters()) has them
        else:
            params = list(params)
        groups = params if params and isinstance(params[0], dict) else [dict(params=params)]
        if len(groups) > hip.ADAMW_MAX_GROUPS:
            raise GavaError(f"FusedAdamW takes at most {hip.ADAMW_MAX_GROUPS} param groups, got {len(groups)}")
        for grp in groups:
            _check_flags(grp)
            ps = grp["params"]
            for p in ([ps] if isinstance(ps, torch.Tensor) else list(ps)):
                check_param(p)
        self._steps = None       # one device fp32 vector; state[p]["step"] is its element self._index[id(p)]
        self._index = {}
        self._sig = None         # signature of every pointer in the uploaded table
        self._table = None       # (host ctypes table, device buffer, number of chunks, entries)
        self._targets = (None, {})
        self._clip = None        # (workspace, tensor_norm, stats, parameters in table order), allocated with the table
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, **_TORCH_GROUP_DEFAULTS)
        super().__init__(params, defaults)

    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        if len(self.param_groups) > hip.ADAMW_MAX_GROUPS:
            raise GavaError(f"FusedAdamW takes at most {hip.ADAMW_MAX_GROUPS} param groups, got {len(self.param_groups)}")
        _check_flags(self.param_groups[-1])
        for p in self.param_groups[-1]["params"]:
            check_param(p)
            self._index.setdefault(id(p), len(self._index))
        self._sig = None

    @property
    def max_grad_norm(self):
        return self._max_grad_norm

    @max_grad_norm.setter
    def max_grad_norm(self, v):
        self._max_grad_norm = check_max_grad_norm(v)

    def grad_norms(self):
        """{parameter: 0-dim view of the norm of its unscaled gradient} as the last step with max_grad_norm measured it (0 for a
        parameter that had no gradient); empty before the first such step.  Like the views in `last` they show the device
        buffers of the current table: the next step overwrites them, or, when a gradient or a pack has moved and the table is
        rebuilt, leaves them behind with stale values.  Read (or clone) them before the next step."""
        if not self.last:
            return {}
        _ws, tensor_norm, _stats, params = self._clip
        return {p: tensor_norm[i] for i, p in enumerate(params)}

    # ---- state --------------------------------------------------------------------------------------------------------
    def _step_vector(self, device):
        n = len(self._index)
        if self._steps is None or self._steps.numel() < n or self._steps.device != device:
            new = torch.zeros(n, dtype=torch.float32, device=device)
            if self._steps is not None:
                new[:self._steps.numel()].copy_(self._steps)
            self._steps = new
            for grp in self.param_groups:
                for p in grp["params"]:
                    if "step" in self.state.get(p, {}):
                        self.state[p]["step"] = new[self._index[id(p)]]
        return self._steps

    def _adopt_steps(self):
        """After load_state_dict: move the loaded step counts (torch.optim.AdamW keeps them as host tensors) into the vector."""
        have = [p for grp in self.param_groups for p in grp["params"] if "step" in self.state.get(p, {})]
        if not have:
            return
        loaded = [self.state[p]["step"] for p in have]
        self._steps = None
        steps = self._step_vector(have[0].device)
        for p, val in zip(have, loaded):
            view = steps[self._index[id(p)]]
            view.copy_(torch.as_tensor(val, dtype=torch.float32))
            self.state[p]["step"] = view

    def state_dict(self):
        sd = super().state_dict()
        # (the per-parameter dicts of the base class's result ARE the live ones: new dicts, with a step that is no view of the vector)
        sd["state"] = {k: ({**st, "step": st["step"].clone()} if "step" in st else st) for k, st in sd["state"].items()}
        return sd

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._index = {}
        for grp in self.param_groups:
            _check_flags(grp)
            for p in grp["params"]:
                self._index.setdefault(id(p), len(self._index))
        self._adopt_steps()
        self._sig = None

    # ---- the packed copies of a VitaCLIP ---------------------------------------------------------------------------------
    def _packs(self):
        m = self._model
        if m is None:
            return None, None
        fw = m._packed if m._packed is not None and "w_sqkv" in m._packed else None
        bw = m._bwd_packs.get("vision")
        return fw, (bw[1] if bw is not None else None)

    def _copy_targets(self, fw, bw):
        """{id(parameter): copy fields of its table entry} for the packs that exist now; cached by the packs' pointers."""
        m = self._model
        if fw is None and bw is None:
            return {}
        sig = [m.prec]
        if fw is not None:
            sig += [t.data_ptr() for k in ("w_sqkv", "w_sout", "b_sqkv") for t in fw[k]]
        if bw is not None:
            sig += [L[k].data_ptr() for L in bw["layers"] for k in ("w_sqkv", "w_sqkv_t", "w_sout", "w_sout_t")]
        sig = tuple(sig)
        if self._targets[0] == sig:
            return self._targets[1]
        out = {}
        h16 = hip.h16_dtype(m.prec)
        for i, blk in enumerate(m.visual.blocks):
            s = blk.summary_attn_layer
            D = s.out_proj.weight.shape[1]
            for j, proj in enumerate((s.q_proj, s.k_proj, s.v_proj, s.out_proj)):
                w = dict(rows=proj.weight.shape[0], cols=D)
                name, off = ("w_sout", 0) if j == 3 else ("w_sqkv", j * D)        # q, k, v: row blocks / column blocks of one copy
                if fw is not None:
                    t = fw[name][i]
                    if t.dtype != h16 or not t.is_contiguous() or t.shape[1] != D:
                        raise GavaError(f"FusedAdamW: the packed {name} is not a contiguous {h16} matrix of width {D}")
                    w.update(copy16=t.data_ptr() + off * D * 2, ld16=D, prec16=m.prec)
                    if j < 3:
                        b = fw["b_sqkv"][i]
                        if b.dtype != torch.float32 or not b.is_contiguous():
                            raise GavaError("FusedAdamW: the packed b_sqkv is not a contiguous fp32 vector")
                        out[id(proj.bias)] = dict(rows=1, cols=D, copy_f32=b.data_ptr() + off * 4, ld_f32=D)
                if bw is not None:
                    t, tt = bw["layers"][i][name], bw["layers"][i][name + "_t"]
                    if t.dtype != torch.bfloat16 or tt.dtype != torch.bfloat16 or not t.is_contiguous() or not tt.is_contiguous():
                        raise GavaError(f"FusedAdamW: the backward pack's {name} copies are not contiguous bf16 matrices")
                    w.update(copy_bf16=t.data_ptr() + off * D * 2, ld_bf16=D, copy_bf16_t=tt.data_ptr() + off * 2, ld_bf16_t=tt.shape[1])
                out[id(proj.weight)] = w
        self._targets = (sig, out)
        return out

    # ---- the table ----------------------------------------------------------------------------------------------------------
    def _build_table(self, entries, targets, device):
        lib = hip.load()
        n = len(entries)
        tab = (hip.AdamWTensor * n)()
        for e, (p, g, gi) in zip(tab, entries):
            e.p, e.n, e.group = p.data_ptr(), p.numel(), gi
            if g is None:
                continue
            st = self.state[p]
            e.g, e.m, e.v, e.step = g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr()
            for k, val in targets.get(id(p), {}).items():
                setattr(e, k, val)
        n_groups = len(self.param_groups)
        count = lib.gava_adamw_plan(tab, n, n_groups, None, 0)
        hip.check(min(count, 0), "gava_adamw_plan")
        chunks = (hip.AdamWChunk * max(count, 1))()
        hip.check(min(lib.gava_adamw_plan(tab, n, n_groups, chunks, count), 0), "gava_adamw_plan")
        # a fresh pinned buffer per upload: an earlier asynchronous copy may still be reading the previous one
        tbytes, cbytes = C.sizeof(tab), C.sizeof(hip.AdamWChunk) * count
        host = torch.empty(tbytes + max(cbytes, 16), dtype=torch.uint8, pin_memory=True)
        C.memmove(host.data_ptr(), tab, tbytes)
        if cbytes:
            C.memmove(host.data_ptr() + tbytes, chunks, cbytes)
        dev = host.to(device, non_blocking=True)
        self._table = (tab, dev, count, tbytes)
        self._clip = None
        if self.max_grad_norm is not None:
            self._build_clip_buffers(entries, device)

    def _build_clip_buffers(self, entries, device):
        """gava_grad_norm's workspace (a double per chunk and per tensor) and outputs; they live as long as the table."""
        n, count = len(entries), self._table[2]
        self._clip = (torch.empty(count + n, dtype=torch.float64, device=device), torch.empty(n, dtype=torch.float32, device=device),
                      torch.empty(4, dtype=torch.float32, device=device), [p for p, _g, _gi in entries])

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if len(self.param_groups) > hip.ADAMW_MAX_GROUPS:
            raise GavaError(f"FusedAdamW takes at most {hip.ADAMW_MAX_GROUPS} param groups, got {len(self.param_groups)}")
        device = None
        entries, sig, updated = [], [], []
        for gi, grp in enumerate(self.param_groups):
            _check_flags(grp)
            for p in grp["params"]:
                g = p.grad
                if device is None:
                    device = p.device
                elif p.device != device:
                    raise GavaError(f"FusedAdamW: all parameters must live on one device (got {device} and {p.device})")
                if g is None:
                    entries.append((p, None, gi))
                    sig.append((p.data_ptr(), 0))
                    continue
                check_grad(p, g)
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = self._step_vector(device)[self._index[id(p)]]
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                entries.append((p, g, gi))
                updated.append(p)
                sig.append((p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr()))
        if not updated:
            return loss
        fw, bw = self._packs()
        targets = self._copy_targets(fw, bw)
        sig = (self._targets[0] if targets else None, len(self.param_groups), tuple(sig))
        if sig != self._sig:
            self._build_table(entries, targets, device)
            self._sig = sig
        tab, dev, n_chunks, tbytes = self._table

        for name, t in (("grad_scale", getattr(self, "grad_scale", None)), ("found_inf", getattr(self, "found_inf", None))):
            if t is not None and not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.device == device and t.numel() == 1):
                raise GavaError(f"FusedAdamW.{name} must be one fp32 value on {device}")
        a = hip.AdamWArgs()
        a.table, a.table_host, a.chunks = dev.data_ptr(), tab, dev.data_ptr() + tbytes
        a.n_tensors, a.n_chunks, a.n_groups = len(tab), n_chunks, len(self.param_groups)
        for gi, grp in enumerate(self.param_groups):
            h = a.groups[gi]
            h.lr, h.eps, h.weight_decay = float(grp["lr"]), float(grp["eps"]), float(grp["weight_decay"])
            h.beta1, h.beta2 = float(grp["betas"][0]), float(grp["betas"][1])
        a.grad_scale, a.found_inf = hip.ptr(getattr(self, "grad_scale", None)), hip.ptr(getattr(self, "found_inf", None))

        # copies that were current before the step are current after it: the kernel writes the copy of every tensor it updates
        before = self._model._summary_weight_versions() if targets else None
        with torch.cuda.device(device):
            if self.max_grad_norm is None:
                hip.check(hip.load().gava_adamw_step(C.byref(a), hip.stream_ptr()), "gava_adamw_step")
                self.last = {}
            else:
                if self._clip is None:      # max_grad_norm was set after the table was built
                    self._build_clip_buffers(entries, device)
                ws, tensor_norm, stats, _params = self._clip
                n = hip.GradNormArgs()
                n.table, n.table_host, n.chunks = a.table, tab, a.chunks
                n.n_tensors, n.n_chunks, n.n_groups = a.n_tensors, a.n_chunks, a.n_groups
                n.grad_scale, n.max_norm = a.grad_scale, self.max_grad_norm
                n.workspace, n.tensor_norm, n.stats = ws.data_ptr(), tensor_norm.data_ptr(), stats.data_ptr()
                hip.check(hip.load().gava_grad_norm(C.byref(n), hip.stream_ptr()), "gava_grad_norm")
                hip.check(hip.load().gava_adamw_step_clipped(C.byref(a), stats.data_ptr(), hip.stream_ptr()), "gava_adamw_step_clipped")
                self.last = dict(grad_norm=stats[0], clip_coef=stats[1], nonfinite=stats[2])
        torch.autograd.graph.increment_version(updated)
        if targets:
            after = self._model._summary_weight_versions()
            for pack, served in ((fw, fw is not None and "w_sqkv_wlo" not in fw), (bw, bw is not None)):
                if served:      # (the weight-lo set is not written here: its pack keeps its versions and the host refresh runs)
                    pack["summary_ver"] = [new if old == was else old for old, was, new in zip(pack["summary_ver"], before, after)]
        return loss
