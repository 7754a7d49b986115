#!/usr/bin/env python
"""Time and count the launches of the auxiliary part of a training step's tail - the video<->NTE head, the support-memory<->text
head, loss_mt and loss_vm, and their backward - on both routes, in one process:

    hip    training.NteHeadFn + MemoryHeadFn + gava_clip_amd.AuxCriterion (gava_nte_head*, gava_memory_head*, ...)
    torch  the traced torch ops of VitaCLIP._forward_impl (aux_heads = "torch", the default) + the same loss terms in torch ops

at the reference's training shape (B = 64 clips, M = 64 memories of S = 5 rows, E = 512, D = 768, 70 NTE combinations) with C = 3
and C = 6 classes.  Launches are counted with torch.profiler (device kernels of one step, as tools/train_head_bench.py counts
them).  Times come from device events around one step (forward + backward, gradients of every parameter, of `summary` and of
`text_features`); the two routes alternate, --repeats times each after --warmup, and the median is reported with the quartiles.
The shapes are small, so these are launch-bound figures: host enqueue time shows wherever the device runs dry.
Writes profiles/aux_heads_bench.json.

    python tools/aux_heads_bench.py [--repeats 200] [--warmup 20] [--sigmoid]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from gava_clip_amd import AuxCriterion, hip  # noqa: E402
from gava_clip_amd.training import MemoryHeadFn, NteHeadFn  # noqa: E402

NUM_COMB = 70


class Heads(nn.Module):
    """The auxiliary heads' parameters as VitaCLIP builds them (model.py), without the towers."""

    def __init__(self, C, E, D, sigmoid):
        super().__init__()
        mlp = lambda: nn.Sequential(nn.Linear(E, E // 4), nn.Tanh(), nn.Linear(E // 4, E // 8))
        self.sum_proj = nn.Linear(D, E)
        self.tf_project = mlp()
        self.memory_project = nn.ModuleList([mlp() for _ in range(C)])
        self.logit_scale_vm = nn.Parameter(torch.tensor(2.302585 if sigmoid else 100.0))
        self.logit_scale_mt = nn.Parameter(torch.tensor(2.302585 if sigmoid else 100.0))
        self.logit_bias_mt = nn.Parameter(torch.tensor(-10.0)) if sigmoid else None
        self.table = None

    def torch_route(self, summary, text_features, memory, video_nte):       # VitaCLIP._forward_impl, aux_heads = "torch"
        sp = self.sum_proj(summary)
        sp = sp / sp.norm(dim=-1, keepdim=True)
        with torch.no_grad():
            valid_idx = ((video_nte.sum(dim=-1).sum(dim=-1)) != 0).float()
            valid_mat = valid_idx.unsqueeze(1) * valid_idx.unsqueeze(0)
        video_nte = video_nte / video_nte.norm(dim=-1, keepdim=True)
        similarity = torch.bmm(sp.unsqueeze(0).expand(NUM_COMB, -1, -1), video_nte.permute(1, 2, 0)).mean(0)
        logits_mat = self.logit_scale_vm * (similarity * valid_mat)
        logits_vm = F.log_softmax(logits_mat, dim=-1) + F.log_softmax(logits_mat, dim=-2)
        memory = memory.mean(dim=1)
        logits_mt = torch.empty(memory.size(0), 0).to(memory.device)
        for cid, mproj in enumerate(self.memory_project):
            tf = self.tf_project(text_features[cid])
            tf = tf / tf.norm(dim=-1, keepdim=True)
            memo = mproj(memory)
            memo = memo / memo.norm(dim=-1, keepdim=True)
            logits_mt = torch.concat([logits_mt, (self.logit_scale_mt * memo @ tf.t()).unsqueeze(-1)], dim=1)
        logits_mt = F.log_softmax(logits_mt, dim=-1)
        if self.logit_bias_mt is not None:
            logits_mt += self.logit_bias_mt
        return logits_mt, logits_vm

    def hip_route(self, summary, text_features, memory, video_nte):         # aux_heads = "hip"
        logits_vm = NteHeadFn.apply(summary, self.sum_proj.weight, self.sum_proj.bias, video_nte, self.logit_scale_vm)
        params = list(self.tf_project.parameters()) + [q for mp in self.memory_project for q in mp.parameters()]
        if self.table is None:
            self.table = hip.pointer_table(params[4:], memory.device)
        logits_mt = MemoryHeadFn.apply(memory, text_features, self.logit_scale_mt, self.logit_bias_mt, self.table, *params)
        return logits_mt, logits_vm


def torch_terms(logits_mt, labels, logits_vm, sigmoid, w_mt, w_vm):         # training/train.py:454-475
    if sigmoid:
        t = F.one_hot(labels, num_classes=logits_mt.shape[-1]).float()
        loss_mt = (w_mt * ((-F.logsigmoid((t * 2 - 1.0) * logits_mt)).sum(-1) * w_mt)).mean()
    else:
        loss_mt = (w_mt * F.cross_entropy(logits_mt, labels, reduction="none")).mean()
    return loss_mt, -w_vm * torch.diag(logits_vm).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--sigmoid", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("aux_heads_bench measures on the GPU: no device found")
    B = M = 64
    S, E, D = 5, 512, 768
    out = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "sigmoid": args.sigmoid, "cases": {}}
    for C in (3, 6):
        g = torch.Generator().manual_seed(C)
        heads = Heads(C, E, D, args.sigmoid).cuda()
        summary = torch.randn(B, D, generator=g).cuda().requires_grad_()
        tf = torch.randn(C, E, generator=g)
        text_features = (tf / tf.norm(dim=-1, keepdim=True)).cuda().requires_grad_()
        memory, video_nte = torch.randn(M, S, E, generator=g).cuda(), torch.randn(B, NUM_COMB, E, generator=g).cuda()
        labels = torch.randint(0, C, (M,), generator=g).cuda()
        crit = AuxCriterion(memory_loss_weight=1.0, vnte_loss_weight=1.0, sigmoid=args.sigmoid)

        def step(route):
            heads.zero_grad(set_to_none=True)
            summary.grad = text_features.grad = None
            if route == "hip":
                lmt, lvm = heads.hip_route(summary, text_features, memory, video_nte)
                loss_mt, loss_vm = crit(lmt, labels, lvm)
            else:
                lmt, lvm = heads.torch_route(summary, text_features, memory, video_nte)
                loss_mt, loss_vm = torch_terms(lmt, labels, lvm, args.sigmoid, 1.0, 1.0)
            (loss_mt + loss_vm).backward()
            return loss_mt.detach(), loss_vm.detach(), summary.grad

        results = {r: step(r) for r in ("hip", "torch")}                  # the two routes compute the same thing
        agree = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(results["hip"], results["torch"]))
        times = {"hip": [], "torch": []}
        for i in range(args.warmup + args.repeats):
            for route in ("hip", "torch"):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                step(route)
                t1.record()
                t1.synchronize()
                if i >= args.warmup:
                    times[route].append(t0.elapsed_time(t1) * 1e3)
        res = {}
        for route in ("hip", "torch"):
            with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA, torch.profiler.ProfilerActivity.CPU]) as prof:
                step(route)
                torch.cuda.synchronize()
            kernels = [e for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "emcpy" not in e.name and "emset" not in e.name]
            q = statistics.quantiles(times[route], n=4)
            res[route] = {"median_us": round(q[1], 2), "q1_us": round(q[0], 2), "q3_us": round(q[2], 2), "device_kernels": len(kernels),
                          "device_us": round(sum(e.device_time for e in kernels), 2)}
        out["cases"][f"C{C}"] = dict(B=B, M=M, S=S, C=C, E=E, D=D, routes_agree_rel=agree, **res)
        print(f"C{C}", json.dumps(out["cases"][f"C{C}"]))
    path = os.path.join(REPO, "profiles", "aux_heads_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", path)


if __name__ == "__main__":
    main()
