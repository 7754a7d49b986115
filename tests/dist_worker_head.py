"""Worker for tests/test_distributed_head.py: DistributedDataParallel around the model with the HIP training head and the device
criterion (one process per rank, rendezvous on 127.0.0.1; modelled on tests/dist_worker.py)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from dist_worker import _init  # noqa: E402


def ddp_train_head_gpu(rank, world, port, out_dir):
    """Each rank backpropagates its own clips through HeadFn and TrainCriterion, DDP averages the gradients; they must equal those
    of one process on the concatenated batch (the criterion is a mean over samples, the ranks hold equal shares)."""
    from torch.nn.parallel import DistributedDataParallel as DDP
    from gava_clip_amd import TrainCriterion, VitaCLIP, synth
    from gava_clip_amd.config import TINY
    from helpers import model_kwargs, synth_torch_state
    _init(rank, world, port)
    torch.set_num_threads(2)
    b = 2
    x = torch.from_numpy(synth.synth_clip(b * world, TINY.num_frames, TINY.input_size)).cuda()
    y = torch.arange(b * world, device="cuda") % 3

    def fresh():
        m = VitaCLIP(**model_kwargs(TINY))
        m.load_state_dict(synth_torch_state(TINY, 3), strict=True)
        m.train_head = "hip"
        return m.cuda().train()

    crit = TrainCriterion(focal_ordinal=True, beta=0.2)
    ddp = DDP(fresh(), find_unused_parameters=False)
    crit(ddp(x[rank * b:(rank + 1) * b])[0], y[rank * b:(rank + 1) * b]).backward()
    torch.cuda.synchronize()
    calls = ddp.module.last.get("head_fn_calls", 0)
    single = fresh()
    crit(single(x)[0], y).backward()
    torch.cuda.synchronize()
    worst, n = 0.0, 0
    for (name, p), (_, q) in zip(ddp.module.named_parameters(), single.named_parameters()):
        if q.grad is None:
            assert p.grad is None, name
            continue
        n += 1
        worst = max(worst, float((p.grad - q.grad).norm() / (q.grad.norm() + 1e-12)))
    np.save(os.path.join(out_dir, f"ddphead{rank}.npy"), np.array([worst, n, calls]))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    fn, rank, world, port, out_dir = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    {"ddp_train_head_gpu": ddp_train_head_gpu}[fn](rank, world, port, out_dir)
