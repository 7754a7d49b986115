"""Worker for tests/test_train_frames.py: DistributedDataParallel around VitaCLIP.forward_frames, one process per rank,
rendezvous on 127.0.0.1 (the gloo rehearsal route of tests/dist_worker.py)."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))


class FramesModel(torch.nn.Module):
    """DDP hooks run on forward(): a module whose forward IS forward_frames (what a training script wraps)."""

    def __init__(self, model, pre):
        super().__init__()
        self.model, self.pre = model, pre

    def forward(self, videos):
        return self.model.forward_frames(videos, self.pre)


def ddp_frames_gpu(rank, world, port, out_dir):
    """Each rank backpropagates its own decoded videos through forward_frames, DDP averages the gradients; they must equal
    those of one process on all the videos with the loss averaged (the bound of test_ddp_gradients_equal_single_process)."""
    from torch.nn.parallel import DistributedDataParallel as DDP
    from gava_clip_amd import VitaCLIP
    from gava_clip_amd.config import TINY
    from gava_clip_amd.preprocess import ClipPreprocessor
    from helpers import model_kwargs, synth_torch_state
    from train_preprocess_ref import video
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    b = 2
    shapes = [(11, 90, 130), (6, 120, 80), (9, 64, 64), (14, 70, 200)]
    vids = [video(*shapes[i % len(shapes)], 300 + i).cuda() for i in range(b * world)]
    y = torch.arange(b * world, device="cuda") % 3
    pre = ClipPreprocessor(num_frames=TINY.num_frames, sampling_rate=2, spatial_size=TINY.input_size)

    def fresh():
        m = VitaCLIP(**model_kwargs(TINY))
        m.load_state_dict(synth_torch_state(TINY, 3), strict=True)
        return m.cuda().train()

    ddp = DDP(FramesModel(fresh(), pre), find_unused_parameters=False)
    logits = ddp(vids[rank * b:(rank + 1) * b])[0]
    torch.nn.functional.cross_entropy(logits, y[rank * b:(rank + 1) * b]).backward()
    torch.cuda.synchronize()
    single = fresh()
    torch.nn.functional.cross_entropy(single.forward_frames(vids, pre)[0], y).backward()
    torch.cuda.synchronize()
    worst, n = 0.0, 0
    for (name, p), (_, q) in zip(ddp.module.model.named_parameters(), single.named_parameters()):
        if q.grad is None:
            assert p.grad is None, name
            continue
        n += 1
        worst = max(worst, float((p.grad - q.grad).norm() / (q.grad.norm() + 1e-12)))
    np.save(os.path.join(out_dir, f"ddpframes{rank}.npy"), np.array([worst, n]))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    fn, rank, world, port, out_dir = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5]
    {"ddp_frames_gpu": ddp_frames_gpu}[fn](rank, world, port, out_dir)
