"""Multi-process training with the HIP head (two ranks, gloo, sharing cuda:0), beside tests/test_distributed.py."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.gpu
def test_ddp_gradients_with_hip_head_equal_single_process(tmp_path):
    """DistributedDataParallel (training/train.py:347) with train_head = "hip" and TrainCriterion: the averaged gradients of
    every trainable parameter == the single-process ones on the concatenated batch, to the 2e-2 norm-wise that
    tests/test_distributed.py asserts for the torch head (the backward's own accuracy)."""
    world, port = 2, _free_port()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", OMP_NUM_THREADS="2", GAVA_TEST_BACKEND="gloo")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dist_worker_head.py"), "ddp_train_head_gpu", str(r), str(world),
                               str(port), str(tmp_path)], env=env) for r in range(world)]
    try:
        codes = [p.wait(timeout=600) for p in procs]
    finally:
        for p in procs:          # only the exact children this test started
            if p.poll() is None:
                p.kill()
    assert codes == [0] * world
    for r in range(world):
        worst, n, calls = np.load(tmp_path / f"ddphead{r}.npy")
        assert calls == 1 and n > 20 and worst <= 2e-2, (worst, n, calls)
