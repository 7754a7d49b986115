#!/usr/bin/env python
"""Generate tests/golden/tiny_input_grads.npz: the REFERENCE's gradient with respect to the input clip.

Runs only in the build container, where the reference checkout is (tools/gen_golden.py's REF), like tools/gen_golden_loss.py.  It builds the reference's
``VitaCLIP`` at the TINY shape with the synthetic weights (tools/gen_golden.py's own builders, so the model is the one
tiny_grads.npz was made with), feeds it ``x = synth_clip(2, 4, 64)`` with ``requires_grad`` and backpropagates
``sum(w_logits * logits)`` under torch autograd.  Nothing of the model is restated here.

The file holds data only: logits [2, 3], w_logits [2, 3] (seeded), dx [2, 3, 4, 64, 64] float32 - the full gradient, ~0.4 MB.

    python tools/gen_golden_input_grad.py
"""
import os
import sys
import warnings

import numpy as np
import torch

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gen_golden as gg  # noqa: E402

from gava_clip_amd import synth  # noqa: E402
from gava_clip_amd.config import TINY  # noqa: E402


def main():
    torch.set_num_threads(8)
    mod, _ = gg.import_reference()
    assert mod.__file__.startswith(gg.REF)
    model = gg.build_reference(mod, TINY, os.path.join(gg.CLASSES, "updrs_3cls_classes.txt"))
    gg.load_synth(model, TINY, 3)
    model.train()
    x = torch.from_numpy(synth.synth_clip(2, TINY.num_frames, TINY.input_size)).requires_grad_()
    w = torch.randn(2, 3, generator=torch.Generator().manual_seed(2025))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        logits, lmt, lvm = model(x)
    assert lmt is None and lvm is None
    (logits * w).sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all())
    path = os.path.join(gg.REPO, "tests", "golden", "tiny_input_grads.npz")
    np.savez_compressed(path, logits=logits.detach().numpy(), w_logits=w.numpy(), dx=x.grad.numpy())
    print("wrote", path, os.path.getsize(path), "bytes; |dx| =", float(x.grad.norm()))


if __name__ == "__main__":
    main()
