"""Restatement of gava_unpatchify (include/gava_hip.h) in torch, by index arithmetic: the checker of the fold kernel.

tests/test_input_grad_host.py pins `fold` to torch autograd (x.grad of a Conv2d(3, D, P, stride=P) in fp64).  It runs in
the dtype and on the device of its input, so the same code gives the bit-exact fp32 answer for the GRAD and ABSMAX modes and
the fp64 reference of the other two."""
import torch

GRAD, ABSMAX, L2, GRAD_X_INPUT = 0, 1, 2, 3


def fold(dpatch, B, T, size, P, frame_rows, row_offset):
    """dpatch [B*T*frame_rows, ld] (or [B*T, frame_rows, ld]) -> g [B, 3, T, size, size] with
    g[b, c, t, py*P + ky, px*P + kx] = dpatch[(b*T + t), row_offset + py*(size/P) + px, c*P*P + ky*P + kx]."""
    g = size // P
    dp = dpatch.reshape(B * T, frame_rows, dpatch.shape[-1])
    y = torch.arange(size, device=dpatch.device).view(1, size, 1)
    x = torch.arange(size, device=dpatch.device).view(1, 1, size)
    c = torch.arange(3, device=dpatch.device).view(3, 1, 1)
    row = (row_offset + (y // P) * g + x // P).expand(3, size, size)
    col = (c * P * P + (y % P) * P + x % P).expand(3, size, size)
    return dp[:, row, col].view(B, T, 3, size, size).permute(0, 2, 1, 3, 4).contiguous()


def reduce_map(g, mode, x=None):
    """The saliency maps of a gradient g [B, 3, T, S, S] -> [B, T, S, S]; the channel sums in the order c = 0, 1, 2."""
    if mode == ABSMAX:
        return g.abs().amax(dim=1)
    if mode == L2:
        return (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1] + g[:, 2] * g[:, 2]).sqrt()
    if mode == GRAD_X_INPUT:
        return g[:, 0] * x[:, 0] + g[:, 1] * x[:, 1] + g[:, 2] * x[:, 2]
    raise ValueError(mode)


def unpatchify(dpatch, B, T, size, P, frame_rows, row_offset, mode, x=None):
    g = fold(dpatch, B, T, size, P, frame_rows, row_offset)
    return g if mode == GRAD else reduce_map(g, mode, x)
