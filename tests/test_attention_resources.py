"""Code generation of the attention kernels, checked on the host: tools/kernel_resources.py cross-compiles a source file for
gfx950 and reports what the compiler allocated per kernel."""
import os
import re
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# Kernels that already spilled before the backward's tile code was shared (8 bytes per lane): the causal single-pass
# forward at 20 key tiles, a class no model configuration routes to (the text tower has 77 keys: 6 tiles).
SPILLS = ("attention_kernel<PrecF16, 20, true, false, 0>", "attention_kernel<PrecBF16, 20, true, false, 0>")


@pytest.mark.parametrize("src,kernels,count", [
    ("attention_bwd.hip", ("attn_bwd_dq_kernel", "attn_bwd_dkv_kernel", "attn_bwd_dq_stream_kernel", "attn_bwd_dkv_stream_kernel"), 46),
    ("attention.hip", ("attention_kernel", "attention_persist_kernel", "attention_stream_kernel", "attention_f32_kernel"), 30),
])
def test_attention_kernels_compile_without_scratch(src, kernels, count):
    """Every instantiation of every attention kernel keeps its tiles in registers: scratch 0.  The shared tile code of the
    backward is inlined into four kernels with different register budgets; a spill in any of them shows here."""
    out = subprocess.check_output([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), src]).decode()
    print(out)
    rows = [ln for ln in out.splitlines() if "scratch" in ln]
    assert len(rows) == count, len(rows)
    for k in kernels:
        assert any(k + "<" in ln for ln in rows), k
    for ln in rows:
        if any(s in ln for s in SPILLS):
            continue
        assert int(re.search(r"scratch\s+(\d+)", ln).group(1)) == 0, ln
