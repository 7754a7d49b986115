"""CPU: the host side of the attention maps (gava_attention_mass, hip.attention_mass, VitaCLIP.attention_maps).

  * the rollout chain the device runs equals the matrix-product rollout, and keeps sum r = 1;
  * the fp64 reference's rows sum to 1, and the emulation of the kernel's rounding points stays within half the bound on every
    shape, form, regime and precision the GPU test uses; the bound stays below 1e-4 of the block's max|ref| there;
  * every applicable mutation of the reference misses the bound by 10x or more, in every regime;
  * the C ABI's surface: names, the struct mirror, the argument checks that return before any launch;
  * code generation: every instantiation of the new kernel compiles without scratch;
  * the Python refusals that need no device, and the reference fixture's own consistency.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import attention_maps_ref as mr
from attention_maps_ref import F16, BF16
from gava_clip_amd.config import TINY
from helpers import REPO, CLASSES_3, model_kwargs

NAMES = ("gava_attention_mass", "gava_attention_maps_struct_sizes")
EMU_SHARE = 0.5          # the emulation within half the bound: the other half is what it does not model
MUT_FACTOR = 10.0
CASES = mr.TABLE + mr.TABLE_CHAIN


def case_params(c):
    return [p for p in mr.params() if p[0] is c]


def test_chain_equals_matrix_rollout():
    g = torch.Generator().manual_seed(5)
    for n, L in ((197, 3), (17, 2), (5, 1)):
        A = (4 * torch.randn(L, n, n, generator=g, dtype=torch.float64)).softmax(-1)
        chain, mat = mr.rollout_chain(A), mr.rollout_matrix(A)
        assert float((chain - mat).abs().max()) <= 1e-12
        assert abs(float(chain.sum()) - 1) <= 1e-12 and bool((chain > 0).all())
    # one block: r = (e_cls + A[0]) / 2
    A = torch.rand(1, 4, 4, dtype=torch.float64).softmax(-1)
    want = 0.5 * A[0, 0]
    want[0] += 0.5
    assert torch.allclose(mr.rollout_chain(A), want, rtol=0, atol=1e-15)


def test_reference_rows_sum_to_one_and_renorm_is_the_restricted_softmax():
    c = mr.vision(4, 2, 3, 21)
    x = mr.make_inputs(c, "randn", 11, F16)
    mass, _ = mr.reference(c, x, "mass")
    assert mass.shape == (4, 2, mr.n_keys(c)) and float((mass.sum(-1) - c.n).abs().max()) <= 1e-12 * c.n
    w = mr.weights(c, "chain", 11)
    assert float((w.sum(-1) - 1).abs().max()) <= 1e-6
    chain, _ = mr.reference(c, x, "chain", w)
    assert chain.shape == (4, 2, c.n) and float((chain.sum(-1) - w.double().sum(-1)[:, None]).abs().max()) <= 1e-12
    # P over all keys, cut to the frame's own and renormalised per row == softmax over the frame's own keys
    K, _ = mr.gather(c, x)
    Q = x.q.double().view(c.BT, c.n, c.heads, 64).transpose(1, 2)
    P = (Q @ K.transpose(-1, -2)).softmax(-1)[..., :c.n]
    P = P / P.sum(-1, keepdim=True)
    assert float((torch.einsum("fi,fhij->fhj", w.double(), P) - chain).abs().max()) <= 1e-14
    cc = mr.cls(c)
    xc = mr.make_inputs(cc, "randn", 12, BF16)
    row, _ = mr.reference(cc, xc, "cls")
    assert row.shape == (4, 2, mr.n_keys(c)) and float((row.sum(-1) - 1).abs().max()) <= 1e-12


@pytest.mark.parametrize("c", CASES, ids=mr.ar.case_id)
def test_emulation_within_half_the_bound(c):
    for _, form, regime, prec in case_params(c):
        seed = mr.seed_of(c, regime)
        x, w = mr.make_inputs(c, regime, seed, prec), mr.weights(c, form, seed)
        ref, smax = mr.reference(c, x, form, w)
        emu = mr.emulate(c, x, form, w)
        assert emu.shape == ref.shape == (c.BT, c.heads, mr.n_out(c, form)) and torch.isfinite(emu).all()
        r = mr.ratio(c, emu, ref, smax)
        assert r <= EMU_SHARE, (mr.param_id(c, form, regime, prec), r)
        # the issue's condition on the bound itself
        assert float((mr.bound(c, ref, smax) / ref.abs().amax(-1)).max()) < 1e-4


def test_table_covers_what_the_issue_lists():
    keys = {mr.n_keys(c) for c in mr.TABLE}
    assert {31, 32, 33, 64, 65, 224, 225, 410, 416, 417, 640} <= keys and mr.n_keys(mr.TOO_MANY) == 641
    assert any(c.n % 16 == 0 for c in mr.TABLE) and any(c.G == 0 for c in mr.TABLE) and any(not c.has_summary for c in mr.TABLE)
    assert any(c.n_q == 1 and c.qbr == 1 for c in mr.TABLE) and any(c.n_q == 1 and c.qbr > 1 for c in mr.TABLE)
    assert any(c.n == 401 and mr.n_keys(c) == 410 and not c.n_q for c in mr.TABLE)
    assert all(c.heads == 2 and c.BT == 2 * c.T or c.BT == c.T for c in CASES) and any(c.BT == 2 * c.T for c in mr.TABLE)
    assert {c.n for c in mr.TABLE_CHAIN} == {64, 65, 224, 225, 416, 417}          # the LDS classes of the renormalised form
    regimes = {r for _, _, r, _ in mr.params()}
    assert regimes == set(mr.REGIMES)


@pytest.mark.parametrize("mutation", mr.MASS_MUTATIONS)
def test_mutated_reference_misses_the_bound_tenfold(mutation):
    seen = set()
    for c, form, regime, prec in mr.params():
        if not mr.mutation_applies(c, form, regime, mutation):
            continue
        seed = mr.seed_of(c, regime)
        x, w = mr.make_inputs(c, regime, seed, prec), mr.weights(c, form, seed)
        ref, smax = mr.reference(c, x, form, w)
        mut, _ = mr.reference(c, x, form, w, mutate=mutation)
        r = mr.ratio(c, mut, ref, smax)
        assert r >= MUT_FACTOR, (mr.param_id(c, form, regime, prec), r)
        seen.add(regime)
    # every regime in which the mutation can show by construction (attention_maps_ref's docstring says which cannot)
    absent = {"drop_last": {"ramp_down"}, "last_is_key0": {"uniform"}, "head_swap": {"uniform"}}.get(mutation, {"uniform", "ramp_down"})
    assert seen == set(mr.REGIMES) - absent, seen


def test_new_names_are_exported_and_declared():
    from gava_clip_amd import hip
    header = open(os.path.join(REPO, "include", "gava_hip.h")).read()
    declared = set(re.findall(r"\b(gava_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in hip.EXPORTS and name in declared, name
    from gava_clip_amd.build import SOURCES
    assert "attention_maps.hip" in SOURCES
    assert hip.ATTENTION_MASS_MAX_KEYS == mr.MAX_KEYS == 640 and "n_keys <= 640" in header
    assert callable(hip.attention_mass)


def test_struct_matches_header_and_library(tmp_path):
    """sizeof as the C compiler sees the header == the ctypes mirror == what the library reports."""
    from gava_clip_amd import hip
    from gava_clip_amd.build import build
    build(verbose=False)                                               # a no-op unless the library is missing or stale
    src = '#include <stdio.h>\n#include "gava_hip.h"\nint main(){printf("%zu\\n", sizeof(gava_attention_mass_args));return 0;}'
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    size = int(subprocess.check_output([str(tmp_path / "s")]).decode())
    lib = hip.load()
    got = (ctypes.c_size_t * 1)()
    assert lib.gava_attention_maps_struct_sizes(got, 1) == 1
    assert ctypes.sizeof(hip.AttentionMassArgs) == size == got[0]
    assert lib.gava_attention_maps_struct_sizes(None, 0) == 1          # a zero capacity writes nothing


ONE = 64      # a non-null, 16-byte aligned stand-in for a device pointer: every call below returns before it is used


def _args(hip, **kw):
    """A valid call: ViT-B/16 at T = 8, every query of a block, the chain form."""
    a = hip.AttentionMassArgs()
    a.q, a.k, a.ld_qkv, a.side_k, a.ld_side, a.w, a.out = ONE, ONE, 2304, ONE, 1536, ONE, ONE
    a.batch, a.heads, a.n_q, a.n_kmain, a.n_g, a.T, a.has_summary, a.renorm, a.prec = 16, 12, 197, 197, 8, 8, 1, 1, hip.PREC_F16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_attention_mass_refuses_bad_arguments_before_any_launch():
    """GAVA_EINVAL (-1) comes back before anything touches the device, so this runs without one."""
    from gava_clip_amd import hip
    lib = hip.load()
    call = lambda **kw: lib.gava_attention_mass(ctypes.byref(_args(hip, **kw)), None)
    assert lib.gava_attention_mass(None, None) == -1
    assert call(q=None) == -1 and call(k=None) == -1 and call(out=None) == -1                   # null pointers
    assert call(q=ONE + 8) == -1 and call(k=ONE + 2) == -1 and call(side_k=ONE + 8) == -1       # misaligned operands
    assert call(w=ONE + 2) == -1 and call(out=ONE + 1) == -1
    for field in ("batch", "heads", "n_q", "n_kmain"):
        assert call(**{field: 0}) == -1 and call(**{field: -1}) == -1, field
    assert call(ld_qkv=2300) == -1 and call(ld_qkv=760) == -1                                   # not a multiple of 8; below heads*64
    assert call(ld_side=1532) == -1 and call(ld_side=760) == -1 and call(ld_q=12, q_batch_rows=197) == -1
    assert call(side_k=None) == -1 and call(T=0) == -1 and call(T=5) == -1 and call(n_g=-1) == -1   # side rows: no matrix; batch % T
    assert call(n_kmain=624, n_q=1) == -1 and call(n_kmain=624, n_q=1, renorm=0) == -1          # 641 keys, either form
    assert call(n_q=198) == -1                                                                  # more queries than rows of the frame
    assert call(q_batch_rows=196) == -1                                                         # fewer buffer rows than queries
    assert call(renorm=2) == -1 and call(renorm=-1) == -1 and call(prec=2) == -1


def test_kernels_compile_without_scratch():
    """tools/kernel_resources.py on the new file (cross-compiles for gfx950): scratch 0 for every instantiation - four LDS
    classes x two operand types - and the largest class within the 160 KiB of a CU."""
    out = subprocess.check_output([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "attention_maps.hip"]).decode()
    print(out)
    rows = [ln for ln in out.splitlines() if "scratch" in ln]
    assert len(rows) == 8 and all("attention_mass_kernel<" in ln for ln in rows)
    for prec in ("PrecF16", "PrecBF16"):
        for nkt in (4, 14, 26, 40):
            assert any(f"attention_mass_kernel<{prec}, {nkt}>" in ln for ln in rows), (prec, nkt)
    for ln in rows:
        assert int(re.search(r"scratch\s+(\d+)", ln).group(1)) == 0, ln
        assert int(re.search(r"lds\s+(\d+)", ln).group(1)) <= 160 * 1024, ln


def test_python_refusals():
    from gava_clip_amd import hip
    E = hip.GavaError
    q = torch.zeros(8, 128, dtype=torch.float16)
    with pytest.raises(E, match="HIP device"):
        hip.attention_mass(q, q, batch=2, heads=2, n_q=4, n_kmain=4, prec=hip.PREC_F16)


def test_attention_maps_refusals_without_a_device():
    from gava_clip_amd import VitaCLIP
    from gava_clip_amd.hip import GavaError
    from gava_clip_amd.model import AttentionMaps
    m = VitaCLIP(**model_kwargs(TINY, CLASSES_3)).eval()
    x = torch.zeros(1, 3, TINY.num_frames, TINY.input_size, TINY.input_size)
    with pytest.raises(GavaError, match="HIP device"):
        m.attention_maps(x)
    with pytest.raises(GavaError, match="clip batch"):
        m.attention_maps(x[0])
    with pytest.raises(GavaError, match="clip batch"):
        m.attention_maps(x[:, :, :, :32, :32])
    with pytest.raises(GavaError, match="mode"):
        m.attention_maps(x, mode="grad")
    with pytest.raises(GavaError, match="heads"):
        m.attention_maps(x, heads="max")
    with pytest.raises(GavaError, match="heads"):
        m.attention_maps(x, mode="rollout", heads=None)
    for layer in (TINY.num_layers, -TINY.num_layers - 1, None):
        with pytest.raises(GavaError, match="outside"):
            m.attention_maps(x, mode="cls", layer=layer)
    with pytest.raises(GavaError, match="HIP device"):
        m.attention_maps(x, mode="rollout", layer=99)               # rollout ignores `layer`
    r = repr(AttentionMaps("rollout", None, torch.zeros(1, 4, 4, 4), torch.zeros(1, 4), torch.zeros(1, 3)))
    assert "rollout" in r and "patches=(1, 4, 4, 4)" in r


def test_fixture_is_consistent(golden_dir):
    """tests/golden/tiny_attention_maps.npz (tools/gen_golden_attention_maps.py): small, probabilities, and its rollout is the
    chain of its own blocks as far as the CLS rows determine it (the first step)."""
    path = os.path.join(golden_dir, "tiny_attention_maps.npz")
    assert os.path.getsize(path) < 32 << 10
    g = np.load(path)
    L, H, T, G = TINY.num_layers, TINY.num_heads, TINY.num_frames, TINY.num_global_prompts
    n = (TINY.input_size // TINY.patch_size) ** 2 + 1
    assert g["cls"].shape == (L, 2 * T, H, n + G + T + 1) and g["rollout"].shape == (2 * T, n) and g["logits"].shape == (2, 3)
    assert np.abs(g["cls"].astype(np.float64).sum(-1) - 1).max() < 1e-6 and (g["cls"] > 0).all()
    assert np.abs(g["rollout"].astype(np.float64).sum(-1) - 1).max() < 1e-6 and (g["rollout"] > 0).all()
    assert np.abs(g["logits"] - np.load(os.path.join(golden_dir, "tiny.npz"))["logits"]).max() < 1e-5
    # the CLS token keeps at least 2^-L of its own weight through L blocks of (I + A) / 2
    assert (g["rollout"][:, 0] >= 0.5 ** L).all()
