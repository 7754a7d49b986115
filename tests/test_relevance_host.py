"""CPU: the host side of the relevance maps (gava_attention_relevance, hip.attention_relevance, VitaCLIP.relevance_maps).

  * the relevance chain the device runs equals the matrix product it stands for;
  * with every product P G <= 0 the reference is exactly 0, and so is the emulation;
  * the emulation of the kernel's rounding points stays within half the bound on every shape, form, regime, kind of dout and
    precision pair the GPU test uses;
  * every applicable mutation of the reference misses the bound by 10x or more;
  * the C ABI's surface: names, the struct mirror, the argument checks that return before any launch;
  * code generation: every instantiation of the new kernel compiles without scratch;
  * the Python refusals that need no device, and the two reference fixtures' own consistency.
"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import relevance_ref as rr
from relevance_ref import F16, BF16
from gava_clip_amd.config import TINY, VIT_B16_T8
from helpers import REPO, CLASSES_3, model_kwargs

NAMES = ("gava_attention_relevance", "gava_attention_relevance_struct_sizes")
EMU_SHARE = 0.5          # the emulation within half the bound: the other half is what it does not model
MUT_FACTOR = 10.0


def case_params(c):
    return [p for p in rr.params() if p[0] is c]


def _case(c, form, regime, kind, pair):
    seed = rr.seed_of(c, regime)
    return rr.make_inputs(c, regime, seed, pair[0], pair[1], kind), rr.weights(c, form, seed)


def test_chain_equals_matrix_product():
    g = torch.Generator().manual_seed(5)
    for n, L in ((197, 12), (17, 2), (5, 1)):
        A = torch.rand(L, n, n, generator=g, dtype=torch.float64) * (torch.rand(L, n, n, generator=g, dtype=torch.float64) < 0.3) / n
        chain, mat = rr.relevance_chain(A), rr.relevance_matrix(A)
        assert float((chain - mat).abs().max()) <= 1e-12
        assert float(chain[0]) >= 1 and bool((chain >= 0).all())
    A = torch.rand(1, 4, 4, dtype=torch.float64)                        # one block: r = e_cls + A[0]
    want = A[0, 0].clone()
    want[0] += 1
    assert torch.allclose(rr.relevance_chain(A), want, rtol=0, atol=1e-15)


def test_all_negative_products_give_exactly_zero():
    for c in (rr.TABLE[0], rr.cls(rr.TABLE[0])):
        for pair in rr.PAIRS:
            x, w = _case(c, rr.forms(c)[0], "randn", "negative", pair)
            ref, smax, A = rr.reference(c, x, pair[0], w)
            assert float(ref.abs().max()) == 0.0 and float(A.min()) > 0           # the bound's scale does not vanish with it
            assert float(rr.emulate(c, x, pair[0], w).abs().max()) == 0.0
            assert float(rr.reference(c, x, pair[0], w, mutate="no_clamp")[0].max()) < 0


def test_reference_converts_v_as_the_kernel_does():
    """fp16 activations under bf16 gradients: V enters G rounded to bf16, and that rounding is far above the bound."""
    c = rr.TABLE[0]
    x, w = _case(c, "chain", "randn", "random", (BF16, F16))
    assert x.v.dtype == torch.float16 and x.dout.dtype == torch.bfloat16 and bool((x.v.to(torch.bfloat16).to(torch.float16) != x.v).any())
    ref, smax, A = rr.reference(c, x, BF16, w)
    unconverted, _, _ = rr.reference(c, x, F16, w)                      # prec = act: `values` leaves V alone
    assert rr.ratio(c, unconverted, ref, smax, A) >= MUT_FACTOR


@pytest.mark.parametrize("c", rr.TABLE, ids=rr.ar.case_id)
def test_emulation_within_half_the_bound(c):
    for _, form, regime, kind, pair in case_params(c):
        x, w = _case(c, form, regime, kind, pair)
        ref, smax, A = rr.reference(c, x, pair[0], w)
        emu = rr.emulate(c, x, pair[0], w)
        assert emu.shape == ref.shape == (c.BT, c.heads, c.n) and torch.isfinite(emu).all()
        r = rr.ratio(c, emu, ref, smax, A)
        assert r <= EMU_SHARE, (rr.param_id(c, form, regime, kind, pair), r)
        assert float((rr.bound(c, smax, A) / A).max()) < 1e-4


def test_table_covers_what_the_issue_lists():
    assert {rr.n_keys(c) for c in rr.TABLE} == {26, 214, 298, 594} and rr.n_keys(rr.TOO_MANY) == 641
    assert {(rr.n_keys(c) + 15) // 16 for c in rr.TABLE} == {2, 14, 19, 38}          # one per LDS class: <= 4, <= 14, <= 26, <= 40 tiles
    assert all(c.BT == 2 * c.T and c.heads == 2 for c in rr.TABLE)
    for keys in (26, 214, 298, 594):
        assert {rr.n_queries(c) == 1 for c in rr.TABLE if rr.n_keys(c) == keys} == {True, False}
    assert any(c.n_q == 1 and c.qbr > 1 for c in rr.TABLE)
    ps = rr.params()
    assert {p[2] for p in ps} == set(rr.REGIMES) and {p[3] for p in ps} == set(rr.KINDS) and {p[4] for p in ps} == set(rr.PAIRS)


@pytest.mark.parametrize("mutation", rr.MUTATIONS)
def test_mutated_reference_misses_the_bound_tenfold(mutation):
    seen = set()
    for c, form, regime, kind, pair in rr.params():
        if rr.n_keys(c) > 214 or not rr.mutation_applies(c, regime, kind, mutation):
            continue
        x, w = _case(c, form, regime, kind, pair)
        ref, smax, A = rr.reference(c, x, pair[0], w)
        mut, _, _ = rr.reference(c, x, pair[0], w, mutate=mutation)
        r = rr.ratio(c, mut, ref, smax, A)
        assert r >= MUT_FACTOR, (rr.param_id(c, form, regime, kind, pair), r)
        seen.add((regime, kind))
    absent = {"renorm_own": {"ramp_down"}, "drop_last": {"ramp_down"}}.get(mutation, set())
    assert {r for r, _ in seen} == set(rr.REGIMES) - absent, seen
    zero_ok = mutation in ("no_clamp", "abs", "k_for_v")
    assert {k for _, k in seen} == (set(rr.KINDS) if zero_ok else {"random", "mixed"}), seen


def test_new_names_are_exported_and_declared():
    import gava_clip_amd
    from gava_clip_amd import hip
    header = open(os.path.join(REPO, "include", "gava_hip.h")).read()
    declared = set(re.findall(r"\b(gava_[a-z0-9_]+)\s*\(", header))
    for name in NAMES:
        assert name in hip.EXPORTS and name in declared, name
    from gava_clip_amd.build import SOURCES
    assert "attention_relevance.hip" in SOURCES
    assert hip.ATTENTION_RELEVANCE_MAX_KEYS == rr.MAX_KEYS == 640 and "n_kmain + n_side <= 640" in header
    assert callable(hip.attention_relevance)
    from gava_clip_amd.model import RelevanceMaps, VitaCLIP
    assert gava_clip_amd.RelevanceMaps is RelevanceMaps and callable(VitaCLIP.relevance_maps)
    doc = VitaCLIP.relevance_maps.__doc__
    assert "NOT normalised" in doc and "NOT attributed" in doc
    r = repr(RelevanceMaps(torch.zeros(1, 4, 4, 4), torch.zeros(1, 4), torch.zeros(1, 3), torch.zeros(1, dtype=torch.int64)))
    assert "patches=(1, 4, 4, 4)" in r and "target=(1,)" in r


def test_struct_matches_header_and_library(tmp_path):
    """sizeof as the C compiler sees the header == the ctypes mirror == what the library reports."""
    from gava_clip_amd import hip
    from gava_clip_amd.build import build
    build(verbose=False)                                               # a no-op unless the library is missing or stale
    src = '#include <stdio.h>\n#include "gava_hip.h"\nint main(){printf("%zu\\n", sizeof(gava_attention_relevance_args));return 0;}'
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    size = int(subprocess.check_output([str(tmp_path / "s")]).decode())
    lib = hip.load()
    got = (ctypes.c_size_t * 1)()
    assert lib.gava_attention_relevance_struct_sizes(got, 1) == 1
    assert ctypes.sizeof(hip.AttentionRelevanceArgs) == size == got[0]
    assert lib.gava_attention_relevance_struct_sizes(None, 0) == 1     # a zero capacity writes nothing


ONE = 64      # a non-null, 16-byte aligned stand-in for a device pointer: every call below returns before it is used


def _args(hip, **kw):
    """A valid call: ViT-B/16 at T = 8, every query of a block, fp16 activations under bf16 gradients."""
    a = hip.AttentionRelevanceArgs()
    a.q, a.k, a.v, a.ld_qkv, a.side_k, a.ld_side, a.dout, a.ld_dout, a.w, a.out = ONE, ONE, ONE, 2304, ONE, 1536, ONE, 768, ONE, ONE
    a.batch, a.heads, a.n_q, a.n_kmain, a.n_g, a.T, a.has_summary = 16, 12, 197, 197, 8, 8, 1
    a.prec, a.act_prec_set, a.act_prec = hip.PREC_BF16, 1, hip.PREC_F16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_attention_relevance_refuses_bad_arguments_before_any_launch():
    """GAVA_EINVAL (-1) comes back before anything touches the device, so this runs without one."""
    from gava_clip_amd import hip
    lib = hip.load()
    call = lambda **kw: lib.gava_attention_relevance(ctypes.byref(_args(hip, **kw)), None)
    assert lib.gava_attention_relevance(None, None) == -1
    for field in ("q", "k", "v", "dout", "out"):                                                # null pointers
        assert call(**{field: None}) == -1, field
    for field in ("q", "k", "v", "dout", "side_k"):                                             # misaligned operands
        assert call(**{field: ONE + 8}) == -1, field
    assert call(w=ONE + 2) == -1 and call(out=ONE + 1) == -1
    for field in ("batch", "heads", "n_q", "n_kmain"):
        assert call(**{field: 0}) == -1 and call(**{field: -1}) == -1, field
    assert call(ld_qkv=2300) == -1 and call(ld_qkv=760) == -1                                   # not a multiple of 8; below heads*64
    assert call(ld_dout=764) == -1 and call(ld_dout=760) == -1
    assert call(ld_side=1532) == -1 and call(ld_side=760) == -1 and call(ld_q=12, q_batch_rows=197) == -1
    assert call(side_k=None) == -1 and call(T=0) == -1 and call(T=5) == -1 and call(n_g=-1) == -1   # side rows: no matrix; batch % T
    assert call(n_kmain=624, n_q=1) == -1                                                       # 641 keys
    assert call(n_q=198) == -1                                                                  # more queries than rows of the frame
    assert call(q_batch_rows=196) == -1                                                         # fewer buffer rows than queries
    assert call(prec=2) == -1 and call(prec=-1) == -1 and call(act_prec=2) == -1
    assert call(prec=hip.PREC_F16, act_prec=hip.PREC_BF16) == -1                                # no such pairing
    assert call(prec=2, act_prec_set=0) == -1


def test_kernels_compile_without_scratch():
    """tools/kernel_resources.py on the new file (cross-compiles for gfx950): scratch 0 for every instantiation - four LDS
    classes x three precision pairs - and the largest class within the 160 KiB of a CU."""
    out = subprocess.check_output([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "attention_relevance.hip"]).decode()
    print(out)
    rows = [ln for ln in out.splitlines() if "scratch" in ln]
    assert len(rows) == 12 and all("attention_relevance_kernel<" in ln for ln in rows)
    for pair in ("PrecF16, PrecF16", "PrecBF16, PrecBF16", "PrecF16, PrecBF16"):
        for nkt in (4, 14, 26, 40):
            assert any(f"attention_relevance_kernel<{pair}, {nkt}>" in ln for ln in rows), (pair, nkt)
    for ln in rows:
        assert int(re.search(r"scratch\s+(\d+)", ln).group(1)) == 0, ln
        assert int(re.search(r"lds\s+(\d+)", ln).group(1)) <= 160 * 1024, ln


def test_python_refusals():
    from gava_clip_amd import hip
    E = hip.GavaError
    q = torch.zeros(8, 128, dtype=torch.float16)
    with pytest.raises(E, match="HIP device"):
        hip.attention_relevance(q, q, q, q, batch=2, heads=2, n_q=4, n_kmain=4, prec=hip.PREC_F16)


def test_relevance_maps_refusals_without_a_device():
    from gava_clip_amd import VitaCLIP
    from gava_clip_amd.hip import GavaError
    m = VitaCLIP(**model_kwargs(TINY, CLASSES_3)).eval()
    x = torch.zeros(1, 3, TINY.num_frames, TINY.input_size, TINY.input_size)
    with pytest.raises(GavaError, match="HIP device"):
        m.relevance_maps(x)
    with pytest.raises(GavaError, match="clip batch"):
        m.relevance_maps(x[0])
    with pytest.raises(GavaError, match="clip batch"):
        m.relevance_maps(x[:, :, :, :32, :32])
    with pytest.raises(GavaError, match="clip batch"):
        m.relevance_maps(x.to(torch.uint8))


def test_fixtures_are_consistent(golden_dir):
    """tests/golden/{tiny,c1}_relevance.npz (tools/gen_golden_relevance.py): small, data only, the forward they came from is
    the existing fixtures', the target is its top-1, and the values are what a relevance chain can give."""
    for name, base, cfg in (("tiny_relevance", "tiny", TINY), ("c1_relevance", "c1_b16", VIT_B16_T8)):
        path = os.path.join(golden_dir, name + ".npz")
        assert os.path.getsize(path) < 32 << 10
        g = np.load(path)
        assert sorted(g.files) == ["logits", "relevance", "target"]
        n = (cfg.input_size // cfg.patch_size) ** 2 + 1
        assert g["relevance"].shape == (2 * cfg.num_frames, n) and g["relevance"].dtype == np.float32
        assert g["logits"].shape == (2, 3) and g["target"].shape == (2,) and g["target"].dtype == np.int64
        assert np.abs(g["logits"] - np.load(os.path.join(golden_dir, base + ".npz"))["logits"]).max() < 1e-5
        assert (g["target"] == g["logits"].argmax(1)).all()
        r = g["relevance"]
        assert np.isfinite(r).all() and (r[:, 0] >= 1).all() and (r[:, 1:] >= 0).all() and (r[:, 1:].max(1) > 0).all()
