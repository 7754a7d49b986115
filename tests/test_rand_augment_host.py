"""CPU: RandAugment on the device, everything that needs no device.  The numpy restatement (tests/rand_augment_ref.py) against
what the reference's own rand_augment.py returned under Pillow (tests/golden/rand_augment_ref.npz, written by
tools/gen_golden_rand_augment.py) - every sha256 - and, where Pillow is importable, against live Pillow byte for byte; the
policy draws of gava_clip_amd.augment and of the restatement against the recorded plans and generator states; the C ABI's
structs and its refusals, which return before any launch."""
import ctypes
import hashlib
import os
import random
import subprocess

import numpy as np
import pytest

import rand_augment_ref as ref
import train_preprocess_ref as tref
from helpers import REPO

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)
CONFIGS = ("rand-m7-n4-mstd0.5-inc1", "rand-m9-n2", "rand-m5-n3-mstd1-w0")


def fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "rand_augment_ref.npz"))
    cases = []
    for c in range(int(g["n_cases"])):
        policy, n, H, W, T, rate, size, seed, vseed, flat = g[f"case_{c}"].tolist()
        args, filters = g[f"plan_args_{c}"], g[f"plan_filters_{c}"]
        plan = [(str(nm), None if np.isnan(a) else (int(a) if ("Posterize" in nm or "Solarize" in nm) else float(a)),
                 None if f[0] < 0 else [int(v) for v in f]) for nm, a, f in zip(g[f"plan_names_{c}"], args, filters)]
        case = dict(c=c, policy=bool(policy), n=n, H=H, W=W, T=T, rate=rate, size=size, seed=seed, vseed=vseed,
                    flat=None if flat < 0 else flat, name=str(g[f"cfg_{c}"][0]), interpolation=str(g[f"cfg_{c}"][1]),
                    magnitude=g[f"mag_{c}"][0], mstd=g[f"mag_{c}"][1], plan=plan, next=g[f"next_{c}"],
                    sha=g[f"sha256_{c}"].tobytes(), sample=g[f"sample_{c}"])
        if policy:
            case.update(idx=g[f"idx_{c}"].tolist(), box=tuple(g[f"box_{c}"].tolist()), clip_sha=g[f"clip_sha256_{c}"].tobytes(),
                        clip_sample=g[f"clip_sample_{c}"])
        cases.append(case)
    return cases


def source_frames(c):
    """the uint8 [T, H, W, 3] frames a case's plan is applied to"""
    v = ref.video(c["n"], c["H"], c["W"], c["vseed"], c["flat"])
    return v[c["idx"]] if c["policy"] else v


def _seed(s):
    random.seed(s)
    np.random.seed(s)


def _strided(a):
    return a.reshape(-1)[::max(1, a.size // 4096)][:4096]


# ---- 1. the fixture ---------------------------------------------------------------------------------------------------------

def test_fixture_covers_what_it_should(golden_dir):
    cs = fixture(golden_dir)
    ops = [c for c in cs if not c["policy"]]
    names = {c["name"] for c in ops}
    assert set(ref.RAND) | set(ref.RAND_INC) <= names                                        # every op of both lists
    for name in ref.GEOMETRIC[:5]:                                                           # both filters, both signs
        got = {(c["plan"][0][2][0], c["plan"][0][1] > 0) for c in ops if c["name"] == name and c["interpolation"] != "random"}
        assert {(2, True), (2, False), (3, True), (3, False)} <= got, name
    assert any(c["flat"] is not None and c["name"] in ("AutoContrast", "Equalize") for c in ops)
    tiny = [c for c in ops if c["name"] == "Equalize" and c["H"] * c["W"] < 255]
    assert tiny and all(ref.equalize_lut(np.bincount(source_frames(c)[0, :, :, 0].ravel(), minlength=256)) == list(range(256))
                        for c in tiny)                                                       # step == 0
    factors = [c["plan"][0][1] for c in ops if c["name"].replace("Increasing", "") in ("Color", "Contrast", "Brightness", "Sharpness")]
    assert any(0 <= f <= 1 for f in factors) and any(f > 1 for f in factors) and 1.0 in factors
    zero = [c for c in ops if c["name"] == "Rotate" and c["plan"][0][1] == 0]
    assert zero and all(c["mstd"] > 0 and c["magnitude"] == 0 for c in zero)                 # gauss < 0, clipped to 0: a copy
    assert any(len(set(c["plan"][0][2])) == 2 for c in ops if c["interpolation"] == "random")
    assert {(c["H"], c["W"]) for c in ops} >= {(37, 53), (3, 3), (2, 5), (1, 7), (64, 64), (5, 7)}
    policies = [c for c in cs if c["policy"]]
    assert {c["name"] for c in policies} >= set(CONFIGS) and any(c["interpolation"] == "random" for c in policies)
    assert any(len(c["plan"]) == 0 for c in policies) and any(len(c["plan"]) == 4 for c in policies)
    assert os.path.getsize(os.path.join(golden_dir, "rand_augment_ref.npz")) < 512 * 1024


def test_generated_videos_make_the_statistics_ops_work():
    """AutoContrast, Equalize and Contrast change the ramp video (they are identities on noise that fills all 256 bins)"""
    v = ref.video(2, 37, 53, 1)
    for name, arg in (("AutoContrast", None), ("Equalize", None), ("Contrast", 0.5)):
        assert (ref.apply_op(v[0], name, arg) != v[0]).mean() > 0.5, name
    flat = ref.video(1, 37, 53, 1, flat_channel=1)[0]
    assert len(np.unique(flat[..., 1])) == 1 and len(np.unique(flat[..., 0])) > 50


# ---- 2. the restatement ------------------------------------------------------------------------------------------------------

def test_restatement_reproduces_every_golden_case(golden_dir):
    for c in fixture(golden_dir):
        got = ref.apply_plan(source_frames(c), c["plan"])
        assert np.array_equal(_strided(got), c["sample"]), (c["c"], c["name"])
        assert hashlib.sha256(got.tobytes()).digest() == c["sha"], (c["c"], c["name"])
        if c["policy"]:
            clip = tref.preprocess_clip(got, range(c["T"]), *c["box"], c["size"], MEAN, STD).numpy()
            assert np.array_equal(_strided(clip), c["clip_sample"]), c["c"]
            assert hashlib.sha256(clip.tobytes()).digest() == c["clip_sha"], c["c"]


OP_ARGS = (("Rotate", (13.7, -29.0, 0.0)), ("ShearX", (0.21, -0.3)), ("ShearY", (0.17, -0.3)), ("TranslateXRel", (0.31, -0.45)),
           ("TranslateYRel", (0.2, -0.45)), ("Invert", (None,)), ("Posterize", (0, 1, 4, 8)), ("Solarize", (0, 100, 256)),
           ("SolarizeAdd", (0, 77, 110)), ("AutoContrast", (None,)), ("Equalize", (None,)), ("Brightness", (0.1, 1.0, 1.9)),
           ("Contrast", (0.1, 1.0, 1.9)), ("Color", (0.1, 1.0, 1.9)), ("Sharpness", (0.1, 1.0, 1.9)))


def test_restatement_equals_live_pillow_byte_for_byte():
    pytest.importorskip("PIL")
    for h, w in ((37, 53), (3, 3), (2, 5)):
        for flat in (None, 1):
            v = ref.video(2, h, w, 5, flat)
            for name, args in OP_ARGS:
                for arg in args:
                    for filt in ((ref.BILINEAR, ref.BICUBIC) if name in ref.GEOMETRIC else (None,)):
                        for t in range(2):
                            diff = int((ref.apply_op(v[t], name, arg, filt) != ref.pillow_op(v[t], name, arg, filt)).sum())
                            assert diff == 0, ((h, w), flat, name, arg, filt, diff)


# ---- 3. the draws ------------------------------------------------------------------------------------------------------------

def _same_plan(got, want):
    assert len(got) == len(want), (got, want)
    for (n0, a0, f0), (n1, a1, f1) in zip(got, want):
        assert n0 == n1 and a0 == a1 and (None if f0 is None else list(f0)) == f1, (got, want)


def test_plan_draws_reproduce_the_reference(golden_dir):
    """RandAugment.plan / AugmentedClipPreprocessor.sample and the restatement's draw (written independently): the recorded
    indices, plan and box of every policy case, and both generators left in the recorded state."""
    from gava_clip_amd import AugmentedClipPreprocessor, RandAugment
    for c in fixture(golden_dir):
        if c["policy"]:
            pre = AugmentedClipPreprocessor(c["name"], num_frames=c["T"], sampling_rate=c["rate"], spatial_size=c["size"],
                                            interpolation=c["interpolation"])

            def restated():
                idx = tref.draw_frames(c["n"], c["T"], c["rate"])
                plan = ref.draw_plan(c["name"], c["T"], c["interpolation"])
                return (idx, *tref.draw_box(c["H"], c["W"]), plan)

            for draw in (lambda: pre.sample(c["n"], c["H"], c["W"]), restated):
                _seed(c["seed"])
                idx, i, j, h, w, plan = draw()
                nxt = np.array([random.random(), np.random.random()])
                assert list(idx) == c["idx"] and (i, j, h, w) == c["box"], c["c"]
                _same_plan(plan, c["plan"])
                assert np.array_equal(nxt, c["next"]), c["c"]
        else:
            # one op at prob = 1: the same draw through the op-level functions of both implementations
            aug = RandAugment("rand", c["interpolation"])
            aug.magnitude, aug.magnitude_std = c["magnitude"], c["mstd"]
            for draw in (lambda: aug._draw_op(c["name"], c["T"], int(min(c["H"], c["W"]) * 0.45), prob=1.0),
                         lambda: ref.draw_op(c["name"], c["magnitude"], c["mstd"], c["T"], c["interpolation"], prob=1.0)):
                _seed(c["seed"])
                layer = draw()
                nxt = np.array([random.random(), np.random.random()])
                _same_plan([layer], c["plan"])
                assert np.array_equal(nxt, c["next"]), (c["c"], c["name"])


def test_config_strings_parse_as_upstream():
    from gava_clip_amd import RandAugment
    a = RandAugment("rand-m7-n4-mstd0.5-inc1")
    assert (a.magnitude, a.num_layers, a.magnitude_std, a.choice_weights) == (7, 4, 0.5, None) and "ColorIncreasing" in a.names
    assert "ColorIncreasing" in RandAugment("rand-inc0").names                               # bool("0") is True upstream
    b = RandAugment("rand-m9-n2")
    assert (b.magnitude, b.num_layers, b.magnitude_std) == (9, 2, None) and tuple(b.names) == tuple(ref.RAND)
    w = RandAugment("rand-m5-n3-mstd1-w0")
    assert np.array_equal(w.choice_weights, ref.parse("rand-m5-n3-mstd1-w0")[4]) and abs(w.choice_weights.sum() - 1) < 1e-12
    d = RandAugment("rand")
    assert (d.magnitude, d.num_layers) == (10.0, 2)
    assert RandAugment("rand-mstd0.5-mstd2").magnitude_std == 0.5                            # setdefault: the first one stays


# ---- 4. the ABI ---------------------------------------------------------------------------------------------------------------

NAMES = ("gava_augment_hist", "gava_augment_luts", "gava_augment_apply", "gava_augment_struct_sizes")
FIELDS = ("src", "dst", "H", "W", "kind", "op", "filter", "iarg", "factor", "lut_slot", "hist_slot", "m")


def _lib():
    import __graft_entry__ as ge
    from gava_clip_amd import hip
    from gava_clip_amd.build import needs_build
    if needs_build():
        ge.build()
    return hip.load(), hip


def test_names_are_exported_and_declared():
    import re
    lib, hip = _lib()
    header = open(os.path.join(REPO, "include", "gava_hip.h")).read()
    declared = set(re.findall(r"\b(gava_[a-z0-9_]+)\s*\(", header))
    raw = ctypes.CDLL(hip.LIB_PATH)
    for name in NAMES:
        assert name in hip.EXPORTS and name in declared and hasattr(raw, name), name
    from gava_clip_amd.build import SOURCES
    assert "augment.hip" in SOURCES


def test_structs_match_header_and_library(tmp_path):
    lib, hip = _lib()
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "gava_hip.h"\nint main(){' + \
          'printf("%zu %zu\\n", sizeof(gava_augment_desc), sizeof(gava_augment_args));' + \
          "".join(f'printf("%zu\\n", offsetof(gava_augment_desc, {f}));' for f in FIELDS) + \
          'printf("%d %d %d %d %d %d\\n", GAVA_AUG_AFFINE, GAVA_AUG_EQUALIZE, GAVA_AUG_CONTRAST, GAVA_AUG_BICUBIC, GAVA_AUG_TABLE, ' \
          'GAVA_AUG_INVERT);return 0;}'
    (tmp_path / "s.c").write_text(src)
    subprocess.check_call(["gcc", "-I", os.path.join(REPO, "include"), str(tmp_path / "s.c"), "-o", str(tmp_path / "s")])
    out = [int(v) for v in subprocess.check_output([str(tmp_path / "s")]).decode().split()]
    got = (ctypes.c_size_t * 2)()
    assert lib.gava_augment_struct_sizes(got, 2) == 2 and lib.gava_augment_struct_sizes(None, 0) == 2
    assert [ctypes.sizeof(hip.AugmentDesc), ctypes.sizeof(hip.AugmentArgs)] == out[:2] == list(got) and out[0] == 104
    assert [getattr(hip.AugmentDesc, f).offset for f in FIELDS] == out[2:2 + len(FIELDS)]
    assert out[2 + len(FIELDS):] == [hip.AUG_AFFINE, hip.AUG_EQUALIZE, hip.AUG_CONTRAST, hip.AUG_BICUBIC, hip.AUG_TABLE, hip.AUG_INVERT]
    dt = hip.augment_desc_dtype()
    assert dt.itemsize == 104 and [dt.fields[f][1] for f in FIELDS] == out[2:2 + len(FIELDS)]
    sizes17 = (ctypes.c_size_t * 32)()
    assert lib.gava_struct_sizes(sizes17, 32) == 17                                          # the closed list stays closed


def test_augment_kernels_compile_without_scratch():
    """tools/kernel_resources.py on augment.hip (cross-compiles for gfx950): the bicubic path's sixteen pixels and its fp64 chains
    stay in registers"""
    import re
    import sys
    out = subprocess.check_output([sys.executable, os.path.join(REPO, "tools", "kernel_resources.py"), "augment.hip"]).decode()
    rows = [ln for ln in out.splitlines() if "scratch" in ln]
    assert all(k in " ".join(rows) for k in ("augment_hist_kernel", "augment_luts_kernel", "augment_apply_kernel"))
    for ln in rows:
        assert int(re.search(r"scratch\s+(\d+)", ln).group(1)) == 0, ln


ONE = 1 << 20          # a non-null stand-in for a device pointer: every call below returns before it is used
EINVAL = -1


def _args(hip, rows=None, **kw):
    table = (hip.AugmentDesc * 3)()
    for i, d in enumerate(table):
        d.src, d.dst, d.H, d.W = ONE + i * 4096, (1 << 24) + i * 4096, 8, 12
        d.kind, d.op, d.filter, d.factor, d.lut_slot, d.hist_slot = hip.AUG_TABLE, hip.AUG_EQUALIZE, hip.AUG_BICUBIC, 0.5, i, i
        d.m[0] = d.m[4] = 1.0
    for i, fields in (rows or {}).items():
        for k, v in fields.items():
            if k == "m5":
                table[i].m[5] = v
            else:
                setattr(table[i], k, v)
    a = hip.AugmentArgs()
    a.desc_host, a.desc, a.hist, a.luts, a.n, a.n_hist, a.n_luts = ctypes.cast(table, ctypes.c_void_p), ONE, ONE, ONE, 3, 3, 3
    for k, v in kw.items():
        setattr(a, k, v)
    return a, table


def test_every_refusal_returns_before_a_launch():
    lib, hip = _lib()
    inf, nan = float("inf"), float("nan")
    bad_rows = [dict(src=None), dict(dst=None), dict(H=0), dict(W=0), dict(H=-3), dict(H=1 << 15, W=1 << 15),     # 2^30 pixels: 3 GiB
                dict(kind=4), dict(kind=-1), dict(op=8), dict(op=-1), dict(kind=hip.AUG_AFFINE, filter=2),
                dict(kind=hip.AUG_AFFINE, filter=-1), dict(factor=inf), dict(factor=nan), dict(m5=nan), dict(m5=-inf),
                dict(kind=hip.AUG_COLOR, factor=nan), dict(kind=hip.AUG_AFFINE, m5=inf),
                dict(dst=ONE + 4096), dict(dst=ONE + 4096 + 100),                                                 # dst == src, overlap
                dict(lut_slot=3), dict(lut_slot=-1), dict(hist_slot=3), dict(hist_slot=-1),
                dict(op=hip.AUG_POSTERIZE, iarg=-1), dict(op=hip.AUG_SOLARIZE, iarg=257)]
    for fn in (lib.gava_augment_hist, lib.gava_augment_luts, lib.gava_augment_apply):
        assert fn(None, None) == EINVAL
        for fields in bad_rows:
            a, keep = _args(hip, rows={1: fields})
            assert fn(ctypes.byref(a), None) == EINVAL, fields
        for kw in (dict(desc_host=None), dict(desc=None), dict(n=0), dict(n=-1), dict(n_hist=-1), dict(n_luts=-1), dict(hist=None),
                   dict(luts=None), dict(n_hist=2), dict(n_luts=2)):
            a, keep = _args(hip, **kw)
            assert fn(ctypes.byref(a), None) == EINVAL, kw


# ---- 5. refusals of the Python layer -------------------------------------------------------------------------------------------

def test_python_refusals_and_construction():
    from gava_clip_amd import AugmentedClipPreprocessor, RandAugment
    from gava_clip_amd.preprocess import TrainClipPreprocessor
    for interpolation in ("lanczos", "hamming"):
        with pytest.raises(ValueError, match="refuses"):
            RandAugment("rand-m9-n2", interpolation)
        with pytest.raises(ValueError):
            AugmentedClipPreprocessor("rand-m9-n2", interpolation=interpolation)
    for bad in ("augmix-m5", "", "m9-n2", None, 7, "rand-m7.5", "rand-nx2-n2x", "rand-m9-w1", "rand-mstd0.5.1", "rand-w0-n14"):
        with pytest.raises(ValueError):
            RandAugment(bad)
    with pytest.raises(ValueError):
        AugmentedClipPreprocessor(None)
    with pytest.raises(NotImplementedError, match="AugmentedClipPreprocessor"):
        TrainClipPreprocessor(auto_augment="rand-m7-n4-mstd0.5-inc1")
    pre = AugmentedClipPreprocessor("rand-m7-n4-mstd0.5-inc1", mirror=True)
    assert isinstance(pre, TrainClipPreprocessor) and pre.augment.num_layers == 4 and pre.num_frames == 8
    with pytest.raises(ValueError):
        pre.descriptors([], [([0] * 8, 0, 0, 8, 8)])            # a five-field draw has no plan
    src = open(os.path.join(REPO, "gava_clip_amd", "augment.py")).read()
    assert "import PIL" not in src and "from PIL" not in src
