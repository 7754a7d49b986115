"""CPU: what the explanation methods of VitaCLIP share (gava_clip_amd/explain.py).

  * the refusals every method makes, in their one order - the device's comes last, so all of this needs none;
  * the clips per chunk of the kept-activation forward against a brute-force statement of the rule;
  * the collector of chunked logits against the unchunked tensor, and what it allocates;
  * the target and baseline helpers on every form they take.
"""
import itertools
import os

import pytest
import torch

from gava_clip_amd import VitaCLIP, explain, synth, training
from gava_clip_amd.config import TINY
from gava_clip_amd.hip import GavaError
from helpers import CLASSES_3, model_kwargs

S, T, G = TINY.input_size, TINY.num_frames, TINY.input_size // TINY.patch_size
SCORES = torch.zeros(1, T, G, G)

# method -> the call with everything but x (and what a case overrides) right
CALLS = {
    "saliency": lambda m, x, **kw: m.saliency(x, **kw),
    "attention_maps": lambda m, x, **kw: m.attention_maps(x, **kw),
    "relevance_maps": lambda m, x, **kw: m.relevance_maps(x, **kw),
    "perturbation_curves": lambda m, x, **kw: m.perturbation_curves(x, SCORES, **kw),
    "faithfulness": lambda m, x, **kw: m.faithfulness(x, **kw),
    "integrated_gradients": lambda m, x, **kw: m.integrated_gradients(x, **kw),
    "smooth_grad": lambda m, x, **kw: m.smooth_grad(x, **kw),
}
NO_TARGET = ("attention_maps",)
BASELINE = ("perturbation_curves", "integrated_gradients")


@pytest.fixture(scope="module")
def plain_model():
    return VitaCLIP(**model_kwargs(TINY, CLASSES_3)).eval()


@pytest.fixture(scope="module")
def descriptor_model(tmp_path_factory):
    """A ragged (use_descriptor) head, as tests/test_gpu_relevance.py builds it; its knowledge files are read from ./data."""
    root, cwd = tmp_path_factory.mktemp("descriptors"), os.getcwd()
    synth.synth_descriptor_files(str(root), "updrs", (2, 3, 1))
    os.chdir(root)
    try:
        return VitaCLIP(**{**model_kwargs(TINY, CLASSES_3), "text_prompt_init": "cntn_split_uni_disc",
                           "knowledge_version": ["v1", "v2", "v3"], "use_descriptor": True}).eval()
    finally:
        os.chdir(cwd)


@pytest.mark.parametrize("name", sorted(CALLS))
def test_shared_refusals_in_their_order(name, plain_model, descriptor_model):
    m, call = plain_model, CALLS[name]
    x = torch.zeros(1, 3, T, S, S)

    def refused(match, x_, model=m, **kw):
        with torch.no_grad(), pytest.raises(GavaError, match=match) as e:
            call(model, x_, **kw)
        return str(e.value)

    # the clip batch: rank, dtype, channels, size, no clips, no tensor
    for bad in (x[0], x.long(), torch.zeros(1, 4, T, S, S), torch.zeros(1, 3, T, S // 2, S // 2), torch.zeros(1, 3, T, S, S // 2),
                torch.zeros(0, 3, T, S, S), None):
        assert refused("floating-point clip batch", bad).startswith(f"{name} takes")
    if name not in NO_TARGET:
        for target in (3, -1):
            assert refused("outside the 3 classes", x, target=target).startswith(f"{name}: target {target}")
        for target in (torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64)):
            assert refused(r"a tensor target must be int64 \[1\]", x, target=target).startswith(f"{name}:")
        refused("HIP device", x, target=torch.zeros(1, dtype=torch.int64))       # a right target on the CPU: the no-CPU-fallback refusal
        refused("HIP device", x, target=2)
    if name in BASELINE:
        for baseline in ("mean", torch.zeros(4), torch.zeros(1, 3, T, S, S // 2), torch.zeros(3, dtype=torch.int64), None):
            assert refused("baseline must be", x, baseline=baseline).startswith(f"{name}:")
        for baseline in ("zero", "blur", torch.zeros(3), torch.zeros_like(x)):
            refused("HIP device", x, baseline=baseline)
    assert refused("per-descriptor", x, model=descriptor_model).startswith(f"{name}:")
    assert "no CPU fallback" in refused("HIP device", x)                          # everything about the call is right but the device
    # the order: the clip batch before the head, the head before the target, the target before the baseline, the device last
    assert "HIP device" not in refused("clip batch", x[0])
    refused("clip batch", x[0], model=descriptor_model)
    if name not in NO_TARGET:
        refused("clip batch", x[0], target=3)
        refused("per-descriptor", x, model=descriptor_model, target=3)
    if name in BASELINE:
        refused("outside the 3 classes", x, target=3, baseline="mean")


def test_groups_rule_of_the_kept_forward(plain_model):
    """attention_maps and relevance_maps take whole num_frames groups; _check_clips(groups=True) returns the fewest clips that are."""
    m = plain_model
    for frames, unit in ((T, 1), (2 * T, 1), (T // 2, 2), (3, 4)):
        x = torch.zeros(unit, 3, frames, S, S)
        assert m._check_clips("f", x, groups=True) == (unit, frames, unit) and m._check_clips("f", x) == (unit, frames)
        assert m._check_clips("f", torch.zeros(3 * unit, 3, frames, S, S), groups=True) == (3 * unit, frames, unit)
        if unit > 1:
            for call in (m.attention_maps, m.relevance_maps):
                with pytest.raises(GavaError, match=f"{unit + 1} clips of {frames} frames are not whole groups of num_frames = {T}"):
                    call(torch.zeros(unit + 1, 3, frames, S, S))


def _brute_force_step(B, frames, unit, max_clips, kept_bytes, budget):
    """The rule in words: with max_clips, the largest multiple of unit not above it, at least unit, at most B; without, the
    first member of the sequence B / unit, ceil(half), ceil(half of that), ..., 1 (in units) whose kept bytes fit, else one unit."""
    if max_clips is not None:
        return min(B, max([k for k in range(unit, max_clips + 1, unit)] or [unit]))
    seq = [B // unit]
    while seq[-1] > 1:
        seq.append(-(-seq[-1] // 2))
    return next((n * unit for n in seq if kept_bytes(n * unit, frames) <= budget), unit)


def test_group_step_against_the_rule_in_words(plain_model, monkeypatch):
    m = plain_model
    linear = lambda clips, frames: 1000 * clips * frames
    monkeypatch.setattr(training, "kept_bytes", lambda model, clips, frames: linear(clips, frames))
    seen = set()
    for frames in (T, 2 * T, T // 2, 3):
        unit = m._check_clips("f", torch.zeros(4, 3, frames, S, S), groups=True)[2]
        for B in (unit, 2 * unit, 5 * unit):
            for budget in (linear(B, frames), 0, linear(2 * unit, frames)):            # fits everything, nothing, exactly two units
                monkeypatch.setattr(m, "keep_activation_bytes", budget)
                got = m._group_step(B, frames, unit, None)
                assert got == _brute_force_step(B, frames, unit, None, linear, budget), (frames, B, budget)
                assert got % unit == 0 and unit <= got <= B
                seen.add(got // unit)
            for max_clips in (1, unit, unit + 1, 2 * unit, 3 * unit - 1, 3 * unit, 5 * unit, 100):
                got = m._group_step(B, frames, unit, max_clips)
                assert got == _brute_force_step(B, frames, unit, max_clips, None, None), (frames, B, max_clips)
                assert got % unit == 0 and unit <= got <= B
    assert seen == {1, 2, 5}                # 5 units: all of them, two (5 -> 3 -> 2) and one


@pytest.mark.parametrize("B,m", itertools.product((1, 2, 5), (1, 3)))
def test_row_collector_equals_the_unchunked_tensor(B, m, monkeypatch):
    C = 3
    full = torch.arange(B * m * C, dtype=torch.float32).view(B * m, C)
    chunk = lambda i, nb: full[i * m:(i + nb) * m].clone()                             # the fake per-chunk forward
    made, empty = [], torch.empty

    def counting_empty(*a, **kw):
        made.append(tuple(a))
        return empty(*a, **kw)

    for step in sorted({1, 2, B - 1, B, B + 1} - {0}):
        rows, given = explain._Rows(B * m), []
        del made[:]
        monkeypatch.setattr(torch, "empty", counting_empty)
        try:
            for i in range(0, B, step):
                given.append(chunk(i, min(step, B - i)))
                rows.put(i * m, given[-1])
        finally:
            monkeypatch.setattr(torch, "empty", empty)
        assert torch.equal(rows.out, full), step
        if step >= B:
            assert rows.out is given[0] and made == []                                 # one chunk covers the batch: the very tensor
        else:
            assert made == [(B * m, C)] and rows.out.dtype == torch.float32            # one allocation, of the full size


def test_target_and_baseline_helpers(plain_model):
    m = plain_model
    x = torch.zeros(2, 3, T, S, S)
    assert m._as_target(None, 2, x.device) is None
    t = torch.tensor([2, 0])
    assert m._as_target(t, 2, x.device) is t
    full = m._as_target(1, 5, x.device)
    assert full.dtype == torch.int64 and full.tolist() == [1] * 5 and full.device == x.device
    assert m._n_classes() == 3
    like = torch.arange(x.numel(), dtype=torch.float64).view(x.shape)
    forms = (("zero", "zero"), ("blur", "blur"), (torch.ones(3), "tensor"), (torch.ones(3, dtype=torch.float16), "tensor"), (like, "tensor"))
    for baseline, kind in forms:
        assert m._check_baseline("f", baseline, x) == kind
    assert m._make_baseline("zero", "zero", x, None) is None
    for baseline in (torch.ones(3, dtype=torch.float16), like, like.transpose(3, 4)):
        base = m._make_baseline("tensor", baseline, x, None)
        assert base.dtype == torch.float32 and base.is_contiguous() and torch.equal(base.double(), baseline.double())
    # a chunk's rows: a full-size baseline is sliced, None and [3] serve every clip
    channel, full_size = torch.ones(3), like.float()
    assert m._base_rows(None, 1, 1) is None and m._base_rows(channel, 1, 1) is channel
    assert torch.equal(m._base_rows(full_size, 1, 1), full_size[1:2]) and m._base_rows(full_size, 0, 2).shape == x.shape
