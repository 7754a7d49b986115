"""The explanation methods of ``VitaCLIP`` - saliency, attention_maps, relevance_maps, perturbation_curves, faithfulness,
integrated_gradients, smooth_grad - as a mixin (``_Explain``, the idiom of model._HipHost), the steps they share, and the
classes of what they return.

Every method refuses in one order: its own arguments, the clip batch, what depends on the batch's shape, the single-logit
head, the target, max_clips, the baseline and, last, the device - so everything but the device is checked without one.
All arithmetic runs in the HIP kernels (gava_clip_amd/hip.py), through the model's own forward and the vision tower's
backward (gava_clip_amd/training.py); there is no CPU fallback.
"""
import math

import torch

from . import hip, training


class AttentionMaps:
    """What VitaCLIP.attention_maps returns: fp32 device tensors, B clips of T frames as given.
      mode, layer          what was asked for (layer: the block's index from 0; None for "rollout")
      patches [B, T, g, g] the CLS token's attention (or rollout) on the frame's patches, g = S / P
      cls     [B, T]       ... on the CLS token itself
      logits  [B, C]       the inference head on this forward's features
    and for mode "cls" (None for "rollout"; with heads=None every map carries a head axis after T):
      global_prompts [B, T, G], local_prompts [B, T, num_frames] (frame t's CLS on the local prompt of frame t' of its
      num_frames group), summary [B, T]; the five groups of a frame sum to 1."""
    __slots__ = ("mode", "layer", "patches", "cls", "logits", "global_prompts", "local_prompts", "summary")

    def __init__(self, mode, layer, patches, cls, logits, global_prompts=None, local_prompts=None, summary=None):
        self.mode, self.layer, self.patches, self.cls, self.logits = mode, layer, patches, cls, logits
        self.global_prompts, self.local_prompts, self.summary = global_prompts, local_prompts, summary

    def __repr__(self):
        shapes = ", ".join(f"{k}={tuple(getattr(self, k).shape)}" for k in self.__slots__[2:] if getattr(self, k) is not None)
        return f"AttentionMaps(mode={self.mode!r}, layer={self.layer!r}, {shapes})"


class RelevanceMaps:
    """What VitaCLIP.relevance_maps returns: fp32 device tensors, B clips of T frames as given.
      patches [B, T, g, g] the relevance of the frame's patches for the target class, g = S / P; >= 0, not normalised
      cls     [B, T]       ... of the CLS token itself; >= 1
      logits  [B, C]       the raw logits of the forward that was differentiated
      target  [B]          int64: the class each clip was asked about"""
    __slots__ = ("patches", "cls", "logits", "target")

    def __init__(self, patches, cls, logits, target):
        self.patches, self.cls, self.logits, self.target = patches, cls, logits, target

    def __repr__(self):
        return "RelevanceMaps(" + ", ".join(f"{k}={tuple(getattr(self, k).shape)}" for k in self.__slots__) + ")"


class PerturbationCurves:
    """What VitaCLIP.perturbation_curves returns, B clips and S1 steps:
      mode                 "deletion" or "insertion"
      fractions [S1]       fp32 HOST tensor: the share of a ranking's units perturbed at each step (the curves' abscissae)
      logit     [B, S1]    fp32: the target's raw logit on the perturbed clip
      prob      [B, S1]    fp32: its softmax probability
      top1      [B, S1]    int32: the perturbed clip's top-1 class (lowest class on ties)
      auc_logit, auc_prob [B]  fp32: the areas under the two curves (trapezoids over fractions)
      target    [B]        int64: the class each clip was asked about
      ranks     [B, n]     int32: the ranking the perturbation followed, per unit in the scores' own order (0 = first)
    everything but fractions on the device."""
    __slots__ = ("mode", "fractions", "logit", "prob", "top1", "auc_logit", "auc_prob", "target", "ranks")

    def __init__(self, mode, fractions, logit, prob, top1, auc_logit, auc_prob, target, ranks):
        self.mode, self.fractions, self.logit, self.prob, self.top1 = mode, fractions, logit, prob, top1
        self.auc_logit, self.auc_prob, self.target, self.ranks = auc_logit, auc_prob, target, ranks

    def __repr__(self):
        return f"PerturbationCurves(mode={self.mode!r}, " + ", ".join(f"{k}={tuple(getattr(self, k).shape)}" for k in self.__slots__[1:]) + ")"


class PathAttribution:
    """What VitaCLIP.integrated_gradients returns, B clips of T frames as given; device tensors unless said otherwise:
      maps     fp32 [B, T, S, S] (reduce "sum", "abs", "absmax", "l2") or [B, 3, T, S, S] (reduce=None)
      logits   [B, C]      the raw logits of x itself (the path's last step)
      target   [B]         int64: the class each clip was asked about
      sum_attr [B]         fp32: the clip's summed attribution (None with multiply=False)
      delta    [B]         fp32: the completeness residual sum_attr - (f(x) - f(x0)) for the target's logit (None with
                           multiply=False); what is left is the quadrature's error and the bf16 gradient operands'
      alpha, w [m]         fp32 HOST tensors: the path's points and their weights, zero-weight endpoints included"""
    __slots__ = ("maps", "logits", "target", "sum_attr", "delta", "alpha", "w")

    def __init__(self, maps, logits, target, sum_attr, delta, alpha, w):
        self.maps, self.logits, self.target, self.sum_attr, self.delta, self.alpha, self.w = maps, logits, target, sum_attr, delta, alpha, w

    def __repr__(self):
        return "PathAttribution(" + ", ".join(f"{k}={tuple(getattr(self, k).shape)}" for k in self.__slots__ if getattr(self, k) is not None) + ")"


class Faithfulness(dict):
    """What VitaCLIP.faithfulness returns: {method: {"deletion": PerturbationCurves, "insertion": PerturbationCurves}}, the
    methods in the order asked for and the control "random" last.  table() is the text a user reads: per method the mean
    areas over the clips (a faithful map has a LOW deletion area and a HIGH insertion area; "random" is the floor to beat).
    table() copies the areas to the host, so it waits for the device; building the object does not."""

    def table(self):
        rows = [f"{'method':<12}{'del auc_prob':>14}{'ins auc_prob':>14}{'del auc_logit':>15}{'ins auc_logit':>15}"]
        for name, c in self.items():
            d, i = c["deletion"], c["insertion"]
            rows.append(f"{name:<12}{float(d.auc_prob.mean()):>14.4f}{float(i.auc_prob.mean()):>14.4f}"
                        f"{float(d.auc_logit.mean()):>15.4f}{float(i.auc_logit.mean()):>15.4f}")
        return "\n".join(rows)


class _Rows:
    """The logits of a call that runs its clips in chunks.  A chunk that covers every row is kept as the tensor it is; else
    [rows, C] fp32 is allocated once, with the first chunk, and every chunk fills its rows."""

    def __init__(self, rows):
        self.rows, self.out = rows, None

    def put(self, lo, lg):
        if lg.shape[0] == self.rows:
            self.out = lg
            return
        if self.out is None:
            self.out = torch.empty(self.rows, lg.shape[-1], dtype=torch.float32, device=lg.device)
        self.out[lo:lo + lg.shape[0]] = lg


class _Explain:
    """The explanation methods of VitaCLIP and the steps they share.  Expects what VitaCLIP has: `_shape`, `num_frames`,
    `prompt_learner` or `text_features`, `_forward_impl`, `encode_video`, `local_logits`, the text cache of _HipHost."""

    # ---- the shared refusals ----------------------------------------------------------------------
    def _check_clips(self, what, x, groups=False):
        """-> (B, T) of a floating-point clip batch [B, 3, T, S, S] of the model's size; with groups=True also the rule of the
        kept-activation forward - the B*T frames are whole num_frames groups - and -> (B, T, unit), unit = the fewest clips
        that are whole groups."""
        S, Tm = self._shape["size"], self.num_frames
        if not (torch.is_tensor(x) and x.dim() == 5 and x.is_floating_point() and x.shape[1] == 3 and x.shape[3] == x.shape[4] == S
                and x.shape[0] > 0 and x.shape[2] > 0):
            raise hip.GavaError(f"{what} takes a floating-point clip batch [B, 3, T, {S}, {S}], got "
                                f"{(x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x)}")
        B, T = x.shape[0], x.shape[2]
        if not groups:
            return B, T
        unit = Tm // math.gcd(T, Tm)
        if B % unit:
            raise hip.GavaError(f"{what}: {B} clips of {T} frames are not whole groups of num_frames = {Tm}")
        return B, T, unit

    def _check_single_logit(self, what):
        if self.use_text_prompt_learning and self.prompt_learner.n_kv is None:
            raise hip.GavaError(f"{what}: a per-descriptor (use_descriptor / desc_wise) head has no single logit per class")

    def _n_classes(self):
        return self.prompt_learner.n_cls if self.use_text_prompt_learning else self.text_features.shape[0]

    def _check_target(self, what, target, B):
        """target: None, an int (checked against the number of classes) or an int64 [B] tensor (not range-checked: that
        would wait for the device)."""
        if target is None:
            return
        if not torch.is_tensor(target):
            if not 0 <= int(target) < self._n_classes():
                raise hip.GavaError(f"{what}: target {target} is outside the {self._n_classes()} classes")
        elif not (target.dtype == torch.int64 and tuple(target.shape) == (B,)):
            raise hip.GavaError(f"{what}: a tensor target must be int64 [{B}] on the device")

    @staticmethod
    def _as_target(target, B, device):
        """A checked target as the kernels take it: int64 [B] on the device (a tensor is passed through, None stays None)."""
        if target is None or torch.is_tensor(target):
            return target
        return torch.full((B,), int(target), dtype=torch.int64, device=device)

    @staticmethod
    def _check_baseline(what, baseline, x):
        """-> the baseline's kind: "zero", "blur" or "tensor" (floating point, [3] or shaped like x)."""
        kind = baseline if isinstance(baseline, str) else "tensor"
        if kind not in ("zero", "blur", "tensor") or (kind == "tensor" and not (
                torch.is_tensor(baseline) and baseline.is_floating_point() and (tuple(baseline.shape) == (3,) or baseline.shape == x.shape))):
            raise hip.GavaError(f"{what}: baseline must be 'zero', 'blur', a floating-point tensor [3] or one shaped like x, got "
                                f"{(baseline.dtype, tuple(baseline.shape)) if torch.is_tensor(baseline) else baseline!r}")
        return kind

    @staticmethod
    def _make_baseline(kind, baseline, x, taps):
        """The baseline of the fp32 device clips x as the kernels take it: None (zero), fp32 [3] or fp32 shaped like x."""
        if kind == "zero":
            return None
        if kind == "blur":
            # the few dozen taps go up from pinned memory on the stream: a pageable copy would be the call's one host wait
            return hip.blur_clips(x, taps.pin_memory().to(x.device, non_blocking=True))
        return baseline.detach().to(x.device).float().contiguous()

    @staticmethod
    def _base_rows(base, i, nb):
        """The baseline of clips [i, i + nb): a full-size one is sliced, None and [3] serve every clip."""
        return base[i:i + nb] if base is not None and base.dim() == 5 else base

    @staticmethod
    def _check_device(*tensors):
        """The last refusal of every method, in the forward's own words: there is no CPU fallback."""
        if not all(t.is_cuda for t in tensors if torch.is_tensor(t)):
            raise hip.GavaError("VitaCLIP (gava_clip_amd) runs on the HIP device only: move the model and the "
                                "input with .cuda(); there is no CPU fallback")

    # ---- the shared steps -------------------------------------------------------------------------
    def _group_step(self, B, T, unit, max_clips):
        """Clips per chunk of the kept-activation forward, in whole num_frames groups (multiples of unit): max_clips rounded
        down, never below unit nor above B; without it all B clips, halved (rounding up to a group) until the chunk's kept
        activations (training.kept_bytes) fit keep_activation_bytes or one unit is left."""
        if max_clips is not None:
            return min(B, max(int(max_clips) // unit * unit, unit))
        step = B // unit * unit
        while step > unit and training.kept_bytes(self, step, T) > self.keep_activation_bytes:
            step = (step // unit + 1) // 2 * unit
        return step

    def _class_gradient(self, xg, request, target, m=1, ref_step=0):
        """The gradient every map starts from: the grad-enabled forward of the leaf xg with the input request (see
        training.VisionTowerFn), the score sum_b logits[b, target_b] and the vision tower's backward, nothing else.  xg holds m
        copies of every clip, copy-minor.  target: per clip - None (the top-1 class of its copy ref_step, picked on the device),
        an int or int64 [B].  Detaches text_features, the last reference into the graph.
        -> (d score / d xg, or None where the request's fold took it; logits, detached; target int64 [B])."""
        with torch.enable_grad():
            logits = self._forward_impl(xg, None, None, False, input_request=request)[0]
            if target is None:
                target = logits.detach().view(-1, m, logits.shape[-1])[:, ref_step].argmax(dim=1)
            else:
                target = self._as_target(target, xg.shape[0] // m, xg.device)
            score = logits.gather(1, (target.repeat_interleave(m) if m > 1 else target).view(-1, 1)).sum()
            (dx,) = torch.autograd.grad(score, [xg], allow_unused=True)      # runs the vision tower's backward, nothing else
        if torch.is_tensor(self.text_features) and self.text_features.requires_grad:
            self.text_features = self.text_features.detach()        # the last reference into this call's graph
        return dx, logits.detach(), target

    def _maps_logits(self, video):
        """The inference head (gava_similarity_head) on this rank's clip features; text features from the cache when it is
        valid, else from the text tower on the current stream.  Leaves text_features, the cache and `last` alone."""
        if self.use_text_prompt_learning:
            key = self._text_cache_key()
            hit = key is not None and self._text_cache is not None and self._text_cache[0] == key
            text = self._text_cache[1] if hit else self.encode_text()
            n_kv = self.prompt_learner.n_kv
        else:
            text, n_kv = self.text_features.detach().to(device=video.device, dtype=torch.float32).contiguous(), 1
        return self._similarity_head(video, text, text.shape[0] // n_kv, n_kv)[0]

    # ---- input gradients --------------------------------------------------------------------------
    _SALIENCY_MODES = {None: hip.UNPATCH_GRAD, "absmax": hip.UNPATCH_ABSMAX, "l2": hip.UNPATCH_L2, "grad_x_input": hip.UNPATCH_GRAD_X_INPUT}

    def saliency(self, x, target=None, reduce="absmax"):
        """Which pixels and frames of the clips moved a class score: the gradient of sum_b logits[b, target_b] (the raw
        logits) with respect to x, through the HIP backward of the frozen vision tower.
        -> (maps, logits [B, C], target int64 [B]); maps is fp32 [B, T, S, S], per pixel over the three channels
             reduce="absmax"        max_c |g_c|
             reduce="l2"            sqrt(sum_c g_c^2)
             reduce="grad_x_input"  sum_c g_c x_c
        or, with reduce=None, the gradient itself, fp32 [B, 3, T, S, S] - the bits x.grad gets from forward(x) followed by
        the same backward.  The map modes fold the patch gradients straight into the map (gava_unpatchify): the full-size
        gradient is never in memory.
        x: a device clip batch [B, 3, T, S, S] as forward() takes it; it need not require grad (decoded uint8 videos:
        preprocess with `preprocessor.batch(videos)` first).  target: None - the top-1 class of this very forward, picked on the
        device -, an int (checked against the number of classes on the host), or an int64 [B] device tensor, which is NOT
        range-checked (a check would wait for the device; an index outside [0, C) is a device-side fault).
        Works on a model in eval() or train() mode, whatever is trainable; no parameter's .grad is touched, no graph and no
        kept activation survives the call, and the call itself never waits for the device.  memory / video_nte / desc_wise
        have no part in it; a ragged (use_descriptor) head is refused.  With an initialised process group every rank works
        on its own clips, as every grad-enabled forward does."""
        what = "saliency"
        if reduce not in self._SALIENCY_MODES:
            raise hip.GavaError(f"{what}: reduce must be one of 'absmax', 'l2', 'grad_x_input' or None, got {reduce!r}")
        B, _ = self._check_clips(what, x)
        self._check_single_logit(what)
        self._check_target(what, target, B)
        self._check_device(x, target)
        mode = self._SALIENCY_MODES[reduce]
        with torch.cuda.device(x.device):
            xg = x.detach().float().contiguous().requires_grad_()       # a leaf of this call's own: x is left alone
            request = dict(mode=mode, x=xg.detach() if mode == hip.UNPATCH_GRAD_X_INPUT else None)
            dx, logits, target = self._class_gradient(xg, request, target)
        return (dx if mode == hip.UNPATCH_GRAD else request.pop("out")), logits, target

    _IG_MODES = {(True, "sum"): hip.PATH_ATTR_SUM, (True, "abs"): hip.PATH_ATTR_ABS, (True, None): hip.PATH_ATTR,
                 (False, None): hip.PATH_GRAD, (False, "absmax"): hip.PATH_ABSMAX, (False, "l2"): hip.PATH_L2}
    _SMOOTH_MODES = {None: hip.PATH_GRAD, "absmax": hip.PATH_ABSMAX, "l2": hip.PATH_L2}

    def _path_checks(self, what, x, target, m, max_clips, noise=False):
        """The refusals integrated_gradients and smooth_grad share, from the clip batch to max_clips -> (B, T, clips per chunk)."""
        B, T = self._check_clips(what, x)
        S = self._shape["size"]
        if m * T > hip.MAX_GRID_FRAMES:
            raise hip.GavaError(f"{what}: one clip's {m} copies x {T} frames are past the {hip.MAX_GRID_FRAMES} frames one launch covers")
        if noise and S % 2:
            raise hip.GavaError(f"{what}: noise is drawn four floats at a time, an odd size {S} is not supported")
        self._check_single_logit(what)
        self._check_target(what, target, B)
        if isinstance(max_clips, bool) or not isinstance(max_clips, int) or max_clips < 1:
            raise hip.GavaError(f"{what}: max_clips must be an int >= 1, got {max_clips!r}")
        return B, T, max(1, min(max_clips, hip.MAX_GRID_FRAMES // T) // m)

    def _path_maps(self, x, make_copies, mode, w, target, ref_step, step, base=None, signed=None):
        """The body integrated_gradients and smooth_grad share: `step` clips at a time, make_copies(i, nb) -> the m = len(w)
        copies of clips [i, i + nb), fp32 [nb, m, 3, T, S, S]; the grad-enabled forward of the nb * m clips; the vision tower's
        backward with the path request, whose fold (gava_unpatchify_path) reduces each clip's m gradients with the weights w
        straight into the chunk's slice of the result.  target: int64 [B] or None - then the top-1 class of each clip's copy
        ref_step, picked on the device.  base: the baseline of the ATTR modes (None, [3] or shaped like x); signed: an fp32
        [B, T, S, S] tensor that also receives the PATH_ATTR_SUM map (a second fold of the same patch gradients).
        -> (maps, logits fp32 [B * m, C], target int64 [B])."""
        B, _, T, S, _ = x.shape
        m = len(w)
        attr = mode >= hip.PATH_ATTR
        shape = (B, 3, T, S, S) if mode in (hip.PATH_GRAD, hip.PATH_ATTR) else (B, T, S, S)
        maps = torch.empty(shape, dtype=torch.float32, device=x.device)
        aligned = lambda t: t if t.data_ptr() % 16 == 0 else t.clone()        # (a slice of clips of an odd size)
        logits, targets = _Rows(B * m), []
        for i in range(0, B, step):
            nb = min(step, B - i)
            dst = [maps[i:i + nb]] + ([signed[i:i + nb]] if signed is not None else [])
            out = [d if d.data_ptr() % 16 == 0 else torch.empty_like(d) for d in dst]
            b = self._base_rows(base, i, nb)
            request = dict(mode=mode, m=m, w=w, out=out[0], signed=out[1] if signed is not None else None,
                           x=aligned(x[i:i + nb]) if attr else None,
                           baseline=(aligned(b) if b is not None and b.dim() == 5 else b) if attr else None)
            with torch.enable_grad():
                xg = make_copies(i, nb).view(nb * m, 3, T, S, S).requires_grad_()       # a leaf of this call's own
                lg, tg = self._class_gradient(xg, request, target[i:i + nb] if target is not None else None, m, ref_step)[1:]
            for d, o in zip(dst, out):
                if o is not d:
                    d.copy_(o)
            request.clear()
            logits.put(i * m, lg)
            targets.append(tg)
            del xg, lg          # nothing of this chunk is held while the next one runs
        return maps, logits.out, (target if target is not None else targets[0] if len(targets) == 1 else torch.cat(targets, 0))

    def integrated_gradients(self, x, target=None, baseline="zero", steps=16, rule="trapezoid", reduce="sum", multiply=True,
                             blur_sigma=5.0, max_clips=64):
        """Integrated gradients (Sundararajan et al., "Axiomatic Attribution for Deep Networks") of a class's raw logit along
        the straight path from a baseline x0 to the clip -> PathAttribution (see there for the fields):
          a = (x - x0) * sum_k w_k  d logit_target / d x (x0 + alpha_k (x - x0))
        The one map here with a checkable axiom: a clip's attributions sum to f(x) - f(x0) up to the quadrature's error, and
        .delta is that residual (what Captum calls the convergence delta).
          reduce="sum"  [B, T, S, S]  a_0 + a_1 + a_2, signed: what speaks FOR the class is positive
          reduce="abs"  [B, T, S, S]  |a_0| + |a_1| + |a_2|
          reduce=None   [B, 3, T, S, S]  a itself
        multiply=False returns the path-mean gradient G = sum_k w_k grad_k instead; reduce is then None ([B, 3, T, S, S]),
        "absmax" or "l2" (saliency's map rules on G), and sum_attr / delta are None.
        baseline: as for perturbation_curves - "zero", "blur" (blur_sigma), an fp32 tensor [3] or one shaped like x.
        rule="trapezoid": m = steps >= 2 points alpha_k = k / (m - 1), end weights halved; x0 and x are steps 0 and m - 1, so
        f(x0) and f(x) come with the path.  rule="gausslegendre": the `steps` Gauss-Legendre nodes on [0, 1] - exact for
        polynomials of degree 2 steps - 1, where the trapezoid's error falls as 1 / m^2 - plus the two endpoints as zero-weight
        steps (m = steps + 2): their forwards and backwards add nothing to the map and are the price of the residual.
        target: None - the top-1 class of the clip itself, the alpha = 1 row of the same forward, picked on the device -, an
        int (checked on the host) or an int64 [B] device tensor (not range-checked; out of range: NaN sum_attr and delta).
        The m copies of a clip are written by one kernel (gava_path_clips), go through the grad-enabled forward and the
        vision tower's backward as a batch, and the fold reduces their m patch gradients into the clip's one map
        (gava_unpatchify_path): the m full-size gradients are never in memory.  max(1, max_clips // m) whole clips run at a
        time; a chunk's copies (4.8 MB each at 224 px and T = 8) and kept activations are in memory at once.
        Works in eval() and train() mode and under no_grad (the call enables grad for itself); no parameter's .grad is
        touched, nothing survives the call, nothing waits for the device.  A per-descriptor head is refused."""
        what = "integrated_gradients"
        if (bool(multiply), reduce) not in self._IG_MODES:
            raise hip.GavaError(f"{what}: reduce must be 'sum', 'abs' or None (multiply=False: None, 'absmax' or 'l2'), got {reduce!r}")
        mode = self._IG_MODES[(bool(multiply), reduce)]
        alpha, w = hip.path_rule(rule, steps)
        m = len(alpha)
        B, T, step = self._path_checks(what, x, target, m, max_clips)
        kind = self._check_baseline(what, baseline, x)
        taps = hip.gaussian_taps(blur_sigma) if kind == "blur" else None
        self._check_device(x, target)
        dev, P = x.device, self._shape["P"]
        with torch.cuda.device(dev):
            x = x.detach().float().contiguous()
            base = self._make_baseline(kind, baseline, x, taps)
            target = self._as_target(target, B, dev)
            copies = lambda i, nb: hip.path_clips(x[i:i + nb], patch=P, alpha=alpha, baseline=self._base_rows(base, i, nb))
            signed = None
            if multiply and reduce != "sum":
                signed = torch.empty(B, T, x.shape[3], x.shape[4], dtype=torch.float32, device=dev)
            maps, logits, target = self._path_maps(x, copies, mode, w, target, m - 1, step, base=base, signed=signed)
            sum_attr = delta = None
            if multiply:
                d = hip.path_delta(maps if signed is None else signed, logits, target.contiguous(), m=m, k_lo=0, k_hi=m - 1)
                sum_attr, delta = d["sum_attr"], d["delta"]
            logits = logits.view(B, m, -1)[:, m - 1].contiguous()
        return PathAttribution(maps, logits, target, sum_attr, delta, torch.tensor(alpha, dtype=torch.float32), torch.tensor(w, dtype=torch.float32))

    def smooth_grad(self, x, target=None, samples=16, sigma=0.15, relative=True, seed=0, reduce="absmax", max_clips=64):
        """SmoothGrad (Smilkov et al., "SmoothGrad: removing noise by adding noise"): the mean over `samples` noisy copies
        x + sigma_b z, z ~ N(0, 1), of the gradient saliency() takes -> (maps, logits [B, C] of x itself, target int64 [B]),
        like saliency; maps is fp32 [B, T, S, S] (reduce="absmax" / "l2", saliency's map rules on the MEAN gradient) or the mean
        gradient itself, [B, 3, T, S, S] (reduce=None).
        sigma: with relative=True the noise level as a share of each clip's own max - min (gava_clip_range; the paper's 10-20 %),
        else absolute, in the normalised space clips live in.  The noise is counter-based (Philox4x32-10 keyed by `seed`,
        counted by clip, sample and element - gava_path_clips): a call repeats bit for bit, and neither the batch a clip
        arrives in nor max_clips changes its noise.  A clip that holds a NaN gets a NaN map.
        target: None - the top-1 class of x itself - an int or an int64 [B] device tensor, as for saliency.  The plain no-grad
        forward of x that gives `logits` (and that target) runs in every case, max_clips clips at a time (it keeps no
        activations).  Chunks, memory and the guarantees are
        integrated_gradients': max(1, max_clips // samples) clips at a time, the fold (gava_unpatchify_path) averages the
        copies' patch gradients on the way, no .grad is touched, nothing waits for the device."""
        what = "smooth_grad"
        if reduce not in self._SMOOTH_MODES:
            raise hip.GavaError(f"{what}: reduce must be 'absmax', 'l2' or None, got {reduce!r}")
        if isinstance(samples, bool) or not isinstance(samples, int) or not 1 <= samples <= hip.PATH_MAX_STEPS:
            raise hip.GavaError(f"{what}: samples must be an int in [1, {hip.PATH_MAX_STEPS}], got {samples!r}")
        if isinstance(sigma, bool) or not isinstance(sigma, (int, float)) or not (math.isfinite(sigma) and sigma >= 0):
            raise hip.GavaError(f"{what}: sigma must be a finite number >= 0, got {sigma!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
            raise hip.GavaError(f"{what}: seed must be an int in [0, 2^64), got {seed!r}")
        m = samples
        B, T, step = self._path_checks(what, x, target, m, max_clips, noise=True)
        self._check_device(x, target)
        dev, P = x.device, self._shape["P"]
        with torch.cuda.device(dev):
            x = x.detach().float().contiguous()
            plain = min(max_clips, hip.MAX_GRID_FRAMES // T)        # the plain forward keeps nothing: max_clips clips at a time
            rows = _Rows(B)
            with torch.no_grad():
                for i in range(0, B, plain):
                    rows.put(i, self.local_logits(self._forward_impl(x[i:i + plain], None, None, False)[0]))
                self.last["local_batch"] = B
            logits = rows.out
            target = logits.argmax(dim=1) if target is None else self._as_target(target, B, dev)
            sg = hip.clip_range(x, float(sigma))[2] if relative else torch.full((B,), float(sigma), dtype=torch.float32, device=dev)
            copies = lambda i, nb: hip.path_clips(x[i:i + nb], patch=P, sigma=sg[i:i + nb], samples=m, seed=seed, clip0=i)
            maps, _, _ = self._path_maps(x, copies, self._SMOOTH_MODES[reduce], [1.0 / m] * m, target, 0, step)
        return maps, logits, target

    # ---- attention --------------------------------------------------------------------------------
    def attention_maps(self, x, mode="rollout", layer=-1, heads="mean", max_clips=None):
        """What the CLS token of every frame attends to -> AttentionMaps (see there for the fields).
          mode="rollout"  attention rollout of the CLS token through all blocks: row 0 of A^_L ... A^_1, A^_l = (I + mean_h
                          A_l,h) / 2, A_l,h = block l's probabilities restricted to the frame's own tokens (CLS + patches) and
                          renormalised per row - the prompt tokens are rebuilt in every block and carry no path between
                          blocks.  Run as a vector chain from the last block to the first (gava_attention_mass, one launch
                          per block; no matrix product).  patches + cls sum to 1 per frame.  `layer` is ignored, `heads`
                          must be "mean".
          mode="cls"      the CLS row of block `layer` (negative: from the end) over ALL its keys, split by key group:
                          patches, cls, global_prompts, local_prompts, summary; heads="mean" averages over the heads,
                          heads=None keeps them as an axis after T.
        x: a device clip batch [B, 3, T, S, S] as forward() takes it (decoded uint8 videos: `preprocessor.batch(videos)`
        first).  T need not be num_frames: the blocks regroup the B*T frames by the model's num_frames, and so do the local
        prompts' columns.
        The clips run through the activation-keeping forward of the training path (encode_video(kept=...)) under no_grad,
        in chunks of whole num_frames groups whose kept activations (training.kept_bytes) fit keep_activation_bytes;
        max_clips sets the clips per chunk instead.  The buffers are reused from chunk to chunk.  `logits` come from the
        inference head on THIS forward's features: the kept forward packs its operands plainly (no weight-lo pass, no
        16-bit residual pair), so they can differ from forward()'s within the operand rounding.
        Works in eval() and train() mode; no .grad is touched, no graph is left, nothing waits for the device.  With an
        initialised process group every rank keeps its own clips.  A per-descriptor (use_descriptor) head is refused."""
        what = "attention_maps"
        if mode not in ("rollout", "cls"):
            raise hip.GavaError(f"{what}: mode must be 'rollout' or 'cls', got {mode!r}")
        if heads not in ("mean", None):
            raise hip.GavaError(f"{what}: heads must be 'mean' or None, got {heads!r}")
        if mode == "rollout" and heads is None:
            raise hip.GavaError(f"{what}: rollout averages over the heads in every block (heads='mean'); per-head maps are mode='cls'")
        sh, Tm = self._shape, self.num_frames
        NL, D, H, G = sh["layers"], sh["D"], sh["H"], sh["G"]
        if mode == "cls":
            if not (isinstance(layer, int) and -NL <= layer < NL):
                raise hip.GavaError(f"{what}: layer {layer!r} is outside the {NL} blocks")
            layer = layer % NL
        else:
            layer = None
        B, T, unit = self._check_clips(what, x, groups=True)
        g = sh["size"] // sh["P"]
        n1 = g * g + 1
        n_all = n1 + G + Tm + 1
        if n_all > hip.ATTENTION_MASS_MAX_KEYS:
            raise hip.GavaError(f"{what}: {n_all} keys per frame, gava_attention_mass takes at most {hip.ATTENTION_MASS_MAX_KEYS}")
        self._check_single_logit(what)
        step = self._group_step(B, T, unit, max_clips)
        self._check_device(x)
        dev = x.device
        mass = dict(heads=H, n_kmain=n1, prec=self.prec, n_g=G, T=Tm, has_summary=True)
        with torch.cuda.device(dev), torch.no_grad():
            self._attach_encoders()
            self._pack()
            kept = training.alloc_kept(self, step, T, dev)
            video = torch.empty(B, sh["E"], dtype=torch.float32, device=dev)
            maps = torch.empty((B * T, n1) if mode == "rollout" else (B * T, H, n_all), dtype=torch.float32, device=dev)
            for i in range(0, B, step):
                nb = min(step, B - i)
                kb = kept
                if nb != step:          # the last, smaller chunk: the same memory under that chunk's shapes
                    shapes = {k: v.shape for k, v in training.alloc_kept(self, nb, T, "meta").items()}
                    kb = {k: kept[k].view(-1)[:math.prod(shp)].view(shp) for k, shp in shapes.items()}
                video[i:i + nb] = self.encode_video(x[i:i + nb], kept=kb)[0]
                BT = nb * T
                keys = lambda l: dict(k=kb["qkv"][l][:, D:2 * D], side_k=kb["sidekv"][l][:, :D])
                out = maps[i * T:(i + nb) * T]
                if mode == "cls":
                    if layer == NL - 1:     # the kept last block has its CLS queries only, in a buffer of their own
                        hip.attention_mass(kb["last_q"], out=out, batch=BT, n_q=1, q_batch_rows=1, **keys(layer), **mass)
                    else:
                        hip.attention_mass(kb["qkv"][layer][:, :D], out=out, batch=BT, n_q=1, q_batch_rows=n1, **keys(layer), **mass)
                    continue
                r = hip.attention_mass(kb["last_q"], batch=BT, n_q=1, q_batch_rows=1, renorm=True, **keys(NL - 1), **mass).mean(1).mul_(0.5)
                r[:, 0] += 0.5              # r = e_cls / 2 + mean_h A_L[0] / 2
                for l in range(NL - 2, -1, -1):
                    o = hip.attention_mass(kb["qkv"][l][:, :D], batch=BT, n_q=n1, w=r, renorm=True, **keys(l), **mass)
                    r = (0.5 * r).add_(o.mean(1), alpha=0.5)
                out.copy_(r)
            logits = self._maps_logits(video)
        if mode == "rollout":
            m = maps.view(B, T, n1)
            return AttentionMaps(mode, None, m[..., 1:].reshape(B, T, g, g), m[..., 0], logits)
        m = (maps.mean(1) if heads == "mean" else maps).view(B, T, *(() if heads == "mean" else (H,)), n_all)
        return AttentionMaps(mode, layer, m[..., 1:n1].reshape(*m.shape[:-1], g, g), m[..., 0], logits,
                             global_prompts=m[..., n1:n1 + G], local_prompts=m[..., n1 + G:n1 + G + Tm], summary=m[..., n_all - 1])

    def relevance_maps(self, x, target=None, max_clips=None):
        """Which patches and frames of the clips speak FOR a class -> RelevanceMaps (patches [B, T, g, g], cls [B, T], logits
        [B, C], target [B]): gradient-weighted attention relevance (Chefer et al., "Generic Attention-model Explainability",
        the self-attention rule).  It is the class-specific counterpart of attention_maps(mode="rollout"), with every block's
        attention matrix replaced by  A-_l = mean_h max(0, grad A_l,h * A_l,h):
          A_l,h   block l's probabilities over ALL its keys, as the forward used them (not renormalised, unlike the rollout),
          grad    d s / d A_l,h for s = sum_b logits[b, target_b], the raw logits, as saliency() differentiates them,
        both restricted to the frame's own tokens (CLS + patches).  The relevance of the CLS token is row 0 of
        (I + A-_L) ... (I + A-_1), run as the vector chain r <- e_cls, r <- r + r A-_l from the last block to the first
        inside the HIP backward of the vision tower (gava_attention_relevance, one launch per block, on the d mix the backward
        forms anyway; neither the probabilities nor their gradients are ever in memory).
        The result is NOT normalised: its scale is the gradient's (patches >= 0, cls >= 1, no fixed sum); compare maps of one
        call, or normalise them yourself.  The prompt tokens are rebuilt in every block and carry no token identity between
        blocks - the restriction the rollout documents -, so relevance that flows through the local-prompt / summary path
        from frame to frame is NOT attributed; the gradient itself is the true one, prompt path included.
        x: a device clip batch [B, 3, T, S, S] as forward() takes it (decoded uint8 videos: `preprocessor.batch(videos)`
        first).  T need not be num_frames; the B*T frames must be whole num_frames groups, as for attention_maps.  target: as
        for saliency - None (the top-1 class of this very forward, picked on the device), an int (checked on the host) or an
        int64 [B] device tensor (not range-checked).  The clips run in chunks of whole groups whose kept activations
        (training.kept_bytes) fit keep_activation_bytes - a chunk that still does not fit recomputes its blocks, in bf16 -;
        max_clips sets the clips per chunk instead.  Chunking does not change a bit of the result.
        Works in eval() and train() mode, whatever is trainable; no .grad is touched, no graph and no kept activation survives
        the call, nothing waits for the device.  A per-descriptor (use_descriptor) head is refused, and so is a shape with more
        keys per frame than gava_attention_relevance takes."""
        what = "relevance_maps"
        sh = self._shape
        B, T, unit = self._check_clips(what, x, groups=True)
        g = sh["size"] // sh["P"]
        n1 = g * g + 1
        n_all = n1 + sh["G"] + self.num_frames + 1
        if n_all > hip.ATTENTION_RELEVANCE_MAX_KEYS:
            raise hip.GavaError(f"{what}: {n_all} keys per frame, gava_attention_relevance takes at most {hip.ATTENTION_RELEVANCE_MAX_KEYS}")
        self._check_single_logit(what)
        self._check_target(what, target, B)
        step = self._group_step(B, T, unit, max_clips)
        self._check_device(x, target)
        rs, logits, targets = [], [], []
        for i in range(0, B, step):
            tg = target[i:i + step] if torch.is_tensor(target) else target
            r, lg, tg = self._relevance_chunk(x[i:i + step], tg, {})
            rs.append(r), logits.append(lg), targets.append(tg)
        m = (rs[0] if len(rs) == 1 else torch.cat(rs, 0)).view(B, T, n1)
        cat = lambda ts: ts[0] if len(ts) == 1 else torch.cat(ts, 0)
        return RelevanceMaps(m[..., 1:].reshape(B, T, g, g), m[..., 0], cat(logits), target if torch.is_tensor(target) else cat(targets))

    def _relevance_chunk(self, x, target, state):
        """One chunk of relevance_maps: the grad-enabled forward of whole groups and the vision tower's backward with the
        relevance request.  state: the request's state ({}; tests pass dict(capture=[]), see training._relevance_step).
        -> (r fp32 [B*T, n1], logits [B, C], target int64 [B])."""
        with torch.cuda.device(x.device):
            xg = x.detach().float().contiguous().requires_grad_()       # a leaf of this call's own: it makes the tower differentiable
            request = dict(relevance=state)
            _, logits, target = self._class_gradient(xg, request, target)
        state.pop("r", None)
        return request.pop("out"), logits, target

    # ---- faithfulness -----------------------------------------------------------------------------
    def perturbation_curves(self, x, scores, mode="deletion", target=None, steps=10, fractions=None, scope="clip",
                            baseline="zero", blur_sigma=5.0, max_clips=None):
        """How faithful an importance map is to the model: the deletion or insertion curve of every clip (Petsiuk et al.,
        "RISE"; the test Chefer et al. report for relevance) -> PerturbationCurves (see there for the fields).
          mode="deletion"   the most important units are replaced by the baseline first: the target's score should FALL fast
          mode="insertion"  start from the baseline and put the most important units back first: it should RISE fast
        x: fp32 device clips [B, 3, T, S, S], as for saliency.  scores: what to rank by, fp32 on x's device -
        [B, T, g, g] (patches, g = S / P: attention_maps(x).patches, relevance_maps(x).patches), [B, T, S, S] (pixels, summed
        over each patch: saliency(x)[0]) or [B, T] (frames: the maps' .cls, or any per-frame score).  scope="clip" ranks all
        units of a clip together, scope="frame" the patches of every frame among themselves (every frame then loses the same
        number of patches per step; refused for frame scores).  The order is exact: descending, ties to the lower index,
        NaNs last (gava_patch_ranks).
        fractions: the share of a ranking's n units perturbed at each step - by default linspace(0, 1, steps + 1), else a
        strictly increasing list from 0 to 1; step s perturbs the k_s = floor(f_s n + 0.5) first units of the ranking.
        baseline: "zero" (the dataset's mean colour, in the normalised space clips live in), "blur" (the clip itself under a
        Gaussian of blur_sigma pixels, radius ceil(3 sigma), border replicated), an fp32 tensor [3] (one value per channel) or
        one shaped like x.  target: as for saliency - None (each clip's top-1 class on its UNPERTURBED step, picked on the
        device), an int (checked on the host) or an int64 [B] device tensor (out of range: that clip's curves are NaN).
        Evaluation only: call it under torch.no_grad() on a model in eval() mode.  The S1 = len(fractions) perturbed copies
        of a clip are written by one kernel (gava_perturb_clips) and go through the plain forward, max(1, max_clips // S1)
        whole clips at a time; max_clips defaults to the most clips one launch's grid covers (65535 frames).  A chunk's
        nb * S1 perturbed clips are in memory at once (4.8 MB each at 224 px and T = 8) next to the forward's workspace: lower
        max_clips for big batches.  Chunking changes no bit.  The text features are cached for the duration of the call (cache_text_features is restored afterwards).  The
        call ends with one gava_perturb_scores launch over all clips and never waits for the device.
        Several ranks: every rank passes its own clips and gets the curves of its own clips (the forward gathers the
        perturbed clips' features of all ranks, local_logits() takes this rank's rows back out); every rank must therefore
        pass the same B, the same number of fractions and the same max_clips."""
        what = "perturbation_curves"
        if torch.is_grad_enabled() or self.training:
            raise hip.GavaError(f"{what} is an evaluation path: call it under torch.no_grad() on a model in eval() mode")
        if mode not in ("deletion", "insertion"):
            raise hip.GavaError(f"{what}: mode must be 'deletion' or 'insertion', got {mode!r}")
        if scope not in ("clip", "frame"):
            raise hip.GavaError(f"{what}: scope must be 'clip' or 'frame', got {scope!r}")
        B, T = self._check_clips(what, x)
        S, P = self._shape["size"], self._shape["P"]
        g = S // P
        layouts = {(B, T, g, g): "patch", (B, T, S, S): "pixel", (B, T): "frame"}
        if not (torch.is_tensor(scores) and scores.is_floating_point() and tuple(scores.shape) in layouts):
            raise hip.GavaError(f"{what}: scores must be a floating-point [{B}, {T}, {g}, {g}] (patches), [{B}, {T}, {S}, {S}] (pixels) or "
                                f"[{B}, {T}] (frames) tensor, got {(scores.dtype, tuple(scores.shape)) if torch.is_tensor(scores) else type(scores)}")
        layout = layouts[tuple(scores.shape)]
        if layout == "frame" and scope == "frame":
            raise hip.GavaError(f"{what}: scope='frame' ranks the patches of a frame; frame scores have one unit per frame")
        n = T if layout == "frame" else T * g * g if scope == "clip" else g * g
        if n > hip.PERTURB_MAX_UNITS:
            raise hip.GavaError(f"{what}: {n} units per ranking, at most {hip.PERTURB_MAX_UNITS} are supported")
        fr, ks = hip.perturb_thresholds(n, steps, fractions)
        S1 = len(fr)
        fit = hip.MAX_GRID_FRAMES // T
        if fit < S1:
            raise hip.GavaError(f"{what}: one clip's {S1} steps x {T} frames are past the {hip.MAX_GRID_FRAMES} frames one launch covers")
        self._check_single_logit(what)
        self._check_target(what, target, B)
        step = max(1, (fit if max_clips is None else min(fit, int(max_clips))) // S1)
        kind = self._check_baseline(what, baseline, x)
        taps = hip.gaussian_taps(blur_sigma) if kind == "blur" else None
        self._check_device(x, scores, target)
        dev = x.device
        with self._text_features_cached(), torch.cuda.device(dev):
            x = x.detach().float().contiguous()
            ranks = hip.patch_ranks(scores.detach().to(dev).float().contiguous(), patch=P if layout == "pixel" else None, scope=scope)
            base = self._make_baseline(kind, baseline, x, taps)
            target = self._as_target(target, B, dev)
            logits = _Rows(B * S1)
            for i in range(0, B, step):
                nb = min(step, B - i)
                xp = hip.perturb_clips(x[i:i + nb], ranks[i:i + nb], ks, patch=P, mode=mode, baseline=self._base_rows(base, i, nb))
                logits.put(i * S1, self.local_logits(self._forward_impl(xp.view(nb * S1, 3, T, S, S), None, None, False)[0]))
            self.last["local_batch"] = B
            res = hip.perturb_scores(logits.out, fr, ref_step=0 if mode == "deletion" else S1 - 1,
                                     target=target.contiguous() if target is not None else None)
        return PerturbationCurves(mode, torch.tensor(fr, dtype=torch.float32), res["logit"], res["prob"], res["top1"],
                                  res["auc_logit"], res["auc_prob"], res["target"], ranks)

    _FAITHFULNESS_METHODS = ("rollout", "relevance", "saliency", "integrated", "smoothgrad")

    def faithfulness(self, x, methods=("rollout", "relevance", "saliency"), target=None, seed=0, **kw):
        """Which map to believe for this model and these clips: both perturbation curves of every method's map, for one and
        the same target, next to a random ranking -> Faithfulness, {name: {"deletion": ..., "insertion": ...}}; print its
        .table().  methods: any of "rollout" (attention_maps(x).patches), "relevance" (relevance_maps(x, target).patches) and
        "saliency" (saliency(x, target)[0], pixels pooled to patches), and on request "integrated"
        (integrated_gradients(x, target).maps, the signed sum: what speaks FOR the class goes first, as with relevance) and
        "smoothgrad" (smooth_grad(x, target)[0]), both with their defaults; the control "random" ranks by uniform scores drawn from
        a device generator seeded with `seed`, so a call repeats bit for bit.  target: as for perturbation_curves; None is the
        top-1 class of the plain forward of x, picked on the device once and used for every method.  **kw goes to
        perturbation_curves (steps, fractions, scope, baseline, blur_sigma, max_clips; not mode).  Evaluation only, like
        perturbation_curves; the maps' own rules apply to x (whole num_frames groups).  Nothing waits for the device."""
        what = "faithfulness"
        if torch.is_grad_enabled() or self.training:
            raise hip.GavaError(f"{what} is an evaluation path: call it under torch.no_grad() on a model in eval() mode")
        methods = tuple(methods)
        if not methods or any(m not in self._FAITHFULNESS_METHODS for m in methods) or len(set(methods)) != len(methods):
            raise hip.GavaError(f"{what}: methods must be distinct names out of {self._FAITHFULNESS_METHODS}, got {methods!r}")
        if "mode" in kw:
            raise hip.GavaError(f"{what} runs both modes: mode is not an argument")
        B, T = self._check_clips(what, x)
        self._check_single_logit(what)
        self._check_target(what, target, B)
        self._check_device(x, target)
        g = self._shape["size"] // self._shape["P"]
        make = {"rollout": lambda: self.attention_maps(x).patches, "relevance": lambda: self.relevance_maps(x, target).patches,
                "saliency": lambda: self.saliency(x, target)[0], "integrated": lambda: self.integrated_gradients(x, target).maps,
                "smoothgrad": lambda: self.smooth_grad(x, target)[0]}
        with torch.cuda.device(x.device):
            if target is None:
                target = self.local_logits(self._forward_impl(x, None, None, False)[0]).argmax(dim=1)
            target = self._as_target(target, B, x.device)
            maps = {m: make[m]() for m in methods}
            gen = torch.Generator(device=x.device)
            gen.manual_seed(int(seed))
            maps["random"] = torch.rand(B, T, g, g, generator=gen, dtype=torch.float32, device=x.device)
            out = Faithfulness()
            for name, s in maps.items():
                out[name] = {md: self.perturbation_curves(x, s.detach().contiguous(), mode=md, target=target, **kw) for md in ("deletion", "insertion")}
        return out
