"""gava_clip_amd — MI355X (gfx950) implementation of the GaVA-CLIP video-frame forward path.

``from gava_clip_amd import VitaCLIP`` is the drop-in for
``from VitaCLIP_model import VitaCLIP`` (/root/reference/training/train.py:30).
"""
from .config import VitaConfig, VIT_B16_T8, VIT_B16_T16, VIT_L14_T32, TINY, param_shapes  # noqa: F401


def __getattr__(name):  # lazy: importing the package must not need torch/HIP
    if name == "VitaCLIP":
        from .model import VitaCLIP
        return VitaCLIP
    if name == "RelevanceMaps":
        from .model import RelevanceMaps
        return RelevanceMaps
    if name in ("PerturbationCurves", "Faithfulness"):
        from . import model
        return getattr(model, name)
    if name == "TrainCriterion":
        from .training import TrainCriterion
        return TrainCriterion
    if name in ("ClipMixer", "SoftTargetCriterion"):
        from . import training
        return getattr(training, name)
    if name in ("RandAugment", "AugmentedClipPreprocessor"):
        from . import augment
        return getattr(augment, name)
    if name == "AuxCriterion":
        from .training import AuxCriterion
        return AuxCriterion
    if name == "FusedAdamW":
        from .optim import FusedAdamW
        return FusedAdamW
    raise AttributeError(name)
