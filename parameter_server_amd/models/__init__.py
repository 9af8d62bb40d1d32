"""Model families trained through the parameter server."""
from .ffm import FFMConfig, FFMTrainer
from .fm import FMConfig, FMTrainer
from .fwfm import FwFMConfig, FwFMTrainer
from .scorer import FFMScorer, FMScorer, FwFMScorer, ModelScorer
from .sparse_lr import SparseLRConfig, SparseLRTrainer
from .wide_deep import WideDeepConfig, WideDeepTrainer

__all__ = ["SparseLRConfig", "SparseLRTrainer", "WideDeepConfig", "WideDeepTrainer", "FMConfig",
           "FMTrainer", "FFMConfig", "FFMTrainer", "FwFMConfig", "FwFMTrainer", "ModelScorer",
           "FMScorer", "FFMScorer", "FwFMScorer"]
