"""mauv — MI355X-native Monte-Carlo Bayesian tri-modal encoder (Multimodal-AUV hot path).

Host side of the drop-in: PyTorch-ROCm modules whose compute runs entirely in
libmauv_hip.so (hand-written gfx950 HIP kernels behind the C-ABI of include/mauv.h).
"""
from ._lib import lib, MauvError  # noqa: F401  (fails loudly if the HIP library is missing)
from .frozen import FrozenBatchNorm2d, freeze_batchnorm, unfreeze_batchnorm  # noqa: F401
from .attribution import input_gradients, modality_shares, fgsm  # noqa: F401
from .augment import TripletAugment, AugmentedLoader, dihedral, undo_dihedral  # noqa: F401

__version__ = "0.1.0"
