from .fused_l2nn import fused_l2nn, fused_l2nn_argmin
from .brute_force import BruteForceIndex, brute_force_build, knn
from .epsilon_neighborhood import eps_neighbors_l2sq, eps_neighbors_l2sq_csr
from .masked_nn import masked_l2nn, cross_component_nn
from .ivf_flat import (IvfFlatParams, IvfFlatIndex, ivf_flat_build, ivf_flat_extend,
                       ivf_flat_search, ivf_flat_save, ivf_flat_load)

__all__ = ["fused_l2nn", "fused_l2nn_argmin", "knn", "BruteForceIndex",
           "brute_force_build", "eps_neighbors_l2sq", "eps_neighbors_l2sq_csr",
           "masked_l2nn", "cross_component_nn", "IvfFlatParams", "IvfFlatIndex",
           "ivf_flat_build", "ivf_flat_extend", "ivf_flat_search", "ivf_flat_save",
           "ivf_flat_load"]
