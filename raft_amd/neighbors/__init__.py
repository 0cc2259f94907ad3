from .fused_l2nn import fused_l2nn, fused_l2nn_argmin
from .brute_force import BruteForceIndex, brute_force_build, knn
from .epsilon_neighborhood import eps_neighbors_l2sq, eps_neighbors_l2sq_csr
from .masked_nn import masked_l2nn, cross_component_nn
from .ivf_flat import (IvfFlatParams, IvfFlatIndex, ivf_flat_build, ivf_flat_extend,
                       ivf_flat_search, ivf_flat_save, ivf_flat_load)
from .ivf_pq import (IvfPqParams, IvfPqIndex, ivf_pq_build, ivf_pq_extend, ivf_pq_search,
                     ivf_pq_save, ivf_pq_load)
from .refine import refine
from .cagra import (CagraParams, CagraIndex, cagra_build, cagra_optimize, cagra_search,
                    search_kernel_serves, optimize_kernel_serves)
from .nn_descent import nn_descent, nn_descent_kernel_serves

__all__ = ["fused_l2nn", "fused_l2nn_argmin", "knn", "BruteForceIndex",
           "brute_force_build", "eps_neighbors_l2sq", "eps_neighbors_l2sq_csr",
           "masked_l2nn", "cross_component_nn", "IvfFlatParams", "IvfFlatIndex",
           "ivf_flat_build", "ivf_flat_extend", "ivf_flat_search", "ivf_flat_save",
           "ivf_flat_load", "IvfPqParams", "IvfPqIndex", "ivf_pq_build", "ivf_pq_extend",
           "ivf_pq_search", "ivf_pq_save", "ivf_pq_load", "refine", "CagraParams", "CagraIndex",
           "cagra_build", "cagra_optimize", "cagra_search", "search_kernel_serves",
           "optimize_kernel_serves", "nn_descent", "nn_descent_kernel_serves"]
