"""MI355X-native AO-ADMM engine for coupled matrix factorization / PARAFAC2 with the API of MatCoupLy.

`matcouply_amd.decomposition.cmf_aoadmm` / `parafac2_aoadmm` and the `matcouply_amd.penalties` class tree mirror
`matcouply.decomposition` / `matcouply.penalties` (MarieRoald/matcouply v0.1.6); the per-mode ADMM updates run in
hand-written HIP kernels (libmatcouply_hip.so, C ABI in include/matcouply_hip.h).  There is no CPU fallback.
"""
__version__ = "0.1.0"

from . import coupled_matrices, data, decomposition, evaluation, missing, multistart, penalties, projection, random, resampling, similarity  # noqa: F401,E402
from .decomposition import PackedMatrices, best_start, cmf_aoadmm_grid, parafac2_aoadmm_grid  # noqa: F401,E402
from .similarity import factor_match_score, multistart_similarity, permute_cmf  # noqa: F401,E402
from .evaluation import (ModelEvaluation, core_consistency, fit, multistart_evaluation, relative_sse,  # noqa: F401,E402
                         slabwise_sse)
from .projection import Projection, parafac2_project  # noqa: F401,E402
from .resampling import (cmf_aoadmm_resample, cmf_resample_summary, parafac2_als_resample,  # noqa: F401,E402
                         parafac2_aoadmm_heldout_sse, parafac2_aoadmm_resample, resample_heldout_sse, resample_summary,
                         resampling_weights)
from .missing import (cmf_aoadmm_missing, entry_kfold, heldout_entry_sse, impute,  # noqa: F401,E402
                      parafac2_aoadmm_missing)
