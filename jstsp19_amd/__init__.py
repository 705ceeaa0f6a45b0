"""jstsp19_amd — MI355X (gfx950) implementation of the sparse wideband-mmWave channel
estimation solver path of vlaxose/jstsp19, behind the reference's own function signatures.

The compute lives in ``csrc/libjstsp_mi355x.so`` (hand-written HIP, C ABI in
``include/jstsp.h``); this package is the host-side mirror of the reference interface.
There is no CPU fallback: without the built library / without a GPU the calls raise.
"""
from ._lib import Context, JstspError, default_context, load, LIB_PATH, HOST, DEVICE  # noqa: F401
from .solvers import (OMP, sparse_sca_estim, cawgn_estim_out, gradient_head, ls_estimate, colmajor, correlate, empty_colmajor, mc_admm, mc_svt, nmse_spectral, lambda_max_sequence,  # noqa: F401
                      omp_kron, pinv, mmv_omp, tssr, rate, proposed_algorithm, proposed_algorithm_begin, proposed_algorithm_angles, sparse_admm, svt, synthesize, vamp,
                      vamp_kron, beamformer, ase, singular_values, spectrum, cosamp, cosamp_kron,
                      proposed_algorithm_f64, proposed_algorithm_angles_f64, svt_f64, correlate_f64, synthesize_f64,
                      pinv_f64, ls_estimate_f64, mmv_omp_f64, mc_svt_f64, mc_admm_f64, tssr_f64,
                      OMP_f64, omp_kron_f64, sparse_admm_f64, proposed_algorithm_std_f64, proposed_algorithm_angles_std_f64,
                      svd_f64, lowrank_f64, svd_tall_f64, lowrank_tall_f64, nmse_spectral_f64, rate_f64,
                      admm_state_elems, proposed_algorithm_resume_f64, proposed_algorithm_std_resume_f64,
                      proposed_algorithm_resume, proposed_algorithm_angles_resume, support_order, support_order_f64,
                      support_order_wide, support_order_wide_f64, support_top_f64, proposed_algorithm_refresh_f64,
                      support_top, proposed_algorithm_refresh, proposed_algorithm_until_f64, proposed_algorithm_until, refit_f64)

__version__ = "0.1.0"
