"""
ctypes binding of libibo_hip.so (include/ibo_abi.h).

The library is the product's ONLY compute path: if it is missing this module
raises at import, and every compute call raises IBOError(IBO_ERR_NO_DEVICE)
when no MI355X is visible.  Nothing here falls back to NumPy.

Every symbol of the header is bound below and listed in EXPORTED (118 of them: tests/test_cpu_host.py holds the two lists to
the header and to the library), the ibo_qei_* entries of the parallel expected improvement and the ibo_ehvi_* entries of the
two-objective hypervolume improvement, the ibo_ggp_* entries of a GP observed with gradients, the ibo_mes_* entries of
max-value entropy search, the ibo_sgp_* entries of the sparse GP with its likelihood gradient and ibo_ggp_nlml_grad, the
gradient-observation model's likelihood with its gradient, among them.

The five ibo_iacq_* entries of include/ibo_abi_ensemble.h -- acquisitions integrated over an ensemble of handles -- are bound the same
way and listed in EXPORTED_ENSEMBLE (tests/test_marginal_reference.py holds that list to its header and to the library).
"""
import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("IBO_HIP_LIB", os.path.join(_HERE, "libibo_hip.so"))

OK, ERR_ARG, ERR_HIP, ERR_NOT_PD, ERR_STATE, ERR_NO_DEVICE, ERR_COMM = range(7)
K_SE_ARD, K_SE_ISO, K_MATERN3, K_MATERN5 = 0, 1, 2, 3
ACQ_EI, ACQ_PI, ACQ_UCB, ACQ_NONE = 0, 1, 2, 3
ERF_LIBM, ERF_NR = 0, 1
DIAG_UNIT_PLUS_NOISE, DIAG_KERNEL_PLUS_NOISE = 0, 1
CLAMP_NATIVE = 1e-8      # cpp/optimizeGP.cpp:150-153
CLAMP_PY = 10e-8         # ego/gaussianprocess/__init__.py:224
COMM_ID_BYTES = 128

_DP = POINTER(c_double)
OBJECTIVE = ctypes.CFUNCTYPE(c_double, c_int, _DP)


class IBOError(RuntimeError):
    def __init__(self, code, msg):
        RuntimeError.__init__(self, "libibo_hip error %d: %s" % (code, msg))
        self.code = code


class NotPositiveDefinite(IBOError, np.linalg.LinAlgError):
    """raised where the reference's numpy.linalg.cholesky raises LinAlgError"""


if not os.path.exists(LIB_PATH):
    raise ImportError(
        "ibo_amd: %s not found. Build it with `make -C ibo_amd/csrc` (or __graft_entry__.build()); "
        "there is no CPU fallback." % LIB_PATH)

lib = ctypes.CDLL(LIB_PATH)


def _sig(name, restype, *argtypes):
    f = getattr(lib, name)
    f.restype = restype
    f.argtypes = list(argtypes)
    return f


_sig("ibo_abi_version", c_int)
_sig("ibo_last_error", c_char_p)
_sig("ibo_device_count", c_int, POINTER(c_int))
_sig("ibo_device_name", c_int, c_int, c_char_p, c_size_t)
_sig("ibo_selftest_mfma", c_int, c_int, _DP)
_sig("ibo_gpu_time_ms", c_int, c_int, _DP)
_sig("ibo_set_option", c_int, c_char_p, c_int)
_sig("ibo_trim", c_int, c_int)
_sig("ibo_dev_alloc", c_int, c_int, c_size_t, POINTER(c_void_p))
_sig("ibo_dev_free", c_int, c_int, c_void_p)
_sig("ibo_memcpy_h2d", c_int, c_int, c_void_p, c_void_p, c_size_t)
_sig("ibo_memcpy_d2h", c_int, c_int, c_void_p, c_void_p, c_size_t)
_sig("ibo_device_synchronize", c_int, c_int)
_sig("ibo_dev_generation", c_int, c_int, c_void_p, POINTER(ctypes.c_uint64))
_sig("ibo_gp_create", c_int, c_int, POINTER(c_void_p))
_sig("ibo_gp_destroy", c_int, c_void_p)
_sig("ibo_gp_fit", c_int, c_void_p, c_int, c_int, c_int, _DP, _DP, _DP, c_int, c_double, c_double, POINTER(c_int))
_sig("ibo_gp_fit_with_matrix", c_int, c_void_p, c_int, c_int, c_int, _DP, _DP, _DP, c_int, c_double, c_double,
     _DP, POINTER(c_int))
_sig("ibo_gp_extend", c_int, c_void_p, c_int, _DP, _DP, POINTER(c_int))
_sig("ibo_gp_reserve", c_int, c_void_p, c_int)
_sig("ibo_gp_remove", c_int, c_void_p, c_int, POINTER(c_int), _DP, POINTER(c_int))
_sig("ibo_pref_begin", c_int, c_void_p)
_sig("ibo_pref_rinv_mul", c_int, c_void_p, _DP, _DP)
_sig("ibo_pref_newton_step", c_int, c_void_p, c_int, POINTER(c_int64), _DP, _DP, _DP, _DP, POINTER(c_int))
_sig("ibo_pref_finish", c_int, c_void_p, c_int, POINTER(c_int64), _DP, c_double, POINTER(c_int))
_sig("ibo_gp_set_y", c_int, c_void_p, _DP)
_sig("ibo_gp_set_kstar_sf2", c_int, c_void_p, c_double)
_sig("ibo_gp_set_prior", c_int, c_void_p, c_int, _DP, _DP, c_double, _DP, _DP)
_sig("ibo_gp_get_R", c_int, c_void_p, _DP)
_sig("ibo_gp_get_L", c_int, c_void_p, _DP)
_sig("ibo_gp_get_W", c_int, c_void_p, _DP)
_sig("ibo_gp_loo", c_int, c_void_p, _DP, _DP, _DP)
_sig("ibo_gp_info", c_int, c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int), _DP)
_sig("ibo_gp_last_fit_ms", c_int, c_void_p, POINTER(c_float))
_sig("ibo_cov_matrix", c_int, c_int, c_int, c_int, _DP, c_int, c_double, c_int, _DP, c_int, _DP, c_int, c_double, _DP)
_sig("ibo_spd_solve", c_int, c_int, c_int, _DP, c_int, _DP, _DP, POINTER(c_int))
_sig("ibo_spd_inverse", c_int, c_int, c_int, _DP, _DP, POINTER(c_int))
_sig("ibo_posterior_batch", c_int, c_void_p, c_int64, _DP, c_double, _DP, _DP)
_sig("ibo_acq_sweep", c_int, c_void_p, c_int64, c_void_p, c_int, c_double, c_int, c_double, c_double,
     c_int, _DP, c_double, c_int64, c_void_p, c_void_p, c_void_p, _DP, POINTER(c_int64))
_sig("ibo_acq_batch", c_int, c_void_p, c_int64, _DP, c_int, c_double, c_int, c_double, c_double, _DP, _DP, _DP)
_sig("ibo_acq_grad_batch", c_int, c_void_p, c_int64, _DP, c_int, c_double, c_int, c_double, c_double, _DP, _DP, _DP,
     _DP, _DP, _DP)
_sig("ibo_posterior_cov", c_int, c_void_p, c_int64, _DP, c_int, _DP, _DP)
_sig("ibo_posterior_sample", c_int, c_void_p, c_int64, _DP, c_int, c_double, c_int, _DP, _DP, _DP, POINTER(c_int))
_sig("ibo_acq_sweep_incremental", c_int, c_void_p, c_int64, c_void_p, c_int, c_double, c_int, c_double, c_double,
     c_int, _DP, c_double, c_int64, c_void_p, c_void_p, c_void_p, _DP, POINTER(c_int64))
_sig("ibo_last_sweep_kernel_ms", c_int, c_void_p, POINTER(c_float), POINTER(c_char_p))
_sig("ibo_sweep_state_info", c_int, c_void_p, POINTER(c_int64), POINTER(c_int64))
_sig("ibo_sweep_state_levels", c_int, c_void_p, POINTER(c_int), POINTER(c_int), POINTER(c_int64))
_sig("ibo_direct_max", c_int, c_void_p, c_int, _DP, _DP, c_int, c_double, c_int, c_double, c_int, c_int, c_int,
     c_int, _DP, _DP, POINTER(c_int64))
_CON = (c_void_p, c_int, POINTER(c_void_p), _DP, POINTER(c_int))       # obj, ncon, con, thresh, sense of the ibo_cacq_* entries
_sig("ibo_cacq_sweep", c_int, *(_CON + (c_int64, c_void_p, c_int, c_double, c_int, c_double, c_double, c_int, _DP, c_double, c_int64,
                                       c_void_p, c_void_p, c_void_p, _DP, POINTER(c_int64))))
_sig("ibo_cacq_batch", c_int, *(_CON + (c_int64, _DP, c_int, c_double, c_int, c_double, c_double, _DP, _DP, _DP)))
_sig("ibo_cacq_grad_batch", c_int, *(_CON + (c_int64, _DP, c_int, c_double, c_int, c_double, c_double, _DP, _DP)))
_sig("ibo_cacq_direct_max", c_int, *(_CON + (c_int, _DP, _DP, c_int, c_double, c_int, c_double, c_double, c_int, c_int, c_int, c_int,
                                            _DP, _DP, POINTER(c_int64))))
_EHVI = (POINTER(c_void_p), c_int, _DP, _DP)                               # obj[2], nfront, front_host, ref of the ibo_ehvi_* entries
_sig("ibo_ehvi_sweep", c_int, *(_EHVI + (c_int64, c_void_p, c_int, c_double, c_int, _DP, c_double, c_int64, c_void_p, _DP, POINTER(c_int64))))
_sig("ibo_ehvi_batch", c_int, *(_EHVI + (c_int64, _DP, c_int, c_double, _DP)))
_sig("ibo_ehvi_grad_batch", c_int, *(_EHVI + (c_int64, _DP, c_int, c_double, _DP, _DP)))
_sig("ibo_ehvi_direct_max", c_int, *(_EHVI + (c_int, _DP, _DP, c_int, c_double, c_int, c_int, c_int, c_int, _DP, _DP, POINTER(c_int64))))
_sig("ibo_ehvi_scan_ms", c_int, _DP, c_int)
_MES = (c_void_p, c_int, _DP, c_double)                                    # gp, K, ystar_host, s2_offset of the ibo_mes_* value entries
_sig("ibo_mes_sweep", c_int, *(_MES + (c_int64, c_void_p, c_double, c_int, _DP, c_double, c_int64, c_void_p, _DP, POINTER(c_int64))))
_sig("ibo_mes_batch", c_int, *(_MES + (c_int64, _DP, c_double, _DP)))
_sig("ibo_mes_grad_batch", c_int, *(_MES + (c_int64, _DP, c_double, _DP, _DP)))
_sig("ibo_mes_direct_max", c_int, *(_MES + (c_int, _DP, _DP, c_double, c_int, c_int, c_int, c_int, _DP, _DP, POINTER(c_int64))))
_sig("ibo_mes_maxcdf", c_int, c_void_p, c_int64, c_void_p, c_int, _DP, c_double, c_double, _DP, _DP)
_sig("ibo_mes_scan_ms", c_int, _DP, c_int)
_KG = (c_void_p, c_int, _DP)                                               # gp, nref, ref_host of the ibo_kg_* entries
_sig("ibo_kg_sweep", c_int, *(_KG + (c_int64, c_void_p, c_int, c_double, c_int64, c_void_p, _DP, POINTER(c_int64))))
_sig("ibo_kg_batch", c_int, *(_KG + (c_int64, _DP, c_int, c_double, _DP, _DP, _DP, _DP, _DP)))
_sig("ibo_kg_direct_max", c_int, *(_KG + (c_int, _DP, _DP, c_int, c_double, c_int, c_int, c_int, c_int, _DP, _DP, POINTER(c_int64))))
_sig("ibo_kg_stage_ms", c_int, _DP, c_int)
_QEI = (c_void_p, c_int, _DP, c_int, _DP, c_double, c_double, c_double, c_double)   # gp, npend, pend_host, nsamp, Z_host, ymax, xi, clamp_lo, jitter
_sig("ibo_qei_sweep", c_int, *(_QEI + (c_int64, c_void_p, c_int64, c_void_p, _DP, _DP, POINTER(c_int64), POINTER(c_int))))
_sig("ibo_qei_batch", c_int, *(_QEI + (c_int64, _DP, _DP, _DP, _DP, _DP, _DP, _DP, _DP, POINTER(c_int))))
_sig("ibo_qei_direct_max", c_int, *(_QEI + (c_int, _DP, _DP, c_int, c_int, c_int, c_int, _DP, _DP, POINTER(c_int64), POINTER(c_int))))
_sig("ibo_qei_stage_ms", c_int, _DP, c_int)
_PATHS = c_void_p                                                          # ibo_paths_t *
_sig("ibo_paths_create", c_int, c_void_p, c_int, _DP, _DP, c_int, _DP, _DP, POINTER(_PATHS))
_sig("ibo_paths_destroy", c_int, _PATHS)
_sig("ibo_paths_info", c_int, _PATHS, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int))
_sig("ibo_paths_coef", c_int, _PATHS, _DP)
_sig("ibo_paths_sweep", c_int, _PATHS, c_int64, c_void_p, c_int64, c_void_p, _DP, POINTER(c_int64))
_sig("ibo_paths_batch", c_int, _PATHS, c_int64, _DP, _DP)
_sig("ibo_paths_grad_batch", c_int, _PATHS, c_int64, _DP, POINTER(c_int), _DP, _DP)
_sig("ibo_paths_direct_max", c_int, _PATHS, c_int, c_int, _DP, _DP, c_int, c_int, c_int, c_int, _DP, _DP, POINTER(c_int64))
_GGP = c_void_p                                                            # ibo_ggp_t *
_sig("ibo_ggp_create", c_int, c_int, POINTER(_GGP))
_sig("ibo_ggp_destroy", c_int, _GGP)
_sig("ibo_ggp_info", c_int, _GGP, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int), _DP)
_sig("ibo_ggp_fit", c_int, _GGP, c_int, c_int, c_int, _DP, _DP, _DP, _DP, c_int, c_double, c_double, _DP, POINTER(c_int))
_sig("ibo_ggp_get_R", c_int, _GGP, _DP)
_sig("ibo_ggp_get_L", c_int, _GGP, _DP)
_sig("ibo_ggp_acq_batch", c_int, _GGP, c_int64, _DP, c_int, c_double, c_int, c_double, c_double, _DP, _DP, _DP)
_sig("ibo_ggp_acq_sweep", c_int, _GGP, c_int64, c_void_p, c_int, c_double, c_int, c_double, c_double, c_int64,
     c_void_p, c_void_p, c_void_p, _DP, POINTER(c_int64))
_sig("ibo_ggp_direct_max", c_int, _GGP, c_int, _DP, _DP, c_int, c_double, c_int, c_double, c_int, c_int, c_int, c_int,
     _DP, _DP, POINTER(c_int64))
_sig("ibo_ggp_stage_ms", c_int, _DP, c_int)
_sig("ibo_ggp_nlml_grad", c_int, c_int, c_int, c_int, c_int, _DP, _DP, _DP, _DP, c_int, c_double, c_double, _DP, c_int,
     POINTER(c_int), POINTER(c_int), _DP, _DP, _DP)
_sig("ibo_ggp_grad_stage_ms", c_int, _DP, c_int)
_SGP = c_void_p                                                            # ibo_sgp_t *
_sig("ibo_sgp_create", c_int, c_int, POINTER(_SGP))
_sig("ibo_sgp_destroy", c_int, _SGP)
_sig("ibo_sgp_fit", c_int, _SGP, c_int, c_int, _DP, c_int, c_double, c_double, c_double, c_int, c_int, _DP, c_int64, _DP, _DP, _DP,
     POINTER(c_int))
_sig("ibo_sgp_add", c_int, _SGP, c_int64, _DP, _DP, _DP, POINTER(c_int))
_sig("ibo_sgp_acq_batch", c_int, _SGP, c_int64, _DP, c_int, c_double, c_int, c_double, c_double, _DP, _DP, _DP)
_sig("ibo_sgp_acq_sweep", c_int, _SGP, c_int64, c_void_p, c_int, c_double, c_int, c_double, c_double, c_int, _DP, c_double, c_int64,
     c_void_p, c_void_p, c_void_p, _DP, POINTER(c_int64))
_sig("ibo_sgp_direct_max", c_int, _SGP, c_int, _DP, _DP, c_int, c_double, c_int, c_double, c_int, c_int, c_int, c_int,
     _DP, _DP, POINTER(c_int64))
_sig("ibo_sgp_nlml", c_int, _SGP, c_int, _DP)
_sig("ibo_sgp_get", c_int, _SGP, c_int, _DP)
_sig("ibo_sgp_stage_ms", c_int, _DP, c_int)
_sig("ibo_sgp_nlml_grad", c_int, c_int, c_int, c_int, _DP, c_int, c_double, c_double, c_double, c_int, c_int, _DP, c_int64, _DP, _DP,
     c_int, POINTER(c_int), POINTER(c_int), _DP, _DP, _DP, _DP, POINTER(c_int))
_sig("ibo_sgp_grad_stage_ms", c_int, _DP, c_int)
_sig("ibo_direct_host", c_int, OBJECTIVE, c_int, _DP, _DP, c_int, c_int, c_int, c_int, _DP, _DP, POINTER(c_int64))
_sig("ibo_nlml_grid", c_int, c_int, c_int, c_int, c_int, _DP, _DP, c_int, _DP, c_int, _DP, c_double, _DP)
_sig("ibo_nlml_grad", c_int, c_int, c_int, c_int, c_int, _DP, _DP, _DP, c_int, c_double, c_double, c_int,
     POINTER(c_int), POINTER(c_int), _DP, _DP)
_sig("ibo_loo_grad", c_int, c_int, c_int, c_int, c_int, _DP, _DP, _DP, c_int, c_double, c_double, c_int,
     POINTER(c_int), POINTER(c_int), _DP, _DP, _DP, _DP)
_sig("ibo_comm_get_unique_id", c_int, c_char_p)
_sig("ibo_comm_init", c_int, c_int, c_int, c_int, c_char_p, POINTER(c_void_p))
_sig("ibo_comm_destroy", c_int, c_void_p)
_sig("ibo_comm_count", c_int, c_void_p, POINTER(c_int))
_sig("ibo_comm_argmax", c_int, c_void_p, c_double, c_int64, _DP, c_int, _DP, POINTER(c_int64), _DP, POINTER(c_int))
_sig("ibo_comm_allreduce_sum", c_int, c_void_p, _DP, c_int64)
_sig("ibo_acq_sweep_exchange", c_int, c_void_p, c_void_p, c_int, c_int64, c_void_p, c_int, c_double, c_int, c_double, c_double,
     c_int, _DP, c_double, c_int64, _DP, POINTER(c_int64), _DP, POINTER(c_int64), _DP, POINTER(c_int))
_sig("ibo_comm_barrier", c_int, c_void_p)
# legacy libego symbols (kept so the .so is a drop-in under the reference's own ctypes code)
_sig("acqmaxGP", _DP, c_int, _DP, _DP, _DP, _DP, _DP, c_int, c_int, c_int, _DP, c_int, _DP, _DP, c_double, _DP, _DP,
     c_double, c_double, c_int, c_int, c_int)
_sig("direct", _DP, OBJECTIVE, c_int, _DP, _DP, c_int, c_int, c_int)
_sig("logCDFs", c_double, c_int, POINTER(c_int), _DP)

EXPORTED = ["ibo_abi_version", "ibo_last_error", "ibo_device_count", "ibo_device_name", "ibo_selftest_mfma", "ibo_gpu_time_ms",
            "ibo_set_option", "ibo_trim", "ibo_dev_alloc", "ibo_dev_free", "ibo_memcpy_h2d", "ibo_memcpy_d2h",
            "ibo_device_synchronize", "ibo_dev_generation", "ibo_gp_create", "ibo_gp_destroy", "ibo_gp_fit", "ibo_gp_fit_with_matrix",
            "ibo_gp_extend", "ibo_gp_reserve", "ibo_gp_remove", "ibo_pref_begin", "ibo_pref_rinv_mul", "ibo_pref_newton_step", "ibo_pref_finish", "ibo_gp_set_y", "ibo_gp_set_kstar_sf2", "ibo_gp_set_prior", "ibo_gp_get_R", "ibo_gp_get_L",
            "ibo_gp_get_W", "ibo_gp_info", "ibo_gp_last_fit_ms", "ibo_cov_matrix", "ibo_spd_solve", "ibo_spd_inverse", "ibo_posterior_batch",
            "ibo_acq_sweep", "ibo_acq_batch", "ibo_acq_grad_batch", "ibo_posterior_cov", "ibo_posterior_sample", "ibo_acq_sweep_incremental", "ibo_sweep_state_info", "ibo_sweep_state_levels", "ibo_last_sweep_kernel_ms", "ibo_direct_max", "ibo_cacq_sweep", "ibo_cacq_batch", "ibo_cacq_grad_batch", "ibo_cacq_direct_max", "ibo_ehvi_sweep", "ibo_ehvi_batch", "ibo_ehvi_grad_batch", "ibo_ehvi_direct_max", "ibo_ehvi_scan_ms", "ibo_mes_sweep", "ibo_mes_batch", "ibo_mes_grad_batch", "ibo_mes_direct_max", "ibo_mes_maxcdf", "ibo_mes_scan_ms", "ibo_kg_sweep", "ibo_kg_batch", "ibo_kg_direct_max", "ibo_kg_stage_ms", "ibo_qei_sweep", "ibo_qei_batch", "ibo_qei_direct_max", "ibo_qei_stage_ms", "ibo_paths_create", "ibo_paths_destroy", "ibo_paths_info", "ibo_paths_coef", "ibo_paths_sweep", "ibo_paths_batch", "ibo_paths_grad_batch", "ibo_paths_direct_max",
            "ibo_ggp_create", "ibo_ggp_destroy", "ibo_ggp_info", "ibo_ggp_fit", "ibo_ggp_get_R", "ibo_ggp_get_L", "ibo_ggp_acq_batch", "ibo_ggp_acq_sweep",
            "ibo_ggp_direct_max", "ibo_ggp_stage_ms", "ibo_ggp_nlml_grad", "ibo_ggp_grad_stage_ms",
            "ibo_sgp_create", "ibo_sgp_destroy", "ibo_sgp_fit", "ibo_sgp_add", "ibo_sgp_acq_batch", "ibo_sgp_acq_sweep", "ibo_sgp_direct_max",
            "ibo_sgp_nlml", "ibo_sgp_get", "ibo_sgp_stage_ms", "ibo_sgp_nlml_grad", "ibo_sgp_grad_stage_ms", "ibo_direct_host", "ibo_nlml_grid", "ibo_nlml_grad", "ibo_gp_loo", "ibo_loo_grad",
            "ibo_comm_get_unique_id", "ibo_comm_init", "ibo_comm_destroy", "ibo_comm_count", "ibo_comm_argmax", "ibo_comm_allreduce_sum", "ibo_acq_sweep_exchange", "ibo_comm_barrier",
            "acqmaxGP", "direct", "logCDFs"]

# include/ibo_abi_ensemble.h: the integrated acquisitions over an ensemble of handles.  A list of its own, as the header is a file of its
# own: EXPORTED is held to ibo_abi.h symbol for symbol.  A library without these fails at import like one without any other entry.
_IACQ = (POINTER(c_void_p), c_int, _DP)                                   # gp, S, w of the ibo_iacq_* entries
_IACQ_SPEC = (c_int, c_double, c_int, c_double, c_double)                  # acq, parm, erf_mode, clamp_lo, ymax
_sig("ibo_iacq_sweep", c_int, *(_IACQ + (c_int64, c_void_p) + _IACQ_SPEC + (c_int, _DP, c_double, c_int64, c_void_p, c_void_p, c_void_p,
                                                                          _DP, POINTER(c_int64))))
_sig("ibo_iacq_batch", c_int, *(_IACQ + (c_int64, _DP) + _IACQ_SPEC + (_DP, _DP, _DP)))
_sig("ibo_iacq_grad_batch", c_int, *(_IACQ + (c_int64, _DP) + _IACQ_SPEC + (_DP, _DP)))
_sig("ibo_iacq_direct_max", c_int, *(_IACQ + (c_int, _DP, _DP) + _IACQ_SPEC + (c_int, c_int, c_int, c_int, _DP, _DP, POINTER(c_int64))))
_sig("ibo_iacq_stage_ms", c_int, _DP, c_int)

EXPORTED_ENSEMBLE = ["ibo_iacq_sweep", "ibo_iacq_batch", "ibo_iacq_grad_batch", "ibo_iacq_direct_max", "ibo_iacq_stage_ms"]


def check(rc):
    if rc == OK:
        return
    msg = lib.ibo_last_error().decode("utf-8", "replace")
    if rc == ERR_NOT_PD:
        raise NotPositiveDefinite(rc, msg)
    raise IBOError(rc, msg)


# IBO_OPTIONS="key=value,key=value": ibo_set_option switches applied when the package is imported (a whole test or benchmark run under
# another route without touching its code: IBO_OPTIONS=super_min_nb=32 python -m pytest tests -m gpu)
for _kv in [kv for kv in os.environ.get("IBO_OPTIONS", "").split(",") if kv.strip()]:
    _k, _, _v = _kv.partition("=")
    check(lib.ibo_set_option(_k.strip().encode(), int(_v)))


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def dp(a):
    return a.ctypes.data_as(_DP)


def device_count():
    n = c_int(0)
    check(lib.ibo_device_count(ctypes.byref(n)))
    return n.value


def gpu_time_ms(device=None):
    """device time the library has measured with HIP events in this process so far (ibo_gpu_time_ms), ms"""
    v = ctypes.c_double(0.0)
    check(lib.ibo_gpu_time_ms(default_device() if device is None else int(device), ctypes.byref(v)))
    return v.value


def trim(device=None):
    """give back the device workspace ibo_nlml_grid keeps between calls"""
    check(lib.ibo_trim(default_device() if device is None else int(device)))


def default_device():
    return int(os.environ.get("IBO_DEVICE", os.environ.get("LOCAL_RANK", "0")))


class DeviceArray(object):
    """A (M, D) fp64 array resident in HBM (candidate sets, per-candidate outputs)."""

    def __init__(self, shape, device=None):
        self.device = default_device() if device is None else device
        self.shape = tuple(int(s) for s in shape)
        self.nbytes = int(np.prod(self.shape)) * 8
        p = c_void_p()
        check(lib.ibo_dev_alloc(self.device, self.nbytes, ctypes.byref(p)))
        self.ptr = p

    @classmethod
    def from_host(cls, a, device=None):
        a = f64(a)
        d = cls(a.shape, device)
        check(lib.ibo_memcpy_h2d(d.device, d.ptr, a.ctypes.data_as(c_void_p), d.nbytes))
        return d

    def generation(self):
        """the library's generation of this allocation (changes with every upload into it; 0 once freed)"""
        if self.ptr is None:
            return 0
        g = ctypes.c_uint64()
        check(lib.ibo_dev_generation(self.device, self.ptr, ctypes.byref(g)))
        return g.value

    def upload(self, a):
        """overwrite the array's contents from host memory (a new generation: kept sweep state is dropped)"""
        a = f64(a)
        if a.size * 8 != self.nbytes:
            raise ValueError("shape mismatch")
        check(lib.ibo_memcpy_h2d(self.device, self.ptr, a.ctypes.data_as(c_void_p), self.nbytes))

    def to_host(self):
        out = np.empty(self.shape, dtype=np.float64)
        check(lib.ibo_memcpy_d2h(self.device, out.ctypes.data_as(c_void_p), self.ptr, self.nbytes))
        return out

    def view_rows(self, start, stop):
        """non-owning view of rows [start, stop) (row-major)"""
        v = object.__new__(DeviceArray)
        row = int(np.prod(self.shape[1:])) * 8 if len(self.shape) > 1 else 8
        v.device = self.device
        v.shape = (stop - start,) + self.shape[1:]
        v.nbytes = (stop - start) * row
        v.ptr = c_void_p(self.ptr.value + start * row)
        v._base = self
        return v

    def free(self):
        if getattr(self, "ptr", None) is not None and not hasattr(self, "_base"):
            try:
                lib.ibo_dev_free(self.device, self.ptr)
            except Exception:
                pass
        self.ptr = None

    def __del__(self):
        self.free()


def rows(X):
    """an (N, D) float64 C-contiguous matrix from a matrix or a sequence of points; a matrix passes through without the
    per-row work np.vstack does (0.9 ms for 2048 rows -- as much as the factorisation it precedes)"""
    if isinstance(X, np.ndarray) and X.ndim == 2:
        return f64(X)
    return f64(np.vstack(X))
