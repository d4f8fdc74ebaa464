"""ctypes binding of libmisti_hip.so (C ABI: include/misti_hip.h).

The library is the only compute path.  If it is missing or no HIP device is
usable, every compute entry point raises - there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

from . import build as _build

CPFIT, TRUE_EPS, SMOOTH, UNFOLDED = 1, 2, 4, 8
HINT_INTEGER_SPLITS = 1
STATUS_TEXT = {
    0: "ok",
    1: "Hit negative value of migration rate",
    2: "Lambda correction failed",
    3: "Infinite coalescent time (two populations in the last interval)",
    4: "Split time / band / pulse structure invalid for this candidate",
    5: "Non-finite intermediate or iteration cap",
    6: "Stiff interval: the contour solve failed and rate x length exceeds 256 series sub-steps of 96",
}
NUMERIC = 5
CURV_BOUNDARY = 7        # point status of misti_curvature only: no two-sided stencil at this point (STATUS_TEXT stays the engine's)
MAX_BANDS, MAX_PULSES, MAX_PARAMS, MAX_NUMT = 8, 8, 16, 255
LANE_ANY, MAX_LANES = -1, 64
ABI_VERSION = 6
TRACE_MAX_CAND, TRACE_MAX_ITER = 64, 200
SCAN_MAX_BEST = 8
SCAN_MAX_GROUPS = 65535
BOOT_NORMALIZE, BOOT_MAX_CHUNKS, BOOT_MAX_DRAWS = 1, 65535, 1 << 24
PARAM_MAX_SITES = 1 << 36


class Band(C.Structure):
    _fields_ = [("pop", C.c_int32), ("start", C.c_int32), ("end", C.c_int32), ("param", C.c_int32), ("value", C.c_double)]


class Pulse(C.Structure):
    _fields_ = [("pop", C.c_int32), ("time", C.c_int32), ("param", C.c_int32), ("_pad", C.c_int32), ("value", C.c_double)]


class Model(C.Structure):
    _fields_ = [("numT", C.c_int32), ("sample_date", C.c_int32), ("flags", C.c_uint32), ("n_band", C.c_int32),
                ("n_pulse", C.c_int32), ("n_param", C.c_int32), ("mixture_th", C.c_double),
                ("times", C.POINTER(C.c_double)), ("lh", C.POINTER(C.c_double)),
                ("bands", C.POINTER(Band)), ("pulses", C.POINTER(Pulse))]


class Hops(C.Structure):
    """``misti_hops_t``: basin hopping around a search."""
    _fields_ = [("niter", C.c_int32), ("T", C.c_double), ("stepsize", C.c_double), ("interval", C.c_int32),
                ("target_accept_rate", C.c_double), ("stepwise_factor", C.c_double), ("nm_maxfev", C.c_int64),
                ("uniforms", C.c_void_p), ("nfev", C.c_void_p), ("failures", C.c_void_p), ("accepted", C.c_void_p)]


SPLIT_ONE, SPLIT_PER_START, SPLIT_FITTED = 0, 1, 2


class Search(C.Structure):
    """``misti_search_t``: one batched search; the header documents the fields."""
    _fields_ = [("size", C.c_uint32), ("split", C.c_int32), ("split_time", C.c_double), ("split_times", C.c_void_p),
                ("n_start", C.c_int64), ("starts", C.c_void_p), ("rows", C.c_void_p), ("n_rep", C.c_int64), ("jsfs", C.c_void_p),
                ("band_bounds", C.c_void_p), ("pulse_times", C.c_void_p), ("n_box", C.c_int64), ("box_lo", C.c_void_p),
                ("box_hi", C.c_void_p), ("xatol", C.c_double), ("fatol", C.c_double), ("maxiter", C.c_int32),
                ("x", C.c_void_p), ("llh", C.c_void_p), ("nit", C.c_void_p), ("nfev", C.c_void_p), ("status", C.c_void_p),
                ("hops", C.POINTER(Hops))]


DE_MAX_POP, DE_BLOCKS = 256, 5


class DeSearch(C.Structure):
    """``misti_de_t``: differential evolution per search; the header documents the fields."""
    _fields_ = [("size", C.c_uint32), ("split", C.c_int32), ("split_times", C.c_void_p), ("n_start", C.c_int64), ("starts", C.c_void_p),
                ("rows", C.c_void_p), ("n_rep", C.c_int64), ("jsfs", C.c_void_p), ("band_bounds", C.c_void_p), ("pulse_times", C.c_void_p),
                ("n_box", C.c_int64), ("box_lo", C.c_void_p), ("box_hi", C.c_void_p), ("pop", C.c_int32), ("maxiter", C.c_int32),
                ("tol", C.c_double), ("atol", C.c_double), ("F_lo", C.c_double), ("F_hi", C.c_double), ("CR", C.c_double),
                ("seed", C.c_uint64), ("ids", C.c_void_p), ("x", C.c_void_p), ("llh", C.c_void_p), ("nit", C.c_void_p),
                ("nfev", C.c_void_p), ("status", C.c_void_p), ("population", C.c_void_p), ("population_llh", C.c_void_p),
                ("n_points", C.c_void_p)]


ENS_MAX_WALKERS = 256


class EnsSample(C.Structure):
    """``misti_ens_t``: ensemble MCMC per search; the header documents the fields."""
    _fields_ = [("size", C.c_uint32), ("split", C.c_int32), ("split_times", C.c_void_p), ("n_start", C.c_int64), ("init", C.c_void_p),
                ("rows", C.c_void_p), ("n_rep", C.c_int64), ("jsfs", C.c_void_p), ("band_bounds", C.c_void_p), ("pulse_times", C.c_void_p),
                ("n_box", C.c_int64), ("box_lo", C.c_void_p), ("box_hi", C.c_void_p), ("walkers", C.c_int32), ("n_step", C.c_int32),
                ("thin", C.c_int32), ("n_temp", C.c_int32), ("temperature", C.c_void_p), ("a", C.c_double), ("seed", C.c_uint64),
                ("ids", C.c_void_p), ("chain", C.c_void_p), ("chain_llh", C.c_void_p), ("accepted", C.c_void_p), ("last", C.c_void_p),
                ("last_llh", C.c_void_p), ("n_points", C.c_void_p)]


PT_MAX_RUNGS = 64


class PtSample(C.Structure):
    """``misti_pt_t``: tempered ensemble MCMC per fit; the header documents the fields."""
    _fields_ = [("size", C.c_uint32), ("split", C.c_int32), ("split_times", C.c_void_p), ("n_start", C.c_int64), ("init", C.c_void_p),
                ("rows", C.c_void_p), ("n_rep", C.c_int64), ("jsfs", C.c_void_p), ("band_bounds", C.c_void_p), ("pulse_times", C.c_void_p),
                ("n_box", C.c_int64), ("box_lo", C.c_void_p), ("box_hi", C.c_void_p), ("walkers", C.c_int32), ("n_rung", C.c_int32),
                ("n_ladder", C.c_int32), ("n_step", C.c_int32), ("ladder", C.c_void_p), ("thin", C.c_int32), ("swap_every", C.c_int32),
                ("burn", C.c_int32), ("a", C.c_double), ("seed", C.c_uint64), ("ids", C.c_void_p), ("chain", C.c_void_p),
                ("chain_llh", C.c_void_p), ("accepted", C.c_void_p), ("swap_proposed", C.c_void_p), ("swap_accepted", C.c_void_p),
                ("last", C.c_void_p), ("last_llh", C.c_void_p), ("rung_llh", C.c_void_p), ("logz", C.c_void_p), ("n_points", C.c_void_p)]


COORD_LINEAR, COORD_LOG = 0, 1
PRIOR_FLAT, PRIOR_NORMAL, PRIOR_EXPONENTIAL = 0, 1, 2


class Prior(C.Structure):
    """``misti_prior_t``: sampling coordinate and prior per coordinate; the header documents the fields."""
    _fields_ = [("size", C.c_uint32), ("n_prior", C.c_int32), ("scale", C.c_void_p), ("kind", C.c_void_p), ("p0", C.c_void_p), ("p1", C.c_void_p)]


POST_MAX_PROBS = 8
POST_SORT_TILE = 2048                # MISTI_POST_SORT_TILE (csrc/misti_post.h): the samples a workgroup sorts in LDS


class EnsPost(C.Structure):
    """``misti_ens_post_t``: posterior summaries of a chain; the header documents the fields."""
    _fields_ = [("size", C.c_uint32), ("burn", C.c_int32), ("n_prob", C.c_int32), ("probs", C.c_void_p), ("max_lag", C.c_int32), ("c", C.c_double),
                ("mean", C.c_void_p), ("cov", C.c_void_p), ("quant", C.c_void_p), ("tau", C.c_void_p), ("window", C.c_void_p),
                ("best_llh", C.c_void_p), ("best_x", C.c_void_p), ("best_at", C.c_void_p),
                ("n_mass", C.c_int32), ("masses", C.c_void_p), ("hpd", C.c_void_p), ("hpd_at", C.c_void_p), ("order", C.c_void_p)]


JOINT_MAX_PAIRS, JOINT_MAX_BINS = 120, 128
JOINT_SLAB = 4096                    # MISTI_JOINT_SLAB (csrc/misti_joint.h): the samples a histogram workgroup bins


class EnsJoint(C.Structure):
    """``misti_ens_joint_t``: joint regions of coordinate pairs of a chain; the header documents the fields."""
    _fields_ = [("size", C.c_uint32), ("burn", C.c_int32), ("n_pair", C.c_int32), ("pairs", C.c_void_p), ("bins", C.c_void_p), ("range", C.c_void_p),
                ("n_mass", C.c_int32), ("masses", C.c_void_p), ("counts", C.c_void_p), ("range_out", C.c_void_p), ("inside", C.c_void_p),
                ("mode", C.c_void_p), ("level", C.c_void_p), ("cells", C.c_void_p), ("held", C.c_void_p)]


BANDS_TILE = 64                      # BANDS_TILE (csrc/misti_bands.h): the samples and the columns of the gather's LDS tile


class Bands(C.Structure):
    """``misti_bands_t``: trajectory bands of the corrected rates; the header documents the fields."""
    _fields_ = [("size", C.c_uint32), ("n_prob", C.c_int32), ("probs", C.c_void_p), ("count", C.c_void_p), ("mean", C.c_void_p), ("quant", C.c_void_p),
                ("lo", C.c_void_p), ("hi", C.c_void_p), ("workspace_bytes", C.c_int64), ("batch_limit", C.c_int64)]


class MistiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libmisti_hip error %d: %s" % (code, msg))
        self.code = code


_PD, _PI = C.POINTER(C.c_double), C.POINTER(C.c_int32)
# every symbol include/misti_hip.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "misti_abi_version": (C.c_int, []),
    "misti_last_error": (C.c_char_p, []),
    "misti_build_id": (C.c_char_p, []),
    "misti_device_count": (C.c_int, []),
    "misti_create": (C.c_int, [C.POINTER(Model), C.c_int, C.POINTER(C.c_void_p)]),
    "misti_destroy": (C.c_int, [C.c_void_p]),
    "misti_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "misti_get_stream": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p)]),
    "misti_sync": (C.c_int, [C.c_void_p]),
    "misti_set_hints": (C.c_int, [C.c_void_p, C.c_uint32]),
    "misti_eval_batch": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_eval_batch_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_eval_batch_pulses": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_eval_batch_pulses_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                              C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_search": (C.c_int, [C.c_void_p, C.POINTER(Search)]),
    "misti_de_search": (C.c_int, [C.c_void_p, C.POINTER(DeSearch)]),
    "misti_de_draws": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_ensemble_sample": (C.c_int, [C.c_void_p, C.POINTER(EnsSample)]),
    "misti_ens_summary_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.POINTER(EnsPost)]),
    "misti_ensemble_posterior": (C.c_int, [C.c_void_p, C.POINTER(EnsSample), C.POINTER(EnsPost)]),
    "misti_tempered_sample": (C.c_int, [C.c_void_p, C.POINTER(PtSample), C.POINTER(EnsPost)]),
    "misti_ensemble_sample_prior": (C.c_int, [C.c_void_p, C.POINTER(EnsSample), C.POINTER(EnsPost), C.POINTER(Prior)]),
    "misti_tempered_sample_prior": (C.c_int, [C.c_void_p, C.POINTER(PtSample), C.POINTER(EnsPost), C.POINTER(Prior)]),
    "misti_ens_joint_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(EnsJoint)]),
    "misti_ensemble_sample_joint": (C.c_int, [C.c_void_p, C.POINTER(EnsSample), C.POINTER(EnsPost), C.POINTER(Prior), C.POINTER(EnsJoint)]),
    "misti_tempered_sample_joint": (C.c_int, [C.c_void_p, C.POINTER(PtSample), C.POINTER(EnsPost), C.POINTER(Prior), C.POINTER(EnsJoint)]),
    "misti_traj_bands_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Bands)]),
    "misti_traj_bands": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Bands)]),
    "misti_bands_rank": (C.c_int, [C.c_int64, C.c_double, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "misti_ens_log_prior": (C.c_int, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_ens_accept_prior": (C.c_int, [C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "misti_pt_swap": (C.c_int, [C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "misti_ens_draws": (C.c_int, [C.c_uint64, C.c_uint64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_ens_exp": (C.c_int, [C.c_double, C.c_void_p]),
    "misti_ens_accept": (C.c_int, [C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "misti_nm_solve": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_double, C.c_double, C.c_int32,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_nm_solve_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_double,
                                      C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_nm_solve_bounds": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_nm_solve_pulses": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                        C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_nm_solve_split": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                       C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_nm_last_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "misti_nm_last_spec_iterations": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "misti_basinhopping": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                     C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int64, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_basinhopping_rows": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32,
                                          C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_basinhopping_split": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                           C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32,
                                           C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_nm_solve_box": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                     C.c_int64, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int32,
                                     C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_basinhopping_box": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_int64, C.c_void_p, C.c_void_p,
                                         C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32,
                                         C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_enable_solver_trace": (C.c_int, [C.c_void_p, C.c_int]),
    "misti_last_solver_trace": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]),
    "misti_llk_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]),
    "misti_forward_rates": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_forward_rates_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_argmax_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_scan_best_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "misti_scan_profile_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_bootstrap_rows_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_uint64, C.c_int64, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p]),
    "misti_bootstrap_draws": (C.c_int, [C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]),
    "misti_jackknife_rows_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_uint32, C.c_void_p]),
    "misti_jackknife_geometry": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p]),
    "misti_parametric_rows_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int64, C.c_uint64, C.c_int64,
                                            C.c_int64, C.c_void_p, C.c_void_p]),
    "misti_parametric_thresholds": (C.c_int, [C.c_void_p, C.c_void_p]),
    "misti_parametric_counts": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.c_int64, C.c_void_p]),
    "misti_parametric_geometry": (C.c_int, [C.c_int64, C.c_int64, C.c_void_p]),
    "misti_curvature_assemble_dev": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_curvature": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.c_double, C.c_double, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_last_diag": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p]),
    "misti_enable_timing": (C.c_int, [C.c_void_p, C.c_int]),
    "misti_kernel_times": (C.c_int, [C.c_void_p, _PD, C.POINTER(C.c_int64), C.c_int]),
    "misti_tables": (C.c_int, [_PI, _PI]),
    "misti_pair_residuals": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "misti_lsq_probe": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "misti_create_lanes": (C.c_int, [C.POINTER(Model), C.c_int, C.c_int, C.POINTER(C.c_void_p)]),
    "misti_destroy_lanes": (C.c_int, [C.c_void_p]),
    "misti_lanes_size": (C.c_int, [C.c_void_p]),
    "misti_lanes_context": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "misti_lanes_set_hints": (C.c_int, [C.c_void_p, C.c_uint32]),
    "misti_lanes_eval_batch_dev": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "misti_lanes_wait": (C.c_int, [C.c_void_p, C.c_int]),
    "misti_lanes_sync": (C.c_int, [C.c_void_p]),
    "misti_lanes_busy": (C.c_int, [C.c_void_p, C.c_int]),
    "misti_create_multi": (C.c_int, [C.POINTER(Model), C.c_int, _PI, C.POINTER(C.c_void_p)]),
    "misti_destroy_multi": (C.c_int, [C.c_void_p]),
    "misti_multi_size": (C.c_int, [C.c_void_p]),
    "misti_multi_context": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_int)]),
    "misti_multi_eval_batch": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_multi_last_shards": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "misti_multi_last_cost": (C.c_int, [C.c_void_p, _PD]),
    "misti_multi_eval_batch_dev": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                             C.c_int64, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p)]),
    "misti_multi_sync": (C.c_int, [C.c_void_p]),
    "misti_multi_nm_solve": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_double, C.c_double, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "misti_multi_basinhopping": (C.c_int, [C.c_void_p, C.c_int64, C.c_void_p, C.c_double, C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                           C.c_double, C.c_double, C.c_double, C.c_double, C.c_int32, C.c_int64, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

_lib = None


def lib_path():
    return _build.LIB


def load(build_if_missing=True):
    """Load (building first if needed) the shared library and bind every symbol."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if os.environ.get("MISTI_LIB"):
        path = os.environ["MISTI_LIB"]          # an explicitly chosen build (kernel experiments); never rebuilt
    elif build_if_missing and _build.have_hipcc():
        _build.build()                           # no-op when the library is newer than every source and header
    elif not os.path.exists(path):
        raise MistiError(-3, "libmisti_hip.so is not built (%s) and hipcc is not available; run misti_amd.build.build()" % path)
    elif _build.stale():
        import warnings
        warnings.warn("libmisti_hip.so is older than its sources and hipcc is not available to rebuild it", RuntimeWarning)
    # One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64; if this
    # library is loaded first it binds the system ROCm runtime and a later `import torch` brings a second one into
    # the process (observed: torch.cuda then intermittently reports "No HIP GPUs are available", and stream or
    # memory handles cross runtimes).  Loaded after torch, the NEEDED libamdhip64.so.7 resolves to the runtime
    # torch already mapped.  Without torch installed the system runtime is the only one.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(path)
    # MISTI_LIB alone keeps every check: an explicitly chosen build must still be THIS ABI (ctypes signatures of another version mean
    # memory corruption, not an error).  Only the A/B tools (tools/ab_compare.py, tools/stamp_run.py), which load older builds on
    # purpose and call nothing whose signature changed, set MISTI_LIB_AB=1 to relax them.
    experimental = bool(os.environ.get("MISTI_LIB")) and os.environ.get("MISTI_LIB_AB") == "1"
    for name, (res, args) in SYMBOLS.items():
        try:
            fn = getattr(lib, name)      # AttributeError if the .so lacks a declared symbol
        except AttributeError:
            if experimental:             # an older build loaded for an A/B measurement: its missing entry points simply cannot be called
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    if lib.misti_abi_version() != ABI_VERSION and not experimental:
        raise MistiError(-1, "ABI version mismatch: %s is version %d, this binding expects %d (rebuild: python -m misti_amd.build --force)"
                         % (path, lib.misti_abi_version(), ABI_VERSION))
    _lib = lib
    return lib


def build_id():
    """The loaded library's own record of the sources it was built from (``misti_build_id``)."""
    return load().misti_build_id().decode()


def check(code):
    if code != 0:
        raise MistiError(code, load().misti_last_error().decode("utf-8", "replace"))
