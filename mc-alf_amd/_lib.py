"""ctypes binding of libmcalf_hip.so (C ABI in include/mcalf_hip.h).

There is no CPU fallback: if the shared library is missing, or no gfx950 device is
present when a context is created, this fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MCALF_HIP_LIB") or os.path.join(_HERE, "csrc", "libmcalf_hip.so")

MCALF_OK = 0
MCALF_ERR_INVALID, MCALF_ERR_HIP, MCALF_ERR_NODEVICE, MCALF_ERR_RANGE, MCALF_ERR_NOMEM, MCALF_ERR_COMM = -1, -2, -3, -4, -5, -6
MCALF_COMM_ID_BYTES = 128
MCALF_CONV_WRAP_NUMPY = 0
MCALF_CONV_SAME_EDGE_JAX = 1
MCALF_EQW_LAYOUT = 0
MCALF_EQW_AS_WRITTEN = 1

_ERR_NAMES = {-1: "MCALF_ERR_INVALID", -2: "MCALF_ERR_HIP", -3: "MCALF_ERR_NODEVICE",
              -4: "MCALF_ERR_RANGE", -5: "MCALF_ERR_NOMEM", -6: "MCALF_ERR_COMM"}


class mcalf_line(C.Structure):
    _fields_ = [("wrest_A", C.c_double), ("f", C.c_double), ("gamma", C.c_double)]


class mcalf_spec(C.Structure):
    _fields_ = [
        ("npix", C.c_int64),
        ("wl", C.POINTER(C.c_double)),
        ("flux", C.POINTER(C.c_double)),
        ("err", C.POINTER(C.c_double)),
        ("velstep", C.c_double),
        ("nlines", C.c_int32),
        ("lines", C.POINTER(mcalf_line)),
        ("fill", mcalf_line),
        ("ncompmax", C.c_int32),
        ("nfill", C.c_int32),
        ("freespecres", C.c_int32),
        ("freecont", C.c_int32),
        ("specres_fixed", C.c_double),
        ("specres_max", C.c_double),
        ("contval_fixed", C.c_double),
        ("conv_mode", C.c_int32),
        ("device", C.c_int32),
        ("asymmlike", C.c_int32),
        ("asymm_n4", C.c_double),
        ("asymm_n5", C.c_double),
    ]


class mcalf_info_t(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32),
        ("ndim", C.c_int32),
        ("startind", C.c_int32),
        ("endind", C.c_int32),
        ("n_cap", C.c_int32),
        ("tile", C.c_int32),
        ("ntiles", C.c_int32),
        ("device", C.c_int32),
        ("npix", C.c_int64),
        ("arch", C.c_char * 32),
        ("ndevices", C.c_int32),
        ("devices", C.c_int32 * 16),
    ]


(MCALF_PATH_NONE, MCALF_PATH_DEVICE, MCALF_PATH_HOST_ZEROCOPY, MCALF_PATH_HOST_PIPELINED, MCALF_PATH_HOST_STAGED,
 MCALF_PATH_HOST_STREAM) = range(6)


class mcalf_launch_info_t(C.Structure):
    _fields_ = [
        ("path", C.c_int32),
        ("row_blocks", C.c_int32),
        ("persistent", C.c_int32),
        ("grid", C.c_int32),
        ("items", C.c_int64),
        ("lines_per_sync", C.c_int32),
        ("selfhalo", C.c_int32),
        ("pinned_in", C.c_int32),
        ("pinned_out", C.c_int32),
        ("inline_setup", C.c_int32),
        ("ordered", C.c_int32),
        ("stream_setup_wgs", C.c_int32),
        ("stream_polled", C.c_int32),
        ("xcd_mask", C.c_int32),
        ("stream_wgs_min", C.c_int32),
        ("stream_wgs_max", C.c_int32),
        ("stream_fallback", C.c_int32),
        ("devices_used", C.c_int32),
    ]


MCALF_STREAM_FALLBACK_SHAPE, MCALF_STREAM_FALLBACK_TIMEOUT, MCALF_STREAM_FALLBACK_STARVED = 1, 2, 3


class mcalf_broker_t(C.Structure):
    _fields_ = [
        ("slots", C.c_int32),
        ("ndim", C.c_int32),
        ("req", C.c_void_p),
        ("ack", C.c_void_p),
        ("counter_stride", C.c_int64),
        ("theta", C.c_void_p),
        ("theta_stride", C.c_int64),
        ("logl", C.c_void_p),
        ("logl_stride", C.c_int64),
        ("stop", C.c_void_p),
        ("stats", C.c_void_p),
        ("idle_sleep_after_s", C.c_double),
    ]


class mcalf_fit_opts(C.Structure):
    _fields_ = [
        ("max_iter", C.c_int32),
        ("cg_iters", C.c_int32),
        ("rows_per_block", C.c_int32),
        ("reserved", C.c_int32),
        ("lambda0", C.c_double),
        ("ftol", C.c_double),
    ]


class mcalf_slice_opts(C.Structure):
    _fields_ = [
        ("nmoves", C.c_int32),
        ("max_steps", C.c_int32),
        ("ndirs", C.c_int32),
        ("reserved", C.c_int32),
        ("seed", C.c_uint64),
    ]


class mcalf_slice_stats_t(C.Structure):
    _fields_ = [
        ("batch", C.c_int64),
        ("rows_launched", C.c_int64),
        ("trials", C.c_int64),
        ("steps", C.c_int32),
        ("compact", C.c_int32),
    ]


class mcalf_ens_opts(C.Structure):
    _fields_ = [
        ("nsteps", C.c_int32),
        ("thin", C.c_int32),
        ("move", C.c_int32),
        ("reserved", C.c_int32),
        ("scale", C.c_double),
        ("seed", C.c_uint64),
        ("first_iter", C.c_uint64),
    ]


class mcalf_pt_opts(C.Structure):
    _fields_ = [
        ("nsteps", C.c_int32),
        ("thin", C.c_int32),
        ("move", C.c_int32),
        ("ntemps", C.c_int32),
        ("swap_every", C.c_int32),
        ("chain_temps", C.c_int32),
        ("scale", C.c_double),
        ("seed", C.c_uint64),
        ("first_iter", C.c_uint64),
    ]


class mcalf_hmc_opts(C.Structure):
    _fields_ = [
        ("nsteps", C.c_int32),
        ("thin", C.c_int32),
        ("nleap", C.c_int32),
        ("reserved", C.c_int32),
        ("eps", C.c_double),
        ("jitter", C.c_double),
        ("seed", C.c_uint64),
        ("first_iter", C.c_uint64),
    ]


class mcalf_chain_opts(C.Structure):
    _fields_ = [
        ("c", C.c_double),
        ("max_lag", C.c_int64),
    ]


class mcalf_converge_opts(C.Structure):
    _fields_ = [
        ("check_every", C.c_int32),
        ("reserved", C.c_int32),
        ("factor", C.c_double),
        ("rtol", C.c_double),
        ("c", C.c_double),
    ]


class mcalf_nested_opts(C.Structure):
    _fields_ = [
        ("batch", C.c_int32),
        ("nmoves", C.c_int32),
        ("max_steps", C.c_int32),
        ("reserved", C.c_int32),
        ("seed", C.c_uint64),
        ("dlogz", C.c_double),
        ("max_dead", C.c_int64),
    ]


class mcalf_nested_state_t(C.Structure):
    _fields_ = [
        ("nlive", C.c_int64),
        ("ndead", C.c_int64),
        ("rounds", C.c_int64),
        ("nevals", C.c_int64),
        ("unfinished", C.c_int64),
        ("rows_launched", C.c_int64),
        ("logX", C.c_double),
        ("logZ", C.c_double),
        ("max_key", C.c_double),
        ("reason", C.c_int32),
        ("reserved", C.c_int32),
    ]


# why mcalf_nested_advance returned
MCALF_NESTED_BUDGET, MCALF_NESTED_CONVERGED, MCALF_NESTED_PLATEAU, MCALF_NESTED_FULL = 0, 1, 2, 3

# the largest ladder of mcalf_tempered_batch
MCALF_PT_MAX_TEMPS = 64

# the moves of mcalf_ensemble_batch
MCALF_ENS_STRETCH, MCALF_ENS_DE = 0, 1

# status of a row of mcalf_slice_replace_batch
MCALF_SLICE_MAXSTEPS, MCALF_SLICE_DONE, MCALF_SLICE_BAD_START = 0, 1, -1

# status of a row of mcalf_maximize_batch
MCALF_FIT_MAXITER, MCALF_FIT_CONVERGED, MCALF_FIT_ZERO_GRADIENT, MCALF_FIT_LAMBDA, MCALF_FIT_BAD_START = 0, 1, 2, 3, -1


# every symbol include/mcalf_hip.h declares: name -> (restype, argtypes).  Array arguments are void*: a plain address is
# accepted, and so is a typed ctypes pointer made from `ndarray.ctypes`, whatever the element type in the header.
_CTX = C.c_void_p
_P = C.c_void_p            # a host or device array, or an options struct, by address
SYMBOLS = {
    "mcalf_create": (C.c_int, [C.POINTER(mcalf_spec), C.POINTER(_CTX)]),
    "mcalf_create_multi": (C.c_int, [C.POINTER(mcalf_spec), C.POINTER(C.c_int32), C.c_int32, C.POINTER(_CTX)]),
    "mcalf_shard_bounds": (C.c_int, [C.c_int64, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "mcalf_destroy": (None, [_CTX]),
    "mcalf_get_config": (C.c_int, [_CTX, C.c_char_p, C.c_int64]),
    "mcalf_last_launch_sub": (C.c_int, [_CTX, C.c_int32, C.POINTER(mcalf_launch_info_t)]),
    "mcalf_info": (C.c_int, [_CTX, C.POINTER(mcalf_info_t)]),
    "mcalf_last_error": (C.c_char_p, [_CTX]),
    "mcalf_version": (C.c_char_p, []),
    "mcalf_reserve": (C.c_int, [_CTX, C.c_int64]),
    "mcalf_set_chunks": (C.c_int, [_CTX, C.c_int32]),
    "mcalf_get_chunks": (C.c_int32, [_CTX, C.c_int64]),
    # (host pointers as void*: plain addresses are accepted, which spares the hot wrappers two ctypes pointer objects per call)
    "mcalf_loglike_batch": (C.c_int, [_CTX, _P, C.c_int64, _P]),
    "mcalf_model_batch": (C.c_int, [_CTX, _P, C.c_int64, C.c_int32, _P]),
    "mcalf_chi2_batch": (C.c_int, [_CTX, _P, C.c_int64, _P]),
    "mcalf_onecomp_batch": (C.c_int, [_CTX, _P, C.c_int64, C.c_int32, _P]),
    "mcalf_loglike_batch_device": (C.c_int, [_CTX, _P, C.c_int64, _P, _P]),
    "mcalf_model_batch_device": (C.c_int, [_CTX, _P, C.c_int64, C.c_int32, _P, _P]),
    "mcalf_loglike_grad_batch": (C.c_int, [_CTX, _P, C.c_int64, _P, _P]),
    "mcalf_loglike_grad_batch_device": (C.c_int, [_CTX, _P, C.c_int64, _P, _P, _P]),
    "mcalf_loglike_hvp_batch": (C.c_int, [_CTX, _P, _P, C.c_int64, _P]),
    "mcalf_loglike_hvp_batch_device": (C.c_int, [_CTX, _P, _P, C.c_int64, _P, _P]),
    "mcalf_eqw_batch": (C.c_int, [_CTX, _P, C.c_int64, C.c_int32, _P, _P]),
    "mcalf_eqw_batch_device": (C.c_int, [_CTX, _P, C.c_int64, C.c_int32, _P, _P, _P]),
    "mcalf_kinematics_batch": (C.c_int, [_CTX, _P, C.c_int64, _P, C.c_int32, _P, _P]),
    "mcalf_kinematics_batch_device": (C.c_int, [_CTX, _P, C.c_int64, _P, C.c_int32, _P, _P, _P]),
    "mcalf_model_band_batch": (C.c_int, [_CTX, _P, C.c_int64, C.c_int32, _P, C.c_int32, _P, _P, _P, _P]),
    "mcalf_model_band_batch_device": (C.c_int, [_CTX, _P, C.c_int64, C.c_int32, _P, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "mcalf_fisher_matvec_batch": (C.c_int, [_CTX, _P, _P, C.c_int64, _P]),
    "mcalf_fisher_matvec_batch_device": (C.c_int, [_CTX, _P, _P, C.c_int64, _P, _P]),
    "mcalf_maximize_batch": (C.c_int, [_CTX, _P, C.c_int64, _P, _P, _P, _P, _P]),
    "mcalf_maximize_batch_device": (C.c_int, [_CTX, _P, C.c_int64, _P, _P, _P, _P, _P, _P]),
    "mcalf_slice_replace_batch": (C.c_int, [_CTX, _P, _P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P]),
    "mcalf_slice_replace_batch_device": (C.c_int, [_CTX, _P, _P, _P, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mcalf_set_slice_compact": (C.c_int, [_CTX, C.c_int32]),
    "mcalf_slice_last_stats": (C.c_int, [_CTX, C.POINTER(mcalf_slice_stats_t)]),
    "mcalf_ensemble_batch": (C.c_int, [_CTX, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mcalf_ensemble_batch_device": (C.c_int, [_CTX, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mcalf_tempered_batch": (C.c_int, [_CTX, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mcalf_tempered_batch_device": (C.c_int, [_CTX, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mcalf_hmc_batch": (C.c_int, [_CTX, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mcalf_hmc_batch_device": (C.c_int, [_CTX, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mcalf_chain_stats": (C.c_int, [_CTX, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, _P]),
    "mcalf_chain_stats_device": (C.c_int, [_CTX, _P, C.c_int64, C.c_int64, C.c_int32, _P, _P, _P, _P, _P, _P]),
    "mcalf_ensemble_converge": (C.c_int, [_CTX, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mcalf_ensemble_converge_device": (C.c_int, [_CTX, _P, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mcalf_nested_open": (C.c_int, [_CTX, _P, C.c_int64, _P]),
    "mcalf_nested_advance": (C.c_int, [_CTX, C.c_int32, _P]),
    "mcalf_nested_finish": (C.c_int, [_CTX, _P, _P, _P]),
    "mcalf_nested_read": (C.c_int, [_CTX, C.c_int64, C.c_int64, _P, _P, _P, _P]),
    "mcalf_nested_last_round": (C.c_int, [_CTX, _P, _P, _P, _P]),
    "mcalf_nested_close": (C.c_int, [_CTX]),
    "mcalf_nested_footprint": (C.c_int, [_CTX, C.POINTER(C.c_int64)]),
    "mcalf_nested_set_timing": (C.c_int, [_CTX, C.c_int32]),
    "mcalf_nested_last_times": (C.c_int, [_CTX, _P]),
    "mcalf_model_jvp_batch": (C.c_int, [_CTX, _P, _P, C.c_int64, _P]),
    "mcalf_model_jvp_batch_device": (C.c_int, [_CTX, _P, _P, C.c_int64, _P, _P]),
    "mcalf_model_vjp_batch": (C.c_int, [_CTX, _P, _P, C.c_int64, _P]),
    "mcalf_model_vjp_batch_device": (C.c_int, [_CTX, _P, _P, C.c_int64, _P, _P]),
    "mcalf_last_launch": (C.c_int, [_CTX, C.POINTER(mcalf_launch_info_t)]),
    "mcalf_set_cu_mask": (C.c_int, [_CTX, _P, C.c_int32]),
    "mcalf_stream_partition": (C.c_int, [C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mcalf_profile_begin": (C.c_int, [_CTX, C.c_int32]),
    "mcalf_profile_end": (C.c_int, [_CTX, C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    "mcalf_scale_cube_batch": (C.c_int, [_CTX, _P, _P, _P, C.c_int64, C.c_int32, _P]),
    "mcalf_set_prior": (C.c_int, [_CTX, _P, _P, C.c_int32]),
    "mcalf_loglike_cube_batch": (C.c_int, [_CTX, _P, C.c_int64, _P, _P]),
    "mcalf_loglike_cube_batch_device": (C.c_int, [_CTX, _P, C.c_int64, _P, _P, _P]),
    "mcalf_set_gauss_prior": (C.c_int, [_CTX, _P, _P]),
    "mcalf_get_gauss_prior": (C.c_int, [_CTX, _P, _P, _P, C.POINTER(C.c_int32)]),
    "mcalf_lnprior_batch": (C.c_int, [_CTX, _P, C.c_int64, C.c_int32, _P]),
    "mcalf_lnprior_batch_device": (C.c_int, [_CTX, _P, C.c_int64, C.c_int32, _P, _P]),
    "mcalf_set_resident": (C.c_int, [_CTX, C.c_int32]),
    "mcalf_broker_serve_resident": (C.c_int, [_CTX, _P, C.c_int32, _P, C.c_int32, _P, C.c_double]),
    "mcalf_broker_serve": (C.c_int, [C.POINTER(_CTX), C.c_int32, C.POINTER(mcalf_broker_t), C.c_double]),
    "mcalf_comm_unique_id": (C.c_int, [_P]),
    "mcalf_comm_init": (C.c_int, [_CTX, _P, C.c_int32, C.c_int32]),
    "mcalf_comm_info": (C.c_int, [_CTX, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "mcalf_comm_destroy": (C.c_int, [_CTX]),
    "mcalf_comm_set_overlap": (C.c_int, [_CTX, C.c_int32]),
    "mcalf_comm_join": (C.c_int, [_CTX, _P]),
    "mcalf_loglike_gather_device": (C.c_int, [_CTX, _P, C.c_int64, _P, _P, C.c_int32, _P]),
    "mcalf_loglike_gatherv_device": (C.c_int, [_CTX, _P, C.c_int64, _P, _P, C.POINTER(C.c_int64), C.c_int32, _P]),
    "mcalf_voigt_hjerting": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32]),
    "mcalf_voigt_hjerting_nodes": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32]),
    "mcalf_voigt_hjerting_grad": (C.c_int, [_P, _P, C.c_int64, _P, C.c_int32]),
}

_lib = None


def load():
    """Load libmcalf_hip.so once and set the prototypes.  Raises if it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is not built. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C mc-alf_amd/csrc`). There is no CPU fallback for this package.")
    # If torch is (or will be) in the process, its bundled HIP runtime must be the one both
    # sides use, otherwise device pointers cannot be shared: import it first when available.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except Exception:  # pragma: no cover - torch is optional for the host-pointer API
            pass
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, ctx=None):
    if rc == MCALF_OK:
        return
    lib = load()
    msg = lib.mcalf_last_error(ctx)
    raise RuntimeError(f"{_ERR_NAMES.get(rc, rc)}: {msg.decode() if msg else ''}")
