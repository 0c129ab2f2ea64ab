"""ctypes binding of libpmpc_hip.so (include/pmpc_abi.h).

The library is built in-tree by `__graft_entry__.build()` / `make -C pmpc_amd/csrc`.  There is no
CPU path: `load()` raises if the shared object is missing, and every solve raises if no HIP device
is present (the product path must fail loudly rather than fall back)."""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

import numpy as np

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["PMPC_HIP_LIB"]) if os.environ.get("PMPC_HIP_LIB") else _HERE / "libpmpc_hip.so"  # (env: diagnostic / A-B builds)
_lib = None

c_dp = ctypes.POINTER(ctypes.c_double)

# flags of pmpc_problem.flags (include/pmpc_abi.h)
HAS_XBOUNDS, HAS_UBOUNDS, HAS_SLEW, HAS_SLEW0, FORCE_GENERIC, SYMMETRIC_COST, COLD_START, STATIC_CONS_BOUNDS, PREV_IS_LAST_SOLUTION, F32_MATRICES, CONE_OBJECTIVE = 1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024

ABI_SYMBOLS = [
    "c_lqp_solve", "c_lcone_solve", "pmpc_lqp_solve_host", "pmpc_lcone_solve_host", "pmpc_create", "pmpc_destroy", "pmpc_stream", "pmpc_sync", "pmpc_lqp_solve_device",
    "pmpc_comm_unique_id", "pmpc_comm_init", "pmpc_comm_rank", "pmpc_comm_world", "pmpc_linearize_device",
    "pmpc_profile_enable", "pmpc_profile_read", "pmpc_version", "pmpc_lcone_solve_device", "pmpc_particle_costs_device", "pmpc_lsoc_solve_device", "pmpc_comm_init_mock",
    "pmpc_scp_residual_device", "pmpc_profile_read_partial", "pmpc_profile_read_all", "pmpc_scp_loop_device", "pmpc_linearize_device_f32",
    "pmpc_set_option", "pmpc_get_option", "pmpc_abi_struct_sizes", "pmpc_lcone_solve_host_ex", "pmpc_restart_stats",
    "pmpc_linearize_compact_device", "pmpc_expand_jac_device", "pmpc_jac_compact_doubles", "pmpc_jac_live_mask",
    "pmpc_as_sweep_variant", "pmpc_as_sweep_launches", "pmpc_as_sweep_knobs", "pmpc_as_sweep_resources", "pmpc_fast_launches",
    "pmpc_ref_shift_device", "pmpc_ref_shift_bad_pivots", "pmpc_obstacle_cost_grad_device", "pmpc_obstacle_ref_shift_device",
    "pmpc_scp_loop_device_cost", "pmpc_abi_scp_cost_size",
    "pmpc_rollout_device", "pmpc_shift_plan_device",
    "pmpc_keepout_augment_device", "pmpc_abi_scp_cstr_size",
    "pmpc_keepout_strip_residual_device", "pmpc_scp_loop_device_cstr", "pmpc_abi_scp_aug_size", "pmpc_scp_loop_follow_ups",
    "pmpc_shift_active_set_device", "pmpc_warm_shift_device", "pmpc_warm_set_read_device",
    "pmpc_model_compile", "pmpc_model_free_code", "pmpc_model_load", "pmpc_model_unload",
    "pmpc_cost_compile", "pmpc_cost_load", "pmpc_cost_unload", "pmpc_custom_cost_grad_device",
    "pmpc_cstr_compile", "pmpc_cstr_load", "pmpc_cstr_unload", "pmpc_custom_cstr_rows_device", "pmpc_rows_augment_device", "pmpc_cstr_bad_rows",
]
MODEL_CUSTOM0 = 1000  # PMPC_MODEL_CUSTOM0 (include/pmpc_abi.h): ids from here on are runtime-compiled models loaded on a context
COST_CUSTOM0 = 1000  # PMPC_COST_CUSTOM0: ids of runtime-compiled stage costs (a table of their own)
CSTR_CUSTOM0 = 1000  # PMPC_CSTR_CUSTOM0: ids of runtime-compiled state constraints (likewise)


class PmpcProblem(ctypes.Structure):
    _fields_ = (
        [(k, ctypes.c_size_t) for k in ("xdim", "udim", "N", "M")]
        + [("Nc", ctypes.c_longlong), ("flags", ctypes.c_uint), ("reg_x", ctypes.c_double), ("reg_u", ctypes.c_double)]
        + [(k, ctypes.c_void_p) for k in ("x0", "f", "fx", "fu", "X_prev", "U_prev", "Q", "R", "X_ref", "U_ref",
                                          "lx", "ux", "lu", "uu", "slew_reg", "slew_reg0", "slew_um1", "X_out", "U_out", "weights")]
        + [("barrier_mu", ctypes.c_double), ("soc_q", ctypes.c_size_t), ("soc_W", ctypes.c_void_p), ("soc_w0", ctypes.c_void_p),
           ("soc_v", ctypes.c_void_p), ("soc_v0", ctypes.c_double), ("soc_u_interior", ctypes.c_void_p),
           ("cone_count", ctypes.c_size_t), ("cone_sizes", ctypes.POINTER(ctypes.c_int)), ("cone_A", ctypes.c_void_p), ("cone_c", ctypes.c_void_p),
           ("cone_per_stage", ctypes.c_int), ("cone_k", ctypes.c_longlong), ("smooth_cstr", ctypes.c_int), ("smooth_beta", ctypes.c_double)]
    )


class PmpcInfo(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int), ("ipm_iters", ctypes.c_int), ("structured_solves", ctypes.c_int),
                ("fast_path", ctypes.c_int), ("mu", ctypes.c_double), ("slack_res", ctypes.c_double),
                ("max_violation", ctypes.c_double), ("outer_solves", ctypes.c_int), ("active_set_rounds", ctypes.c_int)]


class _KOrId(ctypes.Union):
    _fields_ = [("K", ctypes.c_int), ("id", ctypes.c_int)]


class _PosDimOrUsesU(ctypes.Union):
    _fields_ = [("pos_dim", ctypes.c_int), ("uses_u", ctypes.c_int)]


class _CentresOrCparams(ctypes.Union):
    _fields_ = [("centres", ctypes.c_void_p), ("cparams", ctypes.c_void_p)]


class PmpcScpCost(ctypes.Structure):
    """pmpc_scp_cost (include/pmpc_abi.h): the cost of pmpc_scp_loop_device_cost — kind 1 the built-in obstacles, kind 2 a loaded custom
    cost, whose id / uses_u / cparams share the storage of K / pos_dim / centres."""
    _anonymous_ = ("_a", "_b", "_c")
    _fields_ = [("kind", ctypes.c_int), ("_a", _KOrId), ("_b", _PosDimOrUsesU), ("pos_idx", ctypes.c_int * 3), ("per_stage", ctypes.c_int),
                ("_c", _CentresOrCparams), ("sigma", ctypes.c_void_p), ("w", ctypes.c_void_p)]


class _PosDimOrCstrId(ctypes.Union):
    _fields_ = [("pos_dim", ctypes.c_int), ("id", ctypes.c_int)]


class _CentresOrGparams(ctypes.Union):
    _fields_ = [("centres", ctypes.c_void_p), ("gparams", ctypes.c_void_p)]


class PmpcScpCstr(ctypes.Structure):
    """pmpc_scp_cstr (include/pmpc_abi.h): the constraint of pmpc_scp_loop_device_cstr — kind 1 the built-in keep-out, kind 2 a loaded
    custom constraint, whose id / gparams share the storage of pos_dim / centres (K is the row count of both)."""
    _anonymous_ = ("_a", "_b")
    _fields_ = [("kind", ctypes.c_int), ("K", ctypes.c_int), ("_a", _PosDimOrCstrId), ("pos_idx", ctypes.c_int * 3),
                ("centre_stride_particle", ctypes.c_longlong), ("centre_stride_stage", ctypes.c_longlong),
                ("_b", _CentresOrGparams), ("radius", ctypes.c_void_p)]


class PmpcScpAug(ctypes.Structure):
    """pmpc_scp_aug (include/pmpc_abi.h): the augmented buffers of pmpc_scp_loop_device_cstr."""
    _fields_ = ([(k, ctypes.c_void_p) for k in ("Q", "x0", "lx")] + [(k, ctypes.c_void_p * 2) for k in ("f", "fx", "fu", "X_prev", "X_ref", "xu")]
                + [("X_out", ctypes.c_void_p)])


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ImportError(
            f"{LIB_PATH} is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()' "
            "or make -C pmpc_amd/csrc). pmpc_amd has no CPU fallback.")
    lib = ctypes.CDLL(str(LIB_PATH), mode=ctypes.RTLD_GLOBAL)
    sz, ll, dbl, vp = ctypes.c_size_t, ctypes.c_longlong, ctypes.c_double, ctypes.c_void_p
    common = [c_dp, c_dp, sz, sz, sz, sz, ll] + [c_dp] * 14 + [dbl, dbl] + [c_dp] * 3 + [ll]
    lib.c_lqp_solve.argtypes = common
    lib.c_lqp_solve.restype = None
    lib.c_lcone_solve.argtypes = common + [dbl, ctypes.c_char_p]
    lib.c_lcone_solve.restype = None
    lib.pmpc_lqp_solve_host.argtypes = common + [ctypes.c_uint]
    lib.pmpc_lqp_solve_host.restype = None
    lib.pmpc_lcone_solve_host.argtypes = common + [dbl, ctypes.c_uint, ll]
    lib.pmpc_lcone_solve_host.restype = None
    lib.pmpc_lcone_solve_host_ex.argtypes = common + [dbl, ctypes.c_uint, ll, ctypes.c_int, dbl]
    lib.pmpc_lcone_solve_host_ex.restype = None
    lib.pmpc_create.argtypes = [ctypes.POINTER(vp), ctypes.c_int]
    lib.pmpc_create.restype = ctypes.c_int
    lib.pmpc_destroy.argtypes = [vp]
    lib.pmpc_destroy.restype = None
    lib.pmpc_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_double]
    lib.pmpc_set_option.restype = ctypes.c_int
    lib.pmpc_get_option.argtypes = [vp, ctypes.c_char_p, c_dp]
    lib.pmpc_get_option.restype = ctypes.c_int
    lib.pmpc_stream.argtypes = [vp]
    lib.pmpc_stream.restype = vp
    lib.pmpc_sync.argtypes = [vp]
    lib.pmpc_sync.restype = None
    lib.pmpc_lqp_solve_device.argtypes = [vp, ctypes.POINTER(PmpcProblem), ctypes.POINTER(PmpcInfo), ctypes.c_int]
    lib.pmpc_lqp_solve_device.restype = ctypes.c_int
    lib.pmpc_lcone_solve_device.argtypes = [vp, ctypes.POINTER(PmpcProblem), dbl, ctypes.POINTER(PmpcInfo), ctypes.c_int]
    lib.pmpc_lcone_solve_device.restype = ctypes.c_int
    lib.pmpc_lsoc_solve_device.argtypes = [vp, ctypes.POINTER(PmpcProblem), ctypes.POINTER(PmpcInfo), ctypes.c_int]
    lib.pmpc_lsoc_solve_device.restype = ctypes.c_int
    lib.pmpc_particle_costs_device.argtypes = [vp, ctypes.POINTER(PmpcProblem), vp, vp, vp]
    lib.pmpc_particle_costs_device.restype = ctypes.c_int
    lib.pmpc_comm_unique_id.argtypes = [vp]
    lib.pmpc_comm_unique_id.restype = ctypes.c_int
    lib.pmpc_comm_init.argtypes = [vp, ctypes.c_int, ctypes.c_int, vp]
    lib.pmpc_comm_init.restype = ctypes.c_int
    lib.pmpc_comm_init_mock.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.pmpc_comm_init_mock.restype = ctypes.c_int
    lib.pmpc_comm_rank.argtypes = [vp]
    lib.pmpc_comm_rank.restype = ctypes.c_int
    lib.pmpc_comm_world.argtypes = [vp]
    lib.pmpc_comm_world.restype = ctypes.c_int
    lib.pmpc_linearize_device.argtypes = [vp, ctypes.c_int, sz, sz] + [vp] * 7
    lib.pmpc_linearize_device.restype = ctypes.c_int
    lib.pmpc_linearize_device_f32.argtypes = [vp, ctypes.c_int, sz, sz] + [vp] * 7
    lib.pmpc_linearize_device_f32.restype = ctypes.c_int
    if hasattr(lib, "pmpc_jac_live_mask"):  # (an A/B library of an older source, PMPC_HIP_LIB, may lack the compact-record entry points)
        lib.pmpc_linearize_compact_device.argtypes = [vp, ctypes.c_int, sz, sz] + [vp] * 6
        lib.pmpc_linearize_compact_device.restype = ctypes.c_int
        lib.pmpc_expand_jac_device.argtypes = [vp, ctypes.c_int, sz, sz, vp, vp, vp, ctypes.c_int]
        lib.pmpc_expand_jac_device.restype = ctypes.c_int
        lib.pmpc_jac_compact_doubles.argtypes = [ctypes.c_int, sz, sz]
        lib.pmpc_jac_compact_doubles.restype = ctypes.c_longlong
        lib.pmpc_jac_live_mask.argtypes = [ctypes.c_int, vp, vp]
        lib.pmpc_jac_live_mask.restype = ctypes.c_int
    if hasattr(lib, "pmpc_as_sweep_variant"):  # (likewise)
        lib.pmpc_as_sweep_variant.argtypes = [ctypes.c_int] * 5 + [ctypes.c_uint, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        lib.pmpc_as_sweep_variant.restype = ctypes.c_int
    if hasattr(lib, "pmpc_as_sweep_launches"):  # (likewise)
        lib.pmpc_as_sweep_launches.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
        lib.pmpc_as_sweep_launches.restype = ctypes.c_int
        lib.pmpc_as_sweep_knobs.argtypes = [ctypes.POINTER(ctypes.c_int)]
        lib.pmpc_as_sweep_knobs.restype = None
    if hasattr(lib, "pmpc_fast_launches"):  # (likewise)
        lib.pmpc_fast_launches.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int, ctypes.c_int]
        lib.pmpc_fast_launches.restype = ctypes.c_int
    if hasattr(lib, "pmpc_as_sweep_resources"):  # (likewise)
        lib.pmpc_as_sweep_resources.argtypes = [ctypes.c_int] * 3 + [ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
        lib.pmpc_as_sweep_resources.restype = ctypes.c_int
    lib.pmpc_scp_residual_device.argtypes = [vp, sz, sz, sz, sz] + [vp] * 5
    lib.pmpc_scp_residual_device.restype = ctypes.c_int
    lib.pmpc_profile_enable.argtypes = [vp, ctypes.c_int]
    lib.pmpc_profile_enable.restype = None
    lib.pmpc_profile_read.argtypes = [vp, c_dp, ctypes.POINTER(ctypes.c_longlong)]
    lib.pmpc_profile_read.restype = None
    lib.pmpc_profile_read_partial.argtypes = [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_longlong)]
    lib.pmpc_profile_read_partial.restype = None
    lib.pmpc_restart_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
    lib.pmpc_restart_stats.restype = None
    lib.pmpc_profile_read_all.argtypes = [vp, c_dp, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
    lib.pmpc_profile_read_all.restype = None
    lib.pmpc_scp_loop_device.argtypes = [vp, ctypes.c_int, vp, ctypes.POINTER(PmpcProblem), vp, vp, vp, ctypes.c_int, ctypes.c_int, vp,
                                         ctypes.POINTER(PmpcInfo), ctypes.POINTER(ctypes.c_int)]
    lib.pmpc_scp_loop_device.restype = ctypes.c_int
    if hasattr(lib, "pmpc_scp_loop_device_cost"):  # (likewise: an A/B library of an older source has no cost entry points)
        lib.pmpc_ref_shift_device.argtypes = [vp, sz, sz, vp, vp, vp, vp]
        lib.pmpc_ref_shift_device.restype = ctypes.c_int
        lib.pmpc_ref_shift_bad_pivots.argtypes = [vp, ctypes.c_int]
        lib.pmpc_ref_shift_bad_pivots.restype = ctypes.c_longlong
        lib.pmpc_obstacle_cost_grad_device.argtypes = [vp, ctypes.POINTER(PmpcScpCost), sz, sz, sz, vp, vp]
        lib.pmpc_obstacle_cost_grad_device.restype = ctypes.c_int
        lib.pmpc_obstacle_ref_shift_device.argtypes = [vp, ctypes.POINTER(PmpcScpCost), sz, sz, sz, vp, vp, vp, vp]
        lib.pmpc_obstacle_ref_shift_device.restype = ctypes.c_int
        lib.pmpc_scp_loop_device_cost.argtypes = lib.pmpc_scp_loop_device.argtypes + [ctypes.POINTER(PmpcScpCost)]
        lib.pmpc_scp_loop_device_cost.restype = ctypes.c_int
        lib.pmpc_abi_scp_cost_size.argtypes = []
        lib.pmpc_abi_scp_cost_size.restype = sz
        if lib.pmpc_abi_scp_cost_size() != ctypes.sizeof(PmpcScpCost):
            raise ImportError(f"{LIB_PATH} and pmpc_amd/_lib.py disagree on pmpc_scp_cost: library {lib.pmpc_abi_scp_cost_size()} bytes, "
                              f"binding {ctypes.sizeof(PmpcScpCost)}: rebuild the library")
    if hasattr(lib, "pmpc_shift_plan_device"):  # (likewise: the rollout / plan-shift entry points)
        lib.pmpc_rollout_device.argtypes = [vp, ctypes.c_int, sz, sz, vp, vp, vp, vp]
        lib.pmpc_rollout_device.restype = ctypes.c_int
        lib.pmpc_shift_plan_device.argtypes = [vp, ctypes.c_int, sz, sz, sz] + [vp] * 7
        lib.pmpc_shift_plan_device.restype = ctypes.c_int
    if hasattr(lib, "pmpc_keepout_augment_device"):  # (likewise: the keep-out constraint)
        lib.pmpc_keepout_augment_device.argtypes = [vp, ctypes.POINTER(PmpcScpCstr), sz, sz, sz, sz] + [vp] * 11
        lib.pmpc_keepout_augment_device.restype = ctypes.c_int
        lib.pmpc_abi_scp_cstr_size.argtypes = []
        lib.pmpc_abi_scp_cstr_size.restype = sz
        if lib.pmpc_abi_scp_cstr_size() != ctypes.sizeof(PmpcScpCstr):
            raise ImportError(f"{LIB_PATH} and pmpc_amd/_lib.py disagree on pmpc_scp_cstr: library {lib.pmpc_abi_scp_cstr_size()} bytes, "
                              f"binding {ctypes.sizeof(PmpcScpCstr)}: rebuild the library")
    if hasattr(lib, "pmpc_scp_loop_device_cstr"):  # (likewise: the keep-out constraint in the library loop)
        lib.pmpc_keepout_strip_residual_device.argtypes = [vp, sz, ctypes.c_int, sz, sz, sz] + [vp] * 6
        lib.pmpc_keepout_strip_residual_device.restype = ctypes.c_int
        lib.pmpc_scp_loop_device_cstr.argtypes = lib.pmpc_scp_loop_device_cost.argtypes + [ctypes.POINTER(PmpcScpCstr), ctypes.POINTER(PmpcScpAug)]
        lib.pmpc_scp_loop_device_cstr.restype = ctypes.c_int
        lib.pmpc_scp_loop_follow_ups.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
        lib.pmpc_scp_loop_follow_ups.restype = None
        lib.pmpc_abi_scp_aug_size.argtypes = []
        lib.pmpc_abi_scp_aug_size.restype = sz
        if lib.pmpc_abi_scp_aug_size() != ctypes.sizeof(PmpcScpAug):
            raise ImportError(f"{LIB_PATH} and pmpc_amd/_lib.py disagree on pmpc_scp_aug: library {lib.pmpc_abi_scp_aug_size()} bytes, "
                              f"binding {ctypes.sizeof(PmpcScpAug)}: rebuild the library")
    if hasattr(lib, "pmpc_warm_shift_device"):  # (likewise: the active set moved along with the plan)
        lib.pmpc_shift_active_set_device.argtypes = [vp, sz, sz, sz, ll, sz] + [vp] * 7
        lib.pmpc_shift_active_set_device.restype = ctypes.c_int
        lib.pmpc_warm_shift_device.argtypes = [vp, sz, sz, sz, ll, sz] + [vp] * 5 + [ctypes.POINTER(ctypes.c_int)]
        lib.pmpc_warm_shift_device.restype = ctypes.c_int
        lib.pmpc_warm_set_read_device.argtypes = [vp, vp, sz]
        lib.pmpc_warm_set_read_device.restype = ctypes.c_int
    if hasattr(lib, "pmpc_model_compile"):  # (likewise: runtime-compiled dynamics models)
        lib.pmpc_model_compile.argtypes = [ctypes.c_char_p] + [ctypes.c_int] * 3 + [ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.c_char_p, sz]
        lib.pmpc_model_compile.restype = ctypes.c_int
        lib.pmpc_model_free_code.argtypes = [vp]
        lib.pmpc_model_free_code.restype = None
        lib.pmpc_model_load.argtypes = [vp, ctypes.c_char_p, sz] + [ctypes.c_int] * 3
        lib.pmpc_model_load.restype = ctypes.c_int
        lib.pmpc_model_unload.argtypes = [vp, ctypes.c_int]
        lib.pmpc_model_unload.restype = ctypes.c_int
    if hasattr(lib, "pmpc_cost_compile"):  # (likewise: runtime-compiled stage costs)
        lib.pmpc_cost_compile.argtypes = [ctypes.c_char_p] + [ctypes.c_int] * 4 + [ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.c_char_p, sz]
        lib.pmpc_cost_compile.restype = ctypes.c_int
        lib.pmpc_cost_load.argtypes = [vp, ctypes.c_char_p, sz] + [ctypes.c_int] * 4
        lib.pmpc_cost_load.restype = ctypes.c_int
        lib.pmpc_cost_unload.argtypes = [vp, ctypes.c_int]
        lib.pmpc_cost_unload.restype = ctypes.c_int
        lib.pmpc_custom_cost_grad_device.argtypes = [vp, ctypes.c_int, sz, sz] + [vp] * 6
        lib.pmpc_custom_cost_grad_device.restype = ctypes.c_int
    if hasattr(lib, "pmpc_cstr_compile"):  # (likewise: runtime-compiled state constraints)
        lib.pmpc_cstr_compile.argtypes = [ctypes.c_char_p] + [ctypes.c_int] * 3 + [ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(sz), ctypes.c_char_p, sz]
        lib.pmpc_cstr_compile.restype = ctypes.c_int
        lib.pmpc_cstr_load.argtypes = [vp, ctypes.c_char_p, sz] + [ctypes.c_int] * 3
        lib.pmpc_cstr_load.restype = ctypes.c_int
        lib.pmpc_cstr_unload.argtypes = [vp, ctypes.c_int]
        lib.pmpc_cstr_unload.restype = ctypes.c_int
        lib.pmpc_custom_cstr_rows_device.argtypes = [vp, ctypes.c_int, sz, sz] + [vp] * 5
        lib.pmpc_custom_cstr_rows_device.restype = ctypes.c_int
        lib.pmpc_rows_augment_device.argtypes = [vp, ctypes.c_int, sz, sz, sz, sz] + [vp] * 13
        lib.pmpc_rows_augment_device.restype = ctypes.c_int
        lib.pmpc_cstr_bad_rows.argtypes = [vp, ctypes.c_int]
        lib.pmpc_cstr_bad_rows.restype = ctypes.c_longlong
    lib.pmpc_version.argtypes = []
    lib.pmpc_version.restype = ctypes.c_char_p
    # layout check: the library's structs against this binding's mirrors (include/pmpc_abi.h: pmpc_abi_struct_sizes)
    if not hasattr(lib, "pmpc_abi_struct_sizes"):
        raise ImportError(f"{LIB_PATH} predates this binding (no pmpc_abi_struct_sizes): rebuild it (make -C pmpc_amd/csrc)")
    lib.pmpc_abi_struct_sizes.argtypes = [ctypes.POINTER(sz), ctypes.POINTER(sz)]
    lib.pmpc_abi_struct_sizes.restype = None
    sp, si = sz(0), sz(0)
    lib.pmpc_abi_struct_sizes(ctypes.byref(sp), ctypes.byref(si))
    if (sp.value, si.value) != (ctypes.sizeof(PmpcProblem), ctypes.sizeof(PmpcInfo)):
        raise ImportError(f"{LIB_PATH} ({lib.pmpc_version().decode()}) and pmpc_amd/_lib.py disagree on the ABI structs: library "
                          f"{sp.value}/{si.value} bytes, binding {ctypes.sizeof(PmpcProblem)}/{ctypes.sizeof(PmpcInfo)}: rebuild the library")
    _lib = lib
    return lib


def jac_live_mask(model: int, x: int, u: int):
    """(fx_mask (x, x), fu_mask (x, u)) as [row, column] boolean arrays: the Jacobian entries of a built-in model that its compact
    records store per (particle, stage); every other entry is taken as a constant of the particle.  Host only."""
    lib = load()
    mx, mu = np.zeros(x * x, dtype=np.uint8), np.zeros(x * u, dtype=np.uint8)
    got = lib.pmpc_jac_live_mask(int(model), mx.ctypes.data, mu.ctypes.data)
    if got < 0:
        raise ValueError(f"model {model} is not a built-in model")
    if got != 100 * x + u:
        raise ValueError(f"model {model}: compact records are for dims {got // 100} x {got % 100}, not {x} x {u}")
    return mx.reshape(x, x).T.astype(bool), mu.reshape(u, x).T.astype(bool)  # (column-major blocks)


AS_SWEEP_FLAGS = ("defect", "as_settled_in", "mat32", "cone_H", "xb_D", "as_uraw", "as_T")  # bit k of `flags` below


def as_sweep_variant(sweep: str, x: int, u: int, M: int, Nc: int, flags: int, knobs=None):
    """(variant, compiled, dims): the template arguments the launcher of the active-set factor ("bwd") / forward ("fwd") sweep would
    pick (pmpc_amd/csrc/as_variant.h) as a tuple — bwd (mode, skip, defect, ex, f32), fwd (defect, pf2, cone, f32, sens) —, whether
    that instantiation exists for (x, u), and whether the pair has (fp32-storage, cone, state-box) sweeps at all.  knobs:
    (deep2_maxm, deep_maxm, fwd_pf2_maxm), None = the defaults.  Host only."""
    lib = load()
    out = (ctypes.c_int * 8)()
    kn = (ctypes.c_int * 3)(*knobs) if knobs is not None else None
    got = lib.pmpc_as_sweep_variant({"bwd": 0, "fwd": 1}[sweep], x, u, M, Nc, flags, kn, out)
    if got < 0:
        raise ValueError(f"({x}, {u}) is not a compiled pair of the active-set sweeps")
    return tuple(out[:5]), bool(got), tuple(bool(v) for v in out[5:8])


def as_sweep_resources(sweep: str, x: int, u: int, variant):
    """{"regs", "scratch_bytes", "lds_bytes", "max_threads"} of the compiled instantiation `variant` (a record as as_sweep_variant
    returns it) of the factor ("bwd") / forward ("fwd") sweep for (x, u), from the loaded code object; None if that variant is not
    compiled for the pair.  Needs a device, launches nothing."""
    out = (ctypes.c_int * 4)()
    got = load().pmpc_as_sweep_resources({"bwd": 0, "fwd": 1}[sweep], x, u, (ctypes.c_int * 5)(*(int(v) for v in variant)), out)
    if got == -2:
        return None
    if got == -1:
        raise ValueError(f"({x}, {u}) is not a compiled pair of the active-set sweeps")
    if got != 0:
        raise RuntimeError(f"pmpc_as_sweep_resources: HIP error {got}")
    return dict(zip(("regs", "scratch_bytes", "lds_bytes", "max_threads"), (int(v) for v in out)))


def as_sweep_code(sweep: str, variant) -> int:
    """Where pmpc_as_sweep_launches keeps the count of a variant record (the tuple as_sweep_variant returns): the layout that
    include/pmpc_abi.h states."""
    a, b, c, d, e = (int(v) for v in variant)
    if sweep == "bwd":  # (mode, skip, defect, ex, f32)
        return a + 3 * (b + 2 * (c + 2 * (d + 3 * e)))
    return a + 2 * b + 4 * c + 8 * d + 16 * e  # (defect, pf2, cone, f32, sens)


def as_sweep_launches(sweep: str, reset: bool = False):
    """Launch counts of this process's active-set factor ("bwd") / forward ("fwd") sweeps per variant, indexed by as_sweep_code;
    reset: start counting afresh.  Counts launches, not work: a sweep enqueued behind the round that finished the solve returns at once."""
    lib = load()
    sw = {"bwd": 0, "fwd": 1}[sweep]
    n = lib.pmpc_as_sweep_launches(sw, None, 0, 0)
    out = (ctypes.c_ulonglong * n)()
    lib.pmpc_as_sweep_launches(sw, out, n, int(reset))
    return [int(v) for v in out]


FAST_LAUNCH_KINDS = {"sweep": 0, "cond": 1, "cons": 2}
CONS_SOLVE_VARIANTS = ("plain", "blocked", "lds", "reg12", "reg17")


def fast_sweep_code(factor, hxb, hub, deep) -> int:
    """Where fast_launches("sweep") keeps the count of k_bwd_fast<.., FACTOR, HXB, HUB, DEEP> (include/pmpc_abi.h)."""
    return int(bool(factor)) + 2 * int(bool(hxb)) + 4 * int(bool(hub)) + 8 * int(bool(deep))


def cons_solve_code(variant: str, factor) -> int:
    """Where fast_launches("cons") keeps the count of a dense consensus solve: variant of CONS_SOLVE_VARIANTS, factor or vector-only."""
    return CONS_SOLVE_VARIANTS.index(variant) + 5 * int(bool(factor))


def fast_launches(kind: str, reset: bool = False):
    """Launch counts of this process's equality / interior-point kernels (pmpc_fast_launches): kind "sweep" indexed by fast_sweep_code,
    "cond" by 0 k_cond_fast / 1 k_cond_fast_grouped, "cons" by cons_solve_code; reset: start counting afresh."""
    lib = load()
    kd = FAST_LAUNCH_KINDS[kind]
    n = lib.pmpc_fast_launches(kd, None, 0, 0)
    out = (ctypes.c_ulonglong * n)()
    lib.pmpc_fast_launches(kd, out, n, int(reset))
    return [int(v) for v in out]


def scp_loop_follow_ups(reset: bool = False):
    """(behind, after): iterations of this process's library SCP loops whose follow-up (residual, next linearisation) was taken as
    enqueued behind the sub-problem's first batch of rounds / was enqueued after the solve had returned; reset: start counting afresh."""
    out = (ctypes.c_ulonglong * 2)()
    load().pmpc_scp_loop_follow_ups(out, int(reset))
    return int(out[0]), int(out[1])


def as_sweep_knobs():
    """(deep2_maxm, deep_maxm, fwd_pf2_maxm) as the launchers of this process read them from the environment (once)."""
    out = (ctypes.c_int * 3)()
    load().pmpc_as_sweep_knobs(out)
    return tuple(out)


def dptr(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_dp)
