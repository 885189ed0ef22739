"""ctypes binding of libglsamd.so (include/gls_op.h) — Python mirror of the
reference's OperatorBase<Number> interface (include/operator_base.h:13-73)
for the matrix-free GLS Navier–Stokes operator on MI355X.

Vectors are torch tensors on the GPU (torch is plumbing: device memory and
streams); every compute call goes through the HIP kernels of libglsamd.so.
There is no CPU fallback: a missing library or GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIBDIR = os.path.normpath(os.path.join(_HERE, "..", "lib"))
_lib = None

GLS_F64, GLS_F32 = 0, 1
GLS_INCREMENT_FORM, GLS_CONSIDER_TIME_DERIVATIVE, GLS_CELL_WISE_STAB = 1, 2, 4
GLS_DETERMINISTIC = 8

# exported symbols of include/gls_op.h (checked by tests/test_abi.py)
EXPORTS = [
    "gls_op_create", "gls_op_destroy", "gls_op_set_parameters", "gls_op_m",
    "gls_op_precision", "gls_op_set_linearization_point", "gls_op_set_previous_solution",
    "gls_op_vmult", "gls_op_vmult_interface_down", "gls_op_vmult_interface_up",
    "gls_op_vmult_cells", "gls_op_vmult_init", "gls_op_apply_identity_rows",
    "gls_op_evaluate_residual", "gls_op_evaluate_residual_plain", "gls_op_evaluate_rhs",
    "gls_op_set_constraint_values", "gls_gmres_solve",
    "gls_op_compute_inverse_diagonal", "gls_op_upload_tables", "gls_op_download_tables",
    "gls_op_geometry_counts", "gls_op_vmult_bytes", "gls_mg_create", "gls_mg_destroy",
    "gls_mg_setup", "gls_mg_get_relaxation", "gls_mg_vcycle", "gls_mg_prolongate_add",
    "gls_mg_restrict_add", "gls_mg_interpolate", "gls_mg_smooth", "gls_last_error",
    "gls_dist_unique_id", "gls_dist_create", "gls_dist_destroy", "gls_dist_vmult",
    "gls_dist_vmult_group", "gls_dist_interior_bricks", "gls_op_set_vector_layout",
    "gls_op_get_max_u", "gls_mg_set_vector_layout", "gls_dist_update_ghost_values",
    "gls_dist_get_max_u", "gls_op_compute_diagonal", "gls_op_invert_diagonal", "gls_mg_relax",
    "gls_dist_compress_add", "gls_op_brick_shape", "gls_op_sweep_stats", "gls_op_cell_permutation",
    "gls_op_set_sweep_spin_bound",
    "gls_timer_enable", "gls_timer_reset", "gls_timer_n_sections", "gls_timer_section",
    "gls_timer_report", "gls_timer_begin", "gls_timer_end",
    "gls_discover_bricks", "gls_mg_coarse_statistics", "gls_mg_coarse_setup_times",
    "gls_amg_create", "gls_amg_destroy", "gls_amg_vmult", "gls_amg_info", "gls_mg_coarse_amg",
    "gls_amg_level_matrix",
    "gls_dist_mg_create", "gls_dist_mg_destroy", "gls_dist_mg_set_linearization_point",
    "gls_dist_mg_setup", "gls_dist_mg_get_relaxation", "gls_dist_mg_vcycle",
    "gls_dist_gmres_solve", "gls_op_element_matrices",
    "gls_op_system_matrix", "gls_op_n_outflow_faces", "gls_op_outflow_face_points",
    "gls_op_set_outflow_target",
    "gls_op_set_force_faces", "gls_op_surface_force", "gls_op_surface_force_faces",
    "gls_op_set_probe_points", "gls_op_probe", "gls_dist_surface_force", "gls_dist_probe",
    "gls_mg_set_coarse_direct", "gls_mg_coarse_direct_info",
    "gls_nd_plan_create", "gls_nd_plan_destroy", "gls_nd_plan_info", "gls_nd_plan_node",
    "gls_ilu_create", "gls_ilu_refactor", "gls_ilu_destroy", "gls_ilu_vmult", "gls_ilu_info",
    "gls_ilu_factors", "gls_ilu_host_factor", "gls_amg_create_ilu", "gls_gmres_solve_prec",
    "gls_mg_set_coarse_ilu", "gls_mg_set_coarse_amg_ilu", "gls_mg_coarse_ilu",
    "gls_op_system_matrix_device", "gls_op_invalidate_system", "gls_op_set_matrix_based",
    "gls_assemble_plan_host",
    "gls_ilu_refactor_device", "gls_ilu_create_device", "gls_ilu_factor_info",
    "gls_ilu_factor_host", "gls_mg_set_coarse_ilu_device",
    "gls_op_set_node_constraints", "gls_op_n_node_constraints", "gls_op_distribute",
]

GLS_PREC_MG, GLS_PREC_ILU, GLS_PREC_AMG = 0, 1, 2

GLS_COARSE_DENSE, GLS_COARSE_ND = 0, 1

GLS_MEM_DEVICE, GLS_MEM_HOST = 0, 1


class OpDesc(C.Structure):
    _fields_ = [("dim", C.c_int), ("degree", C.c_int), ("precision", C.c_int),
                ("n_cells", C.c_int64), ("n_nodes", C.c_int64), ("n_owned_nodes", C.c_int64),
                ("cell_nodes", C.c_void_p), ("node_coords", C.c_void_p),
                ("node_cmask", C.c_void_p), ("cell_measure", C.c_void_p),
                ("cell_hmin", C.c_void_p), ("brick", C.c_int * 3),
                ("n_outflow_faces", C.c_int64), ("outflow_cells", C.c_void_p),
                ("outflow_face_no", C.c_void_p), ("outflow_kind", C.c_void_p),
                ("mapping_degree", C.c_int), ("mapping_points", C.c_void_p),
                ("node_master", C.c_void_p)]

OUTFLOW_KIND = {"cut": 1, "nitsche": 2}


class OpParams(C.Structure):
    _fields_ = [("nu", C.c_double), ("c1", C.c_double), ("c2", C.c_double),
                ("theta", C.c_double), ("w0", C.c_double), ("dt", C.c_double),
                ("order", C.c_int), ("flags", C.c_int)]


class AMGParams(C.Structure):
    _fields_ = [("block_size", C.c_int), ("threshold", C.c_double),
                ("smoother_sweeps", C.c_int), ("coarse_max_size", C.c_int),
                ("elliptic", C.c_int), ("max_levels", C.c_int),
                ("chebyshev_alpha", C.c_double)]


def amg_params(block_size=1, threshold=1e-4, smoother_sweeps=2, coarse_max_size=2000,
               elliptic=True, max_levels=10, chebyshev_alpha=10.0):
    """glsAMGParams; the defaults are TrilinosWrappers::PreconditionAMG::
    AdditionalData()'s (one constant mode, threshold 1e-4, 2 smoother sweeps,
    elliptic) with the ML parameters deal.II sets ("coarse: max size" 2000,
    "smoother: Chebyshev alpha" 10)."""
    return AMGParams(int(block_size), float(threshold), int(smoother_sweeps),
                     int(coarse_max_size), int(bool(elliptic)), int(max_levels),
                     float(chebyshev_alpha))


class MGDesc(C.Structure):
    _fields_ = [("n_levels", C.c_int), ("smoothing_n_iterations", C.c_int),
                ("smoothing_eig_n_iterations", C.c_int), ("smoothing_range", C.c_double),
                ("coarse_n_iterations", C.c_int), ("outer_precision", C.c_int),
                ("compute_evs_n_levels", C.c_int), ("coarse_iterate", C.c_int),
                ("coarse_reltol", C.c_double), ("coarse_maxiter", C.c_int),
                ("coarse_amg", C.c_int), ("amg", AMGParams)]


class CoarseDirectInfo(C.Structure):
    _fields_ = [("method", C.c_int), ("requested", C.c_int), ("max_leaf_cells", C.c_int),
                ("n_free", C.c_int64), ("tree_nodes", C.c_int), ("depth", C.c_int),
                ("max_own", C.c_int), ("max_boundary", C.c_int),
                ("stored_entries", C.c_int64), ("stored_bytes", C.c_int64),
                ("plan_ms", C.c_double), ("factor_ms", C.c_double), ("narrow_ms", C.c_double)]


class NdPlanInfo(C.Structure):
    _fields_ = [("n_dofs", C.c_int64), ("n_tree_nodes", C.c_int), ("depth", C.c_int),
                ("sum_own", C.c_int64), ("stored_entries", C.c_int64),
                ("max_own", C.c_int), ("max_boundary", C.c_int)]


class NdPlanNode(C.Structure):
    _fields_ = [("parent", C.c_int), ("child", C.c_int * 2), ("level", C.c_int),
                ("n_own", C.c_int), ("n_boundary", C.c_int), ("n_cells", C.c_int),
                ("own", C.POINTER(C.c_int32)), ("boundary", C.POINTER(C.c_int32)),
                ("map", C.POINTER(C.c_int32)), ("cells", C.POINTER(C.c_int32))]


class ILUParams(C.Structure):
    _fields_ = [("fill_level", C.c_int), ("atol", C.c_double), ("rtol", C.c_double)]


class AMGIluParams(C.Structure):
    _fields_ = [("smoother_ilu", C.c_int), ("coarse_ilu", C.c_int), ("fill_level", C.c_int),
                ("atol", C.c_double), ("rtol", C.c_double)]


class DeviceCSR(C.Structure):
    _fields_ = [("n", C.c_int64), ("nnz", C.c_int64), ("row_ptr", C.c_void_p),
                ("cols", C.c_void_p), ("vals", C.c_void_p)]


class AssemblePlanHost(C.Structure):
    _fields_ = [("n_dofs", C.c_int64), ("nnz", C.c_int64), ("n_pairs", C.c_int64),
                ("n_incidence", C.c_int64), ("max_cells_per_node", C.c_int),
                ("row_ptr", C.c_void_p), ("cols", C.c_void_p), ("pair_ptr", C.c_void_p),
                ("pair_node", C.c_void_p), ("pair_off", C.c_void_p), ("inc_ptr", C.c_void_p),
                ("inc_cell", C.c_void_p), ("inc_point", C.c_void_p)]


def ilu_params(fill_level=0, atol=1e-12, rtol=1.0):
    """glsILUParams; the defaults are the reference's PreconditionerILU
    (preconditioner.cc:5-28)"""
    return ILUParams(int(fill_level), float(atol), float(rtol))


def amg_ilu_params(smoother_ilu=True, coarse_ilu=True, fill_level=1, atol=1e-6, rtol=1.0):
    """glsAMGIluParams; the defaults are the reference's non-default AMG
    parameters (multigrid.h:52-53, multigrid.cc:403-413)"""
    return AMGIluParams(int(bool(smoother_ilu)), int(bool(coarse_ilu)), int(fill_level),
                        float(atol), float(rtol))


class ILUInfo(C.Structure):
    _fields_ = [("n", C.c_int64), ("nnz_a", C.c_int64), ("nnz_l", C.c_int64),
                ("nnz_u", C.c_int64), ("levels_l", C.c_int), ("levels_u", C.c_int),
                ("launches_l", C.c_int), ("launches_u", C.c_int), ("max_level_rows", C.c_int),
                ("group", C.c_int), ("narrow", C.c_int), ("chain", C.c_int),
                ("min_pivot", C.c_double), ("symbolic_ms", C.c_double),
                ("numeric_ms", C.c_double), ("upload_ms", C.c_double)]


class ILUHostFactor(C.Structure):
    _fields_ = [("n", C.c_int64), ("nnz_l", C.c_int64), ("nnz_u", C.c_int64),
                ("levels_l", C.c_int), ("levels_u", C.c_int), ("launches_l", C.c_int),
                ("launches_u", C.c_int), ("group", C.c_int), ("narrow", C.c_int),
                ("chain", C.c_int), ("min_pivot", C.c_double),
                ("l_row_ptr", C.c_void_p), ("l_cols", C.c_void_p), ("u_row_ptr", C.c_void_p),
                ("u_cols", C.c_void_p), ("l_vals", C.c_void_p), ("u_vals", C.c_void_p),
                ("row_level_l", C.c_void_p), ("row_level_u", C.c_void_p),
                ("order_l", C.c_void_p), ("order_u", C.c_void_p),
                ("launch_l", C.c_void_p), ("launch_u", C.c_void_p),
                ("solve_dst", C.c_void_p), ("solve_src", C.c_void_p)]


class ILUFactorInfo(C.Structure):
    _fields_ = [("levels", C.c_int), ("launches", C.c_int), ("chains", C.c_int),
                ("narrow", C.c_int), ("group", C.c_int), ("rows", C.c_int), ("chain", C.c_int),
                ("device", C.c_int), ("max_row", C.c_int64), ("max_row_limit", C.c_int64),
                ("factor_ms", C.c_double)]


class ILUFactorHost(C.Structure):
    _fields_ = [("n", C.c_int64), ("nnz_l", C.c_int64), ("nnz_u", C.c_int64),
                ("max_row", C.c_int64), ("levels", C.c_int), ("launches", C.c_int),
                ("chains", C.c_int), ("narrow", C.c_int), ("group", C.c_int), ("rows", C.c_int),
                ("chain", C.c_int), ("min_pivot", C.c_double),
                ("l_row_ptr", C.c_void_p), ("l_cols", C.c_void_p), ("u_row_ptr", C.c_void_p),
                ("u_cols", C.c_void_p), ("l_vals", C.c_void_p), ("u_vals", C.c_void_p),
                ("row_level", C.c_void_p), ("order", C.c_void_p), ("launch", C.c_void_p)]


class DistDesc(C.Structure):
    _fields_ = [("rank", C.c_int), ("world", C.c_int), ("nccl_id", C.c_void_p),
                ("group", C.c_void_p), ("n_peers", C.c_int), ("peers", C.c_void_p),
                ("send_count", C.c_void_p), ("send_nodes", C.c_void_p),
                ("recv_begin", C.c_void_p), ("recv_count", C.c_void_p)]


class GMRESDesc(C.Structure):
    _fields_ = [("max_n_tmp_vectors", C.c_int), ("max_iterations", C.c_int),
                ("absolute_tolerance", C.c_double), ("relative_tolerance", C.c_double)]


class GMRESResult(C.Structure):
    _fields_ = [("n_iterations", C.c_int), ("n_restarts", C.c_int), ("converged", C.c_int),
                ("initial_residual", C.c_double), ("final_residual", C.c_double),
                ("tolerance", C.c_double)]


def lib_path():
    return os.path.join(LIBDIR, "libglsamd.so")


def lib():
    global _lib
    if _lib is None:
        path = os.environ.get("GLS_AMD_LIB") or lib_path()
        if not os.path.exists(path):
            raise RuntimeError(f"{path} missing: run `make amd` (or __graft_entry__.build())")
        L = C.CDLL(path)
        vp, i64 = C.c_void_p, C.c_int64
        L.gls_op_create.argtypes = [C.POINTER(OpDesc), C.POINTER(vp)]
        L.gls_op_destroy.argtypes = [vp]
        L.gls_op_set_parameters.argtypes = [vp, C.POINTER(OpParams)]
        L.gls_op_m.argtypes = [vp]
        L.gls_op_m.restype = i64
        L.gls_op_precision.argtypes = [vp]
        L.gls_op_set_linearization_point.argtypes = [vp, vp, vp]
        L.gls_op_set_previous_solution.argtypes = [vp, vp, C.c_int, vp, vp]
        L.gls_op_vmult.argtypes = [vp, vp, vp, vp]
        L.gls_op_vmult_interface_down.argtypes = [vp, vp, vp, vp]
        L.gls_op_vmult_interface_up.argtypes = [vp, vp, vp, vp]
        L.gls_op_vmult_cells.argtypes = [vp, vp, vp, i64, i64, vp]
        L.gls_op_vmult_init.argtypes = [vp, vp, vp, vp]
        L.gls_op_apply_identity_rows.argtypes = [vp, vp, vp, vp]
        L.gls_op_evaluate_residual.argtypes = [vp, vp, vp, vp]
        L.gls_op_evaluate_residual_plain.argtypes = [vp, vp, vp, vp]
        L.gls_op_evaluate_rhs.argtypes = [vp, vp, vp]
        L.gls_op_set_constraint_values.argtypes = [vp, vp, vp]
        L.gls_op_set_node_constraints.argtypes = [vp, i64, vp, vp, vp, vp]
        L.gls_op_n_node_constraints.argtypes = [vp, C.POINTER(i64), C.POINTER(C.c_int)]
        L.gls_op_distribute.argtypes = [vp, vp, C.c_int, vp]
        L.gls_op_compute_inverse_diagonal.argtypes = [vp, vp, vp]
        L.gls_op_upload_tables.argtypes = [vp, vp, vp]
        L.gls_op_download_tables.argtypes = [vp, vp, vp]
        L.gls_op_geometry_counts.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
        L.gls_op_vmult_bytes.argtypes = [vp]
        L.gls_op_vmult_bytes.restype = C.c_double
        L.gls_mg_create.argtypes = [C.POINTER(MGDesc), vp, vp, C.POINTER(vp)]
        L.gls_mg_destroy.argtypes = [vp]
        L.gls_mg_setup.argtypes = [vp, vp]
        L.gls_mg_get_relaxation.argtypes = [vp, C.c_int, C.POINTER(C.c_double),
                                            C.POINTER(C.c_double)]
        L.gls_mg_vcycle.argtypes = [vp, vp, vp, vp]
        for f in ("gls_mg_prolongate_add", "gls_mg_restrict_add", "gls_mg_interpolate"):
            getattr(L, f).argtypes = [vp, C.c_int, vp, vp, vp]
        L.gls_mg_smooth.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp]
        L.gls_dist_unique_id.argtypes = [vp]
        L.gls_dist_create.argtypes = [vp, C.POINTER(DistDesc), C.POINTER(vp)]
        L.gls_dist_destroy.argtypes = [vp]
        L.gls_dist_vmult.argtypes = [vp, vp, vp, vp]
        L.gls_dist_vmult_group.argtypes = [vp, vp, vp, C.c_int, vp]
        L.gls_dist_interior_bricks.argtypes = [vp, C.POINTER(i64), C.POINTER(i64)]
        L.gls_gmres_solve.argtypes = [vp, vp, C.POINTER(GMRESDesc), vp, vp,
                                      C.POINTER(GMRESResult), vp]
        L.gls_op_set_vector_layout.argtypes = [vp, C.c_int, vp]
        L.gls_op_get_max_u.argtypes = [vp, vp, C.POINTER(C.c_double), vp]
        L.gls_mg_set_vector_layout.argtypes = [vp, C.c_int, vp]
        L.gls_dist_update_ghost_values.argtypes = [vp, vp, vp]
        L.gls_dist_get_max_u.argtypes = [vp, vp, C.POINTER(C.c_double), vp]
        L.gls_op_compute_diagonal.argtypes = [vp, vp, vp]
        L.gls_op_invert_diagonal.argtypes = [vp, vp, vp]
        L.gls_mg_relax.argtypes = [vp, C.c_int, vp, vp, vp, vp, C.c_double, C.c_int, vp]
        L.gls_dist_compress_add.argtypes = [vp, vp, vp]
        L.gls_op_brick_shape.argtypes = [vp, vp]
        L.gls_op_sweep_stats.argtypes = [vp, vp, vp]
        L.gls_op_set_sweep_spin_bound.argtypes = [vp, C.c_int64]
        L.gls_op_cell_permutation.argtypes = [vp, vp]
        L.gls_op_element_matrices.argtypes = [vp, vp]
        L.gls_op_system_matrix.argtypes = [vp, C.POINTER(i64), vp, vp, vp]
        L.gls_op_n_outflow_faces.argtypes = [vp, C.POINTER(i64), C.POINTER(C.c_int)]
        L.gls_op_outflow_face_points.argtypes = [vp, vp]
        L.gls_op_set_outflow_target.argtypes = [vp, vp, vp]
        L.gls_op_system_matrix_device.argtypes = [vp, C.POINTER(DeviceCSR), vp]
        L.gls_op_invalidate_system.argtypes = [vp]
        L.gls_op_set_matrix_based.argtypes = [vp, C.c_int]
        L.gls_assemble_plan_host.argtypes = [C.c_int, C.c_int, i64, i64, vp, vp,
                                             C.POINTER(AssemblePlanHost)]
        L.gls_op_set_force_faces.argtypes = [vp, i64, vp, vp, vp, C.c_int]
        L.gls_op_surface_force.argtypes = [vp, vp, vp, vp]
        L.gls_op_surface_force_faces.argtypes = [vp, vp, vp, vp]
        L.gls_op_set_probe_points.argtypes = [vp, i64, vp, vp, vp]
        L.gls_op_probe.argtypes = [vp, vp, vp, vp]
        L.gls_dist_surface_force.argtypes = [vp, vp, vp, vp]
        L.gls_dist_probe.argtypes = [vp, vp, vp, vp]
        L.gls_mg_coarse_statistics.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.gls_mg_coarse_setup_times.argtypes = [vp, vp, C.POINTER(C.c_int)]
        L.gls_amg_create.argtypes = [i64, vp, vp, vp, C.POINTER(AMGParams), C.POINTER(vp)]
        L.gls_amg_destroy.argtypes = [vp]
        L.gls_amg_destroy.restype = None
        L.gls_amg_vmult.argtypes = [vp, vp, vp, vp]
        L.gls_amg_info.argtypes = [vp, C.POINTER(C.c_int), vp, vp, vp]
        L.gls_amg_level_matrix.argtypes = [vp, C.c_int, C.c_int, C.POINTER(i64), C.POINTER(i64),
                                           vp, vp, vp]
        L.gls_mg_coarse_amg.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_double)]
        L.gls_dist_mg_create.argtypes = [vp, vp, vp]
        L.gls_dist_mg_destroy.argtypes = [vp]
        L.gls_dist_mg_destroy.restype = None
        L.gls_dist_mg_set_linearization_point.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp]
        L.gls_dist_mg_setup.argtypes = [vp, C.c_int, vp]
        L.gls_dist_mg_get_relaxation.argtypes = [vp, C.c_int, C.POINTER(C.c_double),
                                                 C.POINTER(C.c_double)]
        L.gls_dist_mg_vcycle.argtypes = [vp, C.c_int, vp, vp, vp]
        L.gls_dist_gmres_solve.argtypes = [vp, vp, C.c_int, vp, vp, vp, vp, vp]
        L.gls_discover_bricks.argtypes = [C.c_int, C.c_int, i64, vp, vp, vp]
        L.gls_mg_set_coarse_direct.argtypes = [vp, C.c_int, C.c_int]
        L.gls_mg_coarse_direct_info.argtypes = [vp, C.POINTER(CoarseDirectInfo)]
        L.gls_nd_plan_create.argtypes = [vp, i64, C.c_int, i64, vp, C.c_int, C.POINTER(vp)]
        L.gls_nd_plan_destroy.argtypes = [vp]
        L.gls_nd_plan_destroy.restype = None
        L.gls_nd_plan_info.argtypes = [vp, C.POINTER(NdPlanInfo)]
        L.gls_nd_plan_node.argtypes = [vp, C.c_int, C.POINTER(NdPlanNode)]
        L.gls_ilu_create.argtypes = [i64, vp, vp, vp, C.POINTER(ILUParams), C.POINTER(vp)]
        L.gls_ilu_refactor.argtypes = [vp, vp]
        L.gls_ilu_destroy.argtypes = [vp]
        L.gls_ilu_destroy.restype = None
        L.gls_ilu_vmult.argtypes = [vp, vp, vp, vp]
        L.gls_ilu_info.argtypes = [vp, C.POINTER(ILUInfo)]
        L.gls_ilu_factors.argtypes = [vp, C.c_int, C.POINTER(i64), vp, vp, vp]
        L.gls_ilu_host_factor.argtypes = [i64, vp, vp, vp, C.POINTER(ILUParams),
                                          C.POINTER(ILUHostFactor)]
        L.gls_ilu_refactor_device.argtypes = [vp, vp, vp]
        L.gls_ilu_create_device.argtypes = [C.POINTER(DeviceCSR), C.POINTER(ILUParams), vp,
                                            C.POINTER(vp)]
        L.gls_ilu_factor_info.argtypes = [vp, C.POINTER(ILUFactorInfo)]
        L.gls_ilu_factor_host.argtypes = [i64, vp, vp, vp, C.POINTER(ILUParams),
                                          C.POINTER(ILUFactorHost)]
        L.gls_mg_set_coarse_ilu_device.argtypes = [vp, C.c_int]
        L.gls_amg_create_ilu.argtypes = [i64, vp, vp, vp, C.POINTER(AMGParams),
                                         C.POINTER(AMGIluParams), C.POINTER(vp)]
        L.gls_gmres_solve_prec.argtypes = [vp, C.c_int, vp, C.POINTER(GMRESDesc), vp, vp,
                                           C.POINTER(GMRESResult), vp]
        L.gls_mg_set_coarse_ilu.argtypes = [vp, C.POINTER(ILUParams)]
        L.gls_mg_set_coarse_amg_ilu.argtypes = [vp, C.POINTER(AMGIluParams)]
        L.gls_mg_coarse_ilu.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_double)]
        L.gls_last_error.restype = C.c_char_p
        L.gls_timer_enable.argtypes = [C.c_int, C.POINTER(C.c_int)]
        L.gls_timer_reset.argtypes = []
        L.gls_timer_n_sections.argtypes = []
        L.gls_timer_n_sections.restype = i64
        L.gls_timer_section.argtypes = [i64, C.c_char_p, i64, C.POINTER(i64),
                                        C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.gls_timer_begin.argtypes = [C.c_char_p, vp, C.POINTER(vp)]
        L.gls_timer_end.argtypes = [vp]
        L.gls_timer_report.argtypes = [C.c_char_p, i64]
        L.gls_timer_report.restype = i64
        _lib = L
    return _lib


class GlsError(RuntimeError):
    pass


# ---- timer sections (gls_timer_*: MyTimerOutput / MyScope, timer.h:194-413)
def timer_enable(on=True):
    """Tally the library's timer sections (host wall time and GPU time
    between events on each section's stream); returns the previous state.
    Sections are roctx ranges either way."""
    was = C.c_int(0)
    _check(lib().gls_timer_enable(1 if on else 0, C.byref(was)))
    return bool(was.value)


def timer_reset():
    _check(lib().gls_timer_reset())


def timer_sections():
    """{name: {"calls", "host_ms", "gpu_ms"}} (gpu_ms None without events);
    reading waits for the sections' pending events."""
    L = lib()
    out = {}
    name = C.create_string_buffer(256)
    for i in range(L.gls_timer_n_sections()):
        calls, hms, gms = C.c_int64(0), C.c_double(0), C.c_double(0)
        _check(L.gls_timer_section(i, name, 256, C.byref(calls), C.byref(hms), C.byref(gms)))
        out[name.value.decode()] = {"calls": calls.value, "host_ms": hms.value,
                                    "gpu_ms": gms.value if gms.value >= 0 else None}
    return out


class timer_scope:
    """MyScope (timer.h:342-413) around the caller's own code: a timer
    section (roctx range; tallied when timing is on) on torch's current
    stream, e.g. `with glsamd.timer_scope("newton::solve"): ...`."""

    def __init__(self, name, stream=None):
        self.name, self.stream = name.encode(), stream
        self.tok = C.c_void_p()

    def __enter__(self):
        s = self.stream if self.stream is not None else _stream_or_null()
        _check(lib().gls_timer_begin(self.name, s, C.byref(self.tok)))
        return self

    def __exit__(self, *exc):
        _check(lib().gls_timer_end(self.tok))
        return False


def _stream_or_null():
    try:
        import torch
        if torch.cuda.is_available():
            return _stream()
    except ImportError:
        pass
    return None


def timer_report():
    """The tally as TimerOutput-style text (print_wall_time_statistics)."""
    L = lib()
    n = L.gls_timer_report(None, 0)
    buf = C.create_string_buffer(int(n))
    L.gls_timer_report(buf, n)
    return buf.value.decode()


def _check(rc):
    if rc != 0:
        raise GlsError(lib().gls_last_error().decode())


def _stream():
    """torch's current stream on the current device, as the C ABI's stream
    argument.  torch._C._cuda_getCurrentRawStream returns the handle without
    building a Stream object (3.0 us per call on the box for the public
    form, profiles/r06/explore/host_overhead.txt); the public form where it
    is absent."""
    import torch
    raw = getattr(torch._C, "_cuda_getCurrentRawStream", None)
    if raw is not None:
        return C.c_void_p(raw(torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _vptr(v):
    """Device tensor or host numpy array (GLS_MEM_HOST layouts)."""
    if isinstance(v, np.ndarray):
        assert v.flags["C_CONTIGUOUS"]
        return C.c_void_p(v.ctypes.data)
    return _ptr(v)


class _DeviceArray:
    """A 1D device array the library owns, through __cuda_array_interface__
    (torch.as_tensor views it without a copy; torch takes no read-only
    flag: the callers copy and never write through the view)."""

    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = dict(shape=(int(n),), typestr=typestr,
                                             data=(int(ptr), False), version=2, strides=None)


def assemble_plan_host(cell_nodes, cmask, dim, degree, n_nodes=None):
    """gls_assemble_plan_host (host only, no GPU): dict with the CSR pattern
    (row_ptr, cols), the node pairs (pair_ptr, pair_node, pair_off) and the
    node->cell incidence (inc_ptr, inc_cell, inc_point)."""
    cn = np.ascontiguousarray(cell_nodes, dtype=np.uint32)
    cm = np.ascontiguousarray(cmask, dtype=np.uint8)
    n_nodes = len(cm) if n_nodes is None else int(n_nodes)
    n_cells = cn.shape[0] if cn.ndim == 2 else 0
    P = AssemblePlanHost()
    args = (int(dim), int(degree), n_cells, n_nodes, cn.ctypes.data, cm.ctypes.data, C.byref(P))
    _check(lib().gls_assemble_plan_host(*args))
    out = dict(row_ptr=np.empty(P.n_dofs + 1, np.int64), cols=np.empty(P.nnz, np.int32),
               pair_ptr=np.empty(n_nodes + 1, np.int64), pair_node=np.empty(P.n_pairs, np.int32),
               pair_off=np.empty(P.n_pairs, np.int32), inc_ptr=np.empty(n_nodes + 1, np.int64),
               inc_cell=np.empty(P.n_incidence, np.int32),
               inc_point=np.empty(P.n_incidence, np.int32))
    for k, v in out.items():
        setattr(P, k, v.ctypes.data)
    _check(lib().gls_assemble_plan_host(*args))
    out.update(n_dofs=P.n_dofs, nnz=P.nnz, n_pairs=P.n_pairs, n_incidence=P.n_incidence,
               max_cells_per_node=P.max_cells_per_node)
    return out


def discover_bricks(mesh_or_cells, dim=None, degree=None):
    """gls_discover_bricks: (shape, perm) for a cell list in any order (host
    only).  Accepts a mesh (cell_nodes, dim, degree) or a cell_nodes array."""
    if dim is None:
        cn, dim, degree = mesh_or_cells.cell_nodes, mesh_or_cells.dim, mesh_or_cells.degree
    else:
        cn = mesh_or_cells
    cn = np.ascontiguousarray(cn, dtype=np.uint32)
    shape = (C.c_int * 3)()
    perm = np.empty(cn.shape[0], dtype=np.int64)
    _check(lib().gls_discover_bricks(int(dim), int(degree), cn.shape[0], cn.ctypes.data, shape,
                                     perm.ctypes.data))
    return tuple(shape), perm


class NavierStokesOperator:
    """Mirror of NavierStokesOperator<dim, Number> (operator_ns.h:17-189) over
    the HIP C-ABI.  precision: "f64" (fine level, Number=double) or "f32"
    (MG levels, MGNumber=float, config.h:6-7)."""

    def __init__(self, mesh, cmask, precision="f64", cells=None, n_owned_nodes=None,
                 brick=None, outflow=None, node_constraints=None, node_master=None):
        import torch
        if not torch.cuda.is_available():
            raise GlsError("NavierStokesOperator needs a GPU (no CPU fallback by design)")
        self.mesh = mesh
        self.dim = mesh.dim
        self.degree = mesh.degree
        self.prec = GLS_F64 if precision in ("f64", "double", GLS_F64) else GLS_F32
        self.dtype = torch.float64 if self.prec == GLS_F64 else torch.float32
        cell_nodes = mesh.cell_nodes if cells is None else mesh.cell_nodes[cells]
        meas, hmin = mesh.cell_measure()
        if cells is not None:
            meas, hmin = meas[cells], hmin[cells]
        self._keep = [np.ascontiguousarray(cell_nodes, dtype=np.uint32),
                      np.ascontiguousarray(mesh.coords, dtype=np.float64),
                      np.ascontiguousarray(cmask, dtype=np.uint8),
                      np.ascontiguousarray(meas), np.ascontiguousarray(hmin)]
        k = self._keep
        self.n_cells = k[0].shape[0]
        if brick is None:
            brick = mesh.brick() if cells is None else (0, 0, 0)
        elif brick == "auto":  # any cell order: bricks discovered by the library
            brick = (-1, -1, -1)
        self.brick = tuple(brick)
        d = OpDesc(self.dim, self.degree, self.prec, self.n_cells, mesh.n_nodes,
                   mesh.n_nodes if n_owned_nodes is None else n_owned_nodes,
                   k[0].ctypes.data, k[1].ctypes.data, k[2].ctypes.data, k[3].ctypes.data,
                   k[4].ctypes.data, (C.c_int * 3)(*self.brick))
        if outflow is not None:
            # (cells, face_no, kind): the weak outflow faces (all_outflow_bcs_*,
            # operator_ns.cc:79-95); kind "cut" / "nitsche" or per face 1 / 2
            fc, fn, kind = outflow
            fc = np.ascontiguousarray(fc, dtype=np.int64)
            fn = np.ascontiguousarray(fn, dtype=np.int32)
            if isinstance(kind, str):
                kind = np.full(len(fc), OUTFLOW_KIND[kind], dtype=np.int32)
            kind = np.ascontiguousarray(kind, dtype=np.int32)
            self._keep += [fc, fn, kind]
            d.n_outflow_faces = len(fc)
            d.outflow_cells, d.outflow_face_no, d.outflow_kind = (
                fc.ctypes.data, fn.ctypes.data, kind.ctypes.data)
        mp = getattr(mesh, "mapping_points", None)
        mapping = mp() if callable(mp) else None
        if mapping is not None:
            # MappingQ of the parent (FE_Q_iso_Q1 level): per-cell support points
            mdeg, pts = mapping
            pts = np.ascontiguousarray(pts if cells is None else pts[cells], dtype=np.float64)
            self._keep.append(pts)
            d.mapping_degree, d.mapping_points = int(mdeg), pts.ctypes.data
        self.node_master = None
        if node_master is not None:
            # periodic boundaries (Mesh.periodic_nodes / Deck.node_master):
            # node_master[slave] = master, every other node itself
            if mapping is not None:
                raise NotImplementedError("a periodic node map on an FE_Q_iso_Q1 level")
            nm = np.ascontiguousarray(node_master, dtype=np.int64)
            if nm.shape != (mesh.n_nodes,):
                raise GlsError("node_master: expected one entry per node")
            self._keep.append(nm)
            self.node_master = nm
            d.node_master = nm.ctypes.data
        h = C.c_void_p()
        _check(lib().gls_op_create(C.byref(d), C.byref(h)))
        self.h = h
        self.n_dofs = lib().gls_op_m(h)
        dims = (C.c_int * 3)()
        _check(lib().gls_op_brick_shape(h, dims))
        self.brick_shape = tuple(dims)  # what runs: (0, 0, 0) = per-cell kernel
        if node_constraints is not None:
            self.set_node_constraints(*node_constraints)

    def set_node_constraints(self, nodes, comp, coef):
        """No-normal-flux rows u[nodes[i]][comp[i]] = sum_e coef[i][e]
        u[nodes[i]][e] (Mesh.node_constraints / Deck.node_constraints;
        gls_op_set_node_constraints): vmult becomes C^T A C with identity rows
        on the eliminated components.  Empty arrays clear."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int64).ravel()
        comp = np.ascontiguousarray(comp, dtype=np.int32).ravel()
        coef = np.ascontiguousarray(coef, dtype=np.float64).reshape(-1)
        if len(comp) != len(nodes) or len(coef) != len(nodes) * self.dim:
            raise GlsError("set_node_constraints: expected nodes [n], comp [n], coef [n][dim]")
        _check(lib().gls_op_set_node_constraints(self.h, len(nodes), nodes.ctypes.data,
                                                 comp.ctypes.data, coef.ctypes.data, _stream()))
        self.node_constraint_rows = (nodes, comp, coef.reshape(-1, self.dim))

    @property
    def n_node_constraints(self):
        """(rows, colours of the diagonal's unit-vector applies)."""
        n, c = C.c_int64(), C.c_int()
        _check(lib().gls_op_n_node_constraints(self.h, C.byref(n), C.byref(c)))
        return n.value, c.value

    def distribute(self, vec, homogeneous=False):
        """AffineConstraints::distribute in place (gls_op_distribute):
        Dirichlet components take 0 (homogeneous) or the constraint values,
        eliminated components their rows' combination."""
        _check(lib().gls_op_distribute(self.h, _vptr(vec), 1 if homogeneous else 0, _stream()))
        return vec

    def extract_constant_modes(self):
        """NavierStokesOperator::extract_constant_modes (operator_ns.cc:
        175-193, DoFTools::extract_constant_modes over all dim+1 components):
        one boolean dof mask per component, node-major numbering (the AMG
        near-null space a Trilinos coarse solver takes)."""
        nc = self.dim + 1
        comp = np.arange(self.n_dofs) % nc
        return [comp == c for c in range(nc)]

    @property
    def n_outflow_faces(self):
        n, q = C.c_int64(), C.c_int()
        _check(lib().gls_op_n_outflow_faces(self.h, C.byref(n), C.byref(q)))
        return n.value, q.value

    def outflow_face_points(self):
        """[face][point][dim] face quadrature points (gls_op_outflow_face_points)."""
        n, q = self.n_outflow_faces
        x = np.empty((n, q, self.dim))
        _check(lib().gls_op_outflow_face_points(self.h, x.ctypes.data))
        return x

    def set_outflow_target(self, target, stream=None):
        """Nitsche target velocity at the face points, [face][point][dim]
        (face_target_velocity, operator_ns.cc:478-521)."""
        n, q = self.n_outflow_faces
        t = np.ascontiguousarray(target, dtype=np.float64)
        if t.size != n * q * self.dim:
            raise GlsError("set_outflow_target: expected [faces][points][dim]")
        _check(lib().gls_op_set_outflow_target(self.h, t.ctypes.data, stream))

    def element_matrices(self):
        """[cell][row i][col j] element matrices (gls_op_element_matrices;
        local dof = point * (dim+1) + component)."""
        nd = (self.degree + 1) ** self.dim * (self.dim + 1)
        out = np.empty((self.n_cells, nd, nd))
        _check(lib().gls_op_element_matrices(self.h, out.ctypes.data))
        return np.ascontiguousarray(out.transpose(0, 2, 1))

    def system_matrix(self):
        """OperatorBase::get_system_matrix as a scipy CSR matrix over the
        node-major dofs (gls_op_system_matrix)."""
        import scipy.sparse as sp
        nnz = C.c_int64()
        _check(lib().gls_op_system_matrix(self.h, C.byref(nnz), None, None, None))
        rp = np.empty(self.n_dofs + 1, dtype=np.int64)
        cols = np.empty(nnz.value, dtype=np.int64)
        vals = np.empty(nnz.value)
        _check(lib().gls_op_system_matrix(self.h, C.byref(nnz), rp.ctypes.data, cols.ctypes.data,
                                          vals.ctypes.data))
        return sp.csr_matrix((vals, cols, rp), shape=(self.n_dofs, self.n_dofs))

    def cell_permutation(self):
        """perm[internal cell] = caller cell (identity unless bricks were
        discovered)."""
        p = np.empty(self.n_cells, dtype=np.int64)
        _check(lib().gls_op_cell_permutation(self.h, p.ctypes.data))
        return p

    def sweep_stats(self):
        """(resident smoothing launches, slot waits that hit their spin
        bound) on this multigrid level (gls_op_sweep_stats)."""
        n, c = C.c_uint64(0), C.c_uint64(0)
        _check(lib().gls_op_sweep_stats(self.h, C.byref(n), C.byref(c)))
        return int(n.value), int(c.value)

    def set_sweep_spin_bound(self, polls):
        """Polls of a neighbour's slot before a resident sweep's wait gives
        up (gls_op_set_sweep_spin_bound; 0 forces the stall path: tests)."""
        _check(lib().gls_op_set_sweep_spin_bound(self.h, int(polls)))

    def __del__(self):
        try:
            if self.h:
                lib().gls_op_destroy(self.h)
                self.h = None
        except Exception:
            pass

    # --- OperatorBase-like API
    def m(self):
        return self.n_dofs

    def set_parameters(self, nu, c1=1.0, c2=1.0, theta=1.0, w0=0.0, dt=1.0, order=0,
                       increment_form=True, consider_time_derivative=False,
                       cell_wise_stabilization=False, deterministic=False):
        """deterministic: GLS_DETERMINISTIC (not a reference parameter) --
        bitwise reproducible results run to run (ordered lattice
        accumulation, colour-by-colour diagonal and restriction), slower"""
        flags = ((GLS_INCREMENT_FORM if increment_form else 0)
                 | (GLS_CONSIDER_TIME_DERIVATIVE if consider_time_derivative else 0)
                 | (GLS_CELL_WISE_STAB if cell_wise_stabilization else 0)
                 | (GLS_DETERMINISTIC if deterministic else 0))
        self.params = OpParams(nu, c1, c2, theta, w0, dt, order, flags)
        _check(lib().gls_op_set_parameters(self.h, C.byref(self.params)))

    def initialize_dof_vector(self):
        import torch
        return torch.zeros(self.n_dofs, dtype=self.dtype, device="cuda")

    def _dev(self, v):
        import torch
        if isinstance(v, np.ndarray):
            v = torch.from_numpy(v)
        return v.to(device="cuda", dtype=self.dtype).contiguous()

    def _arg(self, v):
        """A vector argument in the current layout: numpy (host layout) or a
        device tensor."""
        if getattr(self, "_memory", "device") == "host":
            return np.ascontiguousarray(v, dtype=np.float64 if self.prec == GLS_F64
                                        else np.float32)
        return self._dev(v)

    def set_linearization_point(self, vec):
        v = self._arg(vec)
        _check(lib().gls_op_set_linearization_point(self.h, _vptr(v), _stream()))

    def set_previous_solution(self, history, weights):
        hs = [self._arg(h) for h in history]
        ptrs = (C.c_void_p * len(hs))(*[_vptr(h).value for h in hs])
        w = np.ascontiguousarray(weights, dtype=np.float64)
        _check(lib().gls_op_set_previous_solution(self.h, C.cast(ptrs, C.c_void_p), len(hs),
                                                  w.ctypes.data, _stream()))
        self._hist_keep = hs

    def vmult(self, dst, src):
        _check(lib().gls_op_vmult(self.h, _vptr(dst), _vptr(src), _stream()))
        return dst

    def Tvmult(self, dst, src):
        """OperatorBase::Tvmult forwards to vmult (operator_base.cc:12-18)."""
        self.vmult(dst, src)

    def vmult_interface_down(self, dst, src):
        """OperatorBase::vmult_interface_down (operator_ns.cc:734-753): on a
        globally refined level (no refinement-edge dofs) the vmult."""
        _check(lib().gls_op_vmult_interface_down(self.h, _vptr(dst), _vptr(src), _stream()))
        return dst

    def vmult_interface_up(self, dst, src):
        """OperatorBase::vmult_interface_up (operator_ns.cc:755-787): dst = 0
        without refinement-edge dofs (has_edge_constrained_indices false)."""
        _check(lib().gls_op_vmult_interface_up(self.h, _vptr(dst), _vptr(src), _stream()))
        return dst

    def invalidate_system(self):
        """OperatorBase::invalidate_system (operator_ns.cc:229-232): the
        device system matrix is assembled again at its next use
        (gls_op_invalidate_system; system_matrix() assembles on every call)."""
        _check(lib().gls_op_invalidate_system(self.h))

    def set_matrix_based(self, on=True):
        """NavierStokesOperatorMatrixBased (operator_ns.cc:1525-1590, the
        deck's "use matrix free ns operator": false): vmult is the SpMV of the
        device system matrix (gls_op_set_matrix_based)."""
        _check(lib().gls_op_set_matrix_based(self.h, 1 if on else 0))

    def system_matrix_device_raw(self):
        """gls_op_system_matrix_device: (n, nnz, row_ptr, cols, vals), the
        last three the operator's own device addresses."""
        m = DeviceCSR()
        _check(lib().gls_op_system_matrix_device(self.h, C.byref(m), _stream()))
        return m.n, m.nnz, m.row_ptr, m.cols, m.vals

    def system_matrix_device(self):
        """The device system matrix as torch tensors (row_ptr int64, cols
        int32, vals float64): copies, valid after the next invalidation too."""
        import torch
        n, nnz, rp, ci, va = self.system_matrix_device_raw()
        out = tuple(torch.as_tensor(_DeviceArray(p, cnt, ts), device="cuda").clone()
                    for p, cnt, ts in ((rp, n + 1, "<i8"), (ci, nnz, "<i4"), (va, nnz, "<f8")))
        torch.cuda.synchronize()
        return out

    def get_constraints(self):
        """The homogeneous constraints the operator resolves
        (get_constraints, operator_ns.cc:157-160): per node the constrained
        component bits, node-major."""
        return np.asarray(self._keep[2])

    def vmult_init(self, dst, src):
        _check(lib().gls_op_vmult_init(self.h, _ptr(dst), _ptr(src), _stream()))

    def apply_identity_rows(self, dst, src):
        _check(lib().gls_op_apply_identity_rows(self.h, _ptr(dst), _ptr(src), _stream()))

    def vmult_cells(self, dst, src, begin, end):
        _check(lib().gls_op_vmult_cells(self.h, _ptr(dst), _ptr(src), int(begin), int(end),
                                        _stream()))

    def evaluate_residual(self, dst, src):
        """operator_ns.cc:648-682: distribute the inhomogeneous constraints
        on a copy of src, residual cell loop, set_zero, *= -1."""
        _check(lib().gls_op_evaluate_residual(self.h, _vptr(dst), _vptr(src), _stream()))
        return dst

    def evaluate_residual_plain(self, dst, src):
        """The same on src as it is (no distribute)."""
        _check(lib().gls_op_evaluate_residual_plain(self.h, _vptr(dst), _vptr(src), _stream()))
        return dst

    def evaluate_rhs(self, dst):
        """operator_ns.cc:622-646: residual of the zero vector with the
        inhomogeneous constraints distributed."""
        _check(lib().gls_op_evaluate_rhs(self.h, _vptr(dst), _stream()))
        return dst

    def set_constraint_values(self, values):
        """constraints_inhomogeneous (main.cc:879-891): a dof vector whose
        constrained components hold the Dirichlet values (None: all zero)."""
        if values is None:
            _check(lib().gls_op_set_constraint_values(self.h, None, _stream()))
            return
        v = self._dev(values)
        _check(lib().gls_op_set_constraint_values(self.h, _ptr(v), _stream()))
        self._inhom_keep = v

    def compute_inverse_diagonal(self, diag):
        _check(lib().gls_op_compute_inverse_diagonal(self.h, _vptr(diag), _stream()))
        return diag

    def compute_diagonal(self, diag):
        """Assembled (not inverted) diagonal: the rank-local half of a
        partitioned compute_inverse_diagonal."""
        _check(lib().gls_op_compute_diagonal(self.h, _ptr(diag), _stream()))
        return diag

    def invert_diagonal(self, diag):
        _check(lib().gls_op_invert_diagonal(self.h, _ptr(diag), _stream()))
        return diag

    def get_max_u(self, vec):
        """OperatorBase::get_max_u (operator_ns.cc:530-568): max |u(x_q)|."""
        out = C.c_double()
        _check(lib().gls_op_get_max_u(self.h, _vptr(vec), C.byref(out), _stream()))
        return out.value

    # --- SimulationCylinder::postprocess (simulation.cc:433-549)
    def set_force_faces(self, cells, face_no, n_q_1d=3):
        """The boundary faces of surface_force as (cells, face_no) (what
        glsmesh.boundary_faces returns; cells index this operator's cell
        list), QGauss(n_q_1d) per face direction (reference: 3); the geometry
        is the mesh's the operator was built on."""
        fc = np.ascontiguousarray(cells, dtype=np.int64)
        fn = np.ascontiguousarray(face_no, dtype=np.int32)
        if fc.shape != fn.shape or fc.ndim != 1:
            raise GlsError("set_force_faces: cells and face_no must be 1D and of one length")
        _check(lib().gls_op_set_force_faces(self.h, len(fc), fc.ctypes.data, fn.ctypes.data,
                                            self._keep[1].ctypes.data, int(n_q_1d)))
        self.n_force_faces = len(fc)

    def surface_force(self, vec):
        """Sum over the force faces of (-p I + 2 nu eps(u)) . n JxW, n the
        normal pointing into the cell (simulation.cc:487-495): ndarray [dim]."""
        out = np.zeros(self.dim)
        _check(lib().gls_op_surface_force(self.h, _vptr(vec), out.ctypes.data, _stream()))
        return out

    def surface_force_faces(self, vec):
        """The same per face, [n_faces][dim], in the order of set_force_faces."""
        out = np.zeros((getattr(self, "n_force_faces", 0), self.dim))
        _check(lib().gls_op_surface_force_faces(self.h, _vptr(vec), out.ctypes.data, _stream()))
        return out

    def set_probe_points(self, xyz):
        """Points [n_points][dim] of probe(); returns the number of cells
        found per point (0: the point is in no cell of this operator)."""
        x = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, self.dim)
        found = np.zeros(len(x), dtype=np.int64)
        _check(lib().gls_op_set_probe_points(self.h, len(x), x.ctypes.data,
                                             self._keep[1].ctypes.data, found.ctypes.data))
        self.n_probe_points = len(x)
        return found

    def probe(self, vec):
        """All dim+1 components at the probe points, averaged over the cells
        that contain a point (point_values<1>(avg), simulation.cc:537-538):
        ndarray [n_points][dim+1]."""
        out = np.zeros((getattr(self, "n_probe_points", 0), self.dim + 1))
        _check(lib().gls_op_probe(self.h, _vptr(vec), out.ctypes.data, _stream()))
        return out

    def set_vector_layout(self, memory="device", dof_map=None):
        """Caller vector layout (gls_op_set_vector_layout): memory "host"
        (numpy arrays, staged) or "device" (torch tensors); dof_map[i] = the
        node-major dof of caller dof i (deal.II numbering), or None."""
        m = np.ascontiguousarray(dof_map, dtype=np.int64) if dof_map is not None else None
        _check(lib().gls_op_set_vector_layout(self.h, GLS_MEM_HOST if memory == "host"
                                              else GLS_MEM_DEVICE,
                                              None if m is None else m.ctypes.data))
        self._map_keep = m
        self._memory = memory

    def download_tables(self):
        nq = (self.degree + 1) ** self.dim
        nf = 2 + 3 * self.dim + self.dim ** 2
        t = np.empty((self.n_cells, nq, nf))
        cw = np.empty((self.n_cells, 2))
        _check(lib().gls_op_download_tables(self.h, t.ctypes.data, cw.ctypes.data))
        return t, cw

    def upload_tables(self, tables, cellwise=None):
        t = np.ascontiguousarray(tables, dtype=np.float64)
        cw = None if cellwise is None else np.ascontiguousarray(cellwise, dtype=np.float64)
        _check(lib().gls_op_upload_tables(self.h, t.ctypes.data,
                                          None if cw is None else cw.ctypes.data))

    def geometry_counts(self):
        g, c = C.c_int64(), C.c_int64()
        _check(lib().gls_op_geometry_counts(self.h, C.byref(g), C.byref(c)))
        return g.value, c.value

    def vmult_bytes(self):
        return lib().gls_op_vmult_bytes(self.h)


def dist_unique_id():
    """128-byte RCCL unique id (one rank creates it, all ranks use it)."""
    b = (C.c_char * 128)()
    _check(lib().gls_dist_unique_id(C.cast(b, C.c_void_p)))
    return bytes(b)


class PartitionedOperator:
    """The rank-local half of a partitioned NavierStokesOperator: ghost
    import / compress(add) over RCCL (nccl_id given) or inside an in-process
    group of ranks on one device (nccl_id None, `group` = a member created
    before).  op: the rank-local NavierStokesOperator; recv blocks: per peer
    the [begin, begin + count) local ghost nodes it owns; send_nodes: per peer
    the owned local nodes that are ghosts there, in the peer's ghost order."""

    def __init__(self, op, rank, world, peers, send_nodes, recv_blocks, nccl_id=None,
                 group=None):
        self.op = op
        peers = [int(q) for q in peers]
        self._keep = [np.ascontiguousarray(peers, dtype=np.int32),
                      np.ascontiguousarray([len(send_nodes[q]) for q in peers], dtype=np.int64),
                      np.ascontiguousarray(np.concatenate([np.asarray(send_nodes[q], np.int64)
                                                           for q in peers])
                                           if peers else np.zeros(0), dtype=np.uint32),
                      np.ascontiguousarray([recv_blocks[q][0] for q in peers], dtype=np.int64),
                      np.ascontiguousarray([recv_blocks[q][1] for q in peers], dtype=np.int64)]
        k = self._keep
        idb = None
        if nccl_id is not None:
            idb = (C.c_char * 128).from_buffer_copy(bytes(nccl_id))
            self._keep.append(idb)
        d = DistDesc(rank, world, None if idb is None else C.cast(idb, C.c_void_p),
                     None if group is None else group.h, len(peers), k[0].ctypes.data,
                     k[1].ctypes.data, k[2].ctypes.data, k[3].ctypes.data, k[4].ctypes.data)
        h = C.c_void_p()
        _check(lib().gls_dist_create(op.h, C.byref(d), C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if self.h:
                lib().gls_dist_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def vmult(self, dst, src):
        _check(lib().gls_dist_vmult(self.h, _ptr(dst), _ptr(src), _stream()))
        return dst

    def update_ghost_values(self, vec):
        _check(lib().gls_dist_update_ghost_values(self.h, _ptr(vec), _stream()))

    def compress_add(self, vec):
        _check(lib().gls_dist_compress_add(self.h, _ptr(vec), _stream()))

    def get_max_u(self, vec):
        """get_max_u of the partitioned operator: ghost import, local max,
        RCCL all-reduce max (operator_ns.cc:540-567)."""
        out = C.c_double()
        _check(lib().gls_dist_get_max_u(self.h, _ptr(vec), C.byref(out), _stream()))
        return out.value

    def surface_force(self, vec):
        """surface_force of the partitioned operator: ghost import, the
        rank's own faces (op.set_force_faces), all-reduce sum
        (simulation.cc:509-510)."""
        out = np.zeros(self.op.dim)
        _check(lib().gls_dist_surface_force(self.h, _ptr(vec), out.ctypes.data, _stream()))
        return out

    def probe(self, vec):
        """probe of the partitioned operator (every rank sets the same
        points): value sums and cell counts all-reduced, then divided."""
        out = np.zeros((getattr(self.op, "n_probe_points", 0), self.op.dim + 1))
        _check(lib().gls_dist_probe(self.h, _ptr(vec), out.ctypes.data, _stream()))
        return out

    def interior_bricks(self):
        a, b = C.c_int64(), C.c_int64()
        _check(lib().gls_dist_interior_bricks(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    @staticmethod
    def vmult_group(members, dsts, srcs):
        n = len(members)
        hs = (C.c_void_p * n)(*[m.h.value for m in members])
        ds = (C.c_void_p * n)(*[d.data_ptr() for d in dsts])
        ss = (C.c_void_p * n)(*[s.data_ptr() for s in srcs])
        _check(lib().gls_dist_vmult_group(C.cast(hs, C.c_void_p), C.cast(ds, C.c_void_p),
                                          C.cast(ss, C.c_void_p), n, _stream()))
        return dsts


class DistMGDesc(C.Structure):
    _fields_ = [("mg", MGDesc), ("child", C.c_void_p), ("owned_global_nodes", C.c_void_p),
                ("n_global_nodes", C.c_void_p), ("coarse_global", C.c_void_p),
                ("coarse_local_global", C.c_void_p), ("n_redundant_levels", C.c_int),
                ("redundant_ops", C.c_void_p), ("redundant_child", C.c_void_p)]


def _handles(objs):
    n = len(objs)
    return (C.c_void_p * n)(*[o.h.value for o in objs]), n


def _ptrs(ts):
    return (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


class PartitionedMultigrid:
    """The rank-local handle of the native partitioned multigrid
    (gls_dist_mg_*, csrc/dist_mg.hip): PreconditionerGMG over partitioned
    level operators (PartitionedOperator handles of one rank, coarse to
    fine).  child[l] (l >= 1): rank-local child lattice with the global-first
    NOT_OWNER bits; owned_global_nodes[l]: global ids of the owned nodes;
    coarse_global (direct coarse solve): a NavierStokesOperator on the whole
    coarse mesh with coarse_l2g (level-0 local node -> global node).
    Agglomeration (glsDistMGDesc n_redundant_levels): redundant_ops, the
    global NavierStokesOperators of the levels below level 0 (coarsest
    first), and redundant_child[l] (l = 1 .. len(redundant_ops); entry 0
    unused) the global child lattices up to coarse_global's mesh: those
    levels run single-domain on every rank.  The team methods take every
    handle this process drives: [self] for an RCCL rank, all members of an
    in-process group in rank order (tests)."""

    def __init__(self, levels, child, owned_global_nodes, n_global_nodes,
                 smoothing_n_iterations=5, smoothing_eig_n_iterations=20, smoothing_range=20.0,
                 coarse_n_iterations=10, outer_precision="f64", compute_evs_n_levels=0,
                 coarse_global=None, coarse_l2g=None, redundant_ops=None, redundant_child=None):
        n = len(levels)
        outer = GLS_F64 if outer_precision in ("f64", GLS_F64) else GLS_F32
        md = MGDesc(n, smoothing_n_iterations, smoothing_eig_n_iterations, smoothing_range,
                    coarse_n_iterations, outer, compute_evs_n_levels, 0, 1e-4, 10000)
        self._keep = [None] + [np.ascontiguousarray(c, dtype=np.uint32) for c in child[1:]]
        self._own = [np.ascontiguousarray(g, dtype=np.int64) for g in owned_global_nodes]
        self._ng = np.ascontiguousarray(n_global_nodes, dtype=np.int64)
        chp = (C.c_void_p * n)(*([None] + [c.ctypes.data for c in self._keep[1:]]))
        ogp = (C.c_void_p * n)(*[g.ctypes.data for g in self._own])
        self._l2g = None if coarse_l2g is None else np.ascontiguousarray(coarse_l2g, np.int64)
        self.coarse_global = coarse_global
        nr = len(redundant_ops) if redundant_ops else 0
        self.redundant_ops = list(redundant_ops or [])
        self._rch = [None] + [np.ascontiguousarray(c, dtype=np.uint32)
                              for c in (redundant_child or [None])[1:]]
        rop = (C.c_void_p * max(nr, 1))(*[o.h.value for o in self.redundant_ops])
        rch = (C.c_void_p * (nr + 1))(*([None] + [c.ctypes.data for c in self._rch[1:]]))
        d = DistMGDesc(md, C.cast(chp, C.c_void_p), C.cast(ogp, C.c_void_p),
                       self._ng.ctypes.data,
                       None if coarse_global is None else coarse_global.h,
                       None if self._l2g is None else self._l2g.ctypes.data, nr,
                       C.cast(rop, C.c_void_p) if nr else None,
                       C.cast(rch, C.c_void_p) if nr else None)
        lv = (C.c_void_p * n)(*[L.h.value for L in levels])
        h = C.c_void_p()
        _check(lib().gls_dist_mg_create(C.byref(d), C.cast(lv, C.c_void_p), C.byref(h)))
        self.h = h
        self._ptr_keep = (chp, ogp, lv, rop, rch)
        self.levels = levels

    def __del__(self):
        try:
            if self.h:
                lib().gls_dist_mg_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def relaxation(self, level):
        w, lam = C.c_double(), C.c_double()
        _check(lib().gls_dist_mg_get_relaxation(self.h, level, C.byref(w), C.byref(lam)))
        return w.value, lam.value

    @staticmethod
    def set_linearization_point(team, u_fine, hist_fine=None, weights=None):
        hs, n = _handles(team)
        us = _ptrs(u_fine)
        nh = 0 if not hist_fine else len(hist_fine[0])
        hrows = [_ptrs(h) for h in hist_fine] if nh else []
        hp = (C.c_void_p * n)(*[C.cast(r, C.c_void_p).value for r in hrows]) if nh else None
        w = None
        if weights is not None:
            w = np.ascontiguousarray(weights, dtype=np.float64)
        _check(lib().gls_dist_mg_set_linearization_point(
            C.cast(hs, C.c_void_p), n, C.cast(us, C.c_void_p),
            None if hp is None else C.cast(hp, C.c_void_p), nh,
            None if w is None else w.ctypes.data, _stream()))

    @staticmethod
    def setup(team):
        hs, n = _handles(team)
        _check(lib().gls_dist_mg_setup(C.cast(hs, C.c_void_p), n, _stream()))

    @staticmethod
    def vcycle(team, dsts, srcs):
        hs, n = _handles(team)
        _check(lib().gls_dist_mg_vcycle(C.cast(hs, C.c_void_p), n, C.cast(_ptrs(dsts), C.c_void_p),
                                        C.cast(_ptrs(srcs), C.c_void_p), _stream()))
        return dsts


def dist_gmres_solve(ops, mgs, xs, bs, n_max_iterations=10000, absolute_tolerance=1e-12,
                     relative_tolerance=1e-8, max_n_tmp_vectors=30):
    """gls_dist_gmres_solve: LinearSolverGMRES::solve on rank-local vectors of
    the FP64 partitioned operator (PartitionedOperator handles of the team),
    preconditioned by the native partitioned multigrid (or identity, mgs
    None).  Returns the result dict; raises GlsError on no convergence."""
    hs, n = _handles(ops)
    ms = None if mgs is None else _handles(mgs)[0]
    desc = GMRESDesc(max_n_tmp_vectors, n_max_iterations, absolute_tolerance, relative_tolerance)
    res = GMRESResult()
    rc = lib().gls_dist_gmres_solve(C.cast(hs, C.c_void_p),
                                    None if ms is None else C.cast(ms, C.c_void_p), n,
                                    C.byref(desc), C.cast(_ptrs(xs), C.c_void_p),
                                    C.cast(_ptrs(bs), C.c_void_p), C.byref(res), _stream())
    out = {f: getattr(res, f) for f, _ in GMRESResult._fields_}
    _check(rc)
    return out


class AMG:
    """TrilinosWrappers::PreconditionAMG over the C-ABI (gls_amg_*): built
    from a scipy CSR matrix (initialize), vmult = one V-cycle on device FP64
    vectors.  The substitute for Trilinos ML (csrc/amg.hip).  smoother_type
    "ILU" / coarse_type "ILU" (the reference's non-default parameters,
    multigrid.cc:403-413) replace the Chebyshev smoother / the dense coarsest
    solve by ILU(ilu_fill) steps; the defaults give the Chebyshev / direct
    form."""

    def __init__(self, matrix, smoother_type="Chebyshev", coarse_type="direct", ilu_fill=1,
                 ilu_atol=1e-6, ilu_rtol=1.0, **params):
        import torch
        if not torch.cuda.is_available():
            raise GlsError("AMG needs a GPU (no CPU fallback by design)")
        if smoother_type not in ("Chebyshev", "ILU"):
            raise ValueError(f"smoother_type: 'Chebyshev' or 'ILU', not {smoother_type!r}")
        if coarse_type not in ("direct", "ILU"):
            raise ValueError(f"coarse_type: 'direct' or 'ILU', not {coarse_type!r}")
        A = matrix.tocsr()
        A.sort_indices()
        rp = np.ascontiguousarray(A.indptr, dtype=np.int64)
        ci = np.ascontiguousarray(A.indices, dtype=np.int64)
        va = np.ascontiguousarray(A.data, dtype=np.float64)
        self.prm = amg_params(**params)
        h = C.c_void_p()
        if smoother_type == "ILU" or coarse_type == "ILU":
            self.ilu_prm = amg_ilu_params(smoother_type == "ILU", coarse_type == "ILU", ilu_fill,
                                          ilu_atol, ilu_rtol)
            _check(lib().gls_amg_create_ilu(A.shape[0], rp.ctypes.data, ci.ctypes.data,
                                            va.ctypes.data, C.byref(self.prm),
                                            C.byref(self.ilu_prm), C.byref(h)))
        else:
            _check(lib().gls_amg_create(A.shape[0], rp.ctypes.data, ci.ctypes.data,
                                        va.ctypes.data, C.byref(self.prm), C.byref(h)))
        self.h = h
        self.n = A.shape[0]

    @staticmethod
    def _info_of(h):
        nl = C.c_int()
        _check(lib().gls_amg_info(h, C.byref(nl), None, None, None))
        sizes = np.zeros(nl.value, dtype=np.int64)
        nnz = np.zeros(nl.value, dtype=np.int64)
        lam = np.zeros(nl.value)
        _check(lib().gls_amg_info(h, C.byref(nl), sizes.ctypes.data, nnz.ctypes.data,
                                  lam.ctypes.data))
        return {"levels": nl.value, "sizes": sizes.tolist(), "nnz": nnz.tolist(),
                "lambda": lam.tolist()}

    def info(self):
        return self._info_of(self.h)

    def level_matrix(self, level, which="A"):
        """the device hierarchy's A / P / R of a level as scipy CSR"""
        import scipy.sparse as sp
        w = {"A": 0, "P": 1, "R": 2}[which]
        n, nnz = C.c_int64(), C.c_int64()
        _check(lib().gls_amg_level_matrix(self.h, level, w, C.byref(n), C.byref(nnz), None, None,
                                          None))
        rp = np.zeros(n.value + 1, dtype=np.int32)
        ci = np.zeros(nnz.value, dtype=np.int32)
        va = np.zeros(nnz.value)
        _check(lib().gls_amg_level_matrix(self.h, level, w, C.byref(n), C.byref(nnz),
                                          rp.ctypes.data, ci.ctypes.data, va.ctypes.data))
        m = int(ci.max()) + 1 if nnz.value else 0
        return sp.csr_matrix((va, ci, rp), shape=(n.value, max(m, 1)))

    def vmult(self, dst, src):
        _check(lib().gls_amg_vmult(self.h, _vptr(dst), _vptr(src), _stream()))
        return dst

    def __del__(self):
        try:
            if self.h:
                lib().gls_amg_destroy(self.h)
                self.h = None
        except Exception:
            pass


def _csr_arrays(matrix):
    """(n, row_ptr, cols, vals) of a scipy matrix as the C ABI takes them
    (int64 indices, columns ascending per row)"""
    A = matrix.tocsr()
    if not A.has_sorted_indices:
        A = A.sorted_indices()
    return (A.shape[0], np.ascontiguousarray(A.indptr, dtype=np.int64),
            np.ascontiguousarray(A.indices, dtype=np.int64),
            np.ascontiguousarray(A.data, dtype=np.float64))


def _ilu_info_of(h):
    i = ILUInfo()
    _check(lib().gls_ilu_info(h, C.byref(i)))
    return {k: getattr(i, k) for k, _ in ILUInfo._fields_}


class ILU:
    """TrilinosWrappers::PreconditionILU over the C-ABI (gls_ilu_*): ILU(k)
    of a scipy CSR matrix in its own row order, factorised on the host after
    Ifpack's diagonal modification (atol, rtol); vmult = U^-1 L^-1 on device
    FP64 vectors (csrc/ilu.hip).  The defaults are the reference's
    PreconditionerILU (preconditioner.cc:5-28).  GLS_ILU_CHAIN / GLS_ILU_GROUP
    / GLS_ILU_NARROW are read when the object is created.

    The numeric phase also runs on the device (csrc/ilu_factor.hip, bitwise
    equal to the host's): refactor_device on a factor made either way,
    from_operator / refactor_from_operator from the operator's device system
    matrix; GLS_ILU_FACTOR_CHAIN / GLS_ILU_FACTOR_NARROW are read with the
    others."""

    def __init__(self, matrix, fill_level=0, atol=1e-12, rtol=1.0):
        import torch
        if not torch.cuda.is_available():
            raise GlsError("ILU needs a GPU (no CPU fallback by design)")
        n, rp, ci, va = _csr_arrays(matrix)
        self.prm = ILUParams(int(fill_level), float(atol), float(rtol))
        h = C.c_void_p()
        _check(lib().gls_ilu_create(n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data,
                                    C.byref(self.prm), C.byref(h)))
        self.h, self.n, self.nnz = h, n, va.shape[0]

    def refactor(self, matrix_or_values):
        """new values on the same pattern: a scipy matrix or its data array"""
        va = (_csr_arrays(matrix_or_values)[3] if hasattr(matrix_or_values, "tocsr")
              else np.ascontiguousarray(matrix_or_values, dtype=np.float64))
        if va.shape[0] != self.nnz:
            raise GlsError(f"ILU.refactor: {va.shape[0]} values for a pattern of {self.nnz}")
        _check(lib().gls_ilu_refactor(self.h, va.ctypes.data))

    @classmethod
    def from_operator(cls, op, fill_level=0, atol=1e-12, rtol=1.0):
        """gls_ilu_create_device on the operator's device system matrix
        (assembled on the current stream if it is not valid): the pattern goes
        to the host once for the symbolic phase, the values stay on the device"""
        self = cls.__new__(cls)
        self.h = None
        self.prm = ILUParams(int(fill_level), float(atol), float(rtol))
        n, nnz, rp, ci, va = op.system_matrix_device_raw()
        m = DeviceCSR(n, nnz, rp, ci, va)
        h = C.c_void_p()
        _check(lib().gls_ilu_create_device(C.byref(m), C.byref(self.prm), _stream(), C.byref(h)))
        self.h, self.n, self.nnz = h, n, nnz
        return self

    def refactor_from_operator(self, op):
        """gls_ilu_refactor_device with the operator's device system matrix at
        its current state (the pattern this factor was made from)"""
        n, nnz, _, _, va = op.system_matrix_device_raw()
        if n != self.n or nnz != self.nnz:
            raise GlsError(f"ILU.refactor_from_operator: a matrix of {n} rows and {nnz} entries "
                           f"for a pattern of {self.n} and {self.nnz}")
        _check(lib().gls_ilu_refactor_device(self.h, C.c_void_p(va), _stream()))

    def refactor_device(self, values):
        """new values on the same pattern from a float64 CUDA tensor (the
        order of the matrix's data array); the factorisation runs on the
        device, on the current stream"""
        import torch
        if not (isinstance(values, torch.Tensor) and values.is_cuda
                and values.dtype == torch.float64):
            raise GlsError("ILU.refactor_device: values must be a float64 CUDA tensor")
        if values.dim() != 1 or values.shape[0] != self.nnz:
            raise GlsError(f"ILU.refactor_device: {tuple(values.shape)} values for a pattern "
                           f"of {self.nnz}")
        values = values.contiguous()
        _check(lib().gls_ilu_refactor_device(self.h, _ptr(values), _stream()))

    def factor_info(self):
        """glsILUFactorInfo as a dict: levels, launches, chains, narrow, group,
        rows, chain, device (the last factorisation ran there), max_row,
        max_row_limit, factor_ms"""
        i = ILUFactorInfo()
        _check(lib().gls_ilu_factor_info(self.h, C.byref(i)))
        return {k: getattr(i, k) for k, _ in ILUFactorInfo._fields_}

    def vmult(self, dst, src):
        _check(lib().gls_ilu_vmult(self.h, _vptr(dst), _vptr(src), _stream()))
        return dst

    def info(self):
        return _ilu_info_of(self.h)

    def factors(self):
        """(L, U) as scipy CSR in the original row order: L strictly lower
        (unit diagonal implied), U with the pivots"""
        import scipy.sparse as sp
        out = []
        for which in (0, 1):
            nnz = C.c_int64()
            _check(lib().gls_ilu_factors(self.h, which, C.byref(nnz), None, None, None))
            rp = np.zeros(self.n + 1, dtype=np.int64)
            ci = np.zeros(nnz.value, dtype=np.int64)
            va = np.zeros(nnz.value)
            _check(lib().gls_ilu_factors(self.h, which, C.byref(nnz), rp.ctypes.data,
                                         ci.ctypes.data, va.ctypes.data))
            out.append(sp.csr_matrix((va, ci, rp), shape=(self.n, self.n)))
        return tuple(out)

    def __del__(self):
        try:
            if self.h:
                lib().gls_ilu_destroy(self.h)
                self.h = None
        except Exception:
            pass


def ilu_host_factor(matrix, fill_level=0, atol=1e-12, rtol=1.0, solve=None):
    """gls_ilu_host_factor (host only, no GPU): dict with L, U (scipy CSR as
    ILU.factors), level_l / level_u (level of each row), order_l / order_u
    (row at each scheduled position), launch_l / launch_u (rows of first
    position, end position, first level, end level, chain flag), the counts,
    and with `solve` the host solve U^-1 L^-1 solve over the schedule."""
    import scipy.sparse as sp
    n, rp, ci, va = _csr_arrays(matrix)
    prm = ILUParams(int(fill_level), float(atol), float(rtol))
    f = ILUHostFactor()
    args = (n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, C.byref(prm), C.byref(f))
    _check(lib().gls_ilu_host_factor(*args))
    a = {"l_row_ptr": np.zeros(n + 1, np.int64), "l_cols": np.zeros(f.nnz_l, np.int64),
         "l_vals": np.zeros(f.nnz_l), "u_row_ptr": np.zeros(n + 1, np.int64),
         "u_cols": np.zeros(f.nnz_u, np.int64), "u_vals": np.zeros(f.nnz_u),
         "row_level_l": np.zeros(n, np.int32), "row_level_u": np.zeros(n, np.int32),
         "order_l": np.zeros(n, np.int32), "order_u": np.zeros(n, np.int32),
         "launch_l": np.zeros((f.launches_l, 5), np.int32),
         "launch_u": np.zeros((f.launches_u, 5), np.int32)}
    if solve is not None:
        a["solve_src"] = np.ascontiguousarray(solve, dtype=np.float64)
        a["solve_dst"] = np.zeros(n)
    for k, v in a.items():
        setattr(f, k, v.ctypes.data)
    _check(lib().gls_ilu_host_factor(*args))
    out = {k: getattr(f, k) for k in ("n", "nnz_l", "nnz_u", "levels_l", "levels_u",
                                      "launches_l", "launches_u", "group", "narrow", "chain",
                                      "min_pivot")}
    out["L"] = sp.csr_matrix((a["l_vals"], a["l_cols"], a["l_row_ptr"]), shape=(n, n))
    out["U"] = sp.csr_matrix((a["u_vals"], a["u_cols"], a["u_row_ptr"]), shape=(n, n))
    for k in ("order_l", "order_u", "launch_l", "launch_u"):
        out[k] = a[k]
    out["level_l"], out["level_u"] = a["row_level_l"], a["row_level_u"]
    if solve is not None:
        out["solve"] = a["solve_dst"]
    return out


def ilu_factor_host(matrix, fill_level=0, atol=1e-12, rtol=1.0):
    """gls_ilu_factor_host (host only, no GPU): the emulation of the device
    factorisation.  dict with L, U (as ilu_host_factor, bitwise equal to it),
    level / order of L's schedule, launch (rows of first position, end
    position, first level, end level, chain flag) and the counts."""
    import scipy.sparse as sp
    n, rp, ci, va = _csr_arrays(matrix)
    prm = ILUParams(int(fill_level), float(atol), float(rtol))
    f = ILUFactorHost()
    args = (n, rp.ctypes.data, ci.ctypes.data, va.ctypes.data, C.byref(prm), C.byref(f))
    _check(lib().gls_ilu_factor_host(*args))
    a = {"l_row_ptr": np.zeros(n + 1, np.int64), "l_cols": np.zeros(f.nnz_l, np.int64),
         "l_vals": np.zeros(f.nnz_l), "u_row_ptr": np.zeros(n + 1, np.int64),
         "u_cols": np.zeros(f.nnz_u, np.int64), "u_vals": np.zeros(f.nnz_u),
         "row_level": np.zeros(n, np.int32), "order": np.zeros(n, np.int32),
         "launch": np.zeros((f.launches, 5), np.int32)}
    for k, v in a.items():
        setattr(f, k, v.ctypes.data)
    _check(lib().gls_ilu_factor_host(*args))
    out = {k: getattr(f, k) for k in ("n", "nnz_l", "nnz_u", "max_row", "levels", "launches",
                                      "chains", "narrow", "group", "rows", "chain", "min_pivot")}
    out["L"] = sp.csr_matrix((a["l_vals"], a["l_cols"], a["l_row_ptr"]), shape=(n, n))
    out["U"] = sp.csr_matrix((a["u_vals"], a["u_cols"], a["u_row_ptr"]), shape=(n, n))
    out["level"], out["order"], out["launch"] = a["row_level"], a["order"], a["launch"]
    return out


class NdPlan:
    """The nested-dissection plan of the "nd" direct coarse solver on its own
    (host only, no GPU): the elimination tree over the cells of a cell ->
    node table, node_dofs[n] dofs of mesh node n taking part (plan dofs are
    numbered node by node).  nodes[t]: dict of parent, child, level, own (I),
    boundary (B), map (position of each B entry in the parent's I then B) and
    a leaf's cells; node 0 is the root."""

    def __init__(self, cell_nodes, node_dofs, max_leaf_cells):
        cn = np.ascontiguousarray(cell_nodes, dtype=np.uint32)
        nd = np.ascontiguousarray(node_dofs, dtype=np.int32)
        h = C.c_void_p()
        _check(lib().gls_nd_plan_create(cn.ctypes.data, cn.shape[0], cn.shape[1], nd.shape[0],
                                        nd.ctypes.data, int(max_leaf_cells), C.byref(h)))
        try:
            i = NdPlanInfo()
            _check(lib().gls_nd_plan_info(h, C.byref(i)))
            self.info = {"n_dofs": i.n_dofs, "tree_nodes": i.n_tree_nodes, "depth": i.depth,
                         "sum_own": i.sum_own, "stored_entries": i.stored_entries,
                         "max_own": i.max_own, "max_boundary": i.max_boundary}
            self.nodes = []
            for t in range(i.n_tree_nodes):
                n = NdPlanNode()
                _check(lib().gls_nd_plan_node(h, t, C.byref(n)))

                def arr(p, k):
                    return np.array(p[:k], dtype=np.int32)
                self.nodes.append({"parent": n.parent, "child": (n.child[0], n.child[1]),
                                   "level": n.level, "own": arr(n.own, n.n_own),
                                   "boundary": arr(n.boundary, n.n_boundary),
                                   "map": arr(n.map, n.n_boundary),
                                   "cells": arr(n.cells, n.n_cells)})
        finally:
            lib().gls_nd_plan_destroy(h)


class Multigrid:
    """PreconditionerGMG (multigrid.h:61-141) over the C-ABI: level operators
    (MGNumber = float by default), damped-Jacobi relaxation smoother with a
    power-iteration relaxation factor, MGTwoLevelTransfer, V-cycle."""

    def __init__(self, level_ops, child_lattices, smoothing_n_iterations=5,
                 smoothing_eig_n_iterations=20, smoothing_range=20.0, coarse_n_iterations=20,
                 outer_precision="f64", compute_evs_n_levels=0, coarse_iterate=False,
                 coarse_reltol=1e-4, coarse_maxiter=10000, coarse_amg=None,
                 coarse_direct="dense", coarse_leaf_cells=None, coarse_ilu=None,
                 coarse_amg_ilu=None):
        if coarse_direct not in ("dense", "nd"):
            raise ValueError(f"coarse_direct: 'dense' or 'nd', not {coarse_direct!r}")
        self.ops = list(level_ops)
        self._child = [None] + [np.ascontiguousarray(c, dtype=np.uint32)
                                for c in child_lattices]
        n = len(self.ops)
        arr = (C.c_void_p * n)(*[op.h.value for op in self.ops])
        ch = (C.c_void_p * n)(*[0 if c is None else c.ctypes.data for c in self._child])
        outer = GLS_F64 if outer_precision in ("f64", GLS_F64) else GLS_F32
        self.desc = MGDesc(n, smoothing_n_iterations, smoothing_eig_n_iterations,
                           smoothing_range, coarse_n_iterations, outer, compute_evs_n_levels,
                           int(bool(coarse_iterate)), coarse_reltol, coarse_maxiter)
        if coarse_amg is not None:
            # "gmg coarse grid solver": "AMG": a dict of amg_params() keywords
            # or an AMGParams
            self.desc.coarse_amg = 1
            self.desc.amg = (coarse_amg if isinstance(coarse_amg, AMGParams)
                             else amg_params(**coarse_amg))
        self.outer_dtype = None
        h = C.c_void_p()
        _check(lib().gls_mg_create(C.byref(self.desc), C.cast(arr, C.c_void_p),
                                   C.cast(ch, C.c_void_p), C.byref(h)))
        self.h = h
        if coarse_direct != "dense" or coarse_leaf_cells is not None:
            # the form of the direct coarse solver (coarse_n_iterations < 0):
            # "nd" = nested dissection over the coarse cells, coarse_leaf_cells
            # cells per leaf of its tree (None: the library's default)
            _check(lib().gls_mg_set_coarse_direct(
                self.h, GLS_COARSE_ND if coarse_direct == "nd" else GLS_COARSE_DENSE,
                int(coarse_leaf_cells or 0)))
        if coarse_ilu is not None:
            # "gmg coarse grid solver": "ILU": a dict of ilu_params() keywords
            # or an ILUParams; the dict's device=True also turns on
            # gls_mg_set_coarse_ilu_device (assembly and factorisation on the
            # device)
            device = False
            if not isinstance(coarse_ilu, ILUParams):
                coarse_ilu = dict(coarse_ilu)
                device = bool(coarse_ilu.pop("device", False))
                coarse_ilu = ilu_params(**coarse_ilu)
            self._coarse_ilu = coarse_ilu
            _check(lib().gls_mg_set_coarse_ilu(self.h, C.byref(self._coarse_ilu)))
            if device:
                _check(lib().gls_mg_set_coarse_ilu_device(self.h, 1))
        if coarse_amg_ilu is not None:
            # the coarse AMG's ILU smoother / coarsest solve: a dict of
            # amg_ilu_params() keywords or an AMGIluParams
            self._coarse_amg_ilu = (coarse_amg_ilu if isinstance(coarse_amg_ilu, AMGIluParams)
                                    else amg_ilu_params(**coarse_amg_ilu))
            _check(lib().gls_mg_set_coarse_amg_ilu(self.h, C.byref(self._coarse_amg_ilu)))

    def coarse_ilu(self):
        """(ILU info dict, setup ms) of the coarse ILU (coarse_ilu given), or
        None before setup."""
        h, ms = C.c_void_p(), C.c_double()
        _check(lib().gls_mg_coarse_ilu(self.h, C.byref(h), C.byref(ms)))
        if not h.value:
            return None
        return _ilu_info_of(h), ms.value

    def set_coarse_direct(self, coarse_direct, coarse_leaf_cells=None):
        """The direct coarse solver's form ("dense" | "nd"), before setup()."""
        _check(lib().gls_mg_set_coarse_direct(
            self.h, GLS_COARSE_ND if coarse_direct == "nd" else GLS_COARSE_DENSE,
            int(coarse_leaf_cells or 0)))

    def coarse_direct_info(self):
        """The direct coarse solver after the last setup(): method ("dense" |
        "nd": the one that is live, "dense" after a fallback), requested, nf,
        tree_nodes, depth, max_own, max_boundary, stored_entries,
        stored_bytes, and the wall ms of the last setup (plan_ms: 0 when the
        plan was reused; factor_ms: fronts + factorisation; narrow_ms: the
        stored copies)."""
        i = CoarseDirectInfo()
        _check(lib().gls_mg_coarse_direct_info(self.h, C.byref(i)))
        names = {GLS_COARSE_DENSE: "dense", GLS_COARSE_ND: "nd"}
        return {"method": names[i.method], "requested": names[i.requested],
                "max_leaf_cells": i.max_leaf_cells, "nf": i.n_free, "tree_nodes": i.tree_nodes,
                "depth": i.depth, "max_own": i.max_own, "max_boundary": i.max_boundary,
                "stored_entries": i.stored_entries, "stored_bytes": i.stored_bytes,
                "plan_ms": i.plan_ms, "factor_ms": i.factor_ms, "narrow_ms": i.narrow_ms}

    def __del__(self):
        try:
            if self.h:
                lib().gls_mg_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def setup(self):
        _check(lib().gls_mg_setup(self.h, _stream()))

    def coarse_statistics(self):
        """(GMRES iterations, converged) of the last coarse solve
        (coarse_iterate=True)."""
        it, cv = C.c_int(), C.c_int()
        _check(lib().gls_mg_coarse_statistics(self.h, C.byref(it), C.byref(cv)))
        return it.value, bool(cv.value)

    def coarse_setup_times(self):
        """{assembly_ms, getrf_ms, inverse_ms, colors} of the last dense-coarse
        setup (coarse_n_iterations=-1); inverse_ms: the inverse from the LU
        factors (trtri + trsm by default, GLS_COARSE_REFERENCE=getrs|getri)."""
        ms = (C.c_double * 3)()
        nc = C.c_int()
        _check(lib().gls_mg_coarse_setup_times(self.h, ms, C.byref(nc)))
        return {"assembly_ms": ms[0], "getrf_ms": ms[1], "inverse_ms": ms[2],
                "colors": nc.value}

    def coarse_amg(self):
        """(AMG info dict, setup ms) of the coarse AMG (coarse_amg given), or
        None before setup."""
        h, ms = C.c_void_p(), C.c_double()
        _check(lib().gls_mg_coarse_amg(self.h, C.byref(h), C.byref(ms)))
        if not h.value:
            return None
        return AMG._info_of(h), ms.value

    def relaxation(self, level):
        w, lam = C.c_double(), C.c_double()
        _check(lib().gls_mg_get_relaxation(self.h, level, C.byref(w), C.byref(lam)))
        return w.value, lam.value

    def vcycle(self, dst, src):
        _check(lib().gls_mg_vcycle(self.h, _vptr(dst), _vptr(src), _stream()))
        return dst

    def set_vector_layout(self, memory="device", dof_map=None):
        m = np.ascontiguousarray(dof_map, dtype=np.int64) if dof_map is not None else None
        _check(lib().gls_mg_set_vector_layout(self.h, GLS_MEM_HOST if memory == "host"
                                              else GLS_MEM_DEVICE,
                                              None if m is None else m.ctypes.data))
        self._map_keep = m

    def prolongate_add(self, level, dst_fine, src_coarse):
        _check(lib().gls_mg_prolongate_add(self.h, level, _ptr(dst_fine), _ptr(src_coarse),
                                           _stream()))

    def restrict_add(self, level, dst_coarse, src_fine):
        _check(lib().gls_mg_restrict_add(self.h, level, _ptr(dst_coarse), _ptr(src_fine),
                                         _stream()))

    def interpolate(self, level, dst_coarse, src_fine):
        _check(lib().gls_mg_interpolate(self.h, level, _ptr(dst_coarse), _ptr(src_fine),
                                        _stream()))

    def relax(self, level, x, b, ax, inv_diag, omega, zero_start):
        """x = omega d b (zero_start) or x += omega d (b - ax): one damped
        Jacobi update (the distributed smoother's elementwise half)."""
        _check(lib().gls_mg_relax(self.h, level, _ptr(x), _ptr(b),
                                  None if ax is None else _ptr(ax), _ptr(inv_diag),
                                  float(omega), int(zero_start), _stream()))

    def smooth(self, level, x, b, zero_initial_guess=True):
        _check(lib().gls_mg_smooth(self.h, level, _ptr(x), _ptr(b), int(zero_initial_guess),
                                   _stream()))


def build_gmg(meshes, cmasks, params, u_star_fine, history_fine=None, weights=None,
              precision="f32", coarse_iso_q1=False, outflow=None, node_constraints=None,
              node_master=None, **mg_kwargs):
    """Level operators + transfers for a mesh hierarchy (coarse -> fine), the
    linearization point / history interpolated down level by level
    (interpolate_to_mg, main.cc:772-803, 815-832).  coarse_iso_q1: the
    coarsest level with FE_Q_iso_Q1 (glsmesh.IsoQ1Mesh, main.cc:436-446).
    outflow: None, or (kind, boundary id): every level operator gets its
    mesh's outflow faces (the level operators take the outflow sets too,
    main.cc:520-527).  node_constraints: None, or per level (nodes, comp,
    coef) or None (Deck.node_constraints of the level's mesh).  node_master:
    None, or per level the periodic node map or None (Deck.node_master of the
    level's mesh); the child lattices stay the meshes' own, gls_mg_create maps
    them.  Returns (mg, level_ops)."""
    import torch
    if coarse_iso_q1:
        import glsmesh
        meshes = [glsmesh.IsoQ1Mesh(meshes[0])] + list(meshes[1:])
    ops = []
    if node_constraints is None:
        node_constraints = [None] * len(meshes)
    if coarse_iso_q1 and node_constraints[0] is not None:
        raise GlsError("build_gmg: node constraints on an FE_Q_iso_Q1 level are not supported")
    if node_master is None:
        node_master = [None] * len(meshes)
    if coarse_iso_q1 and any(nm is not None for nm in node_master):
        raise NotImplementedError("build_gmg: a periodic node map with an FE_Q_iso_Q1 level is "
                                  "not supported")
    for m, cm, rows, nm in zip(meshes, cmasks, node_constraints, node_master):
        of = None
        if outflow is not None:
            import glsmesh
            fc, fn = glsmesh.boundary_faces(m, outflow[1])
            of = (fc, fn, outflow[0])
        op = NavierStokesOperator(m, cm, precision, outflow=of, node_constraints=rows,
                                  node_master=nm)
        op.set_parameters(**params)
        ops.append(op)
    child = [meshes[l - 1].child_lattice(meshes[l]) for l in range(1, len(meshes))]
    mg = Multigrid(ops, child, **mg_kwargs)
    vecs = [ops[-1]._dev(u_star_fine)]
    hists = [[ops[-1]._dev(h) for h in history_fine]] if history_fine is not None else None
    for l in range(len(ops) - 1, 0, -1):
        v = ops[l - 1].initialize_dof_vector()
        mg.interpolate(l, v, vecs[0])
        vecs.insert(0, v)
        if hists is not None:
            hl = []
            for h in hists[0]:
                t = ops[l - 1].initialize_dof_vector()
                mg.interpolate(l, t, h)
                hl.append(t)
            hists.insert(0, hl)
    for l, op in enumerate(ops):
        op.set_linearization_point(vecs[l])
        if hists is not None and params.get("order", 0) > 0:
            op.set_previous_solution(hists[l], weights)
    torch.cuda.synchronize()
    mg.setup()
    return mg, ops


class LinearSolverGMRES:
    """LinearSolverGMRES (solver_l.h:60-82, solver_l.cc:26-74) over the
    device-resident gls_gmres_solve: right-preconditioned GMRES with 30
    temporary vectors, tolerance max(relative * |b|, absolute), dst zeroed
    first.  `preconditioner` is a Multigrid (one V-cycle per application,
    PreconditionerGMG::vmult), an ILU or an AMG of the operator's system
    matrix ("preconditioner": "ILU" / "AMG", main.cc:382-395) or None
    (identity).  solve() raises GlsError on
    no convergence (deal.II's SolverControl::NoConvergence); the statistics of
    the last solve are in .last (n_iterations = SolverControl::last_step())."""

    def __init__(self, op, preconditioner=None, n_max_iterations=10000,
                 absolute_tolerance=1e-12, relative_tolerance=1e-8, max_n_tmp_vectors=30):
        self.op = op
        self.preconditioner = preconditioner
        self.desc = GMRESDesc(max_n_tmp_vectors, n_max_iterations, absolute_tolerance,
                              relative_tolerance)
        self.last = None

    def initialize(self):
        pass  # solver_l.cc:39-43: nothing to do

    def solve(self, dst, src):
        res = GMRESResult()
        p = getattr(self.preconditioner, "preconditioner", self.preconditioner)
        if isinstance(p, (ILU, AMG)):
            kind = GLS_PREC_ILU if isinstance(p, ILU) else GLS_PREC_AMG
            rc = lib().gls_gmres_solve_prec(self.op.h, kind, p.h, C.byref(self.desc), _vptr(dst),
                                            _vptr(src), C.byref(res), _stream())
        else:
            mg = p.h if p is not None else None
            rc = lib().gls_gmres_solve(self.op.h, mg, C.byref(self.desc), _vptr(dst),
                                       _vptr(src), C.byref(res), _stream())
        self.last = {f: getattr(res, f) for f, _ in GMRESResult._fields_}
        _check(rc)
        return dst
