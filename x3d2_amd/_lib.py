"""ctypes binding of libx3d2_hip.so (the C ABI declared in include/x3d2_hip.h).

The HIP library is the product: there is no CPU fallback.  Importing this
module never needs a GPU, but every compute entry point does."""
import ctypes
import os
import subprocess

from .common import X3dError

HERE = os.path.dirname(os.path.abspath(__file__))
# X3D_SINGLE_PREC=1 (read once, at import): the FP32 flavour of the library (libx3d2_hip_sp.so = the same sources compiled
# with -DX3D_SINGLE_PREC; the reference's -DSINGLE_PREC, src/common.f90:6-12) -- fields, tables, scalars and transforms
# on 4-byte reals.  The host side keeps computing coefficients and wave numbers in float64 and converts at this boundary.
SINGLE = os.environ.get("X3D_SINGLE_PREC") == "1"
LIB_PATH = os.path.join(HERE, "libx3d2_hip_sp.so" if SINGLE else "libx3d2_hip.so")
CSRC = os.path.join(HERE, "csrc")

REAL = ctypes.c_float if SINGLE else ctypes.c_double  # x3d_real of include/x3d2_hip.h
NP_REAL = "float32" if SINGLE else "float64"
c_double_p = ctypes.POINTER(REAL)  # (name kept from the FP64-only days: pointer to the library's real kind)
c_int_p = ctypes.POINTER(ctypes.c_int)
VP = ctypes.c_void_p
I, D, SZT = ctypes.c_int, REAL, ctypes.c_size_t


def torch_real():
    import torch
    return torch.float32 if SINGLE else torch.float64

# name -> (restype, argtypes); kept in step with include/x3d2_hip.h
# (tests/test_abi.py parses the header and compares)
PROTOTYPES = {
    "x3d_last_error": (ctypes.c_char_p, []),
    "x3d_abi_version": (I, []),
    "x3d_real_bytes": (I, []),
    "x3d_backend_create": (I, [ctypes.POINTER(VP), c_int_p, I, VP]),
    "x3d_backend_destroy": (I, [VP]),
    "x3d_backend_create_like": (I, [ctypes.POINTER(VP), VP, c_int_p]),
    "x3d_lazy_enable": (I, [VP, I]),
    "x3d_lazy_set_dist_transeq": (I, [VP, ctypes.c_uint, VP, VP]),
    "x3d_lazy_set_dist_tds": (I, [VP, ctypes.c_uint, VP, VP]),  # (fn: a C function pointer; the Fortran shim's use)
    "x3d_lazy_flush": (I, [VP]),
    "x3d_lazy_sync": (I, [VP]),
    "x3d_lazy_register_block": (I, [VP, VP]),
    "x3d_lazy_unregister_block": (I, [VP, VP]),
    "x3d_tds_pair_zfirst_ok": (I, [VP, VP, VP, c_int_p]),
    "x3d_block_discard": (I, [VP, VP]),
    "x3d_lazy_stats": (I, [VP, ctypes.POINTER(ctypes.c_long)]),
    "x3d_backend_set_stream": (I, [VP, VP]),
    "x3d_backend_set_comm_reserve": (I, [VP, I]),
    "x3d_backend_set_ring": (I, [VP, I, I]),
    "x3d_block_elems": (SZT, [VP]),
    "x3d_padded_dims": (I, [VP, c_int_p]),
    "x3d_device_sync": (I, [VP]),
    "x3d_block_alloc": (I, [VP, ctypes.POINTER(VP)]),
    "x3d_block_free": (I, [VP, VP]),
    "x3d_transpose_xy": (I, [VP, VP, VP, VP, I, I, I]),
    "x3d_transpose_xyz_zxy": (I, [VP, VP, VP, VP, I, I, I]),
    "x3d_transpose_zxy_xyz": (I, [VP, VP, VP, VP, I, I, I]),
    "x3d_poisson_enforce_periodicity_z": (I, [VP, VP, VP]),
    "x3d_poisson_undo_periodicity_z": (I, [VP, VP, VP]),
    "x3d_poisson_postprocess_011": (I, [VP]),
    "x3d_device_alloc": (I, [VP, ctypes.POINTER(VP), ctypes.c_long]),
    "x3d_device_free": (I, [VP, VP]),
    "x3d_copy_to_host": (I, [VP, VP, VP, ctypes.c_long]),
    "x3d_copy_to_device": (I, [VP, VP, VP, ctypes.c_long]),
    "x3d_device_count": (I, [c_int_p]),
    "x3d_ipc_export": (I, [VP, VP, VP]),
    "x3d_ipc_open": (I, [VP, VP, ctypes.POINTER(VP)]),
    "x3d_ipc_close": (I, [VP, VP]),
    "x3d_copy_device": (I, [VP, VP, VP, ctypes.c_long]),
    "x3d_block_fill": (I, [VP, VP, D]),
    "x3d_tdsops_create": (I, [VP, ctypes.POINTER(VP), I, I, I, I] + [c_double_p] * 10),
    "x3d_tdsops_destroy": (I, [VP]),
    "x3d_tdsops_set_penta": (I, [VP, D, D, D] + [c_double_p] * 6 + [I]),
    "x3d_tds_penta_solve": (I, [VP, VP, VP, VP, I, VP, VP]),
    "x3d_tds_solve": (I, [VP, VP, VP, VP, I]),
    "x3d_tds_solve_acc": (I, [VP, VP, VP, VP, I, I, D]),
    "x3d_transeq_acc": (I, [VP, I, VP, VP, VP, VP, VP, VP, D, VP, VP, VP, VP, I]),
    "x3d_npencils": (I, [VP, I]),
    "x3d_pack_halos": (I, [VP, VP, VP, VP, I, I]),
    "x3d_tds_dist_fwd": (I, [VP, VP, VP, VP, VP, VP, VP, VP, I]),
    "x3d_tds_solve_pair": (I, [VP, I, I, VP, VP, VP, VP, VP, VP]),
    "x3d_tds_solve_pair_yperm": (I, [VP, I, VP, VP, VP, VP, VP, VP, I, c_int_p]),
    "x3d_tdsops_halo_rows": (I, [VP, c_int_p]),
    "x3d_tdsops_dims": (I, [VP, c_int_p]),
    "x3d_halo_row_size": (ctypes.c_long, [VP, I]),
    "x3d_pack_halos_multi": (I, [VP, VP, ctypes.POINTER(VP), I, I, I]),
    "x3d_transeq_tile": (I, [VP, I, VP, VP, VP, VP, VP, VP, D, VP, VP, VP, VP, I, VP, VP, I, I, c_int_p]),
    "x3d_transeq_halo_fix": (I, [VP, I, VP, VP, VP, VP, VP, VP, D, VP, VP, VP]),
    "x3d_tds_pair_tile": (I, [VP, I, I, VP, VP, VP, VP, VP, VP, VP, VP, I, I, c_int_p]),
    "x3d_tds_pair_halo_fix": (I, [VP, I, I, VP, VP, VP, VP, VP]),
    "x3d_tds_pair_tile_yperm": (I, [VP, I, VP, VP, VP, VP, VP, VP, VP, VP, I, c_int_p]),
    "x3d_tds_pair_halo_fix_yperm": (I, [VP, I, VP, VP, VP, VP, VP, I]),
    "x3d_tds_solve_lincomb": (I, [VP, I, VP, VP, VP, VP, I, c_double_p, ctypes.POINTER(VP)]),
    "x3d_tds_solve_lincomb_wall": (I, [VP, I, VP, VP, VP, VP, I, c_double_p, ctypes.POINTER(VP), VP]),
    "x3d_tds_solve_mean": (I, [VP, VP, VP, VP, I, c_int_p, D, D, ctypes.POINTER(VP)]),
    "x3d_tds_solve_lincomb_wall_mean": (I, [VP, I, VP, VP, VP, VP, I, c_double_p, ctypes.POINTER(VP), VP, c_int_p, D, D,
                                            ctypes.POINTER(VP)]),
    "x3d_tds_dist_bwd": (I, [VP, VP, VP, VP, VP, VP, I]),
    "x3d_tds_dist_bwd_acc": (I, [VP, VP, VP, VP, VP, VP, I, I, D]),
    "x3d_transeq": (I, [VP, I, VP, VP, VP, VP, VP, VP, D, VP, VP, VP, VP]),
    "x3d_compute_vorticity": (I, [VP, VP, ctypes.POINTER(VP)]),
    "x3d_compute_qcriterion": (I, [VP, VP, ctypes.POINTER(VP)]),
    "x3d_transeq_species": (I, [VP, I, VP, VP, VP, D, VP, VP, VP, I]),
    "x3d_transeq_dist_fwd": (I, [VP, I, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP, VP]),
    "x3d_transeq_dist_bwd": (I, [VP, I, VP, VP, VP, VP, VP, D, VP, VP, VP]),
    "x3d_transeq_dist_bwd_acc": (I, [VP, I, VP, VP, VP, VP, VP, D, VP, VP, VP, I]),
    "x3d_reorder": (I, [VP, VP, VP, I]),
    "x3d_sum_intox": (I, [VP, VP, VP, I]),
    "x3d_veccopy": (I, [VP, VP, VP]),
    "x3d_vecadd": (I, [VP, D, VP, D, VP]),
    "x3d_vecmult": (I, [VP, VP, VP]),
    "x3d_field_scale": (I, [VP, VP, D]),
    "x3d_field_shift": (I, [VP, VP, D]),
    "x3d_backend_counter": (ctypes.c_long, [VP, I]),
    "x3d_backend_switch": (I, [VP, ctypes.c_char_p, ctypes.POINTER(ctypes.c_long)]),
    "x3d_lincomb": (I, [VP, VP, VP, I, c_double_p, ctypes.POINTER(VP)]),
    "x3d_transeq_x_rot": (I, [VP, VP, VP, VP, VP, VP, VP, D, VP, VP, VP, VP, D, VP, c_int_p]),
    "x3d_transeq_x_update": (I, [VP, VP, VP, VP, VP, VP, VP, D, VP, VP, VP, VP, VP, VP, VP, VP, VP, D, c_int_p]),
    "x3d_transeq_x_update_rot": (I, [VP, VP, VP, VP, VP, VP, VP, D, VP, VP, VP, VP, VP, VP, VP, VP, VP, D, D, VP, c_int_p]),
    "x3d_transeq_defer": (I, [VP, I, VP, VP, VP, VP, VP, VP, D, VP, VP, VP, VP, c_int_p]),
    "x3d_pending_flush": (I, [VP, I, VP, VP]),
    "x3d_transeq_stage_ok": (I, [VP, I, VP, VP, VP, VP]),
    "x3d_transeq_lincomb": (I, [VP, I, I, VP, VP, D, VP, VP, VP, VP, VP, VP, I, c_double_p, ctypes.POINTER(VP), I, I]),
    "x3d_transeq_lincomb3": (I, [VP, I, VP, VP, VP, VP, VP, VP, D, VP, VP, VP, VP, ctypes.POINTER(VP), ctypes.POINTER(VP), c_int_p,
                                 c_double_p, ctypes.POINTER(VP), c_int_p, c_int_p, c_int_p]),
    "x3d_transeq_lincomb3_sum": (I, [VP, I, VP, VP, VP, VP, VP, VP, D, VP, VP, VP, VP, ctypes.POINTER(VP), ctypes.POINTER(VP),
                                     c_int_p, c_double_p, ctypes.POINTER(VP), c_int_p, c_int_p, ctypes.POINTER(VP),
                                     ctypes.POINTER(VP), c_double_p, c_int_p]),
    "x3d_lincomb_pending": (I, [VP, I, VP, VP, I, c_double_p, ctypes.POINTER(VP), I, VP, I]),
    "x3d_scalar_product": (I, [VP, VP, VP, c_int_p, c_double_p]),
    "x3d_field_max_sum": (I, [VP, VP, c_int_p, c_double_p, c_double_p]),
    "x3d_field_volume_integral": (I, [VP, VP, c_int_p, c_double_p]),
    "x3d_field_shift_to_mean": (I, [VP, VP, c_int_p, D, D]),
    "x3d_field_mean_shift": (I, [VP, VP, c_int_p, D, D, ctypes.POINTER(VP)]),
    "x3d_field_shift_by": (I, [VP, VP, VP]),
    "x3d_wall_noise": (I, [VP, VP, c_int_p, D, ctypes.c_ulonglong, ctypes.c_ulonglong]),
    "x3d_slice_max_sum": (I, [VP, VP, c_int_p, I, I, c_double_p, c_double_p]),
    "x3d_field_set_face": (I, [VP, VP, c_int_p, D, D, I]),
    "x3d_field_set_face_from_field": (I, [VP, VP, VP, c_int_p, D, I, D]),
    "x3d_set_field_data": (I, [VP, VP, c_double_p, c_int_p]),
    "x3d_get_field_data": (I, [VP, c_double_p, VP, c_int_p]),
    "x3d_set_field_data_pitched": (I, [VP, VP, c_double_p, I, I, c_int_p]),
    "x3d_get_field_data_pitched": (I, [VP, c_double_p, VP, I, I, c_int_p]),
    "x3d_poisson_create": (I, [VP, ctypes.POINTER(VP), c_int_p] + [c_double_p] * 7),
    "x3d_poisson_destroy": (I, [VP]),
    "x3d_poisson_fft_forward": (I, [VP, VP]),
    "x3d_poisson_postprocess_000": (I, [VP]),
    "x3d_poisson_fft_backward": (I, [VP, VP]),
    "x3d_poisson_solve_000": (I, [VP, VP]),
    "x3d_poisson_enforce_periodicity_y": (I, [VP, VP, VP]),
    "x3d_poisson_undo_periodicity_y": (I, [VP, VP, VP]),
    "x3d_poisson_set_stretching": (I, [VP, ctypes.c_int, c_double_p, c_double_p]),
    "x3d_sfftz_spectrum": (I, [VP, ctypes.POINTER(VP), c_int_p, ctypes.POINTER(ctypes.c_long)]),
    "x3d_poisson_create_proxy": (I, [VP, ctypes.POINTER(VP), VP, I, ctypes.c_long, VP, VP]),
    "x3d_poisson_set_stretching_zfirst": (I, [VP, ctypes.c_int, c_double_p, c_double_p]),
    "x3d_poisson_postprocess_010": (I, [VP]),
    "x3d_poisson_solve_010": (I, [VP, VP, VP]),
    "x3d_poisson_solve_010_rows": (I, [VP, VP]),
    "x3d_poisson_solve_010_rows_zfirst": (I, [VP, VP]),
    "x3d_poisson_get_spectral": (I, [VP, c_double_p]),
    "x3d_poisson_set_spectral": (I, [VP, c_double_p]),
    "x3d_sfft_create": (I, [VP, ctypes.POINTER(VP), c_int_p, I, I]),
    "x3d_sfft_create_parts": (I, [VP, ctypes.POINTER(VP), c_int_p, I, I, I]),
    "x3d_sfft_fft_z_part": (I, [VP, VP, I, I]),
    "x3d_sfft_postprocess_000_part": (I, [VP, VP, I]),
    "x3d_sfft_destroy": (I, [VP]),
    "x3d_sfft_sizes": (I, [VP, ctypes.POINTER(ctypes.c_long)]),
    "x3d_sfft_set_waves": (I, [VP] + [c_double_p] * 7),
    "x3d_sfft_forward_local": (I, [VP, VP, VP]),
    "x3d_sfft_fft_z": (I, [VP, VP, I]),
    "x3d_sfft_postprocess_000": (I, [VP, VP]),
    "x3d_sfft_backward_local": (I, [VP, VP, VP]),
    "x3d_sfft010_create": (I, [VP, ctypes.POINTER(VP), c_int_p, I, I]),
    "x3d_sfft010_create_parts": (I, [VP, ctypes.POINTER(VP), c_int_p, I, I, I]),
    "x3d_sfft010_fft_z_part": (I, [VP, VP, I, I]),
    "x3d_sfft010_postprocess_010_part": (I, [VP, VP, I]),
    "x3d_sfft010_destroy": (I, [VP]),
    "x3d_sfft010_sizes": (I, [VP, ctypes.POINTER(ctypes.c_long)]),
    "x3d_sfft010_set_waves": (I, [VP] + [c_double_p] * 7),
    "x3d_sfft010_set_stretching": (I, [VP, I, c_double_p, c_double_p]),
    "x3d_sfft010_periodicity_y": (I, [VP, VP, VP, I]),
    "x3d_sfft010_forward_local": (I, [VP, VP, VP]),
    "x3d_sfft010_fft_z": (I, [VP, VP, I]),
    "x3d_sfft010_postprocess_010": (I, [VP, VP]),
    "x3d_sfft010_backward_local": (I, [VP, VP, VP]),
    "x3d_poisson_zfirst_ok": (I, [VP, c_int_p]),
    "x3d_poisson_zfirst_middle": (I, [VP]),
    "x3d_poisson_zfirst_forward": (I, [VP, VP]),
    "x3d_poisson_zfirst_backward": (I, [VP, VP]),
    "x3d_poisson_solve_000_zfirst": (I, [VP, VP]),
    "x3d_tds_solve_xfft_ok": (I, [VP, VP, c_int_p]),
    "x3d_tds_solve_xfft": (I, [VP, VP, VP, VP]),
    "x3d_poisson_xfft_ok": (I, [VP, c_int_p]),
    "x3d_poisson_zfirst_middle_xpacked": (I, [VP]),
    "x3d_c2c512_x_rows": (I, [VP, VP, ctypes.c_long, ctypes.c_long, I]),
    "x3d_tds_solve_ixfft_ok": (I, [VP, VP, c_int_p]),
    "x3d_tds_solve_ixfft": (I, [VP, VP, VP, VP, D]),
    "x3d_transeq_x_update_xinv_ok": (I, [VP, VP, VP, c_int_p]),
    "x3d_transeq_x_update_xinv": (I, [VP, VP, VP, VP, VP, VP, VP, D, VP, VP, VP, VP, VP, VP, VP, VP, VP, D, c_int_p]),
    "x3d_poisson_xfft_grad_ok": (I, [VP, c_int_p]),
    "x3d_poisson_zfirst_middle_xpacked2": (I, [VP]),
    "x3d_tds_pair_zfirst": (I, [VP, VP, I, VP, VP, VP, VP, VP, VP, c_int_p]),
    "x3d_sfftz_create": (I, [VP, ctypes.POINTER(VP), c_int_p, I, I, I]),
    "x3d_sfftz_destroy": (I, [VP]),
    "x3d_sfftz_sizes": (I, [VP, ctypes.POINTER(ctypes.c_long)]),
    "x3d_sfftz_set_waves": (I, [VP] + [c_double_p] * 7),
    "x3d_sfftz_tds_pair": (I, [VP, I, VP, VP, VP, VP, VP, VP, c_int_p]),
    "x3d_sfftz_z": (I, [VP, VP, I]),
    "x3d_sfftz_z_field": (I, [VP, VP, I]),
    "x3d_sfftz_x_forward": (I, [VP, VP, I]),
    "x3d_sfftz_y_stage": (I, [VP, VP, I, I]),
    "x3d_sfftz_x_backward": (I, [VP, VP, I]),
    "x3d_sfftz_tds_pair_rows": (I, [VP, I, VP, VP, VP, VP, VP, VP, I, I, c_int_p]),
    "x3d_sfftz_z_rows": (I, [VP, VP, I, I, I]),
    "x3d_sfftz_x_forward_rows": (I, [VP, VP, I, I, I]),
    "x3d_sfftz_x_backward_rows": (I, [VP, VP, I, I, I]),
    "x3d_pfft_create": (I, [VP, ctypes.POINTER(VP), c_int_p, I, I, I, I]),
    "x3d_pfft_destroy": (I, [VP]),
    "x3d_pfft_sizes": (I, [VP, ctypes.POINTER(ctypes.c_long)]),
    "x3d_pfft_set_waves": (I, [VP] + [c_double_p] * 7),
    "x3d_pfft_fwd_x": (I, [VP, VP]),
    "x3d_pfft_bwd_x": (I, [VP, VP]),
    "x3d_pfft_fft_y": (I, [VP, I]),
    "x3d_pfft_fft_z": (I, [VP, I]),
    "x3d_pfft_pack_xy": (I, [VP, VP]),
    "x3d_pfft_unpack_xy": (I, [VP, VP]),
    "x3d_pfft_pack_yx": (I, [VP, VP]),
    "x3d_pfft_unpack_yx": (I, [VP, VP]),
    "x3d_pfft_pack_yz": (I, [VP, VP]),
    "x3d_pfft_unpack_yz": (I, [VP, VP]),
    "x3d_pfft_pack_zy": (I, [VP, VP]),
    "x3d_pfft_unpack_zy": (I, [VP, VP]),
    "x3d_pfft_transpose_local": (I, [VP, I]),
    "x3d_pfft_own_chunk": (I, [VP, VP, I]),
    "x3d_pfft_postprocess_000": (I, [VP]),
    "x3d_pfft_create_parts": (I, [VP, ctypes.POINTER(VP), c_int_p, I, I, I, I, I]),
    "x3d_pfft_part_layout": (I, [VP, ctypes.POINTER(ctypes.c_long)]),
    "x3d_pfft_fwd_a_part": (I, [VP, VP, VP, I]),
    "x3d_pfft_fwd_b_part": (I, [VP, VP, VP, I]),
    "x3d_pfft_fwd_c_part": (I, [VP, VP, I]),
    "x3d_pfft_bwd_c_part": (I, [VP, VP, I]),
    "x3d_pfft_bwd_b_part": (I, [VP, VP, VP, I]),
    "x3d_pfft_bwd_a_part": (I, [VP, VP, VP, I]),
    "x3d_stats_update_uvw": (I, [VP, VP, VP, VP, ctypes.POINTER(VP), D]),
    "x3d_stats_update_scalar": (I, [VP, VP, VP, VP, D]),
    "x3d_stats_derive": (I, [VP, ctypes.POINTER(VP), ctypes.POINTER(VP)]),
    "x3d_stats_profile_sums": (I, [VP, VP, VP, VP, c_int_p, I, VP]),
    "x3d_stats_profile_accumulate": (I, [VP, VP, VP, ctypes.c_long, D, D]),
    "x3d_ibm_create": (I, [VP, c_double_p, c_int_p, ctypes.POINTER(VP)]),
    "x3d_ibm_destroy": (I, [VP]),
    "x3d_ibm_counts": (I, [VP, ctypes.POINTER(ctypes.c_long)]),
    "x3d_ibm_body": (I, [VP, VP, VP, VP, VP, c_int_p]),
    "x3d_ibm_set_weights": (I, [VP] + [ctypes.POINTER(ctypes.c_double)] * 3),
    "x3d_ibm_body_loads": (I, [VP, VP, VP, VP, VP, c_int_p, VP, I]),
    "x3d_outflow_params": (I, [VP, VP, c_int_p, D, D, ctypes.POINTER(VP)]),
    "x3d_outflow_params_get": (I, [VP, c_double_p]),
    "x3d_cylinder_apply_bc": (I, [VP, VP, VP, VP, VP, VP, VP, c_int_p, VP]),
    "x3d_inlet_noise": (I, [VP, VP, c_int_p, D, D, ctypes.c_ulonglong, ctypes.c_ulonglong]),
    "x3d_snapshot_pack": (I, [VP, VP, I, c_int_p, c_int_p, c_int_p, c_int_p, I, VP]),
    "x3d_snapshot_copy_async": (I, [VP, VP, VP, ctypes.c_long, VP, c_int_p]),
    "x3d_snapshot_done": (I, [VP, I, c_int_p]),
    "x3d_snapshot_wait": (I, [VP, I]),
    "x3d_checkpoint_pack": (I, [VP, ctypes.POINTER(VP), I, c_int_p, VP, ctypes.POINTER(ctypes.c_ulonglong)]),
    "x3d_checkpoint_sums": (I, [VP, VP, I, ctypes.c_long, ctypes.POINTER(ctypes.c_ulonglong)]),
    "x3d_checkpoint_unpack": (I, [VP, ctypes.POINTER(VP), I, c_int_p, ctypes.c_long, VP]),
    "x3d_spectra_create": (I, [VP, ctypes.POINTER(VP), I, c_int_p, c_int_p, ctypes.POINTER(ctypes.c_double), ctypes.c_double, I]),
    "x3d_spectra_destroy": (I, [VP]),
    "x3d_spectra_sizes": (I, [VP, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_double)]),
    "x3d_spectra_sample": (I, [VP, VP, VP, I]),
    "x3d_spectra_reduce": (I, [VP, VP, I]),
    "x3d_spectra_accumulate": (I, [VP, ctypes.c_long]),
    "x3d_spectra_read": (I, [VP, I, ctypes.POINTER(ctypes.c_double)]),
    "x3d_spectra_load": (I, [VP, ctypes.POINTER(ctypes.c_double)]),
    "x3d_diag_reduce": (I, [VP, VP, VP, VP, ctypes.POINTER(VP), c_int_p, VP, VP]),
    "x3d_diag_max_sum": (I, [VP, VP, c_int_p, VP]),
    "x3d_budget_profile_sums": (I, [VP, VP, c_int_p, I, ctypes.c_double, VP]),
    "x3d_budget_profile_accumulate": (I, [VP, VP, VP, ctypes.c_long, ctypes.c_double, ctypes.c_double]),
    "x3d_les_stress": (I, [VP, ctypes.POINTER(VP), c_int_p, VP, VP]),
    "x3d_les_scalar_flux": (I, [VP, VP, ctypes.POINTER(VP), I, c_int_p, ctypes.POINTER(ctypes.c_double), VP]),
    "x3d_probe_create": (I, [VP, c_int_p, I, c_int_p, I, ctypes.POINTER(VP)]),
    "x3d_probe_sample": (I, [VP, VP, VP, VP, VP, c_int_p, VP]),
    "x3d_probe_destroy": (I, [VP]),
    "x3d_particles_create": (I, [VP, VP, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(VP)]),
    "x3d_particles_destroy": (I, [VP]),
    "x3d_particles_prime": (I, [VP, VP, VP, VP, VP, c_int_p]),
    "x3d_particles_advance": (I, [VP, VP, VP, VP, VP, c_int_p, ctypes.c_double]),
    "x3d_particles_interpolate": (I, [VP, VP, VP, VP, VP, c_int_p, VP, I, VP]),
    "x3d_particles_sort": (I, [VP, VP]),
    "x3d_particles_pack": (I, [VP, VP, VP, ctypes.c_long]),
    "x3d_particles_download": (I, [VP, VP, ctypes.POINTER(ctypes.c_double), c_int_p, c_int_p, c_int_p]),
    "x3d_particles_upload": (I, [VP, VP, ctypes.POINTER(ctypes.c_double), c_int_p, c_int_p, I]),
    "x3d_particles_mp_create": (I, [VP, VP, VP, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double), c_int_p, I, ctypes.POINTER(VP)]),
    "x3d_particles_mp_ghost_pack": (I, [VP, VP, I, VP, VP, VP, c_int_p, VP, VP]),
    "x3d_particles_mp_ghost_unpack": (I, [VP, VP, I, VP, VP]),
    "x3d_particles_mp_prime": (I, [VP, VP, VP, VP, VP, c_int_p]),
    "x3d_particles_mp_move": (I, [VP, VP, ctypes.c_double]),
    "x3d_particles_mp_sample": (I, [VP, VP, VP, VP, VP, c_int_p]),
    "x3d_particles_mp_emigrate": (I, [VP, VP, I, VP, VP]),
    "x3d_particles_mp_immigrate": (I, [VP, VP, I, VP, VP]),
    "x3d_particles_mp_sort": (I, [VP, VP]),
    "x3d_particles_mp_query": (I, [VP, VP, c_int_p]),
    "x3d_particles_mp_pack": (I, [VP, VP, VP, ctypes.c_long]),
    "x3d_particles_mp_download": (I, [VP, VP, ctypes.POINTER(ctypes.c_double), c_int_p, c_int_p, c_int_p, c_int_p, c_int_p]),
    "x3d_particles_mp_upload": (I, [VP, VP, ctypes.POINTER(ctypes.c_double), c_int_p, c_int_p, I, I]),
    "x3d_particles_feedback_enable": (I, [VP, VP, ctypes.c_double] + [ctypes.POINTER(ctypes.c_double)] * 3),
    "x3d_particles_feedback_build": (I, [VP, VP]),
    "x3d_particles_feedback_add": (I, [VP, VP, VP, VP, VP, c_int_p]),
    "x3d_particles_feedback_download": (I, [VP, VP, c_int_p, VP, VP]),
    "x3d_scalars_couple": (I, [VP, ctypes.POINTER(VP), ctypes.POINTER(VP), ctypes.POINTER(VP), ctypes.POINTER(VP), c_int_p, VP]),
    "x3d_scalars_apply_bc": (I, [VP, ctypes.POINTER(VP), I, c_int_p, c_int_p, ctypes.POINTER(ctypes.c_double), I]),
    "x3d_scalars_profile_sums": (I, [VP, VP, VP, VP, ctypes.POINTER(VP), I, c_int_p, I, VP, VP]),
    "x3d_forcing_sizes": (I, [VP, ctypes.POINTER(ctypes.c_long)]),
    "x3d_forcing_project": (I, [VP, VP, VP, VP, VP, VP, ctypes.c_long, VP]),
    "x3d_forcing_coeffs": (I, [VP, VP, VP, I, ctypes.c_double, I, ctypes.c_double, VP, VP]),
    "x3d_forcing_synth": (I, [VP, VP, VP, VP, VP, VP, VP]),
    "x3d_timer_start": (I, [VP]),
    "x3d_timer_stop_ms": (I, [VP, ctypes.POINTER(ctypes.c_float)]),
    "x3d_prof_enable": (I, [VP, I]),
    "x3d_prof_select": (I, [VP, ctypes.c_uint]),
    "x3d_prof_reset": (I, [VP]),
    "x3d_prof_get": (I, [VP, I, I, ctypes.POINTER(ctypes.c_long), ctypes.POINTER(ctypes.c_double)]),
}



class SnapshotVar(ctypes.Structure):
    """x3d_snapshot_var of include/x3d2_hip.h"""
    _fields_ = [("kind", I), ("scale", REAL), ("src", VP * 9)]


class DiagParams(ctypes.Structure):
    """x3d_diag_params of include/x3d2_hip.h"""
    _fields_ = [("ih_x", VP), ("ih_y", VP), ("ih_z", VP), ("first_y", I), ("last_y", I)]


class LesParams(ctypes.Structure):
    """x3d_les_params of include/x3d2_hip.h"""
    _fields_ = [("model", I), ("c2", ctypes.c_double), ("a_x", VP), ("a_y", VP), ("a_z", VP), ("ih_x", VP), ("ih_y", VP),
                ("ih_z", VP)]


class ScalarsParams(ctypes.Structure):
    """x3d_scalars_params of include/x3d2_hip.h"""
    _fields_ = [("ns", I), ("up", ctypes.c_double * 3), ("ri", ctypes.POINTER(ctypes.c_double)),
                ("ref", ctypes.POINTER(ctypes.c_double)), ("grad", ctypes.POINTER(ctypes.c_double))]


class ForcingParams(ctypes.Structure):
    """x3d_forcing_params of include/x3d2_hip.h"""
    _fields_ = [("nglobal", I * 3), ("offset", I * 3), ("nlocal", I * 3), ("periodic", I * 3), ("M", I * 3), ("nband", I),
                ("tw_x", VP), ("tw_y", VP), ("tw_z", VP), ("band", VP), ("kvec", VP)]


class ParticlesDecomp(ctypes.Structure):
    """x3d_particles_decomp of include/x3d2_hip.h"""
    _fields_ = [("nglobal", I * 3), ("offset", I * 3), ("nlocal", I * 3), ("nproc", I * 3), ("rank", I * 3), ("capacity", I),
                ("mig_capacity", I)]


class ParticlesParams(ctypes.Structure):
    """x3d_particles_params of include/x3d2_hip.h"""
    _fields_ = [("n", I), ("order", I), ("wall", I), ("tau", ctypes.c_double), ("g", ctypes.c_double * 3), ("periodic", I * 3),
                ("uniform", I * 3), ("L", ctypes.c_double * 3), ("coords", ctypes.POINTER(ctypes.c_double) * 3)]


class BudgetFields(ctypes.Structure):
    """x3d_budget_fields of include/x3d2_hip.h"""
    _fields_ = [("u", VP), ("v", VP), ("w", VP), ("p", VP), ("grads", VP * 9)]


_lib = None


def build(verbose=False):
    """hipcc-compile every HIP source for gfx950 into x3d2_amd/libx3d2_hip.so
    (cross-compiles without a GPU)."""
    for flavour in ([], ["SP=1"]):  # FP64 (libx3d2_hip.so) and FP32 (libx3d2_hip_sp.so: -DX3D_SINGLE_PREC)
        r = subprocess.run(["make", "-C", CSRC, "-j4"] + flavour, capture_output=True, text=True)
        if verbose or r.returncode != 0:
            print(r.stdout[-4000:], r.stderr[-4000:])
        if r.returncode != 0:
            raise X3dError("building libx3d2_hip%s.so failed" % ("_sp" if flavour else ""))
    return LIB_PATH


def load():
    """dlopen the HIP backend; fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # torch first: its wheel bundles its own HIP runtime and must be the one the
    # process initialises (loading /opt/rocm's copy first leaves two runtimes)
    import torch  # noqa: F401
    # rocFFT compiles its kernels at plan creation (seconds per new transform length on a fresh box); a cache file that
    # travels with the tree (built artefact, git-ignored like the .so) spares every process that compilation
    os.environ.setdefault("ROCFFT_RTC_CACHE_PATH", os.path.join(HERE, "rocfft_rtc_cache.db"))
    if not os.path.exists(LIB_PATH):
        raise X3dError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`"
                       " (the HIP backend has no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError = symbol missing from the .so
        fn.restype = res
        fn.argtypes = args
    want = 4 if SINGLE else 8
    if lib.x3d_real_bytes() != want:  # (a stale or misnamed build: every pointer below would be misread)
        raise X3dError(f"{LIB_PATH} computes in {lib.x3d_real_bytes()}-byte reals, this process expects {want}")
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise X3dError(load().x3d_last_error().decode())


def ints(*v):
    return (ctypes.c_int * len(v))(*[int(x) for x in v])
