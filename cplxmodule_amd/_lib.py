"""ctypes binding of libcplxamd.so (the C ABI declared in include/cplxamd.h).

The library is the product: there is NO fallback.  If it is missing, was built for another
ABI version, or a kernel is asked to run on a non-HIP tensor, this module raises.
"""
import ctypes
import os
import threading
from ctypes import c_double, c_float, c_int, c_int64, c_uint64, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CPLXAMD_LIB") or os.path.join(_HERE, "libcplxamd.so")   # env: A/B builds
ABI_VERSION = 25

F32, BF16, F16, F64 = 0, 1, 2, 3
KL_KINDS = {"real_vd": 0, "real_ard": 1, "cplx_vd": 2, "cplx_ard": 3, "cplx_vd_approx": 4,
            "cplx_vd_scalefree": 5, "cplx_vd_bogus": 6, "real_l0": 7, "real_l1": 8}

_P, _I, _L, _U, _F, _D = c_void_p, c_int, c_int64, c_uint64, c_float, c_double

# name -> argtypes; restype is int unless listed in _RESTYPES
SIGNATURES = {
    "cplxamd_abi_version": [],
    "cplxamd_vd_kl_ws_bytes": [],
    "cplxamd_vd_kl_fwd": [_P, _P, _P, _I, _P, _P, _P, _L, _P],
    "cplxamd_vd_kl_bwd": [_P, _P, _P, _I, _P, _P, _P, _P, _P, _L, _P],
    "cplxamd_vd_kl_fwd_bwd": [_P, _P, _P, _I, _F, _P, _P, _P, _P, _P, _L, _P],
    "cplxamd_vd_log_alpha": [_P, _P, _P, _P, _L, _P],
    "cplxamd_vd_log_alpha_bwd": [_P, _P, _P, _P, _P, _L, _P],
    "cplxamd_cplx_abs_fwd": [_P, _P, _P, _L, _I, _P],
    "cplxamd_cplx_abs_bwd": [_P, _P, _P, _P, _P, _L, _I, _P],
    "cplxamd_mask_mul": [_P, _P, _P, _P, _P, _L, _I, _I, _P],
    "cplxamd_vd_mask": [_P, _P, _P, _F, _P, _P, _P, _L, _P],
    "cplxamd_expi_fwd": [_P, _P, _L, _P],
    "cplxamd_expi_bwd": [_P, _P, _P, _L, _P],
    "cplxamd_lrt_reparam_fwd": [_P, _P, _P, _P, _P, _U, _U, _P, _P, _P, _L, _I, _P],
    "cplxamd_lrt_reparam_bwd": [_P, _P, _P, _P, _P, _U, _U, _P, _P, _L, _I, _I, _P],
    "cplxamd_lrt_reparam_fwd_ex": [_P, _P, _P, _P, _P, _U, _U, _P, _P, _P, _L, _I, _I, _P],
    "cplxamd_lrt_reparam_bwd_ex": [_P, _P, _P, _P, _P, _U, _U, _P, _P, _L, _I, _I, _I, _P],
    "cplxamd_lrt_reparam_bwd_cols_ws_bytes": [_L, _I],
    "cplxamd_lrt_reparam_bwd_cols": [_P, _P, _P, _P, _P, _U, _U, _P, _P, _L, _I, _I, _I, _I, _P, _P, _P, _L, _P],
    "cplxamd_philox_advance": [_P, _P, _P],
    "cplxamd_philox_normal": [_P, _P, _U, _U, _L, _P],
    "cplxamd_philox_uniform": [_P, _U, _U, _L, _P],
    "cplxamd_l0_gate_fwd": [_P, _P, _P, _U, _U, _P, _P, _P, _L, _I, _I, _I, _I, _P, _P, _P],
    "cplxamd_l0_gate_bwd_ws_bytes": [_L, _I],
    "cplxamd_l0_gate_bwd": [_P, _P, _P, _P, _U, _U, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _L, _P],
    "cplxamd_l1_mask": [_P, _F, _P, _P, _P, _L, _P],
    "cplxamd_cgemm": [_P, _P, _L, _L, _P, _P, _L, _L, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I,
                      _I, _I, _I, _P, _L, _P],
    "cplxamd_cgemm_ex": [_P, _P, _L, _L, _P, _P, _L, _L, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I,
                         _I, _I, _P, _I, _P, _L, _P],
    "cplxamd_rgemm_ex": [_P, _L, _L, _P, _L, _L, _P, _P, _I, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _L, _P],
    "cplxamd_vd_prep_kl": [_P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P],
    "cplxamd_cgemm_lrt_dx": [_P, _P, _L, _L, _P, _P, _L, _L, _P, _P, _P, _L, _P, _P, _L, _I, _I, _I, _I, _P],
    "cplxamd_rgemm_lrt_dx": [_P, _L, _L, _P, _L, _L, _P, _P, _L, _P, _L, _I, _I, _I, _I, _P],
    "cplxamd_cgemm_batched": [_P, _P, _L, _L, _L, _P, _P, _L, _L, _L, _P, _P, _L, _L, _I, _I, _I, _I, _I, _I, _I, _P],
    "cplxamd_rgemm": [_P, _L, _L, _P, _L, _L, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _L, _P],
    "cplxamd_gemm_ws_bytes": [_I, _I, _I, _I, _I, _I],
    "cplxamd_cplx_maxpool2d_fwd": [_P, _P, _P, _P, _P, _P, _I, _P],
    "cplxamd_cplx_maxpool2d_bwd": [_P, _P, _P, _P, _P, _P, _I, _P],
    "cplxamd_cplx_maxpool2d_fwd_cl": [_P, _P, _P, _P, _P, _P, _I, _P],
    "cplxamd_cplx_maxpool2d_bwd_cl": [_P, _P, _P, _P, _P, _P, _I, _P],
    "cplxamd_bilinear_reduce_fwd": [_P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P],
    "cplxamd_bilinear_reduce_bwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P],
    "cplxamd_deinterleave": [_P, _P, _P, _L, _I, _P],
    "cplxamd_interleave": [_P, _P, _P, _L, _I, _P],
    "cplxamd_cplx_mul": [_P, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _P],
    "cplxamd_split_relu": [_P, _P, _P, _P, _P, _P, _L, _I, _I, _P],
    "cplxamd_modrelu_fwd": [_P, _P, _P, _F, _I, _P, _P, _L, _I, _P],
    "cplxamd_modrelu_bwd": [_P, _P, _P, _F, _I, _P, _P, _P, _P, _P, _L, _I, _P],
    "cplxamd_cplx_dropout": [_P, _P, _P, _P, _D, _U, _U, _P, _L, _I, _P],
    "cplxamd_nhwc_pad": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "cplxamd_nhwc_pad_f32": [_P, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    "cplxamd_conv2d_nhwc_f32": [_P, _P, _P, _P, _P, _P, _P, _P] + [_I] * 10 + [_L] + [_I] * 4 + [_P],
    "cplxamd_conv2d_nhwc_wgrad_ws_bytes": [_I] * 8,
    "cplxamd_conv2d_nhwc_wgrad_f32_ws_bytes": [_I] * 8,
    "cplxamd_conv2d_nhwc_wgrad_f32": [_P, _P, _P, _P, _P, _P, _P] + [_I] * 9 + [_P, _L, _P],
    "cplxamd_conv2d_nhwc_wgrad": [_P, _P, _P, _P, _P, _P, _P] + [_I] * 9 + [_P, _L, _P],
    "cplxamd_conv2d_nhwc": [_P, _P, _P, _P, _P, _P, _P, _P] + [_I] * 10 + [_L] + [_I] * 5 + [_P],
    "cplxamd_cl_to_nchw": [_P, _P, _L, _I, _L, _P],
    "cplxamd_conv2d_clr_pack_bytes": [_I, _I, _I, _I],
    "cplxamd_conv2d_clr_ws_bytes": [_I],
    "cplxamd_conv2d_clr_pack": [_P, _P, _I, _I, _I, _I, _I, _P],
    "cplxamd_conv2d_clr": [_P, _P, _P, _P, _L] + [_I] * 11 + [_P, _L, _P],
    "cplxamd_conv2d_clr_wgrad_ws_bytes": [_L, _I, _I, _I, _I],
    "cplxamd_conv2d_clr_wgrad": [_P, _P, _P, _I, _P, _L] + [_I] * 10 + [_P, _L, _P],
    "cplxamd_conv2d_cl_pack_bytes": [_I, _I, _I, _I],
    "cplxamd_conv2d_cl_ws_bytes": [_I],
    "cplxamd_conv2d_cl_pack": [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    "cplxamd_conv2d_cl": [_P, _P, _P, _P, _P, _P, _P, _L] + [_I] * 11 + [_P, _L, _P],
    "cplxamd_conv2d_cl2": [_P, _P, _P, _P, _P, _P, _P, _L] + [_I] * 11 + [_P, _L, _P],
    "cplxamd_chansum2": [_P, _P, _P, _P, _L, _I, _L, _I, _P, _P],
    "cplxamd_conv2d_cl2_lrt_dx": [_P] * 8 + [_L] + [_I] * 6 + [_P, _L, _P],
    "cplxamd_conv2d_cl2_mom_chunks": [_L] + [_I] * 10,
    "cplxamd_conv2d_cl2_mom": [_P, _P, _P, _P, _P, _P, _P, _L] + [_I] * 10 + [_P, _L, _P, _L, _P],
    "cplxamd_conv2d_cl_wgrad_ws_bytes": [_L, _I, _I, _I, _I],
    "cplxamd_conv2d_cl_wgrad": [_P, _P, _P, _P, _P, _P, _P, _L] + [_I] * 10 + [_P, _L, _P],
    "cplxamd_cgemm3m_ws_bytes": [_I, _I, _I],
    "cplxamd_abs2": [_P, _P, _P, _L, _I, _I, _P],
    "cplxamd_modulus": [_P, _P, _P, _L, _P],
    "cplxamd_exp": [_P, _P, _L, _I, _P],
    "cplxamd_cast": [_P, _P, _L, _I, _I, _P],
    "cplxamd_split3": [_P, _P, _L, _P, _L, _L, _L, _I, _I, _I, _P],
    "cplxamd_absmax_ws_bytes": [],
    "cplxamd_absmax_scale": [_P, _P, _L, _L, _I, _I, _P, _P, _P],
    "cplxamd_split2h": [_P, _P, _L, _P, _L, _L, _L, _I, _I, _I, _P, _P],
    "cplxamd_cgemm_sc_fl": [_P, _P, _L, _L, _P, _P, _L, _L, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _P, _P, _L,
                            _I, _P],
    "cplxamd_rgemm_sc_fl": [_P, _L, _L, _P, _L, _L, _P, _P, _I, _P, _L, _I, _I, _I, _I, _I, _P, _P, _P, _P, _L, _I, _P],
    "cplxamd_transpose": [_P, _L, _P, _L, _I, _I, _I, _P],
    "cplxamd_colsum_ws_bytes": [_I],
    "cplxamd_colsum": [_P, _L, _P, _I, _I, _I, _P, _P],
    "cplxamd_colsum2": [_P, _P, _L, _P, _P, _I, _I, _I, _P, _P],
    "cplxamd_lrt_dx_accum": [_P, _P, _P, _P, _P, _L, _I, _I, _P],
    "cplxamd_conv2d_fwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P],
    "cplxamd_conv2d_dgrad": [_P, _P, _P, _P, _P, _P, _P, _I, _P],
    "cplxamd_conv2d_wgrad_splits": [_P],
    "cplxamd_conv2d_wgrad_ws_bytes": [_P, _I],
    "cplxamd_conv2d_wgrad": [_P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _L, _P],
    "cplxamd_conv2d_wgrad_bias": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P, _L, _P],
    "cplxamd_conv2d_out_shape": [_P, _P, _P],
    "cplxamd_conv2d_ktab_size": [_P, _I],
    "cplxamd_conv2d_ktab_fill": [_P, _I, _P],
    "cplxamd_conv2d_bf16_fwd": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P],
    "cplxamd_conv2d_bf16_dgrad": [_P, _P, _P, _P, _P, _P, _P, _P, _P],
    "cplxamd_conv2d_bf16_dgrad_f32": [_P, _P, _P, _P, _P, _P, _P, _P, _P],      # (still ABI 25: an export added)
    "cplxamd_conv2d_bf16_wgrad_ws_bytes": [_P, _I],
    "cplxamd_conv2d_bf16_wgrad": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _L, _P],
    "cplxamd_chansum": [_P, _P, _L, _I, _L, _I, _P, _P],
    "cplxamd_bn_ws_bytes": [_I],
    "cplxamd_bn_fwd": [_P, _P, _P, _P, _L, _I, _L, _P, _P, _P, _P, _P, _I, _I, _F, _F, _P, _L, _P],
    "cplxamd_bn_fwd_ex": [_P, _P, _P, _P, _L, _I, _L, _P, _P, _P, _P, _P, _I, _I, _F, _F, _P, _P, _L, _P],
    "cplxamd_bn_bwd": [_P, _P, _P, _P, _P, _P, _L, _I, _L, _P, _P, _P, _P, _I, _I, _P, _L, _P],
    "cplxamd_bn_bwd_sums": [_P, _P, _P, _P, _P, _P, _L, _I, _L, _P, _P, _P, _P, _I, _I, _P, _P, _L, _P],
    "cplxamd_bn_rows_path": [_L, _I, _L],
    "cplxamd_gemm_set_persistent": [_I],
    "cplxamd_gemm_set_family": [_I],
    # ABI 19: per-call launch policy (trailing `flags` in front of the stream) + the dispatch as a pure function
    "cplxamd_cgemm_fl": [_P, _P, _L, _L, _P, _P, _L, _L, _P, _P, _P, _P, _P, _L, _I, _I, _I, _I, _I,
                         _I, _I, _P, _I, _P, _L, _I, _P],
    "cplxamd_rgemm_fl": [_P, _L, _L, _P, _L, _L, _P, _P, _I, _P, _L, _I, _I, _I, _I, _I, _I, _P, _P, _L, _I, _P],
    "cplxamd_cgemm_lrt_dx_fl": [_P, _P, _L, _L, _P, _P, _L, _L, _P, _P, _P, _L, _P, _P, _L, _I, _I, _I, _I, _I, _P],
    "cplxamd_rgemm_lrt_dx_fl": [_P, _L, _L, _P, _L, _L, _P, _P, _L, _P, _L, _I, _I, _I, _I, _I, _P],
    "cplxamd_gemm_plan": [_I] * 10,
    "cplxamd_conv2d_cl_fl": [_P, _P, _P, _P, _P, _P, _P, _L] + [_I] * 11 + [_P, _L, _I, _P],
    "cplxamd_conv2d_cl2_fl": [_P, _P, _P, _P, _P, _P, _P, _L] + [_I] * 11 + [_P, _L, _I, _P],
    "cplxamd_conv2d_cl2_lrt_dx_fl": [_P] * 8 + [_L] + [_I] * 6 + [_P, _L, _I, _P],
    "cplxamd_conv2d_cl2_mom_chunks_fl": [_L] + [_I] * 11,
    "cplxamd_conv2d_cl2_mom_fl": [_P, _P, _P, _P, _P, _P, _P, _L] + [_I] * 10 + [_P, _L, _P, _L, _I, _P],
    "cplxamd_conv2d_cl_wgrad_fl": [_P, _P, _P, _P, _P, _P, _P, _L] + [_I] * 10 + [_P, _L, _I, _P],
    # ABI 24: batch-norm backward without its apply pass + the weight gradient that forms dX while staging it
    "cplxamd_bn_bwd_sums_amax": [_P, _P, _P, _P, _P, _P, _L, _I, _L, _P, _P, _P, _P, _I, _I, _P, _P, _P, _L, _P],
    "cplxamd_absmax_scale_partials": [_P, _I, _P, _P],
    "cplxamd_bn_bwd_coef": [_P, _P, _P, _P, _L, _I, _L, _P, _P, _P, _P, _I, _I, _P, _P, _P, _L, _P],
    "cplxamd_conv2d_cl_wgrad_bn_fl": [_P] * 11 + [_L] + [_I] * 10 + [_P, _L, _I, _P],
    # ABI 23: float64 contractions (parity mode)
    "cplxamd_gemm_f64": [_P, _P, _L, _L, _L, _P, _P, _L, _L, _L, _P, _P, _P, _P, _L, _L, _I, _I, _I, _I, _I, _P],
    "cplxamd_conv2d_f64": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P],
    "cplxamd_expi_f64": [_P, _P, _L, _P],
    # ABI 22: the channels-last convolutions on IEEE-half pieces (float32 out)
    "cplxamd_conv2d_cl2h_fl": [_P, _P, _I, _P, _P, _P, _P, _P, _I, _P, _P, _L] + [_I] * 7 + [_P, _L, _I, _P],
    "cplxamd_conv2d_cl2h_wrap_fl": [_P, _P, _I, _I, _P, _P, _P, _P, _P, _I, _P, _P, _L] + [_I] * 7 + [_P, _L, _I, _P],
    "cplxamd_conv2d_clh_wgrad_ws_bytes": [_L, _I, _I, _I, _I],
    "cplxamd_conv2d_clh_wgrad": [_P, _P, _P, _P, _P, _P, _P, _L] + [_I] * 10 + [_P, _L, _P],
    "cplxamd_conv2d_clh_wgrad_fl": [_P, _P, _P, _P, _P, _P, _P, _L] + [_I] * 10 + [_P, _L, _I, _P],
    "cplxamd_conv2d_clh_wgrad_skip_fl": [_P, _P, _P, _P, _P, _P, _L] + [_I] * 12 + [_P, _L, _I, _P],
    "cplxamd_conv2d_clr_fl": [_P, _P, _P, _P, _L] + [_I] * 11 + [_P, _L, _I, _P],
    "cplxamd_conv2d_clr_wgrad_fl": [_P, _P, _P, _I, _P, _L] + [_I] * 10 + [_P, _L, _I, _P],
    "cplxamd_bn_moments": [_P, _P, _P, _P, _P, _L, _I, _L, _I, _P, _P, _L, _P],
    "cplxamd_bn_fwd_sync": [_P, _P, _P, _P, _L, _I, _L, _P, _P, _P, _P, _P, _I, _F, _F, _P, _P, _P, _L, _P],
    "cplxamd_bn_fwd_partials": [_P, _P, _P, _P, _L, _I, _L, _P, _P, _P, _P, _P, _I, _F, _F, _P, _P, _I, _P, _L, _P],
    "cplxamd_bn_bwd_sync": [_P, _P, _P, _P, _P, _P, _L, _I, _L, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _L, _P],
    # still ABI 25 (exports added, nothing changed): the complex elementary functions
    "cplxamd_cplx_fn_fwd": [_P, _P, _P, _P, _L, _I, _I, _P],
    "cplxamd_cplx_fn_bwd": [_P, _P, _P, _P, _P, _P, _L, _I, _I, _P],
    # still ABI 25: the Welch spectra (F64 = 3 is their dtype code only)
    "cplxamd_welch_plan": [_L, _L, _L, _I, _P, _P],
    "cplxamd_welch_fwd": [_P, _P, _L, _L, _L, _L, _P, _L, _L, _I, _D, _P, _P, _L, _I, _P],
    "cplxamd_welch_bwd": [_P, _P, _L, _L, _L, _L, _P, _L, _L, _I, _D, _P, _P, _P, _L, _L, _P, _L, _I, _P],
    # still ABI 25: the strided complex contraction behind cplx.einsum (the descriptor is a host struct, EinsumDesc)
    "cplxamd_ceinsum": [_P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _P],
    # still ABI 25: its dispatch as a pure function (addresses as integers, plan = int64[5]: ops.einsum_dispatch)
    "cplxamd_einsum_plan": [_P, _U, _U, _U, _U, _I, _P],
    # still ABI 25: the finishing kernels of the semi-unitary initialiser (nn/init.py; F64 is a plane dtype here)
    "cplxamd_init_ws_bytes": [],
    "cplxamd_init_moments": [_P, _P, _L, _I, _P, _P, _P],
    "cplxamd_init_ns_poly": [_P, _P, _P, _P, _I, _D, _D, _I, _P, _P, _P],
    "cplxamd_init_scale_store": [_P, _P, _P, _P, _L, _L, _I, _I, _D, _P, _P, _I, _I, _P],
    # still ABI 25: structured compaction of the masked layers (compact.py)
    "cplxamd_live_index_ws_bytes": [_L, _L],
    "cplxamd_live_index": [_P, _L, _L, _L, _I, _P, _P, _P, _P, _P, _P, _L, _P],
    "cplxamd_gather_axis": [_P, _P, _P, _P, _P, _L, _L, _L, _L, _I, _P],
    "cplxamd_expand_axis": [_P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _L, _I, _P],
    "cplxamd_compact_weight": [_P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _L, _L, _I, _I, _P],
    "cplxamd_expand_weight": [_P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _L, _L, _I, _I, _P],
    # still ABI 25: the native 3-d implicit-GEMM convolution behind CplxConvTranspose3d (csrc/conv3d.hip; geom = int[19])
    "cplxamd_conv3d_out_shape": [_P, _P, _P, _P],
    "cplxamd_conv3d_fwd": [_P, _P, _P, _P, _P, _P, _P, _I, _P],
    "cplxamd_conv3d_dgrad": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P],
    "cplxamd_conv3d_wgrad_ws_bytes": [_P],
    "cplxamd_conv3d_wgrad": [_P, _P, _P, _P, _P, _P, _P, _I, _P, _L, _P],
    # still ABI 25: the Fourier transforms behind cplx.fft / ifft / fft2 / fftn (csrc/fft.hip; the descriptor is a host
    # struct, FftDesc)
    "cplxamd_fft_plan": [_L, _L, _I, _P, _P],
    "cplxamd_fft": [_P, _P, _P, _P, _P, _I, _I, _P, _L, _P],
    # still ABI 25: the real-input / real-output transforms behind cplx.rfft / irfft / hfft / ihfft (csrc/rfft.hip)
    "cplxamd_rfft_plan": [_L, _L, _I, _I, _P, _P, _P, _P],
    "cplxamd_rfft": [_P, _P, _P, _P, _P, _I, _I, _P, _L, _P],
    # still ABI 25: the short-time transforms behind cplx.stft / istft (csrc/stft.hip; the descriptor is StftDesc)
    "cplxamd_stft_plan": [_L, _L, _L, _L, _L, _I, _I, _P, _P, _P, _P, _P, _P, _P],
    "cplxamd_stft_src": [_P, _L, _L],
    "cplxamd_stft_fold": [_P, _L, _P],
    "cplxamd_stft": [_P, _P, _P, _P, _I, _P, _L, _P],
    "cplxamd_istft": [_P, _P, _P, _P, _I, _P, _L, _P],
    # still ABI 25: overlap-save convolution behind cplx.fftconvolve (csrc/fftconv.hip, fftconv_wgrad.hip; the descriptor
    # is FftConvDesc, the plan fills FFTCONV_PLAN_FIELDS int64)
    "cplxamd_fftconv_plan": [_L, _L, _L, _L, _L, _L, _I, _I, _I, _P],
    "cplxamd_fftconv": [_P, _P, _P, _P, _P, _P, _P, _I, _P, _L, _P],
    "cplxamd_fftconv_wgrad": [_P, _P, _P, _P, _P, _P, _P, _I, _P, _L, _P],
    # still ABI 25: the polyphase rate change behind cplx.upfirdn / resample_poly (csrc/upfirdn.hip, upfirdn_wgrad.hip; the
    # descriptor is UpfirdnDesc, the plan fills UPFIRDN_PLAN_FIELDS int64)
    "cplxamd_upfirdn_plan": [_L, _L, _L, _L, _L, _L, _L, _L, _I, _I, _I, _I, _P],
    "cplxamd_upfirdn": [_P, _P, _P, _P, _P, _P, _P, _I, _P],
    "cplxamd_upfirdn_wgrad": [_P, _P, _P, _P, _P, _P, _P, _I, _P, _L, _P],
    # still ABI 25: the chunk-parallel recurrence behind cplx.lfilter / sosfilt (csrc/iir.hip; the descriptor is IirDesc,
    # the plan fills IIR_PLAN_FIELDS int64)
    "cplxamd_iir_plan": [_L, _L, _L, _L, _L, _I, _I, _L, _P],
    "cplxamd_iir": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P],
    "cplxamd_iir_scan": [_P, _P, _P, _P, _P, _P, _P, _P, _L, _L, _L, _L, _I, _I, _P],
    # still ABI 25: the extended pass of that recurrence behind cplx.filtfilt / sosfiltfilt (csrc/filtfilt.hip; the
    # descriptor is FiltFiltDesc, the plan fills FILTFILT_PLAN_FIELDS int64, _src is the pure index map of the extension)
    "cplxamd_filtfilt_plan": [_L, _L, _L, _L, _L, _L, _I, _I, _L, _P],
    "cplxamd_filtfilt_src": [_L, _L, _L, _I, _P],
    "cplxamd_filtfilt_pass": [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _P],
    # still ABI 25: the chirp-z transform behind cplx.czt / zoom_fft (csrc/czt.hip; the descriptor is CztDesc)
    "cplxamd_czt_plan": [_L, _L, _L, _I, _P, _P],
    "cplxamd_czt": [_P, _P, _P, _P, _P, _I, _I, _P, _L, _P],
}

# modes of cplxamd_init_scale_store (CPLXAMD_INIT_SCALE_*)
INIT_SCALE_NORM, INIT_SCALE_STD, INIT_SCALE_CONST = 0, 1, 2


class EinsumDesc(ctypes.Structure):
    """cplxamd_einsum_desc: groups batch, M, N, K; mode 0 of a group is the outermost."""
    _fields_ = [("nmodes", ctypes.c_int32 * 4), ("extent", (ctypes.c_int32 * 8) * 4), ("stride_a", (c_int64 * 8) * 4),
                ("stride_b", (c_int64 * 8) * 4), ("stride_c", (c_int64 * 8) * 4)]


# The descriptors of the signal kernels (Fft, Czt, FftConv, Upfirdn, Iir, FiltFilt) carry up to three batch runs: _runs.py fuses
# the dims into runs and writes them here (`fill`), csrc/runs.h decodes them (`decode_runs`).
class FftDesc(ctypes.Structure):
    """cplxamd_fft_desc: one transformed dim (n, n_in, element strides) and up to three batch runs, run 0 outermost."""
    _fields_ = [("n", c_int64), ("n_in", c_int64), ("x_es", c_int64), ("y_es", c_int64), ("runs", ctypes.c_int32),
                ("inverse", ctypes.c_int32), ("size", c_int64 * 3), ("x_stride", c_int64 * 3), ("y_stride", c_int64 * 3),
                ("scale", c_double)]


class CztDesc(ctypes.Structure):
    """cplxamd_czt_desc: inputs and outputs per vector (n, m), element strides, up to three batch runs (run 0 outermost),
    the contour (log-modulus and turn fraction of w and of a) and the scale."""
    _fields_ = [("n", c_int64), ("m", c_int64), ("x_es", c_int64), ("y_es", c_int64), ("runs", ctypes.c_int32),
                ("flags", ctypes.c_int32), ("size", c_int64 * 3), ("x_stride", c_int64 * 3), ("y_stride", c_int64 * 3),
                ("w_log", c_double), ("w_turn", c_double), ("a_log", c_double), ("a_turn", c_double), ("scale", c_double)]


CZT_A_OUT = 1                                             # CPLXAMD_CZT_A_OUT


class StftDesc(ctypes.Structure):
    """cplxamd_stft_desc: framing (n_fft, hop, frames), the signal (length, pad, pad_mode, strides), the spectrogram
    strides, one row run, the window, the envelope and the imaginary-plane pointers, flags and scale."""
    _fields_ = [("n_fft", c_int64), ("hop", c_int64), ("frames", c_int64), ("length", c_int64), ("pad", c_int64),
                ("rows", c_int64), ("sig_row_stride", c_int64), ("sig_es", c_int64), ("spec_row_stride", c_int64),
                ("spec_frame_stride", c_int64), ("spec_es", c_int64), ("pad_mode", ctypes.c_int32), ("flags", ctypes.c_int32),
                ("window", c_void_p), ("envelope", c_void_p), ("sig_imag", c_void_p), ("scale", c_double)]


class FftConvDesc(ctypes.Structure):
    """cplxamd_fftconv_desc: lengths (a, taps, result / second operand), the window's start, element strides, up to
    three batch runs (run 0 outermost), the correlation flag and the block-length override."""
    _fields_ = [("a_len", c_int64), ("k", c_int64), ("c_len", c_int64), ("start", c_int64), ("a_es", c_int64),
                ("b_es", c_int64), ("runs", ctypes.c_int32), ("conj", ctypes.c_int32), ("log_l", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("size", c_int64 * 3), ("a_stride", c_int64 * 3), ("b_stride", c_int64 * 3),
                ("y_stride", c_int64 * 3)]


# fields of cplxamd_fftconv_plan's output (CPLXAMD_FFTCONV_*)
FFTCONV_PLAN_FIELDS = ("log_l", "S", "blocks", "vectors_per_workgroup", "in_shift", "out_lo", "n_valid", "ws_bytes",
                       "wgrad_log_l", "wgrad_S", "wgrad_blocks", "wgrad_chunks", "wgrad_per_chunk", "wgrad_ws_bytes")


class UpfirdnDesc(ctypes.Structure):
    """cplxamd_upfirdn_desc: lengths (a, taps, result / second operand), the rates and the offset, element strides, up
    to three batch runs (run 0 outermost) and the correlation flag."""
    _fields_ = [("a_len", c_int64), ("k", c_int64), ("c_len", c_int64), ("up", c_int64), ("down", c_int64), ("off", c_int64),
                ("a_es", c_int64), ("b_es", c_int64), ("runs", ctypes.c_int32), ("conj", ctypes.c_int32),
                ("size", c_int64 * 3), ("a_stride", c_int64 * 3), ("b_stride", c_int64 * 3), ("y_stride", c_int64 * 3)]


# fields of cplxamd_upfirdn_plan's output (CPLXAMD_UPFIRDN_*)
UPFIRDN_PLAN_FIELDS = ("T", "tiles", "vectors_per_workgroup", "span", "phases", "jseg", "segs", "lds_bytes", "threads", "grid",
                       "wgrad_Tn", "wgrad_tiles", "wgrad_kb", "wgrad_kblocks", "wgrad_span", "wgrad_lds_bytes",
                       "wgrad_chunks", "wgrad_per_chunk", "wgrad_ws_bytes")


class IirDesc(ctypes.Structure):
    """cplxamd_iir_desc: samples per row, states per section, sections, the cut into segments, x's element stride, up to
    three batch runs (run 0 outermost) and the reverse / conj flags."""
    _fields_ = [("n", c_int64), ("order", c_int64), ("sections", c_int64), ("segments", c_int64), ("seg_len", c_int64),
                ("x_es", c_int64), ("runs", ctypes.c_int32), ("flags", ctypes.c_int32), ("size", c_int64 * 3),
                ("x_stride", c_int64 * 3), ("c_stride", c_int64 * 3), ("y_stride", c_int64 * 3)]


# fields of cplxamd_iir_plan's output (CPLXAMD_IIR_*)
IIR_PLAN_FIELDS = ("chunk", "lanes", "tile", "tiles", "segments", "seg_len", "bucket", "lds_bytes", "threads", "grid",
                   "ws_bytes")
IIR_REVERSE, IIR_CONJ = 1, 2


class FiltFiltDesc(ctypes.Structure):
    """cplxamd_filtfilt_desc: samples per row of x, the extension on each side, the window of logical samples that is
    stored, the cascade and the cut into segments of the extended row, x's element stride, up to three batch runs (run 0
    outermost; z_stride finds the unit state of a row's filter), the reverse / scale flags and the extension mode."""
    _fields_ = [("n", c_int64), ("edge", c_int64), ("y_lo", c_int64), ("y_n", c_int64), ("order", c_int64),
                ("sections", c_int64), ("segments", c_int64), ("seg_len", c_int64), ("x_es", c_int64),
                ("runs", ctypes.c_int32), ("flags", ctypes.c_int32), ("mode", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("size", c_int64 * 3), ("x_stride", c_int64 * 3), ("c_stride", c_int64 * 3), ("z_stride", c_int64 * 3),
                ("y_stride", c_int64 * 3)]


# fields of cplxamd_filtfilt_plan's output (CPLXAMD_IIR_*, then CPLXAMD_FILTFILT_LEN, _SIGNAL_BYTES)
FILTFILT_PLAN_FIELDS = IIR_PLAN_FIELDS + ("ext_len", "signal_bytes")
FILTFILT_MODES = {"odd": 0, "even": 1, "constant": 2}    # CPLXAMD_FILTFILT_ODD / _EVEN / _CONSTANT
FILTFILT_REVERSE, FILTFILT_SCALE = 1, 2


# function codes of cplxamd_cplx_fn_fwd / _bwd (CPLXAMD_FN_*)
CPLX_FN = {"exp": 0, "log": 1, "sin": 2, "cos": 3, "tan": 4, "sinh": 5, "cosh": 6, "tanh": 7}
# entry points that return an int64 (a count or a size in bytes) instead of an error code
_RESTYPES = dict.fromkeys((
    "cplxamd_stft_src", "cplxamd_absmax_ws_bytes", "cplxamd_init_ws_bytes", "cplxamd_conv2d_cl2_mom_chunks",
    "cplxamd_conv2d_cl2_mom_chunks_fl", "cplxamd_vd_kl_ws_bytes", "cplxamd_lrt_reparam_bwd_cols_ws_bytes",
    "cplxamd_l0_gate_bwd_ws_bytes", "cplxamd_bn_ws_bytes", "cplxamd_conv2d_wgrad_ws_bytes",
    "cplxamd_conv2d_bf16_wgrad_ws_bytes", "cplxamd_colsum_ws_bytes", "cplxamd_gemm_ws_bytes",
    "cplxamd_cgemm3m_ws_bytes", "cplxamd_live_index_ws_bytes", "cplxamd_conv3d_wgrad_ws_bytes",
    "cplxamd_conv2d_nhwc_wgrad_ws_bytes", "cplxamd_conv2d_nhwc_wgrad_f32_ws_bytes", "cplxamd_conv2d_cl_pack_bytes",
    "cplxamd_conv2d_cl_ws_bytes", "cplxamd_conv2d_cl_wgrad_ws_bytes", "cplxamd_conv2d_clh_wgrad_ws_bytes",
    "cplxamd_conv2d_clr_pack_bytes", "cplxamd_conv2d_clr_ws_bytes", "cplxamd_conv2d_clr_wgrad_ws_bytes",
), c_int64)

_lib = None

# ---- per-call launch policy (include/cplxamd.h CPLXAMD_LAUNCH_*) ----------------------------------------------------
# The C ABI keeps no mutable launch state: every GEMM / channels-last convolution call carries its flags.  WHO decides
# lives here, on the host: (1) an override registered for the STREAM the call is launched on (`with launch_policy(flags):`
# -- tests, A/B runs, a serving stream that knows it shares the chip; keyed by stream, not by thread, because autograd
# runs a layer's backward on an engine thread but on the forward's stream), else (2) LAUNCH_SHARED while any
# data-parallel hook of this process has collectives in flight (`shared_chip_enter` / `_leave`:
# cplxmodule_amd.dp.BucketHook; the window is a property of the CHIP, so every model launching into it shares), else
# (3) 0 = the library's defaults.  A hipGraph capture bakes in the flags of its capture pass, exactly as it bakes in every
# other launch argument.
LAUNCH_DEFAULT, LAUNCH_SHARED, LAUNCH_EXCLUSIVE = 0, 1, 2


def LAUNCH_FAMILY(mask):
    return 0x100 | ((int(mask) & 0xff) << 16)


_policy = {}               # (device index, raw stream handle) -> flags
_sharing = set()           # id() of the hooks whose collectives are in flight
_policy_lock = threading.Lock()


def _stream_key():
    if not torch.cuda.is_available():
        return (-1, 0)
    idx = torch.cuda.current_device()
    return (idx, _current_stream_handle(idx))


def launch_flags():
    """Flags of the next GEMM / convolution launch on the current stream."""
    if _policy:
        f = _policy.get(_stream_key())
        if f is not None:
            return f
    return LAUNCH_SHARED if _sharing else LAUNCH_DEFAULT


class launch_policy:
    """`with launch_policy(LAUNCH_SHARED):` -- launches on the stream that is current at entry carry these flags until
    exit (forward AND backward: autograd replays a node's backward on its forward's stream)."""

    def __init__(self, flags):
        self.flags = int(flags)

    def __enter__(self):
        self.key = _stream_key()
        with _policy_lock:
            self.prev = _policy.get(self.key)
            _policy[self.key] = self.flags
        return self

    def __exit__(self, *exc):
        with _policy_lock:
            if self.prev is None:
                _policy.pop(self.key, None)
            else:
                _policy[self.key] = self.prev
        return False


def shared_chip_enter(owner):
    with _policy_lock:
        _sharing.add(id(owner))


def shared_chip_leave(owner):
    with _policy_lock:
        _sharing.discard(id(owner))


class CplxAmdError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle.  Raises CplxAmdError if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CplxAmdError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (or cplxmodule_amd/csrc/build.sh).  cplxmodule_amd has no CPU or "
            "pure-torch fallback.")
    try:
        lib = ctypes.CDLL(LIB_PATH)
    except OSError as e:  # pragma: no cover - depends on the host
        raise CplxAmdError(f"cannot load {LIB_PATH}: {e}") from e
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise CplxAmdError(f"{LIB_PATH} does not export `{name}` (stale build?)") from e
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, c_int)
    if lib.cplxamd_abi_version() != ABI_VERSION:
        raise CplxAmdError("libcplxamd.so ABI version mismatch: rebuild the library")
    _lib = lib
    return lib


_ERRORS = {-1: "invalid argument", -2: "misaligned pointer / leading dimension",
           -3: "unsupported shape", -4: "workspace too small"}


def _raise(name, rc):
    what = _ERRORS.get(rc, f"hipError_t {rc}" if rc > 0 else f"error {rc}")
    raise CplxAmdError(f"{name} failed: {what}")


def try_call(name, *args):
    """Like `call`, but returns False when the entry point declines the shape
    (CPLXAMD_ESHAPE = "use the generic kernel"); every other failure raises."""
    rc = getattr(load(), name)(*args)
    if rc == -3:
        return False
    if rc != 0:
        _raise(name, rc)
    return True


def call(name, *args):
    """Invoke an entry point; non-zero return codes become exceptions."""
    rc = getattr(load(), name)(*args)
    if rc != 0:
        _raise(name, rc)


_empty_anchor = {}


def ptr(t):
    """Device pointer of a tensor for the C ABI (None -> NULL).  An EMPTY tensor has no storage
    (data_ptr() == 0), which the library would reject as a missing argument; it gets the address
    of a small per-device anchor instead -- with zero elements nothing is read or written there."""
    if t is None:
        return None
    p = t.data_ptr()
    if p == 0 and t.numel() == 0 and t.is_cuda:
        key = t.device.index
        if key not in _empty_anchor:
            _empty_anchor[key] = torch.zeros(64, dtype=torch.float32, device=t.device)
        p = _empty_anchor[key].data_ptr()
    return c_void_p(p)


# torch.cuda.current_stream() builds a Stream object per call (~8 us: a third of a millisecond per eager step of a
# 125-launch model); the raw handle is one C call
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def _current_stream_handle(idx=None):
    if idx is None:
        idx = torch.cuda.current_device()
    if _raw_stream is not None:
        return _raw_stream(idx)
    return torch.cuda.current_stream(idx).cuda_stream


def stream_ptr():
    return c_void_p(_current_stream_handle())


def scratch_key(device):
    """Key of the per-(device, stream) scratch caches (split-K slabs, BN / KL partial sums, conv slabs): kernels
    launched on two streams must not share a workspace.  During hipGraph capture the capturing stream's key is
    used like any other, so a cache grown inside a capture belongs to that capture's pool only."""
    dev = device if isinstance(device, torch.device) else torch.device(device)     # (a tensor's .device: nothing is built)
    if dev.type != "cuda":
        return (dev.type, dev.index, 0)
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    return (dev.type, idx, _current_stream_handle(idx))


_scratch = {}       # (tag, scratch_key) -> uint8 buffer


def scratch(tag, device, nbytes, floor=0):
    """THE per-(device, stream) scratch workspace: a uint8 buffer of at least `nbytes`, kept per `tag` and
    `scratch_key(device)` and replaced by a larger one (never below `floor` bytes) only when a request outgrows it.
    Tags are separate buffers -- two can be live in one launch (split-K slab + 3M workspace, conv slab + column sums)."""
    key = (tag, scratch_key(device))
    buf = _scratch.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _scratch[key] = torch.empty(max(nbytes, floor), dtype=torch.uint8, device=device)
    return buf


def al16(t):
    """The streaming kernels move 16 bytes per lane: re-home the rare view that is not aligned (None passes)."""
    return t if t is None or t.data_ptr() % 16 == 0 else t.clone()


def ntuple(v, n):
    """`v` n times unless it is a sequence already (stride, padding, dilation, kernel size)."""
    return (v,) * n if isinstance(v, int) else tuple(v)


def plane_code(what, dtype):
    """ABI dtype code of the float64-capable entry points (transforms, spectra); `what` opens the error message."""
    if dtype == torch.float32:
        return F32
    if dtype == torch.bfloat16:
        return BF16
    if dtype == torch.float64:
        return F64
    raise CplxAmdError(f"{what}, got {dtype}")


def dtype_code(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.bfloat16:
        return BF16
    raise CplxAmdError(f"unsupported dtype {t.dtype}: this kernel takes float32 and bfloat16 (float64 is offered for the "
                       "linear / convolution / batch-norm / relevance layers only: cplxmodule_amd/f64.py)")


def require_device(*tensors):
    """Every kernel argument must live on one HIP device; anything else is an error."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise CplxAmdError(
                "cplxmodule_amd runs on MI355X only: got a tensor on "
                f"'{t.device}'.  Move the module and its inputs to 'cuda' (there is no CPU path).")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise CplxAmdError(f"tensors on different devices: {dev} vs {t.device}")
    return dev
