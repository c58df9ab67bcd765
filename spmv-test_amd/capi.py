"""ctypes binding of include/spmv_hip.h (libspmv_hip.so).

Every call goes to the HIP library; there is no Python or CPU implementation behind these
wrappers.  A non-zero status raises :class:`SpmvError` with ``spmv_last_error()``.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "lib" / "libspmv_hip.so"
LAUNCHERS_PATH = PKG_DIR / "lib" / "libspmv_launchers.so"
TESTER_PATH = PKG_DIR / "bin" / "sparse_sgemv"
DIST_LIB_PATH = PKG_DIR / "lib" / "libspmv_dist.so"            # include/spmv_dist.h (RCCL; not loaded by this module)
DIST_SELFTEST_PATH = PKG_DIR / "bin" / "spmv_dist_selftest"

# enum spmv_variant
SCALAR, WAVE, WAVE_PIPE, VECTOR, ADAPTIVE, TILED, PANEL, AUTO, XSKIP = range(9)
# the variants that accept ANY CSR matrix ...
VARIANTS = {"scalar": SCALAR, "wave": WAVE, "wave_pipe": WAVE_PIPE, "vector": VECTOR,
            "adaptive": ADAPTIVE, "tiled": TILED, "panel": PANEL, "auto": AUTO}
# ... and with the one that is limited to dense-ish matrices (its plan refuses the others)
ALL_VARIANTS = dict(VARIANTS, xskip=XSKIP)

# enum spmv_status
OK, ERR_NO_DEVICE, ERR_INVALID, ERR_HIP, ERR_VARIANT, ERR_NOT_PLANNED, ERR_STALE_PLAN = 0, -1, -2, -3, -4, -5, -6

# every symbol include/spmv_hip.h declares: name -> (restype, argtypes)
_i32p, _f32p, _vp = C.c_void_p, C.c_void_p, C.c_void_p   # raw addresses (host or device)
_H = C.c_void_p                                           # spmv_csr_t*
_HP = C.POINTER(C.c_void_p)


class AttnHeads(C.Structure):
    """spmv_attn_heads_t: the heads of one _heads call and, per operand, the floats from head h to head h + 1."""
    _fields_ = [("heads", C.c_int32), ("reserved", C.c_int32)] + [(n, C.c_int64) for n in (
        "q", "k", "v", "o", "d_o", "stats", "delta", "dq", "dk", "dv")]


_HS = C.POINTER(AttnHeads)
SIGNATURES = {
    "spmv_device_count": (C.c_int, []),
    "spmv_last_error": (C.c_char_p, []),
    "spmv_variant_name": (C.c_char_p, [C.c_int]),
    "spmv_last_first_launch_ms": (C.c_float, []),
    "spmv_csr_create_host": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, _i32p, _i32p, _f32p, _HP]),
    "spmv_csr_create_device": (C.c_int, [C.c_int64, C.c_int64, C.c_int64, _i32p, _i32p, _f32p, _HP]),
    "spmv_csr_from_dense_host": (C.c_int, [C.c_int, C.c_int, _f32p, _vp, _HP]),
    "spmv_csr_from_dense_device": (C.c_int, [C.c_int, C.c_int, _f32p, _vp, _HP]),
    "spmv_csr_download": (C.c_int, [_H, _i32p, _i32p, _f32p]),
    "spmv_csr_validate": (C.c_int, [_H, C.c_void_p]),
    "spmv_csr_dims": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "spmv_csr_column_range": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64), _vp]),
    "spmv_csr_destroy": (C.c_int, [_H]),
    "spmv_csr_transpose": (C.c_int, [_H, C.c_int, _vp, _HP]),
    "spmv_csr_transpose_values": (C.c_int, [_H, _H, _vp]),
    "spmv_csr_transpose_gather": (C.c_int, [_H, C.c_int, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "spmv_csr_transpose_map_bytes": (C.c_int64, [_H]),
    "spmv_csr_select_topk": (C.c_int, [_H, _f32p, C.c_int, C.c_int, C.c_int, _vp, _HP]),
    "spmv_csr_select_threshold": (C.c_int, [_H, _f32p, C.c_float, C.c_int, C.c_int, _vp, _HP]),
    "spmv_csr_select_values": (C.c_int, [_H, _H, _vp]),
    "spmv_csr_select_gather": (C.c_int, [_H, C.c_int, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "spmv_csr_select_scatter": (C.c_int, [_H, C.c_int, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "spmv_csr_select_map_bytes": (C.c_int64, [_H]),
    "spmv_csr_copy_arrays": (C.c_int, [_H, _i32p, _i32p, _f32p, _vp]),
    "spmv_csr_spgemm": (C.c_int, [_H, _H, C.c_int, _vp, _HP, C.POINTER(C.c_int64)]),
    "spmv_csr_spgemm_values": (C.c_int, [_H, _H, _H, _vp]),
    "spmv_csr_spgemm_plan_bytes": (C.c_int64, [_H]),
    "spmv_csr_add": (C.c_int, [_H, _H, C.c_float, C.c_float, C.c_int, C.c_int, _vp, _HP]),
    "spmv_csr_add_values": (C.c_int, [_H, _H, _H, C.c_float, C.c_float, _vp]),
    "spmv_csr_add_gather": (C.c_int, [_H, C.c_int, C.c_int, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "spmv_csr_add_plan_bytes": (C.c_int64, [_H]),
    "spmv_csr_trsv_plan": (C.c_int, [_H, C.c_int, C.c_int, _vp]),
    "spmv_csr_trsv": (C.c_int, [_H, C.c_int, C.c_int, _vp, _vp, _vp]),
    "spmv_csr_trsv_plan_bytes": (C.c_int64, [_H, C.c_int]),
    "spmv_csr_trsv_plan_info": (C.c_int, [_H, C.c_int, C.POINTER(C.c_int64)]),
    "spmv_csr_trsv_plan_rows": (C.c_int, [_H, C.c_int, _vp, _vp]),
    "spmv_csr_trsv_describe": (C.c_int, [_H, C.c_int, C.c_char_p, C.c_int]),
    "spmv_csr_ilu0": (C.c_int, [_H, C.c_int, _vp, C.POINTER(_H)]),
    "spmv_csr_ilu0_values": (C.c_int, [_H, _H, _vp]),
    "spmv_csr_ilu0_solve": (C.c_int, [_H, _vp, _vp, _vp]),
    "spmv_csr_ilu0_pivot": (C.c_int, [_H, _vp, C.POINTER(C.c_int64)]),
    "spmv_csr_ilu0_plan_bytes": (C.c_int64, [_H]),
    "spmv_csr_color": (C.c_int, [_H, C.c_uint32, _vp, _i32p, _i32p, _i32p, C.c_int, C.POINTER(C.c_int64)]),
    "spmv_csr_permute": (C.c_int, [_H, _i32p, _i32p, C.c_int, _vp, _HP]),
    "spmv_csr_permute_values": (C.c_int, [_H, _H, _vp]),
    "spmv_csr_permute_gather": (C.c_int, [_H, C.c_int, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "spmv_csr_permute_map_bytes": (C.c_int64, [_H]),
    "spmv_permute_vector": (C.c_int, [_i32p, C.c_int64, C.c_int, _f32p, _f32p, _vp]),
    "spmv_csr_plan": (C.c_int, [_H, C.c_int, _vp]),
    "spmv_csr_run": (C.c_int, [_H, C.c_int, _f32p, _f32p, _vp]),
    "spmv_csr_run_vals16": (C.c_int, [_H, C.c_int, C.c_int, _vp, _f32p, _f32p, _vp]),
    "spmv_csr_values_changed": (C.c_int, [_H]),
    "spmv_csr_spmm_plan": (C.c_int, [_H, _vp]),
    "spmv_csr_spmm": (C.c_int, [_H, C.c_int, _f32p, C.c_int64, _f32p, C.c_int64, _vp]),
    "spmv_csr_spmm_plan_bytes": (C.c_int64, [_H]),
    "spmv_csr_spmm_describe": (C.c_int, [_H, C.c_char_p, C.c_int]),
    "spmv_csr_sddmm": (C.c_int, [_H, C.c_int, _f32p, C.c_int64, _f32p, C.c_int64, _f32p, _vp]),
    # the 16-bit calls: `int dtype` after the handle, every dense matrix a void *
    "spmv_csr_spmm_16": (C.c_int, [_H, C.c_int, C.c_int, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "spmv_csr_sddmm_16": (C.c_int, [_H, C.c_int, C.c_int, _vp, C.c_int64, _vp, C.c_int64, _f32p, _vp]),
    "spmv_csr_spmm_plan_cols": (C.c_int, [_H, C.c_int, _vp]),
    "spmv_csr_spmm_cols": (C.c_int, [_H, C.c_int, C.c_int, _vp, C.c_int64, _vp, C.c_int64, _vp]),
    "spmv_csr_sddmm_cols": (C.c_int, [_H, C.c_int, C.c_int, _vp, C.c_int64, _vp, C.c_int64, _f32p, _vp]),
    "spmv_csr_row_softmax": (C.c_int, [_H, C.c_float, _f32p, _f32p, _vp]),
    "spmv_csr_row_softmax_backward": (C.c_int, [_H, C.c_float, _f32p, _f32p, _f32p, _vp]),
    "spmv_csr_attention_plan": (C.c_int, [_H, _vp]),
    "spmv_csr_attention_plan_bytes": (C.c_int64, [_H]),
    "spmv_csr_attention_plan_heads": (C.c_int, [_H, C.c_int, _vp]),
    "spmv_csr_attention_max_heads": (C.c_int, [_H, C.c_int, C.c_int]),
    "spmv_csr_attention_plan_wide": (C.c_int, [_H, C.c_int, _vp]),
    "spmv_csr_attention_max_heads_wide": (C.c_int, [_H, C.c_int, C.c_int]),
    "spmv_csr_plan_get": (C.c_int, [_H, C.c_int, C.POINTER(C.c_int32)]),
    "spmv_csr_plan_set": (C.c_int, [_H, C.c_int, C.POINTER(C.c_int32), _vp]),
    "spmv_csr_plan_like": (C.c_int, [_H, _H, C.c_int, _vp]),
    "spmv_csr_plan_bytes": (C.c_int64, [_H, C.c_int]),
    "spmv_csr_plan_describe": (C.c_int, [_H, C.c_int, C.c_char_p, C.c_int]),
    "spmv_csr_plan_chunk_order": (C.c_int, [_H, C.c_int]),
    "spmv_csr_time": (C.c_int, [_H, C.c_int, _f32p, _f32p, C.c_int, _vp, C.POINTER(C.c_float)]),
    "spmv_csr_run_host": (C.c_int, [_H, C.c_int, _f32p, _f32p, C.POINTER(C.c_float)]),
    "spmv_dense_gemv": (C.c_int, [C.c_int, C.c_int, _f32p, _f32p, _f32p, C.c_int, _vp]),
    "spmv_dense_gemv_workspace_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "spmv_dense_gemv_ws": (C.c_int, [C.c_int, C.c_int, _f32p, _f32p, _f32p, C.c_int, _vp, C.c_int64, _vp]),
    "spmv_asp_retile": (C.c_int, [C.c_int, C.c_int, _f32p, _f32p, _vp]),
    "spmv_asp_gemv_ws": (C.c_int, [C.c_int, C.c_int, _f32p, _f32p, _f32p, _vp, C.c_int64, _vp]),
    "spmv_dense_gemv_host": (C.c_int, [C.c_int, C.c_int, _f32p, _f32p, _f32p, C.c_int, C.POINTER(C.c_float)]),
    "spmv_tcsr_from_dense_host": (C.c_int, [C.c_int, C.c_int, _f32p, _vp, _HP]),
    "spmv_tcsr_from_dense_device": (C.c_int, [C.c_int, C.c_int, _f32p, _vp, _HP]),
    "spmv_tcsr_sizes": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "spmv_tcsr_download": (C.c_int, [_H, _i32p, _i32p, _f32p]),
    "spmv_tcsr_run": (C.c_int, [_H, _f32p, _f32p, _vp]),
    "spmv_tcsr_run_host": (C.c_int, [_H, _f32p, _f32p, C.POINTER(C.c_float)]),
    "spmv_tcsr_destroy": (C.c_int, [_H]),
    "spmv_bitmap_from_dense_host": (C.c_int, [C.c_int, C.c_int, C.c_int, _f32p, _vp, _HP]),
    "spmv_bitmap_from_dense_device": (C.c_int, [C.c_int, C.c_int, C.c_int, _f32p, _vp, _HP]),
    "spmv_bitmap_sizes": (C.c_int, [_H, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "spmv_bitmap_download": (C.c_int, [_H, _i32p, _f32p]),
    "spmv_bitmap_run": (C.c_int, [_H, _f32p, _f32p, _vp]),
    "spmv_bitmap_run_host": (C.c_int, [_H, _f32p, _f32p, C.POINTER(C.c_float)]),
    "spmv_bitmap_destroy": (C.c_int, [_H]),
    "spmv_synth_fill": (C.c_int, [C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64,
                                  _i32p, _i32p, _f32p, _vp]),
    "spmv_synth_x": (C.c_int, [C.c_uint64, C.c_int64, C.c_int64, _f32p, _vp]),
    "spmv_calib_stream": (C.c_int, [_vp, C.c_int64, _f32p, _vp]),
    "spmv_calib_gather": (C.c_int, [_f32p, C.c_int64, C.c_int64, C.c_int, _f32p, _vp]),
    "spmv_calib_store": (C.c_int, [_f32p, C.c_int64, C.c_int, _vp]),
    "spmv_calib_marker": (C.c_int, [C.c_int, _vp]),
    "spmv_debug_bounds": (C.c_int, [_vp, C.c_int]),
}
# Fused attention, one description per pass: the operands in C argument order as (name, side of this handle that counts its rows,
# width, AttnHeads field, whether it holds the K/V heads of a _gqa call).  The width is "k" or "kv" for a matrix, which the C call
# takes as (pointer, ld); for a vector it is the floats per query, and the C call takes the pointer alone.  `int kv` precedes V.
_ATTN_PASSES = {
    "forward": (("Q", "rows", "k", "q", False), ("K", "cols", "k", "k", True), ("V", "cols", "kv", "v", True),
                ("O", "rows", "kv", "o", False), ("stats", "rows", 2, "stats", False)),
    "backward_q": (("Q", "rows", "k", "q", False), ("K", "cols", "k", "k", True), ("V", "cols", "kv", "v", True),
                   ("O", "rows", "kv", "o", False), ("dO", "rows", "kv", "d_o", False), ("stats", "rows", 2, "stats", False),
                   ("delta", "rows", 1, "delta", False), ("dQ", "rows", "k", "dq", False)),
    # (on the handle of the transposed pattern: rows = keys, cols = queries)
    "backward_kv": (("Q", "cols", "k", "q", False), ("K", "rows", "k", "k", True), ("V", "rows", "kv", "v", True),
                    ("dO", "cols", "kv", "d_o", False), ("stats", "cols", 2, "stats", False), ("delta", "cols", 1, "delta", False),
                    ("dK", "rows", "k", "dk", True), ("dV", "rows", "kv", "dv", True)),
}
_ATTN_MODES = {"one": "", "heads": "_heads", "gqa": "_gqa"}      # the three calls of a pass: the suffix of their names
for _pass, _ops in _ATTN_PASSES.items():
    _tail = [a for n, _, w, _, _ in _ops for a in ([C.c_int] if n == "V" else []) + [_f32p] + ([C.c_int64] if isinstance(w, str) else [])]
    for _mode, _suffix in _ATTN_MODES.items():
        _head = [_H] + ([_HS] if _mode != "one" else []) + ([C.c_int] if _mode == "gqa" else [])      # handle, hs, group
        SIGNATURES[f"spmv_csr_attention_{_pass}{_suffix}"] = (C.c_int, _head + [C.c_float, C.c_int] + _tail + [_vp])
    # the 16-bit call of the pass: the _gqa arguments with `int dtype` after group; every matrix pointer is a void *
    SIGNATURES[f"spmv_csr_attention_{_pass}_16"] = (C.c_int, [_H, _HS, C.c_int, C.c_int, C.c_float, C.c_int] + _tail + [_vp])
    # the biased call of the pass: the _16 arguments with (bias, bias_stride) -- backward_q: and (dBias, dbias_stride) -- after dtype
    SIGNATURES[f"spmv_csr_attention_{_pass}_bias"] = (C.c_int, [_H, _HS, C.c_int, C.c_int] + [_f32p, C.c_int64] * (2 if _pass == "backward_q" else 1)
                                                      + [C.c_float, C.c_int] + _tail + [_vp])
    # the wide call of the pass (widths up to 128): exactly the _bias arguments; a null bias means none
    SIGNATURES[f"spmv_csr_attention_{_pass}_wide"] = SIGNATURES[f"spmv_csr_attention_{_pass}_bias"]
ATTN_FP32, ATTN_BF16, ATTN_FP16 = 0, 1, 2      # enums of include/spmv_hip.h: the dtype of a _16 call (1, 2) or a _bias call
SPGEMM_CLASS_SLOTS = (64, 512, 4096, 32768)     # SPMV_SPGEMM_CLASS_SLOTS: the words of LDS a row of each class of spgemm sorts in
ADD_UNION, ADD_INTERSECT, ADD_MINUS = 0, 1, 2   # enums of include/spmv_hip.h: the op of spmv_csr_add
_ADD_OPS = {"union": ADD_UNION, "intersect": ADD_INTERSECT, "minus": ADD_MINUS}
TRSV_LOWER, TRSV_UPPER = 0, 1                  # enums of include/spmv_hip.h: the uplo of spmv_csr_trsv
TRSV_NON_UNIT, TRSV_UNIT = 0, 1                # ... and its diag
_TRSV_UPLO = {"lower": TRSV_LOWER, "upper": TRSV_UPPER}
SPMV_TRSV_SERIAL_MAX = 32                      # SPMV_TRSV_SERIAL_MAX: the terms of a row that trsv sums as one chain
SPMV_ILU0_SERIAL_MAX = 32                      # SPMV_ILU0_SERIAL_MAX: the stored entries of a row that ilu0 factors in one lane
SPMV_COLOR_SERIAL_MAX = 32                     # SPMV_COLOR_SERIAL_MAX: the neighbour entries of a row that color takes in one lane
PERMUTE_KEEP_MAP, PERMUTE_VIA_TRANSPOSE = 1, 2  # flags of spmv_csr_permute
COLS_MAX_K = 65536                             # SPMV_COLS_MAX_K: the widest k of spmm_cols / sddmm_cols
# CsrMatrix.spmm / spmm_cols / sddmm / sddmm_cols: (method, ATTN_* dtype of its matrices) -> (the C call, its dtype argument
# as a tuple: the narrow fp32 calls take none).  Built here, not per call.
_PRODUCT_CALLS = {}
for _m in ("spmm", "sddmm"):
    _PRODUCT_CALLS[_m, ATTN_FP32] = (f"spmv_csr_{_m}", ())
    for _d in (ATTN_BF16, ATTN_FP16):
        _PRODUCT_CALLS[_m, _d] = (f"spmv_csr_{_m}_16", (_d,))
    for _d in (ATTN_FP32, ATTN_BF16, ATTN_FP16):
        _PRODUCT_CALLS[_m + "_cols", _d] = (f"spmv_csr_{_m}_cols", (_d,))
# test only: the bounds-checked build of the library (SPMV_CHECK_BOUNDS) and its sites (csrc/spmv_internal.hpp BoundsSite)
CHECKED_LIB_PATH = PKG_DIR / "lib" / "libspmv_hip_checked.so"
BOUNDS_SITES = ("k_bs_sums prod", "k_bs_sums acc", "k_bin_sums prod", "k_bin_sums r16", "k_bs_products c16",
                "k_bs_products pvals", "k_bs_products prod store", "k_bs_group store", "k_bs_place load",
                "k_bs_place acc store", "k_bs_place c16/pvals store", "k_bs_fill acc store", "k_bs_fill c16/pvals store",
                "k_panel packed", "k_panel pvals")


class SpmvError(RuntimeError):
    def __init__(self, status: int, message: str):
        super().__init__(f"libspmv_hip status {status}: {message}")
        self.status = status


_lib = None


def use_library(path) -> None:
    """Development aid (tools/explore.py A/B runs): bind to another build of libspmv_hip.so.
    Handles created before the switch must already be closed."""
    global _lib, LIB_PATH
    LIB_PATH = Path(path).resolve()
    _lib = None


def lib() -> C.CDLL:
    """Load libspmv_hip.so (once).  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise FileNotFoundError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C spmv-test_amd`); there is no fallback implementation")
        # torch bundles its own libamdhip64.so.7; importing it first makes this library bind to
        # the same HIP runtime instance, so torch device pointers and streams are valid here.
        import torch  # noqa: F401
        l = C.CDLL(os.fspath(LIB_PATH), mode=C.RTLD_LOCAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def check(status: int) -> None:
    if status != OK:
        raise SpmvError(status, lib().spmv_last_error().decode(errors="replace"))


def device_count() -> int:
    return lib().spmv_device_count()


def _ptr(t) -> int:
    """Address of a torch tensor / numpy array / None."""
    if t is None:
        return 0
    if hasattr(t, "data_ptr"):
        return t.data_ptr()
    return t.ctypes.data


def _width(t, ndim: int = 2):
    """Columns (the last extent) of an ndim-D tensor (None for anything else: the caller's shape check then names it)."""
    return t.shape[ndim - 1] if getattr(t, "ndim", 0) == ndim else None


def _stream_handle(stream=None) -> int:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream()
    return s.cuda_stream


class CsrMatrix:
    """Owner of one ``spmv_csr_t`` handle (a whole matrix or one row-block shard)."""

    def __init__(self, handle: int, keepalive=()):
        self._h = C.c_void_p(handle)
        self._keep = tuple(keepalive)
        r, c, z = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().spmv_csr_dims(self._h, C.byref(r), C.byref(c), C.byref(z)))
        self.rows, self.cols, self.nnz = r.value, c.value, z.value

    # -- constructors ---------------------------------------------------------
    @classmethod
    def from_host(cls, rows, cols, row_ptr, col_idx, vals):
        import numpy as np
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        col_idx = np.ascontiguousarray(col_idx, dtype=np.int32)
        vals = np.ascontiguousarray(vals, dtype=np.float32)
        h = C.c_void_p()
        check(lib().spmv_csr_create_host(rows, cols, int(col_idx.size), _ptr(row_ptr), _ptr(col_idx),
                                         _ptr(vals), C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_device(cls, rows, cols, row_ptr, col_idx, vals):
        """Borrow torch device tensors (int32, int32, float32); they are kept alive by this object."""
        h = C.c_void_p()
        check(lib().spmv_csr_create_device(rows, cols, int(col_idx.numel()), _ptr(row_ptr), _ptr(col_idx),
                                           _ptr(vals), C.byref(h)))
        return cls(h.value, keepalive=(row_ptr, col_idx, vals))

    @classmethod
    def from_dense_host(cls, A):
        """Dense row-major numpy A[M][N] -> CSR of A^T on the device (matrix_csr.cpp:5-23 semantics)."""
        import numpy as np
        A = np.ascontiguousarray(A, dtype=np.float32)
        M, N = A.shape
        h = C.c_void_p()
        check(lib().spmv_csr_from_dense_host(M, N, _ptr(A), 0, C.byref(h)))
        return cls(h.value)

    @classmethod
    def from_dense_device(cls, A):
        M, N = A.shape
        h = C.c_void_p()
        check(lib().spmv_csr_from_dense_device(M, N, _ptr(A), _stream_handle(), C.byref(h)))
        return cls(h.value)

    # -- hot path ---------------------------------------------------------------
    def plan(self, variant: int, stream=None) -> None:
        check(lib().spmv_csr_plan(self._h, variant, _stream_handle(stream)))

    def run(self, variant: int, x, y, stream=None) -> None:
        """Enqueue y = A x on torch's current stream (or ``stream``).  x, y: float32 device tensors."""
        assert x.numel() >= self.cols and y.numel() >= self.rows
        check(lib().spmv_csr_run(self._h, variant, _ptr(x), _ptr(y), _stream_handle(stream)))

    def run_vals16(self, variant: int, vals16, x, y, stream=None) -> None:
        """Enqueue y = A x with the values of A read from ``vals16`` (spmv_csr_run_vals16): a 1-D contiguous bfloat16 or
        float16 device tensor of nnz elements in the handle's storage order, borrowed and read live.  x, y: float32 device
        tensors; every sum is the fp32 call's on the widened values.  SPMV_TILED, SPMV_ADAPTIVE, or SPMV_AUTO resolved to tiled."""
        import torch
        if not isinstance(vals16, torch.Tensor) or vals16.dim() != 1 or not vals16.is_contiguous() or vals16.numel() != self.nnz:
            raise ValueError(f"run_vals16: vals16 must be a contiguous 1-D tensor of nnz = {self.nnz} elements")
        dtype = self._dense_dtype("run_vals16", vals16=vals16.view(vals16.numel(), 1))
        if dtype == ATTN_FP32:
            raise ValueError("run_vals16: vals16 must be bfloat16 or float16 (float32 values are the handle's own: run)")
        assert x.numel() >= self.cols and y.numel() >= self.rows
        check(lib().spmv_csr_run_vals16(self._h, variant, dtype, _ptr(vals16), _ptr(x), _ptr(y), _stream_handle(stream)))

    def column_range(self, stream=None):
        """(smallest, largest) column index referenced; (cols, -1) for a matrix without nonzeros."""
        lo, hi = C.c_int64(), C.c_int64()
        check(lib().spmv_csr_column_range(self._h, C.byref(lo), C.byref(hi), _stream_handle(stream)))
        return lo.value, hi.value

    # -- the transpose (spmv_csr_transpose) ------------------------------------------------------------------------
    def transpose(self, keep_map: bool = False, stream=None) -> "CsrMatrix":
        """A^T as a new handle that owns its arrays, built on the device (waits for the stream).  Row j lists the
        nonzeros of column j in this matrix's storage order.  ``keep_map=True`` keeps the 4-byte-per-nonzero map that
        :meth:`transpose_values` needs."""
        h = C.c_void_p()
        check(lib().spmv_csr_transpose(self._h, 1 if keep_map else 0, _stream_handle(stream), C.byref(h)))
        return CsrMatrix(h.value)

    def transpose_values(self, a: "CsrMatrix", stream=None) -> None:
        """Refresh this handle's values (made by ``a.transpose(keep_map=True)``) from ``a``'s values as they are now:
        one gather launch, asynchronous, graph-capturable; then what :meth:`values_changed` does."""
        check(lib().spmv_csr_transpose_values(self._h, a._h, _stream_handle(stream)))

    def transpose_gather(self, src, dst, stream=None) -> None:
        """On a handle made by ``a.transpose(keep_map=True)``: ``dst[..., i] = src[..., map[i]]``, arrays of nnz 32-bit elements
        in ``a``'s storage order brought into this handle's (the bias of the _bias attention calls for backward_kv).  src, dst:
        (nnz,) or (count, nnz) of one 4-byte dtype with stride(-1) == 1; copied as bits, in one launch."""
        self._move("transpose_gather", lib().spmv_csr_transpose_gather, src, dst, self.nnz, self.nnz, stream)

    def transpose_map_bytes(self) -> int:
        return self._bytes(lib().spmv_csr_transpose_map_bytes)

    # -- selection (spmv_csr_select_*) ------------------------------------------------------------------------------
    SELECT_ABS = 1      # SPMV_SELECT_ABS

    def _select_score(self, who: str, score):
        import torch
        if score is None:
            return None
        if not isinstance(score, torch.Tensor) or score.dtype != torch.float32 or score.dim() != 1 \
                or not score.is_contiguous() or score.numel() != self.nnz or not score.is_cuda:
            raise ValueError(f"{who}: score must be a contiguous 1-D float32 device tensor of nnz = {self.nnz} elements")
        return score

    def _selected(self, h) -> "CsrMatrix":
        s = CsrMatrix(h.value)
        s.select_parent_nnz = self.nnz
        return s

    def select_topk(self, k: int, score=None, abs: bool = False, keep_map: bool = False, stream=None) -> "CsrMatrix":
        """Per row the ``min(k, len)`` nonzeros of the largest ``score`` (``None``: this matrix's own values; ``abs``: by
        ``|score|``), ties to the earlier storage position, as a new handle that owns its arrays (waits for the stream).
        Rows keep their storage order.  ``keep_map=True`` keeps the map :meth:`select_values`, :meth:`select_gather` and
        :meth:`select_scatter` need."""
        if isinstance(k, bool) or not isinstance(k, int) or k < 1:
            raise ValueError(f"select_topk: k = {k!r} (an int >= 1)")
        score = self._select_score("select_topk", score)
        h = C.c_void_p()
        check(lib().spmv_csr_select_topk(self._h, _ptr(score), min(k, 2 ** 31 - 1), self.SELECT_ABS if abs else 0,
                                         1 if keep_map else 0, _stream_handle(stream), C.byref(h)))
        return self._selected(h)

    def select_threshold(self, threshold: float, score=None, abs: bool = False, keep_map: bool = False, stream=None) -> "CsrMatrix":
        """The nonzeros with ``score >= threshold`` (``abs``: ``|score| >= threshold``; a NaN score is never kept) as a new
        handle that owns its arrays (waits for the stream).  The arguments are those of :meth:`select_topk`."""
        threshold = float(threshold)
        if threshold != threshold:
            raise ValueError("select_threshold: the threshold is a NaN")
        score = self._select_score("select_threshold", score)
        h = C.c_void_p()
        check(lib().spmv_csr_select_threshold(self._h, _ptr(score), threshold, self.SELECT_ABS if abs else 0,
                                              1 if keep_map else 0, _stream_handle(stream), C.byref(h)))
        return self._selected(h)

    def select_values(self, a: "CsrMatrix", stream=None) -> None:
        """Refresh this handle's values (made by ``a.select_*(keep_map=True)``) from ``a``'s values as they are now: one
        gather launch, asynchronous, graph-capturable; then what :meth:`values_changed` does."""
        check(lib().spmv_csr_select_values(self._h, a._h, _stream_handle(stream)))

    def _move(self, who: str, fn, src, dst, n_src: int, n_dst: int, stream) -> None:
        """The strided move fn of a derived handle: src (n_src,) or (count, n_src), dst the same over n_dst."""
        import torch
        for name, t, n in (("src", src, n_src), ("dst", dst, n_dst)):
            if not isinstance(t, torch.Tensor) or t.dim() not in (1, 2) or t.element_size() != 4 or t.stride(-1) != 1 \
                    or t.shape[-1] != n or not t.is_cuda:
                raise ValueError(f"{who}: {name} must be a device tensor ({n},) or (count, {n}) of 4-byte elements with stride(-1) == 1")
        if src.dtype != dst.dtype or src.dim() != dst.dim() or src.shape[:-1] != dst.shape[:-1] or src.device != dst.device:
            raise ValueError(f"{who}: src is {src.dtype} {tuple(src.shape)} on {src.device}, dst {dst.dtype} {tuple(dst.shape)} on {dst.device}")
        count = src.shape[0] if src.dim() == 2 else 1
        if count < 1:
            raise ValueError(f"{who}: count = 0")
        stride = lambda t: t.stride(0) if count > 1 else 0
        check(fn(self._h, count, _ptr(src), stride(src), _ptr(dst), stride(dst), _stream_handle(stream)))

    def _parent_nnz(self, who: str) -> int:
        n = getattr(self, "select_parent_nnz", None)
        if n is None:
            raise ValueError(f"{who}: this handle was not made by select_topk / select_threshold")
        return n

    def select_gather(self, src, dst, stream=None) -> None:
        """On a handle made by ``a.select_*(keep_map=True)``: ``dst[..., m] = src[..., map[m]]`` -- arrays of 32-bit elements in
        ``a``'s storage order (``a.nnz`` each) brought into this handle's (``nnz`` each).  src, dst: 1-D or (count, n) of one
        4-byte dtype with stride(-1) == 1; copied as bits, in one launch."""
        self._move("select_gather", lib().spmv_csr_select_gather, src, dst, self._parent_nnz("select_gather"), self.nnz, stream)

    def select_scatter(self, src, dst, stream=None) -> None:
        """The other way: ``dst[..., map[m]] = src[..., m]``; every other element of dst is left as it is (zero-fill dst first
        for a dense gradient in the parent's order)."""
        self._move("select_scatter", lib().spmv_csr_select_scatter, src, dst, self.nnz, self._parent_nnz("select_scatter"), stream)

    def _bytes(self, fn) -> int:
        """What a _map_bytes / _plan_bytes call answers (below 0: a status)."""
        n = fn(self._h)
        if n < 0:
            check(n)
        return n

    def select_map_bytes(self) -> int:
        return self._bytes(lib().spmv_csr_select_map_bytes)

    def copy_arrays(self, row_ptr, col_idx, vals=None, stream=None) -> None:
        """Device-to-device copies of this handle's arrays into the caller's contiguous device tensors (int32 of rows + 1,
        int32 of nnz, float32 of nnz; any may be ``None``), enqueued on the stream: how an owned pattern reaches tensors that
        another handle or a layer borrows."""
        import torch
        for name, t, dt, n in (("row_ptr", row_ptr, torch.int32, self.rows + 1), ("col_idx", col_idx, torch.int32, self.nnz),
                               ("vals", vals, torch.float32, self.nnz)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1 or not t.is_contiguous() or t.numel() != n \
                    or not t.is_cuda:
                raise ValueError(f"copy_arrays: {name} must be a contiguous 1-D {dt} device tensor of {n} elements")
        check(lib().spmv_csr_copy_arrays(self._h, _ptr(row_ptr), _ptr(col_idx), _ptr(vals), _stream_handle(stream)))

    # -- the sparse product (spmv_csr_spgemm) ------------------------------------------------------------------------
    def spgemm(self, b: "CsrMatrix", keep_plan: bool = False, stream=None) -> "CsrMatrix":
        """``self @ b`` as a new handle that owns its arrays (waits for the stream): rows sorted and duplicate-free, the
        pattern structural, every value one fma chain over its terms in storage order.  ``keep_plan=True`` keeps the row lists
        :meth:`spgemm_values` needs.  The result's ``spgemm_products`` is the number of terms."""
        if not isinstance(b, CsrMatrix):
            raise TypeError("spgemm: b must be a CsrMatrix")
        if self.cols != b.rows:
            raise ValueError(f"spgemm: self is {self.rows} x {self.cols}, b is {b.rows} x {b.cols}")
        h, products = C.c_void_p(), C.c_int64(-1)
        check(lib().spmv_csr_spgemm(self._h, b._h, 1 if keep_plan else 0, _stream_handle(stream), C.byref(h), C.byref(products)))
        c = CsrMatrix(h.value)
        c.spgemm_products = products.value
        return c

    def spgemm_values(self, a: "CsrMatrix", b: "CsrMatrix", stream=None) -> None:
        """Recompute this handle's values (made by ``a.spgemm(b, keep_plan=True)``) from the values ``a`` and ``b`` hold now: the
        numeric pass alone, asynchronous, graph-capturable; then what :meth:`values_changed` does."""
        check(lib().spmv_csr_spgemm_values(self._h, a._h, b._h, _stream_handle(stream)))

    def spgemm_plan_bytes(self) -> int:
        return self._bytes(lib().spmv_csr_spgemm_plan_bytes)

    # -- the sparse sum (spmv_csr_add) ------------------------------------------------------------------------------
    def add(self, b: "CsrMatrix", alpha: float = 1.0, beta: float = 1.0, op="union", keep_plan: bool = False, stream=None) -> "CsrMatrix":
        """``alpha * self + beta * b`` on the union, the intersection or the difference (``op``: "union" | "intersect" | "minus"
        or an ``ADD_*`` constant) of the two patterns, as a new handle that owns its arrays (waits for the stream): rows sorted
        and duplicate-free, the pattern structural, every value one chain over ``self``'s terms and then ``b``'s in storage order;
        a side whose coefficient is 0 gives its pattern and no terms.  ``keep_plan=True`` keeps the terms :meth:`add_values` and
        :meth:`add_gather` need."""
        if not isinstance(b, CsrMatrix):
            raise TypeError("add: b must be a CsrMatrix")
        if (self.rows, self.cols) != (b.rows, b.cols):
            raise ValueError(f"add: self is {self.rows} x {self.cols}, b is {b.rows} x {b.cols}")
        if isinstance(op, str):
            if op not in _ADD_OPS:
                raise ValueError(f"add: op = {op!r} (one of {sorted(_ADD_OPS)})")
            op = _ADD_OPS[op]
        if isinstance(op, bool) or not isinstance(op, int):
            raise ValueError(f"add: op = {op!r}")
        h = C.c_void_p()
        check(lib().spmv_csr_add(self._h, b._h, float(alpha), float(beta), op, 1 if keep_plan else 0, _stream_handle(stream), C.byref(h)))
        c = CsrMatrix(h.value)
        c.add_parent_nnz = (self.nnz, b.nnz)
        return c

    def add_values(self, a: "CsrMatrix", b: "CsrMatrix", alpha: float = 1.0, beta: float = 1.0, stream=None) -> None:
        """Recompute this handle's values (made by ``a.add(b, ..., keep_plan=True)``) from the values ``a`` and ``b`` hold now with
        the coefficients given now: one launch, asynchronous, graph-capturable; then what :meth:`values_changed` does."""
        if not isinstance(a, CsrMatrix) or not isinstance(b, CsrMatrix):
            raise TypeError("add_values: a and b must be CsrMatrix")
        check(lib().spmv_csr_add_values(self._h, a._h, b._h, float(alpha), float(beta), _stream_handle(stream)))

    def add_gather(self, side: int, src, dst, stream=None) -> None:
        """On a handle made by ``a.add(b, ..., keep_plan=True)``: ``dst[..., p] = src[..., e]`` for every kept term at storage
        position p of ``side`` (0: a, 1: b) whose entry of this handle is e; every other element of dst is left as it is.  src:
        (nnz,) or (count, nnz) in this handle's order, dst: the same over that side's nnz; one 4-byte dtype, stride(-1) == 1."""
        if isinstance(side, bool) or side not in (0, 1):
            raise ValueError(f"add_gather: side = {side!r} (0: a, 1: b)")
        n = getattr(self, "add_parent_nnz", None)
        if n is None:
            raise ValueError("add_gather: this handle was not made by add")
        self._move("add_gather", lambda h, *rest: lib().spmv_csr_add_gather(h, side, *rest), src, dst, self.nnz, n[side], stream)

    def add_plan_bytes(self) -> int:
        return self._bytes(lib().spmv_csr_add_plan_bytes)

    # -- the triangular solve (spmv_csr_trsv) ----------------------------------------------------------------------
    @staticmethod
    def _trsv_uplo(what: str, uplo) -> int:
        if isinstance(uplo, str):
            if uplo not in _TRSV_UPLO:
                raise ValueError(f"{what}: uplo = {uplo!r} (one of {sorted(_TRSV_UPLO)})")
            return _TRSV_UPLO[uplo]
        if isinstance(uplo, bool) or not isinstance(uplo, int):
            raise ValueError(f"{what}: uplo = {uplo!r}")
        return uplo

    def trsv_plan(self, uplo="lower", thin_rows: int = 0, stream=None) -> None:
        """Analyse one triangle (``uplo``: "lower" | "upper" or a ``TRSV_*`` constant) for :meth:`trsv`: the rows by level, on
        the device (waits for the stream).  Levels of at most ``thin_rows`` rows (0: the library's default) are merged into
        launches of one workgroup.  The plan depends on the pattern alone; planning again replaces it."""
        uplo = self._trsv_uplo("trsv_plan", uplo)
        if isinstance(thin_rows, bool) or not isinstance(thin_rows, int):
            raise ValueError(f"trsv_plan: thin_rows = {thin_rows!r}")
        check(lib().spmv_csr_trsv_plan(self._h, uplo, thin_rows, _stream_handle(stream)))

    def trsv(self, b, x=None, uplo="lower", unit: bool = False, stream=None):
        """Enqueue ``x = T^-1 b`` for the planned triangle T of this (square) matrix; entries of the other triangle are never
        read.  b, x: contiguous float32 device tensors of ``rows`` elements; ``x`` None makes a new one, ``x is b`` solves in
        place.  ``unit=True`` ignores the stored diagonal.  Asynchronous, allocates nothing in the library: graph-capturable.
        Returns x."""
        import torch
        uplo = self._trsv_uplo("trsv", uplo)
        if not isinstance(unit, (bool, int)):
            raise ValueError(f"trsv: unit = {unit!r}")
        if x is None:
            x = torch.empty_like(b)
        for name, t in (("b", b), ("x", x)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or t.numel() < self.rows:
                raise ValueError(f"trsv: {name} must be a contiguous 1-D float32 tensor of at least rows = {self.rows} elements")
        check(lib().spmv_csr_trsv(self._h, uplo, TRSV_UNIT if unit else TRSV_NON_UNIT, _ptr(b), _ptr(x), _stream_handle(stream)))
        return x

    def trsv_plan_bytes(self, uplo="lower") -> int:
        n = lib().spmv_csr_trsv_plan_bytes(self._h, self._trsv_uplo("trsv_plan_bytes", uplo))
        if n < 0:
            check(n)
        return n

    def trsv_plan_info(self, uplo="lower") -> dict:
        """levels, launches of one solve, rows of the widest level, rows of more than SPMV_TRSV_SERIAL_MAX terms, the first row
        whose diagonal is missing or repeated (-1: none), the thin threshold and the cap of levels per merged launch."""
        info = (C.c_int64 * 8)()
        check(lib().spmv_csr_trsv_plan_info(self._h, self._trsv_uplo("trsv_plan_info", uplo), info))
        keys = ("levels", "launches", "widest", "long_rows", "bad_diag_row", "thin_rows", "level_cap")
        return dict(zip(keys, (int(v) for v in info)))

    def trsv_plan_rows(self, uplo="lower"):
        """(level_ptr, order) as numpy int32 arrays: the rows by (level, row) ascending and where every level starts."""
        import numpy as np
        u = self._trsv_uplo("trsv_plan_rows", uplo)
        levels = self.trsv_plan_info(u)["levels"]
        level_ptr, order = np.empty(levels + 1, np.int32), np.empty(self.rows, np.int32)
        check(lib().spmv_csr_trsv_plan_rows(self._h, u, _ptr(level_ptr), _ptr(order)))
        return level_ptr, order

    def trsv_describe(self, uplo="lower") -> str:
        buf = C.create_string_buffer(256)
        check(lib().spmv_csr_trsv_describe(self._h, self._trsv_uplo("trsv_describe", uplo), buf, len(buf)))
        return buf.value.decode()

    # -- the incomplete factorisation (spmv_csr_ilu0) ----------------------------------------------------------------
    def ilu0(self, thin_rows: int = 0, stream=None) -> "CsrMatrix":
        """M = ILU(0) of this (square) matrix as a new handle that owns its arrays, built on the device (waits for the stream):
        this matrix's pattern, L (unit lower) and U (upper) in one handle, with both ``trsv`` plans made with ``thin_rows`` (0:
        the library's default).  Every row must be strictly ascending and store its diagonal (``add`` with an empty matrix sorts,
        ``add`` with I gives a diagonal).  The values are the contract of include/spmv_hip.h, bit for bit."""
        if isinstance(thin_rows, bool) or not isinstance(thin_rows, int):
            raise ValueError(f"ilu0: thin_rows = {thin_rows!r}")
        h = C.c_void_p()
        check(lib().spmv_csr_ilu0(self._h, thin_rows, _stream_handle(stream), C.byref(h)))
        return CsrMatrix(h.value)

    def ilu0_values(self, a: "CsrMatrix", stream=None) -> None:
        """Factor again (this handle was made by ``a.ilu0()``) from the values ``a`` holds now, the pattern unchanged:
        asynchronous, allocates nothing, graph-capturable; then what :meth:`values_changed` does."""
        if not isinstance(a, CsrMatrix):
            raise TypeError("ilu0_values: a must be a CsrMatrix")
        check(lib().spmv_csr_ilu0_values(self._h, a._h, _stream_handle(stream)))

    def ilu0_solve(self, r, z=None, stream=None):
        """Enqueue ``z = U^-1 (L^-1 r)`` on a factor handle: ``trsv`` lower / unit, then upper / non-unit in place.  r, z:
        contiguous float32 device tensors of ``rows`` elements; ``z`` None makes a new one, ``z is r`` solves in place.
        Asynchronous, allocates nothing in the library: graph-capturable.  Returns z."""
        import torch
        if z is None:
            z = torch.empty_like(r)
        for name, t in (("r", r), ("z", z)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.dim() != 1 or not t.is_contiguous() or t.numel() < self.rows:
                raise ValueError(f"ilu0_solve: {name} must be a contiguous 1-D float32 tensor of at least rows = {self.rows} elements")
        check(lib().spmv_csr_ilu0_solve(self._h, _ptr(r), _ptr(z), _stream_handle(stream)))
        return z

    def ilu0_pivot(self, stream=None) -> int:
        """The smallest row whose pivot u_ii is +-0 or not finite after the last factorisation, -1: none (waits for the stream)."""
        row = C.c_int64(-2)
        check(lib().spmv_csr_ilu0_pivot(self._h, _stream_handle(stream), C.byref(row)))
        return row.value

    def ilu0_plan_bytes(self) -> int:
        n = lib().spmv_csr_ilu0_plan_bytes(self._h)
        if n < 0:
            check(n)
        return n

    # -- the multicolour ordering (spmv_csr_color, spmv_csr_permute) -------------------------------------------------
    _COLOR_INFO = ("colors", "rounds", "launches", "largest", "smallest", "sweep_entries", "peak_bytes")

    def color(self, seed: int = 0, stream=None):
        """``(color, perm, color_ptr, info)`` of this (square) matrix's symmetrised pattern: the greedy colouring in descending
        order of ``fmix32(row ^ seed)`` (include/spmv_hip.h "the multicolour ordering", bit for bit).  ``color`` and ``perm`` are
        int32 device tensors of ``rows`` elements -- ``perm`` lists the rows by (colour, row) -- ``color_ptr`` a numpy int32
        array of colours + 1 entries (where every colour starts in ``perm``) and ``info`` a dict of the call's counts.  Waits
        for the stream."""
        import numpy as np
        import torch
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 32:
            raise ValueError(f"color: seed = {seed!r}")
        dev = torch.device("cuda", torch.cuda.current_device())
        color = torch.empty(max(self.rows, 1), dtype=torch.int32, device=dev)                   # (never a null pointer)
        perm = torch.empty(max(self.rows, 1), dtype=torch.int32, device=dev)
        info = (C.c_int64 * 8)()
        cap = 64
        while True:
            color_ptr = np.zeros(cap, np.int32)
            check(lib().spmv_csr_color(self._h, seed, _stream_handle(stream), _ptr(color), _ptr(perm), _ptr(color_ptr), cap, info))
            if info[0] + 1 <= cap:
                break
            cap = int(info[0]) + 1                             # the second call: cap was too small
        return color[:self.rows], perm[:self.rows], color_ptr[:int(info[0]) + 1].copy(), dict(zip(self._COLOR_INFO, (int(v) for v in info)))

    @staticmethod
    def _permutation(who: str, name: str, perm, n: int):
        import torch
        if perm is None:
            return None
        if not isinstance(perm, torch.Tensor) or perm.dtype != torch.int32 or perm.dim() != 1 or not perm.is_contiguous() \
                or perm.numel() != n or not perm.is_cuda:
            raise ValueError(f"{who}: {name} must be a contiguous 1-D int32 device tensor of {n} elements")
        return perm

    def permute(self, row_perm=None, col_perm=None, keep_map: bool = False, via_transpose: bool = False, stream=None) -> "CsrMatrix":
        """B = P A Q^T as a new handle that owns its arrays (waits for the stream): row r of B is row ``row_perm[r]`` of this
        matrix, an entry in column j lands in the column c with ``col_perm[c] == j`` (None: the identity), and every row of B
        ascends by (new column, storage position here).  ``keep_map=True`` keeps the 4-byte-per-nonzero map that
        :meth:`permute_values` and :meth:`permute_gather` need; ``via_transpose=True`` forces the route through two transposes
        (the same bytes).  An array that is no permutation is refused with the first offending index."""
        row_perm = self._permutation("permute", "row_perm", row_perm, self.rows)
        col_perm = self._permutation("permute", "col_perm", col_perm, self.cols)
        flags = (PERMUTE_KEEP_MAP if keep_map else 0) | (PERMUTE_VIA_TRANSPOSE if via_transpose else 0)
        h = C.c_void_p()
        check(lib().spmv_csr_permute(self._h, _ptr(row_perm), _ptr(col_perm), flags, _stream_handle(stream), C.byref(h)))
        return CsrMatrix(h.value)

    def permute_values(self, a: "CsrMatrix", stream=None) -> None:
        """Refresh this handle's values (made by ``a.permute(..., keep_map=True)``) from ``a``'s values as they are now: one
        gather launch, asynchronous, graph-capturable; then what :meth:`values_changed` does."""
        if not isinstance(a, CsrMatrix):
            raise TypeError("permute_values: a must be a CsrMatrix")
        check(lib().spmv_csr_permute_values(self._h, a._h, _stream_handle(stream)))

    def permute_gather(self, src, dst=None, stream=None):
        """On a handle made by ``a.permute(..., keep_map=True)``: ``dst[..., i] = src[..., map[i]]``, arrays of nnz 32-bit
        elements in ``a``'s storage order brought into this handle's.  src, dst: (nnz,) or (count, nnz) of one 4-byte dtype with
        stride(-1) == 1 (``dst`` None makes a new one); copied as bits, in one launch.  Returns dst."""
        import torch
        if dst is None and isinstance(src, torch.Tensor):
            dst = torch.empty_like(src)
        self._move("permute_gather", lib().spmv_csr_permute_gather, src, dst, self.nnz, self.nnz, stream)
        return dst

    def permute_map_bytes(self) -> int:
        return self._bytes(lib().spmv_csr_permute_map_bytes)

    # -- SpMM: k right-hand sides at once (spmv_csr_spmm) ---------------------------------------------------------
    def spmm_plan(self, stream=None) -> None:
        """The plan of spmv_csr_spmm (a function of row_ptr; reads it back and waits for the stream once)."""
        check(lib().spmv_csr_spmm_plan(self._h, _stream_handle(stream)))

    @staticmethod
    def _dense_dtype(what: str, **matrices) -> int:
        """The ATTN_* dtype of a call's dense matrices: 2-D tensors with stride(1) == 1, all float32, all bfloat16 or all
        float16 (the first decides; any other dtype, or a partner of another one, is a ValueError that names the matrix)."""
        import torch
        codes = {torch.float32: ATTN_FP32, torch.bfloat16: ATTN_BF16, torch.float16: ATTN_FP16}
        first = next(iter(matrices.values()))
        want = first.dtype if isinstance(first, torch.Tensor) and first.dtype in codes else torch.float32
        for name, t in matrices.items():
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != want or t.stride(1) != 1:
                kind = "float32" if want == torch.float32 else f"{want} (as {next(iter(matrices))})"
                raise ValueError(f"{what}: {name} must be a 2-D {kind} tensor with stride(1) == 1")
        return codes[want]

    def _spmm(self, what: str, X, Y, stream) -> None:
        """spmm and spmm_cols (`what`): their checks, then the C call of `what` and the matrices' dtype."""
        dtype = self._dense_dtype(what, X=X, Y=Y)
        k = X.shape[1]
        if X.shape[0] != self.cols or Y.shape[0] != self.rows or Y.shape[1] < k:
            raise ValueError(f"{what}: X {tuple(X.shape)} and Y {tuple(Y.shape)} do not fit a {self.rows} x {self.cols} matrix")
        call, head = _PRODUCT_CALLS[what, dtype]
        check(getattr(lib(), call)(self._h, *head, k, _ptr(X), X.stride(0), _ptr(Y), Y.stride(0), _stream_handle(stream)))

    def spmm(self, X, Y, stream=None) -> None:
        """Enqueue Y[:, :k] = A X with k = X.shape[1].  X: (cols, k) and Y: (rows, k or more) 2-D device tensors with
        stride(1) == 1, both float32 (spmv_csr_spmm) or both bfloat16 or float16 (spmv_csr_spmm_16: fp32 values and sums,
        Y rounded once at its store); the leading dimensions are their stride(0), in elements.  Y's columns from k on are
        not written."""
        self._spmm("spmm", X, Y, stream)

    def spmm_describe(self) -> str:
        buf = C.create_string_buffer(256)
        check(lib().spmv_csr_spmm_describe(self._h, buf, 256))
        return buf.value.decode()

    def spmm_plan_bytes(self) -> int:
        n = lib().spmv_csr_spmm_plan_bytes(self._h)
        if n < 0:
            check(n)
        return n

    # -- SDDMM: U X^T sampled at the pattern (spmv_csr_sddmm; the plan is spmm_plan's) ------------------------------
    def _sddmm(self, what: str, U, X, out, stream) -> None:
        """sddmm and sddmm_cols (`what`): their checks, then the C call of `what` and the matrices' dtype."""
        import torch
        dtype = self._dense_dtype(what, U=U, X=X)
        if not isinstance(out, torch.Tensor) or out.dim() != 1 or out.dtype != torch.float32 or not out.is_contiguous():
            raise ValueError(f"{what}: out must be a contiguous 1-D float32 tensor")
        k = U.shape[1]
        if U.shape[0] != self.rows or X.shape[0] != self.cols or X.shape[1] != k or out.shape[0] != self.nnz:
            raise ValueError(f"{what}: U {tuple(U.shape)}, X {tuple(X.shape)} and out {tuple(out.shape)} do not fit a "
                             f"{self.rows} x {self.cols} matrix with {self.nnz} nonzeros")
        call, head = _PRODUCT_CALLS[what, dtype]
        check(getattr(lib(), call)(self._h, *head, k, _ptr(U), U.stride(0), _ptr(X), X.stride(0), _ptr(out), _stream_handle(stream)))

    def sddmm(self, U, X, out, stream=None) -> None:
        """Enqueue out[n] = U[row(n), :k] . X[col(n), :k] for every stored nonzero n, k = U.shape[1] = X.shape[1].
        U: (rows, k) and X: (cols, k) 2-D device tensors with stride(1) == 1, both float32 (spmv_csr_sddmm) or both
        bfloat16 or float16 (spmv_csr_sddmm_16: widened exactly, the fp32 call's sums); the leading dimensions are their
        stride(0), in elements; out: nnz float32 whatever U and X are, contiguous, in this matrix's storage order."""
        self._sddmm("sddmm", U, X, out, stream)

    # -- both products at any k, in column tiles of 64 (spmv_csr_spmm_cols, spmv_csr_sddmm_cols) --------------------------
    def spmm_plan_cols(self, k_max: int, stream=None) -> None:
        """spmm_plan() and the scratch of the long rows' partials for spmm_cols at up to k_max columns (it only grows).  Both
        _cols calls need it to cover their k."""
        check(lib().spmv_csr_spmm_plan_cols(self._h, k_max, _stream_handle(stream)))

    def spmm_cols(self, X, Y, stream=None) -> None:
        """spmm(X, Y) for any k = X.shape[1] up to COLS_MAX_K in one call: every column's bits are the narrow call's."""
        self._spmm("spmm_cols", X, Y, stream)

    def sddmm_cols(self, U, X, out, stream=None) -> None:
        """sddmm(U, X, out) for any k up to COLS_MAX_K in one call: per column tile of 64 the narrow call's number, the tiles'
        numbers added in fp32 in tile order from tile 0's."""
        self._sddmm("sddmm_cols", U, X, out, stream)

    # -- row softmax over the pattern and its backward (spmv_csr_row_softmax; the plan is spmm_plan's) ---------------
    def _nnz_arrays(self, what: str, **arrays) -> None:
        import torch
        for name, t in arrays.items():
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != torch.float32 or not t.is_contiguous():
                raise ValueError(f"{what}: {name} must be a contiguous 1-D float32 tensor")
            if t.shape[0] != self.nnz:
                raise ValueError(f"{what}: {name} holds {t.shape[0]} floats, the matrix has {self.nnz} nonzeros")

    def row_softmax(self, scores, out, scale: float = 1.0, stream=None) -> None:
        """Enqueue out = softmax of scale * scores over every row of the pattern (nnz float32 each, in this matrix's
        storage order; ``out`` may be ``scores``).  An empty row writes nothing."""
        import math
        self._nnz_arrays("row_softmax", scores=scores, out=out)
        if not math.isfinite(scale):
            raise ValueError(f"row_softmax: scale = {scale} is not finite")
        check(lib().spmv_csr_row_softmax(self._h, scale, _ptr(scores), _ptr(out), _stream_handle(stream)))

    def row_softmax_backward(self, P, dP, dS, scale: float = 1.0, stream=None) -> None:
        """Enqueue dS[n] = scale * P[n] * (dP[n] - sum over the row of P dP) (``dS`` may be ``P`` or ``dP``)."""
        import math
        self._nnz_arrays("row_softmax_backward", P=P, dP=dP, dS=dS)
        if not math.isfinite(scale):
            raise ValueError(f"row_softmax_backward: scale = {scale} is not finite")
        check(lib().spmv_csr_row_softmax_backward(self._h, scale, _ptr(P), _ptr(dP), _ptr(dS), _stream_handle(stream)))

    # -- fused attention (spmv_csr_attention_*; no array of nnz floats) ---------------------------------------------
    def attention_plan(self, stream=None) -> None:
        """The SpMM plan if it is missing, and the scratch of the long rows' pieces (waits for the stream once)."""
        check(lib().spmv_csr_attention_plan(self._h, _stream_handle(stream)))

    def attention_plan_bytes(self) -> int:
        n = lib().spmv_csr_attention_plan_bytes(self._h)
        if n < 0:
            check(n)
        return n

    @staticmethod
    def _attention_operands(what: str, scale: float, _dtype=None, **mats) -> None:
        """Every matrix as (tensor, rows, width or None): 2-D float32 (or the call's 16-bit `_dtype`) with stride(1) == 1 (its
        ld is stride(0))."""
        import math
        import torch
        dtype, dname = _dtype or torch.float32, str(_dtype or torch.float32).replace("torch.", "")
        if not math.isfinite(scale):
            raise ValueError(f"{what}: scale = {scale} is not finite")
        for name, (t, n, w) in mats.items():
            if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype != dtype or t.stride(1) != 1:
                raise ValueError(f"{what}: {name} must be a 2-D {dname} tensor with stride(1) == 1")
            if t.shape[0] != n or (w is not None and t.shape[1] != w):
                raise ValueError(f"{what}: {name} is {tuple(t.shape)}, expected ({n}, {w if w is not None else 'width'})")

    @staticmethod
    def _attention_vectors(what: str, **vecs) -> None:
        import torch
        for name, (t, n) in vecs.items():
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
                raise ValueError(f"{what}: {name} must be a contiguous float32 tensor of {n} elements")

    def attention_forward(self, Q, K, V, O, stats, scale: float = 1.0, stream=None) -> None:
        """Enqueue O = softmax_rows(scale * Q K^T at the pattern) V and stats = (row maximum, 1 / row sum) per query.
        Q: (rows, k), K: (cols, k), V: (cols, kv), O: (rows, kv), stats: (rows, 2)."""
        self._attention_call("forward", "one", (Q, K, V, O, stats), scale, stream)

    def attention_backward_q(self, Q, K, V, O, dO, stats, delta, dQ, scale: float = 1.0, stream=None) -> None:
        """Enqueue delta[i] = dO[i] . O[i] and dQ; reads the forward call's O and stats.  delta: rows floats, dQ: (rows, k)."""
        self._attention_call("backward_q", "one", (Q, K, V, O, dO, stats, delta, dQ), scale, stream)

    def attention_backward_kv(self, Q, K, V, dO, stats, delta, dK, dV, scale: float = 1.0, stream=None) -> None:
        """On the handle of the TRANSPOSED pattern (rows = keys, cols = queries): enqueue dK and dV from the forward call's
        stats and backward_q's delta.  Q, dO: (cols, .), K, V, dK, dV: (rows, .)."""
        self._attention_call("backward_kv", "one", (Q, K, V, dO, stats, delta, dK, dV), scale, stream)

    # -- fused attention, the heads of one pattern in one launch (spmv_csr_attention_*_heads) -----------------------------
    def attention_plan_heads(self, heads: int, stream=None) -> None:
        """The attention plan with the long rows' scratch sized for ``heads`` heads (it only grows; waits for the stream)."""
        check(lib().spmv_csr_attention_plan_heads(self._h, heads, _stream_handle(stream)))

    def attention_max_heads(self, k: int, kv: int) -> int:
        """The most heads one _heads call on this handle takes at these widths (the library's launch limits)."""
        n = lib().spmv_csr_attention_max_heads(self._h, k, kv)
        if n < 0:
            check(n)
        return n

    @staticmethod
    def _attention_heads(what: str, scale: float, mats: dict, vecs: dict, _dtype=None):
        """Every matrix as (tensor, rows, width or None): (heads, rows, width) float32 (or the call's 16-bit `_dtype`) with
        stride(2) == 1, its ld stride(1) and its head stride stride(0); stats (heads, rows, 2) with strides (., 2, 1), delta
        (heads, rows) with stride(1) == 1, both float32 always.  Returns the number of heads."""
        import math
        import torch
        dtype, dname = _dtype or torch.float32, str(_dtype or torch.float32).replace("torch.", "")
        if not math.isfinite(scale):
            raise ValueError(f"{what}: scale = {scale} is not finite")
        heads = None
        for name, (t, n, w) in mats.items():
            if not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype != dtype or t.stride(2) != 1:
                raise ValueError(f"{what}: {name} must be a (heads, rows, width) {dname} tensor with stride(2) == 1")
            heads = t.shape[0] if heads is None else heads
            if t.shape[0] != heads or t.shape[1] != n or (w is not None and t.shape[2] != w):
                raise ValueError(f"{what}: {name} is {tuple(t.shape)}, expected ({heads}, {n}, {w if w is not None else 'width'})")
        for name, (t, n, inner) in vecs.items():
            shape = (heads, n) + ((inner,) if inner > 1 else ())
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or tuple(t.shape) != shape \
                    or not t[0].is_contiguous():
                raise ValueError(f"{what}: {name} must be a float32 tensor of shape {shape} whose heads are contiguous")
        return heads

    def attention_forward_heads(self, Q, K, V, O, stats, scale: float = 1.0, stream=None) -> None:
        """attention_forward for all heads in one launch per kernel.  Q: (heads, rows, k), K: (heads, cols, k), V: (heads,
        cols, kv), O: (heads, rows, kv), stats: (heads, rows, 2); an input may have stride(0) == 0 (shared by the heads)."""
        self._attention_call("forward", "heads", (Q, K, V, O, stats), scale, stream)

    def attention_backward_q_heads(self, Q, K, V, O, dO, stats, delta, dQ, scale: float = 1.0, stream=None) -> None:
        """attention_backward_q for all heads in one launch per kernel; delta: (heads, rows), dQ: (heads, rows, k)."""
        self._attention_call("backward_q", "heads", (Q, K, V, O, dO, stats, delta, dQ), scale, stream)

    def attention_backward_kv_heads(self, Q, K, V, dO, stats, delta, dK, dV, scale: float = 1.0, stream=None) -> None:
        """On the handle of the TRANSPOSED pattern: attention_backward_kv for all heads in one launch per kernel.  With a
        shared K or V (stride(0) == 0) dK and dV still come out per head."""
        self._attention_call("backward_kv", "heads", (Q, K, V, dO, stats, delta, dK, dV), scale, stream)

    # -- fused attention, grouped-query heads (spmv_csr_attention_*_gqa) ----------------------------------------------------
    @classmethod
    def _attention_gqa(cls, what: str, scale: float, query_mats: dict, key_mats: dict, vecs: dict, _dtype=None):
        """The query-side matrices and vectors hold H heads, the key-side matrices H_kv; each side under the layout rules of
        _attention_heads.  Returns (H, H_kv, g = H // H_kv); ValueError when H_kv does not divide H."""
        heads = cls._attention_heads(what, scale, query_mats, vecs, _dtype)
        kv_heads = cls._attention_heads(what, scale, key_mats, {}, _dtype)
        if kv_heads < 1 or heads % kv_heads != 0:
            raise ValueError(f"{what}: {heads} query heads on {kv_heads} K/V heads (grouped-query attention needs H_kv to "
                             f"divide H)")
        return heads, kv_heads, heads // kv_heads

    def attention_forward_gqa(self, Q, K, V, O, stats, scale: float = 1.0, stream=None) -> None:
        """attention_forward_heads for grouped-query heads (GQA): Q, O: (H, rows, .), stats: (H, rows, 2), K: (H_kv, cols, k),
        V: (H_kv, cols, kv) with H % H_kv == 0; query head y reads K[y // g], V[y // g], g = H // H_kv, without a copy."""
        self._attention_call("forward", "gqa", (Q, K, V, O, stats), scale, stream)

    def attention_backward_q_gqa(self, Q, K, V, O, dO, stats, delta, dQ, scale: float = 1.0, stream=None) -> None:
        """attention_backward_q_heads for grouped-query heads (GQA): K, V hold H_kv heads, everything else H."""
        self._attention_call("backward_q", "gqa", (Q, K, V, O, dO, stats, delta, dQ), scale, stream)

    def attention_backward_kv_gqa(self, Q, K, V, dO, stats, delta, dK, dV, scale: float = 1.0, stream=None) -> None:
        """On the handle of the TRANSPOSED pattern: attention_backward_kv_heads for grouped-query heads (GQA).  K, V, dK, dV:
        (H_kv, rows, .); Q, dO, stats, delta hold H heads.  dK[c], dV[c] are the per-head results of query heads c g .. c g +
        g - 1 added in the kernel in head order, starting from the first head's value."""
        self._attention_call("backward_kv", "gqa", (Q, K, V, dO, stats, delta, dK, dV), scale, stream)

    # -- fused attention with an additive bias per nonzero (spmv_csr_attention_*_bias; the _gqa layout, any of the three dtypes) --
    def attention_forward_bias(self, Q, K, V, bias, O, stats, scale: float = 1.0, stream=None) -> None:
        """attention_forward_gqa on the scores scale * s + bias.  bias: float32 (nnz,), shared by the heads, or (H, nnz), in this
        handle's storage order, whatever the dtype of the matrices (float32, bfloat16 or float16)."""
        self._attention_call("forward", "gqa", (Q, K, V, O, stats), scale, stream, bias=(bias,))

    def attention_backward_q_bias(self, Q, K, V, bias, O, dO, stats, delta, dQ, dBias=None, scale: float = 1.0, stream=None) -> None:
        """attention_backward_q_gqa with the bias; dBias: float32 (H, nnz), the gradient of the bias per query head (sum it
        over the heads for a shared bias), or None: not written."""
        self._attention_call("backward_q", "gqa", (Q, K, V, O, dO, stats, delta, dQ), scale, stream, bias=(bias, dBias))

    def attention_backward_kv_bias(self, Q, K, V, bias_t, dO, stats, delta, dK, dV, scale: float = 1.0, stream=None) -> None:
        """On the handle of the TRANSPOSED pattern: attention_backward_kv_gqa with bias_t, the bias in this handle's storage
        order (:meth:`transpose_gather` makes it)."""
        self._attention_call("backward_kv", "gqa", (Q, K, V, dO, stats, delta, dK, dV), scale, stream, bias=(bias_t,))

    # -- fused attention at widths up to 128 (spmv_csr_attention_*_wide; the _bias arguments, the bias optional) ----------------
    def attention_plan_wide(self, heads: int, stream=None) -> None:
        """attention_plan_heads(heads) and the scratch of the long rows' pieces at widths above 64 (it only grows).  The _wide
        calls need it at every width."""
        check(lib().spmv_csr_attention_plan_wide(self._h, heads, _stream_handle(stream)))

    def attention_max_heads_wide(self, k: int, kv: int) -> int:
        """The most heads one _wide call on this handle takes at these widths (up to 128)."""
        n = lib().spmv_csr_attention_max_heads_wide(self._h, k, kv)
        if n < 0:
            check(n)
        return n

    def attention_forward_wide(self, Q, K, V, O, stats, bias=None, scale: float = 1.0, stream=None) -> None:
        """attention_forward_bias (bias given) or attention_forward_gqa (bias=None) at widths k, kv <= 128, float32, bfloat16 or
        float16 matrices: Q, O: (H, rows, .), K, V: (H_kv, cols, .).  Up to width 64 it is that call bit for bit."""
        self._attention_call("forward", "gqa", (Q, K, V, O, stats), scale, stream, bias=(bias,), wide=True)

    def attention_backward_q_wide(self, Q, K, V, O, dO, stats, delta, dQ, bias=None, dBias=None, scale: float = 1.0, stream=None) -> None:
        """attention_backward_q_bias or, with bias=None (then dBias must be None), attention_backward_q_gqa at widths up to 128."""
        self._attention_call("backward_q", "gqa", (Q, K, V, O, dO, stats, delta, dQ), scale, stream, bias=(bias, dBias), wide=True)

    def attention_backward_kv_wide(self, Q, K, V, dO, stats, delta, dK, dV, bias_t=None, scale: float = 1.0, stream=None) -> None:
        """On the handle of the TRANSPOSED pattern: attention_backward_kv_bias or, with bias_t=None, attention_backward_kv_gqa at
        widths up to 128."""
        self._attention_call("backward_kv", "gqa", (Q, K, V, dO, stats, delta, dK, dV), scale, stream, bias=(bias_t,), wide=True)

    def _attention_bias(self, what: str, heads: int, bias, dBias=None) -> list:
        """The C arguments of a _bias call's bias: (pointer, stride) of the bias and, if the pass has one, of dBias."""
        import torch
        if bias is None and what.endswith("_wide"):      # (no bias: the unbiased kernels; the library refuses a dBias then)
            if dBias is not None:
                raise ValueError(f"{what}: dBias without a bias")
            return [None, 0, None, 0]
        if not isinstance(bias, torch.Tensor) or bias.dtype != torch.float32 or bias.stride(-1) != 1 \
                or tuple(bias.shape) not in ((self.nnz,), (heads, self.nnz)):
            raise ValueError(f"{what}: bias must be a float32 tensor of ({self.nnz},) or ({heads}, {self.nnz}) with stride(-1) == 1")
        args = [_ptr(bias), bias.stride(0) if bias.dim() == 2 and heads > 1 else 0]
        if dBias is not None and (not isinstance(dBias, torch.Tensor) or dBias.dtype != torch.float32 or dBias.stride(-1) != 1
                                  or tuple(dBias.shape) != (heads, self.nnz)):
            raise ValueError(f"{what}: dBias must be None or a float32 tensor of ({heads}, {self.nnz}) with stride(-1) == 1")
        return args + [_ptr(dBias) if dBias is not None else None, dBias.stride(0) if dBias is not None and heads > 1 else 0]

    def _attention_call(self, spec: str, mode: str, tensors, scale: float, stream, bias=None, wide: bool = False) -> None:
        """Every attention call: pass `spec` of _ATTN_PASSES in `mode` of _ATTN_MODES on `tensors` in the spec's order.
        Matrices that are all torch.bfloat16 or all torch.float16 (stats and delta stay float32) go to the pass's _16 call: the
        same layout rules, every ld and stride counted in elements; a call of one head is one head with every stride 0, a
        _heads call a group of 1.  bias: (bias,) or (bias, dBias) of a _bias call (mode "gqa"), which takes all three dtypes.
        wide: the pass's _wide call, the _bias call's arguments with a bias that may be None."""
        import torch
        what, ops = f"attention_{spec}{'_wide' if wide else '_bias' if bias else _ATTN_MODES[mode]}", _ATTN_PASSES[spec]
        t = dict(zip((o[0] for o in ops), tensors))
        d16 = {torch.bfloat16: ATTN_BF16, torch.float16: ATTN_FP16}.get(getattr(t["Q"], "dtype", None))
        dt = t["Q"].dtype if d16 else None
        if d16:
            for name, _, w, _, _ in ops:
                if isinstance(w, str) and isinstance(t[name], torch.Tensor) and t[name].dtype != dt:
                    raise ValueError(f"{what}: {name} is {t[name].dtype}, Q is {dt} (the matrices of a 16-bit call share one dtype; "
                                     f"stats and delta are float32)")
        nd = 2 if mode == "one" else 3                       # a matrix: (rows, width) or (heads, rows, width)
        width = {"k": _width(t["Q"], nd), "kv": _width(t["V"], nd)}
        n = {"rows": self.rows, "cols": self.cols}
        mats = [(name, kvh, (t[name], n[side], width[w])) for name, side, w, _, kvh in ops if isinstance(w, str)]
        vecs = [(name, t[name], n[side], w) for name, side, w, _, _ in ops if not isinstance(w, str)]
        if mode == "one":
            self._attention_operands(what, scale, dt, **{name: m for name, _, m in mats})
            self._attention_vectors(what, **{name: (v, w * q) for name, v, q, w in vecs})
            head = [C.byref(AttnHeads(heads=1)), 1] if d16 else []
        else:
            vecs = {name: (v, q, w) for name, v, q, w in vecs}
            if mode == "heads":
                heads = kv_heads = self._attention_heads(what, scale, {name: m for name, _, m in mats}, vecs, dt)
                group = [1] if d16 else []
            else:
                heads, kv_heads, g = self._attention_gqa(what, scale, {name: m for name, kvh, m in mats if not kvh},
                                                         {name: m for name, kvh, m in mats if kvh}, vecs, dt)
                group = [g]
            # stride(0) of every tensor; 0 where it holds one head: torch's stride of a dimension of size 1 means nothing
            hs = AttnHeads(heads=heads, **{f: (t[name].stride(0) if (kv_heads if kvh else heads) > 1 else 0)
                                           for name, _, _, f, kvh in ops})
            head = [C.byref(hs)] + group
        args = []
        for name, _, w, _, _ in ops:
            args += ([width["kv"]] if name == "V" else []) + [_ptr(t[name])] + ([t[name].stride(nd - 2)] if isinstance(w, str) else [])
        if bias:
            b = self._attention_bias(what, heads, *bias)[:4 if spec == "backward_q" else 2]
            check(getattr(lib(), f"spmv_csr_{what}")(self._h, *head, d16 or ATTN_FP32, *b, scale, width["k"], *args, _stream_handle(stream)))
            return
        if d16:
            check(getattr(lib(), f"spmv_csr_attention_{spec}_16")(self._h, *head, d16, scale, width["k"], *args, _stream_handle(stream)))
            return
        check(getattr(lib(), f"spmv_csr_{what}")(self._h, *head, scale, width["k"], *args, _stream_handle(stream)))

    def values_changed(self) -> None:
        """The caller rewrote vals (borrowed arrays): plans that hold a copy of them are stale from here on."""
        check(lib().spmv_csr_values_changed(self._h))

    def time(self, variant: int, x, y, iters: int, stream=None) -> float:
        """Mean ms per launch over ``iters`` launches, HIP events on the launch stream."""
        ms = C.c_float()
        check(lib().spmv_csr_time(self._h, variant, _ptr(x), _ptr(y), iters, _stream_handle(stream),
                                  C.byref(ms)))
        return ms.value

    def run_host(self, variant: int, x, y) -> float:
        import numpy as np
        assert x.dtype == np.float32 and y.dtype == np.float32
        ms = C.c_float()
        check(lib().spmv_csr_run_host(self._h, variant, _ptr(x), _ptr(y), C.byref(ms)))
        return ms.value

    def plan_params(self, variant: int):
        """The eight numbers that fix a plan's chunk cuts (spmv_csr_plan_get)."""
        a = (C.c_int32 * 8)()
        check(lib().spmv_csr_plan_get(self._h, variant, a))
        return list(a)

    def plan_set(self, variant: int, params, stream=None) -> None:
        a = (C.c_int32 * 8)(*params)
        check(lib().spmv_csr_plan_set(self._h, variant, a, _stream_handle(stream)))

    def plan_like(self, other: "CsrMatrix", variant: int, stream=None) -> None:
        check(lib().spmv_csr_plan_like(self._h, other._h, variant, _stream_handle(stream)))

    def plan_describe(self, variant: int) -> str:
        buf = C.create_string_buffer(256)
        check(lib().spmv_csr_plan_describe(self._h, variant, buf, 256))
        return buf.value.decode()

    def plan_bytes(self, variant: int) -> int:
        return lib().spmv_csr_plan_bytes(self._h, variant)

    def plan_chunk_order(self, variant: int) -> int:
        """spmv_csr_plan_chunk_order: 0 = no launch of several chunk kinds, 1 = lists, 2 = identity."""
        rc = lib().spmv_csr_plan_chunk_order(self._h, variant)
        if rc < 0:
            check(rc)
        return rc

    def download(self):
        import numpy as np
        rp = np.empty(self.rows + 1, np.int32)
        ci = np.empty(self.nnz, np.int32)
        va = np.empty(self.nnz, np.float32)
        check(lib().spmv_csr_download(self._h, _ptr(rp), _ptr(ci), _ptr(va)))
        return rp, ci, va

    def close(self) -> None:
        if self._h:
            check(lib().spmv_csr_destroy(self._h))
            self._h = C.c_void_p()
            self._keep = ()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TcsrMatrix:
    """Owner of one ``spmv_tcsr_t``: the reference's tiled bitmap-CSR (tcsr.cpp:5-38) on the device."""

    def __init__(self, handle: int, M: int, N: int):
        self._h = C.c_void_p(handle)
        self.M, self.N = M, N
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().spmv_tcsr_sizes(self._h, C.byref(a), C.byref(b), C.byref(c)))
        self.n_blk_idx, self.n_bitmaps, self.nnz = a.value, b.value, c.value

    @classmethod
    def from_dense_host(cls, A):
        import numpy as np
        A = np.ascontiguousarray(A, dtype=np.float32)
        M, N = A.shape
        h = C.c_void_p()
        check(lib().spmv_tcsr_from_dense_host(M, N, _ptr(A), 0, C.byref(h)))
        return cls(h.value, M, N)

    @classmethod
    def from_dense_device(cls, A):
        M, N = A.shape
        h = C.c_void_p()
        check(lib().spmv_tcsr_from_dense_device(M, N, _ptr(A), _stream_handle(), C.byref(h)))
        return cls(h.value, M, N)

    def download(self):
        import numpy as np
        bi = np.empty(self.n_blk_idx, np.int32)
        bm = np.empty(self.n_bitmaps, np.uint32)
        va = np.empty(self.nnz, np.float32)
        check(lib().spmv_tcsr_download(self._h, _ptr(bi), _ptr(bm), _ptr(va)))
        return bi, bm, va

    def run(self, x, y, stream=None) -> None:
        assert x.numel() >= self.M and y.numel() >= self.N
        check(lib().spmv_tcsr_run(self._h, _ptr(x), _ptr(y), _stream_handle(stream)))

    def run_host(self, x, y) -> float:
        ms = C.c_float()
        check(lib().spmv_tcsr_run_host(self._h, _ptr(x), _ptr(y), C.byref(ms)))
        return ms.value

    def close(self) -> None:
        if self._h:
            check(lib().spmv_tcsr_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


BITMAP_FORMATS = {"wsp": 0, "awsp": 1, "awsp_ref": 2}      # enum spmv_bitmap_format


class BitmapMatrix:
    """Owner of one ``spmv_bitmap_t``: the reference's WSP / AWSP / AWSPRef format (wsp.cpp, awsp.cpp,
    awsp_ref.cpp) on the device."""

    def __init__(self, handle: int, fmt: str, M: int, N: int):
        self._h = C.c_void_p(handle)
        self.fmt, self.M, self.N = fmt, M, N
        a, b = C.c_int64(), C.c_int64()
        st = (C.c_int32 * 4)()
        check(lib().spmv_bitmap_sizes(self._h, C.byref(a), C.byref(b), st))
        self.n_bitmaps, self.n_vals, self.stats = a.value, b.value, list(st)

    @classmethod
    def from_dense_host(cls, fmt: str, A):
        import numpy as np
        A = np.ascontiguousarray(A, dtype=np.float32)
        M, N = A.shape
        h = C.c_void_p()
        check(lib().spmv_bitmap_from_dense_host(BITMAP_FORMATS[fmt], M, N, _ptr(A), 0, C.byref(h)))
        return cls(h.value, fmt, M, N)

    @classmethod
    def from_dense_device(cls, fmt: str, A):
        M, N = A.shape
        h = C.c_void_p()
        check(lib().spmv_bitmap_from_dense_device(BITMAP_FORMATS[fmt], M, N, _ptr(A), _stream_handle(), C.byref(h)))
        return cls(h.value, fmt, M, N)

    def download(self):
        import numpy as np
        bm = np.empty(self.n_bitmaps, np.uint32)
        va = np.empty(self.n_vals, np.float32)
        check(lib().spmv_bitmap_download(self._h, _ptr(bm), _ptr(va)))
        return bm, va

    def run(self, x, y, stream=None) -> None:
        assert x.numel() >= self.M and y.numel() >= self.N
        check(lib().spmv_bitmap_run(self._h, _ptr(x), _ptr(y), _stream_handle(stream)))

    def run_host(self, x, y) -> float:
        ms = C.c_float()
        check(lib().spmv_bitmap_run_host(self._h, _ptr(x), _ptr(y), C.byref(ms)))
        return ms.value

    def close(self) -> None:
        if self._h:
            check(lib().spmv_bitmap_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dense_gemv(A, x, y, mode: int, stream=None, workspace=None) -> None:
    """y = A^T x on the dense device matrix; with ``workspace`` (a device tensor of at least
    ``dense_gemv_workspace_bytes(N, mode)`` bytes) through the allocation-free entry."""
    M, N = A.shape
    if workspace is None:
        check(lib().spmv_dense_gemv(M, N, _ptr(A), _ptr(x), _ptr(y), mode, _stream_handle(stream)))
    else:
        check(lib().spmv_dense_gemv_ws(M, N, _ptr(A), _ptr(x), _ptr(y), mode, _ptr(workspace),
                                       workspace.numel() * workspace.element_size(), _stream_handle(stream)))


def dense_gemv_workspace_bytes(N: int, mode: int) -> int:
    return lib().spmv_dense_gemv_workspace_bytes(N, mode)


def asp_retile(A, out, stream=None) -> None:
    """The reference's ASPMatrix layout of the dense device matrix A[M][N] into ``out`` (M*N floats)."""
    M, N = A.shape
    check(lib().spmv_asp_retile(M, N, _ptr(A), _ptr(out), _stream_handle(stream)))


def asp_gemv(M: int, N: int, asp, x, y, workspace, stream=None) -> None:
    """y = A^T x from the ASP layout, rows with x == 0 skipped; ``workspace``: dense_gemv_workspace_bytes(N, 3) bytes."""
    check(lib().spmv_asp_gemv_ws(M, N, _ptr(asp), _ptr(x), _ptr(y), _ptr(workspace),
                                 workspace.numel() * workspace.element_size(), _stream_handle(stream)))


def permute_vector(perm, src, dst=None, inverse: bool = False, stream=None):
    """``dst[r] = src[perm[r]]``, or with ``inverse=True`` ``dst[perm[r]] = src[r]`` (spmv_permute_vector): one launch, bits copied.
    perm: int32, src / dst: float32, contiguous 1-D device tensors of one length; ``dst`` None makes a new one; src and dst must
    not overlap.  Returns dst."""
    import torch
    if dst is None and isinstance(src, torch.Tensor):
        dst = torch.empty_like(src)
    for name, t, dt in (("perm", perm, torch.int32), ("src", src, torch.float32), ("dst", dst, torch.float32)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != 1 or not t.is_contiguous() or t.numel() != perm.numel():
            raise ValueError(f"permute_vector: {name} must be a contiguous 1-D {dt} tensor of perm's length")
    check(lib().spmv_permute_vector(_ptr(perm), perm.numel(), 1 if inverse else 0, _ptr(src), _ptr(dst), _stream_handle(stream)))
    return dst


def synth_fill(seed, row0, n_local, rows, cols, band, row_ptr, col_idx, vals, stream=None) -> None:
    check(lib().spmv_synth_fill(seed, row0, n_local, rows, cols, band, _ptr(row_ptr), _ptr(col_idx),
                                _ptr(vals), _stream_handle(stream)))


def synth_x(seed, j0, n, x, stream=None) -> None:
    check(lib().spmv_synth_x(seed, j0, n, _ptr(x), _stream_handle(stream)))


# -- measurement aids (kernels of known traffic for calibrating rocprofv3's counters; include/spmv_hip.h) ----------
def calib_stream(src, nbytes: int, sink, stream=None) -> None:
    check(lib().spmv_calib_stream(_ptr(src), nbytes, _ptr(sink), _stream_handle(stream)))


def calib_gather(table, table_lines: int, n_lines: int, touch: int, sink, stream=None) -> None:
    check(lib().spmv_calib_gather(_ptr(table), table_lines, n_lines, touch, _ptr(sink), _stream_handle(stream)))


def calib_store(dst, nbytes: int, width: int, stream=None) -> None:
    check(lib().spmv_calib_store(_ptr(dst), nbytes, width, _stream_handle(stream)))


def calib_marker(ident: int, stream=None) -> None:
    check(lib().spmv_calib_marker(ident, _stream_handle(stream)))


def debug_bounds(max_records: int = 64) -> list:
    """TEST ONLY (the checked build): [(site name, violations, largest overrun in bytes)] recorded since the last call, which
    clears them.  The normal library raises SpmvError (SPMV_ERR_INVALID: not instrumented)."""
    import numpy as np
    rec = np.zeros(3 * max_records, np.int64)
    n = lib().spmv_debug_bounds(rec.ctypes.data, max_records)
    if n < 0:
        check(n)
    return [(BOUNDS_SITES[int(rec[3 * i])], int(rec[3 * i + 1]), int(rec[3 * i + 2])) for i in range(min(n, max_records))]
