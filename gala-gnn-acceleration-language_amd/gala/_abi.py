"""ctypes binding of libgala_hip.so — a line-for-line mirror of include/gala_hip.h —
and of libgala_cpu.so (include/gala_cpu.h: the same operator signatures, host pointers).

This is the Python-side stub of the C ABI (the reference-side binding for C++ callers is
`#include "gala_hip.h"`).  Loading fails loudly when the library is
missing: there is no CPU fallback anywhere in the product path; the CPU backend is only
reached by explicitly calling it (call_cpu) or by placing a program's tensors on the host.
"""
from __future__ import annotations

import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgala_hip.so")
CPU_LIB_PATH = os.path.join(_HERE, "libgala_cpu.so")

GALA_OK = 0
GALA_ERR_INVALID_ARG = -1
GALA_ERR_UNSUPPORTED = -2
GALA_ERR_HIP = -3
GALA_ERR_GRAPH = -4

GALA_SPMM_ACCUM = 0x1
GALA_SPMM_SAMPLE = 0x2
GALA_SPMM_EXACT = 0x4
GALA_SPMM_HUB_CHUNKED = 0x8
GALA_SDDVV_ADD = 0
GALA_SDDVV_MUL = 1
GALA_SDDVV_ADD_LRELU = 2
GALA_SOFTMAX_REF = 0
GALA_SOFTMAX_FIXED = 1
GALA_GAT_PARTIAL = 0x10


class gala_split_plan_t(ctypes.Structure):
    _fields_ = [
        ("threshold", ctypes.c_int32),
        ("chunk", ctypes.c_int32),
        ("n_rows_split", ctypes.c_int64),
        ("n_chunks", ctypes.c_int64),
        ("rows", ctypes.c_void_p),
        ("row_chunk0", ctypes.c_void_p),
        ("chunk_row", ctypes.c_void_p),
        ("workspace", ctypes.c_void_p),
        ("ws_cols", ctypes.c_int64),
        ("row_order", ctypes.c_void_p),
        ("aux_stream", ctypes.c_void_p),
        ("aux_events", ctypes.c_void_p * 2),
    ]


class gala_spmm_epilogue_t(ctypes.Structure):
    _fields_ = [
        ("dst_deg_rsqrt", ctypes.c_int32),
        ("Y2", ctypes.c_void_p),
        ("ldy2", ctypes.c_int64),
        ("y2_scale", ctypes.c_void_p),
        ("src_relu", ctypes.c_int32),
        ("src_act", ctypes.c_void_p),
        ("relu_x", ctypes.c_void_p),
        ("ldrx", ctypes.c_int64),
        ("relu_act", ctypes.c_void_p),
    ]


class gala_csr_t(ctypes.Structure):
    _fields_ = [
        ("n_rows", ctypes.c_int64),
        ("n_cols", ctypes.c_int64),
        ("nnz", ctypes.c_int64),
        ("rowptr", ctypes.c_void_p),
        ("col", ctypes.c_void_p),
        ("val", ctypes.c_void_p),
        ("val_heads", ctypes.c_int32),
        ("n_seg", ctypes.c_int32),
        ("seg_bounds", ctypes.c_void_p),
        ("split", ctypes.c_void_p),
        ("val_row_scale", ctypes.c_void_p),
    ]


_P = ctypes.c_void_p
_I64 = ctypes.c_int64
_I32 = ctypes.c_int32
_F = ctypes.c_float
_CSR = ctypes.POINTER(gala_csr_t)

# name -> (restype, argtypes)
SIGNATURES = {
    "gala_abi_version": (ctypes.c_int, []),
    "gala_status_string": (ctypes.c_char_p, [ctypes.c_int]),
    "gala_last_hip_error": (ctypes.c_int, []),
    "gala_spmm_f32": (ctypes.c_int, [_CSR, _P, _I64, _P, _I64, _I32, _P, _P, _I32, _I32, _I32, _I32, _P]),
    "gala_spmm_ex_f32": (ctypes.c_int, [_CSR, _P, _I64, _P, _I64, _I32, _P, _P, _I32, _I32, _I32, _I32,
                                        ctypes.POINTER(gala_spmm_epilogue_t), _P]),
    "gala_row_broadcast_deg_f32": (ctypes.c_int, [_CSR, _I32, _P, _I64, _P, _I64, _P]),
    "gala_degree_f32": (ctypes.c_int, [_CSR, _P, _F, _I32, _I32, _P]),
    "gala_row_broadcast_f32": (ctypes.c_int, [_I64, _I32, _P, _P, _I64, _P, _I64, _P]),
    "gala_ffn_fwd_f32": (ctypes.c_int, [_I64, _I32, _I32, _P, _I64, _P, _P, _P, _I64, _P]),
    "gala_row_scale_relu_f32": (ctypes.c_int, [_I64, _I32, _P, _P, _P, _I64, _P, _I64, _P]),
    "gala_relu_scale_backward_f32": (ctypes.c_int, [_I64, _I32, _P, _P, _I64, _P, _I64, _P, _I64, _P]),
    "gala_sddvv_f32": (ctypes.c_int, [_CSR, _P, _P, _I32, _I32, _F, _P, _P]),
    "gala_row_sum_f32": (ctypes.c_int, [_CSR, _P, _I32, _F, _P, _I32, _P]),
    "gala_row_scale_f32": (ctypes.c_int, [_CSR, _P, _I32, _P, _P]),
    "gala_sddmm_dot_f32": (ctypes.c_int, [_CSR, _P, _I64, _P, _I64, _I32, _I32, _P, _P]),
    "gala_edge_softmax_fwd_f32": (ctypes.c_int, [_CSR, _P, _I32, _I32, _P, _P]),
    "gala_edge_softmax_bwd_f32": (ctypes.c_int, [_CSR, _P, _P, _I32, _I32, _P, _P]),
    "gala_gat_fwd_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _I64, _I32, _I32, _F, _I32, _P, _I64, _P, _P]),
    "gala_gat_bwd_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _I64, _P, _I64, _I32, _I32, _F, _I32, _P, _P, _P, _P]),
    "gala_gat_fwd_attn_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _I64, _I32, _F, _I32, _P, _I64, _P, _P]),
    "gala_gat_bwd_attn_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _I64, _P, _I64, _I32, _F, _P, _P, _P]),
    "gala_gat_fwd_ex_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _P, _I64, _I32, _I32, _F, _I32, _P, _I64, _P,
                                           _P, _P]),
    "gala_gat_bwd_ex_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _P, _I64, _P, _I64, _I32, _I32, _F, _I32, _P,
                                           _P, _P, _P, _P]),
    "gala_gat_bwd_fused_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _P, _I64, _P, _I64, _I32, _I32, _F, _P, _P,
                                              _I64, _P, _P]),
    "gala_gat_fwd_stats_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _P, _I64, _I32, _I32, _F, _P, _I64, _P, _P,
                                              _I64, _P, _P, _P, _P]),
    "gala_gat_bwd_stats_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _I64, _I32, _I32, _F, _P, _P, _I64, _P,
                                              _I64, _P, _P, _I64, _P, _P]),
    "gala_gat_fwd_stats_exact_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _P, _I64, _I32, _I32, _F, _P, _I64, _P,
                                                    _P, _I64, _P, _P, _P]),
    "gala_gat_bwd_stats_exact_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _I64, _P, _I64, _I32, _I32, _F, _P, _P, _I64,
                                                    _P, _I64, _P, _P, _P, _I64, _P, _P, _P]),
    "gala_gat_bwd_stats_exact_t_f32": (ctypes.c_int, [_CSR, _CSR, _P, _P, _P, _I64, _P, _I64, _I32, _I32, _F, _P, _P,
                                                      _I64, _P, _I64, _P, _P, _P, _I64, _P, _P, _P]),
    "gala_csr_is_transpose_i32": (ctypes.c_int, [_CSR, _CSR, _P, _P]),
    "gala_gat_fwd_stats_exact_ex_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _P, _I64, _I32, _I32, _F, _P, _I64,
                                                       _P, _P, _I64, _P, _P, _P, _P]),
    "gala_gat_bwd_exact_pre_ex_f32": (ctypes.c_int, [_CSR, _P, _P, _I64, _I32, _I32, _P, _P, _I64, _P, _I64, _P,
                                                     _P, _P, _P, _P]),
    "gala_gat_bwd_exact_gather_ex_f32": (ctypes.c_int, [_CSR, _P, _P, _I64, _P, _I64, _I32, _I32, _F, _P, _P, _P,
                                                        _I64, _P, _P]),
    "gala_gat_fwd_stats_ex_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _P, _I64, _I32, _I32, _F, _P, _I64, _P,
                                                 _P, _I64, _P, _P, _P, _P, _P]),
    "gala_gat_bwd_stats_ex_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _I64, _P, _I32, _I32, _F, _P, _P, _I64,
                                                 _P, _I64, _P, _P, _I64, _P, _P]),
    "gala_gat_bwd_stats_linear_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _I64, _P, _I32, _I32, _F, _P, _P,
                                                     _I64, _P, _I64, _P, _P, _P, _I64, _P, _P]),
    "gala_gat_fwd_partial_stats_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _P, _I64, _I32, _I32, _F, _P, _I64,
                                                      _P, _P, _I64, _P, _P]),
    "gala_gat_fwd_partial_stats_ex_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _P, _I64, _I32, _I32, _F, _P,
                                                         _I64, _P, _P, _I64, _P, _P, _P, _P]),
    "gala_gat_fwd_continue_f32": (ctypes.c_int, [_CSR, _P, _P, _P, _P, _P, _I64, _I32, _I32, _F, _I32, _P, _I64, _P,
                                                 _P, _I64, _P, _P, _I64, _P, _P, _I64, _P, _P]),
    "gala_head_attn_f32": (ctypes.c_int, [_I64, _I32, _I32, _P, _I64, _P, _P, _P, _P]),
    "gala_head_attn_bwd_f32": (ctypes.c_int, [_I64, _I32, _I32, _P, _P, _P, _I64, _I32, _P]),
    "gala_edge_permute_f32": (ctypes.c_int, [_P, _P, _I64, _I32, _P, _P]),
    "gala_host_csr_build": (ctypes.c_int, [_I64, _I64, _I64, _P, _P, _P, _P, _P]),
    "gala_host_col_breakpoints": (ctypes.c_int64, [_I64, _I64, _P, _I64]),
    "gala_host_col_tile": (ctypes.c_int, [_I64, _P, _P, _P, _I32, _P, _P, _P, _P, _P]),
    "gala_host_sample_ab": (ctypes.c_int, [_I64, _P, _P, _P, _I32, _I32, _I32, _P, _P, _P]),
    "gala_host_split_plan": (ctypes.c_int, [_I64, _P, _I32, _I32, _P, _P, _P, _P, _P]),
    "gala_host_split_threshold": (ctypes.c_int32, [_I64, _I64]),
    "gala_host_csr_transpose": (ctypes.c_int, [_I64, _I64, _P, _P, _P, _P, _P]),
    "gala_host_row_order": (ctypes.c_int, [_I64, _P, _P]),
    "gala_host_gen_graph": (ctypes.c_int, [_I32, _I64, _I64, ctypes.c_uint64, _P, _P]),
    "gala_host_mask_subgraph": (ctypes.c_int, [_I64, _P, _P, _P, _P, _P, _P]),
    "gala_host_mtx_info": (ctypes.c_int, [ctypes.c_char_p, _P, _P, _P, _P, _P, _P]),
    "gala_host_mtx_read": (ctypes.c_int, [ctypes.c_char_p, _P, _P, _P, _I64, _P]),
    "gala_host_mtx_dense_info": (ctypes.c_int, [ctypes.c_char_p, _P, _P]),
    "gala_host_mtx_read_dense": (ctypes.c_int, [ctypes.c_char_p, _P, _I64, _I64, _P]),
    "gala_dense_grad_workspace": (ctypes.c_int64, [_I64, _I32, _I32]),
    "gala_dense_grad_f32": (ctypes.c_int, [_I64, _I32, _I32, _P, _I64, _P, _I64, _P, _P, _I32, _P, _I64, _P]),
    "gala_gat_in_prep_f32": (ctypes.c_int, [_I64, _I32, _P, _I64, _I32, _P, _P, _P, _P]),
    "gala_gat_in_fwd_f32": (ctypes.c_int, [_CSR, _P, _I32, _I32, _I32, _F, _P, _P, _I64, _P, _P, _P, _I64, _P, _P,
                                           _I32, _P]),
    "gala_gat_in_bwd_workspace": (ctypes.c_int64, [_I32]),
    "gala_gat_in_split_ws_cols": (ctypes.c_int64, [_I32]),
    "gala_gat_in_bwd_f32": (ctypes.c_int, [_CSR, _P, _I32, _I32, _I32, _F, _P, _P, _P, _P, _I64, _P, _P, _P, _P,
                                           _I64, _I32, _P]),
    "gala_gat_in_fwd_t_f32": (ctypes.c_int, [_CSR, _P, _I32, _I32, _I32, _F, _P, _P, _I64, _P, _P, _P, _I64, _P,
                                             _P, _I32, _P, _P]),
    "gala_gat_in_bwd_t_f32": (ctypes.c_int, [_I64, _P, _I32, _I32, _I32, _P, _P, _P, _P, _I64, _P, _P, _P, _P, _I64,
                                             _I32, _P]),
    # the rectangular forms (row_base after the graph): a row partition's own rows over its table
    "gala_gat_in_fwd_rect_f32": (ctypes.c_int, [_CSR, _I64, _P, _I32, _I32, _I32, _F, _P, _P, _I64, _P, _P, _P, _I64,
                                                _P, _P, _I32, _P]),
    "gala_gat_in_q_rect_f32": (ctypes.c_int, [_CSR, _I64, _I32, _F, _P, _P, _P]),
    "gala_gat_in_fwd_t_rect_f32": (ctypes.c_int, [_CSR, _I64, _P, _I32, _I32, _I32, _F, _P, _P, _I64, _P, _P, _P,
                                                  _I64, _P, _P, _I32, _P, _P]),
    "gala_gat_in_bwd_rect_f32": (ctypes.c_int, [_CSR, _I64, _P, _I32, _I32, _I32, _F, _P, _P, _P, _P, _I64, _P, _P,
                                                _P, _P, _I64, _I32, _P]),
    "gala_gat_in_q_gather_f32": (ctypes.c_int, [_I64, _P, _I64, _I32, _P, _P, _P]),
    "gala_gat_in_q_scatter_f32": (ctypes.c_int, [_I64, _P, _I64, _I64, _I32, _P, _P, _P]),
}


class GalaError(RuntimeError):
    def __init__(self, fn: str, status: int, hip_error: int = 0):
        name = {0: "GALA_OK", -1: "GALA_ERR_INVALID_ARG", -2: "GALA_ERR_UNSUPPORTED",
                -3: "GALA_ERR_HIP", -4: "GALA_ERR_GRAPH"}.get(status, str(status))
        msg = f"{fn} failed: {name}"
        if status == GALA_ERR_HIP:
            msg += f" (hipError {hip_error})"
        super().__init__(msg)
        self.status = status


_lib = None


GALA_GAT_IN_RELU = 1
GALA_GAT_IN_WS_FWD, GALA_GAT_IN_WS_FWD_T, GALA_GAT_IN_WS_BWD = 0, 1, 2  # gala_gat_in_split_ws_cols modes
ABI_VERSION = 6  # GALA_ABI_VERSION of include/gala_hip.h these bindings mirror


def lib() -> ctypes.CDLL:
    """Load libgala_hip.so (raises if it was not built: no fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C gala-gnn-acceleration-language_amd`")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.gala_abi_version() != ABI_VERSION:  # the struct layouts below are ABI_VERSION's
            raise ImportError(f"{LIB_PATH} has ABI {L.gala_abi_version()}, this module expects {ABI_VERSION}: rebuild it")
        _lib = L
    return _lib


def check(fn: str, status: int) -> None:
    if status != GALA_OK:
        raise GalaError(fn, status, lib().gala_last_hip_error() if status == GALA_ERR_HIP else 0)


def call(fn: str, *args) -> int:
    status = getattr(lib(), fn)(*args)
    check(fn, status)
    return status


# operators with a host-CPU counterpart gala_cpu_X in libgala_cpu.so (include/gala_cpu.h)
CPU_OPS = ("gala_spmm_f32", "gala_spmm_ex_f32", "gala_row_broadcast_deg_f32", "gala_degree_f32", "gala_row_broadcast_f32", "gala_row_scale_relu_f32",
           "gala_relu_scale_backward_f32", "gala_ffn_fwd_f32", "gala_sddvv_f32",
           "gala_row_sum_f32", "gala_row_scale_f32", "gala_sddmm_dot_f32",
           "gala_edge_softmax_fwd_f32", "gala_edge_softmax_bwd_f32", "gala_gat_fwd_f32",
           "gala_gat_bwd_f32", "gala_gat_fwd_attn_f32", "gala_gat_bwd_attn_f32",
           "gala_gat_fwd_ex_f32", "gala_gat_bwd_ex_f32", "gala_gat_bwd_fused_f32",
           "gala_gat_fwd_stats_f32", "gala_gat_bwd_stats_f32", "gala_gat_fwd_partial_stats_f32",
           "gala_gat_fwd_stats_ex_f32", "gala_gat_bwd_stats_ex_f32", "gala_gat_fwd_partial_stats_ex_f32",
           "gala_gat_fwd_continue_f32", "gala_gat_bwd_stats_linear_f32", "gala_gat_fwd_stats_exact_f32",
           "gala_gat_bwd_stats_exact_f32", "gala_gat_fwd_stats_exact_ex_f32", "gala_gat_bwd_exact_pre_ex_f32",
           "gala_gat_bwd_exact_gather_ex_f32", "gala_gat_bwd_stats_exact_t_f32", "gala_csr_is_transpose_i32",
           "gala_head_attn_f32",
           "gala_head_attn_bwd_f32", "gala_edge_permute_f32", "gala_dense_grad_workspace",
           "gala_dense_grad_f32", "gala_gat_in_prep_f32", "gala_gat_in_fwd_f32", "gala_gat_in_bwd_workspace",
           "gala_gat_in_bwd_f32", "gala_gat_in_fwd_rect_f32", "gala_gat_in_bwd_rect_f32",
           "gala_gat_in_q_gather_f32", "gala_gat_in_q_scatter_f32")


def cpu_name(fn: str) -> str:
    return "gala_cpu_" + fn[len("gala_"):]


_cpu_lib = None


def cpu_lib() -> ctypes.CDLL:
    """Load libgala_cpu.so (raises if it was not built)."""
    global _cpu_lib
    if _cpu_lib is None:
        if not os.path.exists(CPU_LIB_PATH):
            raise ImportError(f"{CPU_LIB_PATH} is missing: build it with "
                              "`make -C gala-gnn-acceleration-language_amd`")
        L = ctypes.CDLL(CPU_LIB_PATH)
        for name in CPU_OPS:
            res, args = SIGNATURES[name]
            fn = getattr(L, cpu_name(name))
            fn.restype = res
            fn.argtypes = args
        _cpu_lib = L
    return _cpu_lib


def call_cpu(fn: str, *args) -> int:
    """The host-CPU backend's gala_cpu_X for the gala_X name `fn` (host pointers)."""
    status = getattr(cpu_lib(), cpu_name(fn))(*args)
    if status != GALA_OK:
        raise GalaError(cpu_name(fn), status)
    return status
