"""ctypes binding of libgfv.so (the C ABI declared in include/gfv.h).

Plumbing only: converts torch CUDA tensors to raw device pointers and launches on torch's current HIP stream.
There is NO fallback: if the shared library is missing or a call fails, this raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GFV_LIB", os.path.join(HERE, "libgfv.so"))

c_float_p = C.c_void_p
c_int_p = C.c_void_p

OP_NONE, OP_BIAS_GELU, OP_MUL_DGELU = 0, 1, 2
IN_NONE, IN_GELU, IN_LN, IN_LNBWD = 0, 1, 2, 3
FIN_PLAIN, FIN_LN, FIN_LNBWD = 0, 1, 2
CHAIN_ROW_OWNER, CHAIN_COLUMN_OWNER = 1, 2   # gfv_rowtile_args_t.flags
DW_COLSCALE = 8   # gfv_dw_tile_t.a_op flag: per-column power-of-two scales of raw-input activations


class Seg(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("idx", C.c_void_p), ("width", C.c_int32), ("ld", C.c_int32),
                ("csr_rowptr", C.c_void_p), ("csr_scale", C.c_void_p), ("save", C.c_void_p)]


class Layer(C.Structure):
    _fields_ = [("W", C.c_void_p), ("bias", C.c_void_p), ("K", C.c_int32), ("N", C.c_int32), ("op", C.c_int32),
                ("ldw", C.c_int32), ("save", C.c_void_p), ("aux", C.c_void_p), ("Wh", C.c_void_p),
                ("bias2", C.c_void_p)]


class RowtileArgs(C.Structure):
    _fields_ = [
        ("M", C.c_int32), ("nseg", C.c_int32), ("seg", Seg * 3), ("in_add", C.c_void_p), ("in_op", C.c_int32),
        ("nlayers", C.c_int32), ("in_gamma", C.c_void_p), ("in_beta", C.c_void_p), ("in_aux", C.c_void_p),
        ("gadd", C.c_void_p), ("gadd_s", C.c_void_p), ("gadd_r", C.c_void_p), ("in_save", C.c_void_p),
        ("ln_partial", C.c_void_p), ("layer", Layer * 3), ("fin_op", C.c_int32), ("hidden", C.c_int32),
        ("fin_gamma", C.c_void_p), ("fin_beta", C.c_void_p), ("fin_aux", C.c_void_p), ("fin_presave", C.c_void_p),
        ("res", C.c_void_p * 3), ("res_ld", C.c_int32 * 3), ("out_ld", C.c_int32 * 3), ("out", C.c_void_p * 3),
        ("out_nores", C.c_void_p), ("padd", C.c_void_p), ("padd_s", C.c_void_p), ("padd_r", C.c_void_p),
        ("padd_ld", C.c_int32), ("flags", C.c_int32), ("wmax", C.c_void_p),
        ("gscale", C.c_void_p), ("gscale_ld", C.c_int32), ("product_form", C.c_int32),
        ("fin_stats", C.c_void_p), ("in_stats", C.c_void_p), ("dw_partial", C.c_void_p), ("dw_partial_stride", C.c_int64),
        ("dw_in", C.c_void_p), ("dw_in_ld", C.c_int32), ("reserved2_", C.c_int32),
        ("rc_Wh", C.c_void_p * 2), ("rc_bias", C.c_void_p * 2),
    ]


ABI_VERSION = 3   # GFV_ABI_VERSION of include/gfv.h this binding is written against

DW_FUSED_FLOATS = 2 * 128 * 128 + 4 * 128   # floats per workgroup block of a fused weight-gradient launch (include/gfv.h)
# ... and where its pieces start, restating gfv_rowtile_args_t.dw_partial (include/gfv.h:200-201):
# [dW3 (128 x 128) | db3 (128) | dW2 (128 x 128) | db2 (128) | dgamma (128) | dbeta (128)]
DW_FUSED_WB = 128 * 128 + 128         # floats of one dW | db pair
DW_FUSED_OFF_W3 = 0                   # dW3 | db3
DW_FUSED_OFF_W2 = DW_FUSED_WB         # dW2 | db2
DW_FUSED_OFF_LN = 2 * DW_FUSED_WB     # dgamma | dbeta (2 * 128 floats)
assert DW_FUSED_OFF_LN + 256 == DW_FUSED_FLOATS


class WimgDesc(C.Structure):
    _fields_ = [("W", C.c_void_p), ("img", C.c_void_p), ("ldw", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("reserved", C.c_int32)]


class DwTile(C.Structure):
    _fields_ = [("G", C.c_void_p), ("A", C.c_void_p), ("idx", C.c_void_p), ("in_add", C.c_void_p),
                ("a_gamma", C.c_void_p), ("a_beta", C.c_void_p), ("ldg", C.c_int32), ("n_out", C.c_int32),
                ("width", C.c_int32), ("ld", C.c_int32), ("a_op", C.c_int32), ("ld_out", C.c_int32),
                ("out_off", C.c_int64), ("db_off", C.c_int64), ("gscale", C.c_void_p)]


class ReducePiece(C.Structure):
    _fields_ = [("partial", C.c_void_p), ("out", C.c_void_p), ("chunk_stride", C.c_int64), ("n_chunks", C.c_int32),
                ("rows", C.c_int32), ("cols", C.c_int32), ("ld_in", C.c_int32), ("ld_out", C.c_int32), ("reserved", C.c_int32)]


class TransMlp(C.Structure):
    _fields_ = [("x", C.c_void_p), ("res", C.c_void_p), ("img_out", C.c_void_p), ("img_pre", C.c_void_p), ("img_post", C.c_void_p),
                ("b_out", C.c_void_p), ("b_pre", C.c_void_p), ("b_post", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
                ("wmax", C.c_void_p), ("fx1", C.c_void_p), ("z", C.c_void_p), ("out", C.c_void_p), ("M", C.c_int32),
                ("reserved", C.c_int32)]


class TransMlpBwd(C.Structure):
    _fields_ = [("g", C.c_void_p), ("g_add", C.c_void_p), ("g_sum", C.c_void_p), ("z", C.c_void_p), ("fx1", C.c_void_p),
                ("img_post_t", C.c_void_p), ("img_pre_t", C.c_void_p), ("img_out_t", C.c_void_p), ("gamma", C.c_void_p),
                ("wmax", C.c_void_p), ("g_z", C.c_void_p), ("g_fx1", C.c_void_p), ("g_out_x", C.c_void_p),
                ("ln_partial", C.c_void_p), ("gscale", C.c_void_p), ("M", C.c_int32), ("reserved", C.c_int32)]


class FvmMesh(C.Structure):
    """gfv_fvm_mesh_t (include/gfv.h): the mesh tables of a batch for the fused finite-volume launches."""
    _fields_ = ([("N", C.c_int32), ("E", C.c_int32), ("C", C.c_int32), ("B", C.c_int32), ("terms", C.c_int32), ("mode", C.c_int32),
                 ("smooth", C.c_int32), ("reserved", C.c_int32)]
                + [(n, C.c_void_p) for n in (
                    "node_type", "batch", "ftype", "cbatch", "gcell_ptr", "pos", "fpos", "y", "centroid", "area", "theta", "sigma",
                    "uvp_dim", "dt", "crow", "kcell", "kS", "frow", "fk", "nfrow", "nfcol2", "nrow", "ncell", "An", "rn",
                    "xo_rowptr", "xo_in", "xo_B", "sumB")])


POOL_MAX_GRAPHS, POOL_MAX_ATTRS, POOL_ROW_HEAD = 64, 56, 8   # GFV_POOL_* of include/gfv.h
EVAL_RECORD = 16   # GFV_EVAL_RECORD of include/gfv.h: floats per row of the table gfv_eval_collect fills
# GFV_TRAIN_LOG_* of include/gfv.h: logical elements per chunk, head words of a ring row, words per entry-table row, buckets at most
TRAIN_LOG_CHUNK, TRAIN_LOG_HEAD, TRAIN_LOG_ENTRY_RECORD, TRAIN_LOG_MAX_BUCKETS = 1024, 16, 8, 32
# GFV_MARCH_* of include/gfv.h: words of the march record, head words and per-graph words of a history row, the two flags
MARCH_RECORD, MARCH_HEAD, MARCH_GRAPH, MARCH_CONVERGED, MARCH_CAPPED = 16, 8, 8, 1, 2
WINDOW_RECORD = 8   # GFV_WINDOW_RECORD of include/gfv.h: words of a sampling window's record
# GFV_FIELD_STATS_* of include/gfv.h: words of the record (the window's), planes of the double sums, planes of the float state
FIELD_STATS_RECORD, FIELD_STATS_SUMS, FIELD_STATS_AUX = WINDOW_RECORD, 7, 9
# GFV_TIME_BC_* of include/gfv.h: doubles of a waveform record, words of the control record, doubles of a history row, points of a
# table at most, the kinds of gfv_time_bc_update
TIME_BC_RECORD, TIME_BC_CTL, TIME_BC_HIST, TIME_BC_TABLE_MAX = 8, 4, 3, 1024
TIME_BC_NONE, TIME_BC_CONST, TIME_BC_RAMP_LINEAR, TIME_BC_RAMP_SMOOTH, TIME_BC_SINE, TIME_BC_TABLE, TIME_BC_TABLE_PERIODIC = range(7)
# GFV_TIME_SCHEME_* of include/gfv.h: words of the record, the schemes of gfv_time_scheme_update
TIME_SCHEME_RECORD, TIME_SCHEME_BDF1, TIME_SCHEME_BDF2 = 4, 1, 2
# GFV_STEP_CONTROL_* of include/gfv.h: words of the control record, floats of the parameters, rows of the per-graph state
STEP_CONTROL_RECORD, STEP_CONTROL_PARAMS, STEP_CONTROL_STATE = 4, 8, 4
# GFV_WALL_FORCE_* of include/gfv.h: words of the record (the window's), sums per graph, faces per chunk at most
WALL_FORCE_RECORD, WALL_FORCE_SUMS, WALL_FORCE_CHUNK = WINDOW_RECORD, 6, 64
# GFV_PROBE_* of include/gfv.h: words of the record (the window's), doubles per probe and sample
PROBE_RECORD, PROBE_SUMS = WINDOW_RECORD, 9
# GFV_FLOW_* of include/gfv.h: words of the record (the window's), summed and maximised columns per graph, cells per chunk at most
FLOW_RECORD, FLOW_SUMS, FLOW_MAXS, FLOW_CHUNK = WINDOW_RECORD, 10, 2, 64
# GFV_SCHED_* of include/gfv.h: doubles of a schedule record, milestones at most, the modes and the kinds of gfv_lr_schedule
SCHED_RECORD, SCHED_MAX_MILESTONES = 32, 8
SCHED_EVAL, SCHED_TICK, SCHED_FOLLOW = 0, 1, 2
SCHED_STEPEXP, SCHED_EXP, SCHED_GRADUAL, SCHED_TABLE, SCHED_PLATEAU = 1, 2, 3, 4, 5
# GFV_BALANCE_* of include/gfv.h: doubles of a balance record, partial sums of the statistic, the kinds of gfv_loss_balance
BALANCE_RECORD, BALANCE_LANES = 32, 64
BALANCE_INVERSE, BALANCE_PROGRESS = 1, 2
OBS_RECORD = 4   # GFV_OBS_RECORD of include/gfv.h: floats per graph of the record gfv_obs_fwd writes (obs, W, gobs, tot)
POOL_COPY, POOL_ADD, POOL_ROWPTR, POOL_FILL = 0, 1, 2, 3


class PoolArgs(C.Structure):
    """gfv_pool_args_t (include/gfv.h): the arena and the batch of one gfv_pool_assemble launch."""
    _fields_ = [("table_host", C.c_void_p), ("table_dev", C.c_void_p), ("n_entries", C.c_int32), ("n_attrs", C.c_int32),
                ("max_graphs", C.c_int32), ("slice_chunk", C.c_int32), ("max_chunks", C.c_int64),
                ("attr_info", C.c_int32 * POOL_MAX_ATTRS), ("dst", C.c_void_p * POOL_MAX_ATTRS),
                ("dst_cap_words", C.c_int64 * POOL_MAX_ATTRS), ("small", C.c_void_p * 6), ("B", C.c_int32),
                ("reserved", C.c_int32), ("idx", C.c_int32 * POOL_MAX_GRAPHS)]


RENEW_KINDS = {None: 0, "parabolic": 1, "uniform": 2, "uniform_aoa": 3, "Taylor_Green": 4}   # GFV_RENEW_* of include/gfv.h


class RenewRec(C.Structure):
    """gfv_renew_rec_t (include/gfv.h): one entry of a gfv_pool_renew launch."""
    _fields_ = [("x", C.c_void_p), ("y", C.c_void_p), ("theta", C.c_void_p), ("dt", C.c_void_p), ("uvp_dim", C.c_void_p),
                ("node_type", C.c_void_p), ("pos", C.c_void_p), ("yrange", C.c_void_p), ("U", C.c_double), ("cos_aoa", C.c_double),
                ("sin_aoa", C.c_double), ("coef", C.c_float * 13), ("N", C.c_int32), ("inlet_kind", C.c_int32),
                ("init_kind", C.c_int32)]


_lib = None

_SIGNATURES = {
    "gfv_pool_renew": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_pool_args_bytes": (C.c_size_t, []),
    "gfv_pool_table_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gfv_pool_table_check": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_pool_assemble": (C.c_int, [C.POINTER(PoolArgs), C.c_void_p]),
    "gfv_pool_payback": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_int64, C.c_void_p, C.c_void_p]),
    "gfv_abi_version": (C.c_int, []),
    "gfv_struct_size": (C.c_int, [C.c_int32]),
    "gfv_seg_gather_sum": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_seg_gather_sum_nnz": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_int64, C.c_void_p]),
    "gfv_seg_gather_sum_ex": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                        C.c_int32, C.c_int32, C.c_int64, C.c_int64, C.c_void_p]),
    "gfv_seg_gather_sum_ln": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                        C.c_int64, C.c_int64, C.c_void_p]),
    "gfv_transpose_batch": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_status_flags": (C.c_int, [C.POINTER(C.c_int32)]),
    "gfv_status_mirror": (C.c_int, [C.POINTER(C.POINTER(C.c_int32))]),
    "gfv_status_publish": (C.c_int, [C.c_void_p]),
    "gfv_profile_enable": (C.c_int, [C.c_int]),
    "gfv_profile_collect": (C.c_int, [C.c_int, C.POINTER(C.c_double)]),
    "gfv_profile_reset": (C.c_int, []),
    "gfv_profile_set_sizes": (C.c_int, [C.c_double, C.c_double]),
    "gfv_gather_pair": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_void_p]),
    "gfv_get_limit": (C.c_int, [C.c_int32]),
    "gfv_set_limit": (C.c_int, [C.c_int32, C.c_int32]),
    "gfv_limit_name": (C.c_char_p, [C.c_int32]),
    "gfv_rowtile_tiles": (C.c_int, [C.c_int32]),
    "gfv_rowtile_chain": (C.c_int, [C.POINTER(RowtileArgs), C.c_void_p]),
    "gfv_rowtile_last_path": (C.c_int, []),
    "gfv_rowtile_ln_rows": (C.c_int, [C.c_int32]),
    "gfv_rowtile_last_ln_rows": (C.c_int, []),
    "gfv_rowtile_dw_partials": (C.c_int, []),
    "gfv_rowtile_dw_partials_m": (C.c_int, [C.c_int32]),
    "gfv_rowtile_fuses_dw": (C.c_int, [C.POINTER(RowtileArgs)]),
    "gfv_dw_chunks": (C.c_int, [C.c_int32]),
    "gfv_linear_dw_workspace_floats": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    "gfv_linear_dw": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(Seg), C.c_int32, C.c_void_p, C.c_int32,
                                C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_linear_dw_ex": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(Seg), C.c_int32, C.c_void_p, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_int32, C.c_void_p]),
    "gfv_linear_dw_gs": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(Seg), C.c_int32, C.c_void_p, C.c_int32,
                                   C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                   C.c_int32, C.c_void_p]),
    "gfv_dw_slabs": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_dw_multi_workspace_floats": (C.c_size_t, [C.c_int32, C.c_int32, C.c_int64]),
    "gfv_dw_multi": (C.c_int, [C.POINTER(DwTile), C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                               C.c_void_p]),
    "gfv_reduce_partials": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_concat_offsets": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_f16split_enabled": (C.c_int, []),
    "gfv_set_f16split": (C.c_int, [C.c_int32]),
    "gfv_set_f16split_thread": (C.c_int, [C.c_int32]),
    "gfv_hidden_size": (C.c_int, []),
    "gfv_set_hidden_size": (C.c_int, [C.c_int32]),
    "gfv_weight_image_bytes": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gfv_weight_absmax": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "gfv_weight_images": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p]),
    "gfv_weight_images_form": (C.c_int, [C.c_void_p]),
    "gfv_reduce_partials_2d": (C.c_int, [C.c_void_p, C.c_int32, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gfv_reduce_multi": (C.c_int, [C.POINTER(ReducePiece), C.c_int32, C.c_void_p]),
    "gfv_reduce_partials_seg": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gfv_transpose": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_slice_softmax_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_slice_softmax_bwd_blocks": (C.c_int, [C.c_int32]),
    "gfv_slice_softmax_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_slice_token_partial": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "gfv_slice_attention_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_slice_attention_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_deslice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_slice_gw": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_slice_softmax_token": (C.c_int, [C.c_void_p] * 7 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_slice_post_bwd": (C.c_int, [C.c_void_p] * 14 + [C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_phi_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_phi_fwd_ts": (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_phi_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_wlsq_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_wlsq_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_wlsq_fwd_ex": (C.c_int, [C.c_void_p] * 8 + [C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_wlsq_bwd_ex": (C.c_int, [C.c_void_p] * 10 + [C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_wlsq_fwd_full": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_wlsq_bwd_full": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_face_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_cell_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_cell_fwd_ex": (C.c_int, [C.c_void_p] * 19 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gfv_graph_loss": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_cell_to_node": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_fvm_bwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_fvm_bwd_ex": (C.c_int, [C.c_void_p] * 26 + [C.c_int32] * 4 + [C.c_void_p] * 3),
    "gfv_khop_workspace_ints": (C.c_size_t, [C.c_int32, C.c_int32]),
    "gfv_khop_count": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gfv_khop_fill": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_wlsq_moments": (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_interp2_fwd": (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_interp2_bwd": (C.c_int, [C.c_void_p] * 6 + [C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_graph_norm_stats": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "gfv_graph_norm_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "gfv_graph_norm_stats_ws": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_normalizer_blocks": (C.c_int, [C.c_int32]),
    "gfv_normalizer_update": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_node_prep": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_edge_attr": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_adam_step_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_adam_step_guarded_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "gfv_grad_accum_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_grad_guard_accum_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    "gfv_adam_step_accum_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "gfv_ema_init": (C.c_int, [C.c_void_p, C.c_float, C.c_int32, C.c_int32, C.c_void_p]),
    "gfv_adam_step_ema_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_adam_step_groups_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "gfv_grad_guard_workspace_bytes": (C.c_size_t, []),
    "gfv_grad_guard_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_prep_workspace_bytes": (C.c_size_t, [C.c_int32]),
    "gfv_prep_stats": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_prep_apply": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "gfv_fvm_fwd_tail": (C.c_int, [C.POINTER(FvmMesh)] + [C.c_void_p] * 11),
    "gfv_fvm_bwd_fused": (C.c_int, [C.POINTER(FvmMesh)] + [C.c_void_p] * 10),
    "gfv_adam_state_init": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_float, C.c_void_p]),
    "gfv_train_loss_dev": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_train_loss": (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_plan_create": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p]),
    "gfv_plan_destroy": (C.c_int, [C.c_void_p]),
    "gfv_plan_table": (C.c_int, [C.c_void_p, C.c_int32, C.POINTER(C.c_void_p), C.POINTER(C.c_int64)]),
    "gfv_plan_sizes": (C.c_int, [C.c_void_p, C.POINTER(C.c_int64)]),
    "gfv_rollout_advance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                      C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    "gfv_sweep_mirror_create": (C.c_int, [C.c_int32, C.POINTER(C.POINTER(C.c_int32)), C.POINTER(C.c_void_p)]),
    "gfv_sweep_mirror_free": (C.c_int, [C.POINTER(C.c_int32)]),
    "gfv_sweep_advance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "gfv_march_advance": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                    C.c_int32] + [C.c_void_p] * 6 + [C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                                                     C.c_void_p, C.c_void_p]),
    "gfv_field_stats_update": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_time_bc_update": (C.c_int, [C.c_void_p] * 7 + [C.c_int32, C.c_int32] + [C.c_void_p] * 4 + [C.c_int32] + [C.c_void_p] * 3
                           + [C.c_int32] * 3 + [C.c_void_p]),
    "gfv_time_scheme_update": (C.c_int, [C.c_void_p] * 4 + [C.c_int32, C.c_int32] + [C.c_void_p] * 6),
    "gfv_step_control_rate": (C.c_int, [C.c_void_p] * 8 + [C.c_int32, C.c_int32] + [C.c_void_p] * 14 + [C.c_int32, C.c_void_p]),
    "gfv_step_control_rows": (C.c_int, [C.c_void_p] * 3 + [C.c_int32, C.c_int32] + [C.c_void_p] * 6),
    "gfv_wall_force_grad": (C.c_int, [C.c_void_p] * 9 + [C.c_int32, C.c_int32] + [C.c_void_p] * 4),
    "gfv_wall_force_sum": (C.c_int, [C.c_void_p] * 3 + [C.c_int32] + [C.c_void_p] * 9 + [C.c_int32] * 3 + [C.c_void_p] * 7
                           + [C.c_int32, C.c_void_p]),
    "gfv_probe_sample": (C.c_int, [C.c_void_p] * 6 + [C.c_int32] + [C.c_void_p] * 4 + [C.c_int32, C.c_void_p]),
    "gfv_flow_integrals": (C.c_int, [C.c_void_p] * 13 + [C.c_int32] * 3 + [C.c_void_p] * 5 + [C.c_int32, C.c_void_p, C.c_void_p]),
    "gfv_lr_schedule": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_loss_balance": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "gfv_obs_fwd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
                    + [C.c_void_p] * 11),
    "gfv_obs_bwd": (C.c_int, [C.c_void_p] * 9 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "gfv_obs_gather": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "gfv_eval_collect": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                   C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                   C.c_void_p]),
    "gfv_train_log_chunks": (C.c_int64, [C.c_int64]),
    "gfv_train_log_workspace_bytes": (C.c_size_t, [C.c_int64]),
    "gfv_train_log_row_words": (C.c_int32, [C.c_int32, C.c_int32]),
    "gfv_train_log_norms": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                      C.c_void_p]),
    "gfv_train_log_append": (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_void_p]),
    "gfv_anderson_gram": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_int32, C.c_double, C.c_double, C.c_int32] + [C.c_void_p] * 10 + [C.c_int32, C.c_void_p,
                                                                                                         C.c_void_p]),
    "gfv_anderson_mix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                   C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                   C.c_void_p]),
    "gfv_sweep_anderson_gram": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                          C.c_int32, C.c_double, C.c_double, C.c_int32, C.c_int32] + [C.c_void_p] * 14),
    "gfv_sweep_anderson_mix": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_double, C.c_int32] + [C.c_void_p] * 6),
    "gfv_sweep_advance_aa": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                       C.c_int32] + [C.c_void_p] * 10),
    "gfv_trans_mlp_fwd": (C.c_int, [C.POINTER(TransMlp), C.c_void_p]),
    "gfv_trans_mlp_bwd": (C.c_int, [C.POINTER(TransMlpBwd), C.c_void_p]),
    "gfv_trans_mlp_ln_rows": (C.c_int, [C.c_int32]),
    "gfv_record_begin": (C.c_int, []),
    "gfv_record_count": (C.c_int, []),
    "gfv_record_end": (C.c_int64, []),
    "gfv_record_length": (C.c_int, [C.c_int64]),
    "gfv_record_replay": (C.c_int, [C.c_int64, C.c_int32, C.c_int32]),
    "gfv_record_free": (C.c_int, [C.c_int64]),
    "gfv_stream_wait": (C.c_int, [C.c_void_p, C.c_void_p]),
    "gfv_record_delay_side": (C.c_int, [C.c_int64, C.c_void_p, C.c_int32]),
    "gfv_lbfgs_workspace_doubles": (C.c_size_t, [C.c_int32, C.c_int64]),
    "gfv_lbfgs_pair": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_double, C.c_int32, C.c_void_p]),
    "gfv_lbfgs_multidot": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                     C.c_void_p]),
    "gfv_lbfgs_coef": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_int32,
                                 C.c_void_p]),
    "gfv_lbfgs_combine": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_void_p, C.c_void_p]),
    "gfv_lbfgs_dot": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                C.c_void_p]),
    "gfv_lbfgs_axpy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.c_void_p]),
}


class PlanDesc(C.Structure):
    """gfv_plan_desc_t (include/gfv.h)."""
    _fields_ = [("n_nodes", C.c_int64), ("n_faces", C.c_int64), ("n_cells", C.c_int64), ("n_incidences", C.c_int64),
                ("n_stencil_pairs", C.c_int64), ("n_support_pairs", C.c_int64),
                ("edge_index", C.c_void_p), ("cells_node", C.c_void_p), ("cells_face", C.c_void_p),
                ("cells_index", C.c_void_p), ("face_node_x", C.c_void_p), ("support_edge", C.c_void_p)]


# table ids of gfv_plan_table, in the order of the enum in include/gfv.h
PLAN_TABLES = ("ES", "ER", "N_ROWPTR", "N_COL_NODE", "N_COL_EDGE2", "INV_DEG", "S_ROWPTR", "S_COL", "R_ROWPTR", "R_COL",
               "X_ROWPTR", "X_OUT", "X_ORDER", "XO_ROWPTR", "XO_IN", "XO_ORDER", "CROW", "K_ORDER", "KFACE", "KNODE", "KCELL",
               "FROW", "FK", "NROW", "NCELL")


def declared_symbols():
    return list(_SIGNATURES)


def register(name, restype, argtypes):
    _SIGNATURES[name] = (restype, argtypes)
    if _lib is not None:
        fn = getattr(_lib, name)
        fn.restype, fn.argtypes = restype, argtypes


_recording = None   # gfv.cmdlist: while a step is being recorded, launches go through a noting proxy


def load(raw=False):
    """Load libgfv.so or raise.  No CPU / PyTorch fallback exists for the product path."""
    global _lib
    if _lib is not None:
        return _lib if (_recording is None or raw) else _recording
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"libgfv.so not found at {LIB_PATH}: build it with `python gen-fvgn-steady_amd/gfv/build.py` "
            "(hipcc --offload-arch=gfx950). The HIP extension is mandatory; there is no fallback path.")
    lib = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in _SIGNATURES.items():
        fn = getattr(lib, name)  # raises AttributeError if the symbol is missing
        fn.restype, fn.argtypes = restype, argtypes
    # the binding and the library must agree on the ABI: version and the layout of every argument struct
    if lib.gfv_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libgfv.so has ABI {lib.gfv_abi_version()}, this binding is written for {ABI_VERSION}: rebuild it "
                           "(python gen-fvgn-steady_amd/gfv/build.py)")
    for which, st in enumerate((Seg, Layer, RowtileArgs, WimgDesc, DwTile, ReducePiece, PlanDesc, TransMlp, TransMlpBwd, FvmMesh,
                                RenewRec)):
        if lib.gfv_struct_size(which) != C.sizeof(st):
            raise RuntimeError(f"libgfv.so: struct {st.__name__} is {lib.gfv_struct_size(which)} bytes in the library, "
                               f"{C.sizeof(st)} in the binding")
    if lib.gfv_pool_args_bytes() != C.sizeof(PoolArgs):
        raise RuntimeError(f"libgfv.so: gfv_pool_args_t is {lib.gfv_pool_args_bytes()} bytes in the library, "
                           f"{C.sizeof(PoolArgs)} in the binding")
    _lib = lib
    return lib if (_recording is None or raw) else _recording


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def stream_wait(waiter, waited):
    """`waiter.wait_stream(waited)` through the library (include/gfv.h gfv_stream_wait): the same event record + stream wait,
    and part of a natively recorded step (gfv/cmdlist.py)."""
    check(load().gfv_stream_wait(C.c_void_p(waiter.cuda_stream), C.c_void_p(waited.cuda_stream)), "gfv_stream_wait")


_limit_ids = None


def limit_id(name):
    """Index of a dispatch limit (csrc/gfv_limits.h) by the name of its environment variable, e.g. "GFV_CBWD_MAX_M"."""
    global _limit_ids
    if _limit_ids is None:
        lib, ids, i = load(raw=True), {}, 0
        while True:
            n = lib.gfv_limit_name(i)
            if not n:
                break
            ids[n.decode()] = i
            i += 1
        _limit_ids = ids
    return _limit_ids[name]


def get_limit(name):
    return load(raw=True).gfv_get_limit(limit_id(name))


class limits:
    """`with L.limits(GFV_CBWD_MAX_M=100000): ...` - move dispatch limits for the duration of a block (tests, A/B tools)."""

    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        lib = load(raw=True)
        self.old = {k: lib.gfv_get_limit(limit_id(k)) for k in self.kw}
        for k, v in self.kw.items():
            check(lib.gfv_set_limit(limit_id(k), int(v)), "gfv_set_limit")
        return self

    def __exit__(self, *exc):
        lib = load(raw=True)
        for k, v in self.old.items():
            lib.gfv_set_limit(limit_id(k), v)
        return False


MAX_PARAM_GROUPS, MAX_PARAM_RUNS, GROUP_FROZEN = 32, 1024, 1   # GFV_MAX_PARAM_GROUPS, GFV_MAX_PARAM_RUNS, GFV_GROUP_FROZEN (include/gfv.h gfv_adam_step_groups_dev)
GUARD_CLIP, GUARD_SKIP_NONFINITE, GUARD_SKIP_FLAG = 1, 2, 4   # policy / decision bits of guard[8] (include/gfv.h gfv_grad_guard_dev)
FLAG_NAMES = {1: "GFV_FLAG_DW_RANGE (a weight-gradient operand left the fp16 range)",
              2: "GFV_FLAG_CHAIN_RANGE (a hidden activation left the fixed-scale fp16 window of the column-owner chain kernels)"}
_status_word = None


def status_mirror():
    """The library's pinned, device-mapped copy of the status word (include/gfv.h gfv_status_mirror) as a ctypes int32
    pointer; kernels that end a step publish into it, the host reads it without a synchronisation."""
    global _status_word
    if _status_word is None:
        p = C.POINTER(C.c_int32)()
        check(load(raw=True).gfv_status_mirror(C.byref(p)), "gfv_status_mirror")
        _status_word = p
    return _status_word


def status_publish():
    """Enqueue the publication of the status word on the current stream (callers without the fused Adam at their end)."""
    status_mirror()
    check(load().gfv_status_publish(stream_ptr()), "gfv_status_publish")


def raise_on_status(where):
    """Non-blocking check of what the kernels of EARLIER steps raised: a non-zero mirror is cleared (together with the device
    word: that one read synchronises, on the error path only) and turned into a FloatingPointError naming the flags."""
    w = status_mirror()
    v = int(w[0])
    if not v:
        return
    w[0] = 0
    flags = C.c_int32(0)
    load(raw=True).gfv_status_flags(C.byref(flags))   # clears the device word
    v |= int(flags.value)
    names = [n for bit, n in FLAG_NAMES.items() if v & bit] or [f"flags {v:#x}"]
    raise FloatingPointError(f"libgfv status word raised before {where}: " + "; ".join(names) + ".  The split-fp16 products of that "
                             "step lost fp32 accuracy (or overflowed): run with GFV_F16SPLIT=0 (fp32 MFMA) or rescale the model")


def ptr(t):
    if t is None:
        return None
    assert t.is_cuda, "libgfv works on device memory only"
    return t.data_ptr()


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"libgfv: {what} failed with code {rc}")


def f32c(t):
    assert t.dtype == torch.float32 and t.is_contiguous(), (t.dtype, t.is_contiguous())
    return t


def i32c(t):
    assert t.dtype == torch.int32 and t.is_contiguous()
    return t
