"""ctypes loader for libspeck_amd.so.  Fails loudly: there is no fallback path."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# (SPECK_LIB: another build of the same library, e.g. the sanitizer build of `make ASAN=1`)
LIB_PATH = os.environ.get("SPECK_LIB") or os.path.join(_HERE, "libspeck_amd.so")

NUM_SYM_BINS = 16
NUM_NUM_BINS = 16


class DCsr(C.Structure):
    # field-for-field include/speck_c_api.h: speck_dcsr (reference dCSR<T>, include/dCSR.h:9-16)
    _fields_ = [("rows", C.c_uint64), ("cols", C.c_uint64), ("nnz", C.c_uint64),
                ("data", C.c_void_p), ("row_offsets", C.c_void_p), ("col_ids", C.c_void_p)]


class CTimings(C.Structure):
    _fields_ = [("measureAll", C.c_int32), ("measureCompleteTime", C.c_int32)] + [
        (n, C.c_float) for n in ("init", "countProducts", "loadBalanceCounting", "globalMapsCounting",
                                 "spGEMMCounting", "allocC", "loadBalanceNumeric",
                                 "globalMapsNumeric", "spGEMMNumeric", "sorting", "cleanup",
                                 "complete")]


class CStats(C.Structure):
    _fields_ = [("sum_products", C.c_uint64), ("nnz_c", C.c_uint64), ("max_row_ops", C.c_uint32),
                ("max_row_nnz_c", C.c_uint32),
                ("sym_bin_rows", C.c_uint32 * NUM_SYM_BINS), ("num_bin_rows", C.c_uint32 * NUM_NUM_BINS),
                ("num_bin_bytes", C.c_uint64 * NUM_NUM_BINS), ("sym_bin_bytes", C.c_uint64 * NUM_SYM_BINS),
                ("num_bin_ms", C.c_float * NUM_NUM_BINS), ("sym_bin_ms", C.c_float * NUM_SYM_BINS),
                ("analysis_ms", C.c_float), ("scan_ms", C.c_float),
                ("sym_light_ms", C.c_float), ("num_light_ms", C.c_float),
                ("sym_tiny_ms", C.c_float), ("num_tiny_ms", C.c_float),
                ("kernel_events_valid", C.c_int32), ("numeric_reruns", C.c_int32),
                ("graph_replays", C.c_int32), ("graph_captures", C.c_int32),
                ("sym_phase_ms", C.c_float), ("num_phase_ms", C.c_float),
                ("replayed", C.c_int32), ("nf_direct", C.c_int32), ("pool_fallbacks", C.c_int32),
                ("esc_fused", C.c_int32), ("scratch_pool_bytes", C.c_uint64),
                ("pred_stages", C.c_int32), ("eager_speculated", C.c_int32), ("one_walk", C.c_int32),
                ("walk_misses", C.c_int32), ("eager_through", C.c_int32)]


class CSortInfo(C.Structure):
    # include/speck_c_api.h: speck_sort_info
    _fields_ = [("rows_in_order", C.c_uint64), ("rows_sorted", C.c_uint64 * 3), ("duplicates", C.c_uint64),
                ("nnz_out", C.c_uint64)]


class CMaskedInfo(C.Structure):
    # include/speck_c_api.h: speck_masked_info
    _fields_ = [("rows_idle", C.c_uint64), ("rows_class", C.c_uint64 * 3), ("products", C.c_uint64), ("hits", C.c_uint64),
                ("nnz_out", C.c_uint64)]


class CSelectParams(C.Structure):
    # include/speck_c_api.h: speck_select_params
    _fields_ = [("flags", C.c_uint32), ("band_lo", C.c_int64), ("band_hi", C.c_int64), ("row_base", C.c_uint64),
                ("abs_threshold", C.c_double), ("pattern", C.POINTER(DCsr))]


class CSelectInfo(C.Structure):
    # include/speck_c_api.h: speck_select_info
    _fields_ = [("kept", C.c_uint64), ("dropped", C.c_uint64), ("rows_unchanged", C.c_uint64), ("nnz_out", C.c_uint64)]


class CAddInfo(C.Structure):
    # include/speck_c_api.h: speck_add_info
    _fields_ = [("only_a", C.c_uint64), ("only_b", C.c_uint64), ("both", C.c_uint64), ("nnz_out", C.c_uint64)]


class CReduceInfo(C.Structure):
    # include/speck_c_api.h: speck_reduce_info
    _fields_ = [("rows_empty", C.c_uint64), ("rows_split", C.c_uint64), ("tiles", C.c_uint64), ("entries", C.c_uint64)]


class CScaleParams(C.Structure):
    # include/speck_c_api.h: speck_scale_params
    _fields_ = [("map", C.c_uint32), ("row_mode", C.c_uint32), ("col_mode", C.c_uint32), ("alpha", C.c_double),
                ("d_row", C.c_void_p), ("d_col", C.c_void_p)]


class CScaleInfo(C.Structure):
    # include/speck_c_api.h: speck_scale_info
    _fields_ = [("entries", C.c_uint64), ("nonfinite", C.c_uint64), ("tiles", C.c_uint64)]


class CSpmvInfo(C.Structure):
    # include/speck_c_api.h: speck_spmv_info
    _fields_ = [("rows_empty", C.c_uint64), ("rows_split", C.c_uint64), ("tiles", C.c_uint64), ("entries", C.c_uint64)]


class CSpmmInfo(C.Structure):
    # include/speck_c_api.h: speck_spmm_info
    _fields_ = [("rows_empty", C.c_uint64), ("rows_split", C.c_uint64), ("tiles", C.c_uint64), ("entries", C.c_uint64),
                ("terms", C.c_uint64)]


class CSemiringInfo(C.Structure):
    # include/speck_c_api.h: speck_semiring_info
    _fields_ = [("rows_empty", C.c_uint64), ("rows_split", C.c_uint64), ("tiles", C.c_uint64), ("entries", C.c_uint64),
                ("terms", C.c_uint64), ("changed", C.c_uint64)]


class CSddmmParams(C.Structure):
    # include/speck_c_api.h: speck_sddmm_params
    _fields_ = [("mode", C.c_uint32), ("k", C.c_uint32), ("alpha", C.c_double), ("beta", C.c_double),
                ("d_U", C.c_void_p), ("ldu", C.c_uint64), ("d_V", C.c_void_p), ("ldv", C.c_uint64)]


class CSddmmParamsB32(C.Structure):
    # include/speck_c_api.h: speck_sddmm_params_b32 (speck_sddmm_params with the blocks in float: pointers either way)
    _fields_ = list(CSddmmParams._fields_)


class CSddmmInfo(C.Structure):
    # include/speck_c_api.h: speck_sddmm_info
    _fields_ = [("entries", C.c_uint64), ("terms", C.c_uint64), ("nonfinite", C.c_uint64), ("tiles", C.c_uint64),
                ("lanes", C.c_uint64)]


class CSoftmaxParams(C.Structure):
    # include/speck_c_api.h: speck_softmax_params
    _fields_ = [("mode", C.c_uint32), ("reserved", C.c_uint32), ("alpha", C.c_double), ("d_G", C.c_void_p),
                ("d_row_max", C.c_void_p), ("d_row_sum", C.c_void_p)]


class CSoftmaxInfo(C.Structure):
    # include/speck_c_api.h: speck_softmax_info
    _fields_ = [("entries", C.c_uint64), ("nonfinite", C.c_uint64), ("rows_empty", C.c_uint64), ("rows_split", C.c_uint64),
                ("tiles", C.c_uint64)]


class CTplanInfo(C.Structure):
    # include/speck_c_api.h: speck_tplan_info
    _fields_ = [("rows", C.c_uint64), ("cols", C.c_uint64), ("nnz", C.c_uint64), ("cols_empty", C.c_uint64),
                ("max_col_entries", C.c_uint64), ("bytes", C.c_uint64)]


class CSpmmTInfo(C.Structure):
    # include/speck_c_api.h: speck_spmm_t_info
    _fields_ = [("cols_empty", C.c_uint64), ("cols_split", C.c_uint64), ("tiles", C.c_uint64), ("entries", C.c_uint64),
                ("terms", C.c_uint64)]


class CDcoo(C.Structure):
    # include/speck_c_api.h: speck_dcoo (reference COO<T>, include/COO.h) with the width of its indices
    _fields_ = [("rows", C.c_uint64), ("cols", C.c_uint64), ("nnz", C.c_uint64), ("data", C.c_void_p),
                ("row_ids", C.c_void_p), ("col_ids", C.c_void_p), ("index_bytes", C.c_uint32)]


class CFromCooInfo(C.Structure):
    # include/speck_c_api.h: speck_from_coo_info
    _fields_ = [("entries", C.c_uint64), ("rows_empty", C.c_uint64), ("max_row_entries", C.c_uint64),
                ("sorted_input", C.c_uint64), ("sort_passes", C.c_uint64)]


class CExtractParams(C.Structure):
    # include/speck_c_api.h: speck_extract_params
    _fields_ = [("n_rows", C.c_uint64), ("out_cols", C.c_uint64), ("d_row_index", C.c_void_p), ("d_col_map", C.c_void_p),
                ("index_bytes", C.c_uint32)]


class CExtractInfo(C.Structure):
    # include/speck_c_api.h: speck_extract_info
    _fields_ = [("rows_out", C.c_uint64), ("rows_empty", C.c_uint64), ("gross", C.c_uint64), ("nnz_out", C.c_uint64),
                ("dropped", C.c_uint64), ("cols_kept", C.c_uint64), ("max_row_entries", C.c_uint64)]


class CTopKParams(C.Structure):
    # include/speck_c_api.h: speck_topk_params
    _fields_ = [("k", C.c_uint64), ("mode", C.c_uint32), ("reserved", C.c_uint32)]


class CTopKInfo(C.Structure):
    # include/speck_c_api.h: speck_topk_info
    _fields_ = [("rows", C.c_uint64), ("rows_cut", C.c_uint64), ("entries_in", C.c_uint64), ("nnz_out", C.c_uint64),
                ("dropped", C.c_uint64), ("max_row_entries", C.c_uint64), ("ties_cut", C.c_uint64), ("nan_kept", C.c_uint64)]


class CSampleParams(C.Structure):
    # include/speck_c_api.h: speck_sample_params
    _fields_ = [("k", C.c_uint64), ("seed", C.c_uint64), ("row_base", C.c_uint64), ("n_rows", C.c_uint64),
                ("d_row_index", C.c_void_p), ("index_bytes", C.c_uint32), ("mode", C.c_uint32)]


class CSampleInfo(C.Structure):
    # include/speck_c_api.h: speck_sample_info
    _fields_ = [("rows_out", C.c_uint64), ("rows_empty", C.c_uint64), ("rows_cut", C.c_uint64), ("gross", C.c_uint64),
                ("nnz_out", C.c_uint64), ("max_row_entries", C.c_uint64)]


class CBmatBlock(C.Structure):
    # include/speck_c_api.h: speck_bmat_block
    _fields_ = [("block_row", C.c_uint32), ("block_col", C.c_uint32), ("M", C.POINTER(DCsr))]


class CBmatParams(C.Structure):
    # include/speck_c_api.h: speck_bmat_params
    _fields_ = [("block_rows", C.c_uint32), ("block_cols", C.c_uint32), ("n_blocks", C.c_uint32),
                ("blocks", C.POINTER(CBmatBlock)), ("row_sizes", C.POINTER(C.c_uint64)), ("col_sizes", C.POINTER(C.c_uint64))]


class CBmatInfo(C.Structure):
    # include/speck_c_api.h: speck_bmat_info
    _fields_ = [("blocks", C.c_uint64), ("rows_out", C.c_uint64), ("cols_out", C.c_uint64), ("nnz_out", C.c_uint64),
                ("pieces", C.c_uint64), ("rows_empty", C.c_uint64), ("max_row_entries", C.c_uint64)]


class CBmatLayoutOut(C.Structure):
    # include/speck_c_api.h: speck_bmat_layout_out
    _fields_ = [("rows", C.c_uint64), ("cols", C.c_uint64), ("nnz", C.c_uint64), ("pieces", C.c_uint64),
                ("row_origins", C.POINTER(C.c_uint64)), ("col_origins", C.POINTER(C.c_uint64))]


# every symbol include/speck_c_api.h declares, with its ctypes signature
_P = C.POINTER
_SIGS = {
    "speck_config_create": (C.c_int, [C.c_int, _P(C.c_void_p)]),
    "speck_config_destroy": (C.c_int, [C.c_void_p]),
    "speck_config_info": (C.c_int, [C.c_void_p, _P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    "speck_config_handles": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "speck_config_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "speck_config_set_option": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int64]),
    "speck_config_profile_kernels": (C.c_int, [C.c_void_p, C.c_int]),
    "speck_last_stats": (C.c_int, [C.c_void_p, _P(CStats)]),
    "speck_multiply_f64": (C.c_int, [C.c_void_p, _P(DCsr), _P(DCsr), _P(DCsr), _P(CTimings)]),
    "speck_multiply_f32": (C.c_int, [C.c_void_p, _P(DCsr), _P(DCsr), _P(DCsr), _P(CTimings)]),
    "speck_analysis": (C.c_int, [C.c_void_p, _P(DCsr), _P(DCsr), C.c_void_p, C.c_void_p, C.c_void_p,
                                 C.c_void_p, _P(C.c_uint64), _P(C.c_uint32)]),
    "speck_symbolic": (C.c_int, [C.c_void_p, _P(DCsr), _P(DCsr), C.c_void_p, _P(C.c_uint64)]),
    "speck_partition_rows": (C.c_int, [C.c_void_p, _P(DCsr), _P(DCsr), C.c_int, _P(C.c_uint64)]),
    "speck_dcsr_alloc": (C.c_int, [_P(DCsr), C.c_uint64, C.c_uint64, C.c_uint64, C.c_int, C.c_size_t]),
    "speck_dcsr_free": (C.c_int, [_P(DCsr)]),
    "speck_dcsr_upload": (C.c_int, [_P(DCsr), C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                    C.c_void_p, C.c_void_p, C.c_size_t]),
    "speck_dcsr_upload_padded": (C.c_int, [_P(DCsr), C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32]),
    "speck_dcsr_copy": (C.c_int, [_P(DCsr), _P(DCsr), C.c_size_t, C.c_uint32]),
    "speck_dcsr_download": (C.c_int, [_P(DCsr), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "speck_dcsr_update": (C.c_int, [_P(DCsr), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "speck_compare_f64": (C.c_int, [C.c_void_p, _P(DCsr), _P(DCsr), C.c_int, C.c_double, _P(C.c_uint64)]),
    "speck_transpose_f64": (C.c_int, [C.c_void_p, _P(DCsr), _P(DCsr)]),
    "speck_transpose_f32": (C.c_int, [C.c_void_p, _P(DCsr), _P(DCsr)]),
    "speck_sort_rows_f64": (C.c_int, [C.c_void_p, _P(DCsr), C.c_int, _P(CSortInfo)]),
    "speck_sort_rows_f32": (C.c_int, [C.c_void_p, _P(DCsr), C.c_int, _P(CSortInfo)]),
    "speck_multiply_masked_f64": (C.c_int, [C.c_void_p, _P(DCsr), _P(DCsr), _P(DCsr), _P(DCsr), C.c_int, _P(CMaskedInfo)]),
    "speck_multiply_masked_f32": (C.c_int, [C.c_void_p, _P(DCsr), _P(DCsr), _P(DCsr), _P(DCsr), C.c_int, _P(CMaskedInfo)]),
    "speck_select_f64": (C.c_int, [C.c_void_p, _P(DCsr), _P(CSelectParams), _P(DCsr), _P(CSelectInfo)]),
    "speck_select_f32": (C.c_int, [C.c_void_p, _P(DCsr), _P(CSelectParams), _P(DCsr), _P(CSelectInfo)]),
    "speck_add_f64": (C.c_int, [C.c_void_p, C.c_double, _P(DCsr), C.c_double, _P(DCsr), _P(DCsr), C.c_int, _P(CAddInfo)]),
    "speck_add_f32": (C.c_int, [C.c_void_p, C.c_double, _P(DCsr), C.c_double, _P(DCsr), _P(DCsr), C.c_int, _P(CAddInfo)]),
    "speck_reduce_f64": (C.c_int, [C.c_void_p, _P(DCsr), C.c_int, C.c_void_p, _P(C.c_double), _P(CReduceInfo)]),
    "speck_reduce_f32": (C.c_int, [C.c_void_p, _P(DCsr), C.c_int, C.c_void_p, _P(C.c_double), _P(CReduceInfo)]),
    "speck_scale_f64": (C.c_int, [C.c_void_p, _P(DCsr), _P(CScaleParams), _P(DCsr), _P(CScaleInfo)]),
    "speck_scale_f32": (C.c_int, [C.c_void_p, _P(DCsr), _P(CScaleParams), _P(DCsr), _P(CScaleInfo)]),
    "speck_spmv_f64": (C.c_int, [C.c_void_p, C.c_double, _P(DCsr), C.c_void_p, C.c_double, C.c_void_p, _P(CSpmvInfo)]),
    "speck_spmv_f32": (C.c_int, [C.c_void_p, C.c_double, _P(DCsr), C.c_void_p, C.c_double, C.c_void_p, _P(CSpmvInfo)]),
    "speck_spmm_f64": (C.c_int, [C.c_void_p, C.c_double, _P(DCsr), C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p,
                                 C.c_uint64, _P(CSpmmInfo)]),
    "speck_spmm_f32": (C.c_int, [C.c_void_p, C.c_double, _P(DCsr), C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p,
                                 C.c_uint64, _P(CSpmmInfo)]),
    "speck_spmv_sr_f64": (C.c_int, [C.c_void_p, C.c_int, _P(DCsr), C.c_void_p, C.c_void_p, C.c_void_p, _P(CSemiringInfo)]),
    "speck_spmv_sr_f32": (C.c_int, [C.c_void_p, C.c_int, _P(DCsr), C.c_void_p, C.c_void_p, C.c_void_p, _P(CSemiringInfo)]),
    "speck_spmm_sr_f64": (C.c_int, [C.c_void_p, C.c_int, _P(DCsr), C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64,
                                    C.c_void_p, C.c_uint64, _P(CSemiringInfo)]),
    "speck_spmm_sr_f32": (C.c_int, [C.c_void_p, C.c_int, _P(DCsr), C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_uint64,
                                    C.c_void_p, C.c_uint64, _P(CSemiringInfo)]),
    "speck_sddmm_f64": (C.c_int, [C.c_void_p, _P(DCsr), _P(CSddmmParams), _P(DCsr), _P(CSddmmInfo)]),
    "speck_sddmm_f32": (C.c_int, [C.c_void_p, _P(DCsr), _P(CSddmmParams), _P(DCsr), _P(CSddmmInfo)]),
    "speck_softmax_f64": (C.c_int, [C.c_void_p, _P(DCsr), _P(CSoftmaxParams), _P(DCsr), _P(CSoftmaxInfo)]),
    "speck_softmax_f32": (C.c_int, [C.c_void_p, _P(DCsr), _P(CSoftmaxParams), _P(DCsr), _P(CSoftmaxInfo)]),
    "speck_tplan_create": (C.c_int, [C.c_void_p, _P(DCsr), _P(C.c_void_p), _P(CTplanInfo)]),
    "speck_tplan_destroy": (C.c_int, [C.c_void_p]),
    "speck_spmm_t_f64": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, _P(DCsr), C.c_void_p, C.c_uint64, C.c_uint32, C.c_double,
                                   C.c_void_p, C.c_uint64, _P(CSpmmTInfo)]),
    "speck_spmm_t_f32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, _P(DCsr), C.c_void_p, C.c_uint64, C.c_uint32, C.c_double,
                                   C.c_void_p, C.c_uint64, _P(CSpmmTInfo)]),
    "speck_spmm_f64_b32": (C.c_int, [C.c_void_p, C.c_double, _P(DCsr), C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p,
                                     C.c_uint64, _P(CSpmmInfo)]),
    "speck_spmm_f32_b32": (C.c_int, [C.c_void_p, C.c_double, _P(DCsr), C.c_void_p, C.c_uint64, C.c_uint32, C.c_double, C.c_void_p,
                                     C.c_uint64, _P(CSpmmInfo)]),
    "speck_spmm_t_f64_b32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, _P(DCsr), C.c_void_p, C.c_uint64, C.c_uint32,
                                       C.c_double, C.c_void_p, C.c_uint64, _P(CSpmmTInfo)]),
    "speck_spmm_t_f32_b32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_double, _P(DCsr), C.c_void_p, C.c_uint64, C.c_uint32,
                                       C.c_double, C.c_void_p, C.c_uint64, _P(CSpmmTInfo)]),
    "speck_sddmm_f64_b32": (C.c_int, [C.c_void_p, _P(DCsr), _P(CSddmmParamsB32), _P(DCsr), _P(CSddmmInfo)]),
    "speck_sddmm_f32_b32": (C.c_int, [C.c_void_p, _P(DCsr), _P(CSddmmParamsB32), _P(DCsr), _P(CSddmmInfo)]),
    "speck_from_coo_f64": (C.c_int, [C.c_void_p, _P(CDcoo), _P(DCsr), _P(CFromCooInfo)]),
    "speck_from_coo_f32": (C.c_int, [C.c_void_p, _P(CDcoo), _P(DCsr), _P(CFromCooInfo)]),
    "speck_to_coo": (C.c_int, [C.c_void_p, _P(DCsr), C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p]),
    "speck_extract_f64": (C.c_int, [C.c_void_p, _P(DCsr), _P(CExtractParams), _P(DCsr), _P(CExtractInfo)]),
    "speck_extract_f32": (C.c_int, [C.c_void_p, _P(DCsr), _P(CExtractParams), _P(DCsr), _P(CExtractInfo)]),
    "speck_topk_f64": (C.c_int, [C.c_void_p, _P(DCsr), _P(CTopKParams), _P(DCsr), _P(CTopKInfo)]),
    "speck_topk_f32": (C.c_int, [C.c_void_p, _P(DCsr), _P(CTopKParams), _P(DCsr), _P(CTopKInfo)]),
    "speck_sample_f64": (C.c_int, [C.c_void_p, _P(DCsr), _P(CSampleParams), _P(DCsr), _P(CSampleInfo)]),
    "speck_sample_f32": (C.c_int, [C.c_void_p, _P(DCsr), _P(CSampleParams), _P(DCsr), _P(CSampleInfo)]),
    "speck_bmat_layout": (C.c_int, [_P(CBmatParams), _P(CBmatLayoutOut)]),
    "speck_bmat_f64": (C.c_int, [C.c_void_p, _P(CBmatParams), _P(DCsr), _P(CBmatInfo)]),
    "speck_bmat_f32": (C.c_int, [C.c_void_p, _P(CBmatParams), _P(DCsr), _P(CBmatInfo)]),
    "speck_compare_f32": (C.c_int, [C.c_void_p, _P(DCsr), _P(DCsr), C.c_int, C.c_double, _P(C.c_uint64)]),
    "speck_compare_bounded_f64": (C.c_int, [C.c_void_p, _P(DCsr), _P(DCsr), _P(DCsr), C.c_double, _P(C.c_uint64),
                                            _P(C.c_uint64)]),
    "speck_gen_matrix": (C.c_int, [C.c_char_p, C.c_double, C.c_uint64, C.c_int, _P(C.c_void_p)]),
    "speck_load_mtx": (C.c_int, [C.c_char_p, _P(C.c_void_p)]),
    "speck_store_mtx": (C.c_int, [C.c_void_p, C.c_char_p, C.c_int]),
    "speck_load_hicsr": (C.c_int, [C.c_char_p, _P(C.c_void_p)]),
    "speck_store_hicsr": (C.c_int, [C.c_void_p, C.c_char_p]),
    "speck_load_matrix": (C.c_int, [C.c_char_p, C.c_int, _P(C.c_void_p)]),
    "speck_host_csr_dims": (C.c_int, [C.c_void_p, _P(C.c_uint64), _P(C.c_uint64), _P(C.c_uint64)]),
    "speck_host_csr_copy": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "speck_host_csr_from_arrays": (C.c_int, [C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p,
                                             C.c_void_p, _P(C.c_void_p)]),
    "speck_host_csr_free": (C.c_int, [C.c_void_p]),
    "speck_comm_unique_id": (C.c_int, [C.c_int, C.c_void_p]),
    "speck_comm_init": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, _P(C.c_void_p)]),
    "speck_comm_destroy": (C.c_int, [C.c_void_p]),
    "speck_comm_info": (C.c_int, [C.c_void_p, _P(C.c_int), _P(C.c_int), _P(C.c_int)]),
    "speck_gatherv_csr": (C.c_int, [C.c_void_p, C.c_int, _P(DCsr), C.c_uint64, C.c_size_t, _P(DCsr)]),
    "speck_gather_plan_create": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_size_t,
                                           C.c_int, _P(C.c_void_p)]),
    "speck_gather_start": (C.c_int, [C.c_void_p, C.c_int, _P(DCsr)]),
    "speck_gather_wait": (C.c_int, [C.c_void_p, C.c_int, _P(DCsr)]),
    "speck_gather_plan_layout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "speck_gather_plan_destroy": (C.c_int, [C.c_void_p]),
    "speck_status_string": (C.c_char_p, [C.c_int]),
    "speck_version": (C.c_char_p, []),
}

_LIB = None


def load():
    """Load libspeck_amd.so (built in-tree by `make` / __graft_entry__.build())."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build the HIP extension first (`make` or "
            "`python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGS.items():
        fn = getattr(lib, name)  # AttributeError = a declared symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _LIB = lib
    return lib


def declared_symbols():
    return sorted(_SIGS)
