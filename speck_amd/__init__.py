"""speck_amd -- MI355X-native SpGEMM (C = A*B, CSR in / CSR out) behind the spECK host API.

The product is the C-ABI shared library ``libspeck_amd.so`` (hand-written HIP for gfx950,
sources under ``speck_amd/csrc``); this package is only the thin ctypes mirror of the
reference's host interface used by the tests and the benchmark harness.
"""
from .api import (  # noqa: F401
    SpeckError, Timings, dCSR, spECKConfig, HostCSR, MultiplyspECK, BoundMultiply, analysis, symbolic,
    partition_rows, compare, compare_bounded, transpose, gen_matrix, load_matrix, load_mtx, store_mtx, load_hicsr,
    store_hicsr, lib_path, sort_rows, SortInfo, SORT_REG_MAX, SORT_LDS_MAX,
    TRANSPOSE_TILE, TRANSPOSE_BLOCKS, TRANSPOSE_WAVE_SHARE, COMPARE_MAX_WAVES, COPY_MAX_THREADS,
    multiply_masked, MaskedInfo, MASK_GROUP_MAX, MASK_LDS_MAX,
    select, tril, triu, SelectInfo, SELECT_TILE_ROWS, SELECT_LONG_ROW_AVG,
    SELECT_BAND, SELECT_ABS, SELECT_PATTERN, SELECT_NOT_BAND, SELECT_NOT_ABS, SELECT_NOT_PATTERN,
    add, symmetrize, AddInfo, ADD_UNION, ADD_TILE_ROWS, ADD_LONG_ROW_AVG, ADD_TILE_ENTRIES,
    reduce, ReduceInfo, REDUCE_SUM, REDUCE_ABS_SUM, REDUCE_SQ_SUM, REDUCE_MAX, REDUCE_MIN, REDUCE_ABS_MAX, REDUCE_OPS,
    REDUCE_TILE_ENTRIES, REDUCE_THREAD_ENTRIES, REDUCE_WAVE_ENTRIES,
    scale, normalize_rows, pattern_ones, ScaleInfo, MAP_IDENTITY, MAP_ABS, MAP_SQUARE, MAP_ONE, SCALE_MAPS,
    SCALE_NONE, SCALE_MUL, SCALE_DIV, SCALE_TILE_ENTRIES,
    spmv, SpmvInfo, SPMV_TILE_ENTRIES,
    spmm, SpmmInfo, SPMM_MAX_RHS, SPMM_COLUMN_BLOCK, SPMM_COLUMN_BLOCK_B32,
    TransposePlan, transpose_plan, TplanInfo, spmm_t, spmv_t, SpmmTInfo,
    from_coo, from_edge_index, to_coo, FromCooInfo, COO_TILE_ENTRIES,
    extract, gather_rows, select_columns, induced_subgraph, permute, ExtractInfo, EXTRACT_TILE_ENTRIES,
    topk, TopKInfo, TOPK_LARGEST, TOPK_SMALLEST, TOPK_LARGEST_ABS, TOPK_MODES, TOPK_GROUP_MAX, TOPK_LDS_MAX,
    sample_neighbors, SampleInfo, SAMPLE_WITHOUT_REPLACEMENT, SAMPLE_WITH_REPLACEMENT, SAMPLE_GROUP_MAX, SAMPLE_LDS_MAX,
    SAMPLE_TILE_ENTRIES,
    bmat, vstack, hstack, block_diag, bmat_layout, BmatInfo, BmatLayout, BMAT_TILE_ENTRIES, BMAT_MAX_BLOCKS,
    sddmm, sddmm_lanes, SddmmInfo, SDDMM_MAX_K, SDDMM_TILE_ENTRIES, SDDMM_AXPBY, SDDMM_HADAMARD, SDDMM_MODES,
    softmax, softmax_backward, SoftmaxInfo, SOFTMAX_NORMALIZED, SOFTMAX_EXP, SOFTMAX_BACKWARD, SOFTMAX_MODES,
    SOFTMAX_TILE_ENTRIES,
    spmv_sr, spmm_sr, SemiringInfo, SEMIRINGS, SR_MIN_PLUS, SR_MAX_PLUS, SR_MIN_TIMES, SR_MAX_TIMES, SR_MIN_SECOND,
    SR_MAX_SECOND,
)
from .graph import sssp, connected_components  # noqa: F401
