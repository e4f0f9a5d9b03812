"""hnsw_rs_amd -- MI355X-native HNSW search engine behind the API of the Rust `hnsw` crate of
Gumo-A/hnsw_rs.  The product is libhnsw_mi355x.so (HIP kernels for gfx950 + host index, C ABI in
include/hnsw_mi355x.h); this package is its thin host-side mirror of the reference's interface.
"""
from ._lib import (DIVERSE_POOL_MAX, DROP_MAX_N, FROM_ROWS_MAX_TERMS, FUSE_MAX_CANDS, FUSE_MIN, FUSE_SUM, GROUP_POOL_MAX, LATE_MAX_CANDS, LATE_MAX_DOCS, LATE_MAX_VECS, LATE_SUM, LATE_SUM_SQ, MASK_NONE, MULTI_MAX_VECS, RADIUS_MAX_N, RADIUS_MORE, RANGES_MAX, VEC_F32, VEC_QUANT8, UINT32_MAX,  # noqa: F401
                   HnswError, lib)
from .hnsw import (HNSW, Graph, MaskSet, Point, device_count, draw_levels, kernel_log, kernel_name, pack_allow,  # noqa: F401
                   pack_allow_many, pack_ranges, synth_rows)
from .grouped import group_by_label  # noqa: F401
from .diverse import mmr_select  # noqa: F401
from .from_rows import compose_rows, drop_ids  # noqa: F401
from .multi import fuse_lists  # noqa: F401
from .late import late_interaction  # noqa: F401
from .docs import score_documents  # noqa: F401
from ._lib import DOCS_MAX_IN, DOCS_MAX_ROWS  # noqa: F401
from .refine import RowTable, f32_to_f16, refine_device, refine_lists  # noqa: F401
from ._lib import REFINE_MAX_DIM, REFINE_POOL_MAX, ROWS_F16, ROWS_F32  # noqa: F401
from .hybrid import admissible_of, filters_of, fuse_ranked  # noqa: F401
from ._lib import HYBRID_LINEAR, HYBRID_MAX_EXT, HYBRID_RRF  # noqa: F401
from .boost import boost_device, boost_lists  # noqa: F401
from ._lib import BOOST_MAX_ATTRS, BOOST_POOL_MAX  # noqa: F401
from .radius import radius_cut, radius_ladder, to_csr  # noqa: F401
from .partitioned import PartitionedIndex, merge_topk  # noqa: F401
