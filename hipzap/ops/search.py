"""Vector search kernels (csrc/search.hip): exact top-k by inner product over a bf16 corpus.

``HzSearchParams`` is the parameter block of both kinds: ``HZ_K_SEARCH_SCAN`` (one workgroup per tile
of ``tile_rows()`` corpus rows, all queries of the launch resident in LDS, the tile's best ``k`` keys per
query into ``cand``) and ``HZ_K_SEARCH_MERGE`` (one workgroup per query, ``ntile x k`` keys -> the final
``k``). ``HZ_K_SEARCH_FSCAN`` (``FilterScanParams``: the same block plus a live bitmap, per-row tags and
per-query ``{mask, value}`` filters) is the scan over the rows that pass. ``HZ_K_SEARCH_QSCAN``
(``QuantScanParams``: that block plus one fp32 scale per row) is the filtered scan over rows of OCP e4m3fn bytes.
``HZ_K_SEARCH_BSCAN`` (``BinScanParams``: the filtered block over uint32 sign-bit rows, ``ldc`` in words) scores
``D - 2 popcount(query bits xor row bits)``, the queries binarised in the kernel.
``HZ_K_SEARCH_BXSCAN`` (``BinBatchScanParams``) is that scan for any number of queries: a workgroup walks a slab of
``span`` tiles for 32 queries with a running top-k and a threshold, and ``HZ_K_SEARCH_MERGEN`` reduces the slab lists.
``HZ_K_SEARCH_RESCORE`` (``RescoreParams``) is the second stage of a two-stage search: one workgroup per query
re-scores the ``R`` bf16 rows that a merge's ``out_id`` names and writes the best ``k`` of them.
``HZ_K_SEARCH_LSCAN`` (``ListScanParams``) is the filtered scan over an IVF index's lists: workgroup (j, q) scans
the j-th tile of the lists that ``probes[q]`` names; ``HZ_K_SEARCH_QLSCAN`` (``QuantListScanParams``: that block plus
one fp32 scale per stored row) is the list scan over rows of e4m3fn bytes.
``HZ_K_SEARCH_MSCAN`` (``SelfScanParams``) scores rows of the corpus, named by ``qid``, against every tile with the
bf16 MFMA, ``SELF_QB`` queries a workgroup; ``HZ_K_SEARCH_MERGEN`` is the merge for any number of queries over the
same block.
``HZ_K_SEARCH_XSCAN`` (``BatchScanParams``: that block with device fp32 ``queries`` where ``qid`` is) is the self scan
over external queries, each split into three bf16 terms; ``HZ_K_SEARCH_MERGEN`` takes its block as it stands and
``HZ_K_SEARCH_RESCOREN`` is the rescore (``RescoreParams``) for any number of queries.
``HZ_K_SEARCH_PQXSCAN`` (``PqBatchScanParams``: the batch block over uint8 code rows, ``ldc`` in bytes, plus the bf16
table ``cb8`` of :func:`hipzap.search.pq_table_bf16`) is the batch scan over product-quantised rows, each MFMA fragment
gathered from that table by a code byte; ``HZ_K_SEARCH_PQRESCORE`` (``PqRescoreParams``) re-scores its candidates with ``HZ_K_SEARCH_PQSCAN``'s bits.
``HZ_K_SEARCH_QXSCAN`` (``QuantBatchScanParams``: the batch block over e4m3 byte rows, ``ldc`` in bytes, plus ``scales``)
is the batch scan over fp8 rows, decoded to bf16 in registers; ``HZ_K_SEARCH_LXSCAN`` (``ListBatchScanParams``) is the batch
scan over a work list of (stored tile, up to 64 queries) items of an IVF index and ``HZ_K_SEARCH_RESCOREP``
(``RescorePosParams``) the rescore of external ids against rows in stored order; ``HZ_K_SEARCH_QRESCORE`` (``QuantRescoreParams``) re-scores
its candidates with ``HZ_K_SEARCH_QSCAN``'s bits.
``HZ_K_SEARCH_ASSIGN`` (``AssignParams``) writes the nearest of ``C`` bf16 centroids for every row of a tile with the
same MFMA, ``HZ_K_SEARCH_CMEAN`` (``CmeanParams``) the means of the clusters ``order`` / ``seg_off`` describe.
``HZ_K_SEARCH_GRAPH`` (``GraphParams``) is the beam search over a fixed-degree neighbour graph of the corpus, one workgroup
per query and the whole walk in one launch; its scores are ``HZ_K_SEARCH_SCAN``'s bits.
``HZ_K_GRAPH_SEED`` (``GraphSeedParams``) scores a query batch against a table of seed rows with the bf16 MFMA and writes
each query's best ``E`` seed ids: the entry rows the walk reads per query (``GraphParams.estride``).
``HZ_K_GRAPH_PRUNE`` (``GraphPruneParams``) reorders kNN lists by their detour counts, one wave per row, integers only
(:func:`hipzap.search.graph_prune_ref` is its result in numpy); ``graph_prune_lists`` is the job over host lists
(``hz_graph_prune``).
``HZ_K_SEARCH_PQLUT`` (``PqLutParams``) writes each query's table of inner products with the 256 sub-centroids of every
sub-space of a product quantiser; ``HZ_K_SEARCH_PQSCAN`` (``PqScanParams``: the filtered block over uint8 code rows,
``ldc`` in bytes, plus the table) adds M table entries per row, one query's table resident in LDS per workgroup.
``HZ_K_SEARCH_PQASSIGN`` (``PqAssignParams``) writes, for every bf16 row and sub-space, the nearest of the 256
sub-centroids under squared L2 in plain fp32 operations (:func:`hipzap.search.pq_assign_f32` is its bits in numpy);
``pq_encode_rows`` is the batch job over host rows built on it (``hz_pq_encode``).
``HZ_K_SEARCH_PQUPDATE`` (``PqUpdateParams``) turns those codes into new sub-centroids: each mean one fp64 sum over its
members in ascending row order from -0.0, divided by the count and rounded to fp32
(:func:`hipzap.search.pq_means_seq` is its bits in numpy); ``pq_train_rows`` is the device-resident training loop over
the two kinds (``hz_pq_train``).
torch-free: indexes (:mod:`hipzap.search`) are served without it."""
from __future__ import annotations

import ctypes as C

from .. import _native as N

MAX_Q, MAX_K = 16, 128  # HZ_SEARCH_MAX_Q, HZ_SEARCH_MAX_K (csrc/hipzap.h)
SELF_QB = 64                     # HZ_SEARCH_SELF_QB: queries per workgroup of the self scan
SELF_MAX_Q = 65535 * SELF_QB     # HZ_SEARCH_SELF_MAX_Q: the self scan's and its merge's limit on Q
INDEX_SELF_MAX_Q = 1024          # HZ_INDEX_SELF_MAX_Q: ids per hz_index_neighbors call
ASSIGN_CB = 64                   # HZ_SEARCH_ASSIGN_CB: centroids per block of the assign kernel
ASSIGN_MAX_C = 65536             # HZ_SEARCH_ASSIGN_MAX_C: the most centroids (hipzap.search.IVF_MAX_LISTS)
PQ_MAX_M, PQ_MAX_DSUB, PQ_KSUB = 96, 64, 256  # HZ_SEARCH_PQ_MAX_M, HZ_SEARCH_PQ_MAX_DSUB; sub-centroids per sub-space
# HZ_SEARCH_PQU_CG, _TILE, _BATCH: centroids per workgroup of the update kernel, rows per tile, members per list batch
PQ_UPDATE_CG, PQ_UPDATE_TILE, PQ_UPDATE_BATCH = 16, 256, 384
# HZ_SEARCH_GRAPH_MAX_BEAM, _CAP_SMALL, _CAP_LARGE: the graph search's beam limit and its two visited tables (slots)
GRAPH_MAX_BEAM, GRAPH_CAP_SMALL, GRAPH_CAP_LARGE = 256, 4096, 16384
GRAPH_THREADS = 256              # one thread per entry and per neighbour slot: E <= 256, width * deg <= 256
GRAPH_SEED_MAX, GRAPH_SEED_MAX_E = 8192, 64  # HZ_GRAPH_SEED_MAX, HZ_GRAPH_SEED_MAX_E: seed ids a table holds, entries per query


@N.params_of("HZ_K_SEARCH_MERGE")
@N.params_of("HZ_K_SEARCH_SCAN")
class SearchParams(C.Structure):
    _fields_ = [("corpus", C.c_void_p), ("queries", C.c_void_p), ("cand", C.c_void_p), ("out_score", C.c_void_p),
                ("out_id", C.c_void_p), ("N", C.c_int), ("D", C.c_int), ("Q", C.c_int), ("k", C.c_int),
                ("ldc", C.c_int), ("ntile", C.c_int), ("cand_bytes", C.c_uint64)]


_FILTER_FIELDS = [("live", C.c_void_p), ("tags", C.c_void_p), ("filt", C.c_void_p), ("live_bytes", C.c_uint64)]


@N.params_of("HZ_K_SEARCH_FSCAN")
class FilterScanParams(C.Structure):
    """HzSearchFilterParams: the fields of ``SearchParams``, then the filter's."""
    _fields_ = SearchParams._fields_ + _FILTER_FIELDS

    def scan_params(self) -> SearchParams:
        """The leading ``SearchParams`` of this block (what the merge takes)."""
        return SearchParams.from_buffer_copy(self)


@N.params_of("HZ_K_SEARCH_QSCAN")
class QuantScanParams(C.Structure):
    """HzSearchQuantParams: the fields of ``FilterScanParams`` (``corpus``: uint8 rows, ``ldc`` in bytes), then
    ``scales`` (fp32 [N])."""
    _fields_ = FilterScanParams._fields_ + [("scales", C.c_void_p)]

    def scan_params(self) -> SearchParams:
        return SearchParams.from_buffer_copy(self)


@N.params_of("HZ_K_SEARCH_BSCAN")
class BinScanParams(C.Structure):
    """HzSearchBinParams: the fields of ``FilterScanParams`` (``corpus``: uint32 sign-bit rows [N][ldc], ``ldc`` in
    words; ``live`` is required)."""
    _fields_ = list(FilterScanParams._fields_)

    def scan_params(self) -> SearchParams:
        """The merge's block: it reads no row, but checks a bf16 pitch, so ``ldc`` = D there."""
        sp = SearchParams.from_buffer_copy(self)
        sp.ldc = sp.D
        return sp


@N.params_of("HZ_K_SEARCH_BXSCAN")
class BinBatchScanParams(C.Structure):
    """HzSearchBinBatchParams: ``corpus`` uint32 sign-bit rows [N][ldc] (``ldc`` in words), device fp32 ``queries``
    [Q][D], the required ``live`` bitmap, ``cand`` [nslab][Q][k] keys, the merge's outputs, the byte counts and shape,
    then ``span`` (tiles a workgroup walks; 0: the launcher's choice) and ``nslab``."""
    _fields_ = [("corpus", C.c_void_p), ("queries", C.c_void_p), ("live", C.c_void_p), ("cand", C.c_void_p),
                ("out_score", C.c_void_p), ("out_id", C.c_void_p), ("live_bytes", C.c_uint64), ("cand_bytes", C.c_uint64),
                ("N", C.c_int), ("D", C.c_int), ("Q", C.c_int), ("k", C.c_int), ("ldc", C.c_int), ("ntile", C.c_int),
                ("span", C.c_int), ("nslab", C.c_int)]

    def merge_params(self, nslab: int) -> "SelfScanParams":
        """The block ``HZ_K_SEARCH_MERGEN`` takes over the ``nslab`` slab lists: N = nslab tiles (it reads no row)."""
        mp = SelfScanParams(cand=self.cand, out_score=self.out_score, out_id=self.out_id, cand_bytes=self.cand_bytes,
                            N=int(nslab) * tile_rows(), D=self.D, Q=self.Q, k=self.k, ldc=self.D)
        return mp


@N.params_of("HZ_K_SEARCH_PQLUT")
class PqLutParams(C.Structure):
    """HzSearchPqLutParams: ``queries`` fp32 [Q][D], ``codebook`` fp32 [M][256][D / M], ``lut`` fp32 [Q][M][256] out."""
    _fields_ = [("queries", C.c_void_p), ("codebook", C.c_void_p), ("lut", C.c_void_p), ("lut_bytes", C.c_uint64),
                ("D", C.c_int), ("M", C.c_int), ("Q", C.c_int), ("pad_", C.c_int)]


@N.params_of("HZ_K_SEARCH_PQSCAN")
class PqScanParams(C.Structure):
    """HzSearchPqParams: the fields of ``FilterScanParams`` (``corpus``: uint8 code rows [N][ldc], ``ldc`` in bytes;
    ``live`` is required), then ``lut`` (the table kind's output), ``lut_bytes``, ``M`` and ``span`` (0: the
    launcher's choice)."""
    _fields_ = FilterScanParams._fields_ + [("lut", C.c_void_p), ("lut_bytes", C.c_uint64), ("M", C.c_int),
                                            ("span", C.c_int)]

    def scan_params(self) -> SearchParams:
        """The merge's block: it reads no row, but checks a bf16 pitch, so ``ldc`` = D there."""
        sp = SearchParams.from_buffer_copy(self)
        sp.ldc = sp.D
        return sp


@N.params_of("HZ_K_SEARCH_PQASSIGN")
class PqAssignParams(C.Structure):
    """HzSearchPqAssignParams: ``rows`` bf16 [N][ldr], ``codebook`` fp32 [M][256][D / M], ``codes`` uint8 [N][ldc] out
    (``ldc`` in bytes), ``dist`` fp32 [N][M] out or null with ``dist_bytes``."""
    _fields_ = [("rows", C.c_void_p), ("codebook", C.c_void_p), ("codes", C.c_void_p), ("dist", C.c_void_p),
                ("dist_bytes", C.c_uint64), ("N", C.c_longlong), ("D", C.c_int), ("M", C.c_int),
                ("ldr", C.c_longlong), ("ldc", C.c_longlong)]


@N.params_of("HZ_K_SEARCH_PQUPDATE")
class PqUpdateParams(C.Structure):
    """HzSearchPqUpdateParams: ``rows`` bf16 [N][ldr], ``codes`` uint8 [N][ldc] (``ldc`` in bytes), ``codebook_in`` and
    ``codebook_out`` fp32 [M][256][D / M] (they may be one buffer), ``counts`` int32 [M][256] out or null."""
    _fields_ = [("rows", C.c_void_p), ("codes", C.c_void_p), ("codebook_in", C.c_void_p), ("codebook_out", C.c_void_p),
                ("counts", C.c_void_p), ("N", C.c_longlong), ("D", C.c_int), ("M", C.c_int),
                ("ldr", C.c_longlong), ("ldc", C.c_longlong)]


@N.params_of("HZ_K_SEARCH_RESCOREN")
@N.params_of("HZ_K_SEARCH_RESCORE")
class RescoreParams(C.Structure):
    """HzSearchRescoreParams: ``rows`` bf16 [N][ldc] (device or mapped pinned host memory), ``queries`` fp32
    [Q][D], ``in_id`` int32 [Q][R] (-1: an empty slot), the outputs [Q][k]."""
    _fields_ = [("rows", C.c_void_p), ("queries", C.c_void_p), ("in_id", C.c_void_p), ("out_score", C.c_void_p),
                ("out_id", C.c_void_p), ("N", C.c_int), ("D", C.c_int), ("Q", C.c_int), ("R", C.c_int),
                ("k", C.c_int), ("ldc", C.c_int)]


@N.params_of("HZ_K_SEARCH_LSCAN")
class ListScanParams(C.Structure):
    """HzSearchListParams: the fields of ``FilterScanParams`` (``N`` stored rows, whole tiles; ``cand`` holds
    [P][Q][k] keys), then ``probes`` (device int32 [Q][nprobe], or 0: every list), ``list_off`` (int32 [nlist + 1]),
    ``list_tiles`` (int32 [N / tile_rows()]), ``rowid`` (int32 [N]) and ``nlist``, ``nprobe``, ``P``."""
    _fields_ = FilterScanParams._fields_ + [("probes", C.c_void_p), ("list_off", C.c_void_p), ("list_tiles", C.c_void_p),
                                            ("rowid", C.c_void_p), ("nlist", C.c_int), ("nprobe", C.c_int),
                                            ("P", C.c_int), ("pad_", C.c_int)]

    def merge_params(self) -> SearchParams:
        """The merge's block for this scan's candidates: ``ntile`` = P, so N = P * 256."""
        sp = SearchParams.from_buffer_copy(self)
        sp.N = self.P * 256
        return sp


@N.params_of("HZ_K_SEARCH_QLSCAN")
class QuantListScanParams(C.Structure):
    """HzSearchQuantListParams: the fields of ``ListScanParams`` (``corpus``: uint8 rows, ``ldc`` in bytes), then
    ``scales`` (fp32 [N] in stored order)."""
    _fields_ = ListScanParams._fields_ + [("scales", C.c_void_p)]

    def merge_params(self) -> SearchParams:
        sp = SearchParams.from_buffer_copy(self)
        sp.N = self.P * 256
        return sp


@N.params_of("HZ_K_SEARCH_MERGEN")
@N.params_of("HZ_K_SEARCH_MSCAN")
class SelfScanParams(C.Structure):
    """HzSearchSelfParams: ``corpus`` bf16 [N][ldc], ``qid`` device int32 [Q] (the rows that are the queries), the
    required ``live`` bitmap, ``cand`` [ntile][Q][k] keys, the merge's outputs [Q][k], then the byte counts and shape."""
    _fields_ = [("corpus", C.c_void_p), ("qid", C.c_void_p), ("live", C.c_void_p), ("cand", C.c_void_p),
                ("out_score", C.c_void_p), ("out_id", C.c_void_p), ("live_bytes", C.c_uint64), ("cand_bytes", C.c_uint64),
                ("N", C.c_int), ("D", C.c_int), ("Q", C.c_int), ("k", C.c_int), ("ldc", C.c_int), ("ntile", C.c_int),
                ("skip_self", C.c_int), ("pad_", C.c_int)]


@N.params_of("HZ_K_SEARCH_XSCAN")
class BatchScanParams(C.Structure):
    """HzSearchBatchParams: ``SelfScanParams`` with ``queries`` (device fp32 [Q][D], 16-B aligned) where ``qid`` is and
    two unused ints where ``skip_self`` is -- the same layout, so ``HZ_K_SEARCH_MERGEN`` takes it as it stands."""
    _fields_ = [("corpus", C.c_void_p), ("queries", C.c_void_p), ("live", C.c_void_p), ("cand", C.c_void_p),
                ("out_score", C.c_void_p), ("out_id", C.c_void_p), ("live_bytes", C.c_uint64), ("cand_bytes", C.c_uint64),
                ("N", C.c_int), ("D", C.c_int), ("Q", C.c_int), ("k", C.c_int), ("ldc", C.c_int), ("ntile", C.c_int),
                ("pad_", C.c_int * 2)]

    def merge_params(self) -> SelfScanParams:
        """The block as ``HZ_K_SEARCH_MERGEN`` reads it."""
        return SelfScanParams.from_buffer_copy(self)


@N.params_of("HZ_K_SEARCH_PQXSCAN")
class PqBatchScanParams(C.Structure):
    """HzSearchPqBatchParams: the fields of ``BatchScanParams`` with ``codes`` (uint8 [N][ldc], ``ldc`` in bytes) where
    ``corpus`` is, then ``cb8`` (device bf16 [D / 8][256][8]), ``cb8_bytes`` and ``M``."""
    _fields_ = [("codes", C.c_void_p)] + BatchScanParams._fields_[1:] + [("cb8", C.c_void_p), ("cb8_bytes", C.c_uint64),
                                                                         ("M", C.c_int), ("pad2_", C.c_int)]

    def merge_params(self) -> SelfScanParams:
        """The block as ``HZ_K_SEARCH_MERGEN`` reads it."""
        return SelfScanParams.from_buffer_copy(self)


@N.params_of("HZ_K_SEARCH_PQRESCORE")
class PqRescoreParams(C.Structure):
    """HzSearchPqRescoreParams: ``codes`` uint8 [N][ldc], ``codebook`` fp32 [M][256][D / M], ``queries`` fp32 [Q][D],
    ``in_id`` / ``in_score`` [Q][R] (a merge's outputs), the outputs [Q][k] and ``out_last`` fp32 [Q]."""
    _fields_ = [("codes", C.c_void_p), ("codebook", C.c_void_p), ("queries", C.c_void_p), ("in_id", C.c_void_p),
                ("in_score", C.c_void_p), ("out_score", C.c_void_p), ("out_id", C.c_void_p), ("out_last", C.c_void_p),
                ("N", C.c_int), ("D", C.c_int), ("M", C.c_int), ("Q", C.c_int), ("R", C.c_int), ("k", C.c_int),
                ("ldc", C.c_int), ("pad_", C.c_int)]


@N.params_of("HZ_K_SEARCH_QXSCAN")
class QuantBatchScanParams(C.Structure):
    """HzSearchQuantBatchParams: the fields of ``BatchScanParams`` with ``codes`` (e4m3 uint8 [N][ldc], ``ldc`` in bytes)
    where ``corpus`` is, then ``scales`` (device fp32 [N]) and ``scales_bytes``."""
    _fields_ = [("codes", C.c_void_p)] + BatchScanParams._fields_[1:] + [("scales", C.c_void_p), ("scales_bytes", C.c_uint64)]

    def merge_params(self) -> SelfScanParams:
        """The block as ``HZ_K_SEARCH_MERGEN`` reads it."""
        return SelfScanParams.from_buffer_copy(self)


@N.params_of("HZ_K_SEARCH_QRESCORE")
class QuantRescoreParams(C.Structure):
    """HzSearchQuantRescoreParams: ``codes`` e4m3 uint8 [N][ldc], ``scales`` fp32 [N], ``queries`` fp32 [Q][D],
    ``in_id`` / ``in_score`` [Q][R] (a merge's outputs), the outputs [Q][k] and ``out_last`` fp32 [Q]."""
    _fields_ = [("codes", C.c_void_p), ("scales", C.c_void_p), ("queries", C.c_void_p), ("in_id", C.c_void_p),
                ("in_score", C.c_void_p), ("out_score", C.c_void_p), ("out_id", C.c_void_p), ("out_last", C.c_void_p),
                ("N", C.c_int), ("D", C.c_int), ("Q", C.c_int), ("R", C.c_int), ("k", C.c_int), ("ldc", C.c_int)]


@N.params_of("HZ_K_SEARCH_LXSCAN")
class ListBatchScanParams(C.Structure):
    """HzSearchListBatchParams: the fields of ``BatchScanParams`` over the stored rows of an IVF index (``N`` a whole
    number of tiles; ``cand`` holds [P][Q][k] keys), then ``rowid`` (int32 [N]), the work list -- ``items`` (device int32
    [nwork][4]: tile, slot offset, first entry, nq) and ``entries`` (device int32 [nent][2]: query, base slot) with their
    byte counts -- and ``nwork``, ``nent``, ``P``."""
    _fields_ = BatchScanParams._fields_ + [("rowid", C.c_void_p), ("items", C.c_void_p), ("entries", C.c_void_p),
                                           ("items_bytes", C.c_uint64), ("entries_bytes", C.c_uint64),
                                           ("nwork", C.c_int), ("nent", C.c_int), ("P", C.c_int), ("pad2_", C.c_int)]

    def merge_params(self) -> SelfScanParams:
        """``HZ_K_SEARCH_MERGEN``'s block for this scan's candidates: ``ntile`` = P, so N = P * 256."""
        mp = SelfScanParams.from_buffer_copy(self)
        mp.N = self.P * 256
        return mp


@N.params_of("HZ_K_SEARCH_RESCOREP")
class RescorePosParams(C.Structure):
    """HzSearchRescorePosParams: ``RescoreParams`` over rows in stored order -- ``in_id`` / ``out_id`` are external ids
    and ``pos`` (device int32 [npos]) maps an id to its stored row."""
    _fields_ = [("rows", C.c_void_p), ("queries", C.c_void_p), ("in_id", C.c_void_p), ("out_score", C.c_void_p),
                ("out_id", C.c_void_p), ("pos", C.c_void_p), ("N", C.c_int), ("D", C.c_int), ("Q", C.c_int),
                ("R", C.c_int), ("k", C.c_int), ("ldc", C.c_int), ("npos", C.c_int), ("pad_", C.c_int)]


@N.params_of("HZ_K_SEARCH_GRAPH")
class GraphParams(C.Structure):
    """HzSearchGraphParams: ``corpus`` bf16 [N][ldc], ``queries`` device fp32 [Q][D], ``graph`` device int32 [N][deg]
    (an entry outside [0, N) is padding), ``entries`` device int32 [E], the outputs [Q][k] and ``out_stats`` (int32
    [Q][2]: iterations, rows scored; or null). ``estride`` > 0: ``entries`` is [Q][estride], a row per query."""
    _fields_ = [("corpus", C.c_void_p), ("queries", C.c_void_p), ("graph", C.c_void_p), ("entries", C.c_void_p),
                ("out_score", C.c_void_p), ("out_id", C.c_void_p), ("out_stats", C.c_void_p), ("N", C.c_int),
                ("D", C.c_int), ("Q", C.c_int), ("k", C.c_int), ("ldc", C.c_int), ("beam", C.c_int), ("deg", C.c_int),
                ("width", C.c_int), ("iters", C.c_int), ("E", C.c_int), ("estride", C.c_int), ("pad_", C.c_int)]


@N.params_of("HZ_K_GRAPH_SEED")
class GraphSeedParams(C.Structure):
    """HzGraphSeedParams: ``corpus`` bf16 [N][ldc], ``queries`` device fp32 [Q][D], ``seeds`` device int32 [S], ``out``
    device int32 [Q][estride]: each query's best ``E`` seed ids, best first, then -1."""
    _fields_ = [("corpus", C.c_void_p), ("queries", C.c_void_p), ("seeds", C.c_void_p), ("out", C.c_void_p),
                ("N", C.c_int), ("D", C.c_int), ("Q", C.c_int), ("S", C.c_int), ("E", C.c_int), ("ldc", C.c_int),
                ("estride", C.c_int), ("pad_", C.c_int)]


@N.params_of("HZ_K_GRAPH_PRUNE")
class GraphPruneParams(C.Structure):
    """HzGraphPruneParams: ``knn`` device int32 [N][W] (best first), ``order`` and ``detours`` (or null) device int32
    [N][W]."""
    _fields_ = [("knn", C.c_void_p), ("order", C.c_void_p), ("detours", C.c_void_p), ("N", C.c_int), ("W", C.c_int)]


@N.params_of("HZ_K_SEARCH_ASSIGN")
class AssignParams(C.Structure):
    """HzSearchAssignParams: ``corpus`` bf16 [N][ldc], ``cent`` bf16 [C][ldk], the required ``live`` bitmap (any
    bitmap: a row without its bit gets -1 / -inf), ``out_list`` int32 [N], ``out_score`` fp32 [N]."""
    _fields_ = [("corpus", C.c_void_p), ("cent", C.c_void_p), ("live", C.c_void_p), ("out_list", C.c_void_p),
                ("out_score", C.c_void_p), ("live_bytes", C.c_uint64), ("N", C.c_int), ("D", C.c_int), ("C", C.c_int),
                ("ldc", C.c_int), ("ldk", C.c_int), ("ntile", C.c_int)]


@N.params_of("HZ_K_SEARCH_CMEAN")
class CmeanParams(C.Structure):
    """HzSearchCmeanParams: ``order`` device int32 [M] (the members' row ids, cluster after cluster), ``seg_off`` device
    int32 [C + 1], ``cent`` bf16 [C][ldk] in and out, ``cent32`` fp32 [C][D] out or null."""
    _fields_ = [("corpus", C.c_void_p), ("order", C.c_void_p), ("seg_off", C.c_void_p), ("cent", C.c_void_p),
                ("cent32", C.c_void_p), ("N", C.c_int), ("D", C.c_int), ("C", C.c_int), ("M", C.c_int), ("ldc", C.c_int),
                ("ldk", C.c_int), ("cosine", C.c_int), ("pad_", C.c_int)]


def _sigs(lib):
    P, U64 = C.c_void_p, C.c_uint64
    N._sig(lib, "hz_search_assign_launch", C.c_int, C.POINTER(AssignParams), P)
    N._sig(lib, "hz_search_cmean_launch", C.c_int, C.POINTER(CmeanParams), P)
    N._sig(lib, "hz_index_assign", C.c_int, P, C.c_int, P, C.c_int, P, P, P)
    N._sig(lib, "hz_index_cmean", C.c_int, P, C.c_int, P, C.c_longlong, P, C.c_int, P, P)
    N._sig(lib, "hz_search_self_scratch_bytes", U64, C.c_longlong, C.c_longlong, C.c_int)
    N._sig(lib, "hz_search_mscan_launch", C.c_int, C.POINTER(SelfScanParams), P)
    N._sig(lib, "hz_search_mergen_launch", C.c_int, C.POINTER(SelfScanParams), P)
    N._sig(lib, "hz_search_xscan_launch", C.c_int, C.POINTER(BatchScanParams), P)
    N._sig(lib, "hz_search_rescoren_launch", C.c_int, C.POINTER(RescoreParams), P)
    N._sig(lib, "hz_index_search_batch", C.c_int, P, C.c_int, P, C.c_int, C.c_int, C.c_int, P, P, P)
    N._sig(lib, "hz_search_pqxscan_launch", C.c_int, C.POINTER(PqBatchScanParams), P)
    N._sig(lib, "hz_search_pqrescore_launch", C.c_int, C.POINTER(PqRescoreParams), P)
    N._sig(lib, "hz_index_search_batch_pq", C.c_int, P, C.c_int, P, C.c_int, C.c_int, C.c_int, P, P, P)
    N._sig(lib, "hz_search_qxscan_launch", C.c_int, C.POINTER(QuantBatchScanParams), P)
    N._sig(lib, "hz_search_qrescore_launch", C.c_int, C.POINTER(QuantRescoreParams), P)
    N._sig(lib, "hz_index_search_batch_q", C.c_int, P, C.c_int, P, C.c_int, C.c_int, C.c_int, P, P, P)
    N._sig(lib, "hz_search_lxscan_launch", C.c_int, C.POINTER(ListBatchScanParams), P)
    N._sig(lib, "hz_search_rescorep_launch", C.c_int, C.POINTER(RescorePosParams), P)
    N._sig(lib, "hz_search_graph_launch", C.c_int, C.POINTER(GraphParams), P)
    N._sig(lib, "hz_graph_prune_launch", C.c_int, C.POINTER(GraphPruneParams), P)
    N._sig(lib, "hz_graph_prune", C.c_int, C.c_int, P, C.c_longlong, C.c_int, P, P)
    N._sig(lib, "hz_index_set_graph", C.c_int, P, P, C.c_longlong, C.c_int, P, C.c_int)
    N._sig(lib, "hz_index_search_graph", C.c_int, P, C.c_int, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P)
    N._sig(lib, "hz_graph_seed_launch", C.c_int, C.POINTER(GraphSeedParams), P)
    N._sig(lib, "hz_index_set_graph_seeds", C.c_int, P, P, C.c_int)
    N._sig(lib, "hz_index_search_graph2", C.c_int, P, C.c_int, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P)
    N._sig(lib, "hz_index_probes_batch", C.c_int, P, C.c_int, P, C.c_int, C.c_int, C.c_int, P, P, P)
    N._sig(lib, "hz_index_search_batch_ivf", C.c_int, P, C.c_int, P, C.c_int, P, C.c_int, C.c_int, C.c_int, P, P, P)
    N._sig(lib, "hz_index_search_batch_ivf_invert_us", C.c_double, P, C.c_int)
    N._sig(lib, "hz_index_neighbors", C.c_int, P, C.c_int, P, C.c_int, C.c_int, C.c_int, P, P)
    N._sig(lib, "hz_index_neighbors_max", C.c_int, P, C.c_int)
    N._sig(lib, "hz_search_tile_rows", C.c_int)
    N._sig(lib, "hz_search_scratch_bytes", U64, C.c_longlong, C.c_int, C.c_int)
    N._sig(lib, "hz_search_scan_launch", C.c_int, C.POINTER(SearchParams), P)
    N._sig(lib, "hz_search_merge_launch", C.c_int, C.POINTER(SearchParams), P)
    N._sig(lib, "hz_search_fscan_launch", C.c_int, C.POINTER(FilterScanParams), P)
    N._sig(lib, "hz_search_qscan_launch", C.c_int, C.POINTER(QuantScanParams), P)
    N._sig(lib, "hz_search_rescore_launch", C.c_int, C.POINTER(RescoreParams), P)
    N._sig(lib, "hz_search_bscan_launch", C.c_int, C.POINTER(BinScanParams), P)
    N._sig(lib, "hz_search_bxscan_launch", C.c_int, C.POINTER(BinBatchScanParams), P)
    N._sig(lib, "hz_search_bxscan_span", C.c_int, C.c_longlong, C.c_longlong, C.c_int)
    N._sig(lib, "hz_search_bxscan_scratch_bytes", U64, C.c_longlong, C.c_longlong, C.c_int, C.c_int)
    N._sig(lib, "hz_index_search_batch_b", C.c_int, P, C.c_int, P, C.c_int, C.c_int, C.c_int, P, P)
    N._sig(lib, "hz_index_add_b", C.c_int, P, P, C.c_longlong, P, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_add_br", C.c_int, P, P, P, C.c_longlong, P, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_read_state_b", C.c_int, P, P, P, P, C.c_longlong)
    N._sig(lib, "hz_search_pqlut_launch", C.c_int, C.POINTER(PqLutParams), P)
    N._sig(lib, "hz_search_pqscan_launch", C.c_int, C.POINTER(PqScanParams), P)
    N._sig(lib, "hz_search_pq_span", C.c_int, C.c_longlong, C.c_int, C.c_int)
    N._sig(lib, "hz_search_pqassign_launch", C.c_int, C.POINTER(PqAssignParams), P)
    N._sig(lib, "hz_pq_encode", C.c_int, C.c_int, P, C.c_longlong, C.c_int, C.c_int, P, C.c_longlong, P, P)
    N._sig(lib, "hz_search_pqupdate_launch", C.c_int, C.POINTER(PqUpdateParams), P)
    N._sig(lib, "hz_pq_train", C.c_int, C.c_int, P, C.c_longlong, C.c_int, C.c_int, P, C.c_int, P)
    N._sig(lib, "hz_index_add_p", C.c_int, P, P, C.c_longlong, P, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_add_pr", C.c_int, P, P, P, C.c_longlong, P, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_read_state_p", C.c_int, P, P, P, P, C.c_longlong)
    N._sig(lib, "hz_index_read_codebook", C.c_int, P, P)
    N._sig(lib, "hz_index_describe4", C.c_int, P, C.POINTER(U64))
    N._sig(lib, "hz_search_lscan_launch", C.c_int, C.POINTER(ListScanParams), P)
    N._sig(lib, "hz_search_qlscan_launch", C.c_int, C.POINTER(QuantListScanParams), P)
    N._sig(lib, "hz_search_code_warm", C.c_int)
    N._sig(lib, "hz_index_last_error", C.c_char_p)
    N._sig(lib, "hz_index_open", P, C.c_char_p, C.c_int, C.c_int)
    N._sig(lib, "hz_index_describe", C.c_int, P, C.POINTER(U64))
    N._sig(lib, "hz_index_search", C.c_int, P, C.c_int, P, C.c_int, C.c_int, P, P)
    N._sig(lib, "hz_index_close", None, P)
    N._sig(lib, "hz_index_open2", P, C.c_char_p, C.c_int, C.c_int, C.c_longlong)
    N._sig(lib, "hz_index_describe2", C.c_int, P, C.POINTER(U64))
    N._sig(lib, "hz_index_search_filtered", C.c_int, P, C.c_int, P, P, C.c_int, C.c_int, P, P)
    N._sig(lib, "hz_index_add", C.c_int, P, P, C.c_longlong, P, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_delete", C.c_int, P, P, C.c_longlong, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_set_tags", C.c_int, P, P, P, C.c_longlong)
    N._sig(lib, "hz_index_read_state", C.c_int, P, P, P, P, C.c_longlong)
    N._sig(lib, "hz_index_add_q", C.c_int, P, P, P, C.c_longlong, P, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_read_state_q", C.c_int, P, P, P, P, P, C.c_longlong)
    N._sig(lib, "hz_index_open3", P, C.c_char_p, C.c_int, C.c_int, C.c_longlong, C.c_int)
    N._sig(lib, "hz_index_search2", C.c_int, P, C.c_int, P, P, C.c_int, C.c_int, C.c_int, P, P)
    N._sig(lib, "hz_index_add_qr", C.c_int, P, P, P, P, C.c_longlong, P, C.POINTER(C.c_longlong))
    N._sig(lib, "hz_index_read_rescore", C.c_int, P, P, C.c_longlong)
    N._sig(lib, "hz_index_search3", C.c_int, P, C.c_int, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P)
    N._sig(lib, "hz_index_probes", C.c_int, P, C.c_int, P, C.c_int, C.c_int, P)
    N._sig(lib, "hz_index_describe3", C.c_int, P, C.POINTER(U64))


N._EXTRA_SIGS.append(_sigs)
if N._lib is not None:  # the library was loaded before this module
    _sigs(N._lib)


def tile_rows() -> int:
    """Corpus rows per scan workgroup (a tile)."""
    return int(N.lib().hz_search_tile_rows())


def scratch_bytes(n: int, q: int, k: int) -> int:
    """Bytes of candidate scratch a search of (N, Q, k) needs; 0 for a refused shape."""
    return int(N.lib().hz_search_scratch_bytes(int(n), int(q), int(k)))


def launch(prm: SearchParams, stream: int = 0) -> tuple:
    """Scan then merge on ``stream``: (scan code, merge code); the merge is not launched after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_scan_launch(C.byref(prm), stream)
    return rc, (lib.hz_search_merge_launch(C.byref(prm), stream) if rc == 0 else None)


def launch_filtered(prm: FilterScanParams, stream: int = 0) -> tuple:
    """Filtered scan then merge on ``stream``: (scan code, merge code); no merge after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_fscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    sp = prm.scan_params()
    return rc, lib.hz_search_merge_launch(C.byref(sp), stream)


def launch_quant(prm: QuantScanParams, stream: int = 0) -> tuple:
    """Quantised scan then merge on ``stream``: (scan code, merge code); no merge after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_qscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    sp = prm.scan_params()
    return rc, lib.hz_search_merge_launch(C.byref(sp), stream)


def launch_bin(prm: BinScanParams, stream: int = 0) -> tuple:
    """Binary scan then merge on ``stream``: (scan code, merge code); no merge after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_bscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    sp = prm.scan_params()
    return rc, lib.hz_search_merge_launch(C.byref(sp), stream)


def bin_batch_span(n: int, q: int, k: int) -> int:
    """The tiles per workgroup a bulk binary scan of (N, Q, k) takes with ``span`` = 0 on the current device; 0 for a
    refused shape."""
    return int(N.lib().hz_search_bxscan_span(int(n), int(q), int(k)))


def bin_batch_scratch_bytes(n: int, q: int, k: int, span: int = 0) -> int:
    """Bytes of candidate scratch a bulk binary scan of (N, Q, k) needs at ``span``: nslab * Q * k * 8; 0 for a refused
    shape."""
    return int(N.lib().hz_search_bxscan_scratch_bytes(int(n), int(q), int(k), int(span)))


def launch_pq_lut(prm: PqLutParams, stream: int = 0) -> int:
    """The table launch (``HZ_K_SEARCH_PQLUT``) on ``stream`` -> its code (0, or negative: nothing ran)."""
    return int(N.lib().hz_search_pqlut_launch(C.byref(prm), stream))


def launch_pq(prm: PqScanParams, stream: int = 0) -> tuple:
    """Product-quantised scan (over a table ``launch_pq_lut`` wrote) then merge on ``stream``: (scan code, merge
    code); no merge after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_pqscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    sp = prm.scan_params()
    return rc, lib.hz_search_merge_launch(C.byref(sp), stream)


def pq_span(n: int, q: int, m: int) -> int:
    """The tiles per workgroup a scan of (N, Q) over rows of M codes takes with ``span`` = 0 on the current device; 0
    for a refused shape."""
    return int(N.lib().hz_search_pq_span(int(n), int(q), int(m)))


def launch_pq_assign(prm: PqAssignParams, stream: int = 0) -> int:
    """The assign launch (``HZ_K_SEARCH_PQASSIGN``) on ``stream`` -> its code (0, or negative: nothing ran)."""
    return int(N.lib().hz_search_pqassign_launch(C.byref(prm), stream))


def pq_encode_rows(bits, codebook, *, device: int = 0, chunk_rows: int = 0, want_dist: bool = False):
    """``hz_pq_encode``: bf16 rows ``bits`` (uint16 [n, D], host) against ``codebook`` (fp32 [M, 256, D / M], host) on
    ``device`` -> (codes uint8 [n, M], dist fp32 [n, M] or None). ``chunk_rows``: rows per device pass, 0 for the
    default. A refused shape is a ValueError with the launcher's code, a device failure a RuntimeError."""
    import numpy as np
    bits = np.ascontiguousarray(bits, np.uint16)
    cb = np.ascontiguousarray(codebook, np.float32)
    if bits.ndim != 2 or cb.ndim != 3 or cb.shape[1] != PQ_KSUB or cb.shape[0] * cb.shape[2] != bits.shape[1]:
        raise ValueError(f"rows must be uint16 [n, D] and the codebook fp32 [M, {PQ_KSUB}, D / M], got {list(bits.shape)} "
                         f"and {list(cb.shape)}")
    n, d = bits.shape
    m = cb.shape[0]
    codes = np.empty((n, m), np.uint8)
    dist = np.empty((n, m), np.float32) if want_dist else None
    lib = N.lib()
    rc = int(lib.hz_pq_encode(int(device), bits.ctypes.data, n, d, m, cb.ctypes.data, int(chunk_rows), codes.ctypes.data,
                              dist.ctypes.data if want_dist else None))
    if rc:
        msg = (lib.hz_index_last_error() or b"").decode()
        if rc in (-140, -141):
            raise (ValueError if rc == -141 else RuntimeError)(msg or f"hz_pq_encode failed ({rc})")
        raise ValueError(f"hz_pq_encode refused n = {n}, dim = {d}, m = {m} ({rc}: csrc/hipzap.h HZ_K_SEARCH_PQASSIGN)")
    return codes, dist


def launch_pq_update(prm: PqUpdateParams, stream: int = 0) -> int:
    """The update launch (``HZ_K_SEARCH_PQUPDATE``) on ``stream`` -> its code (0, or negative: nothing ran)."""
    return int(N.lib().hz_search_pqupdate_launch(C.byref(prm), stream))


def pq_train_rows(bits, codebook, iters: int, *, device: int = 0, want_counts: bool = False):
    """``hz_pq_train``: ``iters`` Lloyd iterations over the bf16 rows ``bits`` (uint16 [n, D], host) from ``codebook``
    (fp32 [M, 256, D / M], host; not modified) on ``device``, the rows uploaded once and nothing copied back before
    the end -> the new codebook, or (codebook, counts int32 [M, 256] of the last iteration) with ``want_counts``
    (zeros when ``iters`` is 0). A refused shape or a negative ``iters`` is a ValueError, a device failure a
    RuntimeError."""
    import numpy as np
    bits = np.ascontiguousarray(bits, np.uint16)
    cb = np.array(codebook, np.float32, order="C")  # a copy: the job works in place
    if bits.ndim != 2 or cb.ndim != 3 or cb.shape[1] != PQ_KSUB or cb.shape[0] * cb.shape[2] != bits.shape[1]:
        raise ValueError(f"rows must be uint16 [n, D] and the codebook fp32 [M, {PQ_KSUB}, D / M], got {list(bits.shape)} "
                         f"and {list(cb.shape)}")
    n, d = bits.shape
    m = cb.shape[0]
    counts = np.zeros((m, PQ_KSUB), np.int32) if want_counts else None
    lib = N.lib()
    rc = int(lib.hz_pq_train(int(device), bits.ctypes.data, n, d, m, cb.ctypes.data, int(iters),
                             counts.ctypes.data if want_counts else None))
    if rc:
        msg = (lib.hz_index_last_error() or b"").decode()
        if rc in (-140, -141):
            raise (ValueError if rc == -141 else RuntimeError)(msg or f"hz_pq_train failed ({rc})")
        raise ValueError(f"hz_pq_train refused n = {n}, dim = {d}, m = {m} ({rc}: csrc/hipzap.h HZ_K_SEARCH_PQUPDATE)")
    return (cb, counts) if want_counts else cb


def launch_rescore(prm: RescoreParams, stream: int = 0) -> int:
    """The rescore launch on ``stream`` -> its code (0, or negative for a refused block: nothing ran)."""
    return int(N.lib().hz_search_rescore_launch(C.byref(prm), stream))


def launch_list(prm: ListScanParams, stream: int = 0) -> tuple:
    """List scan then merge (over the P candidate lists) on ``stream``: (scan code, merge code); no merge after a
    refused scan."""
    lib = N.lib()
    rc = lib.hz_search_lscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    sp = prm.merge_params()
    return rc, lib.hz_search_merge_launch(C.byref(sp), stream)


def launch_quant_list(prm: QuantListScanParams, stream: int = 0) -> tuple:
    """Quantised list scan then merge (over the P candidate lists) on ``stream``: (scan code, merge code); no merge
    after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_qlscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    sp = prm.merge_params()
    return rc, lib.hz_search_merge_launch(C.byref(sp), stream)


def self_scratch_bytes(n: int, q: int, k: int) -> int:
    """Bytes of candidate scratch a self scan of (N, Q, k) needs; 0 for a refused shape."""
    return int(N.lib().hz_search_self_scratch_bytes(int(n), int(q), int(k)))


def launch_self(prm: SelfScanParams, stream: int = 0) -> tuple:
    """Self scan then its merge on ``stream``: (scan code, merge code); no merge after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_mscan_launch(C.byref(prm), stream)
    return rc, (lib.hz_search_mergen_launch(C.byref(prm), stream) if rc == 0 else None)


def launch_batch(prm: BatchScanParams, stream: int = 0) -> tuple:
    """Batch scan then ``HZ_K_SEARCH_MERGEN`` over the same block on ``stream``: (scan code, merge code); no merge after
    a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_xscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    mp = prm.merge_params()
    return rc, lib.hz_search_mergen_launch(C.byref(mp), stream)


def launch_pq_batch(prm: PqBatchScanParams, stream: int = 0) -> tuple:
    """The pq batch scan then ``HZ_K_SEARCH_MERGEN`` over the same block on ``stream``: (scan code, merge code); no merge
    after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_pqxscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    mp = prm.merge_params()
    return rc, lib.hz_search_mergen_launch(C.byref(mp), stream)


def launch_pq_rescore(prm: PqRescoreParams, stream: int = 0) -> int:
    """The codebook rescore (``HZ_K_SEARCH_PQRESCORE``) on ``stream`` -> its code (0, or negative: nothing ran)."""
    return int(N.lib().hz_search_pqrescore_launch(C.byref(prm), stream))


def launch_quant_batch(prm: QuantBatchScanParams, stream: int = 0) -> tuple:
    """The fp8 batch scan then ``HZ_K_SEARCH_MERGEN`` over the same block on ``stream``: (scan code, merge code); no merge
    after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_qxscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    mp = prm.merge_params()
    return rc, lib.hz_search_mergen_launch(C.byref(mp), stream)


def launch_quant_rescore(prm: QuantRescoreParams, stream: int = 0) -> int:
    """The fp8 rescore (``HZ_K_SEARCH_QRESCORE``) on ``stream`` -> its code (0, or negative: nothing ran)."""
    return int(N.lib().hz_search_qrescore_launch(C.byref(prm), stream))


def launch_list_batch(prm: ListBatchScanParams, stream: int = 0) -> tuple:
    """The list batch scan (``HZ_K_SEARCH_LXSCAN``) then ``HZ_K_SEARCH_MERGEN`` over its P candidate slots on ``stream``:
    (scan code, merge code); no merge after a refused scan."""
    lib = N.lib()
    rc = lib.hz_search_lxscan_launch(C.byref(prm), stream)
    if rc:
        return rc, None
    mp = prm.merge_params()
    return rc, lib.hz_search_mergen_launch(C.byref(mp), stream)


def launch_rescore_pos(prm: RescorePosParams, stream: int = 0) -> int:
    """The stored-order rescore (``HZ_K_SEARCH_RESCOREP``) on ``stream`` -> its code (0, or negative: nothing ran)."""
    return int(N.lib().hz_search_rescorep_launch(C.byref(prm), stream))


def launch_rescore_n(prm: RescoreParams, stream: int = 0) -> int:
    """The rescore launch for any number of queries (``HZ_K_SEARCH_RESCOREN``) on ``stream`` -> its code."""
    return int(N.lib().hz_search_rescoren_launch(C.byref(prm), stream))


def graph_max_iters(entries: int, width: int, deg: int) -> int:
    """The most iterations the large visited table allows (``entries + iters * width * deg`` at most half its slots)."""
    return (GRAPH_CAP_LARGE // 2 - int(entries)) // (int(width) * int(deg))


def launch_graph(prm: GraphParams, stream: int = 0) -> int:
    """The graph search (``HZ_K_SEARCH_GRAPH``) on ``stream`` -> its code (0, or negative: nothing ran)."""
    return int(N.lib().hz_search_graph_launch(C.byref(prm), stream))


def launch_graph_seed(prm: GraphSeedParams, stream: int = 0) -> int:
    """The seed kernel (``HZ_K_GRAPH_SEED``) on ``stream`` -> its code (0, or negative: nothing ran)."""
    return int(N.lib().hz_graph_seed_launch(C.byref(prm), stream))


def launch_graph_prune(prm: GraphPruneParams, stream: int = 0) -> int:
    """The pruning kernel (``HZ_K_GRAPH_PRUNE``) on ``stream`` -> its code (0, or negative: nothing ran)."""
    return int(N.lib().hz_graph_prune_launch(C.byref(prm), stream))


def graph_prune_lists(knn, *, device: int = 0, want_detours: bool = False):
    """``hz_graph_prune``: kNN lists ``knn`` (int32 [N, W], host, best first) on ``device`` -> (order int32 [N, W],
    detours int32 [N, W] or None) by the rule of ``HZ_K_GRAPH_PRUNE``. A refused shape is a ValueError with the
    launcher's code, a device failure a RuntimeError."""
    import numpy as np
    knn = np.ascontiguousarray(knn, np.int32)
    if knn.ndim != 2:
        raise ValueError(f"knn must be int32 [N, W], got {list(knn.shape)}")
    n, w = knn.shape
    order = np.empty((n, w), np.int32)
    det = np.empty((n, w), np.int32) if want_detours else None
    lib = N.lib()
    rc = int(lib.hz_graph_prune(int(device), knn.ctypes.data, n, w, order.ctypes.data, det.ctypes.data if want_detours else None))
    if rc == -242 or rc > 0:
        raise RuntimeError((lib.hz_index_last_error() or b"").decode() or f"hz_graph_prune failed ({rc})")
    if rc:
        raise ValueError(f"hz_graph_prune refused N = {n}, W = {w} ({rc}: csrc/hipzap.h HZ_K_GRAPH_PRUNE)")
    return order, det
