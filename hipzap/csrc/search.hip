// hipzap vector search for gfx950 (CDNA4): exact top-k by inner product over a bf16 or e4m3 corpus.
//   * search_scan  — one workgroup per tile of HZ_SEARCH_TILE rows: every row is read once and scored
//                    against all Q queries of the launch (resident in LDS); the tile's best k per query.
//                    One template; its instantiations are the kinds SCAN (bf16 rows), FSCAN (bf16 rows that
//                    pass a live bit and a per-query tag predicate) and QSCAN (FSCAN over OCP e4m3fn byte
//                    rows with one fp32 scale per row)
//   * search_lscan — the filtered scan over an IVF index's lists (kinds LSCAN: bf16 rows, QLSCAN: e4m3 rows with
//                    row scales): workgroup (j, q) scores the j-th tile of the lists query q probes against that
//                    query alone, with the template's pieces
//   * search_merge — one workgroup per query: ntile x k candidates -> the final k, best first
//   * search_mscan — the self scan (kind MSCAN): the queries are rows of the corpus named by id; workgroup (tile, block
//                    of 64 queries) scores them with the bf16 MFMA and cuts before it ranks. Kind MERGEN is
//                    search_merge behind a launcher that takes any number of queries
//   * search_xscan — the batch scan (kind XSCAN): the self scan over EXTERNAL fp32 queries, each split in registers
//                    into three bf16 terms that sum to it, so the MFMA scores the unrounded query. Kind RESCOREN is
//                    search_rescore behind a launcher that takes any number of queries
//   * search_assign — the nearest centroid of every row (kind ASSIGN): the self scan with the roles turned, a running
//                    top-1 key per row; search_cmean (kind CMEAN): a cluster's mean in a fixed summation order
//   * search_bscan — the filtered scan over sign-bit rows (kind BSCAN): one word per 32 columns, the queries binarised
//                    in the kernel, score = D - 2 popcount(q xor r); its lists go to search_merge like any other
//   * search_pqlut / search_pqscan — product-quantised rows (kinds PQLUT, PQSCAN): a per-query table of the query's
//                    inner products with 256 sub-centroids per sub-space, then the filtered scan over rows of M code
//                    bytes, a workgroup holding ONE query's table in LDS and adding M lookups per row
//   * search_pqassign — the nearest of 256 sub-centroids for every row and sub-space (kind PQASSIGN): what training
//                    and encoding a product quantiser need, in plain fp32 operations numpy reproduces bit for bit
// See HzSearchParams (hipzap.h) for the order rule and DESIGN.md 4l / 4m / 4n / 4p / 4q / 4s / 4t / 4u / 4v / 4w / 4x for the
// reasoning.
#include <stdio.h>

#include <type_traits>

#include "common.h"
#include "hipzap.h"

HZ_DEBUG_UNIT(search)

namespace {

constexpr int T = HZ_SEARCH_TILE;  // rows per tile = threads of a scan workgroup
constexpr int ROWS = 4;            // rows a wave scores at a time (their loads in flight together)
constexpr int MERGE_THREADS = 256;
constexpr int MERGE_E = 8;         // candidates a merge thread loads per round
constexpr int MERGE_POOL = HZ_SEARCH_MAX_K + MERGE_THREADS * MERGE_E;

// fp32 bits -> unsigned with the same order as the floats (no NaN reaches the kernels); -0.0 -> +0.0
__device__ __forceinline__ unsigned orderable(float f) {
  unsigned u = __float_as_uint(f);
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float unorderable(unsigned o) {
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// ------------------------------------------------------------------------------------------- scan
// search_scan_kernel<Fmt, NC, FILT>: row format, 16-B chunks per lane (sized to D at launch), filtered or not.
// Wave w of the workgroup owns rows w*64 .. w*64+63 of the tile, ROWS at a time. Lane l holds the 16-B chunks
// l, l + 64, ... of a row, Fmt::E elements each.
// CONTRACT: score(q, r) is ONE fmaf chain per lane over the lane's elements in ascending column order starting
// from +0 (a lane past the row's end keeps +0), then the xor butterfly over the 64 lane sums (32, 16, ..., 1),
// then, for a scaled format, ONE fp32 multiply by the row's scale; then orderable(). All of it is fixed by D
// alone, so the bits of a score depend on the query's D values, the row's D elements and the row's scale, and
// on nothing else: not on N, Q, k, the row's position or tile, the other queries, the filter, or what dead
// rows hold. The three kinds share these statements, so a passing (q, r) scores the same bits in all of them.
// No NaN reaches the kernels (the writers refuse non-finite rows and queries): orderable() of a real score is never 0.
// Each (row, query) score lands in LDS as an order-preserving u32; thread t then ranks row t of the tile among
// the tile's rows (higher score first, then the lower row) and the rows ranked below k write their key to
// slot `rank` of the tile's list; the slots past the tile's passing rows are zero-filled.
// Per variant:
//   * unfiltered (SCAN): every row of the tile is loaded and scored; no pass bits exist, in LDS or registers.
//   * filtered (FSCAN, QSCAN): pass(q, r) = live(r) && (filt == null || (tags[r] & mask[q]) == value[q]). The
//     kernel's start stages the tile's 8 live words, its T tag words and the Q {mask, value} pairs (one
//     coalesced read each) and thread t folds them into row t's pass bits. The row loop reads the pass bits of
//     its (wave-uniform) rows through readfirstlane: a row with no pass bit is not loaded, and a group of ROWS
//     such rows only writes its Q x ROWS sentinels, one per lane -- scalar branches, no divergence. A failing
//     (q, r) is the sentinel 0 in the score array, below orderable() of every real float, whatever the row holds (the uninitialised
//     rows between count and capacity included). A passing row's rank counts only keys above it, all real,
//     so it is below the tile's pass count; sentinel rows write nothing.
//   * Bf16Rows: 8 elements per chunk, NC 1 .. 4; a chunk is unpacked inside the query loop.
//   * E4m3Rows (QSCAN; filtered only, live bitmap required): 16 elements per chunk, NC 1 .. 2; a group's bytes
//     are decoded to fp32 ONCE, before the query loop. Thread t stages scales[row0 + t] iff row t passes for
//     some query, so neither the bytes nor the scale of a dead row is ever loaded (NaN codes, NaN or inf
//     scales).
// Addresses: corpus rows [tile*T, min(N, tile*T + T)) at row * ldc elements + chunk * 16 B under
// chunk < D / E, the Q x D queries, and cand[(tile*Q + q)*k + s] with s < k -- `rank` is the one data-dependent
// index and is used only under `rank < k`. Filtered: live words [row0/32, row0/32 + 8) under word*32 < N (the
// launcher checks live_bytes), tags[row0 + t] under t < rows, filt[i] under i < 2Q. Scaled: scales[row0 + t]
// under t < rows.
//
// A row format (what each member means: DESIGN.md 4l, "One template, three kinds"): Elem is the stored element
// (`ldc` counts these), E the elements per 16-B chunk, MAX_NC the chunks per lane at D = 2048.
struct Bf16Rows {
  using Elem = unsigned short;
  static constexpr int E = 8, MAX_NC = 4;
  static constexpr bool WIDEN_ONCE = false, SCALED = false;
  template <bool FILT>
  using Args = std::conditional_t<FILT, HzSearchFilterParams, HzSearchParams>;
  static __device__ __forceinline__ void widen(const u32x4 v, float* f) { unpack8(v, f); }
};
struct E4m3Rows {
  using Elem = unsigned char;
  static constexpr int E = 16, MAX_NC = 2;
  static constexpr bool WIDEN_ONCE = true, SCALED = true;
  template <bool FILT>
  using Args = std::enable_if_t<FILT, HzSearchQuantParams>;
  // v_cvt_pk_f32_fp8: exact for the 254 finite codes, subnormals and -0 included
  static __device__ __forceinline__ void widen(const u32x4 v, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[i], false);  // bytes 0, 1 of the word
      const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)v[i], true);   // bytes 2, 3
      f[4 * i] = lo[0];
      f[4 * i + 1] = lo[1];
      f[4 * i + 2] = hi[0];
      f[4 * i + 3] = hi[1];
    }
  }
};

// the nested parameter blocks: each kind's block starts with the blocks of the kinds it extends
__host__ __device__ inline const HzSearchParams& scan_part(const HzSearchParams& a) { return a; }
__host__ __device__ inline const HzSearchParams& scan_part(const HzSearchFilterParams& a) { return a.s; }
__host__ __device__ inline const HzSearchParams& scan_part(const HzSearchQuantParams& a) { return a.f.s; }
__host__ __device__ inline const HzSearchFilterParams& filter_part(const HzSearchFilterParams& a) { return a; }
__host__ __device__ inline const HzSearchFilterParams& filter_part(const HzSearchQuantParams& a) { return a.f; }
__host__ __device__ inline const HzSearchFilterParams& filter_part(const HzSearchBinParams& a) { return a.f; }
__host__ __device__ inline const HzSearchFilterParams& filter_part(const HzSearchPqParams& a) { return a.f; }

// Dynamic LDS of a scan, in the kernel's order: queries [Q][D], scores [Q][T]; filtered: pass bits [T], the
// tile's live words [T / 32], filters [Q][2]; scaled: the passing rows' scales [T]. At most 144 KiB (Q = 16,
// D = 2048) + 1184 B + 1 KiB.
constexpr size_t lds_bytes(int Q, int D, bool filtered, bool scaled) {
  return ((size_t)Q * D + (size_t)Q * T + (filtered ? T + T / 32 + 2 * (size_t)Q : 0) + (scaled ? T : 0)) * 4;
}

__device__ __forceinline__ void stage_queries(const HzSearchParams& p, float* qs) {
  for (int i = threadIdx.x; i < p.Q * (p.D >> 2); i += T)
    reinterpret_cast<f32x4*>(qs)[i] = reinterpret_cast<const f32x4*>(p.queries)[i];
}

// Filtered: row t's pass bits over the queries into pmask[t] (rows past the tile's end: 0) and, for a scaled
// format, the scale of a passing row into scl[t]. One barrier inside; the caller's barrier publishes the result.
template <class Fmt, class A>
__device__ __forceinline__ void stage_pass_bits(const A& a, unsigned* pmask, float* scl, long row0, int rows) {
  const HzSearchFilterParams& fp = filter_part(a);
  const HzSearchParams& p = fp.s;
  unsigned* lv = pmask + T;      // [T / 32] live words of the tile
  unsigned* fl = lv + T / 32;    // [Q][2]
  const int t = threadIdx.x;
  unsigned tag = 0u;
  if (fp.tags && t < rows && HZ_DCHECK(row0 + t < (long)p.N)) tag = fp.tags[row0 + t];
  if (t < T / 32) {
    const long word = (row0 >> 5) + t;
    lv[t] = (word * 32 < (long)p.N && HZ_DCHECK((word + 1) * 4 <= (long)fp.live_bytes)) ? fp.live[word] : 0u;
  }
  if (fp.filt && t < 2 * p.Q && HZ_DCHECK(t < 2 * HZ_SEARCH_MAX_Q)) fl[t] = fp.filt[t];
  __syncthreads();
  unsigned bits = 0u;
  if (t < rows && ((lv[t >> 5] >> (t & 31)) & 1u)) {
    bits = (1u << p.Q) - 1u;  // Q <= 16
    if (fp.filt) {
      bits = 0u;
      for (int q = 0; q < p.Q; ++q) bits |= (unsigned)((tag & fl[2 * q]) == fl[2 * q + 1]) << q;
    }
  }
  pmask[t] = bits;
  if constexpr (Fmt::SCALED) {
    float s = 0.f;
    if (bits != 0u && HZ_DCHECK(t < rows && row0 + t < (long)p.N)) s = a.scales[row0 + t];
    scl[t] = s;
  }
}

// Which rows of a group are loaded and which (q, r) are scored. Unfiltered: the rows before the tile's end,
// for every query. Filtered: row r's pass bits (bit q = query q), wave-uniform.
template <bool FILT>
struct GroupPass {
  int r0, rows;  // the group's first row, the tile's rows
  __device__ __forceinline__ bool row(int r) const { return r0 + r < rows; }
  __device__ __forceinline__ bool pair(int, int) const { return true; }
};
template <>
struct GroupPass<true> {
  unsigned pm[ROWS];
  __device__ __forceinline__ bool row(int r) const { return pm[r] != 0u; }
  __device__ __forceinline__ bool pair(int q, int r) const { return (pm[r] >> q) & 1u; }
};

// The group in `v` (rows r0 .. r0 + ROWS - 1 of the tile) against every query: the contract's fmaf chain,
// butterfly and scale multiply, then the order-preserving score, or the sentinel 0 for a failing (q, r).
template <class Fmt, int NC, bool FILT>
__device__ __forceinline__ void score_group(const HzSearchParams& p, const float* qs, unsigned* sc, const float* scl,
                                            const u32x4 (&v)[ROWS][NC], const GroupPass<FILT>& pass, int lane, int nch,
                                            int r0, int rows) {
  constexpr int E = Fmt::E;
  float f[Fmt::WIDEN_ONCE ? ROWS : 1][Fmt::WIDEN_ONCE ? NC : 1][E], rs[ROWS];  // WIDEN_ONCE: the group as fp32
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    if constexpr (Fmt::SCALED) rs[r] = scl[r0 + r];  // every lane reads the same word: an LDS broadcast
    if constexpr (Fmt::WIDEN_ONCE) {
#pragma unroll
      for (int c = 0; c < NC; ++c) Fmt::widen(v[r][c], f[r][c]);
    }
  }
  for (int q = 0; q < p.Q; ++q) {
    float acc[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[r] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c * 64 + lane < nch) {
        const f32x4* qv4 = reinterpret_cast<const f32x4*>(qs + q * p.D + (c * 64 + lane) * E);
        float qv[E];
#pragma unroll
        for (int i = 0; i < E / 4; ++i) {
          const f32x4 x = qv4[i];
          qv[4 * i] = x[0], qv[4 * i + 1] = x[1], qv[4 * i + 2] = x[2], qv[4 * i + 3] = x[3];
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
          float g[E];
          const float* fr = g;
          if constexpr (Fmt::WIDEN_ONCE) fr = f[r][c];
          else Fmt::widen(v[r][c], g);
#pragma unroll
          for (int e = 0; e < E; ++e) acc[r] = fmaf(qv[e], fr[e], acc[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      float s = warp_sum(acc[r]);
      if constexpr (Fmt::SCALED) s *= rs[r];
      if (lane == r && r0 + r < rows) sc[q * T + r0 + r] = pass.pair(q, r) ? orderable(s) : 0u;
    }
  }
}

// Thread t ranks row t among the tile's scores `sc` ([T]) of one query and writes that query's candidate list
// `out`: the passing rows' best k keys, then key 0. `id` is the id field of row t's key: the row's position, or
// (HZ_K_SEARCH_LSCAN) the external id that rowid[] gives it. Unfiltered: every row passes, the pass count is `rows`.
template <bool FILT>
__device__ __forceinline__ void rank_query(const unsigned* sc, unsigned long long* out, bool slot_ok, int k, int rows,
                                           unsigned id) {
  const int t = threadIdx.x;
  // np: the tile's passing rows that can take a slot. Unfiltered: every row passes, so a thread past the
  // tile's end skips the loop and a real row needs no sentinel test.
  unsigned mine = 0u;
  int rank = 0, np = FILT ? 0 : min(k, rows);
  if (FILT || t < rows) {
    if (t < rows) mine = sc[t];
    for (int j = 0; j < rows; ++j) {  // every lane reads the same word: an LDS broadcast
      const unsigned o = sc[j];
      rank += (o > mine) || (o == mine && j < t);
      if constexpr (FILT) np += o != 0u;
    }
  }
  if ((FILT ? mine != 0u : t < rows) && rank < (FILT ? k : np) && slot_ok)
    out[rank] = ((unsigned long long)mine << 32) | (unsigned)~id;
  if (t >= np && t < k && slot_ok) out[t] = 0ull;  // the slots past the passing rows (k <= 128 < T)
}

// The tile's candidate lists of every query of the launch, the id of a key being the row's position.
template <bool FILT>
__device__ __forceinline__ void rank_tile(const HzSearchParams& p, const unsigned* sc, int tile, long row0, int rows) {
  for (int q = 0; q < p.Q; ++q) {
    unsigned long long* out = p.cand + ((long)tile * p.Q + q) * p.k;
    const bool slot_ok = HZ_DCHECK(((long)tile * p.Q + q + 1) * p.k * 8 <= (long)p.cand_bytes);
    rank_query<FILT>(sc + q * T, out, slot_ok, p.k, rows, (unsigned)(row0 + threadIdx.x));
  }
}

// The row loop of a scan workgroup: wave w scores rows w*64 .. w*64+63 of the tile at `row0` (`rows` of them)
// against the p.Q queries in `qs`, ROWS at a time, into sc[q * T + row]. Filtered: a row with no pass bit is not
// loaded and a group of such rows only writes its sentinels (the group skip).
template <class Fmt, int NC, bool FILT>
__device__ __forceinline__ void scan_rows(const HzSearchParams& p, const float* qs, unsigned* sc, const unsigned* pmask,
                                          const float* scl, long row0, int rows, int lane, int w, int nch) {
  const typename Fmt::Elem* corpus = reinterpret_cast<const typename Fmt::Elem*>(p.corpus);
  for (int g = 0; g < 64; g += ROWS) {  // wave-uniform bounds
    const int r0 = w * 64 + g;
    if (r0 >= rows) break;
    GroupPass<FILT> pass;
    if constexpr (FILT) {
      unsigned any = 0u;
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {  // r0 + r < T: rows past the tile's end have pass bits 0
        pass.pm[r] = __builtin_amdgcn_readfirstlane(pmask[r0 + r]);
        any |= pass.pm[r];
      }
      if (__builtin_expect(any == 0u, 0)) {  // scalar: nothing of this group is loaded or scored
        static_assert(ROWS * HZ_SEARCH_MAX_Q <= 64, "one lane per (q, r) sentinel");
        if (lane < ROWS * p.Q && r0 + lane % ROWS < rows) sc[lane / ROWS * T + r0 + lane % ROWS] = 0u;
        continue;
      }
    } else {
      pass.r0 = r0, pass.rows = rows;
    }
    u32x4 v[ROWS][NC];  // this lane's chunks of the group's rows, zeros where nothing is loaded
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        v[r][c] = u32x4{0u, 0u, 0u, 0u};
        if (pass.row(r) && c * 64 + lane < nch && HZ_DCHECK(row0 + r0 + r < (long)p.N))
          v[r][c] = *reinterpret_cast<const u32x4*>(corpus + (row0 + r0 + r) * p.ldc + (c * 64 + lane) * Fmt::E);
      }
    score_group<Fmt, NC>(p, qs, sc, scl, v, pass, lane, nch, r0, rows);
  }
}

template <class Fmt, int NC, bool FILT>
__global__ __launch_bounds__(T) void search_scan_kernel(const typename Fmt::template Args<FILT> a) {
  const HzSearchParams& p = scan_part(a);
  extern __shared__ __attribute__((aligned(16))) float lds[];  // lds_bytes()
  float* qs = lds;                                                      // [Q][D]
  unsigned* sc = reinterpret_cast<unsigned*>(lds + p.Q * p.D);          // [Q][T]
  unsigned* pmask = nullptr;  // filtered: [T] pass bits, then the tile's live words and the filters
  float* scl = nullptr;       // scaled: [T] scales of the passing rows
  if constexpr (FILT) pmask = sc + p.Q * T;
  if constexpr (Fmt::SCALED) scl = reinterpret_cast<float*>(pmask + T + T / 32 + 2 * p.Q);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = blockIdx.x;
  const int nch = p.D >> __builtin_ctz(Fmt::E);
  if (!HZ_DCHECK(tile < p.ntile && p.D <= NC * 64 * Fmt::E && p.ldc >= p.D && (long)tile * T < (long)p.N)) return;
  const long row0 = (long)tile * T;
  const int rows = (int)min((long)T, (long)p.N - row0);
  stage_queries(p, qs);
  if constexpr (FILT) stage_pass_bits<Fmt>(a, pmask, scl, row0, rows);
  __syncthreads();

  scan_rows<Fmt, NC, FILT>(p, qs, sc, pmask, scl, row0, rows, lane, w, nch);
  __syncthreads();
  rank_tile<FILT>(p, sc, tile, row0, rows);
}

// ------------------------------------------------------------------------------------ binary scan
// search_bscan_kernel<NCH> (HZ_K_SEARCH_BSCAN): the filtered scan over sign-bit rows of W = D / 32
// words (D % 128 == 0: whole 16-B chunks). NCH is the 16-B chunks a thread holds, sized to W at launch.
// CONTRACT (hipzap.h): score(q, r) = (float)(D - 2 * popcount(qbits ^ rbits)), qbits the query's D "sign bit clear"
// bits in the row's bit order. An integer sum, so no summation order exists: the bits depend on the query's sign
// bits and the row's words only. The query words past W and the row words that are not loaded are zero and add 0.
//   * query bits: wave w takes the 64-column blocks w, w + 4, ... of the Q x D fp32 queries; one ballot of "sign
//     clear" is two words of qb[q][WB] in LDS (WB = 4 NCH). -0.0 gives bit 0, like the rows' writer.
//   * pass bits: stage_pass_bits as the filtered kinds use it (BinRows: an unscaled format).
//   * scoring: thread t owns row t of the tile and holds its words in registers (16-B loads, only if some query
//     passes for the row); a wave whose 64 rows all fail loads nothing and writes its sentinels (a scalar branch).
//     Per query: xor + popcount against qb[q], whose reads are LDS broadcasts.
//   * ranking and the candidate lists: rank_tile<true>, then HZ_K_SEARCH_MERGE.
// Addresses: queries[q*D + i] under q < Q, i < D; corpus words [(row0 + t)*ldc + 4c, + 4) under t < rows, row < N
// and 4c < W <= ldc; live, tags, filt as in stage_pass_bits; cand through rank_tile (`rank < k`).
// Static LDS: qb 4 NCH * 16 words, scores [16][T], pass bits, live words and filters: at most 21,664 B.
struct BinRows {
  static constexpr bool SCALED = false;
};

template <int NCH>
__global__ __launch_bounds__(T) void search_bscan_kernel(const HzSearchBinParams a) {
  constexpr int WB = NCH * 4;  // words a thread holds; the query words from W to WB are zero
  const HzSearchParams& p = a.f.s;
  __shared__ __attribute__((aligned(16))) unsigned qb[HZ_SEARCH_MAX_Q * WB];
  __shared__ unsigned sc[HZ_SEARCH_MAX_Q * T];
  __shared__ unsigned pmask[T + T / 32 + 2 * HZ_SEARCH_MAX_Q];  // pass bits, the tile's live words, {mask, value}
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int tile = blockIdx.x;
  const int W = p.D >> 5;
  if (!HZ_DCHECK(tile < p.ntile && p.D >= 128 && p.D % 128 == 0 && W <= WB && p.ldc >= W && p.Q >= 1 &&
                 p.Q <= HZ_SEARCH_MAX_Q && (long)tile * T < (long)p.N))
    return;
  const long row0 = (long)tile * T;
  const int rows = (int)min((long)T, (long)p.N - row0);
  const int nblk = p.D >> 6;  // 64-column blocks of a query: two words each
  for (int i = w; i < p.Q * nblk; i += T / 64) {  // wave-uniform bounds
    const int q = i / nblk, c = i - q * nblk;
    float x = -1.f;
    if (HZ_DCHECK(q < p.Q && c * 64 + lane < p.D)) x = p.queries[(long)q * p.D + c * 64 + lane];
    const unsigned long long m = __ballot((__float_as_uint(x) >> 31) == 0u);
    if (lane == 0) qb[q * WB + 2 * c] = (unsigned)m, qb[q * WB + 2 * c + 1] = (unsigned)(m >> 32);
  }
  if (W < WB)
    for (int i = t; i < p.Q * (WB - W); i += T) qb[i / (WB - W) * WB + W + i % (WB - W)] = 0u;
  stage_pass_bits<BinRows>(a, pmask, nullptr, row0, rows);
  __syncthreads();

  const unsigned pm = pmask[t];  // 0 for a row past the tile's end
  if (__ballot(pm != 0u) != 0ull) {  // scalar: some row of this wave passes for some query
    const unsigned* corpus = reinterpret_cast<const unsigned*>(p.corpus);
    u32x4 v[NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
      v[c] = u32x4{0u, 0u, 0u, 0u};
      if (pm != 0u && c * 4 < W && HZ_DCHECK(t < rows && row0 + t < (long)p.N))
        v[c] = *reinterpret_cast<const u32x4*>(corpus + (row0 + t) * p.ldc + c * 4);
    }
    for (int q = 0; q < p.Q; ++q) {
      int pop = 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        const u32x4 x = *reinterpret_cast<const u32x4*>(qb + q * WB + c * 4);  // every lane reads the same words
        pop += __popc(v[c][0] ^ x[0]) + __popc(v[c][1] ^ x[1]) + __popc(v[c][2] ^ x[2]) + __popc(v[c][3] ^ x[3]);
      }
      sc[q * T + t] = ((pm >> q) & 1u) ? orderable((float)(p.D - 2 * pop)) : 0u;
    }
  } else {
    for (int q = 0; q < p.Q; ++q) sc[q * T + t] = 0u;
  }
  __syncthreads();
  rank_tile<true>(p, sc, tile, row0, rows);
}

// ------------------------------------------------------------------------------ product quantisation
// search_pqlut_kernel (HZ_K_SEARCH_PQLUT): grid (M, Q), PQ_KSUB threads. Thread c of workgroup (m, q)
// writes lut[(q*M + m)*256 + c]: the contract's fmaf chain over the dsub columns of sub-space m, ascending from +0.
// Addresses: queries[q*D + m*dsub + j] and codebook[(m*256 + c)*dsub + j] under j < dsub, m < M, q < Q; the one store
// under ((q*M + m)*256 + c + 1) * 4 <= lut_bytes.
constexpr int PQ_KSUB = 256;  // sub-centroids per sub-space: one code byte
__global__ __launch_bounds__(PQ_KSUB) void search_pqlut_kernel(const HzSearchPqLutParams a) {
  const int m = blockIdx.x, q = blockIdx.y, c = threadIdx.x;
  if (!HZ_DCHECK(m < a.M && q < a.Q && a.M >= 1 && a.D % a.M == 0)) return;
  const int dsub = a.D / a.M;
  const float* qv = a.queries + (long)q * a.D + m * dsub;       // every lane reads the same words
  const float* cv = a.codebook + ((long)m * PQ_KSUB + c) * dsub;
  float acc = 0.f;
  for (int j = 0; j < dsub; ++j) acc = fmaf(qv[j], cv[j], acc);
  const long at = ((long)q * a.M + m) * PQ_KSUB + c;
  if (HZ_DCHECK((at + 1) * 4 <= (long)a.lut_bytes)) a.lut[at] = acc;
}

// search_pqscan_kernel<NCH> (HZ_K_SEARCH_PQSCAN): the filtered scan over rows of M = 16 NCH code bytes against ONE
// query's table. Grid (ceil(ntile / span), Q); workgroup (g, q) copies lut[q] (M KiB) from global memory into LDS
// once, with 16-B loads, then walks the tiles g*span .. g*span + span - 1 (those below ntile). Per tile:
//   * pass bits: stage_pass_bits as the list scan uses it, over this workgroup's query alone (Q = 1, its {mask, value}).
//   * scoring: thread t owns row t and loads its NCH 16-B chunks only if the row passes for query q; a wave whose 64
//     rows all fail loads nothing and writes its sentinels (a scalar branch). score = the contract's sum: M plain
//     fp32 additions, m ascending from +0, of tab[m*256 + code[m]] -- one ds_read_b32 each, at random banks.
//   * ranking: rank_query<true>, the piece rank_tile is made of, into cand[(tile*Q + q)*k ..]: the layout
//     HZ_K_SEARCH_MERGE and HZ_K_SEARCH_RESCORE consume.
// Nothing of a score depends on the tile, on span or on the grid: the table is a function of (query, codebook) and
// the sum's order is fixed by M.
// Addresses: lut 16-B words [q*M*64, (q + 1)*M*64) under lut_bytes; corpus bytes [(row0 + t)*ldc + 16c, + 16) under
// t < rows, row < N and 16c < M <= ldc; live, tags, filt as in stage_pass_bits; cand through rank_query (`rank < k`).
// LDS: dynamic M KiB (the table), static scores [T], pass bits, live words and one filter: 2,096 B.
template <int NCH>
__global__ __launch_bounds__(T) void search_pqscan_kernel(const HzSearchPqParams a) {
  const HzSearchParams& p = a.f.s;
  extern __shared__ __attribute__((aligned(16))) float tab[];  // [M][256]
  __shared__ unsigned sc[T];
  __shared__ unsigned pmask[T + T / 32 + 2];  // pass bits, the tile's live words, {mask, value}
  const int t = threadIdx.x;
  const int q = blockIdx.y;
  const int M = NCH * 16;
  if (!HZ_DCHECK(a.M == M && a.span >= 1 && q < p.Q && p.Q >= 1 && p.Q <= HZ_SEARCH_MAX_Q && p.ldc >= M &&
                 (long)blockIdx.x * a.span < (long)p.ntile))
    return;
  {
    const f32x4* src = reinterpret_cast<const f32x4*>(a.lut) + (long)q * M * (PQ_KSUB / 4);
    for (int i = t; i < M * (PQ_KSUB / 4); i += T)
      if (HZ_DCHECK((((long)q * M * (PQ_KSUB / 4)) + i + 1) * 16 <= (long)a.lut_bytes))
        reinterpret_cast<f32x4*>(tab)[i] = src[i];
  }
  const unsigned char* corpus = reinterpret_cast<const unsigned char*>(p.corpus);
  HzSearchFilterParams f1 = a.f;  // what stage_pass_bits reads: this query and its {mask, value}, as in the list scan
  f1.s.Q = 1;
  if (f1.filt) f1.filt += 2 * q;
#pragma unroll 1
  for (int s = 0; s < a.span; ++s) {  // workgroup-uniform bounds
    const int tile = blockIdx.x * a.span + s;
    if (tile >= p.ntile) break;
    if (!HZ_DCHECK((long)tile * T < (long)p.N)) break;
    const long row0 = (long)tile * T;
    const int rows = (int)min((long)T, (long)p.N - row0);
    stage_pass_bits<BinRows>(f1, pmask, nullptr, row0, rows);  // its barrier also ends the last tile's reads of sc
    __syncthreads();                                           // and, in the first round, publishes the table

    const bool pass = pmask[t] & 1u;  // false for a row past the tile's end
    unsigned key = 0u;
    if (__ballot(pass) != 0ull) {  // scalar: some row of this wave passes for this query
      u32x4 v[NCH];
#pragma unroll
      for (int c = 0; c < NCH; ++c) {
        v[c] = u32x4{0u, 0u, 0u, 0u};
        if (pass && HZ_DCHECK(t < rows && row0 + t < (long)p.N))
          v[c] = *reinterpret_cast<const u32x4*>(corpus + (row0 + t) * p.ldc + c * 16);
      }
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < NCH; ++c)
#pragma unroll
        for (int w = 0; w < 4; ++w)
#pragma unroll
          for (int b = 0; b < 4; ++b) {
            const unsigned code = (v[c][w] >> (8 * b)) & 0xFFu;
            const int m = c * 16 + w * 4 + b;
            if (HZ_DCHECK(code < (unsigned)PQ_KSUB)) acc = acc + tab[m * PQ_KSUB + code];
          }
      if (pass) key = orderable(acc);
    }
    sc[t] = key;
    __syncthreads();
    unsigned long long* out = p.cand + ((long)tile * p.Q + q) * p.k;
    const bool slot_ok = HZ_DCHECK(((long)tile * p.Q + q + 1) * p.k * 8 <= (long)p.cand_bytes);
    rank_query<true>(sc, out, slot_ok, p.k, rows, (unsigned)(row0 + t));
  }
}

// search_pqassign_kernel<NQ> (HZ_K_SEARCH_PQASSIGN): for every row and sub-space the nearest of the 256
// sub-centroids under squared L2, in the contract's arithmetic (hipzap.h): plain fp32 subtract, multiply, add, one
// rounding each, j ascending from +0; contraction is switched off for the whole function. NQ = ceil(dsub / 4): a
// sub-vector and a centroid are held as DP = 4 NQ columns, the ones from dsub on ZERO in both -- t = 0 - 0 = +0 and
// acc + +0 = acc for every value acc can hold (never -0: acc starts at +0 and every term is >= +0 or NaN), so the
// padded sum has the bits of the dsub-term one and every instantiation agrees with every other.
// Grid (ceil(N / T), M / 16); workgroup (tile, g) walks the sub-spaces m = 16 g .. 16 g + 15. Per sub-space: the
// workgroup copies codebook[m] (256 x dsub fp32) into LDS as [256][DP] (16-B copies when dsub % 4 == 0, else word by
// word with the zero columns), thread t loads its row's dsub bf16 values (16-B loads when dsub % 8 == 0, else one
// element at a time: a sub-vector of an odd dsub is not 16-B aligned) and walks c = 0 .. 255: every lane reads the
// SAME centroid words (an LDS broadcast, ds_read_b128), 3 DP vector operations per centroid, then the strict
// `d < best`. Four sub-spaces make one code word and one 16-B store of distances; the four words of a group leave as
// one 16-B store of codes.
// Addresses: codebook words [m*256*dsub, (m + 1)*256*dsub) under m < M; rows[(row0 + t)*ldr + m*dsub + j] under
// row0 + t < N, j < dsub, m*dsub + dsub <= D <= ldr; codes bytes [(row0 + t)*ldc + 16 g, + 16) under 16 g + 16 <= M <=
// ldc and row < N; dist words [(row0 + t)*M + 16 g + 4 q, + 4) under (that end) * 4 <= dist_bytes.
// LDS: dynamic DP KiB. Registers: DP floats of the row, no scratch at any NQ (the resource table is in DESIGN.md 4x).
template <int NQ>
__global__ __launch_bounds__(T) void search_pqassign_kernel(const HzSearchPqAssignParams a) {
#pragma clang fp contract(off)
  constexpr int DP = NQ * 4;
  extern __shared__ __attribute__((aligned(16))) float cent[];  // [256][DP]
  const int t = threadIdx.x, g = blockIdx.y;
  if (!HZ_DCHECK(a.M >= 16 && a.M % 16 == 0 && a.D % a.M == 0 && g * 16 + 16 <= a.M && (a.D / a.M + 3) / 4 == NQ &&
                 a.ldr >= a.D && a.ldc >= a.M && (long)blockIdx.x * T < (long)a.N))
    return;
  const int dsub = a.D / a.M;
  const long row = (long)blockIdx.x * T + t;
  const bool real = row < (long)a.N;
  const long cb_words = (long)a.M * PQ_KSUB * dsub;
  u32x4 words = {0u, 0u, 0u, 0u};
#pragma unroll 1
  for (int q = 0; q < 4; ++q) {
    unsigned word = 0u;
    f32x4 d4 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = g * 16 + q * 4 + i;
      __syncthreads();  // the last sub-space's reads of `cent` are done
      const float* src = a.codebook + (long)m * PQ_KSUB * dsub;
      if (dsub == DP) {
        for (int e = t; e < PQ_KSUB * NQ; e += T)
          if (HZ_DCHECK((long)m * PQ_KSUB * dsub + 4l * e + 4 <= cb_words))
            reinterpret_cast<f32x4*>(cent)[e] = reinterpret_cast<const f32x4*>(src)[e];
      } else {
        for (int e = t; e < PQ_KSUB * DP; e += T) {
          const int c = e / DP, j = e % DP;
          float v = 0.f;
          if (j < dsub && HZ_DCHECK((long)m * PQ_KSUB * dsub + c * dsub + j < cb_words)) v = src[c * dsub + j];
          cent[e] = v;
        }
      }
      float x[DP];
#pragma unroll
      for (int j = 0; j < DP; ++j) x[j] = 0.f;
      if (real && HZ_DCHECK(row < (long)a.N && m * dsub + dsub <= a.D)) {
        const unsigned short* rp = a.rows + row * a.ldr + m * dsub;
        if (NQ % 2 == 0 && dsub == DP) {  // dsub % 8 == 0: the sub-vector is whole 16-B chunks
#pragma unroll
          for (int ch = 0; ch < NQ / 2; ++ch) unpack8(*reinterpret_cast<const u32x4*>(rp + ch * 8), x + ch * 8);
        } else {
#pragma unroll
          for (int j = 0; j < DP; ++j)
            if (j < DP - 4 || j < dsub) x[j] = bf2f(rp[j]);  // DP - 4 < dsub: only the last four columns ask
        }
      }
      __syncthreads();
      float best = 0.f;
      unsigned code = 0u;
#pragma unroll 2
      for (int c = 0; c < PQ_KSUB; ++c) {
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < NQ; ++k) {
          const f32x4 cv = *reinterpret_cast<const f32x4*>(cent + c * DP + k * 4);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const float tj = x[k * 4 + j] - cv[j];
            const float sq = tj * tj;
            acc = acc + sq;
          }
        }
        if (c == 0 || acc < best) {
          best = acc;
          code = (unsigned)c;
        }
      }
      word |= code << (8 * i);
      d4[i] = best;
    }
    words[0] = q == 0 ? word : words[0];
    words[1] = q == 1 ? word : words[1];
    words[2] = q == 2 ? word : words[2];
    words[3] = q == 3 ? word : words[3];
    const long at = row * a.M + g * 16 + q * 4;
    if (real && a.dist && HZ_DCHECK(row < (long)a.N && (at + 4) * 4 <= (long)a.dist_bytes))
      *reinterpret_cast<f32x4*>(a.dist + at) = d4;
  }
  if (real && HZ_DCHECK(row < (long)a.N && g * 16 + 16 <= a.ldc))
    *reinterpret_cast<u32x4*>(a.codes + row * a.ldc + g * 16) = words;
}

// -------------------------------------------------------------------------------------- list scan
// search_lscan_kernel<Fmt, NC> (HZ_K_SEARCH_LSCAN: Bf16Rows; HZ_K_SEARCH_QLSCAN: E4m3Rows, 4q): the
// filtered scan over an indirect, per-query set of tiles. Grid (P, Q); workgroup (j, q) finds the j-th tile of
// query q's probe set and scores it against query q ALONE with the template's pieces at Q = 1 (stage_queries,
// stage_pass_bits, scan_rows with its group skip, score_group), so a passing (q, r) has the bits of the filtered
// scan of its row format (kind 31's for bf16 rows, kind 34's for e4m3 rows) and a dead or padding row is never
// loaded: neither its elements nor, for e4m3 rows, its scale.
// Addressing: thread i < nprobe reads probes[q*nprobe + i] = l, and under (unsigned)l < nlist the pair
// a = list_off[l], b = list_off[l + 1]; under 0 <= a <= b <= ntile its count b - a and start a go to LDS, else
// the count -1. Every thread then walks the nprobe counts in probe order (LDS broadcasts): the running sum
// finds the probe whose range holds j and the index x = a + (j - sum before) < b <= ntile into list_tiles, whose
// length is ntile. tile = list_tiles[x] is used under (unsigned)tile < ntile. A count of -1, a j at or past the
// total and a tile out of range all end in k zero keys for this workgroup's slot and nothing else read.
// probes == NULL: tile = j under j < ntile. rowid[row0 + t] is read once per tile (coalesced) under
// row0 + t < N; N = ntile * T (the launcher refuses anything else), so every tile is whole. E4m3Rows:
// scales[row0 + t] under the same bound, and only for a passing row (stage_pass_bits).
// Dynamic LDS: lds_bytes(1, D, true, SCALED) = (D + 2 T + T / 32 + 2 (+ T)) * 4 <= 11,304 B; static: 2 x 128 ints.
template <class Fmt>
using ListArgs = std::conditional_t<Fmt::SCALED, HzSearchQuantListParams, HzSearchListParams>;
__host__ __device__ inline const HzSearchListParams& list_part(const HzSearchListParams& a) { return a; }
__host__ __device__ inline const HzSearchListParams& list_part(const HzSearchQuantListParams& a) { return a.l; }
// the block the template's pieces read for one query: the filtered scan's, with the row scales where the format has them
__device__ __forceinline__ HzSearchFilterParams one_query(const HzSearchFilterParams& f, const HzSearchListParams&) { return f; }
__device__ __forceinline__ HzSearchQuantParams one_query(const HzSearchFilterParams& f, const HzSearchQuantListParams& a) {
  return HzSearchQuantParams{f, a.scales};
}

template <class Fmt, int NC>
__global__ __launch_bounds__(T) void search_lscan_kernel(const ListArgs<Fmt> args) {
  const HzSearchListParams& a = list_part(args);
  const HzSearchParams& p = a.f.s;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  __shared__ int pcnt[HZ_SEARCH_MAX_K], poff[HZ_SEARCH_MAX_K];  // the probed lists' tile counts and starts
  float* qs = lds;                                        // [D]
  unsigned* sc = reinterpret_cast<unsigned*>(lds + p.D);  // [T]
  unsigned* pmask = sc + T;                               // [T] pass bits, the tile's live words, {mask, value}
  float* scl = nullptr;                                   // scaled: [T] scales of the passing rows
  if constexpr (Fmt::SCALED) scl = reinterpret_cast<float*>(pmask + T + T / 32 + 2);
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int j = blockIdx.x, q = blockIdx.y;
  const int nch = p.D >> __builtin_ctz(Fmt::E);
  if (!HZ_DCHECK(j < a.P && q < p.Q && p.k >= 1 && p.k <= HZ_SEARCH_MAX_K && p.D <= NC * 64 * Fmt::E && p.ldc >= p.D &&
                 p.N == p.ntile * T && a.nlist >= 1))
    return;
  unsigned long long* out = p.cand + ((long)j * p.Q + q) * p.k;
  const bool slot_ok = HZ_DCHECK(((long)j * p.Q + q + 1) * p.k * 8 <= (long)p.cand_bytes);
  int tile = -1;
  if (a.probes) {
    if (!HZ_DCHECK(a.nprobe >= 1 && a.nprobe <= HZ_SEARCH_MAX_K)) return;
    if (t < a.nprobe) {
      const int l = a.probes[(long)q * a.nprobe + t];
      int cnt = -1, off = 0;
      if ((unsigned)l < (unsigned)a.nlist) {
        const int lo = a.list_off[l], hi = a.list_off[l + 1];
        if (lo >= 0 && lo <= hi && hi <= p.ntile) cnt = hi - lo, off = lo;
      }
      pcnt[t] = cnt, poff[t] = off;
    }
    __syncthreads();
    int sum = 0, at = -1;
    bool bad = false;
    for (int i = 0; i < a.nprobe; ++i) {  // every lane reads the same words: LDS broadcasts
      const int c = pcnt[i];
      bad |= c < 0;
      if (at < 0 && c > 0 && j < sum + c) at = poff[i] + (j - sum);
      sum += c > 0 ? c : 0;
    }
    if (!bad && at >= 0 && HZ_DCHECK(at < p.ntile)) tile = a.list_tiles[at];
  } else {
    tile = j;
  }
  if ((unsigned)tile >= (unsigned)p.ntile) {  // an idle workgroup (block-uniform): its slot holds no candidate
    if (t < p.k && slot_ok) out[t] = 0ull;
    return;
  }
  const long row0 = (long)tile * T;
  unsigned id = 0u;
  if (HZ_DCHECK(row0 + t < (long)p.N)) id = (unsigned)a.rowid[row0 + t];
  HzSearchFilterParams f1 = a.f;  // what the template's pieces read: this query, and its {mask, value}
  f1.s.Q = 1;
  f1.s.queries = p.queries + (long)q * p.D;
  if (f1.filt) f1.filt += 2 * q;
  const auto one = one_query(f1, args);
  stage_queries(f1.s, qs);
  stage_pass_bits<Fmt>(one, pmask, scl, row0, T);
  __syncthreads();
  scan_rows<Fmt, NC, true>(f1.s, qs, sc, pmask, scl, row0, T, lane, w, nch);
  __syncthreads();
  rank_query<true>(sc, out, slot_ok, p.k, T, id);
}

// ------------------------------------------------------------------------------------------ merge
// Query q's ntile * k keys, MERGE_THREADS * MERGE_E per round. `best` holds the k best so far, best first
// (zeros at the start). A key survives a round iff it is above best[k - 1]; the survivors are compacted
// behind `best` (positions from a wave prefix sum, no atomics) and every entry of the pool is ranked among
// the pool: the k highest, in order, are the new `best`. A round with more than 2k survivors (the first ones)
// first drops every key below the k-th largest of the threads' own maxima. Keys of real rows are distinct (the id is part
// of the key) and key 0 never survives, so ranks are distinct and the result is a function of the key SET:
// it does not depend on the round a key arrives in. Most rounds have no survivor and only load.
// cnt per thread -> this thread's exclusive offset among the workgroup's survivors and their total (thread
// order: a prefix sum over each wave, then the waves' totals in wave order). Two barriers: `wave_cnt` is
// free again on return.
__device__ __forceinline__ void merge_offsets(int cnt, int lane, int w, int* wave_cnt, int& off, int& total) {
  int incl = cnt;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wave_cnt[w] = incl;
  __syncthreads();
  off = incl - cnt;
  total = 0;
#pragma unroll
  for (int i = 0; i < MERGE_THREADS / 64; ++i) {
    if (i < w) off += wave_cnt[i];
    total += wave_cnt[i];
  }
  __syncthreads();
}

__global__ __launch_bounds__(MERGE_THREADS) void search_merge_kernel(const HzSearchParams p) {
  __shared__ unsigned long long best[HZ_SEARCH_MAX_K];
  __shared__ unsigned long long pool[MERGE_POOL];
  __shared__ unsigned long long tmax[MERGE_THREADS];
  __shared__ unsigned long long thr2;
  __shared__ int wave_cnt[MERGE_THREADS / 64];
  const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (!HZ_DCHECK(q < p.Q && p.k >= 1 && p.k <= HZ_SEARCH_MAX_K)) return;
  const long per_tile = (long)p.Q * p.k;
  const int total = p.ntile * p.k;  // < 2^23 tiles x 128
  if (t < p.k) best[t] = 0ull;
  __syncthreads();
  for (int base = 0; base < total; base += MERGE_THREADS * MERGE_E) {
    const unsigned long long thr = best[p.k - 1];
    unsigned long long key[MERGE_E];
    int cnt = 0;
#pragma unroll
    for (int e = 0; e < MERGE_E; ++e) {
      const int i = base + e * MERGE_THREADS + t;  // candidate i of query q: tile i / k, slot i % k
      key[e] = 0ull;
      if (i < total) {
        const int tile = i / p.k;
        const long at = tile * per_tile + (long)q * p.k + (i - tile * p.k);
        if (HZ_DCHECK((at + 1) * 8 <= (long)p.cand_bytes)) key[e] = p.cand[at];
      }
      if (key[e] <= thr) key[e] = 0ull;
      cnt += key[e] != 0ull;
    }
    int off = 0, nsurv = 0;
    merge_offsets(cnt, lane, w, wave_cnt, off, nsurv);
    if (nsurv == 0) continue;  // block-uniform
    if (nsurv > 2 * p.k) {
      // many survivors (the first rounds): only the round's k best can matter. The k-th largest of the
      // threads' own maxima has k keys at or above it, so every key below it is out.
      unsigned long long m = 0ull;
#pragma unroll
      for (int e = 0; e < MERGE_E; ++e) m = key[e] > m ? key[e] : m;
      tmax[t] = m;
      __syncthreads();
      int rank = 0;
      for (int j = 0; j < MERGE_THREADS; ++j) {
        const unsigned long long o = tmax[j];
        rank += (o > m) || (o == m && j < t);
      }
      if (rank == p.k - 1) thr2 = m;  // exactly one thread: ranks are distinct
      __syncthreads();
      const unsigned long long lo = thr2;
      cnt = 0;
#pragma unroll
      for (int e = 0; e < MERGE_E; ++e) {
        if (key[e] < lo) key[e] = 0ull;
        cnt += key[e] != 0ull;
      }
      merge_offsets(cnt, lane, w, wave_cnt, off, nsurv);
    }
    if (t < p.k) pool[t] = best[t];
#pragma unroll
    for (int e = 0; e < MERGE_E; ++e)
      if (key[e] != 0ull && p.k + off < MERGE_POOL) pool[p.k + off++] = key[e];
    __syncthreads();
    const int n = p.k + nsurv;
    for (int i = t; i < n; i += MERGE_THREADS) {
      const unsigned long long mine = pool[i];
      int rank = 0;
      for (int j = 0; j < n; ++j) {
        const unsigned long long o = pool[j];
        rank += (o > mine) || (o == mine && j < i);  // equal keys: only the zeros of an unfilled `best`
      }
      if (rank < p.k) best[rank] = mine;
    }
    __syncthreads();
  }
  if (t < p.k) {
    const unsigned long long key = best[t];
    const long at = (long)q * p.k + t;
    p.out_score[at] = key ? unorderable((unsigned)(key >> 32)) : -__builtin_inff();
    p.out_id[at] = key ? (int)~(unsigned)key : -1;
  }
}

// ---------------------------------------------------------------------------------------- rescore
// search_rescore_kernel<NC>: the second stage of a two-stage search. Workgroup q scores query q
// against the R rows that in_id[q][0 .. R) names and writes the best k of them. A slot is real iff
// (unsigned)id < (unsigned)N; every other value (the merge's -1 of an unused slot) is an empty slot: nothing is
// loaded for it and its score is the sentinel 0. Wave w takes the slots w*ROWS .. w*ROWS + ROWS - 1, then the
// next RESCORE_THREADS / 64 * ROWS on, their 16-byte loads in flight together; the group's scores come from
// score_group<Bf16Rows, NC> with one query, so a real (q, r) has the bits of HZ_K_SEARCH_SCAN for that query and
// row. Thread t < R then ranks slot t among the R: higher score first, then the lower id, then the lower slot
// (stage one's ids are distinct; the slot only keeps ranks distinct when a caller repeats an id). The slots
// ranked below k write out[rank]; the slots from the number of real candidates to k get -inf / -1.
// 512 threads: R = 128 is 32 groups of ROWS, four per wave, and up to 8 x ROWS rows are in flight per query --
// the launch is latency-bound (at most 16 workgroups, rows that may lie in pinned host memory), not
// occupancy-bound; 1024 threads would halve the register budget that NC = 4 needs for its 16 chunks in flight.
// Addresses: queries[q*D + i] under i < D, in_id[q*R + t] under t < R, rows[id*ldc + chunk*8 ..] under
// (unsigned)id < (unsigned)N and chunk < D / 8 -- the one data-dependent address --, out_*[q*k + s] under s < k.
constexpr int RESCORE_THREADS = 512;
static_assert(HZ_SEARCH_MAX_K % ROWS == 0 && HZ_SEARCH_MAX_K <= T, "a group never reads past ids[] / sc[]");

template <int NC>
__global__ __launch_bounds__(RESCORE_THREADS) void search_rescore_kernel(const HzSearchRescoreParams a) {
  __shared__ __attribute__((aligned(16))) float qs[2048];  // the query
  __shared__ unsigned sc[HZ_SEARCH_MAX_K];                  // orderable scores, 0 for an empty slot
  __shared__ int ids[HZ_SEARCH_MAX_K];                      // in_id[q], -1 past R
  const int q = blockIdx.x, t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nch = a.D >> 3;
  if (!HZ_DCHECK(q < a.Q && a.D >= 8 && a.D % 8 == 0 && a.D <= NC * 64 * 8 && a.D <= 2048 && a.ldc >= a.D && a.N >= 1 &&
                 a.R >= 1 && a.R <= HZ_SEARCH_MAX_K && a.k >= 1 && a.k <= a.R))
    return;
  for (int i = t; i < a.D >> 2; i += RESCORE_THREADS)
    if (HZ_DCHECK((long)q * a.D + 4 * i + 4 <= (long)a.Q * a.D))
      reinterpret_cast<f32x4*>(qs)[i] = reinterpret_cast<const f32x4*>(a.queries + (long)q * a.D)[i];
  if (t < HZ_SEARCH_MAX_K) {
    int id = -1;
    if (t < a.R && HZ_DCHECK((long)q * a.R + t < (long)a.Q * a.R)) id = a.in_id[(long)q * a.R + t];
    ids[t] = id;
  }
  __syncthreads();

  HzSearchParams one{};  // what score_group reads of the scan's block: one query of D values
  one.Q = 1, one.D = a.D;
  for (int r0 = w * ROWS; r0 < a.R; r0 += RESCORE_THREADS / 64 * ROWS) {  // wave-uniform bounds
    GroupPass<true> pass;
    int id[ROWS];
    unsigned any = 0u;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {  // r0 + r < HZ_SEARCH_MAX_K: the slots past R hold -1
      id[r] = __builtin_amdgcn_readfirstlane(ids[r0 + r]);
      pass.pm[r] = (unsigned)id[r] < (unsigned)a.N ? 1u : 0u;
      any |= pass.pm[r];
    }
    if (any == 0u) {  // scalar: nothing of this group is loaded or scored
      if (lane < ROWS && r0 + lane < a.R) sc[r0 + lane] = 0u;
      continue;
    }
    u32x4 v[ROWS][NC];  // this lane's chunks of the group's rows, zeros where nothing is loaded
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        v[r][c] = u32x4{0u, 0u, 0u, 0u};
        if (pass.row(r) && c * 64 + lane < nch &&
            HZ_DCHECK(id[r] >= 0 && id[r] < a.N && (long)id[r] * a.ldc + (c * 64 + lane) * 8 + 8 <= ((long)a.N - 1) * a.ldc + a.D))
          v[r][c] = *reinterpret_cast<const u32x4*>(a.rows + (long)id[r] * a.ldc + (c * 64 + lane) * 8);
      }
    score_group<Bf16Rows, NC>(one, qs, sc, nullptr, v, pass, lane, nch, r0, a.R);
  }
  __syncthreads();

  if (t < a.R) {
    const unsigned mine = sc[t];
    const int me = ids[t];
    int rank = 0, nreal = 0;
    for (int j = 0; j < a.R; ++j) {  // every lane reads the same words: LDS broadcasts
      const unsigned o = sc[j];
      const int oid = ids[j];
      rank += (o > mine) || (o == mine && (oid < me || (oid == me && j < t)));
      nreal += o != 0u;
    }
    const long at = (long)q * a.k;
    if (mine != 0u && rank < a.k && HZ_DCHECK(at + rank < (long)a.Q * a.k)) {  // real keys only above a real key
      a.out_score[at + rank] = unorderable(mine);
      a.out_id[at + rank] = me;
    }
    if (t >= nreal && t < a.k && HZ_DCHECK(at + t < (long)a.Q * a.k)) {
      a.out_score[at + t] = -__builtin_inff();
      a.out_id[at + t] = -1;
    }
  }
}

template <int NC = 1>
void rescore_dispatch(const HzSearchRescoreParams& a, hipStream_t st) {
  if constexpr (NC < Bf16Rows::MAX_NC) {
    if (a.D > NC * 64 * Bf16Rows::E) return rescore_dispatch<NC + 1>(a, st);
  }
  hipLaunchKernelGGL(search_rescore_kernel<NC>, dim3(a.Q), dim3(RESCORE_THREADS), 0, st, a);
}

// -------------------------------------------------------------------------------------- self scan
// search_mscan_kernel (HZ_K_SEARCH_MSCAN): workgroup (tile, qb) scores the tile's T rows against the
// QB rows that qid[qb*QB ..] names. Both operands are bf16 rows of the corpus, so a lane's MFMA fragment -- 8
// consecutive columns of one row -- is one 16-byte load for either operand and nothing is staged or converted:
// the A operand is the query rows (read by id; every workgroup of the block re-reads the same QB rows, which stay
// in L2), the B operand the tile's rows. Wave w owns rows w*64 .. w*64+63 of the tile as four groups of 16 and
// holds the 64 x 64 scores of its rows against the block's queries in 16 accumulators of 4 floats.
// CONTRACT (hipzap.h): acc = mfma_f32_16x16x32_bf16(query fragment, row fragment, acc) over the columns 32s ..
// 32s+31, s ascending, from +0. The k-steps are loaded two at a time, one pair ahead of the MFMAs.
// Which rows: the tile's live words are staged with the bits from N on cleared. A group whose 16 live bits are 0
// is not loaded and its MFMAs are skipped (a scalar branch); a dead row of a mixed group is loaded and scores the
// sentinel 0, like (q, r) with skip_self and r == qid[q] and every pair of a query whose id is outside [0, N).
// A NaN pattern in a dead row reaches only that row's own column of the product.
// Selection: the scores land in LDS as order-preserving u32, sc[q][row] (row stride T + 4 words: the four lane
// groups of a store hit different banks). Wave w then takes the queries w, w + 4, ... one at a time; lane l holds
// rows l, l + 64, l + 128, l + 192 as keys. For k <= 64 the wave first finds, by a radix search over the top
// MSCAN_CUT_BITS bits of the lanes' maxima (one ballot per bit), the largest prefix that at least k maxima reach:
// k keys lie at or above it, so every key below it is out. The survivors are compacted into the wave's pool
// (positions from ballots, no atomics) and ranked among themselves; ranks below k write cand[rank]. Keys of real
// rows are distinct, so the list is a function of the tile's key set. k > 64: every passing key is a survivor.
// Addresses: qid[q] under q < Q; corpus[id*ldc + ..] under (unsigned)id < N; the tile's rows under row < N; live
// words [row0/32, row0/32 + 8) under word*32 < N (the launcher checks live_bytes); cand[(tile*Q + q)*k + s] under
// q < Q and s < k -- `rank` is used only under rank < k.
constexpr int QB = HZ_SEARCH_SELF_QB;
constexpr int MSCAN_TS = T + 4;        // words per query in the score array
constexpr int MSCAN_CUT_BITS = 20;     // sign, exponent and 11 mantissa bits of the score
static_assert(QB == 64 && T == 256 && QB % 16 == 0, "the fragment and selection maps below");
// dynamic LDS: scores [QB][MSCAN_TS] u32, the waves' pools [4][T] u64, the block's ids [QB], live words [T / 32]
constexpr size_t MSCAN_LDS = (size_t)QB * MSCAN_TS * 4 + 4 * (size_t)T * 8 + QB * 4 + T / 32 * 4;

// The tile's live words -> lv[T / 32] with the bits from N on cleared (threads t < T / 32; the caller's barrier
// publishes them). live words [row0/32, row0/32 + 8) under word*32 < N: the launchers check live_bytes.
__device__ __forceinline__ void stage_live_words(const unsigned* live, unsigned long long live_bytes, int N, long row0, int rows,
                                                 unsigned* lv) {
  const int t = threadIdx.x;
  if (t < T / 32) {
    const long word = (row0 >> 5) + t;
    unsigned v = 0u;
    if (word * 32 < (long)N && HZ_DCHECK((word + 1) * 4 <= (long)live_bytes)) v = live[word];
    const int left = rows - t * 32;  // the tile's rows from this word on
    if (left < 32) v &= left <= 0 ? 0u : (1u << left) - 1u;
    lv[t] = v;
  }
}

// The selection of the self scan and of the batch scan (the comment above: radix cut, compaction, ranking): the
// block's nq queries from the score array sc[q][row] into cand[(tile*Q + q0 + q)*k ..], wave w taking the queries
// w, w + 4, ... one at a time through its pool.
__device__ __forceinline__ void mscan_select(const unsigned* sc, unsigned long long* pool, unsigned long long* cand,
                                             unsigned long long cand_bytes, int Q, int k, int tile, int q0, int nq, long row0,
                                             int w, int lane) {
  unsigned long long* mine_pool = pool + w * T;
  for (int i = 0; i * 4 < nq; ++i) {  // block-uniform trips: the barriers below are reached by every wave
    const int q = i * 4 + w;
    const bool valid = q < nq;  // wave-uniform
    int n = 0, npass = 0;
    if (valid) {
      unsigned long long key[4];
      unsigned mx = 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned s = sc[q * MSCAN_TS + j * 64 + lane];
        key[j] = s ? ((unsigned long long)s << 32) | (unsigned)~(unsigned)(row0 + j * 64 + lane) : 0ull;
        npass += __popcll(__ballot(s != 0u));
        mx = s > mx ? s : mx;
      }
      unsigned thr = 0u;
      if (k <= 64) {  // the largest prefix that at least k of the lanes' maxima reach; 0: fewer than k lanes pass
        for (int bit = 31; bit >= 32 - MSCAN_CUT_BITS; --bit) {
          const unsigned c = thr | (1u << bit);
          if (__popcll(__ballot(mx >= c)) >= k) thr = c;
        }
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool keep = key[j] != 0ull && (unsigned)(key[j] >> 32) >= thr;
        const unsigned long long m = __ballot(keep);
        const int at = n + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (keep && HZ_DCHECK(at < T)) mine_pool[at] = key[j];
        n += __popcll(m);
      }
    }
    __syncthreads();
    if (valid) {
      const long slot = (long)tile * Q + q0 + q;
      unsigned long long* out = cand + slot * k;
      const bool slot_ok = HZ_DCHECK(q0 + q < Q && (slot + 1) * k * 8 <= (long)cand_bytes);
      for (int e = lane; e < n; e += 64) {
        const unsigned long long mine = mine_pool[e];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += mine_pool[j] > mine;  // every lane reads the same word: a broadcast
        if (rank < k && slot_ok) out[rank] = mine;
      }
      const int filled = min(k, npass);  // n >= filled: the cut keeps at least k keys, or every passing one
      for (int s = lane; s < k; s += 64)
        if (s >= filled && slot_ok) out[s] = 0ull;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(T) void search_mscan_kernel(const HzSearchSelfParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  unsigned* sc = reinterpret_cast<unsigned*>(lds);                                     // [QB][MSCAN_TS]
  unsigned long long* pool = reinterpret_cast<unsigned long long*>(sc + QB * MSCAN_TS);  // [4][T]
  int* qids = reinterpret_cast<int*>(pool + 4 * T);                                    // [QB], -1: no query
  unsigned* lv = reinterpret_cast<unsigned*>(qids + QB);                               // [T / 32]
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int tile = blockIdx.x, q0 = blockIdx.y * QB;
  if (!HZ_DCHECK(tile < p.ntile && (long)tile * T < (long)p.N && q0 < p.Q && p.D >= 32 && p.D % 32 == 0 && p.D <= 2048 &&
                 p.ldc >= p.D && p.k >= 1 && p.k <= HZ_SEARCH_MAX_K))
    return;
  const long row0 = (long)tile * T;
  const int rows = (int)min((long)T, (long)p.N - row0);
  const int nq = min(QB, p.Q - q0);
  if (t < QB) {
    int id = -1;
    if (t < nq && HZ_DCHECK(q0 + t < p.Q)) id = p.qid[q0 + t];
    qids[t] = (unsigned)id < (unsigned)p.N ? id : -1;
  }
  stage_live_words(p.live, p.live_bytes, p.N, row0, rows, lv);
  __syncthreads();

  const int lr = lane & 15, lh = lane >> 4;
  unsigned gm[4], any = 0u;  // the live bits of this wave's four groups (wave-uniform)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int g = w * 4 + j;
    gm[j] = (__builtin_amdgcn_readfirstlane(lv[g >> 1]) >> ((g & 1) * 16)) & 0xffffu;
    any |= gm[j];
  }
  f32x4 acc[4][4];  // [query group][row group]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (any != 0u) {
    const bf16_t* arow[4];
    const bf16_t* brow[4];
    bool aok[4], bok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = qids[i * 16 + lr];
      aok[i] = id >= 0 && HZ_DCHECK(id < p.N);
      arow[i] = p.corpus + (long)(aok[i] ? id : 0) * p.ldc + lh * 8;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = w * 64 + j * 16 + lr;
      bok[j] = gm[j] != 0u && r < rows && HZ_DCHECK(row0 + r < (long)p.N);
      brow[j] = p.corpus + (row0 + (bok[j] ? r : 0)) * p.ldc + lh * 8;
    }
    const int nk = p.D >> 5;
    bf16x8 a[2][2][4], b[2][2][4];  // [buffer][k-step of the pair][group]
    auto load = [&](int buf, int kk) {  // the k-steps kk and kk + 1 (columns under D: kk*32 + lh*8 + 8 <= D)
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          a[buf][s][i] = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
          b[buf][s][i] = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
          if (kk + s < nk) {
            if (aok[i]) a[buf][s][i] = *reinterpret_cast<const bf16x8*>(arow[i] + (kk + s) * 32);
            if (bok[i]) b[buf][s][i] = *reinterpret_cast<const bf16x8*>(brow[i] + (kk + s) * 32);
          }
        }
    };
    auto mma = [&](int buf, int kk) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
        if (kk + s < nk) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (gm[j] != 0u) {
#pragma unroll
              for (int i = 0; i < 4; ++i)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[buf][s][i], b[buf][s][j], acc[i][j], 0, 0, 0);
            }
        }
    };
    load(0, 0);
    for (int kk = 0; kk < nk; kk += 4) {  // two pairs per trip, so the buffer index is a constant
      if (kk + 2 < nk) load(1, kk + 2);
      mma(0, kk);
      if (kk + 4 < nk) load(0, kk + 4);
      if (kk + 2 < nk) mma(1, kk + 2);
    }
  }
  // lane holds score(query i*16 + lh*4 + e, row w*64 + j*16 + lr) in acc[i][j][e]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = i * 16 + lh * 4 + e;
      const int id = qids[q];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = w * 64 + j * 16 + lr;
        const bool pass = ((gm[j] >> lr) & 1u) && id >= 0 && !(p.skip_self && (long)id == row0 + r);
        sc[q * MSCAN_TS + r] = pass ? orderable(acc[i][j][e]) : 0u;
      }
    }
  __syncthreads();

  mscan_select(sc, pool, p.cand, p.cand_bytes, p.Q, p.k, tile, q0, nq, row0, w, lane);
}

// ------------------------------------------------------------------------------------- batch scan
// search_xscan_kernel (HZ_K_SEARCH_XSCAN): the self scan with an EXTERNAL A operand. Workgroup (tile,
// qb) scores the tile's T rows against the fp32 queries qb*QB .. qb*QB + QB - 1. The grid, the B-operand loads, the
// live words and the group skip, the score array, the selection and the candidate layout are the self scan's (the
// shared functions above); there is no qid and no skip_self.
// A operand: a lane's fragment is 8 consecutive columns of one query, two 16-byte loads of fp32, split in registers
// into three bf16x8 fragments (split3 below; hipzap.h states the split). A query slot at or past Q loads nothing;
// a group of 16 slots past Q is neither split nor multiplied (a scalar branch).
// CONTRACT (hipzap.h): one set of accumulators; per 32-column step the MFMAs of an accumulator are issued in the
// order l, m, h, the steps in column order from +0. Every product of a bf16 term and a bf16 row value is exact.
// Registers: the k-steps are loaded ONE at a time, one ahead of the MFMAs -- a step's A operand is 8 VGPRs per query
// group where the self scan's is 4, so its pairs would not fit beside the 64 accumulators at 2 waves per SIMD.
// Addresses: queries[q*D + kk*32 + lh*8 .. + 8) under q < Q and kk < D / 32; the tile's rows under row < N; live
// words through stage_live_words; cand through mscan_select (q < Q, `rank` used only under rank < k).
// dynamic LDS: scores [QB][MSCAN_TS] u32, the waves' pools [4][T] u64, live words [T / 32]
constexpr size_t XSCAN_LDS = (size_t)QB * MSCAN_TS * 4 + 4 * (size_t)T * 8 + T / 32 * 4;

// the bits of one term of the split: a term whose exponent field is zero becomes a zero of its sign
__device__ __forceinline__ unsigned split_term(unsigned b) { return (b & 0x7f800000u) ? b : (b & 0x80000000u); }

// x -> the fp32 bits of h', m', l' (each a bf16 value: the low 16 bits are zero). h = the top 16 bits of x,
// m = the top 16 bits of x - h, l = (x - h) - m, both differences exact in fp32; then split_term on each.
__device__ __forceinline__ void split3(float x, unsigned& h, unsigned& m, unsigned& l) {
  const unsigned hb = __float_as_uint(x) & 0xffff0000u;
  const float r1 = x - __uint_as_float(hb);
  const unsigned mb = __float_as_uint(r1) & 0xffff0000u;
  const unsigned lb = __float_as_uint(r1 - __uint_as_float(mb));
  h = split_term(hb), m = split_term(mb), l = split_term(lb);
}

// 8 consecutive columns of a query -> its three MFMA fragments
__device__ __forceinline__ void split_frag(const f32x4 lo, const f32x4 hi, bf16x8& fh, bf16x8& fm, bf16x8& fl) {
  const float x[8] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  u32x4 wh, wm, wl;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned h0, m0, l0, h1, m1, l1;
    split3(x[2 * j], h0, m0, l0);
    split3(x[2 * j + 1], h1, m1, l1);
    wh[j] = (h0 >> 16) | h1, wm[j] = (m0 >> 16) | m1, wl[j] = (l0 >> 16) | l1;  // the low halves are zero
  }
  fh = __builtin_bit_cast(bf16x8, wh), fm = __builtin_bit_cast(bf16x8, wm), fl = __builtin_bit_cast(bf16x8, wl);
}

__global__ __launch_bounds__(T) void search_xscan_kernel(const HzSearchBatchParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  unsigned* sc = reinterpret_cast<unsigned*>(lds);                                     // [QB][MSCAN_TS]
  unsigned long long* pool = reinterpret_cast<unsigned long long*>(sc + QB * MSCAN_TS);  // [4][T]
  unsigned* lv = reinterpret_cast<unsigned*>(pool + 4 * T);                            // [T / 32]
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int tile = blockIdx.x, q0 = blockIdx.y * QB;
  if (!HZ_DCHECK(tile < p.ntile && (long)tile * T < (long)p.N && q0 < p.Q && p.D >= 32 && p.D % 32 == 0 && p.D <= 2048 &&
                 p.ldc >= p.D && p.k >= 1 && p.k <= HZ_SEARCH_MAX_K))
    return;
  const long row0 = (long)tile * T;
  const int rows = (int)min((long)T, (long)p.N - row0);
  const int nq = min(QB, p.Q - q0);
  stage_live_words(p.live, p.live_bytes, p.N, row0, rows, lv);
  __syncthreads();

  const int lr = lane & 15, lh = lane >> 4;
  unsigned gm[4], any = 0u;  // the live bits of this wave's four groups (wave-uniform)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int g = w * 4 + j;
    gm[j] = (__builtin_amdgcn_readfirstlane(lv[g >> 1]) >> ((g & 1) * 16)) & 0xffffu;
    any |= gm[j];
  }
  f32x4 acc[4][4];  // [query group][row group]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  if (any != 0u) {
    const float* arow[4];
    const bf16_t* brow[4];
    bool aok[4], gok[4], bok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int q = i * 16 + lr;
      gok[i] = i * 16 < nq;  // wave-uniform: the group holds a query
      aok[i] = q < nq && HZ_DCHECK(q0 + q < p.Q);
      arow[i] = p.queries + (long)(aok[i] ? q0 + q : 0) * p.D + lh * 8;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = w * 64 + j * 16 + lr;
      bok[j] = gm[j] != 0u && r < rows && HZ_DCHECK(row0 + r < (long)p.N);
      brow[j] = p.corpus + (row0 + (bok[j] ? r : 0)) * p.ldc + lh * 8;
    }
    const int nk = p.D >> 5;
    f32x4 a[2][4][2];  // [buffer][query group][half of the 8 columns]
    bf16x8 b[2][4];    // [buffer][row group]
    auto load = [&](int buf, int kk) {  // the k-step kk < nk (columns under D: kk*32 + lh*8 + 8 <= D)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        a[buf][i][0] = a[buf][i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
        b[buf][i] = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
        if (aok[i]) {
          a[buf][i][0] = *reinterpret_cast<const f32x4*>(arow[i] + kk * 32);
          a[buf][i][1] = *reinterpret_cast<const f32x4*>(arow[i] + kk * 32 + 4);
        }
        if (bok[i]) b[buf][i] = *reinterpret_cast<const bf16x8*>(brow[i] + kk * 32);
      }
    };
    auto mma = [&](int buf) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (gok[i]) {
          bf16x8 fh, fm, fl;
          split_frag(a[buf][i][0], a[buf][i][1], fh, fm, fl);
#pragma unroll
          for (int j = 0; j < 4; ++j)  // the contract's order for every accumulator: l, then m, then h
            if (gm[j] != 0u) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fl, b[buf][j], acc[i][j], 0, 0, 0);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (gm[j] != 0u) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fm, b[buf][j], acc[i][j], 0, 0, 0);
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (gm[j] != 0u) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fh, b[buf][j], acc[i][j], 0, 0, 0);
        }
    };
    load(0, 0);
    for (int kk = 0; kk < nk; kk += 2) {  // two steps per trip, so the buffer index is a constant
      if (kk + 1 < nk) load(1, kk + 1);
      mma(0);
      if (kk + 2 < nk) load(0, kk + 2);
      if (kk + 1 < nk) mma(1);
    }
  }
  // lane holds score(query i*16 + lh*4 + e, row w*64 + j*16 + lr) in acc[i][j][e]
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int q = i * 16 + lh * 4 + e;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int r = w * 64 + j * 16 + lr;
        const bool pass = ((gm[j] >> lr) & 1u) && q < nq;
        sc[q * MSCAN_TS + r] = pass ? orderable(acc[i][j][e]) : 0u;
      }
    }
  __syncthreads();

  mscan_select(sc, pool, p.cand, p.cand_bytes, p.Q, p.k, tile, q0, nq, row0, w, lane);
}

// ------------------------------------------------------------------------- nearest centroid, means
// search_assign_kernel (HZ_K_SEARCH_ASSIGN): the self scan with the roles turned. Workgroup `tile`
// scores its T rows against all C centroids, CB at a time: the A operand is the centroid block (every workgroup
// re-reads the same C rows, which stay in L2; nothing is staged), the B operand the tile's rows. Wave w owns rows
// w*64 .. w*64+63 as four groups of 16; the fragment map, the k-step pairs and their two-pairs-ahead schedule are
// search_mscan_kernel's, so acc = mfma_f32_16x16x32_bf16(centroid fragment, row fragment, acc) over the columns
// 32s .. 32s+31, s ascending, from +0, are that kernel's bits for the same two D-vectors (CONTRACT, hipzap.h).
// A group of 16 centroids from C on is not multiplied (a scalar branch); a centroid from C on inside a mixed group
// loads zeros and is left out of the selection.
// Selection: after a block lane (lr, lh) holds score(c0 + i*16 + lh*4 + e, row j*16 + lr) in acc[i][j][e]; it folds
// the 16 keys (orderable(score) << 32) | ~c of each row group into the group's running key, 4 keys a lane. After
// the last block the four lanes lh = 0..3 of a row are reduced with two xor shuffles and lane lh == 0 writes.
// Which rows: as in the self scan (live words staged with the bits from N on cleared; a group with no bit set is
// neither loaded nor multiplied; a dead row of a mixed group is loaded, its column dropped). Every row < N of the
// tile is written: a row without its bit gets -1 / -inf.
// Addresses: cent[c*ldk + ..] under c < C; the tile's rows under row < N; live words [row0/32, row0/32 + 8) under
// word*32 < N (the launcher checks live_bytes); out_list / out_score [row0 + r] under row0 + r < N.
constexpr int CB = HZ_SEARCH_ASSIGN_CB;
static_assert(CB == 64 && T == 256, "the fragment map below");

__global__ __launch_bounds__(T) void search_assign_kernel(const HzSearchAssignParams p) {
  __shared__ unsigned lv[T / 32];
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int tile = blockIdx.x;
  if (!HZ_DCHECK(tile < p.ntile && (long)tile * T < (long)p.N && p.D >= 32 && p.D % 32 == 0 && p.D <= 2048 && p.ldc >= p.D &&
                 p.ldk >= p.D && p.C >= 1 && p.C <= HZ_SEARCH_ASSIGN_MAX_C))
    return;
  const long row0 = (long)tile * T;
  const int rows = (int)min((long)T, (long)p.N - row0);
  if (t < T / 32) {
    const long word = (row0 >> 5) + t;
    unsigned v = 0u;
    if (word * 32 < (long)p.N && HZ_DCHECK((word + 1) * 4 <= (long)p.live_bytes)) v = p.live[word];
    const int left = rows - t * 32;  // the tile's rows from this word on
    if (left < 32) v &= left <= 0 ? 0u : (1u << left) - 1u;
    lv[t] = v;
  }
  __syncthreads();

  const int lr = lane & 15, lh = lane >> 4;
  unsigned gm[4], any = 0u;  // the bits of this wave's four row groups (wave-uniform)
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int g = w * 4 + j;
    gm[j] = (__builtin_amdgcn_readfirstlane(lv[g >> 1]) >> ((g & 1) * 16)) & 0xffffu;
    any |= gm[j];
  }
  unsigned long long best[4] = {0ull, 0ull, 0ull, 0ull};  // per row group: this lane's best key so far
  if (any != 0u) {
    const bf16_t* brow[4];
    bool bok[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = w * 64 + j * 16 + lr;
      bok[j] = gm[j] != 0u && r < rows && HZ_DCHECK(row0 + r < (long)p.N);
      brow[j] = p.corpus + (row0 + (bok[j] ? r : 0)) * p.ldc + lh * 8;
    }
    const int nk = p.D >> 5;
    for (int c0 = 0; c0 < p.C; c0 += CB) {  // block-uniform
      const bf16_t* arow[4];
      bool aok[4], gok[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int c = c0 + i * 16 + lr;
        gok[i] = c0 + i * 16 < p.C;  // wave-uniform: the group holds a centroid
        aok[i] = c < p.C && HZ_DCHECK(c >= 0 && c < p.C);
        arow[i] = p.cent + (long)(aok[i] ? c : 0) * p.ldk + lh * 8;
      }
      f32x4 acc[4][4];  // [centroid group][row group]
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
      bf16x8 a[2][2][4], b[2][2][4];  // [buffer][k-step of the pair][group]
      auto load = [&](int buf, int kk) {  // the k-steps kk and kk + 1 (columns under D: kk*32 + lh*8 + 8 <= D)
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            a[buf][s][i] = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
            b[buf][s][i] = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
            if (kk + s < nk) {
              if (aok[i]) a[buf][s][i] = *reinterpret_cast<const bf16x8*>(arow[i] + (kk + s) * 32);
              if (bok[i]) b[buf][s][i] = *reinterpret_cast<const bf16x8*>(brow[i] + (kk + s) * 32);
            }
          }
      };
      auto mma = [&](int buf, int kk) {
#pragma unroll
        for (int s = 0; s < 2; ++s)
          if (kk + s < nk) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
              if (gm[j] != 0u) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                  if (gok[i])
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[buf][s][i], b[buf][s][j], acc[i][j], 0, 0, 0);
              }
          }
      };
      load(0, 0);
      for (int kk = 0; kk < nk; kk += 4) {  // two pairs per trip, so the buffer index is a constant
        if (kk + 2 < nk) load(1, kk + 2);
        mma(0, kk);
        if (kk + 4 < nk) load(0, kk + 4);
        if (kk + 2 < nk) mma(1, kk + 2);
      }
      // lane holds score(c0 + i*16 + lh*4 + e, row w*64 + j*16 + lr) in acc[i][j][e]
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int c = c0 + i * 16 + lh * 4 + e;
          if (c < p.C) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const unsigned long long key = ((unsigned long long)orderable(acc[i][j][e]) << 32) | (unsigned)~(unsigned)c;
              best[j] = key > best[j] ? key : best[j];
            }
          }
        }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    unsigned long long k = best[j];
    const unsigned long long k1 = __shfl_xor(k, 16);
    k = k1 > k ? k1 : k;
    const unsigned long long k2 = __shfl_xor(k, 32);
    k = k2 > k ? k2 : k;
    const int r = w * 64 + j * 16 + lr;
    if (lh == 0 && r < rows && HZ_DCHECK(row0 + r < (long)p.N)) {
      const bool pass = ((gm[j] >> lr) & 1u) != 0u && k != 0ull;
      p.out_list[row0 + r] = pass ? (int)~(unsigned)k : -1;
      p.out_score[row0 + r] = pass ? unorderable((unsigned)(k >> 32)) : -__builtin_inff();
    }
  }
}

// search_cmean_kernel (HZ_K_SEARCH_CMEAN): workgroup c, the mean of the rows order[seg_off[c] ..
// seg_off[c + 1]). SUMMATION ORDER (hipzap.h): nch = D / 8 chunks of 8 columns, G = 256 / nch member lanes; thread
// (g, chunk) adds the members at positions g, g + G, ... in that order (four loads in flight, added in position
// order), the G partials of a column are added in g order, then one division by the count.
// Addresses: seg_off[c], seg_off[c + 1] under c < C; order[i] under lo <= i < hi with 0 <= lo <= hi <= M;
// corpus[id*ldc + ..] under (unsigned)id < N; cent / cent32 [c][d] under c < C and d < D.
constexpr int CMEAN_THREADS = 256;
constexpr int CMEAN_UNROLL = 4;

__global__ __launch_bounds__(CMEAN_THREADS) void search_cmean_kernel(const HzSearchCmeanParams p) {
  __shared__ float part[CMEAN_THREADS * 8];  // [G][D]: G * D = (256 / nch) * nch * 8 <= 2048
  __shared__ float wsum[4];
  const int t = threadIdx.x, c = blockIdx.x;
  if (!HZ_DCHECK(c < p.C && p.D >= 32 && p.D % 32 == 0 && p.D <= 2048 && p.ldc >= p.D && p.ldk >= p.D)) return;
  const int lo = p.seg_off[c], hi = p.seg_off[c + 1];
  if (lo < 0 || hi < lo || hi > p.M) return;  // block-uniform: not a segment of `order`
  const int m = hi - lo;
  int count = 0;  // the members inside [0, N)
  for (int base = 0; base < m; base += CMEAN_THREADS) {
    const int i = base + t;
    count += __syncthreads_count(i < m && (unsigned)p.order[lo + i] < (unsigned)p.N);
  }
  if (count == 0) return;  // block-uniform
  const int nch = p.D >> 3, G = CMEAN_THREADS / nch;
  const int g = t / nch, chunk = t - g * nch;
  if (g < G) {
    float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int i = g; i < m; i += G * CMEAN_UNROLL) {
      u32x4 v[CMEAN_UNROLL];
      bool ok[CMEAN_UNROLL];
#pragma unroll
      for (int u = 0; u < CMEAN_UNROLL; ++u) {
        const int at = i + u * G;
        int id = -1;
        if (at < m && HZ_DCHECK(lo + at < p.M)) id = p.order[lo + at];
        ok[u] = (unsigned)id < (unsigned)p.N;
        v[u] = u32x4{0u, 0u, 0u, 0u};
        if (ok[u]) v[u] = *reinterpret_cast<const u32x4*>(p.corpus + (long)id * p.ldc + chunk * 8);
      }
#pragma unroll
      for (int u = 0; u < CMEAN_UNROLL; ++u)
        if (ok[u]) {
          float f[8];
          unpack8(v[u], f);
#pragma unroll
          for (int e = 0; e < 8; ++e) s[e] += f[e];
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) part[g * p.D + chunk * 8 + e] = s[e];
  }
  __syncthreads();
  float mean[8];  // columns t, t + 256, ...
  float ss = 0.f;
  const float n = (float)count;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int d = t + u * CMEAN_THREADS;
    mean[u] = 0.f;
    if (d < p.D) {
      float v = part[d];
      for (int gg = 1; gg < G; ++gg) v += part[gg * p.D + d];
      mean[u] = v / n;
      ss += mean[u] * mean[u];
    }
  }
  float inv = 1.f;
  if (p.cosine) {  // block-uniform
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) ss += __shfl_xor(ss, o);
    if ((t & 63) == 0) wsum[t >> 6] = ss;
    __syncthreads();
    const float tot = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    inv = fmaxf(sqrtf(tot), 1e-12f);
  }
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int d = t + u * CMEAN_THREADS;
    if (d < p.D && HZ_DCHECK(c < p.C)) {
      const float v = p.cosine ? mean[u] / inv : mean[u];
      if (p.cent32) p.cent32[(long)c * p.D + d] = v;
      p.cent[(long)c * p.ldk + d] = f2bf(v);
    }
  }
}

// one refusal list for both launchers: the kernels then have no address that the data can move out of
// its buffer. Fills ntile. `need`: the bytes `cand` must hold, 0 for the scan's hz_search_scratch_bytes(N, Q, k).
int search_check(HzSearchParams& p, unsigned long long need = 0) {
  if (!p.corpus || !p.queries || !p.cand || !p.out_score || !p.out_id) return -1;
  if (p.D < 8 || p.D % 8 || p.D > 2048 || p.ldc < p.D || p.ldc % 8) return -2;
  if (p.N < 1) return -3;  // N is an int: N >= 2^31 cannot be expressed (hz_search_scratch_bytes refuses it)
  if (p.Q < 1 || p.Q > HZ_SEARCH_MAX_Q) return -4;
  if (p.k < 1 || p.k > HZ_SEARCH_MAX_K) return -5;
  if ((reinterpret_cast<uintptr_t>(p.corpus) & 15) || (reinterpret_cast<uintptr_t>(p.queries) & 15) ||
      (reinterpret_cast<uintptr_t>(p.cand) & 7) || (reinterpret_cast<uintptr_t>(p.out_score) & 3) ||
      (reinterpret_cast<uintptr_t>(p.out_id) & 3))
    return -6;
  if (!need) need = hz_search_scratch_bytes(p.N, p.Q, p.k);
  if (!need || p.cand_bytes < need) return -7;
  p.ntile = (int)(((long)p.N + T - 1) / T);
  return 0;
}

// the filtered kinds' refusals, after search_check's
int filter_check(const HzSearchFilterParams& f) {
  if (!f.live || (reinterpret_cast<uintptr_t>(f.live) & 3)) return -12;
  if (f.live_bytes < 4ull * (((unsigned long long)f.s.N + 31) / 32)) return -13;
  if (f.filt && !f.tags) return -14;
  if ((reinterpret_cast<uintptr_t>(f.tags) & 3) || (reinterpret_cast<uintptr_t>(f.filt) & 3)) return -15;
  return 0;
}

// dynamic LDS above 64 KiB is allowed per kernel and device: once, outside any capture (an index does it
// at open through hz_search_code_warm; a direct launch here). Every instantiation scan_dispatch can reach.
template <class Fmt, bool FILT, int NC = 1>
int raise_lds_limit_of() {
  HZ_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&search_scan_kernel<Fmt, NC, FILT>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  if constexpr (NC < Fmt::MAX_NC) return raise_lds_limit_of<Fmt, FILT, NC + 1>();
  return 0;
}
int raise_lds_limit() {
  static bool done[64];
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return -8;
  if (done[d]) return 0;
  if (const int rc = raise_lds_limit_of<Bf16Rows, false>()) return rc;
  if (const int rc = raise_lds_limit_of<Bf16Rows, true>()) return rc;
  if (const int rc = raise_lds_limit_of<E4m3Rows, true>()) return rc;
  done[d] = true;
  return 0;
}

// the instantiation with the fewest chunks per lane that covers D
template <class Fmt, bool FILT, int NC = 1>
void scan_dispatch(const typename Fmt::template Args<FILT>& a, const HzSearchParams& p, hipStream_t st) {
  if constexpr (NC < Fmt::MAX_NC) {
    if (p.D > NC * 64 * Fmt::E) return scan_dispatch<Fmt, FILT, NC + 1>(a, p, st);
  }
  hipLaunchKernelGGL((search_scan_kernel<Fmt, NC, FILT>), dim3(p.ntile), dim3(T),
                     lds_bytes(p.Q, p.D, FILT, Fmt::SCALED), st, a);
}

// a checked parameter block (ntile filled) -> the launch
template <class Fmt, bool FILT>
int scan_launch(const typename Fmt::template Args<FILT>& a, hipStream_t st) {
  if (const int rc = raise_lds_limit()) return rc;
  scan_dispatch<Fmt, FILT>(a, scan_part(a), st);
  return (int)hipGetLastError();
}

}  // namespace

extern "C" int hz_search_tile_rows(void) { return T; }

extern "C" unsigned long long hz_search_scratch_bytes(long long N, int Q, int k) {
  if (N < 1 || N >= (1ll << 31) || Q < 1 || Q > HZ_SEARCH_MAX_Q || k < 1 || k > HZ_SEARCH_MAX_K) return 0;
  return (unsigned long long)((N + T - 1) / T) * Q * k * 8ull;
}

extern "C" int hz_search_scan_launch(const HzSearchParams* pp, hipStream_t st) {
  HzSearchParams p = *pp;
  if (const int rc = search_check(p)) return rc;
  return scan_launch<Bf16Rows, false>(p, st);
}

extern "C" int hz_search_fscan_launch(const HzSearchFilterParams* pp, hipStream_t st) {
  HzSearchFilterParams f = *pp;
  if (const int rc = search_check(f.s)) return rc;
  if (const int rc = filter_check(f)) return rc;
  return scan_launch<Bf16Rows, true>(f, st);
}

// The filtered launcher's refusals with the byte rows' dimension rules: -16 D % 16, -17 D < 16, -18 D > 2048,
// -19 ldc < D, -23 ldc % 16 (ldc in bytes), -24 scales null, -25 scales not 4-byte aligned.
extern "C" int hz_search_qscan_launch(const HzSearchQuantParams* pp, hipStream_t st) {
  HzSearchQuantParams qp = *pp;
  HzSearchParams& p = qp.f.s;
  if (p.D < 16) return -17;
  if (p.D % 16) return -16;
  if (p.D > 2048) return -18;
  if (p.ldc < p.D) return -19;
  if (p.ldc % 16) return -23;
  if (const int rc = search_check(p)) return rc;
  if (const int rc = filter_check(qp.f)) return rc;
  if (!qp.scales) return -24;
  if (reinterpret_cast<uintptr_t>(qp.scales) & 3) return -25;
  return scan_launch<E4m3Rows, true>(qp, st);
}

// The binary scan's own refusal list (hipzap.h): -80 .. -92. Buckets of 16-B chunks per thread: W <= 8, 24, 32, 64.
extern "C" int hz_search_bscan_launch(const HzSearchBinParams* pp, hipStream_t st) {
  if (!pp) return -80;
  HzSearchBinParams a = *pp;
  HzSearchFilterParams& f = a.f;
  HzSearchParams& p = f.s;
  if (!p.corpus || !p.queries || !p.cand || !p.out_score || !p.out_id) return -80;
  if (p.D % 128) return -81;
  if (p.D < 128) return -82;
  if (p.D > 2048) return -83;
  const int W = p.D / 32;
  if (p.ldc < W || p.ldc % 4) return -84;
  if (p.N < 1) return -85;
  if (p.Q < 1 || p.Q > HZ_SEARCH_MAX_Q) return -86;
  if (p.k < 1 || p.k > HZ_SEARCH_MAX_K) return -87;
  if ((reinterpret_cast<uintptr_t>(p.corpus) & 15) || (reinterpret_cast<uintptr_t>(p.queries) & 15) ||
      (reinterpret_cast<uintptr_t>(p.cand) & 7) || (reinterpret_cast<uintptr_t>(p.out_score) & 3) ||
      (reinterpret_cast<uintptr_t>(p.out_id) & 3) || (reinterpret_cast<uintptr_t>(f.live) & 3) ||
      (reinterpret_cast<uintptr_t>(f.tags) & 3) || (reinterpret_cast<uintptr_t>(f.filt) & 3))
    return -88;
  if (!f.live) return -89;
  if (f.live_bytes < 4ull * (((unsigned long long)p.N + 31) / 32)) return -90;
  if (f.filt && !f.tags) return -91;
  const unsigned long long need = hz_search_scratch_bytes(p.N, p.Q, p.k);
  if (!need || p.cand_bytes < need) return -92;
  p.ntile = (int)(((long)p.N + T - 1) / T);
  const dim3 grid(p.ntile), block(T);
  if (W <= 8) hipLaunchKernelGGL(search_bscan_kernel<2>, grid, block, 0, st, a);
  else if (W <= 24) hipLaunchKernelGGL(search_bscan_kernel<6>, grid, block, 0, st, a);
  else if (W <= 32) hipLaunchKernelGGL(search_bscan_kernel<8>, grid, block, 0, st, a);
  else hipLaunchKernelGGL(search_bscan_kernel<16>, grid, block, 0, st, a);
  return (int)hipGetLastError();
}

namespace {

// the shape rules of product-quantised rows (hipzap.h): -114 M % 16, -115 M outside 16..96, -113 D % M,
// -116 D / M outside 1..64, -117 D > 2048
int pq_shape_check(int D, int M) {
  if (M % 16) return -114;
  if (M < 16 || M > HZ_SEARCH_PQ_MAX_M) return -115;
  if (D < 1 || D % M) return -113;
  if (D / M > HZ_SEARCH_PQ_MAX_DSUB) return -116;
  if (D > 2048) return -117;
  return 0;
}

template <int NCH>
int raise_pq_lds_limit_of() {
  HZ_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&search_pqscan_kernel<NCH>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, HZ_SEARCH_PQ_MAX_M * 1024));
  if constexpr (NCH < HZ_SEARCH_PQ_MAX_M / 16) return raise_pq_lds_limit_of<NCH + 1>();
  return 0;
}

// The table of M = 80 or 96 is above 64 KiB of dynamic LDS: allowed once per device, outside any capture, where the
// device's compute units are counted too (hz_search_code_warm at an index's open; a direct launch here).
int pq_cus[64];
int pq_device_setup(int* cus) {
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return -8;
  if (!pq_cus[d]) {
    int n = 0;
    if (const int rc = raise_pq_lds_limit_of<1>()) return rc;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, d) != hipSuccess || n < 1) return -8;
    pq_cus[d] = n;
  }
  if (cus) *cus = pq_cus[d];
  return 0;
}

// Tiles per workgroup. M >= 80: the table lets ONE workgroup live on a compute unit, so nothing hides its copy of
// the table (M KiB) but the tiles that follow it: the span that leaves about two workgroups per compute unit over the
// grid (ceil(ntile / span), Q). M <= 64: two or more workgroups share a compute unit, one's copy runs under another's
// lookups, and more, shorter workgroups balance better: that span, but at most max(2, M / 16) (the sweep over spans in
// DESIGN.md 4w / profiles/search_pq/span.json). A score's bits do not depend on the choice.
int pq_auto_span(long ntile, int Q, int cus, int M) {
  long span = (ntile * Q + 2l * cus - 1) / (2l * cus);
  if (M < 80) span = min(span, (long)max(2, M / 16));
  return (int)max(1l, min(span, ntile));
}

template <int NCH = 1>
void pqscan_dispatch(const HzSearchPqParams& a, const dim3 grid, hipStream_t st) {
  if constexpr (NCH < HZ_SEARCH_PQ_MAX_M / 16) {
    if (a.M > NCH * 16) return pqscan_dispatch<NCH + 1>(a, grid, st);
  }
  hipLaunchKernelGGL(search_pqscan_kernel<NCH>, grid, dim3(T), (size_t)a.M * 1024, st, a);
}

}  // namespace

extern "C" int hz_search_pq_span(long long N, int Q, int M) {
  if (N < 1 || N >= (1ll << 31) || Q < 1 || Q > HZ_SEARCH_MAX_Q || M < 16 || M > HZ_SEARCH_PQ_MAX_M || M % 16) return 0;
  int cus = 0;
  if (pq_device_setup(&cus)) return 0;
  return pq_auto_span((long)((N + T - 1) / T), Q, cus, M);
}

// The product-quantised kinds' refusal list (hipzap.h): -112 .. -128.
extern "C" int hz_search_pqlut_launch(const HzSearchPqLutParams* pp, hipStream_t st) {
  if (!pp) return -112;
  const HzSearchPqLutParams a = *pp;
  if (!a.queries || !a.codebook || !a.lut) return -112;
  if (const int rc = pq_shape_check(a.D, a.M)) return rc;
  if (a.Q < 1 || a.Q > HZ_SEARCH_MAX_Q) return -120;
  if ((reinterpret_cast<uintptr_t>(a.queries) & 15) || (reinterpret_cast<uintptr_t>(a.codebook) & 15) ||
      (reinterpret_cast<uintptr_t>(a.lut) & 15))
    return -122;
  if (a.lut_bytes < (unsigned long long)a.Q * a.M * 1024ull) return -127;
  hipLaunchKernelGGL(search_pqlut_kernel, dim3(a.M, a.Q), dim3(PQ_KSUB), 0, st, a);
  return (int)hipGetLastError();
}

extern "C" int hz_search_pqscan_launch(const HzSearchPqParams* pp, hipStream_t st) {
  if (!pp) return -112;
  HzSearchPqParams a = *pp;
  HzSearchFilterParams& f = a.f;
  HzSearchParams& p = f.s;
  if (!p.corpus || !p.queries || !p.cand || !p.out_score || !p.out_id || !a.lut) return -112;
  if (const int rc = pq_shape_check(p.D, a.M)) return rc;
  if (p.ldc < a.M || p.ldc % 16) return -118;
  if (p.N < 1) return -119;
  if (p.Q < 1 || p.Q > HZ_SEARCH_MAX_Q) return -120;
  if (p.k < 1 || p.k > HZ_SEARCH_MAX_K) return -121;
  if ((reinterpret_cast<uintptr_t>(p.corpus) & 15) || (reinterpret_cast<uintptr_t>(p.queries) & 15) ||
      (reinterpret_cast<uintptr_t>(a.lut) & 15) || (reinterpret_cast<uintptr_t>(p.cand) & 7) ||
      (reinterpret_cast<uintptr_t>(p.out_score) & 3) || (reinterpret_cast<uintptr_t>(p.out_id) & 3) ||
      (reinterpret_cast<uintptr_t>(f.live) & 3) || (reinterpret_cast<uintptr_t>(f.tags) & 3) ||
      (reinterpret_cast<uintptr_t>(f.filt) & 3))
    return -122;
  if (!f.live) return -123;
  if (f.live_bytes < 4ull * (((unsigned long long)p.N + 31) / 32)) return -124;
  if (f.filt && !f.tags) return -125;
  const unsigned long long need = hz_search_scratch_bytes(p.N, p.Q, p.k);
  if (!need || p.cand_bytes < need) return -126;
  if (a.lut_bytes < (unsigned long long)p.Q * a.M * 1024ull) return -127;
  if (a.span < 0) return -128;
  p.ntile = (int)(((long)p.N + T - 1) / T);
  int cus = 0;
  if (const int rc = pq_device_setup(&cus)) return rc;
  if (a.span == 0) a.span = pq_auto_span(p.ntile, p.Q, cus, a.M);
  if (a.span > p.ntile) a.span = p.ntile;
  pqscan_dispatch(a, dim3((p.ntile + a.span - 1) / a.span, p.Q), st);
  return (int)hipGetLastError();
}

namespace {

template <int NQ = 1>
void pqassign_dispatch(const HzSearchPqAssignParams& a, const int nq, const dim3 grid, hipStream_t st) {
  if constexpr (NQ < HZ_SEARCH_PQ_MAX_DSUB / 4) {
    if (nq > NQ) return pqassign_dispatch<NQ + 1>(a, nq, grid, st);
  }
  hipLaunchKernelGGL(search_pqassign_kernel<NQ>, grid, dim3(T), (size_t)NQ * 4 * PQ_KSUB * sizeof(float), st, a);
}

}  // namespace

// The assign kind's refusal list (hipzap.h): -129 .. -139. At most 64 KiB of dynamic LDS: no attribute to raise.
extern "C" int hz_search_pqassign_launch(const HzSearchPqAssignParams* pp, hipStream_t st) {
  if (!pp) return -129;
  const HzSearchPqAssignParams a = *pp;
  if (!a.rows || !a.codebook || !a.codes) return -129;
  if (a.M < 1) return -132;  // before the division
  if (a.D % a.M) return -130;
  if (a.M % 16) return -131;
  if (a.M < 16 || a.M > HZ_SEARCH_PQ_MAX_M) return -132;
  if (a.D / a.M < 1 || a.D / a.M > HZ_SEARCH_PQ_MAX_DSUB) return -133;
  if (a.D > 2048) return -134;
  if (a.ldr < a.D || a.ldr % 8) return -135;
  if (a.ldc < a.M || a.ldc % 16) return -136;
  if (a.N < 1) return -137;
  if ((reinterpret_cast<uintptr_t>(a.rows) & 15) || (reinterpret_cast<uintptr_t>(a.codebook) & 15) ||
      (reinterpret_cast<uintptr_t>(a.codes) & 15) || (reinterpret_cast<uintptr_t>(a.dist) & 15))
    return -138;
  if (a.dist && a.dist_bytes < (unsigned long long)a.N * a.M * 4ull) return -139;
  const int dsub = a.D / a.M;
  pqassign_dispatch(a, (dsub + 3) / 4, dim3((unsigned)((a.N + T - 1) / T), a.M / 16), st);
  return (int)hipGetLastError();
}

namespace {

template <class Fmt, int NC = 1>
void lscan_dispatch(const ListArgs<Fmt>& args, hipStream_t st) {
  const HzSearchListParams& a = list_part(args);
  const HzSearchParams& p = a.f.s;
  if constexpr (NC < Fmt::MAX_NC) {
    if (p.D > NC * 64 * Fmt::E) return lscan_dispatch<Fmt, NC + 1>(args, st);
  }
  hipLaunchKernelGGL((search_lscan_kernel<Fmt, NC>), dim3(a.P, p.Q), dim3(T), lds_bytes(1, p.D, true, Fmt::SCALED), st, args);
}

// The filtered launcher's refusals (-7: cand_bytes below P*Q*k*8), then the list tables' (hipzap.h). Fills ntile.
int list_check(HzSearchListParams& a) {
  HzSearchParams& p = a.f.s;
  if (a.P < 1 || (long long)a.P * T >= (1ll << 31)) return -42;
  const unsigned long long need =
      (p.Q >= 1 && p.Q <= HZ_SEARCH_MAX_Q && p.k >= 1 && p.k <= HZ_SEARCH_MAX_K) ? (unsigned long long)a.P * p.Q * p.k * 8ull : 0;
  if (const int rc = search_check(p, need ? need : 1)) return rc;  // Q or k out of range: refused before -7
  if (const int rc = filter_check(a.f)) return rc;
  if (a.nlist < 1) return -40;
  if (a.probes && (a.nprobe < 1 || a.nprobe > a.nlist || a.nprobe > HZ_SEARCH_MAX_K)) return -41;
  if (p.N % T) return -43;
  if (!a.probes && a.P != p.ntile) return -42;
  if (!a.list_off || !a.list_tiles || !a.rowid) return -44;
  if ((reinterpret_cast<uintptr_t>(a.probes) & 3) || (reinterpret_cast<uintptr_t>(a.list_off) & 3) ||
      (reinterpret_cast<uintptr_t>(a.list_tiles) & 3) || (reinterpret_cast<uintptr_t>(a.rowid) & 3))
    return -45;
  return 0;
}

}  // namespace

extern "C" int hz_search_lscan_launch(const HzSearchListParams* pp, hipStream_t st) {
  HzSearchListParams a = *pp;
  if (const int rc = list_check(a)) return rc;
  lscan_dispatch<Bf16Rows>(a, st);
  return (int)hipGetLastError();
}

// The byte rows' dimension rules of the quantised launcher (-16 .. -19, -23), the list launcher's refusals, then
// -24 scales null, -25 scales not 4-byte aligned.
extern "C" int hz_search_qlscan_launch(const HzSearchQuantListParams* pp, hipStream_t st) {
  HzSearchQuantListParams qa = *pp;
  const HzSearchParams& p = qa.l.f.s;
  if (p.D < 16) return -17;
  if (p.D % 16) return -16;
  if (p.D > 2048) return -18;
  if (p.ldc < p.D) return -19;
  if (p.ldc % 16) return -23;
  if (const int rc = list_check(qa.l)) return rc;
  if (!qa.scales) return -24;
  if (reinterpret_cast<uintptr_t>(qa.scales) & 3) return -25;
  lscan_dispatch<E4m3Rows>(qa, st);
  return (int)hipGetLastError();
}

extern "C" int hz_search_merge_launch(const HzSearchParams* pp, hipStream_t st) {
  HzSearchParams p = *pp;
  if (const int rc = search_check(p)) return rc;
  hipLaunchKernelGGL(search_merge_kernel, dim3(p.Q), dim3(MERGE_THREADS), 0, st, p);
  return (int)hipGetLastError();
}

// The scan's D / ldc (-2), N (-3) and Q (-4: outside 1..max_q) rules; then -30 R outside 1..HZ_SEARCH_MAX_K, -31 k
// outside 1..R, -32 a null pointer, -33 rows or queries not 16-B aligned or in_id / out_* not 4-B aligned.
static int rescore_check(const HzSearchRescoreParams& a, int max_q) {
  if (a.D < 8 || a.D % 8 || a.D > 2048 || a.ldc < a.D || a.ldc % 8) return -2;
  if (a.N < 1) return -3;
  if (a.Q < 1 || a.Q > max_q) return -4;
  if (a.R < 1 || a.R > HZ_SEARCH_MAX_K) return -30;
  if (a.k < 1 || a.k > a.R) return -31;
  if (!a.rows || !a.queries || !a.in_id || !a.out_score || !a.out_id) return -32;
  if ((reinterpret_cast<uintptr_t>(a.rows) & 15) || (reinterpret_cast<uintptr_t>(a.queries) & 15) ||
      (reinterpret_cast<uintptr_t>(a.in_id) & 3) || (reinterpret_cast<uintptr_t>(a.out_score) & 3) ||
      (reinterpret_cast<uintptr_t>(a.out_id) & 3))
    return -33;
  return 0;
}

extern "C" int hz_search_rescore_launch(const HzSearchRescoreParams* pp, hipStream_t st) {
  const HzSearchRescoreParams a = *pp;
  if (const int rc = rescore_check(a, HZ_SEARCH_MAX_Q)) return rc;
  rescore_dispatch(a, st);
  return (int)hipGetLastError();
}

// search_rescore_kernel as it stands (one workgroup per query; its body indexes by q in 64 bits and has no limit on
// Q) behind a launcher that takes Q up to the self scan's limit
extern "C" int hz_search_rescoren_launch(const HzSearchRescoreParams* pp, hipStream_t st) {
  const HzSearchRescoreParams a = *pp;
  if (const int rc = rescore_check(a, HZ_SEARCH_SELF_MAX_Q)) return rc;
  rescore_dispatch(a, st);
  return (int)hipGetLastError();
}

namespace {

// the self scan's dynamic LDS is above 64 KiB: allowed once per device, outside any capture (hz_search_code_warm
// at an index's open; a direct launch here)
int raise_mscan_lds_limit() {
  static bool done[64];
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return -8;
  if (done[d]) return 0;
  HZ_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&search_mscan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)MSCAN_LDS));
  done[d] = true;
  return 0;
}

// what the self scan and its merge both refuse: -55 N, -56 Q, -57 k, -60 cand_bytes. Fills ntile.
int self_check(HzSearchSelfParams& p) {
  if (p.N < 1) return -55;
  if (p.Q < 1 || p.Q > HZ_SEARCH_SELF_MAX_Q) return -56;
  if (p.k < 1 || p.k > HZ_SEARCH_MAX_K) return -57;
  if (p.cand_bytes < hz_search_self_scratch_bytes(p.N, p.Q, p.k)) return -60;
  p.ntile = (int)(((long)p.N + T - 1) / T);
  return 0;
}

}  // namespace

extern "C" unsigned long long hz_search_self_scratch_bytes(long long N, long long Q, int k) {
  if (N < 1 || N >= (1ll << 31) || Q < 1 || Q > HZ_SEARCH_SELF_MAX_Q || k < 1 || k > HZ_SEARCH_MAX_K) return 0;
  return (unsigned long long)((N + T - 1) / T) * (unsigned long long)Q * k * 8ull;  // < 2^23 * 2^22 * 2^7 * 2^3
}

extern "C" int hz_search_mscan_launch(const HzSearchSelfParams* pp, hipStream_t st) {
  HzSearchSelfParams p = *pp;
  if (!p.corpus || !p.qid || !p.live || !p.cand) return -50;
  if (p.D % 32) return -51;
  if (p.D < 32) return -52;
  if (p.D > 2048) return -53;
  if (p.ldc < p.D || p.ldc % 8) return -54;
  if ((reinterpret_cast<uintptr_t>(p.corpus) & 15) || (reinterpret_cast<uintptr_t>(p.cand) & 7) ||
      (reinterpret_cast<uintptr_t>(p.qid) & 3) || (reinterpret_cast<uintptr_t>(p.live) & 3))
    return -58;
  if (p.N >= 1 && p.live_bytes < 4ull * (((unsigned long long)p.N + 31) / 32)) return -59;
  if (const int rc = self_check(p)) return rc;
  if (const int rc = raise_mscan_lds_limit()) return rc;
  hipLaunchKernelGGL(search_mscan_kernel, dim3(p.ntile, (p.Q + QB - 1) / QB), dim3(T), MSCAN_LDS, st, p);
  return (int)hipGetLastError();
}

namespace {

int raise_xscan_lds_limit() {  // as raise_mscan_lds_limit
  static bool done[64];
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return -8;
  if (done[d]) return 0;
  HZ_CHECK(hipFuncSetAttribute(reinterpret_cast<const void*>(&search_xscan_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)XSCAN_LDS));
  done[d] = true;
  return 0;
}

}  // namespace

// The batch scan's refusals (hipzap.h): the self scan's -50 .. -60 as -100 .. -110, then -111 for the queries.
extern "C" int hz_search_xscan_launch(const HzSearchBatchParams* pp, hipStream_t st) {
  HzSearchBatchParams p = *pp;
  if (!p.corpus || !p.queries || !p.live || !p.cand) return -100;
  if (p.D % 32) return -101;
  if (p.D < 32) return -102;
  if (p.D > 2048) return -103;
  if (p.ldc < p.D || p.ldc % 8) return -104;
  if (p.N < 1) return -105;
  if (p.Q < 1 || p.Q > HZ_SEARCH_SELF_MAX_Q) return -106;
  if (p.k < 1 || p.k > HZ_SEARCH_MAX_K) return -107;
  if ((reinterpret_cast<uintptr_t>(p.corpus) & 15) || (reinterpret_cast<uintptr_t>(p.cand) & 7) ||
      (reinterpret_cast<uintptr_t>(p.live) & 3))
    return -108;
  if (p.live_bytes < 4ull * (((unsigned long long)p.N + 31) / 32)) return -109;
  if (p.cand_bytes < hz_search_self_scratch_bytes(p.N, p.Q, p.k)) return -110;
  if (reinterpret_cast<uintptr_t>(p.queries) & 15) return -111;
  p.ntile = (int)(((long)p.N + T - 1) / T);
  if (const int rc = raise_xscan_lds_limit()) return rc;
  hipLaunchKernelGGL(search_xscan_kernel, dim3(p.ntile, (p.Q + QB - 1) / QB), dim3(T), XSCAN_LDS, st, p);
  return (int)hipGetLastError();
}

// search_merge_kernel as it stands (its body has no limit on Q: one workgroup per query) behind the self scan's block
extern "C" int hz_search_mergen_launch(const HzSearchSelfParams* pp, hipStream_t st) {
  HzSearchSelfParams s = *pp;
  if (!s.cand || !s.out_score || !s.out_id) return -50;
  if ((reinterpret_cast<uintptr_t>(s.cand) & 7) || (reinterpret_cast<uintptr_t>(s.out_score) & 3) ||
      (reinterpret_cast<uintptr_t>(s.out_id) & 3))
    return -58;
  if (const int rc = self_check(s)) return rc;
  HzSearchParams p{};
  p.cand = s.cand, p.out_score = s.out_score, p.out_id = s.out_id;
  p.N = s.N, p.D = s.D, p.Q = s.Q, p.k = s.k, p.ldc = s.ldc, p.ntile = s.ntile, p.cand_bytes = s.cand_bytes;
  hipLaunchKernelGGL(search_merge_kernel, dim3(p.Q), dim3(MERGE_THREADS), 0, st, p);
  return (int)hipGetLastError();
}

extern "C" int hz_search_assign_launch(const HzSearchAssignParams* pp, hipStream_t st) {
  HzSearchAssignParams p = *pp;
  if (!p.corpus || !p.cent || !p.live || !p.out_list || !p.out_score) return -61;
  if (p.D % 32) return -62;
  if (p.D < 32) return -63;
  if (p.D > 2048) return -64;
  if (p.ldc < p.D || p.ldc % 8 || p.ldk < p.D || p.ldk % 8) return -65;
  if (p.N < 1) return -66;
  if (p.C < 1 || p.C > HZ_SEARCH_ASSIGN_MAX_C) return -67;
  if ((reinterpret_cast<uintptr_t>(p.corpus) & 15) || (reinterpret_cast<uintptr_t>(p.cent) & 15) ||
      (reinterpret_cast<uintptr_t>(p.live) & 3) || (reinterpret_cast<uintptr_t>(p.out_list) & 3) ||
      (reinterpret_cast<uintptr_t>(p.out_score) & 3))
    return -68;
  if (p.live_bytes < 4ull * (((unsigned long long)p.N + 31) / 32)) return -69;
  p.ntile = (int)(((long)p.N + T - 1) / T);
  hipLaunchKernelGGL(search_assign_kernel, dim3(p.ntile), dim3(T), 0, st, p);
  return (int)hipGetLastError();
}

extern "C" int hz_search_cmean_launch(const HzSearchCmeanParams* pp, hipStream_t st) {
  const HzSearchCmeanParams p = *pp;
  if (!p.corpus || !p.order || !p.seg_off || !p.cent) return -70;
  if (p.D % 32) return -71;
  if (p.D < 32) return -72;
  if (p.D > 2048) return -73;
  if (p.ldc < p.D || p.ldc % 8 || p.ldk < p.D || p.ldk % 8) return -74;
  if (p.N < 1) return -75;
  if (p.C < 1 || p.C > HZ_SEARCH_ASSIGN_MAX_C) return -76;
  if (p.M < 0) return -77;
  if ((reinterpret_cast<uintptr_t>(p.corpus) & 15) || (reinterpret_cast<uintptr_t>(p.cent) & 15) ||
      (reinterpret_cast<uintptr_t>(p.order) & 3) || (reinterpret_cast<uintptr_t>(p.seg_off) & 3) ||
      (reinterpret_cast<uintptr_t>(p.cent32) & 3))
    return -78;
  if (p.cosine != 0 && p.cosine != 1) return -79;
  hipLaunchKernelGGL(search_cmean_kernel, dim3(p.C), dim3(CMEAN_THREADS), 0, st, p);
  return (int)hipGetLastError();
}

// Load this translation unit's device code without a launch (see hz_conv_code_warm in conv.hip).
__global__ void hz_search_code_warm_kernel() {}
extern "C" int hz_search_code_warm(void) {
  hipFuncAttributes a;
  if (const int rc = (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&hz_search_code_warm_kernel))) return rc;
  if (const int rc = raise_lds_limit()) return rc;
  if (const int rc = raise_mscan_lds_limit()) return rc;
  if (const int rc = raise_xscan_lds_limit()) return rc;
  return pq_device_setup(nullptr);
}
