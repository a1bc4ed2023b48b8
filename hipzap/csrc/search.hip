// hipzap vector search for gfx950 (CDNA4): exact top-k by inner product over a bf16 corpus.
//   * search_scan  — one workgroup per tile of HZ_SEARCH_TILE rows: every row is read once and scored
//                    against all Q queries of the launch (resident in LDS); the tile's best k per query
//   * search_fscan — the scan over the rows that pass a live bit and a per-query tag predicate
//   * search_qscan — the filtered scan over OCP e4m3fn byte rows with one fp32 scale per row
//   * search_merge — one workgroup per query: ntile x k candidates -> the final k, best first
// See HzSearchParams (hipzap.h) for the order rule and DESIGN.md 4l / 4m / 4n for the reasoning.
#include <stdio.h>

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
// Wave w of the workgroup owns rows w*64 .. w*64+63 of the tile, ROWS at a time. Lane l holds the 16-B
// chunks l, l + 64, ... of a row (NC of them, sized to D at launch). score(q, r): every lane runs ONE
// fmaf chain over its elements in ascending column order starting from +0 (a lane past the row's end keeps
// +0), then the 64 lane sums meet in a xor butterfly (32, 16, ..., 1). Both orders are fixed by D alone,
// so the bits of a score depend on the query's and the row's D values and on nothing else: not on the
// row's position, its tile, N, Q, k or the other queries. Each (row, query) score lands in LDS as an
// order-preserving u32; thread t then ranks row t of the tile among the tile's rows (higher score first,
// then the lower row) and the rows ranked below k write their key to slot `rank` of the tile's list.
// Addresses: corpus rows [tile*T, min(N, tile*T + T)), the Q x D queries, and cand[(tile*Q + q)*k + s]
// with s < k -- `rank` is the one data-dependent index and is used only under `rank < k`.
template <int NC>
__global__ __launch_bounds__(T) void search_scan_kernel(const HzSearchParams p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* qs = lds;                                              // [Q][D]
  unsigned* sc = reinterpret_cast<unsigned*>(lds + p.Q * p.D);  // [Q][T]
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int tile = blockIdx.x;
  const int nch = p.D >> 3;
  if (!HZ_DCHECK(tile < p.ntile && p.D <= NC * 512 && p.ldc >= p.D && (long)tile * T < (long)p.N)) return;
  const long row0 = (long)tile * T;
  const int rows = (int)min((long)T, (long)p.N - row0);
  for (int i = threadIdx.x; i < p.Q * (p.D >> 2); i += T)
    reinterpret_cast<f32x4*>(qs)[i] = reinterpret_cast<const f32x4*>(p.queries)[i];
  __syncthreads();

  for (int g = 0; g < 64; g += ROWS) {  // wave-uniform bounds
    const int r0 = w * 64 + g;
    if (r0 >= rows) break;
    u32x4 v[ROWS][NC];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        v[r][c] = u32x4{0u, 0u, 0u, 0u};
        if (r0 + r < rows && c * 64 + lane < nch && HZ_DCHECK(row0 + r0 + r < (long)p.N))
          v[r][c] = *reinterpret_cast<const u32x4*>(p.corpus + (row0 + r0 + r) * p.ldc + (c * 64 + lane) * 8);
      }
    for (int q = 0; q < p.Q; ++q) {
      float acc[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) acc[r] = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c * 64 + lane < nch) {
          const float* qp = qs + q * p.D + (c * 64 + lane) * 8;
          const f32x4 qa = *reinterpret_cast<const f32x4*>(qp), qb = *reinterpret_cast<const f32x4*>(qp + 4);
          const float qv[8] = {qa[0], qa[1], qa[2], qa[3], qb[0], qb[1], qb[2], qb[3]};
#pragma unroll
          for (int r = 0; r < ROWS; ++r) {
            float f[8];
            unpack8(v[r][c], f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[r] = fmaf(qv[e], f[e], acc[r]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const float s = warp_sum(acc[r]);
        if (lane == r && r0 + r < rows) sc[q * T + r0 + r] = orderable(s);
      }
    }
  }
  __syncthreads();

  const int t = threadIdx.x;
  const int kk = min(p.k, rows);
  for (int q = 0; q < p.Q; ++q) {
    unsigned long long* out = p.cand + ((long)tile * p.Q + q) * p.k;
    const bool slot_ok = HZ_DCHECK(((long)tile * p.Q + q + 1) * p.k * 8 <= (long)p.cand_bytes);
    if (t < rows) {
      const unsigned mine = sc[q * T + t];
      int rank = 0;
      for (int j = 0; j < rows; ++j) {  // every lane reads the same word: an LDS broadcast
        const unsigned o = sc[q * T + j];
        rank += (o > mine) || (o == mine && j < t);
      }
      if (rank < kk && slot_ok)
        out[rank] = ((unsigned long long)mine << 32) | (unsigned)~(unsigned)(row0 + t);
    }
    if (t >= kk && t < p.k && slot_ok) out[t] = 0ull;  // a partial tile's unused slots (k <= 128 < T)
  }
}

// ------------------------------------------------------------------------------------- filtered scan
// The scan with pass(q, r) = live(r) && (filt == null || (tags[r] & mask[q]) == value[q]). Beside the
// queries, the kernel's start stages the tile's 8 live words, its T tag words and the Q {mask, value} pairs
// (one coalesced read each); thread t then folds them into pm[t], row t's pass bits over the queries. The
// row loop reads pm of its (wave-uniform) rows through readfirstlane: a row with no pass bit is not
// loaded, and a group of ROWS such rows only writes its sentinels -- scalar branches, no divergence. What a
// dead row holds (the uninitialised rows between count and capacity included) never reaches a register.
// A failing (q, r) is the sentinel 0 in `sc`, below orderable() of every real float. Ranking: a passing
// row's rank counts only keys above it, all real, so it is below the tile's pass count `np`; sentinel rows
// write nothing and slots np .. k-1 are zero-filled.
// Addresses beyond the scan's: live words [row0/32, row0/32 + 8) under word*32 < N (the launcher checks
// live_bytes), tags[row0 + t] under t < rows, filt[i] under i < 2Q.
//
// score_group: one group of ROWS rows (r0 .. r0 + ROWS - 1 of the tile, already in `v`) against every query: the fmaf
// chains and the butterfly of search_scan_kernel, statement for statement (the score bits are the same by
// construction; the unfiltered kernel keeps its own copy so that its code object does not change). `pm[r]`
// holds row r's pass bits (bit q = query q); a failing (q, r) writes the sentinel 0 instead of its score.
template <int NC>
__device__ __forceinline__ void score_group(const HzSearchParams& p, const float* qs, unsigned* sc,
                                            const u32x4 (&v)[ROWS][NC], const unsigned (&pm)[ROWS], int lane, int nch,
                                            int r0, int rows) {
  for (int q = 0; q < p.Q; ++q) {
    float acc[ROWS];
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[r] = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if (c * 64 + lane < nch) {
        const float* qp = qs + q * p.D + (c * 64 + lane) * 8;
        const f32x4 qa = *reinterpret_cast<const f32x4*>(qp), qb = *reinterpret_cast<const f32x4*>(qp + 4);
        const float qv[8] = {qa[0], qa[1], qa[2], qa[3], qb[0], qb[1], qb[2], qb[3]};
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
          float f[8];
          unpack8(v[r][c], f);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[r] = fmaf(qv[e], f[e], acc[r]);
        }
      }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const float s = warp_sum(acc[r]);
      if (lane == r && r0 + r < rows) sc[q * T + r0 + r] = ((pm[r] >> q) & 1u) ? orderable(s) : 0u;
    }
  }
}

template <int NC>
__global__ __launch_bounds__(T) void search_fscan_kernel(const HzSearchFilterParams fp) {
  const HzSearchParams& p = fp.s;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* qs = lds;                                              // [Q][D]
  unsigned* sc = reinterpret_cast<unsigned*>(lds + p.Q * p.D);  // [Q][T]
  unsigned* pmask = sc + p.Q * T;                               // [T]: tags, then pass bits
  unsigned* lv = pmask + T;                                     // [T / 32] live words of the tile
  unsigned* fl = lv + T / 32;                                   // [Q][2]
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = threadIdx.x;
  const int tile = blockIdx.x;
  const int nch = p.D >> 3;
  if (!HZ_DCHECK(tile < p.ntile && p.D <= NC * 512 && p.ldc >= p.D && (long)tile * T < (long)p.N)) return;
  const long row0 = (long)tile * T;
  const int rows = (int)min((long)T, (long)p.N - row0);
  for (int i = t; i < p.Q * (p.D >> 2); i += T)
    reinterpret_cast<f32x4*>(qs)[i] = reinterpret_cast<const f32x4*>(p.queries)[i];
  unsigned tag = 0u;
  if (fp.tags && t < rows && HZ_DCHECK(row0 + t < (long)p.N)) tag = fp.tags[row0 + t];
  if (t < T / 32) {
    const long word = (row0 >> 5) + t;
    lv[t] = (word * 32 < (long)p.N && HZ_DCHECK((word + 1) * 4 <= (long)fp.live_bytes)) ? fp.live[word] : 0u;
  }
  if (fp.filt && t < 2 * p.Q && HZ_DCHECK(t < 2 * HZ_SEARCH_MAX_Q)) fl[t] = fp.filt[t];
  __syncthreads();
  {
    unsigned bits = 0u;
    if (t < rows && ((lv[t >> 5] >> (t & 31)) & 1u)) {
      bits = (1u << p.Q) - 1u;  // Q <= 16
      if (fp.filt) {
        bits = 0u;
        for (int q = 0; q < p.Q; ++q) bits |= (unsigned)((tag & fl[2 * q]) == fl[2 * q + 1]) << q;
      }
    }
    pmask[t] = bits;
  }
  __syncthreads();

  for (int g = 0; g < 64; g += ROWS) {  // wave-uniform bounds
    const int r0 = w * 64 + g;
    if (r0 >= rows) break;
    unsigned pm[ROWS], any = 0u;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {  // r0 + r < T: rows past the tile's end have pass bits 0
      pm[r] = __builtin_amdgcn_readfirstlane(pmask[r0 + r]);
      any |= pm[r];
    }
    if (any == 0u) {  // scalar: nothing of this group is loaded or scored
      if (lane < ROWS && r0 + lane < rows)
        for (int q = 0; q < p.Q; ++q) sc[q * T + r0 + lane] = 0u;
      continue;
    }
    u32x4 v[ROWS][NC];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        v[r][c] = u32x4{0u, 0u, 0u, 0u};
        if (pm[r] != 0u && c * 64 + lane < nch && HZ_DCHECK(row0 + r0 + r < (long)p.N))
          v[r][c] = *reinterpret_cast<const u32x4*>(p.corpus + (row0 + r0 + r) * p.ldc + (c * 64 + lane) * 8);
      }
    score_group<NC>(p, qs, sc, v, pm, lane, nch, r0, rows);
  }
  __syncthreads();

  for (int q = 0; q < p.Q; ++q) {
    unsigned long long* out = p.cand + ((long)tile * p.Q + q) * p.k;
    const bool slot_ok = HZ_DCHECK(((long)tile * p.Q + q + 1) * p.k * 8 <= (long)p.cand_bytes);
    const unsigned mine = t < rows ? sc[q * T + t] : 0u;
    int rank = 0, np = 0;
    for (int j = 0; j < rows; ++j) {  // every lane reads the same word: an LDS broadcast
      const unsigned o = sc[q * T + j];
      rank += (o > mine) || (o == mine && j < t);
      np += o != 0u;
    }
    if (mine != 0u && rank < p.k && slot_ok)
      out[rank] = ((unsigned long long)mine << 32) | (unsigned)~(unsigned)(row0 + t);
    if (t >= np && t < p.k && slot_ok) out[t] = 0ull;  // the slots past the passing rows (k <= 128 < T)
  }
}

// ------------------------------------------------------------------------------------ quantised scan
// search_fscan_kernel's structure over rows of OCP e4m3fn bytes with one fp32 scale per row
// (HzSearchQuantParams; always with a live bitmap, tags and filter optional). Staging is the filtered scan's;
// after the pass bits are known, thread t reads scales[row0 + t] into LDS iff row t passes for some query
// (one coalesced read of at most 1 KB), so neither the bytes nor the scale of a dead row is ever loaded:
// they may be NaN codes and NaN or inf scales. Lane l holds the 16-B chunks l, l + 64 of a row: 16 elements
// each, NC = 1 up to D = 1024 and 2 up to 2048. A group's bytes are decoded to fp32 ONCE, before the loop
// over the queries (v_cvt_pk_f32_fp8: exact for the 254 finite codes, subnormals and -0 included).
// score(q, r): every lane runs one fmaf chain over its elements in ascending column order from +0 (a lane
// past the row's end keeps +0), the 64 sums meet in the xor butterfly, and the sum is multiplied ONCE, in
// fp32, by scales[r]; then orderable().
// CONTRACT: the bits of score(q, r) depend on the query's D values, the row's D codes and the row's scale,
// and on nothing else: not on N, Q, k, the row's position or tile, the other queries, the filter, or what
// dead rows hold. Ranking, candidate layout and zero fill are search_fscan_kernel's.
// Addresses beyond the filtered scan's: the byte rows at (row0 + r) * ldc + chunk * 16 under chunk < D / 16
// and row < N, scales[row0 + t] under t < rows.
__device__ __forceinline__ void decode16(const u32x4 v, float* f) {
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

template <int NC>
__global__ __launch_bounds__(T) void search_qscan_kernel(const HzSearchQuantParams qp) {
  const HzSearchFilterParams& fp = qp.f;
  const HzSearchParams& p = fp.s;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* qs = lds;                                              // [Q][D]
  unsigned* sc = reinterpret_cast<unsigned*>(lds + p.Q * p.D);  // [Q][T]
  unsigned* pmask = sc + p.Q * T;                               // [T]: pass bits
  unsigned* lv = pmask + T;                                     // [T / 32] live words of the tile
  unsigned* fl = lv + T / 32;                                   // [Q][2]
  float* scl = reinterpret_cast<float*>(fl + 2 * p.Q);          // [T]: the scales of the passing rows
  const unsigned char* rows8 = reinterpret_cast<const unsigned char*>(p.corpus);
  const int lane = threadIdx.x & 63;
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = threadIdx.x;
  const int tile = blockIdx.x;
  const int nch = p.D >> 4;
  if (!HZ_DCHECK(tile < p.ntile && p.D <= NC * 1024 && p.ldc >= p.D && (long)tile * T < (long)p.N)) return;
  const long row0 = (long)tile * T;
  const int rows = (int)min((long)T, (long)p.N - row0);
  for (int i = t; i < p.Q * (p.D >> 2); i += T)
    reinterpret_cast<f32x4*>(qs)[i] = reinterpret_cast<const f32x4*>(p.queries)[i];
  unsigned tag = 0u;
  if (fp.tags && t < rows && HZ_DCHECK(row0 + t < (long)p.N)) tag = fp.tags[row0 + t];
  if (t < T / 32) {
    const long word = (row0 >> 5) + t;
    lv[t] = (word * 32 < (long)p.N && HZ_DCHECK((word + 1) * 4 <= (long)fp.live_bytes)) ? fp.live[word] : 0u;
  }
  if (fp.filt && t < 2 * p.Q && HZ_DCHECK(t < 2 * HZ_SEARCH_MAX_Q)) fl[t] = fp.filt[t];
  __syncthreads();
  {
    unsigned bits = 0u;
    if (t < rows && ((lv[t >> 5] >> (t & 31)) & 1u)) {
      bits = (1u << p.Q) - 1u;  // Q <= 16
      if (fp.filt) {
        bits = 0u;
        for (int q = 0; q < p.Q; ++q) bits |= (unsigned)((tag & fl[2 * q]) == fl[2 * q + 1]) << q;
      }
    }
    pmask[t] = bits;
    float s = 0.f;
    if (bits != 0u && HZ_DCHECK(t < rows && row0 + t < (long)p.N)) s = qp.scales[row0 + t];
    scl[t] = s;
  }
  __syncthreads();

  for (int g = 0; g < 64; g += ROWS) {  // wave-uniform bounds
    const int r0 = w * 64 + g;
    if (r0 >= rows) break;
    unsigned pm[ROWS], any = 0u;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {  // r0 + r < T: rows past the tile's end have pass bits 0
      pm[r] = __builtin_amdgcn_readfirstlane(pmask[r0 + r]);
      any |= pm[r];
    }
    if (any == 0u) {  // scalar: nothing of this group is loaded or scored
      if (lane < ROWS && r0 + lane < rows)
        for (int q = 0; q < p.Q; ++q) sc[q * T + r0 + lane] = 0u;
      continue;
    }
    u32x4 v[ROWS][NC];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        v[r][c] = u32x4{0u, 0u, 0u, 0u};
        if (pm[r] != 0u && c * 64 + lane < nch && HZ_DCHECK(row0 + r0 + r < (long)p.N))
          v[r][c] = *reinterpret_cast<const u32x4*>(rows8 + (row0 + r0 + r) * p.ldc + (c * 64 + lane) * 16);
      }
    float f[ROWS][NC][16], rs[ROWS];  // decoded once for all queries
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      rs[r] = scl[r0 + r];  // every lane reads the same word: an LDS broadcast
#pragma unroll
      for (int c = 0; c < NC; ++c) decode16(v[r][c], f[r][c]);
    }
    for (int q = 0; q < p.Q; ++q) {
      float acc[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) acc[r] = 0.f;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c * 64 + lane < nch) {
          const f32x4* qv4 = reinterpret_cast<const f32x4*>(qs + q * p.D + (c * 64 + lane) * 16);
          float qv[16];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const f32x4 x = qv4[i];
            qv[4 * i] = x[0], qv[4 * i + 1] = x[1], qv[4 * i + 2] = x[2], qv[4 * i + 3] = x[3];
          }
#pragma unroll
          for (int r = 0; r < ROWS; ++r)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[r] = fmaf(qv[e], f[r][c][e], acc[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const float s = warp_sum(acc[r]) * rs[r];
        if (lane == r && r0 + r < rows) sc[q * T + r0 + r] = ((pm[r] >> q) & 1u) ? orderable(s) : 0u;
      }
    }
  }
  __syncthreads();

  for (int q = 0; q < p.Q; ++q) {
    unsigned long long* out = p.cand + ((long)tile * p.Q + q) * p.k;
    const bool slot_ok = HZ_DCHECK(((long)tile * p.Q + q + 1) * p.k * 8 <= (long)p.cand_bytes);
    const unsigned mine = t < rows ? sc[q * T + t] : 0u;
    int rank = 0, np = 0;
    for (int j = 0; j < rows; ++j) {  // every lane reads the same word: an LDS broadcast
      const unsigned o = sc[q * T + j];
      rank += (o > mine) || (o == mine && j < t);
      np += o != 0u;
    }
    if (mine != 0u && rank < p.k && slot_ok)
      out[rank] = ((unsigned long long)mine << 32) | (unsigned)~(unsigned)(row0 + t);
    if (t >= np && t < p.k && slot_ok) out[t] = 0ull;  // the slots past the passing rows (k <= 128 < T)
  }
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

// one refusal list for both launchers: the kernels then have no address that the data can move out of
// its buffer. Fills ntile.
int search_check(HzSearchParams& p) {
  if (!p.corpus || !p.queries || !p.cand || !p.out_score || !p.out_id) return -1;
  if (p.D < 8 || p.D % 8 || p.D > 2048 || p.ldc < p.D || p.ldc % 8) return -2;
  if (p.N < 1) return -3;  // N is an int: N >= 2^31 cannot be expressed (hz_search_scratch_bytes refuses it)
  if (p.Q < 1 || p.Q > HZ_SEARCH_MAX_Q) return -4;
  if (p.k < 1 || p.k > HZ_SEARCH_MAX_K) return -5;
  if ((reinterpret_cast<uintptr_t>(p.corpus) & 15) || (reinterpret_cast<uintptr_t>(p.queries) & 15) ||
      (reinterpret_cast<uintptr_t>(p.cand) & 7) || (reinterpret_cast<uintptr_t>(p.out_score) & 3) ||
      (reinterpret_cast<uintptr_t>(p.out_id) & 3))
    return -6;
  const unsigned long long need = hz_search_scratch_bytes(p.N, p.Q, p.k);
  if (!need || p.cand_bytes < need) return -7;
  p.ntile = (int)(((long)p.N + T - 1) / T);
  return 0;
}

// dynamic LDS above 64 KiB is allowed per kernel and device: once, outside any capture (an index does it
// at open through hz_search_code_warm; a direct launch here)
int raise_lds_limit() {
  static bool done[64];
  int d = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return -8;
  if (done[d]) return 0;
  const void* fns[10] = {reinterpret_cast<const void*>(&search_scan_kernel<1>),
                        reinterpret_cast<const void*>(&search_scan_kernel<2>),
                        reinterpret_cast<const void*>(&search_scan_kernel<3>),
                        reinterpret_cast<const void*>(&search_scan_kernel<4>),
                        reinterpret_cast<const void*>(&search_fscan_kernel<1>),
                        reinterpret_cast<const void*>(&search_fscan_kernel<2>),
                        reinterpret_cast<const void*>(&search_fscan_kernel<3>),
                        reinterpret_cast<const void*>(&search_fscan_kernel<4>),
                        reinterpret_cast<const void*>(&search_qscan_kernel<1>),
                        reinterpret_cast<const void*>(&search_qscan_kernel<2>)};
  for (const void* f : fns) HZ_CHECK(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
  done[d] = true;
  return 0;
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
  const size_t lds = ((size_t)p.Q * p.D + (size_t)p.Q * T) * 4;  // <= 16 * (2048 + 256) * 4 = 144 KiB
  if (const int rc = raise_lds_limit()) return rc;
  switch ((p.D / 8 + 63) / 64) {
    case 1: hipLaunchKernelGGL((search_scan_kernel<1>), dim3(p.ntile), dim3(T), lds, st, p); break;
    case 2: hipLaunchKernelGGL((search_scan_kernel<2>), dim3(p.ntile), dim3(T), lds, st, p); break;
    case 3: hipLaunchKernelGGL((search_scan_kernel<3>), dim3(p.ntile), dim3(T), lds, st, p); break;
    default: hipLaunchKernelGGL((search_scan_kernel<4>), dim3(p.ntile), dim3(T), lds, st, p); break;
  }
  return (int)hipGetLastError();
}

extern "C" int hz_search_fscan_launch(const HzSearchFilterParams* pp, hipStream_t st) {
  HzSearchFilterParams f = *pp;
  HzSearchParams& p = f.s;
  if (const int rc = search_check(p)) return rc;
  if (!f.live || (reinterpret_cast<uintptr_t>(f.live) & 3)) return -12;
  if (f.live_bytes < 4ull * (((unsigned long long)p.N + 31) / 32)) return -13;
  if (f.filt && !f.tags) return -14;
  if ((reinterpret_cast<uintptr_t>(f.tags) & 3) || (reinterpret_cast<uintptr_t>(f.filt) & 3)) return -15;
  // the scan's LDS plus the pass bits [T], the tile's live words and the Q filters: <= 144 KiB + 1184 B
  const size_t lds = ((size_t)p.Q * p.D + (size_t)p.Q * T + T + T / 32 + 2 * (size_t)p.Q) * 4;
  if (const int rc = raise_lds_limit()) return rc;
  switch ((p.D / 8 + 63) / 64) {
    case 1: hipLaunchKernelGGL((search_fscan_kernel<1>), dim3(p.ntile), dim3(T), lds, st, f); break;
    case 2: hipLaunchKernelGGL((search_fscan_kernel<2>), dim3(p.ntile), dim3(T), lds, st, f); break;
    case 3: hipLaunchKernelGGL((search_fscan_kernel<3>), dim3(p.ntile), dim3(T), lds, st, f); break;
    default: hipLaunchKernelGGL((search_fscan_kernel<4>), dim3(p.ntile), dim3(T), lds, st, f); break;
  }
  return (int)hipGetLastError();
}

// The filtered launcher's refusals with the byte rows' dimension rules: -16 D % 16, -17 D < 16, -18 D > 2048,
// -19 ldc < D, -23 ldc % 16 (ldc in bytes), -24 scales null, -25 scales not 4-byte aligned.
extern "C" int hz_search_qscan_launch(const HzSearchQuantParams* pp, hipStream_t st) {
  HzSearchQuantParams qp = *pp;
  HzSearchFilterParams& f = qp.f;
  HzSearchParams& p = f.s;
  if (p.D < 16) return -17;
  if (p.D % 16) return -16;
  if (p.D > 2048) return -18;
  if (p.ldc < p.D) return -19;
  if (p.ldc % 16) return -23;
  if (const int rc = search_check(p)) return rc;
  if (!f.live || (reinterpret_cast<uintptr_t>(f.live) & 3)) return -12;
  if (f.live_bytes < 4ull * (((unsigned long long)p.N + 31) / 32)) return -13;
  if (f.filt && !f.tags) return -14;
  if ((reinterpret_cast<uintptr_t>(f.tags) & 3) || (reinterpret_cast<uintptr_t>(f.filt) & 3)) return -15;
  if (!qp.scales) return -24;
  if (reinterpret_cast<uintptr_t>(qp.scales) & 3) return -25;
  // the filtered scan's LDS plus the tile's scales [T]: <= 144 KiB + 1184 B + 1 KiB
  const size_t lds = ((size_t)p.Q * p.D + (size_t)p.Q * T + T + T / 32 + 2 * (size_t)p.Q + T) * 4;
  if (const int rc = raise_lds_limit()) return rc;
  if (p.D <= 1024) hipLaunchKernelGGL((search_qscan_kernel<1>), dim3(p.ntile), dim3(T), lds, st, qp);
  else hipLaunchKernelGGL((search_qscan_kernel<2>), dim3(p.ntile), dim3(T), lds, st, qp);
  return (int)hipGetLastError();
}

extern "C" int hz_search_merge_launch(const HzSearchParams* pp, hipStream_t st) {
  HzSearchParams p = *pp;
  if (const int rc = search_check(p)) return rc;
  hipLaunchKernelGGL(search_merge_kernel, dim3(p.Q), dim3(MERGE_THREADS), 0, st, p);
  return (int)hipGetLastError();
}

// Load this translation unit's device code without a launch (see hz_conv_code_warm in conv.hip).
__global__ void hz_search_code_warm_kernel() {}
extern "C" int hz_search_code_warm(void) {
  hipFuncAttributes a;
  if (const int rc = (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&hz_search_code_warm_kernel))) return rc;
  return raise_lds_limit();
}
