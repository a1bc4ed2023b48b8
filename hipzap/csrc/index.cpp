// .hzidx vector indexes (hipzap.h "vector search"): the bf16 row block of a file in device memory and a
// fixed set of search contexts over it. A search copies its queries into the context's pinned slot and
// replays the context's program for its (Q, k): H2D copy of the slot, scan, merge, D2H copies of the
// scores and ids, then waits on the context's stream. Q and k size the merge grid and the candidate
// layout, which a captured graph holds by value, so a program is built, run once eagerly and captured
// on the first search of each (Q, k), and replayed from then on (at most 16 x 128 small programs).
//
// A live index: the rows are allocated for a capacity of whole tiles, beside them a live
// bitmap and one tag word per row. An index that was never mutated, searched without a filter, runs the
// program above. Every other search runs the FILTERED program of its (Q, k): H2D copy of the slot (the
// {mask, value} pairs in front of the queries), filtered scan, merge, two D2H copies. Its N is the count
// rounded up to a whole tile (the rows past the count are dead in the bitmap), so deletes, tag writes and
// adds inside the last tile change device data only and keep every captured program; an add that crosses
// a tile boundary, or a growth (new allocations), destroys the programs, which are re-captured on next use.
// A mutation holds every context's mutex and synchronises its copies before it releases them.
//
// An fp8 index (a version-3 file): the rows are e4m3fn bytes and beside them lies one fp32 scale
// per row. It ALWAYS replays the quantised-scan program of its (Q, k) -- H2D, qscan, merge, two D2H -- with the
// filtered programs' N and mask 0 / value 0 when there is no filter; the invalidation rules are the same.
//
// A two-stage index (a version-4 file): an fp8 index that also holds its rows as a bf16 index
// would, in device memory or in pinned host memory that the kernel reads through its mapped address. A search
// with refine = R replays H2D, qscan at k = R, merge at k = R into the context's intermediate buffer, rescore
// of those R ids into out_dev, two D2H; refine = 0 replays the fp8 program above. R is part of a program's key.
//
// An IVF index (a version-5 file): a bf16 index whose rows, tags and bitmap are stored list by list
// in whole tiles; `count` here is the stored row count (the file's capacity), `n_ext` the number of vectors, and
// every public id is an external id that `pos_of` maps to its stored row. A search with nprobe lists replays
// H2D, scan + merge over the centroids at k = nprobe into the context's probe buffer, the list scan over those
// lists with P = the tiles of the nprobe largest lists, merge over the P candidate lists, two D2H; nprobe = 0
// (every list) has no coarse stage. nprobe is part of a program's key. Rows are never added.
//
// An fp8 IVF index (a version-6 or version-7 file): version 5's layout over e4m3 rows with one scale
// per stored row; the list scan of its programs is HZ_K_SEARCH_QLSCAN, the coarse stage (bf16 centroids) is the
// same. Version 7 also holds the vectors' bf16 rows BY EXTERNAL ID (`n_ext` rows, device or pinned host memory):
// with refine = R the list scan and its merge run at k = R into the context's intermediate buffer and
// HZ_K_SEARCH_RESCORE re-scores those external ids against rrows[id] with N = n_ext. R is part of the key too.
//
// A binary index (a version-8 or version-9 file): the rows are sign bits, dim / 32 words each, with no
// scales. It replays version 3's programs with HZ_K_SEARCH_BSCAN in place of the quantised scan (the scan's block
// carries the pitch in words, the merge's keeps ldc = dim), and version 9 (bf16 rescore rows, either placement)
// replays version 4's two-stage programs; keys and invalidation rules are the same.
//
// A product-quantised index (a version-10 or version-11 file): the rows are M code bytes, beside them
// lies the fp32 codebook [M][256][dim / M] (device memory, a host mirror for hz_index_read_codebook) and every context
// holds a table scratch [MAX_Q][M][256] fp32. It replays version 3's programs with HZ_K_SEARCH_PQLUT and
// HZ_K_SEARCH_PQSCAN in place of the quantised scan (the scan's block carries the pitch in bytes, the merge's keeps
// ldc = dim), and version 11 replays version 4's two-stage programs; keys and invalidation rules are the same.
//
// Neighbours of stored rows (a plain bf16 index): hz_index_neighbors replays H2D of the ids,
// HZ_K_SEARCH_MSCAN, HZ_K_SEARCH_MERGEN, two D2H, with the filtered programs' N (the rows past the count are dead
// in the bitmap) and so under their invalidation rules. A context's buffers for it (ids, results, candidate
// scratch) are allocated on the first such call; the scratch grows to the largest (n, k) asked for.
//
// Bulk search (a plain bf16 index): hz_index_search_batch replays H2D of the queries, HZ_K_SEARCH_XSCAN
// and HZ_K_SEARCH_MERGEN at k = R, HZ_K_SEARCH_RESCOREN of those ids against the index's own rows (R -> k) and three
// D2H (scores, ids, stage one's scores), with the neighbours programs' N and rules and their candidate scratch.
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

#include "hipzap.h"

namespace {

thread_local std::string g_err;
std::nullptr_t fail(const std::string& m) {
  g_err = m;
  return nullptr;
}

constexpr uint64_t kTile = HZ_SEARCH_TILE;
constexpr size_t kFiltBytes = (size_t)HZ_SEARCH_MAX_Q * 2 * 4;  // [MAX_Q][2] u32 in front of the queries

struct Ctx {
  std::mutex mu;
  hipStream_t st = nullptr;
  char* slot_host = nullptr;          // pinned: the filters [MAX_Q][2] u32, then the queries
  char* slot_dev = nullptr;
  float* q_host = nullptr;            // slot_host + kFiltBytes: [MAX_Q][dim]
  float* q_dev = nullptr;
  unsigned long long* cand = nullptr;
  uint64_t cand_bytes = 0;
  char* out_dev = nullptr;            // [MAX_Q][MAX_K] fp32 scores, then [MAX_Q][MAX_K] int32 ids
  char* out_host = nullptr;           // pinned, the same layout
  float* lut = nullptr;               // pq8 only: the queries' tables [MAX_Q][M][256] fp32
  char* mid_dev = nullptr;            // two-stage only: stage one's scores and ids, the layout of out_dev
  char* probe_dev = nullptr;          // IVF only: the coarse stage's scores and list ids, the layout of out_dev
  unsigned long long* ccand = nullptr;  // IVF only: the coarse stage's candidate scratch
  uint64_t ccand_bytes = 0;
  // neighbours only, allocated on first use: the ids (pinned, device), the results [SELF_MAX_Q][MAX_K] scores then
  // ids (device, pinned) and the candidate scratch [tiles][n][k], grown on demand
  int* nid_host = nullptr;
  int* nid_dev = nullptr;
  char* nout_dev = nullptr;
  char* nout_host = nullptr;
  unsigned long long* ncand = nullptr;  // shared with bulk search
  uint64_t ncand_bytes = 0;
  // bulk search only, allocated on first use: the queries [SELF_MAX_Q][dim] (pinned, device), stage one's results and
  // the final ones (device, the layout of nout_dev), and pinned: scores, ids, then stage one's scores
  float* bq_host = nullptr;
  float* bq_dev = nullptr;
  char* bmid_dev = nullptr;
  char* bout_dev = nullptr;
  char* bout_host = nullptr;
  // clustering only (hz_index_assign / hz_index_cmean), device memory allocated on first use and grown on demand:
  // centroids bf16 [C][dim]; live AND mask, cap / 8 bytes; lists int32 then scores fp32, [scan rows] each; the
  // members int32 [M]; seg_off int32 [C + 1]; the fp32 centroids [C][dim]
  enum { kClCent, kClMask, kClOut, kClOrder, kClSeg, kClCent32, kClBufs };
  void* cl[kClBufs] = {};
  uint64_t cl_bytes[kClBufs] = {};
  // (Q, k, filtered, R, 0; R = 0: one stage); IVF: (Q, k, 1, R, nprobe; 0: every list) and (Q, nprobe, 2, 0, 0):
  // probes alone; neighbours: (n, k, 3, skip_self, 0); bulk search: (Q, k, 4, R, 0)
  std::map<std::tuple<int, int, int, int, int>, HzProgram> progs;
};

constexpr size_t kOutHalf = (size_t)HZ_SEARCH_MAX_Q * HZ_SEARCH_MAX_K * 4;
constexpr size_t kSelfOutHalf = (size_t)HZ_INDEX_SELF_MAX_Q * HZ_SEARCH_MAX_K * 4;

uint64_t round_up(uint64_t v, uint64_t m) { return (v + m - 1) / m * m; }

// the unsigned integer value of `"key": <digits>` in the JSON header. The writer puts these keys last, after
// the labels, so the LAST occurrence is the key itself even when a label spells the same word
// (`strict`: the colon must follow the key at once -- a version-3 file may lack the key, and a label that
// spells it is followed by a comma or a bracket)
bool json_u64(const std::string& js, const char* key, uint64_t* out, bool strict = false) {
  const std::string k = std::string("\"") + key + "\"";
  size_t at = js.rfind(k);
  if (at == std::string::npos) return false;
  if (strict && (at + k.size() >= js.size() || js[at + k.size()] != ':')) return false;
  at = js.find(':', at + k.size());
  if (at == std::string::npos) return false;
  ++at;
  while (at < js.size() && js[at] == ' ') ++at;
  if (at >= js.size() || js[at] < '0' || js[at] > '9') return false;
  *out = std::strtoull(js.c_str() + at, nullptr, 10);
  return true;
}

struct Index {
  int device = 0;
  HzIndexHeader h{};                  // of the file; `count` below is the open index's
  uint64_t count = 0, cap = 0;        // rows in use (ids 0 .. count-1), rows allocated (whole tiles)
  uint64_t live_count = 0;
  bool mutated = false;               // the unfiltered program (N = the file's count, all live) no longer holds
  bool has_tags = false;
  bool fp8 = false;                   // a version-3, 4, 6 or 7 file: e4m3fn byte rows and `scales`
  bool bin = false;                   // a version-8 or 9 file: sign-bit rows, dim / 32 words each (never with fp8 or ivf)
  bool pq = false;                    // a version-10 or 11 file: pq8 rows, pq_m code bytes each (never with fp8, bin or ivf)
  int pq_m = 0;                       // sub-spaces = bytes per row; dsub = dim / pq_m
  float* codebook = nullptr;          // device fp32 [pq_m][256][dim / pq_m]
  std::vector<float> codebook_host;   // its mirror
  unsigned short* rows = nullptr;     // bf16 [cap][dim], or uint8 [cap][dim] of an fp8 index
  float* scales = nullptr;            // device, cap floats (fp8 only)
  bool rescore = false;               // a version-4, 7 or 9 file: `rrows` beside the fp8 or sign-bit rows
  bool rescore_host = false;          // rrows is pinned host memory (hipHostMalloc), else device memory
  unsigned short* rrows = nullptr;    // bf16 [cap][dim] ([n_ext][dim], by external id, of an IVF index), the allocation
  unsigned short* rrows_dev = nullptr;  // the address the rescore kernel reads (the mapped address of a host block)
  unsigned* live = nullptr;          // device, cap / 32 words
  unsigned* tags = nullptr;           // device, cap words
  std::vector<uint32_t> live_host, tags_host;  // mirrors, sized like the device buffers
  bool ivf = false;                   // a version-5, 6 or 7 file
  int self_max = HZ_INDEX_SELF_MAX_Q;  // the ids one hz_index_neighbors call takes (hz_index_neighbors_max)
  uint64_t n_ext = 0;                 // IVF: the number of vectors (external ids 0 .. n_ext-1)
  int nlist = 0, nprobe_default = 0;
  unsigned short* centroids = nullptr;  // device bf16 [nlist][dim]
  int* ivf_tables = nullptr;          // device: list_off [nlist + 1], list_tiles [tiles], rowid [count], one block
  std::vector<int32_t> pos_of;        // external id -> stored row
  std::vector<int> tiles_desc;        // the lists' tile counts, largest first
  std::vector<std::unique_ptr<Ctx>> ctx;

  ~Index() {
    (void)hipSetDevice(device);
    for (auto& c : ctx) {
      if (c->st) (void)hipStreamSynchronize(c->st);
      for (auto& kv : c->progs) hz_prog_destroy(kv.second);
      if (c->slot_host) (void)hipHostFree(c->slot_host);
      if (c->out_host) (void)hipHostFree(c->out_host);
      if (c->slot_dev) (void)hipFree(c->slot_dev);
      if (c->cand) (void)hipFree(c->cand);
      if (c->out_dev) (void)hipFree(c->out_dev);
      if (c->mid_dev) (void)hipFree(c->mid_dev);
      if (c->lut) (void)hipFree(c->lut);
      if (c->probe_dev) (void)hipFree(c->probe_dev);
      if (c->ccand) (void)hipFree(c->ccand);
      if (c->nid_host) (void)hipHostFree(c->nid_host);
      if (c->nout_host) (void)hipHostFree(c->nout_host);
      if (c->nid_dev) (void)hipFree(c->nid_dev);
      if (c->nout_dev) (void)hipFree(c->nout_dev);
      if (c->ncand) (void)hipFree(c->ncand);
      if (c->bq_host) (void)hipHostFree(c->bq_host);
      if (c->bout_host) (void)hipHostFree(c->bout_host);
      if (c->bq_dev) (void)hipFree(c->bq_dev);
      if (c->bmid_dev) (void)hipFree(c->bmid_dev);
      if (c->bout_dev) (void)hipFree(c->bout_dev);
      for (void* b : c->cl)
        if (b) (void)hipFree(b);
      if (c->st) (void)hipStreamDestroy(c->st);
    }
    free_rescore(rrows);
    if (rows) (void)hipFree(rows);
    if (live) (void)hipFree(live);
    if (tags) (void)hipFree(tags);
    if (scales) (void)hipFree(scales);
    if (centroids) (void)hipFree(centroids);
    if (codebook) (void)hipFree(codebook);
    if (ivf_tables) (void)hipFree(ivf_tables);
  }

  // the stored row of a public id, -1 for an id outside the index
  int64_t pos(int id) const {
    if (id < 0 || (uint64_t)id >= (ivf ? n_ext : count)) return -1;
    return ivf ? pos_of[id] : id;
  }

  uint64_t rowb() const { return pq ? (uint64_t)pq_m : bin ? h.dim / 8 : fp8 ? h.dim : h.dim * 2ull; }  // bytes per stored row
  const char* dtype_name() const { return pq ? "pq8" : bin ? "bin_sign" : fp8 ? "fp8_e4m3" : "bf16"; }
  uint64_t codebook_bytes() const { return pq ? 256ull * h.dim * 4 : 0; }  // pq_m * 256 * (dim / pq_m) floats
  uint64_t lut_bytes() const { return pq ? (uint64_t)HZ_SEARCH_MAX_Q * pq_m * 1024 : 0; }  // per context
  // what the by-name refusals call a quantised index without lists
  const char* quant_name() const { return pq ? "a pq8 index" : bin ? "a bin_sign index" : "an fp8_e4m3 index"; }
  uint64_t row_bytes() const { return cap * rowb(); }
  uint64_t scan_rows() const { return round_up(count, kTile); }  // the filtered programs' N
  uint64_t rescore_rows(uint64_t for_cap) const { return ivf ? n_ext : for_cap; }  // an IVF index holds them by id
  uint64_t rescore_bytes() const { return rescore ? rescore_rows(cap) * h.dim * 2 : 0; }

  // a block for the rescore rows in the index's placement: *p the allocation, *dev what a kernel reads
  bool alloc_rescore(uint64_t bytes, unsigned short** p, unsigned short** dev) const {
    if (!rescore_host) {
      if (hipMalloc(reinterpret_cast<void**>(p), bytes) != hipSuccess) return false;
      *dev = *p;
      return true;
    }
    if (hipHostMalloc(reinterpret_cast<void**>(p), bytes, hipHostMallocMapped) != hipSuccess) return false;
    return hipHostGetDevicePointer(reinterpret_cast<void**>(dev), *p, 0) == hipSuccess;
  }
  void free_rescore(unsigned short* p) const {
    if (p) (void)(rescore_host ? hipHostFree(p) : hipFree(p));
  }

  void drop_programs() {  // the caller holds every context's mutex
    for (auto& c : ctx) {
      for (auto& kv : c->progs) hz_prog_destroy(kv.second);
      c->progs.clear();
    }
  }

  // the first mutation: the unfiltered programs (N = the file's count, all live) are never replayed again
  void set_mutated() {  // the caller holds every context's mutex
    if (mutated) return;
    mutated = true;
    for (auto& c : ctx)
      for (auto it = c->progs.begin(); it != c->progs.end();) {
        if (std::get<2>(it->first) == 0) {
          hz_prog_destroy(it->second);
          it = c->progs.erase(it);
        } else {
          ++it;
        }
      }
  }

  // the context's program for (Q, k, filtered, R), built on first use (the caller holds c.mu). R > 0 (a
  // two-stage index only): stage one runs at k = R into mid_dev and the rescore writes the k results.
  HzProgram program(Ctx& c, int Q, int k, bool filtered, int R, bool* fresh) {
    const auto key = std::make_tuple(Q, k, (int)filtered, R, 0);
    auto it = c.progs.find(key);
    *fresh = it == c.progs.end();
    if (!*fresh) return it->second;
    HzSearchQuantParams qp{};
    HzSearchFilterParams& f = qp.f;
    HzSearchParams& p = f.s;
    p.corpus = rows;
    p.queries = c.q_dev;
    p.cand = c.cand;
    char* stage1 = R ? c.mid_dev : c.out_dev;
    p.out_score = reinterpret_cast<float*>(stage1);
    p.out_id = reinterpret_cast<int*>(stage1 + kOutHalf);
    p.N = (int)(filtered ? scan_rows() : count);
    p.D = p.ldc = (int)h.dim;
    p.Q = Q;
    p.k = R ? R : k;
    HzSearchRescoreParams rp{};
    rp.rows = rrows_dev;
    rp.queries = c.q_dev;
    rp.in_id = p.out_id;
    rp.out_score = reinterpret_cast<float*>(c.out_dev);
    rp.out_id = reinterpret_cast<int*>(c.out_dev + kOutHalf);
    rp.N = p.N, rp.D = rp.ldc = p.D, rp.Q = Q, rp.R = R, rp.k = k;
    p.cand_bytes = c.cand_bytes;
    f.live = live;
    f.tags = tags;
    f.filt = reinterpret_cast<const unsigned*>(c.slot_dev);
    f.live_bytes = cap / 8;
    qp.scales = scales;
    HzSearchBinParams bp{};  // sign-bit rows: the filtered block with the pitch in words (the merge keeps ldc = D)
    bp.f = f;
    bp.f.s.ldc = (int)h.dim / 32;
    HzSearchPqLutParams lp{};  // pq8 rows: the queries' tables, then the scan over the code bytes (pitch in bytes)
    lp.queries = c.q_dev, lp.codebook = codebook, lp.lut = c.lut, lp.lut_bytes = lut_bytes();
    lp.D = (int)h.dim, lp.M = pq_m, lp.Q = Q;
    HzSearchPqParams pp{};
    pp.f = f;
    pp.f.s.ldc = pq_m;
    pp.lut = c.lut, pp.lut_bytes = lut_bytes(), pp.M = pq_m, pp.span = 0;
    HzProgram g = hz_prog_create();
    const size_t qk = (size_t)Q * k * 4, qb = (size_t)Q * h.dim * 4;
    int rc;
    if (filtered) {
      rc = hz_prog_add_memcpy(g, c.slot_dev, c.slot_host, kFiltBytes + qb, 0);
      if (!rc && pq) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_PQLUT, &lp, sizeof(lp), 0);
      if (!rc) rc = pq  ? hz_prog_add_kernel(g, HZ_K_SEARCH_PQSCAN, &pp, sizeof(pp), 0)
                  : bin ? hz_prog_add_kernel(g, HZ_K_SEARCH_BSCAN, &bp, sizeof(bp), 0)
                  : fp8 ? hz_prog_add_kernel(g, HZ_K_SEARCH_QSCAN, &qp, sizeof(qp), 0)
                        : hz_prog_add_kernel(g, HZ_K_SEARCH_FSCAN, &f, sizeof(f), 0);
    } else {
      rc = hz_prog_add_memcpy(g, c.q_dev, c.q_host, qb, 0);
      if (!rc) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_SCAN, &p, sizeof(p), 0);
    }
    if (!rc) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_MERGE, &p, sizeof(p), 0);
    if (!rc && R) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_RESCORE, &rp, sizeof(rp), 0);
    if (!rc) rc = hz_prog_add_memcpy(g, c.out_host, c.out_dev, qk, 0);
    if (!rc) rc = hz_prog_add_memcpy(g, c.out_host + kOutHalf, c.out_dev + kOutHalf, qk, 0);
    if (rc) {
      hz_prog_destroy(g);
      return nullptr;
    }
    c.progs[key] = g;
    return g;
  }

  // The candidate scratch of the neighbours and bulk-search programs for (n, k) (the caller holds c.mu): one too
  // small is replaced, and with it the context's programs of both sorts, which hold its address by value.
  bool self_scratch(Ctx& c, int n, int k) {
    const uint64_t need = hz_search_self_scratch_bytes((long long)scan_rows(), n, k);
    if (!need) return false;
    if (need <= c.ncand_bytes) return true;
    for (auto it = c.progs.begin(); it != c.progs.end();) {
      if (std::get<2>(it->first) == 3 || std::get<2>(it->first) == 4) {
        hz_prog_destroy(it->second);
        it = c.progs.erase(it);
      } else {
        ++it;
      }
    }
    if (c.ncand) (void)hipFree(c.ncand);
    c.ncand = nullptr, c.ncand_bytes = 0;
    if (hipMalloc(reinterpret_cast<void**>(&c.ncand), need) != hipSuccess) return false;
    c.ncand_bytes = need;
    return true;
  }

  // The bulk-search program of (Q, k, R) (the caller holds c.mu): H2D of the queries, batch scan and merge at k = R
  // into bmid_dev, rescore of those ids against `rows` into bout_dev, D2H of the scores, the ids and stage one's scores.
  HzProgram batch_program(Ctx& c, int Q, int k, int R, bool* fresh) {
    const size_t qbytes = (size_t)HZ_INDEX_SELF_MAX_Q * h.dim * 4;
    if (!c.bq_host) {
      bool ok = hipHostMalloc(reinterpret_cast<void**>(&c.bq_host), qbytes, hipHostMallocDefault) == hipSuccess;
      ok = ok && hipHostMalloc(reinterpret_cast<void**>(&c.bout_host), 3 * kSelfOutHalf, hipHostMallocDefault) == hipSuccess;
      ok = ok && hipMalloc(reinterpret_cast<void**>(&c.bq_dev), qbytes) == hipSuccess;
      ok = ok && hipMalloc(reinterpret_cast<void**>(&c.bmid_dev), 2 * kSelfOutHalf) == hipSuccess;
      ok = ok && hipMalloc(reinterpret_cast<void**>(&c.bout_dev), 2 * kSelfOutHalf) == hipSuccess;
      if (!ok) {
        if (c.bq_host) (void)hipHostFree(c.bq_host);
        if (c.bout_host) (void)hipHostFree(c.bout_host);
        if (c.bq_dev) (void)hipFree(c.bq_dev);
        if (c.bmid_dev) (void)hipFree(c.bmid_dev);
        if (c.bout_dev) (void)hipFree(c.bout_dev);
        c.bq_host = c.bq_dev = nullptr, c.bout_host = c.bmid_dev = c.bout_dev = nullptr;
        return nullptr;
      }
    }
    if (!self_scratch(c, Q, R)) return nullptr;
    const auto key = std::make_tuple(Q, k, 4, R, 0);
    auto it = c.progs.find(key);
    *fresh = it == c.progs.end();
    if (!*fresh) return it->second;
    HzSearchBatchParams p{};
    p.corpus = rows;
    p.queries = c.bq_dev;
    p.live = live;
    p.cand = c.ncand;
    p.out_score = reinterpret_cast<float*>(c.bmid_dev);
    p.out_id = reinterpret_cast<int*>(c.bmid_dev + kSelfOutHalf);
    p.live_bytes = cap / 8;
    p.cand_bytes = c.ncand_bytes;
    p.N = (int)scan_rows();
    p.D = p.ldc = (int)h.dim;
    p.Q = Q, p.k = R;
    HzSearchRescoreParams rp{};
    rp.rows = rows;
    rp.queries = c.bq_dev;
    rp.in_id = p.out_id;
    rp.out_score = reinterpret_cast<float*>(c.bout_dev);
    rp.out_id = reinterpret_cast<int*>(c.bout_dev + kSelfOutHalf);
    rp.N = p.N, rp.D = rp.ldc = p.D, rp.Q = Q, rp.R = R, rp.k = k;
    HzProgram g = hz_prog_create();
    const size_t qk = (size_t)Q * k * 4;
    int rc = hz_prog_add_memcpy(g, c.bq_dev, c.bq_host, (size_t)Q * h.dim * 4, 0);
    if (!rc) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_XSCAN, &p, sizeof(p), 0);
    if (!rc) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_MERGEN, &p, sizeof(p), 0);  // the same layout: hipzap.h
    if (!rc) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_RESCOREN, &rp, sizeof(rp), 0);
    if (!rc) rc = hz_prog_add_memcpy(g, c.bout_host, c.bout_dev, qk, 0);
    if (!rc) rc = hz_prog_add_memcpy(g, c.bout_host + kSelfOutHalf, c.bout_dev + kSelfOutHalf, qk, 0);
    if (!rc) rc = hz_prog_add_memcpy(g, c.bout_host + 2 * kSelfOutHalf, c.bmid_dev, (size_t)Q * R * 4, 0);
    if (rc) {
      hz_prog_destroy(g);
      return nullptr;
    }
    c.progs[key] = g;
    return g;
  }

  // The neighbours program of (n, k, skip_self) (the caller holds c.mu): H2D of the ids, self scan, merge, two D2H.
  // Its buffers come first, then the candidate scratch (self_scratch).
  HzProgram self_program(Ctx& c, int n, int k, int skip_self, bool* fresh) {
    if (!c.nid_host) {
      bool ok = hipHostMalloc(reinterpret_cast<void**>(&c.nid_host), (size_t)HZ_INDEX_SELF_MAX_Q * 4, hipHostMallocDefault) == hipSuccess;
      ok = ok && hipHostMalloc(reinterpret_cast<void**>(&c.nout_host), 2 * kSelfOutHalf, hipHostMallocDefault) == hipSuccess;
      ok = ok && hipMalloc(reinterpret_cast<void**>(&c.nid_dev), (size_t)HZ_INDEX_SELF_MAX_Q * 4) == hipSuccess;
      ok = ok && hipMalloc(reinterpret_cast<void**>(&c.nout_dev), 2 * kSelfOutHalf) == hipSuccess;
      if (!ok) {
        if (c.nid_host) (void)hipHostFree(c.nid_host);
        if (c.nout_host) (void)hipHostFree(c.nout_host);
        if (c.nid_dev) (void)hipFree(c.nid_dev);
        if (c.nout_dev) (void)hipFree(c.nout_dev);
        c.nid_host = c.nid_dev = nullptr, c.nout_host = c.nout_dev = nullptr;
        return nullptr;
      }
    }
    if (!self_scratch(c, n, k)) return nullptr;
    const auto key = std::make_tuple(n, k, 3, skip_self, 0);
    auto it = c.progs.find(key);
    *fresh = it == c.progs.end();
    if (!*fresh) return it->second;
    HzSearchSelfParams p{};
    p.corpus = rows;
    p.qid = c.nid_dev;
    p.live = live;
    p.cand = c.ncand;
    p.out_score = reinterpret_cast<float*>(c.nout_dev);
    p.out_id = reinterpret_cast<int*>(c.nout_dev + kSelfOutHalf);
    p.live_bytes = cap / 8;
    p.cand_bytes = c.ncand_bytes;
    p.N = (int)scan_rows();
    p.D = p.ldc = (int)h.dim;
    p.Q = n, p.k = k, p.skip_self = skip_self;
    HzProgram g = hz_prog_create();
    const size_t nk = (size_t)n * k * 4;
    int rc = hz_prog_add_memcpy(g, c.nid_dev, c.nid_host, (size_t)n * 4, 0);
    if (!rc) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_MSCAN, &p, sizeof(p), 0);
    if (!rc) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_MERGEN, &p, sizeof(p), 0);
    if (!rc) rc = hz_prog_add_memcpy(g, c.nout_host, c.nout_dev, nk, 0);
    if (!rc) rc = hz_prog_add_memcpy(g, c.nout_host + kSelfOutHalf, c.nout_dev + kSelfOutHalf, nk, 0);
    if (rc) {
      hz_prog_destroy(g);
      return nullptr;
    }
    c.progs[key] = g;
    return g;
  }

  // The IVF programs (the caller holds c.mu). probes_only: H2D of the queries, scan + merge over the centroids
  // at k = nprobe, D2H of the list ids. Else the search of (Q, k) over nprobe lists, 0 for every list; R > 0 (an
  // index with rescore rows): the list scan and its merge run at k = R into mid_dev and the rescore writes the k
  // results from the rows held by external id.
  HzProgram ivf_program(Ctx& c, int Q, int k, int nprobe, int R, bool probes_only, bool* fresh) {
    const auto key = probes_only ? std::make_tuple(Q, nprobe, 2, 0, 0) : std::make_tuple(Q, k, 1, R, nprobe);
    auto it = c.progs.find(key);
    *fresh = it == c.progs.end();
    if (!*fresh) return it->second;
    HzSearchParams cp{};  // the coarse stage: the centroids are a small bf16 corpus
    cp.corpus = centroids;
    cp.queries = c.q_dev;
    cp.cand = c.ccand;
    cp.out_score = reinterpret_cast<float*>(c.probe_dev);
    cp.out_id = reinterpret_cast<int*>(c.probe_dev + kOutHalf);
    cp.N = nlist, cp.D = cp.ldc = (int)h.dim, cp.Q = Q, cp.k = nprobe;
    cp.cand_bytes = c.ccand_bytes;
    HzSearchListParams lp{};
    HzSearchParams& p = lp.f.s;
    p.corpus = rows;
    p.queries = c.q_dev;
    p.cand = c.cand;
    char* stage1 = R ? c.mid_dev : c.out_dev;
    p.out_score = reinterpret_cast<float*>(stage1);
    p.out_id = reinterpret_cast<int*>(stage1 + kOutHalf);
    p.N = (int)count, p.D = p.ldc = (int)h.dim, p.Q = Q, p.k = R ? R : k;
    HzSearchRescoreParams rp{};  // stage one's ids are external ids: the rescore rows are held by id
    rp.rows = rrows_dev;
    rp.queries = c.q_dev;
    rp.in_id = p.out_id;
    rp.out_score = reinterpret_cast<float*>(c.out_dev);
    rp.out_id = reinterpret_cast<int*>(c.out_dev + kOutHalf);
    rp.N = (int)n_ext, rp.D = rp.ldc = p.D, rp.Q = Q, rp.R = R, rp.k = k;
    p.cand_bytes = c.cand_bytes;
    lp.f.live = live;
    lp.f.tags = tags;
    lp.f.filt = reinterpret_cast<const unsigned*>(c.slot_dev);
    lp.f.live_bytes = cap / 8;
    const int ntile = (int)(count / kTile);
    lp.probes = nprobe ? cp.out_id : nullptr;
    lp.list_off = ivf_tables;
    lp.list_tiles = ivf_tables + nlist + 1;
    lp.rowid = lp.list_tiles + ntile;
    lp.nlist = nlist, lp.nprobe = nprobe;
    lp.P = ntile;
    if (nprobe) {  // the most tiles nprobe lists can hold
      lp.P = 0;
      for (int i = 0; i < nprobe && i < (int)tiles_desc.size(); ++i) lp.P += tiles_desc[i];
    }
    HzSearchParams mp = p;  // the merge over the P candidate lists
    mp.N = lp.P * (int)kTile;
    HzSearchQuantListParams qlp{};
    qlp.l = lp;
    qlp.scales = scales;
    HzProgram g = hz_prog_create();
    const size_t qk = (size_t)Q * k * 4, qb = (size_t)Q * h.dim * 4;
    int rc = probes_only ? hz_prog_add_memcpy(g, c.q_dev, c.q_host, qb, 0)
                         : hz_prog_add_memcpy(g, c.slot_dev, c.slot_host, kFiltBytes + qb, 0);
    if (!rc && nprobe) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_SCAN, &cp, sizeof(cp), 0);
    if (!rc && nprobe) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_MERGE, &cp, sizeof(cp), 0);
    if (probes_only) {
      if (!rc) rc = hz_prog_add_memcpy(g, c.out_host + kOutHalf, c.probe_dev + kOutHalf, (size_t)Q * nprobe * 4, 0);
    } else {
      if (!rc) rc = fp8 ? hz_prog_add_kernel(g, HZ_K_SEARCH_QLSCAN, &qlp, sizeof(qlp), 0)
                        : hz_prog_add_kernel(g, HZ_K_SEARCH_LSCAN, &lp, sizeof(lp), 0);
      if (!rc) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_MERGE, &mp, sizeof(mp), 0);
      if (!rc && R) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_RESCORE, &rp, sizeof(rp), 0);
      if (!rc) rc = hz_prog_add_memcpy(g, c.out_host, c.out_dev, qk, 0);
      if (!rc) rc = hz_prog_add_memcpy(g, c.out_host + kOutHalf, c.out_dev + kOutHalf, qk, 0);
    }
    if (rc) {
      hz_prog_destroy(g);
      return nullptr;
    }
    c.progs[key] = g;
    return g;
  }

  // device buffers for `new_cap` rows (whole tiles); the first `count` rows, their tags and the bitmap move
  // over (device-to-device on `st`, synchronised), the rest is dead: zero bitmap, zero tags, rows untouched.
  // The caller holds every context's mutex (or the index is not yet shared) and drops the programs.
  int reallocate(uint64_t new_cap, hipStream_t st) {
    unsigned short* nrows = nullptr;
    unsigned *nlive = nullptr, *ntags = nullptr;
    float* nscales = nullptr;
    unsigned short *nrr = nullptr, *nrr_dev = nullptr;
    const uint64_t cand_bytes = hz_search_scratch_bytes((long long)new_cap, HZ_SEARCH_MAX_Q, HZ_SEARCH_MAX_K);
    if (!cand_bytes) return -21;  // 2^31 rows and above
    std::vector<unsigned long long*> ncand(ctx.size(), nullptr);
    bool ok = hipMalloc(reinterpret_cast<void**>(&nrows), new_cap * rowb()) == hipSuccess;
    if (fp8) ok = ok && hipMalloc(reinterpret_cast<void**>(&nscales), new_cap * 4) == hipSuccess;
    if (rescore) ok = ok && alloc_rescore(rescore_rows(new_cap) * h.dim * 2, &nrr, &nrr_dev);
    ok = ok && hipMalloc(reinterpret_cast<void**>(&nlive), new_cap / 8) == hipSuccess;
    ok = ok && hipMalloc(reinterpret_cast<void**>(&ntags), new_cap * 4) == hipSuccess;
    for (size_t i = 0; ok && i < ctx.size(); ++i)
      ok = hipMalloc(reinterpret_cast<void**>(&ncand[i]), cand_bytes) == hipSuccess;
    ok = ok && hipMemsetAsync(nlive, 0, new_cap / 8, st) == hipSuccess;
    ok = ok && hipMemsetAsync(ntags, 0, new_cap * 4, st) == hipSuccess;
    if (ok && rows) {
      ok = hipMemcpyAsync(nrows, rows, count * rowb(), hipMemcpyDeviceToDevice, st) == hipSuccess;
      if (fp8) ok = ok && hipMemcpyAsync(nscales, scales, count * 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
      if (rescore && !rescore_host)
        ok = ok && hipMemcpyAsync(nrr, rrows, count * h.dim * 2, hipMemcpyDeviceToDevice, st) == hipSuccess;
      ok = ok && hipMemcpyAsync(ntags, tags, count * 4, hipMemcpyDeviceToDevice, st) == hipSuccess;
      ok = ok && hipMemcpyAsync(nlive, live, round_up(count, 32) / 8, hipMemcpyDeviceToDevice, st) == hipSuccess;
    }
    ok = ok && hipStreamSynchronize(st) == hipSuccess;
    if (!ok) {
      (void)hipFree(nrows), (void)hipFree(nlive), (void)hipFree(ntags), (void)hipFree(nscales);
      free_rescore(nrr);
      for (auto* p : ncand) (void)hipFree(p);
      return -22;
    }
    // a host block is copied by the CPU: no search runs (the caller holds the contexts) and the stream is idle
    if (rescore && rescore_host && rrows) std::memcpy(nrr, rrows, count * h.dim * 2);
    (void)hipFree(rows), (void)hipFree(live), (void)hipFree(tags), (void)hipFree(scales);
    free_rescore(rrows);
    rows = nrows, live = nlive, tags = ntags, scales = nscales, cap = new_cap;
    rrows = nrr, rrows_dev = nrr_dev;
    for (size_t i = 0; i < ctx.size(); ++i) {
      (void)hipFree(ctx[i]->cand);
      ctx[i]->cand = ncand[i];
      ctx[i]->cand_bytes = cand_bytes;
    }
    live_host.resize(cap / 32, 0u);
    tags_host.resize(cap, 0u);
    return 0;
  }
};

// every context's mutex, in index order: no search runs, and none starts, while a mutation holds them
struct AllLocked {
  std::vector<std::unique_lock<std::mutex>> lk;
  explicit AllLocked(Index& x) {
    for (auto& c : x.ctx) lk.emplace_back(c->mu);
  }
};

// host words [w0, w1) of a mirror -> the device buffer, on `st`
int push_words(unsigned* dev, const std::vector<uint32_t>& host, uint64_t w0, uint64_t w1, hipStream_t st) {
  if (w1 <= w0) return 0;
  return (int)hipMemcpyAsync(dev + w0, host.data() + w0, (w1 - w0) * 4, hipMemcpyHostToDevice, st);
}

}  // namespace

extern "C" {

const char* hz_index_last_error(void) { return g_err.c_str(); }

void* hz_index_open3(const char* path, int device, int nctx, long long reserve_rows, int rescore_host) {
  g_err.clear();
  if (nctx <= 0) nctx = 2;
  if (nctx > 16) return fail("index: at most 16 contexts");
  if (reserve_rows < 0 || reserve_rows >= (1ll << 31)) return fail("index: reserve must be in 0..2^31-1 rows");
  const int fd = open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) return fail(std::string("index: cannot open ") + path);
  HzIndexHeader h{};
  struct stat sb {};
  bool got = fstat(fd, &sb) == 0 && pread(fd, &h, sizeof(h), 0) == (ssize_t)sizeof(h);
  std::string js;
  if (got && std::memcmp(h.magic, HZ_INDEX_MAGIC, 8) == 0 && h.version >= 2 && h.version <= 11 && h.json_len < (1u << 30)) {
    js.resize(h.json_len);
    got = pread(fd, &js[0], h.json_len, sizeof(h)) == (ssize_t)h.json_len;
  }
  close(fd);
  if (!got || std::memcmp(h.magic, HZ_INDEX_MAGIC, 8) != 0) return fail(std::string("index: not a .hzidx file: ") + path);
  if (h.version < 1 || h.version > 11) return fail("index: unknown format version " + std::to_string(h.version));
  const bool ivf = h.version >= 5 && h.version <= 7;
  const bool fp8 = h.version == 3 || h.version == 4 || h.version == 6 || h.version == 7;
  const bool bin = h.version == 8 || h.version == 9;
  const bool pq = h.version == 10 || h.version == 11;
  const bool rescore = h.version == 4 || h.version == 7 || h.version == 9 || h.version == 11;
  const std::string vname = "version-" + std::to_string(h.version);
  if (fp8 != (js.rfind("\"dtype\": \"fp8_e4m3\"") != std::string::npos))
    return fail("index: the dtype of the JSON header disagrees with a " + vname + " file");
  if (bin != (js.rfind("\"dtype\": \"bin_sign\"") != std::string::npos))
    return fail("index: the dtype of the JSON header disagrees with a " + vname + " file");
  if (pq != (js.rfind("\"dtype\": \"pq8\"") != std::string::npos))
    return fail("index: the dtype of the JSON header disagrees with a " + vname + " file");
  if (!ivf && js.rfind("\"ivf\": {") != std::string::npos)
    return fail("index: an ivf block in a " + vname + " file (it belongs to versions 5, 6 and 7)");
  uint64_t pq_u[4] = {0, 0, 0, 0};  // m, ksub, dsub, codebook_off
  if (pq) {
    static const char* keys[4] = {"m", "ksub", "dsub", "codebook_off"};
    if (js.rfind("\"pq\": {") == std::string::npos) return fail("index: a " + vname + " file without a pq block");
    for (int i = 0; i < 4; ++i)
      if (!json_u64(js, keys[i], &pq_u[i], true)) return fail(std::string("index: the pq block lacks ") + keys[i]);
    if (pq_u[1] != 256) return fail("index: pq ksub must be 256, got " + std::to_string(pq_u[1]));
    const uint64_t m = pq_u[0];
    if (m < 16 || m > HZ_SEARCH_PQ_MAX_M || m % 16 || h.dim < 1 || h.dim > 2048 || h.dim % m || h.dim / m > HZ_SEARCH_PQ_MAX_DSUB ||
        pq_u[2] != h.dim / m)
      return fail("index: pq needs m % 16 == 0, 16 <= m <= 96, dim % m == 0, dsub = dim / m in 1..64 and dim <= 2048, got m = " +
                  std::to_string(m) + ", dsub = " + std::to_string(pq_u[2]) + ", dim = " + std::to_string(h.dim));
  } else if (js.rfind("\"pq\": {") != std::string::npos) {
    return fail("index: a pq block in a " + vname + " file (it belongs to versions 10 and 11)");
  }
  if (fp8 && (h.dim < 16 || h.dim % 16 || h.dim > 2048))
    return fail("index: dim of an fp8 index must be a multiple of 16 in 16..2048");
  if (bin && (h.dim < 128 || h.dim % 128 || h.dim > 2048))
    return fail("index: dim of a binary index must be a multiple of 128 in 128..2048");
  if (!pq && (h.dim < 8 || h.dim % 8 || h.dim > 2048)) return fail("index: dim must be a multiple of 8 in 8..2048");
  if (h.count < 1 || h.count >= (1ull << 31)) return fail("index: count must be in 1..2^31-1");
  if (h.metric > HZ_INDEX_IP) return fail("index: unknown metric");
  // an IVF file's blocks hold `capacity` stored rows (whole tiles); from here on h.count is that number
  const uint64_t n_ext = h.count;
  uint64_t ivf_u[6] = {0, 0, 0, 0, 0, 0};  // nlist, nprobe, then the four offsets
  if (ivf) {
    static const char* keys[6] = {"nlist", "nprobe", "centroids_off", "list_off_off", "list_tiles_off", "rowid_off"};
    uint64_t stored = 0;
    if (js.rfind("\"ivf\"") == std::string::npos || !json_u64(js, "capacity", &stored, true))
      return fail("index: a " + vname + " file without an ivf block or capacity");
    for (int i = 0; i < 6; ++i)
      if (!json_u64(js, keys[i], &ivf_u[i], true)) return fail(std::string("index: the ivf block lacks ") + keys[i]);
    if (stored < n_ext || stored % kTile || stored >= (1ull << 31))
      return fail("index: capacity of an IVF index must be whole tiles holding count rows");
    if (ivf_u[0] < 1 || ivf_u[0] > std::min<uint64_t>(n_ext, 65536) || ivf_u[1] < 1 ||
        ivf_u[1] > std::min<uint64_t>(ivf_u[0], HZ_SEARCH_MAX_K))
      return fail("index: ivf nlist / nprobe out of range");
    h.count = stored;
  }
  const uint64_t bytes = pq ? h.count * pq_u[0] : bin ? h.count * (h.dim / 8) : h.count * h.dim * (fp8 ? 1 : 2),
                 fsize = (uint64_t)sb.st_size;
  if (h.data_off % 4096 || h.data_off < sizeof(h) + h.json_len || h.data_off + bytes > fsize)
    return fail("index: row block outside the file");
  uint64_t tags_off = 0, live_off = 0;
  const uint64_t tag_bytes = h.count * 4, live_bytes = round_up(h.count, 32) / 8;
  uint64_t scales_off = 0, after_rows = h.data_off + bytes;
  bool blocks = h.version == 2 || ivf;  // tags and a bitmap in the file
  if (fp8) {
    if (!json_u64(js, "scales_off", &scales_off, true)) return fail("index: a " + vname + " file without scales_off");
    if (scales_off % 4096 || scales_off < after_rows || scales_off > fsize || h.count * 4 > fsize - scales_off)
      return fail("index: scales block outside the file");
    after_rows = scales_off + h.count * 4;
  }
  const uint64_t cb_off = pq_u[3], cb_len = pq ? 256ull * h.dim * 4 : 0;
  if (pq) {
    if (cb_off % 4096 || cb_off < after_rows || cb_off > fsize || cb_len > fsize - cb_off)
      return fail("index: codebook block unaligned, overlapping the rows or outside the file");
    after_rows = cb_off + cb_len;
  }
  if (fp8 || bin || pq) {
    const bool t = json_u64(js, "tags_off", &tags_off, true), l = json_u64(js, "live_off", &live_off, true);
    if (t != l) return fail("index: a " + vname + " file with only one of tags_off / live_off");
    if (ivf && !t) return fail("index: a " + vname + " file without tags_off / live_off");
    blocks = t;
  }
  uint64_t rescore_off = 0;
  const uint64_t rescore_len = n_ext * h.dim * 2;  // [count][dim]: an IVF file holds them by external id
  if (fp8 || bin || pq) {
    const bool off = json_u64(js, "rescore_off", &rescore_off, true);
    const bool key = js.rfind("\"rescore\": \"bf16\"") != std::string::npos;
    if (rescore && !(off && key)) return fail("index: a " + vname + " file without rescore / rescore_off");
    if (!rescore && (off || key)) return fail("index: a " + vname + " file with rescore keys (they belong to versions " + (pq ? "4, 7, 9 and 11" : bin ? "4, 7 and 9" : "4 and 7") + ")");
  }
  if (blocks) {
    if (!fp8 && !bin && !pq && (!json_u64(js, "tags_off", &tags_off) || !json_u64(js, "live_off", &live_off)))
      return fail("index: a version-2 file without tags_off / live_off");
    if (tags_off % 4096 || live_off % 4096 || tags_off < after_rows || live_off < after_rows ||
        tags_off > fsize || tag_bytes > fsize - tags_off || live_off > fsize || live_bytes > fsize - live_off)
      return fail("index: tags or live block outside the file");
    after_rows = std::max(after_rows, std::max(tags_off + tag_bytes, live_off + live_bytes));
  }
  // the IVF tables: read, and checked before anything reaches the device -- the list scan trusts them
  const uint64_t ntile = h.count / kTile;
  std::vector<unsigned short> cent_host;
  std::vector<int32_t> tables_host;  // list_off [nlist + 1], list_tiles [ntile], rowid [h.count]
  std::vector<int32_t> pos_of;
  std::vector<int> tiles_desc;
  if (ivf) {
    const uint64_t nlist = ivf_u[0];
    const uint64_t len[4] = {nlist * h.dim * 2, (nlist + 1) * 4, ntile * 4, h.count * 4};
    cent_host.resize(nlist * h.dim);
    tables_host.resize(nlist + 1 + ntile + h.count);
    char* dst[4] = {reinterpret_cast<char*>(cent_host.data()), reinterpret_cast<char*>(tables_host.data()),
                    reinterpret_cast<char*>(tables_host.data() + nlist + 1),
                    reinterpret_cast<char*>(tables_host.data() + nlist + 1 + ntile)};
    const int tfd = open(path, O_RDONLY | O_CLOEXEC);
    bool ok = tfd >= 0;
    for (int i = 0; ok && i < 4; ++i) {
      const uint64_t off = ivf_u[2 + i];
      if (off % 4096 || off < after_rows || off > fsize || len[i] > fsize - off) {
        close(tfd);
        return fail("index: an ivf block is unaligned, overlaps another block or lies outside the file");
      }
      after_rows = off + len[i];
      uint64_t done = 0;
      while (done < len[i]) {
        const ssize_t n = pread(tfd, dst[i] + done, len[i] - done, (off_t)(off + done));
        if (n <= 0) break;
        done += (uint64_t)n;
      }
      ok = done == len[i];
    }
    if (tfd >= 0) close(tfd);
    if (!ok) return fail("index: cannot read the ivf blocks");
    const int32_t* loff = tables_host.data();
    const int32_t* ltiles = loff + nlist + 1;
    const int32_t* rowid = ltiles + ntile;
    if (loff[0] != 0 || (uint64_t)loff[nlist] != ntile) return fail("index: ivf list_off does not rise from 0 to the tile count");
    for (uint64_t l = 0; l < nlist; ++l) {
      if (loff[l + 1] < loff[l]) return fail("index: ivf list_off does not rise from 0 to the tile count");
      tiles_desc.push_back(loff[l + 1] - loff[l]);
    }
    std::sort(tiles_desc.begin(), tiles_desc.end(), std::greater<int>());
    std::vector<char> seen(ntile, 0);
    for (uint64_t i = 0; i < ntile; ++i) {
      if (ltiles[i] < 0 || (uint64_t)ltiles[i] >= ntile || seen[ltiles[i]])
        return fail("index: ivf list_tiles is not a permutation of the tile ids");
      seen[ltiles[i]] = 1;
    }
    pos_of.assign(n_ext, -1);
    uint64_t real = 0;
    for (uint64_t r = 0; r < h.count; ++r) {
      if (rowid[r] == -1) continue;
      if (rowid[r] < 0 || (uint64_t)rowid[r] >= n_ext || pos_of[rowid[r]] != -1)
        return fail("index: ivf rowid is not a permutation of the ids over the stored rows");
      pos_of[rowid[r]] = (int32_t)r, ++real;
    }
    if (real != n_ext) return fail("index: ivf rowid is not a permutation of the ids over the stored rows");
  }
  // the rescore block lies after every other block (the ivf tables included)
  if (rescore && (rescore_off % 4096 || rescore_off < after_rows || rescore_off > fsize || rescore_len > fsize - rescore_off))
    return fail("index: rescore block unaligned, overlapping another block or outside the file");
  if (hipSetDevice(device) != hipSuccess) return fail("index: hipSetDevice failed");
  auto idx = std::make_unique<Index>();
  idx->device = device;
  idx->h = h;
  idx->count = h.count;
  idx->fp8 = fp8;
  idx->bin = bin;
  idx->pq = pq;
  idx->pq_m = (int)pq_u[0];
  idx->rescore = rescore;
  idx->rescore_host = rescore && rescore_host != 0;
  idx->ivf = ivf;
  idx->n_ext = n_ext;
  idx->nlist = (int)ivf_u[0], idx->nprobe_default = (int)ivf_u[1];
  idx->pos_of = std::move(pos_of);
  idx->tiles_desc = std::move(tiles_desc);
  if (hz_search_code_warm()) return fail("index: device code load failed");
  for (int i = 0; i < nctx; ++i) {
    auto c = std::make_unique<Ctx>();
    const size_t sb_ = kFiltBytes + (size_t)HZ_SEARCH_MAX_Q * h.dim * 4;
    bool ok = hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void**>(&c->slot_host), sb_, hipHostMallocDefault) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void**>(&c->out_host), 2 * kOutHalf, hipHostMallocDefault) == hipSuccess;
    ok = ok && hipMalloc(reinterpret_cast<void**>(&c->slot_dev), sb_) == hipSuccess;
    ok = ok && hipMalloc(reinterpret_cast<void**>(&c->out_dev), 2 * kOutHalf) == hipSuccess;
    if (rescore) ok = ok && hipMalloc(reinterpret_cast<void**>(&c->mid_dev), 2 * kOutHalf) == hipSuccess;
    if (pq) ok = ok && hipMalloc(reinterpret_cast<void**>(&c->lut), idx->lut_bytes()) == hipSuccess;
    if (ivf) {
      c->ccand_bytes = hz_search_scratch_bytes((long long)ivf_u[0], HZ_SEARCH_MAX_Q, HZ_SEARCH_MAX_K);
      ok = ok && hipMalloc(reinterpret_cast<void**>(&c->probe_dev), 2 * kOutHalf) == hipSuccess;
      ok = ok && hipMalloc(reinterpret_cast<void**>(&c->ccand), c->ccand_bytes) == hipSuccess;
    }
    if (ok) {
      std::memset(c->slot_host, 0, sb_);
      c->q_host = reinterpret_cast<float*>(c->slot_host + kFiltBytes);
      c->q_dev = reinterpret_cast<float*>(c->slot_dev + kFiltBytes);
    }
    idx->ctx.push_back(std::move(c));
    if (!ok) return fail("index: context allocation failed");
  }
  hipStream_t st = idx->ctx[0]->st;
  const uint64_t cap = round_up(std::max<uint64_t>(h.count, (uint64_t)reserve_rows), kTile);
  if (idx->reallocate(cap, st)) return fail("index: device allocation failed");
  const uint64_t words = live_bytes / 4;
  if (blocks) {
    const uint64_t off[4] = {h.data_off, tags_off, live_off, scales_off}, len[4] = {bytes, tag_bytes, live_bytes, h.count * 4};
    void* dst[4] = {idx->rows, idx->tags, idx->live, idx->scales};
    if (hz_upload_file(path, fp8 ? 4 : 3, off, len, dst, st)) return fail(std::string("index: ") + hz_plan_last_error());
    bool ok = hipStreamSynchronize(st) == hipSuccess;
    // the mirrors come back from the device copy (one read of the file); bits past the count are cleared
    ok = ok && hipMemcpy(idx->tags_host.data(), idx->tags, tag_bytes, hipMemcpyDeviceToHost) == hipSuccess;
    ok = ok && hipMemcpy(idx->live_host.data(), idx->live, live_bytes, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) return fail("index: upload failed");
    if (h.count % 32) idx->live_host[words - 1] &= (1u << (h.count % 32)) - 1u;
    if (push_words(idx->live, idx->live_host, words - 1, words, st) || hipStreamSynchronize(st) != hipSuccess)
      return fail("index: upload failed");
    for (uint64_t w = 0; w < words; ++w) idx->live_count += (uint64_t)__builtin_popcount(idx->live_host[w]);
    idx->has_tags = true;
    idx->mutated = idx->live_count < h.count;
  } else {
    const uint64_t off[2] = {h.data_off, scales_off}, len[2] = {bytes, h.count * 4};
    void* dst[2] = {idx->rows, idx->scales};
    if (hz_upload_file(path, fp8 ? 2 : 1, off, len, dst, st)) return fail(std::string("index: ") + hz_plan_last_error());
    for (uint64_t r = 0; r < h.count; ++r) idx->live_host[r >> 5] |= 1u << (r & 31);
    idx->live_count = h.count;
    if (push_words(idx->live, idx->live_host, 0, words, st) || hipStreamSynchronize(st) != hipSuccess)
      return fail("index: upload failed");
  }
  if (ivf) {
    bool ok = hipMalloc(reinterpret_cast<void**>(&idx->centroids), cent_host.size() * 2) == hipSuccess;
    ok = ok && hipMalloc(reinterpret_cast<void**>(&idx->ivf_tables), tables_host.size() * 4) == hipSuccess;
    ok = ok && hipMemcpy(idx->centroids, cent_host.data(), cent_host.size() * 2, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && hipMemcpy(idx->ivf_tables, tables_host.data(), tables_host.size() * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) return fail("index: ivf upload failed");
    // a padding row is dead whatever the file's bitmap says: the list scan never loads it
    const int32_t* rowid = tables_host.data() + idx->nlist + 1 + ntile;
    uint64_t cleared = 0;
    for (uint64_t r = 0; r < h.count; ++r)
      if (rowid[r] < 0 && (idx->live_host[r >> 5] >> (r & 31) & 1u)) idx->live_host[r >> 5] &= ~(1u << (r & 31)), ++cleared;
    if (cleared) {
      idx->live_count -= cleared;
      if (push_words(idx->live, idx->live_host, 0, words, st) || hipStreamSynchronize(st) != hipSuccess)
        return fail("index: upload failed");
    }
  }
  if (pq) {  // the codebook: file -> host mirror -> device
    idx->codebook_host.resize(cb_len / 4);
    const int cfd = open(path, O_RDONLY | O_CLOEXEC);
    uint64_t done = 0;
    while (cfd >= 0 && done < cb_len) {
      const ssize_t n = pread(cfd, reinterpret_cast<char*>(idx->codebook_host.data()) + done, cb_len - done, (off_t)(cb_off + done));
      if (n <= 0) break;
      done += (uint64_t)n;
    }
    if (cfd >= 0) close(cfd);
    if (done != cb_len) return fail("index: cannot read the codebook block");
    if (hipMalloc(reinterpret_cast<void**>(&idx->codebook), cb_len) != hipSuccess ||
        hipMemcpy(idx->codebook, idx->codebook_host.data(), cb_len, hipMemcpyHostToDevice) != hipSuccess)
      return fail("index: codebook upload failed");
  }
  if (rescore && idx->rescore_host) {  // the file's block straight into the pinned rows
    const int rfd = open(path, O_RDONLY | O_CLOEXEC);
    uint64_t done = 0;
    while (rfd >= 0 && done < rescore_len) {
      const ssize_t n = pread(rfd, reinterpret_cast<char*>(idx->rrows) + done, rescore_len - done, (off_t)(rescore_off + done));
      if (n <= 0) break;
      done += (uint64_t)n;
    }
    if (rfd >= 0) close(rfd);
    if (done != rescore_len) return fail("index: cannot read the rescore block");
  } else if (rescore) {
    void* dst[1] = {idx->rrows};
    if (hz_upload_file(path, 1, &rescore_off, &rescore_len, dst, st) || hipStreamSynchronize(st) != hipSuccess)
      return fail(std::string("index: rescore upload failed: ") + hz_plan_last_error());
  }
  return idx.release();
}

void* hz_index_open2(const char* path, int device, int nctx, long long reserve_rows) {
  return hz_index_open3(path, device, nctx, reserve_rows, 0);
}

void* hz_index_open(const char* path, int device, int nctx) { return hz_index_open2(path, device, nctx, 0); }

int hz_index_describe(void* h, uint64_t* out) {
  if (!h || !out) return -1;
  Index* x = static_cast<Index*>(h);
  AllLocked all(*x);
  uint64_t progs = 0, dev = x->row_bytes() + x->cap / 8 + x->cap * 4 + (x->fp8 ? x->cap * 4 : 0);
  if (!x->rescore_host) dev += x->rescore_bytes();
  dev += x->codebook_bytes();
  for (auto& c : x->ctx) {
    progs += c->progs.size();
    dev += x->lut_bytes();
    dev += c->cand_bytes + kFiltBytes + (uint64_t)HZ_SEARCH_MAX_Q * x->h.dim * 4 + 2 * kOutHalf + (c->mid_dev ? 2 * kOutHalf : 0);
    dev += c->ncand_bytes + (c->nid_dev ? (uint64_t)HZ_INDEX_SELF_MAX_Q * 4 + 2 * kSelfOutHalf : 0);  // neighbours, once used
    dev += c->bq_dev ? (uint64_t)HZ_INDEX_SELF_MAX_Q * x->h.dim * 4 + 4 * kSelfOutHalf : 0;  // bulk search, once used
    for (const uint64_t b : c->cl_bytes) dev += b;  // clustering, once used
  }
  const uint64_t v[8] = {x->count, x->h.dim, x->h.metric, x->ctx.size(), (uint64_t)hz_search_tile_rows(), progs, dev, x->cap};
  std::memcpy(out, v, sizeof(v));
  return 0;
}

int hz_index_describe2(void* h, uint64_t* out) {
  if (!h || !out) return -1;
  Index* x = static_cast<Index*>(h);
  AllLocked all(*x);
  const uint64_t v[8] = {x->cap, x->live_count, x->has_tags, x->mutated, x->scan_rows(), x->pq ? 3u : x->bin ? 2u : x->fp8 ? 1u : 0u,
                       x->rescore ? 1u : 0u, x->rescore_host ? 1u : 0u};
  std::memcpy(out, v, sizeof(v));
  return 0;
}

int hz_index_describe3(void* h, uint64_t* out) {
  if (!h || !out) return -1;
  Index* x = static_cast<Index*>(h);
  AllLocked all(*x);
  const uint64_t v[8] = {x->ivf ? 1u : 0u, (uint64_t)x->nlist, (uint64_t)x->nprobe_default, x->ivf ? x->count / kTile : 0,
                         x->ivf ? x->n_ext : x->count, x->h.version, 0, 0};
  std::memcpy(out, v, sizeof(v));
  return 0;
}

int hz_index_describe4(void* h, uint64_t* out) {
  if (!h || !out) return -1;
  Index* x = static_cast<Index*>(h);
  AllLocked all(*x);
  uint64_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (x->pq) {
    v[0] = (uint64_t)x->pq_m, v[1] = x->h.dim / (uint64_t)x->pq_m, v[2] = x->codebook_bytes(), v[3] = x->lut_bytes();
    if (hipSetDevice(x->device) == hipSuccess) v[4] = (uint64_t)hz_search_pq_span((long long)x->scan_rows(), 1, x->pq_m);
  }
  std::memcpy(out, v, sizeof(v));
  return 0;
}

int hz_index_search3(void* h, int ctx, const float* queries, const unsigned* filt, int Q, int k, int refine, int nprobe,
                     float* out_score, int* out_id) {
  Index* x = static_cast<Index*>(h);
  if (!x || !queries || !out_score || !out_id) return -1;
  if (ctx < 0 || ctx >= (int)x->ctx.size()) return -9;
  if (Q < 1 || Q > HZ_SEARCH_MAX_Q) return -4;
  if (k < 1 || k > HZ_SEARCH_MAX_K) return -5;
  if (x->ivf && refine && !x->rescore) {
    g_err = "index: an IVF index has no rescore rows unless it is a version-7 file";
    return -34;
  }
  if (refine && !x->rescore) {
    g_err = std::string("index: refine needs rescore rows (") + (x->pq ? "a version-11 file" : x->bin ? "a version-9 file" : "a version-4 or version-7 file") +
            "), the index holds " + x->dtype_name() + " rows only";
    return -27;
  }
  if (refine && (refine < k || refine > HZ_SEARCH_MAX_K)) {
    g_err = "index: refine must be 0 or in k.." + std::to_string(HZ_SEARCH_MAX_K) + ", got " + std::to_string(refine);
    return -28;
  }
  if (nprobe && !x->ivf) {
    g_err = "index: nprobe needs an IVF index (a version-5, 6 or 7 file)";
    if (x->bin || x->pq) g_err += std::string(", this one is ") + x->quant_name() + " of version " + std::to_string(x->h.version);
    return -34;
  }
  if (x->ivf && (nprobe < 0 || (nprobe > HZ_SEARCH_MAX_K && nprobe < x->nlist))) {
    g_err = "index: nprobe must be 0 (every list) or in 1..min(nlist, " + std::to_string(HZ_SEARCH_MAX_K) + "), got " +
            std::to_string(nprobe);
    return -34;
  }
  if (x->ivf && nprobe >= x->nlist) nprobe = 0;  // every list: no coarse stage
  Ctx& c = *x->ctx[ctx];
  std::lock_guard<std::mutex> lk(c.mu);
  if (hipSetDevice(x->device) != hipSuccess) return -10;
  const bool filtered = x->fp8 || x->bin || x->pq || x->mutated || filt != nullptr || x->ivf;
  bool fresh = false;
  HzProgram g = x->ivf ? x->ivf_program(c, Q, k, nprobe, refine, false, &fresh) : x->program(c, Q, k, filtered, refine, &fresh);
  if (!g) return -11;
  std::memcpy(c.q_host, queries, (size_t)Q * x->h.dim * 4);
  if (filtered) {  // no filter: mask 0, value 0 passes every tag
    if (filt) std::memcpy(c.slot_host, filt, (size_t)Q * 8);
    else std::memset(c.slot_host, 0, (size_t)Q * 8);
  }
  // first use: one eager run (it also answers this search), then the capture for the next ones
  int rc = fresh ? hz_prog_run(g, c.st) : hz_prog_replay(g, c.st);
  if (!rc) rc = (int)hipStreamSynchronize(c.st);
  if (rc) return rc;
  std::memcpy(out_score, c.out_host, (size_t)Q * k * 4);
  std::memcpy(out_id, c.out_host + kOutHalf, (size_t)Q * k * 4);
  if (fresh) {
    rc = hz_prog_capture(g, c.st);
    if (!rc) rc = (int)hipStreamSynchronize(c.st);
  }
  return rc;
}

int hz_index_search2(void* h, int ctx, const float* queries, const unsigned* filt, int Q, int k, int refine,
                     float* out_score, int* out_id) {
  return hz_index_search3(h, ctx, queries, filt, Q, k, refine, 0, out_score, out_id);
}

int hz_index_probes(void* h, int ctx, const float* queries, int Q, int nprobe, int* out_list) {
  Index* x = static_cast<Index*>(h);
  if (!x || !queries || !out_list) return -1;
  if (ctx < 0 || ctx >= (int)x->ctx.size()) return -9;
  if (Q < 1 || Q > HZ_SEARCH_MAX_Q) return -4;
  if (!x->ivf || nprobe < 1 || nprobe > x->nlist || nprobe > HZ_SEARCH_MAX_K) {
    g_err = x->ivf ? "index: nprobe must be in 1..min(nlist, " + std::to_string(HZ_SEARCH_MAX_K) + "), got " + std::to_string(nprobe)
                   : std::string("index: probes needs an IVF index (a version-5, 6 or 7 file)") +
                         (x->bin || x->pq ? std::string(", this one is ") + x->quant_name() + " of version " + std::to_string(x->h.version)
                                          : std::string());
    return -34;
  }
  Ctx& c = *x->ctx[ctx];
  std::lock_guard<std::mutex> lk(c.mu);
  if (hipSetDevice(x->device) != hipSuccess) return -10;
  bool fresh = false;
  HzProgram g = x->ivf_program(c, Q, 0, nprobe, 0, true, &fresh);
  if (!g) return -11;
  std::memcpy(c.q_host, queries, (size_t)Q * x->h.dim * 4);
  int rc = fresh ? hz_prog_run(g, c.st) : hz_prog_replay(g, c.st);
  if (!rc) rc = (int)hipStreamSynchronize(c.st);
  if (rc) return rc;
  std::memcpy(out_list, c.out_host + kOutHalf, (size_t)Q * nprobe * 4);
  if (fresh) {
    rc = hz_prog_capture(g, c.st);
    if (!rc) rc = (int)hipStreamSynchronize(c.st);
  }
  return rc;
}

int hz_index_neighbors_max(void* h, int set) {
  Index* x = static_cast<Index*>(h);
  if (!x || set < 0 || set > HZ_INDEX_SELF_MAX_Q) return -1;
  AllLocked all(*x);
  if (set) x->self_max = set;
  return x->self_max;
}

int hz_index_neighbors(void* h, int ctx, const int* ids, int n, int k, int skip_self, float* out_score, int* out_id) {
  Index* x = static_cast<Index*>(h);
  if (!x || !ids || !out_score || !out_id) return -1;
  if (ctx < 0 || ctx >= (int)x->ctx.size()) return -9;
  if (x->fp8 || x->ivf || x->bin || x->pq) {
    g_err = std::string("index: neighbors is built for plain bf16 indexes (versions 1 and 2), this one is ") +
            (x->ivf ? (x->fp8 ? "an fp8 IVF index" : "an IVF index") : x->quant_name()) + " of version " +
            std::to_string(x->h.version);
    return -35;
  }
  if (x->h.dim % 32) {
    g_err = "index: neighbors needs dim % 32 == 0 (one MFMA step is 32 columns), got dim = " + std::to_string(x->h.dim);
    return -36;
  }
  if (k < 1 || k > HZ_SEARCH_MAX_K) {
    g_err = "index: k must be in 1.." + std::to_string(HZ_SEARCH_MAX_K) + ", got " + std::to_string(k);
    return -5;
  }
  skip_self = skip_self ? 1 : 0;
  Ctx& c = *x->ctx[ctx];
  std::lock_guard<std::mutex> lk(c.mu);  // count, the bitmap mirror and self_max change only under every context's mutex
  if (n < 1 || n > x->self_max) {
    g_err = "index: neighbors takes 1.." + std::to_string(x->self_max) + " ids a call, got " + std::to_string(n);
    return -4;
  }
  for (int i = 0; i < n; ++i) {
    if (ids[i] < 0 || (uint64_t)ids[i] >= x->count) {
      g_err = "index: id " + std::to_string(ids[i]) + " is outside [0, " + std::to_string(x->count) + ")";
      return -20;
    }
    if (!(x->live_host[(uint64_t)ids[i] >> 5] >> (ids[i] & 31) & 1u)) {
      g_err = "index: id " + std::to_string(ids[i]) + " is deleted";
      return -37;
    }
  }
  if (hipSetDevice(x->device) != hipSuccess) return -10;
  bool fresh = false;
  HzProgram g = x->self_program(c, n, k, skip_self, &fresh);
  if (!g) return -11;
  std::memcpy(c.nid_host, ids, (size_t)n * 4);
  int rc = fresh ? hz_prog_run(g, c.st) : hz_prog_replay(g, c.st);
  if (!rc) rc = (int)hipStreamSynchronize(c.st);
  if (rc) return rc;
  std::memcpy(out_score, c.nout_host, (size_t)n * k * 4);
  std::memcpy(out_id, c.nout_host + kSelfOutHalf, (size_t)n * k * 4);
  if (fresh) {
    rc = hz_prog_capture(g, c.st);
    if (!rc) rc = (int)hipStreamSynchronize(c.st);
  }
  return rc;
}

int hz_index_search_batch(void* h, int ctx, const float* queries, int Q, int k, int R, float* out_score, int* out_id,
                          float* out_stage1_last) {
  Index* x = static_cast<Index*>(h);
  if (!x || !queries || !out_score || !out_id || !out_stage1_last) return -1;
  if (ctx < 0 || ctx >= (int)x->ctx.size()) return -9;
  if (x->fp8 || x->ivf || x->bin || x->pq) {
    g_err = std::string("index: search_batch is built for plain bf16 indexes (versions 1 and 2), this one is ") +
            (x->ivf ? (x->fp8 ? "an fp8 IVF index" : "an IVF index") : x->quant_name()) + " of version " +
            std::to_string(x->h.version);
    return -44;
  }
  if (x->h.dim % 32) {
    g_err = "index: search_batch needs dim % 32 == 0 (one MFMA step is 32 columns), got dim = " + std::to_string(x->h.dim);
    return -45;
  }
  if (k < 1 || k > HZ_SEARCH_MAX_K) {
    g_err = "index: k must be in 1.." + std::to_string(HZ_SEARCH_MAX_K) + ", got " + std::to_string(k);
    return -5;
  }
  if (R < k || R > HZ_SEARCH_MAX_K) {
    g_err = "index: candidates must be in k.." + std::to_string(HZ_SEARCH_MAX_K) + ", got " + std::to_string(R) + " with k = " +
            std::to_string(k);
    return -28;
  }
  Ctx& c = *x->ctx[ctx];
  std::lock_guard<std::mutex> lk(c.mu);  // count and self_max change only under every context's mutex
  if (Q < 1 || Q > x->self_max) {
    g_err = "index: search_batch takes 1.." + std::to_string(x->self_max) + " queries a call, got " + std::to_string(Q);
    return -4;
  }
  if (hipSetDevice(x->device) != hipSuccess) return -10;
  bool fresh = false;
  HzProgram g = x->batch_program(c, Q, k, R, &fresh);
  if (!g) return -11;
  std::memcpy(c.bq_host, queries, (size_t)Q * x->h.dim * 4);
  int rc = fresh ? hz_prog_run(g, c.st) : hz_prog_replay(g, c.st);
  if (!rc) rc = (int)hipStreamSynchronize(c.st);
  if (rc) return rc;
  std::memcpy(out_score, c.bout_host, (size_t)Q * k * 4);
  std::memcpy(out_id, c.bout_host + kSelfOutHalf, (size_t)Q * k * 4);
  const float* s1 = reinterpret_cast<const float*>(c.bout_host + 2 * kSelfOutHalf);  // [Q][R], best first
  for (int q = 0; q < Q; ++q) out_stage1_last[q] = s1[(size_t)q * R + R - 1];
  if (fresh) {
    rc = hz_prog_capture(g, c.st);
    if (!rc) rc = (int)hipStreamSynchronize(c.st);
  }
  return rc;
}

namespace {

// a clustering buffer of a context of at least `need` bytes: kept when large enough, else replaced (the caller
// holds c.mu and nothing is in flight on c.st)
void* cl_buffer(Ctx& c, int which, uint64_t need) {
  if (need <= c.cl_bytes[which] && c.cl[which]) return c.cl[which];
  if (c.cl[which]) (void)hipFree(c.cl[which]);
  c.cl[which] = nullptr, c.cl_bytes[which] = 0;
  if (hipMalloc(&c.cl[which], need) != hipSuccess) return nullptr;
  c.cl_bytes[which] = need;
  return c.cl[which];
}

// what both clustering calls refuse: -9 the context, -38 an fp8 or an IVF index, -39 dim % 32, -40 C
int cluster_check(const Index* x, int ctx, int C, const char* call) {
  if (ctx < 0 || ctx >= (int)x->ctx.size()) return -9;
  if (x->fp8 || x->ivf || x->bin || x->pq) {
    g_err = std::string("index: ") + call + " is built for plain bf16 indexes (versions 1 and 2), this one is " +
            (x->ivf ? (x->fp8 ? "an fp8 IVF index" : "an IVF index") : x->quant_name()) + " of version " +
            std::to_string(x->h.version);
    return -38;
  }
  if (x->h.dim % 32) {
    g_err = std::string("index: ") + call + " needs dim % 32 == 0 (one MFMA step is 32 columns), got dim = " + std::to_string(x->h.dim);
    return -39;
  }
  if (C < 1 || C > HZ_SEARCH_ASSIGN_MAX_C) {
    g_err = "index: the number of centroids must be in 1.." + std::to_string(HZ_SEARCH_ASSIGN_MAX_C) + ", got " + std::to_string(C);
    return -40;
  }
  return 0;
}

}  // namespace

int hz_index_assign(void* h, int ctx, const unsigned short* cent_bits, int C, const unsigned* mask_words, int* out_list,
                    float* out_score) {
  Index* x = static_cast<Index*>(h);
  if (!x || !cent_bits || !out_list || !out_score) return -1;
  if (const int rc = cluster_check(x, ctx, C, "assign")) return rc;
  Ctx& c = *x->ctx[ctx];
  std::lock_guard<std::mutex> lk(c.mu);  // count and the bitmap mirror change only under every context's mutex
  if (x->count < 1) return 0;
  if (hipSetDevice(x->device) != hipSuccess) return -10;
  const uint64_t n = x->scan_rows(), dim = x->h.dim, words = x->cap / 32, used = (x->count + 31) / 32;
  void* cent = cl_buffer(c, Ctx::kClCent, (uint64_t)C * dim * 2);
  void* mask = cl_buffer(c, Ctx::kClMask, words * 4);
  void* out = cl_buffer(c, Ctx::kClOut, n * 8);
  if (!cent || !mask || !out) return -11;
  std::vector<uint32_t> bits(words, 0u);  // live AND mask; the rows from count on stay dead
  for (uint64_t i = 0; i < used; ++i) bits[i] = x->live_host[i] & (mask_words ? mask_words[i] : ~0u);
  HzSearchAssignParams p{};
  p.corpus = x->rows;
  p.cent = static_cast<const unsigned short*>(cent);
  p.live = static_cast<const unsigned*>(mask);
  p.out_list = static_cast<int*>(out);
  p.out_score = reinterpret_cast<float*>(static_cast<char*>(out) + n * 4);
  p.live_bytes = words * 4;
  p.N = (int)n, p.D = p.ldc = p.ldk = (int)dim, p.C = C;
  int rc = (int)hipMemcpyAsync(cent, cent_bits, (uint64_t)C * dim * 2, hipMemcpyHostToDevice, c.st);
  if (!rc) rc = (int)hipMemcpyAsync(mask, bits.data(), words * 4, hipMemcpyHostToDevice, c.st);
  if (!rc) rc = hz_launch_kernel(HZ_K_SEARCH_ASSIGN, &p, c.st);
  if (!rc) rc = (int)hipMemcpyAsync(out_list, p.out_list, x->count * 4, hipMemcpyDeviceToHost, c.st);
  if (!rc) rc = (int)hipMemcpyAsync(out_score, p.out_score, x->count * 4, hipMemcpyDeviceToHost, c.st);
  const int rs = (int)hipStreamSynchronize(c.st);  // `bits` and the caller's arrays are in use until here
  return rc ? rc : rs;
}

int hz_index_cmean(void* h, int ctx, const int* order, long long M, const int* seg_off, int C, unsigned short* cent_bits_inout,
                   float* cent32_out) {
  Index* x = static_cast<Index*>(h);
  if (!x || !seg_off || !cent_bits_inout || (!order && M > 0)) return -1;
  if (const int rc = cluster_check(x, ctx, C, "cmean")) return rc;
  if (M < 0 || M >= (1ll << 31)) {
    g_err = "index: the number of members must be in [0, 2^31), got " + std::to_string(M);
    return -41;
  }
  for (int i = 0; i <= C; ++i) {
    const long long lo = i ? seg_off[i - 1] : 0, want_hi = M;
    if (seg_off[i] < lo || seg_off[i] > want_hi || (i == 0 && seg_off[0] != 0) || (i == C && seg_off[C] != M)) {
      g_err = "index: seg_off must run 0 = seg_off[0] <= ... <= seg_off[C] = " + std::to_string(M) + ", got seg_off[" +
              std::to_string(i) + "] = " + std::to_string(seg_off[i]);
      return -42;
    }
  }
  Ctx& c = *x->ctx[ctx];
  std::lock_guard<std::mutex> lk(c.mu);
  for (long long i = 0; i < M; ++i)
    if (order[i] < 0 || (uint64_t)order[i] >= x->count) {
      g_err = "index: member id " + std::to_string(order[i]) + " is outside [0, " + std::to_string(x->count) + ")";
      return -43;
    }
  if (M == 0) return 0;  // every segment is empty: every centroid keeps its value
  if (hipSetDevice(x->device) != hipSuccess) return -10;
  const uint64_t dim = x->h.dim;
  void* cent = cl_buffer(c, Ctx::kClCent, (uint64_t)C * dim * 2);
  void* ord = cl_buffer(c, Ctx::kClOrder, (uint64_t)M * 4);
  void* seg = cl_buffer(c, Ctx::kClSeg, ((uint64_t)C + 1) * 4);
  void* c32 = cent32_out ? cl_buffer(c, Ctx::kClCent32, (uint64_t)C * dim * 4) : nullptr;
  if (!cent || !ord || !seg || (cent32_out && !c32)) return -11;
  HzSearchCmeanParams p{};
  p.corpus = x->rows;
  p.order = static_cast<const int*>(ord);
  p.seg_off = static_cast<const int*>(seg);
  p.cent = static_cast<unsigned short*>(cent);
  p.cent32 = static_cast<float*>(c32);
  p.N = (int)x->count, p.D = p.ldc = p.ldk = (int)dim, p.C = C, p.M = (int)M;
  p.cosine = x->h.metric == 0 ? 1 : 0;
  int rc = (int)hipMemcpyAsync(cent, cent_bits_inout, (uint64_t)C * dim * 2, hipMemcpyHostToDevice, c.st);
  if (!rc && c32) rc = (int)hipMemcpyAsync(c32, cent32_out, (uint64_t)C * dim * 4, hipMemcpyHostToDevice, c.st);  // an empty segment keeps the caller's values
  if (!rc) rc = (int)hipMemcpyAsync(ord, order, (uint64_t)M * 4, hipMemcpyHostToDevice, c.st);
  if (!rc) rc = (int)hipMemcpyAsync(seg, seg_off, ((uint64_t)C + 1) * 4, hipMemcpyHostToDevice, c.st);
  if (!rc) rc = hz_launch_kernel(HZ_K_SEARCH_CMEAN, &p, c.st);
  if (!rc) rc = (int)hipMemcpyAsync(cent_bits_inout, cent, (uint64_t)C * dim * 2, hipMemcpyDeviceToHost, c.st);
  if (!rc && c32) rc = (int)hipMemcpyAsync(cent32_out, c32, (uint64_t)C * dim * 4, hipMemcpyDeviceToHost, c.st);
  const int rs = (int)hipStreamSynchronize(c.st);
  return rc ? rc : rs;
}

int hz_index_search_filtered(void* h, int ctx, const float* queries, const unsigned* filt, int Q, int k, float* out_score,
                             int* out_id) {
  return hz_index_search2(h, ctx, queries, filt, Q, k, 0, out_score, out_id);
}

int hz_index_search(void* h, int ctx, const float* queries, int Q, int k, float* out_score, int* out_id) {
  return hz_index_search_filtered(h, ctx, queries, nullptr, Q, k, out_score, out_id);
}

}  // extern "C"

namespace {

// hz_index_add / hz_index_add_q / hz_index_add_qr: `data` holds n rows in the index's own format, `scales` n
// floats (fp8) or NULL, `rr` the n bf16 rescore rows (a two-stage index) or NULL
int add_rows(Index* x, const void* data, const float* scales, const unsigned short* rr, long long n, const unsigned* tags,
             long long* first_id) {
  AllLocked all(*x);
  if (hipSetDevice(x->device) != hipSuccess) return -10;
  const uint64_t first = x->count, last = first + (uint64_t)n;
  if (last > (1ull << 31) - kTile) return -21;  // the capacity is whole tiles and below 2^31
  hipStream_t st = x->ctx[0]->st;
  const uint64_t scan_before = x->scan_rows();
  if (last > x->cap) {  // grow by doubling: new allocations, device-to-device copies, a swap
    x->drop_programs();
    const uint64_t want = std::min<uint64_t>(round_up(std::max(last, 2 * x->cap), kTile), (1ull << 31) - kTile);
    if (const int rc = x->reallocate(want, st)) return rc;
  }
  // rows and tags first: above `count` they are dead, so a failure here leaves nothing a search can see
  for (uint64_t r = first; r < last; ++r) x->tags_host[r] = tags ? tags[r - first] : 0u;
  const uint64_t rb = x->rowb();
  int rc = (int)hipMemcpyAsync(reinterpret_cast<char*>(x->rows) + first * rb, data, (uint64_t)n * rb, hipMemcpyHostToDevice, st);
  if (!rc && scales) rc = (int)hipMemcpyAsync(x->scales + first, scales, (uint64_t)n * 4, hipMemcpyHostToDevice, st);
  if (!rc && rr) {  // like the other halves: dead above `count` until the live bits are set
    if (x->rescore_host) std::memcpy(x->rrows + first * x->h.dim, rr, (uint64_t)n * x->h.dim * 2);
    else rc = (int)hipMemcpyAsync(x->rrows + first * x->h.dim, rr, (uint64_t)n * x->h.dim * 2, hipMemcpyHostToDevice, st);
  }
  if (!rc) rc = push_words(x->tags, x->tags_host, first, last, st);
  if (!rc) rc = (int)hipStreamSynchronize(st);
  if (rc) return rc;
  // then the live bits; if their copy fails the mirror is rolled back and the old words are pushed again
  const uint64_t w0 = first >> 5, w1 = (last + 31) >> 5;
  const std::vector<uint32_t> before(x->live_host.begin() + w0, x->live_host.begin() + w1);
  for (uint64_t r = first; r < last; ++r) x->live_host[r >> 5] |= 1u << (r & 31);
  rc = push_words(x->live, x->live_host, w0, w1, st);
  if (!rc) rc = (int)hipStreamSynchronize(st);
  if (rc) {
    std::copy(before.begin(), before.end(), x->live_host.begin() + w0);
    (void)push_words(x->live, x->live_host, w0, w1, st);
    (void)hipStreamSynchronize(st);
    return rc;
  }
  for (uint64_t r = first; r < last && tags && !x->has_tags; ++r) x->has_tags = tags[r - first] != 0;
  x->count = last;
  x->live_count += (uint64_t)n;
  x->set_mutated();
  if (x->scan_rows() != scan_before) x->drop_programs();  // the filtered programs hold N and ntile by value
  if (first_id) *first_id = (long long)first;
  return 0;
}

int no_ivf_add() {
  g_err = "index: IVF indexes do not take hz_index_add yet";
  return -34;
}

int wrong_dtype(const Index* x, const char* call, const char* takes) {
  g_err = std::string("index: ") + call + " takes " + takes + " rows, the index holds " + x->dtype_name();
  return -26;
}

}  // namespace

extern "C" {

int hz_index_add(void* h, const unsigned short* rows_bf16, long long n, const unsigned* tags, long long* first_id) {
  Index* x = static_cast<Index*>(h);
  if (!x || !rows_bf16 || n < 1) return -1;
  if (x->ivf) return no_ivf_add();
  if (x->fp8 || x->bin || x->pq) return wrong_dtype(x, "hz_index_add", "bf16");
  return add_rows(x, rows_bf16, nullptr, nullptr, n, tags, first_id);
}

int hz_index_add_q(void* h, const unsigned char* codes, const float* scales, long long n, const unsigned* tags,
                   long long* first_id) {
  Index* x = static_cast<Index*>(h);
  if (!x || !codes || !scales || n < 1) return -1;
  if (x->ivf) return no_ivf_add();
  if (!x->fp8) return wrong_dtype(x, "hz_index_add_q", "fp8_e4m3");
  if (x->rescore) {
    g_err = "index: hz_index_add_q adds fp8 rows only; an index with rescore rows takes hz_index_add_qr (codes, scales and bf16 rows)";
    return -29;
  }
  return add_rows(x, codes, scales, nullptr, n, tags, first_id);
}

int hz_index_add_qr(void* h, const unsigned char* codes, const float* scales, const unsigned short* rows_bf16, long long n,
                    const unsigned* tags, long long* first_id) {
  Index* x = static_cast<Index*>(h);
  if (!x || !codes || !scales || !rows_bf16 || n < 1) return -1;
  if (x->ivf) return no_ivf_add();
  if (!x->fp8) return wrong_dtype(x, "hz_index_add_qr", "fp8_e4m3");
  if (!x->rescore) {
    g_err = "index: hz_index_add_qr needs an index with rescore rows (a version-4 file); use hz_index_add_q";
    return -29;
  }
  return add_rows(x, codes, scales, rows_bf16, n, tags, first_id);
}

// sign-bit rows (a version-8 file): n rows of dim / 32 words
int hz_index_add_b(void* h, const unsigned* words, long long n, const unsigned* tags, long long* first_id) {
  Index* x = static_cast<Index*>(h);
  if (!x || !words || n < 1) return -1;
  if (x->ivf) return no_ivf_add();
  if (!x->bin) return wrong_dtype(x, "hz_index_add_b", "bin_sign");
  if (x->rescore) {
    g_err = "index: hz_index_add_b adds sign-bit rows only; an index with rescore rows takes hz_index_add_br (words and bf16 rows)";
    return -29;
  }
  return add_rows(x, words, nullptr, nullptr, n, tags, first_id);
}

// a two-stage binary index (a version-9 file): words and bf16 rows together, the live bits set last
int hz_index_add_br(void* h, const unsigned* words, const unsigned short* rows_bf16, long long n, const unsigned* tags,
                    long long* first_id) {
  Index* x = static_cast<Index*>(h);
  if (!x || !words || !rows_bf16 || n < 1) return -1;
  if (x->ivf) return no_ivf_add();
  if (!x->bin) return wrong_dtype(x, "hz_index_add_br", "bin_sign");
  if (!x->rescore) {
    g_err = "index: hz_index_add_br needs an index with rescore rows (a version-9 file); use hz_index_add_b";
    return -29;
  }
  return add_rows(x, words, nullptr, rows_bf16, n, tags, first_id);
}

// pq8 rows (a version-10 file): n rows of pq_m code bytes, encoded by the caller against the index's codebook
int hz_index_add_p(void* h, const unsigned char* codes, long long n, const unsigned* tags, long long* first_id) {
  Index* x = static_cast<Index*>(h);
  if (!x || !codes || n < 1) return -1;
  if (x->ivf) return no_ivf_add();
  if (!x->pq) return wrong_dtype(x, "hz_index_add_p", "pq8");
  if (x->rescore) {
    g_err = "index: hz_index_add_p adds pq8 rows only; an index with rescore rows takes hz_index_add_pr (codes and bf16 rows)";
    return -29;
  }
  return add_rows(x, codes, nullptr, nullptr, n, tags, first_id);
}

// a two-stage pq8 index (a version-11 file): codes and bf16 rows together, the live bits set last
int hz_index_add_pr(void* h, const unsigned char* codes, const unsigned short* rows_bf16, long long n, const unsigned* tags,
                    long long* first_id) {
  Index* x = static_cast<Index*>(h);
  if (!x || !codes || !rows_bf16 || n < 1) return -1;
  if (x->ivf) return no_ivf_add();
  if (!x->pq) return wrong_dtype(x, "hz_index_add_pr", "pq8");
  if (!x->rescore) {
    g_err = "index: hz_index_add_pr needs an index with rescore rows (a version-11 file); use hz_index_add_p";
    return -29;
  }
  return add_rows(x, codes, nullptr, rows_bf16, n, tags, first_id);
}

int hz_index_delete(void* h, const int* ids, long long n, long long* newly_deleted) {
  Index* x = static_cast<Index*>(h);
  if (!x || (!ids && n > 0) || n < 0) return -1;
  AllLocked all(*x);
  if (hipSetDevice(x->device) != hipSuccess) return -10;
  for (long long i = 0; i < n; ++i)
    if (x->pos(ids[i]) < 0) return -20;
  uint64_t lo = ~0ull, hi = 0, gone = 0;
  for (long long i = 0; i < n; ++i) {
    const uint64_t r = (uint64_t)x->pos(ids[i]);
    const uint64_t w = r >> 5;
    const uint32_t bit = 1u << (r & 31);
    if (!(x->live_host[w] & bit)) continue;
    x->live_host[w] &= ~bit;
    lo = std::min(lo, w), hi = std::max(hi, w + 1), ++gone;
  }
  if (gone) {
    hipStream_t st = x->ctx[0]->st;
    int rc = push_words(x->live, x->live_host, lo, hi, st);
    if (!rc) rc = (int)hipStreamSynchronize(st);
    if (rc) return rc;
    x->live_count -= gone;
    x->set_mutated();
  }
  if (newly_deleted) *newly_deleted = (long long)gone;
  return 0;
}

int hz_index_set_tags(void* h, const int* ids, const unsigned* tags, long long n) {
  Index* x = static_cast<Index*>(h);
  if (!x || ((!ids || !tags) && n > 0) || n < 0) return -1;
  AllLocked all(*x);
  if (hipSetDevice(x->device) != hipSuccess) return -10;
  for (long long i = 0; i < n; ++i)
    if (x->pos(ids[i]) < 0) return -20;
  uint64_t lo = ~0ull, hi = 0;
  for (long long i = 0; i < n; ++i) {
    const uint64_t r = (uint64_t)x->pos(ids[i]);
    x->tags_host[r] = tags[i];
    if (tags[i]) x->has_tags = true;
    lo = std::min<uint64_t>(lo, r), hi = std::max<uint64_t>(hi, r + 1);
  }
  if (n == 0) return 0;
  hipStream_t st = x->ctx[0]->st;
  int rc = push_words(x->tags, x->tags_host, lo, hi, st);
  if (!rc) rc = (int)hipStreamSynchronize(st);
  return rc;
}

}  // extern "C"

namespace {

// the first `n` (<= count) rows, scales (fp8), tag words and ceil(n / 32) live words back to the host (for save)
int read_state(Index* x, void* rows_out, float* scales_out, unsigned* tags_out, unsigned* live_out, long long n) {
  AllLocked all(*x);
  if ((uint64_t)n > x->count) return -20;
  if (hipSetDevice(x->device) != hipSuccess) return -10;
  if (tags_out) std::memcpy(tags_out, x->tags_host.data(), (size_t)n * 4);
  if (live_out) std::memcpy(live_out, x->live_host.data(), (size_t)(((uint64_t)n + 31) / 32) * 4);
  int rc = 0;
  if (scales_out && n) rc = (int)hipMemcpy(scales_out, x->scales, (uint64_t)n * 4, hipMemcpyDeviceToHost);
  if (!rc && rows_out && n) rc = (int)hipMemcpy(rows_out, x->rows, (uint64_t)n * x->rowb(), hipMemcpyDeviceToHost);
  return rc;
}

}  // namespace

extern "C" {

// any output pointer may be NULL
int hz_index_read_state(void* h, unsigned short* rows_out, unsigned* tags_out, unsigned* live_out, long long n) {
  Index* x = static_cast<Index*>(h);
  if (!x || n < 0) return -1;
  if (x->fp8 || x->bin || x->pq) return wrong_dtype(x, "hz_index_read_state", "bf16");
  return read_state(x, rows_out, nullptr, tags_out, live_out, n);
}

int hz_index_read_state_q(void* h, unsigned char* codes_out, float* scales_out, unsigned* tags_out, unsigned* live_out,
                          long long n) {
  Index* x = static_cast<Index*>(h);
  if (!x || n < 0) return -1;
  if (!x->fp8) return wrong_dtype(x, "hz_index_read_state_q", "fp8_e4m3");
  return read_state(x, codes_out, scales_out, tags_out, live_out, n);
}

int hz_index_read_state_b(void* h, unsigned* words_out, unsigned* tags_out, unsigned* live_out, long long n) {
  Index* x = static_cast<Index*>(h);
  if (!x || n < 0) return -1;
  if (!x->bin) return wrong_dtype(x, "hz_index_read_state_b", "bin_sign");
  return read_state(x, words_out, nullptr, tags_out, live_out, n);
}

int hz_index_read_state_p(void* h, unsigned char* codes_out, unsigned* tags_out, unsigned* live_out, long long n) {
  Index* x = static_cast<Index*>(h);
  if (!x || n < 0) return -1;
  if (!x->pq) return wrong_dtype(x, "hz_index_read_state_p", "pq8");
  return read_state(x, codes_out, nullptr, tags_out, live_out, n);
}

int hz_index_read_codebook(void* h, float* codebook_out) {
  Index* x = static_cast<Index*>(h);
  if (!x || !codebook_out) return -1;
  if (!x->pq) return wrong_dtype(x, "hz_index_read_codebook", "pq8");
  std::memcpy(codebook_out, x->codebook_host.data(), x->codebook_bytes());
  return 0;
}

// the first n (<= count) rescore rows back to the host (for save)
int hz_index_read_rescore(void* h, unsigned short* rows_out, long long n) {
  Index* x = static_cast<Index*>(h);
  if (!x || !rows_out || n < 0) return -1;
  AllLocked all(*x);
  if (!x->rescore) {
    g_err = "index: hz_index_read_rescore needs an index with rescore rows (a version-4 or version-7 file)";
    if (x->bin) g_err = "index: hz_index_read_rescore needs an index with rescore rows (a version-9 file)";
    if (x->pq) g_err = "index: hz_index_read_rescore needs an index with rescore rows (a version-11 file)";
    return -29;
  }
  if ((uint64_t)n > x->rescore_rows(x->count)) return -20;
  if (hipSetDevice(x->device) != hipSuccess) return -10;
  const uint64_t bytes = (uint64_t)n * x->h.dim * 2;
  if (x->rescore_host) std::memcpy(rows_out, x->rrows, bytes);
  else if (n) return (int)hipMemcpy(rows_out, x->rrows, bytes, hipMemcpyDeviceToHost);
  return 0;
}

void hz_index_close(void* h) { delete static_cast<Index*>(h); }

// hz_pq_encode (hipzap.h): no index, a stream and four device buffers of its own, all released on
// every way out. Per chunk: H2D of the rows, HZ_K_SEARCH_PQASSIGN, D2H of the codes (and distances), one synchronise.
int hz_pq_encode(int device, const unsigned short* rows_bf16, long long n, int dim, int m, const float* codebook,
                 long long chunk_rows, unsigned char* codes_out, float* dist_out) {
  if (!rows_bf16 || !codebook || !codes_out) return -129;
  if (m < 1) return -132;  // before the division
  if (dim % m) return -130;
  if (m % 16) return -131;
  if (m < 16 || m > HZ_SEARCH_PQ_MAX_M) return -132;
  if (dim / m < 1 || dim / m > HZ_SEARCH_PQ_MAX_DSUB) return -133;
  if (dim > 2048) return -134;
  if (n < 1) return -137;
  if (chunk_rows < 0) {
    g_err = "pq_encode: chunk_rows must be 0 (the default) or positive, got " + std::to_string(chunk_rows);
    return -141;
  }
  const uint64_t chunk = (uint64_t)std::min<long long>(n, chunk_rows ? chunk_rows : 65536);
  const uint64_t cb_bytes = (uint64_t)256 * dim * 4;  // [m][256][dim / m] fp32
  hipStream_t st = nullptr;
  unsigned short* d_rows = nullptr;
  float* d_cb = nullptr;
  unsigned char* d_codes = nullptr;
  float* d_dist = nullptr;
  int rc = 0;
  const auto step = [&](hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    g_err = std::string("pq_encode: ") + what + " failed: " + hipGetErrorString(e);
    rc = -140;
    return false;
  };
  if (step(hipSetDevice(device), "hipSetDevice") && step(hipStreamCreateWithFlags(&st, hipStreamNonBlocking), "hipStreamCreate") &&
      step(hipMalloc(&d_rows, chunk * dim * 2), "hipMalloc of the row buffer") &&
      step(hipMalloc(&d_cb, cb_bytes), "hipMalloc of the codebook") &&
      step(hipMalloc(&d_codes, chunk * m), "hipMalloc of the code buffer") &&
      (!dist_out || step(hipMalloc(&d_dist, chunk * m * 4), "hipMalloc of the distance buffer")) &&
      step(hipMemcpyAsync(d_cb, codebook, cb_bytes, hipMemcpyHostToDevice, st), "the codebook's copy")) {
    for (uint64_t at = 0; at < (uint64_t)n && !rc; at += chunk) {
      const uint64_t rows = std::min<uint64_t>(chunk, (uint64_t)n - at);
      if (!step(hipMemcpyAsync(d_rows, rows_bf16 + at * dim, rows * dim * 2, hipMemcpyHostToDevice, st), "a row chunk's copy")) break;
      HzSearchPqAssignParams p{};
      p.rows = d_rows;
      p.codebook = d_cb;
      p.codes = d_codes;
      p.dist = d_dist;
      p.dist_bytes = d_dist ? rows * m * 4 : 0;
      p.N = (long long)rows;
      p.D = dim;
      p.M = m;
      p.ldr = dim;
      p.ldc = m;
      if (const int lrc = hz_search_pqassign_launch(&p, st)) {
        if (lrc > 0) step((hipError_t)lrc, "the assign launch");
        else rc = lrc;
        break;
      }
      if (!step(hipMemcpyAsync(codes_out + at * m, d_codes, rows * m, hipMemcpyDeviceToHost, st), "a code chunk's copy")) break;
      if (d_dist && !step(hipMemcpyAsync(dist_out + at * m, d_dist, rows * m * 4, hipMemcpyDeviceToHost, st), "a distance chunk's copy"))
        break;
      if (!step(hipStreamSynchronize(st), "hipStreamSynchronize")) break;
    }
  }
  if (st) (void)hipStreamSynchronize(st);
  if (d_rows) (void)hipFree(d_rows);
  if (d_cb) (void)hipFree(d_cb);
  if (d_codes) (void)hipFree(d_codes);
  if (d_dist) (void)hipFree(d_dist);
  if (st) (void)hipStreamDestroy(st);
  return rc;
}

}  // extern "C"
