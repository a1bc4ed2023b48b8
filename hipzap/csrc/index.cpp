// .hzidx vector indexes (hipzap.h "vector search"): the bf16 row block of a file in device memory and a
// fixed set of search contexts over it. A search copies its queries into the context's pinned slot and
// replays the context's program for its (Q, k): H2D copy of the slot, scan, merge, D2H copies of the
// scores and ids, then waits on the context's stream. Q and k size the merge grid and the candidate
// layout, which a captured graph holds by value, so a program is built, run once eagerly and captured
// on the first search of each (Q, k), and replayed from then on (at most 16 x 128 small programs).
#include <fcntl.h>
#include <hip/hip_runtime.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "hipzap.h"

namespace {

thread_local std::string g_err;
std::nullptr_t fail(const std::string& m) {
  g_err = m;
  return nullptr;
}

struct Ctx {
  std::mutex mu;
  hipStream_t st = nullptr;
  float* q_host = nullptr;            // pinned [MAX_Q][dim]
  float* q_dev = nullptr;
  unsigned long long* cand = nullptr;
  uint64_t cand_bytes = 0;
  char* out_dev = nullptr;            // [MAX_Q][MAX_K] fp32 scores, then [MAX_Q][MAX_K] int32 ids
  char* out_host = nullptr;           // pinned, the same layout
  std::map<std::pair<int, int>, HzProgram> progs;
};

constexpr size_t kOutHalf = (size_t)HZ_SEARCH_MAX_Q * HZ_SEARCH_MAX_K * 4;

struct Index {
  int device = 0;
  HzIndexHeader h{};
  unsigned short* rows = nullptr;
  uint64_t row_bytes = 0;
  std::vector<std::unique_ptr<Ctx>> ctx;

  ~Index() {
    (void)hipSetDevice(device);
    for (auto& c : ctx) {
      if (c->st) (void)hipStreamSynchronize(c->st);
      for (auto& kv : c->progs) hz_prog_destroy(kv.second);
      if (c->q_host) (void)hipHostFree(c->q_host);
      if (c->out_host) (void)hipHostFree(c->out_host);
      if (c->q_dev) (void)hipFree(c->q_dev);
      if (c->cand) (void)hipFree(c->cand);
      if (c->out_dev) (void)hipFree(c->out_dev);
      if (c->st) (void)hipStreamDestroy(c->st);
    }
    if (rows) (void)hipFree(rows);
  }

  // the context's program for (Q, k), built on first use (the caller holds c.mu)
  HzProgram program(Ctx& c, int Q, int k, bool* fresh) {
    auto it = c.progs.find({Q, k});
    *fresh = it == c.progs.end();
    if (!*fresh) return it->second;
    HzSearchParams p{};
    p.corpus = rows;
    p.queries = c.q_dev;
    p.cand = c.cand;
    p.out_score = reinterpret_cast<float*>(c.out_dev);
    p.out_id = reinterpret_cast<int*>(c.out_dev + kOutHalf);
    p.N = (int)h.count;
    p.D = p.ldc = (int)h.dim;
    p.Q = Q;
    p.k = k;
    p.cand_bytes = c.cand_bytes;
    HzProgram g = hz_prog_create();
    const size_t qk = (size_t)Q * k * 4;
    int rc = hz_prog_add_memcpy(g, c.q_dev, c.q_host, (size_t)Q * h.dim * 4, 0);
    if (!rc) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_SCAN, &p, sizeof(p), 0);
    if (!rc) rc = hz_prog_add_kernel(g, HZ_K_SEARCH_MERGE, &p, sizeof(p), 0);
    if (!rc) rc = hz_prog_add_memcpy(g, c.out_host, c.out_dev, qk, 0);
    if (!rc) rc = hz_prog_add_memcpy(g, c.out_host + kOutHalf, c.out_dev + kOutHalf, qk, 0);
    if (rc) {
      hz_prog_destroy(g);
      return nullptr;
    }
    c.progs[{Q, k}] = g;
    return g;
  }
};

}  // namespace

extern "C" {

const char* hz_index_last_error(void) { return g_err.c_str(); }

void* hz_index_open(const char* path, int device, int nctx) {
  g_err.clear();
  if (nctx <= 0) nctx = 2;
  if (nctx > 16) return fail("index: at most 16 contexts");
  const int fd = open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) return fail(std::string("index: cannot open ") + path);
  HzIndexHeader h{};
  struct stat sb {};
  const bool got = fstat(fd, &sb) == 0 && pread(fd, &h, sizeof(h), 0) == (ssize_t)sizeof(h);
  close(fd);
  if (!got || std::memcmp(h.magic, HZ_INDEX_MAGIC, 8) != 0) return fail(std::string("index: not a .hzidx file: ") + path);
  if (h.version != 1) return fail("index: unknown format version " + std::to_string(h.version));
  if (h.dim < 8 || h.dim % 8 || h.dim > 2048) return fail("index: dim must be a multiple of 8 in 8..2048");
  if (h.count < 1 || h.count >= (1ull << 31)) return fail("index: count must be in 1..2^31-1");
  if (h.metric > HZ_INDEX_IP) return fail("index: unknown metric");
  const uint64_t bytes = h.count * h.dim * 2;
  if (h.data_off % 4096 || h.data_off < sizeof(h) + h.json_len || h.data_off + bytes > (uint64_t)sb.st_size)
    return fail("index: row block outside the file");
  if (hipSetDevice(device) != hipSuccess) return fail("index: hipSetDevice failed");
  auto idx = std::make_unique<Index>();
  idx->device = device;
  idx->h = h;
  idx->row_bytes = bytes;
  if (hz_search_code_warm()) return fail("index: device code load failed");
  if (hipMalloc(reinterpret_cast<void**>(&idx->rows), bytes) != hipSuccess) return fail("index: device allocation failed");
  const uint64_t cand_bytes = hz_search_scratch_bytes((long long)h.count, HZ_SEARCH_MAX_Q, HZ_SEARCH_MAX_K);
  for (int i = 0; i < nctx; ++i) {
    auto c = std::make_unique<Ctx>();
    const size_t qb = (size_t)HZ_SEARCH_MAX_Q * h.dim * 4;
    bool ok = hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void**>(&c->q_host), qb, hipHostMallocDefault) == hipSuccess;
    ok = ok && hipHostMalloc(reinterpret_cast<void**>(&c->out_host), 2 * kOutHalf, hipHostMallocDefault) == hipSuccess;
    ok = ok && hipMalloc(reinterpret_cast<void**>(&c->q_dev), qb) == hipSuccess;
    ok = ok && hipMalloc(reinterpret_cast<void**>(&c->cand), cand_bytes) == hipSuccess;
    ok = ok && hipMalloc(reinterpret_cast<void**>(&c->out_dev), 2 * kOutHalf) == hipSuccess;
    c->cand_bytes = cand_bytes;
    idx->ctx.push_back(std::move(c));
    if (!ok) return fail("index: context allocation failed");
  }
  const uint64_t off = h.data_off;
  void* dst = idx->rows;
  if (hz_upload_file(path, 1, &off, &bytes, &dst, idx->ctx[0]->st)) return fail(std::string("index: ") + hz_plan_last_error());
  if (hipStreamSynchronize(idx->ctx[0]->st) != hipSuccess) return fail("index: upload failed");
  return idx.release();
}

int hz_index_describe(void* h, uint64_t* out) {
  if (!h || !out) return -1;
  Index* x = static_cast<Index*>(h);
  uint64_t progs = 0, dev = x->row_bytes;
  for (auto& c : x->ctx) {
    std::lock_guard<std::mutex> lk(c->mu);
    progs += c->progs.size();
    dev += c->cand_bytes + (uint64_t)HZ_SEARCH_MAX_Q * x->h.dim * 4 + 2 * kOutHalf;
  }
  const uint64_t v[8] = {x->h.count, x->h.dim, x->h.metric, x->ctx.size(), (uint64_t)hz_search_tile_rows(), progs, dev, 0};
  std::memcpy(out, v, sizeof(v));
  return 0;
}

int hz_index_search(void* h, int ctx, const float* queries, int Q, int k, float* out_score, int* out_id) {
  Index* x = static_cast<Index*>(h);
  if (!x || !queries || !out_score || !out_id) return -1;
  if (ctx < 0 || ctx >= (int)x->ctx.size()) return -9;
  if (Q < 1 || Q > HZ_SEARCH_MAX_Q) return -4;
  if (k < 1 || k > HZ_SEARCH_MAX_K) return -5;
  Ctx& c = *x->ctx[ctx];
  std::lock_guard<std::mutex> lk(c.mu);
  if (hipSetDevice(x->device) != hipSuccess) return -10;
  bool fresh = false;
  HzProgram g = x->program(c, Q, k, &fresh);
  if (!g) return -11;
  std::memcpy(c.q_host, queries, (size_t)Q * x->h.dim * 4);
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

void hz_index_close(void* h) { delete static_cast<Index*>(h); }

}  // extern "C"
