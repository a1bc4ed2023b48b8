// hipzap native runtime: static op programs with hipGraph capture/replay.
//
// A model is lowered once (at cold start) into a Program: an ordered list of fully bound
// kernel launches (all pointers fixed into a static activation arena, weights packed), plus
// fork/join markers that put independent branches (e.g. a ResNet downsample conv) on side
// streams. The warm path is the Program captured as ONE hipGraph and replayed per request,
// so per-request host cost is a single hipGraphLaunch (north star "warm-path
// invocation captured as a hipGraph"). Nothing here allocates or synchronises inside the
// launch sequence, so capture is always legal (cdna_hip_programming.md §6 Guideline 9).
#include <hip/hip_runtime.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>
#include <dlfcn.h>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "common.h"
#include "hipzap.h"
#include "reqcopy.h"

namespace {

struct Op {
  int slot;  // 0 = main stream, k>0 = side stream k
  enum Type { KERNEL, MEMCPY, FORK, JOIN } type;
  int kind;               // KERNEL: HZ_K_*
  std::vector<char> prm;  // KERNEL: the kind's parameter block; MEMCPY: HzMemcpyArgs (captured by value)
};

struct Program {
  std::vector<Op> ops;
  std::vector<hipStream_t> side;     // side[k-1]
  std::vector<hipEvent_t> fork_ev;   // one per fork/join op (indexed by op)
  hipGraph_t graph = nullptr;
  // atomic: a program captured lazily (hz_prog_capture from one thread) may be replayed op by op
  // (hz_prog_replay from another) until the instantiated graph is published
  std::atomic<hipGraphExec_t> exec{nullptr};
  int max_slot = 0;

  ~Program() {
    if (hipGraphExec_t x = exec.load()) (void)hipGraphExecDestroy(x);
    if (graph) (void)hipGraphDestroy(graph);
    for (auto s : side) (void)hipStreamDestroy(s);
    for (auto e : fork_ev)
      if (e) (void)hipEventDestroy(e);
  }

  int ensure_streams() {
    while ((int)side.size() < max_slot) {
      hipStream_t s;
      if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return -1;
      side.push_back(s);
    }
    // one event per fork/join op (kernel ops need none: a program without branches touches no
    // HIP object on the host side, which is what the host-sanitizer test relies on)
    while (fork_ev.size() < ops.size()) {
      hipEvent_t e = nullptr;
      if (ops[fork_ev.size()].type >= Op::FORK &&
          hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
        return -1;
      fork_ev.push_back(e);
    }
    return 0;
  }

  int run(hipStream_t main) {
    if (ensure_streams()) return -1;
    for (size_t i = 0; i < ops.size(); ++i) {
      Op& op = ops[i];
      hipStream_t s = op.slot == 0 ? main : side[op.slot - 1];
      int rc = 0;
      const char* what = "";
      switch (op.type) {
        case Op::KERNEL:
          what = hz_kernel_name(op.kind);
          rc = hz_launch_kernel(op.kind, op.prm.data(), s);
          break;
        case Op::MEMCPY: {
          const HzMemcpyArgs* m = reinterpret_cast<const HzMemcpyArgs*>(op.prm.data());
          what = "memcpy";
          rc = (int)hipMemcpyAsync(m->dst, m->src, m->bytes, hipMemcpyDefault, s);
          break;
        }
        case Op::FORK:  // side waits for main
          what = "fork";
          rc = (int)hipEventRecord(fork_ev[i], main);
          if (!rc) rc = (int)hipStreamWaitEvent(side[op.slot - 1], fork_ev[i], 0);
          break;
        case Op::JOIN:  // main waits for side
          what = "join";
          rc = (int)hipEventRecord(fork_ev[i], side[op.slot - 1]);
          if (!rc) rc = (int)hipStreamWaitEvent(main, fork_ev[i], 0);
          break;
      }
      if (rc) {
        fprintf(stderr, "hipzap: program op %zu (%s) failed rc=%d\n", i, what, rc);
        return rc;
      }
    }
    return 0;
  }
};

}  // namespace

size_t hz_excl_pad(const void* fn, size_t dyn) {
  static const size_t target = [] {
    const char* e = getenv("HIPZAP_EXCL_LDS");
    return e ? (size_t)strtoul(e, nullptr, 10) : (size_t)0;
  }();
  if (!target || target > 160 * 1024) return dyn;
  hipFuncAttributes a;
  if (hipFuncGetAttributes(&a, fn) != hipSuccess) return dyn;
  const size_t tot = a.sharedSizeBytes + dyn;
  return tot >= target ? dyn : dyn + (target - tot);
}

extern "C" {

HzProgram hz_prog_create(void) { return new Program(); }
void hz_prog_destroy(HzProgram p) { delete static_cast<Program*>(p); }
int hz_prog_num_ops(HzProgram p) { return (int)static_cast<Program*>(p)->ops.size(); }

static int add_op(Program* P, int slot, Op::Type type, int kind = 0, const void* prm = nullptr, size_t size = 0) {
  if (P->exec) return -3;  // frozen after capture
  if (slot < 0 || slot > 8) return -4;
  if (slot > P->max_slot) P->max_slot = slot;
  const char* b = static_cast<const char*>(prm);
  P->ops.push_back(Op{slot, type, kind, std::vector<char>(b, b + size)});
  return 0;
}

int hz_prog_add_kernel(HzProgram h, int kind, const void* params, size_t size, int slot) {
  // the launcher reads a whole parameter struct: refuse unknown kinds and short records (a plan
  // image's op record, for instance) instead of reading past them when the op is replayed
  const size_t need = hz_kernel_param_size(kind);
  if (!need || size < need) return -101;
  return add_op(static_cast<Program*>(h), slot, Op::KERNEL, kind, params, size);
}
int hz_prog_add_memcpy(HzProgram h, void* dst, const void* src, size_t bytes, int slot) {
  const HzMemcpyArgs m = {dst, src, bytes};
  return add_op(static_cast<Program*>(h), slot, Op::MEMCPY, 0, &m, sizeof(m));
}
int hz_prog_add_fork(HzProgram h, int slot) {
  if (slot < 1) return -4;
  return add_op(static_cast<Program*>(h), slot, Op::FORK);
}
int hz_prog_add_join(HzProgram h, int slot) {
  if (slot < 1) return -4;
  return add_op(static_cast<Program*>(h), slot, Op::JOIN);
}

int hz_prog_run(HzProgram h, hipStream_t st) { return static_cast<Program*>(h)->run(st); }

int hz_prog_capture(HzProgram h, hipStream_t st) {
  Program* P = static_cast<Program*>(h);
  if (P->exec) return 0;
  if (P->ensure_streams()) return -1;
  hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) return (int)e;
  int rc = P->run(st);
  hipGraph_t g = nullptr;
  e = hipStreamEndCapture(st, &g);
  if (rc) {
    if (g) (void)hipGraphDestroy(g);
    return rc;
  }
  if (e != hipSuccess) return (int)e;
  P->graph = g;
  hipGraphExec_t x = nullptr;
  e = hipGraphInstantiate(&x, g, nullptr, nullptr, 0);
  if (e != hipSuccess) return (int)e;
  // upload once so the first replay does not pay for it; then publish
  (void)hipGraphUpload(x, st);
  P->exec.store(x);
  return 0;
}

int hz_prog_prepare(HzProgram h) {  // the side streams / events a run needs, made before any run
  return static_cast<Program*>(h)->ensure_streams();
}

int hz_prog_is_captured(HzProgram h) { return static_cast<Program*>(h)->exec.load() != nullptr; }

int hz_prog_replay(HzProgram h, hipStream_t st) {
  Program* P = static_cast<Program*>(h);
  hipGraphExec_t x = P->exec.load();
  if (!x) return P->run(st);
  return (int)hipGraphLaunch(x, st);
}

double hz_prog_bench(HzProgram* progs, hipStream_t* streams, int n, int iters) {
  auto t0 = std::chrono::steady_clock::now();
  for (int it = 0; it < iters; ++it)
    for (int i = 0; i < n; ++i)
      if (hz_prog_replay(progs[i], streams[i])) return -1.0;
  for (int i = 0; i < n; ++i)
    if (hipStreamSynchronize(streams[i]) != hipSuccess) return -2.0;
  auto t1 = std::chrono::steady_clock::now();
  return std::chrono::duration<double, std::micro>(t1 - t0).count();
}

// out[0] = host submission time (us), out[1] = submission + drain (us).
// threads != 0: one host thread per stream submits its own replays concurrently.
int hz_prog_bench2(HzProgram* progs, hipStream_t* streams, int n, int iters, int threads, double* out) {
  auto t0 = std::chrono::steady_clock::now();
  int rc = 0;
  if (!threads) {
    for (int it = 0; it < iters && !rc; ++it)
      for (int i = 0; i < n && !rc; ++i) rc = hz_prog_replay(progs[i], streams[i]);
  } else {
    std::vector<std::thread> th;
    std::vector<int> rcs(n, 0);
    for (int i = 0; i < n; ++i)
      th.emplace_back([&, i] {
        for (int it = 0; it < iters && !rcs[i]; ++it) rcs[i] = hz_prog_replay(progs[i], streams[i]);
      });
    for (auto& t : th) t.join();
    for (int r : rcs) rc |= r;
  }
  auto t1 = std::chrono::steady_clock::now();
  for (int i = 0; i < n; ++i)
    if (hipStreamSynchronize(streams[i]) != hipSuccess) rc = -2;
  auto t2 = std::chrono::steady_clock::now();
  out[0] = std::chrono::duration<double, std::micro>(t1 - t0).count();
  out[1] = std::chrono::duration<double, std::micro>(t2 - t0).count();
  return rc;
}

// Closed-loop serving benchmark: one host thread per context, each serving `iters` requests
// back to back the way a request thread does: copy the payload into the pinned input, replay,
// wait for THIS request's completion, copy the result out. Per-request latency (submission ->
// result in host memory) goes to lat_us[ctx * iters + i]; wall_us = total wall time. Unlike
// hz_prog_bench (replays queued back to back, no host work), every request here pays its own
// host copies and synchronisation, so throughput and p99 are what concurrent clients see.
int hz_serve_bench(HzProgram* progs, hipStream_t* streams, void** in_dst, void** in_src, uint64_t in_bytes,
                   void** out_src, void** out_dst, uint64_t out_bytes, int n, int iters, double* lat_us,
                   double* wall_us) {
  std::vector<std::thread> th;
  std::vector<int> rcs(n, 0);
  auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < n; ++i)
    th.emplace_back([&, i] {
      for (int it = 0; it < iters && !rcs[i]; ++it) {
        auto a = std::chrono::steady_clock::now();
        if (in_bytes) memcpy(in_dst[i], in_src[i], in_bytes);
        int rc = hz_prog_replay(progs[i], streams[i]);
        if (!rc) rc = (int)hipStreamSynchronize(streams[i]);
        if (!rc && out_bytes) memcpy(out_dst[i], out_src[i], out_bytes);
        rcs[i] = rc;
        lat_us[(size_t)i * iters + it] =
            std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a).count();
      }
    });
  for (auto& t : th) t.join();
  *wall_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  int rc = 0;
  for (int r : rcs) rc |= r;
  return rc;
}

}  // extern "C"

// ---- request slots (hipzap.h): device-resident, host-writable input buffers ----
//
// On a large-BAR system the whole of device memory is mapped into the process, and the runtime's
// pointer query reports the host address of a fine-grained device allocation. A request thread then
// writes its payload straight into HBM (write-combined PCIe writes, reqcopy.h) and the first kernel
// of the replay reads it at memory speed instead of pulling it over PCIe inside the launch chain
// (profiles/reqslot). No managed memory, no page migration, no command on any GPU queue.
namespace {

// the runtime's pointer query, found in the already loaded runtime (no link-time dependency; a
// host-only build without it simply has no device slots)
using PointerInfoFn = hsa_status_t (*)(const void*, hsa_amd_pointer_info_t*, void* (*)(size_t), uint32_t*,
                                       hsa_agent_t**);

// host address of a device allocation as the runtime reports it, or nullptr. Asks; never dereferences.
void* reported_host_address(void* dev) {
  static const PointerInfoFn fn = reinterpret_cast<PointerInfoFn>(dlsym(RTLD_DEFAULT, "hsa_amd_pointer_info"));
  if (!fn || !dev) return nullptr;
  hsa_amd_pointer_info_t pi;
  memset(&pi, 0, sizeof(pi));
  pi.size = sizeof(pi);
  if (fn(dev, &pi, nullptr, nullptr, nullptr) != HSA_STATUS_SUCCESS) return nullptr;
  if (pi.type != HSA_EXT_POINTER_TYPE_HSA || !pi.hostBaseAddress || !pi.agentBaseAddress) return nullptr;
  const char* base = static_cast<const char*>(pi.agentBaseAddress);
  const char* p = static_cast<const char*>(dev);
  if (p < base || p >= base + pi.sizeInBytes) return nullptr;
  return static_cast<char*>(pi.hostBaseAddress) + (p - base);
}

bool reqslot_disabled() {
  const char* e = getenv("HIPZAP_REQSLOT");
  return e && (!strcmp(e, "host") || !strcmp(e, "0") || !strcmp(e, "off"));
}

}  // namespace

extern "C" int hz_reqslot_probe(void) {
  static std::atomic<int> cache[64];  // 0 unknown, 1 no, 2 yes
  if (reqslot_disabled()) return 0;
  int d = -1, large_bar = 0;
  if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 64) return 0;
  if (const int c = cache[d].load()) return c - 1;
  int yes = 0;
  if (hipDeviceGetAttribute(&large_bar, hipDeviceAttributeIsLargeBar, d) == hipSuccess && large_bar) {
    void* p = nullptr;
    if (hipExtMallocWithFlags(&p, 4096, hipDeviceMallocFinegrained) == hipSuccess) {
      yes = reported_host_address(p) != nullptr;
      (void)hipFree(p);
    }
  }
  (void)hipGetLastError();
  cache[d].store(yes + 1);
  return yes;
}

extern "C" int hz_reqslot_alloc(uint64_t bytes, void** dev, void** host, int* kind) {
  if (!dev || !host || !kind) return -1;
  *dev = *host = nullptr;
  *kind = HZ_REQSLOT_PINNED;
  // whole 16-byte units: the streaming copy may round a payload's last unit up (reqcopy.h)
  const size_t cap = bytes ? (size_t(bytes) + 15) & ~size_t(15) : 256;
  if (hz_reqslot_probe()) {
    void* p = nullptr;
    if (hipExtMallocWithFlags(&p, cap, hipDeviceMallocFinegrained) == hipSuccess) {
      void* h = reported_host_address(p);
      if (h && hipMemset(p, 0, cap) == hipSuccess && hipDeviceSynchronize() == hipSuccess) {
        *dev = p;
        *host = h;
        *kind = HZ_REQSLOT_DEVICE;
        return 0;
      }
      (void)hipFree(p);
    }
    (void)hipGetLastError();  // fall back to pinned host memory
  }
  void* p = nullptr;
  const hipError_t e = hipHostMalloc(&p, cap, hipHostMallocDefault);
  if (e != hipSuccess) return (int)e;
  memset(p, 0, cap);
  *dev = *host = p;
  return 0;
}

extern "C" int hz_reqslot_free(void* dev, int kind) {
  if (!dev) return 0;
  return (int)(kind == HZ_REQSLOT_DEVICE ? hipFree(dev) : hipHostFree(dev));
}

extern "C" void hz_reqslot_write(void* dst, const void* src, uint64_t n, uint64_t cap) {
  hz_reqcopy(dst, src, (size_t)n, (size_t)cap);
  hz_reqcopy_fence();
}

extern "C" int hz_reqslot_copy_bench(void** slots, const void* src, uint64_t n, int threads, int iters,
                                     int streaming, double* out) {
  if (threads < 1 || iters < 1 || !slots || !src || !out) return -1;
  std::vector<std::vector<double>> v(threads);
  std::vector<std::thread> th;
  for (int t = 0; t < threads; ++t)
    th.emplace_back([&, t] {
      for (int it = 0; it < iters; ++it) {
        const auto a = std::chrono::steady_clock::now();
        if (streaming)
          hz_reqslot_write(slots[t], src, n, (n + 15) & ~uint64_t(15));
        else
          memcpy(slots[t], src, n);
        v[t].push_back(std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a).count());
      }
    });
  for (auto& t : th) t.join();
  std::vector<double> all;
  for (auto& x : v) all.insert(all.end(), x.begin(), x.end());
  std::sort(all.begin(), all.end());
  out[0] = all.front();
  out[1] = all[all.size() / 2];
  return 0;
}

// 1 when this library was built with the measured-negative experiment kernels (HZ_EXPERIMENTS)
extern "C" int hz_experiments(void) { return HZ_EXPERIMENTS; }

extern "C" int hz_prog_replay_n(HzProgram h, hipStream_t st, int n) {
  for (int i = 0; i < n; ++i) {
    const int rc = hz_prog_replay(h, st);
    if (rc) return rc;
  }
  return 0;
}

// adapters: the kinds whose launcher takes scalars or a cfg beside its parameter struct
static int hz_conv_op(const HzConvOp* o, hipStream_t st) { return hz_conv_launch(&o->p, o->cfg, st); }
static int hz_conv2_op(const HzConv2Op* o, hipStream_t st) { return hz_conv2_launch(&o->a, &o->b, o->cfg, st); }
static int hz_avgpool_op(const HzAvgpoolArgs* a, hipStream_t st) {
  return hz_avgpool_launch(a->x, a->out, a->N, a->HW, a->C, a->blocked, st);
}
static int hz_preprocess_op(const HzPreprocessArgs* a, hipStream_t st) {
  return hz_preprocess_launch(a->src, a->dst, a->N, a->Cin, a->H, a->W, a->Cpad, a->mode, a->mean, a->inv_std, st);
}
static int hz_step_bump_op(const HzStepBumpArgs* a, hipStream_t st) { return hz_step_bump_launch(a->step, a->n, st); }
static int hz_diag_op(const HzDiagArgs* a, hipStream_t st) {
  return hz_diag_launch(a->kind, a->blocks, a->threads, a->a, a->b, a->bytes, st);
}

// The resize launcher is referenced weakly: a host-only program that links runtime.cpp with its own
// stub launchers (tests/native/runtime_host_asan.cpp) need not define it; the library always does
// (vision.hip), and a missing launcher is an error, not a skipped launch.
extern "C" __attribute__((weak)) int hz_resize_preprocess_launch(const HzResizeParams* p, hipStream_t st);
static int hz_resize_preprocess_op(const HzResizeParams* p, hipStream_t st) {
  return hz_resize_preprocess_launch ? hz_resize_preprocess_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_resize_patchify_launch(const HzResizeParams* p, hipStream_t st);
static int hz_resize_patchify_op(const HzResizeParams* p, hipStream_t st) {
  return hz_resize_patchify_launch ? hz_resize_patchify_launch(p, st) : -102;
}
// (the pooled-embedding launcher likewise: transformer.hip in the library)
extern "C" __attribute__((weak)) int hz_pool_embed_launch(const HzPoolEmbedParams* p, hipStream_t st);
static int hz_pool_embed_op(const HzPoolEmbedParams* p, hipStream_t st) {
  return hz_pool_embed_launch ? hz_pool_embed_launch(p, st) : -102;
}
// (the pooled-feature launcher: vision.hip in the library)
extern "C" __attribute__((weak)) int hz_pool_norm_launch(const HzPoolNormParams* p, hipStream_t st);
static int hz_pool_norm_op(const HzPoolNormParams* p, hipStream_t st) {
  return hz_pool_norm_launch ? hz_pool_norm_launch(p, st) : -102;
}
// (the search launchers: search.hip in the library)
extern "C" __attribute__((weak)) int hz_search_scan_launch(const HzSearchParams* p, hipStream_t st);
static int hz_search_scan_op(const HzSearchParams* p, hipStream_t st) {
  return hz_search_scan_launch ? hz_search_scan_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_merge_launch(const HzSearchParams* p, hipStream_t st);
static int hz_search_merge_op(const HzSearchParams* p, hipStream_t st) {
  return hz_search_merge_launch ? hz_search_merge_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_fscan_launch(const HzSearchFilterParams* p, hipStream_t st);
static int hz_search_fscan_op(const HzSearchFilterParams* p, hipStream_t st) {
  return hz_search_fscan_launch ? hz_search_fscan_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_qscan_launch(const HzSearchQuantParams* p, hipStream_t st);
static int hz_search_qscan_op(const HzSearchQuantParams* p, hipStream_t st) {
  return hz_search_qscan_launch ? hz_search_qscan_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_rescore_launch(const HzSearchRescoreParams* p, hipStream_t st);
static int hz_search_rescore_op(const HzSearchRescoreParams* p, hipStream_t st) {
  return hz_search_rescore_launch ? hz_search_rescore_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_lscan_launch(const HzSearchListParams* p, hipStream_t st);
static int hz_search_lscan_op(const HzSearchListParams* p, hipStream_t st) {
  return hz_search_lscan_launch ? hz_search_lscan_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_qlscan_launch(const HzSearchQuantListParams* p, hipStream_t st);
static int hz_search_qlscan_op(const HzSearchQuantListParams* p, hipStream_t st) {
  return hz_search_qlscan_launch ? hz_search_qlscan_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_mscan_launch(const HzSearchSelfParams* p, hipStream_t st);
static int hz_search_mscan_op(const HzSearchSelfParams* p, hipStream_t st) {
  return hz_search_mscan_launch ? hz_search_mscan_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_mergen_launch(const HzSearchSelfParams* p, hipStream_t st);
static int hz_search_mergen_op(const HzSearchSelfParams* p, hipStream_t st) {
  return hz_search_mergen_launch ? hz_search_mergen_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_assign_launch(const HzSearchAssignParams* p, hipStream_t st);
static int hz_search_assign_op(const HzSearchAssignParams* p, hipStream_t st) {
  return hz_search_assign_launch ? hz_search_assign_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_cmean_launch(const HzSearchCmeanParams* p, hipStream_t st);
static int hz_search_cmean_op(const HzSearchCmeanParams* p, hipStream_t st) {
  return hz_search_cmean_launch ? hz_search_cmean_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_bscan_launch(const HzSearchBinParams* p, hipStream_t st);
static int hz_search_bscan_op(const HzSearchBinParams* p, hipStream_t st) {
  return hz_search_bscan_launch ? hz_search_bscan_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_xscan_launch(const HzSearchBatchParams* p, hipStream_t st);
static int hz_search_xscan_op(const HzSearchBatchParams* p, hipStream_t st) {
  return hz_search_xscan_launch ? hz_search_xscan_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_rescoren_launch(const HzSearchRescoreParams* p, hipStream_t st);
static int hz_search_rescoren_op(const HzSearchRescoreParams* p, hipStream_t st) {
  return hz_search_rescoren_launch ? hz_search_rescoren_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_pqlut_launch(const HzSearchPqLutParams* p, hipStream_t st);
static int hz_search_pqlut_op(const HzSearchPqLutParams* p, hipStream_t st) {
  return hz_search_pqlut_launch ? hz_search_pqlut_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_pqscan_launch(const HzSearchPqParams* p, hipStream_t st);
static int hz_search_pqscan_op(const HzSearchPqParams* p, hipStream_t st) {
  return hz_search_pqscan_launch ? hz_search_pqscan_launch(p, st) : -102;
}
extern "C" __attribute__((weak)) int hz_search_pqassign_launch(const HzSearchPqAssignParams* p, hipStream_t st);
static int hz_search_pqassign_op(const HzSearchPqAssignParams* p, hipStream_t st) {
  return hz_search_pqassign_launch ? hz_search_pqassign_launch(p, st) : -102;
}

// everything below is generated from the kernel table (hipzap.h HZ_KERNELS)
extern "C" int hz_launch_kernel(int kind, const void* prm, hipStream_t st) {
  switch (kind) {
#define X(NAME, value, T, fn, unit) \
  case value: return fn(static_cast<const T*>(prm), st);
    HZ_KERNELS(X)
#undef X
    default: return -100;
  }
}

// bytes of the parameter struct hz_launch_kernel reads for `kind` (0: unknown kind)
extern "C" size_t hz_kernel_param_size(int kind) {
  switch (kind) {
#define X(NAME, value, T, fn, unit) \
  case value: return sizeof(T);
    HZ_KERNELS(X)
#undef X
    default: return 0;
  }
}

extern "C" const char* hz_kernel_name(int kind) {
  switch (kind) {
#define X(NAME, value, T, fn, unit) \
  case value: return "HZ_K_" #NAME;
    HZ_KERNELS(X)
#undef X
    default: return nullptr;
  }
}

extern "C" unsigned hz_kernel_code_unit(int kind) {
  switch (kind) {
#define X(NAME, value, T, fn, unit) \
  case value: return HZ_UNIT_##unit;
    HZ_KERNELS(X)
#undef X
    default: return 0;
  }
}
