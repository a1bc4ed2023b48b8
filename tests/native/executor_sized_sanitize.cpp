// Host-side sanitizer check of the executor's sized submit (csrc/executor.cpp hz_exec_submit_sized):
// a request smaller than its pinned input copies only its own bytes. Built with -Xarch_host
// -fsanitize=address,undefined or thread by tests/test_resize_cpu.py, stand-alone (no GPU: the
// replay and the four HIP event calls the executor makes are defined here, as in
// executor_host_sanitize.cpp).
//
// Two inputs per slot (a payload of up to kCap bytes and a 32-byte header carrying its length, like a
// resize plan's image + dims). The fake program sums the first `len` payload bytes at replay time and
// reports the byte after them. Payloads live in exact-size heap blocks: a copy of the whole pinned
// input would read past them (an ASan report), and the byte after a short payload must still be what
// the slot held before (the tail is not touched).
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "hipzap.h"

namespace {

constexpr int kCap = 4096;
constexpr uint8_t kFill = 0xA5;  // what every slot's payload buffer holds before the first request

struct FakeProg {
  uint8_t* payload;
  int32_t* header;
  int64_t* out;  // {sum of the first header[0] bytes, the byte after them (or -1 at kCap)}
};

struct FakeEvent {
  std::atomic<int64_t> ready_ns{0};
};

int64_t now_ns() {
  return std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

}  // namespace

extern "C" int hz_prog_replay(HzProgram p, hipStream_t) {
  auto* fp = static_cast<FakeProg*>(p);
  const int len = fp->header[0];
  int64_t s = 0;
  for (int i = 0; i < len; ++i) s += fp->payload[i];
  fp->out[0] = s;
  fp->out[1] = len < kCap ? fp->payload[len] : -1;
  return 0;
}

hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned) {
  *ev = reinterpret_cast<hipEvent_t>(new FakeEvent());
  return hipSuccess;
}

hipError_t hipEventRecord(hipEvent_t ev, hipStream_t) {
  reinterpret_cast<FakeEvent*>(ev)->ready_ns.store(now_ns() + 20000, std::memory_order_release);
  return hipSuccess;
}

hipError_t hipEventQuery(hipEvent_t ev) {
  return now_ns() >= reinterpret_cast<FakeEvent*>(ev)->ready_ns.load(std::memory_order_acquire) ? hipSuccess
                                                                                                  : hipErrorNotReady;
}

hipError_t hipEventDestroy(hipEvent_t ev) {
  delete reinterpret_cast<FakeEvent*>(ev);
  return hipSuccess;
}

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); \
      return 1;                                                    \
    }                                                              \
  } while (0)

int main() {
  constexpr int kSlots = 3, kClients = 6, kIters = 200;
  std::vector<std::vector<uint8_t>> payloads(kSlots, std::vector<uint8_t>(kCap, kFill));
  std::vector<std::vector<int32_t>> headers(kSlots, std::vector<int32_t>(8, 0));
  std::vector<std::vector<int64_t>> outs(kSlots, std::vector<int64_t>(2, 0));
  std::vector<FakeProg> progs(kSlots);
  std::vector<HzProgram> hp;
  std::vector<hipStream_t> streams(kSlots, nullptr);
  std::vector<void*> host_in(2 * kSlots), host_out;
  for (int i = 0; i < kSlots; ++i) {
    progs[i] = {payloads[i].data(), headers[i].data(), outs[i].data()};
    hp.push_back(&progs[i]);
    host_in[i] = payloads[i].data();           // host_in[k * n + i]
    host_in[kSlots + i] = headers[i].data();
    host_out.push_back(outs[i].data());
  }
  const uint64_t in_bytes[2] = {kCap, 32};
  void* ex = hz_exec_create(hp.data(), streams.data(), host_in.data(), in_bytes, 2, host_out.data(), 16, kSlots);
  CHECK(ex != nullptr);
  {  // argument checks: no sizes, a size above the pinned input
    std::vector<uint8_t> pl(16, 1);
    int32_t hd[8] = {16};
    const void* in[2] = {pl.data(), hd};
    int64_t out[2];
    const uint64_t too_big[2] = {kCap + 1, 32}, hdr_big[2] = {16, 33};
    CHECK(hz_exec_submit_sized(ex, in, nullptr, out, nullptr) == -1);
    CHECK(hz_exec_submit_sized(ex, in, too_big, out, nullptr) == -2);
    CHECK(hz_exec_submit_sized(ex, in, hdr_big, out, nullptr) == -2);
  }
  // phase 1: every request is shorter than kCap / 2 -- the byte after it is still the initial fill
  // phase 2: full-size requests of byte 7, then short ones again: their tail byte is the stale 7
  std::atomic<int> bad{0};
  for (int phase = 0; phase < 3; ++phase) {
    std::vector<std::thread> th;
    for (int c = 0; c < kClients; ++c)
      th.emplace_back([&, c] {
        for (int it = 0; it < kIters; ++it) {
          const int len = phase == 1 ? kCap : 1 + (c * 131 + it * 17) % (kCap / 2);
          const uint8_t v = phase == 1 ? 7 : (uint8_t)(1 + (c + it) % 5);
          std::unique_ptr<uint8_t[]> pl(new uint8_t[len]);  // exact size: an over-read is an ASan report
          std::memset(pl.get(), v, len);
          int32_t hd[8] = {len};
          const void* in[2] = {pl.get(), hd};
          const uint64_t nb[2] = {(uint64_t)len, 32};
          int64_t out[2] = {-5, -5};
          double lat = -1;
          if (hz_exec_submit_sized(ex, in, nb, out, &lat) || lat < 0) {
            bad.fetch_add(1);
            continue;
          }
          if (out[0] != (int64_t)v * len) bad.fetch_add(1);
          const int64_t tail = out[1];
          if (phase == 0 && tail != kFill && !(tail >= 1 && tail <= 5)) bad.fetch_add(1);  // fill or an earlier short payload
          if (phase == 1 && tail != -1) bad.fetch_add(1);
          if (phase == 2 && tail != 7 && tail != kFill && !(tail >= 1 && tail <= 5)) bad.fetch_add(1);  // stale bytes only
        }
      });
    for (auto& t : th) t.join();
    CHECK(bad.load() == 0);
  }
  uint64_t served = 0, polls = 0;
  hz_exec_stats(ex, &served, &polls);
  CHECK(served == 3ull * kClients * kIters);
  hz_exec_destroy(ex);
  {  // a dynamic-batching executor refuses sized requests
    void* bx = hz_exec_create_batched(hp.data(), streams.data(), host_in.data(), in_bytes, 2, host_out.data(), 16,
                                      kSlots, 2, 50.0, 1);
    CHECK(bx != nullptr);
    std::vector<uint8_t> pl(16, 1);
    int32_t hd[8] = {16};
    const void* in[2] = {pl.data(), hd};
    const uint64_t nb[2] = {16, 32};
    int64_t out[2];
    CHECK(hz_exec_submit_sized(bx, in, nb, out, nullptr) == -1);
    hz_exec_destroy(bx);
  }
  printf("executor sized sanitize: ok\n");
  return 0;
}
