// Write-only streaming copy of a request payload into a device-resident request slot.
//
// A device-resident slot (hz_reqslot_alloc, runtime.cpp) is fine-grained device memory that the CPU
// writes through the PCIe BAR: write-combined, uncached. Reading it back costs a PCIe round trip
// per access, and a partly filled write-combining buffer leaves as several small bus writes. So the
// copy never reads the destination and stores whole, 16-byte-aligned 16-byte units with
// non-temporal stores; the caller's payload may start at any address. hz_reqcopy_fence() orders the
// stores before whatever publishes the slot (the executor's queue push, a replay).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__x86_64__) || defined(__i386__)
#include <emmintrin.h>
#define HZ_REQCOPY_SSE2 1
#else
#include <atomic>
#define HZ_REQCOPY_SSE2 0
#endif

// Copies n bytes of src to dst. `cap` = bytes the caller owns from dst on (>= n). Bytes of the last
// 16-byte unit past n are written as zero when cap covers the whole unit (one full unit instead of a
// partial one); otherwise the tail goes out in 8/4/2/1-byte stores and nothing past n is touched.
// A dst that is not 16-byte aligned gets the same small stores up to the first aligned unit.
static inline void hz_reqcopy(void* dst, const void* src, size_t n, size_t cap) {
  unsigned char* d = static_cast<unsigned char*>(dst);
  const unsigned char* s = static_cast<const unsigned char*>(src);
  auto small = [&](size_t m) {  // m < 16 bytes at d, write-only
    for (size_t w = 8; w; w >>= 1)
      if (m & w) {
        std::memcpy(d, s, w);  // (a fixed-size memcpy: one store of w bytes, no read of d)
        d += w, s += w;
      }
  };
  const size_t mis = reinterpret_cast<uintptr_t>(d) & 15;
  if (mis) {
    const size_t head = 16 - mis < n ? 16 - mis : n;
    small(head);
    n -= head;
    cap -= head;
  }
#if HZ_REQCOPY_SSE2
  size_t i = 0;
  for (; i + 64 <= n; i += 64) {
    const __m128i a = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + i));
    const __m128i b = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + i + 16));
    const __m128i c = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + i + 32));
    const __m128i e = _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + i + 48));
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + i), a);
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + i + 16), b);
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + i + 32), c);
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + i + 48), e);
  }
  for (; i + 16 <= n; i += 16)
    _mm_stream_si128(reinterpret_cast<__m128i*>(d + i), _mm_loadu_si128(reinterpret_cast<const __m128i*>(s + i)));
  d += i, s += i;
  n -= i, cap -= i;
  if (n) {
    if (cap >= 16) {
      alignas(16) unsigned char last[16] = {};
      std::memcpy(last, s, n);
      _mm_stream_si128(reinterpret_cast<__m128i*>(d), _mm_load_si128(reinterpret_cast<const __m128i*>(last)));
    } else {
      small(n);
    }
  }
#else
  (void)cap;
  std::memcpy(d, s, n);
#endif
}

// Store fence: every hz_reqcopy store of this thread is globally visible (has left the
// write-combining buffers) before any later store.
static inline void hz_reqcopy_fence() {
#if HZ_REQCOPY_SSE2
  _mm_sfence();
#else
  std::atomic_thread_fence(std::memory_order_seq_cst);
#endif
}
