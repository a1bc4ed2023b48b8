// Host-side sanitizer check of the request slots' streaming copy (csrc/reqcopy.h), stand-alone and
// CPU only: built with host ASan + UBSan (host code only) by tests/test_reqslot_cpu.py.
//
// Sources and destinations are exact-size heap blocks, so a read past the payload or a store past
// the bytes the caller owns (`cap`) is an ASan report. Sizes 0, 1, 15, 16, 17 and one 224 x 224 x 3
// image; sources at every byte phase; destinations 16-byte aligned (a slot) and at odd offsets (a row
// of a batched slot); cap = n (nothing past the payload may be touched) and cap = n rounded up to 16
// bytes (the last unit may be completed, with zeros).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "reqcopy.h"

#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); \
      return 1;                                                    \
    }                                                              \
  } while (0)

namespace {

constexpr unsigned char kGuard = 0xEE;

unsigned char pat(size_t i, size_t salt) { return (unsigned char)(i * 131 + salt * 17 + 3); }

// one copy: src at byte phase `sph` of a heap block, dst at offset `dph` of a 16-byte aligned heap
// block of exactly dph + cap bytes
int one(size_t n, size_t sph, size_t dph, bool padded) {
  const size_t cap = padded ? n + ((16 - (dph + n) % 16) % 16) : n;
  std::unique_ptr<unsigned char[]> sb(new unsigned char[sph + n + 1]);  // (+1: new[0] blocks are legal but odd)
  unsigned char* src = sb.get() + sph;
  for (size_t i = 0; i < n; ++i) src[i] = pat(i, n + sph);
  void* raw = nullptr;
  CHECK(posix_memalign(&raw, 16, dph + cap ? dph + cap : 16) == 0);
  unsigned char* db = static_cast<unsigned char*>(raw);
  std::memset(db, kGuard, dph + cap);
  hz_reqcopy(db + dph, src, n, cap);
  hz_reqcopy_fence();
  int bad = 0;
  for (size_t i = 0; i < dph; ++i) bad += db[i] != kGuard;                 // nothing before the destination
  for (size_t i = 0; i < n; ++i) bad += db[dph + i] != pat(i, n + sph);    // the payload
  for (size_t i = n; i < cap; ++i) bad += db[dph + i] != 0 && db[dph + i] != kGuard;  // zero fill or untouched
  free(raw);
  CHECK(bad == 0);
  return 0;
}

}  // namespace

int main() {
  const size_t sizes[] = {0, 1, 15, 16, 17, 150528};
  for (size_t n : sizes)
    for (size_t sph = 0; sph < 17; ++sph)
      for (size_t dph : {size_t(0), size_t(1), size_t(4), size_t(15)})
        for (bool padded : {false, true})
          if (one(n, sph, dph, padded)) {
            fprintf(stderr, "n=%zu src phase %zu dst phase %zu padded %d\n", n, sph, dph, (int)padded);
            return 1;
          }
  // a whole slot: cap is the slot's 16-byte rounded size, the payload any shorter length
  for (size_t n : {size_t(150528 - 5), size_t(33), size_t(31)})
    if (one(n, 3, 0, true)) return 1;
  printf("reqcopy host sanitize: ok\n");
  return 0;
}
