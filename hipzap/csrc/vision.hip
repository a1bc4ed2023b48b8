// Vision helper kernels: NHWC max-pool, global average pool, image pre-processing.
//  All are HBM/latency bound: 16-B vector loads (8 bf16
// channels per lane), one output vector per lane, grid sized to the output.
#include "common.h"
#include "hipzap.h"

HZ_DEBUG_UNIT(vision)

namespace {

// K x K window. With K known at compile time (the ResNet 3x3/2 stem pool) every tap is loaded
// before the first max: out-of-range taps are clamped to the nearest border pixel, which lies in
// the same window (a window overlapping the image contains its clamped taps), so the max is
// unchanged and no load is predicated — one memory round trip instead of a dependent chain of
// K*K (the runtime-K loop below compiled to one wait per tap).
template <int K>
__global__ __launch_bounds__(256) void maxpool_kernel(const HzPoolParams p) {
  const int C8 = p.C >> 3;
  const long total = (long)p.N * p.P * p.Q * C8;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c8 = i % C8;
  long t = i / C8;
  const int q = t % p.Q;
  t /= p.Q;
  const int pp = t % p.P;
  const int n = t / p.P;
  float m[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
  const int h0 = pp * p.stride - p.pad, w0 = q * p.stride - p.pad;
  if (!HZ_DCHECK(h0 < p.H && w0 < p.W && h0 + p.k > 0 && w0 + p.k > 0)) return;  // window overlaps the image
  if constexpr (K > 0) {
    u32x4 v[K * K];
#pragma unroll
    for (int r = 0; r < K; ++r) {
      const int ih = min(max(h0 + r, 0), p.H - 1);
#pragma unroll
      for (int s = 0; s < K; ++s) {
        const int iw = min(max(w0 + s, 0), p.W - 1);
        v[r * K + s] = *reinterpret_cast<const u32x4*>(p.x + (((long)n * p.H + ih) * p.W + iw) * p.C + c8 * 8);
      }
    }
#pragma unroll
    for (int j = 0; j < K * K; ++j) {
      float f[8];
      unpack8(v[j], f);
#pragma unroll
      for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], f[e]);
    }
  } else {
    for (int r = 0; r < p.k; ++r) {
      const int ih = h0 + r;
      if ((unsigned)ih >= (unsigned)p.H) continue;
      for (int s = 0; s < p.k; ++s) {
        const int iw = w0 + s;
        if ((unsigned)iw >= (unsigned)p.W) continue;
        const u32x4 v = *reinterpret_cast<const u32x4*>(p.x + (((long)n * p.H + ih) * p.W + iw) * p.C + c8 * 8);
        float f[8];
        unpack8(v, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], f[e]);
      }
    }
  }
  *reinterpret_cast<u32x4*>(p.out + i * 8) = pack8(m);
}

// [N, HW, C] -> [N, C]. One block per (image, 64 channels): 8 channel groups x 32 pixel
// lanes, so every lane issues only ceil(HW/32) independent 16-B loads (a serial HW loop per
// lane was a 49-deep dependent load chain: 15.7 us on MI355X), then an LDS reduction.
__global__ __launch_bounds__(256) void avgpool_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ out,
                                                      int N, int HW, int C, int blocked) {
  __shared__ float red[32][65];
  const int t = threadIdx.x, cg = t & 7, pl = t >> 3;
  const int cblk = C >> 6;
  const int n = blockIdx.x / cblk, c0 = (blockIdx.x - n * cblk) * 64;
  float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const int c = c0 + cg * 8;
  // blocked: [N][C/32][HW][32]; else NHWC [N][HW][C]
  const bf16_t* base = blocked ? x + (((long)n * (C >> 5) + (c >> 5)) * HW) * 32 + (c & 31) : x + (long)n * HW * C + c;
  const long pstride = blocked ? 32 : C;
  for (int j = pl; j < HW; j += 32) {
    float f[8];
    unpack8(*reinterpret_cast<const u32x4*>(base + (long)j * pstride), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] += f[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[pl][cg * 8 + e] = s[e];
  __syncthreads();
  if (t < 64) {
    float a = 0.f;
#pragma unroll 8
    for (int q = 0; q < 32; ++q) a += red[q][t];
    out[(long)n * C + c0 + t] = f2bf(a / HW);
  }
}

// Fused global-average-pool + FC (one launch instead of avgpool + FC GEMM + a kernel boundary).
// Block = one 16-row weight group x one image (blockIdx.y); its 4 waves split the channels
// (K) four ways, so each wave pools ONLY its own C/4 channels (fp32, into its LDS slice) and
// then dots them with its K-quarter of the group's weights; the 4 partial sums meet in LDS.
// Pooling: lane l reads 16 B (8 channels) of channel block (l>>2) of the wave's slice at every
// pixel. Weights are fragment-major (one contiguous 1 KiB per 32-deep k-step); the 4 lanes
// sharing an output row (l, l^16, l^32, l^48) reduce by shuffles.
// Latency: the wave's first WB weight fragments are issued before the pooling (independent of
// it). NB = ceil(HW/8) > 0 additionally issues ALL pixel loads before the first use (one round
// trip instead of one per 8 pixels) but needs 384 VGPRs at HW = 49: one workgroup per CU, which
// measured -1.5 % at 8 concurrent request streams (profiles/r1_ab/vision_latency.txt), so the
// runtime loop (NB = 0) is the default (HZ_POOLFC_STATIC).
#ifndef HZ_POOLFC_PB
#define HZ_POOLFC_PB 16  // pixel loads in flight per lane in the runtime loop: 4 round trips at HW = 49 (8: 7)
#endif
template <int NB>
__global__ __launch_bounds__(256) void pool_fc_kernel(const HzPoolFcParams p) {
  extern __shared__ __attribute__((aligned(16))) float pooled[];  // [C] + [4][16] partials
  constexpr int WB = 16;  // weight fragments in flight per wave
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.y, g = blockIdx.x;
  const int ncb = p.C >> 5;
  const int cpw = (ncb + 3) >> 2;  // channel blocks per wave
  const int cb_lo = wave * cpw, cb_hi = min(ncb, cb_lo + cpw);
  const float inv = 1.f / p.HW;
  const int ks = p.C >> 5;
  const bf16_t* wg = p.w + ((long)g * ks * 64 + lane) * 8;
  if (!HZ_DCHECK(p.ldo >= p.N && p.C % 32 == 0)) return;
  // first batch of weight fragments: independent of the pooling, so in flight with it
  u32x4 wv[WB];
#pragma unroll
  for (int j = 0; j < WB; ++j) wv[j] = *reinterpret_cast<const u32x4*>(wg + (long)min(cb_lo + j, cb_hi - 1) * 512);
  if (p.pooled) {  // x = the fp32 channel means already (a tail seam, block.hip): copy the wave's slice
    const float* xp = reinterpret_cast<const float*>(p.x) + (long)b * p.C;
    for (int c = cb_lo * 32 + lane * 4; c < cb_hi * 32; c += 256)
      *reinterpret_cast<f32x4*>(pooled + c) = *reinterpret_cast<const f32x4*>(xp + c);
  }
  for (int cb0 = cb_lo; cb0 < (p.pooled ? cb_lo : cb_hi); cb0 += 16) {
    const int cb = cb0 + (lane >> 2), sub = lane & 3;
    if (cb < cb_hi) {
      const bf16_t* src = p.x + (((long)b * ncb + cb) * p.HW) * 32 + sub * 8;
      float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
      if constexpr (NB > 0) {
        u32x4 v[NB * 8];
#pragma unroll
        for (int j = 0; j < NB * 8; ++j) v[j] = *reinterpret_cast<const u32x4*>(src + min(j, p.HW - 1) * 32);
#pragma unroll
        for (int j = 0; j < NB * 8; ++j) {
          float f[8];
          unpack8(v[j], f);
          const float wj = j < p.HW ? 1.f : 0.f;
#pragma unroll
          for (int e = 0; e < 8; ++e) s[e] += wj * f[e];
        }
      } else {
        for (int hw0 = 0; hw0 < p.HW; hw0 += HZ_POOLFC_PB) {  // PB independent loads in flight per lane
          u32x4 v[HZ_POOLFC_PB];
#pragma unroll
          for (int j = 0; j < HZ_POOLFC_PB; ++j)
            v[j] = *reinterpret_cast<const u32x4*>(src + min(hw0 + j, p.HW - 1) * 32);
#pragma unroll
          for (int j = 0; j < HZ_POOLFC_PB; ++j) {
            float f[8];
            unpack8(v[j], f);
            const float wj = hw0 + j < p.HW ? 1.f : 0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) s[e] += wj * f[e];
          }
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) pooled[cb * 32 + sub * 8 + e] = s[e] * inv;
    }
  }
  // the wave reads back only its own slice: a wave-level LDS fence is enough
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const float* pl = pooled + (lane >> 4) * 8;
  float acc = 0.f;
  for (int k0 = cb_lo; k0 < cb_hi; k0 += WB) {
    if (k0 != cb_lo) {  // later batches (C/4 > WB*32 channels per wave)
#pragma unroll
      for (int j = 0; j < WB; ++j) wv[j] = *reinterpret_cast<const u32x4*>(wg + (long)min(k0 + j, cb_hi - 1) * 512);
    }
#pragma unroll
    for (int j = 0; j < WB; ++j) {
      const int k = min(k0 + j, cb_hi - 1);
      float f[8];
      unpack8(wv[j], f);
      const f32x4 p0 = *reinterpret_cast<const f32x4*>(pl + k * 32);
      const f32x4 p1 = *reinterpret_cast<const f32x4*>(pl + k * 32 + 4);
      const float d = f[0] * p0[0] + f[1] * p0[1] + f[2] * p0[2] + f[3] * p0[3] + f[4] * p1[0] + f[5] * p1[1] +
                      f[6] * p1[2] + f[7] * p1[3];
      acc += k0 + j < cb_hi ? d : 0.f;
    }
  }
  acc += __shfl_xor(acc, 16, 64);
  acc += __shfl_xor(acc, 32, 64);
  float* part = pooled + p.C;  // [4 waves][16 rows]
  if (lane < 16) part[wave * 16 + lane] = acc;
  __syncthreads();
  const int n = g * 16 + t;
  if (t < 16 && n < p.N)
    p.out[(long)b * p.ldo + n] = part[t] + part[16 + t] + part[32 + t] + part[48 + t] + (p.bias ? p.bias[n] : 0.f);
}

// Global average pool [+ L2 normalisation] without the classifier: the ResNet embedding head
// (HzPoolNormParams). One workgroup per image; thread t owns channels 8t .. 8t + 7 (256 threads cover
// C = 2048), a thread whose channels lie past C loads and stores nothing and joins the norm's reductions
// with zeros. pooled == 0: per pixel one 16-B load of the channel-blocked input, HZ_POOLNORM_PB pixel
// loads in flight per lane; the pixels of a channel are summed in ascending order in fp32 and multiplied
// by 1.f / HW -- pool_fc_kernel's statements, so a channel mean has that kernel's bits. pooled == 1: x is
// the fp32 [B][C] channel means a tail seam wrote (block.hip): two 16-B loads, no arithmetic before the
// norm. normalize: squares summed per thread in channel order, a butterfly over the wave, the four wave
// values through LDS in wave order, then a true division by max(sqrt(sum), 1e-12): pool_embed_kernel's
// rule. Nothing crosses a workgroup and there is no atomic: an image's bits depend on that image alone.
// No address depends on data; columns C .. ldo - 1 of `out` are never written.
// Depth: the grid is B workgroups of one wave per SIMD, so occupancy hides nothing and VGPRs are free;
// the wall time is (round trips) x (L2-hit 180-225 cycles, HBM-miss ~900). 32 loads (128 VGPRs) make
// HW = 49 and 64 two round trips (16: four); 64 would be one, at 256 load VGPRs next to the rest.
#ifndef HZ_POOLNORM_PB
#define HZ_POOLNORM_PB 32
#endif
__global__ __launch_bounds__(256) void pool_norm_kernel(const HzPoolNormParams p) {
  __shared__ float sq[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int b = blockIdx.x;
  if (!HZ_DCHECK(p.C >= 32 && p.C % 32 == 0 && p.C <= 2048 && p.HW >= 1 && p.ldo >= p.C)) return;
  const bool own = t * 8 < p.C;
  float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (own && p.pooled) {
    const float* xp = reinterpret_cast<const float*>(p.x) + (long)b * p.C + t * 8;
    const f32x4 a = *reinterpret_cast<const f32x4*>(xp), c = *reinterpret_cast<const f32x4*>(xp + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] = a[e], s[4 + e] = c[e];
  } else if (own) {
    const float inv = 1.f / p.HW;
    const int cb = t >> 2, sub = t & 3;
    const bf16_t* src = p.x + (((long)b * (p.C >> 5) + cb) * p.HW) * 32 + sub * 8;
    for (int hw0 = 0; hw0 < p.HW; hw0 += HZ_POOLNORM_PB) {  // PB independent loads in flight per lane
      u32x4 v[HZ_POOLNORM_PB];
#pragma unroll
      for (int j = 0; j < HZ_POOLNORM_PB; ++j)
        v[j] = *reinterpret_cast<const u32x4*>(src + min(hw0 + j, p.HW - 1) * 32);
#pragma unroll
      for (int j = 0; j < HZ_POOLNORM_PB; ++j) {
        float f[8];
        unpack8(v[j], f);
        const float wj = hw0 + j < p.HW ? 1.f : 0.f;
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += wj * f[e];
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = s[e] * inv;
  }
  if (p.normalize) {  // (workgroup-uniform: every thread reaches the barrier)
    float ss = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) ss += s[e] * s[e];
    ss = warp_sum(ss);
    if (lane == 0) sq[wave] = ss;
    __syncthreads();
    const float nrm = fmaxf(sqrtf(sq[0] + sq[1] + sq[2] + sq[3]), 1e-12f);
#pragma unroll
    for (int e = 0; e < 8; ++e) s[e] = s[e] / nrm;
  }
  if (!own) return;
  float* o = p.out + (long)b * p.ldo + t * 8;
  if ((p.ldo & 3) == 0) {  // rows of `out` stay 16-B aligned
    *reinterpret_cast<f32x4*>(o) = f32x4{s[0], s[1], s[2], s[3]};
    *reinterpret_cast<f32x4*>(o + 4) = f32x4{s[4], s[5], s[6], s[7]};
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = s[e];
  }
}

// mode 0: src fp32 NCHW (already normalised unless mean/inv_std given)
// mode 1: src uint8 NHWC (raw image bytes, normalised with mean/inv_std in 0..1 scale)
__global__ __launch_bounds__(256) void preprocess_kernel(const void* __restrict__ src, bf16_t* __restrict__ dst,
                                                         int N, int Cin, int H, int W, int Cpad, int mode,
                                                         const float* __restrict__ mean,
                                                         const float* __restrict__ inv_std) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // pixel index
  const long HWl = (long)H * W;
  if (i >= N * HWl) return;
  const long n = i / HWl, hw = i - n * HWl;
  // every channel's load (and the normalisation constants) issued before the first use: a
  // runtime channel loop waited once per channel — over PCIe when the request is read zero-copy
  float v[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float f = 0.f;
    if (c < Cin) {
      if (mode == 0) f = reinterpret_cast<const float*>(src)[(n * Cin + c) * HWl + hw];
      else f = (float)reinterpret_cast<const unsigned char*>(src)[i * Cin + c];
    }
    v[c] = f;
  }
  // a byte: one fused multiply-add for u / 255 - mean, written out -- preprocess_u8c3_kernel's form, so
  // both kernels store the same bits for the same pixel whatever the compiler would contract
  if (mean) {
#pragma unroll
    for (int c = 0; c < 8; ++c)
      if (c < Cin) v[c] = (mode == 0 ? v[c] - mean[c] : __builtin_fmaf(v[c], 1.0f / 255.0f, -mean[c])) * inv_std[c];
  } else if (mode != 0) {
#pragma unroll
    for (int c = 0; c < 8; ++c) v[c] = v[c] * (1.0f / 255.0f);
  }
  bf16_t* o = dst + i * Cpad;
  *reinterpret_cast<u32x4*>(o) = pack8(v);
  for (int c = 8; c < Cpad; c += 8) *reinterpret_cast<u32x4*>(o + c) = u32x4{0, 0, 0, 0};
}

// uint8 HWC, 3 channels (the request payload of the vision models), read zero-copy from pinned host
// memory: the generic kernel's per-thread byte loads at stride 3 make every wave instruction touch the
// same three 64 B lines again (uncached over PCIe). Here a workgroup owns 1024 pixels = 3072 bytes:
// three fully coalesced dword loads per thread (768 distinct dwords, each read once), restaged through
// LDS so thread t then owns bytes [12t, 12t+12) = 4 whole pixels. Needs npix % 4 == 0 and a 4-byte
// aligned source (checked by the launcher; the generic kernel covers the rest).
__global__ __launch_bounds__(256) void preprocess_u8c3_kernel(const unsigned* __restrict__ src,
                                                              bf16_t* __restrict__ dst, long npix, int Cpad,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ inv_std) {
  __shared__ __attribute__((aligned(16))) unsigned buf[768];
  const int t = threadIdx.x;
  const long ndw = npix / 4 * 3;
  const long d0 = (long)blockIdx.x * 768;
  // the block's 3 KiB of request bytes as 16-B loads by threads 0..191 (zero-copy: the request is
  // read across PCIe, so fewer, wider requests: 1 KiB per wave instruction instead of 256 B)
  u32x4 r = u32x4{0u, 0u, 0u, 0u};
  if (t < 192) {
    const long d = d0 + 4 * t;
    if (d + 4 <= ndw) {
      r = *reinterpret_cast<const u32x4*>(src + d);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] = d + k < ndw ? src[d + k] : 0u;
    }
  }
  float mu[3] = {0.f, 0.f, 0.f}, is[3] = {1.f, 1.f, 1.f};
  if (mean) {
#pragma unroll
    for (int c = 0; c < 3; ++c) mu[c] = mean[c], is[c] = inv_std[c];
  }
  if (t < 192) *reinterpret_cast<u32x4*>(buf + 4 * t) = r;
  __syncthreads();
  const long px = (long)blockIdx.x * 1024 + 4 * t;
  if (px >= npix) return;
  const unsigned w[3] = {buf[3 * t], buf[3 * t + 1], buf[3 * t + 2]};
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    float v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int b = 3 * q + c;  // byte within the thread's 12
      const float u = (float)((w[b >> 2] >> (8 * (b & 3))) & 0xffu);
      // u / 255 - mean as one fused multiply-add (what the compiler made of it; preprocess_kernel does the same)
      v[c] = mean ? __builtin_fmaf(u, 1.0f / 255.0f, -mu[c]) * is[c] : u * (1.0f / 255.0f);
    }
    bf16_t* o = dst + (px + q) * Cpad;
    *reinterpret_cast<u32x4*>(o) = pack8(v);
    for (int c = 8; c < Cpad; c += 8) *reinterpret_cast<u32x4*>(o + c) = u32x4{0, 0, 0, 0};
  }
}

// ---- resize + centre crop + normalise (HzResizeParams) ----
// The taps of one output index of torch's antialiased bilinear resize (align_corners = false): source
// indices [lo, hi), weight(j) = max(0, 1 - |(j - center + 0.5) * inv|), normalised by their sum. Both
// ends are clamped into [0, in], so a tap index is a valid source index whatever the geometry says.
struct RszTaps {
  float center, inv;
  int lo, hi;
};
__device__ __forceinline__ int rsz_index(float v, int lo, int hi) {
  return min(max((int)fminf(fmaxf(v, 0.f), 1.0e9f), lo), hi);
}
__device__ __forceinline__ RszTaps rsz_taps(int i, float scale, int in) {
  const float support = scale >= 1.f ? scale : 1.f;
  RszTaps t;
  t.center = scale * ((float)i + 0.5f);
  t.inv = scale >= 1.f ? 1.f / scale : 1.f;
  t.lo = rsz_index(t.center - support + 0.5f, 0, in);
  t.hi = rsz_index(t.center + support + 0.5f, t.lo, in);
  return t;
}
__device__ __forceinline__ float rsz_weight(const RszTaps& t, int j) {
  return fmaxf(0.f, 1.f - fabsf(((float)j - t.center + 0.5f) * t.inv));
}
__device__ __forceinline__ float rsz_inv_total(const RszTaps& t) {
  float s = 0.f;
  for (int j = t.lo; j < t.hi; ++j) s += rsz_weight(t, j);
  return s > 0.f ? 1.f / s : 0.f;
}

#define HZ_RSZ_ROWS 8   // output rows per workgroup
#define HZ_RSZ_UNITS 8  // 16-B staging loads per thread per chunk: 256 * 8 * 16 B = 32 KiB of LDS
// A workgroup owns HZ_RSZ_ROWS output rows of one image, thread x one output column (3 channels). It
// walks the source rows the band's vertical taps cover: a chunk of rows is staged in LDS by aligned
// 16-B loads of only the columns the crop's horizontal taps cover (the request is read zero-copy from
// pinned host memory: wide requests, each byte once per band), the next chunk's loads are issued into
// registers before the staged one is consumed. Per source row a thread forms its horizontally filtered
// pixel from LDS and adds it into the band's output rows with their vertical weights (fp32 throughout;
// no intermediate image). Geometry comes from dims[b] and is wave-uniform except the thread's own column.
// rsz_band is that computation, shared by the two kernels below so that both form the same value for
// the same pixel: v[r][c] = the normalised fp32 pixel (band row r, the thread's column, channel c).
// Every thread of the workgroup runs it to the end (its barriers are workgroup-uniform); a thread past
// the crop's last column computes column crop - 1 again. `stage` is free once it returns.
__device__ __forceinline__ void rsz_band(const HzResizeParams& p, u32x4* stage, float (&v)[HZ_RSZ_ROWS][3]) {
  constexpr int R = HZ_RSZ_ROWS, U = HZ_RSZ_UNITS;
  const int t = threadIdx.x, b = blockIdx.y, oy0 = blockIdx.x * R;
  const int* d = p.dims + (long)b * 8;
  const int H = min(max(d[0], 1), p.maxH), W = min(max(d[1], 1), p.maxW);
  const int rh = min(max(d[2], 1), 1 << 16), rw = min(max(d[3], 1), 1 << 16);
  const int top = min(max(d[4], 0), 1 << 16), left = min(max(d[5], 0), 1 << 16);
  const float sy = (float)H / (float)rh, sx = (float)W / (float)rw;
  const unsigned char* img = p.image + (long)b * p.cap_bytes;

  RszTaps ty[R];
  float ity[R];
  int yhi = 0;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    ty[r] = rsz_taps(top + oy0 + r, sy, H);
    if (r > 0 && oy0 + r >= p.crop) ty[r].lo = ty[r].hi = ty[r - 1].hi;  // past the last output row: no taps
    ity[r] = rsz_inv_total(ty[r]);
    yhi = max(yhi, ty[r].hi);
  }
  const int ylo = ty[0].lo;
  const RszTaps tx = rsz_taps(left + min(t, p.crop - 1), sx, W);
  const float itx = rsz_inv_total(tx);
  // the columns any thread reads: [xlo, xhi) pixels; a staged row holds them from the 16-B boundary below
  const int xlo = rsz_taps(left, sx, W).lo;
  const int xhi = max(rsz_taps(left + p.crop - 1, sx, W).hi, xlo);
  const int upr = ((xhi - xlo) * 3 + 30) >> 4;  // 16-B units per staged row (launcher: <= 256 * U)
  const int NR = (256 * U) / upr;                // rows per chunk
  const long row_bytes = (long)W * 3;

  float acc[R][3];
#pragma unroll
  for (int r = 0; r < R; ++r) acc[r][0] = acc[r][1] = acc[r][2] = 0.f;

  u32x4 reg[U];
  auto fetch = [&](int y0) {
    const int nr = min(NR, yhi - y0);
#pragma unroll
    for (int i = 0; i < U; ++i) {
      const int u = t + 256 * i;
      const int row = u / upr, cu = u - row * upr;
      reg[i] = u32x4{0u, 0u, 0u, 0u};
      if (row < nr) {
        const long a = (((long)(y0 + row) * row_bytes + (long)xlo * 3) & ~15L) + (long)cu * 16;
        if (a + 16 <= p.cap_bytes) reg[i] = *reinterpret_cast<const u32x4*>(img + a);
      }
    }
  };
  if (ylo < yhi) fetch(ylo);
  const unsigned char* lds = reinterpret_cast<const unsigned char*>(stage);
  for (int y0 = ylo; y0 < yhi; y0 += NR) {
#pragma unroll
    for (int i = 0; i < U; ++i) stage[t + 256 * i] = reg[i];
    __syncthreads();
    if (y0 + NR < yhi) fetch(y0 + NR);
    const int nr = min(NR, yhi - y0);
    for (int row = 0; row < nr; ++row) {
      const int y = y0 + row;
      const int off = (int)(((long)y * row_bytes + (long)xlo * 3) & 15L);
      const unsigned char* s = lds + row * upr * 16 + off + (tx.lo - xlo) * 3;
      float h0 = 0.f, h1 = 0.f, h2 = 0.f;
      for (int j = tx.lo; j < tx.hi; ++j, s += 3) {
        const float w = rsz_weight(tx, j);
        h0 += w * (float)s[0];
        h1 += w * (float)s[1];
        h2 += w * (float)s[2];
      }
      h0 *= itx, h1 *= itx, h2 *= itx;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const float wy = (y >= ty[r].lo && y < ty[r].hi) ? rsz_weight(ty[r], y) * ity[r] : 0.f;
        acc[r][0] += wy * h0;
        acc[r][1] += wy * h1;
        acc[r][2] += wy * h2;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) v[r][c] = (acc[r][c] * (1.0f / 255.0f) - p.mean[c]) * p.inv_std[c];
}

// -> bf16 NHWC8 [B][crop][crop][8], channels 3..7 zero: one 16-B store per pixel.
__global__ __launch_bounds__(256) void resize_preprocess_kernel(const HzResizeParams p) {
  __shared__ __attribute__((aligned(16))) u32x4 stage[256 * HZ_RSZ_UNITS];
  constexpr int R = HZ_RSZ_ROWS;
  const int t = threadIdx.x, b = blockIdx.y, oy0 = blockIdx.x * R;
  float v[R][3];
  rsz_band(p, stage, v);
  if (t >= p.crop) return;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int oy = oy0 + r;
    if (oy >= p.crop) break;
    const float o[8] = {v[r][0], v[r][1], v[r][2], 0, 0, 0, 0, 0};
    *reinterpret_cast<u32x4*>(p.out + (((long)b * p.crop + oy) * p.crop + t) * 8) = pack8(o);
  }
}

// -> bf16 ViT patch rows [B * n * n][3 * 16 * 16], n = crop / 16, column (c, ky, kx): patchify_kernel's
// layout, written without the NHWC8 image in between. crop % 16 == 0 (launcher), so a band of 8 output
// rows is the upper or lower half (h) of one row of patches: ky in [8h, 8h + 8). A thread's 8 x 3
// values go as bf16 into an LDS tile [px][c][r][kx] (the staging buffer, free after the band's final
// barrier; 12 KiB at crop 256). For a fixed (px, c) the tile's 8 x 16 values are the 256 contiguous
// bytes at column c * 256 + h * 128 of patch row px, so 16-B chunk q of the tile goes to chunk q & 15
// of run q >> 4: consecutive lanes store consecutive 16 bytes. Threads past the crop's last column own
// no pixel but take part in the barrier and the write-out (crop 16: 48 chunks, 240 such threads).
__global__ __launch_bounds__(256) void resize_patchify_kernel(const HzResizeParams p) {
  __shared__ __attribute__((aligned(16))) u32x4 stage[256 * HZ_RSZ_UNITS];
  constexpr int R = HZ_RSZ_ROWS;
  const int t = threadIdx.x, b = blockIdx.y;
  float v[R][3];
  rsz_band(p, stage, v);  // ends on a barrier whenever it wrote `stage`
  bf16_t* tile = reinterpret_cast<bf16_t*>(stage);
  if (t < p.crop) {
    const int px = t >> 4, kx = t & 15;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
      for (int r = 0; r < R; ++r) tile[((px * 3 + c) * R + r) * 16 + kx] = f2bf(v[r][c]);
  }
  __syncthreads();
  const int n = p.crop >> 4, py = blockIdx.x >> 1, h = blockIdx.x & 1;
  bf16_t* row0 = p.out + ((long)b * n + py) * n * 768 + h * 128;
  for (int q = t; q < n * 48; q += 256) {
    const int run = q >> 4, px = run / 3, c = run - px * 3;
    *reinterpret_cast<u32x4*>(row0 + (long)px * 768 + c * 256 + (q & 15) * 8) = stage[q];
  }
}

// mode 2 (ViT patch embedding as a plain GEMM): src fp32 NCHW -> bf16 patch rows
// [N * (H/P) * (W/P)][Cin * P * P], column (c, ky, kx) = the flattened [D][Cin][P][P] conv weight's
// K order, so the patch projection is a row-major GEMM with K = Cin * P * P (768 at P = 16, Cin = 3)
// instead of an implicit-GEMM conv over 8-channel padded pixels (K 2048). A thread owns one
// (patch, c, ky) run of P pixels: P / 4 16-B loads, P / 8 16-B stores.
template <int P>
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst,
                                                       int N, int Cin, int H, int W,
                                                       const float* __restrict__ mean,
                                                       const float* __restrict__ inv_std) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // (patch row, c, ky)
  const int px = W / P, py = H / P;
  const long runs = (long)N * py * px * Cin * P;
  if (i >= runs) return;
  const int ky = (int)(i % P);
  const long t = i / P;
  const int c = (int)(t % Cin);
  const long row = t / Cin;  // n * py * px + pyi * px + pxi
  const int pxi = (int)(row % px);
  const long t2 = row / px;
  const int pyi = (int)(t2 % py);
  const long n = t2 / py;
  const float* s = src + ((n * Cin + c) * H + (long)pyi * P + ky) * W + (long)pxi * P;
  float v[P];
#pragma unroll
  for (int q = 0; q < P / 4; ++q) {
    const f32x4 f = *reinterpret_cast<const f32x4*>(s + 4 * q);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[4 * q + e] = f[e];
  }
  if (mean) {
    const float mu = mean[c], is = inv_std[c];
#pragma unroll
    for (int e = 0; e < P; ++e) v[e] = (v[e] - mu) * is;
  }
  bf16_t* o = dst + row * ((long)Cin * P * P) + (c * P + ky) * P;
#pragma unroll
  for (int q = 0; q < P / 8; ++q) *reinterpret_cast<u32x4*>(o + 8 * q) = pack8(v + 8 * q);
}

__global__ void cast_f32_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, long n) {
  const long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i + 3 < n) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + i);
    *reinterpret_cast<u32x2*>(y + i) = u32x2{pack2(v[0], v[1]), pack2(v[2], v[3])};
  } else {
    for (long j = i; j < n; ++j) y[j] = f2bf(x[j]);
  }
}
__global__ void cast_bf16_f32_kernel(const bf16_t* __restrict__ x, float* __restrict__ y, long n) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) y[i] = bf2f(x[i]);
}

}  // namespace

extern "C" int hz_maxpool_launch(const HzPoolParams* pp, hipStream_t st) {
  const HzPoolParams& p = *pp;
  if (!p.x || !p.out) return -1;
  if (p.C < 1 || p.C % 8 || p.N < 1 || p.H < 1 || p.W < 1 || p.P < 1 || p.Q < 1) return -1;
  if (p.k < 1 || p.stride < 1 || p.pad < 0 || p.pad >= p.k) return -1;
  // every window overlaps the image (with pad < k its first row and column do already)
  if ((long)(p.P - 1) * p.stride - p.pad >= p.H || (long)(p.Q - 1) * p.stride - p.pad >= p.W) return -1;
  const long total = (long)p.N * p.P * p.Q * (p.C / 8);
  // clamped taps are only inside the window when the padding is smaller than the window
  if (p.k == 3 && p.pad < 3) HZ_LAUNCH(maxpool_kernel<3>, dim3((total + 255) / 256), dim3(256), 0, st, p);
  else HZ_LAUNCH(maxpool_kernel<0>, dim3((total + 255) / 256), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

extern "C" int hz_avgpool_launch(const unsigned short* x, unsigned short* out, int N, int HW, int C, int blocked,
                                 hipStream_t st) {
  if (!x || !out || N < 1 || HW < 1 || C < 1 || C % 64) return -1;
  HZ_LAUNCH(avgpool_kernel, dim3(N * (C / 64)), dim3(256), 0, st, x, out, N, HW, C, blocked);
  return (int)hipGetLastError();
}

extern "C" int hz_pool_fc_launch(const HzPoolFcParams* pp, hipStream_t st) {
  const HzPoolFcParams& p = *pp;
  if (!p.x || !p.w || !p.out) return -1;
  if (p.C < 32 || p.C % 32 || p.C > 16384 || p.HW < 1 || p.N < 1 || p.B < 1 || p.ldo < p.N) return -1;
  const int groups = (p.N + 15) / 16;
  const size_t lds = (size_t)(p.C + 64) * sizeof(float);
  const dim3 grid(groups, p.B);
#ifndef HZ_POOLFC_STATIC
#define HZ_POOLFC_STATIC 0  // 1: measured -1.5 % at 8 streams (384 VGPRs, one workgroup per CU)
#endif
  switch (HZ_POOLFC_STATIC ? (p.HW + 7) / 8 : 0) {  // compile-time pixel batches: every pooling load in flight
    case 1: HZ_LAUNCH(pool_fc_kernel<1>, grid, dim3(256), lds, st, p); break;
    case 2: HZ_LAUNCH(pool_fc_kernel<2>, grid, dim3(256), lds, st, p); break;
    case 4: HZ_LAUNCH(pool_fc_kernel<4>, grid, dim3(256), lds, st, p); break;
    case 7: HZ_LAUNCH(pool_fc_kernel<7>, grid, dim3(256), lds, st, p); break;  // 7x7 (ResNet @224)
    default: HZ_LAUNCH(pool_fc_kernel<0>, grid, dim3(256), lds, st, p); break;
  }
  return (int)hipGetLastError();
}

extern "C" int hz_pool_norm_launch(const HzPoolNormParams* pp, hipStream_t st) {
  const HzPoolNormParams& p = *pp;
  if (!p.x || !p.out || ((uintptr_t)p.x & 15) || ((uintptr_t)p.out & 15)) return -1;  // 16-B loads and stores
  if (p.B < 1 || p.HW < 1) return -1;
  if (p.C < 32 || p.C % 32 || p.C > 2048) return -1;  // 256 threads x 8 channels
  if (p.ldo < p.C) return -1;
  HZ_LAUNCH(pool_norm_kernel, dim3(p.B), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

#ifndef HZ_PREPROC_GENERIC
#define HZ_PREPROC_GENERIC 0  // 1: uint8 3-channel payloads through the generic per-pixel kernel (A/B)
#endif
extern "C" int hz_preprocess_launch(const void* src, unsigned short* dst, int N, int Cin, int H, int W, int Cpad,
                                    int mode, const float* mean, const float* inv_std, hipStream_t st) {
  if (!src || !dst || mode < 0 || mode > 2 || N < 1 || H < 1 || W < 1 || (mean && !inv_std)) return -1;
  if (mode == 2) {  // patch rows; Cpad carries the patch size
    if (Cpad != 16 || H % 16 || W % 16 || Cin < 1 || Cin > 8 || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15))
      return -1;
    const long runs = (long)N * (H / 16) * (W / 16) * Cin * 16;
    HZ_LAUNCH(patchify_kernel<16>, dim3((runs + 255) / 256), dim3(256), 0, st,
                       static_cast<const float*>(src), reinterpret_cast<bf16_t*>(dst), N, Cin, H, W, mean, inv_std);
    return (int)hipGetLastError();
  }
  if (Cpad < 8 || Cpad % 8 || Cin < 1 || Cin > 8) return -1;
  const long total = (long)N * H * W;
  if (mode == 1 && Cin == 3 && total % 4 == 0 && ((uintptr_t)src & 15) == 0 && !HZ_PREPROC_GENERIC) {
    HZ_LAUNCH(preprocess_u8c3_kernel, dim3((total + 1023) / 1024), dim3(256), 0, st,
                       static_cast<const unsigned*>(src), dst, total, Cpad, mean, inv_std);
    return (int)hipGetLastError();
  }
  HZ_LAUNCH(preprocess_kernel, dim3((total + 255) / 256), dim3(256), 0, st, src, dst, N, Cin, H, W, Cpad,
                     mode, mean, inv_std);
  return (int)hipGetLastError();
}

extern "C" int hz_resize_preprocess_launch(const HzResizeParams* pp, hipStream_t st) {
  const HzResizeParams& p = *pp;
  if (p.B < 1 || p.crop < 1 || p.crop > 256 || p.maxH < 1 || p.maxW < 1 || !p.image || !p.dims || !p.out) return -1;
  // a staged row (maxW * 3 bytes + alignment slack) must fit the kernel's LDS chunk
  if (((long)p.maxW * 3 + 30) >> 4 > 256 * HZ_RSZ_UNITS) return -1;
  if (p.cap_bytes % 16 || (long long)p.maxH * p.maxW * 3 > p.cap_bytes) return -1;
  if (((uintptr_t)p.image & 15) || ((uintptr_t)p.out & 15) || ((uintptr_t)p.dims & 3)) return -1;
  const dim3 grid((p.crop + HZ_RSZ_ROWS - 1) / HZ_RSZ_ROWS, p.B);
  HZ_LAUNCH(resize_preprocess_kernel, grid, dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

extern "C" int hz_resize_patchify_launch(const HzResizeParams* pp, hipStream_t st) {
  const HzResizeParams& p = *pp;
  if (p.B < 1 || p.crop < 16 || p.crop > 256 || p.crop % 16 || p.maxH < 1 || p.maxW < 1 || !p.image || !p.dims ||
      !p.out)
    return -1;
  if (((long)p.maxW * 3 + 30) >> 4 > 256 * HZ_RSZ_UNITS) return -1;  // as above: a staged row fits the chunk
  if (p.cap_bytes % 16 || (long long)p.maxH * p.maxW * 3 > p.cap_bytes) return -1;
  if (((uintptr_t)p.image & 15) || ((uintptr_t)p.out & 15) || ((uintptr_t)p.dims & 3)) return -1;
  static_assert(HZ_RSZ_ROWS == 8 && 3 * HZ_RSZ_ROWS * 256 * 2 <= 256 * HZ_RSZ_UNITS * 16,
                "a band is half a patch row and its bf16 tile fits the staging buffer");
  const dim3 grid(p.crop / HZ_RSZ_ROWS, p.B);
  HZ_LAUNCH(resize_patchify_kernel, grid, dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

extern "C" int hz_cast_f32_bf16(const float* x, unsigned short* y, long n, hipStream_t st) {
  if (n < 1) return 0;  // nothing to convert: no launch (a grid of zero blocks is an error)
  if (!x || !y) return -1;
  const long threads = (n + 3) / 4;
  HZ_LAUNCH(cast_f32_bf16_kernel, dim3((threads + 255) / 256), dim3(256), 0, st, x, y, n);
  return (int)hipGetLastError();
}
extern "C" int hz_cast_bf16_f32(const unsigned short* x, float* y, long n, hipStream_t st) {
  if (n < 1) return 0;
  if (!x || !y) return -1;
  HZ_LAUNCH(cast_bf16_f32_kernel, dim3((n + 255) / 256), dim3(256), 0, st, x, y, n);
  return (int)hipGetLastError();
}

// Load this translation unit's device code now (hipFuncGetAttributes makes the runtime load the
// code object of the fatbin that holds the kernel, without a launch or a stream): the plan loader
// calls it on a helper thread while the weight blob uploads, so the first request does not pay
// the load (csrc/plan.cpp hz_plan_open).
__global__ void hz_vision_code_warm_kernel() {}
extern "C" int hz_vision_code_warm(void) {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&hz_vision_code_warm_kernel));
}
