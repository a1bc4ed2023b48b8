// Measures the fp32 device math of the AWD-LSTM decode kernels (csrc/lstm.hip, csrc/common.h gumbel_of)
// against fp64 on dense grids: the source of E_SIG, E_TANH and E_LOG in tests/lm_oracle.py.
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -munsafe-fp-atomics scripts/native/ulp_probe.hip -o scripts/native/ulp_probe
// Output: one line per (function, bin of 2^24 / 64 arguments): name bin x_first x_some max_abs_err max_rel_err
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

constexpr int NBIN = 64;

__device__ void upd(unsigned long long* slot, double v) {
  if (!(v >= 0.0)) v = INFINITY;  // NaN counts as infinite error
  atomicMax(slot, (unsigned long long)__double_as_longlong(v));
}

// f: 0 sigmoid via __expf on [-16,16]; 1 tanhf on [-8,8]; 2 __expf on [-16,16];
//    3 inner: L = -__logf(u), u = (k + 0.5f) 2^-24 for all k in [0, 2^24) (every second one is a u of
//    gumbel_of); 4 outer: __logf(x), x log-spaced in [2^-26, 32]; 5 gumbel_of's whole expression on the
//    u of 3 against fp64 of the exact (k + .5) / 2^24 (k + 0.5f is not exact above 2^23: why gumbel_of
//    takes 23 bits)
__global__ void probe(int f, long n, unsigned long long* out, double* xr) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int bin = (int)(i * NBIN / n);
  float got;
  double ref, x;
  if (f == 0) {
    const float xf = -16.f + 32.f * ((float)i / (float)n);
    x = xf;
    got = 1.f / (1.f + __expf(-xf));
    ref = 1.0 / (1.0 + exp(-(double)xf));
  } else if (f == 1) {
    const float xf = -8.f + 16.f * ((float)i / (float)n);
    x = xf;
    got = tanhf(xf);
    ref = tanh((double)xf);
  } else if (f == 2) {
    const float xf = -16.f + 32.f * ((float)i / (float)n);
    x = xf;
    got = __expf(xf);
    ref = exp((double)xf);
  } else if (f == 3) {
    const float u = ((float)(unsigned)i + 0.5f) * (1.0f / 16777216.0f);
    x = u;
    if (u >= 1.f) return;
    got = -__logf(u);
    ref = -log((double)u);
  } else if (f == 4) {
    const float xf = exp2f(-26.f + 31.f * ((float)i / (float)n));
    x = xf;
    got = __logf(xf);
    ref = log((double)xf);
  } else {
    const float u = ((float)(unsigned)i + 0.5f) * (1.0f / 16777216.0f);
    x = ((double)i + 0.5) / 16777216.0;
    got = -__logf(-__logf(u));
    ref = -log(-log(x));
  }
  const double e = fabs((double)got - ref);
  upd(out + 2 * bin, e);
  upd(out + 2 * bin + 1, ref != 0.0 ? e / fabs(ref) : (e == 0.0 ? 0.0 : INFINITY));
  if (i == (long)bin * n / NBIN || i * NBIN == (long)bin * n) xr[2 * bin] = x;
  xr[2 * bin + 1] = x;  // some x of the bin (racy on purpose: any member will do)
}

int main() {
  const char* names[6] = {"sigmoid", "tanhf", "expf", "log_inner", "log_outer", "gumbel"};
  const long ns[6] = {1L << 24, 1L << 24, 1L << 24, 1L << 24, 1L << 24, 1L << 24};
  unsigned long long* d;
  double* xr;
  if (hipMalloc(&d, NBIN * 2 * 8) != hipSuccess || hipMalloc(&xr, NBIN * 2 * 8) != hipSuccess) return 2;
  for (int f = 0; f < 6; ++f) {
    hipMemset(d, 0, NBIN * 2 * 8);
    hipMemset(xr, 0, NBIN * 2 * 8);
    hipLaunchKernelGGL(probe, dim3((unsigned)((ns[f] + 255) / 256)), dim3(256), 0, 0, f, ns[f], d, xr);
    if (hipDeviceSynchronize() != hipSuccess) return 3;
    std::vector<double> h(NBIN * 2), hx(NBIN * 2);
    hipMemcpy(h.data(), d, NBIN * 2 * 8, hipMemcpyDeviceToHost);
    hipMemcpy(hx.data(), xr, NBIN * 2 * 8, hipMemcpyDeviceToHost);
    for (int b = 0; b < NBIN; ++b) {
      char line[256];
      snprintf(line, sizeof line, "%s %d %.9g %.9g %.6e %.6e\n", names[f], b, hx[2 * b], hx[2 * b + 1], h[2 * b],
               h[2 * b + 1]);
      fputs(line, stdout);
    }
  }
  return 0;
}
