// reduce_check.hip -- checks vr_stage.h wave_min / wave_max (DPP + permlane swaps) and the joint
// packed reduction wave_min2x3 against a brute-force reduction over random inputs, every lane and
// every wave.
// Build: hipcc --offload-arch=gfx950 -O3 -I../../volume_renderer_amd/csrc reduce_check.hip
#include <hip/hip_runtime.h>
#include <stdio.h>
#include "vr_stage.h"

__global__ void k(const int *in, int *bad) {
  const int lane = threadIdx.x & 63;
  const int base = (blockIdx.x * blockDim.x + threadIdx.x) & ~63;
  const int v = in[base + lane];
  const int mn = vr::wave_min(v), mx = vr::wave_max(v);
  int bmn = in[base], bmx = in[base];
  for (int i = 1; i < 64; ++i) {
    bmn = min(bmn, in[base + i]);
    bmx = max(bmx, in[base + i]);
  }
  if (mn != bmn || mx != bmx) atomicAdd(bad, 1);
}

// three packed words per lane, made of six int16 fields of the wave's neighbours' inputs
__device__ __forceinline__ int field(const int *in, int base, int lane, int f) {
  return in[base + ((lane * 7 + 11 * f + 3) & 63)] * (f & 1 ? -3 : 2) + f;
}
__global__ void k3(const int *in, int *bad) {
  const int lane = threadIdx.x & 63;
  const int base = (blockIdx.x * blockDim.x + threadIdx.x) & ~63;
  int w[3], r[3];
  for (int j = 0; j < 3; ++j) w[j] = vr::pk2(field(in, base, lane, 2 * j), field(in, base, lane, 2 * j + 1));
  vr::wave_min2x3(w[0], w[1], w[2], r[0], r[1], r[2]);
  int ok = 1;
  for (int f = 0; f < 6; ++f) {
    int m = field(in, base, 0, f);
    for (int i = 1; i < 64; ++i) m = min(m, field(in, base, i, f));
    const int got = (f & 1) ? vr::pk_hi(r[f >> 1]) : vr::pk_lo(r[f >> 1]);
    ok &= got == m;
  }
  if (!ok) atomicAdd(bad, 1);
}

int main() {
  const int n = 64 * 4096;
  int *h = new int[n];
  unsigned s = 12345u;
  for (int i = 0; i < n; ++i) {
    s = s * 1664525u + 1013904223u;
    h[i] = (int)(s >> 8) % 4000 - 2000;
  }
  int *d, *bad, hb = 0, hb3 = 0;
  hipMalloc(&d, n * sizeof(int));
  hipMalloc(&bad, 2 * sizeof(int));
  hipMemcpy(d, h, n * sizeof(int), hipMemcpyHostToDevice);
  hipMemset(bad, 0, 2 * sizeof(int));
  k<<<n / 256, 256>>>(d, bad);
  k3<<<n / 256, 256>>>(d, bad + 1);
  hipMemcpy(&hb, bad, sizeof(int), hipMemcpyDeviceToHost);
  hipMemcpy(&hb3, bad + 1, sizeof(int), hipMemcpyDeviceToHost);
  printf("wave_min/wave_max mismatching lanes: %d of %d\n", hb, n);
  printf("wave_min2x3 mismatching lanes: %d of %d\n", hb3, n);
  return hb != 0 || hb3 != 0;
}
