// valu_rates.hip [OUT.json] -- issue throughput of the VALU instruction classes the ray-march uses
// (cycles per wave-instruction per SIMD, 16 independent chains per lane), at 8 and at 5 waves per
// SIMD (the march kernel's occupancy).  Two clocks per figure: wall time (HIP events) at the nominal
// clock the runtime reports, and the shader-clock counter (s_memtime) read by every wave around its
// own loop; s_memtime against the fixed-rate s_memrealtime gives the clock the body really ran at.
// With OUT.json: the table tools/isa_hot.py weights a loop's instruction mix by
// (tools/microbench/valu_costs.json).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#include <vector>

#define R16(X) X(0) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15)

// per wave: tm[4 w] = s_memtime delta and tm[4 w + 1] = s_memrealtime delta of its loop, tm[4 w + 2],
// tm[4 w + 3] = s_memrealtime at its start and end (their span over all waves against the kernel's
// wall time gives that counter's rate, and the sum of the deltas over the span the waves resident)
#define KERNEL(NAME, ASM)                                                                    \
  __global__ __launch_bounds__(256) void NAME(uint32_t *out, uint64_t *tm, uint32_t c, int iters) { \
    uint32_t v[16];                                                                          \
    for (int i = 0; i < 16; ++i) v[i] = threadIdx.x * 16 + i;                                \
    uint64_t w[16];                                                                          \
    for (int i = 0; i < 16; ++i) w[i] = v[i];                                                \
    (void)w;                                                                                 \
    const uint64_t m64 = 0x5555555555555555ull + c;                                          \
    (void)m64;                                                                               \
    const uint64_t t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime(); \
    for (int it = 0; it < iters; ++it) {                                                     \
      _Pragma("unroll") for (int i = 0; i < 16; ++i) { ASM; }                                \
    }                                                                                        \
    const uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime(); \
    uint32_t s = 0;                                                                          \
    for (int i = 0; i < 16; ++i) s += v[i] + (uint32_t)w[i];                                 \
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;                                          \
    if ((threadIdx.x & 63) == 0) {                                                           \
      const uint32_t wv = blockIdx.x * 4 + (threadIdx.x >> 6);                               \
      tm[4 * wv] = t1 - t0;                                                                  \
      tm[4 * wv + 1] = r1 - r0;                                                              \
      tm[4 * wv + 2] = r0;                                                                   \
      tm[4 * wv + 3] = r1;                                                                   \
    }                                                                                        \
  }

#define QP " quad_perm:[0,0,2,2] row_mask:0xf bank_mask:0xf"

KERNEL(k_fma, asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(v[i]) : "v"(c), "v"(v[(i + 1) & 15])))
KERNEL(k_fmac, asm volatile("v_fmac_f32 %0, %1, %2" : "+v"(v[i]) : "v"(c), "v"(v[(i + 1) & 15])))
KERNEL(k_fmaak, asm volatile("v_fmaak_f32 %0, %0, %1, 0x3f7ff000" : "+v"(v[i]) : "v"(c)))
KERNEL(k_fmamk, asm volatile("v_fmamk_f32 %0, %0, 0x3f7ff000, %1" : "+v"(v[i]) : "v"(c)))
KERNEL(k_mul, asm volatile("v_mul_f32 %0, %0, %1" : "+v"(v[i]) : "v"(c)))
KERNEL(k_addf, asm volatile("v_add_f32 %0, %0, %1" : "+v"(v[i]) : "v"(c)))
KERNEL(k_subf, asm volatile("v_sub_f32 %0, %1, %0" : "+v"(v[i]) : "v"(c)))
KERNEL(k_maxf, asm volatile("v_max_f32 %0, %0, %1" : "+v"(v[i]) : "v"(c)))
KERNEL(k_med3f, asm volatile("v_med3_f32 %0, %0, %1, %2" : "+v"(v[i]) : "v"(c), "v"(v[(i + 1) & 15])))
KERNEL(k_pkfma, asm volatile("v_pk_fma_f32 %0, %0, %1, %1" : "+v"(w[i]) : "v"((uint64_t)c)))
KERNEL(k_pkmul, asm volatile("v_pk_mul_f32 %0, %0, %1" : "+v"(w[i]) : "v"((uint64_t)c)))
KERNEL(k_pkadd, asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(w[i]) : "v"((uint64_t)c)))
KERNEL(k_addu, asm volatile("v_add_u32 %0, %0, %1" : "+v"(v[i]) : "v"(c)))
KERNEL(k_add3u, asm volatile("v_add3_u32 %0, %0, %1, %2" : "+v"(v[i]) : "v"(c), "v"(v[(i + 1) & 15])))
KERNEL(k_addlshl, asm volatile("v_add_lshl_u32 %0, %0, %1, 2" : "+v"(v[i]) : "v"(c)))
KERNEL(k_lshladd, asm volatile("v_lshl_add_u32 %0, %0, 2, %1" : "+v"(v[i]) : "v"(c)))
KERNEL(k_lshl, asm volatile("v_lshlrev_b32 %0, 1, %0" : "+v"(v[i])))
KERNEL(k_and, asm volatile("v_and_b32 %0, %0, %1" : "+v"(v[i]) : "v"(c)))
KERNEL(k_xor, asm volatile("v_xor_b32 %0, %0, %1" : "+v"(v[i]) : "v"(c)))
KERNEL(k_andor, asm volatile("v_and_or_b32 %0, %0, %1, %2" : "+v"(v[i]) : "v"(c), "v"(v[(i + 1) & 15])))
KERNEL(k_bfi, asm volatile("v_bfi_b32 %0, %1, %0, %2" : "+v"(v[i]) : "v"(c), "v"(v[(i + 1) & 15])))
KERNEL(k_mini, asm volatile("v_min_i32 %0, %0, %1" : "+v"(v[i]) : "v"(c)))
KERNEL(k_med3i, asm volatile("v_med3_i32 %0, %0, %1, %2" : "+v"(v[i]) : "v"(c), "v"(v[(i + 1) & 15])))
KERNEL(k_mad24, asm volatile("v_mad_u32_u24 %0, %0, %1, %2" : "+v"(v[i]) : "v"(c), "v"(v[(i + 1) & 15])))
KERNEL(k_cvt, asm volatile("v_cvt_i32_f32 %0, %0" : "+v"(v[i])))
KERNEL(k_cvtf, asm volatile("v_cvt_f32_i32 %0, %0" : "+v"(v[i])))
KERNEL(k_floor, asm volatile("v_floor_f32 %0, %0" : "+v"(v[i])))
KERNEL(k_fract, asm volatile("v_fract_f32 %0, %0" : "+v"(v[i])))
KERNEL(k_rndne, asm volatile("v_rndne_f32 %0, %0" : "+v"(v[i])))
KERNEL(k_cnd, asm volatile("v_cmp_gt_f32 vcc, %0, %1\n v_cndmask_b32 %0, %0, %1, vcc" : "+v"(v[i]) : "v"(c) : "vcc"))
KERNEL(k_cmp, asm volatile("v_cmp_gt_f32 vcc, %0, %1" : : "v"(v[i]), "v"(c) : "vcc"))
KERNEL(k_cmp64, asm volatile("v_cmp_gt_f32_e64 s[2:3], %0, %1" : : "v"(v[i]), "v"(c) : "s2", "s3"))
// the selects alone: the mask is set before the loop (VOP2 reads vcc, VOP3 any SGPR pair)
KERNEL(k_cnd2, asm volatile("v_cndmask_b32_e32 %0, %0, %1, vcc" : "+v"(v[i]) : "v"(v[(i + 1) & 15])))
KERNEL(k_cnd3, asm volatile("v_cndmask_b32_e64 %0, %0, %1, %2" : "+v"(v[i]) : "v"(v[(i + 1) & 15]), "s"(m64)))
KERNEL(k_mullo, asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(v[i]) : "v"(c)))
KERNEL(k_lshl64, asm volatile("v_lshl_add_u64 %0, %0, 2, %0" : "+v"(w[i])))
KERNEL(k_sqrt, asm volatile("v_sqrt_f32 %0, %0" : "+v"(v[i])))
KERNEL(k_rsq, asm volatile("v_rsq_f32 %0, %0" : "+v"(v[i])))
KERNEL(k_rcp, asm volatile("v_rcp_f32 %0, %0" : "+v"(v[i])))
KERNEL(k_mov, asm volatile("v_mov_b32 %0, %1" : "=v"(v[i]) : "v"(v[(i + 1) & 15])))
KERNEL(k_readlane, asm volatile("v_readlane_b32 s2, %0, 3" : : "v"(v[i]) : "s2"))
// DPP: the source register was written 15 instructions earlier (no wait states owed)
KERNEL(k_movdpp, asm volatile("v_mov_b32_dpp %0, %1" QP : "+v"(v[i]) : "v"(v[(i + 1) & 15])))
KERNEL(k_fmacdpp, asm volatile("v_fmac_f32_dpp %0, %1, %2" QP : "+v"(v[i]) : "v"(v[(i + 1) & 15]), "v"(c)))
// the depth-lane compositing step both ways (per step): a DPP move and an fma, or the fused fmac
KERNEL(k_movdpp_fma, uint32_t t; asm volatile("v_mov_b32_dpp %1, %2" QP "\n v_fma_f32 %0, %3, %1, %0"
                                              : "+v"(v[i]), "=&v"(t) : "v"(v[(i + 1) & 15]), "v"(c)))

typedef void (*kfn)(uint32_t *, uint64_t *, uint32_t, int);
int main(int argc, char **argv) {
  uint32_t *o;
  uint64_t *tm;
  const int maxblocks = 2048;
  hipMalloc(&o, 256u * maxblocks * 4);
  hipMalloc(&tm, (size_t)maxblocks * 4 * 4 * 8);
  hipEvent_t e0, e1;
  hipEventCreate(&e0);
  hipEventCreate(&e1);
  struct { const char *n; kfn f; } ks[] = {
      {"v_fma_f32", k_fma}, {"v_fmac_f32", k_fmac}, {"v_fmaak_f32", k_fmaak}, {"v_fmamk_f32", k_fmamk},
      {"v_mul_f32", k_mul}, {"v_add_f32", k_addf}, {"v_sub_f32", k_subf}, {"v_max_f32", k_maxf},
      {"v_med3_f32", k_med3f}, {"v_pk_fma_f32", k_pkfma}, {"v_pk_mul_f32", k_pkmul}, {"v_pk_add_f32", k_pkadd},
      {"v_add_u32", k_addu}, {"v_add3_u32", k_add3u}, {"v_add_lshl_u32", k_addlshl}, {"v_lshl_add_u32", k_lshladd},
      {"v_lshlrev_b32", k_lshl}, {"v_and_b32", k_and}, {"v_xor_b32", k_xor}, {"v_and_or_b32", k_andor},
      {"v_bfi_b32", k_bfi}, {"v_min_i32", k_mini}, {"v_med3_i32", k_med3i}, {"v_mad_u32_u24", k_mad24},
      {"v_cvt_i32_f32", k_cvt}, {"v_cvt_f32_i32", k_cvtf}, {"v_floor_f32", k_floor}, {"v_fract_f32", k_fract},
      {"v_rndne_f32", k_rndne}, {"v_cmp+v_cndmask", k_cnd}, {"v_cmp_gt_f32", k_cmp}, {"v_cmp_gt_f32_e64", k_cmp64},
      {"v_cndmask_b32_e32", k_cnd2}, {"v_cndmask_b32_e64", k_cnd3}, {"v_mul_lo_u32", k_mullo},
      {"v_lshl_add_u64", k_lshl64}, {"v_sqrt_f32", k_sqrt}, {"v_rsq_f32", k_rsq}, {"v_rcp_f32", k_rcp},
      {"v_mov_b32", k_mov}, {"v_readlane_b32", k_readlane}, {"v_mov_b32_dpp", k_movdpp},
      {"v_fmac_f32_dpp", k_fmacdpp}, {"v_mov_b32_dpp+v_fma_f32", k_movdpp_fma}};
  int dev;
  hipGetDevice(&dev);
  hipDeviceProp_t p;
  hipGetDeviceProperties(&p, dev);
  const int cus = p.multiProcessorCount, iters = 4000;
  printf("CUs %d, nominal clock %d kHz\n", cus, p.clockRate);
  FILE *js = argc > 1 ? fopen(argv[1], "w") : nullptr;
  if (js) fprintf(js, "{\"nominal_mhz\": %.1f, \"cus\": %d", p.clockRate * 1e-3, cus);
  const int wps[2] = {8, 5};
  for (int wi = 0; wi < 2; ++wi) {
    const int W = wps[wi], blocks = cus * W;  // 4-wave workgroups: W waves per SIMD
    if (blocks > maxblocks) return 2;
    std::vector<uint64_t> h((size_t)blocks * 16);
    printf("%d waves per SIMD: cycles / wave-instr / SIMD by wall time at the nominal clock | by s_memtime | "
           "s_memtime MHz (s_memrealtime taken as 100 MHz) | s_memrealtime MHz by span / wall | waves resident per SIMD\n", W);
    std::vector<double> wallc, memc;
    double mhz_sum = 0, rt_sum = 0, res_sum = 0;
    for (auto &k : ks) {
      for (int rep = 0; rep < 2; ++rep) {
        hipEventRecord(e0);
        k.f<<<blocks, 256>>>(o, tm, 0x3f7ff000u, iters);
        hipEventRecord(e1);
        hipEventSynchronize(e1);
        float ms;
        hipEventElapsedTime(&ms, e0, e1);
        if (rep) {
          hipMemcpy(h.data(), tm, h.size() * 8, hipMemcpyDeviceToHost);
          double dt = 0, dr = 0;
          uint64_t rmin = ~0ull, rmax = 0;
          for (int i = 0; i < blocks * 4; ++i) {
            dt += (double)h[4 * i], dr += (double)h[4 * i + 1];
            rmin = h[4 * i + 2] < rmin ? h[4 * i + 2] : rmin;
            rmax = h[4 * i + 3] > rmax ? h[4 * i + 3] : rmax;
          }
          const double span = (double)(rmax - rmin), resident = span > 0 ? dr / span / (cus * 4.0) : 0;
          dt /= blocks * 4, dr /= blocks * 4;
          const double winstr = (double)iters * 16 * W;  // per SIMD
          const double wall = ms * 1e-3 * p.clockRate * 1e3 / winstr, cyc = dt / winstr;
          const double mhz = dr > 0 ? dt / dr * 100.0 : 0, rt = span / (ms * 1e3);
          mhz_sum += mhz, rt_sum += rt, res_sum += resident;
          wallc.push_back(wall), memc.push_back(cyc);
          printf("%-24s %6.2f | %6.2f | %6.0f | %6.1f | %5.2f  (%.3f ms)\n", k.n, wall, cyc, mhz, rt, resident, ms);
        }
      }
    }
    const int nk = (int)wallc.size();
    printf("means over the bodies: s_memtime %.0f MHz, s_memrealtime %.1f MHz, %.2f waves resident per SIMD\n",
           mhz_sum / nk, rt_sum / nk, res_sum / nk);
    if (js) {
      fprintf(js, ", \"waves_%d\": {\"memtime_mhz\": %.1f, \"memrealtime_mhz\": %.2f, \"resident_waves\": %.2f", W,
              mhz_sum / nk, rt_sum / nk, res_sum / nk);
      for (int pass = 0; pass < 2; ++pass) {
        fprintf(js, ", \"%s\": {", pass ? "memtime" : "wall");
        for (int i = 0; i < nk; ++i) fprintf(js, "%s\"%s\": %.3f", i ? ", " : "", ks[i].n, pass ? memc[i] : wallc[i]);
        fprintf(js, "}");
      }
      fprintf(js, "}");
    }
  }
  if (js) fprintf(js, "}\n"), fclose(js);
  return 0;
}
