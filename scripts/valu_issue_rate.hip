// Issue rate of wave64 vector instructions: what one SIMD sustains at W waves per SIMD, and what the profiler's
// VALU counters say of a kernel that does nothing else (profiles/pq_mmajor_before.txt); and the prices of what a look-up
// address of the PQ scan can be made of (profiles/pq_adc_addr_issue_rate.txt, profiles/pq_adc_dot4_issue_rate.txt).
//   hipcc -O3 --offload-arch=gfx950 -o valu_issue_rate scripts/valu_issue_rate.hip && ./valu_issue_rate
//   rocprofv3 --pmc VALUBusy SQ_INSTS_VALU SQ_ACTIVE_INST_VALU GRBM_GUI_ACTIVE -- ./valu_issue_rate
// Workgroups of 4 waves (one per SIMD); the LDS size keeps exactly W of them on a CU. Per wave: s_memtime ticks
// around 65 536 independent instructions; per kernel: wall time over instructions per SIMD.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <vector>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("hip error %s at %d\n", hipGetErrorString(e_), __LINE__); exit(2); } } while (0)

constexpr int ITER = 4096, UNR = 16;   // 65536 instructions per wave

template <int KIND>
__global__ void k(float *out, long long *ticks, float seed) {
  extern __shared__ char lds[];
  float a[UNR];
  for (int i = 0; i < UNR; i++) a[i] = seed + threadIdx.x * 0.001f + i;
  const float b = seed * 0.5f, c = seed * 0.25f;
  float one = seed, tiny = seed * 0x1p-142f;
  asm volatile("" : "+v"(one), "+v"(tiny));
  if (KIND == 23 || KIND == 26)   // denormal accumulators: they stay below 2^23 ulps over the whole loop
    for (int i = 0; i < UNR; i++) a[i] = __int_as_float((int)(threadIdx.x & 127) + i);
  int v7 = 7;
  asm volatile("" : "+v"(v7));
  int smask = __builtin_amdgcn_readfirstlane(0x7f80 + (int)seed - 1);   // a mask in a scalar register
  // v_dot4_u32_u8 D = sum of a.u8[i] * b.u8[i], plus c: with the one-hot selector 0x80 << (8 k) that is
  // byte k of a, times 128, plus c (profiles/pq_adc_dot4_issue_rate.txt). KIND 30 + k: the selector in a scalar
  // register; 34 + k: in a vector register; vadd: the addend, a vector register in all of them
  constexpr int DOTK = KIND >= 30 && KIND <= 37 ? (KIND - 30) & 3 : KIND == 39 ? 3 : KIND == 38 ? 1 : 0;
  const int ssel = __builtin_amdgcn_readfirstlane((0x80 << (8 * DOTK)) + (int)seed - 1);
  int vsel = ssel, vadd = (int)(threadIdx.x & 31) * 4;
  asm volatile("" : "+v"(vsel), "+v"(vadd));
  if (KIND >= 30 && KIND <= 45)   // small integers: as floats they are the denormals of the mixed loops' v_fma_f32
    for (int i = 0; i < UNR; i++) a[i] = __int_as_float((int)(threadIdx.x & 127) + i);
  __syncthreads();
  const long long t0 = __builtin_readcyclecounter();
  for (int it = 0; it < ITER; it++) {
#pragma unroll
    for (int i = 0; i < UNR; i++) {
      if (KIND >= 30 && KIND <= 33) asm volatile("v_dot4_u32_u8 %0, %0, %1, %2" : "+v"(a[i]) : "s"(ssel), "v"(vadd));
      if (KIND >= 34 && KIND <= 37) asm volatile("v_dot4_u32_u8 %0, %0, %1, %2" : "+v"(a[i]) : "v"(vsel), "v"(vadd));
      if (KIND == 38) asm volatile("v_dot4_u32_u8 %0, %0, %1, 0" : "+v"(a[i]) : "s"(ssel));        // no addend register
      if (KIND == 39) asm volatile("v_dot4_u32_u8 %0, %1, %2, %0" : "+v"(a[i]) : "v"(vadd), "s"(ssel));   // the addend is the chain
      // mixed loops, 1:1: does the price of v_dot4_u32_u8 add to a full-rate instruction's or overlap with it
      if (KIND == 40 || KIND == 41 || KIND == 43) {
        if (i & 1) {
          if (KIND == 40) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(a[i]) : "v"(one), "v"(tiny));
          if (KIND == 41) asm volatile("v_and_b32 %0, 0xff, %0" : "+v"(a[i]));
          if (KIND == 43) asm volatile("v_lshrrev_b32 %0, 1, %0" : "+v"(a[i]));
        } else {
          asm volatile("v_dot4_u32_u8 %0, %0, %1, %2" : "+v"(a[i]) : "s"(ssel), "v"(vadd));
        }
      }
      if (KIND == 42) {   // today's pair: v_and_b32 and the denormal v_fma_f32, 1:1
        if (i & 1) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(a[i]) : "v"(one), "v"(tiny));
        else asm volatile("v_and_b32 %0, 0xff, %0" : "+v"(a[i]));
      }
      if (KIND == 44) {   // byte 3 today: v_lshrrev_b32 and the denormal v_fma_f32, 1:1
        if (i & 1) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(a[i]) : "v"(one), "v"(tiny));
        else asm volatile("v_lshrrev_b32 %0, 1, %0" : "+v"(a[i]));
      }
      if (KIND == 45) {   // dot4 and a half-rate instruction, 1:1
        if (i & 1) asm volatile("v_lshl_add_u32 %0, %0, 7, %1" : "+v"(a[i]) : "v"(b));
        else asm volatile("v_dot4_u32_u8 %0, %0, %1, %2" : "+v"(a[i]) : "s"(ssel), "v"(vadd));
      }
      if (KIND == 0) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
      if (KIND == 1) asm volatile("v_add_f32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
      if (KIND == 2) asm volatile("v_add_f32_dpp %0, %1, %0 row_mirror row_mask:0xf bank_mask:0xf" : "+v"(a[i]) : "v"(a[(i + 1) % UNR]));
      if (KIND == 3) asm volatile("v_lshl_add_u32 %0, %0, 7, %1" : "+v"(a[i]) : "v"(b));
      if (KIND == 4) asm volatile("v_and_b32 %0, 0xff, %0" : "+v"(a[i]));
      if (KIND == 5) asm volatile("v_bfe_u32 %0, %0, 8, 8" : "+v"(a[i]));
      // what a cheaper look-up address could be made of (profiles/pq_adc_addr_issue_rate.txt); v7 holds 7
      if (KIND == 6) asm volatile("v_lshlrev_b32_sdwa %0, %1, %0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0" : "+v"(a[i]) : "v"(v7));
      if (KIND == 7) asm volatile("v_lshlrev_b32_sdwa %0, %1, %0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "+v"(a[i]) : "v"(v7));
      if (KIND == 8) asm volatile("v_lshlrev_b32_sdwa %0, %1, %0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_2" : "+v"(a[i]) : "v"(v7));
      if (KIND == 9) asm volatile("v_lshlrev_b32_sdwa %0, %1, %0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_3" : "+v"(a[i]) : "v"(v7));
      if (KIND == 10) asm volatile("v_or_b32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
      if (KIND == 11) asm volatile("v_add_u32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
      if (KIND == 12) asm volatile("v_lshrrev_b32 %0, 1, %0" : "+v"(a[i]));
      if (KIND == 13) asm volatile("v_and_or_b32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
      if (KIND == 14) asm volatile("v_bfi_b32 %0, %1, %0, %2" : "+v"(a[i]) : "v"(b), "v"(c));
      if (KIND == 15) asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
      if (KIND == 16) asm volatile("v_mad_u32_u24 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
      if (KIND == 17) asm volatile("v_lshl_or_b32 %0, %0, 7, %1" : "+v"(a[i]) : "v"(b));
      if (KIND == 18) asm volatile("v_and_or_b32 %0, %0, %1, %2" : "+v"(a[i]) : "s"(smask), "v"(c));
      // the address as a denormal float: byte -> float, then fma(c, 2^-142, lane offset's bits) = bits c * 128 + offset
      if (KIND == 20) asm volatile("v_cvt_f32_ubyte0 %0, %0" : "+v"(a[i]));
      if (KIND == 21) asm volatile("v_cvt_f32_ubyte1 %0, %0" : "+v"(a[i]));
      if (KIND == 22) asm volatile("v_cvt_f32_ubyte3 %0, %0" : "+v"(a[i]));
      if (KIND == 23) asm volatile("v_fma_f32 %0, %1, %2, %0" : "+v"(a[i]) : "v"(one), "v"(tiny));
      if (KIND == 26) asm volatile("v_fmamk_f32 %0, %1, 0x80, %0" : "+v"(a[i]) : "v"(one));   // the same with 2^-142 as a literal
      if (KIND == 24) asm volatile("v_lshlrev_b32 %0, 7, %0" : "+v"(a[i]));
      if (KIND == 25) asm volatile("v_and_b32 %0, %1, %0" : "+v"(a[i]) : "s"(smask));
      if (KIND == 19) asm volatile("v_mul_u32_u24_sdwa %0, %1, %0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_1" : "+v"(a[i]) : "v"(v7));
    }
  }
  const long long t1 = __builtin_readcyclecounter();
  float s = 0;
  for (int i = 0; i < UNR; i++) s += a[i];
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
  if ((threadIdx.x & 63) == 0) ticks[blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64] = t1 - t0;
}

template <int KIND>
__global__ void kpk(float *out, long long *ticks, float seed) {   // v_pk_add_f32: two floats per lane
  extern __shared__ char lds[];
  typedef float f2 __attribute__((ext_vector_type(2)));
  f2 a[UNR];
  for (int i = 0; i < UNR; i++) a[i] = f2{seed + threadIdx.x * 0.001f + i, seed};
  const f2 b = {seed * 0.5f, seed * 0.25f};
  __syncthreads();
  const long long t0 = __builtin_readcyclecounter();
  for (int it = 0; it < ITER; it++) {
#pragma unroll
    for (int i = 0; i < UNR; i++) asm volatile("v_pk_add_f32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
  }
  const long long t1 = __builtin_readcyclecounter();
  float s = 0;
  for (int i = 0; i < UNR; i++) s += a[i].x + a[i].y;
  out[blockIdx.x * blockDim.x + threadIdx.x] = s;
  if ((threadIdx.x & 63) == 0) ticks[blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64] = t1 - t0;
}

template <typename F>
static void run(const char *name, F kern, int W, float *out, long long *ticks) {
  // workgroups of 4 waves (one per SIMD), exactly W of them fit a CU's 160 KB of LDS
  const int nblk = 256 * W, nthr = 256;
  const int lds = W == 1 ? 100 * 1024 : W == 2 ? 70 * 1024 : W == 4 ? 36 * 1024 : W == 6 ? 24 * 1024 : 19 * 1024;
  CK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  hipLaunchKernelGGL(kern, dim3(nblk), dim3(nthr), lds, 0, out, ticks, 1.0f);   // warm-up
  CK(hipDeviceSynchronize());
  CK(hipEventRecord(e0));
  hipLaunchKernelGGL(kern, dim3(nblk), dim3(nthr), lds, 0, out, ticks, 1.0f);
  CK(hipEventRecord(e1));
  CK(hipDeviceSynchronize());
  float ms = 0;
  CK(hipEventElapsedTime(&ms, e0, e1));
  std::vector<long long> h((size_t)nblk * nthr / 64);
  CK(hipMemcpy(h.data(), ticks, h.size() * 8, hipMemcpyDeviceToHost));
  double sum = 0; long long mx = 0;
  for (long long v : h) { sum += (double)v; if (v > mx) mx = v; }
  const double n = (double)ITER * UNR;
  printf("%-16s W=%d  ticks/wave avg %.0f max %lld  -> ticks per instruction per SIMD %.3f   kernel %.3f ms -> ns per instruction per SIMD %.3f\n",
         name, W, sum / h.size(), mx, sum / h.size() / (n * W), ms, ms * 1e6 / (n * W));
}

int main() {
  float *out; long long *ticks;
  CK(hipMalloc(&out, 256 * 8 * 256 * 4)); CK(hipMalloc(&ticks, 256 * 8 * 4 * 8));
  int clk = 0;
  CK(hipDeviceGetAttribute(&clk, hipDeviceAttributeClockRate, 0));
  printf("clock rate attribute %d kHz; readcyclecounter = s_memtime\n", clk);
  for (int W : {1, 2, 4, 6, 8}) {
    run("v_fma_f32", k<0>, W, out, ticks);
    run("v_add_f32", k<1>, W, out, ticks);
    run("v_add_f32_dpp", k<2>, W, out, ticks);
    run("v_lshl_add_u32", k<3>, W, out, ticks);
    run("v_and_b32", k<4>, W, out, ticks);
    run("v_bfe_u32", k<5>, W, out, ticks);
    run("v_pk_add_f32", kpk<0>, W, out, ticks);
    run("lshlrev_sdwa_b0", k<6>, W, out, ticks);
    run("lshlrev_sdwa_b1", k<7>, W, out, ticks);
    run("lshlrev_sdwa_b2", k<8>, W, out, ticks);
    run("lshlrev_sdwa_b3", k<9>, W, out, ticks);
    run("v_or_b32", k<10>, W, out, ticks);
    run("v_add_u32", k<11>, W, out, ticks);
    run("v_lshrrev_b32", k<12>, W, out, ticks);
    run("v_and_or_b32", k<13>, W, out, ticks);
    run("v_bfi_b32", k<14>, W, out, ticks);
    run("v_perm_b32", k<15>, W, out, ticks);
    run("v_mad_u32_u24", k<16>, W, out, ticks);
    run("v_lshl_or_b32", k<17>, W, out, ticks);
    run("and_or_sgpr", k<18>, W, out, ticks);
    run("mul_u24_sdwa_b1", k<19>, W, out, ticks);
    run("cvt_f32_ubyte0", k<20>, W, out, ticks);
    run("cvt_f32_ubyte1", k<21>, W, out, ticks);
    run("cvt_f32_ubyte3", k<22>, W, out, ticks);
    run("fma_f32_denorm", k<23>, W, out, ticks);
    run("fmamk_f32_denorm", k<26>, W, out, ticks);
    run("v_lshlrev_b32", k<24>, W, out, ticks);
    run("and_b32_sgpr", k<25>, W, out, ticks);
    run("dot4_ssel_b0", k<30>, W, out, ticks);
    run("dot4_ssel_b1", k<31>, W, out, ticks);
    run("dot4_ssel_b2", k<32>, W, out, ticks);
    run("dot4_ssel_b3", k<33>, W, out, ticks);
    run("dot4_vsel_b0", k<34>, W, out, ticks);
    run("dot4_vsel_b1", k<35>, W, out, ticks);
    run("dot4_vsel_b2", k<36>, W, out, ticks);
    run("dot4_vsel_b3", k<37>, W, out, ticks);
    run("dot4_ssel_add0", k<38>, W, out, ticks);
    run("dot4_ssel_acc", k<39>, W, out, ticks);
    run("dot4+fma_denorm", k<40>, W, out, ticks);
    run("dot4+and_b32", k<41>, W, out, ticks);
    run("dot4+lshrrev", k<43>, W, out, ticks);
    run("dot4+lshl_add", k<45>, W, out, ticks);
    run("and+fma_denorm", k<42>, W, out, ticks);
    run("lshr+fma_denorm", k<44>, W, out, ticks);
  }
  return 0;
}
