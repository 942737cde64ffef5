// Does v_mfma_f32_32x32x16_f16 read SUBNORMAL fp16 operands as they are, or as zero?  And do the conversions precision "fp16_act" uses
// (a plain _Float16 cast: v_cvt_pk_f16_f32 / v_cvt_f32_f16) keep subnormal results, round to nearest-even and overflow to infinity?
// One wavefront, one MFMA per question:
//   (a) A[i][0] = 2^-20 (fp16 subnormal, bits 0x0010), B[0][j] = 2^10, all else 0: D = 2^-10 if the operand is read as it is, 0 if flushed;
//   (b) the same with the subnormal in B and the normal value in A;
//   (c) A[i][0] = 2^-14 (smallest normal), B[0][j] = 2^10: D = 2^-4 either way (the control);
//   (d) A[i][k] = 2^-24 (smallest subnormal) for all 16 k, B = 2^12: D = 16 * 2^-12 = 2^-8 if read as they are.
// Conversions: fp32 -> fp16 -> fp32 of 2^-20 (subnormal: kept?), 2^-25 (tie between 0 and 2^-24: to even = 0), 3 * 2^-25 (tie: to even =
// 2^-23), 65519.9 (below the overflow tie: 65504), 65520 (the tie: to infinity), 1 + 2^-11 (tie: to even = 1), 1 + 3 * 2^-11 (tie: 1 + 2^-9).
//   hipcc --offload-arch=gfx950 -O3 tools/mfma_f16_subnormal.hip -o tools/bin/mfma_f16_subnormal && tools/bin/mfma_f16_subnormal
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// A [32][16] and B^T [32][16] as fp16 bit patterns; lane (li, lh) holds row / column li, k = 8 lh .. 8 lh + 7
__global__ void mfma_once(const unsigned short* A, const unsigned short* Bt, float* D) {
  const int lane = threadIdx.x, li = lane & 31, lh = lane >> 5;
  f16x8 a, b;
  for (int i = 0; i < 8; ++i) {
    a[i] = __builtin_bit_cast(_Float16, A[li * 16 + lh * 8 + i]);
    b[i] = __builtin_bit_cast(_Float16, Bt[li * 16 + lh * 8 + i]);
  }
  f32x16 acc;
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc, 0, 0, 0);
  for (int r = 0; r < 16; ++r) {
    const int row = (r & 3) + 8 * (r >> 2) + 4 * lh;
    D[row * 32 + li] = acc[r];
  }
}

__global__ void convert(const float* x, float* y, unsigned* bits, int n) {
  const int i = threadIdx.x;
  if (i >= n) return;
  const f16x2 p = {(_Float16)x[i], (_Float16)x[i]};   // the pair cast the kernels use
  bits[i] = __builtin_bit_cast(unsigned, p) & 0xffffu;
  y[i] = (float)p[1];
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

static int run(const char* name, unsigned short a_bits, bool all_k, unsigned short b_bits, bool swap, float expect_kept, unsigned short* dA,
               unsigned short* dB, float* dD) {
  unsigned short A[32 * 16] = {0}, B[32 * 16] = {0};
  for (int i = 0; i < 32; ++i)
    for (int k = 0; k < (all_k ? 16 : 1); ++k) {
      A[i * 16 + k] = swap ? b_bits : a_bits;
      B[i * 16 + k] = swap ? a_bits : b_bits;
    }
  CK(hipMemcpy(dA, A, sizeof A, hipMemcpyHostToDevice));
  CK(hipMemcpy(dB, B, sizeof B, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(mfma_once, dim3(1), dim3(64), 0, 0, dA, dB, dD);
  float D[1024];
  CK(hipMemcpy(D, dD, sizeof D, hipMemcpyDeviceToHost));
  int kept = 0, zero = 0;
  for (float v : D) { kept += v == expect_kept; zero += v == 0.f; }
  printf("%s: %d / 1024 outputs = %.9g (operand read as it is), %d = 0 (flushed), sample %.9g\n", name, kept, expect_kept, zero, D[37]);
  return 0;
}

int main() {
  unsigned short *dA, *dB;
  float* dD;
  CK(hipMalloc(&dA, 32 * 16 * 2)); CK(hipMalloc(&dB, 32 * 16 * 2)); CK(hipMalloc(&dD, 1024 * 4));
  if (run("(a) subnormal A operand 2^-20 x 2^10", 0x0010, false, 0x6400, false, ldexpf(1.f, -10), dA, dB, dD)) return 1;
  if (run("(b) subnormal B operand 2^-20 x 2^10", 0x0010, false, 0x6400, true, ldexpf(1.f, -10), dA, dB, dD)) return 1;
  if (run("(c) smallest normal 2^-14 x 2^10 (control)", 0x0400, false, 0x6400, false, ldexpf(1.f, -4), dA, dB, dD)) return 1;
  if (run("(d) sixteen smallest subnormals 2^-24 x 2^12", 0x0001, true, 0x6c00, false, ldexpf(1.f, -8), dA, dB, dD)) return 1;
  const float x[7] = {ldexpf(1.f, -20), ldexpf(1.f, -25), ldexpf(3.f, -25), 65519.9f, 65520.f, 1.f + ldexpf(1.f, -11), 1.f + ldexpf(3.f, -11)};
  const float want[7] = {ldexpf(1.f, -20), 0.f, ldexpf(1.f, -23), 65504.f, INFINITY, 1.f, 1.f + ldexpf(1.f, -9)};
  float *dx, *dy, y[7];
  unsigned *db, bits[7];
  CK(hipMalloc(&dx, sizeof x)); CK(hipMalloc(&dy, sizeof x)); CK(hipMalloc(&db, sizeof bits));
  CK(hipMemcpy(dx, x, sizeof x, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(convert, dim3(1), dim3(64), 0, 0, dx, dy, db, 7);
  CK(hipMemcpy(y, dy, sizeof y, hipMemcpyDeviceToHost));
  CK(hipMemcpy(bits, db, sizeof bits, hipMemcpyDeviceToHost));
  int bad = 0;
  for (int i = 0; i < 7; ++i) {
    const bool ok = y[i] == want[i];
    bad += !ok;
    printf("convert %.9g -> fp16 bits 0x%04x -> %.9g (nearest-even, subnormals kept, overflow to infinity: %.9g) %s\n", x[i], bits[i], y[i], want[i],
           ok ? "ok" : "DIFFERS");
  }
  printf("conversions: %d of 7 differ from IEEE round-to-nearest-even\n", bad);
  return 0;
}
