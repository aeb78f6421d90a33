// v_mfma_f32_4x4x1_16b_f32 with the A-broadcast modifier (cbsz:2 abid:LP) as a builder of the 16-lane tick's Gram columns
// (paddlerobotics_amd/csrc/gram16.h).  Three questions, one mode each (no argument: all three):
//   semantics  one wave, distinct values per lane: is reg e of lane l  a[16 (l / 16) + 4 abid + e] * b[l] ?
//   price      cycles a lone wave per SIMD pays (1024 single-wave workgroups, clock64 around 1024 repetitions) for
//              24 MFMAs as four interleaved chains, the same with one / two independent v_fma_f32 between consecutive MFMAs,
//              and for the 96 v_fmac_f32_dpp row_newbcast they replace
//   bits       4 waves = 16 robots: the MFMA columns of (Z,Z), (Z,Z2), (Z2,Z2), (Z2,Z) -- from the builtin one by one and from
//              the tick's scheduled block (gram16_block) -- against the row_newbcast FMA sequence
//              on the device and against an fmaf chain on the host, as int32 bit patterns, over normals, rows of +0 / -0,
//              mixed-sign zeros, denormal-range products and large magnitudes.  Exit status 1 on any mismatch.
//   hipcc --offload-arch=gfx950 -O3 -fno-signed-zeros -ffinite-math-only -o tools/ubench/mfma4x4_bcast tools/ubench/mfma4x4_bcast.hip
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../paddlerobotics_amd/csrc/gram16.h"

using etg::gram4_t;

#define CHECK(x)                                                                       \
  do {                                                                                 \
    hipError_t e_ = (x);                                                               \
    if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 2; } \
  } while (0)

template <int CTRL> __device__ __forceinline__ float dpp_(float x) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, true));
}

// ------------------------------------------------------------------ (a) semantics
__global__ void k_semantics(const float* a, const float* b, float* out) {   // out[abid][lane][e]
  const int l = threadIdx.x;
  const float av = a[l], bv = b[l];
  const gram4_t z = {0.0f, 0.0f, 0.0f, 0.0f};
  const gram4_t r0 = etg::gram4_bcast<0>(z, av, bv), r1 = etg::gram4_bcast<1>(z, av, bv), r2 = etg::gram4_bcast<2>(z, av, bv),
                r3 = etg::gram4_bcast<3>(z, av, bv);
  for (int e = 0; e < 4; e++) {
    out[(0 * 64 + l) * 4 + e] = r0[e]; out[(1 * 64 + l) * 4 + e] = r1[e];
    out[(2 * 64 + l) * 4 + e] = r2[e]; out[(3 * 64 + l) * 4 + e] = r3[e];
  }
}
static int semantics() {
  float ha[64], hb[64], ho[4 * 64 * 4];
  for (int l = 0; l < 64; l++) { ha[l] = (float)(l + 1); hb[l] = (float)(1000 + 7 * l); }   // products are exact integers
  float *da, *db, *dout;
  CHECK(hipMalloc(&da, sizeof(ha))); CHECK(hipMalloc(&db, sizeof(hb))); CHECK(hipMalloc(&dout, sizeof(ho)));
  CHECK(hipMemcpy(da, ha, sizeof(ha), hipMemcpyHostToDevice)); CHECK(hipMemcpy(db, hb, sizeof(hb), hipMemcpyHostToDevice));
  CHECK(hipMemset(dout, 0, sizeof(ho)));
  hipLaunchKernelGGL(k_semantics, dim3(1), dim3(64), 0, 0, da, db, dout);
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(ho, dout, sizeof(ho), hipMemcpyDeviceToHost));
  int bad = 0;
  for (int abid = 0; abid < 4; abid++)
    for (int l = 0; l < 64; l++)
      for (int e = 0; e < 4; e++) {
        const float want = ha[16 * (l / 16) + 4 * abid + e] * hb[l], got = ho[(abid * 64 + l) * 4 + e];
        if (want != got) {
          if (bad < 8) printf("  abid %d lane %2d reg %d: got %.0f (= a[%g] * b[l]?), want %.0f\n", abid, l, e, got, got / hb[l] - 1, want);
          bad++;
        }
      }
  for (int l : {0, 5, 17, 38, 63}) {
    printf("  lane %2d abid 2: a-lanes", l);
    for (int e = 0; e < 4; e++) printf(" %g", ho[(2 * 64 + l) * 4 + e] / hb[l] - 1);
    printf("   (expected %d..%d)\n", 16 * (l / 16) + 8, 16 * (l / 16) + 11);
  }
  printf("semantics: reg e of lane l = a[16 (l / 16) + 4 abid + e] * b[l]: %s (%d of 1024 differ)\n", bad ? "NO" : "yes", bad);
  hipFree(da); hipFree(db); hipFree(dout);
  return bad ? 1 : 0;
}

// ------------------------------------------------------------------ (b) price
#define REP 1024
#define MF(ACC, K, LP) "v_mfma_f32_4x4x1_16b_f32 %[" ACC "], %[z" #K "], %[z" #K "], %[" ACC "] cbsz:2 abid:" #LP "\n"
#define FM(X) "v_fma_f32 %[" X "], %[" X "], %[fa], %[fb]\n"
#define ROW0(K) MF("c0", K, 0) MF("c1", K, 1) MF("c2", K, 2) MF("c3", K, 3)
#define ROW1(K, A, B, C, D) MF("c0", K, 0) FM(A) MF("c1", K, 1) FM(B) MF("c2", K, 2) FM(C) MF("c3", K, 3) FM(D)
#define ROW2(K) MF("c0", K, 0) FM("x0") FM("x1") MF("c1", K, 1) FM("x2") FM("x3") MF("c2", K, 2) FM("x4") FM("x5") MF("c3", K, 3) FM("x6") FM("x7")
#define FM8 FM("x0") FM("x1") FM("x2") FM("x3") FM("x4") FM("x5") FM("x6") FM("x7")
// FMAS: v_fma_f32 between consecutive MFMAs (0, 1, 2); FMAS = -1: the 24 (-2: the 48) v_fma_f32 alone
template <int FMAS> __global__ void k_price_mfma(float* sink, long long* cyc, float fa, float fb) {
  const int l = threadIdx.x;
  float z[6], x[8];
  for (int k = 0; k < 6; k++) z[k] = 0.001f * (float)(l + 1) + 0.01f * (float)k;
  for (int i = 0; i < 8; i++) x[i] = (float)(l + i);
  gram4_t c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0;
#define OPS [c0] "+v"(c0), [c1] "+v"(c1), [c2] "+v"(c2), [c3] "+v"(c3), [x0] "+v"(x[0]), [x1] "+v"(x[1]), [x2] "+v"(x[2]), [x3] "+v"(x[3]), \
            [x4] "+v"(x[4]), [x5] "+v"(x[5]), [x6] "+v"(x[6]), [x7] "+v"(x[7])                                                                 \
            : [z0] "v"(z[0]), [z1] "v"(z[1]), [z2] "v"(z[2]), [z3] "v"(z[3]), [z4] "v"(z[4]), [z5] "v"(z[5]), [fa] "v"(fa), [fb] "v"(fb)
  asm volatile("s_nop 7" : OPS);     // (the operands are in their registers before the first stamp)
  const long long t0 = clock64();
  for (int i = 0; i < REP; i++) {
    if (FMAS == 0) asm volatile(ROW0(0) ROW0(1) ROW0(2) ROW0(3) ROW0(4) ROW0(5) : OPS);
    if (FMAS == 1)
      asm volatile(ROW1(0, "x0", "x1", "x2", "x3") ROW1(1, "x4", "x5", "x6", "x7") ROW1(2, "x0", "x1", "x2", "x3") ROW1(3, "x4", "x5", "x6", "x7")
                   ROW1(4, "x0", "x1", "x2", "x3") ROW1(5, "x4", "x5", "x6", "x7") : OPS);
    if (FMAS == 2) asm volatile(ROW2(0) ROW2(1) ROW2(2) ROW2(3) ROW2(4) ROW2(5) : OPS);
    if (FMAS == -1) asm volatile(FM8 FM8 FM8 : OPS);
    if (FMAS == -2) asm volatile(FM8 FM8 FM8 FM8 FM8 FM8 : OPS);
  }
  asm volatile("s_nop 7\ns_nop 7\ns_nop 3" : OPS);   // the matrix pipe has written the accumulators back before a VALU reads them
#undef OPS
  const long long t1 = clock64();
  float s = 0.0f;
  for (int i = 0; i < 8; i++) s += x[i];
  for (int e = 0; e < 4; e++) s += c0[e] + c1[e] + c2[e] + c3[e];
  sink[blockIdx.x * 64 + l] = s;
  if (l == 0) cyc[blockIdx.x] = t1 - t0;
}
#define FD(R, K) "v_fmac_f32_dpp %" #R ", %[z" #K "], %[z" #K "] row_newbcast:" #R " row_mask:0xf bank_mask:0xf bound_ctrl:1\n"
#define DROW(K) FD(0, K) FD(1, K) FD(2, K) FD(3, K) FD(4, K) FD(5, K) FD(6, K) FD(7, K) FD(8, K) FD(9, K) FD(10, K) FD(11, K) FD(12, K) FD(13, K) FD(14, K) FD(15, K)
__global__ void k_price_dpp(float* sink, long long* cyc, float, float) {
  const int l = threadIdx.x;
  float z[6], a[16];
  for (int k = 0; k < 6; k++) z[k] = 0.001f * (float)(l + 1) + 0.01f * (float)k;
  for (int i = 0; i < 16; i++) a[i] = 0.0f;
#define OPS "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]), "+v"(a[8]), "+v"(a[9]), "+v"(a[10]), \
            "+v"(a[11]), "+v"(a[12]), "+v"(a[13]), "+v"(a[14]), "+v"(a[15])                                                                        \
            : [z0] "v"(z[0]), [z1] "v"(z[1]), [z2] "v"(z[2]), [z3] "v"(z[3]), [z4] "v"(z[4]), [z5] "v"(z[5])
  asm volatile("s_nop 7" : OPS);
  const long long t0 = clock64();
  for (int i = 0; i < REP; i++) asm volatile(DROW(0) DROW(1) DROW(2) DROW(3) DROW(4) DROW(5) : OPS);
  asm volatile("s_nop 1" : OPS);
#undef OPS
  const long long t1 = clock64();
  float s = 0.0f;
  for (int i = 0; i < 16; i++) s += a[i];
  sink[blockIdx.x * 64 + l] = s;
  if (l == 0) cyc[blockIdx.x] = t1 - t0;
}
static int price() {
  const int NB = 1024;
  float* sink; long long* cyc;
  CHECK(hipMalloc(&sink, NB * 64 * sizeof(float))); CHECK(hipMalloc(&cyc, NB * sizeof(long long)));
  typedef void (*KF)(float*, long long*, float, float);
  struct { const char* name; KF f; int mfma, fma, dpp; } ks[] = {
      {"24 MFMA, four interleaved chains (k-major)", k_price_mfma<0>, 24, 0, 0},
      {"24 MFMA + 1 v_fma_f32 after each", k_price_mfma<1>, 24, 24, 0},
      {"24 MFMA + 2 v_fma_f32 after each", k_price_mfma<2>, 24, 48, 0},
      {"24 v_fma_f32 alone", k_price_mfma<-1>, 0, 24, 0},
      {"48 v_fma_f32 alone", k_price_mfma<-2>, 0, 48, 0},
      {"96 v_fmac_f32_dpp row_newbcast (16 columns)", k_price_dpp, 0, 0, 96}};
  std::vector<long long> h(NB);
  printf("price: cycles per repetition of one wave per SIMD (%d single-wave workgroups, %d repetitions): min / median / max\n", NB, REP);
  for (int pass = 0; pass < 2; pass++)   // the first pass warms the clocks up
    for (auto& k : ks) {
      CHECK(hipMemset(cyc, 0, NB * sizeof(long long)));
      hipLaunchKernelGGL(k.f, dim3(NB), dim3(64), 0, 0, sink, cyc, 0.5f, 1.0f);
      CHECK(hipDeviceSynchronize());
      CHECK(hipMemcpy(h.data(), cyc, NB * sizeof(long long), hipMemcpyDeviceToHost));
      std::sort(h.begin(), h.end());
      if (pass) {
        const double lo = (double)h[0] / REP, med = (double)h[NB / 2] / REP, hi = (double)h[NB - 1] / REP;
        printf("  %-46s %8.1f %8.1f %8.1f   per instruction (median) %.2f\n", k.name, lo, med, hi, med / (k.mfma + k.fma + k.dpp));
      }
    }
  hipFree(sink); hipFree(cyc);
  return 0;
}

// ------------------------------------------------------------------ (c) bits
constexpr int NL = 256;     // 4 waves = 16 robots
constexpr int NCASE = 8;
// the four column sets: (a, b) = (Z, Z) A / Ak, (Z, Z2) BA, (Z2, Z2) BB, (Z2, Z) AT; 16 columns each: out[(set * 16 + 4 lp + e) * NL + lane]
// BLOCK: the tick's form, gram16_block (24 instructions and their wait states in one asm block); otherwise the builtin, one by one
template <bool BLOCK> __device__ __forceinline__ void set_mfma(const float* a, const float* b, unsigned* out, int lane) {
  const gram4_t seed = etg::gram4_seed();
  gram4_t acc[4];
  if (BLOCK) {
    etg::gram16_block(acc, seed, a, b);
  } else {
#pragma unroll
    for (int k = 0; k < 6; k++)
#pragma unroll
      for (int lp = 0; lp < 4; lp++) acc[lp] = etg::gram4_bcast(k == 0 ? seed : acc[lp], a[k], b[k], lp);
  }
#pragma unroll
  for (int lp = 0; lp < 4; lp++)
#pragma unroll
    for (int e = 0; e < 4; e++) out[(4 * lp + e) * NL + lane] = __float_as_uint(acc[lp][e]);
}
template <bool BLOCK> __global__ void __launch_bounds__(64) k_bits_mfma(const float* in, unsigned* out) {   // in[case][2][6][NL], out[case][64][NL]
  const int lane = blockIdx.x * 64 + threadIdx.x;
  for (int cs = 0; cs < NCASE; cs++) {
    float Z[6], Z2[6];
    for (int k = 0; k < 6; k++) { Z[k] = in[((cs * 2 + 0) * 6 + k) * NL + lane]; Z2[k] = in[((cs * 2 + 1) * 6 + k) * NL + lane]; }
    unsigned* o = out + (size_t)cs * 64 * NL;
    set_mfma<BLOCK>(Z, Z, o, lane); set_mfma<BLOCK>(Z, Z2, o + 16 * NL, lane); set_mfma<BLOCK>(Z2, Z2, o + 32 * NL, lane);
    set_mfma<BLOCK>(Z2, Z, o + 48 * NL, lane);
  }
}
// the tick's own instructions: a plain product of the row_newbcast value, then five v_fmac_f32_dpp row_newbcast
#define FMAC_DPP(ACC, X, Y, R) asm("v_fmac_f32_dpp %0, %1, %2 row_newbcast:" #R " row_mask:0xf bank_mask:0xf bound_ctrl:1" : "+v"(ACC) : "v"(X), "v"(Y))
#define COLUMN(R)                                                                                   \
  {                                                                                                 \
    float acc = dpp_<0x150 + R>(a[0]) * b[0];                                                       \
    FMAC_DPP(acc, a[1], b[1], R); FMAC_DPP(acc, a[2], b[2], R); FMAC_DPP(acc, a[3], b[3], R);       \
    FMAC_DPP(acc, a[4], b[4], R); FMAC_DPP(acc, a[5], b[5], R);                                     \
    out[R * NL + lane] = __float_as_uint(acc);                                                      \
  }
__device__ __forceinline__ void set_dpp(const float* a, const float* b, unsigned* out, int lane) {
  COLUMN(0) COLUMN(1) COLUMN(2) COLUMN(3) COLUMN(4) COLUMN(5) COLUMN(6) COLUMN(7)
  COLUMN(8) COLUMN(9) COLUMN(10) COLUMN(11) COLUMN(12) COLUMN(13) COLUMN(14) COLUMN(15)
}
__global__ void __launch_bounds__(64) k_bits_dpp(const float* in, unsigned* out) {
  const int lane = blockIdx.x * 64 + threadIdx.x;
  for (int cs = 0; cs < NCASE; cs++) {
    float Z[6], Z2[6];
    for (int k = 0; k < 6; k++) { Z[k] = in[((cs * 2 + 0) * 6 + k) * NL + lane]; Z2[k] = in[((cs * 2 + 1) * 6 + k) * NL + lane]; }
    // (the 2 wait states between a VALU write and a DPP read of the broadcast sources)
    asm volatile("s_nop 1" : "+v"(Z[0]), "+v"(Z[1]), "+v"(Z[2]), "+v"(Z[3]), "+v"(Z[4]), "+v"(Z[5]), "+v"(Z2[0]), "+v"(Z2[1]), "+v"(Z2[2]),
                 "+v"(Z2[3]), "+v"(Z2[4]), "+v"(Z2[5]));
    unsigned* o = out + (size_t)cs * 64 * NL;
    set_dpp(Z, Z, o, lane); set_dpp(Z, Z2, o + 16 * NL, lane); set_dpp(Z2, Z2, o + 32 * NL, lane); set_dpp(Z2, Z, o + 48 * NL, lane);
  }
}
static uint32_t rng_state = 12345u;
static double urand() { rng_state = rng_state * 1664525u + 1013904223u; return ((rng_state >> 8) + 0.5) / 16777216.0; }
static float nrand() { return (float)(std::sqrt(-2.0 * std::log(urand())) * std::cos(6.283185307179586 * urand())); }
static float zero_of(int sign) { const uint32_t u = sign ? 0x80000000u : 0u; float f; memcpy(&f, &u, 4); return f; }   // (bit patterns: no fast-math flag folds the sign)
static const char* case_name[NCASE] = {"random normals", "Z rows all +0", "Z rows all -0", "Z2 rows all -0, Z +0 in odd robots",
                                       "inactive lanes: mixed-sign zeros inside a row", "denormal-range products (entries ~1e-20)",
                                       "mixed 1e-20 / 1 magnitudes with zeros", "large magnitudes (entries ~1e17)"};
static int bits() {
  std::vector<float> in((size_t)NCASE * 2 * 6 * NL);
  auto at = [&](int cs, int w, int k, int l) -> float& { return in[((size_t)(cs * 2 + w) * 6 + k) * NL + l]; };
  for (int cs = 0; cs < NCASE; cs++)
    for (int l = 0; l < NL; l++) {
      const bool dead = urand() < 0.4, dead2 = urand() < 0.4;   // a lane whose contact row is inactive: all six entries are zeros
      for (int k = 0; k < 6; k++) {
        float z = nrand(), z2 = nrand();
        switch (cs) {
          case 1: z = zero_of(0); break;
          case 2: z = zero_of(1); break;
          case 3: z2 = zero_of(1); if ((l / 16) & 1) z = zero_of(0); break;
          case 4: if (dead) z = zero_of(urand() < 0.5); if (dead2) z2 = zero_of(urand() < 0.5); break;
          case 5: z *= 1e-20f; z2 *= 1e-20f; break;
          case 6: if (urand() < 0.5) z *= 1e-20f; if (urand() < 0.5) z2 *= 1e-20f; if (urand() < 0.2) z = zero_of(urand() < 0.5); if (urand() < 0.2) z2 = zero_of(urand() < 0.5); break;
          case 7: z *= 1e17f; z2 *= 1e17f; break;
          default: break;
        }
        at(cs, 0, k, l) = z; at(cs, 1, k, l) = z2;
      }
    }
  const size_t nout = (size_t)NCASE * 64 * NL;
  float* din; unsigned *dm, *dk, *dd;
  CHECK(hipMalloc(&din, in.size() * sizeof(float))); CHECK(hipMalloc(&dm, nout * 4)); CHECK(hipMalloc(&dk, nout * 4)); CHECK(hipMalloc(&dd, nout * 4));
  CHECK(hipMemcpy(din, in.data(), in.size() * sizeof(float), hipMemcpyHostToDevice));
  CHECK(hipMemset(dm, 0xFF, nout * 4)); CHECK(hipMemset(dk, 0xDD, nout * 4)); CHECK(hipMemset(dd, 0xEE, nout * 4));
  hipLaunchKernelGGL(k_bits_mfma<false>, dim3(NL / 64), dim3(64), 0, 0, din, dm);
  hipLaunchKernelGGL(k_bits_mfma<true>, dim3(NL / 64), dim3(64), 0, 0, din, dk);
  hipLaunchKernelGGL(k_bits_dpp, dim3(NL / 64), dim3(64), 0, 0, din, dd);
  CHECK(hipDeviceSynchronize());
  std::vector<unsigned> hm(nout), hk(nout), hd(nout);
  CHECK(hipMemcpy(hm.data(), dm, nout * 4, hipMemcpyDeviceToHost)); CHECK(hipMemcpy(hk.data(), dk, nout * 4, hipMemcpyDeviceToHost));
  CHECK(hipMemcpy(hd.data(), dd, nout * 4, hipMemcpyDeviceToHost));
  int total = 0;
  for (int cs = 0; cs < NCASE; cs++) {
    int bad_dpp = 0, bad_host = 0, bad_block = 0, dpp_host = 0, negz = 0, den = 0;
    for (int set = 0; set < 4; set++)
      for (int col = 0; col < 16; col++)
        for (int l = 0; l < NL; l++) {
          const int wa = set >= 2, wb = (set == 1 || set == 2), src = 16 * (l / 16) + col;
          volatile float acc = fmaf(at(cs, wa, 0, src), at(cs, wb, 0, l), -0.0f);
          for (int k = 1; k < 6; k++) acc = fmaf(at(cs, wa, k, src), at(cs, wb, k, l), acc);
          float accf = acc;
          unsigned want; memcpy(&want, &accf, 4);
          const size_t i = ((size_t)cs * 64 + set * 16 + col) * NL + l;
          if (hm[i] != hd[i]) { if (bad_dpp + bad_host < 4) printf("    case %d set %d col %2d lane %3d: mfma %08x dpp %08x host %08x\n", cs, set, col, l, hm[i], hd[i], want); bad_dpp++; }
          if (hm[i] != want) { if (bad_dpp + bad_host < 4) printf("    case %d set %d col %2d lane %3d: mfma %08x dpp %08x host %08x\n", cs, set, col, l, hm[i], hd[i], want); bad_host++; }
          if (hk[i] != want) { if (bad_block < 4) printf("    case %d set %d col %2d lane %3d: block %08x host %08x\n", cs, set, col, l, hk[i], want); bad_block++; }
          if (hd[i] != want) dpp_host++;
          if (want == 0x80000000u) negz++;
          if ((want & 0x7F800000u) == 0 && (want & 0x007FFFFFu)) den++;
        }
    printf("  %-48s mfma != dpp: %d, mfma != host fmaf: %d, block != host: %d (dpp != host: %d; of %d values %d are -0, %d denormal)\n", case_name[cs],
           bad_dpp, bad_host, bad_block, dpp_host, 64 * NL, negz, den);
    total += bad_dpp + bad_host + bad_block + dpp_host;
  }
  printf("bits: mismatches %d\n", total);
  hipFree(din); hipFree(dm); hipFree(dk); hipFree(dd);
  return total ? 1 : 0;
}

int main(int argc, char** argv) {
  setvbuf(stdout, nullptr, _IONBF, 0);
  const char* mode = argc > 1 ? argv[1] : "all";
  const bool all = !strcmp(mode, "all");
  int rc = 0;
  if (all || !strcmp(mode, "semantics")) rc |= semantics();
  if (rc == 1 && all) { printf("the hardware does something else: nothing below is meaningful\n"); return rc; }
  if (all || !strcmp(mode, "bits")) rc |= bits();
  if (all || !strcmp(mode, "price")) rc |= price();
  return rc;
}
