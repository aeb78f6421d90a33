// gram16.h -- four Gram columns of a 16-lane row in one matrix instruction (gfx950).
//
// The 16-lane tick (etg_core16.h) builds its Delassus columns as sums over the six base coordinates of
//     column(lp, e)  +=  a @ (lane 4 lp + e of MY robot's row)  *  b @ (this lane),      lp = 0..3 (leg), e = 0..3 (sub-lane)
// v_mfma_f32_4x4x1_16b_f32 computes 16 independent 4x4 outer products, one per 4-lane block: lane 4 B + j, register i gets
// a @ (lane 4 B + i) * b @ (lane 4 B + j).  A block is a leg (lane = 4 leg + sub).  The A-broadcast modifier `cbsz:2` groups
// the blocks in fours -- a group is 16 lanes, one robot's DPP row -- and `abid:LP` makes block LP of every group the A operand
// of all four blocks of its group:
//     acc[e]  +=  a @ (lane 4 LP + e of my 16-lane row)  *  b @ (this lane),   e = 0..3,   in EVERY lane, in fixed registers
// which is four v_fmac_f32_dpp row_newbcast:(4 LP + e) in one instruction.  fp32 with k = 1 is one fused multiply-add per
// output: the same bits as the broadcast-FMA chain, given the same order of the k terms and the seed below.
// (tools/ubench/mfma4x4_bcast.hip checks the semantics and the bits and measures the price.)
#pragma once

namespace etg {

typedef float gram4_t __attribute__((ext_vector_type(4)));

// The seed of a column chain.  The broadcast-FMA form starts a column with a plain product; the matrix instruction always adds
// its C operand.  fma(a, b, -0) IS a * b for every input (a product of -0 stays -0), fma(a, b, +0) would turn -0 into +0.
// The quad goes through an empty asm so that no fast-math flag folds the sign away; it is the C operand of the first
// instruction of every chain (whose destination is the chain's accumulator: no instruction per column).
__device__ __forceinline__ gram4_t gram4_seed() {
  gram4_t s = {-0.0f, -0.0f, -0.0f, -0.0f};
  asm("" : "+v"(s));
  return s;
}

// acc[e] + a@(lane 4 LP + e of this lane's 16-lane row) * b, e = 0..3.  The builtin, not inline asm: the compiler places the
// matrix pipe's hazard wait states itself.
template <int LP> __device__ __forceinline__ gram4_t gram4_bcast(gram4_t acc, float a, float b) {
  static_assert(LP >= 0 && LP < 4, "a row has four legs");
  return __builtin_amdgcn_mfma_f32_4x4x1f32(a, b, acc, 2, LP, 0);
}
// lp is a constant after unrolling
__device__ __forceinline__ gram4_t gram4_bcast(gram4_t acc, float a, float b, int lp) {
  switch (lp) {
    case 0: return gram4_bcast<0>(acc, a, b);
    case 1: return gram4_bcast<1>(acc, a, b);
    case 2: return gram4_bcast<2>(acc, a, b);
    default: return gram4_bcast<3>(acc, a, b);
  }
}

// The 16 columns of a row set -- c[lp][e] = sum over k = 0..5 of a[k]@(lane 4 lp + e of the row) * b[k], k ascending -- as ONE
// block of 24 instructions, k-major so that the four chains interleave (an instruction's accumulator was written four
// instructions earlier).  This is the form the tick uses, for two reasons that the disassembly of the builtin form showed
// (profiles/r09_ab_experiments.txt section 2):
//   * a kernel that may use more than 256 registers gets the builtin's accumulators in AGPRs: 4 v_accvgpr_write for the seed
//     and 16 v_accvgpr_read for the results per block, each a full issue slot of a lone wave -- here they are VGPRs;
//   * the scheduler spreads the builtins between VALU work, and a lone wave pays ~15 cycles for the instruction between VALU
//     instructions against 8.2 back to back (tools/ubench/mfma4x4_bcast.hip) -- here they stay together.
// The price is that the compiler does not see the matrix instructions, so the block carries its own wait states, sized by
// what the compiler places around the builtin for this two-pass instruction: 4 wait states before a VALU instruction reads
// a result (here s_nop 7 = 8 behind the last instruction), 2 before another matrix instruction reads it as SrcC (here the
// accumulator was written four instructions earlier: 3), and s_nop 1 kept in hand between the VALU writes of a[] / b[] and
// the first matrix read.  tools/ubench/mfma4x4_bcast.hip compares this block's bits with the builtin's and the FMA chain's.
#define ETG_GRAM_MF(C, S, K, LP) "v_mfma_f32_4x4x1_16b_f32 %[" C "], %[a" #K "], %[b" #K "], %[" S "] cbsz:2 abid:" #LP "\n"
#define ETG_GRAM_ROW(K) ETG_GRAM_MF("c0", "c0", K, 0) ETG_GRAM_MF("c1", "c1", K, 1) ETG_GRAM_MF("c2", "c2", K, 2) ETG_GRAM_MF("c3", "c3", K, 3)
__device__ __forceinline__ void gram16_block(gram4_t (&c)[4], gram4_t seed, const float* a, const float* b) {
  asm("s_nop 1\n"
      ETG_GRAM_MF("c0", "seed", 0, 0) ETG_GRAM_MF("c1", "seed", 0, 1) ETG_GRAM_MF("c2", "seed", 0, 2) ETG_GRAM_MF("c3", "seed", 0, 3)
      ETG_GRAM_ROW(1) ETG_GRAM_ROW(2) ETG_GRAM_ROW(3) ETG_GRAM_ROW(4) ETG_GRAM_ROW(5)
      "s_nop 7\n"
      : [c0] "=&v"(c[0]), [c1] "=&v"(c[1]), [c2] "=&v"(c[2]), [c3] "=&v"(c[3])
      : [seed] "v"(seed), [a0] "v"(a[0]), [a1] "v"(a[1]), [a2] "v"(a[2]), [a3] "v"(a[3]), [a4] "v"(a[4]), [a5] "v"(a[5]),
        [b0] "v"(b[0]), [b1] "v"(b[1]), [b2] "v"(b[2]), [b3] "v"(b[3]), [b4] "v"(b[4]), [b5] "v"(b[5]));
}
#undef ETG_GRAM_ROW
#undef ETG_GRAM_MF

}  // namespace etg
