// The constant-time joint tails of Bob's two split chains modulo N^2:
//   the response    mta_out = a_enc^b (1 + beta' N) r^N      (range_proofs.rs:688-704,
//                   kzen-paillier Mul / Add / encrypt_with_chosen_randomness),
//   the commitment  v = a_enc^alpha (1 + gamma N) beta^N     (range_proofs.rs:283-288),
// each ONE chain of bits(N) squarings.  b < 2^256, beta' and r are SECRET, and so are
// alpha < q^3 < 2^768 (in b's place), gamma mod N (in beta's) and beta (in r's); N and
// a_enc are public.  Below, b, beta' and r stand for either chain's three secrets.
//
// The head is modexp_slide_kernel<KD, G, KL, true> (modexp.hip) over r with
// lo_bit = 32 EL: r enters only as the base, so its schedule depends on N alone.  It
// may run at other lanes than the tail: its state and table rows are KD digits in
// order.  The tail (tail_ct, one body for the four kernels) resumes the head's
// accumulator r^(N >> 32 EL) and runs the last 32 EL squarings.  N's low bits ride
// them in the head's sliding windows (wave-uniform, public: scalar state and scalar
// branches); b rides them as 8 EL fixed 4-bit digits over T2[u] = a_enc^u, u < 16:
// every digit is multiplied in, zero digits as T2[0] = 1, and every row is read by
// scanning all 16 rows through a mask (ct_row).  The exit product takes (1 + beta' N)
// as its streamed operand instead of 1, so it both multiplies the binomial factor in
// and leaves Montgomery form.
//
//   kernel                     key class         KD   KL   EL   squarings
//   mta_tail_ct_kernel         N^2 < 2^4096     144  128    8         256
//   bob_v_tail_ct_kernel       N^2 < 2^4096     144  128   24         768
//   mta_tail_ct6144_kernel     N^2 < 2^6144     216  192    8         256
//   bob_v_tail_ct6144_kernel   N^2 < 2^6144     216  192   24         768
// KD: digits per row of consts, table, state and table2 (Mont29<KD, 8>, KD / 8 per
// lane); KL: limbs per row of a_enc, 1 + beta' N and out; EL: limbs of b per row and
// of N in the scalar shift register (24 = kBobVLimbs).
//
// The exit product's bound, for R = 2^(29 KD): acc < 2 (N^2)', (N^2)' < 2^29 N^2,
// 1 + beta' N < N^2 < 2^(32 KL) and m < R give
//   (acc (1 + beta' N) + m N^2) / R < N^2 (2^30 2^(32 KL) / 2^(29 KD) + 1),
//   KD = 144, KL = 128: R = 2^4176,  N^2 (2^30 2^4096 / 2^4176 + 1) = N^2 (2^-50 + 1) < 2 N^2
//   KD = 216, KL = 192: R = 2^6264,  N^2 (2^30 2^6144 / 2^6264 + 1) = N^2 (2^-90 + 1) < 2 N^2
// exact after carry_exact and one sub_if_ge (tail_ct asserts 29 KD - 32 KL > 30).
//
// Regular access: the launch covers whole waves of 8 instances (the host pads
// with copies of a real instance's public inputs and b = 0, beta' = 0), there is
// no bound check, every operand has its launch-uniform width (a_enc KL limbs, b
// EL, 1 + beta' N KL, N's low EL) and is loaded unconditionally from clamped
// addresses, and no address, branch or trip count depends on b, beta' or r.  b's
// limb in use is loaded from a.b[inst * EL + k] once per 8 digits, k the public loop
// counter, so the address depends on the instance and on k only; with B_REGS all EL
// limbs are loaded once, ahead of the chain, into a VGPR shift register.
// binom_ct_kernel makes 1 + beta' N the same way (binom_kernel of vhash.hip skips
// zero limbs of its factor: public factors only).
//
// Registers: at 27 digits per lane the squaring's 64-bit columns, the operand, its
// doubled digits and the modulus are 135 VGPRs, and the 24-limb shift register of N
// brings v's kernels to 44 and 46 SGPRs.  Three measures keep every instantiation free of scratch at
// two waves per SIMD: b's limb is loaded per 8 digits (above) instead of shifting
// through EL VGPRs; the head's accumulator is loaded after the T2 build (held across
// those products it went to scratch); the lane index is taken afresh at the exit, so
// the word indices and shifts of a_enc's limb-to-digit conversion are worked out
// again for 1 + beta' N and not carried along the chain.  B_REGS is set for
// mta_tail_ct_kernel alone, which has the registers to spare (164 VGPRs): with the
// per-limb loads its 4096 chains measured 3.4 % slower than with the shift register
// (4.76 against 4.60 ms on one MI355X; DESIGN.md, profiles/r14/).
#include "mont29.hpp"
#include "kernels.h"
#include "verify.h"

namespace fsdkr {

namespace {

constexpr int G = 8;
constexpr int WAVE_INST = 64 / G;
constexpr int KD4 = 144, KL4 = 128;   // N^2 < 2^4096
constexpr int KD6 = 216, KL6 = 192;   // N^2 < 2^6144

// digit j of a KL-limb integer: both limbs are always loaded, from an address
// clamped into the row, and masked where the digit lies past the top limb
template <int KL>
__device__ __forceinline__ uint32_t digit_full(const uint32_t* __restrict__ x, int j) {
  const int bit = 29 * j;
  const int w = bit >> 5, sh = bit & 31;
  const uint32_t m0 = 0u - (uint32_t)(w < KL), m1 = 0u - (uint32_t)(w + 1 < KL);
  const uint32_t lo = x[min(w, KL - 1)] & m0;
  const uint32_t hi = x[min(w + 1, KL - 1)] & m1;
  return (uint32_t)(mk64(lo, hi) >> sh) & M29;
}
// limb k < KL of an exact-digit integer in LDS, read without a bound test:
// 32 k / 29 + 2 < KD for every k (128 limbs: 142 < 144; 192 limbs: 212 < 216)
template <int KL, int KD>
__device__ __forceinline__ uint32_t limb_full(const uint32_t* d, int k) {
  static_assert((32 * (KL - 1)) / 29 + 2 < KD, "the three digits of every limb lie inside the row");
  const int bit = 32 * k;
  const int j = bit / 29, sh = bit % 29;
  const uint64_t v = (uint64_t)d[j] | ((uint64_t)d[j + 1] << 29) | ((uint64_t)d[j + 2] << 58);
  return (uint32_t)(v >> sh);
}

template <int KD, int KL, int EL, bool B_REGS = false>
__device__ __forceinline__ void tail_ct(const MtaTailArgs& a, uint32_t* lds) {
  static_assert(KD % G == 0 && KL % G == 0, "whole digits and whole output limbs per lane");
  static_assert(29 * KD - 32 * KL > 30, "exit product below 2 N^2: one sub_if_ge is enough");
  using MT = Mont29<KD, G>;
  constexpr int L = KD / G, LO = KL / G;
  constexpr int STRIDE = cons_stride(KD);
  const int g = threadIdx.x % G;
  const int li = threadIdx.x / G;
  const uint32_t inst = blockIdx.x * WAVE_INST + li;   // whole waves: no bound check
  uint32_t* stream = lds + li * KD;
  const uint32_t* C0 = a.consts + (size_t)a.mod_idx[inst] * STRIDE;   // N^2: the exit product
  const uint32_t* C = C0 + cons_scaled(KD);                            // (N^2)': the chain's modulus
  MT M;
  M.init_lane(g);
#pragma unroll
  for (int j = 0; j < L; ++j) M.n[j] = C[g * L + j];
  M.ninv = 1u;
  const uint32_t w = a.window, tw = 1u << (w - 1);
  const uint32_t* T = a.table + (size_t)inst * (tw + 1) * KD;
  // N's bits below 2^(32 EL): the wave's instances share N (the host's layout), so
  // its low limbs are made wave-uniform and the window schedule runs on the scalar
  // unit; the bits leave from the top of an EL-limb shift register
  uint32_t nw[EL];
  {
    const uint32_t* E = reinterpret_cast<const uint32_t*>(a.exp_ptr[inst]);
#pragma unroll
    for (int k = 0; k < EL; ++k) nw[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)E[k]);
  }
  // the streamed operand of the next product: a row in memory, or this lane's digits
  auto put_row = [&](const uint32_t* row) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < L; ++j) stream[g * L + j] = row[g * L + j];
    __builtin_amdgcn_wave_barrier();
  };
  auto put = [&](const uint32_t* d) {
    __builtin_amdgcn_wave_barrier();
    lds_put<KD, G>(stream, d, g);
    __builtin_amdgcn_wave_barrier();
  };
  // T2[u] = a_enc^u (Montgomery form), u < 16
  uint32_t* T2 = a.table2 + (size_t)inst * 16 * KD;
  {
    const uint32_t* A = a.a_enc + (size_t)inst * KL;
    uint32_t y[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
      y[j] = digit_full<KL>(A, g * L + j);
      T2[g * L + j] = C[KD + g * L + j];   // T2[0] = 1 (R mod (N^2)')
    }
    put_row(C + 2 * KD);                   // R^2: y -> y R
    M.mul_s(y, y, stream);
#pragma unroll
    for (int j = 0; j < L; ++j) T2[KD + g * L + j] = y[j];
    put(y);                                // T2[1] streamed for the powers
#pragma unroll 1
    for (int u = 2; u < 16; ++u) {
      M.mul_s(y, y, stream);
#pragma unroll
      for (int j = 0; j < L; ++j) T2[(size_t)u * KD + g * L + j] = y[j];
    }
  }
  // b's digits leave from the top of a shift register: the limb in use, or all EL
  const uint32_t* B = a.b + (size_t)inst * EL;
  constexpr int BW = B_REGS ? EL : 1;
  uint32_t bw[BW];
  if constexpr (B_REGS) {
#pragma unroll
    for (int k = 0; k < EL; ++k) bw[k] = B[k];
  }
  uint32_t acc[L];   // the head's accumulator, taken after the T2 build
#pragma unroll
  for (int j = 0; j < L; ++j) acc[j] = a.state[(size_t)inst * KD + g * L + j];
  // bits 32 EL - 1 .. 0, limb by limb of b: square; a sliding window of N (at most w
  // bits, from a set bit down to its lowest set bit) multiplies T[d >> 1] in after its
  // last squaring; after every 4th squaring b's digit multiplies its T2 row in
  uint32_t pend = 0, pend_d = 0;   // squarings until the open window's product (0: none), its odd digit
#pragma unroll 1
  for (int k = EL - 1; k >= 0; --k) {
    asm volatile("" : "+s"(k));   // the limb counter stays on the scalar unit
    if constexpr (!B_REGS) bw[0] = B[k];
#pragma unroll 1
    for (int wi = 0; wi < 8; ++wi) {
      asm volatile("" : "+s"(wi));
#pragma unroll 1
      for (int s = 0; s < 4; ++s) {
        if (pend == 0 && (nw[EL - 1] >> 31)) {   // a window starts at this bit
          const uint32_t top = nw[EL - 1] >> (32u - w);   // the next w bits (zeros below bit 0)
          const uint32_t tz = (uint32_t)__builtin_ctz(top);
          pend_d = top >> tz;
          pend = w - tz;
        }
#pragma unroll
        for (int q = EL - 1; q > 0; --q) nw[q] = (nw[q] << 1) | (nw[q - 1] >> 31);
        nw[0] <<= 1;
        put(acc);
        M.sqr_s(acc, acc, stream);
        if (pend != 0 && --pend == 0) {
          put_row(T + (size_t)(pend_d >> 1) * KD);
          M.mul_s(acc, acc, stream);
        }
      }
      const uint32_t nib = bw[BW - 1] >> 28;
#pragma unroll
      for (int q = BW - 1; q > 0; --q) bw[q] = (bw[q] << 4) | (bw[q - 1] >> 28);
      bw[0] <<= 4;
      uint32_t row[L];
      ct_row<L>(row, T2, nib, 16, KD, g);
      put(row);
      M.mul_s(acc, acc, stream);
    }
  }
  // exit: acc (1 + beta' N) / R modulo N^2 itself, the lane index taken afresh
  int ge = g;
  asm volatile("" : "+v"(ge));
  {
    const uint32_t* Bn = a.binom + (size_t)inst * KL;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < L; ++j) {
      M.n[j] = C0[ge * L + j];
      stream[ge * L + j] = digit_full<KL>(Bn, ge * L + j);
    }
    M.ninv = C0[3 * KD];
    __builtin_amdgcn_wave_barrier();
  }
  M.mul(acc, acc, stream);
  M.carry_exact(acc);
  M.sub_if_ge(acc);
  put(acc);
  uint32_t* O = a.out + (size_t)a.out_idx[inst] * KL;
#pragma unroll
  for (int q = 0; q < LO; ++q) O[ge * LO + q] = limb_full<KL, KD>(stream, ge * LO + q);
}

}  // namespace

// plain kernels, found by name in the disassembly (tests/test_*_isa.py)
__global__ __launch_bounds__(64, 2) void mta_tail_ct_kernel(const MtaTailArgs a) {
  __shared__ uint32_t lds[WAVE_INST * KD4];
  tail_ct<KD4, KL4, 8, true>(a, lds);
}

__global__ __launch_bounds__(64, 2) void bob_v_tail_ct_kernel(const MtaTailArgs a) {
  __shared__ uint32_t lds[WAVE_INST * KD4];
  tail_ct<KD4, KL4, (int)kBobVLimbs>(a, lds);
}

__global__ __launch_bounds__(64, 2) void mta_tail_ct6144_kernel(const MtaTailArgs a) {
  __shared__ uint32_t lds[WAVE_INST * KD6];
  tail_ct<KD6, KL6, 8>(a, lds);
}

__global__ __launch_bounds__(64, 2) void bob_v_tail_ct6144_kernel(const MtaTailArgs a) {
  __shared__ uint32_t lds[WAVE_INST * KD6];
  tail_ct<KD6, KL6, (int)kBobVLimbs>(a, lds);
}

// out[p] = 1 + s[p] * n[p] for NL-limb factors (2 NL limbs out), one thread per row
// of a launch of whole waves; every limb of s is multiplied in and every carry
// runs to the top limb, so the instruction stream does not depend on s
template <int NL>
__global__ __launch_bounds__(64) void binom_ct_kernel(const BinomCtArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t* s = a.s + (size_t)p * NL;
  const uint32_t* n = reinterpret_cast<const uint32_t*>(a.n_ptr[p]);
  uint32_t* o = a.out + (size_t)p * 2 * NL;
#pragma unroll 1
  for (int k = 0; k < NL; ++k) o[k] = 0;
#pragma unroll 1
  for (int i = 0; i < NL; ++i) {
    const uint32_t si = s[i];
    uint64_t c = 0;
#pragma unroll 1
    for (int j = 0; j < NL; ++j) {
      c += (uint64_t)si * n[j] + o[i + j];
      o[i + j] = (uint32_t)c;
      c >>= 32;
    }
    o[i + NL] = (uint32_t)c;   // first write of this limb
  }
  uint64_t c = 1;
#pragma unroll 1
  for (int k = 0; k < 2 * NL; ++k) {
    c += o[k];
    o[k] = (uint32_t)c;
    c >>= 32;
  }
}

// nl: N's limbs, 64 or 96; el: limbs of secret exponent, 8 or kBobVLimbs
hipError_t launch_mta_tail_ct(uint32_t nl, uint32_t el, const MtaTailArgs& a, hipStream_t st) {
  if (!a.count_pad || a.count_pad % kMtaTailPad || a.window < 1 || a.window > 7) return hipErrorInvalidValue;
  const dim3 grid(a.count_pad / kMtaTailPad), block(64);
  if (nl == 64 && el == 8) hipLaunchKernelGGL(mta_tail_ct_kernel, grid, block, 0, st, a);
  else if (nl == 64 && el == kBobVLimbs) hipLaunchKernelGGL(bob_v_tail_ct_kernel, grid, block, 0, st, a);
  else if (nl == 96 && el == 8) hipLaunchKernelGGL(mta_tail_ct6144_kernel, grid, block, 0, st, a);
  else if (nl == 96 && el == kBobVLimbs) hipLaunchKernelGGL(bob_v_tail_ct6144_kernel, grid, block, 0, st, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_binom_ct(uint32_t nl, const BinomCtArgs& a, hipStream_t st) {
  if (!a.count_pad || a.count_pad % 64) return hipErrorInvalidValue;
  if (nl == 64) hipLaunchKernelGGL(binom_ct_kernel<64>, dim3(a.count_pad / 64), dim3(64), 0, st, a);
  else if (nl == 96) hipLaunchKernelGGL(binom_ct_kernel<96>, dim3(a.count_pad / 64), dim3(64), 0, st, a);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace fsdkr
