// Bob's MtA response (range_proofs.rs:688-704, kzen-paillier Mul / Add /
// encrypt_with_chosen_randomness):
//   mta_out = a_enc^b (1 + beta' N) r^N mod N^2
// for a 2048-bit class key, as the tail of ONE split chain of bits(N) squarings.
// b (< 2^256), beta' and r are SECRET; N and a_enc are public.
//
// The head is modexp_slide_kernel<144, G, 128, true> (modexp.hip) over r with
// lo_bit = 256: r enters only as the base, so its schedule depends on N alone.  It
// may run at other lanes than this tail: its state and table rows are 144 digits
// in order.
// mta_tail_ct_kernel resumes the head's accumulator r^(N >> 256) and runs the
// last 256 squarings.  N's low bits ride them in the head's sliding windows
// (wave-uniform, public: scalar state and scalar branches); b rides them as 64
// fixed 4-bit digits over T2[u] = a_enc^u, u < 16: every digit is multiplied in,
// zero digits as T2[0] = 1, and every row is read by scanning all 16 rows through
// a mask (ct_row).  The exit product takes (1 + beta' N) as its streamed operand
// instead of 1, so it both multiplies the binomial factor in and leaves
// Montgomery form: with acc < 2 (N^2)' and (N^2)' < 2^29 N^2, R = 2^4176,
//   (acc (1 + beta' N) + m N^2) / R < N^2 (2^-50 + 1) < 2 N^2,
// exact after carry_exact and one sub_if_ge.
//
// Regular access: the launch covers whole waves of 8 instances (the host pads
// with copies of a real instance's public inputs and b = 0, beta' = 0), there is
// no bound check, every operand has its launch-uniform width (a_enc 128 limbs, b
// 8, 1 + beta' N 128, N's low 8) and is loaded unconditionally from clamped
// addresses, and no address, branch or trip count depends on b, beta' or r.
// binom_ct_kernel makes 1 + beta' N the same way (binom_kernel of vhash.hip skips
// zero limbs of its factor: public factors only).
// Keys of the 3072-bit class (N^2 < 2^6144) have tails of their own further down:
// mta_tail_ct6144_kernel and bob_v_tail_ct6144_kernel.
#include "mont29.hpp"
#include "kernels.h"
#include "verify.h"

namespace fsdkr {

namespace {

constexpr int KD = 144, G = 8, K32 = 128, L = KD / G;
constexpr int WAVE_INST = 64 / G;

// the 3072-bit class (mta_tail_ct6144_kernel, bob_v_tail_ct6144_kernel): the head's
// Mont29<216, 8> rows, 27 digits per lane
constexpr int KD6 = 216, K32_6 = 192, L6 = KD6 / G;

// digit j of a KL-limb integer: both limbs are always loaded, from an address
// clamped into the row, and masked where the digit lies past the top limb
template <int KL = K32>
__device__ __forceinline__ uint32_t digit_full(const uint32_t* __restrict__ x, int j) {
  const int bit = 29 * j;
  const int w = bit >> 5, sh = bit & 31;
  const uint32_t m0 = 0u - (uint32_t)(w < KL), m1 = 0u - (uint32_t)(w + 1 < KL);
  const uint32_t lo = x[min(w, KL - 1)] & m0;
  const uint32_t hi = x[min(w + 1, KL - 1)] & m1;
  return (uint32_t)(mk64(lo, hi) >> sh) & M29;
}
// limb k < KL of an exact-digit integer in LDS: 32 k / 29 + 2 < DG for every k
// (128 limbs: 142 < 144; 192 limbs: 212 < 216)
template <int KL = K32, int DG = KD>
__device__ __forceinline__ uint32_t limb_full(const uint32_t* d, int k) {
  static_assert((32 * (KL - 1)) / 29 + 2 < DG, "the three digits of every limb lie inside the row");
  const int bit = 32 * k;
  const int j = bit / 29, sh = bit % 29;
  const uint64_t v = (uint64_t)d[j] | ((uint64_t)d[j + 1] << 29) | ((uint64_t)d[j + 2] << 58);
  return (uint32_t)(v >> sh);
}

}  // namespace

__global__ __launch_bounds__(64, 2) void mta_tail_ct_kernel(const MtaTailArgs a) {
  using MT = Mont29<KD, G>;
  constexpr int STRIDE = cons_stride(KD);
  __shared__ uint32_t lds[WAVE_INST * KD];
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
  // N's bits below 2^256: the wave's instances share N (the host's layout), so
  // its low limbs are made wave-uniform and the window schedule runs on the scalar
  // unit; the bits leave from the top of an 8-limb shift register
  uint32_t nw[8];
  {
    const uint32_t* E = reinterpret_cast<const uint32_t*>(a.exp_ptr[inst]);
#pragma unroll
    for (int k = 0; k < 8; ++k) nw[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)E[k]);
  }
  auto put_row = [&](const uint32_t* row) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < L; ++j) stream[g * L + j] = row[g * L + j];
    __builtin_amdgcn_wave_barrier();
  };
  // T2[u] = a_enc^u (Montgomery form), u < 16
  uint32_t* T2 = a.table2 + (size_t)inst * 16 * KD;
  {
    const uint32_t* A = a.a_enc + (size_t)inst * K32;
    uint32_t y[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
      y[j] = digit_full(A, g * L + j);
      T2[g * L + j] = C[KD + g * L + j];   // T2[0] = 1 (R mod (N^2)')
    }
    put_row(C + 2 * KD);                   // R^2: y -> y R
    M.mul_s(y, y, stream);
#pragma unroll
    for (int j = 0; j < L; ++j) T2[KD + g * L + j] = y[j];
    __builtin_amdgcn_wave_barrier();
    lds_put<KD, G>(stream, y, g);          // T2[1] streamed for the powers
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (int u = 2; u < 16; ++u) {
      M.mul_s(y, y, stream);
#pragma unroll
      for (int j = 0; j < L; ++j) T2[(size_t)u * KD + g * L + j] = y[j];
    }
  }
  // b: 8 limbs in registers; the digits leave from the top, the value shifts left
  uint32_t bw[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) bw[k] = a.b[(size_t)inst * 8 + k];
  uint32_t acc[L];
#pragma unroll
  for (int j = 0; j < L; ++j) acc[j] = a.state[(size_t)inst * KD + g * L + j];
  // bits 255 .. 0: square; a sliding window of N (at most w bits, from a set bit
  // down to its lowest set bit) multiplies T[d >> 1] in after its last squaring;
  // after every 4th squaring b's digit multiplies its T2 row in
  uint32_t pend = 0, pend_d = 0;   // squarings until the open window's product (0: none), its odd digit
#pragma unroll 1
  for (int wi = 63; wi >= 0; --wi) {
    asm volatile("" : "+s"(wi));   // the digit counter stays on the scalar unit
#pragma unroll 1
    for (int s = 0; s < 4; ++s) {
      if (pend == 0 && (nw[7] >> 31)) {   // a window starts at this bit
        const uint32_t top = nw[7] >> (32u - w);   // the next w bits (zeros below bit 0)
        const uint32_t tz = (uint32_t)__builtin_ctz(top);
        pend_d = top >> tz;
        pend = w - tz;
      }
#pragma unroll
      for (int k = 7; k > 0; --k) nw[k] = (nw[k] << 1) | (nw[k - 1] >> 31);
      nw[0] <<= 1;
      __builtin_amdgcn_wave_barrier();
      lds_put<KD, G>(stream, acc, g);
      __builtin_amdgcn_wave_barrier();
      M.sqr_s(acc, acc, stream);
      if (pend != 0 && --pend == 0) {
        put_row(T + (size_t)(pend_d >> 1) * KD);
        M.mul_s(acc, acc, stream);
      }
    }
    const uint32_t nib = bw[7] >> 28;
#pragma unroll
    for (int k = 7; k > 0; --k) bw[k] = (bw[k] << 4) | (bw[k - 1] >> 28);
    bw[0] <<= 4;
    uint32_t row[L];
    ct_row<L>(row, T2, nib, 16, KD, g);
    __builtin_amdgcn_wave_barrier();
    lds_put<KD, G>(stream, row, g);
    __builtin_amdgcn_wave_barrier();
    M.mul_s(acc, acc, stream);
  }
  // exit: acc (1 + beta' N) / R modulo N^2 itself
  {
    const uint32_t* Bn = a.binom + (size_t)inst * K32;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < L; ++j) {
      M.n[j] = C0[g * L + j];
      stream[g * L + j] = digit_full(Bn, g * L + j);
    }
    M.ninv = C0[3 * KD];
    __builtin_amdgcn_wave_barrier();
  }
  M.mul(acc, acc, stream);
  M.carry_exact(acc);
  M.sub_if_ge(acc);
  __builtin_amdgcn_wave_barrier();
  lds_put<KD, G>(stream, acc, g);
  __builtin_amdgcn_wave_barrier();
  uint32_t* O = a.out + (size_t)a.out_idx[inst] * K32;
  constexpr int LO = K32 / G;
#pragma unroll
  for (int k = 0; k < LO; ++k) O[g * LO + k] = limb_full(stream, g * LO + k);
}

// The commitment v of Bob's range proof (range_proofs.rs:283-288),
//   v = a_enc^alpha (1 + gamma N) beta^N mod N^2,
// has the response's shape with alpha < q^3 < 2^768 in b's place, gamma mod N in
// beta's and beta in r's: all three SECRET.  The head ran with lo_bit = 768, so this
// tail runs 768 squarings: N's low 24 limbs in the scalar shift register, alpha as
// 192 digits over T2.  alpha is not held in registers (24 VGPRs on top of the chain's
// would spill): the limb in use is loaded from a.b[inst * 24 + k] once per 8 digits, k
// the public loop counter, so the address depends on the instance and on k only.
// Argument block, launch shape, regular access and the exit product's bound are
// mta_tail_ct_kernel's (above); a.b has 24 limbs per row.
// A kernel of its own: one body for both widths cost mta_tail_ct_kernel 6 VGPRs.
__global__ __launch_bounds__(64, 2) void bob_v_tail_ct_kernel(const MtaTailArgs a) {
  using MT = Mont29<KD, G>;
  constexpr int STRIDE = cons_stride(KD);
  constexpr int EL = (int)kBobVLimbs;
  __shared__ uint32_t lds[WAVE_INST * KD];
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
  // N's bits below 2^768, wave-uniform, in a 24-limb scalar shift register
  uint32_t nw[EL];
  {
    const uint32_t* E = reinterpret_cast<const uint32_t*>(a.exp_ptr[inst]);
#pragma unroll
    for (int k = 0; k < EL; ++k) nw[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)E[k]);
  }
  auto put_row = [&](const uint32_t* row) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < L; ++j) stream[g * L + j] = row[g * L + j];
    __builtin_amdgcn_wave_barrier();
  };
  // T2[u] = a_enc^u (Montgomery form), u < 16
  uint32_t* T2 = a.table2 + (size_t)inst * 16 * KD;
  {
    const uint32_t* A = a.a_enc + (size_t)inst * K32;
    uint32_t y[L];
#pragma unroll
    for (int j = 0; j < L; ++j) {
      y[j] = digit_full(A, g * L + j);
      T2[g * L + j] = C[KD + g * L + j];   // T2[0] = 1 (R mod (N^2)')
    }
    put_row(C + 2 * KD);                   // R^2: y -> y R
    M.mul_s(y, y, stream);
#pragma unroll
    for (int j = 0; j < L; ++j) T2[KD + g * L + j] = y[j];
    __builtin_amdgcn_wave_barrier();
    lds_put<KD, G>(stream, y, g);          // T2[1] streamed for the powers
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (int u = 2; u < 16; ++u) {
      M.mul_s(y, y, stream);
#pragma unroll
      for (int j = 0; j < L; ++j) T2[(size_t)u * KD + g * L + j] = y[j];
    }
  }
  const uint32_t* Al = a.b + (size_t)inst * EL;
  uint32_t acc[L];
#pragma unroll
  for (int j = 0; j < L; ++j) acc[j] = a.state[(size_t)inst * KD + g * L + j];
  // bits 767 .. 0, limb by limb of alpha: square; N's sliding windows multiply T[d >> 1]
  // in after their last squaring; after every 4th squaring alpha's digit multiplies
  // its T2 row in
  uint32_t pend = 0, pend_d = 0;   // squarings until the open window's product (0: none), its odd digit
#pragma unroll 1
  for (int k = EL - 1; k >= 0; --k) {
    asm volatile("" : "+s"(k));   // the limb counter stays on the scalar unit
    uint32_t aw = Al[k];          // the 8 digits of this limb leave from the top
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
        __builtin_amdgcn_wave_barrier();
        lds_put<KD, G>(stream, acc, g);
        __builtin_amdgcn_wave_barrier();
        M.sqr_s(acc, acc, stream);
        if (pend != 0 && --pend == 0) {
          put_row(T + (size_t)(pend_d >> 1) * KD);
          M.mul_s(acc, acc, stream);
        }
      }
      const uint32_t nib = aw >> 28;
      aw <<= 4;
      uint32_t row[L];
      ct_row<L>(row, T2, nib, 16, KD, g);
      __builtin_amdgcn_wave_barrier();
      lds_put<KD, G>(stream, row, g);
      __builtin_amdgcn_wave_barrier();
      M.mul_s(acc, acc, stream);
    }
  }
  // exit: acc (1 + gamma N) / R modulo N^2 itself.  The lane index is taken afresh,
  // so the digit positions are worked out here and not carried along the chain in
  // registers from a_enc's conversion
  int ge = g;
  asm volatile("" : "+v"(ge));
  {
    const uint32_t* Bn = a.binom + (size_t)inst * K32;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < L; ++j) {
      M.n[j] = C0[ge * L + j];
      stream[ge * L + j] = digit_full(Bn, ge * L + j);
    }
    M.ninv = C0[3 * KD];
    __builtin_amdgcn_wave_barrier();
  }
  M.mul(acc, acc, stream);
  M.carry_exact(acc);
  M.sub_if_ge(acc);
  __builtin_amdgcn_wave_barrier();
  lds_put<KD, G>(stream, acc, g);
  __builtin_amdgcn_wave_barrier();
  uint32_t* O = a.out + (size_t)a.out_idx[inst] * K32;
  constexpr int LO = K32 / G;
#pragma unroll
  for (int q = 0; q < LO; ++q) O[ge * LO + q] = limb_full(stream, ge * LO + q);
}

// Both tails for the 3072-bit class: N^2 < 2^6144 at KD6 = 216 digits, 8 lanes of
// L6 = 27, behind the head modexp_slide_kernel<216, 8, 192, true> (the only 192-limb
// shape; state and table rows are its 216 digits in order).  EL = 8: the response,
// 256 squarings; EL = kBobVLimbs: v, 768 squarings.  Argument block, launch shape
// and regular access are mta_tail_ct_kernel's with 192-limb rows of a_enc, 1 + beta' N
// and out, 216-word rows of consts, table, state and table2, and N's low EL limbs in
// the scalar shift register.
// The exit product's bound for R = 2^(29 * 216) = 2^6264: acc < 2 (N^2)',
// (N^2)' < 2^29 N^2, 1 + beta' N < N^2 < 2^6144 and m < R give
//   (acc (1 + beta' N) + m N^2) / R < N^2 (2^30 2^6144 / 2^6264 + 1) = N^2 (2^-90 + 1) < 2 N^2,
// exact after carry_exact and one sub_if_ge.
// Registers: 27 digits per lane make the squaring's 64-bit columns, the operand, its
// doubled digits and the modulus 135 VGPRs, so what the 2048-bit kernels keep live
// beside them does not fit here.  For both widths the secret exponent is read from
// a.b[inst * EL + k] once per 8 digits (bob_v_tail_ct_kernel's way: the address
// depends on the instance and the public counter k only), the head's accumulator is
// loaded after the T2 build, and the lane index is taken afresh at the exit.  One
// body serves both (nothing differs but EL), behind two plain kernels.
namespace {

template <int EL>
__device__ __forceinline__ void tail_ct6144(const MtaTailArgs& a, uint32_t* lds) {
  using MT = Mont29<KD6, G>;
  constexpr int STRIDE = cons_stride(KD6);
  const int g = threadIdx.x % G;
  const int li = threadIdx.x / G;
  const uint32_t inst = blockIdx.x * WAVE_INST + li;   // whole waves: no bound check
  uint32_t* stream = lds + li * KD6;
  const uint32_t* C0 = a.consts + (size_t)a.mod_idx[inst] * STRIDE;   // N^2: the exit product
  const uint32_t* C = C0 + cons_scaled(KD6);                           // (N^2)': the chain's modulus
  MT M;
  M.init_lane(g);
#pragma unroll
  for (int j = 0; j < L6; ++j) M.n[j] = C[g * L6 + j];
  M.ninv = 1u;
  const uint32_t w = a.window, tw = 1u << (w - 1);
  const uint32_t* T = a.table + (size_t)inst * (tw + 1) * KD6;
  // N's bits below 2^(32 EL), wave-uniform, in an EL-limb scalar shift register
  uint32_t nw[EL];
  {
    const uint32_t* E = reinterpret_cast<const uint32_t*>(a.exp_ptr[inst]);
#pragma unroll
    for (int k = 0; k < EL; ++k) nw[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)E[k]);
  }
  auto put_row = [&](const uint32_t* row) {
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < L6; ++j) stream[g * L6 + j] = row[g * L6 + j];
    __builtin_amdgcn_wave_barrier();
  };
  // T2[u] = a_enc^u (Montgomery form), u < 16
  uint32_t* T2 = a.table2 + (size_t)inst * 16 * KD6;
  {
    const uint32_t* A = a.a_enc + (size_t)inst * K32_6;
    uint32_t y[L6];
#pragma unroll
    for (int j = 0; j < L6; ++j) {
      y[j] = digit_full<K32_6>(A, g * L6 + j);
      T2[g * L6 + j] = C[KD6 + g * L6 + j];   // T2[0] = 1 (R mod (N^2)')
    }
    put_row(C + 2 * KD6);                     // R^2: y -> y R
    M.mul_s(y, y, stream);
#pragma unroll
    for (int j = 0; j < L6; ++j) T2[KD6 + g * L6 + j] = y[j];
    __builtin_amdgcn_wave_barrier();
    lds_put<KD6, G>(stream, y, g);            // T2[1] streamed for the powers
    __builtin_amdgcn_wave_barrier();
#pragma unroll 1
    for (int u = 2; u < 16; ++u) {
      M.mul_s(y, y, stream);
#pragma unroll
      for (int j = 0; j < L6; ++j) T2[(size_t)u * KD6 + g * L6 + j] = y[j];
    }
  }
  const uint32_t* Bl = a.b + (size_t)inst * EL;
  // the head's accumulator, taken after the T2 build: held across those products it
  // went to scratch
  uint32_t acc[L6];
#pragma unroll
  for (int j = 0; j < L6; ++j) acc[j] = a.state[(size_t)inst * KD6 + g * L6 + j];
  // bits 32 EL - 1 .. 0, limb by limb of the secret exponent: square; N's sliding
  // windows multiply T[d >> 1] in after their last squaring; after every 4th
  // squaring the exponent's digit multiplies its T2 row in
  uint32_t pend = 0, pend_d = 0;   // squarings until the open window's product (0: none), its odd digit
#pragma unroll 1
  for (int k = EL - 1; k >= 0; --k) {
    asm volatile("" : "+s"(k));   // the limb counter stays on the scalar unit
    uint32_t bw = Bl[k];          // the 8 digits of this limb leave from the top
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
        __builtin_amdgcn_wave_barrier();
        lds_put<KD6, G>(stream, acc, g);
        __builtin_amdgcn_wave_barrier();
        M.sqr_s(acc, acc, stream);
        if (pend != 0 && --pend == 0) {
          put_row(T + (size_t)(pend_d >> 1) * KD6);
          M.mul_s(acc, acc, stream);
        }
      }
      const uint32_t nib = bw >> 28;
      bw <<= 4;
      uint32_t row[L6];
      ct_row<L6>(row, T2, nib, 16, KD6, g);
      __builtin_amdgcn_wave_barrier();
      lds_put<KD6, G>(stream, row, g);
      __builtin_amdgcn_wave_barrier();
      M.mul_s(acc, acc, stream);
    }
  }
  // exit: acc (1 + beta' N) / R modulo N^2 itself, the lane index taken afresh
  int ge = g;
  asm volatile("" : "+v"(ge));
  {
    const uint32_t* Bn = a.binom + (size_t)inst * K32_6;
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int j = 0; j < L6; ++j) {
      M.n[j] = C0[ge * L6 + j];
      stream[ge * L6 + j] = digit_full<K32_6>(Bn, ge * L6 + j);
    }
    M.ninv = C0[3 * KD6];
    __builtin_amdgcn_wave_barrier();
  }
  M.mul(acc, acc, stream);
  M.carry_exact(acc);
  M.sub_if_ge(acc);
  __builtin_amdgcn_wave_barrier();
  lds_put<KD6, G>(stream, acc, g);
  __builtin_amdgcn_wave_barrier();
  uint32_t* O = a.out + (size_t)a.out_idx[inst] * K32_6;
  constexpr int LO = K32_6 / G;
#pragma unroll
  for (int q = 0; q < LO; ++q) O[ge * LO + q] = limb_full<K32_6, KD6>(stream, ge * LO + q);
}

}  // namespace

__global__ __launch_bounds__(64, 2) void mta_tail_ct6144_kernel(const MtaTailArgs a) {
  __shared__ uint32_t lds[WAVE_INST * KD6];
  tail_ct6144<8>(a, lds);
}

__global__ __launch_bounds__(64, 2) void bob_v_tail_ct6144_kernel(const MtaTailArgs a) {
  __shared__ uint32_t lds[WAVE_INST * KD6];
  tail_ct6144<(int)kBobVLimbs>(a, lds);
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

hipError_t launch_mta_tail_ct(const MtaTailArgs& a, hipStream_t st) {
  if (!a.count_pad || a.count_pad % kMtaTailPad || a.window < 1 || a.window > 7) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mta_tail_ct_kernel, dim3(a.count_pad / kMtaTailPad), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_bob_v_tail_ct(const MtaTailArgs& a, hipStream_t st) {
  if (!a.count_pad || a.count_pad % kMtaTailPad || a.window < 1 || a.window > 7) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bob_v_tail_ct_kernel, dim3(a.count_pad / kMtaTailPad), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_mta_tail_ct6144(const MtaTailArgs& a, hipStream_t st) {
  if (!a.count_pad || a.count_pad % kMtaTailPad || a.window < 1 || a.window > 7) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mta_tail_ct6144_kernel, dim3(a.count_pad / kMtaTailPad), dim3(64), 0, st, a);
  return hipGetLastError();
}

hipError_t launch_bob_v_tail_ct6144(const MtaTailArgs& a, hipStream_t st) {
  if (!a.count_pad || a.count_pad % kMtaTailPad || a.window < 1 || a.window > 7) return hipErrorInvalidValue;
  hipLaunchKernelGGL(bob_v_tail_ct6144_kernel, dim3(a.count_pad / kMtaTailPad), dim3(64), 0, st, a);
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
