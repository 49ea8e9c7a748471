// secp256k1 scalar multiplication for SECRET scalars (gfx950, secp256k1_ct.hpp):
//   ec_mul_g_ct          k G, the prover's G*share, G*a_k, G*alpha   refresh_message.rs:51-145,
//                        zk_pdl_with_slack.rs:53-111, range_proofs.rs:480-484
//   ec_msm_ct_term/sum   sum_j s_j P_j for points other than G
// Between a kernel's first vector load and its end no branch, loop bound, memory
// address, shuffle source lane or early exit depends on a scalar: every launch
// covers whole waves of padded inputs (no bound checks), selections go through
// arithmetic masks, and per-thread arrays are indexed by loop counters only.
#include "secp256k1_ct.hpp"
#include "verify.h"

namespace fsdkr {

using namespace ec;

// 0xffffffff iff a == b (a, b < 2^31)
__device__ __forceinline__ uint32_t eq_mask(uint32_t a, uint32_t b) { return 0u - (((a ^ b) - 1u) >> 31); }

// k G by a comb without doublings and without a zero digit: with the 64 nibbles
// k_i of the raw 256-bit scalar (no reduction mod q: the group law absorbs it)
//   k G = sum_i T[i][k_i] - C,  T[i][d] = (d + 1) 16^i G,  C = ((16^64 - 1) / 15) G.
// No table entry is the identity, so every step is one mixed complete addition.
// Four lanes per scalar: lane j sums windows 16j .. 16j+15 (limbs 2j, 2j+1), two
// __shfl_xor rounds of complete additions leave the total in all four lanes,
// and every lane subtracts C and converts (lanes run in lockstep, so a lane-0
// tail would save nothing and cost an exec-mask branch); lane j stores words
// 4j .. 4j+3 of the result.  Window i reads all 16 entries of row i from
// global memory (the 64 KB table stays in L2; the rows a wave reads are those
// of its four j values) and keeps one by mask.
__global__ void __launch_bounds__(64) ec_mul_g_ct_kernel(const EcMulGCtArgs a) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t p = tid >> 2, j = tid & 3u;
  const uint32_t* sc = a.scalars + (size_t)p * 8 + 2 * j;
  uint64_t k = (uint64_t)sc[0] | ((uint64_t)sc[1] << 32);
  __builtin_amdgcn_s_setprio(3);   // a serial EC chain per lane on few waves
  Proj acc;
  proj_set_id(acc);
  const uint4* row = reinterpret_cast<const uint4*>(a.table) + (size_t)j * 16 * 16 * 4;
#pragma unroll 1
  for (int w = 0; w < 16; ++w) {
    const uint32_t nib = (uint32_t)k & 15u;
    k >>= 4;
    uint32_t e[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) e[i] = 0;
#pragma unroll
    for (uint32_t d = 0; d < 16; ++d) {
      const uint32_t m = eq_mask(d, nib);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint4 v = row[d * 4 + q];
        e[4 * q + 0] |= v.x & m;
        e[4 * q + 1] |= v.y & m;
        e[4 * q + 2] |= v.z & m;
        e[4 * q + 3] |= v.w & m;
      }
    }
    Fe x, y;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      x.v[i] = e[i];
      y.v[i] = e[8 + i];
    }
    proj_add_aff_ct(acc, acc, x, y);
    row += 16 * 4;
  }
  // quad sum: lanes (0,1) and (2,3), then the two halves
#pragma unroll 1
  for (int step = 1; step <= 2; step <<= 1) {
    Proj o;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      o.X.v[i] = (uint32_t)__shfl_xor((int)acc.X.v[i], step);
      o.Y.v[i] = (uint32_t)__shfl_xor((int)acc.Y.v[i], step);
      o.Z.v[i] = (uint32_t)__shfl_xor((int)acc.Z.v[i], step);
    }
    proj_add_ct(acc, acc, o);
  }
  Fe x, y;
  fe_load(x, a.table + (size_t)1024 * 16);       // -C
  fe_load(y, a.table + (size_t)1024 * 16 + 8);
  proj_add_aff_ct(acc, acc, x, y);
  proj_to_aff_ct(x, y, acc);
  // lane j's quarter of x | y, chosen by the lane id
  const uint32_t m0 = eq_mask(j, 0), m1 = eq_mask(j, 1), m2 = eq_mask(j, 2), m3 = eq_mask(j, 3);
  uint4 o;
  o.x = (x.v[0] & m0) | (x.v[4] & m1) | (y.v[0] & m2) | (y.v[4] & m3);
  o.y = (x.v[1] & m0) | (x.v[5] & m1) | (y.v[1] & m2) | (y.v[5] & m3);
  o.z = (x.v[2] & m0) | (x.v[6] & m1) | (y.v[2] & m2) | (y.v[6] & m3);
  o.w = (x.v[3] & m0) | (x.v[7] & m1) | (y.v[3] & m2) | (y.v[7] & m3);
  reinterpret_cast<uint4*>(a.out)[(size_t)p * 4 + j] = o;
}

// One thread per term: k P by 64 fixed 4-bit windows from the top (four
// complete doublings, one complete addition of the masked-scan entry) over a
// 16-entry projective table d P, d = 0 .. 15 (d = 0 the identity).  No GLV
// split: its sign handling would be one more thing to mask.
__global__ void __launch_bounds__(64) ec_msm_ct_term_kernel(const EcMsmCtArgs a) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t k[8];
  Fe x, y;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    k[i] = a.scalars[(size_t)q * 8 + i];
    x.v[i] = a.points[(size_t)q * 16 + i];
    y.v[i] = a.points[(size_t)q * 16 + 8 + i];
  }
  __builtin_amdgcn_s_setprio(3);
  Proj T[16];
  proj_set_id(T[0]);
  proj_from_aff_ct(T[1], x, y);
#pragma unroll 1
  for (int d = 2; d < 16; ++d) proj_add_ct(T[d], T[d - 1], T[1]);
  Proj acc;
  proj_set_id(acc);
#pragma unroll 1
  for (int w = 0; w < 64; ++w) {
#pragma unroll 1
    for (int i = 0; i < 4; ++i) proj_dbl_ct(acc, acc);
    const uint32_t nib = k[7] >> 28;   // the top nibble; the scalar shifts left by one window
#pragma unroll
    for (int i = 7; i > 0; --i) k[i] = (k[i] << 4) | (k[i - 1] >> 28);
    k[0] <<= 4;
    Proj e;
#pragma unroll
    for (int i = 0; i < 8; ++i) e.X.v[i] = e.Y.v[i] = e.Z.v[i] = 0;
#pragma unroll 1
    for (uint32_t d = 0; d < 16; ++d) {
      const uint32_t m = eq_mask(d, nib);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        e.X.v[i] |= T[d].X.v[i] & m;
        e.Y.v[i] |= T[d].Y.v[i] & m;
        e.Z.v[i] |= T[d].Z.v[i] & m;
      }
    }
    proj_add_ct(acc, acc, e);
  }
  uint32_t* J = a.scratch + (size_t)q * 24;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    J[i] = acc.X.v[i];
    J[8 + i] = acc.Y.v[i];
    J[16 + i] = acc.Z.v[i];
  }
}

// one thread per output: the sum of its terms by complete additions, then affine
__global__ void __launch_bounds__(64) ec_msm_ct_sum_kernel(const EcMsmCtArgs a) {
  const uint32_t o = blockIdx.x * blockDim.x + threadIdx.x;
  __builtin_amdgcn_s_setprio(3);
  Proj acc;
  proj_set_id(acc);
#pragma unroll 1
  for (uint32_t j = 0; j < a.terms; ++j) {
    const uint32_t* J = a.scratch + ((size_t)o * a.terms + j) * 24;
    Proj t;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      t.X.v[i] = J[i];
      t.Y.v[i] = J[8 + i];
      t.Z.v[i] = J[16 + i];
    }
    proj_add_ct(acc, acc, t);
  }
  Fe x, y;
  proj_to_aff_ct(x, y, acc);
  uint32_t* out = a.out + (size_t)o * 16;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    out[i] = x.v[i];
    out[8 + i] = y.v[i];
  }
}

// count_pad scalars, a multiple of kEcMulGPad: whole waves of four-lane quads
hipError_t launch_ec_mul_g_ct(const EcMulGCtArgs& a, hipStream_t st) {
  if (!a.count_pad || a.count_pad % kEcMulGPad) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ec_mul_g_ct_kernel, dim3(a.count_pad / kEcMulGPad), dim3(64), 0, st, a);
  return hipGetLastError();
}
// count_pad outputs, a multiple of kEcMsmCtPad: count_pad * terms term threads in whole waves
hipError_t launch_ec_msm_ct(const EcMsmCtArgs& a, hipStream_t st) {
  if (!a.count_pad || a.count_pad % kEcMsmCtPad || !a.terms) return hipErrorInvalidValue;
  hipLaunchKernelGGL(ec_msm_ct_term_kernel, dim3(a.count_pad / 64 * a.terms), dim3(64), 0, st, a);
  hipLaunchKernelGGL(ec_msm_ct_sum_kernel, dim3(a.count_pad / 64), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace fsdkr
