// The integer responses of the MtA provers on gfx950 (range_proofs.rs:196-200,
// :330-346): out = e x + y over 32-bit limbs, no modulus, for the public challenge
// e < 2^256 and SECRET x, y (s1 = e a + alpha, s2 = e ro + gamma, t1 = e beta' + gamma,
// t2 = e sigma + tau).  One response is a few hundred MACs, so the shape is about
// regular access, not throughput: a wave holds kRespPad instances of 16 lanes each,
// the rows are staged in LDS by coalesced loads (one thread per response reading
// global memory word by word is what vhash.hip's ped_hash once paid for), every lane
// sums the eight products of its columns k = g, g + 16, .. from LDS, and the carries
// are resolved by one pass over the columns.
//
// Regular access: whole blocks (the host pads every array to count_pad rows, so
// there is no bound check), every trip count comes from (xl, yl) alone, every
// address from the instance index and the loop counters; a lane past the end of a
// row reads a clamped index and masks the value.  The carry pass is a chain of
// 64-bit additions without a branch; the 16 lanes of an instance run it alike over
// the same LDS words and store the same limbs.
#include "prove_geom.hpp"
#include "verify.h"

namespace fsdkr {

namespace {
constexpr uint32_t RL = 16;                 // lanes per instance
constexpr uint32_t RX = 160;                // x behind 7 zero limbs: index 7 + k - i, k < 144
constexpr uint32_t RY = 144;                // y, zero-extended to the padded column count
constexpr uint32_t RS = 160;                // column words: index k + 2, k < 144
static_assert(kRespPad * RL == 64, "one wave per block");
static_assert(kRespMaxLimbs + 8 + 1 <= RY - 7 && RY + 7 <= RX && RY + 2 <= RS, "the padded columns fit the LDS rows");
}  // namespace

__global__ __launch_bounds__(64) void resp_ct_kernel(const RespCtArgs a) {
  __shared__ uint32_t sE[kRespPad][8], sX[kRespPad][RX], sY[kRespPad][RY];
  __shared__ uint32_t sA[kRespPad][RS], sB[kRespPad][RS], sC[kRespPad][RS], sO[kRespPad][RY];
  const uint32_t g = threadIdx.x % RL, li = threadIdx.x / RL;
  const size_t inst = (size_t)blockIdx.x * kRespPad + li;   // whole blocks: no bound check
  const uint32_t xl = a.xl, yl = a.yl, ol = a.ol;
  const uint32_t* x = a.x + inst * xl;
  const uint32_t* y = a.y + inst * yl;
  const uint32_t* e = a.e + inst * 8;
  uint32_t *E = sE[li], *X = sX[li], *Y = sY[li], *A = sA[li], *B = sB[li], *C = sC[li], *O = sO[li];
#pragma unroll
  for (uint32_t t = 0; t < RX / RL; ++t) X[t * RL + g] = 0u;
#pragma unroll
  for (uint32_t t = 0; t < RY / RL; ++t) Y[t * RL + g] = 0u;
  B[g] = 0u;   // B[0], C[0], C[1] have no column below them
  C[g] = 0u;
  __syncthreads();
  // stage the rows: a lane past the row's end loads its last limb and keeps zero
  // (every loop below runs at least once -- xl, yl >= 1 -- and is written bottom-tested
  // and kept rolled (no unrolling, no interleaving: both add remainder code behind
  // a uniform condition tested through VCC), so its only branch is the scalar back-edge)
  uint32_t t = 0;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  do {
    const uint32_t j = t * RL + g, in = j < xl ? 1u : 0u;
    X[7 + j] = x[in ? j : xl - 1] & (0u - in);
  } while (++t < (xl + RL - 1) / RL);
  t = 0;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  do {
    const uint32_t j = t * RL + g, in = j < yl ? 1u : 0u;
    Y[j] = y[in ? j : yl - 1] & (0u - in);
  } while (++t < (yl + RL - 1) / RL);
  E[g & 7u] = e[g & 7u];
  __syncthreads();
  // column k: y_k + sum_i e_i x_(k - i) < 2^68, as three words at k, k + 1, k + 2
  const uint32_t T = (ol + RL - 1) / RL;
  t = 0;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  do {
    const uint32_t k = t * RL + g;
    uint64_t lo = Y[k], hi = 0;
#pragma unroll
    for (uint32_t i = 0; i < 8; ++i) {
      const uint64_t p = (uint64_t)E[i] * X[7 + k - i];
      lo += (uint32_t)p;
      hi += p >> 32;
    }
    hi += lo >> 32;
    A[k] = (uint32_t)lo;
    B[k + 1] = (uint32_t)hi;
    C[k + 2] = (uint32_t)(hi >> 32);
  } while (++t < T);
  __syncthreads();
  uint64_t c = 0;
  uint32_t k = 0;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  do {
    c += (uint64_t)A[k] + B[k] + C[k];
    O[k] = (uint32_t)c;
    c >>= 32;
  } while (++k < ol);
  __syncthreads();
  uint32_t* out = a.out + inst * ol;
  t = 0;
#pragma clang loop unroll(disable) vectorize(disable) interleave(disable)
  do {
    const uint32_t q = min(t * RL + g, ol - 1);   // the lanes past the end repeat the top limb
    out[q] = O[q];
  } while (++t < T);
}

hipError_t launch_resp_ct(const RespCtArgs& a, hipStream_t st) {
  if (!a.count_pad) return hipSuccess;
  if (a.count_pad % kRespPad || !a.xl || !a.yl || a.xl > kRespMaxLimbs || a.yl > kRespMaxLimbs ||
      a.ol != resp_out_limbs(a.xl, a.yl))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(resp_ct_kernel, dim3(a.count_pad / kRespPad), dim3(64), 0, st, a);
  return hipGetLastError();
}

}  // namespace fsdkr
