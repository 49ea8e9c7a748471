// Pedersen-style commitments h1^x h2^y mod N~ for SECRET x, y on gfx950: the
// Lim-Lee comb of comb.hip in regular access (range_proofs.rs:58,62-63,270-295,
// zk_pdl_with_slack.rs:177-186: z, w, z', t of the range proofs, the PDL prover's
// commitment).  h1, h2 and N~ are public and belong to the verifier's key, so
// the tables are those of the public comb (fb_table_kernel's chains,
// comb_build_kernel's levels), with h = 4 rows: 16 entries per table.  The two
// bases of a key share the column count b and have their own block counts
//   v_x = ceil(32 xl / (4 b)),  v_y = ceil(32 yl / (4 b)),
// so one commitment is b - 1 squarings and b (v_x + v_y) - 1 products, and the
// exit product, with no product on the host.
//
// commit_ct_kernel is comb_exp_kernel with two changes: every table read scans
// the 16 rows of its table and keeps one through a mask (ct_row), and each
// column's products run over both bases' blocks.  The digits come from
// comb_sched_kernel as it stands (its addresses depend on public indices only);
// the schedule buffers are secret-derived and the host zeroes them.
//
// Regular access: a block holds instances of ONE key (the host orders them by key
// and pads every key's run to whole blocks with x = y = 0 rows that write a
// scratch row), so there is no bound check, the key's constants and tables are
// addressed from a scalar load, and no address, branch or trip count depends on
// x or y: the loop runs b (v_x + v_y) steps from the launch's limb counts.
#include "commit_geom.hpp"
#include "fixedbase.h"
#include "mont29.hpp"

namespace fsdkr {

template <int KD, int G, int K32>
__global__ __launch_bounds__(BLOCK) void commit_ct_kernel(const CommitCtArgs a) {
  using MT = Mont29<KD, G>;
  constexpr int L = MT::L;
  constexpr int IPB = BLOCK / G;
  constexpr int STRIDE = cons_stride(KD);
  constexpr uint32_t TS = 16;   // rows per table (h = 4)
  static_assert(scaled_ok(KD, K32), "quotient-scaled chains: N' within R/4");
  __shared__ uint32_t lds[IPB * KD];
  const int g = threadIdx.x % G;
  const int li = threadIdx.x / G;
  const uint32_t inst = blockIdx.x * (blockDim.x / G) + li;   // whole blocks: no bound check
  const uint32_t key = a.blk_key[blockIdx.x];                 // block-uniform (scalar)
  uint32_t* stream = lds + li * KD;
  const uint32_t* C0 = a.consts + (size_t)key * STRIDE;
  const uint32_t* C = C0 + cons_scaled(KD);
  MT M;
  M.init_lane(g);
#pragma unroll
  for (int k = 0; k < L; ++k) M.n[k] = C[g * L + k];
  M.ninv = C[3 * KD];
  const uint32_t vx = a.vx, vt = a.vx + a.vy;
  const uint32_t* tx = a.tabx + (size_t)key * a.vx * TS * KD;
  const uint32_t* ty = a.taby + (size_t)key * a.vy * TS * KD;
  const uint16_t* Sx = a.sx + (size_t)inst * a.vx * a.b;
  const uint16_t* Sy = a.sy + (size_t)inst * a.vy * a.b;
  // step (column k from b - 1 down, block j < v_x + v_y): the x blocks of the
  // column, then the y blocks; each base's digits in comb_sched's order
  uint32_t acc[L];
  ct_row<L>(acc, tx, Sx[0], TS, KD, g);
  uint32_t j = 0, ix = 1, iy = 0;
  const uint32_t steps = vt * a.b;
#pragma unroll 1
  for (uint32_t st = 1; st < steps; ++st) {
    if (++j == vt) {   // next column: square first
      j = 0;
      __builtin_amdgcn_wave_barrier();
      lds_put<KD, G>(stream, acc, g);
      __builtin_amdgcn_wave_barrier();
      M.sqr_s(acc, acc, stream);
    }
    const bool in_x = j < vx;   // scalar: the launch's geometry
    const uint32_t* T = in_x ? tx + (size_t)j * TS * KD : ty + (size_t)(j - vx) * TS * KD;
    const uint32_t d = in_x ? Sx[ix] : Sy[iy];
    ix += in_x ? 1u : 0u;
    iy += in_x ? 0u : 1u;
    uint32_t row[L];
    ct_row<L>(row, T, d, TS, KD, g);
    __builtin_amdgcn_wave_barrier();
    lds_put<KD, G>(stream, row, g);
    __builtin_amdgcn_wave_barrier();
    M.mul_s(acc, acc, stream);
  }
  // leave Montgomery form: acc * 1 / R, then exact reduction (modulo N~ itself)
#pragma unroll
  for (int k = 0; k < L; ++k) M.n[k] = C0[g * L + k];
  M.ninv = C0[3 * KD];
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int k = 0; k < L; ++k) stream[g * L + k] = (g == 0 && k == 0) ? 1u : 0u;
  __builtin_amdgcn_wave_barrier();
  M.mul(acc, acc, stream);
  M.carry_exact(acc);
  M.sub_if_ge(acc);
  __builtin_amdgcn_wave_barrier();
  lds_put<KD, G>(stream, acc, g);
  __builtin_amdgcn_wave_barrier();
  uint32_t* O = a.out + (size_t)a.out_idx[inst] * K32;
  constexpr int LO = K32 / G;
#pragma unroll
  for (int k = 0; k < LO; ++k) O[g * LO + k] = limb_of(stream, KD, g * LO + k);
}

template <int KD, int G, int K32>
static hipError_t commit_launch(const CommitCtArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((commit_ct_kernel<KD, G, K32>), dim3(a.blocks), dim3(a.ipb * G), 0, st, a);
  return hipGetLastError();
}

static_assert(kCommitBlock == (uint32_t)BLOCK, "commit_ct_ipb's full block is the kernels' BLOCK");

hipError_t launch_commit_ct(uint32_t k32, const CommitCtArgs& a, hipStream_t st) {
  if (!a.blocks) return hipSuccess;
  if (!a.vx || !a.vy || !a.b || (a.ipb != 64u / kCommitLanes && a.ipb != (uint32_t)BLOCK / kCommitLanes))
    return hipErrorInvalidValue;
  switch (k32) {
    case 64: return commit_launch<72, kCommitLanes, 64>(a, st);
    case 96: return commit_launch<108, kCommitLanes, 96>(a, st);
    default: return hipErrorInvalidValue;
  }
}

}  // namespace fsdkr
