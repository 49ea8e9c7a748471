// Launch geometry of the constant-time two-base comb (comb_ct.hip,
// comb_ct_host.cpp): the column count b, the padded lane count and the
// instances per block.  Host-only arithmetic on counts and limb widths, with
// nothing from HIP, so that a plain C++ program can check it (tests/native/
// commit_geom_host.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace fsdkr {

constexpr int kCommitLanes = 4;            // lanes per commitment
constexpr uint32_t kCommitBlock = 256;     // threads of the full block (kernels.h BLOCK)

// Column count b of the two-base comb with h = 4: the cheapest per commitment,
//   (b - 1) + b (v_x + v_y) + (v_x + v_y) (11 + 4 b) / per_key
// (squarings, products, and a key's eleven table products and 4 b chain squarings per
// table shared by its instances), over 1 <= b <= 64 whose tables fit: a key's
// (v_x + v_y) 16 rows within kCommitKeyBudget (they are re-read by every block of the
// key, so they should stay in L2) and all keys' within `cap`.  0: nothing fits.
constexpr size_t kCommitKeyBudget = (size_t)512 << 10;
inline uint32_t commit_choose_b(uint32_t xl, uint32_t yl, double per_key, size_t n_keys, size_t entry_bytes, size_t cap) {
  uint32_t best = 0;
  double best_cost = 0.0;
  for (uint32_t b = 1; b <= 64; ++b) {
    const uint32_t vx = (8 * xl + b - 1) / b, vy = (8 * yl + b - 1) / b;
    const size_t key_bytes = (size_t)(vx + vy) * 16 * entry_bytes;
    if (key_bytes > kCommitKeyBudget || key_bytes * n_keys > cap) continue;
    const double cost = (double)(b - 1) + (double)b * (vx + vy) + (double)(vx + vy) * (11.0 + 4.0 * b) / per_key;
    if (!best || cost < best_cost) {
      best = b;
      best_cost = cost;
    }
  }
  return best;
}

// lanes of a launch: every key's run padded to whole small blocks (16 instances)
inline uint64_t commit_padded_lanes(const uint32_t* per, size_t n_keys) {
  uint64_t lanes = 0;
  for (size_t k = 0; k < n_keys; ++k) lanes += (uint64_t)((per[k] + 15) / 16 * 16) * kCommitLanes;
  return lanes;
}

// instances per block for a launch of `lanes` lanes in all (as comb_exp picks its block)
inline uint32_t commit_ct_ipb(uint64_t lanes) {
  return lanes <= 256u * 4u * 64u ? 64u / kCommitLanes : kCommitBlock / kCommitLanes;
}

}  // namespace fsdkr
