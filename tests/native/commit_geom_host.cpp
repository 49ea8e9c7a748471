// Host-side view of the launch geometry of fsdkr_pedersen_commit_ct
// (fs-dkr_amd/csrc/commit_geom.hpp, used by comb_ct_host.cpp): reads lines of
//   nl xl yl count n_keys per-key-count...
// from stdin and prints "b vx vy ipb" per line, computed as the entry point does:
// b from count / n_keys and the table entry size of the width (72 digits of 29
// bits at nl = 64, 108 at nl = 96: commit_launch's shapes), the block from the
// padded-lane sum over the per-key counts.  The memory cap is 16 GiB.
#include <cstdio>
#include <vector>

#include "commit_geom.hpp"

int main() {
  unsigned nl, xl, yl, count, nk;
  while (scanf("%u %u %u %u %u", &nl, &xl, &yl, &count, &nk) == 5) {
    if ((nl != 64 && nl != 96) || !nk || !count || nk > 4096) return 1;
    std::vector<uint32_t> per(nk);
    unsigned sum = 0;
    for (unsigned k = 0; k < nk; ++k) {
      if (scanf("%u", &per[k]) != 1) return 1;
      sum += per[k];
    }
    if (sum != count) return 1;
    const size_t KD = nl == 64 ? 72 : 108;
    const uint32_t b = fsdkr::commit_choose_b(xl, yl, (double)count / nk, nk, KD * 4, (size_t)16 << 30);
    if (!b) return 1;
    const uint32_t vx = (8 * xl + b - 1) / b, vy = (8 * yl + b - 1) / b;
    const uint32_t ipb = fsdkr::commit_ct_ipb(fsdkr::commit_padded_lanes(per.data(), nk));
    printf("%u %u %u %u\n", b, vx, vy, ipb);
  }
  return 0;
}
