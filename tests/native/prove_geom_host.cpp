// Host-side view of the whole provers' packing (fs-dkr_amd/csrc/prove_geom.hpp, used
// by mta_prove.cpp and resp_ct.hip), meant to be built with -fsanitize=address,undefined
// and run on its own.  For nl = 64 and 96 it prints the row widths
//   "bob nl xl yl s1 s2 t1 t2" and "alice nl xl yl s1 s2",
// then packs `count` proofs (count from argv, default 5) of exactly-sized heap rows
// through interleave_rows / repeat_keys / take_rows as the entries do and checks every
// limb: the slot order, the zero-extension, that no row is read or written past its
// end (the sanitizer's part), and that take_rows inverts interleave_rows.  Exit
// status 0 and a last line "ok" when everything holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "prove_geom.hpp"

using namespace fsdkr;

static int fail(const char* what, unsigned nl) {
  printf("FAIL %s nl=%u\n", what, nl);
  return 1;
}

// a row value that names its source: (tag, proof, limb)
static uint32_t val(uint32_t tag, uint32_t p, uint32_t k) { return (tag << 24) | (p << 12) | (k + 1); }

static std::vector<uint32_t> rows(uint32_t tag, uint32_t count, uint32_t l) {
  std::vector<uint32_t> v((size_t)count * l);
  for (uint32_t p = 0; p < count; ++p)
    for (uint32_t k = 0; k < l; ++k) v[(size_t)p * l + k] = val(tag, p, k);
  return v;
}

static bool check_slot(const std::vector<uint32_t>& dst, uint32_t dl, uint32_t per, uint32_t slot, uint32_t tag,
                       uint32_t sl, uint32_t count) {
  for (uint32_t p = 0; p < count; ++p)
    for (uint32_t k = 0; k < dl; ++k)
      if (dst[((size_t)p * per + slot) * dl + k] != (k < sl ? val(tag, p, k) : 0u)) return false;
  return true;
}

int main(int argc, char** argv) {
  const uint32_t count = argc > 1 ? (uint32_t)atoi(argv[1]) : 5u;
  if (!count || count > 4000) return 2;
  if (resp_out_limbs(1, 1) != 10 || resp_out_limbs(128, 128) != 137 || resp_out_limbs(8, 40) != 41) return fail("out limbs", 0);
  if (resp_pad(1) != 4 || resp_pad(4) != 4 || resp_pad(5) != 8 || resp_pad(0) != 0) return fail("pad", 0);
  for (uint32_t nl : {64u, 96u}) {
    const BobWidths b = bob_widths(nl);
    printf("bob %u %u %u %u %u %u %u\n", nl, b.xl, b.yl, b.s1, b.s2, b.t1, b.t2);
    const uint32_t xs[4] = {b.b, b.alpha, b.beta_prim, b.gamma}, ys[4] = {b.ro, b.ro_prim, b.sigma, b.tau};
    std::vector<uint32_t> hx((size_t)4 * count * b.xl, 0xdeadbeefu), hy((size_t)4 * count * b.yl, 0xdeadbeefu);
    for (uint32_t s = 0; s < 4; ++s) {
      if (xs[s] > b.xl || ys[s] > b.yl) return fail("bob row wider than the comb's", nl);
      const std::vector<uint32_t> x = rows(1 + s, count, xs[s]), y = rows(5 + s, count, ys[s]);
      interleave_rows(hx.data(), b.xl, 4, s, x.data(), xs[s], count);
      interleave_rows(hy.data(), b.yl, 4, s, y.data(), ys[s], count);
    }
    for (uint32_t s = 0; s < 4; ++s)
      if (!check_slot(hx, b.xl, 4, s, 1 + s, xs[s], count) || !check_slot(hy, b.yl, 4, s, 5 + s, ys[s], count))
        return fail("bob interleave", nl);
    std::vector<uint32_t> key(count), k4((size_t)4 * count);
    for (uint32_t p = 0; p < count; ++p) key[p] = p % 3;
    repeat_keys(k4.data(), key.data(), 4, count);
    for (uint32_t i = 0; i < 4 * count; ++i)
      if (k4[i] != (i / 4) % 3) return fail("repeat_keys", nl);
    // the comb's results back into per-field rows
    const std::vector<uint32_t> cm = rows(9, 4 * count, nl);
    for (uint32_t s = 0; s < 4; ++s) {
      std::vector<uint32_t> f((size_t)count * nl);
      take_rows(f.data(), cm.data(), nl, 4, s, count);
      for (uint32_t p = 0; p < count; ++p)
        for (uint32_t k = 0; k < nl; ++k)
          if (f[(size_t)p * nl + k] != val(9, 4 * p + s, k)) return fail("take_rows", nl);
    }
    const AliceWidths a = alice_widths(nl);
    printf("alice %u %u %u %u %u\n", nl, a.xl, a.yl, a.s1, a.s2);
    const uint32_t ax[2] = {a.a, a.alpha}, ay[2] = {a.ro, a.gamma};
    std::vector<uint32_t> gx((size_t)2 * count * a.xl, 0xdeadbeefu), gy((size_t)2 * count * a.yl, 0xdeadbeefu);
    for (uint32_t s = 0; s < 2; ++s) {
      if (ax[s] > a.xl || ay[s] > a.yl) return fail("alice row wider than the comb's", nl);
      const std::vector<uint32_t> x = rows(1 + s, count, ax[s]), y = rows(5 + s, count, ay[s]);
      interleave_rows(gx.data(), a.xl, 2, s, x.data(), ax[s], count);
      interleave_rows(gy.data(), a.yl, 2, s, y.data(), ay[s], count);
    }
    for (uint32_t s = 0; s < 2; ++s)
      if (!check_slot(gx, a.xl, 2, s, 1 + s, ax[s], count) || !check_slot(gy, a.yl, 2, s, 5 + s, ay[s], count))
        return fail("alice interleave", nl);
    // every response row fits the kernel's LDS rows
    for (uint32_t l : {b.s1, b.s2, b.t1, b.t2, a.s1, a.s2})
      if (l > kRespMaxLimbs + kProveELimbs + 1) return fail("response wider than the kernel's rows", nl);
  }
  printf("ok\n");
  return 0;
}
