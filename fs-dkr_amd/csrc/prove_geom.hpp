// Row widths and packing of the whole-prover entries (mta_prove.cpp, resp_ct.hip):
// the limbs of every response row, the order of the comb's instances and the
// zero-extension of narrower rows.  Host-only arithmetic on counts and limb widths,
// with nothing from HIP, so that a plain C++ program can check it (tests/native/
// prove_geom_host.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace fsdkr {

constexpr uint32_t kProveELimbs = 8;    // the challenge: a SHA-256 digest
constexpr uint32_t kRespPad = 4;        // instances per block of resp_ct_kernel
constexpr uint32_t kRespMaxLimbs = 128; // widest x or y row of resp_ct_kernel

// limbs of e * x + y for e < 2^256, x of xl limbs, y of yl limbs:
// e x < 2^(32 (xl + 8)), so the sum is below 2^(32 max(xl + 8, yl) + 1)
inline uint32_t resp_out_limbs(uint32_t xl, uint32_t yl) {
  const uint32_t a = xl + kProveELimbs;
  return (a > yl ? a : yl) + 1;
}

inline uint32_t resp_pad(uint32_t count) { return (count + kRespPad - 1) / kRespPad * kRespPad; }

// Bob's rows in the width class nl (range_proofs.rs:266-272, :330-346)
struct BobWidths {
  uint32_t b, alpha, beta_prim, gamma, ro, ro_prim, sigma, tau;   // inputs
  uint32_t xl, yl;                                                // the comb's rows
  uint32_t s1, s2, t1, t2;                                        // responses
};
inline BobWidths bob_widths(uint32_t nl) {
  BobWidths w;
  w.b = 8;
  w.alpha = 24;
  w.beta_prim = nl;
  w.gamma = nl + 16;
  w.ro = w.sigma = nl + 8;
  w.ro_prim = w.tau = nl + 24;
  w.xl = nl + 16;   // the widest of b, alpha, beta', gamma
  w.yl = nl + 24;   // the widest of ro, ro', sigma, tau
  w.s1 = resp_out_limbs(w.b, w.alpha);            // 25
  w.s2 = resp_out_limbs(w.ro, w.ro_prim);         // nl + 25
  w.t1 = resp_out_limbs(w.beta_prim, w.gamma);    // nl + 17
  w.t2 = resp_out_limbs(w.sigma, w.tau);          // nl + 25
  return w;
}

// Alice's rows (range_proofs.rs:54-57, :196-200)
struct AliceWidths {
  uint32_t a, alpha, gamma, ro;
  uint32_t xl, yl;
  uint32_t s1, s2;
};
inline AliceWidths alice_widths(uint32_t nl) {
  AliceWidths w;
  w.a = w.alpha = 24;
  w.gamma = nl + 24;
  w.ro = nl + 8;
  w.xl = 24;
  w.yl = nl + 24;
  w.s1 = resp_out_limbs(w.a, w.alpha);   // 33
  w.s2 = resp_out_limbs(w.ro, w.gamma);  // nl + 25
  return w;
}

// The comb's instance rows: proof p's `per` instances are rows per * p .. per * p +
// per - 1.  Copies src [count][sl] into slot `slot` of dst [per * count][dl],
// zero-extended (sl <= dl).
inline void interleave_rows(uint32_t* dst, uint32_t dl, uint32_t per, uint32_t slot, const uint32_t* src, uint32_t sl,
                            uint32_t count) {
  for (uint32_t p = 0; p < count; ++p) {
    uint32_t* d = dst + ((size_t)p * per + slot) * dl;
    memcpy(d, src + (size_t)p * sl, (size_t)sl * 4);
    if (dl > sl) memset(d + sl, 0, (size_t)(dl - sl) * 4);
  }
}

// the inverse for the comb's results: slot `slot` of src [per * count][l] into dst [count][l]
inline void take_rows(uint32_t* dst, const uint32_t* src, uint32_t l, uint32_t per, uint32_t slot, uint32_t count) {
  for (uint32_t p = 0; p < count; ++p) memcpy(dst + (size_t)p * l, src + ((size_t)p * per + slot) * l, (size_t)l * 4);
}

// key_idx of the comb's instances: every proof's row, `per` times
inline void repeat_keys(uint32_t* dst, const uint32_t* key_idx, uint32_t per, uint32_t count) {
  for (uint32_t p = 0; p < count; ++p)
    for (uint32_t s = 0; s < per; ++s) dst[(size_t)p * per + s] = key_idx[p];
}

}  // namespace fsdkr
