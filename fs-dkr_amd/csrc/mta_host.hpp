// Host helpers shared by the MtA entry points (mta.cpp, mta_alice.cpp,
// comb_ct_host.cpp): image layout, bit lengths, the split chains' descriptors and
// lane rules, and the wiping of what held secret values.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "collect.hpp"
#include "ctx.hpp"
#include "fsdkr/fsdkr.h"

namespace fsdkr {

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

inline uint32_t bit_len(const uint32_t* x, uint32_t limbs) {
  for (int k = (int)limbs - 1; k >= 0; --k)
    if (x[k]) return 32u * (uint32_t)k + 32u - (uint32_t)__builtin_clz(x[k]);
  return 0;
}

// zero a host staging copy of secret rows (not elided: volatile stores)
inline void wipe(std::vector<uint32_t>& v) {
  volatile uint32_t* p = v.data();
  for (size_t k = 0; k < v.size(); ++k) p[k] = 0u;
}

// zero a named context buffer on the context's stream (no-op if it was never made)
inline int scrub(Ctx* c, const std::string& name) {
  const auto it = c->bufs.find(name);
  if (it == c->bufs.end() || !it->second.ptr || !it->second.bytes) return FSDKR_OK;
  return c->hip_check(hipMemsetAsync(it->second.ptr, 0, it->second.bytes, c->stream), "scrub");
}

// the split of Bob's chain: s1 <= q^3 < 2^768 and e < 2^256 ride the tail
constexpr uint32_t kBobSplit = 768, kS1Limbs = 24, kELimbs = 8, kEBits = 256;
// elements per simultaneous inversion (one serial chain of ~3 products each per group)
constexpr uint32_t kInvChunk = 32;

// the tail's descriptor block of J's instances: rows of `base` (stride bl limbs)
// and `exp` (el limbs) by output row; the pads (row >= count) run exponent 0
inline void tail_desc(const ModexpJob& J, uint32_t count, uint64_t base, uint32_t bl, uint64_t exp, uint32_t el,
               std::vector<uint8_t>& d) {
  const size_t n = J.size();
  d.assign(n * kTailDescBytes, 0);
  auto* bp = reinterpret_cast<uint64_t*>(d.data());
  auto* ep = reinterpret_cast<uint64_t*>(d.data() + n * 8);
  auto* ln = reinterpret_cast<uint32_t*>(d.data() + n * 16);
  for (size_t k = 0; k < n; ++k) {
    const uint32_t r = J.out_idx[k];
    const uint32_t src = r < count ? r : 0u;
    bp[k] = base + (size_t)src * bl * 4;
    ep[k] = exp + (size_t)src * el * 4;
    ln[k] = r < count ? el : 0u;
  }
}

// instances in key order, cut into groups of at most kInvChunk of one key
inline void inverse_groups(const uint32_t* key, uint32_t reps, uint32_t count, uint32_t n_keys, std::vector<uint32_t>& order,
                    std::vector<uint32_t>& gstart) {
  std::vector<std::vector<uint32_t>> by(n_keys);
  for (uint32_t r = 0; r < reps; ++r)
    for (uint32_t p = 0; p < count; ++p) by[key[p]].push_back(r * count + p);
  order.clear();
  gstart.assign(1, 0u);
  for (const auto& v : by)
    for (size_t s = 0; s < v.size(); s += kInvChunk) {
      const size_t e = std::min(v.size(), s + kInvChunk);
      order.insert(order.end(), v.begin() + s, v.begin() + e);
      gstart.push_back((uint32_t)order.size());
    }
}

// Whole device stages that more than one entry point runs.  Each uploads its rows,
// runs, copies its (public) results to `out` on the host, scrubs what held a secret
// and synchronises; `who` names the entry in error messages.
// fsdkr_pedersen_commit_ct (comb_ct_host.cpp)
int pedersen_commit_ct_run(Ctx* c, const char* who, uint32_t nl, uint32_t count, const uint32_t* x, uint32_t xl,
                           const uint32_t* y, uint32_t yl, const uint32_t* key_idx, const uint32_t* Ntilde,
                           const uint32_t* h1, const uint32_t* h2, uint32_t n_keys, uint32_t* out);
// fsdkr_mta_respond (el = 8) and fsdkr_bob_commit_v (el = kBobVLimbs) (mta.cpp)
int mta_respond_impl(Ctx* c, const char* who, uint32_t nl, uint32_t count, const uint32_t* a_enc, const uint32_t* b,
                     const uint32_t* beta_prim, const uint32_t* r, const uint32_t* n_idx, const uint32_t* ns,
                     uint32_t nk, uint32_t* out, bool want_fused, uint32_t el = 8);

// lanes per chain of the split launch: a forced context setting (tests, tuning)
// where the tail has that shape, else by batch size; 192-limb moduli: 8 lanes
inline int split_group(Ctx* c, const char* who, uint32_t count, bool wide_ok, uint32_t k32, uint32_t* group) {
  const uint32_t f = c->modexp_group;
  if (c->ct) {
    c->fail("%s: public exponents only (constant-time context)", who);
    return FSDKR_E_ARG;
  }
  if (k32 == 192) {
    if (f != 0 && f != 8) {
      c->fail("%s: the 6144-bit split chains run at 8 lanes (forced %u)", who, f);
      return FSDKR_E_ARG;
    }
    *group = 8;
    return FSDKR_OK;
  }
  if (f == 0) *group = keyed_lanes(count);   // as the keyed 4096-bit launches pick their lanes
  else if (f == 4 || f == 8 || f == 16 || (wide_ok && f == kWideGroup)) *group = f;
  else {
    c->fail("%s: the split chains run at 4, 8, 16%s lanes (forced %u)", who, wide_ok ? " or 32" : "", f);
    return FSDKR_E_ARG;
  }
  return FSDKR_OK;
}

}  // namespace fsdkr
