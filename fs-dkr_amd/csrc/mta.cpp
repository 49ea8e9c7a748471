// Bob's MtA range proofs of the C ABI (include/fsdkr/fsdkr.h):
//   fsdkr_modexp_joint3_batch   parity entry of the three-base tail (modexp.hip modexp_tail_kernel J3)
//   fsdkr_modexp_joint3_batch_k the same at a modulus width of 128 or 192 limbs
//   fsdkr_bob_verify            BobProof::verify (range_proofs.rs:360-446) and
//                               BobProofExt::verify (:527-562), `count` proofs in one pass
//   fsdkr_bob_verify_unfused    the same verdicts with three separate mod-N^2 chains (A/B)
//   fsdkr_mta_respond           Bob's response a_enc^b (1 + beta' N) r^N mod N^2 (:688-704), see below
//   fsdkr_mta_respond_unfused   the same values from separate chains and one product (A/B)
//   fsdkr_bob_commit_v          the prover's v = a_enc^alpha (1 + gamma N) beta^N mod N^2 (:283-288)
//   fsdkr_bob_commit_v_unfused  the same values from separate chains and one product (A/B)
// Per proof, in the reference's order: s1 <= q^3 (:374); z^e, mta^e, t^e units
// (:378-406); z' = h1^s1 h2^s2 z^-e, w = h1^t1 h2^t2 t^-e mod N~ (:385-388, :408-411);
// v = a_enc^s1 s^N (1 + t1 N) mta^-e mod N^2 (:396-400); the transcript hash
// (:413-441); with X / u the curve equation G s1 == X e + u (:550-559).
// The pieces: fixed-base combs for the four h1 / h2 powers (bases shared per key),
// a 256-bit modexp job for z^e | t^e, Montgomery's simultaneous inversion, and for
// s^N a_enc^s1 (mta^-1)^e ONE split chain of bits(N) squarings: the head over N's
// bits >= 768, the tail with a_enc (4-bit windows of s1 < 2^768) and mta^-1
// (windows of e < 2^256) riding its squarings.  Two width classes, one per batch:
// nl = 64 (keys up to 2048 bits, N^2 of 128 limbs, 4 / 8 / 16 lanes per chain) and
// nl = 96 (up to 3072 bits, N^2 of 192 limbs, the 8-lane split chain).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "collect.hpp"
#include "ctx.hpp"
#include "fbjob.hpp"
#include "fsdkr/fsdkr.h"
#include "hostbn.hpp"
#include "kernels.h"
#include "mta_host.hpp"
#include "verify.h"

using namespace fsdkr;

extern "C" {

int fsdkr_modexp_joint3_batch_k(fsdkr_ctx* ctx, uint32_t k32, uint32_t count, const uint32_t* base,
                                const uint32_t* base2, const uint32_t* exp2, uint32_t exp2_limbs, const uint32_t* base3,
                                const uint32_t* exp3, const uint32_t* mod_idx, const uint32_t* mods,
                                const uint32_t* mod_exp, uint32_t exp_limbs, uint32_t n_mod, uint32_t* out) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return FSDKR_E_ARG;
  const char* who = "fsdkr_modexp_joint3_batch";
  if (k32 != 128 && k32 != 192) {
    c->fail("%s: unsupported modulus width %u limbs", who, k32);
    return FSDKR_E_UNSUPPORTED;
  }
  if (count == 0) return FSDKR_OK;
  const uint32_t K = k32;
  if (!base || !base2 || !exp2 || !mod_idx || !mods || !mod_exp || !out || !n_mod || !exp_limbs || !exp2_limbs ||
      exp2_limbs > kS1Limbs || (base3 == nullptr) != (exp3 == nullptr)) {
    c->fail("%s: bad argument", who);
    return FSDKR_E_ARG;
  }
  uint32_t ebits = 1;
  for (uint32_t m = 0; m < n_mod; ++m) {
    if ((mods[(size_t)m * K] & 1u) == 0) {
      c->fail("%s: modulus %u is even", who, m);
      return FSDKR_E_ARG;
    }
    ebits = std::max(ebits, bit_len(mod_exp + (size_t)m * exp_limbs, exp_limbs));
  }
  for (uint32_t i = 0; i < count; ++i)
    if (mod_idx[i] >= n_mod) {
      c->fail("%s: mod_idx[%u] out of range", who, i);
      return FSDKR_E_ARG;
    }
  uint32_t group = 16;
  int rc;
  if ((rc = split_group(c, who, count, true, K, &group))) return rc;
  const uint32_t per_wave = 64 / group;
  const size_t cap = (size_t)count + (size_t)n_mod * per_wave;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = al256(off + (bytes ? bytes : 1)); return o; };
  const size_t o_b = take((size_t)count * K * 4), o_b2 = take((size_t)count * K * 4),
               o_e2 = take((size_t)count * exp2_limbs * 4), o_b3 = take((size_t)count * K * 4),
               o_e3 = take((size_t)count * kELimbs * 4), o_m = take((size_t)n_mod * K * 4),
               o_me = take((size_t)n_mod * exp_limbs * 4), o_out = take(((size_t)count + 1) * K * 4),
               o_desc = take(cap * 36), o_d2 = take(cap * kTailDescBytes), o_d3 = take(cap * kTailDescBytes);
  uint8_t* dev = (uint8_t*)c->buf("mxj3", off);
  if (!dev) {
    c->fail("%s: device allocation failed", who);
    return FSDKR_E_OOM;
  }
  auto DI = [&](size_t o) { return (uint64_t)(uintptr_t)(dev + o); };
  ModexpJob J;
  J.k32 = K;
  for (uint32_t i = 0; i < count; ++i)
    J.add(DI(o_b + (size_t)i * K * 4), K, DI(o_me + (size_t)mod_idx[i] * exp_limbs * 4), exp_limbs, ebits, mod_idx[i]);
  if (!group_by_exponent(J, per_wave, count)) {
    c->fail("%s: instances not wave-uniform", who);
    return FSDKR_E_ARG;
  }
  std::vector<uint8_t> desc, d2, d3;
  J.pack(desc);
  tail_desc(J, count, DI(o_b2), K, DI(o_e2), exp2_limbs, d2);
  if (base3) tail_desc(J, count, DI(o_b3), K, DI(o_e3), kELimbs, d3);
  auto up = [&](size_t o, const void* src, size_t bytes) {
    return c->hip_check(hipMemcpyAsync(dev + o, src, bytes, hipMemcpyHostToDevice, c->stream), "H2D joint3");
  };
  if ((rc = up(o_b, base, (size_t)count * K * 4)) || (rc = up(o_b2, base2, (size_t)count * K * 4)) ||
      (rc = up(o_e2, exp2, (size_t)count * exp2_limbs * 4)) || (rc = up(o_m, mods, (size_t)n_mod * K * 4)) ||
      (rc = up(o_me, mod_exp, (size_t)n_mod * exp_limbs * 4)) || (rc = up(o_desc, desc.data(), desc.size())) ||
      (rc = up(o_d2, d2.data(), d2.size())))
    return rc;
  if (base3 && ((rc = up(o_b3, base3, (size_t)count * K * 4)) || (rc = up(o_e3, exp3, (size_t)count * kELimbs * 4)) ||
                (rc = up(o_d3, d3.data(), d3.size()))))
    return rc;
  uint32_t* cons = nullptr;
  if ((rc = setup_moduli(c, K, reinterpret_cast<const uint32_t*>(dev + o_m), n_mod, &cons,
                         group == kWideGroup ? "joint3_w" : "joint3", group == kWideGroup ? kWideGroup : 0u)))
    return rc;
  const uint32_t flags = ga_desc_flags(true, group);
  SplitArgs head;
  head.lo_bit = kBobSplit;
  SplitArgs tail = head;
  tail.tail = true;
  tail.d_desc2 = dev + o_d2;
  if (base3) {
    tail.d_desc3 = dev + o_d3;
    tail.exp3_bits = kEBits;
  }
  const size_t n = J.size();
  uint32_t* d_out = reinterpret_cast<uint32_t*>(dev + o_out);
  if ((rc = launch_modexp_desc(c, K, (uint32_t)n, ebits, dev + o_desc, cons, d_out, c->stream, "mxt_joint3", 0, group,
                               flags, &head)) ||
      (rc = launch_modexp_desc(c, K, (uint32_t)n, ebits, dev + o_desc, cons, d_out, c->stream, "mxt_joint3", 0, group,
                               flags, &tail)))
    return rc;
  if ((rc = c->hip_check(hipMemcpyAsync(out, d_out, (size_t)count * K * 4, hipMemcpyDeviceToHost, c->stream), "D2H")))
    return rc;
  return c->sync();
}

int fsdkr_modexp_joint3_batch(fsdkr_ctx* ctx, uint32_t count, const uint32_t* base, const uint32_t* base2,
                              const uint32_t* exp2, uint32_t exp2_limbs, const uint32_t* base3, const uint32_t* exp3,
                              const uint32_t* mod_idx, const uint32_t* mods, const uint32_t* mod_exp,
                              uint32_t exp_limbs, uint32_t n_mod, uint32_t* out) {
  return fsdkr_modexp_joint3_batch_k(ctx, 128, count, base, base2, exp2, exp2_limbs, base3, exp3, mod_idx, mods, mod_exp,
                                     exp_limbs, n_mod, out);
}

static int bob_verify_impl(Ctx* c, const char* who, const fsdkr_bob_batch* b, uint8_t* verdict, bool fused) {
  if (!b) {
    c->fail("%s: null batch", who);
    return FSDKR_E_ARG;
  }
  const uint32_t count = b->count, nk = b->n_keys, nl = b->nl, nn = 2 * b->nl;
  if (count == 0) return FSDKR_OK;
  if (!verdict || !nk || !b->N || !b->Ntilde || !b->h1 || !b->h2 || !b->key_idx || !b->a_enc || !b->mta || !b->z ||
      !b->t || !b->s || !b->e || !b->s1 || !b->s2 || !b->t1 || !b->t2 || (b->X == nullptr) != (b->u == nullptr) ||
      !b->el || !b->s1l || !b->s2l || !b->t1l || !b->t2l || b->el > 64 || b->s1l > 64) {
    c->fail("%s: bad argument", who);
    return FSDKR_E_ARG;
  }
  if (nl != 64 && nl != 96) {
    c->fail("%s: unsupported modulus width %u limbs", who, nl);
    return FSDKR_E_UNSUPPORTED;
  }
  // digits per row of the inversion scratch: the kernels' shapes of both widths
  const size_t kdl = (size_t)shape_digits(nl), kdn = (size_t)shape_digits(nn);
  const bool ext = b->X != nullptr;
  for (uint32_t k = 0; k < nk; ++k) {
    const uint32_t *N = b->N + (size_t)k * nl, *Nt = b->Ntilde + (size_t)k * nl;
    if (!(N[0] & 1u) || !(Nt[0] & 1u) || bit_len(N, nl) < 2 || bit_len(Nt, nl) < 2) {
      c->fail("%s: key %u: N and Ntilde must be odd and above 1", who, k);
      return FSDKR_E_ARG;
    }
  }
  for (uint32_t p = 0; p < count; ++p)
    if (b->key_idx[p] >= nk) {
      c->fail("%s: key_idx[%u] out of range", who, p);
      return FSDKR_E_ARG;
    }
  uint32_t group = 16;
  int rc;
  if ((rc = split_group(c, who, count, false, nn, &group))) return rc;
  const uint32_t* key = b->key_idx;

  // ---- host pre-pass -------------------------------------------------------
  static const uint32_t kQ[8] = {0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u,
                                 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  const hbn::Limbs q = hbn::from(kQ, 8), q3 = hbn::mul(hbn::mul(q, q), q);
  std::vector<uint8_t> pre(count, 1), inf(count, 0);
  std::vector<uint32_t> s1a((size_t)count * kS1Limbs, 0u), ea((size_t)count * kELimbs, 0u);
  for (uint32_t p = 0; p < count; ++p) {
    const uint32_t* s1 = b->s1 + (size_t)p * b->s1l;
    if (hbn::cmp_raw(s1, b->s1l, q3.data(), q3.size()) > 0) pre[p] = 0;   // :374 (s1 == q^3 passes)
    else memcpy(&s1a[(size_t)p * kS1Limbs], s1, std::min(b->s1l, kS1Limbs) * 4);
    const uint32_t* e = b->e + (size_t)p * b->el;
    bool wide = false;
    for (uint32_t k = kELimbs; k < b->el; ++k) wide = wide || e[k] != 0;
    if (!wide) memcpy(&ea[(size_t)p * kELimbs], e, std::min(b->el, kELimbs) * 4);
    // a challenge of 256 bits or more never equals the hash; e = 0 only if the hash is 0
    if (wide || hbn::is_zero_raw(&ea[(size_t)p * kELimbs], kELimbs)) pre[p] = 0;
    if (ext) inf[p] = hbn::is_zero_raw(b->X + (size_t)p * 16, 16) || hbn::is_zero_raw(b->u + (size_t)p * 16, 16);
  }
  std::vector<uint32_t> NN((size_t)nk * nn), h1r((size_t)nk * nl), h2r((size_t)nk * nl);
  uint32_t nbits = 1;
  for (uint32_t k = 0; k < nk; ++k) {
    const hbn::Limbs N = hbn::from(b->N + (size_t)k * nl, nl), Nt = hbn::from(b->Ntilde + (size_t)k * nl, nl);
    hbn::store(hbn::mul(N, N), &NN[(size_t)k * nn], nn);
    hbn::store(hbn::mod(hbn::from(b->h1 + (size_t)k * nl, nl), Nt), &h1r[(size_t)k * nl], nl);
    hbn::store(hbn::mod(hbn::from(b->h2 + (size_t)k * nl, nl), Nt), &h2r[(size_t)k * nl], nl);
    nbits = std::max(nbits, bit_len(b->N + (size_t)k * nl, nl));
  }
  // rows at or above their modulus are reduced for the arithmetic (a copy, made only then)
  auto reduced = [&](const uint32_t* src, uint32_t L, const uint32_t* mods, uint32_t ML,
                     std::vector<uint32_t>& store) -> const uint32_t* {
    for (uint32_t p = 0; p < count; ++p) {
      const uint32_t* m = mods + (size_t)key[p] * ML;
      if (hbn::cmp_raw(src + (size_t)p * L, L, m, ML) < 0) continue;
      if (store.empty()) store.assign(src, src + (size_t)count * L);
      hbn::store(hbn::mod(hbn::from(src + (size_t)p * L, L), hbn::from(m, ML)), &store[(size_t)p * L], L);
    }
    return store.empty() ? src : store.data();
  };
  std::vector<uint32_t> v_a, v_m, v_z, v_t, v_s;
  const uint32_t* a_red = reduced(b->a_enc, nn, NN.data(), nn, v_a);
  const uint32_t* m_red = reduced(b->mta, nn, NN.data(), nn, v_m);
  const uint32_t* z_red = reduced(b->z, nl, b->Ntilde, nl, v_z);
  const uint32_t* t_red = reduced(b->t, nl, b->Ntilde, nl, v_t);
  const uint32_t* s_red = reduced(b->s, nl, NN.data(), nn, v_s);
  // 1 + t1 N = 1 + (t1 mod N) N  (mod N^2): the honest t1 = e beta' + gamma is wider than N
  std::vector<uint32_t> t1r((size_t)count * nl, 0u);
  for (uint32_t p = 0; p < count; ++p) {
    const uint32_t* t1 = b->t1 + (size_t)p * b->t1l;
    const uint32_t* N = b->N + (size_t)key[p] * nl;
    if (hbn::cmp_raw(t1, b->t1l, N, nl) < 0) memcpy(&t1r[(size_t)p * nl], t1, std::min(b->t1l, nl) * 4);
    else hbn::store(hbn::mod(hbn::from(t1, b->t1l), hbn::from(N, nl)), &t1r[(size_t)p * nl], nl);
  }
  uint32_t s1bits = 1, s2bits = 1, t1bits = 1, t2bits = 1;
  for (uint32_t p = 0; p < count; ++p) {
    s1bits = std::max(s1bits, bit_len(&s1a[(size_t)p * kS1Limbs], kS1Limbs));
    s2bits = std::max(s2bits, bit_len(b->s2 + (size_t)p * b->s2l, b->s2l));
    t1bits = std::max(t1bits, bit_len(b->t1 + (size_t)p * b->t1l, b->t1l));
    t2bits = std::max(t2bits, bit_len(b->t2 + (size_t)p * b->t2l, b->t2l));
  }

  // ---- device image --------------------------------------------------------
  const size_t C = count, rl = (size_t)nl * 4, rn = (size_t)nn * 4;
  const uint32_t per_wave = 64 / group;
  const size_t cap = C + (size_t)nk * per_wave;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = al256(off + (bytes ? bytes : 1)); return o; };
  const size_t o_N = take(nk * rl), o_Nt = take(nk * rl), o_NN = take(nk * rn), o_h1 = take(nk * rl), o_h2 = take(nk * rl);
  const size_t o_a = take(C * rn), o_m = take(C * rn), o_z = take(C * rl), o_t = take(C * rl), o_s = take(C * rl);
  const size_t o_ar = v_a.empty() ? o_a : take(C * rn), o_mr = v_m.empty() ? o_m : take(C * rn);
  const size_t o_zt = take(2 * C * rl);   // z | t reduced (the z^e | t^e bases)
  const size_t o_e = take(C * b->el * 4), o_ea = take(C * kELimbs * 4), o_s1 = take(C * kS1Limbs * 4);
  const size_t o_s1raw = take(C * b->s1l * 4), o_s2 = take(C * b->s2l * 4), o_t1 = take(C * b->t1l * 4);
  const size_t o_t1r = take(C * rl), o_t2 = take(C * b->t2l * 4), o_X = take(ext ? C * 64 : 0), o_u = take(ext ? C * 64 : 0);
  const size_t o_one = take(rn), o_pre = take(C), o_ec = take(C);
  // descriptors
  const size_t o_gdesc = take(cap * 36), o_gd2 = take(cap * kTailDescBytes), o_gd3 = take(cap * kTailDescBytes);
  const size_t o_zdesc = take(2 * C * 32), o_udesc = take(fused ? 0 : 2 * C * 32 + 512);
  const size_t o_iy = take(3 * C * 8), o_im = take(3 * C * 8), o_iord = take(3 * C * 4), o_igs = take((3 * C + 2 * nk + 2) * 4);
  const size_t o_bs = take(C * 8), o_bn = take(C * 8);
  const size_t o_p3 = take(3 * C * sizeof(Prod3Operand)), o_p3m = take(3 * C * 4), o_hn = take(C * 8);
  // results
  const size_t o_minv = take(C * rn), o_um = take(C * 4), o_zte = take(2 * C * rl), o_ztinv = take(2 * C * rl);
  const size_t o_uzt = take(2 * C * 4), o_fb = take(4 * C * rl), o_binom = take(C * rn), o_ga = take((C + 1) * rn);
  const size_t o_un = take(fused ? 0 : 3 * C * rn);   // unfused: a_enc^s1 | mta^e | (mta^e)^-1
  const size_t o_v0 = take(fused ? 0 : C * rn), o_p3u = take(fused ? 0 : C * sizeof(Prod3Operand));
  const size_t o_zw = take(2 * C * rl), o_v = take(C * rn);
  const size_t o_iscr = take(C * (kdn + 2 * kdl) * 4);
  uint8_t* dev = (uint8_t*)c->buf("bob_io", off);
  if (!dev) {
    c->fail("%s: device allocation failed (%zu bytes)", who, off);
    return FSDKR_E_OOM;
  }
  auto DA = [&](size_t o) { return (uint64_t)(uintptr_t)(dev + o); };
  auto PU = [&](size_t o) { return reinterpret_cast<uint32_t*>(dev + o); };
  hipStream_t st = c->stream;
  auto up = [&](size_t o, const void* src, size_t bytes) {
    return bytes ? c->hip_check(hipMemcpyAsync(dev + o, src, bytes, hipMemcpyHostToDevice, st), "H2D bob") : (int)FSDKR_OK;
  };
  std::vector<uint32_t> one(nn, 0u);
  one[0] = 1;

  // GA: s^N mod N^2, regrouped so every wave shares its exponent N
  ModexpJob J;
  J.k32 = nn;
  for (uint32_t p = 0; p < count; ++p)
    J.add(DA(o_s + p * rl), nl, DA(o_N + key[p] * rl), nl, bit_len(b->N + (size_t)key[p] * nl, nl), key[p]);
  if (!group_by_exponent(J, per_wave, count)) {
    c->fail("%s: instances not wave-uniform", who);
    return FSDKR_E_ARG;
  }
  std::vector<uint8_t> gdesc, gd2, gd3;
  J.pack(gdesc);
  if (fused) {
    tail_desc(J, count, DA(o_ar), nn, DA(o_s1), kS1Limbs, gd2);
    tail_desc(J, count, DA(o_minv), nn, DA(o_ea), kELimbs, gd3);
  }
  // z^e | t^e mod N~
  ModexpJob Jz;
  Jz.k32 = nl;
  for (uint32_t i = 0; i < 2 * count; ++i)
    Jz.add(DA(o_zt + i * rl), nl, DA(o_ea + (size_t)(i % count) * kELimbs * 4), kELimbs, kEBits, key[i % count]);
  std::vector<uint8_t> zdesc;
  Jz.pack(zdesc);
  // unfused: a_enc^s1 | mta^e mod N^2 as chains of their own
  ModexpJob Ju, Jm;
  std::vector<uint8_t> udesc;
  if (!fused) {
    Ju.k32 = Jm.k32 = nn;
    for (uint32_t p = 0; p < count; ++p) {
      Ju.add(DA(o_ar + p * rn), nn, DA(o_s1 + (size_t)p * kS1Limbs * 4), kS1Limbs, std::max(s1bits, 1u), key[p]);
      Jm.add(DA(o_mr + p * rn), nn, DA(o_ea + (size_t)p * kELimbs * 4), kELimbs, kEBits, key[p]);
    }
    Ju.pack(udesc);
    udesc.resize(al256(udesc.size()));
    Jm.pack(udesc);
  }
  // inverses: mta (fused; unfused mta^e) mod N^2, then z^e | t^e mod N~
  std::vector<uint64_t> iy(3 * C), im(3 * C);
  std::vector<uint32_t> ord_nn, gs_nn, ord_nl, gs_nl;
  inverse_groups(key, 1, count, nk, ord_nn, gs_nn);
  inverse_groups(key, 2, count, nk, ord_nl, gs_nl);
  for (uint32_t p = 0; p < count; ++p) {
    iy[p] = fused ? DA(o_mr + p * rn) : DA(o_un + (C + p) * rn);
    im[p] = DA(o_NN + key[p] * rn);
  }
  for (uint32_t i = 0; i < 2 * count; ++i) {
    iy[C + i] = DA(o_zte + i * rl);
    im[C + i] = DA(o_Nt + key[i % count] * rl);
  }
  std::vector<uint32_t> iord(ord_nn);
  iord.insert(iord.end(), ord_nl.begin(), ord_nl.end());
  std::vector<uint32_t> igs(gs_nn);
  const size_t igs_nl = igs.size();
  igs.insert(igs.end(), gs_nl.begin(), gs_nl.end());
  // fixed-base job: h1^s1 | h2^s2 | h1^t1 | h2^t2, bases [h1_k | h2_k]
  FbJob fb;
  fb.k32 = nl;
  for (uint32_t k = 0; k < nk; ++k) fb.add_base(DA(o_h1 + k * rl), nl, k);
  for (uint32_t k = 0; k < nk; ++k) fb.add_base(DA(o_h2 + k * rl), nl, k);
  const uint32_t h1bits = std::max(s1bits, t1bits), h2bits = std::max(s2bits, t2bits);
  for (uint32_t p = 0; p < count; ++p) {
    fb.add(key[p], DA(o_s1 + (size_t)p * kS1Limbs * 4), kS1Limbs, h1bits, DA(o_fb + (0 * C + p) * rl));
    fb.add(key[p], DA(o_t1 + (size_t)p * b->t1l * 4), b->t1l, h1bits, DA(o_fb + (2 * C + p) * rl));
  }
  for (uint32_t p = 0; p < count; ++p) {
    fb.add(nk + key[p], DA(o_s2 + (size_t)p * b->s2l * 4), b->s2l, h2bits, DA(o_fb + (1 * C + p) * rl));
    fb.add(nk + key[p], DA(o_t2 + (size_t)p * b->t2l * 4), b->t2l, h2bits, DA(o_fb + (3 * C + p) * rl));
  }
  fb.finalize();
  // binom, products, hash
  std::vector<uint64_t> bs(C), bn(C), hn(C);
  std::vector<Prod3Operand> p3(3 * C);
  std::vector<uint32_t> p3m(3 * C);
  for (uint32_t p = 0; p < count; ++p) {
    bs[p] = DA(o_t1r + p * rl);
    bn[p] = hn[p] = DA(o_N + key[p] * rl);
    // z' = h1^s1 h2^s2 (z^e)^-1, w = h1^t1 h2^t2 (t^e)^-1 mod N~
    p3[p] = Prod3Operand{DA(o_fb + (0 * C + p) * rl), DA(o_fb + (1 * C + p) * rl), DA(o_ztinv + p * rl), nl, nl, nl, 0};
    p3[C + p] = Prod3Operand{DA(o_fb + (2 * C + p) * rl), DA(o_fb + (3 * C + p) * rl), DA(o_ztinv + (C + p) * rl),
                             nl, nl, nl, 0};
    // v = (chain) (1 + t1 N) mod N^2
    p3[2 * C + p] = Prod3Operand{fused ? DA(o_ga + p * rn) : DA(o_v0 + p * rn), DA(o_binom + p * rn), DA(o_one), nn, nn, nn, 0};
    p3m[p] = p3m[C + p] = p3m[2 * C + p] = key[p];
  }
  std::vector<Prod3Operand> p3u;   // unfused: s^N a_enc^s1 (mta^e)^-1
  if (!fused) {
    p3u.resize(C);
    for (uint32_t p = 0; p < count; ++p)
      p3u[p] = Prod3Operand{DA(o_ga + p * rn), DA(o_un + p * rn), DA(o_un + (2 * C + p) * rn), nn, nn, nn, 0};
  }
  std::vector<uint32_t> zt((size_t)2 * count * nl);
  memcpy(zt.data(), z_red, C * rl);
  memcpy(zt.data() + (size_t)count * nl, t_red, C * rl);

  if ((rc = up(o_N, b->N, nk * rl)) || (rc = up(o_Nt, b->Ntilde, nk * rl)) || (rc = up(o_NN, NN.data(), nk * rn)) ||
      (rc = up(o_h1, h1r.data(), nk * rl)) || (rc = up(o_h2, h2r.data(), nk * rl)) || (rc = up(o_a, b->a_enc, C * rn)) ||
      (rc = up(o_m, b->mta, C * rn)) || (rc = up(o_z, b->z, C * rl)) || (rc = up(o_t, b->t, C * rl)) ||
      (rc = up(o_s, s_red, C * rl)) || (!v_a.empty() && (rc = up(o_ar, a_red, C * rn))) ||
      (!v_m.empty() && (rc = up(o_mr, m_red, C * rn))) || (rc = up(o_zt, zt.data(), 2 * C * rl)) ||
      (rc = up(o_e, b->e, C * b->el * 4)) || (rc = up(o_ea, ea.data(), C * kELimbs * 4)) ||
      (rc = up(o_s1, s1a.data(), C * kS1Limbs * 4)) || (rc = up(o_s1raw, b->s1, C * b->s1l * 4)) ||
      (rc = up(o_s2, b->s2, C * b->s2l * 4)) || (rc = up(o_t1, b->t1, C * b->t1l * 4)) ||
      (rc = up(o_t1r, t1r.data(), C * rl)) || (rc = up(o_t2, b->t2, C * b->t2l * 4)) ||
      (ext && ((rc = up(o_X, b->X, C * 64)) || (rc = up(o_u, b->u, C * 64)))) || (rc = up(o_one, one.data(), rn)) ||
      (rc = up(o_pre, pre.data(), C)) || (rc = up(o_gdesc, gdesc.data(), gdesc.size())) ||
      (fused && ((rc = up(o_gd2, gd2.data(), gd2.size())) || (rc = up(o_gd3, gd3.data(), gd3.size())))) ||
      (rc = up(o_zdesc, zdesc.data(), zdesc.size())) || (!fused && (rc = up(o_udesc, udesc.data(), udesc.size()))) ||
      (rc = up(o_iy, iy.data(), iy.size() * 8)) || (rc = up(o_im, im.data(), im.size() * 8)) ||
      (rc = up(o_iord, iord.data(), iord.size() * 4)) || (rc = up(o_igs, igs.data(), igs.size() * 4)) ||
      (rc = up(o_bs, bs.data(), C * 8)) || (rc = up(o_bn, bn.data(), C * 8)) || (rc = up(o_hn, hn.data(), C * 8)) ||
      (rc = up(o_p3, p3.data(), p3.size() * sizeof(Prod3Operand))) || (rc = up(o_p3m, p3m.data(), p3m.size() * 4)) ||
      (!fused && (rc = up(o_p3u, p3u.data(), p3u.size() * sizeof(Prod3Operand)))))
    return rc;
  if (ext && (rc = c->hip_check(hipMemsetAsync(dev + o_ec, 0, C, st), "memset ec"))) return rc;

  // ---- kernels -------------------------------------------------------------
  uint32_t *cons_nl = nullptr, *cons_nn = nullptr;
  if ((rc = setup_moduli(c, nl, PU(o_Nt), nk, &cons_nl, "bob_nl")) || (rc = setup_moduli(c, nn, PU(o_NN), nk, &cons_nn, "bob_nn")))
    return rc;
  uint32_t* iscr = PU(o_iscr);   // [C][kdn] for the N^2 inverse, then [2C][kdl] for the N~ ones
  hipEvent_t ready = nullptr, side_done = nullptr;
  auto drop = [&](int r) {
    if (ready) (void)hipEventDestroy(ready);
    if (side_done) (void)hipEventDestroy(side_done);
    ready = side_done = nullptr;
    return r;
  };
  if ((rc = c->hip_check(hipEventCreateWithFlags(&ready, hipEventDisableTiming), "event")) ||
      (rc = c->hip_check(hipEventCreateWithFlags(&side_done, hipEventDisableTiming), "event")) ||
      (rc = c->hip_check(hipEventRecord(ready, st), "event record")))   // uploads and constants are in
    return drop(rc);
  auto inverse_nn = [&](uint32_t* out, uint32_t* unit) {
    BatchInverseArgs a{(const uint64_t*)(dev + o_iy), (const uint64_t*)(dev + o_im), PU(o_iord), PU(o_igs), out, unit,
                       iscr, (uint32_t)gs_nn.size() - 1};
    c->mark("inverse", true);
    const int r = c->hip_check(launch_inverse_batch(nn, a, st), "inverse nn");
    c->mark("inverse", false);
    return r;
  };
  const uint32_t flags = ga_desc_flags(true, group);
  const uint32_t gn = (uint32_t)J.size();
  SplitArgs head;
  head.lo_bit = kBobSplit;
  if (fused) {
    // mta^-1 (and mta's unit flag), then s^N a_enc^s1 (mta^-1)^e in one chain
    if ((rc = inverse_nn(PU(o_minv), PU(o_um)))) return drop(rc);
    SplitArgs tail = head;
    tail.tail = true;
    tail.d_desc2 = dev + o_gd2;
    tail.d_desc3 = dev + o_gd3;
    tail.exp3_bits = kEBits;
    if ((rc = launch_modexp_desc(c, nn, gn, nbits, dev + o_gdesc, cons_nn, PU(o_ga), st, "mxt_bob", 0, group, flags, &head)) ||
        (rc = launch_modexp_desc(c, nn, gn, nbits, dev + o_gdesc, cons_nn, PU(o_ga), st, "mxt_bob", 0, group, flags, &tail)))
      return drop(rc);
  } else {
    // s^N (keyed sliding windows; at 192 limbs the general kernel's fixed windows, as the
    // other two), a_enc^s1, mta^e and its inverse, then their product
    if ((rc = launch_modexp_desc(c, nn, gn, nbits, dev + o_gdesc, cons_nn, PU(o_ga), st, "mxt_bob", 0, group, flags)) ||
        (rc = launch_modexp_desc(c, nn, count, Ju.exp_bits, dev + o_udesc, cons_nn, PU(o_un), st, "mxt_bob_u")) ||
        (rc = launch_modexp_desc(c, nn, count, kEBits, dev + o_udesc + al256(Ju.desc_bytes()), cons_nn,
                                 PU(o_un) + C * nn, st, "mxt_bob_m")) ||
        (rc = inverse_nn(PU(o_un) + 2 * C * nn, PU(o_um))))
      return drop(rc);
    Prod3Args pu{(const Prod3Operand*)(dev + o_p3u), PU(o_p3m), cons_nn, PU(o_v0), count};
    if ((rc = c->hip_check(launch_prod3(nn, pu, st), "prod3 nn"))) return drop(rc);
  }
  // the N~ side -- z^e | t^e, their inverses, the fixed-base job -- on a side stream
  // beside the N^2 chains enqueued above (at 16 lanes they leave SIMD slots free)
  {
    hipStream_t ss = c->side_stream(1);
    (void)hipStreamWaitEvent(ss, ready, 0);
    StreamScope scope(c, ss);
    if ((rc = launch_modexp_desc(c, nl, 2 * count, kEBits, dev + o_zdesc, cons_nl, PU(o_zte), ss, "mxt_bob_z")))
      return drop(rc);
    BatchInverseArgs a{(const uint64_t*)(dev + o_iy) + C, (const uint64_t*)(dev + o_im) + C, PU(o_iord) + C,
                       PU(o_igs) + igs_nl, PU(o_ztinv), PU(o_uzt), iscr + C * kdn, (uint32_t)gs_nl.size() - 1};
    c->mark("inverse", true);
    rc = c->hip_check(launch_inverse_batch(nl, a, ss), "inverse nl");
    c->mark("inverse", false);
    if (rc || (rc = fb_run(c, fb, cons_nl, "bob")) ||
        (rc = c->hip_check(hipEventRecord(side_done, ss), "event record")))
      return drop(rc);
  }
  (void)hipStreamWaitEvent(st, side_done, 0);
  drop(0);
  {
    BinomArgs a{(const uint64_t*)(dev + o_bs), (const uint64_t*)(dev + o_bn), nl, nl, nn, PU(o_binom), count};
    if ((rc = c->hip_check(launch_binom(a, st), "binom"))) return rc;
    Prod3Args pa{(const Prod3Operand*)(dev + o_p3), PU(o_p3m), cons_nl, PU(o_zw), 2 * count};
    if ((rc = c->hip_check(launch_prod3(nl, pa, st), "prod3 nl"))) return rc;
    Prod3Args pb{(const Prod3Operand*)(dev + o_p3) + 2 * C, PU(o_p3m) + 2 * C, cons_nn, PU(o_v), count};
    if ((rc = c->hip_check(launch_prod3(nn, pb, st), "prod3 nn"))) return rc;
  }
  {
    BobHashArgs h{(const uint64_t*)(dev + o_hn), PU(o_a), PU(o_m), PU(o_z), PU(o_t), PU(o_zw), PU(o_zw) + C * nl,
                  PU(o_v), PU(o_e), ext ? PU(o_X) : nullptr, ext ? PU(o_u) : nullptr, nl, nn, nl, b->el,
                  dev + o_pre, count};
    c->mark("bob_hash", true);
    rc = c->hip_check(launch_bob_hash(h, st), "bob_hash");
    c->mark("bob_hash", false);
    if (rc) return rc;
  }
  if (ext) {   // G s1 == X e + u  (:550-559)
    PdlU1Args u{PU(o_s1raw), PU(o_ea), PU(o_X), PU(o_u), b->s1l, dev + o_ec, count};
    c->mark("ec", true);
    rc = c->hip_check(launch_pdl_u1(u, st), "pdl_u1");
    c->mark("ec", false);
    if (rc) return rc;
  }
  std::vector<uint8_t> hv(count), ec(count, 1);
  std::vector<uint32_t> um(count), uzt(2 * C);
  if ((rc = c->hip_check(hipMemcpyAsync(hv.data(), dev + o_pre, C, hipMemcpyDeviceToHost, st), "D2H bob")) ||
      (rc = c->hip_check(hipMemcpyAsync(um.data(), dev + o_um, C * 4, hipMemcpyDeviceToHost, st), "D2H bob")) ||
      (rc = c->hip_check(hipMemcpyAsync(uzt.data(), dev + o_uzt, 2 * C * 4, hipMemcpyDeviceToHost, st), "D2H bob")) ||
      (ext && (rc = c->hip_check(hipMemcpyAsync(ec.data(), dev + o_ec, C, hipMemcpyDeviceToHost, st), "D2H bob"))))
    return rc;
  if ((rc = c->sync())) return rc;
  for (uint32_t p = 0; p < count; ++p) {
    // s1 bound, then the three inverses (:374-406); only then the coordinates' unwrap (:428-431)
    const bool gate = pre[p] && uzt[p] && um[p] && uzt[C + p];
    verdict[p] = !gate ? 0 : inf[p] ? 2 : (hv[p] && (ec[p] & 1u)) ? 1 : 0;
  }
  return FSDKR_OK;
}

int fsdkr_bob_verify(fsdkr_ctx* ctx, const fsdkr_bob_batch* batch, uint8_t* verdict) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return FSDKR_E_ARG;
  return bob_verify_impl(c, "fsdkr_bob_verify", batch, verdict, true);
}

int fsdkr_bob_verify_unfused(fsdkr_ctx* ctx, const fsdkr_bob_batch* batch, uint8_t* verdict) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return FSDKR_E_ARG;
  return bob_verify_impl(c, "fsdkr_bob_verify_unfused", batch, verdict, false);
}

}  // extern "C"

// ---- Bob's MtA response --------------------------------------------------------
// mta_out = Paillier::add(Paillier::mul(ek, a_enc, b), Enc(beta'; r))
//         = a_enc^b (1 + beta' N) r^N mod N^2        (range_proofs.rs:688-704)
// with b, beta' and r secret.  Fused: the head of r^N over N's bits >= 256
// (modexp_slide_kernel: r is only the base; nl = 64: 16, 8 or 4 lanes by batch size,
// nl = 96: 8 lanes, the only 192-limb shape), then the 8-lane mta_tail_ct_kernel
// (nl = 96: mta_tail_ct6144_kernel; mta_ct.hip), which carries a_enc^b along the last
// 256 squarings in regular access and takes 1 + beta' N as the operand of its exit
// product.  Composed (unfused, or nl = 96 with 4 or 16 lanes forced): a_enc^b through
// the regular-access modexp, r^N as fsdkr_paillier_encrypt runs it, and prod3 of the
// two with 1 + beta' N; nothing returns to the host in between.
//
// The commitment v of Bob's range proof, a_enc^alpha (1 + gamma N) beta^N mod N^2
// (range_proofs.rs:283-288), is the same computation with alpha < q^3 < 2^768 in b's
// place: el = 24 limbs of secret exponent instead of 8, so the head stops at bit 768
// and bob_v_tail_ct_kernel (nl = 96: bob_v_tail_ct6144_kernel) runs the rest; composed,
// a_enc^alpha is a 768-bit regular-access modexp.  Its buffers have names of their own
// (other sizes).
namespace {

struct RespondNames {
  const char *io, *table, *state, *t2, *ct, *mark;
};
constexpr RespondNames kRespNames{"resp_io", "mxt_resp", "mxt_resp_state", "mxt_resp_t2", "mxt_resp_ct", "mta_tail_ct"};
constexpr RespondNames kBobVNames{"bobv_io", "mxt_bobv", "mxt_bobv_state", "mxt_bobv_t2", "mxt_bobv_ct", "bob_v_tail_ct"};

}  // namespace

// el: limbs per row of the secret exponent b, 8 (the response) or kBobVLimbs (v: alpha);
// shared with the provers of mta_prove.cpp (mta_host.hpp)
int fsdkr::mta_respond_impl(Ctx* c, const char* who, uint32_t nl, uint32_t count, const uint32_t* a_enc,
                            const uint32_t* b, const uint32_t* beta_prim, const uint32_t* r, const uint32_t* n_idx,
                            const uint32_t* ns, uint32_t nk, uint32_t* out, bool want_fused, uint32_t el) {
  const RespondNames& nm = el == 8 ? kRespNames : kBobVNames;
  if (nl != 64 && nl != 96) {
    c->fail("%s: unsupported modulus width %u limbs", who, nl);
    return FSDKR_E_UNSUPPORTED;
  }
  if (count == 0) return FSDKR_OK;
  if (!a_enc || !b || !beta_prim || !r || !n_idx || !ns || !out || !nk) {
    c->fail("%s: bad argument", who);
    return FSDKR_E_ARG;
  }
  const uint32_t nn = 2 * nl;
  // 192 limbs have the 8-lane head only: other forced lanes keep the composed path
  const bool fused = want_fused && (nl == 64 || c->modexp_group == 0 || c->modexp_group == kMtaTailPad);
  if (fused && c->modexp_group != 0 && c->modexp_group != kMtaTailPad) {
    c->fail("%s: the fused chain runs at 8 lanes (forced %u)", who, c->modexp_group);
    return FSDKR_E_ARG;
  }
  std::vector<uint32_t> NN((size_t)nk * nn);
  uint32_t nbits = 1;
  for (uint32_t k = 0; k < nk; ++k) {
    const uint32_t* N = ns + (size_t)k * nl;
    if (!(N[0] & 1u) || bit_len(N, nl) < 2) {
      c->fail("%s: key %u: N must be odd and above 1", who, k);
      return FSDKR_E_ARG;
    }
    const hbn::Limbs Nv = hbn::from(N, nl);
    hbn::store(hbn::mul(Nv, Nv), &NN[(size_t)k * nn], nn);
    nbits = std::max(nbits, bit_len(N, nl));
  }
  for (uint32_t p = 0; p < count; ++p) {
    if (n_idx[p] >= nk) {
      c->fail("%s: n_idx[%u] out of range", who, p);
      return FSDKR_E_ARG;
    }
    if (hbn::cmp_raw(a_enc + (size_t)p * nn, nn, &NN[(size_t)n_idx[p] * nn], nn) >= 0) {   // public
      c->fail("%s: a_enc[%u] is not reduced modulo N^2", who, p);
      return FSDKR_E_ARG;
    }
  }
  const size_t C = count, rl = (size_t)nl * 4, rn = (size_t)nn * 4;
  auto DA0 = [](size_t o) { return (uint64_t)o; };   // offsets until the buffer exists
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = al256(off + (bytes ? bytes : 1)); return o; };
  const size_t o_N = take(nk * rl), o_NN = take(nk * rn), o_r = take(C * rl);
  // r^N: every wave shares its exponent N.  Fused: 8 chains per wave, the pads write a
  // scratch row; composed: as fsdkr_paillier_encrypt (the pads rewrite their own row)
  ModexpJob J;
  J.k32 = nn;
  for (uint32_t p = 0; p < count; ++p)
    J.add(DA0(o_r + p * rl), nl, DA0(o_N + n_idx[p] * rl), nl, fused ? bit_len(ns + (size_t)n_idx[p] * nl, nl) : 32 * nl,
          n_idx[p]);
  uint32_t G = 0, flags = 0;
  if (fused) {
    // state and table rows are the class's digits in order whatever the lanes, so at
    // 128 limbs the head picks its lanes as the keyed launches do (a batch that leaves
    // the chip half empty at 8 lanes runs 16) unless 8 are forced; the runs of one key
    // are padded to whole waves of both kernels: 8 chains of the tail, 16 of a 4-lane head
    G = (c->modexp_group || nl == 96) ? kMtaTailPad : keyed_lanes(count);
    if (!group_by_exponent(J, std::max(kMtaTailPad, 64 / G), count)) {
      c->fail("%s: instances not wave-uniform", who);
      return FSDKR_E_ARG;
    }
    flags = ga_desc_flags(true, G);
  } else if (nn == 128) {
    G = keyed_lanes(count);
    if (group_by_exponent(J, 64 / G, kPadSelf)) flags = kDescOutIdx | kDescSlide;
    else G = 0;
  }
  // rows of the tail's operands: launch order (fused) or the caller's (composed)
  const size_t n = fused ? J.size() : C, n64 = (n + 63) / 64 * 64;
  std::vector<uint32_t> row(n);   // the caller's instance behind row k; a pad repeats the chain before it
  std::vector<uint8_t> pad(n, 0);
  for (size_t k = 0; k < n; ++k) {
    const uint32_t o = fused ? J.out_idx[k] : (uint32_t)k;
    pad[k] = o >= count;
    row[k] = pad[k] ? row[k - 1] : o;   // a run's pads follow its chains
  }
  const size_t o_a = take(n * rn), o_b = take(n * el * 4), o_bp = take(n64 * rl), o_np = take(n64 * 8);
  const size_t o_binom = take(n64 * rn), o_desc = take(J.desc_bytes()), o_out = take((C + 1) * rn);
  const size_t o_ab = take(fused ? 0 : C * rn), o_rn = take(fused ? 0 : C * rn), o_cdesc = take(fused ? 0 : C * 32);
  const size_t o_ops = take(fused ? 0 : C * sizeof(Prod3Operand)), o_midx = take(fused ? 0 : C * 4);
  uint8_t* dev = (uint8_t*)c->buf(nm.io, off);
  if (!dev) {
    c->fail("%s: device allocation failed (%zu bytes)", who, off);
    return FSDKR_E_OOM;
  }
  auto DA = [&](size_t o) { return (uint64_t)(uintptr_t)(dev + o); };
  auto PU = [&](size_t o) { return reinterpret_cast<uint32_t*>(dev + o); };
  for (size_t k = 0; k < J.size(); ++k) {   // offsets -> device addresses
    J.base_ptr[k] += (uint64_t)(uintptr_t)dev;
    J.exp_ptr[k] += (uint64_t)(uintptr_t)dev;
  }
  std::vector<uint32_t> ha(n * nn), hb(n * el, 0u), hbp(n64 * nl, 0u);
  std::vector<uint64_t> hnp(n64, DA(o_N));
  for (size_t k = 0; k < n; ++k) {
    const uint32_t p = row[k];
    memcpy(&ha[k * nn], a_enc + (size_t)p * nn, rn);
    hnp[k] = DA(o_N + n_idx[p] * rl);
    if (pad[k]) continue;   // b = 0, beta' = 0
    memcpy(&hb[k * el], b + (size_t)p * el, el * 4);
    memcpy(&hbp[k * nl], beta_prim + (size_t)p * nl, rl);
  }
  std::vector<uint8_t> desc, cdesc;
  J.pack(desc);
  std::vector<Prod3Operand> ops;
  std::vector<uint32_t> midx;
  if (!fused) {
    ModexpJob Jc;   // a_enc^b: secret exponents of 32 el bits
    Jc.k32 = nn;
    for (uint32_t p = 0; p < count; ++p) Jc.add(DA(o_a + p * rn), nn, DA(o_b + (size_t)p * el * 4), el, 32 * el, n_idx[p]);
    Jc.pack(cdesc);
    ops.resize(C);
    midx.assign(n_idx, n_idx + count);
    for (uint32_t p = 0; p < count; ++p)
      ops[p] = Prod3Operand{DA(o_ab + p * rn), DA(o_rn + p * rn), DA(o_binom + p * rn), nn, nn, nn, 0};
  }
  hipStream_t st = c->stream;
  auto up = [&](size_t o, const void* src, size_t bytes) {
    return bytes ? c->hip_check(hipMemcpyAsync(dev + o, src, bytes, hipMemcpyHostToDevice, st), "H2D respond") : (int)FSDKR_OK;
  };
  auto run = [&]() -> int {
    int rc;
    if ((rc = up(o_N, ns, nk * rl)) || (rc = up(o_NN, NN.data(), nk * rn)) || (rc = up(o_r, r, C * rl)) ||
        (rc = up(o_a, ha.data(), n * rn)) || (rc = up(o_b, hb.data(), n * el * 4)) || (rc = up(o_bp, hbp.data(), n64 * rl)) ||
        (rc = up(o_np, hnp.data(), n64 * 8)) || (rc = up(o_desc, desc.data(), desc.size())) ||
        (rc = up(o_cdesc, cdesc.data(), cdesc.size())) || (rc = up(o_ops, ops.data(), ops.size() * sizeof(Prod3Operand))) ||
        (rc = up(o_midx, midx.data(), midx.size() * 4)))
      return rc;
    uint32_t* cons = nullptr;
    if ((rc = setup_moduli(c, nn, PU(o_NN), nk, &cons, "resp"))) return rc;
    BinomCtArgs ba{PU(o_bp), (const uint64_t*)(dev + o_np), PU(o_binom), (uint32_t)n64};
    c->mark("binom_ct", true);
    rc = c->hip_check(launch_binom_ct(nl, ba, st), "binom_ct");
    c->mark("binom_ct", false);
    if (rc) return rc;
    if (fused) {
      SplitArgs head;
      head.lo_bit = el == 8 ? kMtaTailLo : kBobVTailLo;   // 32 el: the secret exponent rides the tail
      if ((rc = launch_modexp_desc(c, nn, (uint32_t)n, nbits, dev + o_desc, cons, PU(o_out), st, nm.table, 0, G, flags,
                                   &head)))
        return rc;
      const uint32_t w = choose_slide_window(nbits);   // the head's window (launch_modexp_desc)
      const DevBuf tb = c->bufs[nm.table], sb = c->bufs[nm.state];
      uint32_t* t2 = (uint32_t*)c->buf(nm.t2, n * 16 * (size_t)shape_digits(nn) * 4);
      if (!tb.ptr || !sb.ptr || !t2) {
        c->fail("%s: device allocation failed (tail tables)", who);
        return FSDKR_E_OOM;
      }
      const size_t n8 = n * 8, n4 = n * 4;
      const uint8_t* d = dev + o_desc;
      MtaTailArgs ta{(const uint64_t*)(d + n8), (const uint32_t*)(d + 2 * n8 + 2 * n4), (const uint32_t*)(d + 2 * n8 + 4 * n4),
                     cons, (const uint32_t*)tb.ptr, (const uint32_t*)sb.ptr, w, PU(o_a), PU(o_b), PU(o_binom), t2,
                     PU(o_out), (uint32_t)n};
      c->mark(nm.mark, true);
      rc = c->hip_check(launch_mta_tail_ct(nl, el, ta, st), nm.mark);
      c->mark(nm.mark, false);
      if (rc) return rc;
    } else {
      {
        CtScope ct(c);
        if ((rc = launch_modexp_desc(c, nn, count, 32 * el, dev + o_cdesc, cons, PU(o_ab), st, nm.ct))) return rc;
      }
      if ((rc = launch_modexp_desc(c, nn, (uint32_t)J.size(), 32 * nl, dev + o_desc, cons, PU(o_rn), st, nm.table, 0, G,
                                   flags)))
        return rc;
      Prod3Args pa{(const Prod3Operand*)(dev + o_ops), PU(o_midx), cons, PU(o_out), count};
      c->mark("prod3", true);
      rc = c->hip_check(launch_prod3(nn, pa, st), "prod3 respond");
      c->mark("prod3", false);
      if (rc) return rc;
    }
    return c->hip_check(hipMemcpyAsync(out, dev + o_out, C * rn, hipMemcpyDeviceToHost, st), "D2H respond");
  };
  const int rc = run();
  // scrub what held b, beta', r or a value made from them: the operand image, the
  // head's window table and state (powers of r), the regular-access table
  int rs = FSDKR_OK;
  for (const char* name : {nm.io, nm.table, nm.state, nm.t2, nm.ct}) {
    const int q = scrub(c, name);
    if (!rs) rs = q;
  }
  const int ry = c->sync();
  wipe(hb);   // the host rows of b and beta', once the uploads are done with them
  wipe(hbp);
  return rc ? rc : rs ? rs : ry;
}

extern "C" {

int fsdkr_mta_respond(fsdkr_ctx* ctx, uint32_t nl, uint32_t count, const uint32_t* a_enc, const uint32_t* b,
                      const uint32_t* beta_prim, const uint32_t* r, const uint32_t* n_idx, const uint32_t* ns,
                      uint32_t n_keys, uint32_t* out) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return FSDKR_E_ARG;
  return mta_respond_impl(c, "fsdkr_mta_respond", nl, count, a_enc, b, beta_prim, r, n_idx, ns, n_keys, out, true);
}

int fsdkr_mta_respond_unfused(fsdkr_ctx* ctx, uint32_t nl, uint32_t count, const uint32_t* a_enc, const uint32_t* b,
                              const uint32_t* beta_prim, const uint32_t* r, const uint32_t* n_idx, const uint32_t* ns,
                              uint32_t n_keys, uint32_t* out) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return FSDKR_E_ARG;
  return mta_respond_impl(c, "fsdkr_mta_respond_unfused", nl, count, a_enc, b, beta_prim, r, n_idx, ns, n_keys, out, false);
}

int fsdkr_bob_commit_v(fsdkr_ctx* ctx, uint32_t nl, uint32_t count, const uint32_t* a_enc, const uint32_t* alpha,
                       const uint32_t* gamma, const uint32_t* beta, const uint32_t* n_idx, const uint32_t* ns,
                       uint32_t n_keys, uint32_t* out) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return FSDKR_E_ARG;
  return mta_respond_impl(c, "fsdkr_bob_commit_v", nl, count, a_enc, alpha, gamma, beta, n_idx, ns, n_keys, out, true,
                          kBobVLimbs);
}

int fsdkr_bob_commit_v_unfused(fsdkr_ctx* ctx, uint32_t nl, uint32_t count, const uint32_t* a_enc, const uint32_t* alpha,
                               const uint32_t* gamma, const uint32_t* beta, const uint32_t* n_idx, const uint32_t* ns,
                               uint32_t n_keys, uint32_t* out) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return FSDKR_E_ARG;
  return mta_respond_impl(c, "fsdkr_bob_commit_v_unfused", nl, count, a_enc, alpha, gamma, beta, n_idx, ns, n_keys, out,
                          false, kBobVLimbs);
}

}  // extern "C"
