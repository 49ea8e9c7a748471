// fsdkr_alice_verify of the C ABI (include/fsdkr/fsdkr.h): AliceProof::verify
// (range_proofs.rs:112-164) of `count` independent proofs in one device pass, the
// check of the first message of GG20's MtA (c_A = Enc(a; r) with its range proof).
// Per proof, in the reference's order: s1 <= q^3 (:121); z^e a unit mod N~
// (:125-129); cipher^e a unit mod N^2 (:141-145); w = h1^s1 h2^s2 z^-e mod N~
// (:131-135); u = (1 + s1 N) s^N cipher^-e mod N^2 (:137-151); the transcript
// hash H(N, N + 1, cipher, z, u, w) == e (:153-163).
// An assembly of the pieces of fsdkr_bob_verify (mta.cpp) and of collect(): the
// fixed-base combs for h1^s1 | h2^s2 (public exponents, bases shared per key), a
// 256-bit modexp job for z^e with Montgomery's simultaneous inversion, cipher^-1 by
// the same inversion (cipher^e is a unit iff cipher is), and s^N (cipher^-1)^e as
// ONE split chain: the head over N's high bits, the two-base tail with cipher^-1
// riding its squarings in 4-bit windows of e < 2^256.  nl = 64: GA's split at bit
// 256 (4 / 8 / 16 lanes); nl = 96: the 192-limb two-base tail of
// fsdkr_modexp_joint3_batch_k (split at bit 768, 8 lanes).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
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

extern "C" int fsdkr_alice_verify(fsdkr_ctx* ctx, const fsdkr_alice_batch* b, uint8_t* verdict) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return FSDKR_E_ARG;
  const char* who = "fsdkr_alice_verify";
  if (!b) {
    c->fail("%s: null batch", who);
    return FSDKR_E_ARG;
  }
  const uint32_t count = b->count, nk = b->n_keys, nl = b->nl, nn = 2 * b->nl;
  if (count == 0) return FSDKR_OK;
  if (!verdict || !nk || !b->N || !b->Ntilde || !b->h1 || !b->h2 || !b->key_idx || !b->cipher || !b->z || !b->s ||
      !b->e || !b->s1 || !b->s2 || !b->el || !b->s1l || !b->s2l || b->el > 64 || b->s1l > 64) {
    c->fail("%s: bad argument", who);
    return FSDKR_E_ARG;
  }
  if (nl != 64 && nl != 96) {
    c->fail("%s: unsupported modulus width %u limbs", who, nl);
    return FSDKR_E_UNSUPPORTED;
  }
  const size_t kdl = (size_t)shape_digits(nl), kdn = (size_t)shape_digits(nn);
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
  const uint32_t lo_bit = nn == 128 ? 256u : kBobSplit;

  // ---- host pre-pass -------------------------------------------------------
  static const uint32_t kQ[8] = {0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u,
                                 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
  const hbn::Limbs q = hbn::from(kQ, 8), q3 = hbn::mul(hbn::mul(q, q), q);
  std::vector<uint8_t> pre(count, 1);
  std::vector<uint32_t> s1a((size_t)count * kS1Limbs, 0u), ea((size_t)count * kELimbs, 0u);
  for (uint32_t p = 0; p < count; ++p) {
    const uint32_t* s1 = b->s1 + (size_t)p * b->s1l;
    if (hbn::cmp_raw(s1, b->s1l, q3.data(), q3.size()) > 0) pre[p] = 0;   // :121 (s1 == q^3 passes)
    else memcpy(&s1a[(size_t)p * kS1Limbs], s1, std::min(b->s1l, kS1Limbs) * 4);
    const uint32_t* e = b->e + (size_t)p * b->el;
    bool wide = false;
    for (uint32_t k = kELimbs; k < b->el; ++k) wide = wide || e[k] != 0;
    if (!wide) memcpy(&ea[(size_t)p * kELimbs], e, std::min(b->el, kELimbs) * 4);
    // a challenge of 256 bits or more never equals the hash; e = 0 only if the hash is 0
    if (wide || hbn::is_zero_raw(&ea[(size_t)p * kELimbs], kELimbs)) pre[p] = 0;
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
  std::vector<uint32_t> v_c, v_z, v_s;
  const uint32_t* c_red = reduced(b->cipher, nn, NN.data(), nn, v_c);
  const uint32_t* z_red = reduced(b->z, nl, b->Ntilde, nl, v_z);
  const uint32_t* s_red = reduced(b->s, nl, NN.data(), nn, v_s);
  // 1 + s1 N = 1 + (s1 mod N) N  (mod N^2)
  std::vector<uint32_t> s1r((size_t)count * nl, 0u);
  for (uint32_t p = 0; p < count; ++p) {
    const uint32_t* s1 = &s1a[(size_t)p * kS1Limbs];
    const uint32_t* N = b->N + (size_t)key[p] * nl;
    if (hbn::cmp_raw(s1, kS1Limbs, N, nl) < 0) memcpy(&s1r[(size_t)p * nl], s1, std::min(kS1Limbs, nl) * 4);
    else hbn::store(hbn::mod(hbn::from(s1, kS1Limbs), hbn::from(N, nl)), &s1r[(size_t)p * nl], nl);
  }
  uint32_t s1bits = 1, s2bits = 1;
  for (uint32_t p = 0; p < count; ++p) {
    s1bits = std::max(s1bits, bit_len(&s1a[(size_t)p * kS1Limbs], kS1Limbs));
    s2bits = std::max(s2bits, bit_len(b->s2 + (size_t)p * b->s2l, b->s2l));
  }

  // ---- device image --------------------------------------------------------
  const size_t C = count, rl = (size_t)nl * 4, rn = (size_t)nn * 4;
  const uint32_t per_wave = 64 / group;
  const size_t cap = C + (size_t)nk * per_wave;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = al256(off + (bytes ? bytes : 1)); return o; };
  const size_t o_N = take(nk * rl), o_Nt = take(nk * rl), o_NN = take(nk * rn), o_h1 = take(nk * rl), o_h2 = take(nk * rl);
  const size_t o_c = take(C * rn), o_z = take(C * rl), o_s = take(C * rl);
  const size_t o_cr = v_c.empty() ? o_c : take(C * rn), o_zr = v_z.empty() ? o_z : take(C * rl);
  const size_t o_e = take(C * b->el * 4), o_ea = take(C * kELimbs * 4), o_s1 = take(C * kS1Limbs * 4);
  const size_t o_s1r = take(C * rl), o_s2 = take(C * b->s2l * 4), o_one = take(rn), o_pre = take(C);
  // descriptors
  const size_t o_gdesc = take(cap * 36), o_gd2 = take(cap * kTailDescBytes), o_zdesc = take(C * 32);
  const size_t o_iy = take(2 * C * 8), o_im = take(2 * C * 8), o_iord = take(2 * C * 4), o_igs = take((2 * C + 2 * nk + 2) * 4);
  const size_t o_bs = take(C * 8), o_bn = take(C * 8), o_hn = take(C * 8), o_hc = take(C * 8);
  const size_t o_p3 = take(2 * C * sizeof(Prod3Operand)), o_p3m = take(2 * C * 4);
  // results
  const size_t o_cinv = take(C * rn), o_uc = take(C * 4), o_ze = take(C * rl), o_zinv = take(C * rl), o_uz = take(C * 4);
  const size_t o_fb = take(2 * C * rl), o_binom = take(C * rn), o_ga = take((C + 1) * rn);
  const size_t o_w = take(C * rl), o_u = take(C * rn);
  const size_t o_iscr = take(C * (kdn + kdl) * 4);
  uint8_t* dev = (uint8_t*)c->buf("alice_io", off);
  if (!dev) {
    c->fail("%s: device allocation failed (%zu bytes)", who, off);
    return FSDKR_E_OOM;
  }
  auto DA = [&](size_t o) { return (uint64_t)(uintptr_t)(dev + o); };
  auto PU = [&](size_t o) { return reinterpret_cast<uint32_t*>(dev + o); };
  hipStream_t st = c->stream;
  auto up = [&](size_t o, const void* src, size_t bytes) {
    return bytes ? c->hip_check(hipMemcpyAsync(dev + o, src, bytes, hipMemcpyHostToDevice, st), "H2D alice") : (int)FSDKR_OK;
  };
  std::vector<uint32_t> one(nn, 0u);
  one[0] = 1;

  // s^N mod N^2, regrouped so every wave shares its exponent N; cipher^-1 rides the tail
  ModexpJob J;
  J.k32 = nn;
  for (uint32_t p = 0; p < count; ++p)
    J.add(DA(o_s + p * rl), nl, DA(o_N + key[p] * rl), nl, bit_len(b->N + (size_t)key[p] * nl, nl), key[p]);
  if (!group_by_exponent(J, per_wave, count)) {
    c->fail("%s: instances not wave-uniform", who);
    return FSDKR_E_ARG;
  }
  std::vector<uint8_t> gdesc, gd2;
  J.pack(gdesc);
  tail_desc(J, count, DA(o_cinv), nn, DA(o_ea), kELimbs, gd2);
  // z^e mod N~
  ModexpJob Jz;
  Jz.k32 = nl;
  for (uint32_t p = 0; p < count; ++p)
    Jz.add(DA(o_zr + p * rl), nl, DA(o_ea + (size_t)p * kELimbs * 4), kELimbs, kEBits, key[p]);
  std::vector<uint8_t> zdesc;
  Jz.pack(zdesc);
  // inverses: cipher mod N^2, then z^e mod N~
  std::vector<uint64_t> iy(2 * C), im(2 * C);
  std::vector<uint32_t> ord_nn, gs_nn, ord_nl, gs_nl;
  inverse_groups(key, 1, count, nk, ord_nn, gs_nn);
  inverse_groups(key, 1, count, nk, ord_nl, gs_nl);
  for (uint32_t p = 0; p < count; ++p) {
    iy[p] = DA(o_cr + p * rn);
    im[p] = DA(o_NN + key[p] * rn);
    iy[C + p] = DA(o_ze + p * rl);
    im[C + p] = DA(o_Nt + key[p] * rl);
  }
  std::vector<uint32_t> iord(ord_nn);
  iord.insert(iord.end(), ord_nl.begin(), ord_nl.end());
  std::vector<uint32_t> igs(gs_nn);
  const size_t igs_nl = igs.size();
  igs.insert(igs.end(), gs_nl.begin(), gs_nl.end());
  // fixed-base job: h1^s1 | h2^s2, bases [h1_k | h2_k]
  FbJob fb;
  fb.k32 = nl;
  for (uint32_t k = 0; k < nk; ++k) fb.add_base(DA(o_h1 + k * rl), nl, k);
  for (uint32_t k = 0; k < nk; ++k) fb.add_base(DA(o_h2 + k * rl), nl, k);
  for (uint32_t p = 0; p < count; ++p)
    fb.add(key[p], DA(o_s1 + (size_t)p * kS1Limbs * 4), kS1Limbs, s1bits, DA(o_fb + p * rl));
  for (uint32_t p = 0; p < count; ++p)
    fb.add(nk + key[p], DA(o_s2 + (size_t)p * b->s2l * 4), b->s2l, s2bits, DA(o_fb + (C + p) * rl));
  fb.finalize();
  // binom, products, hash
  std::vector<uint64_t> bs(C), bn(C), hn(C), hc(C);
  std::vector<Prod3Operand> p3(2 * C);
  std::vector<uint32_t> p3m(2 * C);
  for (uint32_t p = 0; p < count; ++p) {
    bs[p] = DA(o_s1r + p * rl);
    bn[p] = hn[p] = DA(o_N + key[p] * rl);
    hc[p] = DA(o_c + p * rn);   // hashed as given
    // w = h1^s1 h2^s2 (z^e)^-1 mod N~;  u = (chain) (1 + s1 N) mod N^2
    p3[p] = Prod3Operand{DA(o_fb + p * rl), DA(o_fb + (C + p) * rl), DA(o_zinv + p * rl), nl, nl, nl, 0};
    p3[C + p] = Prod3Operand{DA(o_ga + p * rn), DA(o_binom + p * rn), DA(o_one), nn, nn, nn, 0};
    p3m[p] = p3m[C + p] = key[p];
  }

  if ((rc = up(o_N, b->N, nk * rl)) || (rc = up(o_Nt, b->Ntilde, nk * rl)) || (rc = up(o_NN, NN.data(), nk * rn)) ||
      (rc = up(o_h1, h1r.data(), nk * rl)) || (rc = up(o_h2, h2r.data(), nk * rl)) || (rc = up(o_c, b->cipher, C * rn)) ||
      (rc = up(o_z, b->z, C * rl)) || (rc = up(o_s, s_red, C * rl)) || (!v_c.empty() && (rc = up(o_cr, c_red, C * rn))) ||
      (!v_z.empty() && (rc = up(o_zr, z_red, C * rl))) || (rc = up(o_e, b->e, C * b->el * 4)) ||
      (rc = up(o_ea, ea.data(), C * kELimbs * 4)) || (rc = up(o_s1, s1a.data(), C * kS1Limbs * 4)) ||
      (rc = up(o_s1r, s1r.data(), C * rl)) || (rc = up(o_s2, b->s2, C * b->s2l * 4)) || (rc = up(o_one, one.data(), rn)) ||
      (rc = up(o_pre, pre.data(), C)) || (rc = up(o_gdesc, gdesc.data(), gdesc.size())) ||
      (rc = up(o_gd2, gd2.data(), gd2.size())) || (rc = up(o_zdesc, zdesc.data(), zdesc.size())) ||
      (rc = up(o_iy, iy.data(), iy.size() * 8)) || (rc = up(o_im, im.data(), im.size() * 8)) ||
      (rc = up(o_iord, iord.data(), iord.size() * 4)) || (rc = up(o_igs, igs.data(), igs.size() * 4)) ||
      (rc = up(o_bs, bs.data(), C * 8)) || (rc = up(o_bn, bn.data(), C * 8)) || (rc = up(o_hn, hn.data(), C * 8)) ||
      (rc = up(o_hc, hc.data(), C * 8)) || (rc = up(o_p3, p3.data(), p3.size() * sizeof(Prod3Operand))) ||
      (rc = up(o_p3m, p3m.data(), p3m.size() * 4)))
    return rc;

  // ---- kernels -------------------------------------------------------------
  uint32_t *cons_nl = nullptr, *cons_nn = nullptr;
  if ((rc = setup_moduli(c, nl, PU(o_Nt), nk, &cons_nl, "alice_nl")) ||
      (rc = setup_moduli(c, nn, PU(o_NN), nk, &cons_nn, "alice_nn")))
    return rc;
  uint32_t* iscr = PU(o_iscr);   // [C][kdn] for the N^2 inverse, then [C][kdl] for the N~ one
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
  {
    // cipher^-1 (and cipher's unit flag), then s^N (cipher^-1)^e in one chain
    BatchInverseArgs a{(const uint64_t*)(dev + o_iy), (const uint64_t*)(dev + o_im), PU(o_iord), PU(o_igs), PU(o_cinv),
                       PU(o_uc), iscr, (uint32_t)gs_nn.size() - 1};
    c->mark("inverse", true);
    rc = c->hip_check(launch_inverse_batch(nn, a, st), "inverse nn");
    c->mark("inverse", false);
    if (rc) return drop(rc);
    const uint32_t flags = ga_desc_flags(true, group);
    const uint32_t gn = (uint32_t)J.size();
    SplitArgs head;
    head.lo_bit = lo_bit;
    SplitArgs tail = head;
    tail.tail = true;
    tail.d_desc2 = dev + o_gd2;
    if ((rc = launch_modexp_desc(c, nn, gn, nbits, dev + o_gdesc, cons_nn, PU(o_ga), st, "mxt_alice", 0, group, flags, &head)) ||
        (rc = launch_modexp_desc(c, nn, gn, nbits, dev + o_gdesc, cons_nn, PU(o_ga), st, "mxt_alice", 0, group, flags, &tail)))
      return drop(rc);
  }
  // the N~ side -- z^e, its inverse, the fixed-base job -- on a side stream beside the
  // N^2 chains enqueued above
  {
    hipStream_t ss = c->side_stream(1);
    (void)hipStreamWaitEvent(ss, ready, 0);
    StreamScope scope(c, ss);
    if ((rc = launch_modexp_desc(c, nl, count, kEBits, dev + o_zdesc, cons_nl, PU(o_ze), ss, "mxt_alice_z")))
      return drop(rc);
    BatchInverseArgs a{(const uint64_t*)(dev + o_iy) + C, (const uint64_t*)(dev + o_im) + C, PU(o_iord) + C,
                       PU(o_igs) + igs_nl, PU(o_zinv), PU(o_uz), iscr + C * kdn, (uint32_t)gs_nl.size() - 1};
    c->mark("inverse", true);
    rc = c->hip_check(launch_inverse_batch(nl, a, ss), "inverse nl");
    c->mark("inverse", false);
    if (rc || (rc = fb_run(c, fb, cons_nl, "alice")) ||
        (rc = c->hip_check(hipEventRecord(side_done, ss), "event record")))
      return drop(rc);
  }
  (void)hipStreamWaitEvent(st, side_done, 0);
  drop(0);
  {
    BinomArgs a{(const uint64_t*)(dev + o_bs), (const uint64_t*)(dev + o_bn), nl, nl, nn, PU(o_binom), count};
    if ((rc = c->hip_check(launch_binom(a, st), "binom"))) return rc;
    Prod3Args pa{(const Prod3Operand*)(dev + o_p3), PU(o_p3m), cons_nl, PU(o_w), count};
    if ((rc = c->hip_check(launch_prod3(nl, pa, st), "prod3 nl"))) return rc;
    Prod3Args pb{(const Prod3Operand*)(dev + o_p3) + C, PU(o_p3m) + C, cons_nn, PU(o_u), count};
    if ((rc = c->hip_check(launch_prod3(nn, pb, st), "prod3 nn"))) return rc;
  }
  {
    AliceHashArgs h{(const uint64_t*)(dev + o_hn), (const uint64_t*)(dev + o_hc), PU(o_z), PU(o_u), PU(o_w), PU(o_e),
                    nl, nn, nl, b->el, dev + o_pre, count, nullptr};
    c->mark("alice_hash", true);
    rc = c->hip_check(launch_alice_hash(h, st), "alice_hash");
    c->mark("alice_hash", false);
    if (rc) return rc;
  }
  std::vector<uint8_t> hv(count);
  std::vector<uint32_t> uc(count), uz(count);
  if ((rc = c->hip_check(hipMemcpyAsync(hv.data(), dev + o_pre, C, hipMemcpyDeviceToHost, st), "D2H alice")) ||
      (rc = c->hip_check(hipMemcpyAsync(uc.data(), dev + o_uc, C * 4, hipMemcpyDeviceToHost, st), "D2H alice")) ||
      (rc = c->hip_check(hipMemcpyAsync(uz.data(), dev + o_uz, C * 4, hipMemcpyDeviceToHost, st), "D2H alice")))
    return rc;
  if ((rc = c->sync())) return rc;
  // the s1 bound, then the two inverses (:121-145), then the hash
  for (uint32_t p = 0; p < count; ++p) verdict[p] = (pre[p] && uz[p] && uc[p] && hv[p]) ? 1 : 0;
  return FSDKR_OK;
}
