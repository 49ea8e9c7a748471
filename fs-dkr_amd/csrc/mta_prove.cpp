// The whole MtA provers of the C ABI (include/fsdkr/fsdkr.h):
//   fsdkr_bob_prove     BobProof::generate (range_proofs.rs:448-515), every draw an input
//   fsdkr_alice_prove   AliceProof::generate (:168-202)
//   fsdkr_resp_ct       parity entry of resp_ct_kernel: out = e x + y
// Round 1 is the stages of the existing entries (mta_host.hpp): ONE constant-time comb
// for the commitments mod N~ (pedersen_commit_ct_run: z, z', t, w of Bob, z, w of
// Alice) and the fused constant-time chain for the value mod N^2 (mta_respond_impl at
// 24 limbs: Bob's v = a_enc^alpha (1 + gamma N) beta^N; Alice's u = (1 + alpha N)
// beta^N is the same chain with a_enc = 1 and a zero exponent row, so alpha enters
// through the constant-time binomial, not fsdkr_paillier_encrypt's, which skips zero
// limbs of its message).  Each stage scrubs what it held; the commitments are public
// and come back to the host in between, as the entries return them.
// Round 2 (prove_round2) stays on the device: the transcript hash writes e
// (bob_challenge_kernel / alice_challenge_kernel), r^e mod N runs through the
// public-exponent modexp with the challenge rows as its exponents, prod3 multiplies
// beta in and reduces exactly, and resp_ct_kernel forms the integer responses.
// r^e never leaves the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "fsdkr/fsdkr.h"
#include "hostbn.hpp"
#include "kernels.h"
#include "mta_host.hpp"
#include "prove_geom.hpp"
#include "verify.h"

using namespace fsdkr;

namespace {

struct RespJob {   // out = e x + y, rows on the host
  const uint32_t* x;
  uint32_t xl;
  const uint32_t* y;
  uint32_t yl;
  uint32_t* out;
};

struct PubRows {   // a hashed value per proof, rows on the host
  const uint32_t* src;
  uint32_t limbs;
};

// the key table's checks shared by both provers (all public)
int check_keys(Ctx* c, const char* who, uint32_t nl, uint32_t count, uint32_t nk, const uint32_t* N,
               const uint32_t* Ntilde, const uint32_t* h1, const uint32_t* h2, const uint32_t* key_idx) {
  for (uint32_t k = 0; k < nk; ++k) {
    const uint32_t *n = N + (size_t)k * nl, *nt = Ntilde + (size_t)k * nl;
    if (!(n[0] & 1u) || !(nt[0] & 1u) || bit_len(n, nl) < 2 || bit_len(nt, nl) < 2) {
      c->fail("%s: key %u: N and Ntilde must be odd and above 1", who, k);
      return FSDKR_E_ARG;
    }
    if (hbn::cmp_raw(h1 + (size_t)k * nl, nl, nt, nl) >= 0 || hbn::cmp_raw(h2 + (size_t)k * nl, nl, nt, nl) >= 0) {
      c->fail("%s: key %u: h1, h2 must be below Ntilde", who, k);
      return FSDKR_E_ARG;
    }
  }
  for (uint32_t p = 0; p < count; ++p)
    if (key_idx[p] >= nk) {
      c->fail("%s: key_idx[%u] out of range", who, p);
      return FSDKR_E_ARG;
    }
  return FSDKR_OK;
}

// e = H(N, N + 1, pub..) per proof; s = r^e beta mod N; the jobs' e x + y.  pub: Bob's
// a_enc, mta, z, z', t, v, w (bob: 7 rows) or Alice's cipher, z, u, w (4 rows).
int prove_round2(Ctx* c, const char* who, bool bob, uint32_t nl, uint32_t count, uint32_t nk, const uint32_t* N,
                 const uint32_t* key_idx, const PubRows* pub, const uint32_t* r, const uint32_t* beta, const RespJob* jobs,
                 uint32_t* e_out, uint32_t* s_out) {
  const uint32_t npub = bob ? 7u : 4u, njobs = bob ? 4u : 2u;
  const size_t C = count, Cp = resp_pad(count), rl = (size_t)nl * 4;
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = al256(off + (bytes ? bytes : 1)); return o; };
  // public image
  const size_t o_N = take(nk * rl), o_np = take(C * 8), o_cp = take(bob ? 0 : C * 8), o_one = take(rl), o_idx = take(C * 4);
  size_t o_pub[7];
  for (uint32_t k = 0; k < npub; ++k) o_pub[k] = take(C * pub[k].limbs * 4);
  const size_t o_e = take(Cp * kProveELimbs * 4), o_desc = take(C * 32), o_ops = take(C * sizeof(Prod3Operand));
  const size_t pub_bytes = off;
  off = 0;
  // secret image: r, beta, r^e, s, and per job x | y | out (count_pad rows, the pads zero)
  const size_t o_r = take(C * rl), o_b = take(C * rl), o_re = take(C * rl), o_s = take(C * rl);
  size_t o_x[4], o_y[4], o_o[4];
  uint32_t ol[4];
  for (uint32_t j = 0; j < njobs; ++j) {
    ol[j] = resp_out_limbs(jobs[j].xl, jobs[j].yl);
    o_x[j] = take(Cp * jobs[j].xl * 4);
    o_y[j] = take(Cp * jobs[j].yl * 4);
    o_o[j] = take(Cp * ol[j] * 4);
  }
  const size_t sec_bytes = off;
  uint8_t* dev = (uint8_t*)c->buf("prove_io", pub_bytes);
  uint8_t* sec = (uint8_t*)c->buf("prove_secret", sec_bytes);
  if (!dev || !sec) {
    c->fail("%s: device allocation failed (%zu bytes)", who, pub_bytes + sec_bytes);
    return FSDKR_E_OOM;
  }
  auto DA = [&](const uint8_t* base, size_t o) { return (uint64_t)(uintptr_t)(base + o); };
  auto PU = [&](uint8_t* base, size_t o) { return reinterpret_cast<uint32_t*>(base + o); };
  std::vector<uint64_t> np(C), cp(bob ? 0 : C);   // cp: the cipher rows by address (Alice's hash reads them so)
  std::vector<uint32_t> one(nl, 0u);
  one[0] = 1;
  std::vector<Prod3Operand> ops(C);
  ModexpJob J;   // r^e mod N: the exponents are the challenge kernel's rows
  J.k32 = nl;
  for (uint32_t p = 0; p < count; ++p) {
    np[p] = DA(dev, o_N + key_idx[p] * rl);
    if (!bob) cp[p] = DA(dev, o_pub[0] + (size_t)p * pub[0].limbs * 4);
    J.add(DA(sec, o_r + p * rl), nl, DA(dev, o_e + (size_t)p * kProveELimbs * 4), kProveELimbs, kEBits, key_idx[p]);
    ops[p] = Prod3Operand{DA(sec, o_re + p * rl), DA(sec, o_b + p * rl), DA(dev, o_one), nl, nl, nl, 0};
  }
  std::vector<uint8_t> desc;
  J.pack(desc);
  hipStream_t st = c->stream;
  auto up = [&](uint8_t* base, size_t o, const void* src, size_t bytes) {
    return bytes ? c->hip_check(hipMemcpyAsync(base + o, src, bytes, hipMemcpyHostToDevice, st), "H2D prove") : (int)FSDKR_OK;
  };
  auto run = [&]() -> int {
    int rc;
    // the pads of e and of the jobs' rows are zero
    if ((rc = c->hip_check(hipMemsetAsync(sec, 0, sec_bytes, st), "memset prove")) ||
        (rc = c->hip_check(hipMemsetAsync(dev + o_e, 0, Cp * kProveELimbs * 4, st), "memset prove")))
      return rc;
    if ((rc = up(dev, o_N, N, nk * rl)) || (rc = up(dev, o_np, np.data(), C * 8)) || (rc = up(dev, o_cp, cp.data(), cp.size() * 8)) ||
        (rc = up(dev, o_one, one.data(), rl)) || (rc = up(dev, o_idx, key_idx, C * 4)) ||
        (rc = up(dev, o_desc, desc.data(), desc.size())) || (rc = up(dev, o_ops, ops.data(), C * sizeof(Prod3Operand))) ||
        (rc = up(sec, o_r, r, C * rl)) || (rc = up(sec, o_b, beta, C * rl)))
      return rc;
    for (uint32_t k = 0; k < npub; ++k)
      if ((rc = up(dev, o_pub[k], pub[k].src, C * pub[k].limbs * 4))) return rc;
    for (uint32_t j = 0; j < njobs; ++j)
      if ((rc = up(sec, o_x[j], jobs[j].x, C * jobs[j].xl * 4)) || (rc = up(sec, o_y[j], jobs[j].y, C * jobs[j].yl * 4)))
        return rc;
    uint32_t* cons = nullptr;
    if ((rc = setup_moduli(c, nl, PU(dev, o_N), nk, &cons, "prove_n"))) return rc;
    size_t m = c->tbeg("prove_challenge", st);
    if (bob) {
      BobHashArgs h{(const uint64_t*)(dev + o_np), PU(dev, o_pub[0]), PU(dev, o_pub[1]), PU(dev, o_pub[2]), PU(dev, o_pub[4]),
                    PU(dev, o_pub[3]), PU(dev, o_pub[6]), PU(dev, o_pub[5]), nullptr, nullptr, nullptr, nl, 2 * nl, nl,
                    kProveELimbs, nullptr, count};
      rc = c->hip_check(launch_bob_challenge(h, PU(dev, o_e), st), "bob_challenge");
    } else {
      AliceHashArgs h{(const uint64_t*)(dev + o_np), (const uint64_t*)(dev + o_cp), PU(dev, o_pub[1]), PU(dev, o_pub[2]),
                      PU(dev, o_pub[3]), nullptr, nl, 2 * nl, nl, kProveELimbs, nullptr, count, nullptr};
      rc = c->hip_check(launch_alice_challenge(h, PU(dev, o_e), st), "alice_challenge");
    }
    c->tend(m, st);
    if (rc) return rc;
    m = c->tbeg("prove_re", st);
    rc = launch_modexp_desc(c, nl, count, kEBits, dev + o_desc, cons, PU(sec, o_re), st, "mxt_prove");
    c->tend(m, st);
    if (rc) return rc;
    Prod3Args pa{(const Prod3Operand*)(dev + o_ops), PU(dev, o_idx), cons, PU(sec, o_s), count};
    c->mark("prod3", true);
    rc = c->hip_check(launch_prod3(nl, pa, st), "prod3 prove");
    c->mark("prod3", false);
    if (rc) return rc;
    m = c->tbeg("prove_resp", st);
    for (uint32_t j = 0; j < njobs && !rc; ++j) {
      RespCtArgs ra{PU(dev, o_e), PU(sec, o_x[j]), PU(sec, o_y[j]), PU(sec, o_o[j]), jobs[j].xl, jobs[j].yl, ol[j],
                    (uint32_t)Cp};
      rc = c->hip_check(launch_resp_ct(ra, st), "resp_ct launch");
    }
    c->tend(m, st);
    if (rc) return rc;
    if ((rc = c->hip_check(hipMemcpyAsync(e_out, dev + o_e, C * kProveELimbs * 4, hipMemcpyDeviceToHost, st), "D2H prove")) ||
        (rc = c->hip_check(hipMemcpyAsync(s_out, sec + o_s, C * rl, hipMemcpyDeviceToHost, st), "D2H prove")))
      return rc;
    for (uint32_t j = 0; j < njobs; ++j)
      if ((rc = c->hip_check(hipMemcpyAsync(jobs[j].out, sec + o_o[j], C * ol[j] * 4, hipMemcpyDeviceToHost, st), "D2H prove")))
        return rc;
    return FSDKR_OK;
  };
  const int rc = run();
  // scrub what held r, beta, the response operands or a value made from them: the
  // secret image (r^e among it) and the window table of the r^e chain
  int rs = FSDKR_OK;
  for (const char* name : {"prove_secret", "mxt_prove"}) {
    const int q = scrub(c, name);
    if (!rs) rs = q;
  }
  const int ry = c->sync();
  return rc ? rc : rs ? rs : ry;
}

}  // namespace

extern "C" {

int fsdkr_resp_ct(fsdkr_ctx* ctx, uint32_t count, const uint32_t* e, const uint32_t* x, uint32_t xl, const uint32_t* y,
                  uint32_t yl, uint32_t* out) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return FSDKR_E_ARG;
  const char* who = "fsdkr_resp_ct";
  if (xl < 1 || xl > kRespMaxLimbs || yl < 1 || yl > kRespMaxLimbs) {
    c->fail("%s: rows of 1 to %u limbs (xl %u, yl %u)", who, kRespMaxLimbs, xl, yl);
    return FSDKR_E_ARG;
  }
  if (count == 0) return FSDKR_OK;
  if (!e || !x || !y || !out) {
    c->fail("%s: null pointer", who);
    return FSDKR_E_ARG;
  }
  const size_t C = count, Cp = resp_pad(count);
  const uint32_t ol = resp_out_limbs(xl, yl);
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = al256(off + bytes); return o; };
  const size_t o_e = take(Cp * kProveELimbs * 4), o_x = take(Cp * xl * 4), o_y = take(Cp * yl * 4), o_o = take(Cp * ol * 4);
  uint8_t* sec = (uint8_t*)c->buf("resp_secret", off);
  if (!sec) {
    c->fail("%s: device allocation failed (%zu bytes)", who, off);
    return FSDKR_E_OOM;
  }
  hipStream_t st = c->stream;
  auto run = [&]() -> int {
    int rc;
    if ((rc = c->hip_check(hipMemsetAsync(sec, 0, off, st), "memset resp")) ||
        (rc = c->hip_check(hipMemcpyAsync(sec + o_e, e, C * kProveELimbs * 4, hipMemcpyHostToDevice, st), "H2D resp")) ||
        (rc = c->hip_check(hipMemcpyAsync(sec + o_x, x, C * xl * 4, hipMemcpyHostToDevice, st), "H2D resp")) ||
        (rc = c->hip_check(hipMemcpyAsync(sec + o_y, y, C * yl * 4, hipMemcpyHostToDevice, st), "H2D resp")))
      return rc;
    RespCtArgs ra{(const uint32_t*)(sec + o_e), (const uint32_t*)(sec + o_x), (const uint32_t*)(sec + o_y),
                  (uint32_t*)(sec + o_o), xl, yl, ol, (uint32_t)Cp};
    const size_t m = c->tbeg("prove_resp", st);
    rc = c->hip_check(launch_resp_ct(ra, st), "resp_ct launch");
    c->tend(m, st);
    if (rc) return rc;
    return c->hip_check(hipMemcpyAsync(out, sec + o_o, C * ol * 4, hipMemcpyDeviceToHost, st), "D2H resp");
  };
  const int rc = run();
  const int rs = scrub(c, "resp_secret");
  const int ry = c->sync();
  return rc ? rc : rs ? rs : ry;
}

int fsdkr_bob_prove(fsdkr_ctx* ctx, const fsdkr_bob_prove_batch* b, fsdkr_bob_proofs* o) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return FSDKR_E_ARG;
  const char* who = "fsdkr_bob_prove";
  if (!b) {
    c->fail("%s: null batch", who);
    return FSDKR_E_ARG;
  }
  const uint32_t count = b->count, nk = b->n_keys, nl = b->nl, nn = 2 * b->nl;
  if (nl != 64 && nl != 96) {
    c->fail("%s: unsupported modulus width %u limbs", who, nl);
    return FSDKR_E_UNSUPPORTED;
  }
  if (count == 0) return FSDKR_OK;
  if (!o || !nk || !b->N || !b->Ntilde || !b->h1 || !b->h2 || !b->key_idx || !b->a_enc || !b->mta || !b->b ||
      !b->beta_prim || !b->r || !b->alpha || !b->beta || !b->gamma || !b->gamma_mod_n || !b->ro || !b->ro_prim ||
      !b->sigma || !b->tau || !o->z || !o->t || !o->s || !o->e || !o->s1 || !o->s2 || !o->t1 || !o->t2) {
    c->fail("%s: null pointer", who);
    return FSDKR_E_ARG;
  }
  int rc;
  if ((rc = check_keys(c, who, nl, count, nk, b->N, b->Ntilde, b->h1, b->h2, b->key_idx))) return rc;
  // a_enc is public: an unreduced one is refused here, before any secret row is uploaded
  // (the v stage would refuse it too, but only after the comb has run)
  {
    std::vector<uint32_t> NN((size_t)nk * nn);
    for (uint32_t k = 0; k < nk; ++k) {
      const hbn::Limbs Nv = hbn::from(b->N + (size_t)k * nl, nl);
      hbn::store(hbn::mul(Nv, Nv), &NN[(size_t)k * nn], nn);
    }
    for (uint32_t p = 0; p < count; ++p)
      if (hbn::cmp_raw(b->a_enc + (size_t)p * nn, nn, &NN[(size_t)b->key_idx[p] * nn], nn) >= 0) {
        c->fail("%s: a_enc[%u] is not reduced modulo N^2", who, p);
        return FSDKR_E_ARG;
      }
  }
  const BobWidths w = bob_widths(nl);
  const size_t C = count;
  // round 1: z = h1^b h2^ro, z' = h1^alpha h2^ro', t = h1^beta' h2^sigma, w = h1^gamma h2^tau
  std::vector<uint32_t> hx(4 * C * w.xl), hy(4 * C * w.yl), k4(4 * C), cm(4 * C * nl);
  interleave_rows(hx.data(), w.xl, 4, 0, b->b, w.b, count);
  interleave_rows(hx.data(), w.xl, 4, 1, b->alpha, w.alpha, count);
  interleave_rows(hx.data(), w.xl, 4, 2, b->beta_prim, w.beta_prim, count);
  interleave_rows(hx.data(), w.xl, 4, 3, b->gamma, w.gamma, count);
  interleave_rows(hy.data(), w.yl, 4, 0, b->ro, w.ro, count);
  interleave_rows(hy.data(), w.yl, 4, 1, b->ro_prim, w.ro_prim, count);
  interleave_rows(hy.data(), w.yl, 4, 2, b->sigma, w.sigma, count);
  interleave_rows(hy.data(), w.yl, 4, 3, b->tau, w.tau, count);
  repeat_keys(k4.data(), b->key_idx, 4, count);
  rc = pedersen_commit_ct_run(c, who, nl, 4 * count, hx.data(), w.xl, hy.data(), w.yl, k4.data(), b->Ntilde, b->h1, b->h2,
                              nk, cm.data());
  wipe(hx);
  wipe(hy);
  if (rc) return rc;
  // v = a_enc^alpha (1 + gamma N) beta^N mod N^2 (a_enc unreduced: FSDKR_E_ARG there)
  std::vector<uint32_t> v(C * nn);
  if ((rc = mta_respond_impl(c, who, nl, count, b->a_enc, b->alpha, b->gamma_mod_n, b->beta, b->key_idx, b->N, nk, v.data(),
                             true, kBobVLimbs)))
    return rc;
  std::vector<uint32_t> zp(C * nl), wv(C * nl);
  take_rows(o->z, cm.data(), nl, 4, 0, count);
  take_rows(zp.data(), cm.data(), nl, 4, 1, count);
  take_rows(o->t, cm.data(), nl, 4, 2, count);
  take_rows(wv.data(), cm.data(), nl, 4, 3, count);
  const PubRows pub[7] = {{b->a_enc, nn}, {b->mta, nn}, {o->z, nl}, {zp.data(), nl}, {o->t, nl}, {v.data(), nn}, {wv.data(), nl}};
  const RespJob jobs[4] = {{b->b, w.b, b->alpha, w.alpha, o->s1},
                           {b->ro, w.ro, b->ro_prim, w.ro_prim, o->s2},
                           {b->beta_prim, w.beta_prim, b->gamma, w.gamma, o->t1},
                           {b->sigma, w.sigma, b->tau, w.tau, o->t2}};
  return prove_round2(c, who, true, nl, count, nk, b->N, b->key_idx, pub, b->r, b->beta, jobs, o->e, o->s);
}

int fsdkr_alice_prove(fsdkr_ctx* ctx, const fsdkr_alice_prove_batch* b, fsdkr_alice_proofs* o) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return FSDKR_E_ARG;
  const char* who = "fsdkr_alice_prove";
  if (!b) {
    c->fail("%s: null batch", who);
    return FSDKR_E_ARG;
  }
  const uint32_t count = b->count, nk = b->n_keys, nl = b->nl, nn = 2 * b->nl;
  if (nl != 64 && nl != 96) {
    c->fail("%s: unsupported modulus width %u limbs", who, nl);
    return FSDKR_E_UNSUPPORTED;
  }
  if (count == 0) return FSDKR_OK;
  if (!o || !nk || !b->N || !b->Ntilde || !b->h1 || !b->h2 || !b->key_idx || !b->cipher || !b->a || !b->r || !b->alpha ||
      !b->beta || !b->gamma || !b->ro || !o->z || !o->s || !o->e || !o->s1 || !o->s2) {
    c->fail("%s: null pointer", who);
    return FSDKR_E_ARG;
  }
  int rc;
  if ((rc = check_keys(c, who, nl, count, nk, b->N, b->Ntilde, b->h1, b->h2, b->key_idx))) return rc;
  const AliceWidths w = alice_widths(nl);
  const size_t C = count;
  // round 1: z = h1^a h2^ro, w = h1^alpha h2^gamma
  std::vector<uint32_t> hx(2 * C * w.xl), hy(2 * C * w.yl), k2(2 * C), cm(2 * C * nl);
  interleave_rows(hx.data(), w.xl, 2, 0, b->a, w.a, count);
  interleave_rows(hx.data(), w.xl, 2, 1, b->alpha, w.alpha, count);
  interleave_rows(hy.data(), w.yl, 2, 0, b->ro, w.ro, count);
  interleave_rows(hy.data(), w.yl, 2, 1, b->gamma, w.gamma, count);
  repeat_keys(k2.data(), b->key_idx, 2, count);
  rc = pedersen_commit_ct_run(c, who, nl, 2 * count, hx.data(), w.xl, hy.data(), w.yl, k2.data(), b->Ntilde, b->h1, b->h2,
                              nk, cm.data());
  wipe(hx);
  wipe(hy);
  if (rc) return rc;
  // u = (1 + alpha N) beta^N mod N^2: the chain of v with a_enc = 1 and exponent rows of zero
  std::vector<uint32_t> u(C * nn), ones(C * nn, 0u), zero(C * kBobVLimbs, 0u), al(C * nl, 0u);
  for (uint32_t p = 0; p < count; ++p) {
    ones[(size_t)p * nn] = 1u;
    memcpy(&al[(size_t)p * nl], b->alpha + (size_t)p * w.alpha, (size_t)std::min(w.alpha, nl) * 4);
  }
  rc = mta_respond_impl(c, who, nl, count, ones.data(), zero.data(), al.data(), b->beta, b->key_idx, b->N, nk, u.data(), true,
                        kBobVLimbs);
  wipe(al);
  if (rc) return rc;
  std::vector<uint32_t> wv(C * nl);
  take_rows(o->z, cm.data(), nl, 2, 0, count);
  take_rows(wv.data(), cm.data(), nl, 2, 1, count);
  const PubRows pub[4] = {{b->cipher, nn}, {o->z, nl}, {u.data(), nn}, {wv.data(), nl}};
  const RespJob jobs[2] = {{b->a, w.a, b->alpha, w.alpha, o->s1}, {b->ro, w.ro, b->gamma, w.gamma, o->s2}};
  return prove_round2(c, who, false, nl, count, nk, b->N, b->key_idx, pub, b->r, b->beta, jobs, o->e, o->s);
}

}  // extern "C"
