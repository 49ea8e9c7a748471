// fsdkr_pedersen_commit_ct of the C ABI (include/fsdkr/fsdkr.h): h1^x h2^y mod N~
// for secret x, y as ONE constant-time comb per commitment (comb_ct.hip).
// Per call: the chains P_m = base^(2^(m b)) of every key's h1 and h2
// (fb_table_kernel, window b), the 16-row tables of both bases (comb_build_kernel),
// the digit schedules of x and y (comb_sched_kernel) and commit_ct_kernel.  The
// geometry (b, v_x, v_y) comes from the limb counts and the instances per key
// alone: no exponent value or bit length is looked at on the host or the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "commit_geom.hpp"
#include "ctx.hpp"
#include "fbjob.hpp"
#include "fixedbase.h"
#include "fsdkr/fsdkr.h"
#include "hostbn.hpp"
#include "kernels.h"
#include "mta_host.hpp"

using namespace fsdkr;

extern "C" int fsdkr_pedersen_commit_ct(fsdkr_ctx* ctx, uint32_t nl, uint32_t count, const uint32_t* x, uint32_t xl,
                                        const uint32_t* y, uint32_t yl, const uint32_t* key_idx,
                                        const uint32_t* Ntilde, const uint32_t* h1, const uint32_t* h2,
                                        uint32_t n_keys, uint32_t* out) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c) return FSDKR_E_ARG;
  return pedersen_commit_ct_run(c, "fsdkr_pedersen_commit_ct", nl, count, x, xl, y, yl, key_idx, Ntilde, h1, h2, n_keys,
                                out);
}

// the whole stage, shared with the provers of mta_prove.cpp (mta_host.hpp)
int fsdkr::pedersen_commit_ct_run(Ctx* c, const char* who, uint32_t nl, uint32_t count, const uint32_t* x, uint32_t xl,
                                  const uint32_t* y, uint32_t yl, const uint32_t* key_idx, const uint32_t* Ntilde,
                                  const uint32_t* h1, const uint32_t* h2, uint32_t n_keys, uint32_t* out) {
  if (nl != 64 && nl != 96) {
    c->fail("%s: unsupported modulus width %u limbs", who, nl);
    return FSDKR_E_UNSUPPORTED;
  }
  if (count == 0) return FSDKR_OK;
  if (!x || !y || !key_idx || !Ntilde || !h1 || !h2 || !out || !n_keys || xl < 1 || xl > 128 || yl < 1 || yl > 128) {
    c->fail("%s: bad argument", who);
    return FSDKR_E_ARG;
  }
  if (c->modexp_group != 0 && c->modexp_group != (uint32_t)kCommitLanes) {
    c->fail("%s: the comb runs at %d lanes (forced %u)", who, kCommitLanes, c->modexp_group);
    return FSDKR_E_ARG;
  }
  const uint32_t nk = n_keys;
  for (uint32_t k = 0; k < nk; ++k) {
    const uint32_t* Nt = Ntilde + (size_t)k * nl;
    if (!(Nt[0] & 1u) || bit_len(Nt, nl) < 2) {
      c->fail("%s: key %u: Ntilde must be odd and above 1", who, k);
      return FSDKR_E_ARG;
    }
    // the bases are public: an unreduced one is refused, not silently reduced
    if (hbn::cmp_raw(h1 + (size_t)k * nl, nl, Nt, nl) >= 0 || hbn::cmp_raw(h2 + (size_t)k * nl, nl, Nt, nl) >= 0) {
      c->fail("%s: key %u: h1, h2 must be below Ntilde", who, k);
      return FSDKR_E_ARG;
    }
  }
  std::vector<uint32_t> per(nk, 0u);
  for (uint32_t p = 0; p < count; ++p) {
    if (key_idx[p] >= nk) {
      c->fail("%s: key_idx[%u] out of range", who, p);
      return FSDKR_E_ARG;
    }
    ++per[key_idx[p]];
  }
  // ---- geometry and launch order -------------------------------------------------
  const size_t KD = (size_t)shape_digits(nl), C = count, rl = (size_t)nl * 4;
  const uint32_t b = commit_choose_b(xl, yl, (double)count / nk, nk, KD * 4, comb_mem_cap(c));
  if (!b) {
    c->fail("%s: the tables of %u keys do not fit the device", who, nk);
    return FSDKR_E_OOM;
  }
  const uint32_t vx = (8 * xl + b - 1) / b, vy = (8 * yl + b - 1) / b;
  const uint32_t ipb = commit_ct_ipb(commit_padded_lanes(per.data(), nk));
  // a key's run, padded to whole blocks; keys without instances take no block
  std::vector<uint32_t> start(nk + 1, 0u), blk_key;
  for (uint32_t k = 0; k < nk; ++k) {
    const uint32_t nb = (per[k] + ipb - 1) / ipb;
    start[k + 1] = start[k] + nb * ipb;
    blk_key.insert(blk_key.end(), nb, k);
  }
  const size_t n = start[nk], blocks = blk_key.size();
  std::vector<uint32_t> out_idx(n, count);   // pads write the scratch row
  std::vector<uint32_t> hx(n * xl, 0u), hy(n * yl, 0u), fill(start.begin(), start.end() - 1);
  for (uint32_t p = 0; p < count; ++p) {
    const size_t r = fill[key_idx[p]]++;
    out_idx[r] = p;
    memcpy(&hx[r * xl], x + (size_t)p * xl, (size_t)xl * 4);
    memcpy(&hy[r * yl], y + (size_t)p * yl, (size_t)yl * 4);
  }
  CombParams px, py;
  px.h = py.h = 4;
  px.b = py.b = b;
  px.v = vx;
  py.v = vy;
  CombJob jx, jy;
  jx.init(px, nl, nk, (uint32_t)n);
  jy.init(py, nl, nk, (uint32_t)n);
  const uint32_t ex = 4 * vx, ey = 4 * vy;   // chain entries per base
  // ---- device images: public (keys, descriptors, chains, tables, results) and secret --
  size_t off = 0;
  auto take = [&](size_t bytes) { const size_t o = off; off = al256(off + (bytes ? bytes : 1)); return o; };
  const size_t o_Nt = take(nk * rl), o_h = take(2 * nk * rl);
  const size_t o_bptr = take(2 * nk * 8), o_blen = take(2 * nk * 4), o_bmod = take(2 * nk * 4), o_toff = take(2 * nk * 4),
               o_bh = take(2 * nk * 4), o_ul = take(jx.ulist.size() * 2);
  const size_t o_epx = take(n * 8), o_epy = take(n * 8), o_elx = take(n * 4), o_ely = take(n * 4);
  const size_t o_bk = take(blocks * 4), o_oi = take(n * 4);
  const size_t desc_end = off;
  const size_t o_chain = take((size_t)nk * (ex + ey) * KD * 4), o_tx = take(jx.table_bytes()), o_ty = take(jy.table_bytes());
  const size_t o_out = take((C + 1) * rl);
  const size_t pub_bytes = off;
  off = 0;
  const size_t o_x = take(n * xl * 4), o_y = take(n * yl * 4);
  const size_t o_sx = take(jx.sched_bytes() + 256), o_sy = take(jy.sched_bytes() + 256);
  const size_t sec_bytes = off;
  uint8_t* dev = (uint8_t*)c->buf("commit_io", pub_bytes);
  uint8_t* sec = (uint8_t*)c->buf("commit_secret", sec_bytes);
  if (!dev || !sec) {
    c->fail("%s: device allocation failed (%zu bytes)", who, pub_bytes + sec_bytes);
    return FSDKR_E_OOM;
  }
  auto DA = [&](const uint8_t* base, size_t o) { return (uint64_t)(uintptr_t)(base + o); };
  auto U32 = [&](size_t o) { return reinterpret_cast<uint32_t*>(dev + o); };
  std::vector<uint8_t> img(desc_end, 0);
  memcpy(&img[o_Nt], Ntilde, nk * rl);
  memcpy(&img[o_h], h1, nk * rl);
  memcpy(&img[o_h + nk * rl], h2, nk * rl);
  {
    auto* bptr = reinterpret_cast<uint64_t*>(&img[o_bptr]);
    auto *blen = reinterpret_cast<uint32_t*>(&img[o_blen]), *bmod = reinterpret_cast<uint32_t*>(&img[o_bmod]),
         *toff = reinterpret_cast<uint32_t*>(&img[o_toff]), *bh = reinterpret_cast<uint32_t*>(&img[o_bh]);
    for (uint32_t q = 0; q < 2 * nk; ++q) {   // bases [h1_k | h2_k]
      const bool isx = q < nk;
      bptr[q] = DA(dev, o_h + (size_t)q * rl);
      blen[q] = nl;
      bmod[q] = isx ? q : q - nk;
      toff[q] = isx ? q * ex : nk * ex + (q - nk) * ey;
      bh[q] = isx ? ex : ey;
    }
    memcpy(&img[o_ul], jx.ulist.data(), jx.ulist.size() * 2);
    auto *epx = reinterpret_cast<uint64_t*>(&img[o_epx]), *epy = reinterpret_cast<uint64_t*>(&img[o_epy]);
    auto *elx = reinterpret_cast<uint32_t*>(&img[o_elx]), *ely = reinterpret_cast<uint32_t*>(&img[o_ely]);
    for (size_t i = 0; i < n; ++i) {
      epx[i] = DA(sec, o_x + i * xl * 4);
      epy[i] = DA(sec, o_y + i * yl * 4);
      elx[i] = xl;
      ely[i] = yl;
    }
    memcpy(&img[o_bk], blk_key.data(), blocks * 4);
    memcpy(&img[o_oi], out_idx.data(), n * 4);
  }
  hipStream_t st = c->stream;
  auto run = [&]() -> int {
    int rc;
    if ((rc = c->hip_check(hipMemcpyAsync(dev, img.data(), img.size(), hipMemcpyHostToDevice, st), "H2D commit")) ||
        (rc = c->hip_check(hipMemcpyAsync(sec + o_x, hx.data(), n * xl * 4, hipMemcpyHostToDevice, st), "H2D commit")) ||
        (rc = c->hip_check(hipMemcpyAsync(sec + o_y, hy.data(), n * yl * 4, hipMemcpyHostToDevice, st), "H2D commit")))
      return rc;
    uint32_t* cons = nullptr;
    if ((rc = setup_moduli(c, nl, U32(o_Nt), nk, &cons, "commit"))) return rc;
    // schedules (they need only the exponents), chains, tables
    CombSchedArgs sx{(const uint64_t*)(dev + o_epx), U32(o_elx), (uint16_t*)(sec + o_sx), 4, vx, b, (uint32_t)n};
    CombSchedArgs sy{(const uint64_t*)(dev + o_epy), U32(o_ely), (uint16_t*)(sec + o_sy), 4, vy, b, (uint32_t)n};
    size_t m = c->tbeg("commit_sched", st);
    if (!(rc = c->hip_check(launch_comb_sched(sx, st), "comb_sched launch")))
      rc = c->hip_check(launch_comb_sched(sy, st), "comb_sched launch");
    c->tend(m, st);
    if (rc) return rc;
    uint32_t* chain = U32(o_chain);
    FbTableArgs ta{(const uint64_t*)(dev + o_bptr), U32(o_blen), U32(o_bmod), U32(o_toff), U32(o_bh), cons, chain, b,
                   2 * nk, 0};
    m = c->tbeg("commit_tables", st);
    rc = c->hip_check(launch_fb_table(nl, ta, st), "commit chain launch");
    if (!rc) {
      CombDev dx{U32(o_toff), U32(o_bmod), nullptr, nullptr, nullptr, nullptr, nullptr,
                 reinterpret_cast<const uint16_t*>(dev + o_ul), U32(o_tx), nullptr};
      CombDev dy = dx;
      dy.ptoff = U32(o_toff) + nk;
      dy.bmod = U32(o_bmod) + nk;
      dy.comb = U32(o_ty);
      if (!(rc = comb_build_launch(c, jx, dx, chain, cons, st))) rc = comb_build_launch(c, jy, dy, chain, cons, st);
    }
    c->tend(m, st);
    if (rc) return rc;
    CommitCtArgs ca{U32(o_tx), U32(o_ty), (const uint16_t*)(sec + o_sx), (const uint16_t*)(sec + o_sy), U32(o_bk),
                    U32(o_oi), cons, U32(o_out), vx, vy, b, ipb, (uint32_t)blocks};
    m = c->tbeg("commit_ct", st);
    rc = c->hip_check(launch_commit_ct(nl, ca, st), "commit_ct launch");
    c->tend(m, st);
    if (rc) return rc;
    return c->hip_check(hipMemcpyAsync(out, dev + o_out, C * rl, hipMemcpyDeviceToHost, st), "D2H commit");
  };
  const int rc = run();
  // scrub what held x, y or their digit schedules; then the host staging rows
  const int rs = scrub(c, "commit_secret");
  const int ry = c->sync();
  wipe(hx);
  wipe(hy);
  return rc ? rc : rs ? rs : ry;
}
