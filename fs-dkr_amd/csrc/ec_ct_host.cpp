// C ABI of the secret-scalar secp256k1 entry points (ec_ct.hip): the comb table
// of G (public data, built once per process on the host with OpenSSL and kept
// in a context buffer), the padded launches and the scrub of every device
// buffer that held a scalar.
#include <hip/hip_runtime.h>
#include <openssl/bn.h>
#include <openssl/ec.h>
#include <openssl/obj_mac.h>

#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "fsdkr/fsdkr.h"
#include "verify.h"

using namespace fsdkr;

namespace {

// T[i][d] = (d + 1) 16^i G for i < 64, d < 16, then -C with
// C = sum_i 16^i G = ((16^64 - 1) / 15) G: kEcCombEntries affine points of 16
// limbs.  Empty on an OpenSSL failure.
std::vector<uint32_t> build_comb() {
  std::vector<uint32_t> tab((size_t)kEcCombEntries * 16, 0u);
  EC_GROUP* grp = EC_GROUP_new_by_curve_name(NID_secp256k1);
  BN_CTX* bc = BN_CTX_new();
  BIGNUM *x = BN_new(), *y = BN_new();
  EC_POINT *B = grp ? EC_POINT_new(grp) : nullptr, *T = grp ? EC_POINT_new(grp) : nullptr,
           *C = grp ? EC_POINT_new(grp) : nullptr;
  bool ok = grp && bc && x && y && B && T && C;
  auto put = [&](const EC_POINT* p, size_t at) {   // every stored point is finite
    uint8_t xb[32], yb[32];
    if (EC_POINT_is_at_infinity(grp, p) || EC_POINT_get_affine_coordinates(grp, p, x, y, bc) != 1 ||
        BN_bn2lebinpad(x, xb, 32) != 32 || BN_bn2lebinpad(y, yb, 32) != 32)
      return false;
    std::memcpy(tab.data() + at * 16, xb, 32);
    std::memcpy(tab.data() + at * 16 + 8, yb, 32);
    return true;
  };
  ok = ok && EC_POINT_copy(B, EC_GROUP_get0_generator(grp)) == 1 && EC_POINT_set_to_infinity(grp, C) == 1;
  for (size_t i = 0; ok && i < 64; ++i) {
    ok = EC_POINT_add(grp, C, C, B, bc) == 1 && EC_POINT_copy(T, B) == 1;
    for (size_t d = 0; ok && d < 16; ++d) {
      ok = put(T, i * 16 + d);
      if (ok && d < 15) ok = EC_POINT_add(grp, T, T, B, bc) == 1;
    }
    ok = ok && EC_POINT_copy(B, T) == 1;   // 16^(i+1) G
  }
  ok = ok && EC_POINT_invert(grp, C, bc) == 1 && put(C, 64 * 16);
  EC_POINT_free(B);
  EC_POINT_free(T);
  EC_POINT_free(C);
  BN_free(x);
  BN_free(y);
  BN_CTX_free(bc);
  EC_GROUP_free(grp);
  if (!ok) tab.clear();
  return tab;
}

// the context's device copy of the comb table (uploaded on first use)
int comb_table(Ctx* c, const uint32_t** d_tab) {
  static const std::vector<uint32_t> tab = build_comb();   // outlives every upload
  if (tab.empty()) {
    c->fail("fsdkr_ec_mul_g_ct: comb table build failed");
    return FSDKR_E_ARG;
  }
  const auto it = c->bufs.find("ec_comb");
  if (it != c->bufs.end() && it->second.ptr) {
    *d_tab = (const uint32_t*)it->second.ptr;
    return FSDKR_OK;
  }
  void* d = c->buf("ec_comb", tab.size() * 4);
  if (!d) return FSDKR_E_OOM;
  *d_tab = (const uint32_t*)d;
  const int rc = c->hip_check(hipMemcpyAsync(d, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, c->stream),
                              "H2D comb");
  if (rc) {   // not cached: the next call uploads again
    (void)hipFree(d);
    c->bufs.erase("ec_comb");
  }
  return rc;
}

inline size_t round_up(size_t n, size_t m) { return (n + m - 1) / m * m; }

}  // namespace

extern "C" {

int fsdkr_ec_mul_g_ct(fsdkr_ctx* ctx, uint32_t count, const uint32_t* scalars, uint32_t* out) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c || !scalars || !out) return FSDKR_E_ARG;
  if (count == 0) return FSDKR_OK;
  StreamScope scope(c, c->aux_stream());   // overlaps a launched collect batch
  PrioScope prio(c, 3);
  const size_t pad = round_up(count, kEcMulGPad);
  const size_t sc_bytes = pad * 32, out_bytes = pad * 64;
  uint8_t* d = (uint8_t*)c->buf("ecg_ct", sc_bytes + out_bytes);
  if (!d) return FSDKR_E_OOM;
  uint32_t* d_sc = (uint32_t*)d;
  uint32_t* d_out = (uint32_t*)(d + sc_bytes);
  const uint32_t* d_tab = nullptr;
  int rc;
  if ((rc = comb_table(c, &d_tab))) return rc;
  // the padding lanes multiply by zero: whole waves, no bound check in the kernel
  rc = c->hip_check(hipMemsetAsync(d_sc, 0, sc_bytes, c->stream), "memset sc");
  if (!rc)
    rc = c->hip_check(hipMemcpyAsync(d_sc, scalars, (size_t)count * 32, hipMemcpyHostToDevice, c->stream), "H2D sc");
  if (!rc) {
    EcMulGCtArgs a{d_tab, d_sc, d_out, (uint32_t)pad};
    c->mark("ec_ct", true);
    rc = c->hip_check(launch_ec_mul_g_ct(a, c->stream), "ec_mul_g_ct");
    c->mark("ec_ct", false);
  }
  if (!rc)
    rc = c->hip_check(hipMemcpyAsync(out, d_out, (size_t)count * 64, hipMemcpyDeviceToHost, c->stream), "D2H");
  // scrub the secret scalars whatever happened to the uploads and the launch
  const int rs = c->hip_check(hipMemsetAsync(d_sc, 0, sc_bytes, c->stream), "scrub sc");
  const int ry = c->sync();
  return rc ? rc : rs ? rs : ry;
}

int fsdkr_ec_msm_ct(fsdkr_ctx* ctx, uint32_t count, uint32_t terms, const uint32_t* points, const uint32_t* scalars,
                    uint32_t* out) {
  Ctx* c = reinterpret_cast<Ctx*>(ctx);
  if (!c || !points || !scalars || !out || terms == 0) return FSDKR_E_ARG;
  if (count == 0) return FSDKR_OK;
  StreamScope scope(c, c->aux_stream());   // overlaps a launched collect batch
  PrioScope prio(c, 3);
  const size_t pad = round_up(count, kEcMsmCtPad);
  if (pad * terms > 0xffffffffull / 24) {   // 32-bit thread and scratch indices
    c->fail("fsdkr_ec_msm_ct: %u x %u terms exceed one launch", count, terms);
    return FSDKR_E_ARG;
  }
  const size_t np = (size_t)count * terms, npad = pad * terms;
  const size_t pt_bytes = npad * 64, sc_bytes = npad * 32, out_bytes = pad * 64, scr_bytes = npad * 96;
  uint8_t* d = (uint8_t*)c->buf("msm_ct", pt_bytes + sc_bytes + out_bytes + scr_bytes);
  if (!d) return FSDKR_E_OOM;
  uint32_t* d_pts = (uint32_t*)d;
  uint32_t* d_sc = (uint32_t*)(d + pt_bytes);
  uint32_t* d_out = (uint32_t*)(d + pt_bytes + sc_bytes);
  uint32_t* d_scr = (uint32_t*)(d + pt_bytes + sc_bytes + out_bytes);
  int rc;
  // the padding terms are 0 * infinity: whole waves, no bound check in the kernels
  rc = c->hip_check(hipMemsetAsync(d, 0, pt_bytes + sc_bytes, c->stream), "memset msm_ct");
  if (!rc) rc = c->hip_check(hipMemcpyAsync(d_pts, points, np * 64, hipMemcpyHostToDevice, c->stream), "H2D pts");
  if (!rc) rc = c->hip_check(hipMemcpyAsync(d_sc, scalars, np * 32, hipMemcpyHostToDevice, c->stream), "H2D sc");
  if (!rc) {
    EcMsmCtArgs a{d_pts, d_sc, terms, d_out, (uint32_t)pad, d_scr};
    c->mark("ec_ct", true);
    rc = c->hip_check(launch_ec_msm_ct(a, c->stream), "ec_msm_ct");
    c->mark("ec_ct", false);
  }
  if (!rc)
    rc = c->hip_check(hipMemcpyAsync(out, d_out, (size_t)count * 64, hipMemcpyDeviceToHost, c->stream), "D2H");
  // scrub the secret scalars and the per-term products k_j P_j
  int rs = c->hip_check(hipMemsetAsync(d_sc, 0, sc_bytes, c->stream), "scrub sc");
  if (!rs) rs = c->hip_check(hipMemsetAsync(d_scr, 0, scr_bytes, c->stream), "scrub terms");
  const int ry = c->sync();
  return rc ? rc : rs ? rs : ry;
}

}  // extern "C"
