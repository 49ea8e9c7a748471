// Branch-free secp256k1 field / group layer for SECRET scalars (gfx950).
//
// Replaces libsecp256k1's constant-time secp256k1_ecmult_gen behind curv
// `Point::generator() * Scalar` on the prover side (refresh_message.rs:51-145,
// zk_pdl_with_slack.rs:53-111, range_proofs.rs:480-484).  secp256k1.hpp keeps
// serving the public-scalar kernels of collect(); nothing here changes it.
//
// Field elements are secp256k1.hpp's Fe (8 little-endian u32 limbs, fully
// reduced).  Its fe_add / fe_sub / fe_mul all end in `if (carry)` /
// `if (fe_ge_p(r))` corrections, so none of them is reused: every reduction
// here computes both candidates and keeps one through an arithmetic mask
// (m = 0u - bit; r = (a & m) | (b & ~m)).  Only its plain data movers
// (fe_load, fe_set_u32) and constants are shared.
//
// Points are homogeneous projective (X : Y : Z) on y^2 z = x^3 + 7 z^3, the
// identity is (0 : 1 : 0).  The group has prime order, so the complete
// formulas of Renes, Costello and Batina (EUROCRYPT 2016, a = 0, b3 = 21) hold
// for every pair of inputs: P + P, P + (-P) and the identity on either side
// take the same instructions as any other sum.
#pragma once
#include "secp256k1.hpp"

namespace fsdkr {
namespace ec {

// r = (a & m) | (b & ~m), m = 0 or ~0
EC_D void fe_select_ct(Fe& r, const Fe& a, const Fe& b, uint32_t m) {
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = (a.v[i] & m) | (b.v[i] & ~m);
}

// r + cc 2^256 (cc = 0 or 1, value < 2p) -> fully reduced
EC_D void fe_tail_ct(Fe& r, uint32_t cc) {
  // t = r + 2^32 + 977 (mod 2^256) = value - p when the value is >= p
  Fe t;
  uint64_t c = (uint64_t)r.v[0] + 977u;
  t.v[0] = (uint32_t)c;
  c = (c >> 32) + (uint64_t)r.v[1] + 1u;
  t.v[1] = (uint32_t)c;
  c >>= 32;
#pragma unroll
  for (int i = 2; i < 8; ++i) {
    c += r.v[i];
    t.v[i] = (uint32_t)c;
    c >>= 32;
  }
  // a carry out of t <=> r >= p; cc set <=> the value passed 2^256
  const uint32_t m = 0u - (cc | (uint32_t)c);
  fe_select_ct(r, t, r, m);
}

EC_D void fe_add_ct(Fe& r, const Fe& a, const Fe& b) {
  uint64_t c = 0;
  Fe s;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)a.v[i] + b.v[i];
    s.v[i] = (uint32_t)c;
    c >>= 32;
  }
  fe_tail_ct(s, (uint32_t)c);
  r = s;
}

EC_D void fe_sub_ct(Fe& r, const Fe& a, const Fe& b) {
  int64_t br = 0;
  uint32_t t[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int64_t d = (int64_t)a.v[i] - b.v[i] + br;
    t[i] = (uint32_t)d;
    br = d >> 32;
  }
  const uint32_t m = (uint32_t)br;   // 0 or ~0: add p back under the mask
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)t[i] + (P_LIMBS[i] & m);
    r.v[i] = (uint32_t)c;
    c >>= 32;
  }
}

// r = a * k mod p for a small constant k (3, 8, 21)
EC_D void fe_mul_small_ct(Fe& r, const Fe& a, uint32_t k) {
  uint64_t c = 0;
  Fe s;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)a.v[i] * k;
    s.v[i] = (uint32_t)c;
    c >>= 32;
  }
  // fold h 2^256 = h (2^32 + 977), h < k
  const uint64_t h = c;
  c = (uint64_t)s.v[0] + h * 977u;
  s.v[0] = (uint32_t)c;
  c = (c >> 32) + (uint64_t)s.v[1] + h;
  s.v[1] = (uint32_t)c;
  c >>= 32;
#pragma unroll
  for (int i = 2; i < 8; ++i) {
    c += s.v[i];
    s.v[i] = (uint32_t)c;
    c >>= 32;
  }
  fe_tail_ct(s, (uint32_t)c);
  r = s;
}

// r = a * b mod p: secp256k1.hpp's product scanning and two folds, with the
// last wrap and the final subtraction masked
EC_D void fe_mul_ct(Fe& r, const Fe& a, const Fe& b) {
  uint32_t t[16];
  uint64_t acc = 0;
  uint32_t acc_hi = 0;
#pragma unroll
  for (int col = 0; col < 15; ++col) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = col - i;
      if (j < 0 || j > 7) continue;   // compile-time indices
      const uint64_t p = (uint64_t)a.v[i] * b.v[j];
      const uint64_t s = acc + p;
      acc_hi += (uint32_t)(s < acc);
      acc = s;
    }
    t[col] = (uint32_t)acc;
    acc = (acc >> 32) | ((uint64_t)acc_hi << 32);
    acc_hi = 0;
  }
  t[15] = (uint32_t)acc;
  // u = L + H 977 + (H << 32)   (2^256 == 2^32 + 977 mod p)
  uint32_t u[10];
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    uint64_t s = c;
    if (i < 8) s += t[i];
    if (i < 8) s += (uint64_t)t[8 + i] * 977u;
    if (i >= 1 && i <= 8) s += t[8 + i - 1];
    u[i] = (uint32_t)s;
    c = s >> 32;
  }
  // second fold of u[8..9] (< 2^34)
  const uint64_t h = ((uint64_t)u[9] << 32) | u[8];
  Fe s;
  uint64_t s0 = (uint64_t)u[0] + (h & 0xFFFFFFFFu) * 977u;
  s.v[0] = (uint32_t)s0;
  uint64_t s1 = (s0 >> 32) + (uint64_t)u[1] + (h >> 32) * 977u + (h & 0xFFFFFFFFu);
  s.v[1] = (uint32_t)s1;
  uint64_t s2 = (s1 >> 32) + (uint64_t)u[2] + (h >> 32);
  s.v[2] = (uint32_t)s2;
  uint64_t cc = s2 >> 32;
#pragma unroll
  for (int i = 3; i < 8; ++i) {
    cc += u[i];
    s.v[i] = (uint32_t)cc;
    cc >>= 32;
  }
  // s + cc 2^256 < 2^256 + 2^67 < 2p: one masked correction covers the wrap and s >= p
  fe_tail_ct(s, (uint32_t)cc);
  r = s;
}

EC_D void fe_sqr_ct(Fe& r, const Fe& a) { fe_mul_ct(r, a, a); }

// a^(p-2) (Fermat) by the addition chain of libsecp256k1's field inverse: 255
// squarings and 15 multiplications.  The exponent is public, so the chain is
// fixed; it runs as 15 steps "square n times, multiply by a kept power" with
// one squaring and one product body, the step's operand picked by masks made
// from the step tables (x_k stands for a^(2^k - 1)).  Maps 0 to 0.
//   step      0   1   2   3   4    5    6    7    8     9    10   11 12 13 14
//   gives    x2  x3  x6  x9  x11  x22  x44  x88  x176  x220 x223  then the tail 0..0101101
__constant__ const uint8_t INV_NSQR[15] = {1, 1, 3, 3, 2, 11, 22, 44, 88, 44, 3, 23, 5, 3, 2};
// operand: 0 a, 1 x2, 2 x3, 3 x22, 4 x44, 5 the step's own input
__constant__ const uint8_t INV_OP[15] = {0, 0, 2, 2, 1, 5, 5, 5, 5, 4, 2, 3, 0, 1, 0};
// the result is kept as: 0 nothing, 1 x2, 2 x3, 3 x22, 4 x44
__constant__ const uint8_t INV_KEEP[15] = {1, 2, 0, 0, 0, 3, 4, 0, 0, 0, 0, 0, 0, 0, 0};

EC_D void fe_inv_ct(Fe& r, const Fe& a) {
  Fe x = a, x2 = a, x3 = a, x22 = a, x44 = a;
#pragma unroll 1
  for (int st = 0; st < 15; ++st) {
    const Fe in = x;
    const uint32_t n = INV_NSQR[st], op = INV_OP[st], keep = INV_KEEP[st];
#pragma unroll 1
    for (uint32_t i = 0; i < n; ++i) fe_sqr_ct(x, x);
    const uint32_t m0 = 0u - (uint32_t)(op == 0), m1 = 0u - (uint32_t)(op == 1), m2 = 0u - (uint32_t)(op == 2),
                   m3 = 0u - (uint32_t)(op == 3), m4 = 0u - (uint32_t)(op == 4), m5 = 0u - (uint32_t)(op == 5);
    Fe f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      f.v[i] = (a.v[i] & m0) | (x2.v[i] & m1) | (x3.v[i] & m2) | (x22.v[i] & m3) | (x44.v[i] & m4) | (in.v[i] & m5);
    fe_mul_ct(x, x, f);
    fe_select_ct(x2, x, x2, 0u - (uint32_t)(keep == 1));
    fe_select_ct(x3, x, x3, 0u - (uint32_t)(keep == 2));
    fe_select_ct(x22, x, x22, 0u - (uint32_t)(keep == 3));
    fe_select_ct(x44, x, x44, 0u - (uint32_t)(keep == 4));
  }
  r = x;
}

struct Proj {
  Fe X, Y, Z;
};

EC_D void proj_set_id(Proj& p) {
  fe_set_u32(p.X, 0);
  fe_set_u32(p.Y, 1);
  fe_set_u32(p.Z, 0);
}

// affine (x, y) -> (x : y : 1); the ABI's infinity (0, 0) -> (0 : 1 : 0) by mask
EC_D void proj_from_aff_ct(Proj& p, const Fe& x, const Fe& y) {
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) o |= x.v[i] | y.v[i];
  const uint32_t inf = (uint32_t)(((uint64_t)o - 1u) >> 63);   // 1 iff x == y == 0
  p.X = x;
  p.Y = y;
  p.Y.v[0] |= inf;
  fe_set_u32(p.Z, 1u ^ inf);
}

// the tail shared by the full and the mixed addition: from
//   xx = X1X2, yy = Y1Y2, zz0 = Z1Z2, s = X1Y2 + X2Y1, u = Y1Z2 + Y2Z1, w = X1Z2 + X2Z1
EC_D void proj_add_tail_ct(Proj& r, const Fe& xx, const Fe& yy, const Fe& zz0, const Fe& s, const Fe& u, const Fe& w) {
  Fe zz, xx3, w21, d, e, t0, t1;
  fe_mul_small_ct(zz, zz0, 21);
  fe_mul_small_ct(xx3, xx, 3);
  fe_mul_small_ct(w21, w, 21);
  fe_sub_ct(d, yy, zz);
  fe_add_ct(e, yy, zz);
  Proj o;
  fe_mul_ct(t0, s, d);
  fe_mul_ct(t1, u, w21);
  fe_sub_ct(o.X, t0, t1);          // X3 = s (yy - zz) - b3 u w
  fe_mul_ct(t0, e, d);
  fe_mul_ct(t1, xx3, w21);
  fe_add_ct(o.Y, t0, t1);          // Y3 = (yy + zz)(yy - zz) + b3 3xx w
  fe_mul_ct(t0, u, e);
  fe_mul_ct(t1, xx3, s);
  fe_add_ct(o.Z, t0, t1);          // Z3 = u (yy + zz) + 3xx s
  r = o;
}

// r = p + q, complete (12 products)
EC_D void proj_add_ct(Proj& r, const Proj& p, const Proj& q) {
  Fe xx, yy, zz0, s, u, w, a, b;
  fe_mul_ct(xx, p.X, q.X);
  fe_mul_ct(yy, p.Y, q.Y);
  fe_mul_ct(zz0, p.Z, q.Z);
  fe_add_ct(a, p.X, p.Y);
  fe_add_ct(b, q.X, q.Y);
  fe_mul_ct(s, a, b);
  fe_sub_ct(s, s, xx);
  fe_sub_ct(s, s, yy);
  fe_add_ct(a, p.Y, p.Z);
  fe_add_ct(b, q.Y, q.Z);
  fe_mul_ct(u, a, b);
  fe_sub_ct(u, u, yy);
  fe_sub_ct(u, u, zz0);
  fe_add_ct(a, p.X, p.Z);
  fe_add_ct(b, q.X, q.Z);
  fe_mul_ct(w, a, b);
  fe_sub_ct(w, w, xx);
  fe_sub_ct(w, w, zz0);
  proj_add_tail_ct(r, xx, yy, zz0, s, u, w);
}

// r = p + (x2 : y2 : 1), complete for a finite (x2, y2) (11 products)
EC_D void proj_add_aff_ct(Proj& r, const Proj& p, const Fe& x2, const Fe& y2) {
  Fe xx, yy, s, u, w, a, b;
  fe_mul_ct(xx, p.X, x2);
  fe_mul_ct(yy, p.Y, y2);
  fe_add_ct(a, p.X, p.Y);
  fe_add_ct(b, x2, y2);
  fe_mul_ct(s, a, b);
  fe_sub_ct(s, s, xx);
  fe_sub_ct(s, s, yy);
  fe_mul_ct(u, y2, p.Z);
  fe_add_ct(u, u, p.Y);
  fe_mul_ct(w, x2, p.Z);
  fe_add_ct(w, w, p.X);
  proj_add_tail_ct(r, xx, yy, p.Z, s, u, w);
}

// r = 2 p, complete (8 products)
EC_D void proj_dbl_ct(Proj& r, const Proj& p) {
  Fe t, z, z3, xy, yz, d, e, tz;
  fe_sqr_ct(t, p.Y);
  fe_sqr_ct(z, p.Z);
  fe_mul_small_ct(z, z, 21);       // z = b3 Z^2
  fe_mul_ct(xy, p.X, p.Y);
  fe_mul_ct(yz, p.Y, p.Z);
  fe_mul_small_ct(z3, z, 3);
  fe_sub_ct(d, t, z3);             // t - 3z
  fe_add_ct(e, t, z);              // t + z
  fe_mul_ct(tz, t, z);
  fe_mul_small_ct(tz, tz, 8);
  Proj o;
  fe_mul_ct(o.X, xy, d);
  fe_add_ct(o.X, o.X, o.X);        // X3 = 2 X Y (t - 3z)
  fe_mul_ct(o.Y, d, e);
  fe_add_ct(o.Y, o.Y, tz);         // Y3 = (t - 3z)(t + z) + 8 t z
  fe_mul_ct(o.Z, t, yz);
  fe_mul_small_ct(o.Z, o.Z, 8);    // Z3 = 8 t Y Z
  r = o;
}

// (X : Y : Z) -> affine x | y; the identity (Z = 0) comes out as (0, 0), the
// ABI's infinity, because fe_inv_ct maps 0 to 0
EC_D void proj_to_aff_ct(Fe& x, Fe& y, const Proj& p) {
  Fe zi;
  fe_inv_ct(zi, p.Z);
  fe_mul_ct(x, p.X, zi);
  fe_mul_ct(y, p.Y, zi);
}

}  // namespace ec
}  // namespace fsdkr
