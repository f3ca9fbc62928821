// b2f_curve.h -- short Weierstrass curves y^2 = x^3 + b (a = 0) over the base fields of
// b2f_field.h, on the device: the point arithmetic of the commitments (b2f_msm.hip).
//
// Affine points are (x, y) in base-field Montgomery form, 16 words; the identity is all-zero
// ((0, 0) is on neither curve: 0 != b). The accumulator is in extended Jacobian coordinates
// (XYZZ: x = X / ZZ, y = Y / ZZZ, ZZ^3 = ZZZ^2), the identity being ZZ = 0 (stored all-zero).
// Formulas: the Explicit-Formulas Database's short Weierstrass "xyzz" set with a = 0
// (add-2008-s, madd-2008-s, dbl-2008-s-1, mdbl-2008-s-1); field products (`mul` calls) each:
//   madd 10, add 14, dbl 9, mdbl 6, to_affine 5 + one inv_safegcd.
// Every routine is complete over its inputs: an identity accumulator or addend, equal points
// (the difference P = 0, R = 0: the doubling) and opposite points (P = 0, R != 0: the identity)
// take their own branches. A point with y = 0 doubles to the identity (ZZ3 = (2y)^2 ZZ = 0); the
// two curves have odd prime order and no such point. Off-curve input gives a meaningless point
// and touches no memory.
#pragma once
#include "b2f_field.h"

namespace b2f {
namespace curve {

using field::Fe;

struct Affine {
  Fe x, y;
};
struct Xyzz {
  Fe x, y, zz, zzz;
};

__device__ __forceinline__ bool is_identity(const Affine& p) { return field::is_zero(p.x) && field::is_zero(p.y); }
__device__ __forceinline__ bool is_identity(const Xyzz& p) { return field::is_zero(p.zz); }

__device__ __forceinline__ Xyzz xyzz_identity() {
  Xyzz r;
  r.x = r.y = r.zz = r.zzz = field::fe_zero();
  return r;
}
__device__ __forceinline__ Affine affine_identity() {
  Affine r;
  r.x = r.y = field::fe_zero();
  return r;
}

template <class F>
__device__ __forceinline__ Fe fe_neg(const Fe& a) {  // -a mod p (0 stays 0)
  return field::sub<F>(field::fe_zero(), a);
}
template <class F>
__device__ __forceinline__ Fe fe_dbl(const Fe& a) {
  return field::add<F>(a, a);
}

template <class F>
__device__ __forceinline__ Affine neg(const Affine& p) {
  Affine r;
  r.x = p.x;
  r.y = fe_neg<F>(p.y);
  return r;
}
template <class F>
__device__ __forceinline__ Xyzz neg(const Xyzz& p) {
  Xyzz r = p;
  r.y = fe_neg<F>(p.y);
  return r;
}

template <class F>
__device__ __forceinline__ Xyzz from_affine(const Affine& p) {
  Xyzz r;
  if (is_identity(p)) return xyzz_identity();
  r.x = p.x;
  r.y = p.y;
  r.zz = r.zzz = field::one<F>();
  return r;
}

// 2 p of an affine p != identity (mdbl-2008-s-1, a = 0)
template <class F>
__device__ __noinline__ Xyzz mdbl(const Affine& p) {
  using namespace field;
  const Fe u = fe_dbl<F>(p.y);
  const Fe v = mul<F>(u, u);
  const Fe w = mul<F>(u, v);
  const Fe s = mul<F>(p.x, v);
  const Fe xx = mul<F>(p.x, p.x);
  const Fe m = add<F>(fe_dbl<F>(xx), xx);
  Xyzz r;
  r.x = sub<F>(mul<F>(m, m), fe_dbl<F>(s));
  r.y = sub<F>(mul<F>(m, sub<F>(s, r.x)), mul<F>(w, p.y));
  r.zz = v;
  r.zzz = w;
  if (is_zero(v)) return xyzz_identity();  // y = 0: a 2-torsion point (neither curve has one)
  return r;
}

// 2 p (dbl-2008-s-1, a = 0); the identity stays the identity (ZZ3 = V ZZ = 0)
template <class F>
__device__ __noinline__ Xyzz dbl(const Xyzz& p) {
  using namespace field;
  const Fe u = fe_dbl<F>(p.y);
  const Fe v = mul<F>(u, u);
  const Fe w = mul<F>(u, v);
  const Fe s = mul<F>(p.x, v);
  const Fe xx = mul<F>(p.x, p.x);
  const Fe m = add<F>(fe_dbl<F>(xx), xx);
  Xyzz r;
  r.zz = mul<F>(v, p.zz);
  if (is_zero(r.zz)) return xyzz_identity();
  r.x = sub<F>(mul<F>(m, m), fe_dbl<F>(s));
  r.y = sub<F>(mul<F>(m, sub<F>(s, r.x)), mul<F>(w, p.y));
  r.zzz = mul<F>(w, p.zzz);
  return r;
}

// acc + q, q affine (madd-2008-s)
template <class F>
__device__ __forceinline__ Xyzz madd(const Xyzz& acc, const Affine& q) {
  using namespace field;
  if (is_identity(q)) return acc;
  if (is_identity(acc)) return from_affine<F>(q);
  const Fe u2 = mul<F>(q.x, acc.zz);
  const Fe s2 = mul<F>(q.y, acc.zzz);
  const Fe p = sub<F>(u2, acc.x);
  const Fe r = sub<F>(s2, acc.y);
  if (is_zero(p)) {
    if (is_zero(r)) return mdbl<F>(q);  // equal points
    return xyzz_identity();             // opposite points
  }
  const Fe pp = mul<F>(p, p);
  const Fe ppp = mul<F>(p, pp);
  const Fe qq = mul<F>(acc.x, pp);
  Xyzz o;
  o.x = sub<F>(sub<F>(mul<F>(r, r), ppp), fe_dbl<F>(qq));
  o.y = sub<F>(mul<F>(r, sub<F>(qq, o.x)), mul<F>(acc.y, ppp));
  o.zz = mul<F>(acc.zz, pp);
  o.zzz = mul<F>(acc.zzz, ppp);
  return o;
}

// a + b (add-2008-s)
template <class F>
__device__ __forceinline__ Xyzz add(const Xyzz& a, const Xyzz& b) {
  using namespace field;
  if (is_identity(b)) return a;
  if (is_identity(a)) return b;
  const Fe u1 = mul<F>(a.x, b.zz);
  const Fe u2 = mul<F>(b.x, a.zz);
  const Fe s1 = mul<F>(a.y, b.zzz);
  const Fe s2 = mul<F>(b.y, a.zzz);
  const Fe p = sub<F>(u2, u1);
  const Fe r = sub<F>(s2, s1);
  if (is_zero(p)) {
    if (is_zero(r)) return dbl<F>(a);
    return xyzz_identity();
  }
  const Fe pp = mul<F>(p, p);
  const Fe ppp = mul<F>(p, pp);
  const Fe qq = mul<F>(u1, pp);
  Xyzz o;
  o.x = sub<F>(sub<F>(mul<F>(r, r), ppp), fe_dbl<F>(qq));
  o.y = sub<F>(mul<F>(r, sub<F>(qq, o.x)), mul<F>(s1, ppp));
  o.zz = mul<F>(mul<F>(a.zz, b.zz), pp);
  o.zzz = mul<F>(mul<F>(a.zzz, b.zzz), ppp);
  return o;
}

// k * p for a canonical scalar k (any 256-bit integer) and an affine p, left-to-right double and
// add with mixed additions: the full-width sibling of b2f_msm.hip's 16-bit small_mul. About
// 9 products per bit below the top one and 10 per set bit. The scalar is shifted left a bit a step
// and its top bit tested, so no word of it is indexed by a variable; leading zero bits cost the
// shift alone. With a scalar the whole wave shares (a kernel argument: b2f_ipa.hip's collapse) the
// branch is uniform.
template <class F>
__device__ Xyzz scalar_mul(const Affine& p, Fe k) {
  Xyzz r = xyzz_identity();
  if (is_identity(p)) return r;
  bool started = false;
#pragma unroll 1
  for (int b = 0; b < 256; b++) {
    const bool bit = k.w[7] >> 31;
#pragma unroll
    for (int i = 7; i > 0; i--) k.w[i] = (k.w[i] << 1) | (k.w[i - 1] >> 31);
    k.w[0] <<= 1;
    if (!started && !bit) continue;
    if (started) r = dbl<F>(r);
    if (bit) r = madd<F>(r, p);
    started = true;
  }
  return r;
}

// The affine form of p (the identity: all zero): one inversion (of ZZZ; 1 / ZZ = (ZZ / ZZZ)^2
// since ZZ^3 = ZZZ^2) and five products. `ok` is inv_safegcd's.
template <class F>
__device__ Affine to_affine(const Xyzz& p, bool& ok) {
  using namespace field;
  ok = true;
  if (is_identity(p)) return affine_identity();
  const Fe i = inv_safegcd<F>(p.zzz, ok);
  const Fe t = mul<F>(p.zz, i);
  Affine r;
  r.x = mul<F>(p.x, mul<F>(t, t));
  r.y = mul<F>(p.y, i);
  return r;
}

__device__ __forceinline__ Affine load_affine(const uint64_t* p) {
  Affine r;
  r.x = field::load(p);
  r.y = field::load(p + 4);
  return r;
}
__device__ __forceinline__ void store_affine(uint64_t* p, const Affine& a) {
  field::store(p, a.x);
  field::store(p + 4, a.y);
}
__device__ __forceinline__ Xyzz load_xyzz(const uint64_t* p) {
  Xyzz r;
  r.x = field::load(p);
  r.y = field::load(p + 4);
  r.zz = field::load(p + 8);
  r.zzz = field::load(p + 12);
  return r;
}
__device__ __forceinline__ void store_xyzz(uint64_t* p, const Xyzz& a) {
  field::store(p, a.x);
  field::store(p + 4, a.y);
  field::store(p + 8, a.zz);
  field::store(p + 12, a.zzz);
}

}  // namespace curve
}  // namespace b2f
