// b2f_fixed_base.hip -- batched fixed-base scalar multiplication: out[i] = [s_i] B for one base B
// and n scalars (b2f_fixed_base_mul_dev). With s_i = tau^i and B the generator this is the first
// half of halo2's ParamsKZG::setup (g[i] = [tau^i] G); b2f_group_ntt_dev is the second.
// DESIGN.md §4.12.
//
// Forms 0/1 are Vesta, 2/3 BN254 G1 (b2f_curve.h); points are affine, base-field Montgomery form,
// 64 bytes, the identity all zero (b2f_msm_dev's layout).
//
// The table. A scalar is FB_WINDOWS = 32 windows of FB_C = 8 bits, recoded to signed digits
// d_w in [-127, 128] with s = sum_w d_w 2^(8 w). Entry (w, j), 1 <= j <= 128, at index
// w * 128 + (j - 1), is the affine point [j 2^(8 w)] B: 4,096 points, 256 KiB, which an XCD's
// 4 MiB L2 holds whole; a lane's gather is one whole 64-byte point. One launch builds it, one lane
// per entry, by the full-width scalar_mul of b2f_curve.h on the integer j 2^(8 w) (<= 2^255 at
// w = 31, j = 128: it fits the 256 bits scalar_mul takes, and [m] B needs no reduction of m).
// The longest lane walks 255 doublings; the build is a one-time cost per (curve, base), cached
// by the context (b2f_api_prover.hip).
//
// The recoding. With carry_0 = 0, t_w = byte_w(s) + carry_w; t_w > 128 gives d_w = t_w - 256
// and carry_{w+1} = 1, else d_w = t_w and carry_{w+1} = 0. t_w <= 256, so d_w is in [-127, 128]
// and the magnitudes are the table's 1..128. No carry leaves the top window for a reduced scalar:
// both group orders are below 2^255, so byte_31(s) <= 127, t_31 <= 128 and the rule "> 128"
// (not ">= 128") sets no carry. A scalar that is not reduced (>= 2^255) would lose that carry:
// the contract asks for reduced scalars and the result is then merely a wrong point.
//
// The per-output kernel: one lane per scalar, the low window first. The scalar is shifted right a
// byte a step, so no word of it is indexed by a variable. A zero digit is skipped, a negative one
// negates y; the accumulator is XYZZ and every addition the complete madd (the identity
// accumulator of the first non-zero digit; a partial sum equal to the top window's entry modulo
// the group order, m = d 2^248 - r with |m| < 2^248, which s = 2 d 2^248 - r reaches: the
// doubling; the opposite case needs a partial sum of 0 mod r, which only the unreduced s = r
// reaches, and it then gives the identity as it should). Then one to_affine per lane and a 64-byte
// store.
// An index into the table is w * 128 + (t - 1) with w < 32 and 1 <= t <= 128 for any 256-bit
// input, reduced or not, so no scalar reads outside the table.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/b2f.h"
#include "b2f_curve.h"
#include "b2f_field.h"
#include "b2f_launch.h"

namespace b2f {

namespace {

using namespace field;
using namespace curve;

constexpr uint32_t FB_THREADS = 128;
constexpr uint32_t FB_C = 8, FB_WINDOWS = 32, FB_HALF = 1u << (FB_C - 1);  // 128 entries per window
constexpr uint32_t FB_POINTS = FB_WINDOWS * FB_HALF;

struct Words8 {
  uint64_t v[8];
};

// table[w * 128 + j - 1] = affine([j 2^(8 w)] base)
template <class C>
__global__ __launch_bounds__(FB_THREADS) void fb_table_kernel(const Words8 base, uint64_t* __restrict__ table,
                                                              int* sticky) {
  using F = typename C::Base;
  const uint32_t e = blockIdx.x * FB_THREADS + threadIdx.x;
  if (e >= FB_POINTS) return;
  const uint32_t w = e / FB_HALF, j = e % FB_HALF + 1;
  Fe k = fe_zero();
  const uint32_t bit = FB_C * w, word = bit >> 5, sh = bit & 31;  // sh in {0, 8, 16, 24}
#pragma unroll
  for (uint32_t i = 0; i < 8; i++)
    if (i == word) k.w[i] = j << sh;  // j <= 2^7, so j << 24 <= 2^31 stays in the word
  Affine b;
  b.x = load_words(base.v);
  b.y = load_words(base.v + 4);
  bool ok = true;
  const Affine r = to_affine<F>(scalar_mul<F>(b, k), ok);
  if (!ok) atomicOr(sticky, 1 << B2F_ERR_CHECK);
  store_affine(table + 8ull * e, r);
}

template <class C, bool MONT>
__global__ __launch_bounds__(FB_THREADS) void fb_mul_kernel(const uint64_t* __restrict__ scalars, uint64_t len,
                                                            const uint64_t* __restrict__ table,
                                                            uint64_t* __restrict__ out, int* sticky) {
  using F = typename C::Base;
  const uint64_t i = (uint64_t)blockIdx.x * FB_THREADS + threadIdx.x;
  if (i >= len) return;
  Fe k = load(scalars + 4 * i);
  if (MONT) k = to_canonical<typename C::Scalar>(k);
  Xyzz acc = xyzz_identity();
  uint32_t carry = 0;
#pragma unroll 1
  for (uint32_t w = 0; w < FB_WINDOWS; w++) {
    uint32_t t = (k.w[0] & 0xffu) + carry;
#pragma unroll
    for (int q = 0; q < 7; q++) k.w[q] = (k.w[q] >> 8) | (k.w[q + 1] << 24);
    k.w[7] >>= 8;
    const bool negative = t > FB_HALF;
    carry = negative ? 1u : 0u;
    if (negative) t = 256u - t;  // the magnitude, 1..127
    if (t == 0) continue;
    Affine p = load_affine(table + 8ull * (w * FB_HALF + (t - 1)));
    if (negative) p = neg<F>(p);
    acc = madd<F>(acc, p);
  }
  bool ok = true;
  const Affine r = to_affine<F>(acc, ok);
  if (!ok) atomicOr(sticky, 1 << B2F_ERR_CHECK);
  store_affine(out + 8 * i, r);
}

// The blinding of an IPA round's cross terms (b2f_ipa_open_dev), one workgroup:
//   out[0] = L + [value_l z] U + [l_rand] W      out[1] = R + [value_r z] U + [r_rand] W
// from the tables of U and W. Four multiples of 32 signed digits each: lane t holds digit t % 32 of
// multiple t / 32 (0: value_l z on U, 1: l_rand on W, 2: value_r z on U, 3: r_rand on W), gathers
// its one table entry, and the 64 lanes of an output are summed by a tree in LDS; the output's
// first lane adds the round's raw point and converts to affine. No lane walks a doubling chain:
// the depth is one gather, six additions and one inversion. values: (value_l, value_r) in the
// form; z: canonical; rand: (l_rand, r_rand) in the form. An identity output raises B2F_ERR_FIELD
// (halo2 refuses to write it to the transcript).
constexpr uint32_t FB_BLIND_THREADS = 4 * FB_WINDOWS;
struct BlindLds {
  uint32_t w[FB_BLIND_THREADS][33];
};
template <class C, bool MONT>
__global__ __launch_bounds__(FB_BLIND_THREADS) void fb_blind_kernel(
    const uint64_t* __restrict__ lr_raw, const uint64_t* __restrict__ values, const uint64_t* __restrict__ z,
    const uint64_t* __restrict__ rand, const uint64_t* __restrict__ table_u, const uint64_t* __restrict__ table_w,
    uint64_t* __restrict__ out, int* sticky) {
  using F = typename C::Base;
  using FS = typename C::Scalar;
  __shared__ BlindLds lds;
  const uint32_t t = threadIdx.x, m = t / FB_WINDOWS, w = t % FB_WINDOWS, which = m >> 1;
  Fe k;
  if (m & 1u) {
    k = load(rand + 4 * which);
    if (MONT) k = to_canonical<FS>(k);
  } else {
    // mul(x, y) = x y / R: a Montgomery value against the canonical z is the canonical product; a
    // canonical value gives it over R, which to_mont undoes
    k = mul<FS>(load(values + 4 * which), load(z));
    if (!MONT) k = to_mont<FS>(k);
  }
  // the recoding of fb_mul_kernel, kept up to this lane's window
  uint32_t carry = 0, digit = 0;
  bool negative = false;
#pragma unroll 1
  for (uint32_t q = 0; q <= w; q++) {
    digit = (k.w[0] & 0xffu) + carry;
#pragma unroll
    for (int i = 0; i < 7; i++) k.w[i] = (k.w[i] >> 8) | (k.w[i + 1] << 24);
    k.w[7] >>= 8;
    negative = digit > FB_HALF;
    carry = negative ? 1u : 0u;
    if (negative) digit = 256u - digit;
  }
  Xyzz acc = xyzz_identity();
  if (digit != 0) {  // 1 <= digit <= 128, w < 32: inside the table for any 256-bit scalar
    Affine p = load_affine(((m & 1u) ? table_w : table_u) + 8ull * (w * FB_HALF + (digit - 1)));
    if (negative) p = neg<F>(p);
    acc = from_affine<F>(p);
  }
  auto put = [&](uint32_t at, const Xyzz& v) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      lds.w[at][i] = v.x.w[i];
      lds.w[at][8 + i] = v.y.w[i];
      lds.w[at][16 + i] = v.zz.w[i];
      lds.w[at][24 + i] = v.zzz.w[i];
    }
  };
  auto get = [&](uint32_t at) {
    Xyzz v;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      v.x.w[i] = lds.w[at][i];
      v.y.w[i] = lds.w[at][8 + i];
      v.zz.w[i] = lds.w[at][16 + i];
      v.zzz.w[i] = lds.w[at][24 + i];
    }
    return v;
  };
  put(t, acc);
  __syncthreads();
  const uint32_t lane = t & (2 * FB_WINDOWS - 1);  // within the output's 64 lanes
#pragma unroll 1
  for (uint32_t s = FB_WINDOWS; s > 0; s >>= 1) {
    if (lane < s) {
      acc = add<F>(acc, get(t + s));
      put(t, acc);
    }
    __syncthreads();
  }
  if (lane == 0) {
    acc = madd<F>(acc, load_affine(lr_raw + 8ull * which));
    bool ok = true;
    const Affine r = to_affine<F>(acc, ok);
    if (!ok) atomicOr(sticky, 1 << B2F_ERR_CHECK);
    if (is_identity(r)) atomicOr(sticky, 1 << B2F_ERR_FIELD);
    store_affine(out + 8ull * which, r);
  }
}

}  // namespace

void fixed_base_plan_of(uint32_t* window_bits, uint32_t* windows, uint64_t* table_points, uint64_t* table_bytes) {
  if (window_bits) *window_bits = FB_C;
  if (windows) *windows = FB_WINDOWS;
  if (table_points) *table_points = FB_POINTS;
  if (table_bytes) *table_bytes = 64ull * FB_POINTS;
}

hipError_t launch_fixed_base_table(const uint64_t* base, uint32_t form, uint64_t* d_table, int* sticky,
                                   hipStream_t s) {
  Words8 b;
  for (int i = 0; i < 8; i++) b.v[i] = base[i];
  with_curve(form, [&](auto c) {
    hipLaunchKernelGGL((fb_table_kernel<decltype(c)>), dim3(FB_POINTS / FB_THREADS), dim3(FB_THREADS), 0, s, b,
                       d_table, sticky);
    return 0;
  });
  return hipGetLastError();
}

hipError_t launch_fixed_base_mul(const uint64_t* d_scalars, uint64_t len, uint32_t form, const uint64_t* d_table,
                                 uint64_t* d_out, int* sticky, hipStream_t s) {
  const dim3 grid((uint32_t)((len + FB_THREADS - 1) / FB_THREADS)), block(FB_THREADS);
  with_curve_form(form, [&](auto c, auto mont) {
    hipLaunchKernelGGL((fb_mul_kernel<decltype(c), decltype(mont)::value>), grid, block, 0, s, d_scalars, len,
                       d_table, d_out, sticky);
  });
  return hipGetLastError();
}

hipError_t launch_fixed_base_blind(const uint64_t* d_lr_raw, const uint64_t* d_values, const uint64_t* d_z,
                                   const uint64_t* d_rand, uint32_t form, const uint64_t* d_table_u,
                                   const uint64_t* d_table_w, uint64_t* d_out, int* sticky, hipStream_t s) {
  with_curve_form(form, [&](auto c, auto mont) {
    hipLaunchKernelGGL((fb_blind_kernel<decltype(c), decltype(mont)::value>), dim3(1), dim3(FB_BLIND_THREADS), 0, s,
                       d_lr_raw, d_values, d_z, d_rand, d_table_u, d_table_w, d_out, sticky);
  });
  return hipGetLastError();
}

}  // namespace b2f
