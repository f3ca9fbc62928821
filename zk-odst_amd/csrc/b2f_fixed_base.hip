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

}  // namespace b2f
