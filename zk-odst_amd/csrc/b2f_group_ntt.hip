// b2f_group_ntt.hip -- the group NTT: the discrete Fourier transform of n = 2^k curve points over
// the scalar field's 2^k domain (halo2's g_to_lagrange: best_fft over points with omega^-1, then
// n^-1). DESIGN.md §4.10.
//
//   forward  out[i] = sum_j [omega^(i j)] in[j]
//   inverse  out[i] = [n^-1] sum_j [omega^(-i j)] in[j]
//
// Forms 0/1 are Vesta, 2/3 BN254 G1 (b2f_curve.h); points are affine, base-field Montgomery form,
// 64 bytes, the identity all zero (b2f_msm_dev's layout), in and out.
//
// Radix 2, decimation in time, in place in d_out, one launch per stage:
//   permute   out[rev(i)] = in[i] (a copy), or the swap of i and rev(i) when d_out == d_in
//   stage 1   (a, c) -> (a + c, a - c): the twiddle is 1, no scalar multiplication. The inverse
//             does its scaling here: (A, C) = ([n^-1] a, [n^-1] c), then (A + C, A - C). These are
//             the call's n uniform-scalar multiplications; in this stage they cost no pass over
//             the points and no affine conversion of their own.
//   stage s   (2 <= s <= k) half = 2^(s-1), 2^(k-s) blocks of 2^s points: for block b and j < half,
//             a = x[b 2^s + j], c = x[a + half], t = [w^(j 2^(k-s))] c, (a, c) <- (a + t, a - t).
// The working set stays affine: every stage ends in two to_affine per butterfly, so a point is
// 64 bytes, lives in d_out itself, and the butterfly is the existing affine scalar_mul followed
// by two mixed additions (t + a, -t + a). An XYZZ working set would double the bytes, need
// scratch for n points and a scalar_mul over a projective base; the conversion it saves is
// 0.3-2.3 % of a scalar multiplication.
//
// Twiddle-uniform waves: within a stage every block uses the same half twiddles, so a launch maps
// its n/2 butterflies as e = j 2^(k-s) + b: the block index runs fastest and the twiddle index
// slowest. While a stage has at least 64 blocks, the 64 lanes of a wave share j: the kernel
// (UNIFORM) takes j from the wave's first lane, the scalar arrives by a wave-uniform load and
// the `if (bit) madd` branch of scalar_mul is uniform, as in b2f_ipa.hip's collapse. A lane's
// accesses are whole 64-byte points at any stride. The last six stages (fewer than 64 blocks) run
// the same kernel with a per-lane twiddle and a divergent branch.
//
// The twiddles are the n/2 canonical powers of omega (or omega^-1), built by launch_ipa_powers
// into the context's scratch on every call. Every routine used on points is complete (identity,
// equal and opposite operands), so structured inputs need no care here.
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

constexpr uint32_t GN_THREADS = 128;
constexpr uint32_t GN_COPY_THREADS = 256;

// omega^(2^(k-1)) must be -1: one lane, k - 1 squarings
template <class FS>
__global__ void gntt_root_check_kernel(const Words4 omega, uint32_t k, int* sticky) {
  Fe w = to_mont<FS>(load_words(omega.v));
#pragma unroll 1
  for (uint32_t i = 1; i < k; i++) w = mul<FS>(w, w);
  if (!fe_eq(w, sub<FS>(fe_zero(), one<FS>()))) atomicOr(sticky, 1 << B2F_ERR_FIELD);
}

// out[rev(i)] = in[i]; in == out: the swap, by the lower index of a pair
__global__ __launch_bounds__(GN_COPY_THREADS) void gntt_permute_kernel(const uint64_t* in, uint64_t* out,
                                                                       uint32_t k) {
  const uint32_t i = blockIdx.x * GN_COPY_THREADS + threadIdx.x;
  if (i >= (1u << k)) return;
  const uint32_t r = __brev(i) >> (32 - k);
  if (in != out) {
    store_affine(out + 8ull * r, load_affine(in + 8ull * i));
  } else if (i < r) {
    const Affine a = load_affine(in + 8ull * i), b = load_affine(in + 8ull * r);
    store_affine(out + 8ull * i, b);
    store_affine(out + 8ull * r, a);
  }
}

template <class F>
__device__ __forceinline__ void store_pair(uint64_t* pa, uint64_t* pc, const Xyzz& ra, const Xyzz& rc,
                                           int* sticky) {
  bool ok_a = true, ok_c = true;
  const Affine a = to_affine<F>(ra, ok_a);
  const Affine c = to_affine<F>(rc, ok_c);
  if (!(ok_a && ok_c)) atomicOr(sticky, 1 << B2F_ERR_CHECK);
  store_affine(pa, a);
  store_affine(pc, c);
}

// stage 1: (x[2e], x[2e+1]) <- (a + c, a - c), with SCALE both scaled by ninv (canonical) first
template <class C, bool SCALE>
__global__ __launch_bounds__(GN_THREADS) void gntt_first_kernel(uint64_t* x, uint32_t pairs, const Words4 ninv,
                                                                int* sticky) {
  using F = typename C::Base;
  const uint32_t e = blockIdx.x * GN_THREADS + threadIdx.x;
  if (e >= pairs) return;
  uint64_t* pa = x + 16ull * e;
  const Affine a = load_affine(pa), c = load_affine(pa + 8);
  Xyzz ra, rc;
  if (SCALE) {
    const Fe s = load_words(ninv.v);
    const Xyzz sa = scalar_mul<F>(a, s);
    const Xyzz sc = scalar_mul<F>(c, s);
    ra = add<F>(sa, sc);
    rc = add<F>(sa, neg<F>(sc));
  } else {
    const Xyzz sa = from_affine<F>(a);
    ra = madd<F>(sa, c);
    rc = madd<F>(sa, neg<F>(c));
  }
  store_pair<F>(pa, pa + 8, ra, rc, sticky);
}

// stage s >= 2: butterfly e = j 2^lb + b of block b (lb = k - s), twiddle tw[j 2^lb]
template <class C, bool UNIFORM>
__global__ __launch_bounds__(GN_THREADS) void gntt_stage_kernel(uint64_t* x, const uint64_t* __restrict__ tw,
                                                                uint32_t k, uint32_t s, int* sticky) {
  using F = typename C::Base;
  const uint32_t e = blockIdx.x * GN_THREADS + threadIdx.x;
  if (e >= (1u << (k - 1))) return;
  const uint32_t lb = k - s;
  const uint32_t b = e & ((1u << lb) - 1u), j = e >> lb;
  Fe w;
  if (UNIFORM) {  // 2^lb >= 64: the wave's lanes share j
    const uint32_t ju = __builtin_amdgcn_readfirstlane(e) >> lb;
    w = load(tw + 4ull * ((uint64_t)ju << lb));
#pragma unroll
    for (int i = 0; i < 8; i++) w.w[i] = __builtin_amdgcn_readfirstlane(w.w[i]);
  } else {
    w = load(tw + 4ull * ((uint64_t)j << lb));
  }
  uint64_t* pa = x + 8ull * (((uint64_t)b << s) + j);
  uint64_t* pc = pa + (8ull << (s - 1));
  const Affine a = load_affine(pa);
  const Xyzz t = scalar_mul<F>(load_affine(pc), w);
  const Xyzz ra = madd<F>(t, a);
  const Xyzz rc = madd<F>(neg<F>(t), a);
  store_pair<F>(pa, pc, ra, rc, sticky);
}

inline uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }

}  // namespace

uint64_t group_ntt_scalar_muls(uint32_t k) {
  const uint64_t n = 1ull << k;
  return n + (n / 2) * (k - 1);
}

size_t group_ntt_scratch_bytes(uint32_t k) { return k < 2 ? 0 : (size_t)align256(16ull << k); }

hipError_t launch_group_ntt(const uint64_t* d_in, uint32_t k, const uint64_t* omega, const uint64_t* tw_base,
                            const uint64_t* ninv, uint32_t form, uint64_t* d_out, void* scratch, int* sticky,
                            hipStream_t s) {
  const uint32_t n = 1u << k, pairs = n / 2;
  uint64_t* tw = reinterpret_cast<uint64_t*>(scratch);
  with_field(form, [&](auto f) {
    hipLaunchKernelGGL((gntt_root_check_kernel<decltype(f)>), dim3(1), dim3(1), 0, s, words4(omega), k, sticky);
    return 0;
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  if (k >= 2) {
    e = launch_ipa_powers(tw_base, pairs, form & ~1u, tw, s);  // canonical scalars
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(gntt_permute_kernel, dim3((n + GN_COPY_THREADS - 1) / GN_COPY_THREADS), dim3(GN_COPY_THREADS),
                     0, s, d_in, d_out, k);
  const dim3 grid((pairs + GN_THREADS - 1) / GN_THREADS), block(GN_THREADS);
  const uint64_t zero[4] = {0, 0, 0, 0};
  with_curve(form, [&](auto c) {
    using C = decltype(c);
    if (ninv)
      hipLaunchKernelGGL((gntt_first_kernel<C, true>), grid, block, 0, s, d_out, pairs, words4(ninv), sticky);
    else
      hipLaunchKernelGGL((gntt_first_kernel<C, false>), grid, block, 0, s, d_out, pairs, words4(zero), sticky);
    for (uint32_t st = 2; st <= k; st++) {
      if (k - st >= 6)
        hipLaunchKernelGGL((gntt_stage_kernel<C, true>), grid, block, 0, s, d_out, tw, k, st, sticky);
      else
        hipLaunchKernelGGL((gntt_stage_kernel<C, false>), grid, block, 0, s, d_out, tw, k, st, sticky);
    }
    return 0;
  });
  return hipGetLastError();
}

}  // namespace b2f
