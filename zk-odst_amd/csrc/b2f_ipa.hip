// b2f_ipa.hip -- the device side of the inner product argument's opening rounds (halo2_proofs
// 0.3.0 poly/commitment/prover.rs::create_proof's loop) over three vectors of length len = 2^j:
// the coefficients p, the powers b and the generators G. DESIGN.md §4.8.
//
//   round  L = <p[half..], G[..half]>   R = <p[..half], G[half..]>   (points, affine)
//          value_l = <p[half..], b[..half]>   value_r = <p[..half], b[half..]>   (field)
//   fold   p[i] += p[half+i] u^-1   b[i] += b[half+i] u   G[i] = affine(G[i] + [u] G[half+i])
//
// For the three separate calls the transcript, the blinding and the U / W terms are the caller's and
// every challenge is a host argument. b2f_ipa_open_dev queues the whole loop:
// per round the same round launches, the blinding of L and R from the tables of U and W
// (b2f_fixed_base.hip), ipa_challenge_kernel (absorb L_j, R_j; squeeze u_j; u_j^-1; f) on the
// device transcript of b2f_transcript.h, and the fold kernels' entries that read u_j from memory;
// then ipa_finish_kernel (c, and c and f absorbed). Forms 0/1 are Vesta, 2/3 BN254 G1
// (b2f_curve.h); scalars are in `form`, points in base-field Montgomery form.
//
// Cross terms: a long round views p as a block of two columns of `half` rows, column 0 against
// G[half..] (R) and column 1 against G[..half] (L), and runs ONE Pippenger pass of b2f_msm.hip with
// per-column base offsets: one recode, one sort, one set of reduction levels for both points. A
// short round (len <= ipa_direct_max_len) is one launch of ipa_round_direct_kernel: a workgroup per
// output, every lane a double-and-add over its elements, an LDS tree, one to_affine; two more
// workgroups of the same launch form the two inner products. Measured, the switch-over is len = 2
// (see IPA_DIRECT_MAX_LEN below).
//
// The inner products are bilinear in the column data: mul(x, y) = x y / R, so a Montgomery pair
// gives the Montgomery form of the product, and a canonical pair gives x y / R, which the total is
// corrected for by one product with R^2. (The linear passes of b2f_open.hip need no such step;
// this one does.) The scalar folds are linear with Montgomery-form multipliers u, u^-1 and work in
// either form as they are.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/b2f.h"
#include "b2f_curve.h"
#include "b2f_field.h"
#include "b2f_launch.h"
#include "b2f_transcript.h"

namespace b2f {

namespace {

using namespace field;
using namespace curve;

constexpr uint32_t IPA_THREADS = 256;
constexpr uint32_t IPA_C = 4, IPA_TILE = IPA_THREADS * IPA_C;  // inner-product tile
constexpr uint32_t COLLAPSE_THREADS = 128;
// The longest round the direct kernel takes (a power of two), from the sweep of tools/bench_ipa.py
// --sweep (profiles/ipa_bench.jsonl): the two paths tie at len = 2 (2.4 against
// 2.3 ms on Vesta, inside the spread of either) and the Pippenger pass is ahead at every length from
// 4 up (by 0.2-0.8 ms up to 512, then by the direct kernel's linear growth). Both are bound by one
// wave's chain of 255 dependent doublings; the direct lane also has its ~128 mixed additions in
// that chain, the Pippenger pass has them in other lanes. So the direct kernel keeps len = 2 (one
// launch against a dozen, the same time) and stays the diagnostics library's cross-check.
constexpr uint64_t IPA_DIRECT_MAX_LEN = 2;

inline uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }

// ---- b = (1, x, x^2, ..) ------------------------------------------------------------------------
template <class F, bool MONT>
__global__ __launch_bounds__(IPA_THREADS) void ipa_powers_kernel(const Words4 x, uint64_t len,
                                                                 uint64_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * IPA_THREADS + threadIdx.x;
  if (i >= len) return;
  Fe v = pow_entry<F>(load_words(x.v), (uint32_t)i);
  if (!MONT) v = to_canonical<F>(v);
  store(out + 4 * i, v);
}

// ---- LDS helpers: one XYZZ (32 words, padded to 33) or one field element per thread --------------
struct PointLds {
  uint32_t w[IPA_THREADS][33];
};
__device__ __forceinline__ void lds_put(PointLds& l, uint32_t t, const Xyzz& p) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    l.w[t][i] = p.x.w[i];
    l.w[t][8 + i] = p.y.w[i];
    l.w[t][16 + i] = p.zz.w[i];
    l.w[t][24 + i] = p.zzz.w[i];
  }
}
__device__ __forceinline__ Xyzz lds_get(const PointLds& l, uint32_t t) {
  Xyzz p;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    p.x.w[i] = l.w[t][i];
    p.y.w[i] = l.w[t][8 + i];
    p.zz.w[i] = l.w[t][16 + i];
    p.zzz.w[i] = l.w[t][24 + i];
  }
  return p;
}
__device__ __forceinline__ void lds_put_fe(PointLds& l, uint32_t t, const Fe& a) {
#pragma unroll
  for (int i = 0; i < 8; i++) l.w[t][i] = a.w[i];
}
__device__ __forceinline__ Fe lds_get_fe(const PointLds& l, uint32_t t) {
  Fe a;
#pragma unroll
  for (int i = 0; i < 8; i++) a.w[i] = l.w[t][i];
  return a;
}
// the workgroup's sum of `acc`, valid in thread 0
template <class F>
__device__ __forceinline__ Fe block_sum(PointLds& l, Fe acc) {
  const uint32_t t = threadIdx.x;
  lds_put_fe(l, t, acc);
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = IPA_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
      acc = add<F>(acc, lds_get_fe(l, t + s));
      lds_put_fe(l, t, acc);
    }
    __syncthreads();
  }
  return acc;
}

// ---- a short round in one launch -----------------------------------------------------------------
// Workgroup 0: L, 1: R, 2: value_l, 3: value_r.
template <class C, bool MONT>
__global__ __launch_bounds__(IPA_THREADS) void ipa_round_direct_kernel(const uint64_t* __restrict__ p,
                                                                       const uint64_t* __restrict__ b,
                                                                       const uint64_t* __restrict__ g,
                                                                       uint32_t half, uint64_t* __restrict__ lr,
                                                                       uint64_t* __restrict__ values, int* sticky) {
  using F = typename C::Base;
  using FS = typename C::Scalar;
  __shared__ PointLds lds;
  const uint32_t t = threadIdx.x, which = blockIdx.x & 1u;
  // which = 0: the high half of p against the low half of the other vector (L, value_l)
  const uint64_t* ps = p + 4ull * (which ? 0 : half);
  if (blockIdx.x < 2) {
    const uint64_t* gs = g + 8ull * (which ? half : 0);
    Xyzz acc = xyzz_identity();
#pragma unroll 1
    for (uint32_t i = t; i < half; i += IPA_THREADS) {
      Fe s = load(ps + 4ull * i);
      if (MONT) s = to_canonical<FS>(s);
      acc = add<F>(acc, scalar_mul<F>(load_affine(gs + 8ull * i), s));
    }
    lds_put(lds, t, acc);
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = IPA_THREADS / 2; s > 0; s >>= 1) {
      if (t < s) {
        acc = add<F>(acc, lds_get(lds, t + s));
        lds_put(lds, t, acc);
      }
      __syncthreads();
    }
    if (t == 0) {
      bool ok = true;
      const Affine a = to_affine<F>(acc, ok);
      if (!ok) atomicOr(sticky, 1 << B2F_ERR_CHECK);
      store_affine(lr + 8ull * which, a);
    }
  } else {
    const uint64_t* bs = b + 4ull * (which ? half : 0);
    Fe acc = fe_zero();
#pragma unroll 1
    for (uint32_t i = t; i < half; i += IPA_THREADS) acc = add<FS>(acc, mul<FS>(load(ps + 4ull * i), load(bs + 4ull * i)));
    acc = block_sum<FS>(lds, acc);
    if (t == 0) {
      if (!MONT) acc = to_mont<FS>(acc);  // the sum of x y / R, times R
      store(values + 4ull * which, acc);
    }
  }
}

// ---- inner products of a long round ---------------------------------------------------------------
// partial[y * ntiles + tile] = the tile's sum of products (y = 0: value_l, 1: value_r); the eight
// loads of a lane are issued before the first product
template <class FS>
__global__ __launch_bounds__(IPA_THREADS) void ipa_ip_tiles_kernel(const uint64_t* __restrict__ p,
                                                                   const uint64_t* __restrict__ b, uint32_t half,
                                                                   uint32_t ntiles, uint64_t* __restrict__ partial) {
  __shared__ PointLds lds;
  const uint32_t t = threadIdx.x, which = blockIdx.y;
  const uint64_t* ps = p + 4ull * (which ? 0 : half);
  const uint64_t* bs = b + 4ull * (which ? half : 0);
  const uint64_t s0 = (uint64_t)blockIdx.x * IPA_TILE + t;
  Fe x[IPA_C], y[IPA_C];
#pragma unroll
  for (uint32_t j = 0; j < IPA_C; j++) {
    const uint64_t i = s0 + j * IPA_THREADS;
    x[j] = i < half ? load(ps + 4 * i) : fe_zero();
    y[j] = i < half ? load(bs + 4 * i) : fe_zero();
  }
  Fe acc = mul<FS>(x[0], y[0]);
#pragma unroll
  for (uint32_t j = 1; j < IPA_C; j++) acc = add<FS>(acc, mul<FS>(x[j], y[j]));
  acc = block_sum<FS>(lds, acc);
  if (t == 0) store(partial + 4ull * ((uint64_t)which * ntiles + blockIdx.x), acc);
}

// Workgroups 0 / 1: the sum of a value's partials, corrected and stored. Workgroup 2: the two
// points of the Pippenger pass (column 0 = R, column 1 = L) to lr = (L, R).
template <class FS, bool MONT>
__global__ __launch_bounds__(IPA_THREADS) void ipa_combine_kernel(const uint64_t* __restrict__ partial,
                                                                  uint32_t ntiles, const uint64_t* __restrict__ rl,
                                                                  uint64_t* __restrict__ lr,
                                                                  uint64_t* __restrict__ values) {
  __shared__ PointLds lds;
  const uint32_t t = threadIdx.x;
  if (blockIdx.x == 2) {
    if (t < 16) lr[t] = rl[(t + 8) & 15];
    return;
  }
  const uint64_t* src = partial + 4ull * blockIdx.x * ntiles;
  Fe acc = fe_zero();
#pragma unroll 1
  for (uint32_t i = t; i < ntiles; i += IPA_THREADS) acc = add<FS>(acc, load(src + 4ull * i));
  acc = block_sum<FS>(lds, acc);
  if (t == 0) {
    if (!MONT) acc = to_mont<FS>(acc);
    store(values + 4ull * blockIdx.x, acc);
  }
}

// ---- the folds ------------------------------------------------------------------------------------
// Each fold kernel has two entries over one body: the multipliers as kernel arguments (the host's
// challenge, b2f_ipa_fold_dev) or read from device memory where the challenge kernel left them
// (b2f_ipa_open_dev: chal[0..3] = u canonical, [4..7] = u Montgomery, [8..11] = u^-1 Montgomery).
// p[i] += p[half + i] u^-1, b[i] += b[half + i] u: lane i touches rows i and half + i only
template <class FS>
__device__ __forceinline__ void fold_scalars_body(uint64_t* __restrict__ p, uint64_t* __restrict__ b, uint32_t half,
                                                  const Fe& u_mont, const Fe& uinv_mont) {
  const uint32_t i = blockIdx.x * IPA_THREADS + threadIdx.x;
  if (i >= half) return;
  const Fe plo = load(p + 4ull * i), phi = load(p + 4ull * (half + i));
  const Fe blo = load(b + 4ull * i), bhi = load(b + 4ull * (half + i));
  store(p + 4ull * i, add<FS>(plo, mul<FS>(phi, uinv_mont)));
  store(b + 4ull * i, add<FS>(blo, mul<FS>(bhi, u_mont)));
}
template <class FS>
__global__ __launch_bounds__(IPA_THREADS) void ipa_fold_scalars_kernel(uint64_t* __restrict__ p,
                                                                       uint64_t* __restrict__ b, uint32_t half,
                                                                       const Words4 u_mont, const Words4 uinv_mont) {
  fold_scalars_body<FS>(p, b, half, load_words(u_mont.v), load_words(uinv_mont.v));
}
template <class FS>
__global__ __launch_bounds__(IPA_THREADS) void ipa_fold_scalars_ptr_kernel(uint64_t* __restrict__ p,
                                                                           uint64_t* __restrict__ b, uint32_t half,
                                                                           const uint64_t* __restrict__ chal) {
  fold_scalars_body<FS>(p, b, half, load(chal + 4), load(chal + 8));
}

// G[i] = affine(G[i] + [u] G[half + i]): one lane per point, u (canonical) the same for the wave
template <class C>
__device__ __forceinline__ void collapse_body(uint64_t* __restrict__ g, uint32_t half, const Fe& u, int* sticky) {
  using F = typename C::Base;
  const uint32_t i = blockIdx.x * COLLAPSE_THREADS + threadIdx.x;
  if (i >= half) return;
  const Affine lo = load_affine(g + 8ull * i);
  Xyzz acc = scalar_mul<F>(load_affine(g + 8ull * (half + i)), u);
  acc = madd<F>(acc, lo);
  bool ok = true;
#ifdef B2F_IPA_NO_AFFINE  // ablation builds only (tools/bench_ipa.py): the collapse without its inversion
  Affine a;
  a.x = acc.x;
  a.y = acc.y;
#else
  const Affine a = to_affine<F>(acc, ok);
#endif
  if (!ok) atomicOr(sticky, 1 << B2F_ERR_CHECK);
  store_affine(g + 8ull * i, a);
}
template <class C>
__global__ __launch_bounds__(COLLAPSE_THREADS) void ipa_collapse_kernel(uint64_t* __restrict__ g, uint32_t half,
                                                                        const Words4 u, int* sticky) {
  collapse_body<C>(g, half, load_words(u.v), sticky);
}
// u from memory: every lane reads the same words and the first lane's copy is taken, so the
// scalar is wave-uniform for the compiler too and scalar_mul's branches stay uniform
template <class C>
__global__ __launch_bounds__(COLLAPSE_THREADS) void ipa_collapse_ptr_kernel(uint64_t* __restrict__ g, uint32_t half,
                                                                            const uint64_t* __restrict__ chal,
                                                                            int* sticky) {
  Fe u = load(chal);
#pragma unroll
  for (int i = 0; i < 8; i++) u.w[i] = (uint32_t)__builtin_amdgcn_readfirstlane((int)u.w[i]);
  collapse_body<C>(g, half, u, sticky);
}

// ---- the challenge of a round of the one-call opening ------------------------------------------------
// One workgroup of one wave. lr: the blinded (L_j, R_j), affine; four lanes convert the four
// coordinates to their canonical bytes, then lane 0 absorbs the two points, squeezes u_j, inverts
// it and moves f on:  f += l_rand u^-1 + r_rand u  (f and rand in the form). u goes to out_u
// (canonical) and, with its Montgomery form and inverse, to chal for the folds. u = 0 raises
// B2F_ERR_FIELD (halo2 would fail to invert it); its inverse is then written as zero.
template <class C, bool MONT>
__global__ __launch_bounds__(64) void ipa_challenge_kernel(const uint64_t* __restrict__ lr,
                                                           const uint64_t* __restrict__ rand,
                                                           uint64_t* __restrict__ state, uint64_t* __restrict__ out_u,
                                                           uint64_t* __restrict__ chal, uint64_t* __restrict__ f,
                                                           int* sticky) {
  using FS = typename C::Scalar;
  __shared__ transcript::State st;
  __shared__ uint8_t bytes[130];
  const uint32_t t = threadIdx.x;
  if (t < 4) {
    const Fe c = to_canonical<typename C::Base>(load(lr + 4 * t));
    transcript::put_bytes(bytes + 65 * (t >> 1) + 1 + 32 * (t & 1u), c);
    if (!(t & 1u)) bytes[65 * (t >> 1)] = 1;
  }
  __syncthreads();
  if (t != 0) return;
  transcript::tr_load(st, state);
  transcript::tr_absorb(st, bytes, 130);
  const Fe u = transcript::tr_squeeze<FS>(st);
  transcript::tr_store(st, state);
  const Fe u_mont = to_mont<FS>(u);
  bool ok = true;
  Fe uinv_mont = fe_zero();
  if (is_zero(u)) atomicOr(sticky, 1 << B2F_ERR_FIELD);
  else uinv_mont = inv_safegcd<FS>(u_mont, ok);
  if (!ok) atomicOr(sticky, 1 << B2F_ERR_CHECK);
  Fe fm = load(f), l = load(rand), r = load(rand + 4);
  if (!MONT) {
    fm = to_mont<FS>(fm);
    l = to_mont<FS>(l);
    r = to_mont<FS>(r);
  }
  fm = add<FS>(fm, add<FS>(mul<FS>(l, uinv_mont), mul<FS>(r, u_mont)));
  if (!MONT) fm = to_canonical<FS>(fm);
  store(f, fm);
  store(out_u, u);
  store(chal, u);
  store(chal + 4, u_mont);
  store(chal + 8, uinv_mont);
}

// After the last round: c = p[0] to cf[0..3], and c then f (cf[4..7]) absorbed as scalars.
template <class FS, bool MONT>
__global__ __launch_bounds__(64) void ipa_finish_kernel(const uint64_t* __restrict__ p, uint64_t* __restrict__ state,
                                                        uint64_t* __restrict__ cf) {
  __shared__ transcript::State st;
  __shared__ uint8_t stage[33];
  if (threadIdx.x != 0) return;
  const Fe c = load(p), f = load(cf + 4);
  transcript::tr_load(st, state);
  transcript::tr_absorb_scalar(st, stage, MONT ? to_canonical<FS>(c) : c);
  transcript::tr_absorb_scalar(st, stage, MONT ? to_canonical<FS>(f) : f);
  transcript::tr_store(st, state);
  store(cf, c);
}

}  // namespace

uint64_t ipa_direct_max_len() { return IPA_DIRECT_MAX_LEN; }

size_t ipa_scratch_bytes(uint64_t len) {
  const uint64_t half = len / 2, ntiles = (half + IPA_TILE - 1) / IPA_TILE;
  return (size_t)(256 + align256(2 * ntiles * 32));
}

hipError_t launch_ipa_powers(const uint64_t* x, uint64_t len, uint32_t form, uint64_t* d_b, hipStream_t s) {
  with_form(form, [&](auto f, auto mont) {
    hipLaunchKernelGGL((ipa_powers_kernel<decltype(f), decltype(mont)::value>),
                       dim3((uint32_t)((len + IPA_THREADS - 1) / IPA_THREADS)), dim3(IPA_THREADS), 0, s, words4(x), len,
                       d_b);
  });
  return hipGetLastError();
}

hipError_t launch_ipa_round_direct(const uint64_t* d_p, const uint64_t* d_b, const uint64_t* d_g, uint64_t len,
                                   uint32_t form, uint64_t* d_lr, uint64_t* d_values, int* sticky, hipStream_t s) {
  with_curve_form(form, [&](auto c, auto mont) {
    hipLaunchKernelGGL((ipa_round_direct_kernel<decltype(c), decltype(mont)::value>), dim3(4), dim3(IPA_THREADS), 0, s,
                       d_p, d_b, d_g, (uint32_t)(len / 2), d_lr, d_values, sticky);
  });
  return hipGetLastError();
}

hipError_t launch_ipa_round_long(const MsmPlan& plan, const uint64_t* d_p, const uint64_t* d_b, const uint64_t* d_g,
                                 uint64_t len, uint32_t form, uint64_t* d_lr, uint64_t* d_values, void* msm_scratch,
                                 void* ipa_scratch, int* sticky, hipStream_t s) {
  const uint32_t half = (uint32_t)(len / 2), ntiles = (half + IPA_TILE - 1) / IPA_TILE;
  uint64_t* rl = reinterpret_cast<uint64_t*>(ipa_scratch);
  uint64_t* partial = reinterpret_cast<uint64_t*>((char*)ipa_scratch + 256);
  // column 0 = p[..half] against G[half..] (R), column 1 = p[half..] against G[..half] (L)
  const MsmBaseOffsets off = {{half, 0, 0, 0}};
  hipError_t e = launch_msm(plan, d_p, half, half, 2, d_g, form, rl, msm_scratch, sticky, s, &off);
  if (e != hipSuccess) return e;
  with_form(form, [&](auto f, auto mont) {
    using FS = decltype(f);
    hipLaunchKernelGGL((ipa_ip_tiles_kernel<FS>), dim3(ntiles, 2), dim3(IPA_THREADS), 0, s, d_p, d_b, half, ntiles,
                       partial);
    hipLaunchKernelGGL((ipa_combine_kernel<FS, decltype(mont)::value>), dim3(3), dim3(IPA_THREADS), 0, s, partial,
                       ntiles, rl, d_lr, d_values);
  });
  return hipGetLastError();
}

hipError_t launch_ipa_fold(uint64_t* d_p, uint64_t* d_b, uint64_t* d_g, uint64_t len, const uint64_t* u,
                           const uint64_t* u_mont, const uint64_t* uinv_mont, uint32_t form, int* sticky,
                           hipStream_t s) {
  const uint32_t half = (uint32_t)(len / 2);
  with_field(form, [&](auto f) {
    hipLaunchKernelGGL((ipa_fold_scalars_kernel<decltype(f)>), dim3((half + IPA_THREADS - 1) / IPA_THREADS),
                       dim3(IPA_THREADS), 0, s, d_p, d_b, half, words4(u_mont), words4(uinv_mont));
    return 0;
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  with_curve(form, [&](auto c) {
    hipLaunchKernelGGL((ipa_collapse_kernel<decltype(c)>), dim3((half + COLLAPSE_THREADS - 1) / COLLAPSE_THREADS),
                       dim3(COLLAPSE_THREADS), 0, s, d_g, half, words4(u), sticky);
    return 0;
  });
  return hipGetLastError();
}

hipError_t launch_ipa_fold_ptr(uint64_t* d_p, uint64_t* d_b, uint64_t* d_g, uint64_t len, const uint64_t* d_chal,
                               uint32_t form, int* sticky, hipStream_t s) {
  const uint32_t half = (uint32_t)(len / 2);
  with_field(form, [&](auto f) {
    hipLaunchKernelGGL((ipa_fold_scalars_ptr_kernel<decltype(f)>), dim3((half + IPA_THREADS - 1) / IPA_THREADS),
                       dim3(IPA_THREADS), 0, s, d_p, d_b, half, d_chal);
    return 0;
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  with_curve(form, [&](auto c) {
    hipLaunchKernelGGL((ipa_collapse_ptr_kernel<decltype(c)>), dim3((half + COLLAPSE_THREADS - 1) / COLLAPSE_THREADS),
                       dim3(COLLAPSE_THREADS), 0, s, d_g, half, d_chal, sticky);
    return 0;
  });
  return hipGetLastError();
}

hipError_t launch_ipa_challenge(const uint64_t* d_lr, const uint64_t* d_rand, uint64_t* d_state, uint32_t form,
                                uint64_t* d_u, uint64_t* d_chal, uint64_t* d_f, int* sticky, hipStream_t s) {
  with_curve_form(form, [&](auto c, auto mont) {
    hipLaunchKernelGGL((ipa_challenge_kernel<decltype(c), decltype(mont)::value>), dim3(1), dim3(64), 0, s, d_lr,
                       d_rand, d_state, d_u, d_chal, d_f, sticky);
  });
  return hipGetLastError();
}

hipError_t launch_ipa_finish(const uint64_t* d_p, uint64_t* d_state, uint32_t form, uint64_t* d_cf, hipStream_t s) {
  with_form(form, [&](auto f, auto mont) {
    hipLaunchKernelGGL((ipa_finish_kernel<decltype(f), decltype(mont)::value>), dim3(1), dim3(64), 0, s, d_p, d_state,
                       d_cf);
  });
  return hipGetLastError();
}

#ifdef B2F_DIAG
// Diagnostics build only: B2F_DIAG_IPA_DIRECT=<len> read at the call replaces ipa_direct_max_len
// (0: every round takes the Pippenger pass; a value >= 2^28: every round the direct kernel).
// 0: unset; 1: *len holds the forced value; -1: anything but 1..10 decimal digits without a
// leading zero (a lone 0 excepted). There is no fallback: the caller refuses the call on -1.
int diag_ipa_direct(uint64_t* len) {
  const char* v = getenv("B2F_DIAG_IPA_DIRECT");
  *len = 0;
  if (!v) return 0;
  if (v[0] == '0') return v[1] ? -1 : 1;
  uint64_t x = 0;
  int digits = 0;
  for (const char* q = v; *q; q++) {
    if (*q < '0' || *q > '9' || ++digits > 10) return -1;
    x = x * 10 + (uint64_t)(*q - '0');
  }
  if (!digits) return -1;
  *len = x;
  return 1;
}
#endif

}  // namespace b2f
