// b2f_ntt.hip -- batched number-theoretic transform of prover columns (b2f_ntt_columns_dev):
// halo2's lagrange_to_coeff / coeff_to_lagrange / coeff_to_extended over pasta Fp or BN254 Fr,
// on columns of 32-byte elements as every prover-column call here writes them. DESIGN.md §4.4.
//
// Tile transform: a workgroup of 256 threads holds 1,024 elements in LDS, word-planar
// (lds[8][1024 + pad] u32: lanes on consecutive elements hit consecutive banks; one pad word per
// 32 keeps the bit-reversed load conflict-free), as B = 1024 / L independent transforms of
// length L = 2^l. Elements are loaded bit-reversed and the stages run decimation in time, two
// stages per LDS round trip (radix 4 in registers: 4 elements, 4 products), a last radix-2 round
// when l is odd. Butterfly twiddles come from one table of the 2^min(k,10)-th root.
//
// Pass plan (n = 2^k = n_1 n_2 .. n_P, n_d = 2^l[d]):
//   k <= 10        one pass: the tile holds 1024 / n whole columns.
//   k  > 10        P = ceil(k / 8) passes of l[d] <= 8, so every tile holds B >= 4 transforms and
//                  every global access is a run of B (or n_1) adjacent elements, >= 128 bytes.
// Input index i = (i_1 .. i_P), i_1 most significant; output index o = (o_1 .. o_P), o_1 least
// significant. Pass d transforms digit i_d -> o_d and multiplies by omega^(N_prev hi o_d), N_prev
// = n_1 .. n_{d-1}, hi = the natural value of the digits not yet transformed. Pass 1 goes in ->
// out and stores (o_1 | i_2 .. i_P) with the remaining digits in reversed significance (i_2
// lowest); every later pass then works in place on its own index set
// {lo + N_prev (j + n_d h)} for a block of B adjacent (lo, h), and the last one leaves natural
// order. No n-sized scratch.
//
// Scaling: forward multiplies input row i by shift^i while loading it in pass 1; inverse runs the
// same passes with omega^-1 and multiplies output row j by n^-1 shift^-j while storing the last
// pass. Powers come from two-level tables (base^lo, base^(hi 2^h0), h0 = ceil(k / 2)): one extra
// product per use instead of an n-entry table. All table entries are Montgomery form, so data in
// either form goes through unchanged in form (mul(a_canonical, w_mont) = a w canonical).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/b2f.h"
#include "b2f_field.h"
#include "b2f_launch.h"

namespace b2f {

using namespace field;

namespace {

constexpr uint32_t NT_LOG = 10;
constexpr uint32_t NT = 1u << NT_LOG;       // elements per tile
constexpr uint32_t NT_THREADS = 256;
constexpr uint32_t NT_LDSW = NT + NT / 32;  // words per plane, one pad word per 32
constexpr uint32_t NT_MAXP = 4;

// table block of one (field, k, omega, shift, direction), in 32-byte elements:
//   [0, 8)      header (NttHeader)
//   [8, 520)    W[t] = r^t, t < 2^(mlog - 1), r = w^(n / 2^mlog), mlog = min(k, 10)
//   then T0[a] = w^a (a < 2^h0), T1[b] = w^(b 2^h0) (b < 2^(k - h0)),
//        S0[a] = c0 s^a,          S1[b] = s^(b 2^h0)
// with w = omega (forward) or omega^-1, s = shift or shift^-1, c0 = 1 or n^-1.
constexpr uint32_t NT_W_OFF = 8;
constexpr uint32_t NT_T0_OFF = NT_W_OFF + NT / 2;

struct NttHeader {
  Fe w, r, wh, s, sh, c0;
  uint32_t bad;  // omega is not a primitive 2^k-th root of unity
  uint32_t pad[15];
};
static_assert(sizeof(NttHeader) == NT_W_OFF * 32, "header = 8 elements");

struct NttPass {
  const uint64_t* src;
  uint64_t* dst;
  uint64_t src_rows, dst_rows;  // column strides
  uint64_t in_len;              // rows of src that are read (pass 0); the rest are zero
  const uint64_t* tab;
  int* sticky;
  uint32_t k, n_cols, col0;
  uint32_t P, p;
  uint32_t l[NT_MAXP];
  uint32_t h0, mlog;
  uint32_t prescale, postscale;
};

__host__ __device__ inline uint32_t ntt_h0(uint32_t k) { return (k + 1) / 2; }

__device__ __forceinline__ Fe tab_load(const uint64_t* tab, uint32_t idx) { return load(tab + 4ull * idx); }

// One lane: the inverses, the derived roots and the primitive-root check.
template <class F>
__global__ void ntt_setup_kernel(uint64_t* tab, Words4 omega, Words4 shift, uint32_t k, uint32_t inverse) {
  if (blockIdx.x || threadIdx.x) return;
  const uint32_t h0 = ntt_h0(k), mlog = k < NT_LOG ? k : NT_LOG;
  NttHeader H;
  Fe w = to_mont<F>(load_words(omega.v));
  bool bad = is_zero(w);
  if (bad) w = one<F>();
  if (inverse && !bad) w = inv<F>(w);
  Fe t = w;
  for (uint32_t i = 0; i + 1 < k; i++) t = mul<F>(t, t);
  if (!fe_eq(t, sub<F>(fe_zero(), one<F>()))) bad = true;  // w^(n/2) must be -1
  H.w = w;
  Fe r = w;
  for (uint32_t i = 0; i < k - mlog; i++) r = mul<F>(r, r);
  H.r = r;
  Fe wh = w;
  for (uint32_t i = 0; i < h0; i++) wh = mul<F>(wh, wh);
  H.wh = wh;
  Fe s = to_mont<F>(load_words(shift.v));  // non-zero: checked on the host
  if (inverse) s = inv<F>(s);
  H.s = s;
  Fe sh = s;
  for (uint32_t i = 0; i < h0; i++) sh = mul<F>(sh, sh);
  H.sh = sh;
  H.c0 = inverse ? inv<F>(from_u32<F>(1u << k)) : one<F>();
  H.bad = bad ? 1u : 0u;
  for (int i = 0; i < 15; i++) H.pad[i] = 0;
  *reinterpret_cast<NttHeader*>(tab) = H;
}

// One lane per table entry.
template <class F>
__global__ __launch_bounds__(256) void ntt_tables_kernel(uint64_t* tab, uint32_t k) {
  const uint32_t h0 = ntt_h0(k), mlog = k < NT_LOG ? k : NT_LOG;
  const uint32_t nw = 1u << (mlog - 1), n0 = 1u << h0, n1 = 1u << (k - h0);
  const NttHeader* H = reinterpret_cast<const NttHeader*>(tab);
  uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < nw) {
    store(tab + 4ull * (NT_W_OFF + g), fe_pow<F>(H->r, g));
    return;
  }
  g -= nw;
  if (g < n0) {
    store(tab + 4ull * (NT_T0_OFF + g), fe_pow<F>(H->w, g));
    return;
  }
  g -= n0;
  if (g < n1) {
    store(tab + 4ull * (NT_T0_OFF + n0 + g), fe_pow<F>(H->wh, g));
    return;
  }
  g -= n1;
  if (g < n0) {
    store(tab + 4ull * (NT_T0_OFF + n0 + n1 + g), mul<F>(H->c0, fe_pow<F>(H->s, g)));
    return;
  }
  g -= n0;
  if (g < n1) store(tab + 4ull * (NT_T0_OFF + 2 * n0 + n1 + g), fe_pow<F>(H->sh, g));
}

__device__ __forceinline__ uint32_t lds_at(uint32_t q) { return q + (q >> 5); }

__device__ __forceinline__ Fe lds_get(const uint32_t* lds, uint32_t q) {
  const uint32_t a = lds_at(q);
  Fe r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.w[i] = lds[i * NT_LDSW + a];
  return r;
}
__device__ __forceinline__ void lds_put(uint32_t* lds, uint32_t q, const Fe& x) {
  const uint32_t a = lds_at(q);
#pragma unroll
  for (int i = 0; i < 8; i++) lds[i * NT_LDSW + a] = x.w[i];
}

// base^e from a two-level table pair (lo at `off`, hi at `off + 2^h0`)
template <class F>
__device__ __forceinline__ Fe pow2(const uint64_t* tab, uint32_t off, uint32_t h0, uint32_t e) {
  const uint32_t lo = e & ((1u << h0) - 1u), hi = e >> h0;
  return mul<F>(tab_load(tab, off + lo), tab_load(tab, off + (1u << h0) + hi));
}

// The digits not yet transformed after pass p, d = p+1 .. P-1: natural value (digit p+1 most
// significant) <-> stored value (digit p+1 least significant).
__device__ __forceinline__ uint32_t nat_to_sto(const NttPass& a, uint32_t x, uint32_t bits) {
  uint32_t out = 0, sh = 0;
  for (uint32_t d = a.p + 1; d < a.P; d++) {
    bits -= a.l[d];
    out |= ((x >> bits) & ((1u << a.l[d]) - 1u)) << sh;
    sh += a.l[d];
  }
  return out;
}
__device__ __forceinline__ uint32_t sto_to_nat(const NttPass& a, uint32_t x, uint32_t bits) {
  uint32_t out = 0, sh = 0;
  for (uint32_t d = a.p + 1; d < a.P; d++) {
    bits -= a.l[d];
    out |= ((x >> sh) & ((1u << a.l[d]) - 1u)) << bits;
    sh += a.l[d];
  }
  return out;
}

// 4 waves per SIMD (128 VGPRs, 8 bytes of scratch per lane): four workgroups per CU, 132 KiB of
// its LDS. Unbounded, the kernel takes 130-132 VGPRs and runs three; measured 2-3 % slower.
template <class F>
__global__ __launch_bounds__(NT_THREADS, 4) void ntt_pass_kernel(const NttPass a) {
  __shared__ uint32_t lds[8 * NT_LDSW];
  const uint32_t tid = threadIdx.x;
  const uint32_t l = a.l[a.p];
  const bool single = a.P == 1;
  const uint32_t sj = single ? 0u : NT_LOG - l;  // bit offset of the transform index in the tile
  const uint32_t Lm = (1u << l) - 1u, Bm = (1u << sj) - 1u;
  uint32_t lp = 0;  // log2 N_prev
  for (uint32_t d = 0; d < a.p; d++) lp += a.l[d];
  const uint32_t lrem = a.k - lp - l;  // bits of the digits not yet transformed
  const uint32_t nmask = (1u << a.k) - 1u;
  const uint64_t* tab = a.tab;
  const uint32_t n0 = 1u << a.h0, n1 = 1u << (a.k - a.h0);
  const uint32_t t_off = NT_T0_OFF, s_off = NT_T0_OFF + n0 + n1;
  if (a.p == 0 && tid == 0 && blockIdx.x == 0 && blockIdx.y == 0 &&
      reinterpret_cast<const NttHeader*>(tab)->bad)
    atomicOr(a.sticky, 1 << B2F_ERR_FIELD);

  // ---- load, bit-reversed in the transform index
#pragma unroll
  for (uint32_t r = 0; r < NT / NT_THREADS; r++) {
    const uint32_t e = tid + NT_THREADS * r;
    uint32_t b, j, col, row;
    bool valid;
    if (single) {
      j = e & Lm;
      b = e >> l;
      col = a.col0 + blockIdx.y * (NT >> l) + b;
      row = j;
      valid = col < a.n_cols && row < a.in_len;
    } else {
      b = e & Bm;
      j = e >> sj;
      col = a.col0 + blockIdx.y;
      const uint32_t f = (blockIdx.x << sj) + b;
      if (a.p == 0) {
        row = (j << lrem) | f;
        valid = row < a.in_len;
      } else {
        row = (f & ((1u << lp) - 1u)) | (j << lp) | ((f >> lp) << (lp + l));
        valid = true;
      }
    }
    Fe x = fe_zero();
    if (valid) {
      const uint64_t* base = a.p == 0 ? a.src + (uint64_t)col * a.src_rows * 4 : a.dst + (uint64_t)col * a.dst_rows * 4;
      x = load(base + 4ull * row);
      if (a.p == 0 && a.prescale) x = mul<F>(x, pow2<F>(tab, s_off, a.h0, row));
    }
    const uint32_t rj = __brev(j) >> (32 - l);
    lds_put(lds, single ? ((b << l) | rj) : ((rj << sj) | b), x);
  }
  __syncthreads();

  // ---- stages: two per round trip, then one if l is odd
  uint32_t s = 0;
  for (; s + 1 < l; s += 2) {
    const uint32_t p0 = s + sj;
    const uint32_t q00 = ((tid >> p0) << (p0 + 2)) | (tid & ((1u << p0) - 1u));
    const uint32_t q01 = q00 | (1u << p0), q10 = q00 | (2u << p0), q11 = q00 | (3u << p0);
    const uint32_t jl = (q00 >> sj) & ((1u << s) - 1u);
    Fe x0 = lds_get(lds, q00), x1 = lds_get(lds, q01), x2 = lds_get(lds, q10), x3 = lds_get(lds, q11);
    {
      const Fe t = tab_load(tab, NT_W_OFF + (jl << (a.mlog - s - 1)));
      const Fe m1 = mul<F>(x1, t), m3 = mul<F>(x3, t);
      x1 = sub<F>(x0, m1);
      x0 = add<F>(x0, m1);
      x3 = sub<F>(x2, m3);
      x2 = add<F>(x2, m3);
    }
    {
      const Fe ta = tab_load(tab, NT_W_OFF + (jl << (a.mlog - s - 2)));
      const Fe tb = tab_load(tab, NT_W_OFF + ((jl + (1u << s)) << (a.mlog - s - 2)));
      const Fe m2 = mul<F>(x2, ta), m3 = mul<F>(x3, tb);
      x2 = sub<F>(x0, m2);
      x0 = add<F>(x0, m2);
      x3 = sub<F>(x1, m3);
      x1 = add<F>(x1, m3);
    }
    lds_put(lds, q00, x0);
    lds_put(lds, q01, x1);
    lds_put(lds, q10, x2);
    lds_put(lds, q11, x3);
    __syncthreads();
  }
  if (s < l) {
    const uint32_t p0 = s + sj;
#pragma unroll 1
    for (uint32_t r = 0; r < 2; r++) {
      const uint32_t u = tid + NT_THREADS * r;
      const uint32_t q0 = ((u >> p0) << (p0 + 1)) | (u & ((1u << p0) - 1u));
      const uint32_t q1 = q0 | (1u << p0);
      const uint32_t jl = (q0 >> sj) & ((1u << s) - 1u);
      const Fe t = tab_load(tab, NT_W_OFF + (jl << (a.mlog - s - 1)));
      const Fe x0 = lds_get(lds, q0);
      const Fe m = mul<F>(lds_get(lds, q1), t);
      lds_put(lds, q0, add<F>(x0, m));
      lds_put(lds, q1, sub<F>(x0, m));
    }
    __syncthreads();
  }

  // ---- store: inter-pass twiddle, or the inverse's scale on the last pass
#pragma unroll 1
  for (uint32_t r = 0; r < NT / NT_THREADS; r++) {
    const uint32_t e = tid + NT_THREADS * r;
    if (single) {
      const uint32_t j = e & Lm, b = e >> l;
      const uint32_t col = a.col0 + blockIdx.y * (NT >> l) + b;
      if (col >= a.n_cols) continue;
      Fe x = lds_get(lds, e);
      if (a.postscale) x = mul<F>(x, pow2<F>(tab, s_off, a.h0, j));
      store(a.dst + ((uint64_t)col * a.dst_rows + j) * 4, x);
      continue;
    }
    uint64_t* out = a.dst + (uint64_t)(a.col0 + blockIdx.y) * a.dst_rows * 4;
    if (a.p == 0) {  // o fastest: runs of n_1 adjacent output rows
      const uint32_t o = e & Lm, b = e >> l;
      const uint32_t f = (blockIdx.x << sj) + b;  // natural value of the remaining digits
      Fe x = lds_get(lds, (o << sj) | b);
      const uint32_t ex = (uint32_t)(((uint64_t)f * o) & nmask);
      x = mul<F>(x, pow2<F>(tab, t_off, a.h0, ex));
      store(out + 4ull * (o | (nat_to_sto(a, f, lrem) << l)), x);
    } else {
      const uint32_t b = e & Bm, o = e >> sj;
      const uint32_t f = (blockIdx.x << sj) + b;
      const uint32_t lo = f & ((1u << lp) - 1u), h = f >> lp;
      const uint32_t row = lo | (o << lp) | (h << (lp + l));
      Fe x = lds_get(lds, e);
      if (a.p + 1 < a.P) {
        const uint32_t hn = sto_to_nat(a, h, lrem);
        const uint32_t ex = (uint32_t)((((uint64_t)hn << lp) * o) & nmask);
        x = mul<F>(x, pow2<F>(tab, t_off, a.h0, ex));
      } else if (a.postscale) {
        x = mul<F>(x, pow2<F>(tab, s_off, a.h0, row));
      }
      store(out + 4ull * row, x);
    }
  }
}

void ntt_plan(uint32_t k, uint32_t* P, uint32_t* l) {
  for (uint32_t d = 0; d < NT_MAXP; d++) l[d] = 0;
  if (k <= NT_LOG) {
    *P = 1;
    l[0] = k;
    return;
  }
  const uint32_t np = (k + 7) / 8;
  for (uint32_t d = 0; d < np; d++) l[d] = k / np + (d < k % np ? 1u : 0u);
  *P = np;
}

}  // namespace

// The plan a k gets (host): out = {P, l[0..3]}.
void ntt_plan_of(uint32_t k, uint32_t* out) { ntt_plan(k, out, out + 1); }

size_t ntt_table_bytes(uint32_t k) {
  const uint32_t h0 = ntt_h0(k);
  return 32ull * (NT_T0_OFF + 2ull * ((1ull << h0) + (1ull << (k - h0))));
}

// Fill a table block for (field of form, k, omega, shift, direction).
hipError_t launch_ntt_tables(void* d_tab, uint32_t form, uint32_t k, const uint64_t* omega,
                             const uint64_t* shift, uint32_t direction, hipStream_t s) {
  uint64_t* tab = static_cast<uint64_t*>(d_tab);
  const uint32_t h0 = ntt_h0(k), mlog = k < NT_LOG ? k : NT_LOG;
  const uint32_t total = (1u << (mlog - 1)) + 2u * ((1u << h0) + (1u << (k - h0)));
  with_field(form, [&](auto f) {
    using F = decltype(f);
    hipLaunchKernelGGL(ntt_setup_kernel<F>, dim3(1), dim3(64), 0, s, tab, words4(omega), words4(shift), k, direction);
    hipLaunchKernelGGL(ntt_tables_kernel<F>, dim3((total + 255) / 256), dim3(256), 0, s, tab, k);
  });
  return hipGetLastError();
}

hipError_t launch_ntt(const uint64_t* d_in, uint64_t in_rows, uint64_t in_len, uint32_t n_cols,
                      uint32_t k, uint32_t form, uint32_t direction, bool shift_is_one, uint64_t* d_out,
                      uint64_t out_rows, const void* d_tab, int* sticky, hipStream_t s,
                      const uint32_t* plan) {
  NttPass a;
  a.src = d_in;
  a.dst = d_out;
  a.src_rows = in_rows;
  a.dst_rows = out_rows;
  a.in_len = in_len;
  a.tab = static_cast<const uint64_t*>(d_tab);
  a.sticky = sticky;
  a.k = k;
  a.n_cols = n_cols;
  // plan: {P, l[0..3]} in place of ntt_plan's (diagnostics library only, checked by its caller:
  // k > 10, 2 <= P <= 4, every l[d] in 1..8, their sum k); null from every product caller
  if (plan) {
    a.P = plan[0];
    for (uint32_t d = 0; d < NT_MAXP; d++) a.l[d] = d < plan[0] ? plan[1 + d] : 0u;
  } else {
    ntt_plan(k, &a.P, a.l);
  }
  a.h0 = ntt_h0(k);
  a.mlog = k < NT_LOG ? k : NT_LOG;
  a.prescale = direction == B2F_NTT_FORWARD && !shift_is_one;
  a.postscale = direction == B2F_NTT_INVERSE;
  const uint32_t per_y = a.P == 1 ? NT >> k : 1u;  // columns per grid row
  const uint32_t tiles = a.P == 1 ? 1u : 1u << (k - NT_LOG);
  const uint64_t max_cols = 65535ull * per_y;
  for (uint64_t c0 = 0; c0 < n_cols; c0 += max_cols) {
    const uint64_t nc = n_cols - c0 < max_cols ? n_cols - c0 : max_cols;
    const dim3 grid(tiles, (uint32_t)((nc + per_y - 1) / per_y));
    a.col0 = (uint32_t)c0;
    for (uint32_t p = 0; p < a.P; p++) {
      a.p = p;
      with_field(form,
                 [&](auto f) { hipLaunchKernelGGL(ntt_pass_kernel<decltype(f)>, grid, dim3(NT_THREADS), 0, s, a); });
    }
  }
  return hipGetLastError();
}

}  // namespace b2f
