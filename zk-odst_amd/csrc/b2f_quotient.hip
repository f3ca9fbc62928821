// b2f_quotient.hip -- the permutation and lookup terms of the quotient numerator on the extended
// coset and the division by the vanishing polynomial (b2f_lagrange_selectors_dev,
// b2f_quotient_permutation_dev, b2f_quotient_lookup_dev, b2f_quotient_divide_dev): halo2_proofs
// 0.3.0 plonk/permutation/prover.rs Committed::construct, plonk/lookup/prover.rs
// Committed::construct and EvaluationDomain::divide_by_vanishing_poly. DESIGN.md §4.5.
//
// One thread per extended row, one pass per call: every column element is a pair of 16-byte loads
// (adjacent lanes read adjacent 32-byte elements), each term is folded into the row's accumulator
// as soon as it is formed, and one element is stored. Nothing is written but h.
//
// The arithmetic is Montgomery-form whatever `form` is: the canonical forms convert at load and
// store (one product each way). The challenges reach the kernels as a block of Montgomery-form
// constants that a one-lane kernel writes first (QuotConsts; uniform loads in the row kernels).
//
// X_i = shift omega_ext^i comes from a two-level table, X_i = T0[i mod 2^h0] T1[i >> h0] with
// T0[a] = shift omega^a, T1[b] = omega^(b 2^h0), h0 = ceil(ext_k / 2): one product per row and
// 2^h0 + 2^(ext_k - h0) entries (48 KiB at ext_k = 19, L2-resident) instead of an n_ext-entry
// column. The context caches the block per (field, ext_k, omega, shift), and the inverse divisors
// of the vanishing divide per (field, k, ext_k, omega, shift).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/b2f.h"
#include "b2f_field.h"

namespace b2f {

using namespace field;

namespace {

constexpr uint32_t QT_THREADS = 256;

// table block of one (field, ext_k, omega, shift), in 32-byte elements:
//   [0]  header: word 0 != 0 when omega is not a primitive 2^ext_k-th root of unity
//   then T0[a] = shift omega^a (a < 2^h0), T1[b] = omega^(b 2^h0) (b < 2^(ext_k - h0))
constexpr uint32_t QT_T0_OFF = 1;

struct Words4 {
  uint64_t v[4];
};

// the challenges of one call, Montgomery form
struct QuotConsts {
  Fe beta, gamma, y;
  Fe ys;     // y^sets
  Fe bd[8];  // beta delta^j
};

__host__ __device__ inline uint32_t quot_h0(uint32_t ext_k) { return (ext_k + 1) / 2; }

template <class F>
__device__ __forceinline__ bool primitive_root(const Fe& w, uint32_t k) {  // w^(2^(k-1)) == -1
  Fe t = w;
  for (uint32_t i = 0; i + 1 < k; i++) t = mul<F>(t, t);
  return fe_eq(t, sub<F>(fe_zero(), one<F>()));
}

template <class F, bool MONT>
__device__ __forceinline__ Fe ld(const uint64_t* p) {
  const Fe x = load(p);
  return MONT ? x : to_mont<F>(x);
}
template <class F, bool MONT>
__device__ __forceinline__ void st(uint64_t* p, const Fe& x) {
  store(p, MONT ? x : to_canonical<F>(x));
}

// One lane per table entry; lane 0 also checks the root.
template <class F>
__global__ __launch_bounds__(QT_THREADS) void quot_xtab_kernel(uint64_t* tab, Words4 omega, Words4 shift,
                                                               uint32_t ext_k) {
  const uint32_t h0 = quot_h0(ext_k), n0 = 1u << h0, n1 = 1u << (ext_k - h0);
  const uint32_t g = blockIdx.x * QT_THREADS + threadIdx.x;
  if (g >= n0 + n1) return;
  const Fe w = to_mont<F>(load_words(omega.v));
  if (g == 0) {
    Fe hdr = fe_zero();
    hdr.w[0] = primitive_root<F>(w, ext_k) ? 0u : 1u;
    store(tab, hdr);
  }
  if (g < n0) {
    store(tab + 4ull * (QT_T0_OFF + g), mul<F>(to_mont<F>(load_words(shift.v)), fe_pow<F>(w, g)));
    return;
  }
  Fe wh = w;
  for (uint32_t i = 0; i < h0; i++) wh = mul<F>(wh, wh);
  store(tab + 4ull * (QT_T0_OFF + g), fe_pow<F>(wh, g - n0));
}

// One lane: the challenges as Montgomery-form constants.
template <class F>
__global__ void quot_consts_kernel(QuotConsts* c, Words4 beta, Words4 gamma, Words4 y, Words4 delta,
                                   uint32_t sets) {
  if (blockIdx.x || threadIdx.x) return;
  const Fe b = to_mont<F>(load_words(beta.v)), d = to_mont<F>(load_words(delta.v));
  const Fe yy = to_mont<F>(load_words(y.v));
  c->beta = b;
  c->gamma = to_mont<F>(load_words(gamma.v));
  c->y = yy;
  c->ys = fe_pow<F>(yy, sets);
  Fe t = b;
  for (int j = 0; j < 8; j++) {
    c->bd[j] = t;
    t = mul<F>(t, d);
  }
}

// l_0, l_last, l_active over the 2^k rows of the Lagrange basis
template <class F>
__global__ __launch_bounds__(QT_THREADS) void quot_selectors_kernel(uint64_t* out, uint64_t out_rows,
                                                                    uint32_t n, uint32_t usable,
                                                                    uint32_t mont) {
  const uint32_t i = blockIdx.x * QT_THREADS + threadIdx.x;
  if (i >= n) return;
  const Fe z = fe_zero();
  Fe o = z;
  o.w[0] = 1;
  if (mont) o = one<F>();
  store(out + 4ull * i, i == 0 ? o : z);
  store(out + 4ull * (out_rows + i), i == usable ? o : z);
  store(out + 4ull * (2 * out_rows + i), i < usable ? o : z);
}

struct QuotPerm {
  const uint64_t *l, *adv, *sigma, *z, *h_in;
  uint64_t* h_out;
  const uint64_t* xtab;
  const QuotConsts* c;
  int* sticky;
  uint64_t rows;        // column stride of every block
  uint32_t ext_k, rot;  // rot = 2^(ext_k - k) extended rows per circuit row
  uint32_t last_rot;    // usable_rows * rot: the rotation that links two sets
  uint32_t chunk_len, sets;
  uint32_t colmap;      // nibble j: the advice column of v_j
};

// Terms in halo2's order: e_0, e_1, the sets - 1 links, the sets products; T = 2 sets + 1. The
// first sets + 1 fold into `head` and the products into `prod` in the same loop over the sets, so
// z_s of the row is loaded once for its link and its product: h = head y^sets + prod.
template <class F, bool MONT>
__global__ __launch_bounds__(QT_THREADS) void quot_perm_kernel(const QuotPerm a) {
  const uint32_t i = blockIdx.x * QT_THREADS + threadIdx.x;
  const uint32_t mask = (1u << a.ext_k) - 1u;
  if (i == 0 && (uint32_t)a.xtab[0]) atomicOr(a.sticky, 1 << B2F_ERR_FIELD);
  if (i > mask) return;
  const QuotConsts& c = *a.c;
  const uint32_t h0 = quot_h0(a.ext_k);
  const Fe x = mul<F>(load(a.xtab + 4ull * (QT_T0_OFF + (i & ((1u << h0) - 1u)))),
                      load(a.xtab + 4ull * (QT_T0_OFF + (1u << h0) + (i >> h0))));
  const Fe l0 = ld<F, MONT>(a.l + 4ull * i);
  const Fe lact = ld<F, MONT>(a.l + 4ull * (2 * a.rows + i));
  Fe head = a.h_in ? ld<F, MONT>(a.h_in + 4ull * i) : fe_zero();
  Fe zc = ld<F, MONT>(a.z + 4ull * i);
  head = add<F>(mul<F>(head, c.y), mul<F>(l0, sub<F>(one<F>(), zc)));
  {
    const Fe zl = a.sets > 1 ? ld<F, MONT>(a.z + 4ull * ((a.sets - 1) * a.rows + i)) : zc;
    const Fe llast = ld<F, MONT>(a.l + 4ull * (a.rows + i));
    head = add<F>(mul<F>(head, c.y), mul<F>(llast, sub<F>(mul<F>(zl, zl), zl)));
  }
  const uint32_t i_next = (i + a.rot) & mask, i_link = (i + a.last_rot) & mask;
  Fe prod = fe_zero();
  uint32_t j = 0;
#pragma unroll 1
  for (uint32_t s = 0; s < a.sets; s++) {
    const uint64_t* zs = a.z + 4ull * s * a.rows;
    if (s) {
      zc = ld<F, MONT>(zs + 4ull * i);
      const Fe zp = ld<F, MONT>(zs - 4ull * a.rows + 4ull * i_link);
      head = add<F>(mul<F>(head, c.y), mul<F>(l0, sub<F>(zc, zp)));
    }
    Fe left = ld<F, MONT>(zs + 4ull * i_next), right = zc;
    const uint32_t j_end = j + a.chunk_len < 8u ? j + a.chunk_len : 8u;
#pragma unroll 1
    for (; j < j_end; j++) {
      const uint32_t col = (a.colmap >> (4 * j)) & 15u;
      const Fe vg = add<F>(ld<F, MONT>(a.adv + 4ull * (col * a.rows + i)), c.gamma);
      const Fe sg = ld<F, MONT>(a.sigma + 4ull * (j * a.rows + i));
      left = mul<F>(left, add<F>(vg, mul<F>(c.beta, sg)));
      right = mul<F>(right, add<F>(vg, mul<F>(c.bd[j], x)));
    }
    prod = add<F>(mul<F>(prod, c.y), mul<F>(lact, sub<F>(left, right)));
  }
  st<F, MONT>(a.h_out + 4ull * i, add<F>(mul<F>(head, c.ys), prod));
}

struct QuotLookup {
  const uint64_t *l, *lk, *h_in;
  uint64_t* h_out;
  const QuotConsts* c;
  uint64_t rows;
  uint32_t ext_k, rot;
};

template <class F, bool MONT>
__global__ __launch_bounds__(QT_THREADS) void quot_lookup_kernel(const QuotLookup a) {
  const uint32_t i = blockIdx.x * QT_THREADS + threadIdx.x;
  const uint32_t mask = (1u << a.ext_k) - 1u;
  if (i > mask) return;
  const QuotConsts& c = *a.c;
  const uint32_t i_next = (i + a.rot) & mask, i_prev = (i - a.rot) & mask;
  const Fe l0 = ld<F, MONT>(a.l + 4ull * i);
  const Fe lact = ld<F, MONT>(a.l + 4ull * (2 * a.rows + i));
  const Fe z = ld<F, MONT>(a.lk + 4ull * (4 * a.rows + i));
  Fe h = a.h_in ? ld<F, MONT>(a.h_in + 4ull * i) : fe_zero();
  h = add<F>(mul<F>(h, c.y), mul<F>(l0, sub<F>(one<F>(), z)));
  {
    const Fe llast = ld<F, MONT>(a.l + 4ull * (a.rows + i));
    h = add<F>(mul<F>(h, c.y), mul<F>(llast, sub<F>(mul<F>(z, z), z)));
  }
  const Fe ap = ld<F, MONT>(a.lk + 4ull * (2 * a.rows + i));
  const Fe sp = ld<F, MONT>(a.lk + 4ull * (3 * a.rows + i));
  {
    const Fe zn = ld<F, MONT>(a.lk + 4ull * (4 * a.rows + i_next));
    const Fe left = mul<F>(mul<F>(zn, add<F>(ap, c.beta)), add<F>(sp, c.gamma));
    const Fe ain = ld<F, MONT>(a.lk + 4ull * i);
    const Fe tab = ld<F, MONT>(a.lk + 4ull * (a.rows + i));
    const Fe right = mul<F>(mul<F>(z, add<F>(ain, c.beta)), add<F>(tab, c.gamma));
    h = add<F>(mul<F>(h, c.y), mul<F>(lact, sub<F>(left, right)));
  }
  const Fe d = sub<F>(ap, sp);
  h = add<F>(mul<F>(h, c.y), mul<F>(l0, d));
  const Fe apm = ld<F, MONT>(a.lk + 4ull * (2 * a.rows + i_prev));
  h = add<F>(mul<F>(h, c.y), mul<F>(mul<F>(lact, d), sub<F>(ap, apm)));
  st<F, MONT>(a.h_out + 4ull * i, h);
}

// (X_i^n - 1)^-1 has period rot = 2^(ext_k - k) in i: X_i^n = shift^n (omega^n)^(i mod rot).
// Divisor block of one (field, k, ext_k, omega, shift), in 32-byte elements: [0] header, word 0 =
// QT_DIV_FIELD when omega is no primitive root or some divisor is zero (| QT_DIV_CHECK when an
// inversion did not converge), zeroed before the launch; then the rot inverses. One lane per
// residue; lane 0 also checks the root.
constexpr uint32_t QT_DIV_FIELD = 1, QT_DIV_CHECK = 2;

template <class F>
__global__ __launch_bounds__(QT_THREADS) void quot_divisor_kernel(uint64_t* dtab, Words4 omega, Words4 shift,
                                                                  uint32_t k, uint32_t ext_k) {
  const uint32_t r = blockIdx.x * QT_THREADS + threadIdx.x;
  if (r >= (1u << (ext_k - k))) return;
  uint32_t* flags = reinterpret_cast<uint32_t*>(dtab);
  const Fe w = to_mont<F>(load_words(omega.v));
  if (r == 0 && !primitive_root<F>(w, ext_k)) atomicOr(flags, QT_DIV_FIELD);
  Fe zeta = w, sn = to_mont<F>(load_words(shift.v));
  for (uint32_t i = 0; i < k; i++) {
    zeta = mul<F>(zeta, zeta);
    sn = mul<F>(sn, sn);
  }
  const Fe d = sub<F>(mul<F>(sn, fe_pow<F>(zeta, r)), one<F>());
  Fe di = fe_zero();
  if (is_zero(d)) {
    atomicOr(flags, QT_DIV_FIELD);
  } else {
    bool ok;
    di = inv_safegcd<F>(d, ok);
    if (!ok) atomicOr(flags, QT_DIV_CHECK);
  }
  store(dtab + 4ull * (1 + r), di);
}

// The table entries are Montgomery form, so h goes through in either form unchanged in form
// (mul(a canonical, w Montgomery) = a w canonical).
template <class F>
__global__ __launch_bounds__(QT_THREADS) void quot_divide_kernel(const uint64_t* h_in, uint64_t* h_out,
                                                                 const uint64_t* dtab, uint32_t ext_k,
                                                                 uint32_t rot, int* sticky) {
  const uint32_t i = blockIdx.x * QT_THREADS + threadIdx.x;
  if (i == 0) {
    const uint32_t flags = (uint32_t)dtab[0];
    if (flags & QT_DIV_FIELD) atomicOr(sticky, 1 << B2F_ERR_FIELD);
    if (flags & QT_DIV_CHECK) atomicOr(sticky, 1 << B2F_ERR_CHECK);
  }
  if (i >> ext_k) return;
  store(h_out + 4ull * i, mul<F>(load(h_in + 4ull * i), load(dtab + 4ull * (1 + (i & (rot - 1u))))));
}

Words4 words4(const uint64_t* v) {
  Words4 w;
  for (int i = 0; i < 4; i++) w.v[i] = v[i];
  return w;
}

dim3 row_grid(uint32_t log_rows) { return dim3(((1u << log_rows) + QT_THREADS - 1) / QT_THREADS); }

void launch_consts(uint32_t form, void* d_consts, const uint64_t* beta, const uint64_t* gamma, const uint64_t* y,
                   const uint64_t* delta, uint32_t sets, hipStream_t s) {
  QuotConsts* c = static_cast<QuotConsts*>(d_consts);
  if ((form >> 1) & 1u)
    hipLaunchKernelGGL(quot_consts_kernel<Bn254>, dim3(1), dim3(64), 0, s, c, words4(beta), words4(gamma),
                       words4(y), words4(delta), sets);
  else
    hipLaunchKernelGGL(quot_consts_kernel<Pallas>, dim3(1), dim3(64), 0, s, c, words4(beta), words4(gamma),
                       words4(y), words4(delta), sets);
}

}  // namespace

size_t quot_xtab_bytes(uint32_t ext_k) {
  const uint32_t h0 = quot_h0(ext_k);
  return 32ull * (QT_T0_OFF + (1ull << h0) + (1ull << (ext_k - h0)));
}

size_t quot_consts_bytes() { return sizeof(QuotConsts); }

hipError_t launch_quot_xtab(void* d_tab, uint32_t form, uint32_t ext_k, const uint64_t* omega,
                            const uint64_t* shift, hipStream_t s) {
  const uint32_t h0 = quot_h0(ext_k);
  const uint32_t total = (1u << h0) + (1u << (ext_k - h0));
  const dim3 grid((total + QT_THREADS - 1) / QT_THREADS);
  uint64_t* tab = static_cast<uint64_t*>(d_tab);
  if ((form >> 1) & 1u)
    hipLaunchKernelGGL(quot_xtab_kernel<Bn254>, grid, dim3(QT_THREADS), 0, s, tab, words4(omega), words4(shift), ext_k);
  else
    hipLaunchKernelGGL(quot_xtab_kernel<Pallas>, grid, dim3(QT_THREADS), 0, s, tab, words4(omega), words4(shift), ext_k);
  return hipGetLastError();
}

hipError_t launch_lagrange_selectors(uint32_t k, uint32_t usable_rows, uint32_t form, uint64_t* d_out,
                                     uint64_t out_rows, hipStream_t s) {
  if ((form >> 1) & 1u)
    hipLaunchKernelGGL(quot_selectors_kernel<Bn254>, row_grid(k), dim3(QT_THREADS), 0, s, d_out, out_rows,
                       1u << k, usable_rows, form & 1u);
  else
    hipLaunchKernelGGL(quot_selectors_kernel<Pallas>, row_grid(k), dim3(QT_THREADS), 0, s, d_out, out_rows,
                       1u << k, usable_rows, form & 1u);
  return hipGetLastError();
}

hipError_t launch_quot_permutation(uint32_t k, uint32_t ext_k, uint32_t usable_rows, const uint64_t* d_l,
                                   const uint64_t* d_advice, const uint64_t* d_sigma, const uint64_t* d_z,
                                   uint32_t chunk_len, uint64_t rows, const uint64_t* delta,
                                   const uint64_t* beta, const uint64_t* gamma, const uint64_t* y,
                                   const uint64_t* d_h_in, uint64_t* d_h_out, uint32_t form, uint32_t colmap,
                                   const void* d_xtab, void* d_consts, int* sticky, hipStream_t s) {
  QuotPerm a;
  a.l = d_l;
  a.adv = d_advice;
  a.sigma = d_sigma;
  a.z = d_z;
  a.h_in = d_h_in;
  a.h_out = d_h_out;
  a.xtab = static_cast<const uint64_t*>(d_xtab);
  a.c = static_cast<const QuotConsts*>(d_consts);
  a.sticky = sticky;
  a.rows = rows;
  a.ext_k = ext_k;
  a.rot = 1u << (ext_k - k);
  a.last_rot = usable_rows << (ext_k - k);
  a.chunk_len = chunk_len;
  a.sets = (8 + chunk_len - 1) / chunk_len;
  a.colmap = colmap;
  launch_consts(form, d_consts, beta, gamma, y, delta, a.sets, s);
  const dim3 block(QT_THREADS), grid = row_grid(ext_k);
  switch (form) {
    case B2F_FP_CANONICAL:
      hipLaunchKernelGGL((quot_perm_kernel<Pallas, false>), grid, block, 0, s, a);
      break;
    case B2F_FP_MONTGOMERY:
      hipLaunchKernelGGL((quot_perm_kernel<Pallas, true>), grid, block, 0, s, a);
      break;
    case B2F_FP_BN254_CANONICAL:
      hipLaunchKernelGGL((quot_perm_kernel<Bn254, false>), grid, block, 0, s, a);
      break;
    default:
      hipLaunchKernelGGL((quot_perm_kernel<Bn254, true>), grid, block, 0, s, a);
  }
  return hipGetLastError();
}

hipError_t launch_quot_lookup(uint32_t k, uint32_t ext_k, const uint64_t* d_l, const uint64_t* d_lookup,
                              uint64_t rows, const uint64_t* beta, const uint64_t* gamma, const uint64_t* y,
                              const uint64_t* d_h_in, uint64_t* d_h_out, uint32_t form, void* d_consts,
                              hipStream_t s) {
  QuotLookup a;
  a.l = d_l;
  a.lk = d_lookup;
  a.h_in = d_h_in;
  a.h_out = d_h_out;
  a.c = static_cast<const QuotConsts*>(d_consts);
  a.rows = rows;
  a.ext_k = ext_k;
  a.rot = 1u << (ext_k - k);
  const uint64_t one_w[4] = {1, 0, 0, 0};  // delta: the lookup has no identity columns
  launch_consts(form, d_consts, beta, gamma, y, one_w, 0, s);
  const dim3 block(QT_THREADS), grid = row_grid(ext_k);
  switch (form) {
    case B2F_FP_CANONICAL:
      hipLaunchKernelGGL((quot_lookup_kernel<Pallas, false>), grid, block, 0, s, a);
      break;
    case B2F_FP_MONTGOMERY:
      hipLaunchKernelGGL((quot_lookup_kernel<Pallas, true>), grid, block, 0, s, a);
      break;
    case B2F_FP_BN254_CANONICAL:
      hipLaunchKernelGGL((quot_lookup_kernel<Bn254, false>), grid, block, 0, s, a);
      break;
    default:
      hipLaunchKernelGGL((quot_lookup_kernel<Bn254, true>), grid, block, 0, s, a);
  }
  return hipGetLastError();
}

size_t quot_divisor_bytes(uint32_t k, uint32_t ext_k) { return 32ull * (1 + (1ull << (ext_k - k))); }

// Fill a divisor block for (field of form, k, ext_k, omega, shift).
hipError_t launch_quot_divisors(void* d_dtab, uint32_t form, uint32_t k, uint32_t ext_k, const uint64_t* omega,
                                const uint64_t* shift, hipStream_t s) {
  uint64_t* dtab = static_cast<uint64_t*>(d_dtab);
  const hipError_t e = hipMemsetAsync(dtab, 0, 32, s);
  if (e != hipSuccess) return e;
  const dim3 block(QT_THREADS), grid = row_grid(ext_k - k);
  if ((form >> 1) & 1u)
    hipLaunchKernelGGL(quot_divisor_kernel<Bn254>, grid, block, 0, s, dtab, words4(omega), words4(shift), k, ext_k);
  else
    hipLaunchKernelGGL(quot_divisor_kernel<Pallas>, grid, block, 0, s, dtab, words4(omega), words4(shift), k, ext_k);
  return hipGetLastError();
}

hipError_t launch_quot_divide(uint32_t k, uint32_t ext_k, const uint64_t* d_h_in, uint64_t* d_h_out,
                              uint32_t form, const void* d_dtab, int* sticky, hipStream_t s) {
  const uint64_t* dtab = static_cast<const uint64_t*>(d_dtab);
  const uint32_t rot = 1u << (ext_k - k);
  if ((form >> 1) & 1u)
    hipLaunchKernelGGL(quot_divide_kernel<Bn254>, row_grid(ext_k), dim3(QT_THREADS), 0, s, d_h_in, d_h_out, dtab,
                       ext_k, rot, sticky);
  else
    hipLaunchKernelGGL(quot_divide_kernel<Pallas>, row_grid(ext_k), dim3(QT_THREADS), 0, s, d_h_in, d_h_out, dtab,
                       ext_k, rot, sticky);
  return hipGetLastError();
}

}  // namespace b2f
