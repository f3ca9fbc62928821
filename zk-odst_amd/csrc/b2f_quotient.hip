// b2f_quotient.hip -- the custom-gate, permutation and lookup terms of the quotient numerator on
// the extended coset and the division by the vanishing polynomial (b2f_lagrange_selectors_dev,
// b2f_quotient_gates_dev, b2f_quotient_permutation_dev, b2f_quotient_lookup_dev,
// b2f_quotient_divide_dev): the gates of docs/LAYOUT.md §4 and halo2_proofs
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
#include "b2f_launch.h"

namespace b2f {

using namespace field;

namespace {

constexpr uint32_t QT_THREADS = 256;

// table block of one (field, ext_k, omega, shift), in 32-byte elements:
//   [0]  header: word 0 != 0 when omega is not a primitive 2^ext_k-th root of unity
//   then T0[a] = shift omega^a (a < 2^h0), T1[b] = omega^(b 2^h0) (b < 2^(ext_k - h0))
constexpr uint32_t QT_T0_OFF = 1;

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

// ---------------------------------------------------------------------------------------------
// The custom-gate terms (b2f_quotient_gates_dev): the 74 polynomials of docs/LAYOUT.md §4, each
// times its selector column, folded with y in the order of docs/LAYOUT.md §4.1.
//
// With m_g polynomials p_g,0 .. p_g,m-1 in gate g and S_g terms after the gate's last one,
//   h_out = y^74 h_in + sum_g (q_g y^S_g) P_g,   P_g = sum_t y^(m_g - 1 - t) p_g,t  (Horner in y),
// so a gate costs m_g - 1 Horner products, one for its selector and one for P_g instead of 2 m_g,
// the gates may be visited in any order, and gates with the same polynomials (3/7, 5/9, 6/10/12)
// share P_g: (q_3 y^S_3 + q_7 y^S_7) P_3. The XOR limb sum X_k = a_3 + a_4 - a_2 - 2 a_2@+1 is
// formed once per k for bits 6/10/12, 8 and 13, the dense sum of the ADD blocks once for bits
// 3/7 and 5/9. The weights and the powers of y are Montgomery constants written by a one-lane
// kernel (GateConsts); 2 a and 4 a are doublings.
//
// A thread streams gate by gate: at most three Horner accumulators and one X_k are live next to
// the row's accumulator, never the 67 advice cells of the row. Rotated reads are other rows of the
// same columns, (i + j rot) mod n_ext with n_ext a power of two (a mask: exact even where 11 rot
// exceeds n_ext); lanes sit on adjacent rows, so every one is as coalesced as the rotation-0 read.
// The re-reads (a row's cells are read by up to 12 rows, all within 11 rot rows) are left to the
// caches; the tile order below keeps neighbouring tiles on one L2. DESIGN.md §4.5.

// halo2 column of a_i (b2f_halo2_column_index)
constexpr uint32_t GA0 = 7, GA1 = 8, GA2 = 9, GA3 = 1, GA4 = 2, GA5 = 0, GA6 = 3, GA7 = 4, GA8 = 5, GA9 = 6;
constexpr uint32_t QG_TERMS = 74;
constexpr uint32_t QG_COUNT[16] = {2, 8, 8, 2, 12, 2, 4, 2, 12, 2, 4, 2, 4, 4, 1, 5};

// The cells quot_gates_kernel reads: QG_READS[g][i] has bit j set when gate g reads a_i@j (the
// A(GAi, j) calls of the kernel's blocks, gate by gate; k_0 and the selectors are fixed columns,
// all at rotation 0). b2f_gate_queries is the union over the gates. The kernel is unrolled by
// hand, so nothing derives one from the other at compile time: tests/test_open_ref.py pins this
// table to the gate polynomials of tests/quotient_gates_ref.py, gate by gate through the union,
// and tests/test_gpu_open.py evaluates the chip's own quotient at a point through it.
constexpr uint16_t R0123 = 0x00f, R0246 = 0x055, R0369 = 0x249, R147A = 0x492, R07 = 0x0ff, R0B = 0xfff;
constexpr uint16_t QG_READS[16][10] = {
    //  a_0     a_1            a_2            a_3    a_4    a_5    a_6    a_7    a_8    a_9
    {0, R0123, 0, 0, 0, 0, 0, 1, 1, 0},                                 // 0
    {0, R0369 | R147A, R0369 | R147A, 0, 0, 0, 0, R0369, R0369, 0},      // 1
    {0, R0246, R0246, 0, 0, 0, R0246, R0246, R0246, 0},                  // 2
    {0, R0123, 0, R0123, R0123, R0123, 0, 0, 0, 1},                      // 3
    {R0369 | (R0369 << 1), 0, R0B, R0369, R0369, 0, 0, 0, 0, 0},         // 4
    {0, R0123, 0, R0123, R0123, 0, 0, 0, 0, 1},                          // 5
    {0, 0, R07, R0246, R0246, 0, 0, 0, 0, 0},                            // 6
    {0, R0123, 0, R0123, R0123, R0123, 0, 0, 0, 1},                      // 7
    {R0246, 0, R07, R0246, R0246, 0, R0246, 0, 0, 0},                    // 8
    {0, R0123, 0, R0123, R0123, 0, 0, 0, 0, 1},                          // 9
    {0, 0, R07, R0246, R0246, 0, 0, 0, 0, 0},                            // 10
    {0, R0246, 0, 0, 0, 0, 0, 1, 1, 0},                                  // 11
    {0, 0, R07, R0246, R0246, 0, 0, 0, 0, 0},                            // 12
    {0, 0, R07, R0246, R0246, R0246, 0, 0, 0, 0},                        // 13
    {0, 1, 0, 0, 0, 0, 0, 0, 0, 0},                                      // 14
    {0, R0123, 0, 0, 0, 1, 0, 0, 0, 0},                                  // 15
};

struct GateConsts {
  Fe y, yt;      // y, y^74
  Fe ys[16];     // y^S_g, S_g = the number of terms after gate g's last one
  Fe w8, w16, w30, w64, w65535;
};

template <class F>
__global__ void quot_gate_consts_kernel(GateConsts* c, Words4 y) {
  if (blockIdx.x || threadIdx.x) return;
  const Fe yy = to_mont<F>(load_words(y.v));
  c->y = yy;
  c->yt = fe_pow<F>(yy, QG_TERMS);
  uint32_t after = QG_TERMS;
  for (int g = 0; g < 16; g++) {
    after -= QG_COUNT[g];
    c->ys[g] = fe_pow<F>(yy, after);
  }
  const Fe w16 = from_u32<F>(1u << 16), w32 = mul<F>(w16, w16);
  c->w8 = from_u32<F>(1u << 8);
  c->w16 = w16;
  c->w30 = from_u32<F>(1u << 30);
  c->w64 = mul<F>(w32, w32);
  c->w65535 = from_u32<F>(65535u);
}

struct QuotGates {
  const uint64_t *adv, *fix, *h_in;
  uint64_t* h_out;
  const GateConsts* c;
  uint64_t rows;
  uint32_t ext_k, rot;
};

template <class F, bool MONT>
__global__ __launch_bounds__(QT_THREADS, 2) void quot_gates_kernel(const QuotGates a) {
  // Workgroups b and b + 8 share an L2: deal each of the eight a run of consecutive tiles, so the
  // 11 rot halo rows a tile shares with the next one are fetched into one L2, not two.
  uint32_t tile = blockIdx.x;
  if (!(gridDim.x & 7u)) tile = (blockIdx.x & 7u) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  const uint32_t i = tile * QT_THREADS + threadIdx.x;
  const uint32_t mask = (1u << a.ext_k) - 1u;
  if (i > mask) return;
  const GateConsts& c = *a.c;
  // `row` is i behind an opaque copy renewed at every step: the 84 element addresses of a row
  // are otherwise all formed up front and held (two VGPRs each) until their loads
  uint32_t row = i;
  auto step = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    row = i;
    asm volatile("" : "+v"(row));
  };
  auto A = [&](uint32_t col, uint32_t j) {
    return ld<F, MONT>(a.adv + 4ull * (col * a.rows + ((row + j * a.rot) & mask)));
  };
  auto Q = [&](uint32_t g) { return ld<F, MONT>(a.fix + 4ull * (g * a.rows + row)); };
  auto dbl = [](const Fe& x) { return add<F>(x, x); };
  auto horner = [&](const Fe& P, const Fe& t) { return add<F>(mul<F>(P, c.y), t); };
  auto sel = [&](uint32_t g) { return mul<F>(Q(g), c.ys[g]); };

  Fe acc = a.h_in ? mul<F>(ld<F, MONT>(a.h_in + 4ull * i), c.yt) : fe_zero();

  {  // bits 0 and 11: the two 32-bit halves of a word from its dense limbs
    const Fe a7 = A(GA7, 0), a8 = A(GA8, 0), d0 = A(GA1, 0), d2 = A(GA1, 2);
    Fe P = sub<F>(sub<F>(a7, d0), mul<F>(c.w16, A(GA1, 1)));
    P = horner(P, sub<F>(sub<F>(a8, d2), mul<F>(c.w16, A(GA1, 3))));
    acc = add<F>(acc, mul<F>(sel(0), P));
    P = sub<F>(sub<F>(a7, d0), mul<F>(c.w16, d2));
    P = horner(P, sub<F>(sub<F>(a8, A(GA1, 4)), mul<F>(c.w16, A(GA1, 6))));
    acc = add<F>(acc, mul<F>(sel(11), P));
    // bit 14: the constant
    acc = add<F>(acc, mul<F>(sel(14), sub<F>(d0, Q(16))));
  }
  step();
  {  // bit 15: the f mask
    const Fe f = A(GA5, 0), m = mul<F>(c.w65535, f);
    Fe P = mul<F>(f, sub<F>(f, one<F>()));
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) P = horner(P, sub<F>(A(GA1, k), m));
    acc = add<F>(acc, mul<F>(sel(15), P));
  }
  step();
  {  // bits 3/7 (ADD3) and 5/9 (ADD2): the dense sums, then the carry polynomials
    Fe S2 = fe_zero(), M = fe_zero();
#pragma unroll
    for (int k = 3; k >= 0; k--) {
      const Fe d = sub<F>(add<F>(A(GA3, k), A(GA4, k)), A(GA1, k));
      const Fe m = A(GA5, k);
      S2 = k == 3 ? d : add<F>(mul<F>(S2, c.w16), d);
      M = k == 3 ? m : add<F>(mul<F>(M, c.w16), m);
      step();
    }
    const Fe c9 = A(GA9, 0);
    S2 = sub<F>(S2, mul<F>(c.w64, c9));
    const Fe C2 = mul<F>(c9, sub<F>(c9, one<F>()));
    const Fe C3 = mul<F>(C2, sub<F>(c9, dbl(one<F>())));
    acc = add<F>(acc, mul<F>(add<F>(sel(5), sel(9)), horner(S2, C2)));
    acc = add<F>(acc, mul<F>(add<F>(sel(3), sel(7)), horner(add<F>(S2, M), C3)));
  }
  step();
  {  // bit 1: the rot-24 recomposition
    Fe P = fe_zero();
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
      const uint32_t k1 = (k + 1) & 3u, k2 = (k + 2) & 3u;
      const Fe p0 = sub<F>(sub<F>(A(GA7, 3 * k), A(GA1, 3 * k1 + 1)), mul<F>(c.w8, A(GA1, 3 * k2)));
      P = k ? horner(P, p0) : p0;
      P = horner(P, sub<F>(sub<F>(A(GA8, 3 * k), A(GA2, 3 * k1 + 1)), mul<F>(c.w16, A(GA2, 3 * k2))));
      step();
    }
    acc = add<F>(acc, mul<F>(sel(1), P));
  }
  step();
  {  // bit 4: the XOR of the rot-24 block, split 8 + 8
    Fe P = fe_zero();
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
      Fe x = sub<F>(add<F>(A(GA3, 3 * k), A(GA4, 3 * k)), A(GA2, 3 * k));
      x = sub<F>(sub<F>(x, mul<F>(c.w16, A(GA2, 3 * k + 1))), dbl(A(GA2, 3 * k + 2)));
      P = k ? horner(P, x) : x;
      P = horner(P, A(GA0, 3 * k));
      P = horner(P, A(GA0, 3 * k + 1));
      step();
    }
    acc = add<F>(acc, mul<F>(sel(4), P));
  }
  step();
  {  // bit 2: the rot-63 recomposition
    Fe P = fe_zero();
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
      const Fe zb = A(GA6, 2 * ((k + 3) & 3u));
      const Fe p0 = sub<F>(sub<F>(A(GA7, 2 * k), zb), dbl(A(GA1, 2 * k)));
      P = k ? horner(P, p0) : p0;
      P = horner(P, sub<F>(sub<F>(A(GA8, 2 * k), zb), dbl(dbl(A(GA2, 2 * k)))));
      step();
    }
    acc = add<F>(acc, mul<F>(sel(2), P));
  }
  step();
  {  // the 8-row XOR family: bits 6/10/12, 8 (rot-63: split 15 + 1) and 13 (three inputs)
    Fe P6 = fe_zero(), P8 = fe_zero(), P13 = fe_zero();
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) {
      Fe x = sub<F>(add<F>(A(GA3, 2 * k), A(GA4, 2 * k)), A(GA2, 2 * k));
      x = sub<F>(x, dbl(A(GA2, 2 * k + 1)));
      const Fe x3 = add<F>(x, A(GA5, 2 * k));
      const Fe zb = A(GA6, 2 * k), tag = A(GA0, 2 * k);
      const Fe x8 = sub<F>(x, mul<F>(c.w30, zb));
      P6 = k ? horner(P6, x) : x;
      P13 = k ? horner(P13, x3) : x3;
      P8 = k ? horner(P8, x8) : x8;
      P8 = horner(P8, mul<F>(tag, sub<F>(tag, one<F>())));
      P8 = horner(P8, mul<F>(zb, sub<F>(zb, one<F>())));
      step();
    }
    acc = add<F>(acc, mul<F>(add<F>(add<F>(sel(6), sel(10)), sel(12)), P6));
    acc = add<F>(acc, mul<F>(sel(8), P8));
    acc = add<F>(acc, mul<F>(sel(13), P13));
  }
  st<F, MONT>(a.h_out + 4ull * i, acc);
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

dim3 row_grid(uint32_t log_rows) { return dim3(((1u << log_rows) + QT_THREADS - 1) / QT_THREADS); }

void launch_consts(uint32_t form, void* d_consts, const uint64_t* beta, const uint64_t* gamma, const uint64_t* y,
                   const uint64_t* delta, uint32_t sets, hipStream_t s) {
  QuotConsts* c = static_cast<QuotConsts*>(d_consts);
  with_field(form, [&](auto f) {
    hipLaunchKernelGGL(quot_consts_kernel<decltype(f)>, dim3(1), dim3(64), 0, s, c, words4(beta), words4(gamma),
                       words4(y), words4(delta), sets);
  });
}

}  // namespace

size_t quot_xtab_bytes(uint32_t ext_k) {
  const uint32_t h0 = quot_h0(ext_k);
  return 32ull * (QT_T0_OFF + (1ull << h0) + (1ull << (ext_k - h0)));
}

// b2f_gate_queries: the union of QG_READS over the gates as (halo2 column, rotation) pairs, sorted
// by column then rotation
uint64_t gate_queries(uint32_t* pairs, uint64_t cap) {
  static const uint32_t halo2[10] = {GA0, GA1, GA2, GA3, GA4, GA5, GA6, GA7, GA8, GA9};
  uint16_t by_col[10] = {};
  for (int g = 0; g < 16; g++)
    for (int i = 0; i < 10; i++) by_col[halo2[i]] |= QG_READS[g][i];
  uint64_t count = 0;
  for (uint32_t c = 0; c < 10; c++)
    for (uint32_t j = 0; j < 16; j++)
      if ((by_col[c] >> j) & 1u) {
        if (pairs && count < cap) {
          pairs[2 * count] = c;
          pairs[2 * count + 1] = j;
        }
        count++;
      }
  return count;
}

// one block serves both kinds of term call
size_t quot_consts_bytes() { return sizeof(QuotConsts) > sizeof(GateConsts) ? sizeof(QuotConsts) : sizeof(GateConsts); }

hipError_t launch_quot_xtab(void* d_tab, uint32_t form, uint32_t ext_k, const uint64_t* omega,
                            const uint64_t* shift, hipStream_t s) {
  const uint32_t h0 = quot_h0(ext_k);
  const uint32_t total = (1u << h0) + (1u << (ext_k - h0));
  const dim3 grid((total + QT_THREADS - 1) / QT_THREADS);
  uint64_t* tab = static_cast<uint64_t*>(d_tab);
  with_field(form, [&](auto f) {
    hipLaunchKernelGGL(quot_xtab_kernel<decltype(f)>, grid, dim3(QT_THREADS), 0, s, tab, words4(omega), words4(shift),
                       ext_k);
  });
  return hipGetLastError();
}

hipError_t launch_lagrange_selectors(uint32_t k, uint32_t usable_rows, uint32_t form, uint64_t* d_out,
                                     uint64_t out_rows, hipStream_t s) {
  with_field(form, [&](auto f) {
    hipLaunchKernelGGL(quot_selectors_kernel<decltype(f)>, row_grid(k), dim3(QT_THREADS), 0, s, d_out, out_rows,
                       1u << k, usable_rows, form & 1u);
  });
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
  with_form(form, [&](auto f, auto mont) {
    hipLaunchKernelGGL((quot_perm_kernel<decltype(f), decltype(mont)::value>), grid, block, 0, s, a);
  });
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
  with_form(form, [&](auto f, auto mont) {
    hipLaunchKernelGGL((quot_lookup_kernel<decltype(f), decltype(mont)::value>), grid, block, 0, s, a);
  });
  return hipGetLastError();
}

hipError_t launch_quot_gates(uint32_t k, uint32_t ext_k, const uint64_t* d_advice, const uint64_t* d_fixed,
                             uint64_t rows, const uint64_t* y, const uint64_t* d_h_in, uint64_t* d_h_out,
                             uint32_t form, void* d_consts, hipStream_t s) {
  QuotGates a;
  a.adv = d_advice;
  a.fix = d_fixed;
  a.h_in = d_h_in;
  a.h_out = d_h_out;
  a.c = static_cast<const GateConsts*>(d_consts);
  a.rows = rows;
  a.ext_k = ext_k;
  a.rot = 1u << (ext_k - k);
  GateConsts* c = static_cast<GateConsts*>(d_consts);
  with_field(form, [&](auto f) {
    hipLaunchKernelGGL(quot_gate_consts_kernel<decltype(f)>, dim3(1), dim3(64), 0, s, c, words4(y));
  });
  const dim3 block(QT_THREADS), grid = row_grid(ext_k);
  with_form(form, [&](auto f, auto mont) {
    hipLaunchKernelGGL((quot_gates_kernel<decltype(f), decltype(mont)::value>), grid, block, 0, s, a);
  });
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
  with_field(form, [&](auto f) {
    hipLaunchKernelGGL(quot_divisor_kernel<decltype(f)>, grid, block, 0, s, dtab, words4(omega), words4(shift), k,
                       ext_k);
  });
  return hipGetLastError();
}

hipError_t launch_quot_divide(uint32_t k, uint32_t ext_k, const uint64_t* d_h_in, uint64_t* d_h_out,
                              uint32_t form, const void* d_dtab, int* sticky, hipStream_t s) {
  const uint64_t* dtab = static_cast<const uint64_t*>(d_dtab);
  const uint32_t rot = 1u << (ext_k - k);
  with_field(form, [&](auto f) {
    hipLaunchKernelGGL(quot_divide_kernel<decltype(f)>, row_grid(ext_k), dim3(QT_THREADS), 0, s, d_h_in, d_h_out,
                       dtab, ext_k, rot, sticky);
  });
  return hipGetLastError();
}

}  // namespace b2f
