// b2f_open.hip -- the field side of the opening step over coefficient columns
// (b2f_poly_eval_dev, b2f_poly_combine_dev, b2f_kate_divide_dev): halo2_proofs 0.3.0
// arithmetic.rs eval_polynomial and kate_division and the challenge folds of plonk/prover.rs and
// poly/multiopen/prover.rs. DESIGN.md §4.6.
//
// Every pass here is linear in the column data with Montgomery-form multipliers (powers of the
// points, the scalars), and mul(x, m R) = x m in whatever form x is: a canonical column goes
// through canonical and a Montgomery one Montgomery, bit for bit what converting at load and
// store gives, without the two products. `form` picks the field and nothing else.
//
// A column is cut into tiles of OP_TILE = 1024 coefficients, one workgroup of 256 threads each.
//   tile value   G_t(z) = sum_{s <= i < e} a_i z^(i - s)          (tile_partials)
//   evaluation   p(z)   = sum_t G_t (z^T)^t                        (poly_eval_combine_kernel)
//   division     carry_t = G_t + z^T carry_{t+1}                   (kate_scan_kernel)
//                q_j = S_j + z^(e-1-j) carry_{t+1}                 (kate_apply_kernel)
// The evaluation kernel loads a tile once (thread l holds a_{s + l + 256 j}, j < 4: coalesced,
// in registers) and loops over the column's points: three Horner products in z^256, one with z^l
// from the point's power table, and an add-only reduction. The carries pass between launches, the
// way b2f_gprod.h passes its block totals: there is no in-kernel look-back.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/b2f.h"
#include "b2f_field.h"
#include "b2f_open.h"

namespace b2f {

using namespace field;

namespace {

constexpr uint32_t OP_THREADS = 256, OP_C = 4, OP_TILE = OP_THREADS * OP_C;
// power table of one point, in 32-byte elements: z^0 .. z^256, then z^OP_TILE
constexpr uint32_t OP_PW = OP_THREADS + 2;
constexpr uint32_t OP_MAX_Y = 65535;  // column groups per launch
static_assert(OP_C == 4, "pow_table_kernel squares z^256 twice for z^OP_TILE");

// one distinct queried column of an evaluation call: its (column, point) pairs are consecutive
struct OpGroup {
  uint64_t col;
  uint32_t first_pair, n_pairs;
};
// one dividing column: m points first_pt .. first_pt + m - 1, one per pass
struct OpSlot {
  uint32_t col, m, first_pt, pad;
};
struct OpSpecial {
  uint32_t col, zero;
};

__device__ __forceinline__ Fe shfl_down(const Fe& x, uint32_t d) {
  Fe r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.w[i] = __shfl_down(x.w[i], d, 64);
  return r;
}
__device__ __forceinline__ Fe shfl_lane(const Fe& x, int lane) {
  Fe r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.w[i] = __shfl(x.w[i], lane, 64);
  return r;
}
// the wave's sum, in lane 0
template <class F>
__device__ __forceinline__ Fe wave_sum(Fe v) {
#pragma unroll
  for (uint32_t d = 32; d; d >>= 1) v = add<F>(v, shfl_down(v, d));
  return v;
}

// z^t for t <= 256 and z^OP_TILE of every point: one lane per entry
template <class F>
__global__ __launch_bounds__(OP_THREADS) void pow_table_kernel(uint64_t* tab, const uint64_t* pts,
                                                               uint32_t n_points) {
  const uint64_t g = (uint64_t)blockIdx.x * OP_THREADS + threadIdx.x;
  const uint64_t pt = g / (OP_THREADS + 1);
  const uint32_t t = (uint32_t)(g % (OP_THREADS + 1));
  if (pt >= n_points) return;
  Fe v = pow_entry<F>(load(pts + 4ull * pt), t);
  store(tab + 4ull * (pt * OP_PW + t), v);
  if (t == OP_THREADS) {
    v = mul<F>(v, v);
    v = mul<F>(v, v);
    store(tab + 4ull * (pt * OP_PW + OP_THREADS + 1), v);
  }
}

// The tile values of one column tile at n_pairs points: partial[(first_pair + i) ntiles + tile] =
// G_tile(z_i), z_i = the point pt_of(first_pair + i). The tile's coefficients are loaded once;
// rows >= len read as zero. ws: 64 x 4 elements of LDS.
template <class F, class PtOf>
__device__ __forceinline__ void tile_partials(const uint64_t* src, uint64_t len, uint64_t tile, uint64_t ntiles,
                                              const uint64_t* tab, PtOf pt_of, uint32_t first_pair,
                                              uint32_t n_pairs, uint64_t* partial, Fe (*ws)[4]) {
  const uint32_t l = threadIdx.x;
  const uint64_t s = tile * OP_TILE;
  Fe a[OP_C];
#pragma unroll
  for (uint32_t j = 0; j < OP_C; j++) {
    const uint64_t i = s + l + j * OP_THREADS;
    a[j] = i < len ? load(src + 4ull * i) : fe_zero();
  }
  for (uint32_t c0 = 0; c0 < n_pairs; c0 += 64) {
    const uint32_t cn = n_pairs - c0 < 64u ? n_pairs - c0 : 64u;
#pragma unroll 1
    for (uint32_t pi = 0; pi < cn; pi++) {
      const uint64_t* tb = tab + 4ull * OP_PW * pt_of(first_pair + c0 + pi);
      const Fe zs = load(tb + 4ull * OP_THREADS);
      Fe v = a[OP_C - 1];
#pragma unroll
      for (int j = OP_C - 2; j >= 0; j--) v = add<F>(mul<F>(v, zs), a[j]);
      v = wave_sum<F>(mul<F>(v, load(tb + 4ull * l)));
      if (!(l & 63u)) ws[pi][l >> 6] = v;
    }
    __syncthreads();
    if (l < cn)
      store(partial + 4ull * ((uint64_t)(first_pair + c0 + l) * ntiles + tile),
            add<F>(add<F>(ws[l][0], ws[l][1]), add<F>(ws[l][2], ws[l][3])));
    __syncthreads();
  }
}

struct EvalArgs {
  const uint64_t* cols;
  uint64_t rows, len, ntiles;
  const OpGroup* groups;
  const uint32_t* pair_pt;
  const uint32_t* q_pair;
  const uint64_t* tab;
  uint64_t* partial;
  uint64_t* out;
};

template <class F>
__global__ __launch_bounds__(OP_THREADS) void poly_eval_partial_kernel(const EvalArgs a, uint32_t group0) {
  __shared__ Fe ws[64][4];
  const OpGroup g = a.groups[group0 + blockIdx.y];
  const uint32_t* pp = a.pair_pt;
  tile_partials<F>(a.cols + 4ull * g.col * a.rows, a.len, blockIdx.x, a.ntiles, a.tab,
                   [pp](uint32_t pair) { return pp[pair]; }, g.first_pair, g.n_pairs, a.partial, ws);
}

// out[q] = sum_t G_t (z^T)^t of the query's pair: one workgroup per query
template <class F>
__global__ __launch_bounds__(OP_THREADS) void poly_eval_combine_kernel(const EvalArgs a) {
  __shared__ Fe ws[4];
  const uint32_t q = blockIdx.x, l = threadIdx.x;
  const uint32_t pair = a.q_pair[q];
  const Fe zt = load(a.tab + 4ull * (OP_PW * (uint64_t)a.pair_pt[pair] + OP_THREADS + 1));
  Fe acc = fe_zero();
  if (l < a.ntiles) {
    Fe pw = fe_pow<F>(zt, l);
    Fe step = zt;
    if (a.ntiles > OP_THREADS)
      for (int i = 0; i < 8; i++) step = mul<F>(step, step);  // (z^T)^256
#pragma unroll 1
    for (uint64_t t = l; t < a.ntiles; t += OP_THREADS) {
      acc = add<F>(acc, mul<F>(load(a.partial + 4ull * (pair * a.ntiles + t)), pw));
      if (t + OP_THREADS < a.ntiles) pw = mul<F>(pw, step);
    }
  }
  acc = wave_sum<F>(acc);
  if (!(l & 63u)) ws[l >> 6] = acc;
  __syncthreads();
  if (!l) store(a.out + 4ull * q, add<F>(add<F>(ws[0], ws[1]), add<F>(ws[2], ws[3])));
}

// scalars to Montgomery form
template <class F>
__global__ __launch_bounds__(OP_THREADS) void scalar_prep_kernel(const uint64_t* in, uint64_t* out, uint32_t n) {
  const uint32_t g = blockIdx.x * OP_THREADS + threadIdx.x;
  if (g < n) store(out + 4ull * g, to_mont<F>(load(in + 4ull * g)));
}

struct CombineArgs {
  const uint64_t* cols;
  uint64_t rows, len;
  const uint32_t *first, *col;
  const uint64_t* scal;
  uint64_t* out;
  uint64_t out_rows;
  uint32_t n_out;
};

// One thread per row and output: every input of the row is read once.
template <class F>
__global__ __launch_bounds__(OP_THREADS) void poly_combine_kernel(const CombineArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * OP_THREADS + threadIdx.x;
  if (i >= a.len) return;
  for (uint32_t o = blockIdx.y; o < a.n_out; o += gridDim.y) {
    Fe acc = fe_zero();
    const uint32_t j1 = a.first[o + 1];
#pragma unroll 1
    for (uint32_t j = a.first[o]; j < j1; j++)
      acc = add<F>(acc, mul<F>(load(a.cols + 4ull * (a.col[j] * a.rows + i)), load(a.scal + 4ull * j)));
    store(a.out + 4ull * (o * a.out_rows + i), acc);
  }
}

struct KateArgs {
  const uint64_t* cols;
  uint64_t rows, len, ntiles;
  const OpSlot* slots;
  const OpSpecial* special;
  const uint64_t* tab;
  uint64_t *partial, *carry;  // [slot][tile]
  uint64_t* pp;               // ping-pong: [2][n_pp][len]
  uint64_t* out;
  uint64_t out_rows;
  uint32_t n_pp;
};

__device__ __forceinline__ const uint64_t* kate_src(const KateArgs& a, const OpSlot& d, uint32_t slot,
                                                    uint32_t pass) {
  return pass ? a.pp + 4ull * (((pass - 1) & 1u) * (uint64_t)a.n_pp + slot) * a.len
              : a.cols + 4ull * d.col * a.rows;
}

template <class F>
__global__ __launch_bounds__(OP_THREADS) void kate_partial_kernel(const KateArgs a, uint32_t slot0, uint32_t pass) {
  __shared__ Fe ws[64][4];
  const uint32_t slot = slot0 + blockIdx.y;
  const OpSlot d = a.slots[slot];
  const uint32_t pt = d.first_pt + pass;
  tile_partials<F>(kate_src(a, d, slot, pass), a.len, blockIdx.x, a.ntiles, a.tab,
                   [pt](uint32_t) { return pt; }, slot, 1u, a.partial, ws);
}

// carry_t = G_t + z^T carry_{t+1}, carry_ntiles = 0: one wave per column, 64 tiles at a time from
// the top, a suffix scan with the multiplier (z^T)^(2^s) at step s; the carry of the chunk above
// enters at the chunk's highest tile.
template <class F>
__global__ __launch_bounds__(64) void kate_scan_kernel(const KateArgs a, uint32_t pass) {
  const uint32_t slot = blockIdx.x, lane = threadIdx.x;
  const OpSlot d = a.slots[slot];
  Fe pw[6];
  pw[0] = load(a.tab + 4ull * (OP_PW * (uint64_t)(d.first_pt + pass) + OP_THREADS + 1));
#pragma unroll
  for (int s = 1; s < 6; s++) pw[s] = mul<F>(pw[s - 1], pw[s - 1]);
  Fe cin = fe_zero();
#pragma unroll 1
  for (uint64_t ch = (a.ntiles + 63) / 64; ch-- > 0;) {
    const uint64_t t = ch * 64 + lane;
    Fe v = t < a.ntiles ? load(a.partial + 4ull * (slot * a.ntiles + t)) : fe_zero();
    const Fe top = add<F>(v, mul<F>(cin, pw[0]));
    if (lane == 63) v = top;
#pragma unroll
    for (int s = 0; s < 6; s++) {
      const Fe u = mul<F>(shfl_down(v, 1u << s), pw[s]);
      if (lane + (1u << s) < 64u) v = add<F>(v, u);
    }
    if (t < a.ntiles) store(a.carry + 4ull * (slot * a.ntiles + t), v);
    cin = shfl_lane(v, 0);
  }
}

// One division pass of one column tile. Thread l owns coefficients s + 4 l .. s + 4 l + 3 (through
// LDS, so the global loads and stores stay coalesced): its value G_l, a suffix scan over the
// workgroup with the multiplier z^4, the carry of the tile above, then the recurrence
// q_{i-1} = a_i + z q_i over its own four.
template <class F>
__global__ __launch_bounds__(OP_THREADS) void kate_apply_kernel(const KateArgs a, uint32_t slot0, uint32_t pass) {
  __shared__ u32x4 buf[2][OP_TILE];
  __shared__ Fe wtot[4];
  const uint32_t slot = slot0 + blockIdx.y, l = threadIdx.x, lane = l & 63u, wave = l >> 6;
  const uint64_t tile = blockIdx.x, s = tile * OP_TILE;
  const OpSlot d = a.slots[slot];
  const uint64_t* src = kate_src(a, d, slot, pass);
  uint64_t* dst = pass + 1 == d.m ? a.out + 4ull * d.col * a.out_rows
                                  : a.pp + 4ull * ((pass & 1u) * (uint64_t)a.n_pp + slot) * a.len;
#pragma unroll
  for (uint32_t j = 0; j < OP_C; j++) {
    const uint32_t e = l + j * OP_THREADS;
    const Fe x = s + e < a.len ? load(src + 4ull * (s + e)) : fe_zero();
    buf[0][e] = u32x4{x.w[0], x.w[1], x.w[2], x.w[3]};
    buf[1][e] = u32x4{x.w[4], x.w[5], x.w[6], x.w[7]};
  }
  __syncthreads();
  Fe c[OP_C];
#pragma unroll
  for (uint32_t j = 0; j < OP_C; j++) {
    const u32x4 lo = buf[0][OP_C * l + j], hi = buf[1][OP_C * l + j];
    c[j].w[0] = lo.x; c[j].w[1] = lo.y; c[j].w[2] = lo.z; c[j].w[3] = lo.w;
    c[j].w[4] = hi.x; c[j].w[5] = hi.y; c[j].w[6] = hi.z; c[j].w[7] = hi.w;
  }
  const uint64_t* tb = a.tab + 4ull * OP_PW * (uint64_t)(d.first_pt + pass);
  const Fe z = load(tb + 4);
  Fe v = c[OP_C - 1];
#pragma unroll
  for (int j = OP_C - 2; j >= 0; j--) v = add<F>(mul<F>(v, z), c[j]);
#pragma unroll 1
  for (uint32_t st = 0; st < 6; st++) {
    const Fe u = mul<F>(shfl_down(v, 1u << st), load(tb + 4ull * (OP_C << st)));
    if (lane + (1u << st) < 64u) v = add<F>(v, u);
  }
  if (!lane) wtot[wave] = v;
  __syncthreads();  // every thread has read its coefficients: buf is free again
  // the value entering this wave from above: the waves after it, then the tile above
  Fe cw = tile + 1 < a.ntiles ? load(a.carry + 4ull * (slot * a.ntiles + tile + 1)) : fe_zero();
  const Fe z256 = load(tb + 4ull * OP_THREADS);
#pragma unroll 1
  for (uint32_t w2 = 3; w2 > wave; w2--) cw = add<F>(mul<F>(cw, z256), wtot[w2]);
  v = add<F>(v, mul<F>(cw, load(tb + 4ull * (OP_THREADS - OP_C * lane))));
  Fe q = shfl_down(v, 1);
  if (lane == 63) q = cw;
#pragma unroll
  for (int j = OP_C - 1; j >= 0; j--) {  // q = q_{s + 4 l + j}
    buf[0][OP_C * l + j] = u32x4{q.w[0], q.w[1], q.w[2], q.w[3]};
    buf[1][OP_C * l + j] = u32x4{q.w[4], q.w[5], q.w[6], q.w[7]};
    if (j) q = add<F>(mul<F>(q, z), c[j]);
  }
  __syncthreads();
#pragma unroll
  for (uint32_t j = 0; j < OP_C; j++) {
    const uint32_t e = l + j * OP_THREADS;
    if (s + e < a.len) {
      u32x4* o = reinterpret_cast<u32x4*>(dst + 4ull * (s + e));
      o[0] = buf[0][e];
      o[1] = buf[1][e];
    }
  }
}

// columns with no point (copied) or with len points or more (all zeros)
__global__ __launch_bounds__(OP_THREADS) void kate_special_kernel(const KateArgs a) {
  const uint64_t i = (uint64_t)blockIdx.x * OP_THREADS + threadIdx.x;
  if (i >= a.len) return;
  const OpSpecial d = a.special[blockIdx.y];
  store(a.out + 4ull * (d.col * a.out_rows + i), d.zero ? fe_zero() : load(a.cols + 4ull * (d.col * a.rows + i)));
}

// append a section to the image at a 16-byte boundary; returns its offset in words
size_t blob_put(std::vector<uint64_t>& blob, const void* data, size_t bytes) {
  if (blob.size() & 1u) blob.push_back(0);
  const size_t off = blob.size();
  blob.resize(off + (bytes + 7) / 8, 0);
  if (bytes) memcpy(blob.data() + off, data, bytes);
  return off;
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

int plan_common(OpenPlan& p, uint64_t len, uint32_t form, char* msg, size_t n) {
  if (form > B2F_FP_BN254_MONTGOMERY) {
    snprintf(msg, n, "unknown form %u", form);
    return B2F_ERR_ARG;
  }
  if (len > (1ull << 32)) {
    snprintf(msg, n, "len above 2^32");
    return B2F_ERR_ARG;
  }
  p = OpenPlan();
  p.len = len;
  p.ntiles = (len + OP_TILE - 1) / OP_TILE;
  p.form = form;
  return B2F_OK;
}

void launch_pow_table(const OpenPlan& p, const uint64_t* d_blob, uint64_t* tab, hipStream_t s) {
  const uint64_t total = (uint64_t)p.n_points * (OP_THREADS + 1);
  with_field(p.form, [&](auto f) {
    hipLaunchKernelGGL(pow_table_kernel<decltype(f)>, dim3((uint32_t)((total + OP_THREADS - 1) / OP_THREADS)),
                       dim3(OP_THREADS), 0, s, tab, d_blob + p.off_points, p.n_points);
  });
}

}  // namespace

int open_plan_eval(OpenPlan& p, uint64_t len, uint32_t n_cols, const uint64_t* h_points, uint32_t n_points,
                   const uint32_t* h_queries, uint64_t n_queries, uint32_t form, char* msg, size_t msg_len) {
  if (int rc = plan_common(p, len, form, msg, msg_len)) return rc;
  if (n_queries >= (1ull << 31)) {
    snprintf(msg, msg_len, "more than 2^31 - 1 queries");
    return B2F_ERR_ARG;
  }
  for (uint32_t i = 0; i < n_points; i++)
    if (!fe_canonical(form, h_points + 4ull * i)) {
      snprintf(msg, msg_len, "point %u is >= p", i);
      return B2F_ERR_ARG;
    }
  struct Q {
    uint32_t col, pt, q;
  };
  std::vector<Q> qs(n_queries);
  for (uint64_t q = 0; q < n_queries; q++) {
    qs[q] = Q{h_queries[2 * q], h_queries[2 * q + 1], (uint32_t)q};
    if (qs[q].col >= n_cols || qs[q].pt >= n_points) {
      snprintf(msg, msg_len, "query %llu names column %u of %u, point %u of %u", (unsigned long long)q, qs[q].col,
               n_cols, qs[q].pt, n_points);
      return B2F_ERR_ARG;
    }
  }
  std::sort(qs.begin(), qs.end(), [](const Q& x, const Q& y) { return x.col != y.col ? x.col < y.col : x.pt < y.pt; });
  std::vector<OpGroup> groups;
  std::vector<uint32_t> pair_pt, q_pair(n_queries);
  for (uint64_t i = 0; i < n_queries; i++) {
    const bool new_col = !i || qs[i].col != qs[i - 1].col;
    if (new_col) groups.push_back(OpGroup{qs[i].col, (uint32_t)pair_pt.size(), 0});
    if (new_col || qs[i].pt != qs[i - 1].pt) {
      pair_pt.push_back(qs[i].pt);
      groups.back().n_pairs++;
    }
    q_pair[qs[i].q] = (uint32_t)pair_pt.size() - 1;
  }
  p.n_points = n_points;
  p.n_groups = (uint32_t)groups.size();
  p.n_pairs = (uint32_t)pair_pt.size();
  p.n_queries = n_queries;
  p.off_points = blob_put(p.blob, h_points, 32ull * n_points);
  p.off_a = blob_put(p.blob, groups.data(), sizeof(OpGroup) * groups.size());
  p.off_b = blob_put(p.blob, pair_pt.data(), 4 * pair_pt.size());
  p.off_c = blob_put(p.blob, q_pair.data(), 4 * q_pair.size());
  p.scratch_bytes = align256(32ull * OP_PW * n_points) + 32ull * p.n_pairs * p.ntiles;
  return B2F_OK;
}

hipError_t launch_poly_eval(const OpenPlan& p, const uint64_t* d_cols, uint64_t rows, const void* d_blob,
                            void* d_scratch, uint64_t* d_out, hipStream_t s) {
  const uint64_t* blob = static_cast<const uint64_t*>(d_blob);
  uint64_t* tab = static_cast<uint64_t*>(d_scratch);
  EvalArgs a;
  a.cols = d_cols;
  a.rows = rows;
  a.len = p.len;
  a.ntiles = p.ntiles;
  a.groups = reinterpret_cast<const OpGroup*>(blob + p.off_a);
  a.pair_pt = reinterpret_cast<const uint32_t*>(blob + p.off_b);
  a.q_pair = reinterpret_cast<const uint32_t*>(blob + p.off_c);
  a.tab = tab;
  a.partial = tab + align256(32ull * OP_PW * p.n_points) / 8;
  a.out = d_out;
  launch_pow_table(p, blob, tab, s);
  with_field(p.form, [&](auto f) {
    using F = decltype(f);
    for (uint32_t g0 = 0; g0 < p.n_groups; g0 += OP_MAX_Y) {
      const uint32_t gn = p.n_groups - g0 < OP_MAX_Y ? p.n_groups - g0 : OP_MAX_Y;
      hipLaunchKernelGGL(poly_eval_partial_kernel<F>, dim3((uint32_t)p.ntiles, gn), dim3(OP_THREADS), 0, s, a, g0);
    }
    hipLaunchKernelGGL(poly_eval_combine_kernel<F>, dim3((uint32_t)p.n_queries), dim3(OP_THREADS), 0, s, a);
  });
  return hipGetLastError();
}

int open_plan_combine(OpenPlan& p, uint64_t len, uint32_t n_cols, const uint32_t* h_first, const uint32_t* h_col,
                      const uint64_t* h_scalar, uint32_t n_out, uint32_t form, char* msg, size_t msg_len) {
  if (int rc = plan_common(p, len, form, msg, msg_len)) return rc;
  for (uint32_t o = 0; o < n_out; o++)
    if (h_first[o + 1] < h_first[o]) {
      snprintf(msg, msg_len, "first[%u..%u] decreases", o, o + 1);
      return B2F_ERR_ARG;
    }
  if (h_first[0] != 0) {
    snprintf(msg, msg_len, "first[0] is not 0");
    return B2F_ERR_ARG;
  }
  const uint32_t nnz = h_first[n_out];
  for (uint32_t j = 0; j < nnz; j++) {
    if (h_col[j] >= n_cols) {
      snprintf(msg, msg_len, "term %u names column %u of %u", j, h_col[j], n_cols);
      return B2F_ERR_ARG;
    }
    if (!fe_canonical(form, h_scalar + 4ull * j)) {
      snprintf(msg, msg_len, "scalar %u is >= p", j);
      return B2F_ERR_ARG;
    }
  }
  p.n_out = n_out;
  p.nnz = nnz;
  p.off_points = blob_put(p.blob, h_scalar, 32ull * nnz);
  p.off_a = blob_put(p.blob, h_first, 4ull * (n_out + 1));
  p.off_b = blob_put(p.blob, h_col, 4ull * nnz);
  p.scratch_bytes = 32ull * nnz + 32;
  return B2F_OK;
}

hipError_t launch_poly_combine(const OpenPlan& p, const uint64_t* d_cols, uint64_t rows, const void* d_blob,
                               void* d_scratch, uint64_t* d_out, uint64_t out_rows, hipStream_t s) {
  const uint64_t* blob = static_cast<const uint64_t*>(d_blob);
  uint64_t* scal = static_cast<uint64_t*>(d_scratch);
  CombineArgs a;
  a.cols = d_cols;
  a.rows = rows;
  a.len = p.len;
  a.first = reinterpret_cast<const uint32_t*>(blob + p.off_a);
  a.col = reinterpret_cast<const uint32_t*>(blob + p.off_b);
  a.scal = scal;
  a.out = d_out;
  a.out_rows = out_rows;
  a.n_out = p.n_out;
  const dim3 grid((uint32_t)((p.len + OP_THREADS - 1) / OP_THREADS), p.n_out < OP_MAX_Y ? p.n_out : OP_MAX_Y);
  with_field(p.form, [&](auto f) {
    using F = decltype(f);
    if (p.nnz)
      hipLaunchKernelGGL(scalar_prep_kernel<F>, dim3((p.nnz + OP_THREADS - 1) / OP_THREADS), dim3(OP_THREADS), 0, s,
                         blob + p.off_points, scal, p.nnz);
    hipLaunchKernelGGL(poly_combine_kernel<F>, grid, dim3(OP_THREADS), 0, s, a);
  });
  return hipGetLastError();
}

int open_plan_kate(OpenPlan& p, uint64_t len, uint32_t n_cols, const uint32_t* h_first, const uint64_t* h_points,
                   uint32_t form, char* msg, size_t msg_len) {
  if (int rc = plan_common(p, len, form, msg, msg_len)) return rc;
  if (h_first[0] != 0) {
    snprintf(msg, msg_len, "first[0] is not 0");
    return B2F_ERR_ARG;
  }
  for (uint32_t c = 0; c < n_cols; c++)
    if (h_first[c + 1] < h_first[c]) {
      snprintf(msg, msg_len, "first[%u..%u] decreases", c, c + 1);
      return B2F_ERR_ARG;
    }
  const uint32_t np = h_first[n_cols];
  for (uint32_t i = 0; i < np; i++)
    if (!fe_canonical(form, h_points + 4ull * i)) {
      snprintf(msg, msg_len, "point %u is >= p", i);
      return B2F_ERR_ARG;
    }
  std::vector<OpSlot> slots;
  std::vector<OpSpecial> special;
  for (uint32_t c = 0; c < n_cols; c++) {
    const uint32_t m = h_first[c + 1] - h_first[c];
    if (m == 0 || m >= len)
      special.push_back(OpSpecial{c, m ? 1u : 0u});
    else
      slots.push_back(OpSlot{c, m, h_first[c], 0});
  }
  // longest chain first: the columns still dividing in pass p, and those that need the ping-pong
  // scratch, are then prefixes of the slot list
  std::stable_sort(slots.begin(), slots.end(), [](const OpSlot& x, const OpSlot& y) { return x.m > y.m; });
  p.n_points = np;
  p.n_slots = (uint32_t)slots.size();
  p.n_special = (uint32_t)special.size();
  p.passes = slots.empty() ? 0 : slots[0].m;
  for (const OpSlot& d : slots) p.n_pp += d.m >= 2;
  p.active.assign(p.passes, 0);
  for (const OpSlot& d : slots)
    for (uint32_t q = 0; q < d.m; q++) p.active[q]++;
  p.off_points = blob_put(p.blob, h_points, 32ull * np);
  p.off_a = blob_put(p.blob, slots.data(), sizeof(OpSlot) * slots.size());
  p.off_b = blob_put(p.blob, special.data(), sizeof(OpSpecial) * special.size());
  p.scratch_bytes = align256(32ull * OP_PW * np) + 2 * align256(32ull * p.n_slots * p.ntiles) +
                    2ull * 32 * p.n_pp * len + 32;
  return B2F_OK;
}

hipError_t launch_kate_divide(const OpenPlan& p, const uint64_t* d_cols, uint64_t rows, const void* d_blob,
                              void* d_scratch, uint64_t* d_out, uint64_t out_rows, hipStream_t s) {
  const uint64_t* blob = static_cast<const uint64_t*>(d_blob);
  uint64_t* tab = static_cast<uint64_t*>(d_scratch);
  KateArgs a;
  a.cols = d_cols;
  a.rows = rows;
  a.len = p.len;
  a.ntiles = p.ntiles;
  a.slots = reinterpret_cast<const OpSlot*>(blob + p.off_a);
  a.special = reinterpret_cast<const OpSpecial*>(blob + p.off_b);
  a.tab = tab;
  a.partial = tab + align256(32ull * OP_PW * p.n_points) / 8;
  a.carry = a.partial + align256(32ull * p.n_slots * p.ntiles) / 8;
  a.pp = a.carry + align256(32ull * p.n_slots * p.ntiles) / 8;
  a.out = d_out;
  a.out_rows = out_rows;
  a.n_pp = p.n_pp;
  const uint32_t row_blocks = (uint32_t)((p.len + OP_THREADS - 1) / OP_THREADS);
  for (uint32_t s0 = 0; s0 < p.n_special; s0 += OP_MAX_Y) {
    const uint32_t sn = p.n_special - s0 < OP_MAX_Y ? p.n_special - s0 : OP_MAX_Y;
    KateArgs b = a;
    b.special = a.special + s0;
    hipLaunchKernelGGL(kate_special_kernel, dim3(row_blocks, sn), dim3(OP_THREADS), 0, s, b);
  }
  if (p.passes) launch_pow_table(p, blob, tab, s);
  with_field(p.form, [&](auto f) {
    using F = decltype(f);
    for (uint32_t pass = 0; pass < p.passes; pass++) {
      const uint32_t act = p.active[pass];
      for (uint32_t s0 = 0; s0 < act; s0 += OP_MAX_Y) {
        const uint32_t sn = act - s0 < OP_MAX_Y ? act - s0 : OP_MAX_Y;
        hipLaunchKernelGGL(kate_partial_kernel<F>, dim3((uint32_t)p.ntiles, sn), dim3(OP_THREADS), 0, s, a, s0, pass);
      }
      hipLaunchKernelGGL(kate_scan_kernel<F>, dim3(act), dim3(64), 0, s, a, pass);
      for (uint32_t s0 = 0; s0 < act; s0 += OP_MAX_Y) {
        const uint32_t sn = act - s0 < OP_MAX_Y ? act - s0 : OP_MAX_Y;
        hipLaunchKernelGGL(kate_apply_kernel<F>, dim3((uint32_t)p.ntiles, sn), dim3(OP_THREADS), 0, s, a, s0, pass);
      }
    }
  });
  return hipGetLastError();
}

}  // namespace b2f
