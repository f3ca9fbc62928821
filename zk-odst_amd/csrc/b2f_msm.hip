// b2f_msm.hip -- the commitments: out[c] = sum_i scalar[c][i] base[i], a batched variable-base
// multi-scalar multiplication by Pippenger's bucket method on Vesta (forms 0/1) and BN254 G1
// (forms 2/3). Curve arithmetic: b2f_curve.h (XYZZ accumulators, affine bases).
//
// A call runs passes over (column group, row chunk): `group` columns x `chunk` rows at a time, so
// that a pass has at most 2^24 digits and 2^20 buckets whatever the call's size (msm_plan_of; the
// scratch is sized by the same function). One pass:
//   1. recode_kernel: every scalar, made canonical, becomes `windows` signed c-bit digits
//      d in [-2^(c-1), 2^(c-1)] (a digit above 2^(c-1) borrows 2^c from the next window). A digit
//      is the pair (key, value): key = (column, window, |d| - 1), value = the base's index with the
//      sign in bit 31. Zero digits get the key one past the last bucket and the EMPTY bit: they
//      sort to the end and cost no point addition. A call may give each of its (at most four)
//      columns an offset added to the base's index: column c then runs against bases[off_c ..]
//      (the IPA round's two cross terms, b2f_ipa.hip). windows * c >= 256 and every scalar is below
//      2^255, so the top window never carries out.
//   2. rocprim::radix_sort_pairs groups the digits by key.
//   3. bucket sums, as a reduction by key in levels (reduce_kernel): a level cuts its sorted
//      array into segments of SEG entries, one lane each. A lane adds up each run of equal keys
//      in its segment. A run that neither continues from the previous segment nor into the next
//      is the whole bucket: the lane writes it to the bucket array (it is the only writer: no
//      atomics on points). The (at most two) runs that cross the segment's ends go, with their
//      keys, to the next level's array, two slots per segment (an unused slot is EMPTY and keeps
//      the segment's first / last key, so the next array is sorted too). Level 0 gathers affine
//      bases (mixed additions); the levels above add XYZZ partial sums. The array shrinks by
//      SEG / 2 per level and the last level is one segment, whose runs are all whole.
//      No lane's chain of additions is longer than SEG at any level, whatever the distribution
//      of the scalars: a bucket holding half of a column's rows is SEG-entry pieces at level 0,
//      then SEG-piece sums at level 1, and so on: ceil(log_(SEG/2) n) levels.
//   4. window_kernel: sum_j j B_j of one (column, window) per workgroup: each thread takes a
//      contiguous piece of the buckets, forms its running sums (top down: run += B_j, acc += run)
//      and adds (piece offset) x run by double-and-add; the pieces are summed by an LDS tree.
//   5. horner_kernel: one lane per column combines the windows (c doublings, one addition each),
//      adds the pass into the column's accumulator and, after the last chunk, makes it affine
//      with one inv_safegcd (B2F_ERR_CHECK through the sticky flag if that fails).
//
// b2f_msm_cells_dev commits columns cut from u32 cells (the trace's advice and fixed columns) with
// the same steps 2 to 4 behind a front end of its own: recode_cells_kernel gives a column of `bits`
// bits ceil((bits + 1) / c) windows where a field element has ceil(256 / c), horner_cells_kernel
// runs over those windows alone, tail_kernel multiplies the call's few full scalars (the blinding
// rows) out on a side stream, and finish_cells_kernel adds the two and makes the sum affine.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <rocprim/device/device_radix_sort.hpp>

#include "../../include/b2f.h"
#include "b2f_curve.h"
#include "b2f_field.h"
#include "b2f_launch.h"

namespace b2f {

namespace {

constexpr uint32_t SEG = 32;             // entries per lane and level of the bucket reduction
constexpr uint32_t EMPTY = 0x80000000u;  // key bit: the entry holds no point
constexpr uint32_t KEY_MASK = 0x7fffffffu;
constexpr uint32_t WIN_THREADS = 128;    // window_kernel's workgroup
constexpr uint64_t CAP_ENTRIES = 1ull << 24;  // digits of one pass
constexpr uint64_t CAP_BUCKETS = 1ull << 20;  // buckets of one pass (128 bytes each)
constexpr uint32_t SCALAR_BITS = 255;         // both scalar moduli are below 2^255

inline uint64_t align256(uint64_t x) { return (x + 255) & ~255ull; }
inline uint32_t log2_floor(uint64_t x) {
  uint32_t l = 0;
  while (x >>= 1) l++;
  return l;
}

// The radix sort's temporary storage for n pairs. rocprim's own size query needs a device, and
// the plan is host code, so this is a bound: rocprim 's query on gfx950 returns 8 n (a second
// copy of the keys and values) + n / 16 + a few KiB of histograms and look-back state for
// n = 2^13 .. 2^25 and 256 bytes below that. The launcher asks rocprim for the real figure at every
// pass and fails with hipErrorOutOfMemory if it were ever larger.
inline uint64_t sort_temp_bound(uint64_t n) { return align256(9 * n + (1ull << 20)); }

}  // namespace

uint32_t msm_default_window(uint64_t len) {
  // floor((log2 len + 3) / 2), at least 3: 10 bits at 2^17 and 11 at 2^20, the widths the sweep
  // of tools/bench_msm.py --sweep finds fastest or within 3 % of it on both curves
  // (profiles/msm_bench.jsonl). The time is flat over c = 9..13 there: a wider window
  // has fewer digits to sort and add but more buckets to reduce. Below 2^10 the call is a few
  // launches' latency whatever c is; 3 keeps the digits of a short column few.
  const uint32_t c = (log2_floor(len) + 3) / 2;
  return c < 3 ? 3 : c > 16 ? 16 : c;
}

bool msm_plan_of(uint64_t len, uint32_t n_cols, uint32_t force_c, uint32_t force_g, MsmPlan* p) {
  if (len == 0 || len > (1ull << 28) || n_cols == 0 || force_c > 16) return false;
  memset(p, 0, sizeof *p);
  const uint32_t c = force_c ? force_c : msm_default_window(len);
  p->c = c;
  p->windows = (SCALAR_BITS + 1 + c - 1) / c;  // the scalar's bits and the recoding carry
  p->buckets = 1u << (c - 1);
  const uint64_t wb = (uint64_t)p->windows * p->buckets;
  uint64_t g;
  if (force_g) {
    g = force_g < n_cols ? force_g : n_cols;
    if (g * wb > CAP_BUCKETS || g * p->windows > CAP_ENTRIES) return false;
  } else {
    const uint64_t rows = len < CAP_ENTRIES / p->windows ? len : CAP_ENTRIES / p->windows;
    g = CAP_ENTRIES / (rows * p->windows);
    if (g > CAP_BUCKETS / wb) g = CAP_BUCKETS / wb;
    if (g < 1) g = 1;
    if (g > n_cols) g = n_cols;
  }
  p->group = (uint32_t)g;
  uint64_t chunk = CAP_ENTRIES / (g * p->windows);
  if (chunk > len) chunk = len;
  p->chunk = chunk;
  // Scratch: sized by bounds that grow with len (the pass itself may be smaller): the digits of
  // n_cols columns of len rounded up to a power of two, capped by the pass limit
  uint64_t e = 2ull << log2_floor(len);
  e = e * p->windows;
  if (e > CAP_ENTRIES / n_cols) e = CAP_ENTRIES; else e *= n_cols;
  if (e < g * chunk * p->windows) e = g * chunk * p->windows;  // (never: the bound covers the pass)
  p->cap_entries = e;
  uint64_t bk = wb > CAP_BUCKETS / n_cols ? CAP_BUCKETS : wb * n_cols;
  if (bk < g * wb) bk = g * wb;
  p->cap_buckets = bk;
  const uint64_t n1 = 2 * ((e + SEG - 1) / SEG), n2 = 2 * ((n1 + SEG - 1) / SEG);
  uint64_t off = 0;
  p->off_keys_a = off; off += align256(4 * e);
  p->off_keys_b = off; off += align256(4 * e);
  p->off_vals_a = off; off += align256(4 * e);
  p->off_vals_b = off; off += align256(4 * e);
  p->off_sort = off; p->sort_bytes = sort_temp_bound(e); off += p->sort_bytes;
  p->off_pkey_a = off; off += align256(4 * n1);
  p->off_pkey_b = off; off += align256(4 * n2);
  p->off_ppt_a = off; off += align256(128 * n1);
  p->off_ppt_b = off; off += align256(128 * n2);
  p->off_buckets = off; off += align256(128 * bk);
  // the window sums and column accumulators of a group: g windows <= g windows buckets <= the
  // bucket limit, and g <= n_cols; sized by that (it does not shrink as len grows and g falls)
  const uint64_t gw = n_cols > CAP_BUCKETS / 256 ? CAP_BUCKETS : (uint64_t)n_cols * 256;
  p->off_win = off; off += align256(128 * gw);
  p->off_acc = off; off += align256(128 * (n_cols < CAP_BUCKETS ? n_cols : CAP_BUCKETS));
  p->scratch_bytes = off;
  return true;
}

namespace {

using namespace field;
using namespace curve;

// ---- 1. recode -------------------------------------------------------------------------------
template <class C, bool MONT>
__global__ __launch_bounds__(256) void recode_kernel(const uint64_t* __restrict__ scalars, uint64_t rows,
                                                     uint64_t r0, uint32_t rc, uint32_t col0, uint32_t gc,
                                                     uint32_t c, uint32_t windows, uint32_t buckets,
                                                     const MsmBaseOffsets boff, uint32_t* __restrict__ keys,
                                                     uint32_t* __restrict__ vals) {
  using FS = typename C::Scalar;
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint64_t)gc * rc) return;
  const uint32_t cl = (uint32_t)(t / rc), r = (uint32_t)(t % rc);
  Fe v = load(scalars + ((uint64_t)(col0 + cl) * rows + r0 + r) * 4);
  if (MONT) v = to_canonical<FS>(v);
  const uint32_t half = 1u << (c - 1), sentinel = (gc * windows * buckets) | EMPTY;
  // the column's base offset (all zero unless the call gave any): selected, not indexed
  const uint32_t ci = col0 + cl;
  const uint32_t bo = ci == 0 ? boff.v[0] : ci == 1 ? boff.v[1] : ci == 2 ? boff.v[2] : ci == 3 ? boff.v[3] : 0u;
  uint32_t carry = 0;
  for (uint32_t w = 0; w < windows; w++) {
    const uint32_t bit = w * c;
    uint32_t raw = 0;
    if (bit < 256) {
      const uint32_t wi = bit >> 5, sh = bit & 31;
      uint64_t two = v.w[wi];
      if (wi < 7) two |= (uint64_t)v.w[wi + 1] << 32;
      raw = (uint32_t)(two >> sh) & ((1u << c) - 1);
    }
    raw += carry;
    uint32_t mag, neg = 0;
    if (raw > half) {  // d = raw - 2^c < 0, and the next window gets the 2^c back
      mag = (1u << c) - raw;
      neg = 1;
      carry = 1;
    } else {
      mag = raw;
      carry = 0;
    }
    const uint64_t at = ((uint64_t)w * gc + cl) * rc + r;
    keys[at] = mag ? ((cl * windows + w) * buckets + (mag - 1)) : sentinel;
    vals[at] = ((uint32_t)(r0 + r) + bo) | (neg << 31);
  }
}

// ---- 3. reduction by key ---------------------------------------------------------------------
// One level. LEVEL0: the entries are (key, value) digits and the points affine bases; otherwise
// (key, XYZZ) partial sums of the level below. Output: two slots per segment.
template <class C, bool LEVEL0>
__global__ __launch_bounds__(128) void reduce_kernel(const uint32_t* __restrict__ keys,
                                                     const uint32_t* __restrict__ vals,
                                                     const uint64_t* __restrict__ pts, uint32_t n,
                                                     const uint64_t* __restrict__ bases,
                                                     uint64_t* __restrict__ bucket, uint32_t n_buckets,
                                                     uint32_t* __restrict__ okeys, uint64_t* __restrict__ opts) {
  using F = typename C::Base;
  const uint32_t nseg = (n + SEG - 1) / SEG;
  const uint32_t seg = blockIdx.x * blockDim.x + threadIdx.x;
  if (seg >= nseg) return;
  const uint32_t i0 = seg * SEG, i1 = (n - i0 < SEG) ? n : i0 + SEG;
  const bool has_prev = i0 > 0, has_next = i1 < n;
  const uint32_t prevk = has_prev ? (keys[i0 - 1] & KEY_MASK) : 0;
  const uint32_t nextk = has_next ? (keys[i1] & KEY_MASK) : 0;
  const uint32_t firstk = keys[i0] & KEY_MASK;
  uint32_t cur = firstk;
  bool first_run = true, any = false, slot0 = false, slot1 = false;
  Xyzz acc = xyzz_identity();
  // a run [.., i) of key `cur` ended; open_right: it continues in the next segment
  auto flush = [&](bool open_right) {
    const bool open_left = first_run && has_prev && cur == prevk;
    if (open_left || open_right) {
      const uint32_t slot = first_run ? 0 : 1;
      okeys[2 * seg + slot] = cur | (any ? 0u : EMPTY);
      if (any) store_xyzz(opts + (2ull * seg + slot) * 16, acc);
      if (slot) slot1 = true; else slot0 = true;
    } else if (any && cur < n_buckets) {
      store_xyzz(bucket + (uint64_t)cur * 16, acc);
    }
  };
  // level 0: the next entry's key, value and base (a 64-byte gather) are fetched before the
  // current addition, whose ~10 products hide the gather's latency
  uint32_t kraw = keys[i0], v = 0;
  Affine q = affine_identity();
  if (LEVEL0 && !(kraw & EMPTY)) {
    v = vals[i0];
    q = load_affine(bases + (uint64_t)(v & KEY_MASK) * 8);
  }
#pragma unroll 1
  for (uint32_t i = i0; i < i1; i++) {
    uint32_t kraw_n = EMPTY, v_n = 0;
    Affine q_n = affine_identity();
    if (i + 1 < i1) {
      kraw_n = keys[i + 1];
      if (LEVEL0 && !(kraw_n & EMPTY)) {
        v_n = vals[i + 1];
        q_n = load_affine(bases + (uint64_t)(v_n & KEY_MASK) * 8);
      }
    }
    const uint32_t k = kraw & KEY_MASK;
    if (k != cur) {
      flush(false);
      acc = xyzz_identity();
      any = false;
      cur = k;
      first_run = false;
    }
    if (!(kraw & EMPTY)) {
      if (LEVEL0) {
        if (v >> 31) q = neg<F>(q);
        acc = madd<F>(acc, q);
      } else {
        acc = add<F>(acc, load_xyzz(pts + (uint64_t)i * 16));
      }
      any = true;
    }
    kraw = kraw_n;
    v = v_n;
    q = q_n;
  }
  flush(has_next && cur == nextk);
  if (!slot0) okeys[2 * seg] = firstk | EMPTY;
  if (!slot1) okeys[2 * seg + 1] = cur | EMPTY;
}

// ---- 4. window sums --------------------------------------------------------------------------
// k * p for k < 2^16, left-to-right double and add
template <class F>
__device__ Xyzz small_mul(const Xyzz& p, uint32_t k) {
  Xyzz r = xyzz_identity();
  if (!k) return r;
#pragma unroll 1
  for (int b = 31 - __builtin_clz(k); b >= 0; b--) {
    r = dbl<F>(r);
    if ((k >> b) & 1u) r = add<F>(r, p);
  }
  return r;
}

template <class C>
__global__ __launch_bounds__(WIN_THREADS) void window_kernel(const uint64_t* __restrict__ bucket,
                                                             uint32_t buckets, uint64_t* __restrict__ win) {
  using F = typename C::Base;
  __shared__ uint32_t lds[WIN_THREADS][33];  // one XYZZ per thread, padded against bank conflicts
  const uint32_t t = threadIdx.x;
  const uint64_t* b = bucket + (uint64_t)blockIdx.x * buckets * 16;
  const uint32_t m = (buckets + WIN_THREADS - 1) / WIN_THREADS;
  const uint32_t lo = t * m, hi = lo + m < buckets ? lo + m : buckets;  // buckets [lo, hi): multipliers lo + 1 ..
  Xyzz run = xyzz_identity(), acc = xyzz_identity();
  if (lo < buckets) {
#pragma unroll 1
    for (uint32_t j = hi; j-- > lo;) {
      run = add<F>(run, load_xyzz(b + (uint64_t)j * 16));
      acc = add<F>(acc, run);
    }
    if (lo) acc = add<F>(acc, small_mul<F>(run, lo));
  }
  auto put = [&](const Xyzz& p) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      lds[t][i] = p.x.w[i];
      lds[t][8 + i] = p.y.w[i];
      lds[t][16 + i] = p.zz.w[i];
      lds[t][24 + i] = p.zzz.w[i];
    }
  };
  auto get = [&](uint32_t u) {
    Xyzz p;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      p.x.w[i] = lds[u][i];
      p.y.w[i] = lds[u][8 + i];
      p.zz.w[i] = lds[u][16 + i];
      p.zzz.w[i] = lds[u][24 + i];
    }
    return p;
  };
  put(acc);
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = WIN_THREADS / 2; s > 0; s >>= 1) {
    if (t < s) {
      acc = add<F>(acc, get(t + s));
      put(acc);
    }
    __syncthreads();
  }
  if (t == 0) store_xyzz(win + (uint64_t)blockIdx.x * 16, acc);
}

// ---- 5. Horner over the windows, the column accumulator, the affine output ---------------------
template <class C>
__global__ __launch_bounds__(64) void horner_kernel(const uint64_t* __restrict__ win, uint32_t gc, uint32_t c,
                                                    uint32_t windows, uint64_t* __restrict__ colacc, int first,
                                                    int last, uint64_t* __restrict__ out, int* sticky) {
  using F = typename C::Base;
  const uint32_t cl = blockIdx.x * blockDim.x + threadIdx.x;
  if (cl >= gc) return;
  Xyzz acc = xyzz_identity();
#pragma unroll 1
  for (uint32_t w = windows; w-- > 0;) {
#pragma unroll 1
    for (uint32_t d = 0; d < c; d++) acc = dbl<F>(acc);
    acc = add<F>(acc, load_xyzz(win + ((uint64_t)cl * windows + w) * 16));
  }
  if (!first) acc = add<F>(acc, load_xyzz(colacc + (uint64_t)cl * 16));
  if (!last) {
    store_xyzz(colacc + (uint64_t)cl * 16, acc);
    return;
  }
  bool ok = true;
  const Affine a = to_affine<F>(acc, ok);
  if (!ok) atomicOr(sticky, 1 << B2F_ERR_CHECK);
  store_affine(out + (uint64_t)cl * 8, a);
}

// The scratch of a pass, carved by either plan (MsmPlan, CellsPlan: the same offsets by name).
struct PassScratch {
  uint32_t *keys_a, *keys_b, *vals_a, *vals_b;
  void* sort;
  uint64_t sort_bytes;
  uint32_t* pkey[2];
  uint64_t* ppt[2];
  uint64_t *bucket, *win, *colacc;
};
template <class Plan>
PassScratch carve(const Plan& p, char* scr) {
  PassScratch m;
  m.keys_a = reinterpret_cast<uint32_t*>(scr + p.off_keys_a);
  m.keys_b = reinterpret_cast<uint32_t*>(scr + p.off_keys_b);
  m.vals_a = reinterpret_cast<uint32_t*>(scr + p.off_vals_a);
  m.vals_b = reinterpret_cast<uint32_t*>(scr + p.off_vals_b);
  m.sort = scr + p.off_sort;
  m.sort_bytes = p.sort_bytes;
  m.pkey[0] = reinterpret_cast<uint32_t*>(scr + p.off_pkey_a);
  m.pkey[1] = reinterpret_cast<uint32_t*>(scr + p.off_pkey_b);
  m.ppt[0] = reinterpret_cast<uint64_t*>(scr + p.off_ppt_a);
  m.ppt[1] = reinterpret_cast<uint64_t*>(scr + p.off_ppt_b);
  m.bucket = reinterpret_cast<uint64_t*>(scr + p.off_buckets);
  m.win = reinterpret_cast<uint64_t*>(scr + p.off_win);
  m.colacc = reinterpret_cast<uint64_t*>(scr + p.off_acc);
  return m;
}

// Steps 2 to 4 of a pass: the n digits in keys_a / vals_a, of n_windows (column, window) pairs of
// `buckets` buckets each, become the n_windows window sums in m.win.
template <class C>
hipError_t sort_reduce_windows(const PassScratch& m, uint32_t n, uint32_t n_windows, uint32_t buckets,
                               const uint64_t* d_bases, hipStream_t s) {
  hipError_t e;
  const uint32_t n_buckets = n_windows * buckets;
  uint32_t end_bit = 1;
  while ((1ull << end_bit) <= n_buckets) end_bit++;  // the sentinel key n_buckets sorts too
  size_t need = 0;
  e = rocprim::radix_sort_pairs((void*)nullptr, need, m.keys_a, m.keys_b, m.vals_a, m.vals_b, (size_t)n, 0, end_bit, s);
  if (e != hipSuccess) return e;
  if (need > m.sort_bytes) return hipErrorOutOfMemory;
  need = m.sort_bytes;
  e = rocprim::radix_sort_pairs(m.sort, need, m.keys_a, m.keys_b, m.vals_a, m.vals_b, (size_t)n, 0, end_bit, s);
  if (e != hipSuccess) return e;
  if ((e = hipMemsetAsync(m.bucket, 0, 128ull * n_buckets, s)) != hipSuccess) return e;
  // level 0 reads the sorted digits; level l + 1 reads what level l wrote (ping-pong)
  uint32_t nl = n, nseg = (n + SEG - 1) / SEG;
  hipLaunchKernelGGL((reduce_kernel<C, true>), dim3((nseg + 127) / 128), dim3(128), 0, s, m.keys_b, m.vals_b,
                     (const uint64_t*)nullptr, nl, d_bases, m.bucket, n_buckets, m.pkey[0], m.ppt[0]);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  int src = 0;
  while (nseg > 1) {
    nl = 2 * nseg;
    nseg = (nl + SEG - 1) / SEG;
    hipLaunchKernelGGL((reduce_kernel<C, false>), dim3((nseg + 127) / 128), dim3(128), 0, s, m.pkey[src],
                       (const uint32_t*)nullptr, m.ppt[src], nl, (const uint64_t*)nullptr, m.bucket, n_buckets,
                       m.pkey[src ^ 1], m.ppt[src ^ 1]);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    src ^= 1;
  }
  hipLaunchKernelGGL((window_kernel<C>), dim3(n_windows), dim3(WIN_THREADS), 0, s, m.bucket, buckets, m.win);
  return hipGetLastError();
}

template <class C, bool MONT>
hipError_t run_msm(const MsmPlan& p, const uint64_t* d_scalars, uint64_t rows, uint64_t len, uint32_t n_cols,
                   const uint64_t* d_bases, uint64_t* d_out, char* scr, int* sticky, hipStream_t s,
                   const MsmBaseOffsets& boff) {
  const PassScratch m = carve(p, scr);
  hipError_t e;
  for (uint32_t col0 = 0; col0 < n_cols; col0 += p.group) {
    const uint32_t gc = n_cols - col0 < p.group ? n_cols - col0 : p.group;
    for (uint64_t r0 = 0; r0 < len; r0 += p.chunk) {
      const uint32_t rc = (uint32_t)(len - r0 < p.chunk ? len - r0 : p.chunk);
      const uint64_t n64 = (uint64_t)gc * rc * p.windows;
      const uint32_t n_buckets = gc * p.windows * p.buckets;
      if (n64 > p.cap_entries || n_buckets > p.cap_buckets) return hipErrorInvalidValue;  // the plan's own bound
      const uint64_t threads = (uint64_t)gc * rc;
      hipLaunchKernelGGL((recode_kernel<C, MONT>), dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, s, d_scalars,
                         rows, r0, rc, col0, gc, p.c, p.windows, p.buckets, boff, m.keys_a, m.vals_a);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      if ((e = sort_reduce_windows<C>(m, (uint32_t)n64, gc * p.windows, p.buckets, d_bases, s)) != hipSuccess) return e;
      hipLaunchKernelGGL((horner_kernel<C>), dim3((gc + 63) / 64), dim3(64), 0, s, m.win, gc, p.c, p.windows, m.colacc,
                         r0 == 0 ? 1 : 0, r0 + rc >= len ? 1 : 0, d_out + (uint64_t)col0 * 8, sticky);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

// ---- the cell front end (b2f_msm_cells_dev) ----------------------------------------------------
// 1'. One lane per (column of the group, row of the chunk); consecutive lanes read consecutive
// cells. The column's scalar is its field of the cell, zero from `avail` on (never loaded); it
// becomes the column's own `windows` signed digits in recode_kernel's encoding, at entries
// (wbase + w) * rc + r with keys (wbase + w) * buckets + |d| - 1. windows * c >= bits + 1, so the
// top window's digit is at most 2^(c-1) - 1 plus the carry: it never carries out.
__global__ __launch_bounds__(256) void recode_cells_kernel(const uint32_t* __restrict__ cells,
                                                           const CellColumn* __restrict__ cols, uint32_t r0,
                                                           uint32_t rc, uint32_t gc, uint32_t c, uint32_t buckets,
                                                           uint32_t sentinel, uint32_t* __restrict__ keys,
                                                           uint32_t* __restrict__ vals) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (uint64_t)gc * rc) return;
  const uint32_t cl = (uint32_t)(t / rc), r = (uint32_t)(t % rc);
  const CellColumn d = cols[cl];
  const uint32_t row = r0 + r;
  uint64_t v = 0;  // 64 bits: the top window's shift may be 32
  if (row < d.avail) v = (cells[d.offset + row] >> d.shift) & d.mask;
  const uint32_t half = 1u << (c - 1);
  uint32_t carry = 0;
  for (uint32_t w = 0; w < d.windows; w++) {
    const uint32_t raw = ((uint32_t)(v >> (w * c)) & ((1u << c) - 1)) + carry;
    uint32_t mag, neg = 0;
    if (raw > half) {  // d = raw - 2^c < 0, and the next window gets the 2^c back
      mag = (1u << c) - raw;
      neg = 1;
      carry = 1;
    } else {
      mag = raw;
      carry = 0;
    }
    const uint32_t at = (d.wbase + w) * rc + r;
    keys[at] = mag ? ((d.wbase + w) * buckets + (mag - 1)) : sentinel;
    vals[at] = row | (neg << 31);
  }
}

// 5'. Horner over the column's own windows (windows * c doublings), added into the column's
// accumulator; the affine conversion is finish_cells_kernel's, after the last pass and the tail.
template <class C>
__global__ __launch_bounds__(64) void horner_cells_kernel(const uint64_t* __restrict__ win,
                                                          const CellColumn* __restrict__ cols, uint32_t gc, uint32_t c,
                                                          uint64_t* __restrict__ colacc, int first) {
  using F = typename C::Base;
  const uint32_t cl = blockIdx.x * blockDim.x + threadIdx.x;
  if (cl >= gc) return;
  const CellColumn d = cols[cl];
  Xyzz acc = xyzz_identity();
#pragma unroll 1
  for (uint32_t w = d.windows; w-- > 0;) {
#pragma unroll 1
    for (uint32_t k = 0; k < c; k++) acc = dbl<F>(acc);
    acc = add<F>(acc, load_xyzz(win + (uint64_t)(d.wbase + w) * 16));
  }
  if (!first) acc = add<F>(acc, load_xyzz(colacc + (uint64_t)cl * 16));
  store_xyzz(colacc + (uint64_t)cl * 16, acc);
}

// The tail: one wave per column, lane t the full-width product tail[col][t] * base[len + t]
// (curve::scalar_mul), the lanes' points summed by an LDS tree into tailacc[col].
constexpr uint32_t TAIL_MAX = 64;
template <class C, bool MONT>
__global__ __launch_bounds__(TAIL_MAX) void tail_kernel(const uint64_t* __restrict__ tail, uint32_t tail_rows,
                                                        const uint64_t* __restrict__ bases,
                                                        uint64_t* __restrict__ tailacc) {
  using F = typename C::Base;
  using FS = typename C::Scalar;
  __shared__ uint32_t lds[TAIL_MAX][33];  // one XYZZ per lane, padded against bank conflicts
  const uint32_t t = threadIdx.x;
  Xyzz acc = xyzz_identity();
  if (t < tail_rows) {
    Fe k = load(tail + ((uint64_t)blockIdx.x * tail_rows + t) * 4);
    if (MONT) k = to_canonical<FS>(k);
    acc = scalar_mul<F>(load_affine(bases + (uint64_t)t * 8), k);
  }
  auto put = [&](const Xyzz& p) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      lds[t][i] = p.x.w[i];
      lds[t][8 + i] = p.y.w[i];
      lds[t][16 + i] = p.zz.w[i];
      lds[t][24 + i] = p.zzz.w[i];
    }
  };
  auto get = [&](uint32_t u) {
    Xyzz p;
#pragma unroll
    for (int i = 0; i < 8; i++) {
      p.x.w[i] = lds[u][i];
      p.y.w[i] = lds[u][8 + i];
      p.zz.w[i] = lds[u][16 + i];
      p.zzz.w[i] = lds[u][24 + i];
    }
    return p;
  };
  put(acc);
  __syncthreads();
#pragma unroll 1
  for (uint32_t s = TAIL_MAX / 2; s > 0; s >>= 1) {
    if (t < s) {
      acc = add<F>(acc, get(t + s));
      put(acc);
    }
    __syncthreads();
  }
  if (t == 0) store_xyzz(tailacc + (uint64_t)blockIdx.x * 16, acc);
}

// out[col] = affine(colacc[col] + tailacc[col]) (tailacc null: a call without a tail)
template <class C>
__global__ __launch_bounds__(64) void finish_cells_kernel(const uint64_t* __restrict__ colacc,
                                                          const uint64_t* __restrict__ tailacc, uint32_t n_cols,
                                                          uint64_t* __restrict__ out, int* sticky) {
  using F = typename C::Base;
  const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= n_cols) return;
  Xyzz acc = load_xyzz(colacc + (uint64_t)col * 16);
  if (tailacc) acc = add<F>(acc, load_xyzz(tailacc + (uint64_t)col * 16));
  bool ok = true;
  const Affine a = to_affine<F>(acc, ok);
  if (!ok) atomicOr(sticky, 1 << B2F_ERR_CHECK);
  store_affine(out + (uint64_t)col * 8, a);
}

// the passes over (group, row chunk): every column's accumulator ends in m.colacc[column]
template <class C>
hipError_t run_cell_passes(const CellsPlan& p, const PassScratch& m, const CellColumn* desc, const uint32_t* d_cells,
                           uint64_t len, const uint64_t* d_bases, hipStream_t s) {
  hipError_t e;
  for (size_t g = 0; g + 1 < p.first.size(); g++) {
    const uint32_t col0 = p.first[g], gc = p.first[g + 1] - col0;
    const CellColumn& lastc = p.image[col0 + gc - 1];
    const uint32_t n_windows = lastc.wbase + lastc.windows;
    for (uint64_t r0 = 0; r0 < len; r0 += p.chunk) {
      const uint32_t rc = (uint32_t)(len - r0 < p.chunk ? len - r0 : p.chunk);
      const uint64_t n64 = (uint64_t)n_windows * rc, nb64 = (uint64_t)n_windows * p.buckets;
      if (n64 > p.cap_entries || nb64 > p.cap_buckets) return hipErrorInvalidValue;  // the plan's own bound
      const uint64_t threads = (uint64_t)gc * rc;
      hipLaunchKernelGGL(recode_cells_kernel, dim3((uint32_t)((threads + 255) / 256)), dim3(256), 0, s, d_cells,
                         desc + col0, (uint32_t)r0, rc, gc, p.c, p.buckets, (uint32_t)nb64 | EMPTY, m.keys_a, m.vals_a);
      if ((e = hipGetLastError()) != hipSuccess) return e;
      if ((e = sort_reduce_windows<C>(m, (uint32_t)n64, n_windows, p.buckets, d_bases, s)) != hipSuccess) return e;
      hipLaunchKernelGGL((horner_cells_kernel<C>), dim3((gc + 63) / 64), dim3(64), 0, s, m.win, desc + col0, gc, p.c,
                         m.colacc + (uint64_t)col0 * 16, r0 == 0 ? 1 : 0);
      if ((e = hipGetLastError()) != hipSuccess) return e;
    }
  }
  return hipSuccess;
}

template <class C, bool MONT>
hipError_t run_msm_cells(const CellsPlan& p, const uint32_t* d_cells, uint32_t n_cols, uint64_t len,
                         const uint64_t* d_tail, uint32_t tail_rows, const uint64_t* d_bases, uint64_t* d_out,
                         char* scr, int* sticky, hipStream_t s2, hipEvent_t ev_fork, hipEvent_t ev_join,
                         hipStream_t s) {
  const PassScratch m = carve(p, scr);
  const CellColumn* desc = reinterpret_cast<const CellColumn*>(scr + p.off_desc);
  uint64_t* tailacc = reinterpret_cast<uint64_t*>(scr + p.off_tail);
  hipError_t e = hipSuccess;
  bool forked = false;
  if (tail_rows) {
    // the tail's 255-doubling chains run on s2 beside the cell passes; they read only the caller's
    // tail and bases and write tailacc, which nothing else touches before the join (s2 == s: the
    // diagnostics library's serial form, the overlap's A/B)
    if (s2 != s) {
      if ((e = hipEventRecord(ev_fork, s)) != hipSuccess) return e;
      if ((e = hipStreamWaitEvent(s2, ev_fork, 0)) != hipSuccess) return e;
      forked = true;
    }
    hipLaunchKernelGGL((tail_kernel<C, MONT>), dim3(n_cols), dim3(TAIL_MAX), 0, s2, d_tail, tail_rows,
                       d_bases + len * 8, tailacc);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = run_cell_passes<C>(p, m, desc, d_cells, len, d_bases, s);
  if (forked) {  // on every path: s2 never runs on past the call
    hipError_t j = hipEventRecord(ev_join, s2);
    if (j == hipSuccess) j = hipStreamWaitEvent(s, ev_join, 0);
    if (e == hipSuccess) e = j;
  }
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((finish_cells_kernel<C>), dim3((n_cols + 63) / 64), dim3(64), 0, s, m.colacc,
                     tail_rows ? tailacc : (const uint64_t*)nullptr, n_cols, d_out, sticky);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_msm(const MsmPlan& plan, const uint64_t* d_scalars, uint64_t rows, uint64_t len, uint32_t n_cols,
                      const uint64_t* d_bases, uint32_t form, uint64_t* d_out, void* scratch, int* sticky,
                      hipStream_t s, const MsmBaseOffsets* base_offsets) {
  hipError_t e = hipSuccess;
  MsmBaseOffsets boff = {{0, 0, 0, 0}};
  if (base_offsets) {
    if (n_cols > MSM_OFFSET_COLS) return hipErrorInvalidValue;
    boff = *base_offsets;
  }
  field::with_curve_form(form, [&](auto c, auto mont) {
    using C = decltype(c);
    e = run_msm<C, decltype(mont)::value>(plan, d_scalars, rows, len, n_cols, d_bases, d_out, (char*)scratch, sticky,
                                          s, boff);
  });
  return e;
}

uint32_t msm_cells_default_window(uint64_t len, uint32_t bits) {
  // The fewest windows a width the length can afford gives, at the narrowest width that gives them:
  // the digits (sorted and added) go with the windows, the buckets (cleared and summed) with 2^c.
  // The widest affordable width is floor((log2 len + 2) / 2), in [3, 16]: 9 at 2^17, 11 at 2^20.
  // A 32-bit cell is then 4 windows of 9 bits at 2^17 rows and 3 of 11 at 2^20, a 16-bit limb 2 of
  // 9, a selector bit 1 of 2: the fastest width of the sweep in each of its eight rows (DESIGN.md
  // 4.9, tools/bench_msm_cells.py --sweep).
  uint32_t cmax = (log2_floor(len) + 2) / 2;
  cmax = cmax < 3 ? 3 : cmax > 16 ? 16 : cmax;
  const uint32_t wmin = (bits + 1 + cmax - 1) / cmax;
  return (bits + 1 + wmin - 1) / wmin;
}

bool msm_cells_plan_of(const b2f_cell_column* cols, uint32_t n_cols, uint64_t len, uint32_t force_c, uint32_t force_g,
                       CellsPlan* p) {
  if (!cols || len == 0 || len > (1ull << 28) || n_cols == 0 || n_cols > 4096 || force_c > 16) return false;
  uint32_t max_bits = 0;
  for (uint32_t i = 0; i < n_cols; i++) {
    if (cols[i].bits == 0 || cols[i].bits > 32 || cols[i].shift > 31 || cols[i].shift + cols[i].bits > 32) return false;
    if (cols[i].bits > max_bits) max_bits = cols[i].bits;
  }
  const uint32_t c = force_c ? force_c : msm_cells_default_window(len, max_bits);
  p->c = c;
  p->buckets = 1u << (c - 1);
  p->image.assign(n_cols, CellColumn());
  uint64_t sum_w = 0;
  uint32_t max_w = 0;
  for (uint32_t i = 0; i < n_cols; i++) {
    CellColumn& d = p->image[i];
    d.offset = cols[i].offset;
    d.avail = (uint32_t)(cols[i].avail < len ? cols[i].avail : len);
    d.shift = cols[i].shift;
    d.mask = cols[i].bits == 32 ? 0xffffffffu : (1u << cols[i].bits) - 1;
    d.windows = (cols[i].bits + 1 + c - 1) / c;  // the field's bits and the recoding carry
    d.pad = 0;
    sum_w += d.windows;
    if (d.windows > max_w) max_w = d.windows;
  }
  p->digits = len * sum_w;
  // a chunk of rows holds the widest column; a group is a run of columns whose windows fit the pass
  uint64_t chunk = CAP_ENTRIES / max_w;
  if (chunk > len) chunk = len;
  p->chunk = chunk;
  uint64_t wcap = CAP_ENTRIES / chunk;
  if (wcap > CAP_BUCKETS / p->buckets) wcap = CAP_BUCKETS / p->buckets;
  if (max_w > wcap) return false;
  p->first.assign(1, 0);
  uint32_t w = 0, count = 0;
  for (uint32_t i = 0; i < n_cols; i++) {
    if (count && (w + p->image[i].windows > wcap || (force_g && count == force_g))) {
      p->first.push_back(i);
      w = count = 0;
    }
    p->image[i].wbase = w;
    w += p->image[i].windows;
    count++;
  }
  p->first.push_back(n_cols);
  // Scratch, by bounds that do not shrink as len or n_cols grows (as msm_plan_of's): the call's
  // digits at len rounded up to a power of two and all its windows' buckets, capped by the pass
  uint64_t e = (2ull << log2_floor(len)) * sum_w;
  if (e > CAP_ENTRIES) e = CAP_ENTRIES;
  p->cap_entries = e;
  uint64_t bk = sum_w * p->buckets;
  if (bk > CAP_BUCKETS) bk = CAP_BUCKETS;
  p->cap_buckets = bk;
  const uint64_t n1 = 2 * ((e + SEG - 1) / SEG), n2 = 2 * ((n1 + SEG - 1) / SEG);
  uint64_t off = 0;
  p->off_keys_a = off; off += align256(4 * e);
  p->off_keys_b = off; off += align256(4 * e);
  p->off_vals_a = off; off += align256(4 * e);
  p->off_vals_b = off; off += align256(4 * e);
  p->off_sort = off; p->sort_bytes = sort_temp_bound(e); off += p->sort_bytes;
  p->off_pkey_a = off; off += align256(4 * n1);
  p->off_pkey_b = off; off += align256(4 * n2);
  p->off_ppt_a = off; off += align256(128 * n1);
  p->off_ppt_b = off; off += align256(128 * n2);
  p->off_buckets = off; off += align256(128 * bk);
  p->off_win = off; off += align256(128 * (sum_w < CAP_BUCKETS ? sum_w : CAP_BUCKETS));
  p->off_acc = off; off += align256(128ull * n_cols);
  p->off_tail = off; off += align256(128ull * n_cols);
  p->off_desc = off; off += align256(sizeof(CellColumn) * (uint64_t)n_cols);
  p->scratch_bytes = off;
  return true;
}

hipError_t launch_msm_cells(const CellsPlan& plan, const uint32_t* d_cells, uint32_t n_cols, uint64_t len,
                            const uint64_t* d_tail, uint32_t tail_rows, const uint64_t* d_bases, uint32_t form,
                            uint64_t* d_out, void* scratch, int* sticky, hipStream_t s2, hipEvent_t ev_fork,
                            hipEvent_t ev_join, hipStream_t s) {
  if (tail_rows > TAIL_MAX) return hipErrorInvalidValue;
  hipError_t e = hipSuccess;
  field::with_curve_form(form, [&](auto c, auto mont) {
    using C = decltype(c);
    e = run_msm_cells<C, decltype(mont)::value>(plan, d_cells, n_cols, len, d_tail, tail_rows, d_bases, d_out,
                                                (char*)scratch, sticky, s2, ev_fork, ev_join, s);
  });
  return e;
}

#ifdef B2F_DIAG
// Diagnostics build only: B2F_DIAG_MSM_PLAN=c[,g] read at the call forces the window width
// (1..16) and, optionally, the column group (1..4096) of b2f_msm_dev / b2f_msm_plan and of
// b2f_msm_cells_dev / b2f_msm_cells_plan (tests/test_gpu_msm.py, tests/test_gpu_msm_cells.py: widths
// the product never picks at small lengths). 0: unset; 1: *c and *g
// (0: not given) hold the forced plan; -1: anything else (decimal digits only, no sign, space or
// leading zero). There is no fallback: the caller refuses the call on -1.
int diag_msm_plan(uint32_t* c, uint32_t* g) {
  const char* v = getenv("B2F_DIAG_MSM_PLAN");
  *c = *g = 0;
  if (!v) return 0;
  uint32_t val[2] = {0, 0};
  int nv = 0;
  for (const char* q = v;;) {
    if (nv == 2 || *q < '1' || *q > '9') return -1;
    uint32_t x = 0;
    int digits = 0;
    while (*q >= '0' && *q <= '9') {
      x = x * 10 + (uint32_t)(*q - '0');
      if (++digits > 4) return -1;
      q++;
    }
    val[nv++] = x;
    if (!*q) break;
    if (*q != ',') return -1;
    q++;
  }
  if (val[0] > 16 || (nv == 2 && val[1] > 4096)) return -1;
  *c = val[0];
  *g = nv == 2 ? val[1] : 0;
  return 1;
}
#endif

}  // namespace b2f
