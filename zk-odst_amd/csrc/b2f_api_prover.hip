// b2f_api_prover.hip -- the C ABI of the prover calls of include/b2f.h: column export, the lookup,
// permutation, NTT, quotient and opening steps, the commitments. Host code only: argument checks, the context's
// scratch and table blocks, and the launchers of b2f_launch.h / b2f_open.h. The trace calls, the
// context itself and keygen are in b2f_kernels.hip.
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../include/b2f.h"
#include "b2f_field.h"
#include "b2f_host.h"
#include "b2f_launch.h"
#include "b2f_layout.h"
#include "b2f_open.h"

using namespace b2f;
using field::fe_canonical;

namespace {

// the side stream and events of the grand products (created on first use)
int ensure_side(b2f_ctx* ctx) {
  if (!ctx->s2) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->s2, hipStreamNonBlocking));
  if (!ctx->ev_fork) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
  if (!ctx->ev_join) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
  if (!ctx->s3) HIPCHK(ctx, hipStreamCreateWithFlags(&ctx->s3, hipStreamNonBlocking));
  if (!ctx->ev_tab) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_tab, hipEventDisableTiming));
  if (!ctx->ev_sorted) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->ev_sorted, hipEventDisableTiming));
  return B2F_OK;
}

}  // namespace

extern "C" {

B2F_API int b2f_export_fp_dev(b2f_ctx* ctx, const uint32_t* d_advice, uint64_t total_rows,
                              uint64_t row_begin, uint64_t nrows, uint32_t form,
                              uint64_t* d_out, uint64_t out_rows, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  if (!d_advice || !d_out) return set_err(ctx, B2F_ERR_ARG, "export: null buffer");
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "export: unknown form %u", form);
  if ((uintptr_t)d_out & 15) return set_err(ctx, B2F_ERR_ARG, "export: d_out must be 16-byte aligned");
  if (row_begin > total_rows || nrows > total_rows - row_begin)
    return set_err(ctx, B2F_ERR_ROWS, "export: rows [%llu, +%llu) exceed total_rows %llu",
                   (unsigned long long)row_begin, (unsigned long long)nrows,
                   (unsigned long long)total_rows);
  if (out_rows < nrows) return set_err(ctx, B2F_ERR_ROWS, "export: out_rows < nrows");
  if (nrows == 0) return B2F_OK;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int tk = timed_begin(ctx, B2F_KERNEL_EXPORT, s);
  HIPCHK(ctx, launch_export_fp(d_advice, total_rows, row_begin, nrows, form, d_out, out_rows,
                               ctx->cu_count, reinterpret_cast<unsigned*>(ctx->d_status + 4), s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_export_fixed_fp_dev(b2f_ctx* ctx, const uint32_t* d_fixed, uint64_t total_rows,
                                    uint64_t row_begin, uint64_t nrows, uint32_t form,
                                    uint64_t* d_out, uint64_t out_rows, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  if (!d_fixed || !d_out) return set_err(ctx, B2F_ERR_ARG, "export fixed: null buffer");
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "export fixed: unknown form %u", form);
  if ((uintptr_t)d_out & 15) return set_err(ctx, B2F_ERR_ARG, "export fixed: d_out must be 16-byte aligned");
  if (row_begin > total_rows || nrows > total_rows - row_begin)
    return set_err(ctx, B2F_ERR_ROWS, "export fixed: rows [%llu, +%llu) exceed total_rows %llu",
                   (unsigned long long)row_begin, (unsigned long long)nrows,
                   (unsigned long long)total_rows);
  if (out_rows < nrows) return set_err(ctx, B2F_ERR_ROWS, "export fixed: out_rows < nrows");
  if (nrows >= (1ull << 38)) return set_err(ctx, B2F_ERR_ROWS, "export fixed: 2^38 rows or more in one call");
  if (nrows == 0) return B2F_OK;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int tk = timed_begin(ctx, B2F_KERNEL_EXPORT, s);
  HIPCHK(ctx, launch_export_fixed_fp(d_fixed, row_begin, nrows, form, d_out, out_rows, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_lookup_columns_dev(b2f_ctx* ctx, const uint32_t* d_advice, uint64_t total_rows,
                                   const uint64_t* d_row_begin, uint32_t n_circuits,
                                   uint64_t usable_rows, const uint64_t theta[4],
                                   const uint64_t beta[4], const uint64_t gamma[4], uint32_t form,
                                   uint64_t* d_out, uint64_t out_rows, uint64_t* d_first_bad,
                                   void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  if (!d_advice || !d_row_begin || !theta || !beta || !gamma || !d_out || !d_first_bad)
    return set_err(ctx, B2F_ERR_ARG, "lookup: null buffer");
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "lookup: unknown form %u", form);
  if ((uintptr_t)d_out & 15) return set_err(ctx, B2F_ERR_ARG, "lookup: d_out must be 16-byte aligned");
  if (usable_rows < (1ull << 16) || usable_rows > (1ull << 31))
    return set_err(ctx, B2F_ERR_ROWS, "lookup: usable_rows %llu not in [2^16, 2^31]",
                   (unsigned long long)usable_rows);
  if (out_rows < usable_rows + 1)
    return set_err(ctx, B2F_ERR_ROWS, "lookup: out_rows < usable_rows + 1");
  if (!fe_canonical(form, theta) || !fe_canonical(form, beta) || !fe_canonical(form, gamma))
    return set_err(ctx, B2F_ERR_ARG, "lookup: challenge not a canonical field element");
  if (n_circuits == 0) return B2F_OK;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // circuits per pass: at most 2^24 rows (128 circuits of 2^17), enough workgroups to fill
  // the chip several times over; per-circuit scratch is 1.1 MiB (count, pos, D, LP, samples) +
  // 224 B per 1,024-row block (num products, prefixes, look-back state)
  uint32_t group = (uint32_t)((1ull << 24) / usable_rows);
  if (group < 1) group = 1;
  if (group > n_circuits) group = n_circuits;
  const size_t need = lookup_scratch_bytes(group, usable_rows);
  if (int rc = grow_device(ctx, &ctx->d_lk, &ctx->lk_cap, need, 1, s)) return rc;
  if (int rc = ensure_side(ctx)) return rc;
  int tk = timed_begin(ctx, B2F_KERNEL_LOOKUP, s);
  HIPCHK(ctx, launch_lookup(d_advice, total_rows, d_row_begin, n_circuits, usable_rows, theta, beta,
                            gamma, form, d_out, out_rows, d_first_bad, ctx->d_lk, group,
                            ctx->d_status + 2, ctx->s2, ctx->ev_fork, ctx->ev_join, ctx->s3,
                            ctx->ev_tab, ctx->ev_sorted, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_spread_table_dev(b2f_ctx* ctx, uint64_t usable_rows, uint32_t form, uint64_t* d_out,
                                 uint64_t out_rows, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  if (!d_out || ((uintptr_t)d_out & 15)) return set_err(ctx, B2F_ERR_ARG, "spread table: d_out null or unaligned");
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "spread table: unknown form %u", form);
  if (usable_rows < (1ull << 16) || usable_rows >= (1ull << 32) || out_rows < usable_rows)
    return set_err(ctx, B2F_ERR_ROWS, "spread table: need 2^16 <= usable_rows < 2^32, out_rows >= usable_rows");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int tk = timed_begin(ctx, B2F_KERNEL_EXPORT, s);
  HIPCHK(ctx, launch_spread_table(usable_rows, form, d_out, out_rows, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

}  // extern "C"

namespace {
// The host part shared by the permutation calls: field checks, the instance row map, the mapping
// patterns (built once per rounds, pooled on the device), the instance table (pinned staging,
// async upload) and the scratch (need_scr bytes). *row0 / *used: the circuit's first trace row
// and its rows. Whatever the caller launches next is stream-ordered after the table upload.
// Its steps, shared with the batch call (which stages a table of several circuits):
// perm_check_fields, perm_rounds, perm_patterns, perm_stage (-> the pinned staging to fill),
// perm_upload.
int perm_check_fields(b2f_ctx* ctx, const char* what, uint32_t k, uint32_t form,
                      const uint64_t* const* elems, int n_elems) {
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "%s: unknown form %u", what, form);
  if (k < 10 || k > 30) return set_err(ctx, B2F_ERR_ARG, "%s: k %u not in [10, 30]", what, k);
  for (int i = 0; i < n_elems; i++)
    if (!fe_canonical(form, elems[i])) return set_err(ctx, B2F_ERR_ARG, "%s: omega/delta/beta/gamma not canonical field elements", what);
  return B2F_OK;
}
// need: the rounds of instances 0 .. n - 1 of the row map (B2F_ERR_LAYOUT for a pair that is none)
int perm_rounds(b2f_ctx* ctx, const char* what, const uint64_t* h_offsets, size_t n,
                std::vector<uint32_t>& need) {
  for (size_t i = 0; i < n; i++) {
    const uint64_t R = h_offsets[i + 1] - h_offsets[i];
    if (h_offsets[i + 1] < h_offsets[i] || R < FIXED_ROWS || (R - FIXED_ROWS) % ROUND_ROWS ||
        (R - FIXED_ROWS) / ROUND_ROWS > B2F_MAX_ROUNDS)
      return set_err(ctx, B2F_ERR_LAYOUT, "%s: offsets[%zu..%zu] is not an instance", what, i, i + 1);
    need.push_back((uint32_t)((R - FIXED_ROWS) / ROUND_ROWS));
  }
  return B2F_OK;
}
// mapping patterns of the rounds in need[i0, i1): build the missing ones, rebuild the device
// pool if it lacks any
int perm_patterns(b2f_ctx* ctx, const char* what, const std::vector<uint32_t>& all, size_t i0, size_t i1,
                  hipStream_t s) {
  const std::vector<uint32_t> need(all.begin() + i0, all.begin() + i1);
  bool rebuild = false;
  for (uint32_t r : need) {
    if (!ctx->pm_pat.count(r)) {
      std::vector<uint32_t> m;
      if (!perm_mapping(r, m)) return set_err(ctx, B2F_ERR_ROUNDS, "%s: rounds %u", what, r);
      ctx->pm_pat[r] = std::move(m);
    }
    if (!ctx->pm_pool_off.count(r)) rebuild = true;
  }
  if (rebuild) {
    std::vector<uint32_t> pool;
    ctx->pm_pool_off.clear();
    for (auto& kv : ctx->pm_pat) {
      ctx->pm_pool_off[kv.first] = pool.size();
      pool.insert(pool.end(), kv.second.begin(), kv.second.end());
    }
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (ctx->d_pm_pool) HIPCHK(ctx, hipFree(ctx->d_pm_pool));
    ctx->d_pm_pool = nullptr;
    HIPCHK(ctx, hipMalloc(&ctx->d_pm_pool, 4 * pool.size()));
    HIPCHK(ctx, hipMemcpy(ctx->d_pm_pool, pool.data(), 4 * pool.size(), hipMemcpyHostToDevice));
  }
  return B2F_OK;
}
// The instance table (m u64) is staged in pinned host memory and uploaded asynchronously; the
// host waits only for the previous call's upload (so the staging can be rewritten), or for the
// whole stream when a device buffer grows. *it: the staging to fill before perm_upload.
int perm_stage(b2f_ctx* ctx, size_t m, uint64_t** it) {
  if (ctx->pm_inst_ev_live) {
    HIPCHK(ctx, hipEventSynchronize(ctx->pm_inst_ev));
    ctx->pm_inst_ev_live = false;
  }
  if (int rc = grow_pinned(ctx, (void**)&ctx->h_pm_inst, &ctx->h_pm_inst_cap, m, 8)) return rc;
  if (!ctx->pm_inst_ev) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->pm_inst_ev, hipEventDisableTiming));
  *it = ctx->h_pm_inst;
  return B2F_OK;
}
int perm_upload(b2f_ctx* ctx, size_t m, size_t need_scr, hipStream_t s) {
  if (m > ctx->pm_inst_cap || need_scr > ctx->pm_cap) {  // one wait for the two blocks
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (int rc = grow_device(ctx, (void**)&ctx->d_pm_inst, &ctx->pm_inst_cap, m, 8, s, true)) return rc;
    if (int rc = grow_device(ctx, &ctx->d_pm, &ctx->pm_cap, need_scr, 1, s, true)) return rc;
  }
  // stream-ordered after the previous call's kernels, which read the same device table
  HIPCHK(ctx, hipMemcpyAsync(ctx->d_pm_inst, ctx->h_pm_inst, 8 * m, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipEventRecord(ctx->pm_inst_ev, s));
  ctx->pm_inst_ev_live = true;
  return B2F_OK;
}
int perm_setup(b2f_ctx* ctx, const char* what, const uint64_t* h_offsets, size_t n, uint32_t k,
               uint32_t form, const uint64_t* const* elems, int n_elems, size_t need_scr,
               hipStream_t s, uint64_t* row0, uint64_t* used) {
  if (int rc = perm_check_fields(ctx, what, k, form, elems, n_elems)) return rc;
  *row0 = h_offsets[0];
  std::vector<uint32_t> need;
  if (int rc = perm_rounds(ctx, what, h_offsets, n, need)) return rc;
  *used = h_offsets[n] - *row0;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = perm_patterns(ctx, what, need, 0, n, s)) return rc;
  // n + 1 circuit start rows, then n pool offsets
  const size_t m = 2 * n + 1;
  uint64_t* it = nullptr;
  if (int rc = perm_stage(ctx, m, &it)) return rc;
  for (size_t i = 0; i <= n; i++) it[i] = h_offsets[i] - *row0;
  for (size_t i = 0; i < n; i++) it[n + 1 + i] = ctx->pm_pool_off[need[i]];
  return perm_upload(ctx, m, need_scr, s);
}
}  // namespace

extern "C" {

B2F_API int b2f_permutation_columns_dev(b2f_ctx* ctx, const uint32_t* d_advice, uint64_t total_rows,
                                        const uint64_t* h_offsets, size_t n, uint32_t k,
                                        uint64_t usable_rows, const uint64_t omega[4],
                                        const uint64_t delta[4], const uint64_t beta[4],
                                        const uint64_t gamma[4], uint32_t chunk_len, uint32_t form,
                                        uint64_t* d_sigma, uint64_t* d_z, uint64_t out_rows,
                                        void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  if (!d_advice || !h_offsets || !omega || !delta || !beta || !gamma || !d_z || n == 0)
    return set_err(ctx, B2F_ERR_ARG, "permutation: null buffer or no instances");
  if (chunk_len < 1 || chunk_len > PM_COLS)
    return set_err(ctx, B2F_ERR_ARG, "permutation: chunk_len %u not in [1, 8]", chunk_len);
  if (k < 10 || k > 30) return set_err(ctx, B2F_ERR_ARG, "permutation: k %u not in [10, 30]", k);
  if (((uintptr_t)d_z & 15) || ((uintptr_t)d_sigma & 15))
    return set_err(ctx, B2F_ERR_ARG, "permutation: outputs must be 16-byte aligned");
  const uint64_t n_rows = 1ull << k;
  if (h_offsets[n] > total_rows) return set_err(ctx, B2F_ERR_ROWS, "permutation: instances past total_rows");
  if (h_offsets[n] - h_offsets[0] > usable_rows || usable_rows >= n_rows)
    return set_err(ctx, B2F_ERR_ROWS, "permutation: need used rows %llu <= usable_rows %llu < 2^k",
                   (unsigned long long)(h_offsets[n] - h_offsets[0]), (unsigned long long)usable_rows);
  if (out_rows < usable_rows + 1 || (d_sigma && out_rows < n_rows))
    return set_err(ctx, B2F_ERR_ROWS, "permutation: out_rows too small");
  hipStream_t s = (hipStream_t)stream;
  const uint64_t* elems[4] = {omega, delta, beta, gamma};
  uint64_t row0 = 0, used = 0;
  if (int rc = perm_setup(ctx, "permutation", h_offsets, n, k, form, elems, 4,
                          perm_scratch_bytes(k, usable_rows, n, chunk_len), s, &row0, &used))
    return rc;
  if (int rc = ensure_side(ctx)) return rc;
  int tk = timed_begin(ctx, B2F_KERNEL_PERM, s);
  HIPCHK(ctx, launch_permutation(d_advice, total_rows, row0, ctx->d_pm_inst, n, ctx->d_pm_pool, k,
                                 usable_rows, omega, delta, beta, gamma, chunk_len, form, d_sigma,
                                 d_z, out_rows, ctx->d_pm, ctx->d_status + 2, ctx->s2, ctx->ev_fork,
                                 ctx->ev_join, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_permutation_columns_batch_dev(b2f_ctx* ctx, const uint32_t* d_advice, uint64_t total_rows,
                                              const uint64_t* h_offsets, size_t n,
                                              const uint64_t* h_circuit_first, uint32_t n_circuits,
                                              uint32_t k, uint64_t usable_rows, const uint64_t omega[4],
                                              const uint64_t delta[4], const uint64_t beta[4],
                                              const uint64_t gamma[4], uint32_t chunk_len, uint32_t form,
                                              uint64_t* d_z, uint64_t out_rows, void* stream) {
  const char* what = "permutation batch";
  if (!ctx) return B2F_ERR_ARG;
  if (!d_advice || !h_offsets || !h_circuit_first || !omega || !delta || !beta || !gamma || !d_z || n == 0)
    return set_err(ctx, B2F_ERR_ARG, "%s: null buffer or no instances", what);
  if (n_circuits == 0) return set_err(ctx, B2F_ERR_ARG, "%s: no circuits", what);
  if (n > 0xffffffffull) return set_err(ctx, B2F_ERR_ARG, "%s: more than 2^32 instances", what);
  for (uint32_t c = 0; c < n_circuits; c++)
    if (h_circuit_first[c + 1] <= h_circuit_first[c] || h_circuit_first[c + 1] > n)
      return set_err(ctx, B2F_ERR_ARG, "%s: circuit %u: instances [%llu, %llu) of %zu (boundaries must "
                     "increase strictly and end at or before n)", what, c,
                     (unsigned long long)h_circuit_first[c], (unsigned long long)h_circuit_first[c + 1], n);
  if (chunk_len < 1 || chunk_len > PM_COLS)
    return set_err(ctx, B2F_ERR_ARG, "%s: chunk_len %u not in [1, 8]", what, chunk_len);
  if ((uintptr_t)d_z & 15) return set_err(ctx, B2F_ERR_ARG, "%s: d_z must be 16-byte aligned", what);
  const uint64_t* elems[4] = {omega, delta, beta, gamma};
  if (int rc = perm_check_fields(ctx, what, k, form, elems, 4)) return rc;
  const uint64_t n_rows = 1ull << k;
  if (usable_rows >= n_rows)
    return set_err(ctx, B2F_ERR_ROWS, "%s: need usable_rows %llu < 2^k", what, (unsigned long long)usable_rows);
  if (out_rows < usable_rows + 1) return set_err(ctx, B2F_ERR_ROWS, "%s: out_rows < usable_rows + 1", what);
  std::vector<uint32_t> need;
  if (int rc = perm_rounds(ctx, what, h_offsets, n, need)) return rc;
  if (h_offsets[n] > total_rows) return set_err(ctx, B2F_ERR_ROWS, "%s: instances past total_rows", what);
  for (uint32_t c = 0; c < n_circuits; c++) {
    const uint64_t used = h_offsets[h_circuit_first[c + 1]] - h_offsets[h_circuit_first[c]];
    if (used > usable_rows)
      return set_err(ctx, B2F_ERR_ROWS, "%s: circuit %u uses %llu rows > usable_rows %llu", what, c,
                     (unsigned long long)used, (unsigned long long)usable_rows);
  }
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  const size_t i0 = h_circuit_first[0], i1 = h_circuit_first[n_circuits];
  if (int rc = perm_patterns(ctx, what, need, i0, i1, s)) return rc;
  // the table: one descriptor per circuit (table offset, instances, trace row 0, used rows),
  // then per circuit its n_c + 1 instance starts rebased to its row 0 and its n_c pool offsets
  const uint32_t dw = perm_circ_words();
  const size_t m = (size_t)dw * n_circuits + 2 * (i1 - i0) + n_circuits;
  uint64_t* it = nullptr;
  if (int rc = perm_stage(ctx, m, &it)) return rc;
  size_t at = (size_t)dw * n_circuits;
  for (uint32_t c = 0; c < n_circuits; c++) {
    const size_t a = h_circuit_first[c], b = h_circuit_first[c + 1], nc = b - a;
    const uint64_t row0 = h_offsets[a];
    it[(size_t)dw * c + 0] = at;
    it[(size_t)dw * c + 1] = nc;
    it[(size_t)dw * c + 2] = row0;
    it[(size_t)dw * c + 3] = h_offsets[b] - row0;
    for (size_t i = 0; i <= nc; i++) it[at + i] = h_offsets[a + i] - row0;
    for (size_t i = 0; i < nc; i++) it[at + nc + 1 + i] = ctx->pm_pool_off[need[a + i]];
    at += 2 * nc + 1;
  }
  // circuits per pass: the scratch holds one group's column sets, whatever n_circuits is
  const uint32_t group = perm_batch_group(usable_rows, n_circuits, chunk_len);
  if (int rc = perm_upload(ctx, m, perm_batch_scratch_bytes(k, usable_rows, group, chunk_len), s)) return rc;
  if (int rc = ensure_side(ctx)) return rc;
  int tk = timed_begin(ctx, B2F_KERNEL_PERM, s);
  HIPCHK(ctx, launch_permutation_batch(d_advice, total_rows, ctx->d_pm_inst, n_circuits, group,
                                       ctx->d_pm_pool, k, usable_rows, omega, delta, beta, gamma, chunk_len,
                                       form, d_z, out_rows, ctx->d_pm, ctx->d_status + 2, ctx->s2,
                                       ctx->ev_fork, ctx->ev_join, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_permutation_sigma_dev(b2f_ctx* ctx, const uint64_t* h_offsets, size_t n, uint32_t k,
                                      const uint64_t omega[4], const uint64_t delta[4], uint32_t form,
                                      uint64_t* d_sigma, uint64_t out_rows, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  if (!h_offsets || !omega || !delta || !d_sigma || n == 0)
    return set_err(ctx, B2F_ERR_ARG, "permutation sigma: null buffer or no instances");
  if ((uintptr_t)d_sigma & 15) return set_err(ctx, B2F_ERR_ARG, "permutation sigma: d_sigma must be 16-byte aligned");
  if (k < 10 || k > 30) return set_err(ctx, B2F_ERR_ARG, "permutation sigma: k %u not in [10, 30]", k);
  const uint64_t n_rows = 1ull << k;
  if (h_offsets[n] - h_offsets[0] >= n_rows)
    return set_err(ctx, B2F_ERR_ROWS, "permutation sigma: the instances need %llu rows >= 2^k",
                   (unsigned long long)(h_offsets[n] - h_offsets[0]));
  if (out_rows < n_rows) return set_err(ctx, B2F_ERR_ROWS, "permutation sigma: out_rows < 2^k");
  hipStream_t s = (hipStream_t)stream;
  const uint64_t* elems[2] = {omega, delta};
  uint64_t row0 = 0, used = 0;
  if (int rc = perm_setup(ctx, "permutation sigma", h_offsets, n, k, form, elems, 2, perm_sigma_scratch_bytes(k),
                          s, &row0, &used))
    return rc;
  int tk = timed_begin(ctx, B2F_KERNEL_PERM_SIGMA, s);
  HIPCHK(ctx, launch_permutation_sigma(ctx->d_pm_inst, n, ctx->d_pm_pool, k, omega, delta, form, d_sigma,
                                       out_rows, ctx->d_pm, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

}  // extern "C"

namespace {
bool fe_is_zero(const uint64_t* v) { return !(v[0] | v[1] | v[2] | v[3]); }

// [a, a + an) and [b, b + bn) share a byte
bool ranges_overlap(const void* a, uint64_t an, const void* b, uint64_t bn) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + bn && b0 < a0 + an;
}

// The checks the term calls and the divide share; `what` names the call in messages.
int quot_check_common(b2f_ctx* ctx, const char* what, uint32_t k, uint32_t ext_k, uint64_t rows, uint32_t form,
                      const uint64_t* d_h_in, const uint64_t* d_h_out) {
  if (!d_h_out) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (((uintptr_t)d_h_in | (uintptr_t)d_h_out) & 15)
    return set_err(ctx, B2F_ERR_ARG, "%s: buffers must be 16-byte aligned", what);
  if (k < 1 || ext_k > 28 || k >= ext_k)
    return set_err(ctx, B2F_ERR_ARG, "%s: need 1 <= k < ext_k <= 28, got k %u, ext_k %u", what, k, ext_k);
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "%s: unknown form %u", what, form);
  if (rows < (1ull << ext_k)) return set_err(ctx, B2F_ERR_ROWS, "%s: rows < 2^ext_k", what);
  if (rows > (1ull << 52)) return set_err(ctx, B2F_ERR_ARG, "%s: column stride overflows the address space", what);
  const uint64_t hb = 32ull << ext_k;
  if (d_h_in && d_h_in != d_h_out && ranges_overlap(d_h_in, hb, d_h_out, hb))
    return set_err(ctx, B2F_ERR_ARG, "%s: h_in and h_out overlap without being equal", what);
  return B2F_OK;
}

// The cached block of the domain (field of form, a, b, omega, shift) among the n_tabs of `tabs`,
// or nullptr with *slot = the entry to fill: the next in turn, its buffer grown to `need` bytes,
// not yet live.
int domain_tab_find(b2f_ctx* ctx, b2f_domain_tab* tabs, int n_tabs, uint32_t* next, uint32_t form, uint32_t a,
                    uint32_t b, const uint64_t* omega, const uint64_t* shift, size_t need, hipStream_t s,
                    b2f_domain_tab** found, b2f_domain_tab** slot) {
  *found = *slot = nullptr;
  for (int i = 0; i < n_tabs; i++) {
    b2f_domain_tab& t = tabs[i];
    if (t.live && t.field == (form >> 1) && t.a == a && t.b == b && !memcmp(t.omega, omega, 32) &&
        !memcmp(t.shift, shift, 32))
      *found = &t;
  }
  if (*found) return B2F_OK;
  b2f_domain_tab& t = tabs[(*next)++ % n_tabs];
  t.live = false;
  if (int rc = grow_device(ctx, &t.d, &t.cap, need, 1, s)) return rc;
  t.field = form >> 1;
  t.a = a;
  t.b = b;
  memcpy(t.omega, omega, 32);
  memcpy(t.shift, shift, 32);
  *slot = &t;
  return B2F_OK;
}

// the per-call constant block of the term calls
int quot_consts(b2f_ctx* ctx) {
  if (!ctx->d_quot_consts) HIPCHK(ctx, hipMalloc(&ctx->d_quot_consts, quot_consts_bytes()));
  return B2F_OK;
}

// The host part the evaluation / opening calls share: stage the plan's image in pinned memory,
// grow the device blocks if needed and upload the image on the stream. The host waits only for the
// previous call's upload (so the staging can be rewritten), or for the whole stream when a device
// block has to grow.
int open_upload(b2f_ctx* ctx, const OpenPlan& p, hipStream_t s) {
  const size_t words = p.blob.size() + 2, scratch = p.scratch_bytes + 256;
  if (ctx->op_ev_live) {
    HIPCHK(ctx, hipEventSynchronize(ctx->op_ev));
    ctx->op_ev_live = false;
  }
  if (!ctx->op_ev) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->op_ev, hipEventDisableTiming));
  if (int rc = grow_pinned(ctx, (void**)&ctx->h_op, &ctx->h_op_cap, words, 8)) return rc;
  if (words > ctx->op_blob_cap || scratch > ctx->op_cap) {  // one wait for the two blocks
    HIPCHK(ctx, hipStreamSynchronize(s));
    if (int rc = grow_device(ctx, &ctx->d_op_blob, &ctx->op_blob_cap, words, 8, s, true)) return rc;
    if (int rc = grow_device(ctx, &ctx->d_op, &ctx->op_cap, scratch, 1, s, true)) return rc;
  }
  memcpy(ctx->h_op, p.blob.data(), 8 * p.blob.size());
  HIPCHK(ctx, hipMemcpyAsync(ctx->d_op_blob, ctx->h_op, 8 * p.blob.size(), hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipEventRecord(ctx->op_ev, s));
  ctx->op_ev_live = true;
  return B2F_OK;
}

// The argument checks the three calls share: the column block and its sizes.
int open_check_cols(b2f_ctx* ctx, const char* what, const uint64_t* d_cols, uint64_t rows, uint64_t len,
                    uint32_t n_cols, uint32_t form, const uint64_t* d_out) {
  if (!d_cols || !d_out) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (((uintptr_t)d_cols | (uintptr_t)d_out) & 15)
    return set_err(ctx, B2F_ERR_ARG, "%s: buffers must be 16-byte aligned", what);
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "%s: unknown form %u", what, form);
  if (len == 0 || n_cols == 0) return set_err(ctx, B2F_ERR_ARG, "%s: no columns or no coefficients", what);
  if (len > rows) return set_err(ctx, B2F_ERR_ROWS, "%s: len %llu > rows", what, (unsigned long long)len);
  if (rows > (1ull << 58) / n_cols) return set_err(ctx, B2F_ERR_ARG, "%s: column stride overflows the address space", what);
  return B2F_OK;
}

#ifdef B2F_DIAG
// Diagnostics build only: B2F_DIAG_NTT_PLAN=l1,l2[,l3[,l4]] read at the call replaces the pass plan
// of b2f_ntt_columns_dev (tests/test_gpu_ntt_plans.py: plans the product never picks at small k).
// Returns 0 when the variable is unset (the product plan), 1 with plan = {P, l[0..3]} when it
// holds a plan the pass kernel can run at this k (k > 10, 2..4 digits, each 1..8, summing to k:
// every tile then holds 2^(10 - l) >= 4 whole transforms and every row index stays below 2^k),
// -1 for anything else. There is no fallback: the caller refuses the call on -1.
int diag_ntt_plan(uint32_t k, uint32_t* plan) {
  const char* v = getenv("B2F_DIAG_NTT_PLAN");
  if (!v) return 0;
  uint32_t P = 0, sum = 0;
  for (uint32_t d = 0; d < 5; d++) plan[d] = 0;
  for (const char* c = v;;) {
    if (P == 4 || *c < '1' || *c > '8') return -1;  // one decimal digit per pass
    plan[1 + P] = (uint32_t)(*c - '0');
    sum += plan[1 + P];
    P++;
    c++;
    if (!*c) break;
    if (*c != ',') return -1;
    c++;
  }
  if (k <= 10 || P < 2 || sum != k) return -1;
  plan[0] = P;
  return 1;
}
#endif
}  // namespace

extern "C" {

#ifdef B2F_DIAG
// Host only: the pass plan b2f_ntt_columns_dev would run a 2^k transform with under the current
// environment, out = {P, l[0..3]}; B2F_ERR_ARG where it would refuse the call.
B2F_API int b2f_debug_ntt_plan(uint32_t k, uint32_t* out) {
  if (!out || k < 1 || k > 28) return B2F_ERR_ARG;
  const int forced = diag_ntt_plan(k, out);
  if (forced < 0) return B2F_ERR_ARG;
  if (!forced) ntt_plan_of(k, out);
  return B2F_OK;
}
#endif

B2F_API int b2f_lagrange_selectors_dev(b2f_ctx* ctx, uint32_t k, uint64_t usable_rows, uint32_t form,
                                       uint64_t* d_out, uint64_t out_rows, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  if (!d_out) return set_err(ctx, B2F_ERR_ARG, "selectors: null buffer");
  if ((uintptr_t)d_out & 15) return set_err(ctx, B2F_ERR_ARG, "selectors: d_out must be 16-byte aligned");
  if (k < 1 || k > 28) return set_err(ctx, B2F_ERR_ARG, "selectors: k %u not in [1, 28]", k);
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "selectors: unknown form %u", form);
  if (usable_rows >= (1ull << k))
    return set_err(ctx, B2F_ERR_ROWS, "selectors: usable_rows %llu >= 2^k", (unsigned long long)usable_rows);
  if (out_rows < (1ull << k)) return set_err(ctx, B2F_ERR_ROWS, "selectors: out_rows < 2^k");
  if (out_rows > (1ull << 52)) return set_err(ctx, B2F_ERR_ARG, "selectors: column stride overflows the address space");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_lagrange_selectors(k, (uint32_t)usable_rows, form, d_out, out_rows, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_quotient_gates_dev(b2f_ctx* ctx, uint32_t k, uint32_t ext_k, const uint64_t* d_advice,
                                   const uint64_t* d_fixed, uint64_t rows, const uint64_t y[4],
                                   const uint64_t* d_h_in, uint64_t* d_h_out, uint32_t form, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "quotient gates";
  if (!d_advice || !d_fixed || !y) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (((uintptr_t)d_advice | (uintptr_t)d_fixed) & 15)
    return set_err(ctx, B2F_ERR_ARG, "%s: buffers must be 16-byte aligned", what);
  if (int rc = quot_check_common(ctx, what, k, ext_k, rows, form, d_h_in, d_h_out)) return rc;
  if (!fe_canonical(form, y)) return set_err(ctx, B2F_ERR_ARG, "%s: y is >= p", what);
  const uint64_t hb = 32ull << ext_k;
  if (ranges_overlap(d_h_out, hb, d_advice, B2F_NUM_ADVICE * rows * 32) ||
      ranges_overlap(d_h_out, hb, d_fixed, B2F_NUM_FIXED_FP * rows * 32))
    return set_err(ctx, B2F_ERR_ARG, "%s: h_out overlaps an input block", what);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = quot_consts(ctx)) return rc;
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_quot_gates(k, ext_k, d_advice, d_fixed, rows, y, d_h_in, d_h_out, form,
                                ctx->d_quot_consts, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_quotient_permutation_dev(b2f_ctx* ctx, uint32_t k, uint32_t ext_k, uint64_t usable_rows,
                                         const uint64_t* d_l, const uint64_t* d_advice,
                                         const uint64_t* d_sigma, const uint64_t* d_z, uint32_t chunk_len,
                                         uint64_t rows, const uint64_t omega_ext[4], const uint64_t shift[4],
                                         const uint64_t delta[4], const uint64_t beta[4],
                                         const uint64_t gamma[4], const uint64_t y[4],
                                         const uint64_t* d_h_in, uint64_t* d_h_out, uint32_t form,
                                         void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "quotient permutation";
  if (!d_l || !d_advice || !d_sigma || !d_z || !omega_ext || !shift || !delta || !beta || !gamma || !y)
    return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (((uintptr_t)d_l | (uintptr_t)d_advice | (uintptr_t)d_sigma | (uintptr_t)d_z) & 15)
    return set_err(ctx, B2F_ERR_ARG, "%s: buffers must be 16-byte aligned", what);
  if (int rc = quot_check_common(ctx, what, k, ext_k, rows, form, d_h_in, d_h_out)) return rc;
  if (chunk_len < 1 || chunk_len > 8) return set_err(ctx, B2F_ERR_ARG, "%s: chunk_len %u not in [1, 8]", what, chunk_len);
  const uint64_t* elems[6] = {omega_ext, shift, delta, beta, gamma, y};
  for (const uint64_t* e : elems)
    if (!fe_canonical(form, e)) return set_err(ctx, B2F_ERR_ARG, "%s: a challenge, omega, shift or delta is >= p", what);
  if (fe_is_zero(shift)) return set_err(ctx, B2F_ERR_ARG, "%s: shift is zero", what);
  if (usable_rows >= (1ull << k))
    return set_err(ctx, B2F_ERR_ROWS, "%s: usable_rows %llu >= 2^k", what, (unsigned long long)usable_rows);
  const uint32_t sets = (8 + chunk_len - 1) / chunk_len;
  const uint64_t hb = 32ull << ext_k;
  if (ranges_overlap(d_h_out, hb, d_l, 3 * rows * 32) || ranges_overlap(d_h_out, hb, d_advice, 10 * rows * 32) ||
      ranges_overlap(d_h_out, hb, d_sigma, 8 * rows * 32) || ranges_overlap(d_h_out, hb, d_z, sets * rows * 32))
    return set_err(ctx, B2F_ERR_ARG, "%s: h_out overlaps an input block", what);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = quot_consts(ctx)) return rc;
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  b2f_domain_tab *tab, *slot;
  if (int rc = domain_tab_find(ctx, ctx->quot_tab, b2f_ctx::QUOT_TABS, &ctx->quot_next, form, 0, ext_k, omega_ext,
                               shift, quot_xtab_bytes(ext_k), s, &tab, &slot))
    return rc;
  if (!tab) {
    HIPCHK(ctx, launch_quot_xtab(slot->d, form, ext_k, omega_ext, shift, s));
    slot->live = true;
    tab = slot;
  }
  uint32_t colmap = 0;  // v_j = the advice column of a_{j+1}
  for (int j = 0; j < 8; j++) colmap |= (uint32_t)b2f_halo2_column_index(j + 1) << (4 * j);
  HIPCHK(ctx, launch_quot_permutation(k, ext_k, (uint32_t)usable_rows, d_l, d_advice, d_sigma, d_z, chunk_len,
                                      rows, delta, beta, gamma, y, d_h_in, d_h_out, form, colmap, tab->d,
                                      ctx->d_quot_consts, ctx->d_status + 2, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_quotient_lookup_dev(b2f_ctx* ctx, uint32_t k, uint32_t ext_k, const uint64_t* d_l,
                                    const uint64_t* d_lookup, uint64_t rows, const uint64_t beta[4],
                                    const uint64_t gamma[4], const uint64_t y[4], const uint64_t* d_h_in,
                                    uint64_t* d_h_out, uint32_t form, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "quotient lookup";
  if (!d_l || !d_lookup || !beta || !gamma || !y) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (((uintptr_t)d_l | (uintptr_t)d_lookup) & 15)
    return set_err(ctx, B2F_ERR_ARG, "%s: buffers must be 16-byte aligned", what);
  if (int rc = quot_check_common(ctx, what, k, ext_k, rows, form, d_h_in, d_h_out)) return rc;
  if (!fe_canonical(form, beta) || !fe_canonical(form, gamma) || !fe_canonical(form, y))
    return set_err(ctx, B2F_ERR_ARG, "%s: a challenge is >= p", what);
  const uint64_t hb = 32ull << ext_k;
  if (ranges_overlap(d_h_out, hb, d_l, 3 * rows * 32) || ranges_overlap(d_h_out, hb, d_lookup, 5 * rows * 32))
    return set_err(ctx, B2F_ERR_ARG, "%s: h_out overlaps an input block", what);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = quot_consts(ctx)) return rc;
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_quot_lookup(k, ext_k, d_l, d_lookup, rows, beta, gamma, y, d_h_in, d_h_out, form,
                                 ctx->d_quot_consts, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_quotient_divide_dev(b2f_ctx* ctx, uint32_t k, uint32_t ext_k, const uint64_t omega_ext[4],
                                    const uint64_t shift[4], const uint64_t* d_h_in, uint64_t* d_h_out,
                                    uint32_t form, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "quotient divide";
  if (!d_h_in || !omega_ext || !shift) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  const uint64_t n_ext = ext_k <= 28 ? 1ull << ext_k : 0;  // an ext_k out of range: the check reports it
  if (int rc = quot_check_common(ctx, what, k, ext_k, n_ext, form, d_h_in, d_h_out)) return rc;
  if (!fe_canonical(form, omega_ext) || !fe_canonical(form, shift))
    return set_err(ctx, B2F_ERR_ARG, "%s: omega or shift is >= p", what);
  if (fe_is_zero(shift)) return set_err(ctx, B2F_ERR_ARG, "%s: shift is zero", what);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  b2f_domain_tab *tab, *slot;
  if (int rc = domain_tab_find(ctx, ctx->quot_div, b2f_ctx::QUOT_TABS, &ctx->quot_div_next, form, k, ext_k,
                               omega_ext, shift, quot_divisor_bytes(k, ext_k), s, &tab, &slot))
    return rc;
  if (!tab) {
    HIPCHK(ctx, launch_quot_divisors(slot->d, form, k, ext_k, omega_ext, shift, s));
    slot->live = true;
    tab = slot;
  }
  HIPCHK(ctx, launch_quot_divide(k, ext_k, d_h_in, d_h_out, form, tab->d, ctx->d_status + 2, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_poly_eval_dev(b2f_ctx* ctx, const uint64_t* d_cols, uint64_t rows, uint64_t len, uint32_t n_cols,
                              const uint64_t* h_points, uint32_t n_points, const uint32_t* h_queries,
                              uint64_t n_queries, uint32_t form, uint64_t* d_out, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "poly eval";
  if (!h_points || !h_queries) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (int rc = open_check_cols(ctx, what, d_cols, rows, len, n_cols, form, d_out)) return rc;
  if (n_points == 0 || n_queries == 0) return set_err(ctx, B2F_ERR_ARG, "%s: no points or no queries", what);
  OpenPlan plan;
  char msg[160];
  if (int rc = open_plan_eval(plan, len, n_cols, h_points, n_points, h_queries, n_queries, form, msg, sizeof msg))
    return set_err(ctx, rc, "%s: %s", what, msg);
  if (ranges_overlap(d_out, 32 * n_queries, d_cols, (uint64_t)n_cols * rows * 32))
    return set_err(ctx, B2F_ERR_ARG, "%s: the output overlaps the columns", what);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = open_upload(ctx, plan, s)) return rc;
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_poly_eval(plan, d_cols, rows, ctx->d_op_blob, ctx->d_op, d_out, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_poly_combine_dev(b2f_ctx* ctx, const uint64_t* d_cols, uint64_t rows, uint64_t len,
                                 uint32_t n_cols, const uint32_t* h_first, const uint32_t* h_col,
                                 const uint64_t* h_scalar, uint32_t n_out, uint32_t form, uint64_t* d_out,
                                 uint64_t out_rows, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "poly combine";
  if (!h_first) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (int rc = open_check_cols(ctx, what, d_cols, rows, len, n_cols, form, d_out)) return rc;
  if (n_out == 0) return set_err(ctx, B2F_ERR_ARG, "%s: no outputs", what);
  if (out_rows < len) return set_err(ctx, B2F_ERR_ROWS, "%s: out_rows < len", what);
  if (out_rows > (1ull << 58) / n_out) return set_err(ctx, B2F_ERR_ARG, "%s: column stride overflows the address space", what);
  if (h_first[n_out] && (!h_col || !h_scalar)) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  OpenPlan plan;
  char msg[160];
  if (int rc = open_plan_combine(plan, len, n_cols, h_first, h_col, h_scalar, n_out, form, msg, sizeof msg))
    return set_err(ctx, rc, "%s: %s", what, msg);
  if (ranges_overlap(d_out, (uint64_t)n_out * out_rows * 32, d_cols, (uint64_t)n_cols * rows * 32))
    return set_err(ctx, B2F_ERR_ARG, "%s: the output overlaps the columns", what);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = open_upload(ctx, plan, s)) return rc;
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_poly_combine(plan, d_cols, rows, ctx->d_op_blob, ctx->d_op, d_out, out_rows, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_kate_divide_dev(b2f_ctx* ctx, const uint64_t* d_cols, uint64_t rows, uint64_t len,
                                uint32_t n_cols, const uint32_t* h_first, const uint64_t* h_points,
                                uint32_t form, uint64_t* d_out, uint64_t out_rows, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "kate divide";
  if (!h_first) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (int rc = open_check_cols(ctx, what, d_cols, rows, len, n_cols, form, d_out)) return rc;
  if (out_rows < len) return set_err(ctx, B2F_ERR_ROWS, "%s: out_rows < len", what);
  if (out_rows > (1ull << 58) / n_cols) return set_err(ctx, B2F_ERR_ARG, "%s: column stride overflows the address space", what);
  if (h_first[n_cols] && !h_points) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  OpenPlan plan;
  char msg[160];
  if (int rc = open_plan_kate(plan, len, n_cols, h_first, h_points, form, msg, sizeof msg))
    return set_err(ctx, rc, "%s: %s", what, msg);
  if (ranges_overlap(d_out, (uint64_t)n_cols * out_rows * 32, d_cols, (uint64_t)n_cols * rows * 32))
    return set_err(ctx, B2F_ERR_ARG, "%s: the output overlaps the columns", what);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = open_upload(ctx, plan, s)) return rc;
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_kate_divide(plan, d_cols, rows, ctx->d_op_blob, ctx->d_op, d_out, out_rows, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

}  // extern "C"

namespace {
// The plan of a commitment call: the product's, or under the diagnostics library the one
// B2F_DIAG_MSM_PLAN forces. false: the arguments (or the forced plan) are refused.
bool msm_plan_for(uint64_t len, uint32_t n_cols, uint32_t form, MsmPlan* plan) {
  if (form > B2F_FP_BN254_MONTGOMERY) return false;
  uint32_t fc = 0, fg = 0;
#ifdef B2F_DIAG
  if (diag_msm_plan(&fc, &fg) < 0) return false;
#endif
  return msm_plan_of(len, n_cols, fc, fg, plan);
}
}  // namespace

extern "C" {

B2F_API int b2f_msm_plan(uint64_t len, uint32_t n_cols, uint32_t form, uint32_t* window_bits,
                         uint32_t* windows, uint32_t* group, uint64_t* scratch_bytes) {
  MsmPlan plan;
  if (!msm_plan_for(len, n_cols, form, &plan)) return B2F_ERR_ARG;
  if (window_bits) *window_bits = plan.c;
  if (windows) *windows = plan.windows;
  if (group) *group = plan.group;
  if (scratch_bytes) *scratch_bytes = plan.scratch_bytes;
  return B2F_OK;
}

B2F_API int b2f_msm_dev(b2f_ctx* ctx, const uint64_t* d_scalars, uint64_t rows, uint64_t len,
                        uint32_t n_cols, const uint64_t* d_bases, uint64_t n_bases, uint32_t form,
                        uint64_t* d_out, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "msm";
  if (!d_scalars || !d_bases || !d_out) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (((uintptr_t)d_scalars | (uintptr_t)d_bases | (uintptr_t)d_out) & 15)
    return set_err(ctx, B2F_ERR_ARG, "%s: buffers must be 16-byte aligned", what);
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "%s: unknown form %u", what, form);
  if (len == 0 || n_cols == 0) return set_err(ctx, B2F_ERR_ARG, "%s: no columns or no scalars", what);
  if (len > (1ull << 28)) return set_err(ctx, B2F_ERR_ARG, "%s: len %llu > 2^28", what, (unsigned long long)len);
  if (len > rows) return set_err(ctx, B2F_ERR_ROWS, "%s: len %llu > rows", what, (unsigned long long)len);
  if (len > n_bases) return set_err(ctx, B2F_ERR_ROWS, "%s: len %llu > n_bases", what, (unsigned long long)len);
  if (rows > (1ull << 58) / n_cols || n_bases > (1ull << 57))
    return set_err(ctx, B2F_ERR_ARG, "%s: column stride overflows the address space", what);
  if (ranges_overlap(d_out, 64ull * n_cols, d_scalars, (uint64_t)n_cols * rows * 32) ||
      ranges_overlap(d_out, 64ull * n_cols, d_bases, n_bases * 64))
    return set_err(ctx, B2F_ERR_ARG, "%s: the output overlaps an input", what);
  MsmPlan plan;
  if (!msm_plan_for(len, n_cols, form, &plan))
    return set_err(ctx, B2F_ERR_ARG, "%s: no plan (a forced plan that is malformed or exceeds a pass)", what);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = grow_device(ctx, &ctx->d_msm, &ctx->msm_cap, plan.scratch_bytes, 1, s)) return rc;
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_msm(plan, d_scalars, rows, len, n_cols, d_bases, form, d_out, ctx->d_msm, ctx->d_status + 2, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

}  // extern "C"

namespace {
// The plan of a cell commitment: B2F_OK, or the code the call refuses its counts, descriptors or
// (diagnostics library) forced plan with.
int msm_cells_plan_for(const void* h_cols, uint32_t n_cols, uint64_t len, uint64_t tail_rows, uint32_t form,
                       CellsPlan* plan) {
  if (!h_cols || form > B2F_FP_BN254_MONTGOMERY || tail_rows > 64) return B2F_ERR_ARG;
  uint32_t fc = 0, fg = 0;
#ifdef B2F_DIAG
  if (diag_msm_plan(&fc, &fg) < 0) return B2F_ERR_ARG;
#endif
  return msm_cells_plan_of(static_cast<const b2f_cell_column*>(h_cols), n_cols, len, fc, fg, plan) ? B2F_OK
                                                                                                    : B2F_ERR_ARG;
}

uint32_t cell_columns(uint64_t total_rows, uint64_t row_begin, uint64_t usable_rows, void* out, uint32_t n,
                      bool advice) {
  if (!out || total_rows % 4 != 0 || usable_rows == 0) return 0;
  const uint64_t left = row_begin >= total_rows ? 0 : total_rows - row_begin;
  b2f_cell_column* cols = static_cast<b2f_cell_column*>(out);
  for (uint32_t i = 0; i < n; i++) {
    b2f_cell_column& d = cols[advice ? (uint32_t)b2f_halo2_column_index((int)i) : i];
    d.offset = (advice ? i * total_rows : 0) + row_begin;
    d.avail = usable_rows < left ? usable_rows : left;
    d.shift = advice ? 0 : i;
    d.bits = advice ? 32 : i < 16 ? 1 : 16;
  }
  return n;
}
}  // namespace

extern "C" {

B2F_API uint32_t b2f_advice_cell_columns(uint64_t total_rows, uint64_t row_begin, uint64_t usable_rows,
                                         void* out10) {
  return cell_columns(total_rows, row_begin, usable_rows, out10, B2F_NUM_ADVICE, true);
}

B2F_API uint32_t b2f_fixed_cell_columns(uint64_t total_rows, uint64_t row_begin, uint64_t usable_rows,
                                        void* out17) {
  return cell_columns(total_rows, row_begin, usable_rows, out17, B2F_NUM_FIXED_FP, false);
}

B2F_API int b2f_msm_cells_plan(const void* h_cols, uint32_t n_cols, uint64_t len, uint64_t tail_rows,
                               uint32_t form, uint32_t* window_bits, uint64_t* digits, uint64_t* scratch_bytes) {
  CellsPlan plan;
  if (int rc = msm_cells_plan_for(h_cols, n_cols, len, tail_rows, form, &plan)) return rc;
  if (window_bits) *window_bits = plan.c;
  if (digits) *digits = plan.digits;
  if (scratch_bytes) *scratch_bytes = plan.scratch_bytes;
  return B2F_OK;
}

B2F_API int b2f_msm_cells_dev(b2f_ctx* ctx, const uint32_t* d_cells, uint64_t n_cells, const void* h_cols,
                              uint32_t n_cols, uint64_t len, const uint64_t* d_tail, uint64_t tail_rows,
                              const uint64_t* d_bases, uint64_t n_bases, uint32_t form, uint64_t* d_out,
                              void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "msm cells";
  if (!d_cells || !h_cols || !d_bases || !d_out) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (((uintptr_t)d_cells | (uintptr_t)d_bases | (uintptr_t)d_out | (uintptr_t)d_tail) & 15)
    return set_err(ctx, B2F_ERR_ARG, "%s: buffers must be 16-byte aligned", what);
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "%s: unknown form %u", what, form);
  if (len == 0 || len > (1ull << 28))
    return set_err(ctx, B2F_ERR_ARG, "%s: len %llu not in [1, 2^28]", what, (unsigned long long)len);
  if (n_cols == 0 || n_cols > 4096) return set_err(ctx, B2F_ERR_ARG, "%s: n_cols %u not in [1, 4096]", what, n_cols);
  if (tail_rows > 64) return set_err(ctx, B2F_ERR_ARG, "%s: tail_rows %llu > 64", what, (unsigned long long)tail_rows);
  if ((d_tail != nullptr) != (tail_rows != 0))
    return set_err(ctx, B2F_ERR_ARG, "%s: d_tail and tail_rows must be given together", what);
  if (n_cells > (1ull << 60) || n_bases > (1ull << 57))
    return set_err(ctx, B2F_ERR_ARG, "%s: a block overflows the address space", what);
  CellsPlan plan;
  if (msm_cells_plan_for(h_cols, n_cols, len, tail_rows, form, &plan) != B2F_OK)
    return set_err(ctx, B2F_ERR_ARG, "%s: a column's shift / bits out of range (bits 1..32, shift + bits <= 32), or a "
                   "forced plan that is malformed or exceeds a pass", what);
  const b2f_cell_column* cols = static_cast<const b2f_cell_column*>(h_cols);
  for (uint32_t i = 0; i < n_cols; i++)
    if (cols[i].offset > n_cells || plan.image[i].avail > n_cells - cols[i].offset)
      return set_err(ctx, B2F_ERR_ROWS, "%s: column %u reads cells [%llu, +%u) of %llu", what, i,
                     (unsigned long long)cols[i].offset, plan.image[i].avail, (unsigned long long)n_cells);
  if (len + tail_rows > n_bases)
    return set_err(ctx, B2F_ERR_ROWS, "%s: len + tail_rows %llu > n_bases", what, (unsigned long long)(len + tail_rows));
  if (ranges_overlap(d_out, 64ull * n_cols, d_cells, 4 * n_cells) ||
      ranges_overlap(d_out, 64ull * n_cols, d_bases, n_bases * 64) ||
      (d_tail && ranges_overlap(d_out, 64ull * n_cols, d_tail, 32ull * n_cols * tail_rows)))
    return set_err(ctx, B2F_ERR_ARG, "%s: the output overlaps an input", what);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (tail_rows)
    if (int rc = ensure_side(ctx)) return rc;
  // the descriptors: staged in pinned memory (rewritten once the previous call's upload is done),
  // uploaded on the stream into the scratch, so h_cols is the caller's again when the call returns
  const size_t image_bytes = sizeof(CellColumn) * (size_t)n_cols;
  if (ctx->cells_ev_live) {
    HIPCHK(ctx, hipEventSynchronize(ctx->cells_ev));
    ctx->cells_ev_live = false;
  }
  if (!ctx->cells_ev) HIPCHK(ctx, hipEventCreateWithFlags(&ctx->cells_ev, hipEventDisableTiming));
  if (int rc = grow_pinned(ctx, &ctx->h_cells, &ctx->h_cells_cap, image_bytes, 1)) return rc;
  if (int rc = grow_device(ctx, &ctx->d_msm, &ctx->msm_cap, plan.scratch_bytes, 1, s)) return rc;
  memcpy(ctx->h_cells, plan.image.data(), image_bytes);
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, hipMemcpyAsync((char*)ctx->d_msm + plan.off_desc, ctx->h_cells, image_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(ctx, hipEventRecord(ctx->cells_ev, s));
  ctx->cells_ev_live = true;
  hipStream_t s2 = ctx->s2;
#ifdef B2F_DIAG
  // B2F_DIAG_MSM_TAIL=serial: the tail on the call's own stream (tools/bench_msm_cells.py --tail)
  const char* tail_mode = getenv("B2F_DIAG_MSM_TAIL");
  if (tail_mode && !strcmp(tail_mode, "serial")) s2 = s;
#endif
  HIPCHK(ctx, launch_msm_cells(plan, d_cells, n_cols, len, d_tail, (uint32_t)tail_rows, d_bases, form, d_out,
                               ctx->d_msm, ctx->d_status + 2, s2, ctx->ev_fork, ctx->ev_join, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

}  // extern "C"

namespace {
// Host field helpers of the IPA fold: x R mod p of a canonical x (256 doublings mod p: p < 2^255,
// so 2x never leaves four limbs) and x^-1 mod p by the divsteps of b2f_safegcd.h.
void host_to_mont(uint32_t form, const uint64_t* x, uint64_t* out) {
  field::with_field(form, [&](auto f) {
    using F = decltype(f);
    uint64_t p[4], v[4];
    for (int i = 0; i < 4; i++) {
      p[i] = ((uint64_t)F::P[2 * i + 1] << 32) | F::P[2 * i];
      v[i] = x[i];
    }
    for (int step = 0; step < 256; step++) {
      for (int i = 3; i > 0; i--) v[i] = (v[i] << 1) | (v[i - 1] >> 63);
      v[0] <<= 1;
      bool ge = true;
      for (int i = 3; i >= 0; i--)
        if (v[i] != p[i]) {
          ge = v[i] > p[i];
          break;
        }
      if (ge) {
        uint64_t br = 0;
        for (int i = 0; i < 4; i++) {
          const unsigned __int128 d = (unsigned __int128)v[i] - p[i] - br;
          v[i] = (uint64_t)d;
          br = (uint64_t)(d >> 64) & 1;
        }
      }
    }
    for (int i = 0; i < 4; i++) out[i] = v[i];
    return 0;
  });
}
bool host_inverse(uint32_t form, const uint64_t* x, uint64_t* out) {
  return field::with_field(form, [&](auto f) {
    using F = decltype(f);
    uint32_t xw[8], pw[8], ow[8];
    for (int i = 0; i < 8; i++) {
      xw[i] = (uint32_t)(x[i >> 1] >> (32 * (i & 1)));
      pw[i] = F::P[i];
    }
    const bool ok = sgcd::inverse(xw, pw, ow);
    for (int i = 0; i < 4; i++) out[i] = ((uint64_t)ow[2 * i + 1] << 32) | ow[2 * i];
    return ok;
  });
}

// The longest round the direct kernel takes: the plan constant, or under the diagnostics library
// what B2F_DIAG_IPA_DIRECT forces. false: the forced value is malformed.
bool ipa_direct_for(uint64_t* max_len) {
  *max_len = ipa_direct_max_len();
#ifdef B2F_DIAG
  uint64_t forced = 0;
  const int have = diag_ipa_direct(&forced);
  if (have < 0) return false;
  if (have) *max_len = forced;
#endif
  return true;
}

// what the round and fold calls check alike
int ipa_check_vectors(b2f_ctx* ctx, const char* what, const uint64_t* d_p, const uint64_t* d_b, const uint64_t* d_g,
                      uint64_t len, uint32_t form) {
  if (!d_p || !d_b || !d_g) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (((uintptr_t)d_p | (uintptr_t)d_b | (uintptr_t)d_g) & 15)
    return set_err(ctx, B2F_ERR_ARG, "%s: buffers must be 16-byte aligned", what);
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "%s: unknown form %u", what, form);
  if (len < 2 || len > (1ull << 28) || (len & (len - 1)))
    return set_err(ctx, B2F_ERR_ARG, "%s: len %llu is not a power of two in [2, 2^28]", what, (unsigned long long)len);
  if (ranges_overlap(d_p, 32 * len, d_b, 32 * len) || ranges_overlap(d_p, 32 * len, d_g, 64 * len) ||
      ranges_overlap(d_b, 32 * len, d_g, 64 * len))
    return set_err(ctx, B2F_ERR_ARG, "%s: the three vectors overlap", what);
  return B2F_OK;
}
}  // namespace

extern "C" {

B2F_API uint64_t b2f_ipa_direct_max_len(void) {
  uint64_t m = 0;
  if (!ipa_direct_for(&m)) return ipa_direct_max_len();
  return m;
}

B2F_API int b2f_ipa_powers_dev(b2f_ctx* ctx, const uint64_t h_x[4], uint64_t len, uint32_t form, uint64_t* d_b,
                               void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "ipa powers";
  if (!h_x || !d_b) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if ((uintptr_t)d_b & 15) return set_err(ctx, B2F_ERR_ARG, "%s: d_b must be 16-byte aligned", what);
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "%s: unknown form %u", what, form);
  if (len == 0 || len > (1ull << 28))
    return set_err(ctx, B2F_ERR_ARG, "%s: len %llu not in [1, 2^28]", what, (unsigned long long)len);
  if (!fe_canonical(form, h_x)) return set_err(ctx, B2F_ERR_ARG, "%s: x is >= p", what);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_ipa_powers(h_x, len, form, d_b, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_ipa_round_dev(b2f_ctx* ctx, const uint64_t* d_p, const uint64_t* d_b, const uint64_t* d_g,
                              uint64_t len, uint32_t form, uint64_t* d_lr, uint64_t* d_values, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "ipa round";
  if (!d_lr || !d_values) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (((uintptr_t)d_lr | (uintptr_t)d_values) & 15)
    return set_err(ctx, B2F_ERR_ARG, "%s: buffers must be 16-byte aligned", what);
  if (int rc = ipa_check_vectors(ctx, what, d_p, d_b, d_g, len, form)) return rc;
  const struct {
    const void* at;
    uint64_t bytes;
  } in[3] = {{d_p, 32 * len}, {d_b, 32 * len}, {d_g, 64 * len}};
  for (const auto& v : in)
    if (ranges_overlap(d_lr, 128, v.at, v.bytes) || ranges_overlap(d_values, 64, v.at, v.bytes))
      return set_err(ctx, B2F_ERR_ARG, "%s: an output overlaps an input", what);
  if (ranges_overlap(d_lr, 128, d_values, 64)) return set_err(ctx, B2F_ERR_ARG, "%s: the outputs overlap", what);
  uint64_t direct_max = 0;
  if (!ipa_direct_for(&direct_max)) return set_err(ctx, B2F_ERR_ARG, "%s: the forced switch-over is malformed", what);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (len <= direct_max) {
    int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
    HIPCHK(ctx, launch_ipa_round_direct(d_p, d_b, d_g, len, form, d_lr, d_values, ctx->d_status + 2, s));
    timed_end(ctx, tk, s);
    return B2F_OK;
  }
  MsmPlan plan;
  if (!msm_plan_of(len / 2, 2, 0, 0, &plan)) return set_err(ctx, B2F_ERR_ARG, "%s: no plan", what);
  if (int rc = grow_device(ctx, &ctx->d_msm, &ctx->msm_cap, plan.scratch_bytes, 1, s)) return rc;
  if (int rc = grow_device(ctx, &ctx->d_ipa, &ctx->ipa_cap, ipa_scratch_bytes(len), 1, s)) return rc;
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_ipa_round_long(plan, d_p, d_b, d_g, len, form, d_lr, d_values, ctx->d_msm, ctx->d_ipa,
                                    ctx->d_status + 2, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_ipa_fold_dev(b2f_ctx* ctx, uint64_t* d_p, uint64_t* d_b, uint64_t* d_g, uint64_t len,
                             const uint64_t h_u[4], uint32_t form, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "ipa fold";
  if (!h_u) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (int rc = ipa_check_vectors(ctx, what, d_p, d_b, d_g, len, form)) return rc;
  if (!fe_canonical(form, h_u) || fe_is_zero(h_u)) return set_err(ctx, B2F_ERR_ARG, "%s: u is zero or >= p", what);
  uint64_t uinv[4], u_mont[4], uinv_mont[4];
  if (!host_inverse(form, h_u, uinv)) return set_err(ctx, B2F_ERR_CHECK, "%s: the host inversion of u failed", what);
  host_to_mont(form, h_u, u_mont);
  host_to_mont(form, uinv, uinv_mont);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_ipa_fold(d_p, d_b, d_g, len, h_u, u_mont, uinv_mont, form, ctx->d_status + 2, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

}  // extern "C"

namespace {
// The cached table of a fixed base (b2f_fixed_base_mul_dev, and U and W of b2f_ipa_open_dev): the
// live entry of this (curve, base), or the next slot round-robin claimed for it (never `keep`, the
// other base's entry of the same call). *build: the slot's table is still to be launched (the
// caller does it inside its timed region and then sets live).
int fixed_base_table_slot(b2f_ctx* ctx, const uint64_t* h_base, uint32_t form, const b2f_fixed_base_tab* keep,
                   hipStream_t s, b2f_fixed_base_tab** tab, bool* build) {
  *build = false;
  for (auto& t : ctx->fb_tab)
    if (t.live && t.curve == (form >> 1) && !memcmp(t.base, h_base, 64)) {
      *tab = &t;
      return B2F_OK;
    }
  uint64_t table_bytes = 0;
  fixed_base_plan_of(nullptr, nullptr, nullptr, &table_bytes);
  b2f_fixed_base_tab* t = &ctx->fb_tab[ctx->fb_next++ % b2f_ctx::FB_TABS];
  if (t == keep) t = &ctx->fb_tab[ctx->fb_next++ % b2f_ctx::FB_TABS];
  t->live = false;
  if (int rc = grow_device(ctx, &t->d, &t->cap, table_bytes, 1, s)) return rc;
  t->curve = form >> 1;
  memcpy(t->base, h_base, 64);
  *tab = t;
  *build = true;
  return B2F_OK;
}

// what the transcript calls check alike: the state, the data block of n elements of elem bytes
int transcript_check(b2f_ctx* ctx, const char* what, const uint64_t* d_state, const void* d_data, uint64_t n,
                     uint64_t elem, uint32_t form) {
  if (!d_state || !d_data) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (((uintptr_t)d_state | (uintptr_t)d_data) & 15)
    return set_err(ctx, B2F_ERR_ARG, "%s: buffers must be 16-byte aligned", what);
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "%s: unknown form %u", what, form);
  if (n == 0 || n > (1ull << 20))
    return set_err(ctx, B2F_ERR_ARG, "%s: n %llu not in [1, 2^20]", what, (unsigned long long)n);
  if (ranges_overlap(d_state, B2F_TRANSCRIPT_BYTES, d_data, n * elem))
    return set_err(ctx, B2F_ERR_ARG, "%s: the state overlaps the data", what);
  return B2F_OK;
}
}  // namespace

extern "C" {

B2F_API int b2f_transcript_init_dev(b2f_ctx* ctx, uint64_t* d_state, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "transcript init";
  if (!d_state || ((uintptr_t)d_state & 15)) return set_err(ctx, B2F_ERR_ARG, "%s: d_state null or unaligned", what);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_transcript_init(d_state, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_transcript_absorb_points_dev(b2f_ctx* ctx, uint64_t* d_state, const uint64_t* d_points, uint64_t n,
                                             uint32_t form, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  if (int rc = transcript_check(ctx, "transcript absorb points", d_state, d_points, n, 64, form)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_transcript_absorb(d_state, d_points, (uint32_t)n, form, true, ctx->d_status + 2, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_transcript_absorb_scalars_dev(b2f_ctx* ctx, uint64_t* d_state, const uint64_t* d_scalars, uint64_t n,
                                              uint32_t form, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  if (int rc = transcript_check(ctx, "transcript absorb scalars", d_state, d_scalars, n, 32, form)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_transcript_absorb(d_state, d_scalars, (uint32_t)n, form, false, ctx->d_status + 2, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_transcript_squeeze_dev(b2f_ctx* ctx, uint64_t* d_state, uint32_t form, uint64_t* d_challenge,
                                       void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  if (int rc = transcript_check(ctx, "transcript squeeze", d_state, d_challenge, 1, 32, form)) return rc;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_transcript_squeeze(d_state, form, d_challenge, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_ipa_open_dev(b2f_ctx* ctx, uint64_t* d_p, uint64_t* d_b, uint64_t* d_g, uint64_t len,
                             const uint64_t h_u_point[8], const uint64_t h_w_point[8], const uint64_t* d_z,
                             const uint64_t* d_rand, uint64_t* d_state, uint32_t form, uint64_t* d_lr, uint64_t* d_u,
                             uint64_t* d_cf, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "ipa open";
  if (!h_u_point || !h_w_point || !d_z || !d_rand || !d_state || !d_lr || !d_u || !d_cf)
    return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (((uintptr_t)d_z | (uintptr_t)d_rand | (uintptr_t)d_state | (uintptr_t)d_lr | (uintptr_t)d_u | (uintptr_t)d_cf) & 15)
    return set_err(ctx, B2F_ERR_ARG, "%s: buffers must be 16-byte aligned", what);
  if (int rc = ipa_check_vectors(ctx, what, d_p, d_b, d_g, len, form)) return rc;
  uint64_t any_u = 0, any_w = 0;
  for (int i = 0; i < 8; i++) {
    any_u |= h_u_point[i];
    any_w |= h_w_point[i];
  }
  if (!any_u || !any_w) return set_err(ctx, B2F_ERR_ARG, "%s: U or W is the identity", what);
  uint32_t k = 0;
  while ((1ull << k) < len) k++;
  // every block the call touches: only the two read-only inputs may overlap each other
  const struct {
    const void* at;
    uint64_t bytes;
    bool written;
  } blk[9] = {{d_p, 32 * len, true},       {d_b, 32 * len, true},    {d_g, 64 * len, true},
              {d_z, 32, false},            {d_rand, 64ull * k, false}, {d_state, B2F_TRANSCRIPT_BYTES, true},
              {d_lr, 128ull * k, true},    {d_u, 32ull * k, true},   {d_cf, 64, true}};
  for (int i = 0; i < 9; i++)
    for (int j = i + 1; j < 9; j++)
      if ((blk[i].written || blk[j].written) && ranges_overlap(blk[i].at, blk[i].bytes, blk[j].at, blk[j].bytes))
        return set_err(ctx, B2F_ERR_ARG, "%s: a buffer the call writes overlaps another", what);
  uint64_t direct_max = 0;
  if (!ipa_direct_for(&direct_max)) return set_err(ctx, B2F_ERR_ARG, "%s: the forced switch-over is malformed", what);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // scratch for the largest round, grown before anything is queued: the commitments' block, the
  // rounds' block, and behind it the call's own words (raw L, R; values; the challenge)
  size_t msm_need = 0;
  for (uint64_t ln = len; ln >= 2; ln >>= 1) {
    if (ln <= direct_max) continue;
    MsmPlan plan;
    if (!msm_plan_of(ln / 2, 2, 0, 0, &plan)) return set_err(ctx, B2F_ERR_ARG, "%s: no plan", what);
    if (plan.scratch_bytes > msm_need) msm_need = plan.scratch_bytes;
  }
  const size_t own = ipa_scratch_bytes(len);
  if (msm_need)
    if (int rc = grow_device(ctx, &ctx->d_msm, &ctx->msm_cap, msm_need, 1, s)) return rc;
  if (int rc = grow_device(ctx, &ctx->d_ipa, &ctx->ipa_cap, own + 512, 1, s)) return rc;
  uint64_t* raw = reinterpret_cast<uint64_t*>((char*)ctx->d_ipa + own);  // 16 words
  uint64_t *values = raw + 16, *chal = raw + 24;                          // 8 and 12 words
  b2f_fixed_base_tab *tab_u = nullptr, *tab_w = nullptr;
  bool build_u = false, build_w = false;
  if (int rc = fixed_base_table_slot(ctx, h_u_point, form, nullptr, s, &tab_u, &build_u)) return rc;
  const bool same = !memcmp(h_u_point, h_w_point, 64);
  if (same) tab_w = tab_u;
  else if (int rc = fixed_base_table_slot(ctx, h_w_point, form, tab_u, s, &tab_w, &build_w)) return rc;
  int* sticky = ctx->d_status + 2;
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  if (build_u) {
    HIPCHK(ctx, launch_fixed_base_table(h_u_point, form, (uint64_t*)tab_u->d, sticky, s));
    tab_u->live = true;
  }
  if (build_w) {
    HIPCHK(ctx, launch_fixed_base_table(h_w_point, form, (uint64_t*)tab_w->d, sticky, s));
    tab_w->live = true;
  }
  uint32_t j = 0;
  for (uint64_t ln = len; ln >= 2; ln >>= 1, j++) {
    if (ln <= direct_max) {
      HIPCHK(ctx, launch_ipa_round_direct(d_p, d_b, d_g, ln, form, raw, values, sticky, s));
    } else {
      MsmPlan plan;
      if (!msm_plan_of(ln / 2, 2, 0, 0, &plan)) return set_err(ctx, B2F_ERR_ARG, "%s: no plan", what);
      HIPCHK(ctx, launch_ipa_round_long(plan, d_p, d_b, d_g, ln, form, raw, values, ctx->d_msm, ctx->d_ipa, sticky, s));
    }
    HIPCHK(ctx, launch_fixed_base_blind(raw, values, d_z, d_rand + 8ull * j, form, (const uint64_t*)tab_u->d,
                                        (const uint64_t*)tab_w->d, d_lr + 16ull * j, sticky, s));
    HIPCHK(ctx, launch_ipa_challenge(d_lr + 16ull * j, d_rand + 8ull * j, d_state, form, d_u + 4ull * j, chal,
                                     d_cf + 4, sticky, s));
    HIPCHK(ctx, launch_ipa_fold_ptr(d_p, d_b, d_g, ln, chal, form, sticky, s));
  }
  HIPCHK(ctx, launch_ipa_finish(d_p, d_state, form, d_cf, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_group_ntt_plan(uint32_t k, uint32_t form, uint64_t* scalar_muls, uint64_t* scratch_bytes) {
  if (k < 1 || k > 28 || form > B2F_FP_BN254_MONTGOMERY) return B2F_ERR_ARG;
  if (scalar_muls) *scalar_muls = group_ntt_scalar_muls(k);
  if (scratch_bytes) *scratch_bytes = group_ntt_scratch_bytes(k);
  return B2F_OK;
}

B2F_API int b2f_group_ntt_dev(b2f_ctx* ctx, const uint64_t* d_in, uint32_t k, const uint64_t omega[4],
                              uint32_t direction, uint32_t form, uint64_t* d_out, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "group ntt";
  if (!d_in || !d_out || !omega) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (((uintptr_t)d_in | (uintptr_t)d_out) & 15)
    return set_err(ctx, B2F_ERR_ARG, "%s: buffers must be 16-byte aligned", what);
  if (k < 1 || k > 28) return set_err(ctx, B2F_ERR_ARG, "%s: k %u not in [1, 28]", what, k);
  if (direction > B2F_NTT_INVERSE) return set_err(ctx, B2F_ERR_ARG, "%s: unknown direction %u", what, direction);
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "%s: unknown form %u", what, form);
  if (!fe_canonical(form, omega)) return set_err(ctx, B2F_ERR_ARG, "%s: omega is >= r", what);
  if (d_in != d_out && ranges_overlap(d_in, 64ull << k, d_out, 64ull << k))
    return set_err(ctx, B2F_ERR_ARG, "%s: input and output overlap without being equal", what);
  // omega^-1 and n^-1 for the inverse. A zero omega has no inverse and is no root of unity: the
  // device's root check reports it, the twiddles are then all zero and the output meaningless.
  uint64_t tw_base[4], ninv[4];
  memcpy(tw_base, omega, 32);
  if (direction == B2F_NTT_INVERSE) {
    const uint64_t n[4] = {1ull << k, 0, 0, 0};
    if (!host_inverse(form, n, ninv)) return set_err(ctx, B2F_ERR_CHECK, "%s: the host inversion of n failed", what);
    if (fe_is_zero(omega)) memset(tw_base, 0, 32);
    else if (!host_inverse(form, omega, tw_base))
      return set_err(ctx, B2F_ERR_CHECK, "%s: the host inversion of omega failed", what);
  }
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  if (int rc = grow_device(ctx, &ctx->d_gntt, &ctx->gntt_cap, group_ntt_scratch_bytes(k), 1, s)) return rc;
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  HIPCHK(ctx, launch_group_ntt(d_in, k, omega, tw_base, direction == B2F_NTT_INVERSE ? ninv : nullptr, form, d_out,
                               ctx->d_gntt, ctx->d_status + 2, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API int b2f_fixed_base_plan(uint64_t len, uint32_t form, uint32_t* window_bits, uint32_t* windows,
                                uint64_t* table_points, uint64_t* scratch_bytes) {
  if (len == 0 || len > (1ull << 28) || form > B2F_FP_BN254_MONTGOMERY) return B2F_ERR_ARG;
  fixed_base_plan_of(window_bits, windows, table_points, scratch_bytes);
  return B2F_OK;
}

B2F_API int b2f_fixed_base_mul_dev(b2f_ctx* ctx, const uint64_t h_base[8], const uint64_t* d_scalars, uint64_t len,
                                   uint32_t form, uint64_t* d_out, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  const char* what = "fixed base mul";
  if (!h_base || !d_scalars || !d_out) return set_err(ctx, B2F_ERR_ARG, "%s: null buffer", what);
  if (((uintptr_t)d_scalars | (uintptr_t)d_out) & 15)
    return set_err(ctx, B2F_ERR_ARG, "%s: buffers must be 16-byte aligned", what);
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "%s: unknown form %u", what, form);
  if (len == 0 || len > (1ull << 28))
    return set_err(ctx, B2F_ERR_ARG, "%s: len %llu not in [1, 2^28]", what, (unsigned long long)len);
  if (ranges_overlap(d_out, 64 * len, d_scalars, 32 * len))
    return set_err(ctx, B2F_ERR_ARG, "%s: the output overlaps the scalars", what);
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // the table of this (curve, base): cached, or built into the next slot
  b2f_fixed_base_tab* tab = nullptr;
  bool build = false;
  if (int rc = fixed_base_table_slot(ctx, h_base, form, nullptr, s, &tab, &build)) return rc;
  int tk = timed_begin(ctx, B2F_KERNEL_QUOTIENT, s);
  if (build) {
    HIPCHK(ctx, launch_fixed_base_table(h_base, form, (uint64_t*)tab->d, ctx->d_status + 2, s));
    tab->live = true;
  }
  HIPCHK(ctx, launch_fixed_base_mul(d_scalars, len, form, (const uint64_t*)tab->d, d_out, ctx->d_status + 2, s));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

B2F_API uint64_t b2f_gate_queries(uint32_t* pairs, uint64_t cap) { return gate_queries(pairs, cap); }

B2F_API int b2f_ntt_columns_dev(b2f_ctx* ctx, const uint64_t* d_in, uint64_t in_rows,
                                uint64_t in_len, uint32_t n_cols, uint32_t k,
                                const uint64_t omega[4], const uint64_t shift[4],
                                uint32_t direction, uint32_t form, uint64_t* d_out,
                                uint64_t out_rows, void* stream) {
  if (!ctx) return B2F_ERR_ARG;
  if (!d_in || !d_out || !omega || !shift) return set_err(ctx, B2F_ERR_ARG, "ntt: null buffer");
  if (((uintptr_t)d_in | (uintptr_t)d_out) & 15)
    return set_err(ctx, B2F_ERR_ARG, "ntt: buffers must be 16-byte aligned");
  if (k < 1 || k > 28) return set_err(ctx, B2F_ERR_ARG, "ntt: k %u not in [1, 28]", k);
  if (n_cols == 0 || in_len == 0) return set_err(ctx, B2F_ERR_ARG, "ntt: no columns or no input rows");
  if (direction > B2F_NTT_INVERSE) return set_err(ctx, B2F_ERR_ARG, "ntt: unknown direction %u", direction);
  if (form > B2F_FP_BN254_MONTGOMERY) return set_err(ctx, B2F_ERR_ARG, "ntt: unknown form %u", form);
  if (!fe_canonical(form, omega) || !fe_canonical(form, shift))
    return set_err(ctx, B2F_ERR_ARG, "ntt: omega/shift not canonical field elements");
  if (fe_is_zero(shift)) return set_err(ctx, B2F_ERR_ARG, "ntt: shift is zero");
  const uint64_t n_rows = 1ull << k;
  if (in_len > n_rows) return set_err(ctx, B2F_ERR_ROWS, "ntt: in_len %llu > 2^k", (unsigned long long)in_len);
  if (in_rows < in_len) return set_err(ctx, B2F_ERR_ROWS, "ntt: in_rows < in_len");
  if (out_rows < n_rows) return set_err(ctx, B2F_ERR_ROWS, "ntt: out_rows < 2^k");
  if (in_rows > (1ull << 58) / n_cols || out_rows > (1ull << 58) / n_cols)
    return set_err(ctx, B2F_ERR_ARG, "ntt: column strides overflow the address space");
  const uintptr_t i0 = (uintptr_t)d_in, i1 = i0 + (uint64_t)n_cols * in_rows * 32;
  const uintptr_t o0 = (uintptr_t)d_out, o1 = o0 + (uint64_t)n_cols * out_rows * 32;
  if (i0 < o1 && o0 < i1) return set_err(ctx, B2F_ERR_ARG, "ntt: input and output overlap (no in-place transform)");
  const uint32_t* plan = nullptr;
#ifdef B2F_DIAG
  uint32_t forced[5];
  const int have_plan = diag_ntt_plan(k, forced);
  if (have_plan < 0) return set_err(ctx, B2F_ERR_ARG, "ntt: the forced pass plan does not fit k = %u", k);
  if (have_plan) plan = forced;
#endif
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(ctx, hipSetDevice(ctx->device));
  // the table block of this domain: cached, or built into the next slot
  int tk = timed_begin(ctx, B2F_KERNEL_NTT, s);
  b2f_domain_tab *tab, *slot;
  if (int rc = domain_tab_find(ctx, ctx->ntt_tab, b2f_ctx::NTT_TABS, &ctx->ntt_next, form, k, direction, omega,
                               shift, ntt_table_bytes(k), s, &tab, &slot))
    return rc;
  if (!tab) {
    HIPCHK(ctx, launch_ntt_tables(slot->d, form, k, omega, shift, direction, s));
    slot->live = true;
    tab = slot;
  }
  const bool shift_is_one = shift[0] == 1 && !(shift[1] | shift[2] | shift[3]);
  HIPCHK(ctx, launch_ntt(d_in, in_rows, in_len, n_cols, k, form, direction, shift_is_one, d_out, out_rows,
                         tab->d, ctx->d_status + 2, s, plan));
  timed_end(ctx, tk, s);
  return B2F_OK;
}

}  // extern "C"
