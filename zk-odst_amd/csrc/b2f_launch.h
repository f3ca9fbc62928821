// b2f_launch.h -- the launch API between the C entry points (b2f_kernels.hip, b2f_api_prover.hip)
// and the files that define the kernels. Each defining file includes it too, so a signature that
// drifts from its declaration fails to link (the libraries are linked with --no-undefined). The
// evaluation / opening calls' launchers take a host plan and are declared with it in b2f_open.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/b2f.h"

namespace b2f {

// b2f_lookup.hip
size_t lookup_scratch_bytes(uint32_t group, uint64_t usable_rows);
hipError_t launch_lookup(const uint32_t* d_advice, uint64_t total_rows,
                         const uint64_t* d_row_begin, uint32_t n_circuits, uint64_t usable_rows,
                         const uint64_t* theta, const uint64_t* beta, const uint64_t* gamma,
                         uint32_t form, uint64_t* d_out, uint64_t out_rows, uint64_t* d_first_bad,
                         void* scratch, uint32_t group, int* sticky, hipStream_t s2,
                         hipEvent_t ev_fork, hipEvent_t ev_join, hipStream_t s3, hipEvent_t ev_tab,
                         hipEvent_t ev_sorted, hipStream_t s);
hipError_t launch_spread_table(uint64_t usable_rows, uint32_t form, uint64_t* d_out,
                               uint64_t out_rows, hipStream_t s);

// b2f_perm.hip
size_t perm_scratch_bytes(uint32_t k, uint64_t usable_rows, size_t n_inst, uint32_t chunk_len);
size_t perm_sigma_scratch_bytes(uint32_t k);
size_t perm_batch_scratch_bytes(uint32_t k, uint64_t usable_rows, uint32_t group, uint32_t chunk_len);
uint32_t perm_batch_group(uint64_t usable_rows, uint32_t n_circuits, uint32_t chunk_len);
uint32_t perm_circ_words();
hipError_t launch_permutation_sigma(const uint64_t* d_inst, size_t n_inst, const uint32_t* d_pool, uint32_t k,
                                    const uint64_t* omega, const uint64_t* delta, uint32_t form,
                                    uint64_t* d_sigma, uint64_t out_rows, void* scratch, hipStream_t s);
hipError_t launch_permutation(const uint32_t* d_advice, uint64_t total_rows, uint64_t row0,
                              const uint64_t* d_inst, size_t n_inst, const uint32_t* d_pool,
                              uint32_t k, uint64_t usable_rows, const uint64_t* omega,
                              const uint64_t* delta, const uint64_t* beta, const uint64_t* gamma,
                              uint32_t chunk_len, uint32_t form, uint64_t* d_sigma, uint64_t* d_z,
                              uint64_t out_rows, void* scratch, int* sticky, hipStream_t s2,
                              hipEvent_t ev_fork, hipEvent_t ev_join, hipStream_t s);
hipError_t launch_permutation_batch(const uint32_t* d_advice, uint64_t total_rows, const uint64_t* d_tab,
                                    uint32_t n_circuits, uint32_t group, const uint32_t* d_pool,
                                    uint32_t k, uint64_t usable_rows, const uint64_t* omega,
                                    const uint64_t* delta, const uint64_t* beta, const uint64_t* gamma,
                                    uint32_t chunk_len, uint32_t form, uint64_t* d_z, uint64_t out_rows,
                                    void* scratch, int* sticky, hipStream_t s2, hipEvent_t ev_fork,
                                    hipEvent_t ev_join, hipStream_t s);

// b2f_ntt.hip
size_t ntt_table_bytes(uint32_t k);
hipError_t launch_ntt_tables(void* d_tab, uint32_t form, uint32_t k, const uint64_t* omega,
                             const uint64_t* shift, uint32_t direction, hipStream_t s);
hipError_t launch_ntt(const uint64_t* d_in, uint64_t in_rows, uint64_t in_len, uint32_t n_cols,
                      uint32_t k, uint32_t form, uint32_t direction, bool shift_is_one, uint64_t* d_out,
                      uint64_t out_rows, const void* d_tab, int* sticky, hipStream_t s,
                      const uint32_t* plan = nullptr);
void ntt_plan_of(uint32_t k, uint32_t* out);

// b2f_quotient.hip
size_t quot_xtab_bytes(uint32_t ext_k);
size_t quot_consts_bytes();
hipError_t launch_quot_xtab(void* d_tab, uint32_t form, uint32_t ext_k, const uint64_t* omega,
                            const uint64_t* shift, hipStream_t s);
hipError_t launch_lagrange_selectors(uint32_t k, uint32_t usable_rows, uint32_t form, uint64_t* d_out,
                                     uint64_t out_rows, hipStream_t s);
hipError_t launch_quot_permutation(uint32_t k, uint32_t ext_k, uint32_t usable_rows, const uint64_t* d_l,
                                   const uint64_t* d_advice, const uint64_t* d_sigma, const uint64_t* d_z,
                                   uint32_t chunk_len, uint64_t rows, const uint64_t* delta,
                                   const uint64_t* beta, const uint64_t* gamma, const uint64_t* y,
                                   const uint64_t* d_h_in, uint64_t* d_h_out, uint32_t form, uint32_t colmap,
                                   const void* d_xtab, void* d_consts, int* sticky, hipStream_t s);
hipError_t launch_quot_lookup(uint32_t k, uint32_t ext_k, const uint64_t* d_l, const uint64_t* d_lookup,
                              uint64_t rows, const uint64_t* beta, const uint64_t* gamma, const uint64_t* y,
                              const uint64_t* d_h_in, uint64_t* d_h_out, uint32_t form, void* d_consts,
                              hipStream_t s);
hipError_t launch_quot_gates(uint32_t k, uint32_t ext_k, const uint64_t* d_advice, const uint64_t* d_fixed,
                             uint64_t rows, const uint64_t* y, const uint64_t* d_h_in, uint64_t* d_h_out,
                             uint32_t form, void* d_consts, hipStream_t s);
uint64_t gate_queries(uint32_t* pairs, uint64_t cap);
size_t quot_divisor_bytes(uint32_t k, uint32_t ext_k);
hipError_t launch_quot_divisors(void* d_dtab, uint32_t form, uint32_t k, uint32_t ext_k, const uint64_t* omega,
                                const uint64_t* shift, hipStream_t s);
hipError_t launch_quot_divide(uint32_t k, uint32_t ext_k, const uint64_t* d_h_in, uint64_t* d_h_out,
                              uint32_t form, const void* d_dtab, int* sticky, hipStream_t s);

// b2f_msm.hip: the plan of a commitment call (host only; the one place its scratch is sized) and
// the launcher. force_c / force_g: 0, or the diagnostics library's forced window width / group.
struct MsmPlan {
  uint32_t c, windows, buckets;  // window bits, windows per scalar, buckets per window (2^(c-1))
  uint32_t group;                // columns per pass
  uint64_t chunk;                // rows per pass
  uint64_t cap_entries, cap_buckets;  // what the scratch holds: digits and buckets of one pass
  uint64_t off_keys_a, off_keys_b, off_vals_a, off_vals_b, off_sort, sort_bytes, off_pkey_a, off_pkey_b,
      off_ppt_a, off_ppt_b, off_buckets, off_win, off_acc;
  uint64_t scratch_bytes;
};
uint32_t msm_default_window(uint64_t len);
bool msm_plan_of(uint64_t len, uint32_t n_cols, uint32_t force_c, uint32_t force_g, MsmPlan* plan);
// base_offsets (optional, calls of at most MSM_OFFSET_COLS columns): column c reads base
// row + v[c] where the others read base row; row + v[c] < 2^28 is the caller's to keep.
constexpr uint32_t MSM_OFFSET_COLS = 4;
struct MsmBaseOffsets {
  uint32_t v[MSM_OFFSET_COLS];
};
hipError_t launch_msm(const MsmPlan& plan, const uint64_t* d_scalars, uint64_t rows, uint64_t len, uint32_t n_cols,
                      const uint64_t* d_bases, uint32_t form, uint64_t* d_out, void* scratch, int* sticky,
                      hipStream_t s, const MsmBaseOffsets* base_offsets = nullptr);
#ifdef B2F_DIAG
int diag_msm_plan(uint32_t* c, uint32_t* g);
#endif

// b2f_msm.hip: the commitment of columns cut from u32 cells (b2f_msm_cells_dev). A column of
// `bits` bits has ceil((bits + 1) / c) windows of its own; a pass takes a run of columns (a group)
// and a chunk of rows, at most 2^24 digits and 2^20 buckets as above.
struct CellColumn {  // the device image of one b2f_cell_column, 32 bytes
  uint64_t offset;   // of the column's first cell
  uint32_t avail;    // min(avail, len): rows from here on are zero and never loaded
  uint32_t shift, mask;
  uint32_t windows;  // ceil((bits + 1) / c)
  uint32_t wbase;    // the column's first window among its group's
  uint32_t pad;
};
struct CellsPlan {
  uint32_t c, buckets;
  uint64_t chunk;                 // rows per pass
  uint64_t digits;                // len * (the sum of the columns' windows): what the call recodes
  std::vector<uint32_t> first;    // group g is columns [first[g], first[g + 1])
  std::vector<CellColumn> image;  // n_cols entries
  uint64_t cap_entries, cap_buckets;
  uint64_t off_keys_a, off_keys_b, off_vals_a, off_vals_b, off_sort, sort_bytes, off_pkey_a, off_pkey_b,
      off_ppt_a, off_ppt_b, off_buckets, off_win, off_acc, off_tail, off_desc;
  uint64_t scratch_bytes;
};
uint32_t msm_cells_default_window(uint64_t len, uint32_t bits);
// false: a count or a descriptor out of range, or a forced plan that exceeds a pass
bool msm_cells_plan_of(const b2f_cell_column* cols, uint32_t n_cols, uint64_t len, uint32_t force_c, uint32_t force_g,
                       CellsPlan* plan);
// The descriptors (plan.image) must already be at scratch + plan.off_desc, in stream order. With
// tail_rows != 0 the tail's scalar multiplications run on s2 beside the cell passes (forked after
// ev_fork, joined back into s through ev_join whatever the launches return).
hipError_t launch_msm_cells(const CellsPlan& plan, const uint32_t* d_cells, uint32_t n_cols, uint64_t len,
                            const uint64_t* d_tail, uint32_t tail_rows, const uint64_t* d_bases, uint32_t form,
                            uint64_t* d_out, void* scratch, int* sticky, hipStream_t s2, hipEvent_t ev_fork,
                            hipEvent_t ev_join, hipStream_t s);

// b2f_ipa.hip: the IPA opening rounds. A round of len <= ipa_direct_max_len() is one direct launch;
// a longer one is a two-column launch_msm with base offsets (its plan: msm_plan_of(len / 2, 2, ..),
// its scratch the commitments') plus the inner products, which need ipa_scratch_bytes(len). u, u_mont,
// uinv_mont: the challenge as canonical limbs, and it and its inverse in Montgomery form (host).
uint64_t ipa_direct_max_len();
size_t ipa_scratch_bytes(uint64_t len);
hipError_t launch_ipa_powers(const uint64_t* x, uint64_t len, uint32_t form, uint64_t* d_b, hipStream_t s);
hipError_t launch_ipa_round_direct(const uint64_t* d_p, const uint64_t* d_b, const uint64_t* d_g, uint64_t len,
                                   uint32_t form, uint64_t* d_lr, uint64_t* d_values, int* sticky, hipStream_t s);
hipError_t launch_ipa_round_long(const MsmPlan& plan, const uint64_t* d_p, const uint64_t* d_b, const uint64_t* d_g,
                                 uint64_t len, uint32_t form, uint64_t* d_lr, uint64_t* d_values, void* msm_scratch,
                                 void* ipa_scratch, int* sticky, hipStream_t s);
hipError_t launch_ipa_fold(uint64_t* d_p, uint64_t* d_b, uint64_t* d_g, uint64_t len, const uint64_t* u,
                           const uint64_t* u_mont, const uint64_t* uinv_mont, uint32_t form, int* sticky,
                           hipStream_t s);
// The one-call opening's steps. launch_ipa_challenge: absorb the blinded (L_j, R_j) at d_lr, squeeze u_j to
// d_u (canonical), move f on (d_f, in the form, with d_rand = (l_rand_j, r_rand_j)) and leave u, its
// Montgomery form and its inverse's in the 12 words at d_chal, which launch_ipa_fold_ptr's kernels
// read where launch_ipa_fold's take kernel arguments. launch_ipa_finish: c = p[0] to d_cf[0..3], c and
// f (d_cf[4..7]) absorbed as scalars.
hipError_t launch_ipa_fold_ptr(uint64_t* d_p, uint64_t* d_b, uint64_t* d_g, uint64_t len, const uint64_t* d_chal,
                               uint32_t form, int* sticky, hipStream_t s);
hipError_t launch_ipa_challenge(const uint64_t* d_lr, const uint64_t* d_rand, uint64_t* d_state, uint32_t form,
                                uint64_t* d_u, uint64_t* d_chal, uint64_t* d_f, int* sticky, hipStream_t s);
hipError_t launch_ipa_finish(const uint64_t* d_p, uint64_t* d_state, uint32_t form, uint64_t* d_cf, hipStream_t s);
#ifdef B2F_DIAG
int diag_ipa_direct(uint64_t* len);
#endif

// b2f_group_ntt.hip: the group NTT of 2^k affine points, in place in d_out after a bit-reversing
// copy (or swap, d_out == d_in). omega: the domain's generator (checked on the device); tw_base:
// omega or, for the inverse, omega^-1; ninv: n^-1 for the inverse, nullptr for the forward
// direction; all canonical host limbs. scratch holds group_ntt_scratch_bytes(k): the twiddles.
uint64_t group_ntt_scalar_muls(uint32_t k);
size_t group_ntt_scratch_bytes(uint32_t k);
hipError_t launch_group_ntt(const uint64_t* d_in, uint32_t k, const uint64_t* omega, const uint64_t* tw_base,
                            const uint64_t* ninv, uint32_t form, uint64_t* d_out, void* scratch, int* sticky,
                            hipStream_t s);

// b2f_fixed_base.hip: out[i] = [s_i] B. The plan is constant: the window bits, the windows of a
// scalar, the table's points (windows * 2^(bits - 1), signed digits) and its bytes. The table
// launch fills d_table from the host affine point `base` (8 limbs, base-field Montgomery form); the
// multiplication reads it. Both raise B2F_ERR_CHECK in sticky when an affine conversion fails.
void fixed_base_plan_of(uint32_t* window_bits, uint32_t* windows, uint64_t* table_points, uint64_t* table_bytes);
hipError_t launch_fixed_base_table(const uint64_t* base, uint32_t form, uint64_t* d_table, int* sticky,
                                   hipStream_t s);
hipError_t launch_fixed_base_mul(const uint64_t* d_scalars, uint64_t len, uint32_t form, const uint64_t* d_table,
                                 uint64_t* d_out, int* sticky, hipStream_t s);

// The blinded cross terms of an IPA round from the tables of U and W (b2f_ipa_open_dev):
// d_out[0..7] = L + [value_l z] U + [l_rand] W, d_out[8..15] the same for R. d_lr_raw: the round's (L, R);
// d_values: (value_l, value_r) and d_rand: (l_rand, r_rand), in the form; d_z: canonical. An identity
// output raises B2F_ERR_FIELD in sticky.
hipError_t launch_fixed_base_blind(const uint64_t* d_lr_raw, const uint64_t* d_values, const uint64_t* d_z,
                                   const uint64_t* d_rand, uint32_t form, const uint64_t* d_table_u,
                                   const uint64_t* d_table_w, uint64_t* d_out, int* sticky, hipStream_t s);

// b2f_transcript.hip: the Fiat-Shamir transcript on a 32-word device state. points: d_data holds n
// affine points (64 bytes, base-field Montgomery), else n scalars in `form`. The identity point raises
// B2F_ERR_FIELD in sticky. The challenge is four canonical limbs of the form's scalar field.
hipError_t launch_transcript_init(uint64_t* d_state, hipStream_t s);
hipError_t launch_transcript_absorb(uint64_t* d_state, const uint64_t* d_data, uint32_t n, uint32_t form,
                                    bool points, int* sticky, hipStream_t s);
hipError_t launch_transcript_squeeze(uint64_t* d_state, uint32_t form, uint64_t* d_challenge, hipStream_t s);

// b2f_export.hip
hipError_t launch_export_fp(const uint32_t* d_advice, uint64_t total_rows, uint64_t row_begin,
                            uint64_t nrows, uint32_t form, uint64_t* d_out, uint64_t out_rows,
                            int cu_count, unsigned* tctr, hipStream_t s);
hipError_t launch_export_fixed_fp(const uint32_t* d_fixed, uint64_t row_begin, uint64_t nrows,
                                  uint32_t form, uint64_t* d_out, uint64_t out_rows, hipStream_t s);

// b2f_fused.hip
size_t fused_scratch_bytes(uint64_t tiles);
uint64_t fused_instance_tiles(uint64_t total_rows, uint64_t n);
hipError_t launch_eval_fast(const uint32_t* d_adv, const uint32_t* d_fixed, const uint64_t* d_off, uint32_t n,
                            uint64_t total_rows, void* scratch, uint64_t tiles, const int* d_status,
                            int cu_count, hipStream_t s, const uint32_t** gate, int mode);
// `mode` bit of launch_fill_eval (FZ_NOFIX): the launch leaves the fixed column unwritten. The
// product library honours it (and no other bit); a call under the inject hook runs full.
constexpr int FUSED_MODE_NOFIX = 32;
hipError_t launch_fill_eval(const b2f_input* d_in, uint32_t n, const uint64_t* d_off,
                            uint64_t total_rows, const uint64_t* rec, uint32_t* d_adv,
                            uint32_t* d_fixed, void* scratch, uint64_t tiles,
                            b2f_eval_report* d_rep, const int* d_status, uint64_t inj_row,
                            uint32_t inj_col, uint32_t inj_mask, int mode, int cu_count,
                            unsigned long long* clk, const uint64_t* seg, uint64_t seg_cap,
                            hipStream_t s);

}  // namespace b2f
