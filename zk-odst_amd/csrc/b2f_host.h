// b2f_host.h -- the host state and helpers the two C ABI files share: b2f_kernels.hip (the trace
// calls, the context, keygen) and b2f_api_prover.hip (the prover calls). Host code only; each
// function declared here is defined in b2f_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <map>
#include <vector>

#include "../../include/b2f.h"

// One table block of a domain, cached by (field, two integers, omega, shift): the NTT's twiddle /
// shift-power tables (a = k, b = direction), the quotient's X_i tables (a = 0, b = ext_k) and the
// inverse divisors of the vanishing divide (a = k, b = ext_k). Each table keeps a few blocks,
// replaced round-robin: a prover alternates a few domains, and a repeated call builds nothing.
struct b2f_domain_tab {
  uint32_t field, a, b;
  uint64_t omega[4], shift[4];
  void* d;
  size_t cap;
  bool live;  // set once the launch that fills the block was issued without error
};

// The table of one fixed base (b2f_fixed_base_mul_dev), cached by (curve, base) and replaced
// round-robin like the domain tables; the key is compared on the host.
struct b2f_fixed_base_tab {
  uint32_t curve;
  uint64_t base[8];
  void* d;
  size_t cap;
  bool live;
};

struct b2f_ctx {
  int device;
  char err[512];
  int* d_status;       // [0] fill call, [1] eval call, [2] sticky (cleared by b2f_sync only), [3] fill tile counter,
                       // [4] export tile counter
  uint64_t* d_rec;     // half-round states
  size_t rec_cap;      // in states (16 x u64 each)
  uint64_t* d_seg;     // the fused launch's segment list (count, entries: instance << 32 | m)
  size_t seg_cap;      // in u64 words
  void* d_tiles;       // per-tile instance context (TileInfo, b2f_common.h)
  size_t tiles_cap;
  int timing;
  std::vector<hipEvent_t> pool;  // event pairs, reused after every b2f_kernel_times
  std::vector<int> kinds;        // kernel kind of pair i
  int cu_count;
  unsigned long long* d_clock;  // 32 u64: EVAL_CLOCK phase totals (diagnostics)
  const uint32_t* d_eval_gate;  // the last eval's fast-pass word (0: the fast pass found the trace clean)
  uint64_t inj_row;    // b2f_debug_inject (UINT64_MAX: off)
  uint32_t inj_col, inj_mask;
  // the last full write of a fixed column by the fused call (b2f_fill_eval_dev[_ex]), hook off:
  // B2F_FIXED_RESIDENT is honoured only for a call with these arguments (fx_fixed null: none)
  const uint32_t* fx_fixed;
  const uint64_t* fx_offsets;
  size_t fx_n;
  uint64_t fx_rows;
  uint32_t fused_path;  // b2f_debug_fused_path: 1 the last fused call ran advice-only, 0 full
  void* d_lk;          // lookup-column scratch (b2f_lookup.hip carve)
  size_t lk_cap;
  void* d_fz;          // fused-path scratch: tile descriptors + deferred rows (b2f_fused.hip)
  size_t fz_cap;
  // permutation columns (b2f_perm.hip): keygen mapping patterns per rounds (host cache and
  // the device pool holding them), the per-call instance table, scratch
  std::map<uint32_t, std::vector<uint32_t>> pm_pat;
  std::map<uint32_t, uint64_t> pm_pool_off;  // rounds -> offset in d_pm_pool (u32 units)
  uint32_t* d_pm_pool;
  uint64_t* h_pm_inst;     // pinned staging of the per-call instance table
  size_t h_pm_inst_cap;
  hipEvent_t pm_inst_ev;   // recorded after the table's async upload (the staging is reusable
  bool pm_inst_ev_live;    // once it completes)
  uint64_t* d_pm_inst;
  size_t pm_inst_cap;
  void* d_pm;
  size_t pm_cap;
  // a second stream and two events: the grand products' inversions run beside their block
  // down-sweep (b2f_gprod.h), forked from and joined back to the caller's stream
  hipStream_t s2;
  hipEvent_t ev_fork, ev_join;
  hipStream_t s3;                // the lookup's table pass and sort (beside the count pass)
  hipEvent_t ev_tab, ev_sorted;
  static constexpr int NTT_TABS = 8, QUOT_TABS = 4;
  b2f_domain_tab ntt_tab[NTT_TABS];                         // b2f_ntt.hip
  b2f_domain_tab quot_tab[QUOT_TABS], quot_div[QUOT_TABS];  // b2f_quotient.hip: X_i, divisors
  uint32_t ntt_next, quot_next, quot_div_next;
  void* d_quot_consts;  // the per-call challenge constants of the quotient term calls
  // evaluation / opening calls (b2f_open.hip): the call's host arrays staged in pinned memory and
  // uploaded asynchronously (as the permutation's instance table is), and the scratch
  uint64_t* h_op;
  size_t h_op_cap;  // in u64 words
  hipEvent_t op_ev;
  bool op_ev_live;
  void* d_op_blob;
  size_t op_blob_cap;  // in u64 words
  void* d_op;
  size_t op_cap;
  void* d_msm;  // commitment scratch (b2f_msm.hip: msm_plan_of carves it)
  size_t msm_cap;
  // b2f_msm_cells_dev: the call's column descriptors staged in pinned memory and uploaded
  // asynchronously into d_msm (as the opening's plan is)
  void* h_cells;
  size_t h_cells_cap;  // in bytes
  hipEvent_t cells_ev;
  bool cells_ev_live;
  void* d_ipa;  // IPA round scratch beyond the commitments' (b2f_ipa.hip: ipa_scratch_bytes)
  size_t ipa_cap;
  void* d_gntt;  // the group NTT's twiddles (b2f_group_ntt.hip: group_ntt_scratch_bytes)
  size_t gntt_cap;
  static constexpr int FB_TABS = 4;
  b2f_fixed_base_tab fb_tab[FB_TABS];  // b2f_fixed_base.hip
  uint32_t fb_next;
};

namespace b2f {

constexpr int PM_COLS = 8;  // the permutation argument's columns (a_1 .. a_8)

int set_err(b2f_ctx* ctx, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));

#define HIPCHK(ctx, expr)                                                              \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess)                                                              \
      return set_err(ctx, B2F_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));        \
  } while (0)

// Record the start event of a timed launch; returns the pair index or -1.
int timed_begin(b2f_ctx* ctx, int kind, hipStream_t s);
void timed_end(b2f_ctx* ctx, int i, hipStream_t s);

// A context-owned device block of *cap elements of `elem` bytes: when `need` exceeds *cap, wait
// for the stream (earlier calls may still read the block; synced: the caller already has), free
// the block and allocate `need` elements. A failed allocation leaves *p null and *cap zero.
int grow_device(b2f_ctx* ctx, void** p, size_t* cap, size_t need, size_t elem, hipStream_t s,
                bool synced = false);
// The same for pinned host staging. Nothing is waited for: the caller guards the staging with the
// event of its last upload.
int grow_pinned(b2f_ctx* ctx, void** p, size_t* cap, size_t need, size_t elem);

// Keygen's permutation mapping of one instance (b2f_permutation_mapping); false: rounds too large.
bool perm_mapping(uint32_t rounds, std::vector<uint32_t>& out);

}  // namespace b2f
