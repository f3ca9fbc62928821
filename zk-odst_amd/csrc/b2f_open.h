// b2f_open.h -- the host plan of an evaluation / opening call (b2f_open.hip), shared with the C
// entry points in b2f_api_prover.hip. A plan is the host image of the call's device tables (the
// points, scalars and index lists of the host arrays, grouped as the kernels read them) plus the
// sizes of the device scratch the launches carve. The entry point stages the image in pinned
// memory, uploads it on the call's stream and hands both device blocks to the launcher.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace b2f {

struct OpenPlan {
  std::vector<uint64_t> blob;  // host image of the device tables, sections 16-byte aligned
  size_t scratch_bytes = 0;    // device scratch beyond the image
  uint64_t len = 0, ntiles = 0;
  uint32_t form = 0;
  uint32_t n_points = 0;
  // section offsets in the image, in u64 words
  size_t off_points = 0, off_a = 0, off_b = 0, off_c = 0;
  // poly_eval: groups (distinct queried columns), pairs (distinct (column, point)), queries
  // kate_divide: slots (columns with 0 < m < len, longest chain first), of which n_pp have a chain
  //   of two or more points; specials (copied or zeroed columns); passes = the longest chain
  // poly_combine: n_out outputs, nnz terms
  uint32_t n_groups = 0, n_pairs = 0, n_slots = 0, n_pp = 0, n_special = 0, passes = 0, n_out = 0, nnz = 0;
  uint64_t n_queries = 0;
  std::vector<uint32_t> active;  // kate_divide: slots still dividing in pass p
};

// Each returns B2F_OK or the status to report, with the reason in msg. Nothing is launched.
int open_plan_eval(OpenPlan& p, uint64_t len, uint32_t n_cols, const uint64_t* h_points, uint32_t n_points,
                   const uint32_t* h_queries, uint64_t n_queries, uint32_t form, char* msg, size_t msg_len);
int open_plan_combine(OpenPlan& p, uint64_t len, uint32_t n_cols, const uint32_t* h_first, const uint32_t* h_col,
                      const uint64_t* h_scalar, uint32_t n_out, uint32_t form, char* msg, size_t msg_len);
int open_plan_kate(OpenPlan& p, uint64_t len, uint32_t n_cols, const uint32_t* h_first, const uint64_t* h_points,
                   uint32_t form, char* msg, size_t msg_len);

// d_blob: the uploaded image; d_scratch: p.scratch_bytes of device memory.
hipError_t launch_poly_eval(const OpenPlan& p, const uint64_t* d_cols, uint64_t rows, const void* d_blob,
                            void* d_scratch, uint64_t* d_out, hipStream_t s);
hipError_t launch_poly_combine(const OpenPlan& p, const uint64_t* d_cols, uint64_t rows, const void* d_blob,
                               void* d_scratch, uint64_t* d_out, uint64_t out_rows, hipStream_t s);
hipError_t launch_kate_divide(const OpenPlan& p, const uint64_t* d_cols, uint64_t rows, const void* d_blob,
                              void* d_scratch, uint64_t* d_out, uint64_t out_rows, hipStream_t s);

}  // namespace b2f
