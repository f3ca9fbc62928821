// b2f_transcript.hip -- the device-resident Fiat-Shamir transcript: halo2's Blake2bWrite /
// Challenge255 (halo2_proofs 0.3.0 transcript.rs) on a 256-byte state in device memory
// (b2f_transcript_*_dev, include/b2f.h). DESIGN.md §4.13; the hash and the state are
// b2f_transcript.h's.
//
//   common_point(P)    the byte 1, then x and y of the affine point, 32 little-endian bytes each,
//                      canonical (the device points are base-field Montgomery: converted here)
//   common_scalar(s)   the byte 2, then 32 little-endian bytes of the canonical scalar
//   squeeze_challenge  the byte 0 into the running state; a copy is finalised, its 64 digest
//                      bytes read as a little-endian integer and reduced modulo r
//
// One workgroup. The lanes convert a chunk of TR_THREADS elements to their framed bytes in LDS,
// lane 0 absorbs the chunk, and so on: the conversions (a Montgomery product or two per element)
// are the lanes', the compression one lane's -- about one compression per two points, cheap
// beside the commitments that produce them, so no more is wanted. The identity point (all zero)
// absorbs the byte 1 and 64 zero bytes and raises B2F_ERR_FIELD (halo2 refuses to write it).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/b2f.h"
#include "b2f_curve.h"
#include "b2f_field.h"
#include "b2f_launch.h"
#include "b2f_transcript.h"

namespace b2f {

namespace {

using namespace field;
using namespace curve;
using namespace transcript;

constexpr uint32_t TR_THREADS = 256;  // the elements of a chunk, one per lane
constexpr uint32_t POINT_BYTES = 65, SCALAR_BYTES = 33;

__global__ __launch_bounds__(64) void tr_init_kernel(uint64_t* __restrict__ state) {
  const uint32_t t = threadIdx.x;
  if (t < STATE_WORDS) state[t] = t < 8 ? tr_h0((int)t) : 0;
}

template <class C, bool MONT, bool POINTS>
__global__ __launch_bounds__(TR_THREADS) void tr_absorb_kernel(uint64_t* __restrict__ state,
                                                               const uint64_t* __restrict__ data, uint32_t n,
                                                               int* sticky) {
  constexpr uint32_t SZ = POINTS ? POINT_BYTES : SCALAR_BYTES;
  __shared__ State st;
  __shared__ uint8_t bytes[TR_THREADS * SZ];
  const uint32_t t = threadIdx.x;
  if (t == 0) tr_load(st, state);
#pragma unroll 1
  for (uint32_t base = 0; base < n; base += TR_THREADS) {
    __syncthreads();  // lane 0 is done with the previous chunk (and, the first time, the load)
    const uint32_t i = base + t;
    if (i < n) {
      uint8_t* dst = bytes + SZ * t;
      if (POINTS) {
        const Affine a = load_affine(data + 8ull * i);
        if (is_identity(a)) atomicOr(sticky, 1 << B2F_ERR_FIELD);
        dst[0] = 1;
        put_bytes(dst + 1, to_canonical<typename C::Base>(a.x));
        put_bytes(dst + 33, to_canonical<typename C::Base>(a.y));
      } else {
        Fe s = load(data + 4ull * i);
        if (MONT) s = to_canonical<typename C::Scalar>(s);
        dst[0] = 2;
        put_bytes(dst + 1, s);
      }
    }
    __syncthreads();
    if (t == 0) {
      const uint32_t m = n - base < TR_THREADS ? n - base : TR_THREADS;
      tr_absorb(st, bytes, m * SZ);
    }
  }
  if (t == 0) tr_store(st, state);
}

template <class FS>
__global__ __launch_bounds__(64) void tr_squeeze_kernel(uint64_t* __restrict__ state,
                                                        uint64_t* __restrict__ challenge) {
  __shared__ State st;
  if (threadIdx.x != 0) return;
  tr_load(st, state);
  const Fe c = tr_squeeze<FS>(st);
  store(challenge, c);
  tr_store(st, state);
}

}  // namespace

hipError_t launch_transcript_init(uint64_t* d_state, hipStream_t s) {
  hipLaunchKernelGGL(tr_init_kernel, dim3(1), dim3(64), 0, s, d_state);
  return hipGetLastError();
}

hipError_t launch_transcript_absorb(uint64_t* d_state, const uint64_t* d_data, uint32_t n, uint32_t form,
                                    bool points, int* sticky, hipStream_t s) {
  with_curve_form(form, [&](auto c, auto mont) {
    using C = decltype(c);
    if (points)  // a point's coordinates are Montgomery whatever the form
      hipLaunchKernelGGL((tr_absorb_kernel<C, true, true>), dim3(1), dim3(TR_THREADS), 0, s, d_state, d_data, n,
                         sticky);
    else
      hipLaunchKernelGGL((tr_absorb_kernel<C, decltype(mont)::value, false>), dim3(1), dim3(TR_THREADS), 0, s,
                         d_state, d_data, n, sticky);
  });
  return hipGetLastError();
}

hipError_t launch_transcript_squeeze(uint64_t* d_state, uint32_t form, uint64_t* d_challenge, hipStream_t s) {
  with_field(form, [&](auto f) {
    hipLaunchKernelGGL((tr_squeeze_kernel<decltype(f)>), dim3(1), dim3(64), 0, s, d_state, d_challenge);
    return 0;
  });
  return hipGetLastError();
}

}  // namespace b2f
