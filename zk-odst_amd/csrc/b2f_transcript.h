// b2f_transcript.h -- the Fiat-Shamir transcript on the device: halo2's Blake2bWrite / Challenge255
// (halo2_proofs 0.3.0 transcript.rs) as one lane's work on a state a workgroup keeps in LDS.
// DESIGN.md §4.13. Shared by b2f_transcript.hip (the transcript calls), b2f_ipa.hip (the opening's
// challenge step) and b2f_fieldprobe.hip (the wide reduction under test).
//
// The hash is BLAKE2b, 64-byte digest, no key, personalisation "Halo2-Transcript". The state in
// memory is 32 u64 words (B2F_TRANSCRIPT_BYTES; the layout is ABI, include/b2f.h):
//   0..7 h   8..9 t (bytes compressed so far)   10..25 the block buffer   26 buffered bytes (0..128)
//   27..31 zero
// A full buffer is compressed only when the next byte arrives (BLAKE2's lazy last block: the final
// block carries the flag), so t counts whole blocks and the buffer of a state holds 0..128 bytes.
// Buffer bytes at and past the count are zero: tr_compress clears the buffer behind it, so the
// padding of a finalisation is already there and an exported state is a function of the bytes
// absorbed alone. An imported state need not keep that: the finalisation clears the tail itself.
//
// Everything here that touches the state is one lane's: the caller picks the lane and fences the
// workgroup (__syncthreads) between other lanes' LDS writes and this lane's reads.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "b2f_field.h"

namespace b2f {
namespace transcript {

using field::Fe;

constexpr uint32_t STATE_WORDS = 32;

struct State {  // LDS image of the 32 words (the five zero words are not kept)
  uint64_t h[8];
  uint64_t t[2];
  uint64_t buf[16];
  uint64_t digest[8];  // a finalisation's output: the running h is left alone
  uint32_t count;
};

// IV ^ the parameter block: digest length 64, key length 0, fanout 1, depth 1 in word 0, the
// personalisation "Halo2-Transcript" in words 6 and 7
__device__ __forceinline__ uint64_t tr_iv(int i) {
  constexpr uint64_t IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull,
                              0xa54ff53a5f1d36f1ull, 0x510e527fade682d1ull, 0x9b05688c2b3e6c1full,
                              0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
  return IV[i];
}
__device__ __forceinline__ uint64_t tr_h0(int i) {
  constexpr uint64_t PERSON_LO = 0x72542d326f6c6148ull;  // "Halo2-Tr", little-endian
  constexpr uint64_t PERSON_HI = 0x7470697263736e61ull;  // "anscript"
  const uint64_t iv = tr_iv(i);
  return i == 0 ? iv ^ 0x01010040ull : i == 6 ? iv ^ PERSON_LO : i == 7 ? iv ^ PERSON_HI : iv;
}

__device__ __forceinline__ uint64_t rotr64(uint64_t x, int n) { return (x >> n) | (x << (64 - n)); }

// One compression of the buffer's 128 bytes (t must already count them). last: the final block's
// flag, and the result goes to st.digest and leaves h alone; otherwise it replaces h. The message
// words are read from LDS through the round's permutation; v stays in registers.
__device__ __noinline__ void tr_compress(State& st, bool last) {
  // SIGMA of RFC 7693, two rows to a round pair as bytes
  static constexpr uint8_t SIGMA[10][16] = {
      {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
      {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
      {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
      {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
      {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};
  uint64_t v[16];
#pragma unroll
  for (int i = 0; i < 8; i++) {
    v[i] = st.h[i];
    v[8 + i] = tr_iv(i);
  }
  v[12] ^= st.t[0];
  v[13] ^= st.t[1];
  if (last) v[14] = ~v[14];
#define B2F_TR_G(a, b, c, d, x, y)  \
  v[a] = v[a] + v[b] + (x);         \
  v[d] = rotr64(v[d] ^ v[a], 32);   \
  v[c] = v[c] + v[d];               \
  v[b] = rotr64(v[b] ^ v[c], 24);   \
  v[a] = v[a] + v[b] + (y);         \
  v[d] = rotr64(v[d] ^ v[a], 16);   \
  v[c] = v[c] + v[d];               \
  v[b] = rotr64(v[b] ^ v[c], 63);
#pragma unroll 1
  for (int r = 0; r < 12; r++) {
    const uint8_t* s = SIGMA[r % 10];
    B2F_TR_G(0, 4, 8, 12, st.buf[s[0]], st.buf[s[1]])
    B2F_TR_G(1, 5, 9, 13, st.buf[s[2]], st.buf[s[3]])
    B2F_TR_G(2, 6, 10, 14, st.buf[s[4]], st.buf[s[5]])
    B2F_TR_G(3, 7, 11, 15, st.buf[s[6]], st.buf[s[7]])
    B2F_TR_G(0, 5, 10, 15, st.buf[s[8]], st.buf[s[9]])
    B2F_TR_G(1, 6, 11, 12, st.buf[s[10]], st.buf[s[11]])
    B2F_TR_G(2, 7, 8, 13, st.buf[s[12]], st.buf[s[13]])
    B2F_TR_G(3, 4, 9, 14, st.buf[s[14]], st.buf[s[15]])
  }
#undef B2F_TR_G
  uint64_t h[8];
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] = st.h[i] ^ v[i] ^ v[8 + i];
  if (last) {
#pragma unroll
    for (int i = 0; i < 8; i++) st.digest[i] = h[i];
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++) st.h[i] = h[i];
  }
}

__device__ __forceinline__ void tr_init(State& st) {
#pragma unroll
  for (int i = 0; i < 8; i++) st.h[i] = tr_h0(i);
  st.t[0] = st.t[1] = 0;
#pragma unroll
  for (int i = 0; i < 16; i++) st.buf[i] = 0;
  st.count = 0;
}

// The count of a state from memory is clamped to the buffer: a corrupt word 26 gives a
// meaningless hash and never an access outside the buffer.
__device__ __forceinline__ void tr_load(State& st, const uint64_t* mem) {
#pragma unroll
  for (int i = 0; i < 8; i++) st.h[i] = mem[i];
  st.t[0] = mem[8];
  st.t[1] = mem[9];
#pragma unroll
  for (int i = 0; i < 16; i++) st.buf[i] = mem[10 + i];
  const uint64_t c = mem[26];
  st.count = c > 128 ? 128u : (uint32_t)c;
}
__device__ __forceinline__ void tr_store(const State& st, uint64_t* mem) {
#pragma unroll
  for (int i = 0; i < 8; i++) mem[i] = st.h[i];
  mem[8] = st.t[0];
  mem[9] = st.t[1];
#pragma unroll
  for (int i = 0; i < 16; i++) mem[10 + i] = st.buf[i];
  mem[26] = st.count;
#pragma unroll
  for (int i = 27; i < 32; i++) mem[i] = 0;
}

__device__ __forceinline__ void tr_absorb_byte(State& st, uint8_t byte) {
  if (st.count == 128) {  // the block is no longer the last one: compress it now
    st.t[0] += 128;
    if (st.t[0] < 128) st.t[1]++;
    tr_compress(st, false);
#pragma unroll
    for (int i = 0; i < 16; i++) st.buf[i] = 0;
    st.count = 0;
  }
  reinterpret_cast<uint8_t*>(st.buf)[st.count++] = byte;
}
__device__ __forceinline__ void tr_absorb(State& st, const uint8_t* src, uint32_t n) {
#pragma unroll 1
  for (uint32_t i = 0; i < n; i++) tr_absorb_byte(st, src[i]);
}

// The digest of the bytes absorbed so far as sixteen little-endian u32 words; the state goes on
// un-finalised (only buffer bytes past the count are cleared, which no absorbed byte depends on).
__device__ __forceinline__ void tr_digest(State& st, uint32_t (&words)[16]) {
  uint8_t* bytes = reinterpret_cast<uint8_t*>(st.buf);
#pragma unroll 1
  for (uint32_t i = st.count; i < 128; i++) bytes[i] = 0;
  const uint64_t t0 = st.t[0], t1 = st.t[1];
  st.t[0] += st.count;
  if (st.t[0] < t0) st.t[1]++;
  tr_compress(st, true);
  st.t[0] = t0;
  st.t[1] = t1;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    words[2 * i] = (uint32_t)st.digest[i];
    words[2 * i + 1] = (uint32_t)(st.digest[i] >> 32);
  }
}

// (lo + hi 2^256) mod p, canonical, for any two 256-bit integers (from_uniform_bytes of the
// 64-byte digest). The Montgomery product takes any 256-bit a against b < p: a b < 2^256 p, so
// (a b + m p) / 2^256 < 2p and the one conditional subtraction finishes it. lo * (R mod p) / R =
// lo mod p; hi * (R^2 mod p) / R = hi R mod p.
template <class F>
__device__ __forceinline__ Fe reduce_wide(const Fe& lo, const Fe& hi) {
  using namespace field;
  return add<F>(mul<F>(lo, fe_const<F>(F::R)), mul<F>(hi, fe_const<F>(F::R2)));
}

// squeeze_challenge: absorb the byte 0, finalise a copy, reduce the digest modulo the scalar
// field's modulus. Canonical.
template <class FS>
__device__ __forceinline__ Fe tr_squeeze(State& st) {
  tr_absorb_byte(st, 0);
  uint32_t w[16];
  tr_digest(st, w);
  Fe lo, hi;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    lo.w[i] = w[i];
    hi.w[i] = w[8 + i];
  }
  return reduce_wide<FS>(lo, hi);
}

// The bytes of a canonical element, little-endian, to dst (any alignment)
__device__ __forceinline__ void put_bytes(uint8_t* dst, const Fe& a) {
#pragma unroll
  for (int i = 0; i < 8; i++) {
    dst[4 * i] = (uint8_t)a.w[i];
    dst[4 * i + 1] = (uint8_t)(a.w[i] >> 8);
    dst[4 * i + 2] = (uint8_t)(a.w[i] >> 16);
    dst[4 * i + 3] = (uint8_t)(a.w[i] >> 24);
  }
}

// common_scalar's 33 bytes of a canonical scalar, by one lane; stage: 33 bytes of LDS of its own
__device__ __forceinline__ void tr_absorb_scalar(State& st, uint8_t* stage, const Fe& canonical) {
  stage[0] = 2;
  put_bytes(stage + 1, canonical);
  tr_absorb(st, stage, 33);
}

}  // namespace transcript
}  // namespace b2f
