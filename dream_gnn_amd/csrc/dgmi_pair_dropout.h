// dgmi_pair_dropout.h — "which hidden units of which listed pair survive dropout" as a FUNCTION, shared by the forward
// and the backward kernels of dgmi_pairs_train.hip and restated in numpy by the tests (in the spirit of dgmi_keep.h: no
// mask tensor exists, the backward recomputes what the forward drew).
//
//     keep(seed, layer, e, j)  <=>  p == 0  ||  hash32(key(seed, layer), e, j) < thr,      thr = floor((1 - p) 2^32)
// layer in {1, 2}; e: the POSITION in the pair list (a duplicated pair gets a different mask at each position, as with
// nn.Dropout on the E x H tensor); j < 128 (layer 1) or j < 64 (layer 2).  A kept element is scaled by 1 / (1 - p),
// computed in double and rounded once to fp32 (exactly 2 at p = 0.5, exactly 1 at p = 0).  Nothing depends on the launch
// geometry.
//
// Keys.  The caller's 64-bit seed goes through the splitmix64 finaliser before it keys anything, and each layer's key is
// one more finaliser step: key(seed, layer) = mix64(mix64(seed) + layer).  Sequential or bit-flipped seeds therefore give
// unrelated keys; an element hash that XORs the raw seed into the element id gives translated copies of one pattern for
// such seeds (what edge_hash of dgmi_keep.h does with its low seed word).
//
// Element hash.  Two 32-bit avalanche rounds, as edge_hash: the murmur3 finaliser over e ^ key.lo (pair_hash_e: once per
// pair and layer), then the "lowbias32" mixer over that + key.hi + j * 0x9E3779B9 (pair_hash_j: two multiplies per
// element, j * 0x9E3779B9 folds into a constant wherever j is one).
#ifndef DGMI_PAIR_DROPOUT_H_
#define DGMI_PAIR_DROPOUT_H_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dgmi {

constexpr uint32_t kPairHashJ = 0x9E3779B9u;

// the splitmix64 step: add the golden-ratio increment, then the finaliser
__host__ __device__ inline uint64_t mix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__host__ __device__ inline uint64_t pair_dropout_key(uint64_t seed, int layer) { return mix64(mix64(seed) + (uint64_t)layer); }

__host__ __device__ inline uint32_t pair_hash_e(uint32_t key_lo, uint32_t e) {
  uint32_t x = e ^ key_lo;
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// he: pair_hash_e of the pair; kj = key_hi + j * kPairHashJ
__host__ __device__ inline uint32_t pair_hash_j(uint32_t he, uint32_t kj) {
  uint32_t x = he + kj;
  x ^= x >> 16;
  x *= 0x7FEB352Du;
  x ^= x >> 15;
  x *= 0x846CA68Bu;
  x ^= x >> 16;
  return x;
}

// What a launch passes to its kernel by value; the seed itself is read from device memory by the kernel.
struct PairDropout {
  uint32_t thr;   // floor((1 - p) 2^32); not consulted when all != 0
  uint32_t all;   // p == 0: every element is kept (the threshold would be 2^32)
  float scale;    // 1 / (1 - p), rounded once
};

inline PairDropout pair_dropout_of(float p) {
  PairDropout d;
  const double q = 1.0 - (double)p;
  // 2^32 at p = 0 (and for p <= 2^-54, where 1 - p is 1.0 in double): nothing is dropped.  A larger p below 2^-32
  // gives 2^32 - 1: only a unit whose hash is 0xffffffff is dropped.
  const uint64_t t = (uint64_t)(q * 4294967296.0);
  d.all = t > 0xffffffffull ? 1u : 0u;
  d.thr = d.all ? 0xffffffffu : (uint32_t)t;
  d.scale = (float)(1.0 / q);
  return d;
}

// One layer's state in a kernel: the layer key split in two words, the threshold and the scale.
struct PairMask {
  uint32_t key_lo, key_hi, thr;
  bool all;
  float scale;

  __device__ __forceinline__ PairMask(uint64_t seed, int layer, const PairDropout& d) {
    const uint64_t k = pair_dropout_key(seed, layer);
    key_lo = (uint32_t)k, key_hi = (uint32_t)(k >> 32), thr = d.thr, all = d.all != 0u, scale = d.scale;
  }
  __device__ __forceinline__ uint32_t pair(uint32_t e) const { return pair_hash_e(key_lo, e); }
  // he = pair(e)
  __device__ __forceinline__ bool keep(uint32_t he, uint32_t j) const {
    return all || pair_hash_j(he, key_hi + j * kPairHashJ) < thr;
  }
};

}  // namespace dgmi

#endif  // DGMI_PAIR_DROPOUT_H_
