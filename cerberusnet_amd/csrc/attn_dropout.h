// attn_dropout.h -- the keep decision of the attention core's dropout (detr_attn.hip): ONE definition for the forward, both backward
// kernels and the mask op.  Stateless: a 32-bit integer hash of (seed, plane = b H + h, query index, key index) compared with a
// threshold, so a probability dropped in the forward is dropped again when the backward recomputes it, whichever workgroup owns it.
//
//   mix(x)              murmur3's 32-bit finaliser: x ^= x >> 16; x *= 0x85EBCA6B; x ^= x >> 13; x *= 0xC2B2AE35; x ^= x >> 16
//   plane_key(seed, p)  mix(lo(seed) ^ mix(hi(seed) + 0x9E3779B9 (p + 1)))
//   row_key(pk, i)      mix(pk + 0x85EBCA77 i)
//   keep(rk, j)         mix(rk ^ (0xC2B2AE3D j)) >= threshold
//   threshold(p)        min(2^32 - 1, floor(p 2^32)) for the fp32 value p: P(keep) = 1 - threshold / 2^32
//
// All arithmetic is modulo 2^32.  Within a row the map j -> hash is injective (an odd multiplier, an xor, a bijective finaliser).
// tests/attn_cases.py restates it in torch integer ops; attn_dropout_keep writes it out as a (B,H,Lq,Lk) bool tensor.
#pragma once
#include <stdint.h>

namespace cerb {

__host__ __device__ __forceinline__ uint32_t attn_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x85EBCA6Bu;
    x ^= x >> 13;
    x *= 0xC2B2AE35u;
    x ^= x >> 16;
    return x;
}

__host__ __device__ __forceinline__ uint32_t attn_plane_key(int64_t seed, int plane) {
    const uint64_t s = static_cast<uint64_t>(seed);
    const uint32_t lo = static_cast<uint32_t>(s), hi = static_cast<uint32_t>(s >> 32);
    return attn_mix(lo ^ attn_mix(hi + 0x9E3779B9u * (static_cast<uint32_t>(plane) + 1u)));
}

__host__ __device__ __forceinline__ uint32_t attn_row_key(uint32_t plane_key, int i) {
    return attn_mix(plane_key + 0x85EBCA77u * static_cast<uint32_t>(i));
}

__host__ __device__ __forceinline__ bool attn_keep(uint32_t row_key, int j, uint32_t threshold) {
    return attn_mix(row_key ^ (0xC2B2AE3Du * static_cast<uint32_t>(j))) >= threshold;
}

// p in [0, 1): checked by the caller
static inline uint32_t attn_threshold(float p) {
    const double t = static_cast<double>(p) * 4294967296.0;
    return t >= 4294967295.0 ? 4294967295u : static_cast<uint32_t>(t);
}

}  // namespace cerb
