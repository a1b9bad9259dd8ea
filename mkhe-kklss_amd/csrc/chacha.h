// chacha.h -- the keystream of include/mkhe.h ("device-side sampling"): the (key, nonce) every key-bearing argument struct starts with, and block
// blk of one of its streams -- the ChaCha20 block function (RFC 8439 section 2.3) -- as the 64-bit values of its 8 coefficients.  Every kernel that
// expands the keystream calls chacha_block8: there is no other copy of the rounds.
#pragma once
#include "modarith.h"

namespace mkhe {

// Everything secret a sampling kernel reads travels in its arguments (scalar loads), never in device memory the engine owns.  The argument structs
// of such kernels derive from this one (aggregates, trivially copyable), so a.key and a.nonce_lo read as before and the helpers take the struct.
struct StreamKey {
    u32 key[8];
    u32 nonce_lo, nonce_hi;
};

__device__ __forceinline__ u32 rotl32(u32 x, int n) { return (x << n) | (x >> (32 - n)); }
__device__ __forceinline__ void chacha_qr(u32& a, u32& b, u32& c, u32& d) {
    a += b; d = rotl32(d ^ a, 16);
    c += d; b = rotl32(b ^ c, 12);
    a += b; d = rotl32(d ^ a, 8);
    c += d; b = rotl32(b ^ c, 7);
}

// the 64-bit values of the 8 coefficients of block blk of one stream of k
__device__ __forceinline__ void chacha_block8(const StreamKey& k, u32 blk, u32 stream, u64 (&r)[8]) {
    const u32 in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, k.key[0], k.key[1], k.key[2], k.key[3],
                        k.key[4],    k.key[5],    k.key[6],    k.key[7],    blk,      k.nonce_lo, k.nonce_hi, stream};
    u32 x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = in[i];
#pragma unroll
    for (int n = 0; n < 10; ++n) {
        chacha_qr(x[0], x[4], x[8], x[12]); chacha_qr(x[1], x[5], x[9], x[13]); chacha_qr(x[2], x[6], x[10], x[14]); chacha_qr(x[3], x[7], x[11], x[15]);
        chacha_qr(x[0], x[5], x[10], x[15]); chacha_qr(x[1], x[6], x[11], x[12]); chacha_qr(x[2], x[7], x[8], x[13]); chacha_qr(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (u64)(x[2 * i] + in[2 * i]) | ((u64)(x[2 * i + 1] + in[2 * i + 1]) << 32);
}

}  // namespace mkhe
