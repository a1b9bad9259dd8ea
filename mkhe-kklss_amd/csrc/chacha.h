// chacha.h -- the quarter round of the ChaCha20 block function (RFC 8439 section 2.1), shared by the kernels that expand the keystream of
// include/mkhe.h ("device-side sampling"): small_sample_kernel (encdec_kernels.hip), share_finish_kernel (decshare_kernels.hip), refresh_finish_kernel
// (refresh_kernels.hip), bfv_refresh_finish_kernel (bfv_refresh_kernels.hip), pcks_finish_kernel (pcks_kernels.hip) and the two sampling kernels of
// skenc_kernels.hip; and the block as the 64-bit values of its 8 coefficients, for the four last.
#pragma once
#include "modarith.h"

namespace mkhe {

__device__ __forceinline__ u32 rotl32(u32 x, int n) { return (x << n) | (x >> (32 - n)); }
__device__ __forceinline__ void chacha_qr(u32& a, u32& b, u32& c, u32& d) {
    a += b; d = rotl32(d ^ a, 16);
    c += d; b = rotl32(b ^ c, 12);
    a += b; d = rotl32(d ^ a, 8);
    c += d; b = rotl32(b ^ c, 7);
}

// the 64-bit values of the 8 coefficients of block blk of one stream (include/mkhe.h, "device-side sampling")
__device__ __forceinline__ void chacha_block8(const u32 (&key)[8], u32 nonce_lo, u32 nonce_hi, u32 blk, u32 stream, u64 (&r)[8]) {
    const u32 in[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, key[0], key[1], key[2], key[3],
                        key[4],      key[5],      key[6],      key[7],      blk,    nonce_lo, nonce_hi, stream};
    u32 x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) x[i] = in[i];
#pragma unroll
    for (int k = 0; k < 10; ++k) {
        chacha_qr(x[0], x[4], x[8], x[12]); chacha_qr(x[1], x[5], x[9], x[13]); chacha_qr(x[2], x[6], x[10], x[14]); chacha_qr(x[3], x[7], x[11], x[15]);
        chacha_qr(x[0], x[5], x[10], x[15]); chacha_qr(x[1], x[6], x[11], x[12]); chacha_qr(x[2], x[7], x[8], x[13]); chacha_qr(x[3], x[4], x[9], x[14]);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) r[i] = (u64)(x[2 * i] + in[2 * i]) | ((u64)(x[2 * i + 1] + in[2 * i + 1]) << 32);
}

}  // namespace mkhe
