// chacha.h -- the quarter round of the ChaCha20 block function (RFC 8439 section 2.1), shared by the kernels that expand the keystream of
// include/mkhe.h ("device-side sampling"): small_sample_kernel (encdec_kernels.hip), share_finish_kernel (decshare_kernels.hip) and refresh_finish_kernel (refresh_kernels.hip).
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

}  // namespace mkhe
