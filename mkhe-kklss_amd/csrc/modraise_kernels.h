// modraise_kernels.h -- the one kernel of mkhe_ct_mod_raise (include/mkhe.h, "raising the modulus"): a level-0 ciphertext, read as its centred
// representatives in (-q_0 / 2, q_0 / 2], under the first `lout` moduli.  HBM streaming and write-bound: 8 N polys bytes in, 8 N polys lout out.
#pragma once
#include "modarith.h"

namespace mkhe {

// out [polys][lout][N] <- in [polys][1][N], canonical in and out: with x = in[p][0][n] < q_0 and v = x for x <= (q_0 - 1) / 2, v = x - q_0 above it,
// out[p][l][n] = v mod q_l (limb 0: x itself).  q_l may be shorter than q_0: |v| is reduced for real, then the sign is folded in.  lout >= 2; N is a
// multiple of 8; both buffers are 16-byte aligned and distinct.
void launch_mod_raise(int polys, u64* out, const u64* in, const Mod* mods, int lout, int N, hipStream_t st);

}  // namespace mkhe
