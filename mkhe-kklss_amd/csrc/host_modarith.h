// host_modarith.h -- host number theory behind the device tables: what engine.hip, keygen.hip and the two encoders compute before they upload.
#pragma once
#include <vector>
#include "modarith.h"

namespace mkhe {

typedef unsigned __int128 u128;

static inline u64 mulmod(u64 a, u64 b, u64 q) { return (u64)(((u128)a * b) % q); }
static inline u64 powmod(u64 x, u64 e, u64 q) {
    u64 r = 1 % q; x %= q;
    for (; e; e >>= 1) { if (e & 1) r = mulmod(r, x, q); x = mulmod(x, x, q); }
    return r;
}
static inline u64 inv64(u64 q) { u64 x = q; for (int i = 0; i < 6; ++i) x *= 2 - q * x; return x; }   // q^-1 mod 2^64 (Newton)
static inline u64 to_mont(u64 a, u64 q) { return (u64)(((u128)a << 64) % q); }                      // MForm(a mod q), any 64-bit a
static inline u64 bitrev(u64 x, int bits) { u64 r = 0; for (int i = 0; i < bits; ++i) { r = (r << 1) | (x & 1); x >>= 1; } return r; }

// The permutation table of an encoder's in-place transform: position p holds X[bitrev(p)], slot j is X[t_j] with t_j = (e_j - 1) >> shift,
// e_j = 5^j mod 2N for j < N/2, so pos[bitrev(t_j)] = j.  conj_row: the second row e = 2N - 5^j is slot j + N/2.
// CKKS: shift 2, one row, N/2 points; BFV: shift 1, both rows, N points.
static inline std::vector<u32> slot_positions(int logN, int shift, bool conj_row) {
    const int bits = logN + 1 - shift;
    const u64 N = 1ull << logN;
    std::vector<u32> pos((size_t)1 << bits);
    u64 e = 1;
    for (u64 j = 0; j < N / 2; ++j, e = e * 5 % (2 * N)) {
        pos[bitrev((e - 1) >> shift, bits)] = (u32)j;
        if (conj_row) pos[bitrev((2 * N - e - 1) >> shift, bits)] = (u32)(j + N / 2);
    }
    return pos;
}

}  // namespace mkhe
