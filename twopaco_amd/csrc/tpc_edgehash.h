// tpc_edgehash.h -- the two-strand rolling hash of a canonical (k+1)-mer (an EDGE), shared by the distinct-edge sketch (tpc_sketch.hip)
// and the edge index (tpc_locate.hip).  n = k + 1, h[0..3] = the first four outputs of splitmix64 from state 0x5457504143.  For a
// window w = T[g .. g + n) without an 'N':
//     F = XOR_t rotl64(h[w_t], (n - 1 - t) mod 64)      R = XOR_t rotl64(h[3 - w_t], t mod 64)   (F of the reverse complement)
// and the edge's hash is tpc_mix64(min(F, R)): the same for a window and its reverse complement.  A thread eats its first window
// letter by letter and then rolls both strands, two updates per position.  The constants travel as a kernel argument (SketchTab)
// and are staged into 16 words of LDS (tpc_edge_stage_tab).
#pragma once
#include "tpc_device.h"

struct SketchTab {
    uint64_t h[4];    // h[c]
    uint64_t hn[4];   // rotl64(h[c], n mod 64): what the letter leaving the window contributes to F after one more rotation
    uint64_t hc[4];   // h[3 - c]
    uint64_t hcr[4];  // rotl64(h[3 - c], (n - 1) mod 64): what the letter entering the window contributes to R
};

inline uint64_t tpc_rotl64_host(uint64_t x, int r) { r &= 63; return r ? (x << r) | (x >> (64 - r)) : x; }

// the constants of a window of n letters
inline SketchTab tpc_edge_tab(int n)
{
    SketchTab tab;
    uint64_t state = 0x5457504143ull;
    for (int i = 0; i < 4; i++) {  // splitmix64: the state steps by the golden gamma, tpc_mix64 is its finaliser
        state += 0x9E3779B97F4A7C15ull;
        uint64_t z = state;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        tab.h[i] = z ^ (z >> 31);
    }
    for (int i = 0; i < 4; i++) {
        tab.hn[i] = tpc_rotl64_host(tab.h[i], n);
        tab.hc[i] = tab.h[3 - i];
        tab.hcr[i] = tpc_rotl64_host(tab.h[3 - i], n - 1);
    }
    return tab;
}

__device__ __forceinline__ uint64_t rotl1_64(uint64_t x) { return tpc_rotl1(x, 64, ~0ull); }
__device__ __forceinline__ uint64_t rotr1_64(uint64_t x) { return tpc_rotr1(x, 64); }

// s_t[16]: h, hn, hc, hcr; the caller synchronises before the first read
__device__ __forceinline__ void tpc_edge_stage_tab(uint64_t *s_t, const SketchTab &tab, int tid)
{
    if (tid < 4) { s_t[tid] = tab.h[tid]; s_t[4 + tid] = tab.hn[tid]; s_t[8 + tid] = tab.hc[tid]; s_t[12 + tid] = tab.hcr[tid]; }
}

// eat the window at g0 out of the staged tile: F left to right, R right to left ('N' hashes as code 0 -- such a window is never
// used, it only has to leave the way it came in); ncnt = the 'N's inside it
template <bool LEAN = false>   // LEAN: the loop is not unrolled, for a kernel that is short of scalar registers (tpc_locate.hip)
__device__ __forceinline__ void tpc_edge_eat(const uint64_t *s_t, const uint64_t *s_b, const uint32_t *s_n, uint64_t g0, uint64_t wbase, int n, uint64_t &F, uint64_t &R,
                                             int &ncnt)
{
    F = 0; R = 0; ncnt = 0;
    auto eat = [&](int t) {
        const int c = tpc_tile_char(s_b, s_n, g0 + t, wbase);
        const int cr = tpc_tile_char(s_b, s_n, g0 + n - 1 - t, wbase);
        ncnt += c == TPC_CODE_N;
        F = rotl1_64(F) ^ s_t[c & 3];
        R = rotl1_64(R) ^ s_t[8 + (cr & 3)];
    };
    if (LEAN) {
#pragma nounroll
        for (int t = 0; t < n; t++) eat(t);
    } else {
        for (int t = 0; t < n; t++) eat(t);
    }
}

// from the window at g to the one at g + 1: the edge extends the window by one letter on the positive strand and prepends its
// complement on the negative one
__device__ __forceinline__ void tpc_edge_roll(const uint64_t *s_t, const uint64_t *s_b, const uint32_t *s_n, uint64_t g, uint64_t wbase, int n, uint64_t &F, uint64_t &R,
                                              int &ncnt)
{
    const int c_out = tpc_tile_char(s_b, s_n, g, wbase);
    const int c_in = tpc_tile_char(s_b, s_n, g + n, wbase);
    ncnt += (c_in == TPC_CODE_N) - (c_out == TPC_CODE_N);
    F = rotl1_64(F) ^ s_t[4 + (c_out & 3)] ^ s_t[c_in & 3];
    R = rotr1_64(R ^ s_t[8 + (c_out & 3)]) ^ s_t[12 + (c_in & 3)];
}

__device__ __forceinline__ uint64_t tpc_edge_hash(uint64_t F, uint64_t R) { return tpc_mix64(tpc_min(F, R)); }
