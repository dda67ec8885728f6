// lds_bench.hip -- LDS operation rates that bound the write-combining bins (tpc_bins.h) on MI355X:
// returning / non-returning LDS atomics over a few hundred counters, random ds_or over a slice,
// random ring stores, and the whole push pattern (claim + head read + ring store).
//   hipcc --offload-arch=gfx950 -O3 tools/lds_bench.hip -o tools/lds_bench && tools/lds_bench
#include <hip/hip_runtime.h>
#include <cstdint>
#include <cstdio>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

__device__ __forceinline__ uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }

// MODE 0 atomicAdd returning over NB counters      1 atomicAdd no return over NB counters
//      2 atomicOr no return over 32768 words       3 store b32 random over 32768 words
//      4 store b64 random over 16384               5 load b32 random over 32768 words
//      6 push pattern u32 entries: claim + head read + ring store   7 push pattern u64 entries
//      8 atomicAdd returning on u64 counters (claim packs)          9 load b64 random (table lookups)
template <int MODE, int THREADS, int UNROLL>
__global__ void __launch_bounds__(THREADS) k_lds(uint32_t *out, int iters, int NB, uint32_t salt)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s[];  // 128 KiB data + counters
    uint32_t *cnt = s + 32768;
    uint32_t *head = cnt + 1024;
    for (int i = threadIdx.x; i < 32768 + 2048; i += THREADS) s[i] = 0;
    __syncthreads();
    uint32_t rng = (blockIdx.x * THREADS + threadIdx.x) * 2654435761u + salt;
    uint32_t acc = 0;
    const uint32_t nbm = (uint32_t)NB - 1u;
    const int logcap = MODE == 7 ? 14 - (31 - __builtin_clz(NB)) : 15 - (31 - __builtin_clz(NB));
    for (int it = 0; it < iters; it++) {
        uint32_t r[UNROLL], v[UNROLL], h[UNROLL];
#pragma unroll
        for (int u = 0; u < UNROLL; u++) r[u] = lcg(rng);
        if (MODE == 0) {
#pragma unroll
            for (int u = 0; u < UNROLL; u++) v[u] = atomicAdd(&cnt[r[u] & nbm], 1u);
#pragma unroll
            for (int u = 0; u < UNROLL; u++) acc += v[u];
        } else if (MODE == 1) {
#pragma unroll
            for (int u = 0; u < UNROLL; u++) __hip_atomic_fetch_add(&cnt[r[u] & nbm], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else if (MODE == 2) {
#pragma unroll
            for (int u = 0; u < UNROLL; u++) __hip_atomic_fetch_or(&s[(r[u] >> 5) & 32767u], 1u << (r[u] & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        } else if (MODE == 3) {
#pragma unroll
            for (int u = 0; u < UNROLL; u++) s[r[u] & 32767u] = r[u];
        } else if (MODE == 4) {
#pragma unroll
            for (int u = 0; u < UNROLL; u++) reinterpret_cast<uint64_t *>(s)[r[u] & 16383u] = ((uint64_t)r[u] << 32) | it;
        } else if (MODE == 5) {
#pragma unroll
            for (int u = 0; u < UNROLL; u++) v[u] = s[r[u] & 32767u];
#pragma unroll
            for (int u = 0; u < UNROLL; u++) acc += v[u];
        } else if (MODE == 6) {
#pragma unroll
            for (int u = 0; u < UNROLL; u++) { v[u] = atomicAdd(&cnt[r[u] & nbm], 1u); h[u] = head[r[u] & nbm]; }
#pragma unroll
            for (int u = 0; u < UNROLL; u++)
                if (v[u] - h[u] < 0x40000000u) s[((r[u] & nbm) << logcap) + (v[u] & ((1u << logcap) - 1u))] = r[u];
        } else if (MODE == 7) {
#pragma unroll
            for (int u = 0; u < UNROLL; u++) { v[u] = atomicAdd(&cnt[r[u] & nbm], 1u); h[u] = head[r[u] & nbm]; }
#pragma unroll
            for (int u = 0; u < UNROLL; u++)
                if (v[u] - h[u] < 0x40000000u) reinterpret_cast<uint64_t *>(s)[((r[u] & nbm) << logcap) + (v[u] & ((1u << logcap) - 1u))] = ((uint64_t)r[u] << 32) | v[u];
        } else if (MODE == 8) {
            unsigned long long *c64 = reinterpret_cast<unsigned long long *>(cnt);
            unsigned long long w[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; u++) w[u] = atomicAdd(&c64[r[u] & nbm & 511u], 1ull);
#pragma unroll
            for (int u = 0; u < UNROLL; u++) acc += (uint32_t)w[u];
        } else if (MODE == 9) {
            uint64_t w[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; u++) w[u] = reinterpret_cast<uint64_t *>(s)[r[u] & 63u];
#pragma unroll
            for (int u = 0; u < UNROLL; u++) acc += (uint32_t)w[u];
        }
    }
    __syncthreads();
    uint32_t x = acc;
    for (int i = threadIdx.x; i < 32768 + 2048; i += THREADS) x ^= s[i];
    if (x == 0x12345) out[0] = x;
}

template <int MODE, int THREADS, int UNROLL>
int run(const char *name, uint32_t *out, int NB)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const size_t lds = (32768 + 2048) * 4;
    CK(hipFuncSetAttribute((const void *)k_lds<MODE, THREADS, UNROLL>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int iters = 2048 / UNROLL, blocks = 1024;
    float ms = 0;
    for (int rep = 0; rep < 3; rep++) {
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL((k_lds<MODE, THREADS, UNROLL>), dim3(blocks), dim3(THREADS), lds, 0, out, iters, NB, (uint32_t)rep);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
    }
    const double ops = (double)blocks * THREADS * iters * UNROLL;
    printf("%-44s threads %4d unroll %2d NB %4d: %8.3f ms %9.1f Gops/s  (%.2f lanes/clk/CU)\n", name, THREADS, UNROLL, NB, ms, ops / ms / 1e6,
           ops / ms / 1e6 / 256 / 2.4);
    return 0;
}

// Five adjacent 16-byte rows per character index, as the seed and roll tables of the hash kernels hold them (tpc_qpartition.hip:
// k_q_hash2's s_seed, tpc_partition.hip: s_seed / s_roll).  One fetch = 16 bytes per lane; 1024 threads and 96 KiB of LDS per workgroup,
// so 16 waves per CU as in those kernels.
// MODE 0 every lane reads the row of its own random letter (ds_read_b128, per-lane index)   1 all lanes read one row (ds_read_b128, one address)
//      2 the five rows through uniform loads of a const __restrict__ table, the lane's row by selects: no LDS instruction
//      3 the same loads, the letter as five one-hot lane masks and every row XORed in under its mask by one v_bitop3_b32 per dword
//        (what k_q_hash2 does: the fetch and the XOR into the hash are one step there, so this case has no separate accumulate)
constexpr int ROWS_T = 64, ROWS_UNROLL = 8;
__device__ __forceinline__ uint32_t xor_and(uint32_t v, uint32_t row, uint32_t mask)
{   // v ^ (row & mask): truth table (a & b) ^ c = 0x6A
#if __has_builtin(__builtin_amdgcn_bitop3_b32)
    return __builtin_amdgcn_bitop3_b32(row, mask, v, 0x6Au);
#else
    return v ^ (row & mask);
#endif
}
template <int MODE>
__global__ void __launch_bounds__(1024) k_rows(uint32_t *out, const uint4 *__restrict__ tab, int iters, uint32_t salt)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s[];
    uint4 *rows = reinterpret_cast<uint4 *>(s);
    for (int i = threadIdx.x; i < ROWS_T * 5; i += 1024) rows[i] = tab[i];
    __syncthreads();
    uint32_t rng = (blockIdx.x * 1024 + threadIdx.x) * 2654435761u + salt;
    uint4 acc = make_uint4(0, 0, 0, 0);
    for (int it = 0; it < iters; it++) {
        uint32_t r = lcg(rng);  // 24 bits: eight letters of three bits, folded to 0..4
#pragma unroll
        for (int u = 0; u < ROWS_UNROLL; u++) {
            const uint32_t t = (uint32_t)(it * ROWS_UNROLL + u) & (ROWS_T - 1);  // uniform
            uint32_t c = r & 7u;
            r >>= 3;
            c = c >= 5u ? c - 5u : c;
            uint4 e;
            if (MODE == 3) {
                const uint32_t m0 = 0u - (c & 1u), m1 = 0u - ((c >> 1) & 1u), mn = 0u - (c >> 2);
                const uint32_t mk[5] = {~(m0 | m1 | mn), m0 & ~m1, m1 & ~m0, m0 & m1, mn};
#pragma unroll
                for (int l = 0; l < 5; l++) {
                    const uint4 r = tab[t * 5 + l];
                    acc.x = xor_and(acc.x, r.x, mk[l]); acc.y = xor_and(acc.y, r.y, mk[l]);
                    acc.z = xor_and(acc.z, r.z, mk[l]); acc.w = xor_and(acc.w, r.w, mk[l]);
                }
                continue;
            }
            if (MODE == 0) e = rows[t * 5 + c];
            else if (MODE == 1) e = rows[t * 5 + ((uint32_t)it & 3u)];
            else {
                const bool b0 = (c & 1u) != 0u, b1 = (c & 2u) != 0u, n = c >= 4u;
                const uint4 r0 = tab[t * 5], r1 = tab[t * 5 + 1], r2 = tab[t * 5 + 2], r3 = tab[t * 5 + 3], r4 = tab[t * 5 + 4];
                auto sel = [b0, b1, n](uint32_t a, uint32_t b, uint32_t g, uint32_t d, uint32_t x) {
                    const uint32_t ab = b0 ? b : a, gd = b0 ? d : g, v = b1 ? gd : ab;
                    return n ? x : v;
                };
                e = make_uint4(sel(r0.x, r1.x, r2.x, r3.x, r4.x), sel(r0.y, r1.y, r2.y, r3.y, r4.y), sel(r0.z, r1.z, r2.z, r3.z, r4.z),
                               sel(r0.w, r1.w, r2.w, r3.w, r4.w));
            }
            if (MODE == 1) e.x ^= c;  // (the letters stay live in every mode)
            acc.x ^= e.x; acc.y ^= e.y; acc.z ^= e.z; acc.w ^= e.w;
        }
    }
    if ((acc.x ^ acc.y ^ acc.z ^ acc.w) == 0x12345) out[0] = acc.x;
}

template <int MODE>
int run_rows(const char *name, uint32_t *out, const uint4 *tab)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    const size_t lds = 96 * 1024;  // one workgroup per CU
    CK(hipFuncSetAttribute((const void *)k_rows<MODE>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    const int iters = 2048 / ROWS_UNROLL, blocks = 1024;
    float ms = 0;
    for (int rep = 0; rep < 3; rep++) {
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL((k_rows<MODE>), dim3(blocks), dim3(1024), lds, 0, out, tab, iters, (uint32_t)rep);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        CK(hipEventElapsedTime(&ms, e0, e1));
    }
    const double ops = (double)blocks * 1024 * iters * ROWS_UNROLL;
    // cycles a CU spends per fetch of one wave at 2.4 GHz, 256 CUs (conflict-free ds_read_b128 by the cycle table: 4)
    printf("%-44s threads 1024, 16 waves/CU:        %8.3f ms %9.1f Gops/s  (%.2f lanes/clk/CU, %.1f CU cycles per wave fetch)\n", name, ms, ops / ms / 1e6,
           ops / ms / 1e6 / 256 / 2.4, ms * 1e-3 * 2.4e9 * 256 * 64 / ops);
    return 0;
}

int main()
{
    uint32_t *out;
    CK(hipMalloc(&out, 64));
    {
        uint4 h_tab[ROWS_T * 5];
        uint32_t x = 12345u;
        auto next = [&x] { x = x * 1664525u + 1013904223u; return x >> 8; };
        for (uint4 &v : h_tab) { v.x = next(); v.y = next(); v.z = next(); v.w = next(); }
        uint4 *tab;
        CK(hipMalloc(&tab, sizeof h_tab));
        CK(hipMemcpy(tab, h_tab, sizeof h_tab, hipMemcpyHostToDevice));
        run_rows<0>("b128 of 5 adjacent rows, per-lane letter", out, tab);
        run_rows<1>("b128 of 5 adjacent rows, one row for all", out, tab);
        run_rows<2>("5 rows by uniform loads + selects", out, tab);
        run_rows<3>("5 rows by uniform loads + lane masks", out, tab);
        CK(hipFree(tab));
    }
    for (int NB : {256, 512}) {
        run<0, 1024, 8>("atomicAdd returning, NB counters", out, NB);
        run<0, 1024, 2>("atomicAdd returning, NB counters", out, NB);
        run<0, 512, 8>("atomicAdd returning, NB counters", out, NB);
        run<0, 256, 8>("atomicAdd returning, NB counters", out, NB);
        run<1, 1024, 8>("atomicAdd no return, NB counters", out, NB);
        run<8, 1024, 8>("atomicAdd u64 returning, NB counters", out, NB);
        run<6, 1024, 8>("push u32: claim + head read + ring store", out, NB);
        run<6, 1024, 5>("push u32: claim + head read + ring store", out, NB);
        run<7, 1024, 8>("push u64: claim + head read + ring store", out, NB);
        run<7, 1024, 4>("push u64: claim + head read + ring store", out, NB);
    }
    run<2, 1024, 8>("atomicOr no return, 32768 words", out, 256);
    run<2, 256, 8>("atomicOr no return, 32768 words", out, 256);
    run<2, 256, 1>("atomicOr no return, 32768 words", out, 256);
    run<3, 1024, 8>("store b32 random, 32768 words", out, 256);
    run<4, 1024, 8>("store b64 random, 16384 dwords", out, 256);
    run<5, 1024, 8>("load b32 random, 32768 words", out, 256);
    run<9, 1024, 8>("load b64 random, 64 entries (tables)", out, 256);
    return 0;
}
