// tpc_sketch.hip -- tpc_distinct_sketch: a HyperLogLog sketch (p = 14) of the distinct canonical (k+1)-mers of the uploaded text,
// the edges tpc_pass1_insert puts into the Bloom filter.  The host layer turns the registers into a count (host/filterplan.h) and
// the count into the filter size of `twopaco -f auto`.  The reference has nothing of the kind: its README leaves the filter size
// to a rule of thumb.
//
// Definition (include/twopaco_hip.h restates it; tests/sketch_reference.py evaluates it window by window).  n = k + 1,
// h[0..3] = the first four outputs of splitmix64 from state 0x5457504143.  For every window w = T[g .. g + n) without an 'N':
//     F = XOR_t rotl64(h[w_t], (n - 1 - t) mod 64)      R = XOR_t rotl64(h[3 - w_t], t mod 64)   (F of the reverse complement)
//     x = tpc_mix64(min(F, R));  idx = x >> 50;  v = x << 14;  rank = v ? clz64(v) + 1 : 51;  reg[idx] = max(reg[idx], rank)
//
// Work decomposition: the tile scheme of the first pass (tpc_pass1.hip) -- 256 threads, 32 positions per thread, the tile's packed
// words + halo staged through LDS, every thread eats its first window and then rolls both strands (two rolling updates per
// position, where the partitioned insert's hash does ten) -- but as LONG-LIVED workgroups: a grid of TPC_SKETCH_WG_PER_CU per CU
// strides over the tiles and keeps its registers in LDS, packed four to a 32-bit word (16 KiB; with the staged tile 19.9 KB per
// workgroup, so LDS admits eight workgroups per CU where 32-bit registers would admit two).  A register is READ first and
// updated, with a compare-and-swap on its word, only when the rank is larger: registers saturate after a few thousand windows and
// almost every position is then one LDS byte read.  Each workgroup merges once, at its end, into the 16384 32-bit registers in
// global memory: read first there too, atomicMax when larger.  max is order independent, so the result is bit-exact.
#include "tpc_ctx.h"
#include "tpc_edgehash.h"

#define TPC_HLL_P 14
#define TPC_HLL_M (1 << TPC_HLL_P)
#define TPC_SKETCH_WG_PER_CU 6   // resident at once with room to spare (LDS admits 8): no second wave of workgroups, no tail

int tpc_test_sketch_grid = 0;  // option "test_sketch_grid": at most this many workgroups (0 = TPC_SKETCH_WG_PER_CU per CU)

namespace {

// reg[idx] = max(reg[idx], rank) on the packed LDS registers
__device__ __forceinline__ void reg_max(uint32_t *s_reg, uint32_t idx, uint32_t rank)
{
    uint32_t *w = &s_reg[idx >> 2];
    const uint32_t sh = (idx & 3u) * 8u;
    uint32_t old = *reinterpret_cast<volatile uint32_t *>(w);
    while (((old >> sh) & 0xFFu) < rank) {
        const uint32_t want = (old & ~(0xFFu << sh)) | (rank << sh);
        const uint32_t seen = atomicCAS(w, old, want);
        if (seen == old) break;
        old = seen;
    }
}

__global__ void __launch_bounds__(TPC_TILE_THREADS)
k_distinct_sketch(SketchTab tab, int n, const uint64_t *__restrict__ bases, const uint32_t *__restrict__ nmask, uint64_t n_text, uint64_t n_tiles,
                  uint32_t *reg_global, unsigned long long *n_windows)
{
    __shared__ uint32_t s_reg[TPC_HLL_M / 4];
    __shared__ uint64_t s_b[TPC_TILE_WORDS];
    __shared__ uint32_t s_n[TPC_TILE_WORDS];
    __shared__ uint64_t s_t[16];
    __shared__ uint32_t s_w[4];
    const int tid = threadIdx.x;
    for (int i = tid; i < TPC_HLL_M / 4; i += TPC_TILE_THREADS) s_reg[i] = 0;
    tpc_edge_stage_tab(s_t, tab, tid);
    const int xw = n / 32 + 2;  // the last thread's last window ends (31 + n) / 32 words behind its own
    unsigned counted = 0;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t wfirst = tile * TPC_TILE_THREADS;
        const uint64_t wbase = wfirst - 1;
        __syncthreads();  // (the previous tile's readers are done; first round: the registers are zero)
        tpc_stage_tile(s_b, s_n, bases, nmask, wfirst, xw);
        __syncthreads();
        const uint64_t g0 = (wfirst + tid) * TPC_RUN;
        if (g0 >= n_text) continue;
        uint64_t F, R;
        int ncnt;
        tpc_edge_eat(s_t, s_b, s_n, g0, wbase, n, F, R, ncnt);
        for (int s = 0; s < TPC_RUN; s++) {
            const uint64_t g = g0 + s;
            if (ncnt == 0) {
                const uint64_t x = tpc_edge_hash(F, R);
                const uint32_t idx = (uint32_t)(x >> (64 - TPC_HLL_P));
                const uint64_t v = x << TPC_HLL_P;
                const uint32_t rank = v ? (uint32_t)__builtin_clzll(v) + 1u : (uint32_t)(64 - TPC_HLL_P + 1);
                reg_max(s_reg, idx, rank);
                counted++;
            }
            tpc_edge_roll(s_t, s_b, s_n, g, wbase, n, F, R, ncnt);
        }
    }
    __syncthreads();
    // one merge per workgroup; most registers already hold the maximum once the first workgroups are through
    for (int i = tid; i < TPC_HLL_M / 4; i += TPC_TILE_THREADS) {
        const uint32_t w = s_reg[i];
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t r = (w >> (8 * b)) & 0xFFu;
            uint32_t *dst = reg_global + 4 * i + b;
            if (r && *reinterpret_cast<volatile uint32_t *>(dst) < r) atomicMax(dst, r);
        }
    }
    if (n_windows) {
        for (int off = 32; off > 0; off >>= 1) counted += __shfl_down(counted, off, 64);
        if ((tid & 63) == 0) s_w[tid >> 6] = counted;
        __syncthreads();
        if (tid == 0) {
            const unsigned t = s_w[0] + s_w[1] + s_w[2] + s_w[3];
            if (t) atomicAdd(n_windows, (unsigned long long)t);
        }
    }
}

}  // namespace

extern "C" int tpc_distinct_sketch(tpc_ctx *c, int k, uint8_t *registers_host, uint64_t *n_windows)
{
    if (!c || !registers_host) return fail(c, -1, "bad arguments");
    if (!c->bases) return fail(c, -1, "seq_upload first");
    if (c->text_windowed) return fail(c, -1, "this context holds only its window of the text");
    if (k < 1) return fail(c, -1, "k must be positive");
    const int n = k + 1;
    if (n / 32 + 2 > TPC_XW_MAX)
        return fail(c, -1, "k=%d is too large for the sketch: a window of k + 1 letters must fit the %d halo words of a tile (k <= %d)", k, TPC_XW_MAX, (TPC_XW_MAX - 1) * 32 - 2);
    HIPCHK(c, hipSetDevice(c->device));
    memset(registers_host, 0, TPC_HLL_M);
    if (n_windows) *n_windows = 0;
    if (c->n_text < (uint64_t)n) return 0;  // no window at all
    const SketchTab tab = tpc_edge_tab(n);
    uint32_t *reg_dev = nullptr;
    HIPCHK(c, dev_malloc(c, (void **)&reg_dev, TPC_HLL_M * sizeof(uint32_t)));
    int n_cu = 0;
    if (hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess || n_cu <= 0) { (void)hipGetLastError(); n_cu = 256; }
    const uint64_t grid = std::min<uint64_t>(c->n_tiles, tpc_test_sketch_grid > 0 ? (uint64_t)tpc_test_sketch_grid : (uint64_t)n_cu * TPC_SKETCH_WG_PER_CU);
    std::vector<uint32_t> reg(TPC_HLL_M);
    unsigned long long windows = 0;
    hipError_t e = hipMemsetAsync(reg_dev, 0, TPC_HLL_M * sizeof(uint32_t), c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->counters, 0, sizeof(unsigned long long), c->stream);
    if (e == hipSuccess) {
        Timed t(c, TPC_K_SKETCH);
        hipLaunchKernelGGL(k_distinct_sketch, dim3((uint32_t)grid), dim3(TPC_TILE_THREADS), 0, c->stream, tab, n, c->bases, c->nmask, c->n_text, c->n_tiles, reg_dev, c->counters);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(reg.data(), reg_dev, TPC_HLL_M * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&windows, c->counters, sizeof windows, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(reg_dev);
    if (e != hipSuccess) return fail(c, -10, "tpc_distinct_sketch failed: %s", hipGetErrorString(e));
    for (int i = 0; i < TPC_HLL_M; i++) registers_host[i] = (uint8_t)reg[i];
    if (n_windows) *n_windows = windows;
    return 0;
}
