// tpc_distances.hip -- the GENOME DISTANCE MATRICES of the compacted graph: for every pair of colours how many segments, and how many
// edges ((k+1)-mers), both hold.  Kernels and the C-ABI of the tpc_segments_distances_* group of include/twopaco_hip.h, which defines
// weight, the two matrices and what a row is.  No counterpart in the reference; host/graphformat.h: ComputeDistances is the serial
// statement.
//
// Input: the colour table of the last tpc_segments_colors_build (presence[row][W], first_event[row]) and begin[] / end[] of the event
// table.  The matrices are a weighted Gram product of the S x C presence bit matrix.  A scatter would cost n_colors^2 atomics per row
// (3844 for a core segment of 62 genomes, 16 M at 4000 colours), so the bits are turned colour-major and pairs of columns are ANDed:
//   k_dst_columns  one wave per 64 consecutive rows and presence word w: lane l loads presence[r0 + l][w] (0 past the last row), the
//                  ballot of bit b is the 64-row column word of colour 32w + b, lane b keeps it and stores col[32w + b][r0 / 64].
//                  Colours at or past C (the tail bits of the last word) are not stored, nor ever read.
//   k_dst_planes   one wave per 64 rows: weight = end[e0] - begin[e0] of the row's first event (0 past the last row), the ballot of
//                  bit b is plane[b][r0 / 64]; the OR of the wave's weights goes to one word by one atomicOr per wave: its bit
//                  width is the number of planes B that hold anything, no separate max pass and no host wait.
//   k_dst_gram     a block owns a tile of DST_TILE x DST_TILE colour pairs (upper triangle of tiles, diagonal tiles included) and
//                  walks chunks of DST_CHUNK column words: the 2 x DST_TILE columns and the B planes of the chunk are staged in
//                  LDS (rows padded by one word: the 16 columns a wave reads at once fall into 16 different bank pairs), every
//                  thread owns 2 x 2 pairs and per word computes a = col_i & col_j, segments += popcll(a), and where any of its
//                  four a is not 0, edges += popcll(a & plane_b) << b for b < B.  Accumulators are 64-bit registers kept across
//                  the chunks a block walks; at the end one 64-bit atomicAdd per pair that saw anything.  Integers and a
//                  commutative sum: the result does not depend on the schedule.
//   k_dst_mirror   the upper triangle into the lower.
// Memory: kept until the next segment, colour or distance build 16 B x C^2; during the call 8 B x C x ceil(S / 64) of columns,
// 32 x 8 B x ceil(S / 64) of planes and 64 B of scalars.  None of it exists in a context that never asks for distances, and the
// segment, colour, link and bubble outputs are what they were.  What does not fit the free device memory is refused with an error text.
#include "tpc_stage.h"

namespace {

constexpr uint32_t DST_TILE = TPC_DISTANCES_TILE;  // colours on each side of a block's tile (tpc_ctx.h; tpc_get_stat "distances_tile")
static_assert(DST_TILE == 32, "k_dst_gram gives every one of its 256 threads 2 x 2 pairs of a 32 x 32 tile");
constexpr uint64_t DST_MAX_COLORS = (uint64_t)1 << 24;   // 16 B x C^2 is 2^52 there: no size below can wrap, and no device holds it
constexpr uint32_t DST_CHUNK = 64;                // column words a block stages at once
constexpr uint32_t DST_STRIDE = DST_CHUNK + 1;    // LDS row length: (2 x 32 + 32) rows x 65 x 8 B = 49 920 B
constexpr uint32_t DST_PLANES = 32;               // a weight is end - begin in 32 bits
constexpr uint32_t DST_FLAG_EVENT = 1u;

__device__ __forceinline__ uint32_t dst_width(uint32_t m) { return m ? 32u - (uint32_t)__clz(m) : 0u; }

// col: [n_colors][nw].  Every wave runs whole iterations: the loop's bounds depend on the wave's index only.
__global__ void k_dst_columns(const uint32_t *__restrict__ presence, uint64_t n_rows, uint32_t words, uint32_t n_colors, uint64_t nw,
                              unsigned long long *__restrict__ col)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6), total = nw * words;
    for (uint64_t u = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); u < total; u += waves) {
        const uint64_t g = u / words, r = g * 64 + lane;
        const uint32_t w = (uint32_t)(u % words);
        const uint32_t word = r < n_rows ? presence[r * words + w] : 0u;   // the tail rows: no bit
        unsigned long long mine = 0;
        for (uint32_t b = 0; b < 32; b++) {
            const unsigned long long v = __ballot((word >> b) & 1u);
            if (lane == b) mine = v;
        }
        const uint64_t colour = (uint64_t)w * 32 + lane;
        if (lane < 32 && colour < n_colors) col[colour * nw + g] = mine;  // the tail bits of the last word: no column
    }
}

// plane: [DST_PLANES][nw].  scalars[0]: the OR of every weight, scalars[1]: flags
__global__ void k_dst_planes(const uint32_t *__restrict__ first_event, const uint32_t *__restrict__ begin, const uint32_t *__restrict__ end, uint64_t n_rows,
                             uint64_t n_events, uint64_t nw, unsigned long long *__restrict__ plane, uint32_t *__restrict__ scalars)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t waves = (uint64_t)gridDim.x * (blockDim.x >> 6);
    for (uint64_t g = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); g < nw; g += waves) {
        const uint64_t r = g * 64 + lane;
        uint32_t weight = 0;
        if (r < n_rows) {
            const uint32_t e0 = first_event[r];
            if (e0 < n_events) weight = end[e0] - begin[e0];
            else atomicOr(&scalars[1], DST_FLAG_EVENT);
        }
        unsigned long long mine = 0;
        for (uint32_t b = 0; b < DST_PLANES; b++) {
            const unsigned long long v = __ballot((weight >> b) & 1u);
            if (lane == b) mine = v;
        }
        if (lane < DST_PLANES) plane[(uint64_t)lane * nw + g] = mine;
        const unsigned long long used = __ballot(lane < DST_PLANES && mine != 0);   // bit b: some weight of the wave holds bit b
        if (lane == 0 && used) atomicOr(&scalars[0], (uint32_t)used);
    }
}

// mat: [2][n_colors][n_colors], segments then edges, zero on entry; the upper triangle is written.  grid: x walks the chunks, y the
// tile pairs, both by their strides.  cw: the chunk length in words, 1 .. DST_CHUNK.
__global__ __launch_bounds__(256) void k_dst_gram(const unsigned long long *__restrict__ col, const unsigned long long *__restrict__ plane,
                                                  const uint32_t *__restrict__ scalars, uint32_t n_colors, uint64_t nw, uint32_t cw, uint32_t n_tiles,
                                                  uint64_t n_pairs, uint64_t n_chunks, unsigned long long *__restrict__ mat)
{
    __shared__ unsigned long long s_i[DST_TILE * DST_STRIDE], s_j[DST_TILE * DST_STRIDE], s_p[DST_PLANES * DST_STRIDE];
    const uint32_t planes = dst_width(scalars[0]);
    const uint32_t tx = threadIdx.x & 15u, ty = threadIdx.x >> 4;   // the thread's pairs: i in {ty, ty + 16}, j in {tx, tx + 16}
    for (uint64_t pair = blockIdx.y; pair < n_pairs; pair += gridDim.y) {
        // the pair's tiles: row ti of the upper triangle holds n_tiles - ti of them
        uint32_t ti = 0;
        uint64_t rest = pair;
        while (rest >= n_tiles - ti) { rest -= n_tiles - ti; ti++; }
        const uint32_t tj = ti + (uint32_t)rest;
        unsigned long long seg[4] = {0, 0, 0, 0}, edg[4] = {0, 0, 0, 0};
        for (uint64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
            const uint64_t w0 = chunk * cw;
            __syncthreads();   // the chunk before is read to its end
            for (uint32_t idx = threadIdx.x; idx < DST_TILE * cw; idx += blockDim.x) {
                const uint32_t c = idx / cw, w = idx % cw;
                const uint64_t gw = w0 + w, gi = (uint64_t)ti * DST_TILE + c, gj = (uint64_t)tj * DST_TILE + c;
                s_i[c * DST_STRIDE + w] = (gi < n_colors && gw < nw) ? col[gi * nw + gw] : 0ull;   // ragged tile, partial last chunk: no bit
                s_j[c * DST_STRIDE + w] = (gj < n_colors && gw < nw) ? col[gj * nw + gw] : 0ull;
            }
            for (uint32_t idx = threadIdx.x; idx < planes * cw; idx += blockDim.x) {
                const uint32_t b = idx / cw, w = idx % cw;
                const uint64_t gw = w0 + w;
                s_p[b * DST_STRIDE + w] = gw < nw ? plane[(uint64_t)b * nw + gw] : 0ull;
            }
            __syncthreads();
            for (uint32_t w = 0; w < cw; w++) {
                const unsigned long long i0 = s_i[ty * DST_STRIDE + w], i1 = s_i[(ty + 16) * DST_STRIDE + w];
                const unsigned long long j0 = s_j[tx * DST_STRIDE + w], j1 = s_j[(tx + 16) * DST_STRIDE + w];
                const unsigned long long a[4] = { i0 & j0, i0 & j1, i1 & j0, i1 & j1 };
                for (int q = 0; q < 4; q++) seg[q] += (unsigned long long)__popcll(a[q]);
                if (a[0] | a[1] | a[2] | a[3]) {
                    for (uint32_t b = 0; b < planes; b++) {
                        const unsigned long long p = s_p[b * DST_STRIDE + w];
                        for (int q = 0; q < 4; q++) edg[q] += (unsigned long long)__popcll(a[q] & p) << b;
                    }
                }
            }
        }
        const uint64_t cc = (uint64_t)n_colors * n_colors;
        for (int q = 0; q < 4; q++) {
            const uint64_t gi = (uint64_t)ti * DST_TILE + ty + ((q >> 1) ? 16 : 0), gj = (uint64_t)tj * DST_TILE + tx + ((q & 1) ? 16 : 0);
            if (gi >= n_colors || gj >= n_colors || gi > gj || !seg[q]) continue;   // a diagonal tile computes its lower half for nothing
            atomicAdd(&mat[gi * n_colors + gj], seg[q]);
            if (edg[q]) atomicAdd(&mat[cc + gi * n_colors + gj], edg[q]);
        }
    }
}

__global__ void k_dst_mirror(unsigned long long *__restrict__ mat, uint64_t n_colors)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, cc = n_colors * n_colors;
    for (uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < cc; idx += stride) {
        const uint64_t i = idx / n_colors, j = idx % n_colors;
        if (i > j) { mat[idx] = mat[j * n_colors + i]; mat[cc + idx] = mat[cc + j * n_colors + i]; }
    }
}

unsigned dst_grid(uint64_t n, uint64_t per_block) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + per_block - 1) / per_block, 8192)); }

}  // namespace

extern "C" {

int tpc_segments_distances_build(tpc_ctx *c)
{
    if (!c) return -1;
    distances_drop(c);
    if (int rc = stage_needs_segments(c, "distances", "compare")) return rc;
    if (!c->col.valid) return fail(c, -1, "segment distances: build the colour table first (tpc_segments_colors_build)");
    if (c->opt_distances_chunk_words < 0 || c->opt_distances_chunk_words > (int)DST_CHUNK)
        return fail(c, -1, "segment distances: option test_distances_chunk_words = %d is not in 0 .. %u", c->opt_distances_chunk_words, DST_CHUNK);
    // before any arithmetic with it: the colour stage takes up to 2^31 colours, whose square times 16 B wraps 64 bits
    if (c->col.n_colors > DST_MAX_COLORS)
        return fail(c, -20, "segment distances: %u colours, the two matrices of 16 B x colours^2 are refused beyond %llu colours", c->col.n_colors, (unsigned long long)DST_MAX_COLORS);
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t n_rows = c->col.n_rows, n_colors = c->col.n_colors, n_events = c->seg.events, nw = (n_rows + 63) / 64;
    const uint32_t cw = c->opt_distances_chunk_words ? (uint32_t)c->opt_distances_chunk_words : DST_CHUNK;

    // sizes in 64 bits, summed before the first allocation: C <= 2^24 (checked above) and nw < 2^26, so 16 C^2 <= 2^52 and 8 C nw < 2^53
    const uint64_t mat_bytes = 16 * n_colors * n_colors, col_bytes = 8 * n_colors * nw + 16, plane_bytes = 8 * (uint64_t)DST_PLANES * nw + 16;
    const uint64_t need = mat_bytes + col_bytes + plane_bytes + 64;
    if (int rc = stage_fits(c, "distances", need, "%llu of them the two matrices of %llu x %llu colours, %llu the bit columns of %llu segments", (unsigned long long)mat_bytes,
                            (unsigned long long)n_colors, (unsigned long long)n_colors, (unsigned long long)col_bytes, (unsigned long long)n_rows))
        return rc;
    StageTemps temps;
    unsigned long long *col = nullptr, *plane = nullptr;
    uint32_t *scalars = nullptr;
    auto done = [&](int code) {
        if (code) distances_drop(c);
        return code;
    };
    if (dev_malloc(c, (void **)&c->dst.mat, mat_bytes) != hipSuccess || !temps.get(c, &col, col_bytes) || !temps.get(c, &plane, plane_bytes) || !temps.get(c, &scalars, 64))
        return done(fail(c, -10, "segment distances: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
    hipStream_t s = c->stream;
    bool ok = hipMemsetAsync(c->dst.mat, 0, mat_bytes, s) == hipSuccess && hipMemsetAsync(scalars, 0, 64, s) == hipSuccess;
    uint32_t host_scalars[2] = {0, 0};
    if (ok) {
        Timed t(c, TPC_K_DISTANCES);
        if (nw) {
            const uint64_t n_tiles = (n_colors + DST_TILE - 1) / DST_TILE, n_pairs = n_tiles * (n_tiles + 1) / 2, n_chunks = (nw + cw - 1) / cw;
            hipLaunchKernelGGL(k_dst_columns, dim3(dst_grid(nw * c->col.words, 4)), dim3(256), 0, s, c->col.presence, n_rows, c->col.words, (uint32_t)n_colors, nw, col);
            hipLaunchKernelGGL(k_dst_planes, dim3(dst_grid(nw, 4)), dim3(256), 0, s, c->col.rows, c->seg.ev[0], c->seg.ev[1], n_rows, n_events, nw, plane, scalars);
            // a few thousand blocks in all: few tile pairs leave a block several chunks, whose sums it keeps in registers
            const uint64_t gy = std::min<uint64_t>(n_pairs, 65535), gx = std::max<uint64_t>(1, std::min<uint64_t>(n_chunks, 4096 / gy));
            hipLaunchKernelGGL(k_dst_gram, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, s, col, plane, scalars, (uint32_t)n_colors, nw, cw, (uint32_t)n_tiles, n_pairs,
                               n_chunks, c->dst.mat);
            hipLaunchKernelGGL(k_dst_mirror, dim3(dst_grid(n_colors * n_colors, 256)), dim3(256), 0, s, c->dst.mat, n_colors);
        }
    }
    ok = ok && hipMemcpyAsync(host_scalars, scalars, sizeof host_scalars, hipMemcpyDeviceToHost, s) == hipSuccess;
    const hipError_t waited = hipStreamSynchronize(s), launched = hipGetLastError();
    if (waited != hipSuccess || launched != hipSuccess)
        return done(fail(c, -10, "segment distances: the kernels failed: %s", hipGetErrorString(waited != hipSuccess ? waited : launched)));
    if (!ok) return done(fail(c, -10, "segment distances: a fill or a copy of the stage could not be enqueued"));
    if (host_scalars[1] & DST_FLAG_EVENT) return done(fail(c, -10, "segment distances: a colour row's first event lies outside the event table"));
    c->dst.n_colors = n_colors; c->dst.n_rows = n_rows; c->dst.peak_bytes = need;
    c->dst.planes = host_scalars[0] ? 32 - (uint64_t)__builtin_clz(host_scalars[0]) : 0;
    c->dst.valid = true;
    return 0;
}

int tpc_segments_distances_info(tpc_ctx *c, uint64_t *info)
{
    if (!c) return -1;
    if (!c->dst.valid) return fail(c, -1, "segment distances: tpc_segments_distances_build first");
    if (!info) return fail(c, -1, "segment distances: info required");
    info[0] = c->dst.n_colors; info[1] = c->dst.n_rows; info[2] = c->dst.planes; info[3] = c->dst.peak_bytes;
    return 0;
}

int tpc_segments_distances_fetch(tpc_ctx *c, uint64_t i0, uint64_t n, uint64_t *segments_host, uint64_t *edges_host)
{
    if (!c) return -1;
    if (!c->dst.valid) return fail(c, -1, "segment distances: tpc_segments_distances_build first");
    if ((n && (!segments_host || !edges_host)) || i0 > c->dst.n_colors || n > c->dst.n_colors - i0)
        return fail(c, -1, "segment distances: bad row range (%llu rows at %llu of %llu)", (unsigned long long)n, (unsigned long long)i0, (unsigned long long)c->dst.n_colors);
    HIPCHK(c, hipSetDevice(c->device));
    const uint64_t C = c->dst.n_colors;
    if (n) {
        HIPCHK(c, hipMemcpy(segments_host, c->dst.mat + i0 * C, n * C * 8, hipMemcpyDeviceToHost));
        HIPCHK(c, hipMemcpy(edges_host, c->dst.mat + C * C + i0 * C, n * C * 8, hipMemcpyDeviceToHost));
    }
    return 0;
}

}  // extern "C"
