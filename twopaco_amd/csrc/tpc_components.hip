// tpc_components.hip -- the CONNECTED COMPONENTS of the compacted graph: which segments hang together, and what every piece holds.
// Kernels and the C-ABI of the tpc_segments_components_* group of include/twopaco_hip.h, which defines row, joined, component, root,
// component id and the per-component sums.  No counterpart in the reference; host/graphformat.h: ComputeComponents is the serial
// statement.
//
// Input: the event table of the last tpc_segments_build_*, the link rows of the last tpc_segments_links_build (first_event[r]: the row
// joins the segments of events e - 1 and e) and the colour rows of the last tpc_segments_colors_build (first event, occurrences,
// presence).  The row of every event's segment is made again (tpc_segrows.h); the row of a link's end is link_side(..) >> 1.
//   k_cmp_init    parent[r] = r
//   k_cmp_hook    one thread per link row: a lock-free union-find.  find follows parent[] down to a root (parent[x] == x) and halves
//                 the path on its way; the larger root is hooked under the smaller with a compare-and-swap on parent[hi] that expects
//                 hi, and on failure (hi is no root any more) the link finds again.  parent[x] <= x always, so a tree's root is the
//                 smallest row it holds, whatever the order of the atomics.  Nothing waits for anything: this is hooking, not locking.
//                 EVERY LOOP IS COUNTED: a find follows strictly decreasing parents, so it ends within S steps; a compare-and-swap on
//                 parent[hi] fails only because hi stopped being a root, which happens once per row, so a link retries at most S times.
//                 Both loops stop at `limit` (S + 1, or the option test_components_step_limit), raise a flag and leave; the build then
//                 returns an error text.  parent[] is read and written with relaxed agent-scope atomics only: no parent can sit in a
//                 register across a retry.  Path halving stores an ancestor over a parent; correctness does not depend on it.
//   k_cmp_flatten after the hooking has ended: label[r] = find(r), into a second array, under the same bound; flag[r] = label[r] == r
//   scan          exclusive, over the flags: the id of every root, the total is the number of components P
//   k_cmp_number  component[r] = id[label[r]]
//   k_cmp_rows    one thread per colour row: root[p] at the root row; segments, length, edges and occurrences of the row into the sums
//                 of p = component[r]; presence ORed.  HOT COMPONENT: the common input has one component holding nearly every row, so
//                 lanes compare their p with the lane below, the runs' values are summed by a segmented scan over the wave, and the run
//                 leader issues the run's atomics once (col_run, as the colour stage does).  The presence words of a run are ORed the
//                 same way, and the leader loads the component's word first and skips the atomic when it adds no bit: OR is
//                 idempotent, a saturated component costs reads only.
//   k_cmp_links   one thread per link row: links[p] += 1 at the component of its ends, folded by runs the same way
//   k_cmp_largest the largest segments[p], test first, then atomicMax
// Integers, commutative sums and ORs: the result is exact and does not depend on the schedule.
// Memory: kept until the next segment, link, colour or component build 4 B / row (component), per component 4 B (root), 40 B of sums and
// 4 W B of presence; during the call parent, label and the flags (4 B / row each), 4 B / event of ranks, the first-sight table and the
// scan's scratch.  None of it exists in a context that never asks for components.  What does not fit the free device memory is refused
// with an error text.
#include "tpc_segrows.h"

namespace {

constexpr uint64_t CMP_MAX_ROWS = ((uint64_t)1 << 31) - 1;   // link_side holds row << 1 | strand in 32 bits, all ones is no side
constexpr uint32_t CMP_FLAG_ROW = 1u, CMP_FLAG_EVENT = 2u, CMP_FLAG_GAVE_UP = 4u, CMP_FLAG_ID = 8u;
constexpr int CMP_SUMS = 5;                                   // planes of sums: segments, links, length, edges, occurrences

__device__ __forceinline__ uint32_t cmp_load(uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// x becomes the root of its tree.  false: `limit` steps did not reach it.  HALVE: every row passed gets its grandparent for a parent --
// an ancestor either way, and only a row that is no root (and never becomes one again) is written, so no hook's compare-and-swap sees it
template <bool HALVE>
__device__ __forceinline__ bool cmp_find(uint32_t *parent, uint32_t &x, uint32_t limit)
{
    for (uint32_t step = 0; step < limit; step++) {
        const uint32_t p = cmp_load(&parent[x]);
        if (p == x) return true;
        if (HALVE) {
            const uint32_t g = cmp_load(&parent[p]);
            if (g != p) __hip_atomic_store(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            x = g;
        } else x = p;
    }
    return false;
}

__global__ void k_cmp_init(uint32_t *__restrict__ parent, uint64_t n_rows)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += stride) parent[r] = (uint32_t)r;
}

__global__ void k_cmp_hook(const uint32_t *__restrict__ first_event, uint64_t n_links, const int64_t *__restrict__ name, uint64_t n_events,
                           const uint32_t *__restrict__ table, uint64_t n_table, const uint32_t *__restrict__ rank, uint64_t n_rows, uint32_t *parent,
                           uint32_t limit, uint32_t *__restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_links; r += stride) {
        const uint64_t e = first_event[r];
        if (e == 0 || e >= n_events) { atomicOr(flags, CMP_FLAG_EVENT); continue; }
        const uint32_t from = link_side(name, e - 1, n_events, table, n_table, rank, n_rows), to = link_side(name, e, n_events, table, n_table, rank, n_rows);
        if (from == 0xFFFFFFFFu || to == 0xFFFFFFFFu) { atomicOr(flags, CMP_FLAG_ROW); continue; }  // (a row is below n_rows otherwise)
        uint32_t u = from >> 1, v = to >> 1;
        bool joined = u == v;   // a self-loop, a link that is its own reverse: the row is joined to itself
        for (uint32_t retry = 0; !joined && retry < limit; retry++) {
            if (!cmp_find<true>(parent, u, limit) || !cmp_find<true>(parent, v, limit)) break;
            if (u == v) { joined = true; break; }
            const uint32_t hi = u > v ? u : v, lo = u > v ? v : u;
            uint32_t expected = hi;
            joined = __hip_atomic_compare_exchange_strong(&parent[hi], &expected, lo, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // on failure hi was hooked by somebody else meanwhile: u and v are where they were, the next find goes on from there
        }
        if (!joined) atomicOr(flags, CMP_FLAG_GAVE_UP);
    }
}

// flag: n_rows + 1 entries, the scan's last element is the number of components
__global__ void k_cmp_flatten(uint32_t *parent, uint64_t n_rows, uint32_t limit, uint32_t *__restrict__ label, uint32_t *__restrict__ flag, uint32_t *__restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n_rows; r += stride) {
        if (r == n_rows) { flag[r] = 0; continue; }
        uint32_t x = (uint32_t)r;
        if (!cmp_find<false>(parent, x, limit)) { atomicOr(flags, CMP_FLAG_GAVE_UP); x = (uint32_t)r; }
        label[r] = x;
        flag[r] = x == (uint32_t)r ? 1u : 0u;
    }
}

// id: the exclusive scan of the flags
__global__ void k_cmp_number(const uint32_t *__restrict__ label, const uint32_t *__restrict__ id, uint64_t n_rows, uint32_t *__restrict__ component)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rows; r += stride) component[r] = id[label[r]];
}

// the sum of v over the lanes start .. lane of this lane's run (start: the run's first lane)
__device__ __forceinline__ unsigned long long cmp_run_sum(unsigned long long v, uint32_t lane, uint32_t start)
{
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const unsigned long long below = __shfl_up(v, d);
        if (lane >= start + d) v += below;
    }
    return v;
}

__device__ __forceinline__ uint32_t cmp_run_or(uint32_t v, uint32_t lane, uint32_t start)
{
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t below = __shfl_up(v, d);
        if (lane >= start + d) v |= below;
    }
    return v;
}

// col_rows: the colour table's [4][n_rows] (first event, occurrences, ..).  sums: [CMP_SUMS][n_comp].  A whole wave runs every iteration
// (the stride is a multiple of 64), lanes past the last row take part in the shuffles and ballots and nothing else.
__global__ void k_cmp_rows(const uint32_t *__restrict__ component, const uint32_t *__restrict__ label, uint64_t n_rows, const uint32_t *__restrict__ col_rows,
                           const uint32_t *__restrict__ col_presence, uint32_t words, const uint32_t *__restrict__ begin, const uint32_t *__restrict__ end, uint64_t n_events,
                           uint32_t k, uint32_t *__restrict__ root, unsigned long long *__restrict__ sums, uint32_t *__restrict__ presence, uint64_t n_comp,
                           uint32_t *__restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r - lane < n_rows; r += stride) {
        bool active = r < n_rows;
        uint32_t p = 0xFFFFFFFFu;
        unsigned long long weight = 0, occurrences = 0;
        if (active) {
            p = component[r];
            const uint32_t e0 = col_rows[r];
            active = p < n_comp && e0 < n_events;
            if (!active) { atomicOr(flags, CMP_FLAG_ID); p = 0xFFFFFFFFu; }
            else {
                weight = (unsigned long long)end[e0] - begin[e0];
                occurrences = col_rows[n_rows + r];
                if (label[r] == (uint32_t)r) root[p] = (uint32_t)r;
            }
        }
        const uint32_t p_below = __shfl_up(p, 1);
        const bool head = lane == 0 || p_below != p;   // (the lanes that are not active are runs of their own: they hold all ones)
        const unsigned long long heads = __ballot(head), actives = __ballot(active);
        const uint32_t start = 63u - (uint32_t)__clzll((long long)(heads & (~0ull >> (63u - lane))));
        const unsigned long long run = col_run(lane, heads, actives);
        const uint32_t last = run ? 63u - (uint32_t)__clzll((long long)run) : lane;   // of a leader: the last lane of its run
        const unsigned long long weight_run = __shfl(cmp_run_sum(weight, lane, start), last), occ_run = __shfl(cmp_run_sum(occurrences, lane, start), last);
        const bool leader = head && active;
        if (leader) {
            const unsigned long long n = (unsigned long long)__popcll(run);
            atomicAdd(&sums[p], n);
            atomicAdd(&sums[2 * n_comp + p], weight_run + n * k);   // length = weight + k per segment
            atomicAdd(&sums[3 * n_comp + p], weight_run);
            atomicAdd(&sums[4 * n_comp + p], occ_run);
        }
        for (uint32_t w = 0; w < words; w++) {
            const uint32_t mine = active ? col_presence[r * words + w] : 0u;
            const uint32_t bits = __shfl(cmp_run_or(mine, lane, start), last);
            if (leader && bits) {
                uint32_t *at = &presence[(uint64_t)p * words + w];
                if (bits & ~cmp_load(at)) atomicOr(at, bits);
            }
        }
    }
}

__global__ void k_cmp_links(const uint32_t *__restrict__ first_event, uint64_t n_links, const int64_t *__restrict__ name, uint64_t n_events,
                            const uint32_t *__restrict__ table, uint64_t n_table, const uint32_t *__restrict__ rank, uint64_t n_rows,
                            const uint32_t *__restrict__ component, unsigned long long *__restrict__ links, uint64_t n_comp, uint32_t *__restrict__ flags)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r - lane < n_links; r += stride) {
        bool active = r < n_links;
        uint32_t p = 0xFFFFFFFFu;
        if (active) {
            const uint64_t e = first_event[r];
            const uint32_t from = e == 0 || e >= n_events ? 0xFFFFFFFFu : link_side(name, e - 1, n_events, table, n_table, rank, n_rows);
            const uint32_t to = from == 0xFFFFFFFFu ? from : link_side(name, e, n_events, table, n_table, rank, n_rows);
            // both ends lie in one component: the hooking joined them
            active = from != 0xFFFFFFFFu && to != 0xFFFFFFFFu && component[from >> 1] < n_comp && component[from >> 1] == component[to >> 1];
            if (active) p = component[from >> 1];
            else atomicOr(flags, CMP_FLAG_ID);
        }
        const uint32_t p_below = __shfl_up(p, 1);
        const bool head = lane == 0 || p_below != p;
        const unsigned long long heads = __ballot(head), actives = __ballot(active);
        if (head && active) atomicAdd(&links[p], (unsigned long long)__popcll(col_run(lane, heads, actives)));
    }
}

__global__ void k_cmp_largest(const unsigned long long *__restrict__ segments, uint64_t n_comp, unsigned long long *__restrict__ largest)
{
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n_comp; p += stride) {
        const unsigned long long n = segments[p];
        if (n > __hip_atomic_load(largest, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(largest, n);
    }
}

int cmp_fetch_check(tpc_ctx *c, const char *what, uint64_t total, uint64_t at, uint64_t n, bool missing)
{
    if ((n && missing) || at > total || n > total - at)
        return fail(c, -1, "segment components: bad row range (%llu %ss at %llu of %llu)", (unsigned long long)n, what, (unsigned long long)at, (unsigned long long)total);
    return 0;
}

}  // namespace

extern "C" {

int tpc_segments_components_build(tpc_ctx *c)
{
    if (!c) return -1;
    components_drop(c);
    if (int rc = stage_needs_segments(c, "components", "join")) return rc;
    if (!c->lnk.valid) return fail(c, -1, "segment components: build the link table first (tpc_segments_links_build)");
    if (!c->col.valid) return fail(c, -1, "segment components: build the colour table first (tpc_segments_colors_build)");
    const uint64_t n_events = c->seg.events, n_rows = c->seg.segments, n_links = c->lnk.n_rows;
    const uint32_t words = c->col.words;
    if (n_rows > CMP_MAX_ROWS) return fail(c, -1, "segment components: %llu segments, a row holds at most %llu", (unsigned long long)n_rows, (unsigned long long)CMP_MAX_ROWS);
    if (c->col.n_rows != n_rows) return fail(c, -10, "segment components: the colour table holds %llu rows, the build counted %llu segments", (unsigned long long)c->col.n_rows, (unsigned long long)n_rows);
    if (c->opt_components_step_limit < 0) return fail(c, -1, "segment components: option test_components_step_limit = %d is negative", c->opt_components_step_limit);
    HIPCHK(c, hipSetDevice(c->device));
    // a find passes at most S rows and a link is refused a hook at most S times: S + 1 is never reached
    const uint32_t limit = c->opt_components_step_limit ? (uint32_t)c->opt_components_step_limit : (uint32_t)n_rows + 1;

    // sizes in 64 bits, summed before the first allocation; what is kept per component has its bound: one component per row
    const uint64_t row_bytes = n_rows * 4 + 16, flag_bytes = (n_rows + 1) * 4;
    const uint64_t per_comp = 4 + CMP_SUMS * 8 + (uint64_t)words * 4, kept_bound = n_rows * per_comp + 48;
    size_t scan_flag = 0;
    uint32_t *parent = nullptr, *label = nullptr, *flag = nullptr, *flags = nullptr;
    SegRows idx;
    if (!idx.size(c) || rocprim::exclusive_scan(nullptr, scan_flag, flag, flag, 0u, n_rows + 1, rocprim::plus<uint32_t>(), c->stream) != hipSuccess)
        return fail(c, -10, "segment components: the scan could not be sized");
    idx.scan_alloc = std::max(idx.scan_alloc, scan_flag);   // one scratch for both scans
    const uint64_t need = 3 * row_bytes + flag_bytes + kept_bound + idx.bytes() + 16 + 64;
    if (int rc = stage_fits(c, "components", need, "%llu of them parent, label and component of %llu segments, up to %llu what %u presence words per component take", (unsigned long long)(3 * row_bytes),
                            (unsigned long long)n_rows, (unsigned long long)kept_bound, words))
        return rc;
    StageTemps temps;
    auto done = [&](int code) {
        if (code) components_drop(c);
        return code;
    };
    if (dev_malloc(c, (void **)&c->cmp.component, row_bytes) != hipSuccess || !idx.alloc(c, temps) || !temps.get(c, &parent, row_bytes) || !temps.get(c, &label, row_bytes) ||
        !temps.get(c, &flag, flag_bytes) || !temps.get(c, &flags, 64))
        return done(fail(c, -10, "segment components: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
    unsigned long long *largest = (unsigned long long *)(flags + 2);   // 8 bytes into the 64: flags[0], then the largest component
    hipStream_t s = c->stream;
    bool ok = idx.fill(s) && hipMemsetAsync(flags, 0, 64, s) == hipSuccess;
    uint32_t n_comp = 0, raised = 0;
    unsigned long long largest_host = 0;
    if (ok) {
        Timed t(c, TPC_K_COMPONENTS);   // the whole stage on the stream, the wait for the component count included (as TPC_K_BUBBLES)
        ok = idx.enqueue(c);
        if (ok && n_rows) hipLaunchKernelGGL(k_cmp_init, dim3(col_grid(n_rows)), dim3(256), 0, s, parent, n_rows);
        if (ok && n_links)
            hipLaunchKernelGGL(k_cmp_hook, dim3(col_grid(n_links)), dim3(256), 0, s, c->lnk.rows, n_links, c->seg.name, n_events, idx.table, idx.n_table, idx.rank, n_rows, parent, limit,
                               flags);
        if (ok) {
            hipLaunchKernelGGL(k_cmp_flatten, dim3(col_grid(n_rows + 1)), dim3(256), 0, s, parent, n_rows, limit, label, flag, flags);
            ok = rocprim::exclusive_scan(idx.scan_tmp, scan_flag, flag, flag, 0u, n_rows + 1, rocprim::plus<uint32_t>(), s) == hipSuccess;
        }
        if (ok && n_rows) hipLaunchKernelGGL(k_cmp_number, dim3(col_grid(n_rows)), dim3(256), 0, s, label, flag, n_rows, c->cmp.component);
        // the number of components decides the size of what is kept: the one wait in the middle
        ok = ok && idx.total(s) && hipMemcpyAsync(&n_comp, flag + n_rows, sizeof n_comp, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(&raised, flags, sizeof raised, hipMemcpyDeviceToHost, s) == hipSuccess;
        if (int rc = stage_wait(c, "components", ok)) return done(rc);
        if (idx.scanned != n_rows) return done(fail(c, -10, "segment components: the first bits hold %u segments, the build counted %llu", idx.scanned, (unsigned long long)n_rows));
        if (raised & CMP_FLAG_EVENT) return done(fail(c, -10, "segment components: a link row's first event lies outside the event table"));
        if (raised & CMP_FLAG_ROW) return done(fail(c, -10, "segment components: an event's segment is missing from the first-sight table"));
        if (raised & CMP_FLAG_GAVE_UP)
            return done(fail(c, -10, "segment components: gave up after %u steps of a find or retries of a hook over %llu segments (option test_components_step_limit = %d)", limit,
                             (unsigned long long)n_rows, c->opt_components_step_limit));
        if (n_comp > n_rows || (n_rows && !n_comp)) return done(fail(c, -10, "segment components: %u components of %llu segments", n_comp, (unsigned long long)n_rows));
        const uint64_t root_bytes = (uint64_t)n_comp * 4 + 16, sums_bytes = (uint64_t)n_comp * CMP_SUMS * 8 + 16, presence_bytes = (uint64_t)n_comp * words * 4 + 16;
        if (dev_malloc(c, (void **)&c->cmp.root, root_bytes) != hipSuccess || dev_malloc(c, (void **)&c->cmp.sums, sums_bytes) != hipSuccess ||
            dev_malloc(c, (void **)&c->cmp.presence, presence_bytes) != hipSuccess)
            return done(fail(c, -10, "segment components: hipMalloc failed: %s", hipGetErrorString(hipGetLastError())));
        ok = hipMemsetAsync(c->cmp.root, 0xFF, root_bytes, s) == hipSuccess && hipMemsetAsync(c->cmp.sums, 0, sums_bytes, s) == hipSuccess &&
             hipMemsetAsync(c->cmp.presence, 0, presence_bytes, s) == hipSuccess;
        if (ok && n_rows)
            hipLaunchKernelGGL(k_cmp_rows, dim3(col_grid(n_rows)), dim3(256), 0, s, c->cmp.component, label, n_rows, c->col.rows, c->col.presence, words, c->seg.ev[0], c->seg.ev[1], n_events,
                               (uint32_t)c->seg.k, c->cmp.root, c->cmp.sums, c->cmp.presence, (uint64_t)n_comp, flags);
        if (ok && n_links)
            hipLaunchKernelGGL(k_cmp_links, dim3(col_grid(n_links)), dim3(256), 0, s, c->lnk.rows, n_links, c->seg.name, n_events, idx.table, idx.n_table, idx.rank, n_rows, c->cmp.component,
                               c->cmp.sums + n_comp, (uint64_t)n_comp, flags);
        if (ok && n_comp) hipLaunchKernelGGL(k_cmp_largest, dim3(col_grid(n_comp)), dim3(256), 0, s, c->cmp.sums, (uint64_t)n_comp, largest);
        ok = ok && hipMemcpyAsync(&raised, flags, sizeof raised, hipMemcpyDeviceToHost, s) == hipSuccess &&
             hipMemcpyAsync(&largest_host, largest, sizeof largest_host, hipMemcpyDeviceToHost, s) == hipSuccess;
        c->cmp.peak_bytes = need - kept_bound + root_bytes + sums_bytes + presence_bytes;
    }
    if (int rc = stage_wait(c, "components", ok)) return done(rc);
    if (raised) return done(fail(c, -10, "segment components: a row or a link lies in no component"));
    c->cmp.n_comp = n_comp; c->cmp.n_rows = n_rows; c->cmp.largest = largest_host; c->cmp.words = words;
    c->cmp.valid = true;
    return 0;
}

int tpc_segments_components_info(tpc_ctx *c, uint64_t *info)
{
    if (!c) return -1;
    if (!c->cmp.valid) return fail(c, -1, "segment components: tpc_segments_components_build first");
    if (!info) return fail(c, -1, "segment components: info required");
    info[0] = c->cmp.n_comp; info[1] = c->cmp.n_rows; info[2] = c->cmp.largest; info[3] = c->cmp.peak_bytes;
    return 0;
}

int tpc_segments_components_fetch_members(tpc_ctx *c, uint64_t r0, uint64_t n, uint32_t *component_host)
{
    if (!c) return -1;
    if (!c->cmp.valid) return fail(c, -1, "segment components: tpc_segments_components_build first");
    return fetch_planes(c, "components", "row", c->cmp.component, c->cmp.n_rows, r0, n, { component_host });
}

int tpc_segments_components_fetch_rows(tpc_ctx *c, uint64_t p0, uint64_t n, uint32_t *root_host, uint64_t *segments_host, uint64_t *links_host, uint64_t *length_host,
                                       uint64_t *edges_host, uint64_t *occurrences_host)
{
    if (!c) return -1;
    if (!c->cmp.valid) return fail(c, -1, "segment components: tpc_segments_components_build first");
    uint64_t *const dst[CMP_SUMS] = { segments_host, links_host, length_host, edges_host, occurrences_host };
    bool missing = !root_host;
    for (uint64_t *d : dst) missing = missing || !d;
    if (int rc = cmp_fetch_check(c, "component", c->cmp.n_comp, p0, n, missing)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (!n) return 0;
    HIPCHK(c, hipMemcpy(root_host, c->cmp.root + p0, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < CMP_SUMS; i++) HIPCHK(c, hipMemcpy(dst[i], c->cmp.sums + (uint64_t)i * c->cmp.n_comp + p0, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return 0;
}

int tpc_segments_components_fetch_presence(tpc_ctx *c, uint64_t p0, uint64_t n, uint32_t *words_host)
{
    if (!c) return -1;
    if (!c->cmp.valid) return fail(c, -1, "segment components: tpc_segments_components_build first");
    if (int rc = cmp_fetch_check(c, "component", c->cmp.n_comp, p0, n, !words_host)) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    if (n) HIPCHK(c, hipMemcpy(words_host, c->cmp.presence + p0 * c->cmp.words, n * c->cmp.words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return 0;
}

}  // extern "C"
